"""Dev tool: branched decoding (several questions on one prefilled video) at Nemotron-Nano-9B-v2 dims.

  attention  per attention layer, prefixes of 32 868 and 163 940 keys (2 048 / 10 240 frames), a suffix of 64 rows,
             B in {1, 2, 4, 8, 16} branches: tv_attn_branch_fwd (the prefix shared, read once) against
             tv_attn_decode_fwd(batch = B) on B COPIES of the keys (what B forks made by clone() cost), with the fraction
             of the prefix-read roof (K and V of the prefix once, 8 TB/s);
  step       the whole branched step as one captured graph (random-init 9B weights, a 32 868-token cache) in tokens/s,
             against B sequential single-token steps: B <= 4 (the fused gemv step), B = 8 / 16 on the library GEMM and on the
             fused rows route (TV_ROWS_FUSED=1).
Event-timed graph replays, 3-4 warm-up replays, best of 5 x 10.  No threshold is derived here: the file records what a later
decision about the defaults (TV_ROWS_FUSED for branched steps, the suffix split) rests on.
usage (GPU box): python timeviper_amd/devtools/bench_branch.py [out.json] [--attention-only]
(default out: profiles/branch_decode.json)"""
import gc
import json
import os
import pathlib
import sys

import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parents[2]))
from timeviper_amd import kernels as K      # noqa: E402
from timeviper_amd.model.llm import nano    # noqa: E402
from timeviper_amd.model.llm.decode_graph import GraphedDecodeStep      # noqa: E402

DEV = torch.device("cuda", 0)
BRANCHES = (1, 2, 4, 8, 16)
PREFIXES = (32868, 163940)
SUFFIX = 64
CACHE_TOKENS = 32868
HBM_GBPS = 8000


def replay_us(fn, st, reps=10, rounds=5):
    """us per call of `fn`, captured as one graph and replayed between two events on `st`"""
    with torch.cuda.stream(st):
        fn()
        st.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=st):
            fn()
        for _ in range(3):
            graph.replay()
        st.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        best = 1e9
        for _ in range(rounds):
            e0.record(st)
            for _ in range(reps):
                graph.replay()
            e1.record(st)
            st.synchronize()
            best = min(best, e0.elapsed_time(e1) / reps * 1e3)
    return best


def bench_attention(st, Hq=40, Hkv=8):
    out = []
    for Lp in PREFIXES:
        g = torch.Generator(device=DEV).manual_seed(1)
        kp = torch.randn(1, Lp, Hkv, 128, device=DEV, generator=g).bfloat16()
        vp = torch.randn(1, Lp, Hkv, 128, device=DEV, generator=g).bfloat16()
        prefix_bytes = 2 * Lp * Hkv * 128 * 2
        for B in BRANCHES:
            q = torch.randn(B, 1, Hq, 128, device=DEV, generator=g).bfloat16()
            ks = torch.randn(B, SUFFIX, Hkv, 128, device=DEV, generator=g).bfloat16()
            vs = torch.randn(B, SUFFIX, Hkv, 128, device=DEV, generator=g).bfloat16()
            lens = torch.full((B,), SUFFIX, dtype=torch.int32, device=DEV)
            r = {"prefix_keys": Lp, "suffix": SUFFIX, "branches": B,
                 "branch_us": replay_us(lambda: K.flash_attn_branch(q, kp, vp, ks, vs, seqlens_suffix=lens), st)}
            r["prefix_roof_fraction"] = prefix_bytes / r["branch_us"] / 1e3 / HBM_GBPS
            try:        # B copies of the keys: what B clone()d forks hold and read
                kc = torch.cat([kp.expand(B, -1, -1, -1), ks], dim=1).contiguous()
                vc = torch.cat([vp.expand(B, -1, -1, -1), vs], dim=1).contiguous()
                r["decode_on_copies_us"] = replay_us(lambda: K.flash_attn_decode(q, kc, vc), st)
                r["copies_bytes"] = 2 * kc.numel() * 2
                del kc, vc
            except torch.cuda.OutOfMemoryError:
                r["decode_on_copies_us"] = None
            out.append(r)
            d = r["decode_on_copies_us"]
            print(f"attention Lp {Lp:6d} B {B:2d}: branch {r['branch_us']:8.1f} us ({r['prefix_roof_fraction']:.2f} of the "
                  f"prefix-read roof)   decode on {B} copies {d if d is None else round(d, 1)} us", flush=True)
        del kp, vp
        gc.collect()
        torch.cuda.empty_cache()
    return out


def bench_step(st):
    cfg = nano.NemotronHConfig.nemotron_nano_9b_v2()
    torch.manual_seed(0)
    with torch.device(DEV):
        llm = nano.NemotronHForCausalLM(cfg)
    llm = llm.bfloat16().eval()
    g = torch.Generator(device=DEV).manual_seed(1)
    emb = (torch.randn(1, CACHE_TOKENS, cfg.hidden_size, device=DEV, generator=g) * 0.02).bfloat16()
    host_pos = torch.ones(1, dtype=torch.long)
    room = 4 + 3 + 5 * 10 + 8
    res = {"cache_tokens": CACHE_TOKENS, "weights": "random init, seed 0", "dtype": "bf16", "rows": []}

    def graphed_ms(cache, B):
        """ms per replay of the captured step of `cache` (B rows of one token)"""
        stp = GraphedDecodeStep(lambda ids: llm(input_ids=ids, past_key_values=cache, use_cache=True,
                                                cache_position=host_pos).logits, cache, B, DEV)
        tok = torch.zeros(B, 1, dtype=torch.long, device=DEV)
        for _ in range(4):
            tok = stp.step(tok).view(B, 1)
        torch.cuda.synchronize()
        assert stp.graph is not None, stp.capture_error
        with torch.cuda.stream(st):
            for _ in range(3):
                stp.graph.replay()
            st.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            best = 1e9
            for _ in range(5):
                e0.record(st)
                for _ in range(10):
                    stp.graph.replay()
                e1.record(st)
                st.synchronize()
                best = min(best, e0.elapsed_time(e1) / 10)
        return best

    with torch.inference_mode():
        base = nano.HybridMambaAttentionDynamicCache(cfg, 1, dtype=torch.bfloat16, device=DEV)
        llm(inputs_embeds=emb, past_key_values=base, use_cache=True, cache_position=torch.zeros(1, dtype=torch.long))
        del emb
        cache = base.clone()
        cache.begin_static_decode(room)
        t_dec = graphed_ms(cache, 1)
        res["t_decode_ms"] = t_dec
        print(f"decode step: {t_dec:.3f} ms ({1e3 / t_dec:.0f} tokens/s)", flush=True)
        del cache
        for B in BRANCHES:
            for rows_fused in ((False,) if B <= 4 else (False, True)):
                os.environ["TV_ROWS_FUSED"] = "1" if rows_fused else "0"
                bs = base.branch(B, suffix_cap=room)
                bs.begin_static_decode(room)
                t = graphed_ms(bs, B)
                route = "gemv" if B <= 4 else ("rows" if rows_fused else "library")
                r = {"branches": B, "linear_route": route, "t_step_ms": t, "tokens_per_s": B * 1e3 / t,
                     "sequential_tokens_per_s": 1e3 / t_dec, "speedup": B * t_dec / t}
                res["rows"].append(r)
                print(f"B {B:2d} ({route:7s}): step {t:.3f} ms = {r['tokens_per_s']:.0f} tokens/s, {r['speedup']:.2f} x "
                      f"{B} sequential steps", flush=True)
                del bs
                gc.collect()
                torch.cuda.empty_cache()
        os.environ.pop("TV_ROWS_FUSED", None)
    return res


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out = pathlib.Path(args[0]) if args else pathlib.Path(__file__).resolve().parents[2] / "profiles" / "branch_decode.json"
    st = torch.cuda.Stream()
    res = {"device": torch.cuda.get_device_name(0), "attention": bench_attention(st)}
    if "--attention-only" not in sys.argv:
        res["step"] = bench_step(st)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(res, indent=1) + "\n")
    print("->", out)


if __name__ == "__main__":
    main()
