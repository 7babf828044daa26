"""Dev tool: what sampled decoding costs (tv_sample_logits_fwd in the place of the decode step's argmax).

  kernel   the sampler at B in {1, 4, 16} rows x V in {131 072, 152 064} x the parameter sets of tests/test_sampling_gpu.py,
           on bf16 values widened to fp32 (sigma 3), and beside it the `argmax` it replaces;
  step     the decode step as one captured graph at the `bench.py --config decode` geometry (random-init 9B weights, a
           32 868-token cache): greedy and sampled (T 0.7, top-k 50, top-p 0.95), tokens/s of both, same process.
Event-timed graph replays after warm-up replays, best of 5 x 10.  No threshold is derived here: the file records what the
README row and DESIGN.md state.
usage (GPU box): python timeviper_amd/devtools/bench_sample.py [out.json] [--kernel-only]
(default out: profiles/sample_decode.json)"""
import json
import pathlib
import sys

import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parents[2]))
from timeviper_amd import kernels as K      # noqa: E402
from timeviper_amd.model.llm import nano    # noqa: E402
from timeviper_amd.model.llm.decode_graph import GraphedDecodeStep      # noqa: E402
from timeviper_amd.model.llm.sampling import Sampler                     # noqa: E402

DEV = torch.device("cuda", 0)
ROWS = (1, 4, 16)
VOCABS = (131072, 152064)
PARAMS = ((1.0, 0, 0.9), (0.7, 50, 0.95), (1.3, 0, 0.5), (1.0, 40, 1.0), (1.0, 0, 1.0), (1.0, 1, 1.0))
CACHE_TOKENS = 32868
STEP_PARAMS = dict(temperature=0.7, top_k=50, top_p=0.95)


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


def bench_kernel(st):
    out = []
    for V in VOCABS:
        for B in ROWS:
            g = torch.Generator(device=DEV).manual_seed(B)
            z = (torch.randn(B, V, device=DEV, generator=g) * 3.0).bfloat16().float()
            draws = torch.arange(B, dtype=torch.int64, device=DEV)
            streams = torch.arange(B, dtype=torch.int32, device=DEV)
            ids = torch.empty(B, dtype=torch.int64, device=DEV)
            r = {"vocab": V, "rows": B, "argmax_us": replay_us(lambda: z.argmax(-1), st), "sampler_us": {}}
            for T, k, p in PARAMS:
                r["sampler_us"][f"T{T}_k{k}_p{p}"] = replay_us(
                    lambda: K.sample_logits(z, draws, streams, 1, temperature=T, top_k=k, top_p=p, out=ids), st)
            out.append(r)
            print(f"V {V} B {B:2d}: argmax {r['argmax_us']:6.1f} us   sampler " +
                  "  ".join(f"{n} {t:6.1f}" for n, t in r["sampler_us"].items()), flush=True)
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
    res = {"cache_tokens": CACHE_TOKENS, "weights": "random init, seed 0", "dtype": "bf16", "vocab": cfg.vocab_size,
           "sampler": STEP_PARAMS}

    def graphed_ms(cache, sampler):
        stp = GraphedDecodeStep(lambda ids: llm(input_ids=ids, past_key_values=cache, use_cache=True,
                                                cache_position=host_pos).logits, cache, 1, DEV, sampler=sampler)
        tok = torch.zeros(1, 1, dtype=torch.long, device=DEV)
        for _ in range(4):
            tok = stp.step(tok).view(1, 1)
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
        # greedy, sampled, greedy, sampled: the two are compared inside one process, alternating
        times = {"greedy": [], "sampled": []}
        for _ in range(2):
            for name in ("greedy", "sampled"):
                cache = base.clone()
                cache.begin_static_decode(room)
                sampler = Sampler(DEV, seed=1, **STEP_PARAMS) if name == "sampled" else None
                times[name].append(graphed_ms(cache, sampler))
                del cache
                torch.cuda.empty_cache()
    for name, ts in times.items():
        res[f"{name}_step_ms"] = min(ts)
        res[f"{name}_step_ms_runs"] = ts
        res[f"{name}_tokens_per_s"] = 1e3 / min(ts)
    res["sampled_over_greedy"] = res["sampled_step_ms"] / res["greedy_step_ms"]
    print(f"decode step: greedy {res['greedy_step_ms']:.3f} ms ({res['greedy_tokens_per_s']:.0f} tokens/s), sampled "
          f"{res['sampled_step_ms']:.3f} ms ({res['sampled_tokens_per_s']:.0f} tokens/s): x{res['sampled_over_greedy']:.4f}",
          flush=True)
    return res


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out = pathlib.Path(args[0]) if args else pathlib.Path(__file__).resolve().parents[2] / "profiles" / "sample_decode.json"
    st = torch.cuda.Stream()
    res = {"device": torch.cuda.get_device_name(0), "kernel": bench_kernel(st)}
    if "--kernel-only" not in sys.argv:
        res["step"] = bench_step(st)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(res, indent=1) + "\n")
    print("->", out)


if __name__ == "__main__":
    main()
