"""Dev tool: what a speculative (draft-and-verify) step costs at Nemotron-Nano-9B-v2 dims, against the decode step.

  kernel      tv_selective_state_update_spec, one launch per layer over the 27 layers' states (27 x 5.2 MB fp32) in one
              hipGraph at (n_commit, T): the flush (T = 0), the pure look-ahead (n_commit = 0), the steady state of D drafts
              with a accepted (n_commit = a + 1, T = D + 1), n_commit read from device memory; beside it
              tv_selective_state_update_seq at the same T and the decode step's tv_selective_state_update.
  end to end  the synthetic 9B hybrid (random weights) behind a prefill of 32 868 tokens (2 048 frames): the captured
              single-token step (GraphedDecodeStep) and, for D in {1, 2, 3, 4, 8}, the captured draft-and-verify step
              (GraphedSpecStep, T = D + 1; one graph per slot parity, replayed alternately) in the same process.  The
              step's cost depends on how many tokens the previous step kept (the commit phase), so it is timed with the
              acceptance forced to k = 1 (no draft kept) and k = T (all kept); t_spec(a) is taken linear between the two.
              Break-even mean accepted drafts a*: (a* + 1) / t_spec(a*) = 1 / t_decode.
  gemm        the M = T linear layers of the step per role (every layer's own weights once, as in the step, one graph):
              us per layer, GB/s of weight bytes, fraction of the 8 TB/s read roof; T = 1 on tv_gemv_bf16_fwd beside it.

  --rows      tv_linear_rows_bf16_fwd (the few-token linear layers) against the library: per role and T in {2, 3, 5, 9, 16}
              linear_rows_fused with the role's prologue, F.linear on the same operands and, where the role has a prologue,
              the stand-alone operator + F.linear (median of the repeats, each layer's own weights); then the decode step
              and the draft-and-verify steps with TV_ROWS_FUSED = 0 and = 1 in the same process, each repeated, with the
              spread of the repeats; break-even per D and best_drafts of both.  Writes profiles/rows_linear.json and leaves
              profiles/speculative_decode.json alone.  "stay_on_library" lists the (role, T) where the kernel's median is
              above the library's: what kernels.ROWS_ON_LIBRARY is to hold.

Event-timed on a side stream, 3 warm-up replays, best of 5 x 10 replays; writes a JSON file (default
profiles/speculative_decode.json).  `speculative.DEFAULT_DRAFTS` is "end_to_end" -> "best_drafts" of that file.
usage (GPU box): python timeviper_amd/devtools/bench_speculative.py [out.json] [--kernel-only | --rows [--roles-only]]"""
import gc
import json
import os
import pathlib
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parents[2]))
from timeviper_amd import kernels as K      # noqa: E402
from timeviper_amd.devtools.bench_continue import timed, H, P, G, N, LAYERS      # noqa: E402
from timeviper_amd.model.llm import nano      # noqa: E402
from timeviper_amd.model.llm.decode_graph import GraphedDecodeStep, GraphedSpecStep      # noqa: E402

DEV = torch.device("cuda", 0)
DRAFTS = (1, 2, 3, 4, 8)
CACHE_TOKENS = 2048 * 16 + 100
HBM_PEAK_GBS = 8000.0


def bench_kernel(st):
    g = torch.Generator(device=DEV).manual_seed(0)
    states = [torch.randn(1, H, P, N, device=DEV, generator=g) for _ in range(LAYERS)]
    A = -(torch.rand(H, device=DEV, generator=g) * 15 + 1)
    D, bias = torch.ones(H, device=DEV), torch.full((H,), -2.0, device=DEV)

    def operands(T):
        x = torch.randn(1, T, H, P, device=DEV, generator=g).bfloat16()
        dt = torch.randn(1, T, H, device=DEV, generator=g).bfloat16()
        Bm = (torch.randn(1, G, T, N, device=DEV, generator=g) * 0.5).bfloat16().transpose(1, 2)
        Cm = (torch.randn(1, G, T, N, device=DEV, generator=g) * 0.5).bfloat16().transpose(1, 2)
        return x, dt, Bm, Cm
    rows = []
    for Dn in DRAFTS:
        T = Dn + 1
        prev, new = operands(T), operands(T)
        x1 = [t[:, 0].contiguous() for t in new]
        for nc, tn in sorted({(0, T), (1, T), ((T + 1) // 2, T), (T, T)}) + [(T, 0)]:
            ncd = torch.tensor([nc], dtype=torch.int32, device=DEV)

            def spec():
                for s in states:
                    K.selective_state_update_spec(s, prev, ncd, new if tn else None, A, D=D, dt_bias=bias, dt_softplus=True)
            r = {"drafts": Dn, "n_commit": nc, "T": tn, "spec_us": timed(spec, st)}
            rows.append(r)
            print(f"D {Dn}: n_commit {nc:2d}, T {tn:2d}: spec {r['spec_us']:7.2f} us per layer", flush=True)

        def seq():
            for s in states:
                K.selective_state_update_seq(s, *new[:2], A, *new[2:], D=D, dt_bias=bias, dt_softplus=True)

        def step():
            for s in states:
                K.selective_state_update(s, x1[0], x1[1], A, x1[2], x1[3], D=D, dt_bias=bias, dt_softplus=True)
        rows.append({"drafts": Dn, "T": T, "seq_us": timed(seq, st), "decode_step_us": timed(step, st)})
        print(f"D {Dn}: seq(T={T}) {rows[-1]['seq_us']:7.2f} us, one decode step {rows[-1]['decode_step_us']:7.2f} us per layer",
              flush=True)
    return rows


def replay_ms(graphs, st, reps=10, rounds=5):
    """ms per replay, the graphs taken in turn, between two events on `st`"""
    with torch.cuda.stream(st):
        for i in range(4):
            graphs[i % len(graphs)].replay()
        st.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        best = 1e9
        for _ in range(rounds):
            e0.record(st)
            for i in range(reps):
                graphs[i % len(graphs)].replay()
            e1.record(st)
            st.synchronize()
            best = min(best, e0.elapsed_time(e1) / reps)
    return best


REPLAYS = 4 + 5 * 10         # what replay_ms launches


class ForcedAcceptance(GraphedSpecStep):
    """The captured step with every operation of the real one, but `k` tokens kept whatever the drafts were."""

    def __init__(self, *a, keep, **kw):
        super().__init__(*a, **kw)
        self.keep = torch.full((), int(keep), dtype=torch.int32, device=self.ids.device)

    def _accept(self, p):
        return super()._accept(p) * 0 + self.keep


def bench_gemm(llm, st):
    """The step's linear layers per role at M = T rows, each layer's own weights (what the step streams), one graph."""
    roles = {"mamba in_proj": [], "mamba out_proj": [], "mlp up_proj": [], "mlp down_proj": [], "attn q/k/v": [], "attn o_proj": []}
    for blk in llm.backbone.layers:
        m = blk.mixer
        if blk.block_type == "mamba":
            roles["mamba in_proj"].append(m.in_proj)
            roles["mamba out_proj"].append(m.out_proj)
        elif blk.block_type == "mlp":
            roles["mlp up_proj"].append(m.up_proj)
            roles["mlp down_proj"].append(m.down_proj)
        else:
            roles["attn q/k/v"] += [m.q_proj, m.k_proj, m.v_proj]
            roles["attn o_proj"].append(m.o_proj)
    roles["lm_head"] = [llm.lm_head]
    rows = []
    for role, mods in roles.items():
        nbytes = sum(m.weight.numel() * 2 for m in mods)
        for T in (1,) + tuple(d + 1 for d in DRAFTS):
            xs = [torch.randn(1, T, m.in_features, device=DEV).bfloat16() * 0.1 for m in mods]
            route = nano.linear_route(xs[0])     # T = 1: tv_gemv_bf16_fwd where it applies, else the library GEMM

            def run():
                for m, x in zip(mods, xs):
                    nano._linear(m, x, route)
            with torch.cuda.stream(st):
                run()
                st.synchronize()
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph, stream=st):
                    run()
            ms = replay_ms([graph], st)
            r = {"role": role, "T": T, "layers": len(mods), "us_per_layer": ms * 1e3 / len(mods), "weight_bytes": nbytes,
                 "GBps": nbytes / ms / 1e6, "roof_fraction": nbytes / ms / 1e6 / HBM_PEAK_GBS,
                 "kernel": "tv_gemv_bf16_fwd" if T == 1 else "library GEMM"}
            rows.append(r)
            print(f"gemm {role:15s} T {T}: {r['us_per_layer']:8.1f} us per layer, {r['GBps']:7.0f} GB/s = "
                  f"{r['roof_fraction']:.2f} of the read roof ({r['kernel']})", flush=True)
            del graph
    return rows


ROWS_T = (2, 3, 5, 9, 16)


def graph_ms(run, st, repeats=3):
    """ms of one captured `run` per repeat of replay_ms (best of 5 x 10 replays each)"""
    with torch.cuda.stream(st):
        run()
        st.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=st):
            run()
    return [replay_ms([graph], st) for _ in range(repeats)]


def bench_rows_roles(llm, st):
    """tv_linear_rows_bf16_fwd per role against F.linear and the unfused pair; every layer's own weights, one graph."""
    cfg = llm.config
    roles = {"mamba in_proj": ("rmsnorm", []), "mamba out_proj": ("gated", []), "mlp up_proj": ("rmsnorm", []),
             "mlp down_proj": ("relu2", []), "attn q/k/v (stacked)": ("rmsnorm", []), "attn o_proj": ("none", [])}
    for blk in llm.backbone.layers:
        m = blk.mixer
        if blk.block_type == "mamba":
            roles["mamba in_proj"][1].append((m.in_proj.weight, blk.norm.weight, None))
            roles["mamba out_proj"][1].append((m.out_proj.weight, m.norm.weight, m.norm.group_size))
        elif blk.block_type == "mlp":
            roles["mlp up_proj"][1].append((m.up_proj.weight, blk.norm.weight, None))
            roles["mlp down_proj"][1].append((m.down_proj.weight, None, None))
        else:
            roles["attn q/k/v (stacked)"][1].append((m._qkv_weight(), blk.norm.weight, None))
            roles["attn o_proj"][1].append((m.o_proj.weight, None, None))
    roles["lm_head"] = ("none", [(llm.lm_head.weight, None, None)])
    eps = float(getattr(cfg, "layer_norm_epsilon", 1e-5))
    rows, lose = [], []
    for role, (pro, layers) in roles.items():
        nbytes = sum(w.numel() * 2 for w, _, _ in layers)
        n, k = layers[0][0].shape
        for T in ROWS_T:
            xs = [torch.randn(1, T, k, device=DEV).bfloat16() * 0.1 for _ in layers]
            ds = [torch.randn(1, T, k, device=DEV).bfloat16() * 0.1 for _ in layers]
            sums = [torch.empty_like(x) for x in xs]

            def fused():
                for (w, nw, gs), x, d, so in zip(layers, xs, ds, sums):
                    if pro == "rmsnorm":
                        K.linear_rows_fused(x, w, None, K.GEMV_RMSNORM, delta=d, sum_out=so, norm_weight=nw, eps=eps)
                    elif pro == "gated":
                        K.linear_rows_fused(x, w, None, K.GEMV_GATED, norm_weight=nw, eps=eps, gate=d, group_size=gs)
                    elif pro == "relu2":
                        K.linear_rows_fused(x, w, None, K.GEMV_RELU2)
                    else:
                        K.linear_rows_fused(x, w)

            def library():
                for (w, _, _), x in zip(layers, xs):
                    F.linear(x, w)

            def pair():
                for (w, nw, gs), x, d in zip(layers, xs, ds):
                    if pro == "rmsnorm":
                        f, _ = K.rms_norm(x, nw, eps, residual=d, return_sum=True)
                    elif pro == "gated":
                        f = K.rmsnorm_fn(x, nw, None, z=d, eps=eps, group_size=gs, norm_before_gate=False)
                    else:
                        f = K.relu2(x)
                    F.linear(f, w)
            r = {"role": role, "T": T, "N": n, "K": k, "prologue": pro, "layers": len(layers), "weight_bytes": nbytes}
            for name, fn in (("rows", fused), ("library", library)) + ((("unfused_pair", pair),) if pro != "none" else ()):
                ms = graph_ms(fn, st)
                r[name + "_us_per_layer"] = statistics.median(ms) * 1e3 / len(layers)
                r[name + "_us_repeats"] = [m * 1e3 / len(layers) for m in ms]
            r["rows_roof_fraction"] = nbytes / (r["rows_us_per_layer"] * len(layers)) / 1e3 / HBM_PEAK_GBS
            r["library_roof_fraction"] = nbytes / (r["library_us_per_layer"] * len(layers)) / 1e3 / HBM_PEAK_GBS
            against = r.get("unfused_pair_us_per_layer", r["library_us_per_layer"])
            r["rows_wins"] = r["rows_us_per_layer"] <= against
            if r["rows_us_per_layer"] > r["library_us_per_layer"]:
                lose.append({"role": role, "T": T, "N": n, "K": k})
            rows.append(r)
            print(f"rows {role:22s} T {T:2d}: rows {r['rows_us_per_layer']:7.1f} us ({r['rows_roof_fraction']:.2f} of the roof), "
                  f"library {r['library_us_per_layer']:7.1f} us ({r['library_roof_fraction']:.2f})"
                  + (f", unfused pair {r['unfused_pair_us_per_layer']:7.1f} us" if pro != "none" else ""), flush=True)
    return rows, lose


def bench_rows(st, roles_only=False, repeats=3):
    """profiles/rows_linear.json: the per-role table and the on / off end-to-end pair of one session."""
    cfg = nano.NemotronHConfig.nemotron_nano_9b_v2()
    torch.manual_seed(0)
    with torch.device(DEV):
        llm = nano.NemotronHForCausalLM(cfg)
    llm = llm.bfloat16().eval()
    res = {"device": torch.cuda.get_device_name(0), "weights": "random init, seed 0", "dtype": "bf16"}
    with torch.inference_mode():
        res["roles"], res["stay_on_library"] = bench_rows_roles(llm, st)
        if roles_only:
            res["end_to_end"] = "not measured (--roles-only)"
            return res
        g = torch.Generator(device=DEV).manual_seed(1)
        emb = (torch.randn(1, CACHE_TOKENS, cfg.hidden_size, device=DEV, generator=g) * 0.02).bfloat16()
        host_pos = torch.ones(1, dtype=torch.long)
        base = nano.HybridMambaAttentionDynamicCache(cfg, 1, dtype=torch.bfloat16, device=DEV)
        out = llm(inputs_embeds=emb, past_key_values=base, use_cache=True, cache_position=torch.zeros(1, dtype=torch.long))
        tok = out.logits[:, -1].argmax(-1).view(1, 1)
        del emb, out
        cache = base.clone()
        cache.begin_static_decode(8 + repeats * REPLAYS + 8)
        dec = GraphedDecodeStep(lambda ids: llm(input_ids=ids, past_key_values=cache, use_cache=True,
                                                cache_position=host_pos).logits, cache, 1, DEV)
        for _ in range(4):
            tok = dec.step(tok).view(1, 1)
        torch.cuda.synchronize()
        assert dec.graph is not None, dec.capture_error
        t_dec = statistics.median(replay_ms([dec.graph], st) for _ in range(repeats))
        del dec, cache
        gc.collect()
        torch.cuda.empty_cache()
        e2e = {"cache_tokens": CACHE_TOKENS, "t_decode_ms": t_dec, "repeats": repeats}
        print(f"decode step: {t_dec:.3f} ms", flush=True)
        saved = os.environ.get("TV_ROWS_FUSED")
        for env in ("0", "1"):
            os.environ["TV_ROWS_FUSED"] = env       # (read per call: the captures below take the route it names)
            steps = []
            for Dn in DRAFTS:
                T = Dn + 1
                t, spread = {}, {}
                for keep in (1, T):
                    cache = base.clone()
                    cache.begin_speculation(T, (8 + repeats * REPLAYS + 8) * T)
                    stp = ForcedAcceptance(lambda ids: llm(input_ids=ids, past_key_values=cache, use_cache=True,
                                                           cache_position=host_pos, logits_to_keep=ids.shape[1]).logits,
                                           cache, T, DEV, keep=keep)
                    for i in range(4):
                        k, _ = stp.step(int(tok), [(7 * i + j) % cfg.vocab_size for j in range(Dn)])
                        assert k == keep, (k, keep)
                    torch.cuda.synchronize()
                    assert len(stp.graphs) == 2 and stp.capture_error is None, stp.capture_error
                    first = cache.spec_parity()
                    ms = [replay_ms([stp.graphs[first], stp.graphs[first ^ 1]], st) for _ in range(repeats)]
                    t[keep], spread[keep] = statistics.median(ms), max(ms) - min(ms)
                    del stp, cache
                    gc.collect()
                    torch.cuda.empty_cache()
                slope = (t[T] - t[1]) / Dn
                a_star = (t[1] - t_dec) / (t_dec - slope) if t_dec > slope else float("inf")
                steps.append({"drafts": Dn, "T": T, "t_spec_none_kept_ms": t[1], "t_spec_none_kept_spread_ms": spread[1],
                              "t_spec_all_kept_ms": t[T], "t_spec_all_kept_spread_ms": spread[T],
                              "break_even_accepted": a_star, "speedup_all_accepted": T * t_dec / t[T]})
                print(f"TV_ROWS_FUSED={env} D {Dn}: step {t[1]:.3f} ms (spread {spread[1]:.3f}) .. {t[T]:.3f} ms; "
                      f"break-even a* = {a_star:.2f}", flush=True)
            ok = [r for r in steps if r["break_even_accepted"] <= r["drafts"]]
            e2e["rows_fused_" + ("on" if env == "1" else "off")] = {
                "steps": steps, "best_drafts": min(ok, key=lambda r: r["break_even_accepted"])["drafts"] if ok else None}
        if saved is None:
            del os.environ["TV_ROWS_FUSED"]
        else:
            os.environ["TV_ROWS_FUSED"] = saved
        on, off = (e2e["rows_fused_" + k]["steps"] for k in ("on", "off"))
        d2 = [(a, b) for a, b in zip(on, off) if a["drafts"] == 2][0]
        e2e["d2_margin_ms"] = d2[1]["t_spec_none_kept_ms"] - d2[0]["t_spec_none_kept_ms"]
        e2e["d2_off_spread_ms"] = d2[1]["t_spec_none_kept_spread_ms"]
        e2e["faster_with_rows_fused"] = e2e["d2_margin_ms"] > e2e["d2_off_spread_ms"]
        print(f"D 2, no draft kept: off - on = {e2e['d2_margin_ms']:.3f} ms, spread of off {e2e['d2_off_spread_ms']:.3f} ms",
              flush=True)
        res["end_to_end"] = e2e
    return res


def bench_end_to_end(st):
    cfg = nano.NemotronHConfig.nemotron_nano_9b_v2()
    torch.manual_seed(0)
    with torch.device(DEV):
        llm = nano.NemotronHForCausalLM(cfg)
    llm = llm.bfloat16().eval()
    g = torch.Generator(device=DEV).manual_seed(1)
    emb = (torch.randn(1, CACHE_TOKENS, cfg.hidden_size, device=DEV, generator=g) * 0.02).bfloat16()
    host_pos = torch.ones(1, dtype=torch.long)
    res = {"cache_tokens": CACHE_TOKENS, "weights": "random init, seed 0", "dtype": "bf16", "steps": []}
    with torch.inference_mode():
        base = nano.HybridMambaAttentionDynamicCache(cfg, 1, dtype=torch.bfloat16, device=DEV)
        out = llm(inputs_embeds=emb, past_key_values=base, use_cache=True, cache_position=torch.zeros(1, dtype=torch.long))
        tok = out.logits[:, -1].argmax(-1).view(1, 1)
        del emb, out
        # ---- the captured single-token step
        cache = base.clone()
        cache.begin_static_decode(8 + REPLAYS + 8)
        dec = GraphedDecodeStep(lambda ids: llm(input_ids=ids, past_key_values=cache, use_cache=True,
                                                cache_position=host_pos).logits, cache, 1, DEV)
        for _ in range(4):
            tok = dec.step(tok).view(1, 1)
        torch.cuda.synchronize()
        assert dec.graph is not None, dec.capture_error
        t_dec = replay_ms([dec.graph], st)
        res["t_decode_ms"] = t_dec
        print(f"decode step: {t_dec:.3f} ms ({1e3 / t_dec:.0f} tokens/s)", flush=True)
        del dec, cache
        gc.collect()
        torch.cuda.empty_cache()
        # ---- the captured draft-and-verify step
        for Dn in DRAFTS:
            T = Dn + 1
            t = {}
            for keep in (1, T):
                cache = base.clone()
                cache.begin_speculation(T, (8 + REPLAYS + 8) * T)
                stp = ForcedAcceptance(lambda ids: llm(input_ids=ids, past_key_values=cache, use_cache=True,
                                                       cache_position=host_pos, logits_to_keep=ids.shape[1]).logits,
                                       cache, T, DEV, keep=keep)
                for i in range(4):                   # two eager steps, one capture per slot parity
                    k, _ = stp.step(int(tok), [(7 * i + j) % cfg.vocab_size for j in range(Dn)])
                    assert k == keep, (k, keep)
                torch.cuda.synchronize()
                assert len(stp.graphs) == 2 and stp.capture_error is None, stp.capture_error
                first = cache.spec_parity()          # the parity the next step runs on
                t[keep] = replay_ms([stp.graphs[first], stp.graphs[first ^ 1]], st)
                del stp, cache
                gc.collect()
                torch.cuda.empty_cache()
            # t_spec(a) = t1 + (tT - t1) a / D;  (a* + 1) t_decode = t_spec(a*)
            slope = (t[T] - t[1]) / Dn
            a_star = (t[1] - t_dec) / (t_dec - slope) if t_dec > slope else float("inf")
            r = {"drafts": Dn, "T": T, "t_spec_none_kept_ms": t[1], "t_spec_all_kept_ms": t[T],
                 "break_even_accepted": a_star, "speedup_all_accepted": T * t_dec / t[T]}
            res["steps"].append(r)
            print(f"D {Dn}: step {t[1]:.3f} ms (no draft kept) .. {t[T]:.3f} ms (all kept) = {t[1] / t_dec:.2f} .. "
                  f"{t[T] / t_dec:.2f} decode steps; break-even a* = {a_star:.2f} accepted drafts per step; all accepted: "
                  f"{r['speedup_all_accepted']:.2f} x", flush=True)
        ok = [r for r in res["steps"] if r["break_even_accepted"] <= r["drafts"]]
        res["best_drafts"] = min(ok, key=lambda r: r["break_even_accepted"])["drafts"] if ok else None
        res["gemm_roles"] = bench_gemm(llm, st)
    return res


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out = pathlib.Path(args[0]) if args else pathlib.Path(__file__).resolve().parents[2] / "profiles" / "speculative_decode.json"
    st = torch.cuda.Stream()
    if "--rows" in sys.argv:
        out = pathlib.Path(args[0]) if args else pathlib.Path(__file__).resolve().parents[2] / "profiles" / "rows_linear.json"
        res = bench_rows(st, roles_only="--roles-only" in sys.argv)
        out.parent.mkdir(parents=True, exist_ok=True)
        out.write_text(json.dumps(res, indent=1) + "\n")
        print("->", out)
        return
    res = {"shape": {"H": H, "P": P, "G": G, "N": N, "layers": LAYERS, "dtype": "bf16"}, "kernel_rows": bench_kernel(st),
           "device": torch.cuda.get_device_name(0)}
    res["end_to_end"] = "not measured (--kernel-only)" if "--kernel-only" in sys.argv else bench_end_to_end(st)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(res, indent=1) + "\n")
    print("->", out)


if __name__ == "__main__":
    main()
