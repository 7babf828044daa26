"""Dev tool: the decode step on e4m3 weights (tv_gemv_fp8w_fwd) against tv_gemv_bf16_fwd on the same rounded weights, in
one process -> profiles/fp8w_decode.json.

  roles   the products of one Nemotron-Nano-9B-v2 decode token (in_proj, out_proj, up, down, qkv, o_proj, lm_head) at
          M = 1 and 4: microseconds a launch, and the fraction of the HBM peak over the WEIGHT bytes each kernel streams
          (fp8: N K, bf16: 2 N K).  Each role's launches cycle through enough distinct matrices that none is found in the
          256 MB Infinity Cache, captured as one graph and replayed between two events, the two kernels alternating.
  step    the captured decode step at bench.py --config decode's geometry (the cache of a 32 868-token prefill), bf16 on
          the rounded weights (TV_FP8W=0 at capture) against fp8, two steppers on clones of one cache, alternating.
  logits  relative rms difference of one decode step's logits between the ORIGINAL synthetic weights and the rounded
          ones.  Synthetic Gaussian weights say little about a trained checkpoint: recorded, not judged.

usage (GPU box): python timeviper_amd/devtools/bench_fp8w.py [--skip-step] [--out profiles/fp8w_decode.json]"""
import argparse
import json
import os
import pathlib
import sys

import torch

ROOT = pathlib.Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
from timeviper_amd import kernels as K      # noqa: E402

DEV = torch.device("cuda", 0)
HBM_PEAK_GBS = 8000.0
TOK_PER_FRAME = 16                              # (bench.py)


def graph_us(calls, reps=10):
    """Microseconds per launch of the launches in `calls`, replayed back to back as one graph between two events."""
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        for fn in calls:
            fn()
        st.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=st):
            for fn in calls:
                fn()
        graph.replay()
        st.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        for _ in range(reps):
            graph.replay()
        e1.record(st)
        st.synchronize()
    return e0.elapsed_time(e1) * 1e3 / (reps * len(calls))


def bench_roles(cfg):
    hid, inter = cfg.hidden_size, cfg.intermediate_size
    d_in = cfg.mamba_num_heads * cfg.mamba_head_dim
    conv = d_in + 2 * cfg.n_groups * cfg.ssm_state_size
    nq, nkv = cfg.num_attention_heads * cfg.head_dim, cfg.num_key_value_heads * cfg.head_dim
    roles = [("in_proj", d_in + conv + cfg.mamba_num_heads, hid, "rmsnorm"), ("out_proj", hid, d_in, "gated"),
             ("up_proj", inter, hid, "rmsnorm"), ("down_proj", hid, inter, "relu2"), ("qkv", nq + 2 * nkv, hid, "rmsnorm"),
             ("o_proj", hid, nq, "none"), ("lm_head", cfg.vocab_size, hid, "none")]
    g = torch.Generator(device=DEV).manual_seed(0)
    out = []
    for name, N, Kd, pro in roles:
        nbuf = max(3, int(700e6 // (N * Kd)) + 1)            # > 256 MB of fp8 matrices (twice that in bf16) per cycle
        base = (torch.randn(N, Kd, device=DEV, generator=g) / Kd ** 0.5).bfloat16()
        mats = []
        for i in range(nbuf):
            w8, scale = K.quantize_rows_e4m3(base.roll(i, 0))
            mats.append((K.dequantize_rows_e4m3(w8, scale), w8, scale))
        del base
        nw = torch.ones(Kd, device=DEV)
        for M in (1, 4):
            x = torch.randn(M, 1, Kd, device=DEV, generator=g).bfloat16()
            d = torch.randn(M, 1, Kd, device=DEV, generator=g).bfloat16()
            s = torch.empty_like(x)
            kw = {"rmsnorm": dict(prologue=K.GEMV_RMSNORM, delta=d, sum_out=s, norm_weight=nw, eps=1e-5),
                  "gated": dict(prologue=K.GEMV_GATED, norm_weight=nw, eps=1e-5, gate=d, group_size=Kd // 8),
                  "relu2": dict(prologue=K.GEMV_RELU2), "none": {}}[pro]
            bf = [lambda W=W: K.gemv_fused(x, W, None, **kw) for W, _, _ in mats]
            f8 = [lambda q=q, sc=sc: K.gemv_fp8w_fused(x, q, sc, None, **kw) for _, q, sc in mats]
            t_bf, t_f8 = [], []
            for _ in range(3):                                # alternating
                t_bf.append(graph_us(bf))
                t_f8.append(graph_us(f8))
            ub, u8 = min(t_bf), min(t_f8)
            row = {"role": name, "N": N, "K": Kd, "M": M, "prologue": pro, "matrices_cycled": nbuf,
                   "bf16_us": round(ub, 2), "fp8_us": round(u8, 2), "bf16_us_runs": [round(t, 2) for t in t_bf],
                   "fp8_us_runs": [round(t, 2) for t in t_f8],
                   "bf16_frac_of_hbm_peak": round(N * Kd * 2 / (ub * 1e-6) / 1e9 / HBM_PEAK_GBS, 4),
                   "fp8_frac_of_hbm_peak": round(N * Kd / (u8 * 1e-6) / 1e9 / HBM_PEAK_GBS, 4),
                   "speedup": round(ub / u8, 3)}
            print(json.dumps(row), flush=True)
            out.append(row)
        del mats
        torch.cuda.empty_cache()
    return out


def bench_step(cfg, frames):
    from timeviper_amd.model import build_synthetic_timeviper
    from timeviper_amd.model.llm.decode_graph import GraphedDecodeStep
    from timeviper_amd.model.llm.nano import HybridMambaAttentionDynamicCache
    vlm = build_synthetic_timeviper(cfg, "siglip-vit-so400m-384px", pdrop_type=None, merge_module="no_merge", device=DEV, seed=0)
    llm = vlm.llm_backbone.llm
    L = frames * TOK_PER_FRAME + 100
    g = torch.Generator(device=DEV).manual_seed(1)
    emb = (torch.randn(1, L, cfg.hidden_size, device=DEV, generator=g) * 0.02).bfloat16()
    host_pos, zero = torch.ones(1, dtype=torch.long), torch.zeros(1, dtype=torch.long)
    res = {"prefill_tokens": L}
    with torch.inference_mode():
        def prefill_and_step():
            cache = HybridMambaAttentionDynamicCache(cfg, 1, dtype=torch.bfloat16, device=DEV)
            tok = llm(inputs_embeds=emb, past_key_values=cache, use_cache=True, cache_position=zero).logits[:, -1].argmax(-1).view(1, 1)
            return cache, tok, llm(input_ids=tok, past_key_values=cache, use_cache=True, cache_position=host_pos).logits[:, -1].float()
        _, _, lg_orig = prefill_and_step()
    n = vlm.quantize_llm_weights_e4m3()
    res["matrices_quantized"] = n
    with torch.inference_mode():
        cache, tok, lg_q = prefill_and_step()
        res["logits_relative_rms_difference_original_vs_rounded_weights"] = round(
            float((lg_q - lg_orig).pow(2).mean().sqrt() / lg_orig.pow(2).mean().sqrt()), 5)
        res["argmax_agrees"] = bool(lg_q.argmax(-1).item() == lg_orig.argmax(-1).item())
        n_steps, rounds = 64, 4
        steppers = {}
        for name, env in (("bf16", "0"), ("fp8", "1")):
            os.environ["TV_FP8W"] = env                      # (read per call: the capture bakes the route of its steps in)
            c = cache.clone()
            c.begin_static_decode(8 + n_steps * rounds + 8)
            stp = GraphedDecodeStep(
                lambda ids, c=c: llm(input_ids=ids, past_key_values=c, use_cache=True, cache_position=host_pos).logits, c, 1, DEV)
            t = tok
            for _ in range(6):
                t = stp.step(t).view(1, 1)
            torch.cuda.synchronize()
            assert stp.graph is not None, stp.capture_error
            steppers[name] = (stp, t)
        os.environ.pop("TV_FP8W")
        times = {"bf16": [], "fp8": []}
        for _ in range(rounds):
            for name in ("bf16", "fp8"):
                stp, t = steppers[name]
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(n_steps):
                    t = stp.step(t).view(1, 1)
                e1.record()
                torch.cuda.synchronize()
                steppers[name] = (stp, t)
                times[name].append(e0.elapsed_time(e1) / n_steps)
        for name in times:
            res[f"{name}_step_ms_runs"] = [round(t, 4) for t in times[name]]
            res[f"{name}_step_ms"] = round(min(times[name]), 4)
        res["step_speedup"] = round(res["bf16_step_ms"] / res["fp8_step_ms"], 3)
        res["steps_per_run"] = n_steps
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "fp8w_decode.json"))
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--skip-roles", action="store_true")
    ap.add_argument("--frames", type=int, default=2048)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_fp8w.py: needs a GPU (there is nothing to measure without one)")
    from timeviper_amd.build import ensure_built
    from timeviper_amd.model.llm.nano import NemotronHConfig
    ensure_built()
    torch.cuda.set_device(0)
    cfg = NemotronHConfig.nemotron_nano_9b_v2()
    doc = {"tool": "timeviper_amd/devtools/bench_fp8w.py", "device": torch.cuda.get_device_name(0), "hbm_peak_gbs": HBM_PEAK_GBS,
           "rows_kernel_rows_per_wave": int(os.environ.get("TV_FP8W_ROWS_R", "2")),
           "method": "graph replays between device events, bf16 and fp8 alternating in one process; best of the runs listed"}
    if not a.skip_roles:
        doc["roles"] = bench_roles(cfg)
    if not a.skip_step:
        doc["decode_step"] = bench_step(cfg, a.frames)
    pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    pathlib.Path(a.out).write_text(json.dumps(doc, indent=1) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
