"""Dev tool: the Mamba side of a continuation (T tokens behind a prefilled cache) at Nemotron-Nano-9B-v2 dims — the 27
layers' states (27 x 5.2 MB fp32, no launch finds its state in a cache), one launch sequence per layer in one hipGraph:
  seq    tv_selective_state_update_seq, T tokens in one launch
  steps  T back-to-back launches of tv_selective_state_update (what T decode steps run)
  scan   mamba_chunk_scan_combined(initial_states=cached state, L = T) (the prefill scan from the cached state)
and the attention side: tv_attn_append_fwd at T in {1, 2, 4, 8, 16} against a 32 868-key cache beside flash_attn_func(causal)
and T calls of tv_attn_decode_fwd.  (An end-to-end continuation against graphed decode steps is not part of this tool.)
Event-timed, 3 warm-up replays, best of 5 x 10 replays; writes a JSON file (default profiles/continue_kernels.json).
`CONTINUE_T_SEQ` (model/llm/nano.py) is the largest T at which `seq` is the fastest of the three.
usage (GPU box): python timeviper_amd/devtools/bench_continue.py [out.json]"""
import json
import pathlib
import sys

import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parents[2]))
from timeviper_amd import kernels as K      # noqa: E402

DEV = torch.device("cuda", 0)
H, P, G, N, LAYERS = 128, 80, 8, 128, 27
TS = (1, 2, 4, 8, 16, 32, 64, 128)


def timed(fn, st):
    """us per layer of `fn(layer_state)` over the 27 layers, replayed as one graph"""
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
        for _ in range(5):
            e0.record(st)
            for _ in range(10):
                graph.replay()
            e1.record(st)
            st.synchronize()
            best = min(best, e0.elapsed_time(e1) / 10 / LAYERS * 1e3)
    return best


def timed_plain(fn, st, reps=20):
    """us per call, event-timed on a side stream (eager launches: the attention kernels run for tens of microseconds)"""
    with torch.cuda.stream(st):
        for _ in range(3):
            fn()
        st.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        best = 1e9
        for _ in range(5):
            e0.record(st)
            for _ in range(reps):
                fn()
            e1.record(st)
            st.synchronize()
            best = min(best, e0.elapsed_time(e1) / reps * 1e3)
    return best


def bench_attention(st, Lk=32868, Hq=40, Hkv=8):
    """tv_attn_append_fwd at T query tokens against the 2 048-frame cache, beside flash_attn_func(causal=True) on the same
    tensors (the path such a call took before) and T calls of tv_attn_decode_fwd; fraction of the K / V read roof (8 TB/s)."""
    g = torch.Generator(device=DEV).manual_seed(1)
    k = torch.randn(1, Lk, Hkv, 128, device=DEV, generator=g).bfloat16()
    v = torch.randn(1, Lk, Hkv, 128, device=DEV, generator=g).bfloat16()
    kv_bytes = 2 * Lk * Hkv * 128 * 2
    rows = []
    for T in (1, 2, 4, 8, 16):
        q = torch.randn(1, T, Hq, 128, device=DEV, generator=g).bfloat16()
        q1 = q[:, :1].contiguous()
        r = {"T": T, "append_us": timed_plain(lambda: K.flash_attn_append(q, k, v), st),
             "prefill_kernel_us": timed_plain(lambda: K.flash_attn_func(q, k, v, causal=True), st) if T > 1 else None,
             "decode_x_T_us": timed_plain(lambda: [K.flash_attn_decode(q1, k, v) for _ in range(T)], st)}
        r["append_roof_fraction"] = kv_bytes / r["append_us"] / 1e3 / 8000
        rows.append(r)
        print(f"attention T {T:3d}: append {r['append_us']:8.1f} us ({r['append_roof_fraction']:.2f} of the K / V read roof)   "
              f"flash_attn_func {r['prefill_kernel_us'] or float('nan'):8.1f} us   {T} x decode {r['decode_x_T_us']:8.1f} us",
              flush=True)
    return {"Lk": Lk, "Hq": Hq, "Hkv": Hkv, "kv_bytes": kv_bytes, "rows": rows}


def main():
    out = pathlib.Path(sys.argv[1]) if len(sys.argv) > 1 else \
        pathlib.Path(__file__).resolve().parents[2] / "profiles" / "continue_kernels.json"
    g = torch.Generator(device=DEV).manual_seed(0)
    states = [torch.randn(1, H, P, N, device=DEV, generator=g) for _ in range(LAYERS)]
    A = -(torch.rand(H, device=DEV, generator=g) * 15 + 1)
    D, bias = torch.ones(H, device=DEV), torch.full((H,), -2.0, device=DEV)
    st = torch.cuda.Stream()
    rows = []
    for T in TS:
        x = torch.randn(1, T, H, P, device=DEV, generator=g).bfloat16()
        dt = torch.randn(1, T, H, device=DEV, generator=g).bfloat16()
        # group-major storage, as causal_conv1d_xbc hands B / C over
        Bm = (torch.randn(1, G, T, N, device=DEV, generator=g) * 0.5).bfloat16().transpose(1, 2)
        Cm = (torch.randn(1, G, T, N, device=DEV, generator=g) * 0.5).bfloat16().transpose(1, 2)
        xs = [x[:, t].contiguous() for t in range(T)]
        dts = [dt[:, t].contiguous() for t in range(T)]
        Bs = [Bm[:, t].contiguous() for t in range(T)]
        Cs = [Cm[:, t].contiguous() for t in range(T)]

        def seq():
            for s in states:
                K.selective_state_update_seq(s, x, dt, A, Bm, Cm, D=D, dt_bias=bias, dt_softplus=True)

        def steps():
            for s in states:
                for t in range(T):
                    K.selective_state_update(s, xs[t], dts[t], A, Bs[t], Cs[t], D=D, dt_bias=bias, dt_softplus=True)

        def scan():
            for s in states:
                K.mamba_chunk_scan_combined(x, dt, A, Bm, Cm, chunk_size=128, D=D, dt_bias=bias, dt_softplus=True,
                                            initial_states=s, return_final_states=True)

        r = {"T": T, "seq_us": timed(seq, st), "steps_us": timed(steps, st), "scan_us": timed(scan, st)}
        r["state_bytes"] = 2 * states[0].numel() * 4
        r["seq_GBps"] = r["state_bytes"] / r["seq_us"] / 1e3
        rows.append(r)
        print(f"T {T:4d}: seq {r['seq_us']:8.2f} us   {T} steps {r['steps_us']:8.2f} us   scan(L={T}) {r['scan_us']:8.2f} us "
              f"per layer; seq moves the state at {r['seq_GBps']:7.1f} GB/s", flush=True)
    attn = bench_attention(st)
    best = [r["T"] for r in rows if r["T"] > 1 and r["seq_us"] <= min(r["steps_us"], r["scan_us"])]
    res = {"shape": {"H": H, "P": P, "G": G, "N": N, "layers": LAYERS, "dtype": "bf16"}, "rows": rows, "attention": attn,
           "t_seq": max(best) if best else 1, "device": torch.cuda.get_device_name(0)}
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(res, indent=1) + "\n")
    print("t_seq", res["t_seq"], "->", out)


if __name__ == "__main__":
    main()
