"""Branched decoding on the GPU: `tv_attn_branch_fwd` (one query token per branch, a shared prefix, a suffix per branch)
against the fp64 oracle on the concatenated keys of each branch, and the branched step of a bf16 hybrid against single-token
steps on per-branch clones.

Attention outputs are judged per row by `attn_accuracy.assert_rows_close` (2 eps of bf16, derived there from a CPU emulation
of a correct split-and-merge kernel), log-sum-exps by the `close(.., 1e-3, 2e-3)` tests/test_continue_gpu.py uses for the
append kernel.  The model-level bounds are that file's for the same operators in another summation order: relerr < 3e-2 of
the logits per branch and step, 2e-2 of the SSM / conv states."""
import pytest
import torch

from attn_accuracy import assert_rows_close
from oracle import ops as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
D = 128


def close(a, b, rtol, atol, what=""):
    a, b = a.detach().double().cpu(), torch.as_tensor(b).double().cpu()
    assert a.shape == b.shape, (a.shape, b.shape)
    err = (a - b).abs()
    bad = err > atol + rtol * b.abs()
    assert not bad.any(), f"{what}: {bad.sum().item()} / {bad.numel()} out of tolerance, max abs err {err.max().item():.3e}"


def relerr(a, b):
    a, b = a.detach().double().cpu(), torch.as_tensor(b).double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-12)).item()


@pytest.fixture(scope="module")
def K():
    from timeviper_amd import kernels
    return kernels


def _inputs(B, Hq, Hkv, Lp, cap, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g).bfloat16()
    return r(B, 1, Hq, D), r(1, Lp, Hkv, D), r(1, Lp, Hkv, D), r(B, cap, Hkv, D), r(B, cap, Hkv, D)


def _reference(q, kp, vp, ks, vs, ns, scale=None):
    """attention_ref on cat(prefix, suffix_b[:n_b]) per branch (CPU tensors)"""
    outs, lses = [], []
    for b, n in enumerate(ns):
        k = torch.cat([kp, ks[b:b + 1, :n]], dim=1).float()
        v = torch.cat([vp, vs[b:b + 1, :n]], dim=1).float()
        o, lse = R.attention_ref(q[b:b + 1].float(), k, v, False, scale)
        outs.append(o)
        lses.append(lse)
    return torch.cat(outs, dim=0), torch.cat(lses, dim=0)


def _check(K, q, kp, vp, ks, vs, ns, what, lens="device", poison=True):
    """One kernel call on device copies of the CPU tensors (the rows at and beyond n_b NaN), judged against the oracle."""
    B = q.shape[0]
    ksd, vsd = ks.clone(), vs.clone()
    if poison:
        for b, n in enumerate(ns):
            ksd[b, n:] = float("nan")
            vsd[b, n:] = float("nan")
    sl = None if lens is None else torch.tensor(ns, dtype=torch.int32, device=DEV)
    calls = K.flash_attn_branch_calls()
    o, lse = K.flash_attn_branch(q.to(DEV), kp.to(DEV), vp.to(DEV), ksd.to(DEV), vsd.to(DEV), seqlens_suffix=sl,
                                 return_lse=True)
    assert K.flash_attn_branch_calls() == calls + 1, "fell back"
    assert o.shape == (B, 1, q.shape[2], D) and lse.shape == (B, q.shape[2], 1)
    assert torch.isfinite(o.float()).all() and torch.isfinite(lse).all(), what
    o_ref, lse_ref = _reference(q, kp, vp, ks, vs, ns)
    assert_rows_close(o, o_ref, torch.bfloat16, what)
    close(lse, lse_ref, 1e-3, 2e-3, what + " lse")
    return o, lse


SHAPES = [(1, 5, 1), (3, 5, 1), (4, 5, 1), (2, 16, 2), (16, 8, 1), (16, 40, 8)]      # (B, Hq, Hkv)
LPS = [1, 31, 33, 1000, 3001]
NS = [0, 1, 32, 33, 100]
# per shape every prefix length and every suffix length once (a Latin square: 30 of the 150 combinations)
CASES = [(*SHAPES[s], LPS[i], NS[(i + s) % 5]) for s in range(len(SHAPES)) for i in range(5)]


@pytest.mark.parametrize("B,Hq,Hkv,Lp,n", CASES)
def test_kernel_against_the_oracle(K, B, Hq, Hkv, Lp, n):
    """Columns (branch, head) in one, a nearly full, two and eight blocks; prefixes of one key, one step and a bit, several
    splits; suffixes that are empty, one row, one step, one step and a bit, several steps.  The buffers hold spare rows."""
    cap = n + 7
    q, kp, vp, ks, vs = _inputs(B, Hq, Hkv, Lp, cap, 1000 * B + 10 * Hq + Lp + n)
    _check(K, q, kp, vp, ks, vs, [n] * B, f"branch B {B} H {Hq}/{Hkv} Lp {Lp} n {n}")


def test_unequal_device_lengths_on_strided_tensors(K):
    """n = (0, 1, 33, 100) from device memory; prefix and suffixes are views of larger buffers (row and head strides)."""
    B, Hq, Hkv, Lp, cap = 4, 10, 2, 777, 100
    ns = [0, 1, 33, 100]
    q, kp, vp, ks, vs = _inputs(B, Hq, Hkv, Lp, cap, 3)
    g = torch.Generator().manual_seed(4)
    wide = lambda t, rows: torch.randn(t.shape[0], t.shape[1] + rows, t.shape[2] + 1, 2 * D, generator=g).bfloat16()
    kpw, vpw, ksw, vsw = wide(kp, 5), wide(vp, 5), wide(ks, 9), wide(vs, 9)
    for w, t in ((kpw, kp), (vpw, vp), (ksw, ks), (vsw, vs)):
        w[:, :t.shape[1], 1:, D:] = t
    for b, n in enumerate(ns):
        ksw[b, n:] = float("nan")
        vsw[b, n:] = float("nan")
    dev = [w.to(DEV) for w in (kpw, vpw, ksw, vsw)]
    kpd, vpd = (w[:, :Lp, 1:, D:] for w in dev[:2])
    ksd, vsd = (w[:, :cap, 1:, D:] for w in dev[2:])
    assert not kpd.is_contiguous() and not ksd.is_contiguous()
    sl = torch.tensor(ns, dtype=torch.int32, device=DEV)
    calls = K.flash_attn_branch_calls()
    o, lse = K.flash_attn_branch(q.to(DEV), kpd, vpd, ksd, vsd, seqlens_suffix=sl, return_lse=True)
    assert K.flash_attn_branch_calls() == calls + 1
    o_ref, lse_ref = _reference(q, kp, vp, ks, vs, ns)
    assert_rows_close(o, o_ref, torch.bfloat16, "unequal device lengths, strided")
    close(lse, lse_ref, 1e-3, 2e-3, "lse")
    # lengths beyond the capacity are clamped to it, negative ones to 0
    o2 = K.flash_attn_branch(q.to(DEV), kpd, vpd, ksd[:, :33], vsd[:, :33],
                             seqlens_suffix=torch.tensor([-3, 1, 500, 33], dtype=torch.int32, device=DEV))
    o2_ref, _ = _reference(q, kp, vp, ks, vs, [0, 1, 33, 33])
    assert_rows_close(o2, o2_ref, torch.bfloat16, "clamped lengths")
    with pytest.raises(K.TimeViperHipError):
        K.flash_attn_branch(q.to(DEV), kpd, vpd, ksd, vsd, seqlens_suffix=sl.to(torch.int64))


def test_branches_do_not_see_each_other(K):
    """Branch 0 is the victim: the suffix rows of the OTHER branches hold keys that score about 50 above everything else
    for its queries, and values of 1e4.  Every row still meets the bound."""
    B, Hq, Hkv, Lp, n = 3, 4, 1, 200, 40
    q, kp, vp, ks, vs = _inputs(B, Hq, Hkv, Lp, n, 8)
    target = q[0, 0].float().sum(0)                       # q[0, h] . target / sqrt(D) ~ |q|^2 / sqrt(D) ~ 11 per unit
    g = torch.Generator().manual_seed(9)
    ks[1:] = (5.0 * target + 0.1 * torch.randn(B - 1, n, Hkv, D, generator=g)).bfloat16()
    vs[1:] = 1e4
    s = (q[0, 0].float() @ ks[1, 0, 0].float()) / D ** 0.5
    own = torch.einsum("hd,nd->hn", q[0, 0].float(), torch.cat([kp[0, :, 0], ks[0, :, 0]]).float()) / D ** 0.5
    assert (s - own.max(1).values).min() > 25, (s.tolist(), own.max().item())
    o, _ = _check(K, q, kp, vp, ks, vs, [n] * B, "isolation", lens=None, poison=False)
    assert o[0].float().abs().max() < 10


def test_closed_form_two_constant_values(K):
    """Prefix V is one constant vector, branch b's suffix V another: the output is their convex combination with the weight
    that follows from the fp64 log-sum-exps of the two score sets.  Branch 0's largest score lies in its suffix, branch
    1's in the prefix, branch 2 has no suffix rows."""
    B, Hq, Hkv, Lp, n = 3, 8, 2, 500, 50
    q, kp, _, ks, _ = _inputs(B, Hq, Hkv, Lp, n, 12)
    ks[0, 7] = (0.5 * q[0, 0].float().reshape(Hkv, Hq // Hkv, D).sum(1)).bfloat16()      # scores of ~ 5 for every head
    kp[0, 123] = (0.5 * q[1, 0].float().reshape(Hkv, Hq // Hkv, D).sum(1)).bfloat16()
    g = torch.Generator().manual_seed(13)
    cp = torch.randn(D, generator=g).bfloat16()
    cs = torch.randn(B, D, generator=g).bfloat16()
    vp = cp.expand(1, Lp, Hkv, D).contiguous()
    vs = cs[:, None, None, :].expand(B, n, Hkv, D).contiguous()
    ns = [n, n, 0]
    sl = torch.tensor(ns, dtype=torch.int32, device=DEV)
    o = K.flash_attn_branch(q.to(DEV), kp.to(DEV), vp.to(DEV), ks.to(DEV), vs.to(DEV), seqlens_suffix=sl)
    gq = Hq // Hkv
    want = torch.empty(B, 1, Hq, D, dtype=torch.float64)
    for b in range(B):
        for h in range(Hq):
            sp = (kp[0, :, h // gq].double() @ q[b, 0, h].double()) / D ** 0.5
            ss = (ks[b, :ns[b], h // gq].double() @ q[b, 0, h].double()) / D ** 0.5
            lp, ls = torch.logsumexp(sp, 0), (torch.logsumexp(ss, 0) if ns[b] else torch.tensor(-float("inf")).double())
            w = torch.sigmoid(lp - ls)                    # exp(lp) / (exp(lp) + exp(ls))
            want[b, 0, h] = w * cp.double() + (1 - w) * cs[b].double()
            if b < 2 and h == 0:
                assert (ss.max() > sp.max()) == (b == 0)
    assert_rows_close(o, want, torch.bfloat16, "closed form")


def test_range_and_fallback(K):
    """Inside the range every call is one launch of the kernel; B * gq = 144, head_dim 64 and fp16 are refused by the entry
    point and served by the wrapper's fallback, within the same bound."""
    from timeviper_amd import _capi
    lib = _capi.lib()
    q, kp, vp, ks, vs = _inputs(2, 8, 2, 300, 20, 21)
    calls = K.flash_attn_branch_calls()
    for i in range(3):
        _check(K, q, kp, vp, ks, vs, [20, 20], "in range", lens=None, poison=False)
        assert K.flash_attn_branch_calls() == calls + i + 1

    def entry(q, kp, vp, ks, vs):
        B, _, Hq, Dh = q.shape
        o = torch.empty_like(q)
        ws = torch.empty(1 << 20, dtype=torch.uint8, device=DEV)
        return lib.tv_attn_branch_fwd(
            q.data_ptr(), kp.data_ptr(), vp.data_ptr(), ks.data_ptr(), vs.data_ptr(), o.data_ptr(), None, B, kp.shape[1],
            ks.shape[1], None, Hq, kp.shape[2], Dh, q.stride(0), q.stride(2), kp.stride(1), kp.stride(2), vp.stride(1),
            vp.stride(2), ks.stride(0), ks.stride(1), ks.stride(2), vs.stride(0), vs.stride(1), vs.stride(2), o.stride(0),
            o.stride(2), Dh ** -0.5, K._dt(q), ws.data_ptr(), ws.numel(), None)
    g = torch.Generator().manual_seed(22)
    outside = {
        "144 columns": [torch.randn(*s, generator=g).bfloat16() for s in
                        ((16, 1, 9, D), (1, 300, 1, D), (1, 300, 1, D), (16, 20, 1, D), (16, 20, 1, D))],
        "head_dim 64": [torch.randn(*s, generator=g).bfloat16() for s in
                        ((2, 1, 8, 64), (1, 300, 2, 64), (1, 300, 2, 64), (2, 20, 2, 64), (2, 20, 2, 64))],
        "fp16": [torch.randn(*s, generator=g).half() for s in
                 ((2, 1, 8, D), (1, 300, 2, D), (1, 300, 2, D), (2, 20, 2, D), (2, 20, 2, D))],
    }
    for what, ts in outside.items():
        dev = [t.to(DEV) for t in ts]
        calls = K.flash_attn_branch_calls()
        assert entry(*dev) == -2, (what, lib.tv_last_error())
        ns = [13] * ts[0].shape[0]
        o, lse = K.flash_attn_branch(*dev, seqlens_suffix=torch.tensor(ns, dtype=torch.int32, device=DEV), return_lse=True)
        assert K.flash_attn_branch_calls() == calls, what
        o_ref, lse_ref = _reference(*ts, ns)
        assert_rows_close(o, o_ref, ts[0].dtype, "fallback " + what)
        close(lse, lse_ref, 1e-3, 2e-3, what + " lse")


def test_graph_replays_against_growing_suffixes(K):
    """A captured call with device-side lengths; one more suffix row, the lengths incremented, a replay: the eager call on
    the same data."""
    B, Hq, Hkv, Lp, cap, n = 3, 10, 2, 1500, 48, 31
    q, kp, vp, ks, vs = (t.to(DEV) for t in _inputs(B, Hq, Hkv, Lp, cap, 30))
    sl = torch.full((B,), n, dtype=torch.int32, device=DEV)
    pos = torch.full((1,), n, dtype=torch.int64, device=DEV)
    K.flash_attn_branch(q, kp, vp, ks, vs, seqlens_suffix=sl)          # (one call outside the capture)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        o_g = K.flash_attn_branch(q, kp, vp, ks, vs, seqlens_suffix=sl)
    torch.cuda.current_stream().wait_stream(side)
    for step in range(3):
        if step:
            row = torch.randn(B, 1, Hkv, D, generator=torch.Generator().manual_seed(40 + step)).bfloat16().to(DEV)
            ks.index_copy_(1, pos, row)
            vs.index_copy_(1, pos, -row)
            pos += 1
            sl += 1
        graph.replay()
        eager = K.flash_attn_branch(q, kp, vp, ks, vs, seqlens_suffix=sl)
        assert torch.equal(o_g, eager), step
        o_ref, _ = _reference(q.cpu(), kp.cpu(), vp.cpu(), ks.cpu(), vs.cpu(), [n + step] * B)
        assert_rows_close(o_g, o_ref, torch.bfloat16, f"replay {step}")


# ------------------------------------------------------------------------------------------------ model level
def _toy_hybrid_d128(pattern="M-*M*-"):
    """The d128 bf16 toy hybrid of tests/test_continue_gpu.py."""
    from timeviper_amd.model.llm.nano import NemotronHConfig, NemotronHForCausalLM
    torch.manual_seed(11)
    cfg = NemotronHConfig(vocab_size=256, hidden_size=256, intermediate_size=384, num_hidden_layers=len(pattern),
                          hybrid_override_pattern=pattern, num_attention_heads=8, head_dim=128,
                          num_key_value_heads=2, ssm_state_size=16, mamba_num_heads=8,
                          mamba_n_groups=2, mamba_head_dim=16, mamba_chunk_size=16)
    model = NemotronHForCausalLM(cfg).to(DEV).bfloat16().eval()
    with torch.no_grad():
        for blk in model.backbone.layers:
            if blk.block_type == "attention":
                blk.mixer.q_proj.weight.mul_(8.0)
                blk.mixer.k_proj.weight.mul_(8.0)
        model.lm_head.weight.mul_(20.0)
    return cfg, model


N_PREFILL, N_STEPS = 300, 12
MODEL = {}


def _model_case(B):
    """The model, the prefilled parent, the fixed ids of the teacher-forced steps and the reference transcript — single-token
    steps on per-branch clones — computed once per B and left unchanged."""
    from timeviper_amd.model.llm import nano
    if "model" not in MODEL:
        cfg, model = _toy_hybrid_d128()
        ids = torch.randint(0, cfg.vocab_size, (1, N_PREFILL), generator=torch.Generator().manual_seed(7)).to(DEV)
        with torch.inference_mode():
            parent = nano.HybridMambaAttentionDynamicCache(cfg, 1, dtype=torch.bfloat16, device=DEV)
            model(input_ids=ids, past_key_values=parent, use_cache=True, cache_position=torch.zeros(1, dtype=torch.long))
        MODEL["model"] = (cfg, model, parent)
    cfg, model, parent = MODEL["model"]
    if B not in MODEL:
        feed = torch.randint(0, cfg.vocab_size, (B, N_STEPS), generator=torch.Generator().manual_seed(70 + B)).to(DEV)
        clones, logits = [parent.clone() for _ in range(B)], []
        with torch.inference_mode():
            for t in range(N_STEPS):
                logits.append(torch.cat([model(input_ids=feed[b:b + 1, t:t + 1], past_key_values=clones[b], use_cache=True,
                                               cache_position=torch.tensor([N_PREFILL + t])).logits[:, -1]
                                         for b in range(B)], dim=0))
        MODEL[B] = (feed, clones, torch.stack(logits, dim=0))              # (steps, B, V)
    return (cfg, model, parent) + MODEL[B]


def _branched_transcript(model, parent, feed, graphed):
    from timeviper_amd.model.llm.decode_graph import GraphedDecodeStep
    B = feed.shape[0]
    bs = parent.branch(B, suffix_cap=N_STEPS)
    bs.begin_static_decode(N_STEPS)
    host_pos = torch.ones(1, dtype=torch.long)
    step_fn = lambda ids: model(input_ids=ids, past_key_values=bs, use_cache=True, cache_position=host_pos).logits
    stepper = GraphedDecodeStep(step_fn, bs, B, DEV) if graphed else None
    out = []
    with torch.inference_mode():
        for t in range(N_STEPS):
            if stepper is not None:
                stepper.step(feed[:, t:t + 1])
                out.append(stepper.logits.reshape(B, -1).clone())
            else:
                out.append(step_fn(feed[:, t:t + 1].contiguous())[:, -1].clone())
                bs.advance_static_device()
    if stepper is not None:
        assert stepper.capture_error is None and stepper.graph is not None, stepper.capture_error
    return bs, torch.stack(out, dim=0)


def _assert_branched_step(cfg, parent, bs, got, clones, want, what):
    B = want.shape[1]
    for t in range(N_STEPS):
        for b in range(B):
            err = relerr(got[t, b], want[t, b])
            assert err < 3e-2, (what, t, b, err)
    for i, c in enumerate(cfg.hybrid_override_pattern):
        if c == "M":
            for b in range(B):
                assert relerr(bs.ssm_states[i][b], clones[b].ssm_states[i][0]) < 2e-2, (what, i, b)
                assert relerr(bs.conv_states[i][b], clones[b].conv_states[i][0]) < 2e-2, (what, i, b)
        elif c == "*":
            assert bs.prefix[i][0].data_ptr() == parent.key_cache[i].data_ptr()
            assert bs.key_cache[i].shape == (B, N_STEPS, 2, D) and parent.key_cache[i].shape[1] == N_PREFILL
            for b in range(B):
                assert relerr(bs.key_cache[i][b], clones[b].key_cache[i][0, N_PREFILL:]) < 2e-2, (what, i, b)


@pytest.mark.parametrize("B", [2, 4, 5])
def test_branched_step_equals_single_steps_on_clones(K, B, monkeypatch):
    """12 teacher-forced steps: the branch set's logits against single-token steps on per-branch clones, eagerly and under
    GraphedDecodeStep (whose transcript equals the eager one).  B <= 4 rides the fused gemv step, B = 5 the library GEMM."""
    monkeypatch.delenv("TV_ROWS_FUSED", raising=False)
    cfg, model, parent, feed, clones, want = _model_case(B)
    calls = K.flash_attn_branch_calls()
    bs, eager = _branched_transcript(model, parent, feed, graphed=False)
    assert K.flash_attn_branch_calls() == calls + 2 * N_STEPS            # two attention layers, no fallback
    _assert_branched_step(cfg, parent, bs, eager, clones, want, f"eager B {B}")
    bs_g, graphed = _branched_transcript(model, parent, feed, graphed=True)
    print(f"B {B}: graphed vs eager max abs diff {(graphed - eager).abs().max().item():.3e}")
    assert torch.equal(graphed, eager)
    _assert_branched_step(cfg, parent, bs_g, graphed, clones, want, f"graphed B {B}")


def test_branched_step_on_the_rows_route(K, monkeypatch):
    """TV_ROWS_FUSED=1: one token of 5 sequences takes the fused rows step (no conv epilogue: the conv update is its own
    launch)."""
    from timeviper_amd.model.llm import nano
    cfg, model, parent, feed, clones, want = _model_case(5)
    monkeypatch.setenv("TV_ROWS_FUSED", "1")
    x = torch.zeros(5, 1, cfg.hidden_size, dtype=torch.bfloat16, device=DEV)
    one = torch.ones(1, dtype=torch.long)
    with torch.inference_mode():        # the routes are for forwards without autograd, as every decode step is
        assert nano.linear_route(x, parent, one) == "rows" and nano.fused_route(model.backbone, x, parent, one) == "rows"
        assert nano.linear_route(x[:4], parent, one) == "gemv"
    seen = []
    real = K.linear_rows_fused
    monkeypatch.setattr(K, "linear_rows_fused", lambda *a, **kw: (seen.append(a[0].shape), real(*a, **kw))[1])
    bs, got = _branched_transcript(model, parent, feed, graphed=False)
    assert seen and all(s[0] == 5 and s[1] == 1 for s in seen)
    _assert_branched_step(cfg, parent, bs, got, clones, want, "rows route B 5")
