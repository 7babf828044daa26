"""The row metric of tests/attn_accuracy.py separates a correct attention kernel from a subtly wrong one — on the CPU.

A correct kernel is emulated in torch (fp32 scores, P rounded to the I/O type, fp32 accumulation, output rounded to the
I/O type), in a plain form and in the online-softmax form of the kernels (key tiles, a running maximum, several key
splits merged in fp32 by their log-sum-exp).  Five value-path mutations — each leaves the log-sum-exp correct, so the
suite's tight `lse` checks cannot see them — are applied to the emulation.  The unmutated emulation passes
`assert_rows_close` against `oracle.ops.attention_ref`; every mutation fails it; and, as the record of the gap this
closes, the elementwise `close(o, o_ref, 2e-2, 1e-2)` accepts two of them at 5 000 keys."""
import math

import pytest
import torch

from attn_accuracy import EPS, assert_rows_close, row_bound, row_rel_err
from oracle import ops as R

TILE, SPLITS = 64, 4

# name -> (B, Lq, Lk, Hq, Hkv, D, causal)
CASES = {
    "decode 1000": (1, 1, 1000, 32, 8, 128, True),
    "decode 5000": (1, 1, 5000, 32, 8, 128, True),
    "append T5 3000": (1, 5, 3000, 16, 4, 128, True),
    "non-causal 257x700 d72": (1, 257, 700, 4, 4, 72, False),
    "causal 300x300 d128": (1, 300, 300, 4, 2, 128, True),
}
DTYPES = [torch.bfloat16, torch.float16]
MUTATIONS = ["last_key_dropped", "tile_dropped", "v_rows_swapped", "no_rescale", "equal_merge_weights"]


def _scores(q, k, causal):
    """fp32 scaled scores (B, Hq, Lq, Lk), masked with -inf (bottom-right aligned), and the per-head V (B, Hq, Lk, D)."""
    B, Lq, Hq, D = q.shape
    Lk, rep = k.shape[1], Hq // k.shape[2]
    qf = q.float().permute(0, 2, 1, 3)
    kf = k.float().permute(0, 2, 1, 3).repeat_interleave(rep, dim=1)
    s = qf @ kf.transpose(-1, -2) / math.sqrt(D)
    if causal:
        i, j = torch.arange(Lq)[:, None], torch.arange(Lk)[None, :]
        s = s.masked_fill(j > i + (Lk - Lq), -torch.inf)
    return s


def emulate(q, k, v, causal, dtype, tile=None, splits=1, mutation=None):
    """A correct kernel's arithmetic, or one mutation of it.  tile None: one pass (max, exp, P rounded, P.V, / l).
    tile = keys per step: online softmax inside each of `splits` contiguous key ranges, the partial (O, max, sum) merged
    in fp32 with weights exp(lse_s - lse).  The sum l always adds the UNROUNDED weights: the log-sum-exp stays right
    under every mutation."""
    B, Lq, Hq, D = q.shape
    Lk, rep = k.shape[1], Hq // k.shape[2]
    s = _scores(q, k, causal)
    vf = v.float().permute(0, 2, 1, 3).repeat_interleave(rep, dim=1)
    last = (torch.arange(Lq) + (Lk - Lq)) if causal else torch.full((Lq,), Lk - 1)       # last visible key per query
    mid = (Lk // 2) // TILE * TILE                                                       # first key of the dropped tile

    if mutation == "v_rows_swapped":
        ja, jb = Lk // 3, Lk // 3 + 1
        vf = vf.clone()
        vf[:, :, [ja, jb]] = vf[:, :, [jb, ja]]

    def mutate_p(p, j0):
        """p: rounded weights of the keys j0 .. j0 + n - 1."""
        n = p.shape[-1]
        if mutation == "last_key_dropped":
            rel = last - j0
            rows = ((rel >= 0) & (rel < n)).nonzero().flatten()
            p[:, :, rows, rel[rows]] = 0
        elif mutation == "tile_dropped":
            lo, hi = max(mid - j0, 0), min(mid + TILE - j0, n)
            if lo < hi:
                p[..., lo:hi] = 0
        return p

    def rnd(t):
        return t.to(dtype).float()

    if tile is None:
        m = s.amax(-1, keepdim=True)
        p = torch.exp(s - m)
        l = p.sum(-1, keepdim=True)
        o = (mutate_p(rnd(p), 0) @ vf) / l
        return rnd(o).permute(0, 2, 1, 3)

    chunk = (-(-Lk // splits) + tile - 1) // tile * tile
    parts = []
    for r0 in range(0, Lk, chunk):
        r1 = min(Lk, r0 + chunk)
        m = torch.full((B, Hq, Lq, 1), -torch.inf)
        l = torch.zeros(B, Hq, Lq, 1)
        acc = torch.zeros(B, Hq, Lq, D)
        for j0 in range(r0, r1, tile):
            st = s[..., j0:min(j0 + tile, r1)]
            m_new = torch.maximum(m, st.amax(-1, keepdim=True))
            m_ref = torch.where(torch.isinf(m_new), torch.zeros_like(m_new), m_new)      # no visible key so far
            alpha = torch.exp(m - m_ref)
            p = torch.exp(st - m_ref)
            l = l * alpha + p.sum(-1, keepdim=True)
            pv = mutate_p(rnd(p), j0) @ vf[:, :, j0:j0 + st.shape[-1]]
            acc = (acc if mutation == "no_rescale" else acc * alpha) + pv
            m = m_new
        parts.append((acc, m, l))
    lse_s = torch.stack([m + torch.log(l) for _, m, l in parts])                         # -inf: the split holds no visible key
    o_s = torch.stack([torch.where(l > 0, acc / l.clamp_min(1e-37), torch.zeros_like(acc)) for acc, _, l in parts])
    if mutation == "equal_merge_weights":
        w = torch.full_like(lse_s, 1.0 / len(parts))
    else:
        w = torch.nan_to_num(torch.exp(lse_s - torch.logsumexp(lse_s, dim=0)), nan=0.0)
    return rnd((w * o_s).sum(0)).permute(0, 2, 1, 3)


_INPUTS = {}


def inputs(name, dtype, spiked=False):
    """Seeded q, k, v of a case, rounded to `dtype`, and the oracle's output — computed once and shared.  spiked: one
    late key per kv-head is 3 x the last query's first head of that group: the running maximum jumps by ~ 30 there."""
    key = (name, dtype, spiked)
    if key not in _INPUTS:
        B, Lq, Lk, Hq, Hkv, D, causal = CASES[name]
        g = torch.Generator().manual_seed(len(name) * 1000 + Lk)
        q = torch.randn(B, Lq, Hq, D, generator=g)
        k = torch.randn(B, Lk, Hkv, D, generator=g)
        v = torch.randn(B, Lk, Hkv, D, generator=g)
        if spiked:
            k[:, Lk - 40] = q[:, -1, ::Hq // Hkv] * 3.0
        q, k, v = (t.to(dtype) for t in (q, k, v))
        o_ref, _ = R.attention_ref(q.float(), k.float(), v.float(), causal)
        _INPUTS[key] = (q, k, v, causal, o_ref)
    return _INPUTS[key]


def old_close_accepts(o, o_ref, rtol=2e-2, atol=1e-2):
    err = (o.double() - o_ref.double()).abs()
    return not bool((err > atol + rtol * o_ref.double().abs()).any())


def test_row_rel_err_shape_and_zero_rows():
    ref = torch.zeros(2, 3, 4, 8)
    ref[0, 1, 2] = 1.0
    o = ref.clone()
    assert row_rel_err(o, ref).shape == (2, 3, 4) and float(row_rel_err(o, ref).max()) == 0.0
    assert_rows_close(o, ref, torch.bfloat16, "zero rows")               # zero rows, exactly zero: fine
    o[1, 2, 3, 5] = 1e-30                                                # a zero row that is not exactly zero
    with pytest.raises(AssertionError, match=r"\(1, 2, 3\)"):
        assert_rows_close(o, ref, torch.bfloat16, "zero row")
    o = ref.clone()
    o[0, 1, 2, 0] += 0.1                                                 # rowrel = 0.1 / sqrt(8) = 0.035
    with pytest.raises(AssertionError, match=r"\(0, 1, 2\).*3\.5\d\de-02.*7\.812e-03"):
        assert_rows_close(o, ref, torch.bfloat16, "worst row")
    o[0, 1, 2, 0] = float("nan")
    with pytest.raises(AssertionError):
        assert_rows_close(o, ref, torch.bfloat16, "nan")
    assert row_bound(torch.bfloat16) == 2.0 ** -7 and row_bound(torch.float16) == 2.0 ** -10


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("name", list(CASES))
def test_emulated_correct_kernel_passes(name, dtype):
    """Plain and online / split forms, on the plain and on the spiked inputs: under the bound, and near the 0.77 eps the
    bound's derivation quotes (under 1.2 eps: the headroom of the bound is real)."""
    for spiked in (False, True):
        q, k, v, causal, o_ref = inputs(name, dtype, spiked)
        for kw in ({}, {"tile": TILE, "splits": SPLITS}, {"tile": 32, "splits": 11}):
            o = emulate(q, k, v, causal, dtype, **kw)
            mx = assert_rows_close(o, o_ref, dtype, f"{name} {kw} spiked={spiked}")
            assert mx < 1.2 * EPS[dtype], mx


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("mutation", MUTATIONS)
@pytest.mark.parametrize("name", list(CASES))
def test_every_mutation_fails_the_row_metric(name, mutation, dtype):
    """The mutated emulation exceeds 2 eps on some row, on every case.  no_rescale runs on the spiked inputs (the running
    maximum has to move late for the missing rescale to matter); the others on the plain ones."""
    q, k, v, causal, o_ref = inputs(name, dtype, spiked=(mutation == "no_rescale"))
    online = mutation in ("no_rescale", "equal_merge_weights")
    forms = [{"tile": TILE, "splits": SPLITS}] if online else [{}, {"tile": TILE, "splits": SPLITS}]
    for kw in forms:
        o = emulate(q, k, v, causal, dtype, mutation=mutation, **kw)
        mx = float(row_rel_err(o, o_ref).max())
        print(f"{name} {mutation} {kw}: max rowrel {mx:.3e} = {mx / row_bound(dtype):.1f} x bound")
        with pytest.raises(AssertionError, match="relative error"):
            assert_rows_close(o, o_ref, dtype, f"{name} {mutation}")


def test_smallest_mutation_effect_is_well_above_the_bound():
    """The figure that caps any per-kernel raise of the bound (no bound above half of it): the smallest effect over these
    cases and mutations in bf16 stays at least 1.6 x above 2 eps — the margin the bound's derivation quotes (0.013
    against 0.0078).  With these seeds it is 0.0196: the last key dropped from the 5 000-key decode."""
    worst = min(float(row_rel_err(emulate(*inputs(name, torch.bfloat16, m == "no_rescale")[:4], torch.bfloat16,
                                          mutation=m, tile=TILE, splits=SPLITS),
                                  inputs(name, torch.bfloat16, m == "no_rescale")[4]).max())
                for name in CASES for m in MUTATIONS)
    print(f"smallest mutation effect (bf16): {worst:.3e}")
    assert worst >= 1.6 * row_bound(torch.bfloat16), worst


@pytest.mark.parametrize("mutation", ["last_key_dropped", "v_rows_swapped"])
def test_old_elementwise_check_accepts_the_mutation_at_5000_keys(mutation):
    """The record of the gap: `close(o, o_ref, 2e-2, 1e-2)` — the check every attention output had — passes these two
    wrong kernels on the 5 000-key decode case, element for element; the row metric does not."""
    q, k, v, causal, o_ref = inputs("decode 5000", torch.bfloat16)
    o = emulate(q, k, v, causal, torch.bfloat16, mutation=mutation)
    assert old_close_accepts(o, o_ref), "the old check sees this mutation after all"
    with pytest.raises(AssertionError, match="relative error"):
        assert_rows_close(o, o_ref, torch.bfloat16, mutation)
