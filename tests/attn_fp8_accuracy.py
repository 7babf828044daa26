"""Judging `tv_flash_attn_fp8_fwd` (csrc/attention_fp8.hip) per output row: a CPU emulation of its arithmetic, value-path
mutations of it, inputs whose answer is known in closed form, and the row bound for random inputs.

Emulation (`fp8_attention_emulated`): q, k, v through `oracle.ops.fp8_quantise_ref` (one e4m3 scale per (batch, head)),
fp32 scores, p~ = 2^8 exp2(s - m) rounded to `torch.float8_e4m3fn`, the row sum over the UNROUNDED p~, fp32 P.V, one
rounding to the output type.  Every mutation touches the value path only, so the log-sum-exp stays right.

Closed-form inputs — e4m3 holds them exactly (up to one common factor), so the fp8 rounding vanishes and the 2 eps row
bound of tests/attn_accuracy.py applies (tests/test_attn_fp8_accuracy_cpu.py):
  * key identity  k = 0, v[j] a signature of (batch, key, head, d) over {0, +-1, +-1/2, +-1/4, +-1/8} with a +-1 in every
                  (batch, head): amax = 1, 440 v rounds to 448 v for every symbol, p~ = 2^8 exactly and the fp32 sums are
                  multiples of 2^11 below 2^27: the output is 448/440 x the mean of V over the visible keys.
  * one hot key   keys are random sign vectors, q = 4 k[hot]: both become 448/440 x themselves; every other weight is
                  below 2^-18 of the hot one, p~ < 2^-10 rounds to zero in e4m3 (checked in fp64 by the builder) and the
                  output is the quantised v[hot].  At head_dim 8 two of a few hundred random sign vectors coincide: there
                  the keys are distinct sign vectors (at most 256 keys) and q = 32 k[hot].

Random inputs: `FP8_ROW_BOUND` = 2^-4 (half an e4m3 ulp of one weight).  Measured by the CPU test on the random inputs of
the GPU tests (RANDOM_SHAPES and the one-head-scaled case in bf16 and fp16; the spiked, blind-rows, packed, output-view
and switch cases in bf16: 27 input sets, head_dim >= 64):
  * largest row error of the emulation 0.0414 (bf16 (3, 729, 729) d72), x 1.5 for what the matrix pipe's accumulation
    and exp2 add (about 1e-3 each) = 0.0620: within 1 % of 2^-4 = 0.0625, which is used;
  * smallest effect of a mutation on these inputs 0.186 (the tail tile of 129 x 129 causal: one key, seen by one query;
    next 0.195, the last key dropped at 50 x 700): the bound is 0.34 of it, under the half it may not exceed.
    `scale_of_other_head` moves a row by the ratio of two heads' amax — 4 to 25 % on plain random data, which a bound on
    random data cannot separate from rounding everywhere: it is judged on the inputs whose heads differ in scale (one
    (batch, kv-head) of V times 2^-6: effect 63; the spiked case: 19) and by the one-hot cases, whose neighbouring heads
    differ by factors of two.
On the closed-form inputs the emulation stays under 0.9 eps and the smallest mutation effect is 36 x the 2 eps bound."""
import functools
import math

import torch

from attn_accuracy import EPS, assert_rows_close, row_bound, row_rel_err  # noqa: F401  (re-exported for the tests)
from oracle import ops as R

FP8_ROW_BOUND = 2.0 ** -4
QMAX, E4M3_TOP = 440.0, 448.0          # the quantiser's target for max |x| and the e4m3 value it rounds to
TILE = 64

MUTATIONS = ["last_key_dropped", "tail_tile_dropped", "tile_dropped", "v_rows_swapped", "tile_key_permutation",
             "scale_of_other_head"]


def visible_last(Lq, Lk, causal):
    """Index of the last key each query sees (bottom-right aligned causal mask); negative: no visible key."""
    return torch.arange(Lq) + (Lk - Lq) if causal else torch.full((Lq,), Lk - 1)


def swapped_keys(Lk):
    """The two keys `v_rows_swapped` exchanges: the first two of the middle tile (one of the one-hot positions)."""
    ja = (Lk - 1) // TILE // 2 * TILE
    return (ja, ja + 1) if ja + 1 < Lk else None


# ------------------------------------------------------------------ emulation
def fp8_attention_emulated(q, k, v, causal, out_dtype, mutation=None):
    """The kernel's arithmetic in torch on the CPU (one pass over the keys), or one mutation of it.  Returns (o, lse):
    o (B, Lq, Hq, D) in `out_dtype`, lse (B, Hq, Lq) fp32; rows without a visible key are zero with lse = -inf."""
    assert mutation is None or mutation in MUTATIONS, mutation
    B, Lq, Hq, D = q.shape
    Lk, Hkv = k.shape[1], k.shape[2]
    rep = Hq // Hkv
    qd, kd = R.fp8_quantise_ref(q), R.fp8_quantise_ref(k)
    if mutation == "scale_of_other_head":                      # V dequantised with the next (batch, head)'s amax
        vf = v.float()
        amax = vf.abs().amax(dim=(1, 3), keepdim=True)
        qs = torch.where(amax > 0, torch.full_like(amax, QMAX) / amax, torch.ones_like(amax))   # as fp8_quantise_ref
        other = qs.reshape(B * Hkv).roll(-1).reshape(B, 1, Hkv, 1)
        vd = (vf * qs).to(torch.float8_e4m3fn).float() / other
    else:
        vd = R.fp8_quantise_ref(v)
    qf = qd.permute(0, 2, 1, 3)
    kf = kd.permute(0, 2, 1, 3).repeat_interleave(rep, dim=1)
    vf = vd.permute(0, 2, 1, 3).repeat_interleave(rep, dim=1).contiguous()
    s = (qf @ kf.transpose(-1, -2)) * (math.log2(math.e) / math.sqrt(D))          # log2 domain, fp32
    last = visible_last(Lq, Lk, causal)
    if causal:
        s = s.masked_fill(torch.arange(Lk)[None, :] > last[:, None], -torch.inf)
    m = s.amax(-1, keepdim=True)
    m = torch.where(torch.isinf(m), torch.zeros_like(m), m)                      # no visible key: any finite base
    p = torch.exp2(s - m + 8.0)
    l = p.sum(-1, keepdim=True)
    p8 = p.to(torch.float8_e4m3fn).float()

    if mutation == "last_key_dropped":
        rows = (last >= 0).nonzero().flatten()
        p8[:, :, rows, last[rows]] = 0
    elif mutation == "tail_tile_dropped":
        p8[..., (Lk - 1) // TILE * TILE:] = 0
    elif mutation == "tile_dropped":
        p8[..., TILE:2 * TILE] = 0
    elif mutation == "v_rows_swapped" and swapped_keys(Lk):
        ja, jb = swapped_keys(Lk)
        vf[:, :, [ja, jb]] = vf[:, :, [jb, ja]]
    elif mutation == "tile_key_permutation":
        j = torch.arange(Lk)
        w = j % TILE
        src = torch.where((w >= 4) & (w < 8), j + 4, torch.where((w >= 8) & (w < 12), j - 4, j))
        src = torch.where(src < Lk, src, j)
        vf = vf[:, :, src]

    o = torch.where(l > 0, (p8 @ vf) / l.clamp_min(1e-37), torch.zeros(()))
    lse = torch.where(l > 0, (m - 8.0) * math.log(2.0) + torch.log(l), torch.full_like(l, -torch.inf))
    return o.to(out_dtype).permute(0, 2, 1, 3), lse.squeeze(-1)


def old_check_accepts(o, ref, rel_l2=4.5e-2, rtol=6e-2, atol=5e-2, vmax=4.5):
    """`check(o, ref, TOL_VS_QUANTISED_ORACLE, ...)` of tests/test_attention_fp8_gpu.py as a predicate."""
    o, ref = o.double(), ref.double()
    if not ((o - ref).norm() / ref.norm()).item() < rel_l2:
        return False
    return not bool(((o - ref).abs() > atol * vmax + rtol * ref.abs()).any())


# ------------------------------------------------------------------ closed-form inputs
SYMBOLS = torch.tensor([0, 1, -1, 0.5, -0.5, 0.25, -0.25, 0.125, -0.125], dtype=torch.float64)


@functools.lru_cache(maxsize=None)
def identity_case(B, Lq, Lk, Hq, Hkv, D, causal, dtype):
    """-> q, k, v (CPU, `dtype`), o_ref (B, Lq, Hq, D) fp64, lse_ref (B, Hq, Lq) fp64."""
    g = torch.Generator().manual_seed(Lq * 7 + Lk + D)
    q = torch.randn(B, Lq, Hq, D, generator=g).to(dtype)
    k = torch.zeros(B, Lk, Hkv, D, dtype=dtype)
    b, j = torch.arange(B)[:, None, None, None], torch.arange(Lk)[None, :, None, None]
    h, d = torch.arange(Hkv)[None, None, :, None], torch.arange(D)[None, None, None, :]
    # (B, Lk, Hkv, D) fp64; period 251 in the key index (a period of 9 would sum to zero over any nine keys in a row)
    sig = SYMBOLS[(j * 131 + d * 17 + h * 29 + b * 53) % 251 % 9].clone()
    sig[:, 0, :, 0] = 1.0 - 2.0 * (torch.arange(Hkv) % 2).double()           # a +-1 in every (batch, head): amax = 1
    v = sig.to(dtype)
    # the exactness claims: the I/O type holds the symbols, 440 x symbol rounds to 448 x symbol, so that the quantiser
    # returns 448/440 v (uniformly), and the fp32 sums of 2^8 x 448 v stay multiples of 2^11 below 2^27
    assert torch.equal(v.double(), sig)
    assert torch.equal((v.float() * QMAX).to(torch.float8_e4m3fn).double(), sig * E4M3_TOP)
    assert torch.allclose(R.fp8_quantise_ref(v).double(), sig * (E4M3_TOP / QMAX), rtol=1e-6, atol=0)
    assert torch.equal(sig * E4M3_TOP * 2 ** 8 % 2 ** 11, torch.zeros_like(sig)) and Lk * E4M3_TOP * 2 ** 8 < 2 ** 27
    last = visible_last(Lq, Lk, causal)
    csum = torch.cumsum(sig, dim=1)                                          # exact in fp64
    mean = csum[:, last.clamp_min(0)] / (last + 1).clamp_min(1)[None, :, None, None].double()
    mean = torch.where((last >= 0)[None, :, None, None], mean, torch.zeros(()).double())
    o_ref = (mean * (E4M3_TOP / QMAX)).repeat_interleave(Hq // Hkv, dim=2)
    n = (last + 1).clamp_min(0).double()
    lse_ref = torch.log(n)[None, None, :].expand(B, Hq, Lq)                  # log 0 = -inf: no visible key
    return q, k, v, o_ref, lse_ref


def hot_candidates(Lk):
    """Key positions of the one-hot case, in the order the rows take them: the first key, the last visible one (-1), both
    sides of every multiple of 64 (so of 128 and of 384), then every key — every residue modulo 64 (the tile's key
    permutation) once the rows suffice."""
    edges = [p for mult in range(TILE, Lk, TILE) for p in (mult - 1, mult)]
    rest = [(i * 37) % Lk for i in range(Lk)] if Lk % 37 else list(range(Lk))   # 37 odd and prime: a permutation
    return [0, -1] + edges + rest


@functools.lru_cache(maxsize=None)
def one_hot_case(B, Lq, Lk, Hq, Hkv, D, causal, dtype):
    """-> q, k, v (CPU, `dtype`), o_ref (B, Lq, Hq, D) fp64, lse_ref (B, Hq, Lq) fp64, hot (B, Lq, Hq; -1: no visible key)."""
    g = torch.Generator().manual_seed(Lq * 11 + Lk + D)
    rep = Hq // Hkv
    if D == 8:         # two of a few hundred random sign vectors coincide: take distinct ones, and a steeper query
        assert Lk <= 256
        code = (torch.arange(Lk)[None, :, None] * 37 + torch.arange(Hkv)[None, None, :] * 11 + torch.arange(B)[:, None, None] * 5) % 256
        k = (((code[..., None] >> torch.arange(8)) & 1) * 2 - 1).to(dtype)
        steep = 32.0   # two keys differ in a sign or more: 32 x (448/440)^2 x 2 / sqrt(8) = 23 between their scores
    else:
        k = (torch.randint(0, 2, (B, Lk, Hkv, D), generator=g) * 2 - 1).to(dtype)
        steep = 4.0
    v = torch.randn(B, Lk, Hkv, D, generator=g)
    v = (v * 2.0 ** (torch.arange(B * Hkv).reshape(B, 1, Hkv, 1) % 3)).to(dtype)     # neighbouring heads: other scales
    last = visible_last(Lq, Lk, causal)
    cands = hot_candidates(Lk)
    hot = torch.empty(B, Lq, Hq, dtype=torch.long)
    r = 0
    for b in range(B):
        for i in range(Lq):
            vis = int(last[i])
            for h in range(Hq):
                # (causal, several tokens: one head of every token, another one each, takes its last visible key)
                c = -1 if (causal and Lq > 1 and h == i % Hq) else cands[r % len(cands)]
                hot[b, i, h] = max(vis, -1) if (c < 0 or c > vis) else c
                r += 1
    bi = torch.arange(B)[:, None, None].expand(B, Lq, Hq)
    hk = (torch.arange(Hq) // rep)[None, None, :].expand(B, Lq, Hq)
    q = (k[bi, hot.clamp_min(0), hk].float() * steep).to(dtype)
    # the exactness claims: q and k are 448/440 x themselves after the quantiser, and every other visible key's weight
    # is below 2^-18 of the hot one (p~ < 2^-10: e4m3 rounds it to zero; 2^-10 itself ties to even, zero)
    qd, kd, vd = R.fp8_quantise_ref(q).double(), R.fp8_quantise_ref(k).double(), R.fp8_quantise_ref(v).double()
    assert torch.allclose(qd, q.double() * (E4M3_TOP / QMAX), rtol=1e-6, atol=0)
    assert torch.allclose(kd, k.double() * (E4M3_TOP / QMAX), rtol=1e-6, atol=0)
    s = torch.einsum("bihd,bjhd->bhij", qd, kd.repeat_interleave(rep, dim=2)) / math.sqrt(D)
    s = s.masked_fill(torch.arange(Lk)[None, :] > last[:, None], -torch.inf)
    hot_t = hot.permute(0, 2, 1)                                              # (B, Hq, Lq)
    seen = hot_t >= 0
    s_hot = s.gather(-1, hot_t.clamp_min(0)[..., None]).squeeze(-1)
    others = s.scatter(-1, hot_t.clamp_min(0)[..., None], -torch.inf)
    gap = (s_hot[..., None] - others)[seen]
    assert float(gap.min()) > 18.5 * math.log(2.0), f"a second key weighs {math.exp(-float(gap.min())):.2e} of the hot one"
    rest = torch.exp(others - s_hot[..., None]).sum(-1)
    lse_ref = torch.where(seen, s_hot + torch.log1p(rest), torch.full_like(s_hot, -torch.inf))
    o_ref = torch.where(seen.permute(0, 2, 1)[..., None], vd[bi, hot.clamp_min(0), hk], torch.zeros(()).double())
    return q, k, v, o_ref, lse_ref, hot


# The Latin squares of tests/test_attn_fp8_accuracy_gpu.py: every key count once per family, the other axes cycled with
# different offsets in the two families.  Key counts: 1, 2, 3, 4 and 5 stages of 128 keys (each its own path through the
# counted waits; from 385 keys a ring slot is reused) and both sides of a tile, a stage and the first ring wrap.  Query
# counts: both sides of the switch from the 4-wave to the 8-wave kernel at 128.  Head dims: DT = 2 (8, 64), 3 (72, 88,
# 96) and 4 (104, 128) d-tiles, zero padding at all but 128.  Causal with Lk > Lq (bottom-right alignment) and with
# Lq > Lk (rows without a visible key).
LKS = [1, 63, 64, 65, 127, 128, 129, 256, 257, 384, 385, 513]
LQS = [1, 33, 128, 129, 257]
HEADS = [(2, 2), (10, 2), (7, 1)]                   # head ratios 1:1, 5:1, 7:1
DS_IDENTITY = [8, 64, 72, 88, 96, 104, 128]
DS_ONE_HOT = [64, 72, 88, 96, 104, 128]
BATCH = 2
IDENTITY_CASES = [(BATCH, LQS[i % 5], Lk, *HEADS[i % 3], DS_IDENTITY[i % 7], bool(i % 2)) for i, Lk in enumerate(LKS)]
ONE_HOT_CASES = [(BATCH, LQS[(i + 2) % 5], Lk, *HEADS[(i + 1) % 3], DS_ONE_HOT[(i + 3) % 6], bool((i + 1) % 2))
                 for i, Lk in enumerate(LKS)]
ONE_HOT_CASES += [(BATCH, 33, 128, 10, 2, 8, True), (BATCH, 129, 65, 2, 2, 8, False)]     # head_dim 8: distinct keys


# ------------------------------------------------------------------ random inputs
RANDOM_SHAPES = [                                   # B, Lq, Lk, Hq, Hkv, D, causal: test_attention_fp8_gpu.py's eight ...
    (1, 300, 300, 4, 2, 128, True),
    (1, 1000, 1000, 14, 2, 128, True),
    (2, 77, 500, 4, 4, 64, False),
    (3, 729, 729, 2, 2, 72, False),
    (2, 1025, 1025, 2, 2, 88, False),
    (1, 50, 700, 8, 2, 128, True),
    (1, 257, 129, 2, 1, 96, False),
    (1, 640, 640, 5, 1, 128, True),
    (2, 130, 65, 4, 2, 72, True),                   # ... causal with more queries than keys, one key past a tile
    # 8-wave kernel by one query, ring wrap by one key.  That key is the whole tail tile and only the last query sees
    # it: 12 rows carry `tail_tile_dropped`.  With 12 / 4 heads its effect is 0.244; with 6 / 2 or 10 / 2 (0.11, 0.08) this
    # shape broke the condition on FP8_ROW_BOUND, so the head counts were changed, not the bound.
    (1, 129, 385, 12, 4, 88, True),
]


@functools.lru_cache(maxsize=None)
def random_case(B, Lq, Lk, Hq, Hkv, D, causal, dtype, scaled_head=False):
    """-> q, k, v (CPU, `dtype`; the seed and draws of test_attention_fp8_gpu.py), o_ref, lse_ref of `attention_ref` on the
    quantised inputs.  scaled_head: V of the last (batch, kv-head) times 2^-6."""
    g = torch.Generator().manual_seed(Lq * 5 + Lk + D)
    q = torch.randn(B, Lq, Hq, D, generator=g).to(dtype)
    k = torch.randn(B, Lk, Hkv, D, generator=g).to(dtype)
    v = torch.randn(B, Lk, Hkv, D, generator=g).to(dtype)
    if scaled_head:
        v[B - 1, :, Hkv - 1] *= 2.0 ** -6
    o_ref, lse_ref = R.attention_ref(R.fp8_quantise_ref(q), R.fp8_quantise_ref(k), R.fp8_quantise_ref(v), causal)
    return q, k, v, o_ref, lse_ref


SCALED_HEAD_SHAPE = (2, 129, 257, 4, 2, 72, False)
BLIND_ROWS_SHAPE = (2, 300, 40, 4, 2, 72, True)      # bf16 only: causal, 260 queries without a visible key
PACKED_SHAPE = (2, 129, 129, 4, 2, 72, True)         # bf16 only: q, k, v sliced out of one buffer
OUTPUT_VIEW_SHAPE = (2, 129, 200, 4, 2, 72, False)   # bf16 only: output written into a view


SWITCH_SHAPE = (1, 512, 512, 4, 2, 128, True)        # bf16 only: test_fp8_switch_routes_flash_attn_func


@functools.lru_cache(maxsize=None)
def spiked_case():
    """test_fp8_attention_spiked_max_and_scale_spread's inputs: large running-max jumps at chosen tiles and two heads whose
    magnitudes differ by 100 x.  -> q, k, v (bf16), o_ref on the quantised inputs (causal)."""
    g = torch.Generator().manual_seed(0)
    B, L, H, D = 1, 700, 2, 128
    q = torch.randn(B, L, H, D, generator=g)
    k = torch.randn(B, L, H, D, generator=g)
    v = torch.randn(B, L, H, D, generator=g)
    for pos in (70, 300, 650):
        k[0, pos, :, :] = q[0, 699, :, :] * 3.0
    q[:, :, 1] *= 0.05
    v[:, :, 1] *= 20.0
    q, k, v = (t.bfloat16() for t in (q, k, v))
    o_ref, _ = R.attention_ref(R.fp8_quantise_ref(q), R.fp8_quantise_ref(k), R.fp8_quantise_ref(v), True)
    return q, k, v, o_ref
