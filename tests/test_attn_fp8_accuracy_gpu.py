"""`tv_flash_attn_fp8_fwd` judged per output row (tests/attn_fp8_accuracy.py): inputs with closed-form answers pin WHICH V
row reaches WHICH (query, head) through the transposed, key-permuted, swizzled V image, the ring of three stages and the
padded head dimension, at the 2 eps row bound; random inputs are held to FP8_ROW_BOUND against the oracle on the quantised
inputs.  tests/test_attn_fp8_accuracy_cpu.py runs an emulation of the kernel on these same inputs: it stays inside the
bounds, and six value-path mutations of it do not.

Every call goes through `fp8_call`, which counts the library calls: the fp8 entry point served it, the bf16 one did not."""
import contextlib
import math

import pytest
import torch

import attn_fp8_accuracy as A
from attn_fp8_accuracy import FP8_ROW_BOUND, assert_rows_close, row_bound

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float16]
IDS = ["bf16", "fp16"]


@pytest.fixture(scope="module")
def K():
    from timeviper_amd import kernels
    return kernels


@contextlib.contextmanager
def entry_point_calls(K):
    """Counts the calls of the two prefill attention entry points of the library (each returning TV_OK) inside the block."""
    lib = K._capi.lib()
    counts = {"tv_flash_attn_fp8_fwd": 0, "tv_flash_attn_fwd": 0}
    real = {name: getattr(lib, name) for name in counts}

    def spy(name):
        def call(*args):
            status = real[name](*args)
            counts[name] += status == 0
            return status
        return call

    for name in counts:
        setattr(lib, name, spy(name))
    try:
        yield counts
    finally:
        for name in counts:
            setattr(lib, name, real[name])


def fp8_call(K, q, k, v, causal):
    """flash_attn_fp8_func on the GPU -> (o, lse); the fp8 entry point, not a fallback, served the call."""
    with entry_point_calls(K) as calls:
        o, lse = K.flash_attn_fp8_func(q.to(DEV), k.to(DEV), v.to(DEV), causal=causal, return_lse=True)
    assert calls == {"tv_flash_attn_fp8_fwd": 1, "tv_flash_attn_fwd": 0}, calls
    return o, lse


def check_lse(lse, lse_ref, tol, what):
    """Rows without a visible key: -inf exactly; the others within `tol`."""
    lse, seen = lse.double().cpu(), torch.isfinite(lse_ref)
    assert torch.equal(torch.isinf(lse) & (lse < 0), ~seen), f"{what}: lse = -inf exactly on the rows without a visible key"
    if seen.any():
        err = float((lse - lse_ref)[seen].abs().max())
        print(f"lse {what}: max |err| {err:.3e}, bound {tol:.0e}")
        assert err < tol, f"{what}: lse off by {err:.3e}"


# ------------------------------------------------------------------ closed form: 2 eps
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", A.IDENTITY_CASES, ids=str)
def test_fp8_key_identity(K, case, dtype):
    """Uniform weights over index-signature V rows: 448/440 x the mean of V over the visible keys; lse = log(n visible)
    within a few fp32 ulps of 8 ln 2 + log(256 n)."""
    q, k, v, o_ref, lse_ref = A.identity_case(*case, dtype)
    o, lse = fp8_call(K, q, k, v, case[6])
    assert_rows_close(o, o_ref, dtype, f"fp8 identity {case}", bound=row_bound(dtype))
    check_lse(lse, lse_ref, 1e-5, f"fp8 identity {case}")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", A.ONE_HOT_CASES, ids=str)
def test_fp8_one_hot_key(K, case, dtype):
    """Each (batch, query, head) has its own key: the quantised v of that key; lse = the hot score of the quantised q and k
    plus log1p of the rest (three fp32 roundings of the dequantisation factor on a score of about 50)."""
    q, k, v, o_ref, lse_ref, _ = A.one_hot_case(*case, dtype)
    o, lse = fp8_call(K, q, k, v, case[6])
    assert_rows_close(o, o_ref, dtype, f"fp8 one-hot {case}", bound=row_bound(dtype))
    check_lse(lse, lse_ref, 1e-4, f"fp8 one-hot {case}")


def test_fp8_causal_rows_without_a_visible_key_are_zero(K):
    """Causal with more queries than keys: the wrapper takes the call (bottom-right alignment), the first Lq - Lk rows see
    nothing and are exactly zero with lse = -inf — whole workgroups of them (no stage at all) and part of one."""
    B, Lq, Lk, Hq, Hkv, D, _ = A.BLIND_ROWS_SHAPE
    q, k, v, o_ref, lse_ref = A.random_case(*A.BLIND_ROWS_SHAPE, torch.bfloat16)
    o, lse = fp8_call(K, q, k, v, True)
    blind = Lq - Lk
    assert torch.equal(o[:, :blind].cpu(), torch.zeros(B, blind, Hq, D, dtype=torch.bfloat16))
    assert bool((lse[:, :, :blind] == -math.inf).all()) and bool(torch.isfinite(lse[:, :, blind:]).all())
    assert_rows_close(o, o_ref, torch.bfloat16, "fp8 causal 300 x 40", bound=FP8_ROW_BOUND)


# ------------------------------------------------------------------ exact scalings (bf16: its exponent range holds 2^-6 o)
SC = (2, 129, 257, 4, 2, 72)


def sixtyfourths(shape, seed):
    """randn rounded to multiples of 1/64: bf16 holds them, and them times 8 or 2^-6, exactly."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(*shape, generator=g) * 64).round().clamp(-255, 255) / 64
    assert torch.equal(x.bfloat16().float(), x)
    return x.bfloat16()


@pytest.fixture(scope="module")
def scaling_inputs(K):
    B, Lq, Lk, Hq, Hkv, D = SC
    q, k, v = sixtyfourths((B, Lq, Hq, D), 1), sixtyfourths((B, Lk, Hkv, D), 2), sixtyfourths((B, Lk, Hkv, D), 3)
    o, lse = fp8_call(K, q, k, v, True)
    return q, k, v, o, lse


def test_fp8_value_scale_is_exact(K, scaling_inputs):
    """v 2^-6 -> o 2^-6, bit for bit: the amax and with it the dequantisation factor scale exactly, the e4m3 image is the
    same.  No absolute threshold or flush in the value path."""
    q, k, v, o, lse = scaling_inputs
    os_, lses = fp8_call(K, q, k, v * 2.0 ** -6, True)
    assert torch.equal(os_.float() * 64, o.float()), (os_.float() * 64 - o.float()).abs().max().item()
    assert torch.equal(lses, lse)


def test_fp8_query_and_key_scales_cancel_exactly(K, scaling_inputs):
    """q 8 with k / 8: both dequantisation factors move by exact powers of two, the same bits come out."""
    q, k, v, o, lse = scaling_inputs
    o2, lse2 = fp8_call(K, q * 8, k / 8, v, True)
    assert torch.equal(o2, o) and torch.equal(lse2, lse)


@pytest.mark.parametrize("b,hk", [(0, 1), (1, 0)])
def test_fp8_value_scale_of_one_head_stays_with_that_head(K, scaling_inputs, b, hk):
    """V of ONE (batch, kv-head) times 2^-6: its query heads' rows scale exactly, every other row keeps its bits — an amax
    taken from another batch or head would move them."""
    q, k, v, o, lse = scaling_inputs
    Hq, Hkv = SC[3], SC[4]
    vs = v.clone()
    vs[b, :, hk] = vs[b, :, hk] * 2.0 ** -6
    os_, _ = fp8_call(K, q, k, vs, True)
    factor = torch.ones(SC[0], 1, Hq, 1, device=DEV)
    factor[b, 0, hk * (Hq // Hkv):(hk + 1) * (Hq // Hkv)] = 64
    assert torch.equal(os_.float() * factor, o.float()), (os_.float() * factor - o.float()).abs().max().item()


# ------------------------------------------------------------------ strided operands
def test_fp8_packed_qkv_slices(K):
    """q, k, v as column slices of one (B, L, (Hq + 2 Hkv) D) buffer: the bits of the contiguous call."""
    B, L, _, Hq, Hkv, D, _ = A.PACKED_SHAPE
    q, k, v, o_ref, _ = A.random_case(*A.PACKED_SHAPE, torch.bfloat16)
    packed = torch.cat([q.reshape(B, L, -1), k.reshape(B, L, -1), v.reshape(B, L, -1)], dim=-1).to(DEV)
    qs, ks, vs = (t.view(B, L, -1, D) for t in packed.split([Hq * D, Hkv * D, Hkv * D], dim=-1))
    assert not qs.is_contiguous() and not ks.is_contiguous() and not vs.is_contiguous() and ks.data_ptr() != packed.data_ptr()
    o, lse = fp8_call(K, q, k, v, True)
    o_s, lse_s = fp8_call(K, qs, ks, vs, True)
    assert torch.equal(o_s, o) and torch.equal(lse_s, lse)
    assert_rows_close(o_s, o_ref, torch.bfloat16, "fp8 packed qkv", bound=FP8_ROW_BOUND)


def test_fp8_output_view_with_spare_columns(K):
    """The entry point itself, writing into a view with spare columns on both sides: the bits of the wrapper's call inside,
    the NaN fill untouched around it."""
    from timeviper_amd.kernels import _dt, _p, _stream
    (B, Lq, Lk, Hq, Hkv, D, _), pad = A.OUTPUT_VIEW_SHAPE, 4
    q, k, v, o_ref, _ = A.random_case(*A.OUTPUT_VIEW_SHAPE, torch.bfloat16)
    o, _ = fp8_call(K, q, k, v, False)
    q, k, v = q.to(DEV), k.to(DEV), v.to(DEV)
    buf = torch.full((B, Lq, Hq * D + 2 * pad), math.nan, dtype=torch.bfloat16, device=DEV)
    out = buf[:, :, pad:pad + Hq * D].view(B, Lq, Hq, D)
    assert out.data_ptr() == buf.data_ptr() + 2 * pad and out.stride() == (Lq * (Hq * D + 2 * pad), Hq * D + 2 * pad, D, 1)
    lib = K._capi.lib()
    ws_bytes = lib.tv_flash_attn_fp8_workspace_bytes(B, Lq, Lk, Hq, Hkv)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    K.check(lib.tv_flash_attn_fp8_fwd(
        _p(q), _p(k), _p(v), _p(out), None, B, Lq, Lk, Hq, Hkv, D, *q.stride()[:3], *k.stride()[:3], *v.stride()[:3],
        *out.stride()[:3], 1.0 / math.sqrt(D), 0, _dt(q), _p(ws), ws_bytes, _stream()), "tv_flash_attn_fp8_fwd")
    torch.cuda.synchronize()
    assert torch.equal(out, o)
    assert bool(torch.isnan(buf[:, :, :pad]).all()) and bool(torch.isnan(buf[:, :, pad + Hq * D:]).all())
    assert_rows_close(out, o_ref, torch.bfloat16, "fp8 output view", bound=FP8_ROW_BOUND)


# ------------------------------------------------------------------ random inputs: FP8_ROW_BOUND
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", A.RANDOM_SHAPES, ids=str)
def test_fp8_random_inputs_vs_oracle_on_quantised_inputs(K, shape, dtype):
    q, k, v, o_ref, lse_ref = A.random_case(*shape, dtype)
    o, lse = fp8_call(K, q, k, v, shape[6])
    assert_rows_close(o, o_ref, dtype, f"fp8 random {shape}", bound=FP8_ROW_BOUND)
    # (the row sum adds the unrounded P: what the log-sum-exp sees is the matrix pipe's accumulation of q~ . k~ only —
    # the bound test_attention_fp8_gpu.py states)
    check_lse(lse, lse_ref.double(), 2e-2, f"fp8 random {shape}")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_fp8_random_inputs_with_one_head_of_v_scaled(K, dtype):
    """The inputs on which the CPU test judges `scale_of_other_head`: V of one (batch, kv-head) is 2^-6 of the others."""
    q, k, v, o_ref, _ = A.random_case(*A.SCALED_HEAD_SHAPE, dtype, True)
    o, _ = fp8_call(K, q, k, v, A.SCALED_HEAD_SHAPE[6])
    assert_rows_close(o, o_ref, dtype, f"fp8 random, one head scaled {A.SCALED_HEAD_SHAPE}", bound=FP8_ROW_BOUND)
