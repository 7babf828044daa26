"""tv_gemv_fp8w_fwd (K.gemv_fp8w_fused: the decode step's 1..4-row products on e4m3 weights with one fp32 scale per
output row): the byte <-> k mapping in closed form on both routes (a row per wave for K < 8192, split-K from 8192 on),
what is never read, parity with an fp64 product of the dequantized matrix, the conv epilogue, and the refusals."""
import math

import pytest
import torch

from test_linear_rows_gpu import assert_product, reference

pytestmark = pytest.mark.gpu
DEV = "cuda"
KS = [16, 1008, 1024, 4480, 8192, 8208, 10240]
NS = [1, 7, 9, 37]
GROUP = {1008: 504, 1024: 256, 4480: 560, 8192: 1024, 8208: 1368, 10240: 1280}      # (16 has no group of >= 8 that leaves two)


@pytest.fixture(scope="module")
def K():
    from timeviper_amd import kernels
    return kernels


def _strided(q, ldw, fill=0):
    """q (N, K) e4m3 as a view of rows ldw bytes apart, three more rows behind it; everything else holds `fill`."""
    N, Kd = q.shape
    buf = torch.full((N + 3, ldw), fill, dtype=torch.uint8, device=q.device)
    buf[:N, :Kd] = q.view(torch.uint8)
    return buf.view(torch.float8_e4m3fn)[:N, :Kd]


def _int_case(M, N, Kd, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    q = torch.randint(-8, 9, (N, Kd), device=DEV, generator=g).float()
    x = torch.randint(-8, 9, (M, 1, Kd), device=DEV, generator=g).float()
    return x.bfloat16(), q.to(torch.float8_e4m3fn), q, x


@pytest.mark.parametrize("Kd", KS)
def test_exact_integers(K, Kd):
    """Integers in [-8, 8] on both sides, scale 2^-3: every partial sum is an integer below 2^24, so any order of the
    additions is exact and y must equal bf16(scale (x @ Q^T)) bit for bit — at every k, N, M, row stride and route."""
    calls = K.gemv_fp8w_calls()
    n = 0
    for N in NS:
        scale = torch.full((N,), 0.125, device=DEV)
        for M in (1, 2, 3, 4):
            x, w8, qf, xf = _int_case(M, N, Kd, seed=Kd + 31 * N + M)
            want = (0.125 * (xf.double().view(M, Kd) @ qf.double().t())).float().bfloat16().view(M, 1, N)
            for ldw in (Kd, Kd + 16):
                w = w8 if ldw == Kd else _strided(w8, ldw)
                assert K.gemv_fp8w_takes(x, w)
                y = K.gemv_fp8w_fused(x, w, scale)
                n += 1
                assert y.shape == (M, 1, N) and y.dtype == torch.bfloat16
                assert torch.equal(y, want), (N, M, ldw, (y.float() - want.float()).abs().max().item())
    assert K.gemv_fp8w_calls() == calls + n


@pytest.mark.parametrize("Kd", KS)
def test_position_of_every_byte(K, Kd):
    """One nonzero weight per row at k = n: y[m][n] = x[m][n] Q[n][n] scale[n] — a byte read at another k shows."""
    g = torch.Generator(device=DEV).manual_seed(Kd)
    for M in (1, 3):
        x = torch.randint(1, 9, (M, 1, Kd), device=DEV, generator=g).float()
        d = torch.randint(1, 9, (Kd,), device=DEV, generator=g).float()
        w8 = torch.diag(d).to(torch.float8_e4m3fn)
        scale = torch.full((Kd,), 0.5, device=DEV)
        y = K.gemv_fp8w_fused(x.bfloat16(), w8, scale)
        assert torch.equal(y.float(), x * d * 0.5)


@pytest.mark.parametrize("Kd", KS)
def test_reads_nothing_past_k_or_n(K, Kd):
    """Rows >= N and the bytes between K and ldw hold 0x7F (NaN in e4m3): finite outputs, equal to the dense case."""
    for N, M in ((7, 1), (37, 4), (9, 3)):
        x, w8, _, _ = _int_case(M, N, Kd, seed=Kd + N)
        scale = torch.full((N,), 0.125, device=DEV)
        dense = K.gemv_fp8w_fused(x, w8, scale)
        padded = K.gemv_fp8w_fused(x, _strided(w8, Kd + 16, fill=0x7F), scale)
        assert torch.isfinite(padded.float()).all()
        assert torch.equal(padded, dense)


def _parity_operands(K, M, N, Kd, seed, bias, nw_f32):
    """test_linear_rows_gpu.py's operands (x, delta, gate ~ N(0, 1) / N(0, 0.25), W ~ N(0, 1 / K), bias ~ N(0, 1), norm
    weights 1 + 0.1 N(0, 1)), W rounded to e4m3 against random power-of-two row scales in [2^-12, 2^-4] (saturating at
    448 where the scale is small for the row, down in the subnormals where it is large: every code is met)."""
    g = torch.Generator(device=DEV).manual_seed(M * 7 + N + Kd + seed)
    x = torch.randn(M, 1, Kd, device=DEV, generator=g).bfloat16()
    d = (torch.randn(M, 1, Kd, device=DEV, generator=g) * 0.5).bfloat16()
    z = torch.randn(M, 1, Kd, device=DEV, generator=g).bfloat16()
    W = (torch.randn(N, Kd, device=DEV, generator=g) / math.sqrt(Kd)).bfloat16()
    scale = torch.exp2(torch.randint(-12, -3, (N,), device=DEV, generator=g).float())
    w8 = (W.float() / scale[:, None]).clamp_(-448, 448).to(torch.float8_e4m3fn)
    b = torch.randn(N, device=DEV, generator=g).bfloat16() if bias else None
    nw = 1 + 0.1 * torch.randn(Kd, device=DEV, generator=g)
    return x, d, z, w8, scale, b, (nw.float() if nw_f32 else nw.bfloat16())


PARITY = [(Kd, pro) for Kd in KS for pro in ("none", "rmsnorm", "rmsnorm+delta", "relu2", "gated", "gated-nogate")
          if not (pro.startswith("gated") and Kd == 16) and not (pro.startswith("rmsnorm") and Kd > 8192)]


@pytest.mark.parametrize("Kd,prologue", PARITY)
def test_parity_with_the_dequantized_matrix(K, Kd, prologue):
    """assert_product's criterion (2^-8 |ref| + 2e-3 against fp64) with W = diag(scale) Q — exact in bf16 — and f(x) from
    the stand-alone operators; bias on and off, bf16 and fp32 norm weights."""
    i = 0
    for N in NS:
        for M in (1, 2, 3, 4):
            i += 1
            bias, nw_f32 = bool(i & 1), bool(i & 2)
            x, d, z, w8, scale, b, nw = _parity_operands(K, M, N, Kd, 0, bias, nw_f32)
            f, kw, s_ref = reference(K, prologue, x, d, z, nw, GROUP.get(Kd, 8))
            if s_ref is not None:
                kw["sum_out"] = torch.full_like(x, float("nan"))
            W = K.dequantize_rows_e4m3(w8, scale)
            assert torch.equal(W.float(), w8.float() * scale[:, None])           # exact in bf16
            y = K.gemv_fp8w_fused(x, w8, scale, b, **kw)
            assert y.shape == (M, 1, N) and y.dtype == torch.bfloat16
            assert_product(y, f, W, b, M, N, Kd)
            if s_ref is not None:
                assert torch.equal(kw["sum_out"], s_ref)
            assert torch.equal(K.gemv_fp8w_fused(x, w8, scale, b, **kw), y)      # deterministic


@pytest.mark.parametrize("M", [1, 3])
def test_conv_epilogue(K, M):
    """The conv epilogue against the same product without it followed by K.causal_conv1d_update: bit-equal, state
    included, over several tokens."""
    g = torch.Generator(device=DEV).manual_seed(M)
    Kd, d_in, C, H = 512, 320, 448, 24
    N = d_in + C + H
    w8, scale = K.quantize_rows_e4m3((torch.randn(N, Kd, device=DEV, generator=g) / math.sqrt(Kd)).bfloat16())
    nw = torch.ones(Kd, device=DEV)
    cw = (torch.randn(C, 4, device=DEV, generator=g) * 0.5).bfloat16()
    cb = torch.randn(C, device=DEV, generator=g).bfloat16()
    st_a = torch.randn(M, C, 4, device=DEV, generator=g).bfloat16()
    st_b = st_a.clone()
    for step in range(4):
        x = torch.randn(M, 1, Kd, device=DEV, generator=g).bfloat16()
        two = K.gemv_fp8w_fused(x, w8, scale, None, K.GEMV_RMSNORM, norm_weight=nw, eps=1e-5)
        conv_two = K.causal_conv1d_update(two[:, 0, d_in:d_in + C], st_a, cw, cb, "silu")
        one = K.gemv_fp8w_fused(x, w8, scale, None, K.GEMV_RMSNORM, norm_weight=nw, eps=1e-5, conv=(st_b, cw, cb, d_in))
        assert torch.equal(one[:, 0, d_in:d_in + C], conv_two), step
        assert torch.equal(one[..., :d_in], two[..., :d_in]) and torch.equal(one[..., d_in + C:], two[..., d_in + C:])
        assert torch.equal(st_a, st_b), step


def test_refusals(K):
    g = torch.Generator(device=DEV).manual_seed(0)
    x = torch.randn(1, 1, 512, device=DEV, generator=g).bfloat16()
    w8, scale = K.quantize_rows_e4m3((torch.randn(40, 512, device=DEV, generator=g) / 20).bfloat16())
    K.gemv_fp8w_fused(x, w8, scale)
    calls = K.gemv_fp8w_calls()
    E = K.TimeViperHipError
    with pytest.raises(E):                         # K % 16 != 0
        K.gemv_fp8w_fused(x[..., :504], w8[:, :504], scale)
    assert not K.gemv_fp8w_takes(x[..., :504], w8[:, :504])
    raw = torch.zeros(40 * 512 + 16, dtype=torch.uint8, device=DEV)
    off = raw[8:8 + 40 * 512].view(torch.float8_e4m3fn).view(40, 512)      # W 8 bytes off a 16-byte boundary
    assert off.data_ptr() % 16 == 8 and not K.gemv_fp8w_takes(x, off)
    with pytest.raises(E):
        K.gemv_fp8w_fused(x, off, scale)
    with pytest.raises(E):                         # a bf16 tensor as w8
        K.gemv_fp8w_fused(x, K.dequantize_rows_e4m3(w8, scale), scale)
    with pytest.raises(E):                         # and the bf16 wrapper keeps refusing e4m3
        K.gemv_fused(x, w8)
    assert not K.gemv_takes(x, w8)
    with pytest.raises(E):                         # an fp16 scale
        K.gemv_fp8w_fused(x, w8, scale.half())
    with pytest.raises(E):                         # too few scales
        K.gemv_fp8w_fused(x, w8, scale[:39])
    x5 = torch.randn(5, 1, 512, device=DEV, generator=g).bfloat16()
    assert not K.gemv_fp8w_takes(x5, w8)
    with pytest.raises(E):                         # M = 5
        K.gemv_fp8w_fused(x5, w8, scale)
    with pytest.raises(E):                         # the conv epilogue lives in the row-per-wave kernel
        big, bs = torch.zeros(16, 8192, device=DEV).to(torch.float8_e4m3fn), torch.ones(16, device=DEV)
        st = torch.zeros(1, 8, 4, device=DEV).bfloat16()
        K.gemv_fp8w_fused(torch.zeros(1, 1, 8192, device=DEV).bfloat16(), big, bs,
                          conv=(st, torch.zeros(8, 4, device=DEV).bfloat16(), None, 0))
    assert K.gemv_fp8w_calls() == calls            # none of them launched
