"""tv_linear_rows_bf16_fwd (K.linear_rows_fused: the linear layers of a 2..16-token forward) against the stand-alone
operators + an fp64 product of THEIR bf16 output, in the manner of test_ops_gpu.py::test_gemv_fused_prologues: the
prologue rounds where tv_rmsnorm_fwd / tv_relu2_fwd / tv_rmsnorm_gated_fwd round, so f(x) is compared bit for bit (through
sum_out and a product with the identity) and y to the accumulation order."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
PROLOGUES = ["none", "rmsnorm", "rmsnorm+delta", "relu2", "gated", "gated-nogate"]
GROUP = {8: 8, 136: 8, 4480: 560, 10240: 1280, 15680: 1960}


@pytest.fixture(scope="module")
def K():
    from timeviper_amd import kernels
    return kernels


_eyes = {}


def eye(Kd):
    if Kd not in _eyes:
        _eyes[Kd] = torch.eye(Kd, device=DEV).bfloat16()
    return _eyes[Kd]


def operands(M, N, Kd, seed=0, bias=None, nw_f32=None):
    g = torch.Generator(device=DEV).manual_seed(M * 7 + N + Kd + seed)
    x = torch.randn(1, M, Kd, device=DEV, generator=g).bfloat16()
    d = (torch.randn(1, M, Kd, device=DEV, generator=g) * 0.5).bfloat16()
    z = torch.randn(1, M, Kd, device=DEV, generator=g).bfloat16()
    W = (torch.randn(N, Kd, device=DEV, generator=g) / math.sqrt(Kd)).bfloat16()
    b = torch.randn(N, device=DEV, generator=g).bfloat16()
    if not (N % 2 if bias is None else bias):
        b = None
    nw = (1 + 0.1 * torch.randn(Kd, device=DEV, generator=g))
    nw = nw.float() if (M % 2 == 0 if nw_f32 is None else nw_f32) else nw.bfloat16()
    return x, d, z, W, b, nw


def reference(K, prologue, x, d, z, nw, group):
    """(f(x) by the stand-alone operators, keyword arguments of linear_rows_fused, expected sum or None)"""
    if prologue == "none":
        return x, dict(prologue=K.GEMV_NONE), None
    if prologue == "rmsnorm":
        return K.rms_norm(x, nw, 1e-5), dict(prologue=K.GEMV_RMSNORM, norm_weight=nw, eps=1e-5), None
    if prologue == "rmsnorm+delta":
        f, s_ref = K.rms_norm(x, nw, 1e-5, residual=d, return_sum=True)
        return f, dict(prologue=K.GEMV_RMSNORM, norm_weight=nw, eps=1e-5, delta=d), s_ref
    if prologue == "relu2":
        return K.relu2(x), dict(prologue=K.GEMV_RELU2), None
    gate = z if prologue == "gated" else None
    f = K.rmsnorm_fn(x, nw, None, z=gate, eps=1e-5, group_size=group, norm_before_gate=False)
    return f, dict(prologue=K.GEMV_GATED, norm_weight=nw, eps=1e-5, gate=gate, group_size=group), None


def assert_product(y, f, W, b, M, N, Kd):
    ref = f.double().reshape(M, Kd) @ W.double().t() + (0 if b is None else b.double())
    err = (y.double().reshape(M, N) - ref).abs()
    tol = 2.0 ** -8 * ref.abs() + 2e-3            # one bf16 rounding of y + fp32 accumulation over K
    excess = (err / tol).max().item()
    print(f"max err / tol {excess:.3f}")
    assert (err <= tol).all(), f"max excess {excess:.2f}"


def check(K, M, N, Kd, prologue, identity, **opts):
    x, d, z, W, b, nw = operands(M, N, Kd, **opts)
    f, kw, s_ref = reference(K, prologue, x, d, z, nw, GROUP[Kd])
    sum_out = None
    if s_ref is not None:
        sum_out = torch.full_like(x, float("nan"))
        kw["sum_out"] = sum_out
    assert K.linear_rows_takes(x, W)
    y = K.linear_rows_fused(x, W, b, **kw)
    assert y.shape == (1, M, N) and y.dtype == torch.bfloat16
    assert_product(y, f, W, b, M, N, Kd)
    if sum_out is not None:
        assert torch.equal(sum_out, s_ref)         # every one of the M rows
    assert torch.equal(K.linear_rows_fused(x, W, b, **kw), y)          # deterministic
    if identity:                                   # f(x) itself, bit for bit: rows of the identity pick its elements
        kw.pop("sum_out", None)
        assert torch.equal(K.linear_rows_fused(x, eye(Kd), None, **kw).view(M, Kd), f.view(M, Kd))


@pytest.mark.parametrize("prologue", PROLOGUES)
@pytest.mark.parametrize("Kd", [8, 136, 4480])
@pytest.mark.parametrize("N", [1, 17, 48, 777])
@pytest.mark.parametrize("M", [1, 2, 5, 9, 16])
def test_linear_rows_prologues(K, M, N, Kd, prologue):
    check(K, M, N, Kd, prologue, identity=True)


@pytest.mark.parametrize("M,Kd,prologue", [
    (16, 10240, "gated"), (16, 10240, "gated-nogate"), (16, 15680, "relu2"), (16, 15680, "none"), (9, 10240, "gated"),
    (2, 10240, "gated"), (2, 10240, "gated-nogate"), (2, 15680, "relu2"), (2, 15680, "none"),
])
def test_linear_rows_slices(K, M, Kd, prologue):
    """K beyond what f(x) of M rows takes in LDS: several slices (gated: of whole norm groups), the accumulators kept
    across them; K = 15 680 ends in half a step.  M = 2: the same code with everything in one or two slices."""
    check(K, M, 48, Kd, prologue, identity=False)


@pytest.mark.parametrize("M,N,Kd", [(5, 12000, 136), (3, 16448, 136), (16, 32960, 8)])
def test_linear_rows_several_tiles_per_work_group(K, M, N, Kd):
    """750, 1 028 and 2 060 tiles: 2, 3 and 5 a work-group on 256 compute units — the kernel shapes with 2, 4 and 16
    accumulator tiles (the gated prologue keeps 2 and takes more work-groups)."""
    for prologue in ("none", "rmsnorm+delta", "gated"):
        check(K, M, N, Kd, prologue, identity=False)


@pytest.mark.parametrize("nw_f32", [True, False])
@pytest.mark.parametrize("bias", [True, False])
def test_linear_rows_norm_weight_dtypes_and_bias(K, nw_f32, bias):
    for prologue in ("rmsnorm+delta", "gated"):
        check(K, 5, 48, 136, prologue, identity=True, bias=bias, nw_f32=nw_f32)


def test_linear_rows_strides(K):
    """ldw > K, x_stride > K, delta / gate as column views, y into a column window of a wider buffer."""
    M, N, Kd = 5, 40, 136
    g = torch.Generator(device=DEV).manual_seed(3)
    wide = torch.randn(1, M, 3 * Kd, device=DEV, generator=g).bfloat16()
    x, d, z = wide[..., Kd:2 * Kd], wide[..., :Kd], wide[..., 2 * Kd:]
    Wwide = (torch.randn(N + 8, 2 * Kd, device=DEV, generator=g) / math.sqrt(Kd)).bfloat16()
    W = Wwide[3:3 + N, Kd:]                       # a row and column slice: ldw = 2 K
    nw = (1 + 0.1 * torch.randn(Kd, device=DEV, generator=g))
    assert K.linear_rows_takes(x, W)
    for prologue in PROLOGUES:
        f, kw, s_ref = reference(K, prologue, x.contiguous(), d.contiguous(), z.contiguous(), nw, 136)
        for key, view in (("delta", d), ("gate", z)):
            if kw.get(key) is not None:
                kw[key] = view
        if s_ref is not None:
            sbuf = torch.full((1, M, 2 * Kd), 7.0, device=DEV).bfloat16()
            kw["sum_out"] = sbuf[..., 8:8 + Kd]
        ybuf = torch.full((1, M, N + 24), 5.0, device=DEV).bfloat16()
        y = K.linear_rows_fused(x, W, None, out=ybuf[..., 8:8 + N], **kw)
        assert y.data_ptr() == ybuf[..., 8:].data_ptr()
        assert_product(y, f, W, None, M, N, Kd)
        assert (ybuf[..., :8] == 5).all() and (ybuf[..., 8 + N:] == 5).all()
        if s_ref is not None:
            assert torch.equal(sbuf[..., 8:8 + Kd], s_ref)
            assert (sbuf[..., :8] == 7).all() and (sbuf[..., 8 + Kd:] == 7).all()


@pytest.mark.parametrize("M", [1, 5, 9])
def test_linear_rows_reads_no_row_past_m(K, M):
    """Token columns M..15 of the matrix operand are not read: rows behind the M given ones hold NaN."""
    N, Kd = 48, 136
    x, d, z, W, b, nw = operands(M, N, Kd)
    pad = lambda t: torch.cat([t, torch.full((1, 16 - M, Kd), float("nan"), device=DEV).bfloat16()], dim=1)[:, :M]
    xp, dp, zp = pad(x), pad(d), pad(z)
    for prologue in PROLOGUES:
        f, kw, _ = reference(K, prologue, x, d, z, nw, GROUP[Kd])
        for key, view in (("delta", dp), ("gate", zp)):
            if kw.get(key) is not None:
                kw[key] = view
        y = K.linear_rows_fused(xp, W, b, **kw)
        assert torch.isfinite(y).all()
        assert_product(y, f, W, b, M, N, Kd)


def test_linear_rows_errors(K):
    x, d, z, W, b, nw = operands(4, 48, 136)
    assert not K.linear_rows_takes(torch.zeros(1, 17, 136, device=DEV).bfloat16(), W)
    assert not K.linear_rows_takes(x.float(), W)
    assert not K.linear_rows_takes(torch.zeros(2, 4, 136, device=DEV).bfloat16(), W)
    with pytest.raises(K.TimeViperHipError):
        K.linear_rows_fused(torch.zeros(1, 17, 136, device=DEV).bfloat16(), W)
    wide = torch.zeros(1, 4, 137, device=DEV).bfloat16()
    with pytest.raises(K.TimeViperHipError):
        K.linear_rows_fused(wide[..., 1:], W)                                           # misaligned x
    with pytest.raises(K.TimeViperHipError):
        K.linear_rows_fused(x, W, None, K.GEMV_RMSNORM)                                 # no norm weight
    with pytest.raises(K.TimeViperHipError):
        K.linear_rows_fused(x, W, None, K.GEMV_GATED, norm_weight=nw, group_size=24)    # 24 does not divide 136
