"""Every dispatch branch of csrc/norms.hip against fp64 arithmetic on the same rounded inputs.

Cases, inputs, references and the criterion come from tests/norm_accuracy.py; tests/test_norm_accuracy_cpu.py has judged
the same rows on the CPU and shown that the criterion rejects the faults it is there for.  References are computed in
fp64 with plain torch on the device.  Where the contract is exact (`sum_out`, relu2) the comparison is `torch.equal`."""
import pytest
import torch

import norm_accuracy as NA
from norm_accuracy import BF16, F16, F32, LN_EPS, RMS_EPS, assert_norm_close, tile_rows

pytestmark = pytest.mark.gpu
DEV = "cuda"

LN_RUN = {c.name: c for c in NA.LN_CASES}
RMS_RUN = {c.name: c for c in NA.RMS_CASES}
GATED_RUN = {c.name: c for c in NA.GATED_CASES}
ACT_SIZES, ACT_INPUTS = NA.act_sizes, NA.act_inputs


@pytest.fixture(scope="module")
def K():
    from timeviper_amd import kernels
    return kernels


def _dev(d, rows=None):
    return {k: (None if v is None else (tile_rows(v.to(DEV), rows) if rows and v.dim() == 2 else v.to(DEV)))
            for k, v in d.items()}


def _layer_norm(K, case, i):
    """runs the case; judges y, and sum_out bit for bit where there is a residual"""
    if case.residual:
        y, s = K.layer_norm(i["x"], i["w"], i["b"], LN_EPS, residual=i["delta"], return_sum=True, row_bias=i["rb"])
        assert torch.equal(s, NA.rounded_sum(i["x"], i["delta"])), f"{case.name}: sum_out is not x + delta (row bias excluded)"
    else:
        y = K.layer_norm(i["x"], i["w"], i["b"], LN_EPS, row_bias=i["rb"])
    ref, scale = NA.layernorm_ref64(i["x"], i["w"], i["b"], LN_EPS, i["delta"], i["rb"])
    assert_norm_close(y, ref, scale, case.dtype, case.name, "layernorm")


@pytest.mark.parametrize("name", [c.name for c in NA.LN_MANY])
def test_layernorm_many_rows_kernel(K, name):
    """layernorm_rows_kernel<T, NV, 8, false>: rows = 32 773 >= 32 768, no residual, D / V <= 256 vectors.
    32 773 = 4 096 * 8 + 5: wave 4 096 holds 5 rows (nrow < RPW, the prefetch stops early), and of the 1 025 * 4 = 4 100
    waves launched the last three exit.  NV = ceil(D / V / 64) with V = 8 (16 bits) / 4 (fp32):
    D = 8 / 4: 1 vector, NV 1, one lane;  520 / 260: 65 vectors, NV 2, one lane in the second;  1 152 / 576: 144 vectors,
    NV 3, 16 lanes in the third;  2 048 / 1 024: 256 vectors, NV 4, every lane.  With and without bias and row bias."""
    case = LN_RUN[name]
    _layer_norm(K, case, _dev(NA.ln_inputs(case), case.rows))


@pytest.mark.parametrize("name", [c.name for c in NA.LN_EDGE])
def test_layernorm_dispatch_edges(K, name):
    """The neighbours of `D / V <= 256 && rows >= 32 768 && !delta`, bf16 at D = 1 152 (144 vectors) unless said:
    32 768 rows: rows kernel, every wave full;  32 767: wave kernel;  32 768 with a residual: wave kernel;
    32 768 at D = 2 056 (257 vectors > 256): block kernel;  fp32 at D = 1 152 (288 vectors > 256): block kernel."""
    case = LN_RUN[name]
    _layer_norm(K, case, _dev(NA.ln_inputs(case), case.rows))


@pytest.mark.parametrize("name", [c.name for c in NA.LN_SMALL])
def test_layernorm_residual_and_sum_out(K, name):
    """Wave kernel (D / V <= 256: D = 8, 1 152 in 16 bits; 4, 576 in fp32) and block kernel (2 056, 8 192; 1 028, 4 096)
    with `residual=` and `return_sum=True`, 7 rows without and 13 rows with a row bias (neither a multiple of the 4
    rows of a wave-kernel block): y by the criterion, sum_out == round(x + delta) bit for bit, the row bias not in it."""
    case = LN_RUN[name]
    _layer_norm(K, case, _dev(NA.ln_inputs(case), case.rows))


@pytest.mark.parametrize("name", ["bf16-r13-D1152-b-rb-res-wave", "fp32-r13-D1028-b-rb-res-block"])
def test_layernorm_column_windows(K, name):
    """x and residual as column windows [16, 16 + D) of buffers 48 columns wider: the row strides reach the kernel."""
    case = LN_RUN[name]
    i = _dev(NA.ln_inputs(case), case.rows)
    for k in ("x", "delta"):
        wide = torch.full((case.rows, case.D + 48), float("nan"), dtype=case.dtype, device=DEV)
        wide[:, 16:16 + case.D] = i[k]
        i[k] = wide[:, 16:16 + case.D]
        assert not i[k].is_contiguous()
    _layer_norm(K, case, i)


@pytest.mark.parametrize("name", ["bf16-r32773-D1152-b-rb-rows", "fp32-r32773-D260-nob-rb-rows",
                                  "bf16-r32767-D1152-b-rb-wave"])
def test_layernorm_strided_output_leaves_the_padding_alone(K, name):
    """tv_layernorm_fwd called as kernels.py calls it, with y_stride = D + 24 into a buffer of NaN: all rows x D outputs
    are written (finite, judged) and every padding element is still NaN — many-row kernel (NV 3, NV 2) and wave kernel."""
    from timeviper_amd import _capi
    case = LN_RUN[name]
    i = _dev(NA.ln_inputs(case), case.rows)
    x, ys = i["x"], case.D + 24
    ybuf = torch.full((case.rows, ys), float("nan"), dtype=case.dtype, device=DEV)
    _capi.check(_capi.lib().tv_layernorm_fwd(
        x.data_ptr(), None, i["w"].data_ptr(), None if i["b"] is None else i["b"].data_ptr(), i["rb"].data_ptr(), None,
        ybuf.data_ptr(), case.rows, case.D, x.stride(0), 0, 0, ys, LN_EPS, K._dt(x), K._stream()), "tv_layernorm_fwd")
    y = ybuf[:, :case.D].contiguous()
    assert bool(torch.isfinite(y).all())
    assert bool(torch.isnan(ybuf[:, case.D:]).all()), "the kernel wrote into the padding of y"
    ref, scale = NA.layernorm_ref64(x, i["w"], i["b"], LN_EPS, None, i["rb"])
    assert_norm_close(y, ref, scale, case.dtype, name + " strided y", "layernorm")


def test_layernorm_errors_are_raised(K):
    w = torch.ones(8200, dtype=BF16, device=DEV)
    from timeviper_amd import _capi
    x = torch.zeros(3, 16, dtype=BF16, device=DEV)
    with pytest.raises(K.TimeViperHipError):                         # 12 is no multiple of the 8 channels of a vector
        K.layer_norm(x[:, :12], w[:12], None, LN_EPS)                # (refused as a row stride of 12 already)
    y = torch.empty_like(x)
    with pytest.raises(K.TimeViperHipError, match="multiple"):       # and with row strides of 16, as the width itself
        _capi.check(_capi.lib().tv_layernorm_fwd(x.data_ptr(), None, w.data_ptr(), None, None, None, y.data_ptr(), 3, 12,
                                                 16, 0, 0, 16, LN_EPS, _capi.TV_BF16, K._stream()), "tv_layernorm_fwd")
    with pytest.raises(K.TimeViperHipError, match="larger"):         # 8 200 = 1 025 vectors > 1 024
        K.layer_norm(torch.zeros(3, 8200, dtype=BF16, device=DEV), w, None, LN_EPS)
    flat = torch.zeros(3 * 64 + 8, dtype=BF16, device=DEV)
    with pytest.raises(K.TimeViperHipError, match="aligned"):        # 2 bytes off a 16-byte boundary
        K.layer_norm(flat[1:1 + 3 * 64].view(3, 64), w[:64], None, LN_EPS)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------ RMSNorm, gated RMSNorm
@pytest.mark.parametrize("name", list(RMS_RUN))
def test_rmsnorm(K, name):
    """rmsnorm_kernel (a block per row, up to 4 vectors per lane): D = 8 one lane; 1 152 / 4 480 partly filled first and
    third pass; 8 192 (4 096 in fp32) every lane four times.  fp32 weights (`wf32`, two 16-byte loads per vector) and
    weights in the activation type; with `residual`, the returned sum is round(x + delta) bit for bit."""
    case = RMS_RUN[name]
    i = _dev(NA.rms_inputs(case))
    assert i["w"].dtype == case.wdtype
    if case.residual:
        y, s = K.rms_norm(i["x"], i["w"], RMS_EPS, residual=i["delta"], return_sum=True)
        assert torch.equal(s, NA.rounded_sum(i["x"], i["delta"]))
    else:
        y = K.rms_norm(i["x"], i["w"], RMS_EPS)
    ref, scale = NA.rmsnorm_ref64(i["x"], i["w"], RMS_EPS, i["delta"])
    assert_norm_close(y, ref, scale, case.dtype, name, "rmsnorm")


@pytest.mark.parametrize("name", list(GATED_RUN))
def test_rmsnorm_gated(K, name):
    """rmsnorm_gated_kernel, a wave per (row, group): groups of 8 (one lane), 1 280 (160 vectors: 2.5 per lane) and
    2 048 (256: the limit) in 16 bits, 4 and 1 024 in fp32; rows * groups = 21, 15, 6: the last block is not full.
    x and z are column windows of one wider buffer, as the mixer passes them; with and without z."""
    case = GATED_RUN[name]
    i = _dev(NA.gated_inputs(case))
    x = i["buf"][:, 16:16 + case.D]
    z = i["buf"][:, 16 + case.D:16 + 2 * case.D] if case.gate else None
    assert not x.is_contiguous() and (case.rows * (case.D // case.gs)) % 4
    y = K.rmsnorm_fn(x, i["w"], None, z=z, eps=RMS_EPS, group_size=case.gs, norm_before_gate=False)
    ref, scale = NA.gated_ref64(x, z, i["w"], RMS_EPS, case.gs)
    assert_norm_close(y, ref, scale, case.dtype, name, "gated")


def test_rmsnorm_gated_errors_are_raised(K):
    from timeviper_amd import _capi
    x = torch.zeros(3, 4096, dtype=F16, device=DEV)
    w = torch.ones(4096, dtype=F32, device=DEV)
    with pytest.raises(K.TimeViperHipError, match="larger"):         # 2 056 = 257 vectors > 4 x 64
        K.rmsnorm_fn(x[:, :2056], w[:2056], None, z=None, eps=RMS_EPS, group_size=2056, norm_before_gate=False)
    with pytest.raises(K.TimeViperHipError, match="bad sizes"):      # 1 280 does not divide 2 048
        K.rmsnorm_fn(x[:, :2048], w[:2048], None, z=None, eps=RMS_EPS, group_size=1280, norm_before_gate=False)
    wb = torch.ones(2048, dtype=BF16, device=DEV)                    # the C entry point takes fp32 or the activation type
    y = torch.empty(3, 2048, dtype=F16, device=DEV)
    with pytest.raises(K.TimeViperHipError, match="wdtype"):
        _capi.check(_capi.lib().tv_rmsnorm_gated_fwd(
            x.data_ptr(), None, wb.data_ptr(), y.data_ptr(), 3, 2048, 1024, x.stride(0), 0, y.stride(0), RMS_EPS,
            _capi.TV_F16, _capi.TV_BF16, K._stream()), "tv_rmsnorm_gated_fwd")
    # kernels.py upcasts such a weight to fp32 instead: the same numbers as with the fp32 weight
    a = K.rmsnorm_fn(x[:, :2048] + 1, wb, None, z=None, eps=RMS_EPS, group_size=1024, norm_before_gate=False)
    b = K.rmsnorm_fn(x[:, :2048] + 1, wb.float(), None, z=None, eps=RMS_EPS, group_size=1024, norm_before_gate=False)
    assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------- activations
@pytest.mark.parametrize("size", ["main", "below", "above"])
@pytest.mark.parametrize("dtype", [F32, BF16, F16], ids=["fp32", "bf16", "fp16"])
def test_activations_both_loops(K, dtype, size):
    """gelu_kernel, grid capped at 8 192 x 256 lanes = 2 097 152 vectors a stride; the 4-wide loop runs while
    i + 3 * 2 097 152 < nvec.  main: nvec = 5 * 2 097 152 + 300 (and 3 ragged elements): every lane makes one 4-wide pass,
    lanes below 2 097 152 + 300 one one-vector pass, block 0 the tail.  below / above: nvec = 4 * 2 097 152 -+ 1: the last
    lane stays out of / enters the 4-wide loop.  relu2 bit for bit, gelu against the fp64 erf form; main also in place."""
    n = ACT_SIZES(dtype)[size]
    x = ACT_INPUTS(n, dtype, DEV, 7)
    assert int((x == 0).sum()) > 0 and bool((x.abs() > 6).any()) and bool(torch.signbit(x[1]))
    want = torch.square(torch.relu(x))
    assert torch.equal(K.relu2(x), want), "relu2 differs from square(relu(x))"
    ref, scale = NA.gelu_ref64(x)
    assert_norm_close(K.gelu(x), ref, scale, dtype, f"gelu {size}", "gelu")
    if size == "main":
        xi = x.clone()
        assert K.relu2(xi, inplace=True).data_ptr() == xi.data_ptr() and torch.equal(xi, want)
        xi = x.clone()
        K.gelu(xi, inplace=True)
        assert_norm_close(xi, ref, scale, dtype, "gelu main in place", "gelu")


def test_activation_misaligned_view_raises(K):
    x = torch.zeros(4097, dtype=BF16, device=DEV)
    for f in (K.gelu, K.relu2):
        with pytest.raises(K.TimeViperHipError, match="aligned"):
            f(x[1:])
    torch.cuda.synchronize()
