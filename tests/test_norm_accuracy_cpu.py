"""The criterion of tests/norm_accuracy.py separates the arithmetic of csrc/norms.hip from subtly wrong variants of
it — on the CPU, on the inputs tests/test_norms_dispatch_gpu.py runs the kernels on.

The fp32 restatement of every kernel passes `assert_norm_close` on every case; the constant c of the criterion is at
least four times what the restatement needs; each mutation of the restatement fails on every case it changes the
arithmetic of (the predicate beside each mutation says which those are, and why the others cannot show it)."""
import importlib

import pytest
import torch

import norm_accuracy as NA
from norm_accuracy import BF16, F16, F32, C, LN_EPS, RMS_EPS

DTYPES = [F32, BF16, F16]
IDS = [NA.DTYPE_ID[d] for d in DTYPES]


# ------------------------------------------------------------------------------- one (output, ref, scale) per case
def ln_eval(case, mutation=None):
    i = NA.ln_inputs(case)
    y = NA.layernorm_fp32(i["x"], i["w"], i["b"], LN_EPS, i["delta"], i["rb"], mutation,
                          NA.ln_padded(case.D, case.dtype, case.kernel))
    return (y, *NA.layernorm_ref64(i["x"], i["w"], i["b"], LN_EPS, i["delta"], i["rb"]))


def rms_padded(case):
    lanes = 256 * NA.vec(case.dtype)
    return -(-case.D // lanes) * lanes


def rms_eval(case, mutation=None):
    i = NA.rms_inputs(case)
    y = NA.rmsnorm_fp32(i["x"], i["w"], RMS_EPS, i["delta"], mutation, rms_padded(case))
    return (y, *NA.rmsnorm_ref64(i["x"], i["w"], RMS_EPS, i["delta"]))


def gated_padded(case):
    lanes = 64 * NA.vec(case.dtype)
    return -(-case.gs // lanes) * lanes


def gated_eval(case, mutation=None):
    i = NA.gated_inputs(case)
    y = NA.gated_fp32(i["x"], i["z"], i["w"], RMS_EPS, case.gs, mutation, gated_padded(case))
    return (y, *NA.gated_ref64(i["x"], i["z"], i["w"], RMS_EPS, case.gs))


def gelu_eval(dtype, mutation=None):
    x = NA.act_cpu_values(dtype)
    y = torch.nn.functional.gelu(x.float(), approximate="tanh").to(dtype) if mutation == "tanh" else NA.gelu_fp32(x)
    return (y, *NA.gelu_ref64(x))


OPS = {"layernorm": (NA.LN_CASES, ln_eval), "rmsnorm": (NA.RMS_CASES, rms_eval), "gated": (NA.GATED_CASES, gated_eval)}


def evaluations(op, dtype):
    if op == "gelu":
        return [(f"gelu-{NA.DTYPE_ID[dtype]}", gelu_eval(dtype))]
    cases, ev = OPS[op]
    return [(c.name, ev(c)) for c in cases if c.dtype == dtype]


# ------------------------------------------------------------------------------------------------ the criterion
def test_criterion_names_the_worst_element_and_rejects_nan():
    ref = torch.linspace(0.5, 2.0, 24, dtype=torch.float64).reshape(3, 8)
    scale = ref.abs()
    y = ref.to(BF16)
    NA.assert_norm_close(y, ref, scale, BF16, "rounded once", "rmsnorm")
    bad = y.clone()
    bad[1, 5] = bad[1, 5] * (1 + 2.0 ** -6)                       # two ulps off
    bad[2, 2] = bad[2, 2] * (1 + 2.0 ** -7)                       # one ulp off: the smaller excess
    with pytest.raises(AssertionError, match=r"row 1, column 5.*2 of 24 elements over"):
        NA.assert_norm_close(bad, ref, scale, BF16, "two wrong", "rmsnorm")
    bad = y.clone()
    bad[0, 7] = float("nan")
    with pytest.raises(AssertionError, match=r"row 0, column 7"):
        NA.assert_norm_close(bad, ref, scale, BF16, "nan", "rmsnorm")
    # fp32: only the c term; 18 units of 2^-24 scale are over rmsnorm's c = 16, 14 are not
    r32 = torch.ones(1, 4, dtype=torch.float64)
    NA.assert_norm_close((r32 * (1 + 14 * NA.U)).float(), r32, r32, F32, "14 units", "rmsnorm")
    with pytest.raises(AssertionError, match="row 0, column 0"):
        NA.assert_norm_close((r32 * (1 + 18 * NA.U)).float(), r32, r32, F32, "18 units", "rmsnorm")
    # an fp16 subnormal is judged by the format's spacing there, a zero reference with zero scale exactly
    sub = torch.full((1, 4), 3.3e-6, dtype=torch.float64)
    NA.assert_norm_close(sub.to(F16), sub, sub, F16, "fp16 subnormal", "gated")
    zero = torch.zeros(1, 4, dtype=torch.float64)
    NA.assert_norm_close(torch.tensor([[0.0, -0.0, 0.0, 0.0]]), zero, zero, F32, "exact zero", "layernorm")
    with pytest.raises(AssertionError):
        NA.assert_norm_close(torch.tensor([[0.0, 1e-30, 0.0, 0.0]]), zero, zero, F32, "not zero", "layernorm")
    assert C.keys() == {"layernorm", "rmsnorm", "gated", "gelu"} and all(c >= 16 for c in C.values())


def test_layernorm_cases_reach_every_branch_of_the_dispatch():
    """The `kernel` each case names is what launch_ln's arithmetic gives, and between them the cases reach the many-row
    kernel at NV = 1, 2, 3, 4 with a partly filled last vector (and the full one at NV = 4), the wave and the block
    kernel, in all three dtypes."""
    for c in NA.LN_CASES:
        assert c.D % NA.vec(c.dtype) == 0 and c.kernel == NA.ln_kernel(c.rows, c.D, c.dtype, c.residual), c
    for dt in DTYPES:
        V = NA.vec(dt)
        many = [c for c in NA.LN_MANY if c.dtype == dt]
        assert all(c.kernel == "rows" and c.rows == 32768 + 5 for c in many)
        assert sorted({-(-c.D // V // 64) for c in many}) == [1, 2, 3, 4]
        assert sorted({(c.D // V) % 64 for c in many}) == [0, 1, 16]          # one lane, 2 x 64 + 16, and full
        assert {(c.bias, c.row_bias) for c in many} == {(a, b) for a in (True, False) for b in (True, False)}
        assert {c.kernel for c in NA.LN_SMALL if c.dtype == dt} == {"wave", "block"}
        assert all(c.rows % 4 and c.residual for c in NA.LN_SMALL)
    assert [c.kernel for c in NA.LN_EDGE] == ["rows", "wave", "wave", "block", "block"]
    assert [c.rows for c in NA.LN_EDGE] == [32768, 32767, 32768, 32768, 32768]
    assert (32768 + 5) % 8 == 5 and -(-(32768 + 5) // 32) * 4 - -(-(32768 + 5) // 8) == 3     # tail wave, idle waves


def test_tiled_rows_are_the_judged_rows():
    t = torch.arange(37 * 8.0).reshape(37, 8)
    big = NA.tile_rows(t, 32773)
    assert big.shape == (32773, 8) and torch.equal(big, t[torch.arange(32773) % 37])
    assert NA.tile_rows(t[:7], 7).shape == (7, 8)


def test_gpu_file_runs_the_judged_inputs():
    """tests/test_norms_dispatch_gpu.py takes its cases, its generators, its references and the criterion from the
    helper: what this file judges is what runs on the GPU."""
    G = importlib.import_module("test_norms_dispatch_gpu")
    assert G.NA is NA
    assert set(G.LN_RUN) == {c.name for c in NA.LN_CASES}
    assert set(G.RMS_RUN) == {c.name for c in NA.RMS_CASES} and set(G.GATED_RUN) == {c.name for c in NA.GATED_CASES}
    assert all(G.LN_RUN[c.name] is c for c in NA.LN_CASES)
    assert G.ACT_SIZES is NA.act_sizes and G.ACT_INPUTS is NA.act_inputs
    src = open(G.__file__).read()
    assert "TOL[" not in src and "test_ops_gpu" not in src.replace("test_ops_gpu.py", "")


# ----------------------------------------------------------------------------------- the restatement passes, and c
_MEASURED = {}


def measured(op, dtype):
    """asserts the criterion on every case of (op, dtype); returns the c the restatement needs there"""
    if (op, dtype) not in _MEASURED:
        worst = 0.0
        for name, (y, ref, scale) in evaluations(op, dtype):
            NA.assert_norm_close(y, ref, scale, dtype, name, op)
            worst = max(worst, NA.measured_c(y, ref, scale, dtype))
        _MEASURED[op, dtype] = worst
    return _MEASURED[op, dtype]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("op", list(C))
def test_restatement_passes(op, dtype):
    worst = measured(op, dtype)
    print(f"measured c {op} {NA.DTYPE_ID[dtype]}: {worst:.2f} (chosen {C[op]:g})")
    assert 4 * worst <= C[op], (op, worst)


@pytest.mark.parametrize("op", list(C))
def test_c_is_four_times_the_measured_value(op):
    """c = max(16, 4 x measured), the measured value the largest over the dtypes; rounded up, and not past 8 x."""
    worst = max(measured(op, dt) for dt in DTYPES)
    assert max(16.0, 4 * worst) <= C[op] <= max(16.0, 8 * worst), (op, worst)


# ------------------------------------------------------------------------------------------------- the mutations
def _bits16(c):
    return c.dtype != F32


MUTATIONS = {
    # LayerNorm
    ("layernorm", "row_bias_third_vector"): lambda c: c.row_bias and c.D > 2 * 64 * NA.vec(c.dtype),   # there is a third vector
    ("layernorm", "padded_width"): lambda c: NA.ln_padded(c.D, c.dtype, c.kernel) != c.D,              # the lanes are not all used
    # only the exact rows (|mean| = 192 steps) lose their variance to the cancellation; they exist without a row bias.  In a
    # row of one lane (D <= 8) the sum of the squares has at most 19 bits: E[x^2] - mean^2 is exact there, too
    ("layernorm", "one_pass_variance"): lambda c: not c.row_bias and c.D > 8,
    # var ~ 1e-6 = eps on the std 1e-3 rows; a row bias of 0.05 lifts var to 2.5e-3: eps is 2e-4 of it, seen in fp32 only
    ("layernorm", "eps_omitted"): lambda c: not c.row_bias or c.dtype == F32,
    ("layernorm", "stale_last_row"): lambda c: True,
    ("layernorm", "delta_unrounded"): lambda c: c.residual and _bits16(c),       # in fp32 the fp32 sum IS the rounded one
    # RMSNorm
    ("rmsnorm", "padded_width"): lambda c: rms_padded(c) != c.D,
    ("rmsnorm", "eps_omitted"): lambda c: True,
    ("rmsnorm", "stale_last_row"): lambda c: True,
    ("rmsnorm", "delta_unrounded"): lambda c: c.residual and _bits16(c),
    ("rmsnorm", "weight_in_act_dtype"): lambda c: c.wdtype == F32 and _bits16(c),
    # gated RMSNorm
    ("gated", "padded_width"): lambda c: gated_padded(c) != c.gs,
    ("gated", "eps_omitted"): lambda c: True,
    ("gated", "stale_last_row"): lambda c: True,
    ("gated", "row_mean"): lambda c: c.D // c.gs > 1,
    ("gated", "weight_in_act_dtype"): lambda c: c.wdtype == F32 and _bits16(c),
}


def test_mutation_table_is_complete():
    assert {m for o, m in MUTATIONS if o == "layernorm"} == set(NA.LN_MUTATIONS)
    assert {m for o, m in MUTATIONS if o == "rmsnorm"} == set(NA.RMS_MUTATIONS)
    assert {m for o, m in MUTATIONS if o == "gated"} == set(NA.GATED_MUTATIONS)


@pytest.mark.parametrize("op,mutation", list(MUTATIONS), ids=[f"{o}-{m}" for o, m in MUTATIONS])
def test_every_mutation_fails_the_criterion(op, mutation):
    cases, ev = OPS[op]
    hit = [c for c in cases if MUTATIONS[op, mutation](c)]
    assert {c.dtype for c in hit} >= ({BF16, F16} if mutation in ("delta_unrounded", "weight_in_act_dtype")
                                      else set(DTYPES)), "a dtype has no case that shows this mutation"
    smallest = float("inf")
    for c in hit:
        y, ref, scale = ev(c, mutation)
        ex = float(NA.excess(y, ref, scale, c.dtype, C[op]).max())
        smallest = min(smallest, ex)
        with pytest.raises(AssertionError, match="exceeds half_ulp"):
            NA.assert_norm_close(y, ref, scale, c.dtype, f"{c.name} {mutation}", op)
    print(f"{op} {mutation}: {len(hit)} cases, smallest worst-element excess {smallest:.3e}")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_tanh_gelu_fails_the_criterion(dtype):
    """The tanh approximation is within 5e-4 of the erf form: the absolute 2e-2 of the old check cannot tell them apart."""
    y, ref, scale = gelu_eval(dtype, "tanh")
    assert float((y.double() - ref).abs().max()) < 2e-2
    with pytest.raises(AssertionError, match="exceeds half_ulp"):
        NA.assert_norm_close(y, ref, scale, dtype, "tanh gelu", "gelu")
