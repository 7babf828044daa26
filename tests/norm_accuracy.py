"""Elementwise judgement of the kernels of csrc/norms.hip against an fp64 reference, the inputs the GPU tests run them
on, and an fp32 restatement of each kernel's arithmetic (tests/test_norm_accuracy_cpu.py mutates it).

Criterion, per element, `ref` and `scale` in fp64 from the SAME rounded inputs the kernel reads:

    |y - ref| <= half_ulp(dtype, ref) + c * 2^-24 * scale

  * half_ulp: the kernels compute an fp32 value and round it ONCE to the output type: 2^-8 |ref| for bf16, 2^-11 |ref| for
    fp16, and never less than half the spacing of the format's subnormals (2^-25 for fp16: a gated-norm output below
    2^-14 is a subnormal and cannot be rounded finer; 2^-134 for bf16).  fp32: no such term, the c term bounds that case.
  * scale: LayerNorm |w xhat| + |b|; RMSNorm and gated norm |w xhat|; GELU |x| (the erf polynomial's documented error of
    1.5e-7, times |x| / 2).
  * an output that is not finite where the reference is fails.

c is measured, not guessed: the fp32 torch restatements below round where the kernels round (the sum x + delta to the
activation type; the fp32 row bias added to it in fp32 before the statistics; the mean first, then the sum of squared
deviations; one rounding of the output), tests/test_norm_accuracy_cpu.py runs them on every input family of the GPU
tests (the same generator and seeds; the GPU tests tile the same BASE_ROWS rows to their row count) and takes the largest
err / (2^-24 scale) over the elements whose half-ulp term does not already cover the error; c = max(16, 4 x that).  The
factor 4 is for what the GPU does differently: the order of the sums, rsqrtf / rcpf / exp2f good to 1 ulp, and the erf
polynomial's 1.5e-7.

    operator    measured (fp32 / bf16 / fp16 cases)    c
    layernorm   8.60 / 1.03 / 1.40                     36
    rmsnorm     3.09 / 0 / 0                           16
    gated       4.73 / 0 / 0                           20
    gelu        4.82 / 1.08 / 1.90                     20
(0: the half-ulp term alone covers every element.)

LayerNorm inputs.  The scale above has no term for the rounding of the MEAN: an element that sits on its row's mean has
xhat = 0, scale = |b|, and any fp32 mean fails it.  The inputs therefore keep every element at least half a standard
deviation away from the row mean (|x - mean| = sigma (0.5 + |n|), signs paired so that the mean is the offset), which
bounds min |xhat| at ~ 0.3; offsets stay within 1.5 sigma.  Rows with |mean| >> std, which separate a two-pass variance
from E[x^2] - mean^2, are built so that the two-pass arithmetic is EXACT in fp32 in any summation order: a constant row
(-48: the output must be exactly the bias) and a constant row (96) with one element a step (0.5) above and one a step
below (every partial sum is a multiple of 0.5 below 2^23, the mean is exactly 96, the deviations exactly 0 and +-0.5).
These two families are left out where a row bias is added: 96 + 0.05 is rounded to fp32 before the mean is subtracted,
an error of 2^-24 * 96 on a deviation of 0.05, which the criterion (rightly) has no room for.
Row families cycle with the row index: (sigma 2, mean 0), (sigma 2, mean 3), (sigma 1e-3, mean 0),
(sigma 1e-3, mean -1.5e-3), and without a row bias also the two exact ones."""
import zlib
from collections import namedtuple

import torch

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
DTYPE_ID = {F32: "fp32", BF16: "bf16", F16: "fp16"}
HALF_ULP = {BF16: 2.0 ** -8, F16: 2.0 ** -11, F32: 0.0}
HALF_TINY = {BF16: 2.0 ** -134, F16: 2.0 ** -25, F32: 0.0}       # half the spacing of the subnormals
U = 2.0 ** -24
C = {"layernorm": 36.0, "rmsnorm": 16.0, "gated": 20.0, "gelu": 20.0}
BASE_ROWS = 37          # distinct rows of every norm input; odd, so a tiled copy meets every wave and row slot
LN_EPS, RMS_EPS = 1e-6, 1e-5


def vec(dtype):
    """channels per 16-byte vector"""
    return 4 if dtype == F32 else 8


# ----------------------------------------------------------------------------------------------------- criterion
def tolerance(ref64, scale64, dtype, c):
    return torch.clamp_min(HALF_ULP[dtype] * ref64.abs(), HALF_TINY[dtype]) + c * U * scale64


def excess(y, ref64, scale64, dtype, c):
    """err - tolerance per element (fp64); +inf where the output is not finite."""
    err = (y.double() - ref64).abs()
    ex = err - tolerance(ref64, scale64, dtype, c)
    return torch.where(torch.isfinite(err), ex, torch.full_like(ex, float("inf")))


def measured_c(y, ref64, scale64, dtype):
    """largest (err - half_ulp term) / (2^-24 scale): the c this output needs."""
    err = (y.double() - ref64).abs()
    assert bool(torch.isfinite(err).all())
    over = err - torch.clamp_min(HALF_ULP[dtype] * ref64.abs(), HALF_TINY[dtype])
    need = torch.where(over > 0, over / (U * scale64), torch.zeros_like(over))       # scale 0 and over > 0: inf
    return float(need.max())


def assert_norm_close(y, ref64, scale64, dtype, what, op):
    """Every element of y within the criterion of the module docstring, with c = C[op].  The message names the worst
    row, the worst column and the excess.  Returns the largest err / tolerance (printed: pytest -s)."""
    assert y.shape == ref64.shape == scale64.shape, (y.shape, ref64.shape, scale64.shape)
    assert y.dtype == dtype, (y.dtype, dtype)
    D = y.shape[-1] if y.dim() > 1 else y.numel()
    ex = excess(y, ref64, scale64, dtype, C[op]).reshape(-1, D)
    flat = int(ex.argmax())
    row, col = flat // D, flat % D
    worst = float(ex.flatten()[flat])
    nbad = int((ex > 0).sum())
    print(f"norm-close {what}: worst excess {worst:.3e} at row {row} col {col}, {nbad} of {ex.numel()} over")
    assert worst <= 0, (f"{what}: row {row}, column {col}: |y - ref| exceeds half_ulp + {C[op]:g} * 2^-24 * scale by "
                        f"{worst:.3e} (y {float(y.reshape(-1, D)[row, col]):.9g}, ref "
                        f"{float(ref64.reshape(-1, D)[row, col]):.9g}); {nbad} of {ex.numel()} elements over")


# ------------------------------------------------------------------------------------- fp64 references (any device)
def rounded_sum(x, delta):
    """s = x + delta as the contract has it: added in fp32, rounded to the activation type (`sum_out`, bit for bit)."""
    return x if delta is None else (x.float() + delta.float()).to(x.dtype)


def layernorm_ref64(x, w, b, eps, delta=None, row_bias=None):
    s = rounded_sum(x, delta).double()
    if row_bias is not None:
        s = s + row_bias.double()
    d = s - s.mean(-1, keepdim=True)
    wx = w.double() * (d / torch.sqrt((d * d).mean(-1, keepdim=True) + eps))
    if b is None:
        return wx, wx.abs()
    return wx + b.double(), wx.abs() + b.double().abs().expand_as(wx)


def rmsnorm_ref64(x, w, eps, delta=None):
    s = rounded_sum(x, delta).double()
    ref = w.double() * (s / torch.sqrt((s * s).mean(-1, keepdim=True) + eps))
    return ref, ref.abs()


def gated_ref64(x, z, w, eps, gs):
    u = x.double()
    if z is not None:
        u = u * (z.double() * torch.sigmoid(z.double()))
    g = u.reshape(*u.shape[:-1], -1, gs)
    g = g / torch.sqrt((g * g).mean(-1, keepdim=True) + eps)
    ref = w.double() * g.reshape(u.shape)
    return ref, ref.abs()


def gelu_ref64(x):
    xd = x.double()
    return 0.5 * xd * (1.0 + torch.erf(xd * 0.7071067811865476)), xd.abs()


# --------------------------------------------------------------------- fp32 restatements of the kernels, and mutations
LN_MUTATIONS = ["row_bias_third_vector", "padded_width", "one_pass_variance", "eps_omitted", "stale_last_row",
                "delta_unrounded"]
RMS_MUTATIONS = ["padded_width", "eps_omitted", "stale_last_row", "delta_unrounded", "weight_in_act_dtype"]
GATED_MUTATIONS = ["padded_width", "eps_omitted", "stale_last_row", "row_mean", "weight_in_act_dtype"]


def _sum_fp32(x, delta, mutation):
    if delta is None:
        return x.float()
    s = x.float() + delta.float()
    return s if mutation == "delta_unrounded" else s.to(x.dtype).float()


def layernorm_fp32(x, w, b, eps, delta=None, row_bias=None, mutation=None, padded=None):
    """layernorm_*_kernel in fp32 torch.  `padded`: the width the lanes cover (mutation padded_width)."""
    D = x.shape[-1]
    s = _sum_fp32(x, delta, mutation)
    if row_bias is not None:
        rb = row_bias.float().clone()
        if mutation == "row_bias_third_vector":
            rb[2 * 64 * vec(x.dtype):3 * 64 * vec(x.dtype)] = 0
        s = s + rb
    n = float(padded if mutation == "padded_width" else D)
    mean = s.sum(-1, keepdim=True) / n
    d = s - mean
    if mutation == "one_pass_variance":
        var = (s * s).sum(-1, keepdim=True) / n - mean * mean
    else:
        var = (d * d).sum(-1, keepdim=True) / n
    rstd = torch.rsqrt(var + (0.0 if mutation == "eps_omitted" else torch.tensor(eps, dtype=F32)))
    y = d * rstd * w.float()
    y = (y if b is None else y + b.float()).to(x.dtype)
    if mutation == "stale_last_row":
        y[-1] = y[-2]
    return y


def rmsnorm_fp32(x, w, eps, delta=None, mutation=None, padded=None):
    D = x.shape[-1]
    s = _sum_fp32(x, delta, mutation)
    n = float(padded if mutation == "padded_width" else D)
    rstd = torch.rsqrt((s * s).sum(-1, keepdim=True) / n + (0.0 if mutation == "eps_omitted" else torch.tensor(eps, dtype=F32)))
    wf = w.to(x.dtype).float() if mutation == "weight_in_act_dtype" else w.float()
    y = (wf * (s * rstd)).to(x.dtype)
    if mutation == "stale_last_row":
        y[-1] = y[-2]
    return y


def gated_fp32(x, z, w, eps, gs, mutation=None, padded=None):
    u = x.float()
    if z is not None:
        zf = z.float()
        u = u * (zf * torch.sigmoid(zf))
    g = u.reshape(*u.shape[:-1], -1, gs)
    ssq = (g * g).sum(-1, keepdim=True) / float(padded if mutation == "padded_width" else gs)
    if mutation == "row_mean":
        ssq = ssq.mean(-2, keepdim=True).expand_as(ssq)
    rstd = torch.rsqrt(ssq + (0.0 if mutation == "eps_omitted" else torch.tensor(eps, dtype=F32)))
    wf = w.to(x.dtype).float() if mutation == "weight_in_act_dtype" else w.float()
    y = (wf * (g * rstd).reshape(u.shape)).to(x.dtype)
    if mutation == "stale_last_row":
        y[-1] = y[-2]
    return y


def gelu_fp32(x):
    """gelu_erf of norms.hip: Abramowitz & Stegun 7.1.26 with sqrt(2) / 2 folded into the coefficients."""
    xf = x.float()
    z = xf.abs() * 0.70710678118654752
    t = 1.0 / (0.3275911 * z + 1.0)
    p = 0.750526965 * t - 1.02753365
    p = p * t + 1.00509131
    p = p * t - 0.201169565
    p = p * t + 0.180191725
    p = p * t
    r = 0.70710678118654752 - p * torch.exp2(z * z * -1.4426950408889634)
    return (z * r + 0.5 * xf).to(x.dtype)


# ------------------------------------------------------------------------------------------------ LayerNorm cases
LNCase = namedtuple("LNCase", "name dtype rows D bias row_bias residual kernel")
MANY = 32768 + 5        # 4 097 waves of 8 rows: the last holds 5; 1 025 blocks of 4 waves: three waves of the last exit
# D per NV instantiation of layernorm_rows_kernel (NV = ceil(D / V / 64)), the last vector partly filled
LN_ROWS_D = {16: (8, 520, 1152, 2048), 32: (4, 260, 576, 1024)}
LN_BLOCK_D = {16: (2056, 8192), 32: (1028, 4096)}


def ln_kernel(rows, D, dtype, residual):
    """launch_ln's choice, restated: 'rows' = layernorm_rows_kernel, 'wave' = layernorm_wave_kernel, 'block'."""
    nv = D // vec(dtype)
    if nv <= 256 and rows >= 4096 * 8 and not residual:
        return "rows"
    return "wave" if nv <= 256 else "block"


def ln_padded(D, dtype, kernel):
    """the width the kernel's lanes cover: 64 (256 in the block kernel) lanes x V, times the vectors a lane holds"""
    lanes = (256 if kernel == "block" else 64) * vec(dtype)
    return -(-D // lanes) * lanes


def _ln(dtype, rows, D, bias, row_bias, residual, tag=""):
    k = ln_kernel(rows, D, dtype, residual)
    name = f"{tag}{DTYPE_ID[dtype]}-r{rows}-D{D}-{'b' if bias else 'nob'}-{'rb' if row_bias else 'norb'}" \
           f"{'-res' if residual else ''}-{k}"
    return LNCase(name, dtype, rows, D, bias, row_bias, residual, k)


def _ln_cases():
    many, edge, small = [], [], []
    for dtype in (F32, BF16, F16):
        bits = 32 if dtype == F32 else 16
        for D in LN_ROWS_D[bits]:
            for bias in (True, False):
                for rb in (True, False):
                    many.append(_ln(dtype, MANY, D, bias, rb, False))
        for D in LN_ROWS_D[bits][:1] + LN_ROWS_D[bits][2:3] + LN_BLOCK_D[bits]:
            for rows, rb in ((7, False), (13, True)):
                small.append(_ln(dtype, rows, D, True, rb, True))
    edge.append(_ln(BF16, 32768, 1152, True, True, False))          # exactly at the threshold: rows kernel
    edge.append(_ln(BF16, 32767, 1152, True, True, False))          # one row short: wave kernel
    edge.append(_ln(BF16, 32768, 1152, True, True, True))           # a residual operand: wave kernel
    edge.append(_ln(BF16, 32768, 2056, True, True, False))          # 257 vectors > 256: block kernel
    edge.append(_ln(F32, 32768, 1152, True, True, False))           # fp32: 288 vectors > 256: block kernel
    return many, edge, small


LN_MANY, LN_EDGE, LN_SMALL = _ln_cases()
LN_CASES = LN_MANY + LN_EDGE + LN_SMALL


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _paired(g, rows, D):
    """(rows, D) values sigma-free: |v| = 0.5 + |n|, second half the negated first: zero mean, none within 0.5 of it"""
    half = (0.5 + torch.randn(rows, D // 2, generator=g).abs()) * (torch.randint(0, 2, (rows, D // 2), generator=g) * 2 - 1)
    return torch.cat([half, -half], -1)


def ln_inputs(case):
    """The BASE_ROWS (or fewer) distinct rows of a LayerNorm case, on the CPU: dict x, delta, w, b, rb (None where the
    case has none), rounded to the case's dtype (rb: fp32).  See the module docstring for the row families."""
    P, D, dt = min(case.rows, BASE_ROWS), case.D, case.dtype
    g = _gen("ln", DTYPE_ID[dt], D, case.bias, case.row_bias, case.residual)
    fam = torch.arange(P) % (4 if case.row_bias else 6)
    sigma = torch.tensor([2.0, 2.0, 1e-3, 1e-3, 0.0, 0.0])[fam][:, None]
    off = torch.tensor([0.0, 3.0, 0.0, -1.5e-3, 96.0, -48.0])[fam][:, None]
    s = off + sigma * _paired(g, P, D)
    for r in (fam == 4).nonzero().flatten().tolist():
        i = int(torch.randint(0, D, (1,), generator=g))
        j = (i + 1 + int(torch.randint(0, D - 1, (1,), generator=g))) % D
        s[r, i] += 0.5
        s[r, j] -= 0.5
    out = {"delta": None, "b": None, "rb": None}
    if case.residual:
        t = 0.3 + 0.4 * torch.rand(P, D, generator=g)
        t[fam >= 4] = 0.5
        out["x"], out["delta"] = (s * t).to(dt), (s * (1 - t)).to(dt)
    else:
        out["x"] = s.to(dt)
    out["w"] = (1 + 0.25 * torch.randn(D, generator=g)).to(dt)
    if case.bias:
        out["b"] = (0.5 * torch.randn(D, generator=g)).to(dt)
    if case.row_bias:       # entries of 0.03 .. 0.07, both signs, zero mean
        out["rb"] = (_paired(g, 1, D)[0].sign() * (0.03 + 0.04 * torch.rand(D, generator=g))).float()
        out["rb"][D // 2:] = -out["rb"][:D // 2]
    return out


def tile_rows(t, rows):
    """(P, D) -> (rows, D): row r is t[r % P]"""
    return t.repeat(-(-rows // t.shape[0]), 1)[:rows].contiguous()


# ----------------------------------------------------------------------------------- RMSNorm and gated-norm cases
RMSCase = namedtuple("RMSCase", "name dtype wdtype rows D residual")
GatedCase = namedtuple("GatedCase", "name dtype wdtype rows D gs gate")


def _rms_cases():
    out = []
    for dtype, wdts, Ds in ((BF16, (F32, BF16), (8, 1152, 4480, 8192)), (F16, (F32, F16), (8, 1152, 4480, 8192)),
                            (F32, (F32,), (8, 1152, 4096))):
        for wdt in wdts:
            for D in Ds:
                for res in (False, True):
                    out.append(RMSCase(f"{DTYPE_ID[dtype]}-w{DTYPE_ID[wdt]}-D{D}{'-res' if res else ''}",
                                       dtype, wdt, 7, D, res))
    return out


def _gated_cases():
    out = []
    # (rows, D, gs): rows * groups = 21, 15, 6 waves: none a multiple of the 4 waves of a block
    for dtype, wdts, shapes in ((BF16, (F32, BF16), ((7, 24, 8), (5, 3840, 1280), (3, 4096, 2048))),
                                (F16, (F32, F16), ((7, 24, 8), (5, 3840, 1280), (3, 4096, 2048))),
                                (F32, (F32,), ((7, 12, 4), (3, 2048, 1024)))):
        for wdt in wdts:
            for rows, D, gs in shapes:
                for gate in (True, False):
                    out.append(GatedCase(f"{DTYPE_ID[dtype]}-w{DTYPE_ID[wdt]}-r{rows}-D{D}-g{gs}{'-z' if gate else ''}",
                                         dtype, wdt, rows, D, gs, gate))
    return out


RMS_CASES, GATED_CASES = _rms_cases(), _gated_cases()


def _row_sigma(rows):
    return torch.tensor([2.0, 1e-3])[torch.arange(rows) % 2][:, None]


def rms_inputs(case):
    """x (rows std 2 and std 1e-3 in turn), delta (None without residual), w in the case's weight dtype; CPU."""
    g = _gen("rms", case.name)
    sig = _row_sigma(case.rows)
    x = (sig * torch.randn(case.rows, case.D, generator=g)).to(case.dtype)
    delta = (sig * torch.randn(case.rows, case.D, generator=g)).to(case.dtype) if case.residual else None
    w = (1 + 0.25 * torch.randn(case.D, generator=g)).to(case.wdtype)
    return {"x": x, "delta": delta, "w": w}


def gated_inputs(case):
    """x and z as column windows [16, 16 + D) and [16 + D, 16 + 2 D) of one (rows, 2 D + 32) buffer, the way the mixer
    passes its in_proj output; group k of x is scaled by 1 + k (the groups' rms differ); w; CPU."""
    g = _gen("gated", case.name)
    buf = torch.randn(case.rows, 2 * case.D + 32, generator=g)
    scale = (1.0 + torch.arange(case.D // case.gs)).repeat_interleave(case.gs)
    buf[:, 16:16 + case.D] *= _row_sigma(case.rows) * scale
    buf[:, 16 + case.D:16 + 2 * case.D] *= 2.0
    buf = buf.to(case.dtype)
    w = (1 + 0.25 * torch.randn(case.D, generator=g)).to(case.wdtype)
    return {"buf": buf, "x": buf[:, 16:16 + case.D], "z": buf[:, 16 + case.D:16 + 2 * case.D] if case.gate else None,
            "w": w}


# ------------------------------------------------------------------------------------------------- activations
ACT_GRID = 8192 * 256       # vectors per grid stride of gelu_kernel: the grid is capped at 8 192 blocks of 256 lanes


def act_sizes(dtype):
    """name -> n.  The 4-wide loop runs while i + 3 * ACT_GRID < nvec.  'main': nvec = 5 * ACT_GRID + 300: one 4-wide
    pass for every lane (i < ACT_GRID), then lanes i + 4 * ACT_GRID < nvec take the one-vector loop, then 3 ragged
    elements.  'below' / 'above': nvec = 4 * ACT_GRID -+ 1: without / with the vector that lets the LAST lane
    (i = ACT_GRID - 1) into the 4-wide loop."""
    V = vec(dtype)
    return {"main": (5 * ACT_GRID + 300) * V + 3, "below": (4 * ACT_GRID - 1) * V, "above": (4 * ACT_GRID + 1) * V}


def act_inputs(n, dtype, device, seed):
    """3 * randn rounded to dtype, with exact zeros, -0.0 and |x| > 6 planted; generated on `device`."""
    g = torch.Generator(device=device).manual_seed(seed)
    x = (3.0 * torch.randn(n, generator=g, device=device)).to(dtype)
    x[0:n:1009] = 0.0
    x[1:n:2003] = -0.0
    x[2:n:4001] = 7.5
    x[3:n:4003] = -9.0
    return x


def act_cpu_values(dtype):
    """What the CPU test judges the GELU restatement on.  16-bit: EVERY finite value of the format, so whatever the
    device generator draws has been judged.  fp32: the same family (seeded on the CPU) at 2^20 elements."""
    if dtype == F32:
        return act_inputs(1 << 20, dtype, "cpu", 1)
    v = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(dtype)
    return v[torch.isfinite(v.float())]
