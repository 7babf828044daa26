"""Parity of every HIP operator against the CPU oracle (same seeded inputs) and the
reference-generated golden fixtures.  Calls go through the C ABI (ctypes)."""
import math
import os

import numpy as np
import pytest
from pathlib import Path
import torch

from attn_accuracy import assert_rows_close
from conftest import golden_state_dict, load_golden
from oracle import ops as R

pytestmark = pytest.mark.gpu
DEV = "cuda"


def close(a, b, rtol, atol, what=""):
    a, b = a.detach().double().cpu(), torch.as_tensor(b).double().cpu()
    assert a.shape == b.shape, (a.shape, b.shape)
    err = (a - b).abs()
    tol = atol + rtol * b.abs()
    bad = (err > tol)
    assert not bad.any(), f"{what}: {bad.sum().item()} / {bad.numel()} out of tolerance, max abs err {err.max().item():.3e}"


TOL = {torch.float32: (1e-4, 1e-5), torch.bfloat16: (2e-2, 2e-2), torch.float16: (4e-3, 4e-3)}


@pytest.fixture(scope="module")
def K():
    from timeviper_amd import kernels
    return kernels


# ------------------------------------------------------------------ conv1d
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,L,C,Kw", [(2, 45, 96, 4), (1, 200, 256, 4), (1, 3, 64, 4),
                                      (1, 1, 64, 2), (2, 130, 2048 + 64, 3)])
def test_conv1d(K, dtype, B, L, C, Kw):
    g = torch.Generator().manual_seed(L * 7 + C)
    x = torch.randn(B, L, C, generator=g)
    w = torch.randn(C, Kw, generator=g) * 0.5
    b = torch.randn(C, generator=g) * 0.1
    xd, wd, bd = (t.to(dtype) for t in (x, w, b))
    ref = R.causal_conv1d_ref(xd.float(), wd.float(), bd.float())
    y = K.causal_conv1d_fn(xd.to(DEV).transpose(1, 2), wd.to(DEV), bd.to(DEV), activation="silu")
    assert y.shape == (B, C, L)
    close(y.transpose(1, 2), ref, *TOL[dtype], "conv1d")
    # no bias / no activation
    y2 = K.causal_conv1d_fn(xd.to(DEV).transpose(1, 2), wd.to(DEV), None, activation=None)
    close(y2.transpose(1, 2), R.causal_conv1d_ref(xd.float(), wd.float(), None, None), *TOL[dtype])


def test_conv1d_strided_slice_and_halo(K):
    """x is a column slice of a wider projection (row stride > C); halo continues a shard."""
    g = torch.Generator().manual_seed(1)
    wide = torch.randn(1, 70, 64 + 128 + 8, generator=g).to(torch.bfloat16)
    w = (torch.randn(128, 4, generator=g) * 0.5).to(torch.bfloat16)
    b = (torch.randn(128, generator=g) * 0.1).to(torch.bfloat16)
    xs = wide[:, :, 64:192]
    ref = R.causal_conv1d_ref(xs.float(), w.float(), b.float())
    wd = wide.to(DEV)
    y = K.causal_conv1d_fn(wd[:, :, 64:192].transpose(1, 2), w.to(DEV), b.to(DEV), activation="silu")
    close(y.transpose(1, 2), ref, *TOL[torch.bfloat16])
    y2 = K.causal_conv1d_fn(wd[:, 30:, 64:192].transpose(1, 2), w.to(DEV), b.to(DEV),
                            activation="silu", halo=wd[:, 27:30, 64:192])
    close(y2.transpose(1, 2), ref[:, 30:], *TOL[torch.bfloat16])


def test_conv1d_golden(K):
    g = load_golden("mixer_g1")
    sd = golden_state_dict(g)
    x = torch.from_numpy(g["xBC_pre"]).to(DEV)
    y = K.causal_conv1d_fn(x.transpose(1, 2), sd["conv1d.weight"].squeeze(1).to(DEV),
                           sd["conv1d.bias"].to(DEV), activation="silu")
    close(y.transpose(1, 2), g["xBC_conv"], 1e-4, 1e-5)


def test_conv1d_update(K):
    g = torch.Generator().manual_seed(3)
    st = torch.randn(2, 96, 4, generator=g).to(torch.bfloat16)
    x = torch.randn(2, 96, generator=g).to(torch.bfloat16)
    w = (torch.randn(96, 4, generator=g) * 0.5).to(torch.bfloat16)
    b = (torch.randn(96, generator=g) * 0.1).to(torch.bfloat16)
    yr, sr = R.causal_conv1d_update_ref(x.float(), st.float(), w.float(), b.float())
    sd = st.to(DEV).clone()
    y = K.causal_conv1d_update(x.to(DEV), sd, w.to(DEV), b.to(DEV), "silu")
    close(y, yr, *TOL[torch.bfloat16])
    close(sd, sr, 0, 0)


# ------------------------------------------------------------------- norms
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("rows,D", [(5, 64), (33, 4480), (2, 1152), (1, 8192)])
def test_rmsnorm(K, dtype, rows, D):
    if dtype == torch.float32 and D > 4096:
        pytest.skip("fp32 rows are capped at 4096 columns")
    g = torch.Generator().manual_seed(D)
    x = (torch.randn(rows, D, generator=g) * 2).to(dtype)
    w = (1 + 0.1 * torch.randn(D, generator=g)).to(dtype)
    y = K.rms_norm(x.to(DEV), w.to(DEV), 1e-5)
    close(y, R.rmsnorm_ref(x.float(), w.float(), 1e-5), *TOL[dtype])
    # fused residual add: sum rounded to dtype first, like the reference's bf16 add
    d = (torch.randn(rows, D, generator=g)).to(dtype)
    y2, s2 = K.rms_norm(x.to(DEV), w.to(DEV), 1e-5, residual=d.to(DEV), return_sum=True)
    s_ref = (x + d)
    assert torch.equal(s2.cpu(), s_ref), "residual sum must be bit-exact"
    close(y2, R.rmsnorm_ref(s_ref.float(), w.float(), 1e-5), *TOL[dtype])


def test_rmsnorm_golden(K):
    g = load_golden("rmsnorm")
    y = K.rms_norm(torch.from_numpy(g["x"]).to(DEV), torch.from_numpy(g["w"]).to(DEV), float(g["eps"]))
    close(y, g["y"], 1e-5, 1e-6)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("rows,D,gs", [(7, 64, 64), (19, 10240, 1280), (3, 256, 32), (2, 2048, 2048)])
def test_rmsnorm_gated(K, dtype, rows, D, gs):
    if dtype == torch.float32 and gs > 1024:
        pytest.skip("fp32 groups are capped at 1024 columns")
    g = torch.Generator().manual_seed(D + gs)
    x = torch.randn(rows, D, generator=g).to(dtype)
    z = torch.randn(rows, D, generator=g).to(dtype)
    w = (1 + 0.1 * torch.randn(D, generator=g)).to(dtype)
    y = K.rmsnorm_fn(x.to(DEV), w.to(DEV), None, z.to(DEV), 1e-5, gs, norm_before_gate=False)
    close(y, R.rmsnorm_gated_ref(x.float(), w.float(), z.float(), 1e-5, gs), *TOL[dtype])
    y2 = K.rmsnorm_fn(x.to(DEV), w.to(DEV), None, None, 1e-5, gs, norm_before_gate=False)
    close(y2, R.rmsnorm_gated_ref(x.float(), w.float(), None, 1e-5, gs), *TOL[dtype])


# --------------------------------------------------------------------- scan
def scan_inputs(B, L, H, P, G, N, seed, dtype):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, L, H, P, generator=g).to(dtype)
    dt = (torch.randn(B, L, H, generator=g) * 0.5).to(dtype)
    A = -(torch.rand(H, generator=g) * 15 + 1)
    Bm = (torch.randn(B, L, G, N, generator=g) * 0.5).to(dtype)
    Cm = (torch.randn(B, L, G, N, generator=g) * 0.5).to(dtype)
    D = torch.rand(H, generator=g) + 0.5
    dtv = torch.exp(torch.rand(H, generator=g) * (math.log(0.1) - math.log(1e-3)) + math.log(1e-3))
    dt_bias = dtv + torch.log(-torch.expm1(-dtv))
    return x, dt, A, Bm, Cm, D, dt_bias


def run_scan(K, x, dt, A, Bm, Cm, D, dt_bias, **kw):
    d = lambda t: None if t is None else t.to(DEV)
    return K.mamba_chunk_scan_combined(d(x), d(dt), d(A), d(Bm), d(Cm), chunk_size=64, D=d(D),
                                       dt_bias=d(dt_bias), dt_softplus=True,
                                       return_final_states=True, return_total_decay=True, **kw)


@pytest.mark.parametrize("impl", [1, 0, 6, 8])      # (3 / 4, the slice marches: test_ssd_scan_march_kernels)
@pytest.mark.parametrize("dtype,B,L,H,P,G,N", [
    (torch.float32, 1, 1024, 32, 64, 1, 16),      # BASELINE config 1
    (torch.float32, 2, 77, 8, 8, 2, 16),
    (torch.float32, 1, 5, 4, 24, 4, 40),
    (torch.float32, 2, 1000, 6, 50, 3, 24),       # ragged last chunk, head_dim not a multiple of 4, 16 chunks
    (torch.bfloat16, 1, 300, 16, 80, 2, 128),     # Nano head shape
    (torch.bfloat16, 2, 129, 8, 64, 8, 128),
    (torch.bfloat16, 1, 1, 8, 80, 1, 128),
    (torch.bfloat16, 1, 700, 4, 48, 2, 64),       # bf16 at a d_state the marches do not take
])
def test_ssd_scan(K, impl, dtype, B, L, H, P, G, N):
    if impl == 8 and (N > 64 or L <= 64):
        pytest.skip("the chunk-parallel generic kernel takes d_state <= 64 and at least two chunks")
    if impl == 6 and (dtype != torch.bfloat16 or N != 128):
        pytest.skip("MFMA march kernels are bf16 / d_state 128")
    K.ssd_scan_set_impl(impl)
    try:
        ins = scan_inputs(B, L, H, P, G, N, L + H, dtype)
        f = [t.float() for t in ins]
        y_ref, fin_ref, dec_ref = R.ssd_recurrence_ref(*f[:5], D=f[5], dt_bias=f[6])
        y, fin, dec = run_scan(K, *ins)
        if impl == 8 or (impl == 0 and N <= 64 and L > 64):
            assert K.ssd_scan_last_impl() == 8, "the chunk-parallel generic kernel did not run"
        rt, at = TOL[dtype]
        close(y, y_ref, rt, at * 2, "y")
        close(fin, fin_ref, rt, at, "final state")
        close(dec, dec_ref, 1e-4, 1e-4, "total decay")
        if impl == 8:       # ... and with a state carried in
            g = torch.Generator().manual_seed(L)
            init = torch.randn(B, H, P, N, generator=g)
            y_ref, fin_ref, dec_ref = R.ssd_recurrence_ref(*f[:5], D=f[5], dt_bias=f[6], initial_states=init)
            y, fin, dec = run_scan(K, *ins, initial_states=init.to(DEV))
            close(y, y_ref, rt, at * 2, "y (initial state)")
            close(fin, fin_ref, rt, at, "final state (initial state)")
    finally:
        K.ssd_scan_set_impl(0)


def test_ssd_scan_nano_geometry_vs_oracle(K):
    """The scan at the MODEL's geometry against the token-by-token fp64 recurrence: 128 heads of 80 in 8 groups (16 heads —
    four work-groups of the head march — share one B / C group, modeling_nano.py:639-653), d_state 128, 4 200 tokens (two
    sequence segments and the carried-in correction), A = 1 .. 128 and a raw dt of standard deviation 1.3 as in the
    synthetic 9B model (floating, re-basing, reset and standard steps all occur).  x, B, C come out of the conv + split +
    C.B^T kernel at d_inner 10 240 / G 8 and are checked against the oracle's conv first; the scan then runs on the
    default path with those fragments (head march, asserted)."""
    B, L, H, P, G, N = 1, 4200, 128, 80, 8, 128
    d_in, conv_dim = H * P, H * P + 2 * G * N
    g = torch.Generator().manual_seed(4200)
    xBC = (torch.randn(B, L, conv_dim, generator=g) * 1.5).bfloat16()
    w = (torch.randn(conv_dim, 1, 4, generator=g) * 0.4).bfloat16()
    b = (torch.randn(conv_dim, generator=g) * 0.1).bfloat16()
    dt = (torch.randn(B, L, H, generator=g) * 1.3).bfloat16()
    A = -torch.arange(1, H + 1, dtype=torch.float32)
    D = torch.rand(H, generator=g) + 0.5
    dtv = torch.exp(torch.rand(H, generator=g) * (math.log(0.1) - math.log(1e-3)) + math.log(1e-3))
    dt_bias = dtv + torch.log(-torch.expm1(-dtv))
    x, Bm, Cm, cb = K.causal_conv1d_xbc(xBC.to(DEV), w.to(DEV), b.to(DEV), d_in, G, N, return_cb=True)
    assert cb is not None
    ref = R.causal_conv1d_ref(xBC.float(), w.float(), b.float(), "silu")
    close(x, ref[..., :d_in], *TOL[torch.bfloat16], "conv x")
    close(Bm, ref[..., d_in:d_in + G * N].view(B, L, G, N), *TOL[torch.bfloat16], "conv B")
    close(Cm, ref[..., d_in + G * N:].view(B, L, G, N), *TOL[torch.bfloat16], "conv C")
    xh = x.view(B, L, H, P)
    y, fin, dec = K.mamba_chunk_scan_combined(xh, dt.to(DEV), A.to(DEV), Bm, Cm, chunk_size=128, D=D.to(DEV),
                                              dt_bias=dt_bias.to(DEV), dt_softplus=True, return_final_states=True,
                                              return_total_decay=True, cb=cb)
    assert K.ssd_scan_last_impl() == 6, "the scan did not run on the head-per-wave march"
    # the oracle on the SAME bf16 x / B / C the kernel read
    y_ref, fin_ref, dec_ref = R.ssd_recurrence_ref(xh.float().cpu(), dt.float(), A, Bm.float().cpu(), Cm.float().cpu(), D=D,
                                                   dt_bias=dt_bias)
    close(y, y_ref, 2e-2, 4e-2, "y")
    close(fin, fin_ref, 2e-2, 2e-2, "final state")
    close(dec, dec_ref, 1e-4, 1e-3, "total decay")
    rel = float((y.float().cpu().double() - y_ref).norm() / y_ref.norm())
    assert rel < 6e-3, rel            # bf16 outputs of fp32 sums: the error is the rounding of y


@pytest.mark.parametrize("dtype,H,P,G,N", [(torch.float32, 8, 16, 2, 16), (torch.bfloat16, 16, 80, 8, 128)])
def test_ssd_scan_initial_state_and_sharding(K, dtype, H, P, G, N):
    """shard chaining through initial_states == single pass."""
    L, s = 333, 140
    ins = scan_inputs(1, L, H, P, G, N, 11, dtype)
    x, dt, A, Bm, Cm, D, dt_bias = ins
    y, fin, dec = run_scan(K, *ins)
    y0, f0, d0 = run_scan(K, x[:, :s], dt[:, :s], A, Bm[:, :s], Cm[:, :s], D, dt_bias)
    y1, f1, d1 = run_scan(K, x[:, s:], dt[:, s:], A, Bm[:, s:], Cm[:, s:], D, dt_bias,
                          initial_states=f0)
    rt, at = TOL[dtype]
    close(torch.cat([y0, y1], 1), y.cpu(), rt, at * 2)
    close(f1, fin.cpu(), rt, at)
    close(d0 + d1, dec.cpu(), 1e-4, 1e-4)
    f = [t.float() for t in ins]
    _, fin_ref, _ = R.ssd_recurrence_ref(*f[:5], D=f[5], dt_bias=f[6])
    close(f1, fin_ref, rt, at)


_MARCH_SHAPES = [(1, 1000, 16, 80, 8), (2, 449, 8, 64, 2), (1, 64, 4, 48, 1), (1, 2049, 8, 80, 4), (1, 130, 4, 128, 2),
                 (1, 65, 6, 24, 3), (1, 5000, 8, 80, 8), (1, 4100, 4, 72, 2), (2, 2500, 4, 56, 1)]


@pytest.mark.parametrize("B,L,H,P,G", _MARCH_SHAPES)
def test_ssd_scan_march_kernels(K, B, L, H, P, G):
    """the MFMA march kernels (forced): long sequences, ragged tails, several slice widths,
    initial state in, final state / total decay out, 'tile' head->group map.  6 = the head-per-wave march (falls back to
    4 / 3 by head_dim); 4 = whole-head work-groups (head_dim 56..80): from 2 048 tokens on (few heads) it marches 2 or 4
    sequence segments concurrently and completes the later ones with the carried-in state correction; 3 = slices of a
    head.  One fp32 recurrence (the CPU reference: most of the test's time) serves every kernel of a shape."""
    impls = [6] + ([4] if 56 <= P <= 80 and L != 5000 else []) + ([3] if L < 1000 or P == 72 else [])
    ins = scan_inputs(B, L, H, P, G, 128, 3 * L + H, torch.bfloat16)
    g = torch.Generator().manual_seed(L)
    init = torch.randn(B, H, P, 128, generator=g)
    f = [t.float() for t in ins]
    for gmap in ("block", "tile"):
        y_ref, fin_ref, dec_ref = R.ssd_recurrence_ref(*f[:5], D=f[5], dt_bias=f[6], initial_states=init, group_map=gmap)
        for impl in impls:
            K.ssd_scan_set_impl(impl)
            try:
                y, fin, dec = run_scan(K, *ins, initial_states=init.to(DEV), group_map=gmap)
            finally:
                K.ssd_scan_set_impl(0)
            close(y, y_ref, 2e-2, 4e-2, f"y {gmap} impl {impl}")
            close(fin, fin_ref, 2e-2, 2e-2, f"final state {gmap} impl {impl}")
            close(dec, dec_ref, 1e-4, 1e-4, f"total decay impl {impl}")


@pytest.mark.parametrize("regime,a_lo,a_hi,dt_mean,dt_std", [
    ("no decay to speak of", 1e-4, 1e-3, -3.0, 0.3),       # 2^-0.01 a chunk: the frame never moves, the state grows with L
    ("slow", 0.05, 0.3, -1.0, 0.5),                       # a few bits a chunk: floating steps, a re-base every few chunks
    ("at the reset threshold", 0.9, 1.1, 0.0, 0.05),      # ~ 2^-64 a chunk: chunks fall on both sides of it
    ("at the standard threshold", 2.9, 3.2, 0.0, 0.05),   # ~ 2^-200 a chunk
    ("model-like, wide", 1.0, 16.0, 0.0, 1.3),            # what random weights behind an RMSNorm give (bench.py)
    ("violent", 50.0, 200.0, 1.0, 2.0),                   # every chunk forgets everything: standard steps only
    ("token spikes", 0.01, 0.05, -2.0, 4.0),              # mostly slow, single tokens with dt ~ e^8
])
def test_ssd_scan_decay_regimes(K, regime, a_lo, a_hi, dt_mean, dt_std):
    """Every step kind of the head-per-wave march (floating frame, re-base, reset, standard) and the hand-overs between
    them, against the fp32 recurrence; impl 4 (round 2's slice march) takes the same inputs.  Heads of one work-group
    get different A, so the kinds mix inside a work-group; 2 600 tokens = 2 - 4 sequence segments with carried-in
    corrections."""
    B, L, H, P, G, N = 1, 2600, 16, 80, 2, 128
    g = torch.Generator().manual_seed(len(regime))
    x = torch.randn(B, L, H, P, generator=g).to(torch.bfloat16)
    dt = (torch.randn(B, L, H, generator=g) * dt_std + dt_mean).to(torch.bfloat16)
    A = -(torch.rand(H, generator=g) * (a_hi - a_lo) + a_lo)
    Bm = (torch.randn(B, L, G, N, generator=g) * 0.5).to(torch.bfloat16)
    Cm = (torch.randn(B, L, G, N, generator=g) * 0.5).to(torch.bfloat16)
    D = torch.rand(H, generator=g) + 0.5
    ins = (x, dt, A, Bm, Cm, D, torch.zeros(H))
    init = torch.randn(B, H, P, N, generator=g)
    f = [t.float() for t in ins]
    y_ref, fin_ref, dec_ref = R.ssd_recurrence_ref(*f[:5], D=f[5], dt_bias=f[6], initial_states=init)
    for impl in (6, 4):                # (one reference for both kernels: the CPU recurrence is most of the test's time)
        K.ssd_scan_set_impl(impl)
        try:
            y, fin, dec = run_scan(K, *ins, initial_states=init.to(DEV))
        finally:
            K.ssd_scan_set_impl(0)
        assert torch.isfinite(y.float()).all() and torch.isfinite(fin).all()
        # y is bf16 and its terms are products of bf16-rounded operands (x~ = bf16(w x), C.B^T in bf16 — the reference's
        # chunked kernels round the same way) summed with cancellation: the error is judged against the row's magnitude.
        # Measured: 0.025 - 0.033 for both MFMA kernels in every regime (the fp32 generic kernel: 0.004 = the bf16 store).
        scale = y_ref.abs().amax(dim=-1, keepdim=True).clamp_min(1.0)
        err = ((y.float().cpu() - y_ref).abs() / scale).max().item()
        assert err < 5e-2, (regime, impl, err)
        fscale = fin_ref.abs().amax().clamp_min(1.0)
        ferr = ((fin.cpu() - fin_ref).abs().max() / fscale).item()
        assert ferr < 1e-2, (regime, impl, ferr)
        close(dec, dec_ref, 1e-4, 1e-4 * max(1.0, float(dec_ref.abs().max())), f"total decay (impl {impl})")


@pytest.mark.parametrize("regime,a_lo,a_hi,dt_mean,dt_std,L", [
    ("slow", 0.05, 0.3, -1.0, 0.5, 2600),                  # floating steps, re-basing
    ("at the reset threshold", 0.9, 1.1, 0.0, 0.05, 2600),
    ("at the standard threshold", 2.9, 3.2, 0.0, 0.05, 2600),
    ("model-like, wide", 1.0, 16.0, 0.0, 1.3, 4133),        # every step kind mixed inside a work-group; ragged last chunk
    ("violent", 50.0, 200.0, 1.0, 2.0, 1999),               # standard steps only, t-tiles whose row factors underflow
    ("token spikes", 0.01, 0.05, -2.0, 4.0, 2600),
])
def test_ssd_head_generated_step_is_bit_identical_to_the_cpp_step(K, regime, a_lo, a_hi, dt_mean, dt_std, L):
    """The 64-token step of the head-per-wave march at head_dim 80 x 4 heads per work-group runs as one generated instruction
    stream (csrc/ssd_head_step.inc); `ssd_head_kernel<5,4,2>` is the same arithmetic in the same order per accumulator written
    in C++.  y, the final state and the decay total must agree bit for bit in every step kind (tv_ssd_head_set_asm)."""
    B, H, P, G, N = 1, 16, 80, 2, 128
    g = torch.Generator().manual_seed(7 + len(regime))
    x = torch.randn(B, L, H, P, generator=g).to(torch.bfloat16)
    dt = (torch.randn(B, L, H, generator=g) * dt_std + dt_mean).to(torch.bfloat16)
    A = -(torch.rand(H, generator=g) * (a_hi - a_lo) + a_lo)
    Bm = (torch.randn(B, L, G, N, generator=g) * 0.5).to(torch.bfloat16)
    Cm = (torch.randn(B, L, G, N, generator=g) * 0.5).to(torch.bfloat16)
    D = torch.rand(H, generator=g) + 0.5
    ins = (x, dt, A, Bm, Cm, D, torch.zeros(H))
    init = torch.randn(B, H, P, N, generator=g).to(DEV)
    outs = []
    K.ssd_scan_set_impl(6)
    try:
        for on in (1, 0):
            K.ssd_head_set_asm(on)
            y, fin, dec = run_scan(K, *ins, initial_states=init)
            assert K.ssd_scan_last_impl() == 6
            outs.append((y.clone(), fin.clone(), dec.clone()))
    finally:
        K.ssd_head_set_asm(-1)
        K.ssd_scan_set_impl(0)
    (y1, f1, d1), (y0, f0, d0) = outs
    assert torch.isfinite(y1.float()).all()
    assert torch.equal(y1, y0), (regime, (y1.float() - y0.float()).abs().max().item())
    assert torch.equal(f1, f0), (regime, (f1 - f0).abs().max().item())
    assert torch.equal(d1, d0), regime


@pytest.mark.parametrize("seed", [1, 2])
def test_ssd_head_generated_step_fuzz(K, seed):
    """48 random cases a seed (timeviper_amd/devtools/scan_fuzz.py: shapes, ragged lengths, decay regimes over five decades,
    softplus / dt_limit / D / dt_bias / initial states / strided packed rows / both group maps): generated step == C++ step,
    bit for bit."""
    import importlib.util
    spec = importlib.util.spec_from_file_location(
        "scan_fuzz", Path(__file__).resolve().parent.parent / "timeviper_amd" / "devtools" / "scan_fuzz.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    bad = mod.run(48, seed)
    assert not bad, bad[:3]


@pytest.mark.parametrize("a_lo,a_hi,dt_mean,dt_std", [(0.002, 0.02, -3.0, 0.3), (0.05, 0.3, -1.0, 0.5), (1.0, 16.0, 0.0, 1.3)])
def test_ssd_correction_walker_list_matches_the_grid(K, monkeypatch, a_lo, a_hi, dt_mean, dt_std):
    """The carried-in correction of the segmented march runs its walkers off a list (one per 4 chunks of a (head, boundary)'s horizon,
    persistent work-groups: ssd_correct_list_kernel); TV_CORR_SLOTS=n runs the grid of n work-groups per (head, boundary) instead.
    Every chunk is corrected by exactly one walker either way: y must agree bit for bit — with heads that never forget (whole
    segments corrected), slow ones, and the bench-like mix."""
    B, L, H, P, G, N = 1, 5200, 16, 80, 2, 128           # 82 chunks: 4 - 5 segments
    g = torch.Generator().manual_seed(11)
    x = torch.randn(B, L, H, P, generator=g).to(torch.bfloat16)
    dt = (torch.randn(B, L, H, generator=g) * dt_std + dt_mean).to(torch.bfloat16)
    A = -(torch.rand(H, generator=g) * (a_hi - a_lo) + a_lo)
    Bm = (torch.randn(B, L, G, N, generator=g) * 0.5).to(torch.bfloat16)
    Cm = (torch.randn(B, L, G, N, generator=g) * 0.5).to(torch.bfloat16)
    ins = (x, dt, A, Bm, Cm, torch.ones(H), torch.zeros(H))
    K.ssd_scan_set_impl(6)
    try:
        monkeypatch.delenv("TV_CORR_SLOTS", raising=False)
        y_list, fin_list, _ = run_scan(K, *ins)
        monkeypatch.setenv("TV_CORR_SLOTS", "3")
        y_grid, fin_grid, _ = run_scan(K, *ins)
    finally:
        K.ssd_scan_set_impl(0)
    assert torch.equal(y_list, y_grid), (y_list.float() - y_grid.float()).abs().max().item()
    assert torch.equal(fin_list, fin_grid)
    f = [t.float() for t in ins]
    y_ref = R.ssd_recurrence_ref(*f[:5], D=f[5], dt_bias=f[6])[0]
    scale = y_ref.abs().amax(dim=-1, keepdim=True).clamp_min(1.0)
    assert ((y_list.float().cpu() - y_ref).abs() / scale).max().item() < 5e-2


def test_ssd_scan_golden_and_group_maps(K):
    for tag, gmap in [("g1", "block"), ("g2_tile", "tile"), ("g4_tile", "tile")]:
        g = load_golden(f"mixer_{tag}")
        sd = golden_state_dict(g)
        A = -torch.exp(sd["A_log"])
        T = lambda k: torch.from_numpy(g[k])
        y, fin = K.mamba_chunk_scan_combined(
            T("scan_x").to(DEV), T("scan_dt").to(DEV), A.to(DEV), T("scan_B").to(DEV),
            T("scan_C").to(DEV), chunk_size=16, D=sd["D"].to(DEV), dt_bias=sd["dt_bias"].to(DEV),
            dt_softplus=True, return_final_states=True, group_map=gmap)
        close(y, g["scan_y"], 1e-4, 2e-5, tag)
        close(fin, g["scan_final"], 1e-4, 2e-5, tag)


def test_ssd_scan_strided_views(K):
    """x/B/C are column slices of the conv output, dt of the in_proj output."""
    H, P, G, N, L = 16, 80, 8, 128, 150
    g = torch.Generator().manual_seed(5)
    conv = (torch.randn(1, L, H * P + 2 * G * N, generator=g) * 0.5).to(torch.bfloat16)
    proj = (torch.randn(1, L, 40 + H, generator=g) * 0.5).to(torch.bfloat16)
    _, _, A, _, _, D, dt_bias = scan_inputs(1, L, H, P, G, N, 5, torch.bfloat16)
    x, Bm, Cm = conv.split([H * P, G * N, G * N], dim=-1)
    dt = proj[..., 40:]
    y_ref, fin_ref, _ = R.ssd_recurrence_ref(x.float().view(1, L, H, P), dt.float(), A,
                                             Bm.float().view(1, L, G, N), Cm.float().view(1, L, G, N),
                                             D=D, dt_bias=dt_bias)
    cd, pd = conv.to(DEV), proj.to(DEV)
    xd, Bd, Cd = cd.split([H * P, G * N, G * N], dim=-1)
    y, fin = K.mamba_chunk_scan_combined(
        xd.view(1, L, H, P), pd[..., 40:], A.to(DEV), Bd.view(1, L, G, N), Cd.view(1, L, G, N),
        chunk_size=128, D=D.to(DEV), dt_bias=dt_bias.to(DEV), dt_softplus=True,
        return_final_states=True)
    close(y, y_ref, 2e-2, 4e-2)
    close(fin, fin_ref, 2e-2, 2e-2)


@pytest.mark.parametrize("B,H,P,G,N", [(2, 8, 16, 2, 32), (1, 128, 80, 8, 128), (3, 4, 24, 1, 16), (1, 6, 7, 3, 256),
                                       (1, 4, 8, 2, 40)])      # (N = 40: the thread-per-row kernel)
def test_selective_state_update(K, B, H, P, G, N):
    ins = scan_inputs(B, 1, H, P, G, N, 9, torch.bfloat16)
    x, dt, A, Bm, Cm, D, dt_bias = ins
    g = torch.Generator().manual_seed(2)
    st = torch.randn(B, H, P, N, generator=g)
    y_ref, fin_ref, _ = R.ssd_recurrence_ref(x.float(), dt.float(), A, Bm.float(), Cm.float(), D=D,
                                             dt_bias=dt_bias, initial_states=st)
    sd = st.to(DEV).clone()
    y = K.selective_state_update(sd, x[:, 0].to(DEV), dt[:, 0].to(DEV), A.to(DEV), Bm[:, 0].to(DEV),
                                 Cm[:, 0].to(DEV), D.to(DEV), dt_bias=dt_bias.to(DEV), dt_softplus=True)
    close(y, y_ref[:, 0], 2e-2, 2e-2)
    close(sd, fin_ref, 1e-4, 1e-5)


@pytest.mark.parametrize("L,H,P,G,slow", [(300, 8, 40, 2, False), (1000, 16, 80, 8, True), (64, 4, 64, 1, True),
                                          (5, 8, 80, 4, False), (2000, 8, 80, 8, False)])
def test_ssd_state_correction_completes_a_zero_state_scan(K, L, H, P, G, slow):
    """y(scan from S_in) = y(scan from 0) + exp(cs_t) C_t . S_in: the in-place
    correction on top of the zero-state scan against the oracle recurrence started from S_in.
    `slow`: heads that barely decay (the term stays alive over the whole range); otherwise most heads
    forget within a few chunks and the kernel's early exit is what runs."""
    g = torch.Generator().manual_seed(L + H)
    N = 128
    x = torch.randn(1, L, H, P, generator=g).bfloat16()
    dt = (torch.randn(1, L, H, generator=g) * 0.5 - (4.0 if slow else 0.0)).bfloat16()
    A = -(torch.rand(H, generator=g) * (0.5 if slow else 15) + (0.01 if slow else 1))
    Bm = (torch.randn(1, L, G, N, generator=g) * 0.5).bfloat16()
    Cm = (torch.randn(1, L, G, N, generator=g) * 0.5).bfloat16()
    D = torch.rand(H, generator=g) + 0.5
    dtb = torch.full((H,), -1.0)
    S0 = torch.randn(1, H, P, N, generator=g)
    y_ref, _, _ = R.ssd_recurrence_ref(x.float(), dt.float(), A, Bm.float(), Cm.float(), D=D, dt_bias=dtb,
                                       initial_states=S0)
    d = lambda t: t.to(DEV)
    y0 = K.mamba_chunk_scan_combined(d(x), d(dt), d(A), d(Bm), d(Cm), chunk_size=64, D=d(D), dt_bias=d(dtb),
                                     dt_softplus=True)
    y_direct = K.mamba_chunk_scan_combined(d(x), d(dt), d(A), d(Bm), d(Cm), chunk_size=64, D=d(D), dt_bias=d(dtb),
                                           dt_softplus=True, initial_states=d(S0))
    y = K.ssd_state_correction(y0.clone(), d(dt), d(A), d(Cm), d(S0), dt_bias=d(dtb), dt_softplus=True)
    assert y.data_ptr() != y0.data_ptr()
    # y0 is rounded to bf16 before the carried-in term is added: where the two nearly cancel the
    # result keeps that rounding (half a bf16 ulp of the larger term), so the absolute tolerance
    # scales with the magnitude of the terms
    at = max(4e-2, 8e-3 * float(y_ref.abs().max()))
    close(y, y_ref, 2e-2, at, "corrected zero-state scan vs oracle from S_in")
    close(y, y_direct.float(), 2e-2, at, "corrected zero-state scan vs the kernel started from S_in")
    if not slow and L >= 1000:      # far past every head's horizon nothing may change, bit for bit
        assert torch.equal(y[:, 600:], y0[:, 600:])


def test_ssd_state_correction_truncation_bound(K):
    """The carried-in term is dropped once its factor has fallen below 2^-32 (include/timeviper_hip.h,
    csrc/ssd_correct.hip C_UNDERFLOW): on y = 0, heads from "forgets in a few chunks" to "never forgets" and a
    LARGE entering state, every element the kernel left at zero is below 2^-32 sum_n |C_tn S_pn|, and every
    element it wrote is the exact fp64 term to the bf16 rounding of S_in and of the result."""
    L, H, P, G, N = 4096, 8, 80, 2, 128
    g = torch.Generator().manual_seed(11)
    dt = (torch.randn(1, L, H, generator=g) * 0.3 - 3.0).bfloat16()
    A = -torch.tensor([0.002, 0.01, 0.05, 0.2, 1.0, 4.0, 9.0, 16.0])
    Cm = (torch.randn(1, L, G, N, generator=g) * 0.5).bfloat16()
    dtb = torch.full((H,), -1.0)
    S0 = torch.randn(1, H, P, N, generator=g) * 1.0e3
    d = lambda t: t.to(DEV)
    y = K.ssd_state_correction(torch.zeros(1, L, H, P, dtype=torch.bfloat16, device=DEV), d(dt), d(A), d(Cm), d(S0),
                               dt_bias=d(dtb), dt_softplus=True).double().cpu()[0]            # (L, H, P)
    dtd = torch.nn.functional.softplus(dt.double()[0] + dtb.double())                          # (L, H)
    cs2 = torch.cumsum(dtd * A.double(), 0) * math.log2(math.e)                                # log2 of the factor
    Ch = Cm.double()[0].repeat_interleave(H // G, dim=1)                                       # (L, H, N)
    exact = torch.einsum("lhn,hpn->lhp", Ch, S0.double()[0]) * torch.exp2(cs2)[:, :, None]
    mag = torch.einsum("lhn,hpn->lhp", Ch.abs(), S0.double()[0].abs())
    dropped = (y == 0) & (exact != 0)
    assert dropped.any() and (~dropped).any()
    assert (exact.abs()[dropped] <= 2.0 ** -31.99 * mag[dropped]).all(), "a dropped term exceeds the 2^-32 bound"
    # nothing is dropped before the factor has reached 2^-32 at the START of its 64-token chunk
    first_of_chunk = cs2[(torch.arange(L) // 64) * 64 - 1].clamp(max=0.0)
    first_of_chunk[:64] = 0.0
    assert not (dropped & (first_of_chunk[:, :, None] > -31.99)).any(), "stopped before the horizon"
    err = (y - exact).abs()[~dropped]
    bound = (2.0 ** -7 * mag * torch.exp2(cs2)[:, :, None] + 1e-30)[~dropped]
    assert (err <= bound).all(), f"max excess {(err / bound).max().item():.3f}"


# ---------------------------------------------------------------- attention
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("B,Lq,Lk,Hq,Hkv,D,causal", [
    (1, 200, 200, 8, 2, 128, True),
    (2, 129, 129, 4, 4, 64, True),
    (1, 64, 64, 5, 1, 128, True),
    (1, 100, 333, 8, 2, 128, False),     # TransV cross attention: few queries, many keys
    (1, 9, 21, 4, 2, 16 * 0 + 64, False),
    (3, 729, 729, 2, 2, 72, False),      # SigLIP ViT heads
    (2, 257, 257, 2, 2, 88, False),      # InternVideo2 ViT heads
    (1, 50, 180, 4, 2, 128, True),       # bottom-right aligned causal (Lk > Lq)
    (1, 1, 77, 8, 2, 128, True),         # decode-like single query
    (1, 300, 300, 4, 2, 80, True),
    (1, 130, 130, 4, 2, 96, False),
    (5, 300, 300, 13, 13, 72, False),    # 65 (batch, head) pairs: the XCD-ordered 1-D grid, padded to 72
    (9, 700, 200, 8, 4, 64, False),      # same path, 3 query blocks, GQA, Lk < Lq
])
def test_flash_attention(K, dtype, B, Lq, Lk, Hq, Hkv, D, causal):
    g = torch.Generator().manual_seed(Lq * 3 + Lk + D)
    q = torch.randn(B, Lq, Hq, D, generator=g).to(dtype)
    k = torch.randn(B, Lk, Hkv, D, generator=g).to(dtype)
    v = torch.randn(B, Lk, Hkv, D, generator=g).to(dtype)
    o_ref, lse_ref = R.attention_ref(q.float(), k.float(), v.float(), causal)
    o, lse = K.flash_attn_func(q.to(DEV), k.to(DEV), v.to(DEV), causal=causal, return_lse=True)
    rt, at = (2e-2, 1e-2) if dtype == torch.bfloat16 else (4e-3, 2e-3)
    close(o, o_ref, rt, at, "o")
    assert_rows_close(o, o_ref, dtype, f"prefill {Lq}x{Lk} H {Hq}/{Hkv} d {D} causal {causal}")
    close(lse, lse_ref, 1e-3, 2e-3, "lse")


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("B,Lq,Lk,Hq,Hkv,D", [
    (24, 729, 729, 16, 16, 72),      # SigLIP frames: 144 query blocks per XCD for 32 resident work-groups
    (20, 300, 500, 8, 4, 64),        # Lq != Lk, GQA, 4 k-steps
    (11, 257, 257, 16, 16, 88),      # InternVideo2 heads (6 k-steps), 3 ragged key tiles
    (7, 600, 97, 16, 16, 72),        # two key tiles, the second holds ONE key
    (13, 300, 300, 13, 13, 72),      # 169 (batch, head) pairs padded to 176: the last XCD's range ends early
    (12, 400, 300, 16, 8, 80),       # head_dim 80: K uses all five k-steps, the ones column is V column 80 (chunk 10); GQA
])
def test_flash_attention_streaming(K, dtype, B, Lq, Lk, Hq, Hkv, D):
    """Many short sequences: `flash_fwd_stream_kernel` (one resident work-group per CU walks the query blocks;
    K/V ring, Q prefetch and O stores cross the block seams).  q / k / v are strided views of a packed
    projection, as in the ViT blocks (siglip.py Attention)."""
    g = torch.Generator().manual_seed(Lq * 5 + Lk + D)
    qkv = torch.randn(B, max(Lq, Lk), Hq + 2 * Hkv, D, generator=g).to(dtype).to(DEV)
    q, k, v = qkv[:, :Lq, :Hq], qkv[:, :Lk, Hq:Hq + Hkv], qkv[:, :Lk, Hq + Hkv:]
    # a few dominant keys in late tiles: the running maximum moves after the first tile
    k[:, Lk - 1] *= 4.0
    k[:, Lk // 2] *= 3.0
    o_ref, lse_ref = R.attention_ref(q.float().cpu(), k.float().cpu(), v.float().cpu(), False)
    o, lse = K.flash_attn_func(q, k, v, causal=False, return_lse=True)
    rt, at = (2e-2, 1e-2) if dtype == torch.bfloat16 else (4e-3, 2e-3)
    close(o, o_ref, rt, at, "o")
    assert_rows_close(o, o_ref, dtype, f"ViT auto {B}x{Lq}x{Lk} H {Hq}/{Hkv} d {D}")
    close(lse, lse_ref, 1e-3, 2e-3, "lse")
    o2 = K.flash_attn_func(q, k, v, causal=False)                  # same bits on a second call (no stale ring state)
    assert torch.equal(o, o2)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("B,Lq,Lk,Hq,Hkv,D", [
    (24, 729, 729, 16, 16, 72),      # SigLIP: pad chunks 9..15 of the rings, the ones column is V column 72
    (11, 257, 257, 16, 16, 88),      # InternVideo2: pad chunks 11..15, ones column 88, ragged last tile
    (7, 600, 97, 16, 16, 72),        # the second key tile holds ONE key (its other rows repeat it, weight 0)
    (12, 400, 300, 16, 8, 80),       # head_dim 80: no K pad column inside the k-steps, ones column 80
])
def test_flash_attention_streaming_row_sums_on_the_matrix_pipe(K, dtype, B, Lq, Lk, Hq, Hkv, D):
    """The default streaming kernel takes P's row sums out of the P.V MFMAs (a 1.0 column in the V ring's first pad chunk,
    copy lanes of the pad chunks switched off); `flash_attn_set_variant(3)` is the same kernel with the sums on the vector
    pipe.  Same products, `l` summed from the rounded weights instead of the fp32 ones: the outputs differ by rounding
    only (one step of the output type on a few elements), the log-sum-exp by less than 2e-3."""
    g = torch.Generator().manual_seed(Lq * 11 + Lk + D)
    qkv = torch.randn(B, max(Lq, Lk), Hq + 2 * Hkv, D, generator=g).to(dtype).to(DEV)
    q, k, v = qkv[:, :Lq, :Hq], qkv[:, :Lk, Hq:Hq + Hkv], qkv[:, :Lk, Hq + Hkv:]
    q = q * 2.0                                                    # sharper rows: few keys carry the weight
    k[:, Lk - 1] *= 4.0
    K.flash_attn_set_variant(5)               # (the compiled streaming kernel; 0 = auto takes the generated tile loop for bf16)
    try:
        o1, lse1 = K.flash_attn_func(q, k, v, causal=False, return_lse=True)
        K.flash_attn_set_variant(3)
        o0, lse0 = K.flash_attn_func(q, k, v, causal=False, return_lse=True)
    finally:
        K.flash_attn_set_variant(0)
    assert torch.isfinite(o1.float()).all()
    eps = 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -11
    d = (o1.float() - o0.float()).abs()
    assert (d <= 2 * eps * o0.float().abs() + 1e-6).all(), d.max().item()
    assert (d > 0).float().mean().item() < 0.5                     # most elements round to the same value
    assert (lse1 - lse0).abs().max().item() < 2e-3
    o_ref, _ = R.attention_ref(q.float().cpu(), k.float().cpu(), v.float().cpu(), False)
    e1 = (o1.float().cpu() - o_ref).norm() / o_ref.norm()
    e0 = (o0.float().cpu() - o_ref).norm() / o_ref.norm()
    assert e1 < 1.05 * e0 + 1e-5, (e1.item(), e0.item())           # and is no further from the fp32 oracle
    assert_rows_close(o1, o_ref, dtype, f"ViT variant 5 {B}x{Lq}x{Lk} H {Hq}/{Hkv} d {D}")         # ... row by row, each
    assert_rows_close(o0, o_ref, dtype, f"ViT variant 3 {B}x{Lq}x{Lk} H {Hq}/{Hkv} d {D}")


@pytest.mark.parametrize("B,Lq,Lk,Hq,Hkv,D,sharp", [
    (24, 729, 729, 16, 16, 72, 1.0),     # SigLIP frames: 8 key tiles, the last one holds 57 keys
    (24, 729, 729, 16, 16, 72, 6.0),     # sharp rows with late spikes: the lazy maximum has to move (rescale path)
    (13, 300, 300, 16, 16, 72, 1.0),     # 4 key tiles, 12 keys in the last; query rows past the end in the second block
    (12, 400, 290, 16, 8, 80, 2.0),      # head_dim 80 (no pad column inside the k-steps), grouped K / V heads, Lq != Lk
    (30, 1000, 1000, 16, 16, 72, 1.0),   # 4 query blocks, 11 key tiles
])
def test_flash_attention_generated_tile_loop(K, B, Lq, Lk, Hq, Hkv, D, sharp):
    """`flash_attn_set_variant(4)` (and 0 = auto for bf16): the ViT kernel whose key-tile loop is a generated instruction stream
    (csrc/attention_vit.hpp <- devtools/gen_fa_vit.py: one wave per SIMD, 64 query rows a wave, software-pipelined across
    tiles, lazy running maximum) against the fp32 oracle and the default kernel: as close to the oracle as the default
    kernel is, log-sum-exp to 2e-3, same bits on a second call."""
    g = torch.Generator().manual_seed(Lq * 7 + Lk + D)
    qkv = torch.randn(B, max(Lq, Lk), Hq + 2 * Hkv, D, generator=g).bfloat16().to(DEV)
    q, k, v = qkv[:, :Lq, :Hq], qkv[:, :Lk, Hq:Hq + Hkv], qkv[:, :Lk, Hq + Hkv:]
    q = q * sharp
    if sharp > 2:
        k[:, Lk - 3] *= 3.0                                        # a late key that lifts many rows' maxima by more than 2^24
        k[:, 200] *= 2.0
    K.flash_attn_set_variant(5)               # the compiled streaming kernel
    try:
        o0, lse0 = K.flash_attn_func(q, k, v, causal=False, return_lse=True)
        K.flash_attn_set_variant(4)
        o1, lse1 = K.flash_attn_func(q, k, v, causal=False, return_lse=True)
        o2 = K.flash_attn_func(q, k, v, causal=False)
    finally:
        K.flash_attn_set_variant(0)
    assert torch.isfinite(o1.float()).all() and torch.equal(o1, o2)
    assert not torch.equal(o1, o0) or sharp == 0                   # (another kernel ran: P is rounded relative to another maximum)
    o_ref, lse_ref = R.attention_ref(q.float().cpu(), k.float().cpu(), v.float().cpu(), False)
    close(o1, o_ref, 2e-2, 1e-2, "o")
    close(lse1, lse_ref, 1e-3, 2e-3, "lse")
    e1 = (o1.float().cpu() - o_ref).norm() / o_ref.norm()
    e0 = (o0.float().cpu() - o_ref).norm() / o_ref.norm()
    assert e1 < 1.15 * e0 + 1e-5, (e1.item(), e0.item())
    assert_rows_close(o1, o_ref, torch.bfloat16, f"ViT variant 4 {B}x{Lq}x{Lk} H {Hq}/{Hkv} d {D} sharp {sharp}")
    assert_rows_close(o0, o_ref, torch.bfloat16, f"ViT variant 5 {B}x{Lq}x{Lk} H {Hq}/{Hkv} d {D} sharp {sharp}")


def test_flash_attention_spiked_max(K):
    """force large running-max jumps at chosen tiles (guide rule 26)."""
    g = torch.Generator().manual_seed(0)
    B, L, H, D = 1, 400, 2, 128
    q = torch.randn(B, L, H, D, generator=g)
    k = torch.randn(B, L, H, D, generator=g)
    v = torch.randn(B, L, H, D, generator=g)
    for pos in (70, 200, 390):
        k[0, pos, :, :] = q[0, 399, :, :] * 3.0
    q, k, v = (t.to(torch.bfloat16) for t in (q, k, v))
    o_ref, _ = R.attention_ref(q.float(), k.float(), v.float(), True)
    o = K.flash_attn_func(q.to(DEV), k.to(DEV), v.to(DEV), causal=True)
    close(o, o_ref, 2e-2, 1e-2)
    assert_rows_close(o, o_ref, torch.bfloat16, "prefill spiked max")


# ---------------------------------------------------------------- decode-step linears
@pytest.mark.parametrize("M,N,Kd", [(1, 1000, 4096), (1, 18560, 4096), (3, 777, 4480), (4, 4096, 15680), (1, 131, 64),
                                    (2, 96, 8), (1, 4096, 10240)])
@pytest.mark.parametrize("prologue", ["none", "rmsnorm", "rmsnorm+delta", "relu2", "gated", "gated-nogate"])
def test_gemv_fused_prologues(K, M, N, Kd, prologue):
    """tv_gemv_bf16_fwd against the stand-alone operators + an fp64 product of THEIR bf16 output: the prologue rounds
    where tv_rmsnorm_fwd / tv_relu2_fwd / tv_rmsnorm_gated_fwd round, so f(x) is compared bit for bit (through sum_out
    and a product with the identity) and y to the accumulation order."""
    if prologue.startswith("rmsnorm") and Kd > 8192:
        pytest.skip("the rmsnorm prologue holds rows of <= 8192 channels")
    group = {10240: 1280, 15680: 1960, 4096: 512, 4480: 560, 64: 32, 8: 8}[Kd]
    g = torch.Generator(device=DEV).manual_seed(M * 7 + N + Kd)
    x = torch.randn(M, 1, Kd, device=DEV, generator=g).bfloat16()
    d = (torch.randn(M, 1, Kd, device=DEV, generator=g) * 0.5).bfloat16()
    z = torch.randn(M, 1, Kd, device=DEV, generator=g).bfloat16()
    W = (torch.randn(N, Kd, device=DEV, generator=g) / math.sqrt(Kd)).bfloat16()
    b = torch.randn(N, device=DEV, generator=g).bfloat16() if N % 2 else None
    nw = (1 + 0.1 * torch.randn(Kd, device=DEV, generator=g))
    nw = nw.bfloat16() if M % 2 else nw.float()
    sum_out = None
    if prologue == "none":
        f, kw = x, dict(prologue=K.GEMV_NONE)
    elif prologue == "rmsnorm":
        f, kw = K.rms_norm(x, nw, 1e-5), dict(prologue=K.GEMV_RMSNORM, norm_weight=nw, eps=1e-5)
    elif prologue == "rmsnorm+delta":
        f, s_ref = K.rms_norm(x, nw, 1e-5, residual=d, return_sum=True)
        sum_out = torch.full_like(x, float("nan"))
        kw = dict(prologue=K.GEMV_RMSNORM, norm_weight=nw, eps=1e-5, delta=d, sum_out=sum_out)
    elif prologue == "relu2":
        f, kw = K.relu2(x), dict(prologue=K.GEMV_RELU2)
    else:
        gate = z if prologue == "gated" else None
        f = K.rmsnorm_fn(x, nw, None, z=gate, eps=1e-5, group_size=group, norm_before_gate=False)
        kw = dict(prologue=K.GEMV_GATED, norm_weight=nw, eps=1e-5, gate=gate, group_size=group)
    assert K.gemv_takes(x, W)
    y = K.gemv_fused(x, W, b, **kw)
    assert y.shape == (M, 1, N) and y.dtype == torch.bfloat16
    ref = f.double().view(M, Kd) @ W.double().t() + (0 if b is None else b.double())
    err = (y.double().view(M, N) - ref).abs()
    tol = 2.0 ** -8 * ref.abs() + 2e-3            # one bf16 rounding of y + fp32 accumulation over K
    assert (err <= tol).all(), f"max excess {(err / tol).max().item():.2f}"
    if sum_out is not None:
        assert torch.equal(sum_out, s_ref)
    if Kd <= 4480 and N != 131:                    # f(x) itself, bit for bit: rows of the identity pick its elements
        eye = torch.eye(Kd, device=DEV).bfloat16()
        kw.pop("sum_out", None)
        assert torch.equal(K.gemv_fused(x, eye, None, **kw).view(M, Kd), f.view(M, Kd))


@pytest.mark.parametrize("M", [1, 3])
def test_gemv_fused_conv_epilogue(K, M):
    """The mixer's in_proj -> causal_conv1d_update pair as one launch: rows [row0, row0 + C) of the product go through the
    conv update in the epilogue — bit-equal to the two launches (same product kernel, same conv arithmetic), state
    included, over several tokens."""
    g = torch.Generator(device=DEV).manual_seed(M)
    Kd, d_in, C, H = 512, 320, 448, 24
    N = d_in + C + H
    W = (torch.randn(N, Kd, device=DEV, generator=g) / math.sqrt(Kd)).bfloat16()
    nw = torch.ones(Kd, device=DEV)
    cw = (torch.randn(C, 4, device=DEV, generator=g) * 0.5).bfloat16()
    cb = torch.randn(C, device=DEV, generator=g).bfloat16()
    st_a = torch.randn(M, C, 4, device=DEV, generator=g).bfloat16()
    st_b = st_a.clone()
    for step in range(5):
        x = torch.randn(M, 1, Kd, device=DEV, generator=g).bfloat16()
        two = K.gemv_fused(x, W, None, K.GEMV_RMSNORM, norm_weight=nw, eps=1e-5)
        conv_two = K.causal_conv1d_update(two[:, 0, d_in:d_in + C], st_a, cw, cb, "silu")
        one = K.gemv_fused(x, W, None, K.GEMV_RMSNORM, norm_weight=nw, eps=1e-5, conv=(st_b, cw, cb, d_in))
        assert torch.equal(one[:, 0, d_in:d_in + C], conv_two), step
        assert torch.equal(one[..., :d_in], two[..., :d_in]) and torch.equal(one[..., d_in + C:], two[..., d_in + C:])
        assert torch.equal(st_a, st_b), step
    with pytest.raises(K.TimeViperHipError):
        K.gemv_fused(x, W, None, conv=(st_b[:, :10], cw, cb, d_in))


def test_gemv_fused_strided_rows_and_errors(K):
    g = torch.Generator(device=DEV).manual_seed(0)
    buf = torch.randn(2, 1, 3 * 512, device=DEV, generator=g).bfloat16()
    x, gate = buf[..., 512:1024], buf[..., :512]           # views into wider rows (the mixer's in_proj output)
    W = (torch.randn(300, 512, device=DEV, generator=g) / 20).bfloat16()
    nw = torch.ones(512, device=DEV)
    y = K.gemv_fused(x, W, None, K.GEMV_GATED, norm_weight=nw, eps=1e-5, gate=gate, group_size=128)
    f = K.rmsnorm_fn(x.contiguous(), nw, None, z=gate.contiguous(), eps=1e-5, group_size=128, norm_before_gate=False)
    close(y, (f.float() @ W.float().t()).cpu(), 1e-2, 2e-3)
    assert not K.gemv_takes(torch.zeros(5, 1, 512, device=DEV).bfloat16(), W)          # 5 rows
    assert not K.gemv_takes(x.float(), W)
    with pytest.raises(K.TimeViperHipError):
        K.gemv_fused(torch.zeros(5, 1, 512, device=DEV).bfloat16(), W)
    with pytest.raises(K.TimeViperHipError):
        K.gemv_fused(x, W, None, K.GEMV_RMSNORM)                                        # no norm weight


@pytest.mark.parametrize("B,Lk,Hq,Hkv", [
    (1, 256, 32, 8),         # the smallest cache the split-KV kernel takes: 2 splits x 4 waves x one step
    (1, 257, 32, 8),         # one key in the last step
    (1, 1000, 32, 8),
    (2, 4099, 8, 8),         # no GQA: one real column of the MFMA tile
    (1, 3000, 16, 1),        # 16 q-heads on one kv-head: the whole tile
    (1, 2500, 40, 2),        # 20 q-heads per kv-head: two head blocks
    (3, 777, 12, 4),
    (1, 32868, 32, 8),       # the bench's cache: 2 048 frames
])
def test_flash_attn_decode_split_kv(K, B, Lk, Hq, Hkv):
    """One query token against a cache (modeling_nano.py:1198-1209, q_len 1): fp32 oracle, and the one-row launch of the
    prefill kernel — same operator, other summation order."""
    g = torch.Generator().manual_seed(Lk + Hq)
    q = torch.randn(B, 1, Hq, 128, generator=g).bfloat16()
    k = torch.randn(B, Lk, Hkv, 128, generator=g).bfloat16()
    v = torch.randn(B, Lk, Hkv, 128, generator=g).bfloat16()
    o_ref, lse_ref = R.attention_ref(q.float(), k.float(), v.float(), True)
    qd, kd, vd = q.to(DEV), k.to(DEV), v.to(DEV)
    o, lse = K.flash_attn_decode(qd, kd, vd, return_lse=True)
    close(o, o_ref, 2e-2, 1e-2, "o")
    assert_rows_close(o, o_ref, torch.bfloat16, f"decode B {B} Lk {Lk} H {Hq}/{Hkv}")
    close(lse, lse_ref, 1e-3, 2e-3, "lse")
    # flash_attn_func routes one-query calls here; TV_ATTN_DECODE=0 keeps them on the prefill kernel
    o2 = K.flash_attn_func(qd, kd, vd, causal=True)
    assert torch.equal(o2, o)
    os.environ["TV_ATTN_DECODE"] = "0"
    try:
        o3 = K.flash_attn_func(qd, kd, vd, causal=True)
    finally:
        del os.environ["TV_ATTN_DECODE"]
    close(o, o3.float().cpu(), 2e-2, 1e-2, "against the prefill kernel")
    assert_rows_close(o3, o_ref, torch.bfloat16, f"prefill kernel, one query row, Lk {Lk} H {Hq}/{Hkv}")


def test_flash_attn_decode_device_lengths_and_strided_cache(K):
    """seqlens_k on the device (what a captured decode step replays with): keys past the length are never read into the
    result — they hold NaNs here; the cache buffers are views with a capacity larger than the length."""
    g = torch.Generator().manual_seed(5)
    B, cap, Hq, Hkv = 3, 1500, 32, 8
    lens = [1500, 1, 700]
    q = torch.randn(B, 1, Hq, 128, generator=g).bfloat16().to(DEV)
    kbuf = torch.randn(B, cap + 64, Hkv, 128, generator=g).bfloat16().to(DEV)
    vbuf = torch.randn(B, cap + 64, Hkv, 128, generator=g).bfloat16().to(DEV)
    for b, n in enumerate(lens):
        kbuf[b, n:] = float("nan")
        vbuf[b, n:] = float("nan")
    k, v = kbuf[:, :cap], vbuf[:, :cap]                    # strided views of the capacity buffers
    sl = torch.tensor(lens, dtype=torch.int32, device=DEV)
    o, lse = K.flash_attn_decode(q, k, v, seqlens_k=sl, return_lse=True)
    assert torch.isfinite(o.float()).all() and torch.isfinite(lse).all()
    for b, n in enumerate(lens):
        o_ref, lse_ref = R.attention_ref(q[b:b + 1].float().cpu(), k[b:b + 1, :n].float().cpu(), v[b:b + 1, :n].float().cpu(), True)
        close(o[b:b + 1], o_ref, 2e-2, 1e-2, f"o[{b}]")
        assert_rows_close(o[b:b + 1], o_ref, torch.bfloat16, f"decode device length {n}")
        close(lse[b:b + 1], lse_ref, 1e-3, 2e-3, f"lse[{b}]")
    # a growing cache under ONE set of launch parameters: the length is read on the device
    sl.fill_(10)
    o10 = K.flash_attn_decode(q, k, v, seqlens_k=sl)
    o_ref, _ = R.attention_ref(q[0:1].float().cpu(), k[0:1, :10].float().cpu(), v[0:1, :10].float().cpu(), True)
    close(o10[0:1], o_ref, 2e-2, 1e-2, "length 10")
    assert_rows_close(o10[0:1], o_ref, torch.bfloat16, "decode device length 10")
    with pytest.raises(K.TimeViperHipError):
        K.flash_attn_decode(q, k, v, seqlens_k=sl.to(torch.int64))


def test_flash_attn_decode_spiked_max(K):
    """The running maximum jumps late in a wave's walk and differs by orders of magnitude between splits."""
    g = torch.Generator().manual_seed(1)
    B, Lk, Hq, Hkv = 1, 5000, 32, 8
    q = torch.randn(B, 1, Hq, 128, generator=g)
    k = torch.randn(B, Lk, Hkv, 128, generator=g)
    v = torch.randn(B, Lk, Hkv, 128, generator=g)
    for pos, hq in ((70, 0), (2500, 5), (4999, 31), (33, 17)):
        k[0, pos, hq // 4] = q[0, 0, hq] * 3.0
    q, k, v = (t.bfloat16() for t in (q, k, v))
    o_ref, lse_ref = R.attention_ref(q.float(), k.float(), v.float(), True)
    o, lse = K.flash_attn_decode(q.to(DEV), k.to(DEV), v.to(DEV), return_lse=True)
    close(o, o_ref, 2e-2, 1e-2, "o")
    assert_rows_close(o, o_ref, torch.bfloat16, "decode spiked max")
    close(lse, lse_ref, 1e-3, 2e-3, "lse")


def test_attention_golden_module_level(K):
    """q/k/v projections in torch, attention in HIP: reference NemotronHSdpaAttention output."""
    g = load_golden("attention")
    sd = {k_: v_.to(DEV).to(torch.bfloat16) for k_, v_ in golden_state_dict(g).items()}
    h = torch.from_numpy(g["hidden"]).to(DEV).to(torch.bfloat16)
    Hq, Hkv, D = (int(v) for v in g["meta"])
    B, L, _ = h.shape
    q = (h @ sd["q_proj.weight"].t()).view(B, L, Hq, D)
    k = (h @ sd["k_proj.weight"].t()).view(B, L, Hkv, D)
    v = (h @ sd["v_proj.weight"].t()).view(B, L, Hkv, D)
    o = K.flash_attn_func(q, k, v, causal=True).reshape(B, L, Hq * D) @ sd["o_proj.weight"].t()
    close(o, g["out"], 5e-2, 3e-2)


def test_sdpa_and_varlen_wrappers(K):
    g = torch.Generator().manual_seed(4)
    q = torch.randn(2, 4, 33, 64, generator=g).to(torch.bfloat16)
    k = torch.randn(2, 4, 33, 64, generator=g).to(torch.bfloat16)
    v = torch.randn(2, 4, 33, 64, generator=g).to(torch.bfloat16)
    o_ref, _ = R.attention_ref(q.float().transpose(1, 2), k.float().transpose(1, 2), v.float().transpose(1, 2), False)
    o = K.scaled_dot_product_attention(q.to(DEV), k.to(DEV), v.to(DEV))
    close(o.transpose(1, 2), o_ref, 2e-2, 1e-2)
    assert_rows_close(o.transpose(1, 2), o_ref, torch.bfloat16, "sdpa wrapper")
    qkv = torch.stack([q, k, v], dim=0).permute(1, 3, 0, 2, 4).reshape(2 * 33, 3, 4, 64).contiguous()
    cu = torch.tensor([0, 33, 66], dtype=torch.int32)
    o2 = K.flash_attn_varlen_qkvpacked_func(qkv.to(DEV), cu.to(DEV), 33)
    close(o2.view(2, 33, 4, 64), o_ref, 2e-2, 1e-2)
    assert_rows_close(o2.view(2, 33, 4, 64), o_ref, torch.bfloat16, "varlen wrapper, equal lengths")


# --------------------------------------------------------------- token ops
def test_gather_rows(K):
    g = torch.Generator().manual_seed(8)
    src = torch.randn(500, 4480, generator=g).to(torch.bfloat16)
    idx = torch.randperm(500, generator=g)[:123].sort().values
    out = K.gather_rows(src.to(DEV), idx.to(DEV))
    assert torch.equal(out.cpu(), src[idx])
    src32 = torch.randn(40, 64, generator=g)
    assert torch.equal(K.gather_rows(src32.to(DEV), idx[:10].to(DEV) % 40).cpu(), src32[idx[:10] % 40])
    assert K.gather_rows(src.to(DEV), idx[:0].to(DEV)).shape == (0, 4480)


def test_uniform_keep_indices_bit_exact(K):
    g = load_golden("uniform_indices")
    for n, keep in g["cases"]:
        n, keep = int(n), int(keep)
        got = K.uniform_keep_indices(n, keep).cpu()
        assert torch.equal(got, R.uniform_keep_indices_ref(n, keep)), (n, keep)
        assert torch.equal(got, torch.linspace(0, n - 1, keep, dtype=torch.long)), (n, keep)
    # BASELINE full sizes, with the vision offset
    for n, keep in [(163840, 131072), (160000, 128000), (131072, 98304), (32768, 26214)]:
        got = K.uniform_keep_indices(n, keep, offset=20).cpu()
        assert torch.equal(got, torch.linspace(0, n - 1, keep, dtype=torch.long) + 20)
        assert (got[1:] > got[:-1]).all()          # strictly increasing -> already sorted
    assert torch.equal(K.uniform_keep_indices(10, 1).cpu(), torch.zeros(1, dtype=torch.long))


def test_dropped_indices(K):
    g = torch.Generator().manual_seed(6)
    n, start = 1000, 37
    keep = (torch.randperm(n, generator=g)[:600].sort().values + start)
    allidx = torch.arange(start, start + n)
    ref = allidx[~torch.isin(allidx, keep)]
    got = K.dropped_indices(keep.to(DEV), start, n).cpu()
    assert torch.equal(got, ref)
    assert K.dropped_indices(allidx.to(DEV), start, n).numel() == 0


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_attn_rank_scores(K, dtype):
    g = torch.Generator().manual_seed(12)
    L, Dm, Hq, Hkv, D = 300, 64, 8, 2, 32
    hidden = torch.randn(L, Dm, generator=g).to(dtype)
    qw = (torch.randn(Hq * D, Dm, generator=g) / 8).to(dtype)
    kw = (torch.randn(Hkv * D, Dm, generator=g) / 8).to(dtype)
    vis_start, n_vis, qrow = 10, 250, 279
    ref = R.attn_rank_scores_ref(hidden, qw, kw, Hq, Hkv, D, qrow, vis_start, n_vis)
    hd = hidden.to(DEV)
    q = (hd[qrow:qrow + 1] @ qw.to(DEV).t()).view(Hq, D)
    k = (hd @ kw.to(DEV).t()).view(L, Hkv, D)
    got = K.attn_rank_scores(q, k, qrow + 1, vis_start, n_vis)
    if dtype == torch.float32:
        close(got, ref, 1e-4, 1e-7)
        keep = 100
        assert torch.equal(R.topk_keep_ref(got.cpu(), keep).sort().values,
                           R.topk_keep_ref(ref, keep).sort().values)
    else:
        close(got, ref.float(), 5e-2, 2e-4)
        # bf16: the kept sets may differ only inside the rounding band around the k-th score (tests/keepsets.py)
        from keepsets import assert_keepsets_agree_outside_rounding_band
        for keep in (50, 100, 200):
            assert_keepsets_agree_outside_rounding_band(got, ref, keep)


# -------------------------------------------------------------- patch embed
@pytest.mark.parametrize("F_,C,H,W,p,Dout", [(3, 3, 56, 56, 14, 128), (2, 3, 42, 70, 14, 192),
                                             (1, 3, 32, 32, 16, 64), (5, 3, 28, 28, 14, 1152)])
def test_patch_embed(K, F_, C, H, W, p, Dout):
    g = torch.Generator().manual_seed(H + Dout)
    pix = torch.randn(F_, C, H, W, generator=g).to(torch.bfloat16)
    w = (torch.randn(Dout, C, p, p, generator=g) / math.sqrt(C * p * p)).to(torch.bfloat16)
    b = (torch.randn(Dout, generator=g) * 0.1).to(torch.bfloat16)
    pos = (torch.randn((H // p) * (W // p), Dout, generator=g) * 0.1).to(torch.bfloat16)
    ref = R.patch_embed_ref(pix.float(), w.float(), b.float(), pos.float())
    out = K.patch_embed(pix.to(DEV), w.to(DEV), b.to(DEV), pos.to(DEV))
    close(out, ref, 2e-2, 2e-2)
    out2 = K.patch_embed(pix.to(DEV), w.to(DEV))
    close(out2, R.patch_embed_ref(pix.float(), w.float()), 2e-2, 2e-2)


@pytest.mark.parametrize("p,H,W,Dout,dtype", [(16, 64, 48, 132, torch.bfloat16), (12, 36, 60, 64, torch.float16),
                                              (7, 21, 35, 40, torch.bfloat16), (14, 42, 42, 1152, torch.bfloat16)])
def test_patch_embed_paths(K, p, H, W, Dout, dtype):
    """every staging path: dword rows for patch 16 / 14, the generic vector path (12), scalar rows for
    an odd patch and width (7 x 35), with the packed-weight workspace and (straight through the C
    ABI) without it; channel counts that are not a multiple of the 128-wide tile"""
    from timeviper_amd import _capi
    g = torch.Generator().manual_seed(p * H + W)
    F_, C = 5, 3
    pix = torch.randn(F_, C, H, W, generator=g).to(dtype)
    w = (torch.randn(Dout, C, p, p, generator=g) / (p * 1.7)).to(dtype)
    b = (torch.randn(Dout, generator=g) * 0.1).to(dtype)
    pos = (torch.randn((H // p) * (W // p), Dout, generator=g) * 0.1).to(dtype)
    ref = R.patch_embed_ref(pix.float(), w.float(), b.float(), pos.float())
    tol = TOL[dtype]
    out = K.patch_embed(pix.to(DEV), w.to(DEV), b.to(DEV), pos.to(DEV))
    close(out, ref, *tol, "packed weight")
    pd, wd, bd, psd = pix.to(DEV), w.reshape(Dout, -1).contiguous().to(DEV), b.to(DEV), pos.to(DEV)
    raw = torch.empty_like(out)
    st = _capi.lib().tv_patch_embed_fwd(pd.data_ptr(), wd.data_ptr(), bd.data_ptr(), psd.data_ptr(), raw.data_ptr(),
                                        F_, C, H, W, p, Dout, _capi.TV_BF16 if dtype == torch.bfloat16 else _capi.TV_F16,
                                        None, torch.cuda.current_stream().cuda_stream)
    assert st == 0, _capi.lib().tv_last_error()
    torch.cuda.synchronize()
    close(raw, ref, *tol, "no workspace")
    assert torch.equal(raw, out)          # same products in the same order: bit-identical


def test_patch_embed_video(K):
    g = torch.Generator().manual_seed(77)
    pix = torch.randn(2, 3, 4, 28, 42, generator=g).to(torch.bfloat16)
    w = (torch.randn(96, 3, 1, 14, 14, generator=g) / 24).to(torch.bfloat16)
    b = (torch.randn(96, generator=g) * 0.1).to(torch.bfloat16)
    ref = R.patch_embed_video_ref(pix.float(), w.float(), b.float())
    out = K.patch_embed_video(pix.to(DEV), w.to(DEV), b.to(DEV))
    close(out, ref, 2e-2, 2e-2)


def test_conv1d_xbc_group_major(K):
    """Mamba-2 xBC conv: same numbers as causal_conv1d_fn, B/C returned group-major."""
    g = torch.Generator().manual_seed(21)
    d_in, G, N, L = 160, 2, 128, 77
    wide = torch.randn(2, L, 40 + d_in + 2 * G * N, generator=g).to(torch.bfloat16)
    w = (torch.randn(d_in + 2 * G * N, 4, generator=g) * 0.5).to(torch.bfloat16)
    b = (torch.randn(d_in + 2 * G * N, generator=g) * 0.1).to(torch.bfloat16)
    xs = wide[:, :, 40:]
    ref = R.causal_conv1d_ref(xs.float(), w.float(), b.float())
    x, Bm, Cm = K.causal_conv1d_xbc(wide.to(DEV)[:, :, 40:], w.to(DEV), b.to(DEV), d_in, G, N)
    assert Bm.shape == (2, L, G, N) and Bm.stride(2) == L * N and Bm.stride(1) == N
    close(x, ref[..., :d_in], *TOL[torch.bfloat16])
    close(Bm.reshape(2, L, G * N), ref[..., d_in:d_in + G * N], *TOL[torch.bfloat16])
    close(Cm.reshape(2, L, G * N), ref[..., d_in + G * N:], *TOL[torch.bfloat16])
    # identical bits to the unsplit kernel
    y = K.causal_conv1d_fn(wide.to(DEV)[:, :, 40:].transpose(1, 2), w.to(DEV), b.to(DEV), activation="silu")
    assert torch.equal(y.transpose(1, 2)[..., :d_in], x)
    assert torch.equal(y.transpose(1, 2)[..., d_in:d_in + G * N], Bm.reshape(2, L, G * N))
    # and the scan accepts the group-major views
    H, P = 2, 80
    A = -(torch.rand(H, generator=g) * 15 + 1)
    dt = (torch.randn(2, L, H, generator=g) * 0.5).to(torch.bfloat16)
    y2, fin = K.mamba_chunk_scan_combined(x.view(2, L, H, P), dt.to(DEV), A.to(DEV), Bm, Cm, dt_softplus=True,
                                          return_final_states=True)
    yr, fr, _ = R.ssd_recurrence_ref(x.float().cpu().view(2, L, H, P), dt.float(), A, Bm.float().cpu(), Cm.float().cpu())
    close(y2, yr, 2e-2, 4e-2)
    close(fin, fr, 2e-2, 2e-2)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_layernorm_and_gelu(K, dtype):
    g = torch.Generator().manual_seed(31)
    rows, D = 37, 1152
    x = (torch.randn(rows, D, generator=g) * 2 + 0.5).to(dtype)
    d = torch.randn(rows, D, generator=g).to(dtype)
    w = (1 + 0.1 * torch.randn(D, generator=g)).to(dtype)
    b = (0.1 * torch.randn(D, generator=g)).to(dtype)
    ref = torch.nn.functional.layer_norm(x.float(), (D,), w.float(), b.float(), 1e-6)
    y = K.layer_norm(x.to(DEV), w.to(DEV), b.to(DEV), 1e-6)
    close(y, ref, *TOL[dtype])
    s_ref = x + d
    y2, s2 = K.layer_norm(x.to(DEV), w.to(DEV), b.to(DEV), 1e-6, residual=d.to(DEV), return_sum=True)
    assert torch.equal(s2.cpu(), s_ref)
    close(y2, torch.nn.functional.layer_norm(s_ref.float(), (D,), w.float(), b.float(), 1e-6), *TOL[dtype])
    h = (torch.randn(33, 4304 * 2, generator=g) * 2).to(dtype)
    close(K.gelu(h.to(DEV)), torch.nn.functional.gelu(h.float()), *TOL[dtype])
    for n in (1, 7, 279 * 17):                       # ragged sizes (InternVideo2 toy MLP width 279)
        r = (torch.randn(n, generator=g) * 2).to(dtype)
        close(K.gelu(r.to(DEV)), torch.nn.functional.gelu(r.float()), *TOL[dtype])


@pytest.mark.parametrize("D", [1024, 1152, 4096])     # fp32: wave-per-row kernel up to 1024 columns, block-per-row above
def test_layernorm_large_mean_small_std(K, D):
    """Rows with |mean| >> std: E[x^2] - mean^2 would lose the variance to cancellation (fp32:
    50^2 = 2500 against 0.0025); the kernels take the sum of squared deviations in a second
    register pass, like torch's LayerNorm."""
    g = torch.Generator().manual_seed(77)
    x = 50.0 + 0.05 * torch.randn(19, D, generator=g)
    w = 1 + 0.1 * torch.randn(D, generator=g)
    b = 0.1 * torch.randn(D, generator=g)
    ref = torch.nn.functional.layer_norm(x.double(), (D,), w.double(), b.double(), 1e-6)
    y = K.layer_norm(x.to(DEV), w.to(DEV), b.to(DEV), 1e-6)
    close(y, ref, 2e-3, 2e-3, "layernorm, mean 50 / std 0.05")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_relu2(K, dtype):
    """bit-exact: square(relu(x)) has one rounding in the reference's dtype (modeling_nano.py:993)"""
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(37, 1571, generator=g) * 3).to(dtype)          # ragged: not a multiple of the vector
    ref = torch.square(torch.relu(x))
    y = K.relu2(x.to(DEV))
    assert torch.equal(y.cpu(), ref)
    z = x.to(DEV).clone()
    assert K.relu2(z, inplace=True).data_ptr() == z.data_ptr() and torch.equal(z.cpu(), ref)


def test_zero_length_inputs(K):
    """A rank of the sharded runner can be left with no tokens: every operator must accept
    L = 0 (and a one-token shard with a conv halo)."""
    H, P, G, N = 8, 40, 2, 128
    conv_dim = H * P + 2 * G * N
    e = lambda *s: torch.empty(*s, device=DEV, dtype=torch.bfloat16)
    w, b = torch.randn(conv_dim, 4, device=DEV).bfloat16(), torch.randn(conv_dim, device=DEV).bfloat16()
    x, Bm, Cm = K.causal_conv1d_xbc(e(1, 0, conv_dim), w, b, H * P, G, N)
    assert x.shape == (1, 0, H * P) and Bm.shape == (1, 0, G, N) and Cm.shape == (1, 0, G, N)
    A = -torch.rand(H, device=DEV) - 1
    init = torch.randn(1, H, P, N, device=DEV)
    y, fin, dec = K.mamba_chunk_scan_combined(e(1, 0, H, P), e(1, 0, H), A, Bm, Cm, chunk_size=64,
                                              D=torch.ones(H, device=DEV), dt_softplus=True,
                                              initial_states=init, return_final_states=True,
                                              return_total_decay=True)
    assert y.shape == (1, 0, H, P) and torch.equal(fin, init) and float(dec.abs().max()) == 0.0
    assert K.rms_norm(e(1, 0, 64), torch.ones(64, device=DEV), 1e-5).shape == (1, 0, 64)
    assert K.rmsnorm_fn(e(0, 64), torch.ones(64, device=DEV).bfloat16(), None, e(0, 64), 1e-5, 32,
                        norm_before_gate=False).shape == (0, 64)
    o = K.flash_attn_func(e(1, 0, 4, 64), torch.randn(1, 9, 2, 64, device=DEV).bfloat16(),
                          torch.randn(1, 9, 2, 64, device=DEV).bfloat16(), causal=True)
    assert o.shape == (1, 0, 4, 64)
    # one token + halo == the last row of the same conv over 4 rows
    xs = torch.randn(1, 4, conv_dim, device=DEV).bfloat16()
    full = K.causal_conv1d_xbc(xs, w, b, H * P, G, N)[0]
    one = K.causal_conv1d_xbc(xs[:, 3:], w, b, H * P, G, N, halo=xs[:, :3].contiguous())[0]
    assert torch.equal(one, full[:, 3:])


@pytest.mark.parametrize("Bsz,L,H,P,G", [(1, 300, 16, 80, 2), (2, 129, 8, 64, 8), (1, 2300, 8, 80, 8), (1, 64, 4, 40, 1)])
def test_conv_xbc_with_cb_fragments(K, Bsz, L, H, P, G):
    """tv_causal_conv1d_xbc_cb_fwd: x, B, C bit-identical to the plain conv (with and without a shard halo), and the
    scan fed with its C.B^T fragments bit-identical to the scan that recomputes them in its pre-pass — same bf16
    operands, same MFMA order (the G_{l,s} = C_l . B_s of modeling_nano.py:800-811)."""
    N = 128
    g = torch.Generator().manual_seed(L + H)
    conv_dim = H * P + 2 * G * N
    xs = torch.randn(Bsz, L + 3, conv_dim, generator=g).bfloat16().to(DEV)
    w, b = torch.randn(conv_dim, 4, generator=g).bfloat16().to(DEV), torch.randn(conv_dim, generator=g).bfloat16().to(DEV)
    for halo in (None, xs[:, :3].contiguous()):
        xin = xs[:, 3:]
        x0, B0, C0 = K.causal_conv1d_xbc(xin, w, b, H * P, G, N, halo=halo)
        x1, B1, C1, cb = K.causal_conv1d_xbc(xin, w, b, H * P, G, N, halo=halo, return_cb=True)
        assert cb is not None and cb.dtype == torch.bfloat16
        assert torch.equal(x0, x1) and torch.equal(B0, B1) and torch.equal(C0, C1)
        assert B1.stride(1) == N and C1.stride(1) == N        # group-major storage
        dt = (torch.randn(Bsz, L, H, generator=g) * 0.5).bfloat16().to(DEV)
        A = -(torch.rand(H, generator=g) * 15 + 1).to(DEV)
        D, dtb = torch.ones(H, device=DEV), torch.full((H,), -2.0, device=DEV)
        kw = dict(chunk_size=64, D=D, dt_bias=dtb, dt_softplus=True, return_final_states=True)
        for impl in (3, 4, 6, 0):   # (6 = the head-per-wave march, which consumes the fragments unmasked; 0 = auto)
            if impl == 6 and P not in (32, 64, 80):
                continue
            K.ssd_scan_set_impl(impl)
            try:
                ya, fa = K.mamba_chunk_scan_combined(x0.view(Bsz, L, H, P), dt, A, B0, C0, **kw)
                yb, fb = K.mamba_chunk_scan_combined(x1.view(Bsz, L, H, P), dt, A, B1, C1, cb=cb, **kw)
            finally:
                K.ssd_scan_set_impl(0)
            assert torch.equal(ya, yb) and torch.equal(fa, fb), f"impl {impl}"
    # the fragments are refused for other shapes than the ones they were made for
    with pytest.raises(Exception):
        K.mamba_chunk_scan_combined(x0.view(Bsz, L, H, P), dt, A, B0, C0, cb=cb[:-512], **kw)
    # fp32 / other d_state: no fragments, plain path
    xf = torch.randn(1, 50, 8 * 16 + 2 * 2 * 16, device=DEV)
    out = K.causal_conv1d_xbc(xf, torch.randn(xf.shape[-1], 4, device=DEV), None, 8 * 16, 2, 16, return_cb=True)
    assert out[3] is None


# ---------------------------------------------------------------- ToMe (V3)
def test_tome_hip_matches_reference_golden(K):
    """csrc/tome.hip, fp32, against the reference's own ToMe output (tests/golden/tome.npz:
    729 -> 16 tokens in 6 rounds, and 4-frame clips of 100 tokens)."""
    from timeviper_amd.model.projector.tome import ToMe16_mlp_hd64
    g = load_golden("tome")
    proj = ToMe16_mlp_hd64(64, 48, num_compressed_tokens=16)
    proj.load_state_dict(golden_state_dict(g), strict=True)
    proj = proj.to(DEV).eval()
    x = torch.from_numpy(g["x"]).to(DEV)
    with torch.no_grad():
        merged = proj.merge_tokens(x, 16, "raw")
        y = proj(x, compress=True, local_num_frames=1)
        y2 = proj(torch.from_numpy(g["x2"]).to(DEV), compress=True, local_num_frames=4)
    close(merged, g["merged"], 1e-4, 1e-5, "merged tokens")
    close(y, g["y"], 1e-4, 1e-5, "projector output")
    close(y2, g["y2"], 1e-4, 1e-5, "4-frame clips")


@pytest.mark.parametrize("dtype,F_,T,C,heads", [(torch.bfloat16, 5, 729, 1152, 16), (torch.float32, 3, 257, 128, 16),
                                                (torch.bfloat16, 2, 1024, 1408, 16), (torch.float32, 4, 7, 64, 16)])
def test_tome_round_vs_torch_restatement(K, dtype, F_, T, C, heads):
    """one round against the oracle's step-by-step restatement of tome.py:14-83 (fp64 on the CPU;
    pinned by the reference golden in test_oracle_golden.py); sizes carried from a previous
    round; r up to half the tokens"""
    from oracle.vit import tome_merge_round_ref
    g = torch.Generator().manual_seed(T + C)
    x = torch.randn(F_, T, C, generator=g).to(dtype)
    size = torch.randint(1, 5, (F_, T, 1), generator=g).to(dtype)
    for r, sz in ((T // 2, None), (max(1, T // 5), size)):
        x_ref, s_ref = tome_merge_round_ref(x.double(), None if sz is None else sz.double(), r, heads)
        xo, so = K.tome_merge_round(x.to(DEV), None if sz is None else sz.to(DEV), r, heads)
        assert xo.shape == x_ref.shape and so.shape == s_ref.shape
        assert torch.equal(so.float().cpu(), s_ref.float()), "merged sizes differ (different matching)"
        close(xo, x_ref.float(), *TOL[dtype], f"r={r}")


# ---------------------------------------------------------------- Qwen2 operators
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_rope_and_silu_mul(K, dtype):
    g = torch.Generator().manual_seed(17)
    B, L, Hq, Hkv, D = 1, 77, 6, 2, 128
    qkv = torch.randn(B, L, (Hq + 2 * Hkv) * D, generator=g).to(dtype)        # q, k are column slices
    pos = torch.arange(5, 5 + L)[None]
    inv = 1.0 / (10000.0 ** (torch.arange(0, D, 2).float() / D))
    emb = torch.cat([pos[:, :, None].float() * inv] * 2, dim=-1)
    cos, sin = emb.cos().to(dtype), emb.sin().to(dtype)

    def rot(x):
        return torch.cat((-x[..., D // 2:], x[..., :D // 2]), dim=-1)
    q = qkv[..., :Hq * D].view(B, L, Hq, D)
    k = qkv[..., Hq * D:(Hq + Hkv) * D].view(B, L, Hkv, D)
    q_ref = q.float() * cos.float()[:, :, None] + rot(q.float()) * sin.float()[:, :, None]
    k_ref = k.float() * cos.float()[:, :, None] + rot(k.float()) * sin.float()[:, :, None]
    d = qkv.to(DEV)
    qd = d[..., :Hq * D].view(B, L, Hq, D)
    kd = d[..., Hq * D:(Hq + Hkv) * D].view(B, L, Hkv, D)
    K.apply_rotary_pos_emb_(qd, kd, cos.to(DEV), sin.to(DEV))
    close(qd, q_ref, *TOL[dtype], "rope q")
    close(kd, k_ref, *TOL[dtype], "rope k")
    assert torch.equal(d[..., (Hq + Hkv) * D:].cpu(), qkv[..., (Hq + Hkv) * D:]), "v must be untouched"
    gu = torch.randn(33, 2 * 18944 // 8, generator=g).to(dtype)
    gate, up = gu[:, :gu.shape[1] // 2], gu[:, gu.shape[1] // 2:]
    y = K.silu_mul(gate.to(DEV), up.to(DEV))
    close(y, torch.nn.functional.silu(gate.float()) * up.float(), *TOL[dtype], "silu_mul")


# ---------------------------------------------------------------- ViT linears with fused epilogues (csrc/gemm.hip)
@pytest.mark.parametrize("M,N,Kd", [(256, 256, 128), (512, 512, 256), (300, 260, 384), (1000, 1152, 1152),
                                    (729 * 3, 4352, 1152), (700, 1152, 4352), (1, 256, 128), (257, 4, 128), (5000, 1152, 640)])
@pytest.mark.parametrize("epi", [0, 1, 2])
def test_gemm_fused_epilogues(K, M, N, Kd, epi):
    """tv_gemm_bf16_fwd against an fp64 product of the same bf16 operands: plain bias, bias + exact GELU (applied to
    the bf16-rounded pre-activation, the rounding points of GEMM-then-tv_gelu_fwd) and accumulation into C; ragged M / N
    tiles, two K-tiles (tail only), the ViT's own shapes."""
    g = torch.Generator().manual_seed(M + N + Kd)
    a = (torch.randn(M, Kd, generator=g) * 0.5).bfloat16()
    w = (torch.randn(N, Kd, generator=g) * (1.0 / math.sqrt(Kd))).bfloat16()
    b = torch.randn(N, generator=g).bfloat16()
    c0 = torch.randn(M, N, generator=g).bfloat16()
    acc = a.double() @ w.double().t()
    if epi == 2:
        ref = acc + c0.double()
        out = K.linear_fused(a.to(DEV), w.to(DEV), None, epilogue=2, out=c0.to(DEV).clone())
    else:
        pre = acc + b.double()
        ref = torch.nn.functional.gelu(pre.float().bfloat16().double()) if epi == 1 else pre
        out = K.linear_fused(a.to(DEV), w.to(DEV), b.to(DEV) if M % 2 else b.float().to(DEV), epilogue=epi)
    assert out.shape == (M, N) and out.dtype == torch.bfloat16
    # bf16 output: half an ulp of the result + the fp32 accumulation error (+ one bf16 step of the pre-activation through
    # GELU's slope <= 1.13)
    close(out, ref, 2.0 ** -8 * (2.2 if epi == 1 else 1.0), 1e-2 if epi == 1 else 2e-3, f"gemm epi {epi}")


def test_gemm_fused_gelu_equals_gemm_then_gelu(K):
    """The fused fc1 + GELU keeps the two-pass path's rounding points: identical to tv_gemm_bf16_fwd (bias) followed by
    tv_gelu_fwd, bit for bit; strided input rows (a column slice of a wider tensor) and a strided output."""
    g = torch.Generator().manual_seed(3)
    wide = (torch.randn(900, 1152 + 64, generator=g) * 0.5).bfloat16().to(DEV)
    a = wide[:, 64:]
    w = (torch.randn(512, 1152, generator=g) * 0.03).bfloat16().to(DEV)
    b = torch.randn(512, generator=g).to(DEV)
    two = K.gelu(K.linear_fused(a, w, b, epilogue=0), inplace=True)
    outw = torch.zeros(900, 600, dtype=torch.bfloat16, device=DEV)
    one = K.linear_fused(a, w, b, epilogue=1, out=outw[:, :512])
    assert torch.equal(one, two) and float(outw[:, 512:].abs().max()) == 0.0
    ref = torch.nn.functional.gelu(torch.nn.functional.linear(a, w, b.bfloat16()))
    close(one, ref.float().cpu(), 2e-2, 2e-2, "vs torch (hipBLASLt + GELU)")


@pytest.mark.parametrize("M,N,Kd,grid", [(1024, 1024, 1152, 8), (2187, 4352, 1152, 8), (1500, 1160, 1152, 16),
                                         (1300, 1152, 4352, 8), (729 * 8, 3456, 1408, 64), (256, 256, 1152, 8),
                                         (4096, 1152, 256, 8)])
@pytest.mark.parametrize("epi", [0, 1, 2])
def test_gemm_persistent_kernel(K, M, N, Kd, grid, epi):
    """The persistent GEMM (csrc/gemm_persist.hip: tile epilogue inside the next tile's main loop) forced onto small grids so
    that every work-group walks several tiles, shifted edge tiles in M and N included: against the fp64 product, and
    bit-equal to the per-tile kernel for the bias epilogues.  (The accumulating epilogue has no 256 x 256 persistent form —
    it runs on the per-tile kernel whatever the setting: that case only re-checks the dispatch.)"""
    g = torch.Generator().manual_seed(M + N + Kd + epi)
    a = (torch.randn(M, Kd, generator=g) * 0.5).bfloat16().to(DEV)
    w = (torch.randn(N, Kd, generator=g) * (1.0 / math.sqrt(Kd))).bfloat16().to(DEV)
    b = torch.randn(N, generator=g).bfloat16()
    b = (b if M % 2 else b.float()).to(DEV)
    c0 = torch.randn(M, N, generator=g).bfloat16().to(DEV)
    acc = a.double().cpu() @ w.double().cpu().t()

    def run():
        if epi == 2:
            return K.linear_fused(a, w, None, epilogue=2, out=c0.clone())
        return K.linear_fused(a, w, b, epilogue=epi)
    try:
        K.gemm_set_drip(0)                # (the 256 x 192 kernel has its own test below)
        K.gemm_set_persist(1, grid)
        out = run()
        torch.cuda.synchronize()
        K.gemm_set_persist(0, 0)
        tile = run()
    finally:
        K.gemm_set_persist(-1, 0)
        K.gemm_set_drip(-1)
    if epi == 2:
        ref = acc + c0.double().cpu()
    else:
        pre = acc + b.double().cpu()
        ref = torch.nn.functional.gelu(pre.float().bfloat16().double()) if epi == 1 else pre
    close(out, ref, 2.0 ** -8 * (2.2 if epi == 1 else 1.0), 1e-2 if epi == 1 else 2e-3, f"persistent gemm epi {epi}")
    if epi != 2:
        assert torch.equal(out, tile), "persistent and per-tile kernel differ"
    else:
        close(out, tile.float().cpu(), 2.0 ** -7, 2e-3, "persistent vs per-tile accumulate")


def test_gemm_persistent_repeated_runs_are_identical(K):
    """Race screen for the counted waits: 20 launches of each epilogue on a 64-work-group grid give the same bits."""
    g = torch.Generator().manual_seed(11)
    M, N, Kd = 729 * 16, 1152, 1152
    a = (torch.randn(M, Kd, generator=g) * 0.5).bfloat16().to(DEV)
    w = (torch.randn(N, Kd, generator=g) * 0.03).bfloat16().to(DEV)
    b = torch.randn(N, generator=g).to(DEV)
    c0 = torch.randn(M, N, generator=g).bfloat16().to(DEV)
    try:
        K.gemm_set_persist(1, 64)
        for drip in (0, 1):               # the 256 x 256 persistent kernel, then the 256 x 192 one (csrc/gemm_drip.hip)
            K.gemm_set_drip(drip)
            for epi in (0, 1, 2):
                outs = []
                for _ in range(20):
                    outs.append(K.linear_fused(a, w, None, epilogue=2, out=c0.clone()) if epi == 2
                                else K.linear_fused(a, w, b, epilogue=epi))
                torch.cuda.synchronize()
                for o in outs[1:]:
                    assert torch.equal(o, outs[0]), f"drip {drip} epilogue {epi}: two launches differ"
    finally:
        K.gemm_set_persist(-1, 0)
        K.gemm_set_drip(-1)


@pytest.mark.parametrize("M,N,Kd,grid", [(1024, 1152, 1152, 8), (2187, 4352, 1152, 8), (1500, 1160, 1152, 16),
                                         (1300, 1152, 4352, 8), (729 * 8, 3456, 1408, 64), (256, 192, 1152, 8),
                                         (729 * 16, 1152, 1152, 64)])
@pytest.mark.parametrize("epi", [0, 1, 2])
def test_gemm_drip_kernel(K, M, N, Kd, grid, epi):
    """The 256 x 192 persistent GEMM (csrc/gemm_drip.hip: the finished tile leaves during the next tile's K loop, half of
    it parked in LDS and half in accumulator registers; old C by LDS-DMA into the staging rows; the bias as the
    accumulators' start value) on small grids so that every work-group walks several tiles, shifted edge tiles in M and N
    included: against the fp64 product, and against the per-tile kernel — identical for the accumulating epilogue (same
    order of additions), within one bf16 rounding for the bias epilogues (the bias enters before the products instead of
    after them: a different fp32 rounding order, which flips the final rounding of a few elements in 10 000)."""
    g = torch.Generator().manual_seed(M + N + Kd + epi)
    a = (torch.randn(M, Kd, generator=g) * 0.5).bfloat16().to(DEV)
    w = (torch.randn(N, Kd, generator=g) * (1.0 / math.sqrt(Kd))).bfloat16().to(DEV)
    b = torch.randn(N, generator=g).bfloat16().float().to(DEV)
    c0 = torch.randn(M, N, generator=g).bfloat16().to(DEV)
    acc = a.double().cpu() @ w.double().cpu().t()

    def run():
        if epi == 2:
            return K.linear_fused(a, w, None, epilogue=2, out=c0.clone())
        return K.linear_fused(a, w, b, epilogue=epi)
    try:
        K.gemm_set_persist(1, grid)
        K.gemm_set_drip(1)
        out = run()
        torch.cuda.synchronize()
        K.gemm_set_drip(0)
        K.gemm_set_persist(0, 0)
        tile = run()
    finally:
        K.gemm_set_persist(-1, 0)
        K.gemm_set_drip(-1)
    if epi == 2:
        ref = acc + c0.double().cpu()
    else:
        pre = acc + b.double().cpu()
        ref = torch.nn.functional.gelu(pre.float().bfloat16().double()) if epi == 1 else pre
    close(out, ref, 2.0 ** -8 * (2.2 if epi == 1 else 1.0), 1e-2 if epi == 1 else 2e-3, f"drip gemm epi {epi}")
    if epi == 2:
        assert torch.equal(out, tile), "256 x 192 and per-tile kernel differ (accumulating epilogue)"
    else:
        diff = (out.float() - tile.float()).abs()
        frac = float((diff > 0).float().mean())
        assert frac < 2e-3, f"{frac:.2e} of the elements differ from the per-tile kernel"
        # one bf16 step of the larger of the two (GELU: a step of the pre-activation through a slope <= 1.13, then the
        # output's own rounding)
        lim = torch.maximum(out.float().abs(), tile.float().abs()) * 2.0 ** -7 * (2.3 if epi == 1 else 1.0) + 1e-3
        assert bool((diff <= lim).all()), "more than one bf16 rounding step from the per-tile kernel"


# ---------------------------------------------------------------- ragged / padded batches (flash_attention_class.py:59-91)
def test_flash_attn_varlen_ragged_and_key_padding_mask(K):
    """flash_attn_varlen_qkvpacked_func on a ragged batch (runs of equal and unequal lengths, an empty sequence) against the
    oracle sequence by sequence, and the FlashAttention module's key_padding_mask path (unpad -> kernel -> pad with
    zeros) against the same."""
    from timeviper_amd.model.vit.internvideo2 import FlashAttention
    g = torch.Generator().manual_seed(4)
    H, D = 4, 88
    lens = [257, 257, 100, 0, 33, 33, 33, 300]
    cu = torch.tensor([0] + list(np.cumsum(lens)), dtype=torch.int32)
    qkv = torch.randn(int(cu[-1]), 3, H, D, generator=g).bfloat16()
    out = K.flash_attn_varlen_qkvpacked_func(qkv.to(DEV), cu.to(DEV), max(lens))
    assert out.shape == (int(cu[-1]), H, D)
    for i, n in enumerate(lens):
        if n == 0:
            continue
        x = qkv[int(cu[i]):int(cu[i + 1])].float()[None]
        ref, _ = R.attention_ref(x[:, :, 0], x[:, :, 1], x[:, :, 2], False)
        close(out[int(cu[i]):int(cu[i + 1])], ref[0], 2e-2, 1e-2, f"sequence {i}")
        assert_rows_close(out[int(cu[i]):int(cu[i + 1])], ref[0], torch.bfloat16, f"varlen ragged, sequence {i} of {n}")
    # padded batch: (B, S) mask with holes in the middle and at the ends
    B, S = 3, 120
    mask = torch.rand(B, S, generator=g) > 0.3
    mask[1, :10] = False
    mask[2, 100:] = False
    x = torch.randn(B, S, 3, H, D, generator=g).bfloat16()
    o, _ = FlashAttention()(x.to(DEV), key_padding_mask=mask.to(DEV))
    assert o.shape == (B, S, H, D)
    for b in range(B):
        keep = mask[b].nonzero().flatten()
        xb = x[b, keep].float()[None]
        ref, _ = R.attention_ref(xb[:, :, 0], xb[:, :, 1], xb[:, :, 2], False)
        close(o[b, keep], ref[0], 2e-2, 1e-2, f"batch {b}")
        assert_rows_close(o[b, keep], ref[0], torch.bfloat16, f"key_padding_mask, batch {b}")
        assert float(o[b, ~mask[b]].abs().max()) == 0.0
    # already unpadded input through the module, causal
    o2, _ = FlashAttention()(qkv.to(DEV), cu_seqlens=cu.to(DEV), max_s=max(lens), causal=True)
    x0 = qkv[:257].float()[None]
    ref, _ = R.attention_ref(x0[:, :, 0], x0[:, :, 1], x0[:, :, 2], True)
    close(o2[:257], ref[0], 2e-2, 1e-2, "causal, first sequence")
    assert_rows_close(o2[:257], ref[0], torch.bfloat16, "varlen causal, first sequence")
