"""CPU-side checks of tv_gemv_fp8w_fwd (the decode step's products on e4m3 weights): the symbol and its binding, the
argument checks (made before any HIP call, so they need no device), the wrapper's shape predicate, and the code objects'
scratch use."""
import re

import pytest
import torch

from test_linear_rows_cpu import ROOT, kernel_metadata, needs_tools
from timeviper_amd import build

NAME = "tv_gemv_fp8w_fwd"
P = 0x10000            # a 16-byte aligned address that is never dereferenced: the checks come before the launch
F32 = 0


def call(lib, M=2, N=32, K=64, xs=None, ldw=None, ys=None, pro=0, nw=None, group=0, x=P, W=P, scale=P, y=P, conv=None):
    return lib.tv_gemv_fp8w_fwd(x, W, scale, None, y, M, N, K, K if xs is None else xs, K if ldw is None else ldw,
                                N if ys is None else ys, pro, None, K, None, K, nw, F32, 1e-5, None, 0, group,
                                conv, conv, None, 0, 8 if conv else 0, None)


def test_symbol_is_declared_bound_and_exported():
    from timeviper_amd import _capi
    build.build()
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "timeviper_hip.h").read_text(), flags=re.S)
    decl = re.search(r"int\s+" + NAME + r"\s*\(([^;]*)\)\s*;", header)
    bf16 = re.search(r"int\s+tv_gemv_bf16_fwd\s*\(([^;]*)\)\s*;", header)
    assert decl and bf16
    # tv_gemv_bf16_fwd's argument list and one more pointer
    assert len(_capi.SIGNATURES[NAME][1]) == len(decl.group(1).split(",")) == len(bf16.group(1).split(",")) + 1 == 28
    lib = _capi.lib()
    assert hasattr(lib, NAME) and hasattr(lib, "tv_gemv_fp8w_calls")
    assert lib.tv_abi_version() == _capi.ABI_VERSION == 13           # additive: no bump


@pytest.mark.parametrize("kw,status", [
    (dict(M=0), -1),
    (dict(M=5), -1),
    (dict(K=24), -2),                        # K % 16
    (dict(ldw=72), -2),                      # ldw % 16
    (dict(W=P + 8), -2),                     # misaligned W
    (dict(scale=None), -1),
    (dict(scale=P + 2), -2),
    (dict(x=P + 2), -2),
    (dict(ldw=32), -1),                      # rows of W that overlap
    (dict(pro=1), -1),                       # rmsnorm prologue without a norm weight
    (dict(pro=1, nw=P, K=8208), -2),         # rmsnorm rows of <= 8192 channels
    (dict(pro=3, nw=P, group=24), -1),       # 24 does not divide 64
    (dict(M=4, K=16400, N=8), -2),           # f(x) past the 128 KiB of LDS
    (dict(M=1, K=8192, N=8, conv=P), -2),    # the conv epilogue lives in the row-per-wave kernel
    (dict(pro=7), -1),
])
def test_argument_errors_are_returned_without_a_device(kw, status):
    from timeviper_amd import _capi
    lib = _capi.lib()
    calls = lib.tv_gemv_fp8w_calls()
    assert call(lib, **kw) == status, (kw, lib.tv_last_error())
    assert lib.tv_last_error().startswith(b"gemv_fp8w:")
    assert lib.tv_gemv_fp8w_calls() == calls                # no launch


def test_takes_predicate(monkeypatch):
    from timeviper_amd import kernels as K
    x = lambda *s: torch.zeros(*s, dtype=torch.bfloat16, device="meta")
    w = lambda n, k, dt=torch.float8_e4m3fn: torch.zeros(n, k, dtype=dt, device="meta")
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))    # (shapes and dtypes only: nothing runs)
    assert K.gemv_fp8w_takes(x(1, 1, 64), w(32, 64)) and K.gemv_fp8w_takes(x(4, 1, 64), w(32, 64))
    assert not K.gemv_fp8w_takes(x(5, 1, 64), w(32, 64))
    assert not K.gemv_fp8w_takes(x(1, 1, 72), w(32, 72))                          # K % 16
    assert not K.gemv_fp8w_takes(x(1, 1, 64), w(32, 64, torch.bfloat16))
    assert K.gemv_fp8w_takes(x(1, 1, 64), w(32, 80)[:, :64])                      # rows 80 bytes apart
    assert not K.gemv_fp8w_takes(x(1, 1, 64), w(32, 72)[:, :64])                  # rows 72 bytes apart
    assert not K.gemv_fp8w_takes(x(1, 1, 64), w(64, 32).t())                      # a transposed view
    assert not K.gemv_fp8w_takes(x(4, 1, 16400), w(8, 16400))                     # past the LDS
    assert not K.gemv_takes(x(1, 1, 64), w(32, 64))                               # the bf16 kernel takes no e4m3


@needs_tools
def test_kernels_use_no_scratch(tmp_path):
    """Every instantiation (4 prologues x {1, up to 4} rows of x x {non-temporal, plain} loads x {split-K, 2 or 4 rows a
    wave}) keeps its batches of Q, the converted pairs and its accumulators in registers."""
    md = kernel_metadata("gemv_fp8w.hip", tmp_path)
    kernels = {k: v for k, v in md.items() if "gemv_fp8w" in k}
    assert len(kernels) == 48, list(md)
    for k, v in kernels.items():
        assert v.get("private_segment_fixed_size") == 0 and v.get("vgpr_spill_count", 0) == 0, (k, v)
        assert v.get("vgpr_count", 0) <= 256, (k, v)       # two work-groups a CU: two waves a SIMD
