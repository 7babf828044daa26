"""CPU-side checks of tv_linear_rows_bf16_fwd (the few-token linear layers): the symbol, its binding, its argument checks
(made before any HIP call, so they need no device; tv_gemv_bf16_fwd makes them by the same code, csrc/linear_prologue.hpp,
and is asked the same way), the wrapper's shape predicate, and the code objects' scratch use."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest
import torch

from timeviper_amd import build

ROOT = Path(__file__).resolve().parent.parent
LLVM = Path("/opt/rocm/lib/llvm/bin")
needs_tools = pytest.mark.skipif(not (LLVM / "llvm-objdump").exists() or not (LLVM / "llvm-readelf").exists(),
                                 reason="ROCm LLVM tools not found")
NAME = "tv_linear_rows_bf16_fwd"
P = 0x10000            # a 16-byte aligned address that is never dereferenced: the checks come before the launch
F32, BF16 = 0, 1


def call(lib, M=2, N=32, K=64, xs=None, ldw=None, ys=None, pro=0, nw=None, nw_dt=F32, group=0, x=P, W=P, y=P):
    return lib.tv_linear_rows_bf16_fwd(x, W, None, y, M, N, K, K if xs is None else xs, K if ldw is None else ldw,
                                       N if ys is None else ys, pro, None, 0, None, 0, nw, nw_dt, 1e-5, None, 0, group, None)


def test_symbol_is_declared_bound_and_exported():
    from timeviper_amd import _capi
    build.build()
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "timeviper_hip.h").read_text(), flags=re.S)
    decl = re.search(r"int\s+" + NAME + r"\s*\(([^;]*)\)\s*;", header)
    assert decl, "not declared in include/timeviper_hip.h"
    assert NAME in _capi.SIGNATURES
    assert len(_capi.SIGNATURES[NAME][1]) == len(decl.group(1).split(",")) == 22
    lib = _capi.lib()
    assert hasattr(lib, NAME)
    assert lib.tv_abi_version() == _capi.ABI_VERSION == 13


@pytest.mark.parametrize("kw,status", [
    (dict(M=0), -1),
    (dict(M=17), -1),
    (dict(K=12), -2),
    (dict(pro=1), -1),                       # rmsnorm prologue without a norm weight
    (dict(pro=3, group=32), -1),             # gated prologue without a norm weight
    (dict(pro=3, nw=P, group=24), -1),       # 24 does not divide 64
    (dict(pro=3, nw=P, group=0), -1),
    (dict(x=None), -1),
    (dict(x=P + 2), -2),                     # misaligned x
    (dict(ldw=68), -2),
    (dict(pro=1, nw=P, K=8200), -2),         # rmsnorm rows of <= 8192 channels
    (dict(pro=7), -1),
    (dict(ys=16), -1),                       # rows of y closer than N
    (dict(xs=32), -1),
])
def test_argument_errors_are_returned_without_a_device(kw, status):
    from timeviper_amd import _capi
    lib = _capi.lib()
    assert call(lib, **kw) == status, (kw, lib.tv_last_error())
    assert b"linear_rows" in lib.tv_last_error()


def call_gemv(lib, M=2, N=32, K=64, xs=None, ldw=None, ys=None, pro=0, nw=None, nw_dt=F32, group=0, x=P, W=P, y=P, delta=None,
              sum_out=None):
    return lib.tv_gemv_bf16_fwd(x, W, None, y, M, N, K, K if xs is None else xs, K if ldw is None else ldw,
                                N if ys is None else ys, pro, delta, K, sum_out, K, nw, nw_dt, 1e-5, None, 0, group,
                                None, None, None, 0, 0, None)


@pytest.mark.parametrize("kw,status", [
    (dict(M=0), -1),
    (dict(M=5), -1),
    (dict(K=12), -2),
    (dict(pro=1), -1),                       # rmsnorm prologue without a norm weight
    (dict(pro=3, group=32), -1),             # gated prologue without a norm weight
    (dict(pro=3, nw=P, group=24), -1),       # 24 does not divide 64
    (dict(x=None), -1),
    (dict(x=P + 2), -2),                     # misaligned x
    (dict(ldw=68), -2),
    (dict(pro=1, nw=P, K=8200), -2),         # rmsnorm rows of <= 8192 channels
    (dict(M=4, K=16392, N=8), -2),           # f(x) past the 128 KiB of LDS
    (dict(pro=7), -1),
    # the checks the two kernels share since linear_prologue.hpp: overlapping rows, the sum written over an operand
    (dict(xs=32), -1),
    (dict(ys=16), -1),
    (dict(ldw=32), -1),
    (dict(pro=1, nw=P, sum_out=P), -1),      # sum_out == x
    (dict(pro=1, nw=P, delta=2 * P, sum_out=2 * P), -1),
])
def test_gemv_argument_errors_are_returned_without_a_device(kw, status):
    """tv_gemv_bf16_fwd makes the same checks, by the same code, in front of any HIP call"""
    from timeviper_amd import _capi
    lib = _capi.lib()
    assert call_gemv(lib, **kw) == status, (kw, lib.tv_last_error())
    assert lib.tv_last_error().startswith(b"gemv:")


def test_copies_of_strided_operands_outlive_the_helper(monkeypatch):
    """A delta / gate whose inner stride is not 1 is copied to dense rows: the pointers handed to the C call must belong to
    tensors the wrapper still holds when it launches (a freed copy's block may be handed to the output)."""
    from timeviper_amd import kernels as K
    monkeypatch.setattr(K, "_gpu", lambda *ts: None)
    x = torch.zeros(1, 3, 64, dtype=torch.bfloat16)
    W = torch.zeros(32, 64, dtype=torch.bfloat16)
    wide = torch.ones(1, 3, 128, dtype=torch.bfloat16)
    for kw in (dict(delta=wide[..., ::2], sum_out=torch.empty_like(x), gate=None), dict(delta=None, sum_out=None, gate=wide[..., ::2])):
        x2, args, held = K._linear_operands("t", x, W, None, kw["delta"], kw["sum_out"], None, 1e-5, kw["gate"], 32)
        d2, s2, g2 = held
        assert args[0] == (None if d2 is None else d2.data_ptr()) and args[2] == (None if s2 is None else s2.data_ptr())
        assert args[7] == (None if g2 is None else g2.data_ptr())
        for t, src in ((d2, kw["delta"]), (g2, kw["gate"])):
            if src is not None:
                assert t.stride() == (64, 1) and t.data_ptr() != src.data_ptr() and torch.equal(t, src.reshape(3, 64))
        assert s2 is None or s2.data_ptr() == kw["sum_out"].data_ptr()


def test_takes_predicate():
    from timeviper_amd import kernels as K
    W = torch.zeros(32, 64, dtype=torch.bfloat16, device="meta")
    x = lambda *s, dt=torch.bfloat16: torch.zeros(*s, dtype=dt, device="meta")
    assert not K.linear_rows_takes(x(1, 5, 64), W)         # not a CUDA tensor

    class Cuda:        # the shape / dtype part of the predicate, without a device
        def __init__(self, t): self.t = t
        is_cuda = True
        def data_ptr(self): return 0x10000 + 2 * self.t.storage_offset()
        def __getattr__(self, n): return getattr(self.t, n)
    ok = lambda a, w=W: K.linear_rows_takes(Cuda(a), w)
    assert ok(x(1, 5, 64)) and ok(x(16, 64)) and ok(x(1, 1, 64))
    assert not ok(x(1, 17, 64)) and not ok(x(17, 64))
    assert not ok(x(1, 5, 64, dt=torch.float32))
    assert not ok(x(2, 5, 64))
    assert not ok(x(1, 5, 64), torch.zeros(32, 64, dtype=torch.float32, device="meta"))
    assert not ok(x(1, 5, 60), torch.zeros(32, 60, dtype=torch.bfloat16, device="meta"))
    assert not ok(x(1, 5, 128)[..., ::2])
    assert not ok(x(1, 5, 72)[..., 4:68])                  # rows that do not start on 16 bytes
    assert K.GEMV_NONE == 0 and K.GEMV_GATED == 3


def kernel_metadata(src_name: str, tmp_path: Path) -> dict:
    """{mangled kernel name: {private_segment_fixed_size, vgpr_spill_count, ...}} of lib/obj/<src>.o
    (tests/test_build_cpu.py's helper)"""
    build.ensure_built()
    obj = build.OBJ / (src_name + ".o")
    work = tmp_path / src_name
    work.mkdir()
    shutil.copy(obj, work / obj.name)                      # llvm-objdump --offloading writes next to its input
    subprocess.run([str(LLVM / "llvm-objdump"), "--offloading", obj.name], cwd=work, check=True, capture_output=True)
    dev = [p for p in work.iterdir() if "amdgcn" in p.name]
    assert len(dev) == 1, [p.name for p in work.iterdir()]
    notes = subprocess.run([str(LLVM / "llvm-readelf"), "--notes", dev[0].name], cwd=work, check=True,
                           capture_output=True, text=True).stdout
    out = {}
    for b in re.split(r"\n\s*- \.agpr_count:", notes)[1:]:
        name = re.search(r"\.name:\s*(_Z\S+)", b)
        if not name:
            continue
        d = out.setdefault(name.group(1), {})
        for key in ("private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count", "vgpr_count"):
            m = re.search(r"\." + key + r":\s*(\d+)", b)
            if m:
                d[key] = int(m.group(1))
    return out


@needs_tools
def test_linear_rows_kernels_use_no_scratch(tmp_path):
    """Every instantiation (3 prologues x 4 tile / step shapes + the gated prologue x 2) keeps its accumulators and its two
    batches of W in registers: a spill would put scratch traffic into the stream of weight loads."""
    md = kernel_metadata("linear_rows.hip", tmp_path)
    kernels = {k: v for k, v in md.items() if "linear_rows_kernel" in k}
    assert len(kernels) == 14, list(md)
    for k, v in kernels.items():
        assert v.get("private_segment_fixed_size") == 0 and v.get("vgpr_spill_count", 0) == 0, (k, v)
        assert v.get("vgpr_count", 0) <= 256, (k, v)       # two work-groups a CU: two waves a SIMD
