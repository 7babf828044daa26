"""TEST INFRASTRUCTURE for sampled decoding: the sampler's contract (include/timeviper_hip.h) in numpy — s and
d in float32 exactly as specified, exp and every mass in float64 —, a numpy Philox4x32-10, the reference's own top-p margin,
and a stand-in for `kernels.sample_logits` for the CPU tests of the host logic.  Never imported by the product."""
import contextlib

import numpy as np
import torch

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_LO = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon et al., SC'11; Random123).  counter: 4 words, key: 2 words, each a Python int or an array of
    them; returns the 4 output words as uint32 arrays of the broadcast shape."""
    c = [np.asarray(x, dtype=np.uint64) & _LO for x in counter]
    k = [np.asarray(x, dtype=np.uint64) & _LO for x in key]
    for r in range(10):
        p0, p1 = _M0 * c[0], _M1 * c[2]                       # 32 x 32 -> 64 bits: exact in uint64
        c = [(p1 >> _S32) ^ c[1] ^ k[0], p1 & _LO, (p0 >> _S32) ^ c[3] ^ k[1], p0 & _LO]
        k = [(k[0] + np.uint64(_W0)) & _LO, (k[1] + np.uint64(_W1)) & _LO]
    return [x.astype(np.uint32) for x in c]


def random_word(seed: int, draw: int, stream: int) -> int:
    seed, draw = int(seed) & (2 ** 64 - 1), int(draw) & (2 ** 64 - 1)
    out = philox4x32_10((draw & 0xFFFFFFFF, draw >> 32, int(stream) & 0xFFFFFFFF, 0), (seed & 0xFFFFFFFF, seed >> 32))
    return int(out[0])


def reference(z, temperature=1.0, top_k=0, top_p=1.0):
    """The kept set of one row: dict with s (float32), w (float64 weights), keep (bool mask), n_kept, t (the smallest kept
    s, float32), t_bits, W (mass after top-k), W_kept, margin (the reference's own top-p margin, inf with top-p off)."""
    z = np.asarray(z, dtype=np.float32)
    V = z.shape[0]
    inv_t = np.float32(1.0 / float(temperature))              # formed in double, rounded once
    s = (z * inv_t + np.float32(0.0)).astype(np.float32)      # one fp32 multiply; -0 -> +0
    m = s.max()
    d = (s - m).astype(np.float32)
    w = np.exp(d.astype(np.float64))
    keep = np.ones(V, dtype=bool)
    if 0 < int(top_k) < V:
        t_k = np.partition(s, V - int(top_k))[V - int(top_k)]  # the k-th largest, counting multiplicity
        keep = s >= t_k                                        # ties at the threshold are all kept
    W = float(w[keep].sum())
    margin = float("inf")
    p = float(np.float32(min(float(top_p), 1.0)))             # the C ABI takes a float
    if p < 1.0:
        vals, inv = np.unique(s[keep], return_inverse=True)    # ascending distinct values
        mass = np.bincount(inv, weights=w[keep], minlength=vals.shape[0])[::-1]       # descending order of value
        above = np.concatenate([[0.0], np.cumsum(mass)[:-1]])  # M_>(v): mass of the kept tokens with s > v
        kept_vals = above < p * W                              # monotone: a prefix of the descending values
        j = int(kept_vals.sum()) - 1                           # the last value kept; the top one always is
        t_p = vals[::-1][j]
        margin = min(p * W - above[j], above[j] + mass[j] - p * W) / W
        keep = keep & (s >= t_p)
    t = s[keep].min()
    return {"s": s, "w": w, "keep": keep, "n_kept": int(keep.sum()), "t": t,
            "t_bits": int(np.float32(t).view(np.uint32)), "W": W, "W_kept": float(w[keep].sum()), "margin": margin}


def reference_margin(z, temperature=1.0, top_k=0, top_p=1.0) -> float:
    """min(top_p W - M_>(t), M_>=(t) - top_p W) / W: how far, relative to the kept mass, the reference's own top-p decision
    is from flipping.  A kernel whose masses are off by less than this keeps exactly the reference's set."""
    return reference(z, temperature, top_k, top_p)["margin"]


def cdf(ref):
    """float64 inclusive CDF over the kept set in index order (0 increments at tokens not kept)"""
    return np.cumsum(np.where(ref["keep"], ref["w"], 0.0)) / ref["W_kept"]


def sample(z, seed, draw, stream, temperature=1.0, top_k=0, top_p=1.0):
    """-> (id, n_kept, t_bits, u32) of one row, by the contract"""
    ref = reference(z, temperature, top_k, top_p)
    u = random_word(seed, draw, stream)
    F = cdf(ref)
    i = int(np.searchsorted(F, u / 2.0 ** 32, side="right"))   # the smallest i with F_i > u / 2^32
    i = min(i, int(np.flatnonzero(ref["keep"])[-1]))
    return i, ref["n_kept"], ref["t_bits"], u


SAMPLE_CALLS = []     # (draws, streams, seed, temperature, top_k, top_p) of every stand-in call


def sample_logits_cpu(logits, draws, streams, seed, temperature=1.0, top_k=0, top_p=1.0, out=None, diag=None):
    """stand-in for kernels.sample_logits on CPU tensors"""
    assert logits.dim() == 2 and logits.dtype == torch.float32
    assert draws.dtype == torch.int64 and streams.dtype == torch.int32
    SAMPLE_CALLS.append((draws.tolist(), streams.tolist(), int(seed), float(temperature), int(top_k), float(top_p)))
    res = [sample(logits[b].numpy(), seed, int(draws[b]), int(streams[b]), temperature, top_k, top_p)
           for b in range(logits.shape[0])]
    ids = torch.tensor([r[0] for r in res], dtype=torch.int64)
    if diag is not None:
        diag.copy_(torch.tensor([[r[1], r[2] - (1 << 32) if r[2] >> 31 else r[2], r[3] - (1 << 32) if r[3] >> 31 else r[3],
                                  0] for r in res], dtype=torch.int32))
    if out is not None:
        out.copy_(ids)
        return out
    return ids


@contextlib.contextmanager
def sampling_kernels_cpu():
    """`tests/test_branch_cpu.py`'s stand-ins (on top of cpu_kernel_shim.cpu_kernels()) plus the sampler's"""
    from test_branch_cpu import kernels_cpu
    from timeviper_amd import kernels as K
    with kernels_cpu():
        saved = K.sample_logits
        K.sample_logits = sample_logits_cpu
        try:
            yield
        finally:
            K.sample_logits = saved
