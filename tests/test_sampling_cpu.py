"""Sampled decoding — what can be checked without a GPU: the Philox4x32-10 of the test reference against known answers,
the C ABI of `tv_sample_logits_fwd`, and the host logic of `generate(do_sample=True)` / `generate_branches(do_sample=True)`
on the toy hybrid of tests/test_branch_cpu.py (fp32, lm_head x 20) with `sampling_ref.sample_logits_cpu` standing in for
the kernel: both sides of every equality run the same arithmetic, ids are compared exactly."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import sampling_ref as SR
from sampling_ref import sampling_kernels_cpu
from test_branch_cpu import _parent, _questions

ROOT = Path(__file__).resolve().parent.parent
HOT = 20.0          # a temperature that undoes the lm_head x 20 spread of the toy model: a flat enough distribution


# ------------------------------------------------------------------------------------------------ Philox
@pytest.mark.parametrize("counter, key, want", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(counter, key, want):
    got = SR.philox4x32_10(counter, key)
    assert " ".join(f"{int(x):08x}" for x in got) == want


def test_random_word_uses_draw_stream_and_seed():
    base = SR.random_word(7, 3, 1)
    assert base == int(SR.philox4x32_10((3, 0, 1, 0), (7, 0))[0])
    assert SR.random_word(7 + (5 << 32), (1 << 32) + 5, 2) == int(SR.philox4x32_10((5, 1, 2, 0), (7, 5))[0])
    assert len({base, SR.random_word(8, 3, 1), SR.random_word(7, 4, 1), SR.random_word(7, 3, 2)}) == 4


# ------------------------------------------------------------------------------------------------ the reference itself
def test_reference_rules_on_a_row_with_ties():
    z = np.array([1.0, 3.0, 2.0, 3.0, 2.0, 0.0, 2.0, -1.0], dtype=np.float32)
    r = SR.reference(z, 1.0, top_k=3)                          # the 3rd largest is 2.0: all three 2.0s are kept
    assert r["n_kept"] == 5 and r["t"] == 2.0
    r = SR.reference(z, 1.0, top_k=1)
    assert r["n_kept"] == 2 and r["t"] == 3.0                  # both maxima
    w = np.exp(z.astype(np.float64) - 3.0)
    p = float(2 * w[1] / w.sum()) + 1e-3                       # just above the mass of the two 3.0s: the 2.0s come in, whole
    r = SR.reference(z, 1.0, top_p=p)
    assert r["n_kept"] == 5 and r["t"] == 2.0 and 0 < r["margin"] < 2e-3
    r = SR.reference(z, 1.0, top_p=1e-6)                       # the top token (its whole tie group) is always kept
    assert r["n_kept"] == 2
    r = SR.reference(z, 1.0)
    assert r["n_kept"] == 8 and r["t"] == -1.0 and r["margin"] == float("inf")
    # the draw: u / 2^32 against the CDF over the kept set in index order
    i, n, tb, u = SR.sample(z, seed=1, draw=0, stream=0, top_k=1)
    assert i == (1 if u / 2.0 ** 32 < 0.5 else 3) and n == 2 and tb == int(np.float32(3.0).view(np.uint32))


# ------------------------------------------------------------------------------------------------ C ABI
def test_c_abi_declares_the_sampler():
    from timeviper_amd import _capi, build
    from timeviper_amd import kernels as K
    build.build()
    lib = _capi.lib()
    hdr = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "timeviper_hip.h").read_text(), flags=re.S)
    ctype = {"void*": _capi._p, "const void*": _capi._p, "int": _capi._i, "int64_t": _capi._l, "float": _capi._f}
    m = re.search(r"int tv_sample_logits_fwd\((.*?)\);", hdr, flags=re.S)
    assert m, "tv_sample_logits_fwd is not declared in the header"
    want = [ctype[p.strip().rsplit(" ", 1)[0].strip()] for p in m.group(1).split(",")]
    res, args = _capi.SIGNATURES["tv_sample_logits_fwd"]
    assert res is _capi._i and args == want
    assert hasattr(lib, "tv_sample_logits_fwd") and callable(K.sample_logits)
    assert lib.tv_abi_version() == _capi.ABI_VERSION == 13           # additive: no bump

    def call(logits=16, out=16, draws=16, streams=16, B=1, V=64, inv_t=1.0, top_k=0, top_p=1.0):
        return lib.tv_sample_logits_fwd(logits, out, draws, streams, None, B, V, V, 0, inv_t, top_k, top_p, None)
    # bad arguments are refused before any launch (no GPU here: a launch would fail with another status)
    assert call(logits=None) == -1 and b"null" in lib.tv_last_error()
    assert call(out=None) == -1 and call(draws=None) == -1 and call(streams=None) == -1
    assert call(V=0) == -1 and call(B=0) == -1
    assert call(top_p=0.0) == -1 and b"top_p" in lib.tv_last_error()
    assert call(inv_t=0.0) == -1 and call(inv_t=-1.0) == -1 and call(inv_t=float("inf")) == -1
    assert call(top_k=-1) == -1
    assert call(V=2 ** 18 + 1) == -2 and b"2^18" in lib.tv_last_error()


def test_sample_logits_has_no_cpu_path():
    from timeviper_amd import kernels as K
    from timeviper_amd._capi import TimeViperHipError
    with pytest.raises(TimeViperHipError):
        K.sample_logits(torch.zeros(1, 8), torch.zeros(1, dtype=torch.int64), torch.zeros(1, dtype=torch.int32), seed=0)


# ------------------------------------------------------------------------------------------------ generate
KW = dict(max_new_tokens=7, return_ids=True, eos_token_id=-1)


def _gen(vlm, cache, q, **kw):
    return vlm.generate(q, past_key_values=cache.clone(), **KW, **kw)[0].tolist()


def test_top_k_1_and_temperature_0_are_greedy():
    vlm, cache = _parent("M*-M*-")
    q = _questions(2)[1]
    with sampling_kernels_cpu():
        greedy = _gen(vlm, cache, q)
        SR.SAMPLE_CALLS.clear()
        assert _gen(vlm, cache, q, do_sample=True, top_k=1, seed=3) == greedy
        assert len(SR.SAMPLE_CALLS) >= 7
        SR.SAMPLE_CALLS.clear()
        assert _gen(vlm, cache, q, do_sample=True, temperature=0, seed=3) == greedy
        assert _gen(vlm, cache, q, do_sample=True, temperature=0) == greedy        # greedy needs no seed
        assert _gen(vlm, cache, q, do_sample=False, temperature=0.7, top_p=0.5) == greedy
        assert not SR.SAMPLE_CALLS


def test_seed_decides_the_ids():
    vlm, cache = _parent("M*-M*-")
    q = _questions(2)[1]
    with sampling_kernels_cpu():
        a = _gen(vlm, cache, q, do_sample=True, temperature=HOT, seed=1)
        b = _gen(vlm, cache, q, do_sample=True, temperature=HOT, seed=1)
        c = _gen(vlm, cache, q, do_sample=True, temperature=HOT, seed=2)
        d = _gen(vlm, cache, q, do_sample=True, temperature=HOT, seed=1, sample_stream=1)
    assert a == b and a != c and a != d


def test_draw_indices_count_the_new_tokens():
    vlm, cache = _parent("M*-M*-")
    q = _questions(2)[1]
    with sampling_kernels_cpu():
        SR.SAMPLE_CALLS.clear()
        _gen(vlm, cache, q, do_sample=True, temperature=HOT, top_k=12, top_p=0.9, seed=5, sample_stream=4)
    # one call per emitted token (the loop also looks at the logits behind the last token it feeds, as the greedy loop does)
    assert len(SR.SAMPLE_CALLS) in (7, 8) and [c[0] for c in SR.SAMPLE_CALLS] == [[n] for n in range(len(SR.SAMPLE_CALLS))]
    assert all(c[1:] == ([4], 5, HOT, 12, 0.9) for c in SR.SAMPLE_CALLS)


def test_sampling_needs_a_seed_and_refuses_what_is_not_built():
    vlm, cache = _parent("M*-M*-")
    q = _questions(2)[1]
    with sampling_kernels_cpu():
        with pytest.raises(ValueError, match="seed"):
            _gen(vlm, cache, q, do_sample=True)
        with pytest.raises(NotImplementedError, match="repetition_penalty"):
            _gen(vlm, cache, q, repetition_penalty=1.1)
        with pytest.raises(NotImplementedError, match="num_beams"):
            _gen(vlm, cache, q, num_beams=2)
        greedy = _gen(vlm, cache, q)
        assert _gen(vlm, cache, q, repetition_penalty=1.0, num_beams=1) == greedy


def test_speculative_with_sampling_decodes_plainly():
    vlm, cache = _parent("M*-M*-")
    q = _questions(2)[1]
    with sampling_kernels_cpu():
        want = _gen(vlm, cache, q, do_sample=True, temperature=HOT, seed=9)
        got = _gen(vlm, cache, q, do_sample=True, temperature=HOT, seed=9, speculative=4)
        assert vlm.last_generate_stats["speculative"] is False
    assert got == want


# ------------------------------------------------------------------------------------------------ generate_branches
@pytest.mark.parametrize("pattern", ["M*-M*-", "MM*-"])
def test_sampled_branches_equal_generate_on_clones(pattern):
    vlm, cache = _parent(pattern)
    qs = _questions(3)                                         # lengths 1, 4, 9: a short question answers earlier
    sk = dict(do_sample=True, temperature=HOT, top_k=20, top_p=0.95, seed=11)
    with sampling_kernels_cpu():
        want = [vlm.generate(q, past_key_values=cache.clone(), sample_stream=b, **KW, **sk) for b, q in enumerate(qs)]
        got = vlm.generate_branches(qs, past_key_values=cache, **KW, **sk)
        assert vlm.last_generate_stats["branched"] is True
        greedy = vlm.generate_branches(qs, past_key_values=cache, **KW)
    for g, w in zip(got, want):
        assert torch.equal(g, w), (g.tolist(), w.tolist())
    assert any(not torch.equal(g, w) for g, w in zip(got, greedy))                   # (it did sample)


def test_one_question_n_times_gives_n_samples():
    vlm, cache = _parent("M*-M*-")
    q = _questions(2)[1]
    sk = dict(do_sample=True, temperature=HOT, seed=4)
    with sampling_kernels_cpu():
        got = vlm.generate_branches([q] * 4, past_key_values=cache, **KW, **sk)
        again = vlm.generate_branches([q] * 4, past_key_values=cache, **KW, **sk)
        same = vlm.generate_branches([q] * 4, past_key_values=cache, **KW)
    ans = [g[0].tolist() for g in got]
    assert len(set(map(tuple, ans))) > 1, ans
    assert ans == [g[0].tolist() for g in again]
    assert len({tuple(g[0].tolist()) for g in same}) == 1                            # under argmax: one answer, four times


def test_sequential_fallback_keeps_the_stream_contract():
    vlm, cache = _parent("MM*-")
    qs = [torch.tensor([[b + 1, 2 * b + 3]]) for b in range(17)]                     # 17 questions: out of the lockstep scope
    kw = dict(max_new_tokens=3, return_ids=True, eos_token_id=-1)
    sk = dict(do_sample=True, temperature=HOT, seed=6)
    with sampling_kernels_cpu():
        want = [vlm.generate(q, past_key_values=cache.clone(), sample_stream=b, **kw, **sk) for b, q in enumerate(qs)]
        got = vlm.generate_branches(qs, past_key_values=cache, **kw, **sk)
    assert vlm.last_generate_stats["branched"] is False
    assert all(torch.equal(g, w) for g, w in zip(got, want))
