"""`host_state()` / `restore_host_state()` of the three holders a captured step runs against — the hybrid cache in
static-decode mode, the hybrid cache in speculation mode, a `BranchSet` — host logic, no GPU.

A failed graph capture has run the host bookkeeping of one step and no kernel (llm/decode_graph.py): the stepper takes the
holder's host state in front of the capture and puts it back behind a failure.  Here one real step runs in between (on the
oracle-backed stand-ins of the other CPU model tests) and everything the host side of a step changes has to be back where
it was: the sequence length, the room left, every K / V view's shape, `_kv_len`, and in speculation mode the counters
`spec_check` judges by.

The stack is the toy VLM of tests/test_branch_cpu.py behind a video prefill with two token-drop stages: its two attention
layers hold different numbers of tokens (57 and 41 rows), so a restore that treats the layers alike is seen."""
import contextlib

import pytest
import torch

import test_branch_cpu as tb
import test_speculative_cpu as ts
from oracle import ops as R


LENS = (57, 41)     # rows of the two attention layers behind the prefill


def _decode(q, k, v, seqlens_k=None, softmax_scale=None, return_lse=False, out=None):
    """`kernels.flash_attn_decode` with a device-side key count: the static-decode step's attention"""
    n = k.shape[1] if seqlens_k is None else int(seqlens_k[0])
    assert q.shape[1] == 1 and 1 <= n <= k.shape[1]
    o, lse = R.attention_ref(q, k[:, :n], v[:, :n], True, softmax_scale)
    return (o.to(q.dtype), lse) if return_lse else o.to(q.dtype)


@contextlib.contextmanager
def kernels_cpu():
    from timeviper_amd import kernels as K
    with tb.kernels_cpu(), ts.kernels_cpu():          # (the inner one's `flash_attn_append` takes a key count)
        saved = K.flash_attn_decode
        K.flash_attn_decode = _decode
        try:
            yield
        finally:
            K.flash_attn_decode = saved


@pytest.fixture(scope="module")
def prefilled():
    """The toy VLM and the cache of a 4-frame video turn: shared, never modified (every test works on a clone)."""
    vlm = tb._toy_vlm()
    T, tok = 4, vlm.default_token_id
    ids = torch.tensor([[5, 6] + [tok] * T + [7, 8, 9]])
    pix = torch.randn(T, 3, 96, 96, generator=torch.Generator().manual_seed(0))
    with kernels_cpu():
        _, cache = vlm.generate(ids, pixel_values_videos=pix, return_past_key_values=True, max_new_tokens=4,
                                return_ids=True, eos_token_id=-1)
    lens = [cache._kv_len[i] for i in cache.attention_layers]
    assert lens == list(LENS), lens
    return vlm, cache


def _forward(vlm, holder, ids):
    """One forward behind the prefill, as `generate`'s step functions run it."""
    ids = torch.tensor(ids)
    return vlm.llm_backbone(input_ids=ids, past_key_values=holder, use_cache=True, cache_position=torch.ones(1, dtype=torch.long),
                            position_ids=torch.ones((ids.shape[0], 1), dtype=torch.long),
                            train_pdrop_args=holder.pdrop_args, logits_to_keep=ids.shape[1]).logits


def _observe(holder):
    return {"seq": holder.get_seq_length(), "room": holder.static_room(), "kv_len": list(holder._kv_len),
            "k": [tuple(t.shape) for t in holder.key_cache], "v": [tuple(t.shape) for t in holder.value_cache]}


def test_static_decode_round_trip(prefilled):
    vlm, base = prefilled
    with torch.inference_mode(), kernels_cpu():
        cache = base.clone()
        cache.begin_static_decode(4)
        before = _observe(cache)
        state = cache.host_state()
        _forward(vlm, cache, [[3]])
        cache.advance_static_device()
        after = _observe(cache)
        cache.restore_host_state(state)
        assert _observe(cache) == before
    assert after["seq"] == before["seq"] + 1 and after["room"] == before["room"] - 1           # (the step did move them)
    assert [a - b for a, b in zip(after["kv_len"], before["kv_len"])] == [1 if i in cache.attention_layers else 0
                                                                          for i in range(len(before["kv_len"]))]
    assert after["k"] != before["k"] and after["v"] != before["v"]


def test_speculation_round_trip(prefilled):
    """Room for exactly one forward of 3 tokens: once all 3 are committed a second one is refused, and accepted again
    behind the restore."""
    vlm, base = prefilled
    T = 3
    with torch.inference_mode(), kernels_cpu():
        cache = base.clone()
        cache.begin_speculation(T, 0)
        before = _observe(cache)
        cache.spec_check(T)
        state = cache.host_state()
        _forward(vlm, cache, [[3, 4, 5]])
        cache.commit(T)
        with pytest.raises(RuntimeError, match="used up"):
            cache.spec_check(T)
        cache.restore_host_state(state)
        assert _observe(cache) == before
        cache.spec_check(T)
    # (only the host side goes back: here the step did run on the device, behind a failed capture nothing has)


def test_branch_set_round_trip(prefilled):
    vlm, base = prefilled
    with torch.inference_mode(), kernels_cpu():
        bs = base.clone().branch(2, suffix_cap=4)
        _forward(vlm, bs, [[3], [4]])                      # (a first step: the restore is not one to length zero)
        bs.advance_static_device()
        before = _observe(bs)
        state = bs.host_state()
        _forward(vlm, bs, [[5], [6]])
        bs.advance_static_device()
        after = _observe(bs)
        bs.restore_host_state(state)
        assert _observe(bs) == before
    assert before["seq"] == base.get_seq_length() + 1 and after["seq"] == before["seq"] + 1
    assert after["room"] == before["room"] - 1 == 2
    assert [k[:2] for i, k in enumerate(before["k"]) if i in bs.attention_layers] == [(2, 1), (2, 1)]
    assert [k[:2] for i, k in enumerate(after["k"]) if i in bs.attention_layers] == [(2, 2), (2, 2)]
