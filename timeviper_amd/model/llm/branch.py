"""Branched decoding: several questions about ONE prefilled video, decoded in lockstep.

`HybridMambaAttentionDynamicCache.branch(n)` returns a `BranchSet`: n branches of the parent cache that are decoded
together, one token per branch and step, as the n rows of the same products (the decode step is weight-read bound: n rows
cost little more than one).  What is large is shared, what is small is copied:

  * K / V of every attention layer at its current length is NOT copied: the set holds the parent's tensors as the PREFIX
    every branch sees whole (one prefix length per layer: token-drop stages leave the layers with different lengths);
  * every branch owns a SUFFIX buffer (n, cap, Hkv, D) per attention layer for the tokens fed since the fork (one suffix
    length for all layers and branches: the branches advance in lockstep); the attention of a step is
    `kernels.flash_attn_branch` — the prefix read once for all branches, each branch's suffix rows for itself alone;
  * the conv / SSM states are copied n times into batch-n tensors.

The parent is never written, and must not be appended to while a set made from it is in use (the set would then see rows
that are not part of the fork): every step checks that the parent still holds the storage and the lengths of the fork.

The set is always launch-parameter-static — the write slot and the per-branch key count live on the device — and offers
the static-decode interface of the hybrid cache, so that `GraphedDecodeStep` captures the branched step with
`batch_size = n` as it captures the plain one.  Whoever runs a step eagerly calls `advance_static_device()` behind it.
The suffix rows are kept as the hybrid cache keeps its rows, by the same code (`nano.KVRows`: `_set_len`, `static_room`,
`kv_buffers`, `advance_static_host`, `host_state` / `restore_host_state`); the rest of the cache interface is duck-typed.
"""
from __future__ import annotations

from typing import List, Optional

import torch

from .nano import KVRows

__all__ = ["BranchSet", "MAX_BRANCHES"]

MAX_BRANCHES = 16        # kernels.flash_attn_branch's range (tv_attn_branch_fwd)


class BranchSet(KVRows):
    is_branch_set = True
    speculating = False

    def __init__(self, parent, n: int, suffix_cap: int = 256):
        n, suffix_cap = int(n), int(suffix_cap)
        if n < 1:
            raise ValueError("branch: n >= 1 branches")
        if getattr(parent, "speculating", False):
            raise RuntimeError("branch: the cache is in speculation mode (provisional tokens are not part of it yet); "
                               "call end_speculation() first")
        if not parent.holds_prefill():
            raise RuntimeError("branch: the cache holds no prefill (every attention layer holding its tokens)")
        if parent.key_cache[parent.attention_layers[0]].shape[0] != 1:
            raise RuntimeError("branch: the parent holds one sequence")
        self.parent, self.n = parent, n
        self.dtype = parent.dtype
        self.hybrid_override_pattern = parent.hybrid_override_pattern
        self.conv_kernel_size = parent.conv_kernel_size
        self.has_previous_state = parent.has_previous_state
        self.transformer_layers, self.attention_layers = list(parent.transformer_layers), list(parent.attention_layers)
        rep = lambda t: t.repeat(n, *([1] * (t.dim() - 1)))
        self.conv_states: List[torch.Tensor] = [rep(t) for t in parent.conv_states]
        self.ssm_states: List[torch.Tensor] = [rep(t) for t in parent.ssm_states]
        nl = len(parent.key_cache)
        # the prefix: the parent's own tensors, (1, L_i, Hkv, D)
        self.prefix_len = {i: parent._kv_len[i] for i in self.attention_layers}
        self.prefix = {i: (parent.key_cache[i], parent.value_cache[i]) for i in self.attention_layers}
        # the suffixes, under the names the hybrid cache uses for its rows (KVRows)
        self._kv_buf = [None] * nl
        self._kv_len = [0] * nl
        self.key_cache = [parent.key_cache[i][:0] for i in range(nl)]
        self.value_cache = [parent.value_cache[i][:0] for i in range(nl)]
        self._alloc(max(suffix_cap, 1))
        dev = parent.key_cache[self.attention_layers[0]].device
        self._pos = torch.zeros(1, dtype=torch.int64, device=dev)           # the row a step writes
        self._lens = torch.ones(n, dtype=torch.int32, device=dev)           # rows a step's queries see: that row included
        self.static_decode = False
        pending = getattr(parent, "pending_ids", None)
        self.pending_ids: Optional[torch.Tensor] = None if pending is None else pending.clone()
        if hasattr(parent, "pdrop_args"):       # the drop bookkeeping of the parent's prefill travels with the set
            self.pdrop_args = None if parent.pdrop_args is None else dict(parent.pdrop_args)

    def _alloc(self, cap: int):
        for i in self.attention_layers:
            kp = self.prefix[i][0]
            have = self._kv_len[i]
            kb, vb = (kp.new_zeros((self.n, cap) + tuple(kp.shape[2:])) for _ in range(2))
            if have:
                kb[:, :have], vb[:, :have] = self.key_cache[i], self.value_cache[i]
            self._kv_buf[i] = (kb, vb)
            self._set_len(i, have)

    # ---- what the model's layers ask
    @property
    def suffix_len(self) -> int:
        return self._kv_len[self.attention_layers[0]]

    def get_seq_length(self, layer_idx: Optional[int] = 0) -> int:
        return self.prefix_len[self.attention_layers[0]] + self.suffix_len

    def check_parent(self, layer_idx):
        """The parent still holds what was forked: same storage, same length."""
        p = self.parent
        kp, vp = self.prefix[layer_idx]
        if (p._kv_len[layer_idx] != self.prefix_len[layer_idx] or p.key_cache[layer_idx].data_ptr() != kp.data_ptr()
                or p.value_cache[layer_idx].data_ptr() != vp.data_ptr()):
            raise RuntimeError("branch set: the parent cache was appended to (or its storage replaced) after branch(); "
                               "its branches would see rows that are not part of the fork")

    def write(self, key_states, value_states, layer_idx):
        """The n new rows (n, 1, Hkv, D) of a step into the suffix buffers, at the device-side slot.  Returns the operands
        of `kernels.flash_attn_branch` behind q: (k_prefix, v_prefix, k_suffix, v_suffix, seqlens_suffix)."""
        if key_states.shape[:2] != (self.n, 1):
            raise RuntimeError(f"branch set: a step feeds one token per branch, ({self.n}, 1) ids; got rows of shape "
                               f"{tuple(key_states.shape[:2])}")
        self.check_parent(layer_idx)
        kb, vb = self._kv_buf[layer_idx]
        have = self._kv_len[layer_idx]
        if have + 1 > kb.shape[1]:
            raise RuntimeError("branch set: the suffix buffers are full (branch(n, suffix_cap) / begin_static_decode "
                               "reserved too little)")
        kb.index_copy_(1, self._pos, key_states)
        vb.index_copy_(1, self._pos, value_states)
        self._set_len(layer_idx, have + 1)
        kp, vp = self.prefix[layer_idx]
        return kp, vp, kb, vb, self._lens

    def update(self, key_states, value_states, layer_idx, cache_kwargs=None):
        raise RuntimeError("branch set: attention goes through write() and kernels.flash_attn_branch")

    def update_conv_state(self, layer_idx, new_conv_state, cache_init=False):
        raise RuntimeError("branch set: a prefill belongs to the parent cache")

    def update_ssm_state(self, layer_idx, new_ssm_state):
        self.ssm_states[layer_idx] = new_ssm_state
        return new_ssm_state

    # ---- the static-decode interface (GraphedDecodeStep)
    def begin_static_decode(self, max_new_tokens: int):
        """Room for `max_new_tokens` more steps; from here on the buffers stay where they are."""
        need = self.suffix_len + int(max_new_tokens)
        if need > self._kv_buf[self.attention_layers[0]][0].shape[1]:
            if self.static_decode:
                raise RuntimeError("branch set: static decode: the suffix buffers are fixed")
            self._alloc(need)
        self.static_decode = True

    def end_static_decode(self):
        self.static_decode = False

    def advance_static_device(self):
        """Device side of one finished step (part of a captured graph; behind every eager step too)."""
        self._pos += 1
        self._lens += 1

    def decode_lens(self, layer_idx):
        return self._lens

    def advance_static_host(self):
        """Host side of one REPLAYED step: the check and the bookkeeping `write` does when it runs."""
        for i in self.attention_layers:
            self.check_parent(i)
        super().advance_static_host()
