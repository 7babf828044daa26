"""Host-side mirror of the reference's NemotronH hybrid LM
(`timeviper/model/llm/llm_repo/nano/{configuration_nano,modeling_nano}.py`): same
class names, module tree, parameter names / shapes (state-dict compatible,
SURVEY.md §8b) and forward() signatures — with every hot operator bound to the
gfx950 kernels in `timeviper_amd.kernels` instead of mamba_ssm / causal_conv1d /
flash_attn.  GEMMs stay on torch (hipBLASLt).  Inference (prefill + decode) only.

What is deliberately different from the reference (SURVEY.md §3.2 notes):
  * no per-layer `torch.isnan(...).any()` host sync (:1690) — `check_nan=True`
    restores it;
  * `lm_head` is applied to the positions asked for by `logits_to_keep`
    (default: last token) instead of all L positions (:2433);
  * pdrop "attn" ranking never builds the (L, L) mask (:1848-1857);
  * the residual add of layer i is fused into the RMSNorm of layer i+1.
"""
from __future__ import annotations

import math
import os
import re
from dataclasses import dataclass
from typing import Any, Dict, List, Optional, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from ... import kernels as K
from .pdrop import PdropMixin


# ------------------------------------------------------------------ config
class NemotronHConfig:
    """Field-for-field mirror of the reference's NemotronHConfig
    (configuration_nano.py:133-258)."""

    model_type = "nano"

    def __init__(self, vocab_size=131072, tie_word_embeddings=False, hidden_size=4096,
                 intermediate_size=21504, num_hidden_layers=52,
                 hybrid_override_pattern="M-M-M-M*-M-M-M-M-M*-M-M-M-M-M*-M-M-M-M-M*-M-M-M-M-M-",
                 num_attention_heads=32, head_dim=128, num_key_value_heads=8,
                 mlp_hidden_act="relu2", attention_bias=False, mlp_bias=False, use_bias=False,
                 initializer_range=0.02, layer_norm_epsilon=1e-5, residual_in_fp32=False,
                 use_cache=True, num_logits_to_keep=1, pad_token_id=0, bos_token_id=1,
                 eos_token_id=2, sliding_window=None, max_position_embeddings=4096,
                 attention_dropout=0.0, hidden_dropout=0.0, use_mamba_kernels=True,
                 ssm_state_size=128, mamba_num_heads=128, mamba_n_groups=8, mamba_head_dim=64,
                 mamba_d_conv=4, mamba_expand=2, mamba_hidden_act="silu", mamba_dt_min=0.001,
                 mamba_dt_max=0.1, mamba_dt_limit=(0.0, float("inf")), mamba_dt_init_floor=1e-4,
                 mamba_conv_bias=True, mamba_proj_bias=False, mamba_chunk_size=256,
                 rescale_prenorm_residual=True, merge_module="no_merge", use_pdrop=False,
                 pdrop_type=None, **kwargs):
        assert len(hybrid_override_pattern) == num_hidden_layers, \
            "hybrid_override_pattern must have the same length as num_hidden_layers"
        assert re.match(r"^[*\-M]+$", hybrid_override_pattern), \
            "hybrid_override_pattern must only contain characters 'M', '*', or '-'"
        self.vocab_size = vocab_size
        self.tie_word_embeddings = tie_word_embeddings
        self.hidden_size = hidden_size
        self.intermediate_size = intermediate_size
        self.num_hidden_layers = num_hidden_layers
        self.hybrid_override_pattern = hybrid_override_pattern
        self.num_attention_heads = num_attention_heads
        self.head_dim = head_dim
        self.sliding_window = sliding_window
        self.max_position_embeddings = max_position_embeddings
        self.attention_dropout = attention_dropout
        self.hidden_dropout = hidden_dropout
        self.num_key_value_heads = num_attention_heads if num_key_value_heads is None \
            else num_key_value_heads
        self.mlp_hidden_act = mlp_hidden_act
        self.attention_bias = attention_bias
        self.mlp_bias = mlp_bias
        self.use_bias = use_bias
        self.initializer_range = initializer_range
        self.layer_norm_epsilon = layer_norm_epsilon
        self.residual_in_fp32 = residual_in_fp32
        self.use_cache = use_cache
        self.num_logits_to_keep = num_logits_to_keep
        self.use_mamba_kernels = use_mamba_kernels
        self.n_groups = mamba_n_groups
        self.mamba_head_dim = mamba_head_dim
        self.ssm_state_size = ssm_state_size
        self.mamba_num_heads = mamba_num_heads
        self.conv_kernel = mamba_d_conv
        self.expand = mamba_expand
        self.mamba_hidden_act = mamba_hidden_act
        self.time_step_min = mamba_dt_min
        self.time_step_max = mamba_dt_max
        self.time_step_limit = tuple(mamba_dt_limit)
        self.time_step_floor = mamba_dt_init_floor
        self.use_conv_bias = mamba_conv_bias
        self.mamba_proj_bias = mamba_proj_bias
        self.chunk_size = mamba_chunk_size
        self.rescale_prenorm_residual = rescale_prenorm_residual
        self.merge_module = merge_module
        self.use_pdrop = use_pdrop
        self.pdrop_type = pdrop_type
        self.pad_token_id, self.bos_token_id, self.eos_token_id = \
            pad_token_id, bos_token_id, eos_token_id
        self._attn_implementation = kwargs.pop("attn_implementation", "flash_attention_2")
        self.output_attentions = False
        self.output_hidden_states = False
        self.use_return_dict = True
        for k, v in kwargs.items():
            setattr(self, k, v)

    @property
    def layers_block_type(self):
        return ["mamba" if c == "M" else "attention" if c == "*" else "mlp"
                for c in self.hybrid_override_pattern]

    @classmethod
    def nemotron_nano_9b_v2(cls, **over):
        """NVIDIA-Nemotron-Nano-9B-v2 dims (public config.json)."""
        kw = dict(vocab_size=131072, hidden_size=4480, intermediate_size=15680,
                  num_hidden_layers=56,
                  hybrid_override_pattern="M-M-M-MM-M-M-M*-M-M-M*-M-M-M-M*-M-M-M-M*-M-MM-M-M-M-M-M-",
                  num_attention_heads=40, head_dim=128, num_key_value_heads=8,
                  ssm_state_size=128, mamba_num_heads=128, mamba_n_groups=8, mamba_head_dim=80,
                  mamba_d_conv=4, mamba_chunk_size=128, layer_norm_epsilon=1e-5,
                  max_position_embeddings=131072)
        kw.update(over)
        return cls(**kw)


@dataclass
class BaseModelOutputWithPastAndLabels:
    last_hidden_state: Optional[torch.Tensor] = None
    past_key_values: Any = None
    hidden_states: Optional[Tuple[torch.Tensor, ...]] = None
    attentions: Optional[Tuple[torch.Tensor, ...]] = None
    labels: Optional[torch.Tensor] = None

    def __getitem__(self, i):
        return [v for v in (self.last_hidden_state, self.past_key_values, self.hidden_states,
                            self.labels) if v is not None][i]


@dataclass
class CausalLMOutputWithPast:
    loss: Optional[torch.Tensor] = None
    logits: Optional[torch.Tensor] = None
    past_key_values: Any = None
    hidden_states: Optional[Tuple[torch.Tensor, ...]] = None
    attentions: Optional[Tuple[torch.Tensor, ...]] = None


# ------------------------------------------------------------------- cache
class KVRows:
    """The rows every attention layer holds, for the hybrid cache and for `BranchSet` (llm/branch.py): `_kv_buf[i]` are a
    layer's (k, v) capacity buffers, `_kv_len[i]` the rows of them in use, `key_cache[i]` / `value_cache[i]` the views of
    exactly those rows.  `_set_len` is the one place that moves the three together."""

    def _set_len(self, layer_idx, n):
        """Layer `layer_idx` now holds `n` rows of its buffers."""
        kb, vb = self._kv_buf[layer_idx]
        self._kv_len[layer_idx] = n
        self.key_cache[layer_idx], self.value_cache[layer_idx] = kb[:, :n], vb[:, :n]

    def kv_buffers(self, layer_idx):
        """The capacity buffers of a layer (static decode: what the attention kernel is handed, with `decode_lens`)."""
        return self._kv_buf[layer_idx]

    def static_room(self) -> int:
        """Tokens the fixed buffers still take (a replayed graph writes where its device-side position says: the caller
        must stop before the buffers end — GraphedDecodeStep checks this before every launch)."""
        return min(self._kv_buf[i][0].shape[1] - self._kv_len[i] for i in self.attention_layers)

    def advance_static_host(self):
        """Host side of one REPLAYED step: the bookkeeping the step's cache write does when it runs."""
        for i in self.attention_layers:
            self._set_len(i, self._kv_len[i] + 1)

    # What the host side of a step changes and no kernel reads: the rows every layer holds and, in speculation mode, the host
    # side of `_spec`.  A graph capture runs it without running the step, so a failed capture has to put it back
    # (llm/decode_graph.py).
    def host_state(self):
        return {i: self._kv_len[i] for i in self.attention_layers}, dict(self._spec["host"]) if self.speculating else None

    def restore_host_state(self, state):
        rows, spec = state
        for i, n in rows.items():
            self._set_len(i, n)
        if spec is not None:
            self._spec["host"].update(spec)


class HybridMambaAttentionDynamicCache(KVRows):
    """Per-layer conv / ssm / key / value lists (reference :205-360).  SSM states
    are kept in fp32 (what the scan kernel returns and the decode kernel updates).

    Keys / values: `key_cache[i]` is what the reference holds — (B, L_i, Hkv, D) with every token seen so far — but it is a
    VIEW of a buffer with spare capacity: the reference's `torch.cat` per generated token (:246-251) re-copies the whole
    cache (2 x 135 MB per attention layer and token behind a 2 048-frame prefill); here a token is written in place and the
    buffer grows geometrically when it runs out.

    `begin_static_decode(n)` fixes the buffers for the next n tokens and moves the write position and the key count to
    DEVICE memory: every launch of a decode step then has the same parameters, which is what
    lets `GraphedDecodeStep` replay it as one hipGraph."""

    def __init__(self, config, batch_size, dtype=torch.bfloat16, device=None, kv_reserve=256):
        self.dtype = dtype
        self.hybrid_override_pattern = config.hybrid_override_pattern
        self.has_previous_state = False
        self.conv_kernel_size = config.conv_kernel
        n = config.num_hidden_layers
        empty = lambda: torch.empty((batch_size, 0), device=device)
        self.conv_states: List[torch.Tensor] = [empty() for _ in range(n)]
        self.ssm_states: List[torch.Tensor] = [empty() for _ in range(n)]
        self.key_cache: List[torch.Tensor] = [empty() for _ in range(n)]
        self.value_cache: List[torch.Tensor] = [empty() for _ in range(n)]
        self.transformer_layers = [i for i, c in enumerate(config.hybrid_override_pattern)
                                   if c != "M"]
        self.attention_layers = [i for i, c in enumerate(config.hybrid_override_pattern)
                                 if c == "*"]
        self.kv_reserve = int(kv_reserve)
        self._kv_buf = [None] * n              # (k, v) capacity buffers, (B, cap, Hkv, D)
        self._kv_len = [0] * n
        # static decode: per distinct cache length an int64 (1,) write slot and an int32 (B,) key count, on the device
        self._static, self._static_of, self.static_decode = {}, {}, False
        # ids `generate` emitted but has not run through the model yet (it stops before feeding its last token): the
        # next turn's continuation feeds them in front of its own ids
        self.pending_ids: Optional[torch.Tensor] = None
        # speculation (begin_speculation): T tokens are taken provisionally, commit(k) keeps the first k
        self._mamba_dims = (config.mamba_num_heads * config.mamba_head_dim, config.n_groups, config.ssm_state_size,
                            config.mamba_num_heads)
        self.speculating, self._spec = False, None

    def _reserve(self, layer_idx, need):
        have = self._kv_len[layer_idx]
        buf = self._kv_buf[layer_idx]
        if buf is not None and buf[0].shape[1] >= need:
            return
        if self.static_decode:
            raise RuntimeError("static decode: the key / value buffers are fixed (begin_static_decode reserved too little)")
        k_old, v_old = self.key_cache[layer_idx], self.value_cache[layer_idx]
        shape = (k_old.shape[0], need + max(self.kv_reserve, have // 8)) + tuple(k_old.shape[2:])
        kb, vb = k_old.new_empty(shape), v_old.new_empty(shape)
        kb[:, :have], vb[:, :have] = k_old, v_old
        self._kv_buf[layer_idx] = (kb, vb)
        self._set_len(layer_idx, have)

    def update(self, key_states, value_states, layer_idx, cache_kwargs=None):
        """key/value (B, L, Hkv, D) — sequence-major, the layout the attention kernel reads."""
        new = key_states.shape[1]
        if self.key_cache[layer_idx].shape[-1] == 0:        # prefill: adopt the projections' output, no copy
            self.key_cache[layer_idx], self.value_cache[layer_idx] = key_states, value_states
            self._kv_buf[layer_idx], self._kv_len[layer_idx] = None, new
            return key_states, value_states
        have = self._kv_len[layer_idx]
        self._reserve(layer_idx, have + new)
        kb, vb = self._kv_buf[layer_idx]
        if self.static_decode:
            if new != 1:
                raise RuntimeError("static decode takes one token per step")
            pos = self._static_of[layer_idx][0]
            kb.index_copy_(1, pos, key_states)
            vb.index_copy_(1, pos, value_states)
        else:
            kb[:, have:have + new], vb[:, have:have + new] = key_states, value_states
        self._set_len(layer_idx, have + new)
        return self.key_cache[layer_idx], self.value_cache[layer_idx]

    def holds_prefill(self) -> bool:
        """Behind a prefill: every attention layer holding its tokens."""
        return bool(self.attention_layers) and all(self._kv_len[i] > 0 for i in self.attention_layers)

    def _fix_buffers(self, room: int, seen: int):
        """Room for `room` more rows in buffers that stay where they are, and per distinct cache length (token drop leaves
        the attention layers behind a stage with fewer tokens than the ones in front of it) an int64 (1,) write slot and
        an int32 (B,) key count on the device, shared by the layers that hold it.  `seen`: the count's lead over the slot
        — 1 where a step's query sees the row it writes (static decode), 0 where a forward adds its own T (speculation)."""
        self.end_static_decode()
        for i in self.attention_layers:
            self._reserve(i, self._kv_len[i] + room)
        k0 = self.key_cache[self.attention_layers[0]]
        self._static = {n: (torch.full((1,), n, dtype=torch.int64, device=k0.device),
                            torch.full((k0.shape[0],), n + seen, dtype=torch.int32, device=k0.device))
                        for n in sorted({self._kv_len[i] for i in self.attention_layers})}
        self._static_of = {i: self._static[self._kv_len[i]] for i in self.attention_layers}

    # ---- static decode (fixed launch parameters; see GraphedDecodeStep)
    def begin_static_decode(self, max_new_tokens: int):
        """One token per step for the next `max_new_tokens` steps, every launch with the same parameters (`_fix_buffers`)."""
        if not self.holds_prefill():
            raise RuntimeError("static decode starts behind a prefill (every attention layer holding its tokens)")
        self._fix_buffers(int(max_new_tokens), seen=1)
        self.static_decode = True

    def end_static_decode(self):
        self._static, self._static_of, self.static_decode = {}, {}, False

    def advance_static_device(self):
        """Device side of one finished step (part of the captured graph)."""
        for pos, lens in self._static.values():
            pos += 1
            lens += 1

    def decode_lens(self, layer_idx):
        return self._static_of[layer_idx][1]

    def get_seq_length(self, layer_idx: Optional[int] = 0) -> int:
        if not self.attention_layers:
            return 0
        k = self.key_cache[self.attention_layers[0]]
        return 0 if k.shape[-1] == 0 else k.shape[1]

    def clone(self) -> "HybridMambaAttentionDynamicCache":
        """Deep copy of the conv / SSM states and of K / V at their current lengths (spare capacity is not copied, a
        static-decode mode is not inherited): one prefilled video forks into several questions."""
        if getattr(self, "speculating", False):
            raise RuntimeError("clone: the cache is in speculation mode (provisional tokens are not part of it yet); "
                               "call end_speculation() first")
        new = object.__new__(type(self))
        new.__dict__.update({k: v for k, v in self.__dict__.items()
                             if k not in ("conv_states", "ssm_states", "key_cache", "value_cache", "_kv_buf", "_kv_len",
                                          "_static", "_static_of", "static_decode", "pending_ids", "pdrop_args")})
        new.transformer_layers, new.attention_layers = list(self.transformer_layers), list(self.attention_layers)
        new.conv_states = [t.clone() for t in self.conv_states]
        new.ssm_states = [t.clone() for t in self.ssm_states]
        new.key_cache = [t.clone() for t in self.key_cache]
        new.value_cache = [t.clone() for t in self.value_cache]
        n = len(self.key_cache)
        new._kv_buf = [None] * n
        new._kv_len = list(self._kv_len)
        for i in range(n):
            if self._kv_buf[i] is not None:         # a buffer of exactly the tokens held: the next append grows it
                new._kv_buf[i] = (new.key_cache[i], new.value_cache[i])
        new._static, new._static_of, new.static_decode = {}, {}, False
        pending = getattr(self, "pending_ids", None)
        new.pending_ids = None if pending is None else pending.clone()
        if getattr(self, "pdrop_args", None) is not None:
            new.pdrop_args = dict(self.pdrop_args)
        return new

    def branch(self, n: int, suffix_cap: int = 256):
        """n branches of this cache that are decoded together, one token per branch and step (llm/branch.py): K / V at
        their current lengths are SHARED with the set as the prefix every branch sees (no copy), the conv / SSM states are
        copied n times, every branch gets suffix buffers of `suffix_cap` rows.  This cache is not written by the set and
        must not be appended to while the set is in use.  Raises in speculation mode or without a prefill."""
        from .branch import BranchSet
        return BranchSet(self, n, suffix_cap)

    # ---- speculation: T tokens per forward taken provisionally, the first k kept (see NemotronHMamba2Mixer._speculate)
    def begin_speculation(self, t_max: int, max_new_tokens: int):
        """Behind a prefill: from now on a forward of T <= t_max tokens leaves the conv / SSM states and the committed
        K / V rows as they are, and `commit(k)` decides how many of its tokens the NEXT forward (or `end_speculation`) folds
        in.  Memory holds the committed state at all times.  Per Mamba layer two slots keep a forward's operands (post-conv
        x / B / C, the pre-conv rows and dt) — one being written, one holding the previous forward's; write position, key
        count (the static-decode pairs, one per distinct length) and n_commit live on the device, so that a step has the same
        launch parameters every time (GraphedSpecStep)."""
        if self.speculating:
            raise RuntimeError("begin_speculation: already speculating")
        if not self.holds_prefill():
            raise RuntimeError("speculation starts behind a prefill (every attention layer holding its tokens)")
        t_max, max_new_tokens = int(t_max), int(max_new_tokens)
        if t_max < 1 or max_new_tokens < 0:
            raise ValueError("begin_speculation: t_max >= 1, max_new_tokens >= 0")
        self._fix_buffers(max_new_tokens + t_max, seen=0)
        k0 = self.key_cache[self.attention_layers[0]]
        dev, B = k0.device, k0.shape[0]
        d_in, G, N, H = self._mamba_dims
        slots = {}
        for i, c in enumerate(self.hybrid_override_pattern):
            if c == "M":
                dt = self.conv_states[i].dtype
                mk = lambda n: torch.zeros(B * t_max * n, dtype=dt, device=dev)
                slots[i] = [{"x": mk(d_in), "B": mk(G * N), "C": mk(G * N), "tail": mk(d_in + 2 * G * N + H)} for _ in range(2)]
        self._spec = {"t_max": t_max, "room": max_new_tokens + t_max, "slots": slots,
                      "n_commit": torch.zeros(1, dtype=torch.int32, device=dev),
                      "kidx": torch.arange(self.conv_kernel_size, device=dev), "tidx": torch.arange(t_max, device=dev),
                      "base": {i: self._kv_len[i] for i in self.attention_layers},
                      # everything a forward and a commit change on the host (`_spec_host_end` and `_spec_host_commit` alone
                      # write it, `host_state` copies it whole): flip, the operand slot the next forward writes; t_prev, the
                      # tokens of the last forward; done / last_k, the tokens kept of the forwards before the last one / of
                      # the last one — upper bounds, and flagged as such (exact / last_exact), while a device-side commit has
                      # not been reported (note_committed)
                      "host": {"flip": 0, "t_prev": 0, "done": 0, "exact": True, "last_k": 0, "last_exact": True},
                      "flush": {}, "cidx": None, "rows": {}, "lens_t": {}}
        self.speculating = True

    def _spec_views(self, layer_idx, which, T):
        """Operand views of T tokens in a layer's slot: which = 0 the one this forward writes, 1 the previous forward's."""
        d_in, G, N, H = self._mamba_dims
        B = self.ssm_states[layer_idx].shape[0]
        sl = self._spec["slots"][layer_idx][self._spec["host"]["flip"] ^ which]
        W = d_in + 2 * G * N + H
        return (sl["x"][:B * T * d_in].view(B, T, d_in), sl["B"][:B * G * T * N].view(B, G, T, N),
                sl["C"][:B * G * T * N].view(B, G, T, N), sl["tail"][:B * T * W].view(B, T, W))

    def spec_prev_operands(self, layer_idx):
        """(x, dt, B, C) of the previous forward as the recurrence kernels take them, or None before the first one."""
        T = self._spec["host"]["t_prev"]
        if T == 0:
            return None
        d_in, G, N, H = self._mamba_dims
        x, Bm, Cm, tail = self._spec_views(layer_idx, 1, T)
        return (x.view(x.shape[0], T, H, d_in // H), tail[..., d_in + 2 * G * N:], Bm.transpose(1, 2), Cm.transpose(1, 2))

    # host bookkeeping of a provisional forward, in ONE place: the eager forward runs it beside its device work, a replayed
    # graph (GraphedSpecStep) runs it alone — the capture executed exactly these functions, so the two cannot drift apart
    def spec_check(self, T: int):
        """The host-side checks in front of a provisional forward of T tokens, eager or replayed."""
        sp, h = self._spec, self._spec["host"]
        if T > sp["t_max"]:
            raise RuntimeError(f"speculation: {T} tokens in one forward, begin_speculation reserved t_max = {sp['t_max']}")
        if h["done"] + h["last_k"] + T > sp["room"]:
            raise RuntimeError("speculation: the key / value rows reserved by begin_speculation are used up")

    def _spec_host_end(self, T: int):
        h = self._spec["host"]
        h["done"] += h["last_k"]
        h["exact"] = h["exact"] and h["last_exact"]
        h["flip"] ^= 1
        h["t_prev"], h["last_k"], h["last_exact"] = int(T), 0, True

    def _spec_host_commit(self, k):
        """k: the host value, or None for a device-side commit nobody has reported yet (upper bound: every token)."""
        h = self._spec["host"]
        h["last_k"], h["last_exact"] = (h["t_prev"], False) if k is None else (int(k), True)

    def spec_parity(self) -> int:
        """The operand slot the next forward writes: a captured step is the step of one parity (GraphedSpecStep)."""
        return self._spec["host"]["flip"]

    def spec_replayed(self, T: int):
        """Host side of a REPLAYED step (forward + device-side commit), behind `spec_check(T)` in front of the launch: what
        the captured functions did on the host."""
        self._spec_host_end(T)
        self._spec_host_commit(None)

    def spec_begin_forward(self, T: int):
        """Host checks and the device-side indices of one provisional forward (no host sync)."""
        self.spec_check(T)
        sp = self._spec
        sp["cidx"] = sp["kidx"] + sp["n_commit"]
        sp["rows"] = {n: pos + sp["tidx"][:T] for n, (pos, _) in self._static.items()}
        sp["lens_t"] = {n: lens + T for n, (_, lens) in self._static.items()}

    def spec_commit_conv(self, layer_idx):
        """conv state <- the last K columns of [state | the previous forward's pre-conv rows[:n_commit]]: a gather with a
        device index (nothing to do before the first forward)."""
        T = self._spec["host"]["t_prev"]
        if T == 0:
            return
        cs = self.conv_states[layer_idx]
        d_in, G, N, H = self._mamba_dims
        pre = self._spec_views(layer_idx, 1, T)[3][..., :d_in + 2 * G * N]
        cs.copy_(torch.cat([cs, pre.transpose(1, 2).to(cs.dtype)], dim=-1).index_select(-1, self._spec["cidx"]))

    def spec_end_forward(self, T: int):
        """The forward's tokens are now the provisional ones: none of them kept until `commit` says so."""
        self._spec_host_end(T)
        self._spec["n_commit"].zero_()

    def commit(self, k):
        """Keep the first k tokens of the last forward: an int, or a tensor on the cache's device (no host sync; the caller
        reports the value with `note_committed` once it has read it).  May be called again with a smaller k before the
        next forward."""
        if not self.speculating:
            raise RuntimeError("commit: the cache is not in speculation mode")
        sp = self._spec
        T = sp["host"]["t_prev"]
        if isinstance(k, torch.Tensor):
            kt = k.reshape(1).to(torch.int32).clamp(0, T)
            self._spec_host_commit(None)
        else:
            if not 0 <= int(k) <= T:
                raise ValueError(f"commit: k = {k} outside [0, {T}] (the tokens of the last forward)")
            kt = torch.full((1,), int(k), dtype=torch.int32, device=sp["n_commit"].device)
            self._spec_host_commit(k)
        delta = kt - sp["n_commit"]
        for pos, lens in self._static.values():
            pos += delta
            lens += delta
        sp["n_commit"].copy_(kt)

    def note_committed(self, k: int):
        """Host side of a device-side `commit(tensor)`: the value, once the caller has read it back."""
        if not 0 <= int(k) <= self._spec["host"]["t_prev"]:
            raise ValueError("note_committed: k outside the last forward")
        self._spec_host_commit(k)

    def end_speculation(self):
        """Fold the kept tokens of the last forward in (one flush launch per Mamba layer, the conv state), fix the K / V
        views to the committed length and free the slots: the cache is then what plain steps over the kept tokens leave."""
        if not self.speculating:
            return
        sp, h = self._spec, self._spec["host"]
        if h["t_prev"] > 0:
            sp["cidx"] = sp["kidx"] + sp["n_commit"]
            for i, fl in sp["flush"].items():
                self.spec_commit_conv(i)
                K.selective_state_update_spec(self.ssm_states[i], self.spec_prev_operands(i), sp["n_commit"], None,
                                              fl["A"], dt_bias=fl["dt_bias"], dt_softplus=True, dt_limit=fl["dt_limit"],
                                              group_map=fl["group_map"])
        first = self.attention_layers[0]
        if h["exact"] and h["last_exact"]:
            done = h["done"] + h["last_k"]
        else:       # a device-side commit nobody reported: one read
            done = int(self._static_of[first][0]) - sp["base"][first]
        for i in self.attention_layers:
            self._set_len(i, sp["base"][i] + done)
        self._static, self._static_of = {}, {}
        self.speculating, self._spec = False, None

    def update_conv_state(self, layer_idx, new_conv_state, cache_init=False):
        assert cache_init
        self.conv_states[layer_idx] = new_conv_state
        return new_conv_state

    def update_ssm_state(self, layer_idx, new_ssm_state):
        self.ssm_states[layer_idx] = new_ssm_state
        return new_ssm_state


# ------------------------------------------------------------------ fused-step helpers
ROWS_FUSED_DEFAULT = "0"       # what TV_ROWS_FUSED is taken to be when it is not set


def is_continuation(past_key_values, cache_position) -> bool:
    """A forward behind a finished prefill: a cache and a first position > 0 (one token: the decode step)."""
    return past_key_values is not None and cache_position is not None and int(cache_position[0]) > 0


def linear_route(x, cache=None, cache_position=None) -> Optional[str]:
    """The kernel ONE linear layer runs on for x (B, T, K), by the tensor's device, dtype and shape and the switches (read
    per call):
      "gemv"  tv_gemv_bf16_fwd — one token of 1..4 sequences, unless TV_DECODE_FUSED=0;
      "rows"  tv_linear_rows_bf16_fwd — 2..16 tokens of one sequence behind a prefill (a continuation, a speculative
              step), or one token of 5..16 sequences behind one (a branched step), under TV_ROWS_FUSED=1 (off by default
              until the step is measured faster on an MI355X);
      None    torch.nn.Linear (library GEMM, same arithmetic)."""
    if not (x.is_cuda and x.dtype == torch.bfloat16 and x.dim() == 3 and not torch.is_grad_enabled()):
        return None
    B, T = x.shape[:2]
    if T == 1 and B <= 4:
        return "gemv" if os.environ.get("TV_DECODE_FUSED", "1") != "0" else None
    if (((B == 1 and 2 <= T <= 16) or (T == 1 and 5 <= B <= 16)) and os.environ.get("TV_ROWS_FUSED", ROWS_FUSED_DEFAULT) != "0"
            and is_continuation(cache, cache_position)):
        return "rows"
    return None


def fused_route(model, hidden, cache, cache_position, output_hidden_states=False) -> Optional[str]:
    """The kernel a whole forward runs on, every block through its `step_fused` with the norms and activations in the
    prologues of the products: `linear_route` of the residual stream, where nothing asks for per-layer outputs or NaN
    checks, the hidden size is one the RMSNorm prologue holds and every matrix is bf16.  The decode step ("gemv") also needs
    a prefill behind it and committed tokens (`_speculate` has no conv epilogue)."""
    route = linear_route(hidden, cache, cache_position)
    H = hidden.shape[-1]
    if (route is None or output_hidden_states or model.check_nan or H % 8 or H > 8192
            or not model._all_matrices_bf16()):
        return None
    if route == "gemv" and (not is_continuation(cache, cache_position) or getattr(cache, "speculating", False)):
        return None
    return route


def fp8_copy(holder, params, x=None):
    """The e4m3 copy (w8, scale) `quantize_weights_e4m3` left on `holder` for the matrix made of `params`, or None: no copy,
    TV_FP8W=0 (read per call: bf16 without dropping anything), a copy whose key no longer matches its parameters (they
    were rewritten or moved: that matrix runs on bf16, nothing is re-quantized silently) or, given x, a shape
    tv_gemv_fp8w_fwd does not take."""
    ent = getattr(holder, "_fp8w", None)
    if ent is None or os.environ.get("TV_FP8W", "1") == "0" or ent[0] != K.param_key(params):
        return None
    if x is not None and not K.gemv_fp8w_takes(x, ent[1]):
        return None
    return ent[1], ent[2]


def _gemv_product(lin, x, weight, bias, prologue, fp8=None, **kw):
    """lin(x, weight, bias, prologue, ...), on the e4m3 copy `fp8` of the weight where `lin` is the decode step's
    matrix-vector kernel and the copy's kernel takes the shape."""
    if fp8 is not None and lin is K.gemv_fused and K.gemv_fp8w_takes(x, fp8[0]):
        return K.gemv_fp8w_fused(x, fp8[0], fp8[1], bias, prologue, **kw)
    return lin(x, weight, bias, prologue, **kw)


def _linear(mod: nn.Linear, x: torch.Tensor, route: Optional[str] = None) -> torch.Tensor:
    """mod(x) on the kernel of `route` (`linear_route` of x) where that kernel takes the shapes."""
    if route == "gemv":
        q = fp8_copy(mod, (mod.weight,), x)
        if q is not None:
            return K.gemv_fp8w_fused(x, q[0], q[1], mod.bias)
    if route == "gemv" and K.gemv_takes(x, mod.weight):
        return K.gemv_fused(x, mod.weight, mod.bias)
    if route == "rows" and K.linear_rows_takes(x, mod.weight):
        return K.linear_rows_fused(x, mod.weight, mod.bias)
    return mod(x)


def _norm_linear(lin, hidden, delta, norm, weight, bias, fp8=None, **kw):
    """A block's first product with its RMSNorm (+ the pending residual add, written to a new residual stream) in the
    prologue of `lin` (K.gemv_fused / K.linear_rows_fused; `fp8`: the weight's e4m3 copy, `_gemv_product`).  Returns
    (residual stream, product)."""
    new_hidden = torch.empty_like(hidden) if delta is not None else hidden
    y = _gemv_product(lin, hidden, weight, bias, K.GEMV_RMSNORM, fp8, delta=delta,
                      sum_out=new_hidden if delta is not None else None, norm_weight=norm.weight,
                      eps=norm.variance_epsilon, **kw)
    return new_hidden, y


# a continuation (T > 1 tokens behind a prefill) of up to this many tokens updates the SSM state in place, token by token
# inside one launch; longer ones run the chunked scan from the cached state.  Measured (devtools/bench_continue.py,
# profiles/continue_kernels.json, 9B dims): the largest T at which the sequence kernel is still the fastest of {itself,
# T single-token launches, the scan at L = T} — 26.6 us a layer against 28.4 us for the scan at T = 16, 49.5 against 29.5 at
# T = 32.  TV_CONTINUE_TSEQ overrides it (tests).
CONTINUE_T_SEQ = 16
CONTINUE_LAST_PATH = None      # "seq" / "scan": what the most recent Mamba continuation of this process ran on (tests)


def continue_t_seq() -> int:
    return int(os.environ.get("TV_CONTINUE_TSEQ", CONTINUE_T_SEQ))


# ------------------------------------------------------------------ layers
class MambaRMSNormGated(nn.Module):
    def __init__(self, hidden_size, group_size, eps=1e-5):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(hidden_size))
        self.variance_epsilon = eps
        self.group_size = group_size

    def forward(self, hidden_states, gate=None):
        return K.rmsnorm_fn(x=hidden_states, weight=self.weight, bias=None, z=gate,
                            eps=self.variance_epsilon, group_size=self.group_size,
                            norm_before_gate=False)


class NemotronHRMSNorm(nn.Module):
    def __init__(self, hidden_size, eps=1e-6):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(hidden_size))
        self.variance_epsilon = eps

    def forward(self, hidden_states, residual=None, return_sum=False):
        return K.rms_norm(hidden_states, self.weight, self.variance_epsilon, residual=residual,
                          return_sum=return_sum)


class NemotronHMamba2Mixer(nn.Module):
    """Reference :383-885.  forward() == cuda_kernels_forward's inference branches."""

    def __init__(self, config: NemotronHConfig, layer_idx: int):
        super().__init__()
        self.num_heads = config.mamba_num_heads
        self.hidden_size = config.hidden_size
        self.ssm_state_size = config.ssm_state_size
        self.conv_kernel_size = config.conv_kernel
        self.intermediate_size = config.mamba_num_heads * config.mamba_head_dim
        self.layer_idx = layer_idx
        self.use_conv_bias = config.use_conv_bias
        self.activation = config.mamba_hidden_act
        self.layer_norm_epsilon = config.layer_norm_epsilon
        self.n_groups = config.n_groups
        self.head_dim = config.mamba_head_dim
        self.chunk_size = config.chunk_size
        self.time_step_limit = tuple(config.time_step_limit)
        self.conv_dim = self.intermediate_size + 2 * self.n_groups * self.ssm_state_size
        self.conv1d = nn.Conv1d(self.conv_dim, self.conv_dim, bias=config.use_conv_bias,
                                kernel_size=config.conv_kernel, groups=self.conv_dim,
                                padding=config.conv_kernel - 1)
        projection_size = self.intermediate_size + self.conv_dim + self.num_heads
        self.in_proj = nn.Linear(self.hidden_size, projection_size, bias=config.use_bias)
        self.dt_bias = nn.Parameter(torch.ones(self.num_heads))
        self.A_log = nn.Parameter(torch.log(torch.arange(1, self.num_heads + 1).float()))
        self.norm = MambaRMSNormGated(self.intermediate_size, eps=self.layer_norm_epsilon,
                                      group_size=self.intermediate_size // self.n_groups)
        self.D = nn.Parameter(torch.ones(self.num_heads))
        self.out_proj = nn.Linear(self.intermediate_size, self.hidden_size, bias=config.use_bias)
        self.use_bias = config.use_bias
        self.group_map = "block"  # "tile" reproduces the reference CPU quirk (tests only)

    def _consts(self):
        """(-exp(A_log), D, dt_bias) in fp32 — what the scan kernels take (modeling_nano.py:640, :514-522).
        Derived once per parameter version, not once per call: in a bf16 model the per-call form costs five
        small launches a layer (float, exp, neg, two casts), 27 layers a forward, every decode step."""
        ps = (self.A_log, self.D, self.dt_bias)
        key = K.param_key(ps)
        if key != getattr(self, "_ckey", None):
            with torch.no_grad():
                self._cval = (-torch.exp(self.A_log.detach().float()), self.D.detach().float().contiguous(),
                              self.dt_bias.detach().float().contiguous())
            self._ckey = key
        return self._cval

    def _neg_A(self):
        return self._consts()[0]

    def forward(self, hidden_states, cache_params: Optional[HybridMambaAttentionDynamicCache] = None,
                cache_position=None, attention_mask=None, seq_idx=None,
                initial_states=None, conv_halo=None, return_shard_state=False):
        if seq_idx is not None:
            raise NotImplementedError("sequence packing (seq_idx) is a training feature")
        batch_size, seq_len, _ = hidden_states.shape
        if attention_mask is not None and attention_mask.shape[1] > 1 and attention_mask.shape[0] > 1:
            hidden_states = (hidden_states * attention_mask[:, :, None]).to(hidden_states.dtype)
        projected_states = self.in_proj(hidden_states)
        if is_continuation(cache_params, cache_position):
            gate, y = self._recur(cache_params, projected_states)
            return self.out_proj(self.norm(y, gate))
        d_in = self.intermediate_size
        gate, xBC, dt = projected_states.split([d_in, self.conv_dim, self.num_heads], dim=-1)
        w = self.conv1d.weight.squeeze(1)
        negA, D32, dtb32 = self._consts()

        if cache_params is not None:  # conv state = last K pre-conv inputs, (B, C, K)  (:596-610)
            Kw = self.conv_kernel_size
            xt = xBC.transpose(1, 2)
            cs = F.pad(xt, (Kw - seq_len, 0)) if seq_len < Kw else xt[..., -Kw:]
            cache_params.update_conv_state(self.layer_idx, cs.contiguous(), cache_init=True)
        # causal_conv1d_fn (:619-624) + the x|B|C split (:628-636) in one pass; B and C come
        # back as (B, L, G, N) views of group-major storage
        # (+ the scan's causal C.B^T fragments, multiplied while the B / C tiles are on the chip)
        x, Bm, Cm, cb = K.causal_conv1d_xbc(xBC, w, self.conv1d.bias, d_in, self.n_groups,
                                            self.ssm_state_size, activation=self.activation,
                                            halo=conv_halo, return_cb=True)
        dt_limit = {} if self.time_step_limit == (0.0, float("inf")) \
            else {"dt_limit": self.time_step_limit}
        res = K.mamba_chunk_scan_combined(
            x.view(batch_size, seq_len, -1, self.head_dim), dt, negA, Bm, Cm,
            chunk_size=self.chunk_size, D=D32,
            z=None, seq_idx=None, return_final_states=True, dt_bias=dtb32, dt_softplus=True,
            initial_states=initial_states, group_map=self.group_map,
            return_total_decay=return_shard_state, cb=cb, **dt_limit)
        scan_output, ssm_state = res[0], res[1]
        if cache_params is not None:
            cache_params.update_ssm_state(self.layer_idx, ssm_state)
        scan_output = self.norm(scan_output.view(batch_size, seq_len, -1), gate)
        out = self.out_proj(scan_output)
        if return_shard_state:
            return out, ssm_state, res[2]
        return out

    def _continue(self, cache_params, xBC, dt, w, negA, D32, dtb32):
        """T > 1 tokens behind a prefill (or earlier continuations / decode steps): the conv starts from the cached
        pre-conv rows, the recurrence from the cached state.  Up to `continue_t_seq()` tokens the state stays where it
        is (tv_selective_state_update_seq: every row read and written once); longer runs take the chunked scan with
        the cached state as its initial state.  Returns y in front of the gated norm."""
        global CONTINUE_LAST_PATH
        batch_size, seq_len, _ = xBC.shape
        d_in, Kw, idx = self.intermediate_size, self.conv_kernel_size, self.layer_idx
        conv_state = cache_params.conv_states[idx]                       # (B, C, K): the last K pre-conv rows
        halo = conv_state[..., 1:].transpose(1, 2)                       # (B, K-1, C)
        new_state = torch.cat([conv_state, xBC.transpose(1, 2).to(conv_state.dtype)], dim=-1)[..., -Kw:]
        scan = seq_len > continue_t_seq()
        out = K.causal_conv1d_xbc(xBC, w, self.conv1d.bias, d_in, self.n_groups, self.ssm_state_size,
                                  activation=self.activation, halo=halo, return_cb=scan)
        conv_state.copy_(new_state)                                      # (after the conv has read the halo)
        x, Bm, Cm = out[:3]
        x = x.view(batch_size, seq_len, -1, self.head_dim)
        if scan:
            dt_limit = {} if self.time_step_limit == (0.0, float("inf")) else {"dt_limit": self.time_step_limit}
            y, ssm_state = K.mamba_chunk_scan_combined(
                x, dt, negA, Bm, Cm, chunk_size=self.chunk_size, D=D32, z=None, seq_idx=None,
                return_final_states=True, dt_bias=dtb32, dt_softplus=True,
                initial_states=cache_params.ssm_states[idx], group_map=self.group_map, cb=out[3], **dt_limit)
            cache_params.update_ssm_state(idx, ssm_state)
        else:
            y = K.selective_state_update_seq(cache_params.ssm_states[idx], x, dt, negA, Bm, Cm, D=D32, dt_bias=dtb32,
                                             dt_softplus=True, dt_limit=self.time_step_limit, group_map=self.group_map)
        CONTINUE_LAST_PATH = "scan" if scan else "seq"
        return y.reshape(batch_size, seq_len, d_in)

    def _speculate(self, cache_params, projected_states, w, negA, D32, dtb32):
        """T >= 1 provisional tokens (cache.begin_speculation): the cache's conv / SSM states advance by the tokens KEPT
        of the previous forward only — the conv state by a gather, the SSM state inside the commit phase of
        tv_selective_state_update_spec — and this forward's tokens are computed from there without being stored.  Their
        operands stay in the cache's slot for the next forward's commit phase.  Returns y in front of the gated norm."""
        batch_size, seq_len, _ = projected_states.shape
        d_in, idx = self.intermediate_size, self.layer_idx
        sp = cache_params._spec
        cache_params.spec_commit_conv(idx)
        conv_state = cache_params.conv_states[idx]
        halo = conv_state[..., 1:].transpose(1, 2)                       # (B, K-1, C)
        prev = cache_params.spec_prev_operands(idx)
        xs, Bs, Cs, tail = cache_params._spec_views(idx, 0, seq_len)
        tail.copy_(projected_states[..., d_in:])                         # the pre-conv rows | dt, at a fixed address
        x, Bm, Cm = K.causal_conv1d_xbc_into(tail[..., :self.conv_dim], w, self.conv1d.bias, d_in, self.n_groups,
                                             self.ssm_state_size, (xs, Bs, Cs), activation=self.activation, halo=halo)
        new = (x.view(batch_size, seq_len, -1, self.head_dim), tail[..., self.conv_dim:], Bm, Cm)
        sp["flush"][idx] = {"A": negA, "dt_bias": dtb32, "dt_limit": self.time_step_limit, "group_map": self.group_map}
        y = K.selective_state_update_spec(cache_params.ssm_states[idx], prev, sp["n_commit"], new, negA, D=D32,
                                          dt_bias=dtb32, dt_softplus=True, dt_limit=self.time_step_limit,
                                          group_map=self.group_map)
        return y.reshape(batch_size, seq_len, d_in)

    def _decode(self, cache_params, xBC, dt, w, negA, D32, dtb32, conv_done=False):
        """One token per sequence: the conv update (unless the product's epilogue did it: `conv_done`), the x | B | C
        split, the state update.  Returns y in front of the gated norm."""
        batch_size = xBC.shape[0]
        d_in, gts, idx = self.intermediate_size, self.n_groups * self.ssm_state_size, self.layer_idx
        xBC = xBC[:, 0] if conv_done else K.causal_conv1d_update(xBC[:, 0], cache_params.conv_states[idx], w,
                                                                 self.conv1d.bias, self.activation)
        x, Bm, Cm = torch.split(xBC, [d_in, gts, gts], dim=-1)
        y = K.selective_state_update(
            cache_params.ssm_states[idx], x.reshape(batch_size, self.num_heads, self.head_dim), dt[:, 0], negA,
            Bm.reshape(batch_size, self.n_groups, -1), Cm.reshape(batch_size, self.n_groups, -1), D32, z=None,
            dt_bias=dtb32, dt_softplus=True)
        return y.reshape(batch_size, 1, d_in)

    def _recur(self, cache_params, projected_states, conv_done=False):
        """The tokens of a forward behind a prefill, from in_proj's output to the gated norm's operands (gate, y):
        provisional tokens, several committed ones, or one."""
        gate, xBC, dt = projected_states.split([self.intermediate_size, self.conv_dim, self.num_heads], dim=-1)
        w = self.conv1d.weight.squeeze(1)
        consts = self._consts()
        if getattr(cache_params, "speculating", False):
            return gate, self._speculate(cache_params, projected_states, w, *consts)
        if projected_states.shape[1] > 1:
            return gate, self._continue(cache_params, xBC, dt, w, *consts)
        return gate, self._decode(cache_params, xBC, dt, w, *consts, conv_done)

    def step_fused(self, lin, hidden, delta, norm, cache_params):
        """A forward behind a prefill with the block's RMSNorm (+ residual add) inside in_proj and the gated norm inside
        out_proj: in_proj -> `_recur` -> out_proj (one token: 3 launches).  Returns (residual stream, mixer output)."""
        conv = None
        if hidden.shape[1] == 1 and lin is K.gemv_fused:
            # one token on the gemv route: the conv update rides in the product's epilogue where the kernel offers it
            # (width 4, SiLU, K < 8192).  (One token of 5..16 sequences rides the rows kernel, which has no conv epilogue:
            # `_decode` then runs the conv update as its own launch.)
            conv_state, w = cache_params.conv_states[self.layer_idx], self.conv1d.weight.squeeze(1)
            if (self.conv_kernel_size == 4 and self.activation in ("silu", "swish") and hidden.shape[-1] < 8192
                    and conv_state.dtype == hidden.dtype and conv_state.is_contiguous() and w.is_contiguous()):
                conv = (conv_state, w, self.conv1d.bias, self.intermediate_size)
        new_hidden, proj = _norm_linear(lin, hidden, delta, norm, self.in_proj.weight, self.in_proj.bias,
                                        fp8=fp8_copy(self.in_proj, (self.in_proj.weight,)),
                                        **({} if conv is None else {"conv": conv}))
        gate, y = self._recur(cache_params, proj, conv_done=conv is not None)
        out = _gemv_product(lin, y, self.out_proj.weight, self.out_proj.bias, K.GEMV_GATED,
                            fp8_copy(self.out_proj, (self.out_proj.weight,)), norm_weight=self.norm.weight,
                            eps=self.norm.variance_epsilon, gate=gate, group_size=self.norm.group_size)
        return new_hidden, out


class ReLUSquared(nn.Module):
    def forward(self, x):
        return torch.square(F.relu(x))


class NemotronHMLP(nn.Module):
    def __init__(self, config, layer_idx: Optional[int] = None):
        super().__init__()
        self.config, self.layer_idx = config, layer_idx
        self.hidden_size, self.intermediate_size = config.hidden_size, config.intermediate_size
        self.up_proj = nn.Linear(self.hidden_size, self.intermediate_size, bias=config.mlp_bias)
        self.down_proj = nn.Linear(self.intermediate_size, self.hidden_size, bias=config.mlp_bias)
        assert config.mlp_hidden_act == "relu2"
        self.act_fn = ReLUSquared()

    def forward(self, x):
        # `act_fn` stays for the module tree; the activation runs as one in-place HIP pass
        return self.down_proj(K.relu2(self.up_proj(x), inplace=True))

    def step_fused(self, lin, hidden, delta, norm, cache_params=None):
        """RMSNorm (+ residual add) inside up_proj, relu^2 inside down_proj — 2 launches (the cache is not used)."""
        new_hidden, u = _norm_linear(lin, hidden, delta, norm, self.up_proj.weight, self.up_proj.bias,
                                     fp8=fp8_copy(self.up_proj, (self.up_proj.weight,)))
        return new_hidden, _gemv_product(lin, u, self.down_proj.weight, self.down_proj.bias, K.GEMV_RELU2,
                                         fp8_copy(self.down_proj, (self.down_proj.weight,)))


class NemotronHAttention(nn.Module):
    """Causal GQA attention without positional encoding (reference :1012-1220)."""

    def __init__(self, config: NemotronHConfig, layer_idx: Optional[int] = None):
        super().__init__()
        self.config, self.layer_idx = config, layer_idx
        self.hidden_size = config.hidden_size
        self.num_heads = config.num_attention_heads
        self.head_dim = config.head_dim if config.head_dim is not None \
            else config.hidden_size // config.num_attention_heads
        self.num_key_value_heads = config.num_key_value_heads
        self.num_key_value_groups = self.num_heads // self.num_key_value_heads
        self.is_causal = True
        b = config.attention_bias
        self.q_proj = nn.Linear(self.hidden_size, self.num_heads * self.head_dim, bias=b)
        self.k_proj = nn.Linear(self.hidden_size, self.num_key_value_heads * self.head_dim, bias=b)
        self.v_proj = nn.Linear(self.hidden_size, self.num_key_value_heads * self.head_dim, bias=b)
        self.o_proj = nn.Linear(self.head_dim * self.num_heads, self.hidden_size, bias=b)

    def forward(self, hidden_states, attention_mask=None, position_ids=None,
                past_key_value: Optional[HybridMambaAttentionDynamicCache] = None,
                output_attentions=False, use_cache=False, cache_position=None, **kwargs):
        if attention_mask is not None:
            raise NotImplementedError("padding masks are not on the inference path (mask is None "
                                      "under flash_attention_2, reference :2208-2213)")
        bsz, q_len, _ = hidden_states.size()
        cont = is_continuation(past_key_value, cache_position)
        route = linear_route(hidden_states, past_key_value, cache_position)
        q = _linear(self.q_proj, hidden_states, route).view(bsz, q_len, self.num_heads, self.head_dim)
        k = _linear(self.k_proj, hidden_states, route).view(bsz, q_len, self.num_key_value_heads, self.head_dim)
        v = _linear(self.v_proj, hidden_states, route).view(bsz, q_len, self.num_key_value_heads, self.head_dim)
        o = self._attend(q, k, v, past_key_value, cont)
        o = _linear(self.o_proj, o.reshape(bsz, q_len, self.num_heads * self.head_dim), route)
        return o, None, past_key_value

    def _attend(self, q, k, v, cache, continuation):
        """The new keys / values into the cache (if any) and the attention of the new queries over all of it."""
        q_len = q.shape[1]
        if getattr(cache, "is_branch_set", False):
            # one token of each branch of a shared prefix (llm/branch.py): the rows go into the branches' own suffix buffers,
            # the prefix is read once for all of them
            return K.flash_attn_branch(q, *cache.write(k, v, self.layer_idx))
        if continuation and getattr(cache, "speculating", False):
            return self._attend_provisional(q, k, v, cache)
        if cache is not None:
            k, v = cache.update(k, v, self.layer_idx)
        if cache is not None and q_len == 1 and cache.static_decode:
            # static decode: the whole buffers + the key count on the device (same launch parameters every token)
            kb, vb = cache.kv_buffers(self.layer_idx)
            return K.flash_attn_decode(q, kb, vb, seqlens_k=cache.decode_lens(self.layer_idx))
        if continuation and q_len > 1:
            # a continuation: the T new rows are in the cache, the T queries are its last T tokens (split-KV kernel)
            return K.flash_attn_append(q, k, v)
        return K._flash_attention_forward(q, k, v, attention_mask=None, query_length=q_len, is_causal=self.is_causal)

    def _attend_provisional(self, q, k, v, cache):
        """The attention of a speculative step: the T rows go behind the committed ones (rejected rows are overwritten by
        the next step), the key count comes from the device."""
        kb, vb = cache.kv_buffers(self.layer_idx)
        n = cache._spec["base"][self.layer_idx]
        rows = cache._spec["rows"][n]
        kb.index_copy_(1, rows, k)
        vb.index_copy_(1, rows, v)
        return K.flash_attn_append(q, kb, vb, seqlens_k=cache._spec["lens_t"][n])

    def _qkv_weight(self):
        """[q; k; v] as one (N, K) matrix for the decode token's single product (a copy: 64 MB per layer at 9B dims), rebuilt
        when a projection's storage or version changes."""
        ws = (self.q_proj.weight, self.k_proj.weight, self.v_proj.weight)
        key = K.param_key(ws)
        if getattr(self, "_qkv_key", None) != key:
            self._qkv_cat = torch.cat([w.detach() for w in ws], dim=0).contiguous()
            self._qkv_key = key
        return self._qkv_cat

    def step_fused(self, lin, hidden, delta, norm, cache):
        """A forward behind a prefill: the block's RMSNorm (+ residual add) in the prologue of ONE q / k / v product,
        the cache writes, split-KV attention, o_proj — one token: 4 launches + the cache writes, against 7."""
        B, T = hidden.shape[:2]
        nq, nkv = self.num_heads * self.head_dim, self.num_key_value_heads * self.head_dim
        # (the e4m3 copy of [q; k; v] is keyed by the three projections, as the bf16 concatenation is)
        new_hidden, qkv = _norm_linear(lin, hidden, delta, norm, self._qkv_weight(), None,
                                       fp8=fp8_copy(self, (self.q_proj.weight, self.k_proj.weight, self.v_proj.weight)))
        q, k, v = qkv.split([nq, nkv, nkv], dim=-1)
        q = q.view(B, T, self.num_heads, self.head_dim)
        k = k.view(B, T, self.num_key_value_heads, self.head_dim)
        v = v.view(B, T, self.num_key_value_heads, self.head_dim)
        o = self._attend(q, k, v, cache, True).reshape(B, T, nq)
        # (one token: `_linear`, which asks gemv_takes for the shape; several: the rows kernel takes every shape)
        return new_hidden, (_linear(self.o_proj, o, "gemv") if lin is K.gemv_fused else lin(o, self.o_proj.weight, None, K.GEMV_NONE))


NemotronHFlashAttention2 = NemotronHAttention
NemotronHSdpaAttention = NemotronHAttention
NEMOTRONH_ATTENTION_CLASSES = {"eager": NemotronHAttention,
                               "flash_attention_2": NemotronHFlashAttention2,
                               "sdpa": NemotronHSdpaAttention}


class Qwen2VLCrossAttention(nn.Module):
    """TransV merge module (reference merge_modules/cross_attention.py:65-324):
    text tokens (Q) attend non-causally to the dropped vision tokens (K, V)."""

    def __init__(self, config, layer_idx: Optional[int] = None):
        super().__init__()
        self.config, self.layer_idx = config, layer_idx
        self.hidden_size = config.hidden_size
        self.num_heads = config.num_attention_heads
        self.head_dim = config.head_dim if config.head_dim is not None \
            else config.hidden_size // config.num_attention_heads
        self.num_key_value_heads = config.num_key_value_heads
        self.num_key_value_groups = self.num_heads // self.num_key_value_heads
        self.is_causal = False
        b = config.attention_bias
        self.q_proj = nn.Linear(self.hidden_size, self.num_heads * self.head_dim, bias=b)
        self.k_proj = nn.Linear(self.hidden_size, self.num_key_value_heads * self.head_dim, bias=b)
        self.v_proj = nn.Linear(self.hidden_size, self.num_key_value_heads * self.head_dim, bias=b)
        self.o_proj = nn.Linear(self.num_heads * self.head_dim, self.hidden_size, bias=b)

    def forward(self, hidden_states, encoder_hidden_states, attention_mask=None,
                cross_attention_mask=None, **kwargs):
        if cross_attention_mask is not None:
            raise NotImplementedError("cross_attention_mask is never passed on the path (:1761-1765)")
        bsz, q_len, _ = hidden_states.size()
        kv_len = encoder_hidden_states.size(1)
        q = self.q_proj(hidden_states).view(bsz, q_len, self.num_heads, self.head_dim)
        k = self.k_proj(encoder_hidden_states).view(bsz, kv_len, self.num_key_value_heads, self.head_dim)
        v = self.v_proj(encoder_hidden_states).view(bsz, kv_len, self.num_key_value_heads, self.head_dim)
        o = K.flash_attn_func(q, k, v, causal=False)
        return self.o_proj(o.reshape(bsz, q_len, self.num_heads * self.head_dim)), None


Qwen2VLSdpaCrossAttention = Qwen2VLCrossAttention


class NemotronHBlock(nn.Module):
    def __init__(self, config, layer_idx):
        super().__init__()
        self.config, self.layer_idx = config, layer_idx
        self.residual_in_fp32 = config.residual_in_fp32
        if self.residual_in_fp32:
            # the reference upcasts the residual stream to fp32 (modeling_nano.py:942-943); the fused
            # residual-add + RMSNorm path here carries it in the activation dtype, so a config that
            # asks for fp32 residuals must not run silently with different arithmetic
            raise NotImplementedError("residual_in_fp32=True is not implemented (the checkpoints on the "
                                      "evaluation path, Nemotron-Nano-9B-v2, use False)")
        self.norm = NemotronHRMSNorm(config.hidden_size, eps=config.layer_norm_epsilon)
        self.block_type = config.layers_block_type[layer_idx]
        if self.block_type == "mamba":
            self.mixer = NemotronHMamba2Mixer(config, layer_idx=layer_idx)
        elif self.block_type == "attention":
            self.mixer = NEMOTRONH_ATTENTION_CLASSES[config._attn_implementation](config, layer_idx=layer_idx)
        elif self.block_type == "mlp":
            self.mixer = NemotronHMLP(config, layer_idx=layer_idx)
        else:
            raise ValueError(f"Invalid layer pattern {config.hybrid_override_pattern[layer_idx]}")

    def mix(self, normed, cache_params=None, cache_position=None, attention_mask=None,
            position_ids=None):
        if self.block_type == "mamba":
            return self.mixer(normed, cache_params=cache_params, cache_position=cache_position)
        if self.block_type == "attention":
            return self.mixer(normed, past_key_value=cache_params, cache_position=cache_position,
                              attention_mask=attention_mask, position_ids=position_ids)[0]
        return self.mixer(normed)

    def forward(self, hidden_states, cache_params=None, cache_position=None, attention_mask=None,
                seq_idx=None, position_ids=None):
        residual = hidden_states
        normed = self.norm(hidden_states.to(dtype=self.norm.weight.dtype))
        out = self.mix(normed, cache_params, cache_position, attention_mask, position_ids)
        return residual + out


# --------------------------------------------------------------------- model
class NemotronHModel(PdropMixin, nn.Module):
    """Reference :1449-2273 (inference paths)."""

    def __init__(self, config: NemotronHConfig):
        super().__init__()
        self.config = config
        self.embeddings = nn.Embedding(config.vocab_size, config.hidden_size)
        self.layers = nn.ModuleList([NemotronHBlock(config, layer_idx=i)
                                     for i in range(config.num_hidden_layers)])
        self.use_pdrop = config.use_pdrop
        self.pdrop_args: Dict[str, Any] = {"use_pdrop": config.use_pdrop}
        self.pdrop_types = None
        if self.use_pdrop:
            assert config.pdrop_type is not None, "use_pdrop is True, but pdrop_type is not set"
            self.pdrop_types = [t.split("_") for t in config.pdrop_type.split("-")]
            assert all(len(t) == 3 for t in self.pdrop_types), \
                "pdrop_type should be like 'type_layernum_ratio-...' "
            self.pdrop_args.update({
                "pdrop_compress_types": [t[0] for t in self.pdrop_types],
                "pdrop_layers": [int(t[1]) for t in self.pdrop_types],
                "pdrop_ratios": [1] + [float(t[2]) for t in self.pdrop_types]})
            # the reference injects these later through set_pdrop_args (:2459-2462)
            self.pdrop_compress_types = self.pdrop_args["pdrop_compress_types"]
            self.pdrop_layers = self.pdrop_args["pdrop_layers"]
            self.pdrop_ratios = self.pdrop_args["pdrop_ratios"]
        if config.merge_module == "CrossAttention":
            self.merge_module_names, mods = [], []
            for i, _ in enumerate(self.pdrop_args.get("pdrop_layers", [])):
                if "drop" in self.pdrop_args["pdrop_compress_types"][i]:
                    self.merge_module_names.append("none")
                    mods.append(nn.Identity())
                else:
                    self.merge_module_names.append("attention")
                    mods.append(Qwen2VLSdpaCrossAttention(
                        config, layer_idx=self.pdrop_args["pdrop_layers"][i]))
            self.merge_modules = nn.ModuleList(mods)
            self.alpha = nn.Parameter(torch.zeros(
                sum(1 for m in self.merge_modules if not isinstance(m, nn.Identity))))
        elif config.merge_module == "no_merge":
            self.merge_modules, self.alpha = None, None
        else:
            raise ValueError(f"Invalid merge module name: {config.merge_module}")
        self.merge_ffn_modules, self.alpha_ffn = None, None
        self.norm_f = NemotronHRMSNorm(config.hidden_size, eps=config.layer_norm_epsilon)
        self.check_nan = False
        self.last_pdrop_trace: List[Dict[str, torch.Tensor]] = []
        self._register_load_state_dict_pre_hook(self.load_hook)

    @staticmethod
    def load_hook(state_dict, prefix, *args):
        for k in list(state_dict):
            if "embedding." in k:
                state_dict[k.replace("embedding.", "embeddings.")] = state_dict.pop(k)
                break

    def get_input_embeddings(self):
        return self.embeddings

    def set_input_embeddings(self, new_embeddings):
        self.embeddings = new_embeddings

    def _all_matrices_bf16(self) -> bool:
        """Every 2-D parameter of every block is dense bf16 — what the fused decode step's matrix-vector kernel takes (its
        C ABI carries no weight dtype).  Decided once per parameter set (`_apply` — .to() / .bfloat16() — and
        load_state_dict replace or rewrite the parameters: both reset it)."""
        ok = getattr(self, "_bf16_ok", None)
        if ok is None:
            ok = all(p.dtype == torch.bfloat16 and p.stride(-1) == 1
                     for blk in self.layers for p in blk.mixer.parameters() if p.dim() == 2)
            self._bf16_ok = ok
        return ok

    def _apply(self, fn, *a, **kw):
        self._bf16_ok = None
        return super()._apply(fn, *a, **kw)

    def load_state_dict(self, *a, **kw):
        self._bf16_ok = None
        return super().load_state_dict(*a, **kw)

    def _rank_attention(self, rank_layer):
        """the self-attention module whose q/k projections rank the vision tokens (:1822-1830)"""
        assert self.layers[rank_layer].block_type == "attention"
        return self.layers[rank_layer].mixer

    def forward(self, input_ids=None, inputs_embeds=None, position_ids=None, past_key_values=None,
                use_cache=None, output_attentions=None, output_hidden_states=None,
                return_dict=None, cache_position=None, attention_mask=None, **kwargs):
        if (input_ids is None) ^ (inputs_embeds is not None):
            raise ValueError("You must specify exactly one of input_ids or inputs_embeds")
        if inputs_embeds is None:
            inputs_embeds = self.embeddings(input_ids)
        if attention_mask is not None:
            if self.config._attn_implementation == "flash_attention_2":
                raise ValueError("attention_mask must be None if using flash_attention_2")
            raise NotImplementedError("only the mask-free flash_attention_2 path is implemented")
        use_cache = use_cache if use_cache is not None else self.config.use_cache
        hidden = inputs_embeds
        if cache_position is None:
            cache_position = torch.arange(hidden.shape[1], device=hidden.device)
        if position_ids is None:
            position_ids = cache_position.unsqueeze(0)
            if position_ids.shape[1] == 1 and hidden.shape[1] > 1:      # a continuation given its first position only
                position_ids = position_ids + torch.arange(hidden.shape[1], device=position_ids.device)
        labels = kwargs.get("labels", None)
        all_hidden = () if output_hidden_states else None
        train_pdrop_args = kwargs.get("train_pdrop_args")
        self.last_pdrop_trace = []
        delta = None  # pending mixer output, added inside the next fused norm
        continuation = is_continuation(past_key_values, cache_position)
        if continuation and hidden.shape[1] > 1 and getattr(past_key_values, "static_decode", False):
            raise RuntimeError("continuation: the cache is in static-decode mode (fixed buffers, one token per step); "
                               "call cache.end_static_decode() before appending several tokens")
        speculating = continuation and getattr(past_key_values, "speculating", False)
        if getattr(past_key_values, "speculating", False) and not continuation:
            raise RuntimeError("speculation: the cache takes continuations only (cache_position > 0)")
        if speculating:
            if hidden.shape[1] > continue_t_seq():
                raise RuntimeError(f"speculation: {hidden.shape[1]} tokens in one forward, more than continue_t_seq() = "
                                   f"{continue_t_seq()} (the range of the in-register recurrence)")
            past_key_values.spec_begin_forward(hidden.shape[1])
        # a decode step / a few tokens behind a prefill: every block's norm (+ add) and activation run in the prologues of
        # its products (`fused_route`); resolved per call, so that a replaced K.gemv_fused / K.linear_rows_fused is seen
        route = fused_route(self, hidden, past_key_values, cache_position, output_hidden_states)
        lin = getattr(K, {"gemv": "gemv_fused", "rows": "linear_rows_fused"}[route]) if route else None
        # attention blocks join when their projections carry no bias (the stacked q / k / v product takes none)
        attn_fused = not self.config.attention_bias
        for layer_idx, block in enumerate(self.layers):
            if self.use_pdrop and train_pdrop_args is not None \
                    and layer_idx in self.pdrop_layers \
                    and train_pdrop_args.get("is_interleaved", False) is False:
                stage = self.pdrop_layers.index(layer_idx)
                # ranking and dropping belong to the prefill: a continuation of any length carries no vision tokens
                if hidden.shape[1] != 1 and not continuation:
                    if delta is not None:
                        hidden, delta = hidden + delta, None
                    position_ids, attention_mask, hidden, labels, _ = self.flash_rank_drop(
                        cur_num=stage, rank_layer=layer_idx, features=hidden,
                        position_ids=position_ids, attention_mask=attention_mask, labels=labels,
                        train_pdrop_args=train_pdrop_args)
                else:  # decode / continuation: shift positions by the tokens dropped at this stage (:1666-1689)
                    nv = train_pdrop_args["num_vision_tokens"][0]
                    position_ids = position_ids - (int(nv * self.pdrop_ratios[stage])
                                                   - int(nv * self.pdrop_ratios[stage + 1]))
            if self.check_nan and torch.isnan(hidden).any():
                raise ValueError("NaN detected in hidden_states before mixer block")
            if output_hidden_states:
                all_hidden += ((hidden if delta is None else hidden + delta),)
            # x_{i+1} = x_i + mixer(norm(x_i)); the add of layer i-1 is fused into this norm
            if route and (block.block_type != "attention" or attn_fused):
                hidden, delta = block.mixer.step_fused(lin, hidden, delta, block.norm, past_key_values)
                continue
            if delta is None:
                normed = block.norm(hidden)
            else:
                normed, hidden = block.norm(hidden, residual=delta, return_sum=True)
            delta = block.mix(normed, past_key_values, cache_position, None, position_ids)
        hidden = self.norm_f(hidden, residual=delta) if delta is not None else self.norm_f(hidden)
        if speculating:
            past_key_values.spec_end_forward(hidden.shape[1])
        if output_hidden_states:
            all_hidden += (hidden,)
        return BaseModelOutputWithPastAndLabels(
            last_hidden_state=hidden, past_key_values=past_key_values if use_cache else None,
            hidden_states=all_hidden, attentions=None, labels=labels)


class NemotronHForCausalLM(nn.Module):
    """Reference :2283-2504."""

    def __init__(self, config: NemotronHConfig):
        super().__init__()
        self.config = config
        self.backbone = NemotronHModel(config)
        self.vocab_size = config.vocab_size
        self.lm_head = nn.Linear(config.hidden_size, config.vocab_size, bias=False)
        self.apply(self._init_weights)

    def _init_weights(self, module):
        """Reference :1339-1383."""
        cfg = self.config
        if isinstance(module, NemotronHMamba2Mixer):
            dt = torch.exp(torch.rand(cfg.mamba_num_heads)
                           * (math.log(cfg.time_step_max) - math.log(cfg.time_step_min))
                           + math.log(cfg.time_step_min)).clamp(min=cfg.time_step_floor)
            with torch.no_grad():
                module.dt_bias.copy_(dt + torch.log(-torch.expm1(-dt)))
        if isinstance(module, nn.Linear) and module.bias is not None:
            nn.init.zeros_(module.bias)
        elif isinstance(module, nn.Embedding):
            nn.init.normal_(module.weight, std=cfg.initializer_range)

    @property
    def device(self):
        return self.lm_head.weight.device

    @property
    def dtype(self):
        return self.lm_head.weight.dtype

    def get_input_embeddings(self):
        return self.backbone.get_input_embeddings()

    def set_input_embeddings(self, new_embeddings):
        return self.backbone.set_input_embeddings(new_embeddings)

    def get_output_embeddings(self):
        return self.lm_head

    def new_cache(self, batch_size=1, dtype=None, device=None):
        return HybridMambaAttentionDynamicCache(self.config, batch_size, dtype=dtype or self.dtype,
                                                device=device or self.device)

    # ------------------------------------------------------------------ decode on e4m3 weights
    def _fp8_linears(self):
        """(holder, parameters) of every matrix `quantize_weights_e4m3` covers: each nn.Linear of the blocks' mixers, and
        lm_head unless it is tied to the embeddings.  Embeddings, norms, the conv and A / D / dt are never touched."""
        out = [(m, (m.weight,)) for blk in self.backbone.layers for m in blk.mixer.modules() if isinstance(m, nn.Linear)]
        emb = self.backbone.embeddings.weight
        head = self.lm_head.weight
        if head is not emb and head.data_ptr() != emb.data_ptr():
            out.append((self.lm_head, (head,)))
        return out

    @torch.no_grad()
    def quantize_weights_e4m3(self) -> int:
        """Round every linear weight of the blocks (and an untied lm_head) to e4m3 with one power-of-two scale per output
        row (K.quantize_rows_e4m3), IN PLACE: the bf16 weight becomes the dequantized matrix — exact in bf16 — and the
        (e4m3, scale) pair is kept beside it for the decode step's 1..4-row products (tv_gemv_fp8w_fwd: the same numbers
        at half the bytes).  Every other route — prefill, continuation, the speculative verify forward, the rows kernel,
        the library GEMM — computes with the rounded bf16 weights on the kernels it uses anyway, so the model stays one
        model.  The original weights are gone: reload to get them back.  Returns the number of matrices quantized."""
        pairs = self._fp8_linears()
        for mod, (w,) in pairs:
            if w.dtype != torch.bfloat16 or w.dim() != 2:
                raise TypeError(f"quantize_weights_e4m3: bf16 matrices only (found {w.dtype} {tuple(w.shape)}); "
                                "convert the model with .bfloat16() first")
        for mod, (w,) in pairs:
            w8, scale = K.quantize_rows_e4m3(w)
            w.copy_(K.dequantize_rows_e4m3(w8, scale))
            mod._fp8w = (K.param_key((w,)), w8, scale)         # (the key AFTER the write: it bumps the version)
        for blk in self.backbone.layers:
            att = blk.mixer
            if isinstance(att, NemotronHAttention) and not self.config.attention_bias:
                # the decode token's single [q; k; v] product: scales are per row, so the copy is the concatenation
                projs = (att.q_proj, att.k_proj, att.v_proj)
                w8 = torch.cat([p._fp8w[1] for p in projs], dim=0).contiguous()
                scale = torch.cat([p._fp8w[2] for p in projs], dim=0).contiguous()
                att._fp8w = (K.param_key(tuple(p.weight for p in projs)), w8, scale)
        self._fp8_quantized = True
        return len(pairs)

    def drop_fp8_weights(self) -> None:
        """Free the e4m3 copies; the rounded bf16 weights stay (the decode step streams them again)."""
        for m in self.modules():
            if getattr(m, "_fp8w", None) is not None:
                m._fp8w = None
        self._fp8_quantized = False

    def has_fp8_weights(self) -> bool:
        return bool(getattr(self, "_fp8_quantized", False))

    def _apply(self, fn, *a, **kw):
        self.drop_fp8_weights()          # (.to() / .bfloat16(): the parameters move or change, the copies would not follow)
        return super()._apply(fn, *a, **kw)

    def load_state_dict(self, *a, **kw):
        self.drop_fp8_weights()
        return super().load_state_dict(*a, **kw)

    def set_pdrop_args(self, **kwargs):
        for key, value in kwargs.items():
            setattr(self.backbone, key, value)

    def init_cross_attn_from_self_attn(self):
        if self.backbone.merge_modules is not None:
            layers = self.backbone.pdrop_args.get("pdrop_layers", [])
            for idx, module in enumerate(self.backbone.merge_modules):
                if not isinstance(module, nn.Identity):
                    module.load_state_dict(self.backbone.layers[layers[idx]].mixer.state_dict())

    def forward(self, input_ids=None, inputs_embeds=None, position_ids=None, past_key_values=None,
                labels=None, output_attentions=None, output_hidden_states=None, return_dict=None,
                use_cache=None, cache_position=None, attention_mask=None, logits_to_keep=None,
                **kwargs):
        out = self.backbone(input_ids, past_key_values=past_key_values, inputs_embeds=inputs_embeds,
                            position_ids=position_ids, output_hidden_states=output_hidden_states,
                            use_cache=use_cache, cache_position=cache_position,
                            attention_mask=attention_mask, labels=labels, **kwargs)
        hidden = out.last_hidden_state
        if labels is not None:
            raise NotImplementedError("loss computation is a training feature")
        # reference computes lm_head over all L positions (:2433); generate() needs [:, -1]
        keep = self.config.num_logits_to_keep if logits_to_keep is None else logits_to_keep
        if isinstance(keep, int) and keep > 0:
            hidden = hidden[:, -keep:]
        hidden = hidden.to(self.lm_head.weight.dtype)
        logits = _linear(self.lm_head, hidden, linear_route(hidden, past_key_values, cache_position)).float()
        return CausalLMOutputWithPast(loss=None, logits=logits, past_key_values=out.past_key_values,
                                      hidden_states=out.hidden_states)
