"""Continuation of a prefilled hybrid cache with several tokens in one forward — host logic, no GPU.

The identity under test: a prefill of n tokens followed by a continuation of T tokens produces, at the T new positions,
what one forward over all n + T tokens produces there, and leaves the same cache as T single-token steps.  Kernels are the
oracle-backed stand-ins of `cpu_kernel_shim` plus, here, one for `kernels.selective_state_update_seq` (the fp64 token
recurrence started from the cached state).  Both sides of every comparison run the same fp64-backed operators on an fp32
model and differ only in summation order: the bound is rtol 1e-4 / atol 8e-5, what tests/test_model_cpu.py allows fp32
toy-model logits against the reference."""
import contextlib
import re
from pathlib import Path

import pytest
import torch

from cpu_kernel_shim import cpu_kernels
from oracle import ops as R
from timeviper_amd.model.llm import nano
from timeviper_amd.model.llm.nano import HybridMambaAttentionDynamicCache, NemotronHConfig, NemotronHForCausalLM

ROOT = Path(__file__).resolve().parent.parent
RTOL, ATOL = 1e-4, 8e-5


def _seq(state, x, dt, A, B, C, D=None, dt_bias=None, dt_softplus=False, dt_limit=(0.0, float("inf")),
         group_map="block"):
    y, fin, _ = R.ssd_recurrence_ref(x, dt, A, B, C, D=D, dt_bias=dt_bias, dt_softplus=dt_softplus, dt_limit=dt_limit,
                                     initial_states=state, group_map=group_map)
    state.copy_(fin.to(state.dtype))
    return y.to(x.dtype)


APPEND_CALLS = []


def _append(q, k, v, seqlens_k=None, softmax_scale=None, return_lse=False):
    assert seqlens_k is None and 1 < q.shape[1] <= k.shape[1]
    APPEND_CALLS.append((q.shape[1], k.shape[1]))
    o, lse = R.attention_ref(q, k, v, True, softmax_scale)
    return (o.to(q.dtype), lse) if return_lse else o.to(q.dtype)


@contextlib.contextmanager
def kernels_cpu():
    from timeviper_amd import kernels as K
    with cpu_kernels():
        saved = K.selective_state_update_seq, K.flash_attn_append
        K.selective_state_update_seq, K.flash_attn_append = _seq, _append
        try:
            yield
        finally:
            K.selective_state_update_seq, K.flash_attn_append = saved


def _cfg(pattern="M*-M*-M", **kw):
    base = dict(vocab_size=64, hidden_size=32, intermediate_size=48, num_hidden_layers=len(pattern),
                hybrid_override_pattern=pattern, num_attention_heads=2, head_dim=16, num_key_value_heads=1,
                ssm_state_size=8, mamba_num_heads=4, mamba_n_groups=2, mamba_head_dim=8, mamba_chunk_size=8)
    base.update(kw)
    return NemotronHConfig(**base)


def _model(cfg, seed=0):
    torch.manual_seed(seed)
    return NemotronHForCausalLM(cfg).float().eval()


def _prefill(model, ids, **kw):
    cache = HybridMambaAttentionDynamicCache(model.config, 1, dtype=torch.float32)
    out = model(input_ids=ids, past_key_values=cache, use_cache=True, cache_position=torch.zeros(1, dtype=torch.long),
                logits_to_keep=0, **kw)
    return cache, out.logits


def _assert_same_cache(a, b, cfg):
    for i, c in enumerate(cfg.hybrid_override_pattern):
        if c == "M":
            torch.testing.assert_close(a.conv_states[i], b.conv_states[i], rtol=RTOL, atol=ATOL)
            torch.testing.assert_close(a.ssm_states[i], b.ssm_states[i], rtol=RTOL, atol=ATOL)
        elif c == "*":
            assert a.key_cache[i].shape == b.key_cache[i].shape
            torch.testing.assert_close(a.key_cache[i], b.key_cache[i], rtol=RTOL, atol=ATOL)
            torch.testing.assert_close(a.value_cache[i], b.value_cache[i], rtol=RTOL, atol=ATOL)


@pytest.mark.parametrize("T", [2, 3, 4, 7, 40])
def test_continuation_equals_full_forward_and_single_steps(T):
    cfg = _cfg()
    model = _model(cfg)
    n = 21
    ids = torch.randint(0, cfg.vocab_size, (1, n + T), generator=torch.Generator().manual_seed(T))
    with torch.no_grad(), kernels_cpu():
        full = model(input_ids=ids, logits_to_keep=0).logits
        cache, pre = _prefill(model, ids[:, :n])
        torch.testing.assert_close(pre, full[:, :n], rtol=RTOL, atol=ATOL)
        steps, fork = cache.clone(), cache.clone()
        assert steps.get_seq_length() == n and steps.key_cache[1].data_ptr() != cache.key_cache[1].data_ptr()
        APPEND_CALLS.clear()
        cont = model(input_ids=ids[:, n:], past_key_values=cache, use_cache=True, cache_position=torch.tensor([n]),
                     logits_to_keep=T).logits
        assert APPEND_CALLS == [(T, n + T)] * 2             # both attention layers, the prefill and the steps none
        assert cont.shape == (1, T, cfg.vocab_size)
        last = model(input_ids=ids[:, n:], past_key_values=fork, use_cache=True,
                     cache_position=torch.tensor([n])).logits
        single = [model(input_ids=ids[:, t:t + 1], past_key_values=steps, use_cache=True,
                        cache_position=torch.tensor([t])).logits[:, -1] for t in range(n, n + T)]
    torch.testing.assert_close(cont, full[:, n:], rtol=RTOL, atol=ATOL)
    torch.testing.assert_close(cont, torch.stack(single, dim=1), rtol=RTOL, atol=ATOL)
    assert last.shape == (1, 1, cfg.vocab_size)                          # the default stays the last position
    torch.testing.assert_close(last[:, 0], cont[:, -1], rtol=RTOL, atol=ATOL)
    _assert_same_cache(cache, steps, cfg)
    assert all(cache.key_cache[i].shape[1] == n + T for i in cache.attention_layers)


def test_both_sides_of_t_seq_agree(monkeypatch):
    cfg = _cfg()
    model = _model(cfg, 1)
    n, T = 13, 9
    ids = torch.randint(0, cfg.vocab_size, (1, n + T), generator=torch.Generator().manual_seed(3))
    res = {}
    with torch.no_grad(), kernels_cpu():
        for name, tseq in (("seq", "64"), ("scan", "1")):
            monkeypatch.setenv("TV_CONTINUE_TSEQ", tseq)
            cache, _ = _prefill(model, ids[:, :n])
            logits = model(input_ids=ids[:, n:], past_key_values=cache, use_cache=True,
                           cache_position=torch.arange(n, n + T), logits_to_keep=0).logits
            assert nano.CONTINUE_LAST_PATH == name
            res[name] = (logits, cache)
    torch.testing.assert_close(res["seq"][0], res["scan"][0], rtol=RTOL, atol=ATOL)
    _assert_same_cache(res["seq"][1], res["scan"][1], cfg)


def test_two_continuations_then_steps():
    """prefill + continue + continue + single steps walk the same cache as one forward"""
    cfg = _cfg("MM*-")
    model = _model(cfg, 2)
    ids = torch.randint(0, cfg.vocab_size, (1, 30), generator=torch.Generator().manual_seed(4))
    with torch.no_grad(), kernels_cpu():
        full = model(input_ids=ids, logits_to_keep=0).logits
        cache, _ = _prefill(model, ids[:, :10])
        a = model(input_ids=ids[:, 10:12], past_key_values=cache, cache_position=torch.tensor([10]), logits_to_keep=0).logits
        b = model(input_ids=ids[:, 12:27], past_key_values=cache, cache_position=torch.tensor([12]), logits_to_keep=0).logits
        c = [model(input_ids=ids[:, t:t + 1], past_key_values=cache, cache_position=torch.tensor([t])).logits
             for t in range(27, 30)]
    torch.testing.assert_close(torch.cat([a, b] + c, dim=1), full[:, 10:], rtol=RTOL, atol=ATOL)


def test_token_drop_stage_takes_its_decode_branch_for_any_length():
    pd = "uni_2_0.75-attn_4_0.5"
    cfg = _cfg("M-*M*-M", use_pdrop=True, pdrop_type=pd)
    model = _model(cfg, 3)
    tb, nv, ta, T = 3, 16, 4, 5
    pa = {"first_vision_token_positions": torch.tensor([tb]), "text_prompt_lens": [tb + ta], "num_vision_tokens": [nv],
          "is_interleaved": False}
    g = torch.Generator().manual_seed(5)
    ids = torch.randint(0, cfg.vocab_size, (1, tb + nv + ta + T), generator=g)
    n = tb + nv + ta
    with torch.no_grad(), kernels_cpu():
        cache, _ = _prefill(model, ids[:, :n], train_pdrop_args=pa)
        assert len(model.backbone.last_pdrop_trace) == 2
        before = {i: cache.key_cache[i].shape[1] for i in cache.attention_layers}
        assert before == {2: n - nv + int(nv * 0.75), 4: n - nv + int(nv * 0.5)}
        steps = cache.clone()
        cont = model(input_ids=ids[:, n:], past_key_values=cache, cache_position=torch.tensor([n]),
                     train_pdrop_args=pa, logits_to_keep=0).logits
        assert model.backbone.last_pdrop_trace == []
        single = [model(input_ids=ids[:, t:t + 1], past_key_values=steps, cache_position=torch.tensor([t]),
                        train_pdrop_args=pa).logits[:, -1] for t in range(n, n + T)]
    assert {i: cache.key_cache[i].shape[1] for i in cache.attention_layers} == {i: v + T for i, v in before.items()}
    torch.testing.assert_close(cont, torch.stack(single, dim=1), rtol=RTOL, atol=ATOL)
    _assert_same_cache(cache, steps, cfg)


def test_static_decode_cache_must_be_released_first():
    cfg = _cfg()
    model = _model(cfg)
    ids = torch.randint(0, cfg.vocab_size, (1, 12), generator=torch.Generator().manual_seed(6))
    with torch.no_grad(), kernels_cpu():
        cache, _ = _prefill(model, ids[:, :8])
        cache.begin_static_decode(8)
        with pytest.raises(RuntimeError, match="end_static_decode"):
            model(input_ids=ids[:, 8:], past_key_values=cache, cache_position=torch.tensor([8]))
        cache.end_static_decode()
        model(input_ids=ids[:, 8:], past_key_values=cache, cache_position=torch.tensor([8]))
    assert cache.get_seq_length() == 12


def test_qwen2_rotary_positions_of_a_continuation(monkeypatch):
    from timeviper_amd.model.llm.qwen2 import Qwen2Config, Qwen2ForCausalLM
    cfg = Qwen2Config(vocab_size=64, hidden_size=32, intermediate_size=48, num_hidden_layers=3, num_attention_heads=2,
                      num_key_value_heads=1, use_pdrop=True, pdrop_type="uni_1_0.5")
    torch.manual_seed(0)
    model = Qwen2ForCausalLM(cfg).float().eval()
    tb, nv, ta, T = 2, 8, 3, 4
    n = tb + nv + ta
    pa = {"first_vision_token_positions": torch.tensor([tb]), "text_prompt_lens": [tb + ta], "num_vision_tokens": [nv],
          "is_interleaved": False}
    ids = torch.randint(0, 64, (1, n + T), generator=torch.Generator().manual_seed(1))
    seen = []
    orig = model.model.rotary_emb.forward

    def spy(x, position_ids):
        seen.append(position_ids.clone())
        return orig(x, position_ids)
    monkeypatch.setattr(model.model.rotary_emb, "forward", spy)
    with torch.no_grad(), kernels_cpu():
        out = model(input_ids=ids[:, :n], use_cache=True, train_pdrop_args=pa)
        cache = out.past_key_values
        import copy
        steps = copy.deepcopy(cache)
        seen.clear()
        cont = model(input_ids=ids[:, n:], past_key_values=cache, use_cache=True, train_pdrop_args=pa).logits
        cont_pos = [p.clone() for p in seen]
        step_pos, single = [], []
        for t in range(n, n + T):
            seen.clear()
            single.append(model(input_ids=ids[:, t:t + 1], past_key_values=steps, use_cache=True,
                                train_pdrop_args=pa).logits[:, -1])
            step_pos.append([p.clone() for p in seen])
    assert model.model.last_pdrop_trace == [] and cont.shape[1] == T
    assert len(cont_pos) == 2                                    # before and behind the drop stage
    for k in range(2):
        assert torch.equal(cont_pos[k], torch.cat([sp[k] for sp in step_pos], dim=1))
    assert torch.equal(cont_pos[0], torch.arange(n, n + T)[None]) and torch.equal(cont_pos[1], cont_pos[0] - nv // 2)
    assert cache.key_cache[0].shape[1] == n + T and cache.key_cache[2].shape[1] == n - nv // 2 + T
    torch.testing.assert_close(cont, torch.stack(single, dim=1), rtol=RTOL, atol=ATOL)


def _toy_vlm(seed=3):
    from timeviper_amd.model import HybridTimeViperVLM, get_llm_backbone_and_tokenizer
    from timeviper_amd.model.vit import TimmViTBackbone
    torch.manual_seed(seed)
    cfg = NemotronHConfig(vocab_size=128, hidden_size=64, intermediate_size=96, num_hidden_layers=8,
                          hybrid_override_pattern="M-M*M-*M", num_attention_heads=4, head_dim=16,
                          num_key_value_heads=2, ssm_state_size=16, mamba_num_heads=8,
                          mamba_n_groups=2, mamba_head_dim=8, mamba_chunk_size=16)
    vb = TimmViTBackbone("siglip-vit-b16-224px", depth_override=2, default_image_size=96)
    llm, tokenizer = get_llm_backbone_and_tokenizer(
        "nanov2-9b", llm_max_length=None, attn_implementation="flash_attention_2",
        merge_module="no_merge", use_pdrop=True, pdrop_type="uni_2_0.75-uni_6_0.5", config=cfg)
    vlm = HybridTimeViperVLM("toy", vb, llm, arch_specifier="tome_mlp-16").float().eval()
    with torch.no_grad():
        vlm.llm_backbone.llm.lm_head.weight.mul_(20.0)           # spread the logits: no near-ties under greedy decoding
    return vlm, tokenizer


def test_generate_two_turns_equal_one_transcript():
    vlm, tokenizer = _toy_vlm()
    T, tok = 4, vlm.default_token_id
    ids1 = torch.tensor([[5, 6] + [tok] * T + [7, 8, 9]])
    ids2 = torch.tensor([[10, 11, 12, 13, 14]])
    pix = torch.randn(T, 3, 96, 96, generator=torch.Generator().manual_seed(0))
    kw = dict(max_new_tokens=4, return_ids=True, eos_token_id=-1)
    with kernels_cpu():
        plain = vlm.generate(ids1, pixel_values_videos=pix, **kw)
        first, cache = vlm.generate(ids1, pixel_values_videos=pix, return_past_key_values=True, **kw)
        assert isinstance(plain, torch.Tensor) and torch.equal(plain, first)          # the default call is unchanged
        assert cache.pending_ids.numel() == 0                                         # every emitted id was fed
        fork = cache.clone()
        second = vlm.generate(ids2, past_key_values=cache, answer_prompt="Best Options: (", **kw)
        ref = vlm.generate(torch.cat([ids1, first, ids2], dim=1), pixel_values_videos=pix,
                           answer_prompt="Best Options: (", **kw)
        # a turn that ends on its end-of-sequence token leaves that token pending; the next turn feeds it first
        eos = int(first[0, 1])
        short, cache2 = vlm.generate(ids1, pixel_values_videos=pix, return_past_key_values=True, max_new_tokens=4,
                                     return_ids=True, eos_token_id=eos)
        assert short.tolist() == first[:, :2].tolist() and cache2.pending_ids.tolist() == [[eos]]
        second2 = vlm.generate(ids2, past_key_values=cache2, **kw)
        ref2 = vlm.generate(torch.cat([ids1, short, ids2], dim=1), pixel_values_videos=pix, **kw)
        text, cache3 = vlm.generate(ids2, past_key_values=fork, return_past_key_values=True, max_new_tokens=4,
                                    eos_token_id=-1)
        with pytest.raises(NotImplementedError):
            vlm.generate(ids1, pixel_values_videos=pix, past_key_values=cache3, **kw)
    assert torch.equal(second, ref), (second.tolist(), ref.tolist())
    assert torch.equal(second2, ref2), (second2.tolist(), ref2.tolist())
    assert isinstance(text, str) and cache3 is fork


def test_forward_with_pixels_behind_a_prefill_is_refused():
    vlm, _ = _toy_vlm()
    T, tok = 4, vlm.default_token_id
    ids = torch.tensor([[5] + [tok] * T + [7]])
    pix = torch.randn(T, 3, 96, 96)
    with kernels_cpu(), torch.no_grad():
        cache = vlm.llm_backbone.llm.new_cache(1, dtype=torch.float32)
        vlm(input_ids=ids, pixel_values_videos=pix, past_key_values=cache, use_cache=True,
            cache_position=torch.zeros(1, dtype=torch.long))
        n = cache.get_seq_length()
        with pytest.raises(NotImplementedError, match="continuation"):
            vlm(input_ids=ids, pixel_values_videos=pix, past_key_values=cache, cache_position=torch.tensor([n]))
        out = vlm(input_ids=torch.tensor([[8, 9, 10]]), past_key_values=cache, use_cache=True,
                  cache_position=torch.tensor([n]), logits_to_keep=3)
    assert out.logits.shape[:2] == (1, 3) and cache.get_seq_length() == n + 3


def test_c_abi_declares_the_sequence_update():
    from timeviper_amd import _capi, build
    build.build()
    lib = _capi.lib()
    hdr = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "timeviper_hip.h").read_text(), flags=re.S)
    m = re.search(r"int tv_selective_state_update_seq\((.*?)\);", hdr, flags=re.S)
    assert m, "tv_selective_state_update_seq is not declared in the header"
    params = [p.strip() for p in m.group(1).split(",")]
    ctype = {"void*": _capi._p, "const void*": _capi._p, "int": _capi._i, "int64_t": _capi._l, "float": _capi._f}
    want = [ctype[p.rsplit(" ", 1)[0].strip()] for p in params]
    res, args = _capi.SIGNATURES["tv_selective_state_update_seq"]
    assert res is _capi._i and args == want
    assert hasattr(lib, "tv_selective_state_update_seq")
    for name in ("tv_attn_append_fwd", "tv_attn_append_workspace_bytes", "tv_attn_append_calls",
                 "tv_selective_state_update_seq_last_impl"):
        assert hasattr(lib, name) and name in _capi.SIGNATURES and re.search(rf"\b{name}\(", hdr), name
    m = re.search(r"int tv_attn_append_fwd\((.*?)\);", hdr, flags=re.S)
    ctype["const int*"] = _capi._p
    ctype["size_t"] = _capi._z
    want = [ctype[p.rsplit(" ", 1)[0].strip()] for p in (q.strip() for q in m.group(1).split(","))]
    assert _capi.SIGNATURES["tv_attn_append_fwd"] == (_capi._i, want)
    assert lib.tv_attn_append_workspace_bytes(1, 8, 40, 8, 32868) > 0
    # outside the supported range: refused, nothing launched (65 query tokens; 8 x 20 columns)
    one = 16
    args = lambda T, Hq, Hkv: (one, one, one, one, None, 1, T, 4096, None, Hq, Hkv, 128, *([8] * 12), 0.1, 1, one, 1 << 30, None)
    assert lib.tv_attn_append_fwd(*args(65, 8, 8)) == -2 and lib.tv_attn_append_fwd(*args(8, 40, 2)) == -2
    assert lib.tv_attn_append_fwd(*args(8, 40, 8)[:7], 4, *args(8, 40, 8)[8:]) == -1       # more queries than keys
    assert lib.tv_abi_version() == _capi.ABI_VERSION == 13
    # bad arguments are refused before any launch
    assert lib.tv_selective_state_update_seq(*([None] * 9), 1, 1, 4, 8, 1, 16, *([0] * 12), 1, 1, 0.0, 1.0, 0, None) == -1
