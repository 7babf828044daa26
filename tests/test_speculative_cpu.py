"""Speculative greedy decoding — host logic, no GPU: the prompt-lookup drafter, the cache's provisional tokens and their
rollback, and `generate(speculative=D)` against plain `generate`.

Kernels are the oracle-backed stand-ins of `cpu_kernel_shim` plus, here, fp64 stand-ins for the entry points the feature
adds or drives differently: `kernels.selective_state_update_spec` (commit the first n_commit previous tokens into the state,
then the new tokens from there WITHOUT storing), `kernels.causal_conv1d_xbc_into` and `kernels.flash_attn_append` with a
device-side key count.  Both sides of every comparison run the same fp64-backed operators on an fp32 model; ids are compared
exactly (the toy models' logits are spread: no near-ties), states at rtol 1e-4 / atol 8e-5, the bound of
tests/test_continue_cpu.py for the same operators."""
import contextlib
import math
import re
from pathlib import Path

import pytest
import torch

import cpu_kernel_shim
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


def _spec(state, prev, n_commit, new, A, D=None, dt_bias=None, dt_softplus=False, dt_limit=(0.0, float("inf")),
          group_map="block", out=None):
    nc = int(n_commit)
    kw = dict(dt_bias=dt_bias, dt_softplus=dt_softplus, dt_limit=dt_limit, group_map=group_map)
    if prev is not None:
        nc = min(max(nc, 0), prev[0].shape[1])
        if nc > 0:
            x, dt, B, C = (t[:, :nc] for t in prev)
            _, fin, _ = R.ssd_recurrence_ref(x, dt, A, B, C, D=D, initial_states=state, **kw)
            state.copy_(fin.to(state.dtype))
    else:
        assert nc == 0
    if new is None:
        return None
    x, dt, B, C = new
    y, _, _ = R.ssd_recurrence_ref(x, dt, A, B, C, D=D, initial_states=state, **kw)
    return y.to(x.dtype)


def _conv_into(xBC, weight, bias, d_inner, ngroups, dstate, out, activation="silu", halo=None):
    x, Bm, Cm = cpu_kernel_shim._conv_xbc(xBC, weight, bias, d_inner, ngroups, dstate, activation=activation, halo=halo)
    out[0].copy_(x)
    out[1].copy_(Bm.transpose(1, 2))
    out[2].copy_(Cm.transpose(1, 2))
    return out[0], out[1].transpose(1, 2), out[2].transpose(1, 2)


def _append(q, k, v, seqlens_k=None, softmax_scale=None, return_lse=False):
    if seqlens_k is not None:
        assert seqlens_k.dtype == torch.int32
        n = int(seqlens_k[0])
        assert q.shape[1] <= n <= k.shape[1]
        k, v = k[:, :n], v[:, :n]
    o, lse = R.attention_ref(q, k, v, True, softmax_scale)
    return (o.to(q.dtype), lse) if return_lse else o.to(q.dtype)


@contextlib.contextmanager
def kernels_cpu():
    from timeviper_amd import kernels as K
    names = {"selective_state_update_seq": _seq, "flash_attn_append": _append, "selective_state_update_spec": _spec,
             "causal_conv1d_xbc_into": _conv_into}
    with cpu_kernels():
        saved = {n: getattr(K, n) for n in names}
        for n, f in names.items():
            setattr(K, n, f)
        try:
            yield
        finally:
            for n, f in saved.items():
                setattr(K, n, f)


# ------------------------------------------------------------------------------------------------ drafter
PH = 99          # an image placeholder id


@pytest.mark.parametrize("ids, n, kw, want", [
    # the longest n-gram wins: the 1-gram [3] last occurred in front of 9, the 3-gram [1, 2, 3] in front of 7
    ([1, 2, 3, 7, 8, 4, 3, 9, 1, 2, 3], 2, {}, [7, 8]),
    # the most recent occurrence wins
    ([5, 6, 1, 5, 6, 2, 5, 6], 1, {}, [2]),
    ([5, 6, 1, 5, 6, 2, 5, 6], 3, {}, [2, 5, 6]),
    # no match
    ([1, 2, 3, 4], 3, {}, []),
    ([], 3, {}, []),
    ([4], 3, {}, []),
    # a tail shorter than D
    ([1, 2, 3, 1, 2], 4, {}, [3, 1, 2]),
    ([7, 7], 4, {}, [7]),
    # ngram_min: a 1-gram match is not enough
    ([1, 2, 3, 9, 3], 2, {"ngram_min": 2}, []),
    ([1, 2, 3, 9, 3], 2, {}, [9, 3]),
    # placeholder ids are never proposed: the continuation stops in front of them, an occurrence followed by one is passed over
    ([1, 2, 4, PH, PH, 1, 2], 3, {"exclude_ids": (PH,)}, [4]),
    ([1, 2, 5, 6, 1, 2, PH, 8, 1, 2], 2, {"exclude_ids": (PH,)}, [5, 6]),
    ([1, 2, PH, 8, 1, 2], 2, {"exclude_ids": (PH,)}, []),
])
def test_prompt_lookup_draft(ids, n, kw, want):
    from timeviper_amd.model.llm.speculative import prompt_lookup_draft
    got = prompt_lookup_draft(ids, n, **kw)
    assert got == want and all(isinstance(t, int) for t in got)


# ------------------------------------------------------------------------------------------------ toy models
def _cfg(pattern="M*-M*-", **kw):
    base = dict(vocab_size=64, hidden_size=32, intermediate_size=48, num_hidden_layers=len(pattern),
                hybrid_override_pattern=pattern, num_attention_heads=2, head_dim=16, num_key_value_heads=1,
                ssm_state_size=8, mamba_num_heads=4, mamba_n_groups=2, mamba_head_dim=8, mamba_chunk_size=8)
    base.update(kw)
    return NemotronHConfig(**base)


def _toy_generator(pattern, seed=0):
    """The toy VLM recipe of tests/test_continue_cpu.py around an fp32 hybrid of the given pattern (text-only prompts here)."""
    from timeviper_amd.model import HybridTimeViperVLM, get_llm_backbone_and_tokenizer
    from timeviper_amd.model.vit import TimmViTBackbone
    torch.manual_seed(seed)
    vb = TimmViTBackbone("siglip-vit-b16-224px", depth_override=1, default_image_size=96)
    llm, _ = get_llm_backbone_and_tokenizer("nanov2-9b", llm_max_length=None, attn_implementation="flash_attention_2",
                                            merge_module="no_merge", config=_cfg(pattern))
    vlm = HybridTimeViperVLM("toy", vb, llm, arch_specifier="tome_mlp-16").float().eval()
    with torch.no_grad():
        vlm.llm_backbone.llm.lm_head.weight.mul_(20.0)     # spread the logits: no near-ties under greedy decoding
    return vlm


def _oracle_drafter(prompt, truth, j, vocab):
    """Drafts built from the plain greedy ids: right for the first j drafts of every step, then (true + 1) % vocab."""
    n0 = len(prompt)

    def fn(ids, D):
        assert ids[:n0] == prompt
        at = len(ids) - n0                                # index (in the generated ids) of the first drafted token
        out = []
        for i in range(D):
            t = truth[at + i] if at + i < len(truth) else 0
            out.append(t if i < j else (t + 1) % vocab)
        return out
    return fn


GEN = {}


def _plain(pattern, N=12):
    """The plain greedy run of a toy model, computed once and shared (never modified)."""
    if pattern not in GEN:
        vlm = _toy_generator(pattern)
        prompt = torch.randint(0, 60, (1, 9), generator=torch.Generator().manual_seed(11))
        with kernels_cpu():
            ids, cache = vlm.generate(prompt, max_new_tokens=N, return_ids=True, return_past_key_values=True, eos_token_id=-1)
        assert vlm.last_generate_stats["speculative"] is False and ids.shape == (1, N)
        GEN[pattern] = (vlm, prompt, ids, cache)
    return GEN[pattern]


@pytest.mark.parametrize("pattern", ["M*-M*-", "MM*-"])
@pytest.mark.parametrize("D", [1, 3, 5])
@pytest.mark.parametrize("jsel", ["0", "1", "D"])
def test_generate_speculative_equals_plain(pattern, D, jsel):
    N = 12
    vlm, prompt, plain, plain_cache = _plain(pattern, N)
    j = {"0": 0, "1": min(1, D), "D": D}[jsel]
    truth = plain[0].tolist()
    fn = _oracle_drafter(prompt[0].tolist(), truth, j, 64)
    with kernels_cpu():
        ids, cache = vlm.generate(prompt, max_new_tokens=N, return_ids=True, return_past_key_values=True, speculative=D,
                                  draft_fn=fn, eos_token_id=-1)
    st = vlm.last_generate_stats
    assert st["speculative"] is True and st["graphed"] is False and st["emitted"] == N
    assert torch.equal(ids, plain), (ids.tolist(), plain.tolist())
    assert st["drafted"] == st["steps"] * D
    if j == 0:
        assert st["accepted"] == 0 and st["steps"] == st["emitted"] - 1
    if j == D:
        assert st["drafted"] - D <= st["accepted"] <= st["drafted"]          # all but the final, truncated step
        assert st["steps"] <= math.ceil(st["emitted"] / (D + 1))
    if 0 < j < D:
        assert st["accepted"] == st["steps"] * j or st["accepted"] >= (st["steps"] - 1) * j
    # the returned cache: flushed, out of speculation mode, what the plain run left
    assert not cache.speculating and cache.get_seq_length() == plain_cache.get_seq_length() == prompt.shape[1] + N
    assert cache.pending_ids.numel() == 0 and plain_cache.pending_ids.numel() == 0
    _assert_same_cache(cache, plain_cache, vlm.llm_backbone.llm.config)


def _assert_same_cache(a, b, cfg):
    for i, c in enumerate(cfg.hybrid_override_pattern):
        if c == "M":
            torch.testing.assert_close(a.conv_states[i], b.conv_states[i], rtol=RTOL, atol=ATOL)
            torch.testing.assert_close(a.ssm_states[i], b.ssm_states[i], rtol=RTOL, atol=ATOL)
        elif c == "*":
            assert a.key_cache[i].shape == b.key_cache[i].shape
            torch.testing.assert_close(a.key_cache[i], b.key_cache[i], rtol=RTOL, atol=ATOL)
            torch.testing.assert_close(a.value_cache[i], b.value_cache[i], rtol=RTOL, atol=ATOL)


def test_eos_in_the_middle_of_an_accepted_run():
    N, D = 12, 5
    vlm, prompt, plain, _ = _plain("M*-M*-", N)
    truth = plain[0].tolist()
    eos = truth[3]                                         # step 1 emits truth[1 .. 6] when every draft is right
    assert eos not in truth[:3]
    fn = _oracle_drafter(prompt[0].tolist(), truth, D, 64)
    kw = dict(max_new_tokens=N, return_ids=True, return_past_key_values=True, eos_token_id=eos)
    with kernels_cpu():
        want, want_cache = vlm.generate(prompt, **kw)
        got, cache = vlm.generate(prompt, speculative=D, draft_fn=fn, **kw)
    assert vlm.last_generate_stats["speculative"] is True and vlm.last_generate_stats["steps"] == 1
    assert want.tolist() == [truth[:4]] and torch.equal(got, want)
    assert cache.pending_ids.tolist() == want_cache.pending_ids.tolist() == [[eos]]
    assert cache.get_seq_length() == want_cache.get_seq_length() == prompt.shape[1] + 3
    _assert_same_cache(cache, want_cache, vlm.llm_backbone.llm.config)


def test_two_turns_speculative_then_plain():
    N, D = 12, 3
    vlm, prompt, plain, _ = _plain("MM*-", N)
    fn = _oracle_drafter(prompt[0].tolist(), plain[0].tolist(), 2, 64)
    ids2 = torch.tensor([[10, 11, 12, 13, 14]])
    kw = dict(max_new_tokens=6, return_ids=True, eos_token_id=-1)
    with kernels_cpu():
        first, cache = vlm.generate(prompt, max_new_tokens=N, return_ids=True, return_past_key_values=True, speculative=D,
                                    draft_fn=fn, eos_token_id=-1)
        assert vlm.last_generate_stats["speculative"] is True and torch.equal(first, plain)
        fork = cache.clone()                               # works again behind end_speculation
        second = vlm.generate(ids2, past_key_values=cache, **kw)
        assert vlm.last_generate_stats["speculative"] is False
        first_p, cache_p = vlm.generate(prompt, max_new_tokens=N, return_ids=True, return_past_key_values=True, eos_token_id=-1)
        second_p = vlm.generate(ids2, past_key_values=cache_p, **kw)
        # ... and a speculative second turn on the fork, drafting by prompt lookup
        third = vlm.generate(ids2, past_key_values=fork, speculative=2, **kw)
        assert vlm.last_generate_stats["speculative"] is True
    assert torch.equal(first_p, plain) and torch.equal(second, second_p) and torch.equal(third, second_p)


# ------------------------------------------------------------------------------------------------ cache API
def _prefill(model, ids):
    cache = HybridMambaAttentionDynamicCache(model.config, 1, dtype=torch.float32)
    model(input_ids=ids, past_key_values=cache, use_cache=True, cache_position=torch.zeros(1, dtype=torch.long))
    return cache


@pytest.mark.parametrize("k_as", ["int", "tensor"])
def test_commit_then_end_equals_single_steps(k_as):
    cfg = _cfg("M*-M*-M")
    torch.manual_seed(4)
    model = NemotronHForCausalLM(cfg).float().eval()
    n = 11
    ids = torch.randint(0, cfg.vocab_size, (1, n + 12), generator=torch.Generator().manual_seed(5))
    one = torch.ones(1, dtype=torch.long)
    wrap = (lambda k: torch.tensor(k)) if k_as == "tensor" else (lambda k: k)
    with torch.no_grad(), kernels_cpu():
        cache = _prefill(model, ids[:, :n])
        steps = cache.clone()
        assert not cache.speculating
        cache.begin_speculation(6, 12)
        assert cache.speculating
        with pytest.raises(RuntimeError, match="speculation"):
            cache.clone()
        # forward 1: 5 tokens of which 3 are kept (first said 4, then lowered); forward 2: the 2 rejected ones replaced by 4
        # other tokens, all kept but one; forward 3: one token, kept
        a = model(input_ids=ids[:, n:n + 5], past_key_values=cache, cache_position=one, logits_to_keep=5).logits
        cache.commit(wrap(4))
        cache.commit(wrap(3))
        kept = list(range(n, n + 3))
        b = model(input_ids=ids[:, n + 5:n + 9], past_key_values=cache, cache_position=one, logits_to_keep=4).logits
        cache.commit(wrap(3))
        kept += list(range(n + 5, n + 8))
        c = model(input_ids=ids[:, n + 10:n + 11], past_key_values=cache, cache_position=one, logits_to_keep=1).logits
        cache.commit(wrap(1))
        kept += [n + 10]
        with pytest.raises(ValueError):
            cache.commit(2)
        cache.end_speculation()
        assert not cache.speculating
        single = [model(input_ids=ids[:, t:t + 1], past_key_values=steps, cache_position=one).logits[:, -1] for t in kept]
    assert cache.get_seq_length() == steps.get_seq_length() == n + 7
    _assert_same_cache(cache, steps, cfg)
    # the logits of a kept token are those of its single step (the rejected tokens in front of it left no trace)
    torch.testing.assert_close(a[:, :3], torch.stack(single[:3], dim=1), rtol=RTOL, atol=ATOL)
    torch.testing.assert_close(b[:, :3], torch.stack(single[3:6], dim=1), rtol=RTOL, atol=ATOL)
    torch.testing.assert_close(c[:, 0], single[6], rtol=RTOL, atol=ATOL)
    # afterwards: clone, static decode and a continuation all work
    with torch.no_grad(), kernels_cpu():
        cache.clone()
        model(input_ids=ids[:, :2], past_key_values=cache, cache_position=one)
        cache.begin_static_decode(4)
        cache.end_static_decode()
    assert cache.get_seq_length() == n + 9


def test_speculation_limits():
    cfg = _cfg("M*-")
    torch.manual_seed(1)
    model = NemotronHForCausalLM(cfg).float().eval()
    ids = torch.randint(0, cfg.vocab_size, (1, 30), generator=torch.Generator().manual_seed(2))
    one = torch.ones(1, dtype=torch.long)
    with torch.no_grad(), kernels_cpu():
        cache = _prefill(model, ids[:, :8])
        with pytest.raises(RuntimeError):
            cache.commit(1)                                # not speculating
        cache.begin_speculation(nano.continue_t_seq() + 1, 4)
        with pytest.raises(RuntimeError, match="continue_t_seq"):
            model(input_ids=ids[:, 8:8 + nano.continue_t_seq() + 1], past_key_values=cache, cache_position=one)
        cache.end_speculation()
        assert cache.get_seq_length() == 8
        cache.begin_speculation(2, 4)
        with pytest.raises(RuntimeError, match="t_max"):
            model(input_ids=ids[:, 8:11], past_key_values=cache, cache_position=one)
        with pytest.raises(RuntimeError, match="already"):
            cache.begin_speculation(2, 4)
        cache.end_speculation()
    empty = HybridMambaAttentionDynamicCache(cfg, 1, dtype=torch.float32)
    with pytest.raises(RuntimeError, match="prefill"):
        empty.begin_speculation(2, 4)


def test_out_of_scope_stacks_decode_plainly():
    vlm, prompt, plain, _ = _plain("MM*-", 12)
    from timeviper_amd import kernels as K
    with kernels_cpu(), K.fp8_attention():
        ids = vlm.generate(prompt, max_new_tokens=12, return_ids=True, speculative=3, eos_token_id=-1)
    assert vlm.last_generate_stats["speculative"] is False and torch.equal(ids, plain)
    with pytest.raises(ValueError), kernels_cpu():
        vlm.generate(prompt, max_new_tokens=12, return_ids=True, speculative=0)


# ------------------------------------------------------------------------------------------------ C ABI
def test_c_abi_declares_the_speculative_update():
    from timeviper_amd import _capi, build
    from timeviper_amd import kernels as K
    build.build()
    lib = _capi.lib()
    hdr = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "timeviper_hip.h").read_text(), flags=re.S)
    m = re.search(r"int tv_selective_state_update_spec\((.*?)\);", hdr, flags=re.S)
    assert m, "tv_selective_state_update_spec is not declared in the header"
    ctype = {"void*": _capi._p, "const void*": _capi._p, "const int*": _capi._p, "int": _capi._i, "int64_t": _capi._l,
             "float": _capi._f}
    want = [ctype[p.strip().rsplit(" ", 1)[0].strip()] for p in m.group(1).split(",")]
    res, args = _capi.SIGNATURES["tv_selective_state_update_spec"]
    assert res is _capi._i and args == want
    assert hasattr(lib, "tv_selective_state_update_spec") and hasattr(lib, "tv_selective_state_update_spec_last_impl")
    assert "tv_selective_state_update_spec_last_impl" in _capi.SIGNATURES
    assert callable(K.selective_state_update_spec)
    assert lib.tv_abi_version() == _capi.ABI_VERSION == 13           # additive: no bump

    def call(state=None, A=None, prev=None, t_prev=0, n_commit=0, new=None, t_new=0):
        return lib.tv_selective_state_update_spec(state, A, None, None, *([prev] * 4), t_prev, n_commit, None, *([16] * 10),
                                                  *([new] * 5), t_new, *([16] * 12), 1, 4, 4, 1, 16, 1, 1, 0.0, 1.0, 0, None)
    # bad arguments are refused before any launch: null state, a host n_commit out of range, null operands
    assert call() == -1
    assert call(state=16, A=16, prev=16, t_prev=2, n_commit=3) == -1
    assert call(state=16, A=16, prev=16, t_prev=2, n_commit=-1) == -1
    assert call(state=16, A=16, t_prev=2, n_commit=1) == -1
    assert call(state=16, A=16, t_new=2) == -1
    # nothing to commit and nothing to run: accepted, no launch
    assert call(state=16, A=16) == 0 and call(state=16, A=16, prev=16, t_prev=2, n_commit=0) == 0
