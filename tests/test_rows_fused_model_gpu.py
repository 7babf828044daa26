"""The few-token forwards of the Nemotron-H stack (a continuation, a speculative step) on tv_linear_rows_bf16_fwd: which
calls are made, and that they compute what the unfused route (TV_ROWS_FUSED=0) computes."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
PATTERN = "M-*M*-"


def relerr(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def _toy_hybrid_d128(pattern=PATTERN):
    """(tests/test_continue_gpu.py's toy model)"""
    from timeviper_amd.model.llm.nano import NemotronHConfig, NemotronHForCausalLM
    torch.manual_seed(11)
    cfg = NemotronHConfig(vocab_size=256, hidden_size=256, intermediate_size=384, num_hidden_layers=len(pattern),
                          hybrid_override_pattern=pattern, num_attention_heads=8, head_dim=128,
                          num_key_value_heads=2, ssm_state_size=16, mamba_num_heads=8,
                          mamba_n_groups=2, mamba_head_dim=16, mamba_chunk_size=16)
    model = NemotronHForCausalLM(cfg).to(DEV).bfloat16().eval()
    with torch.no_grad():       # spread the logits
        for blk in model.backbone.layers:
            if blk.block_type == "attention":
                blk.mixer.q_proj.weight.mul_(8.0)
                blk.mixer.k_proj.weight.mul_(8.0)
        model.lm_head.weight.mul_(20.0)
    return cfg, model


N_PREFILL = 300


@pytest.fixture(scope="module")
def toy_prefilled():
    """The model, 300 + 17 token ids and the cache of the 300-token prefill: shared, never modified (tests clone it)."""
    from timeviper_amd.model.llm import nano
    cfg, model = _toy_hybrid_d128()
    ids = torch.randint(0, cfg.vocab_size, (1, N_PREFILL + 17), generator=torch.Generator().manual_seed(7)).to(DEV)
    with torch.inference_mode():
        cache = nano.HybridMambaAttentionDynamicCache(cfg, 1, dtype=torch.bfloat16, device=DEV)
        model(input_ids=ids[:, :N_PREFILL], past_key_values=cache, use_cache=True,
              cache_position=torch.zeros(1, dtype=torch.long))
    return cfg, model, ids, cache


@pytest.fixture
def recorded(monkeypatch):
    """The feature switched on, K.linear_rows_fused wrapped to record (prologue, rows, N) of every call"""
    from timeviper_amd import kernels as K
    monkeypatch.setenv("TV_ROWS_FUSED", "1")
    calls, orig = [], K.linear_rows_fused

    def spy(x, weight, bias=None, prologue=K.GEMV_NONE, **kw):
        calls.append((int(prologue), x.shape[-2], weight.shape[0]))
        return orig(x, weight, bias, prologue, **kw)
    monkeypatch.setattr(K, "linear_rows_fused", spy)
    return calls


def _continue(model, ids, cache, T):
    with torch.inference_mode():
        return model(input_ids=ids[:, N_PREFILL:N_PREFILL + T], past_key_values=cache, use_cache=True,
                     cache_position=torch.tensor([N_PREFILL]), logits_to_keep=T).logits


def _expected_calls(K, cfg, T):
    per = {"M": [K.GEMV_RMSNORM, K.GEMV_GATED], "-": [K.GEMV_RMSNORM, K.GEMV_RELU2], "*": [K.GEMV_RMSNORM, K.GEMV_NONE]}
    want = [p for c in cfg.hybrid_override_pattern for p in per[c]] + [K.GEMV_NONE]         # (+ the lm_head)
    return want


def test_dispatch_of_a_continuation(toy_prefilled, recorded, monkeypatch):
    from timeviper_amd import kernels as K
    cfg, model, ids, prefilled = toy_prefilled
    _continue(model, ids, prefilled.clone(), 5)
    assert [c[0] for c in recorded] == _expected_calls(K, cfg, 5), recorded
    assert all(c[1] == 5 for c in recorded) and recorded[-1][2] == cfg.vocab_size
    for T in (17, 1):
        recorded.clear()
        _continue(model, ids, prefilled.clone(), T)
        assert recorded == [], (T, recorded)
    monkeypatch.setenv("TV_ROWS_FUSED", "0")
    _continue(model, ids, prefilled.clone(), 5)
    assert recorded == []


def test_dispatch_of_a_speculative_step(toy_prefilled, recorded, monkeypatch):
    from timeviper_amd import kernels as K
    cfg, model, ids, prefilled = toy_prefilled
    one = torch.ones(1, dtype=torch.long)
    for env, want in (("1", _expected_calls(K, cfg, 3)), ("0", [])):
        monkeypatch.setenv("TV_ROWS_FUSED", env)
        recorded.clear()
        cache = prefilled.clone()
        with torch.inference_mode():
            cache.begin_speculation(3, 8)
            model(input_ids=ids[:, N_PREFILL:N_PREFILL + 3], past_key_values=cache, use_cache=True, cache_position=one,
                  logits_to_keep=3)
            cache.commit(3)
            cache.end_speculation()
        assert [c[0] for c in recorded] == want, (env, recorded)
        assert all(c[1] == 3 for c in recorded)


def test_continuation_computes_what_the_unfused_route_computes(toy_prefilled, monkeypatch):
    """Same operators with the same rounding points, other summation order in the products: the bounds
    test_continuation_equals_single_steps_bf16 applies to a continuation against single steps (relerr < 3e-2 per position
    of the logits, < 2e-2 of the states; greedy ids where the top-2 gap exceeds the largest logit difference)."""
    cfg, model, ids, prefilled = toy_prefilled
    T = 5
    on, off = prefilled.clone(), prefilled.clone()
    monkeypatch.setenv("TV_ROWS_FUSED", "1")
    lg_on = _continue(model, ids, on, T)
    monkeypatch.setenv("TV_ROWS_FUSED", "0")
    lg_off = _continue(model, ids, off, T)
    for i in range(T):
        err = relerr(lg_on[:, i], lg_off[:, i])
        print(f"position {i}: relerr {err:.2e}")
        assert err < 3e-2, (i, err)
        top2 = lg_off[0, i].float().topk(2).values
        if float(top2[0] - top2[1]) > float((lg_on[0, i] - lg_off[0, i]).abs().max()):
            assert int(lg_on[0, i].argmax()) == int(lg_off[0, i].argmax()), i
    assert on.get_seq_length() == off.get_seq_length() == N_PREFILL + T
    for i, c in enumerate(cfg.hybrid_override_pattern):
        if c == "M":
            assert relerr(on.ssm_states[i], off.ssm_states[i]) < 2e-2, i
            assert relerr(on.conv_states[i], off.conv_states[i]) < 2e-2, i
        elif c == "*":
            assert on.key_cache[i].shape == off.key_cache[i].shape == (1, N_PREFILL + T, 2, 128)
            assert relerr(on.key_cache[i], off.key_cache[i]) < 2e-2, i
            assert relerr(on.value_cache[i], off.value_cache[i]) < 2e-2, i


# ------------------------------------------------------------------ generate (tests/test_speculative_gpu.py's recipe)
SEED = 299         # test_speculative_gpu.py's SEED_GRAPHED: the plain run has no near-tie at any generated position
N_NEW = 16


def _synthetic_vlm(seed):
    from timeviper_amd.model import build_synthetic_timeviper
    from timeviper_amd.model.llm.nano import NemotronHConfig
    cfg = NemotronHConfig(vocab_size=128, hidden_size=256, intermediate_size=384, num_hidden_layers=8,
                          hybrid_override_pattern="M*-M*-M*", num_attention_heads=4, head_dim=128,
                          num_key_value_heads=2, ssm_state_size=16, mamba_num_heads=8,
                          mamba_n_groups=2, mamba_head_dim=16, mamba_chunk_size=16)
    vlm = build_synthetic_timeviper(cfg, "siglip-vit-b16-224px", pdrop_type="uni_2_0.75-uni_5_0.5",
                                    merge_module="no_merge", vit_depth=2, image_size=96, seed=seed)
    with torch.no_grad():       # spread the logits
        for blk in vlm.llm_backbone.llm.backbone.layers:
            if blk.block_type == "attention":
                blk.mixer.q_proj.weight.mul_(10.0)
                blk.mixer.k_proj.weight.mul_(10.0)
        vlm.llm_backbone.llm.lm_head.weight.mul_(20.0)
    return vlm


def _assert_no_near_tie(margins):
    """(test_speculative_gpu.py) greedy ids can only be required to agree where the plain run's top-2 gap exceeds three
    standard deviations of the difference of two logits' errors, each bounded by 3e-2 rms(logits)."""
    print("top-2 gap / rms(logits) of the plain run:", [round(m, 3) for m in margins])
    assert min(margins) > 3 * math.sqrt(2) * 3e-2, margins


@pytest.fixture(scope="module")
def vlm_case():
    vlm = _synthetic_vlm(SEED)
    pix = torch.randn(40, 3, 96, 96, generator=torch.Generator().manual_seed(SEED)).to(DEV).bfloat16()
    ids = torch.tensor([[5, 6, 7] + [vlm.default_token_id] * 40 + [8, 9, 10, 11]], device=DEV)
    out, cache = vlm.generate(ids, pixel_values_videos=pix, max_new_tokens=N_NEW, return_ids=True, eos_token_id=-1,
                              return_past_key_values=True)
    with torch.inference_mode():
        lg = vlm(input_ids=torch.cat([ids, out[:, :-1]], dim=1), pixel_values_videos=pix,
                 logits_to_keep=out.shape[1]).logits[0].float()
    top2 = lg.topk(2, dim=-1).values
    margins = ((top2[:, 0] - top2[:, 1]) / lg.pow(2).mean(-1).sqrt()).tolist()
    return vlm, pix, ids, out, cache, margins


def test_generate_speculative_2_equals_plain(vlm_case, recorded):
    vlm, pix, ids, want, plain_cache, margins = vlm_case
    got, cache = vlm.generate(ids, pixel_values_videos=pix, max_new_tokens=N_NEW, return_ids=True, eos_token_id=-1,
                              return_past_key_values=True, speculative=2)
    st = vlm.last_generate_stats
    print(st)
    assert st["speculative"] is True and st["graphed"] is True and st["capture_error"] is None
    assert recorded and all(c[1] == 3 for c in recorded)            # every step ran its products on the rows kernel
    _assert_no_near_tie(margins)
    assert torch.equal(got, want), (got.tolist(), want.tolist())
    assert not cache.speculating and cache.get_seq_length() == plain_cache.get_seq_length()
    for i, c in enumerate(vlm.llm_backbone.llm.config.hybrid_override_pattern):
        if c == "M":
            assert relerr(cache.ssm_states[i], plain_cache.ssm_states[i]) < 2e-2, i
            assert relerr(cache.conv_states[i], plain_cache.conv_states[i]) < 2e-2, i
        elif c == "*":
            n = cache.get_seq_length()
            assert relerr(cache.key_cache[i][:, :n], plain_cache.key_cache[i][:, :n]) < 2e-2, i
            assert relerr(cache.value_cache[i][:, :n], plain_cache.value_cache[i][:, :n]) < 2e-2, i


def test_conversation_turn_equals_the_unfused_route(vlm_case, recorded, monkeypatch):
    vlm, pix, ids, _, plain_cache, _ = vlm_case
    turn = torch.tensor([[12, 13, 14, 15, 16, 17, 18]], device=DEV)
    kw = dict(max_new_tokens=8, return_ids=True, eos_token_id=-1)
    on = vlm.generate(turn, past_key_values=plain_cache.clone(), **kw)
    assert recorded and recorded[0][1] == 7
    n_calls = len(recorded)
    monkeypatch.setenv("TV_ROWS_FUSED", "0")
    off = vlm.generate(turn, past_key_values=plain_cache.clone(), **kw)
    assert len(recorded) == n_calls
    assert torch.equal(on, off), (on.tolist(), off.tolist())
