"""The Nemotron-H stack after quantize_weights_e4m3(): the decode step's products run on tv_gemv_fp8w_fwd, compute what
the bf16 kernels compute on the same (rounded) weights, and every decode mode keeps its guarantees."""
import contextlib
import os

import pytest
import torch

from test_rows_fused_model_gpu import (N_NEW, N_PREFILL, SEED, _assert_no_near_tie, _synthetic_vlm, _toy_hybrid_d128,
                                       relerr)

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def toy_quantized():
    """The toy model of test_rows_fused_model_gpu.py, quantized, 300 + 17 token ids and the cache of the 300-token
    prefill (on the rounded weights): shared, never modified (tests clone the cache)."""
    from timeviper_amd.model.llm import nano
    cfg, model = _toy_hybrid_d128()
    assert model.quantize_weights_e4m3() == sum({"M": 2, "-": 2, "*": 4}[c] for c in cfg.hybrid_override_pattern) + 1
    ids = torch.randint(0, cfg.vocab_size, (1, N_PREFILL + 17), generator=torch.Generator().manual_seed(7)).to(DEV)
    with torch.inference_mode():
        cache = nano.HybridMambaAttentionDynamicCache(cfg, 1, dtype=torch.bfloat16, device=DEV)
        model(input_ids=ids[:, :N_PREFILL], past_key_values=cache, use_cache=True,
              cache_position=torch.zeros(1, dtype=torch.long))
    return cfg, model, ids, cache


def _steps(model, ids, cache, n):
    out = []
    with torch.inference_mode():
        for i in range(n):
            out.append(model(input_ids=ids[:, N_PREFILL + i:N_PREFILL + i + 1], past_key_values=cache, use_cache=True,
                             cache_position=torch.tensor([N_PREFILL + i])).logits[:, -1])
    return torch.stack(out, dim=1)


def test_every_product_of_a_step_runs_on_the_copies(toy_quantized, monkeypatch):
    from timeviper_amd import kernels as K
    cfg, model, ids, prefilled = toy_quantized
    bf16_calls, orig = [], K.gemv_fused

    def spy(x, weight, *a, **kw):
        bf16_calls.append(tuple(weight.shape))
        return orig(x, weight, *a, **kw)
    monkeypatch.setattr(K, "gemv_fused", spy)
    products = 2 * len(cfg.hybrid_override_pattern) + 1            # two a block (the attention's q / k / v are one) + lm_head
    before = K.gemv_fp8w_calls()
    _steps(model, ids, prefilled.clone(), 3)
    assert K.gemv_fp8w_calls() == before + 3 * products
    assert bf16_calls == []                                        # no quantized matrix on the bf16 kernel
    # TV_FP8W=0, read per call: the same step on the bf16 kernel, nothing dropped
    monkeypatch.setenv("TV_FP8W", "0")
    _steps(model, ids, prefilled.clone(), 1)
    assert K.gemv_fp8w_calls() == before + 3 * products and len(bf16_calls) == products
    assert model.has_fp8_weights()
    monkeypatch.delenv("TV_FP8W")
    # a rewritten matrix runs on bf16 (its key no longer matches), the others stay on their copies
    lin = model.backbone.layers[0].mixer.out_proj
    saved = lin.weight.detach().clone()
    bf16_calls.clear()
    try:
        with torch.no_grad():
            lin.weight.mul_(1.0)
        _steps(model, ids, prefilled.clone(), 1)
        assert bf16_calls == [tuple(lin.weight.shape)]
        assert K.gemv_fp8w_calls() == before + 3 * products + products - 1
    finally:
        with torch.no_grad():
            lin.weight.copy_(saved)
        model.quantize_weights_e4m3()                              # (a fixed point: the weights do not change)
    assert torch.equal(lin.weight, saved)


def test_steps_compute_what_the_bf16_route_computes(toy_quantized, monkeypatch):
    """Same operators and rounding points on the same numbers, other summation order in the products:
    test_rows_fused_model_gpu.py's bounds for that (logits relerr < 3e-2 per position, states and K/V < 2e-2, greedy ids
    where the top-2 gap exceeds the largest logit difference)."""
    cfg, model, ids, prefilled = toy_quantized
    T = 5
    on, off = prefilled.clone(), prefilled.clone()
    lg_on = _steps(model, ids, on, T)
    monkeypatch.setenv("TV_FP8W", "0")
    lg_off = _steps(model, ids, off, T)
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
            assert relerr(on.key_cache[i], off.key_cache[i]) < 2e-2, i
            assert relerr(on.value_cache[i], off.value_cache[i]) < 2e-2, i


# ------------------------------------------------------------------ generate (test_rows_fused_model_gpu.py's recipe)
# The synthetic VLM's seed.  Seed 299 of test_rows_fused_model_gpu.py has no near-tie on its original weights, but rounding
# them to e4m3 moves its smallest top-2 margin to 0.044 rms(logits), under `_assert_no_near_tie`'s 0.127.  The bf16 route
# (TV_FP8W=0) on the rounded weights was run for the seeds 299 .. 442 on an MI355X: 442 is the first whose 16 positions all
# clear the threshold (smallest margin 0.179).  The threshold is that file's, unchanged.
assert SEED == 299
SEED_Q = 442


@contextlib.contextmanager
def _env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update(kv)
    try:
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def _quantized_case(seed):
    """The synthetic VLM of `seed`, quantized; the reference run is the bf16 route (TV_FP8W=0) on the rounded weights,
    eager, with its top-2 margins."""
    vlm = _synthetic_vlm(seed)
    vlm.quantize_llm_weights_e4m3()
    pix = torch.randn(40, 3, 96, 96, generator=torch.Generator().manual_seed(seed)).to(DEV).bfloat16()
    ids = torch.tensor([[5, 6, 7] + [vlm.default_token_id] * 40 + [8, 9, 10, 11]], device=DEV)
    with _env(TV_FP8W="0", TV_DECODE_GRAPH="0"):
        out, cache = vlm.generate(ids, pixel_values_videos=pix, max_new_tokens=N_NEW, return_ids=True, eos_token_id=-1,
                                  return_past_key_values=True)
        assert vlm.last_generate_stats["fp8_weights"] is False and vlm.last_generate_stats["graphed"] is False
    with torch.inference_mode():
        lg = vlm(input_ids=torch.cat([ids, out[:, :-1]], dim=1), pixel_values_videos=pix,
                 logits_to_keep=out.shape[1]).logits[0].float()
    top2 = lg.topk(2, dim=-1).values
    margins = ((top2[:, 0] - top2[:, 1]) / lg.pow(2).mean(-1).sqrt()).tolist()
    return vlm, pix, ids, out, cache, margins


@pytest.fixture(scope="module")
def vlm_quantized():
    return _quantized_case(SEED_Q)


def test_generate_modes_agree(vlm_quantized):
    from timeviper_amd import kernels as K
    vlm, pix, ids, want, bf16_cache, margins = vlm_quantized
    _assert_no_near_tie(margins)
    kw = dict(pixel_values_videos=pix, max_new_tokens=N_NEW, return_ids=True, eos_token_id=-1)
    before = K.gemv_fp8w_calls()
    graphed = vlm.generate(ids, **kw)
    st = vlm.last_generate_stats
    print(st)
    assert st["fp8_weights"] is True and st["graphed"] is True and st["capture_error"] is None
    assert K.gemv_fp8w_calls() > before            # (the eager warm-up steps and the capture launch it)
    assert torch.equal(graphed, want), (graphed.tolist(), want.tolist())          # = the TV_FP8W=0 run
    with _env(TV_DECODE_GRAPH="0"):
        eager = vlm.generate(ids, **kw)
        assert vlm.last_generate_stats["graphed"] is False and vlm.last_generate_stats["fp8_weights"] is True
    assert torch.equal(eager, graphed)
    spec = vlm.generate(ids, speculative=2, **kw)
    st = vlm.last_generate_stats
    assert st["speculative"] is True and st["fp8_weights"] is True
    assert torch.equal(spec, want), (spec.tolist(), want.tolist())


def test_generate_branches_equals_generate_on_clones(vlm_quantized):
    vlm, pix, ids, _, cache, _ = vlm_quantized
    q1 = torch.tensor([[12, 13, 14, 15]], device=DEV)
    q2 = torch.tensor([[21, 22, 23]], device=DEV)
    kw = dict(max_new_tokens=8, return_ids=True, eos_token_id=-1)
    singles = [vlm.generate(q, past_key_values=cache.clone(), **kw) for q in (q1, q2)]
    got = vlm.generate_branches([q1, q2], past_key_values=cache.clone(), **kw)
    st = vlm.last_generate_stats
    print(st)
    assert st["branched"] is True and st["fp8_weights"] is True
    for g, w in zip(got, singles):
        assert torch.equal(g, w), (g.tolist(), w.tolist())
