"""The fused step bodies of the Nemotron-H blocks (`step_fused`: the decode step on K.gemv_fused, a few tokens behind a
prefill on K.linear_rows_fused) — dispatch and state bookkeeping, no GPU.

The two wrappers are replaced by one stand-in that composes the stand-alone operators `cpu_kernel_shim` already stands
in for (rms_norm with the residual add, relu2, rmsnorm_fn with a gate, causal_conv1d_update) with F.linear, and records
every call; `nano.fused_route` (and `nano.linear_route`, which it is built on and which single products ask) is replaced
by a function that decides from shape and continuation alone (no device, dtype or bf16-matrix condition).  Every case
runs once with that route and once with no route (torch.nn.Linear + the stand-alone operators): both sides run the same operators on the same fp32 model, so the bound is the one tests/test_continue_cpu.py
uses for fp64-backed operators on an fp32 model, rtol 1e-4 / atol 8e-5."""
import contextlib

import pytest
import torch
import torch.nn.functional as F

from test_continue_cpu import ATOL, RTOL, _assert_same_cache, _cfg, _model
from test_speculative_cpu import kernels_cpu          # test_continue_cpu's stand-ins + the speculative entry points
from timeviper_amd import kernels as K
from timeviper_amd.model.llm import nano
from timeviper_amd.model.llm.nano import HybridMambaAttentionDynamicCache

N_PREFILL = 12
CALLS = []             # (wrapper name, prologue, rows, N) of every call of the stand-in


def _fused_linear(name):
    def lin(x, weight, bias=None, prologue=K.GEMV_NONE, delta=None, sum_out=None, norm_weight=None, eps=0.0, gate=None,
            group_size=0, conv=None, out=None):
        assert out is None and (conv is None or name == "gemv_fused")
        CALLS.append((name, int(prologue), x.numel() // x.shape[-1], weight.shape[0]))
        if prologue == K.GEMV_RMSNORM:
            if delta is None:
                assert sum_out is None
                f = K.rms_norm(x, norm_weight, eps)
            else:
                f, s = K.rms_norm(x, norm_weight, eps, residual=delta, return_sum=True)
                sum_out.copy_(s)
        elif prologue == K.GEMV_RELU2:
            f = K.relu2(x)
        elif prologue == K.GEMV_GATED:
            f = K.rmsnorm_fn(x=x, weight=norm_weight, bias=None, z=gate, eps=eps, group_size=group_size,
                             norm_before_gate=False)
        else:
            assert prologue == K.GEMV_NONE
            f = x
        y = F.linear(f, weight, bias)
        if conv is not None:
            state, w, b, row0 = conv
            cols = slice(row0, row0 + state.shape[1])
            y[:, 0, cols] = K.causal_conv1d_update(y[:, 0, cols], state, w, b, "silu")
        return y
    return lin


def _linear_route_by_shape(x, cache=None, cache_position=None):
    """nano.linear_route without its device / dtype / switch conditions"""
    B, T = x.shape[:2]
    if T == 1 and B <= 4:
        return "gemv"
    if B == 1 and 2 <= T <= 16 and nano.is_continuation(cache, cache_position):
        return "rows"
    return None


def _route_by_shape(model, hidden, cache=None, cache_position=None, output_hidden_states=False):
    """nano.fused_route from shape and continuation alone: no device, dtype, switch or bf16-matrix condition"""
    route = _linear_route_by_shape(hidden, cache, cache_position)
    if route == "gemv" and (not nano.is_continuation(cache, cache_position) or getattr(cache, "speculating", False)):
        return None
    return route


@contextlib.contextmanager
def routed(route_fn):
    """The CPU kernels, the recording stand-in behind both wrappers (and shape predicates that ask for no device),
    `route_fn` as nano.fused_route and its per-product counterpart as nano.linear_route."""
    names = {"gemv_fused": _fused_linear("gemv_fused"), "linear_rows_fused": _fused_linear("linear_rows_fused"),
             "gemv_takes": lambda x, w: True, "linear_rows_takes": lambda x, w: True}
    with kernels_cpu():
        saved, saved_routes = {n: getattr(K, n) for n in names}, (nano.fused_route, nano.linear_route)
        for n, f in names.items():
            setattr(K, n, f)
        nano.fused_route = route_fn
        nano.linear_route = _no_route if route_fn is _no_route else _linear_route_by_shape
        CALLS.clear()
        try:
            yield
        finally:
            nano.fused_route, nano.linear_route = saved_routes
            for n, f in saved.items():
                setattr(K, n, f)


def _no_route(*a, **kw):
    return None


def _expected(cfg, name, rows):
    """(tests/test_rows_fused_model_gpu.py::_expected_calls, test_fused_decode_step_matches_the_unfused_one) M: rmsnorm-in_proj
    + gated-out_proj; -: rmsnorm-up + relu2-down; *: rmsnorm-[q; k; v] + o; then the head"""
    per = {"M": [K.GEMV_RMSNORM, K.GEMV_GATED], "-": [K.GEMV_RMSNORM, K.GEMV_RELU2], "*": [K.GEMV_RMSNORM, K.GEMV_NONE]}
    pro = [p for c in cfg.hybrid_override_pattern for p in per[c]] + [K.GEMV_NONE]
    return [(name, p, rows) for p in pro]


@pytest.fixture(scope="module")
def toy():
    """The fp32 model, its ids and the cache of the 12-token prefill at batch 2 and at batch 1 (row 0 of the same ids):
    shared, never modified (the cases clone the caches)."""
    cfg = _cfg("M*-M*-M")
    model = _model(cfg)
    ids = torch.randint(0, cfg.vocab_size, (2, N_PREFILL + 5), generator=torch.Generator().manual_seed(12))
    caches = {}
    with torch.no_grad(), routed(_no_route):
        for B in (1, 2):
            caches[B] = HybridMambaAttentionDynamicCache(cfg, B, dtype=torch.float32)
            model(input_ids=ids[:B, :N_PREFILL], past_key_values=caches[B], use_cache=True,
                  cache_position=torch.zeros(1, dtype=torch.long))
    assert CALLS == []
    return cfg, model, ids, caches


def _both(run, prefilled):
    """`run(cache)` -> logits with the route decided by shape and with no route: (logits, cache, calls) of each"""
    res = []
    for fn in (_route_by_shape, _no_route):
        cache = prefilled.clone()
        with torch.no_grad(), routed(fn):
            logits = run(cache)
            res.append((logits, cache, list(CALLS)))
    assert res[1][2] == []
    return res


def _assert_same(cfg, fused, plain, seq_len):
    torch.testing.assert_close(fused[0], plain[0], rtol=RTOL, atol=ATOL)
    _assert_same_cache(fused[1], plain[1], cfg)
    assert fused[1].get_seq_length() == plain[1].get_seq_length() == seq_len
    assert fused[1]._kv_len == plain[1]._kv_len


def test_decode_steps_at_batch_2_take_the_gemv_route(toy):
    cfg, model, ids, caches = toy

    def run(cache):
        return torch.stack([model(input_ids=ids[:, t:t + 1], past_key_values=cache, use_cache=True,
                                  cache_position=torch.tensor([t])).logits[:, -1]
                            for t in range(N_PREFILL, N_PREFILL + 3)], dim=1)
    fused, plain = _both(run, caches[2])
    assert [c[:3] for c in fused[2]] == _expected(cfg, "gemv_fused", 2) * 3, fused[2]
    assert fused[2][-1][3] == cfg.vocab_size
    _assert_same(cfg, fused, plain, N_PREFILL + 3)


def test_a_continuation_of_5_tokens_takes_the_rows_route(toy):
    cfg, model, ids, caches = toy

    def run(cache):
        return model(input_ids=ids[:1, N_PREFILL:N_PREFILL + 5], past_key_values=cache, use_cache=True,
                     cache_position=torch.tensor([N_PREFILL]), logits_to_keep=5).logits
    fused, plain = _both(run, caches[1])
    assert fused[0].shape == (1, 5, cfg.vocab_size)
    assert [c[:3] for c in fused[2]] == _expected(cfg, "linear_rows_fused", 5), fused[2]
    assert fused[2][-1][3] == cfg.vocab_size
    _assert_same(cfg, fused, plain, N_PREFILL + 5)


def test_speculative_steps_take_the_rows_route_and_roll_back(toy):
    cfg, model, ids, caches = toy

    def run(cache):
        cache.begin_speculation(3, 8)
        a = model(input_ids=ids[:1, N_PREFILL:N_PREFILL + 3], past_key_values=cache, use_cache=True,
                  cache_position=torch.tensor([N_PREFILL]), logits_to_keep=3).logits
        cache.commit(2)
        b = model(input_ids=ids[:1, N_PREFILL + 2:N_PREFILL + 4], past_key_values=cache, use_cache=True,
                  cache_position=torch.tensor([N_PREFILL + 2]), logits_to_keep=2).logits
        cache.commit(2)
        cache.end_speculation()
        return torch.cat([a, b], dim=1)
    fused, plain = _both(run, caches[1])
    want = _expected(cfg, "linear_rows_fused", 3) + _expected(cfg, "linear_rows_fused", 2)
    assert [c[:3] for c in fused[2]] == want, fused[2]
    _assert_same(cfg, fused, plain, N_PREFILL + 4)
    assert not fused[1].speculating and not plain[1].speculating
