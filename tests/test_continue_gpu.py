"""Continuation of a prefilled hybrid cache with several tokens in one forward, on the GPU: the T-token state update
(tv_selective_state_update_seq) against the fp64 recurrence, and the model-level identity — a prefill of n tokens + a
continuation of T gives, at the T positions, what one forward over n + T gives — against numbers the REFERENCE produced
(tests/golden/toy_realshape_g1.npz) and against T single-token steps on a cloned cache."""
import math

import pytest
import torch

from attn_accuracy import assert_rows_close
from conftest import golden_state_dict, load_golden
from oracle import ops as R

pytestmark = pytest.mark.gpu
DEV = "cuda"


def close(a, b, rtol, atol, what=""):
    a, b = a.detach().double().cpu(), torch.as_tensor(b).double().cpu()
    assert a.shape == b.shape, (a.shape, b.shape)
    err = (a - b).abs()
    bad = err > atol + rtol * b.abs()
    assert not bad.any(), f"{what}: {bad.sum().item()} / {bad.numel()} out of tolerance, max abs err {err.max().item():.3e}"


def relerr(a, b):
    a, b = a.detach().double().cpu(), torch.as_tensor(b).double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-12)).item()


@pytest.fixture(scope="module")
def K():
    from timeviper_amd import kernels
    return kernels


def scan_inputs(B, L, H, P, G, N, seed, dtype):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, L, H, P, generator=g).to(dtype)
    dt = (torch.randn(B, L, H, generator=g) * 0.5).to(dtype)
    A = -(torch.rand(H, generator=g) * 15 + 1)
    Bm = (torch.randn(B, L, G, N, generator=g) * 0.5).to(dtype)
    Cm = (torch.randn(B, L, G, N, generator=g) * 0.5).to(dtype)
    D = torch.rand(H, generator=g) + 0.5
    dtv = torch.exp(torch.rand(H, generator=g) * (math.log(0.1) - math.log(1e-3)) + math.log(1e-3))
    dt_bias = dtv + torch.log(-torch.expm1(-dtv))
    return x, dt, A, Bm, Cm, D, dt_bias


GUARD = 7.25       # rows behind `state` and `y` that no launch may touch


@pytest.mark.parametrize("group_major", [False, True])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("T", [1, 2, 5, 64])
@pytest.mark.parametrize("B,H,P,G,N", [(2, 8, 16, 2, 32), (1, 128, 80, 8, 128), (3, 4, 24, 1, 16), (1, 6, 7, 3, 256),
                                       (1, 4, 8, 2, 40)])      # (N = 40: the thread-per-row kernel)
def test_selective_state_update_seq(K, B, H, P, G, N, T, dtype, group_major):
    """y: the tolerance of test_selective_state_update.  State after T tokens: within 2 x the error that T successive
    calls of the single-token kernel leave against the same fp64 recurrence (same arithmetic; the factor covers another
    expf / FMA contraction order).  T = 1: the single-token kernel's bits."""
    x, dt, A, Bm, Cm, D, dt_bias = scan_inputs(B, T, H, P, G, N, 9 + T, dtype)
    st = torch.randn(B, H, P, N, generator=torch.Generator().manual_seed(2))
    y_ref, fin_ref, _ = R.ssd_recurrence_ref(x.float(), dt.float(), A, Bm.float(), Cm.float(), D=D, dt_bias=dt_bias,
                                             initial_states=st)
    d = lambda t: t.to(DEV)
    # the existing kernel, T calls
    s_old = d(st).clone()
    y_old = [K.selective_state_update(s_old, d(x[:, t]), d(dt[:, t]), d(A), d(Bm[:, t]), d(Cm[:, t]), d(D),
                                      dt_bias=d(dt_bias), dt_softplus=True) for t in range(T)]
    err_old = (s_old.double().cpu() - fin_ref.double()).abs().max().item()
    # the new kernel: state and y with guard rows behind them
    rows = B * H * P
    sbuf = torch.full((rows + 3, N), GUARD, device=DEV)
    sbuf[:rows] = d(st).view(rows, N)
    s_new = sbuf[:rows].view(B, H, P, N)
    if group_major:        # the (B, T, G, N) views of group-major storage that causal_conv1d_xbc returns
        Bd, Cd = d(Bm).transpose(1, 2).contiguous().transpose(1, 2), d(Cm).transpose(1, 2).contiguous().transpose(1, 2)
    else:
        Bd, Cd = d(Bm), d(Cm)
    ybuf = torch.full((B, T + 1, H, P), GUARD, device=DEV).to(dtype)        # one guard token row behind every batch entry
    y = K.selective_state_update_seq(s_new, d(x), d(dt), d(A), Bd, Cd, D=d(D), dt_bias=d(dt_bias), dt_softplus=True,
                                     out=ybuf[:, :T])
    torch.cuda.synchronize()
    assert y.data_ptr() == ybuf.data_ptr() and torch.all(ybuf[:, T] == GUARD), "rows behind y were written"
    assert y.shape == (B, T, H, P) and y.dtype == dtype
    err_new = (s_new.double().cpu() - fin_ref.double()).abs().max().item()
    print(f"state error after {T} tokens: single-token kernel {err_old:.3e}, sequence kernel {err_new:.3e}")
    close(y, y_ref, 2e-2, 2e-2, "y")
    close(torch.stack(y_old, dim=1), y_ref, 2e-2, 2e-2, "y of the single-token kernel")
    assert err_new <= 2 * err_old, (err_new, err_old)
    assert torch.all(sbuf[rows:] == GUARD), "rows behind the state were written"
    assert K.selective_state_update_seq_last_impl() == (2 if N == 40 else 1)      # lanes share a row / a thread per row
    if T == 1:
        assert torch.equal(s_new, s_old) and torch.equal(y[:, 0], y_old[0])


def test_selective_state_update_seq_dt_limit(K):
    """dt is clamped like the prefill scan's; a state that is not fp32 is refused."""
    B, T, H, P, G, N = 1, 6, 8, 16, 2, 64
    x, dt, A, Bm, Cm, D, dt_bias = scan_inputs(B, T, H, P, G, N, 4, torch.bfloat16)
    st = torch.randn(B, H, P, N, generator=torch.Generator().manual_seed(3))
    lim = (0.02, 0.3)
    y_ref, fin_ref, _ = R.ssd_recurrence_ref(x.float(), dt.float(), A, Bm.float(), Cm.float(), D=D, dt_bias=dt_bias,
                                             initial_states=st, dt_limit=lim)
    d = lambda t: t.to(DEV)
    s = d(st).clone()
    y = K.selective_state_update_seq(s, d(x), d(dt), d(A), d(Bm), d(Cm), D=d(D), dt_bias=d(dt_bias), dt_softplus=True,
                                     dt_limit=lim)
    close(y, y_ref, 2e-2, 2e-2, "y")
    close(s, fin_ref, 1e-4, 1e-5, "state")
    with pytest.raises(K.TimeViperHipError):
        K.selective_state_update_seq(s.half(), d(x), d(dt), d(A), d(Bm), d(Cm))


# ------------------------------------------------------------------ attention of a continuation
def _append_case(K, B, T, Lk, Hq, Hkv, seed):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, T, Hq, 128, generator=g).bfloat16()
    k = torch.randn(B, Lk, Hkv, 128, generator=g).bfloat16()
    v = torch.randn(B, Lk, Hkv, 128, generator=g).bfloat16()
    o_ref, lse_ref = R.attention_ref(q.float(), k.float(), v.float(), True)
    qd, kd, vd = q.to(DEV), k.to(DEV), v.to(DEV)
    calls = K.flash_attn_append_calls()
    o, lse = K.flash_attn_append(qd, kd, vd, return_lse=True)
    assert K.flash_attn_append_calls() == calls + 1, "fell back to the prefill kernel"
    assert torch.isfinite(o.float()).all() and torch.isfinite(lse).all()
    close(o, o_ref, 2e-2, 1e-2, "o")
    assert_rows_close(o, o_ref, torch.bfloat16, f"append B {B} T {T} Lk {Lk} H {Hq}/{Hkv}")
    close(lse, lse_ref, 1e-3, 2e-3, "lse")
    o2 = K.flash_attn_func(qd, kd, vd, causal=True)
    close(o, o2.float().cpu(), 2e-2, 1e-2, "against the prefill kernel")
    assert_rows_close(o2, o_ref, torch.bfloat16, f"prefill kernel on the append case T {T} Lk {Lk} H {Hq}/{Hkv}")


@pytest.mark.parametrize("B,T,Lk,Hq,Hkv", [
    (1, 3, 1000, 40, 8),      # gq 5: 15 columns, one block
    (1, 4, 777, 40, 8),       # 20 columns: a partly filled second block
    (2, 2, 3000, 16, 1),      # gq 16: a token per block
    (1, 3, 2500, 40, 2),      # gq 20: 60 columns, tokens straddle the blocks
    (1, 8, 8, 8, 2),          # T = Lk: the causal prefill of a tiny sequence (token 0 sees key 0 alone)
    (2, 5, 37, 12, 4),        # one step and a bit
    (1, 8, 1027, 32, 8),      # the masked keys 1020 .. 1026 straddle the 32-key step at 1024
    (1, 8, 963, 32, 8),       # 11 splits of 96 keys: the masked keys 956 .. 962 straddle the split boundary at 960
    (1, 8, 32868, 40, 8),     # the bench's cache (2 048 frames), Nano-9B heads
    (1, 64, 4099, 8, 4),      # the most query tokens the kernel takes: 128 columns
])
def test_flash_attn_append(K, B, T, Lk, Hq, Hkv):
    """The last T tokens as queries against the cache (bottom-right causal): fp32 oracle with the tolerances of
    test_flash_attn_decode_split_kv, and the prefill kernel on the same tensors.  Every case runs on the split-KV kernel."""
    _append_case(K, B, T, Lk, Hq, Hkv, Lk + Hq + T)


def test_flash_attn_append_device_lengths_and_strided_cache(K):
    """seqlens_k on the device, NaN-filled capacity behind the length, K / V as views of larger buffers."""
    g = torch.Generator().manual_seed(5)
    B, T, cap, Hq, Hkv = 3, 4, 1500, 40, 8
    lens = [1500, 4, 700]
    q = torch.randn(B, T, Hq, 128, generator=g).bfloat16().to(DEV)
    kbuf = torch.randn(B, cap + 64, Hkv, 128, generator=g).bfloat16().to(DEV)
    vbuf = torch.randn(B, cap + 64, Hkv, 128, generator=g).bfloat16().to(DEV)
    for b, n in enumerate(lens):
        kbuf[b, n:] = float("nan")
        vbuf[b, n:] = float("nan")
    k, v = kbuf[:, :cap], vbuf[:, :cap]
    sl = torch.tensor(lens, dtype=torch.int32, device=DEV)
    calls = K.flash_attn_append_calls()
    o, lse = K.flash_attn_append(q, k, v, seqlens_k=sl, return_lse=True)
    assert K.flash_attn_append_calls() == calls + 1
    assert torch.isfinite(o.float()).all() and torch.isfinite(lse).all()
    for b, n in enumerate(lens):
        o_ref, lse_ref = R.attention_ref(q[b:b + 1].float().cpu(), k[b:b + 1, :n].float().cpu(), v[b:b + 1, :n].float().cpu(), True)
        close(o[b:b + 1], o_ref, 2e-2, 1e-2, f"o[{b}]")
        assert_rows_close(o[b:b + 1], o_ref, torch.bfloat16, f"append device length {n}")
        close(lse[b:b + 1], lse_ref, 1e-3, 2e-3, f"lse[{b}]")
    with pytest.raises(K.TimeViperHipError):
        K.flash_attn_append(q, k, v, seqlens_k=sl.to(torch.int64))


def test_flash_attn_append_outside_its_range_runs_the_prefill_kernel(K):
    g = torch.Generator().manual_seed(6)
    q = torch.randn(1, 70, 8, 128, generator=g).bfloat16().to(DEV)           # 70 query tokens > 64
    k = torch.randn(1, 500, 2, 128, generator=g).bfloat16().to(DEV)
    v = torch.randn(1, 500, 2, 128, generator=g).bfloat16().to(DEV)
    calls = K.flash_attn_append_calls()
    o = K.flash_attn_append(q, k, v)
    assert K.flash_attn_append_calls() == calls
    assert torch.equal(o, K.flash_attn_func(q, k, v, causal=True))


# ------------------------------------------------------------------ model level
def _realshape_model(tag, group_map):
    from timeviper_amd.model.llm.nano import NemotronHConfig, NemotronHForCausalLM
    g = load_golden(f"toy_realshape_{tag}")
    L, ndec, G = (int(v) for v in g["meta"])
    cfg = NemotronHConfig(vocab_size=96, hidden_size=128, intermediate_size=192, num_hidden_layers=3,
                          hybrid_override_pattern="M*-", num_attention_heads=4, head_dim=128, num_key_value_heads=2,
                          ssm_state_size=128, mamba_num_heads=8, mamba_n_groups=G, mamba_head_dim=80, mamba_chunk_size=64,
                          rescale_prenorm_residual=False)
    model = NemotronHForCausalLM(cfg)
    model.load_state_dict(golden_state_dict(g), strict=True)
    model = model.to(DEV).bfloat16().eval()
    for blk in model.backbone.layers:
        if blk.block_type == "mamba":
            blk.mixer.group_map = group_map
    return cfg, model, g, L, ndec


def test_realshape_prefill_plus_continuation_vs_reference_golden():
    """Nano-9B's head shapes (P 80, N 128, d 128) against the reference's own 304-position logits: prefill 300 +
    continue 4 in ONE forward (the in-place sequence kernel), prefill 150 + continue 154 (the scan from the cached
    state), prefill 150 + continue 100 + continue 50 (both above T_seq: the scan) + 4 single steps.  relerr < 3e-2 at every position, the bound of
    test_realshape_prefill_plus_graphed_fused_decode_vs_reference_golden for the same positions."""
    from timeviper_amd import kernels as K
    from timeviper_amd.model.llm import nano
    cfg, model, g, L, ndec = _realshape_model("g1", "block")
    emb = torch.from_numpy(g["embeds"]).to(DEV).bfloat16()
    ref = torch.from_numpy(g["logits"])
    tot = L + ndec
    assert (L, tot) == (300, 304) and nano.continue_t_seq() == nano.CONTINUE_T_SEQ

    def prefill(n):
        cache = nano.HybridMambaAttentionDynamicCache(cfg, 1, dtype=torch.bfloat16, device=DEV)
        model(inputs_embeds=emb[:, :n], past_key_values=cache, use_cache=True,
              cache_position=torch.zeros(1, dtype=torch.long))
        assert K.ssd_scan_last_impl() == 6
        return cache

    def cont(cache, a, b, want):
        nano.CONTINUE_LAST_PATH = None
        calls = K.flash_attn_append_calls()
        out = model(inputs_embeds=emb[:, a:b], past_key_values=cache, use_cache=True, cache_position=torch.tensor([a]),
                    logits_to_keep=0).logits
        assert nano.CONTINUE_LAST_PATH == want and out.shape[1] == b - a
        if want == "seq":
            assert K.selective_state_update_seq_last_impl() == 1
        # one attention layer: the split-KV continuation kernel up to 64 query tokens, the prefill kernel beyond
        assert K.flash_attn_append_calls() - calls == (1 if b - a <= 64 else 0)
        assert cache.get_seq_length() == b
        for i in range(b - a):
            err = relerr(out[:, i], ref[:, a + i])
            assert err < 3e-2, (a + i, err)
        return out

    with torch.inference_mode():
        assert 4 <= nano.continue_t_seq() < 50
        cont(prefill(L), L, tot, "seq")
        cont(prefill(150), 150, tot, "scan")
        cache = prefill(150)
        cont(cache, 150, 250, "scan")
        cont(cache, 250, 300, "scan")
        for t in range(300, tot):
            o = model(inputs_embeds=emb[:, t:t + 1], past_key_values=cache, use_cache=True,
                      cache_position=torch.tensor([t])).logits
            err = relerr(o[:, -1], ref[:, t])
            assert err < 3e-2, (t, err)


def _toy_hybrid_d128(pattern="M-*M*-"):
    from timeviper_amd.model.llm.nano import NemotronHConfig, NemotronHForCausalLM
    torch.manual_seed(11)
    cfg = NemotronHConfig(vocab_size=256, hidden_size=256, intermediate_size=384, num_hidden_layers=len(pattern),
                          hybrid_override_pattern=pattern, num_attention_heads=8, head_dim=128,
                          num_key_value_heads=2, ssm_state_size=16, mamba_num_heads=8,
                          mamba_n_groups=2, mamba_head_dim=16, mamba_chunk_size=16)
    model = NemotronHForCausalLM(cfg).to(DEV).bfloat16().eval()
    with torch.no_grad():       # spread the logits: N(0, 0.02) weights give near-uniform attention and near-tied tokens
        for blk in model.backbone.layers:
            if blk.block_type == "attention":
                blk.mixer.q_proj.weight.mul_(8.0)
                blk.mixer.k_proj.weight.mul_(8.0)
        model.lm_head.weight.mul_(20.0)
    return cfg, model


@pytest.mark.parametrize("T", [2, 8, 33])
def test_continuation_equals_single_steps_bf16(T):
    """Same operators, other summation order: relerr < 3e-2 per position (test_prefill_plus_decode_matches_full_prefill's
    bound).  Greedy ids are compared where the stepwise run's top-2 logit gap exceeds the largest logit difference
    between the two runs at that position; at most 10 % of the positions may fall under that."""
    from timeviper_amd.model.llm import nano
    cfg, model = _toy_hybrid_d128()
    n = 300
    ids = torch.randint(0, cfg.vocab_size, (1, n + T), generator=torch.Generator().manual_seed(7)).to(DEV)
    with torch.inference_mode():
        cache = nano.HybridMambaAttentionDynamicCache(cfg, 1, dtype=torch.bfloat16, device=DEV)
        model(input_ids=ids[:, :n], past_key_values=cache, use_cache=True, cache_position=torch.zeros(1, dtype=torch.long))
        steps = cache.clone()
        cont = model(input_ids=ids[:, n:], past_key_values=cache, use_cache=True, cache_position=torch.tensor([n]),
                     logits_to_keep=T).logits
        assert nano.CONTINUE_LAST_PATH == ("seq" if T <= nano.continue_t_seq() else "scan")
        single = torch.stack([model(input_ids=ids[:, t:t + 1], past_key_values=steps, use_cache=True,
                                    cache_position=torch.tensor([t])).logits[:, -1] for t in range(n, n + T)], dim=1)
    left_out = 0
    for i in range(T):
        err = relerr(cont[:, i], single[:, i])
        assert err < 3e-2, (i, err)
        top2 = single[0, i].float().topk(2).values
        gap, diff = float(top2[0] - top2[1]), float((cont[0, i] - single[0, i]).abs().max())
        if gap > diff:
            assert int(cont[0, i].argmax()) == int(single[0, i].argmax()), i
        else:
            left_out += 1
    print(f"T {T}: {left_out} of {T} positions with a top-2 gap under the logit difference")
    assert left_out <= 0.1 * T, (left_out, T)
    for i, c in enumerate(cfg.hybrid_override_pattern):
        if c == "M":
            # (the pre-conv rows of deeper layers come out of T-row GEMMs here and one-row products there: bf16
            # round-off apart — the bound the fused / unfused decode steps' states are compared with)
            assert relerr(cache.ssm_states[i], steps.ssm_states[i]) < 2e-2
            assert relerr(cache.conv_states[i], steps.conv_states[i]) < 2e-2
        elif c == "*":
            assert cache.key_cache[i].shape == steps.key_cache[i].shape == (1, n + T, 2, 128)


TWO_TURN_SEED = 0          # model / pixel seed of the two-turn test, chosen by the criterion in its docstring


def test_generate_two_turns_with_graphed_decode_equal_the_eager_transcript(monkeypatch):
    """Turn 1 with `return_past_key_values=True`, turn 2 from its cache: ONE continuation forward (pending id + question
    + answer prompt), then the captured decode step again — the ids of the eager single-call generate over the
    concatenated transcript.  Uniform token drop (the follow-up sees the cache as the first turn compressed it).

    The two runs are the same function of the same tokens on different kernels: the first turn's answer tokens go through
    the decode kernels in one and through the prefill kernels in the other, a bf16 difference that
    test_prefill_plus_decode_matches_full_prefill bounds by a relative L2 error of 3e-2 of the logits, i.e. an rms error of
    3e-2 rms(logits) per logit.  Greedy ids can only be required to agree where the REFERENCE run (the single call) has no
    near-tie on that scale, so the random model is picked (TWO_TURN_SEED, the smallest seed that does) such that, at every
    generated position of the single call, the top-2 logit gap exceeds 3 sqrt(2) 3e-2 rms(logits) — three standard
    deviations of the difference of two logits' errors.  The test asserts that property of the reference run before it
    compares, so a change of the seed or of the model cannot silently bring the near-ties back."""
    from timeviper_amd.model import build_synthetic_timeviper
    from timeviper_amd.model.llm import decode_graph
    from timeviper_amd.model.llm.nano import NemotronHConfig
    cfg = NemotronHConfig(vocab_size=128, hidden_size=256, intermediate_size=384, num_hidden_layers=8,
                          hybrid_override_pattern="M*-M*-M*", num_attention_heads=4, head_dim=128,
                          num_key_value_heads=2, ssm_state_size=16, mamba_num_heads=8,
                          mamba_n_groups=2, mamba_head_dim=16, mamba_chunk_size=16)
    vlm = build_synthetic_timeviper(cfg, "siglip-vit-b16-224px", pdrop_type="uni_2_0.75-uni_5_0.5",
                                    merge_module="no_merge", vit_depth=2, image_size=96, seed=TWO_TURN_SEED)
    with torch.no_grad():       # spread the logits
        for blk in vlm.llm_backbone.llm.backbone.layers:
            if blk.block_type == "attention":
                blk.mixer.q_proj.weight.mul_(10.0)
                blk.mixer.k_proj.weight.mul_(10.0)
        vlm.llm_backbone.llm.lm_head.weight.mul_(20.0)
    T, N = 40, 8                 # 40 frames x 16 tokens: every cache holds >= 256 keys after the drops; 8 tokens a turn
    tok = vlm.default_token_id
    ids1 = torch.tensor([[5, 6, 7] + [tok] * T + [8, 9, 10, 11]], device=DEV)
    ids2 = torch.tensor([[12, 13, 14, 15, 16, 17]], device=DEV)
    pix = torch.randn(T, 3, 96, 96, generator=torch.Generator().manual_seed(TWO_TURN_SEED)).to(DEV).bfloat16()
    replays = []
    orig_step = decode_graph.GraphedDecodeStep.step

    def counting_step(self, t):
        out = orig_step(self, t)
        replays.append(self.graph is not None)
        return out
    monkeypatch.setattr(decode_graph.GraphedDecodeStep, "step", counting_step)
    kw = dict(max_new_tokens=N, return_ids=True, eos_token_id=-1)
    first, cache = vlm.generate(ids1, pixel_values_videos=pix, return_past_key_values=True, **kw)
    assert len(replays) == N and all(replays[2:]) and cache.static_decode
    replays.clear()
    second = vlm.generate(ids2, past_key_values=cache, answer_prompt="Best Options: (", **kw)
    assert len(replays) == N and replays[:2] == [False, False] and all(replays[2:])
    monkeypatch.setenv("TV_DECODE_GRAPH", "0")
    replays.clear()
    transcript = torch.cat([ids1, first, ids2], dim=1)
    eager = vlm.generate(transcript, pixel_values_videos=pix, answer_prompt="Best Options: (", **kw)
    assert replays == []
    assert second.shape == eager.shape == (1, N)
    # the reference run has no near-tie (see the docstring): its own logits at the generated positions, by one prefill
    ap = vlm.llm_backbone.tokenizer("Best Options: (", add_special_tokens=False, return_tensors="pt").input_ids.to(DEV)
    with torch.inference_mode():
        lg = vlm(input_ids=torch.cat([transcript, ap, eager[:, :-1]], dim=1), pixel_values_videos=pix,
                 logits_to_keep=N).logits[0].float()
    top2 = lg.topk(2, dim=-1).values
    margin = (top2[:, 0] - top2[:, 1]) / lg.pow(2).mean(-1).sqrt()
    print("top-2 gap / rms(logits) of the single call:", [round(m, 3) for m in margin.tolist()])
    assert margin.min().item() > 3 * math.sqrt(2) * 3e-2, margin.tolist()
    assert torch.equal(second, eager), (second.tolist(), eager.tolist())
