"""K.quantize_rows_e4m3 (e4m3 weights with one power-of-two fp32 scale per output row) and the host logic of
NemotronHForCausalLM.quantize_weights_e4m3, on the CPU."""
import pytest
import torch

from timeviper_amd import kernels as K

STDS = [1e-3, 0.02, 1.0]
N, KD = 48, 1008


def _rows(std, seed=0):
    g = torch.Generator().manual_seed(seed)
    W = (torch.randn(N, KD, generator=g) * std).bfloat16()
    W[5] = 0                                       # one all-zero row
    return W


@pytest.fixture(scope="module", params=STDS)
def case(request):
    W = _rows(request.param)
    w8, scale = K.quantize_rows_e4m3(W)
    return W, w8, scale


def test_layout(case):
    W, w8, scale = case
    assert w8.dtype == torch.float8_e4m3fn and w8.shape == W.shape and w8.stride(1) == 1 and w8.stride(0) % 16 == 0
    assert scale.dtype == torch.float32 and scale.shape == (N,)


def test_scales_are_powers_of_two_in_range(case):
    W, w8, scale = case
    mant, _ = torch.frexp(scale)
    assert torch.equal(mant, torch.full_like(mant, 0.5))           # 2^e exactly
    amax = W.float().abs().amax(dim=1)
    ratio = amax / scale
    nz = amax > 0
    assert (ratio[nz] > 224).all() and (ratio[nz] <= 448).all(), (ratio.min().item(), ratio.max().item())
    assert float(scale[5]) == 1.0 and not nz[5]


def test_dequantization_is_exactly_bf16(case):
    W, w8, scale = case
    deq = w8.float() * scale[:, None]
    assert torch.equal(deq.bfloat16().float(), deq)
    assert torch.equal(K.dequantize_rows_e4m3(w8, scale).float(), deq)


def test_error_bound(case):
    """|W^ - W| <= 2^-4 |W| + scale 2^-10: half an ulp of 3 mantissa bits, plus half the subnormal spacing 2^-9."""
    W, w8, scale = case
    Wf = W.float().double()
    deq = (w8.float() * scale[:, None]).double()
    err = (deq - Wf).abs()
    bound = 2.0 ** -4 * Wf.abs() + scale[:, None].double() * 2.0 ** -10
    print(f"max err / bound {(err / bound.clamp_min(1e-300)).max().item():.3f}")
    assert (err <= bound).all()


def test_no_nan_byte(case):
    W, w8, scale = case
    b = w8.contiguous().view(torch.uint8)
    assert not ((b == 0x7F) | (b == 0xFF)).any()
    assert torch.equal(b[5], torch.zeros_like(b[5]))


def test_boundaries_and_padding():
    """amax exactly 448 2^e and 224 2^e (where log2 alone may land either side), and a K that is no multiple of 16."""
    W = torch.zeros(4, 24).bfloat16()
    W[0, 0], W[1, 3], W[2, 7], W[3, 1] = 448.0, 224.0, -448.0 / 1024, 1.0
    w8, scale = K.quantize_rows_e4m3(W)
    assert scale.tolist() == [1.0, 0.5, 1.0 / 1024, 1.0 / 256]
    assert torch.equal(w8.float() * scale[:, None], W.float())
    assert w8.stride(0) == 32 and w8.shape == (4, 24)
    with pytest.raises(K.TimeViperHipError):
        K.quantize_rows_e4m3(W.float())
    W[0, 0] = float("inf")
    with pytest.raises(K.TimeViperHipError):
        K.quantize_rows_e4m3(W)


# ------------------------------------------------------------------ host logic on a toy model
def _toy(tie=False):
    from timeviper_amd.model.llm.nano import NemotronHConfig, NemotronHForCausalLM
    torch.manual_seed(3)
    cfg = NemotronHConfig(vocab_size=64, hidden_size=64, intermediate_size=96, num_hidden_layers=3,
                          hybrid_override_pattern="M*-", num_attention_heads=4, head_dim=16, num_key_value_heads=2,
                          ssm_state_size=16, mamba_num_heads=8, mamba_n_groups=2, mamba_head_dim=8, mamba_chunk_size=16)
    model = NemotronHForCausalLM(cfg).bfloat16().eval()
    if tie:
        model.lm_head.weight = model.backbone.embeddings.weight
    return model


def _copies(model):
    return [m for m in model.modules() if getattr(m, "_fp8w", None) is not None]


def test_model_quantize_in_place_and_skips():
    from timeviper_amd.model.llm import nano
    model = _toy()
    before = {k: v.clone() for k, v in model.state_dict().items()}
    n = model.quantize_weights_e4m3()
    linears = [m for blk in model.backbone.layers for m in blk.mixer.modules() if isinstance(m, torch.nn.Linear)]
    assert n == len(linears) + 1 == 2 + 4 + 2 + 1 and model.has_fp8_weights()
    for m in linears + [model.lm_head]:
        key, w8, scale = m._fp8w
        assert key == K.param_key((m.weight,))
        assert torch.equal(m.weight, K.dequantize_rows_e4m3(w8, scale))          # the weight IS its dequantized copy
        assert nano.fp8_copy(m, (m.weight,)) is not None
    # everything that is no linear weight of a block (embeddings, norms, conv, A / D / dt, biases) is untouched
    quantized = {id(m.weight) for m in linears + [model.lm_head]}
    for name, p in model.named_parameters():
        if id(p) not in quantized:
            assert torch.equal(p, before[name]), name
        else:
            assert not torch.equal(p, before[name]), name
    # the attention block's [q; k; v] copy is the concatenation of the three
    att = model.backbone.layers[1].mixer
    key, w8, scale = att._fp8w
    assert torch.equal(w8.view(torch.uint8), torch.cat([p._fp8w[1] for p in (att.q_proj, att.k_proj, att.v_proj)]).view(torch.uint8))
    assert torch.equal(K.dequantize_rows_e4m3(w8, scale), att._qkv_weight())
    # quantizing again changes nothing: the rounded weights are fixed points
    snap = {k: v.clone() for k, v in model.state_dict().items()}
    model.quantize_weights_e4m3()
    assert all(torch.equal(v, snap[k]) for k, v in model.state_dict().items())


def test_switch_stale_key_and_drops(monkeypatch):
    from timeviper_amd.model.llm import nano
    model = _toy()
    model.quantize_weights_e4m3()
    lin = model.backbone.layers[0].mixer.in_proj
    monkeypatch.setenv("TV_FP8W", "0")
    assert nano.fp8_copy(lin, (lin.weight,)) is None and lin._fp8w is not None      # bf16 without dropping anything
    monkeypatch.delenv("TV_FP8W")
    assert nano.fp8_copy(lin, (lin.weight,)) is not None
    with torch.no_grad():
        lin.weight.mul_(2.0)                       # rewritten: the key no longer matches, the copy is not used
    assert nano.fp8_copy(lin, (lin.weight,)) is None
    other = model.backbone.layers[0].mixer.out_proj
    assert nano.fp8_copy(other, (other.weight,)) is not None
    model.drop_fp8_weights()
    assert not _copies(model) and not model.has_fp8_weights()

    model.quantize_weights_e4m3()
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    assert _copies(model)
    model.load_state_dict(sd)
    assert not _copies(model)
    model.quantize_weights_e4m3()
    model.to(torch.float32)
    assert not _copies(model) and not model.has_fp8_weights()
    with pytest.raises(TypeError):
        model.quantize_weights_e4m3()              # bf16 matrices only: never a silent conversion


def test_tied_lm_head_is_skipped():
    model = _toy(tie=True)
    emb = model.backbone.embeddings.weight.clone()
    n = model.quantize_weights_e4m3()
    assert n == 8 and getattr(model.lm_head, "_fp8w", None) is None
    assert torch.equal(model.backbone.embeddings.weight, emb)


def test_vlm_forwarding_and_qwen2():
    from timeviper_amd.model.generic_vlm import GenericTimeViperVLM

    class _Backbone:
        def __init__(self, llm):
            self.llm = llm
    vlm = GenericTimeViperVLM.__new__(GenericTimeViperVLM)
    torch.nn.Module.__init__(vlm)
    object.__setattr__(vlm, "llm_backbone", _Backbone(_toy()))
    assert vlm.quantize_llm_weights_e4m3() == 9 and vlm.llm_backbone.llm.has_fp8_weights()
    vlm.drop_llm_fp8_weights()
    assert not vlm.llm_backbone.llm.has_fp8_weights()
    object.__setattr__(vlm, "llm_backbone", _Backbone(torch.nn.Linear(4, 4)))       # (any backbone without the method: Qwen2)
    with pytest.raises(NotImplementedError):
        vlm.quantize_llm_weights_e4m3()
    with pytest.raises(NotImplementedError):
        vlm.drop_llm_fp8_weights()
