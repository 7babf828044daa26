"""Model-level parity on the GPU: the host-side mirror (timeviper_amd.model) with HIP
kernels against reference golden vectors and the CPU oracle."""
import numpy as np
import pytest
import torch

from conftest import golden_state_dict, load_golden
from oracle import model as om
from oracle import ops as R
from oracle import vit as ov
from test_model_cpu import PD, toy_config

pytestmark = pytest.mark.gpu
DEV = "cuda"


def relerr(a, b):
    a, b = a.detach().double().cpu(), torch.as_tensor(b).double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-12)).item()


def mixer_from_golden(g, group_map, dtype):
    from timeviper_amd.model.llm.nano import NemotronHMamba2Mixer
    G, H, P, N, Q, K = (int(v) for v in g["meta"])
    cfg = toy_config(mamba_n_groups=G, mamba_num_heads=H, mamba_head_dim=P, ssm_state_size=N,
                     mamba_chunk_size=Q)
    m = NemotronHMamba2Mixer(cfg, 0)
    m.load_state_dict(golden_state_dict(g), strict=True)
    m.group_map = group_map
    return m.to(DEV).to(dtype).eval(), cfg


@pytest.mark.parametrize("tag,gmap", [("g1", "block"), ("g2_tile", "tile"), ("g4_tile", "tile")])
def test_mixer_fp32_matches_reference(tag, gmap):
    """fp32 end to end: in_proj -> conv -> scan -> gated norm -> out_proj, plus cache states."""
    from timeviper_amd.model.llm.nano import HybridMambaAttentionDynamicCache
    g = load_golden(f"mixer_{tag}")
    m, cfg = mixer_from_golden(g, gmap, torch.float32)
    cache = HybridMambaAttentionDynamicCache(cfg, 2, dtype=torch.float32, device=DEV)
    with torch.no_grad():
        out = m(torch.from_numpy(g["hidden"]).to(DEV), cache_params=cache,
                cache_position=torch.zeros(1, dtype=torch.long))
    assert torch.allclose(out.cpu(), torch.from_numpy(g["out"]), rtol=2e-4, atol=2e-5)
    assert torch.allclose(cache.ssm_states[0].cpu(), torch.from_numpy(g["scan_final"]), rtol=2e-4, atol=2e-5)
    assert torch.allclose(cache.conv_states[0].cpu(), torch.from_numpy(g["conv_state"]), rtol=1e-4, atol=1e-5)


def test_mixer_bf16_close_to_reference():
    g = load_golden("mixer_g1")
    m, _ = mixer_from_golden(g, "block", torch.bfloat16)
    with torch.no_grad():
        out = m(torch.from_numpy(g["hidden"]).to(DEV).bfloat16())
    assert relerr(out, g["out"]) < 3e-2


def load_toy(tag, kw, dtype):
    from timeviper_amd.model.llm.nano import NemotronHForCausalLM
    g = load_golden(f"toy_{tag}")
    model = NemotronHForCausalLM(toy_config(**kw))
    model.load_state_dict(golden_state_dict(g), strict=True)
    return model.to(DEV).to(dtype).eval(), g


def pargs(g):
    tb, nv, ta = (int(v) for v in g["meta"])
    return {"first_vision_token_positions": torch.tensor([tb]), "text_prompt_lens": [tb + ta],
            "num_vision_tokens": [nv], "is_interleaved": False}


@pytest.mark.parametrize("tag,kw", [("plain", {}),
                                    ("pdrop_nomerge", dict(use_pdrop=True, pdrop_type=PD)),
                                    ("pdrop_transv", dict(use_pdrop=True, pdrop_type=PD,
                                                          merge_module="CrossAttention"))])
def test_toy_model_bf16_vs_reference(tag, kw):
    model, g = load_toy(tag, kw, torch.bfloat16)
    emb = torch.from_numpy(g["embeds"]).to(DEV).bfloat16()
    extra = {"train_pdrop_args": pargs(g)} if kw else {}
    with torch.no_grad():
        out = model(inputs_embeds=emb, output_hidden_states=True, logits_to_keep=0, **extra)
    lens = [h.shape[1] for h in out.hidden_states[:-1]]   # per-layer length after any pdrop
    assert lens == list(g["layer_lens"])
    assert out.logits.shape == g["logits"].shape
    if not kw:
        assert relerr(out.logits, g["logits"]) < 6e-2
    else:
        tr = [t["kept"].cpu() for t in model.backbone.last_pdrop_trace]
        tb, nv, ta = (int(v) for v in g["meta"])
        # stage 0 is "uni": bit-exact integer indices
        assert torch.equal(tr[0], R.uniform_keep_indices_ref(nv, 30) + tb)
        assert [len(t) for t in tr] == [30, 20, 10]
        # "attn" stages rank bf16 scores here and fp32 scores in the reference: follow this
        # run's selection in the oracle so the remaining arithmetic is comparable
        sd = golden_state_dict(g)
        cfg = om.OracleConfig.from_hf(model.config, pdrop_type=PD, merge_module=kw.get("merge_module", "no_merge"))
        col = {}
        ref = om.causal_lm_ref(sd, cfg, torch.from_numpy(g["embeds"]), pargs(g), forced_kept=tr, collect=col)
        assert relerr(out.logits, ref) < 6e-2
        own = {}
        om.causal_lm_ref(sd, cfg, torch.from_numpy(g["embeds"]), pargs(g), collect=own)
        if all(torch.equal(a, b) for a, b in zip(tr, own["kept"])):
            assert relerr(out.logits, g["logits"]) < 6e-2
    # default logits_to_keep: last position only (the reference computes all L, :2433)
    with torch.no_grad():
        last = model(inputs_embeds=emb, **extra).logits
    assert last.shape[1] == 1 and torch.equal(last[:, 0], out.logits[:, -1])


def test_pdrop_stage_indices_exact_vs_oracle_fp32():
    """Same hidden states into the oracle's pdrop stage and ours (fp32, no merge): kept
    indices and the gathered features must be identical."""
    model, g = load_toy("pdrop_nomerge", dict(use_pdrop=True, pdrop_type=PD), torch.float32)
    sd = golden_state_dict(g)
    cfg = om.OracleConfig.from_hf(model.config, pdrop_type=PD, merge_module="no_merge")
    tb, nv, ta = (int(v) for v in g["meta"])
    gen = torch.Generator().manual_seed(3)
    for stage, layer, n_img in [(0, 2, 40), (1, 3, 30), (2, 6, 20)]:
        L = tb + n_img + ta
        feats = torch.randn(1, L, 64, generator=gen)
        new_ref, kept_ref, dropped_ref = om.pdrop_stage_ref(sd, "backbone.", cfg, feats, stage, layer,
                                                            tb, nv, tb + ta)
        with torch.no_grad():
            _, _, new, _, _ = model.backbone.pdrop_no_pack(
                feats.to(DEV), stage, layer, model.backbone.pdrop_compress_types[stage], None, None,
                None, torch.tensor([tb]), [nv], [tb + ta])
        kept = model.backbone.last_pdrop_trace[-1]["kept"].cpu()
        assert torch.equal(kept, kept_ref), f"stage {stage}"
        assert torch.equal(new.cpu(), new_ref), f"stage {stage}"


def test_transv_merge_vs_oracle():
    model, g = load_toy("pdrop_transv", dict(use_pdrop=True, pdrop_type=PD,
                                             merge_module="CrossAttention"), torch.bfloat16)
    sd = {k: v.bfloat16().float() for k, v in golden_state_dict(g).items()}
    cfg = om.OracleConfig.from_hf(model.config, pdrop_type=PD, merge_module="CrossAttention")
    tb, nv, ta = (int(v) for v in g["meta"])
    feats = torch.randn(1, tb + nv + ta, 64, generator=torch.Generator().manual_seed(1)).bfloat16()
    new_ref, kept_ref, _ = om.pdrop_stage_ref(sd, "backbone.", cfg, feats.float(), 0, 2, tb, nv, tb + ta)
    with torch.no_grad():
        _, _, new, _, _ = model.backbone.pdrop_no_pack(feats.to(DEV), 0, 2, "uni", None, None, None,
                                                       torch.tensor([tb]), [nv], [tb + ta])
    assert torch.equal(model.backbone.last_pdrop_trace[-1]["kept"].cpu(), kept_ref)
    assert torch.equal(new[0, :tb + 30].cpu().float(), new_ref[0, :tb + 30])   # gathered rows: exact
    assert relerr(new[0, tb + 30:], new_ref[0, tb + 30:]) < 2e-2               # merged text rows


def test_prefill_plus_decode_matches_full_prefill():
    """decode kernels (conv update, state update, 1-query attention) inside the model."""
    from timeviper_amd.model.llm.nano import HybridMambaAttentionDynamicCache
    model, g = load_toy("plain", {}, torch.bfloat16)
    emb = torch.from_numpy(g["embeds"]).to(DEV).bfloat16()
    L = emb.shape[1]
    with torch.no_grad():
        full = model(inputs_embeds=emb, logits_to_keep=0).logits
        cache = HybridMambaAttentionDynamicCache(model.config, 1, dtype=torch.bfloat16, device=DEV)
        model(inputs_embeds=emb[:, :L - 2], past_key_values=cache, use_cache=True,
              cache_position=torch.zeros(1, dtype=torch.long))
        outs = []
        for t in (L - 2, L - 1):
            o = model(inputs_embeds=emb[:, t:t + 1], past_key_values=cache, use_cache=True,
                      cache_position=torch.tensor([t]))
            outs.append(o.logits[:, -1])
    assert relerr(outs[0], full[:, L - 2]) < 3e-2
    assert relerr(outs[1], full[:, L - 1]) < 3e-2


def test_vit_vs_oracle():
    from timeviper_amd.model.vit.siglip import VisionTransformer
    torch.manual_seed(0)
    vit = VisionTransformer(img_size=56, patch_size=14, embed_dim=144, depth=4, num_heads=2,
                            mlp_hidden=256)          # head_dim 72 like so400m
    for p in vit.parameters():
        if p.dim() > 1:
            torch.nn.init.normal_(p, std=0.05)
    pix = torch.randn(3, 3, 56, 56)
    sd = {k: v.detach().bfloat16().float() for k, v in vit.state_dict().items()}
    ref = ov.vit_intermediate_ref(sd, pix.bfloat16().float(), depth=4, num_heads=2, patch=14)
    with torch.no_grad():
        out = vit.to(DEV).bfloat16()(pix.to(DEV).bfloat16())
    assert out.shape == (3, 16, 144)
    assert relerr(out, ref) < 2e-2


VIT_FRAME_BOUND = 2e-2


@pytest.fixture(scope="module")
def vit_many_frames():
    """The toy ViT of test_vit_vs_oracle (same seed, same weights), its 3 frames followed by 2 046 more, and the
    oracle's output — once for both forms, released with the module."""
    from timeviper_amd.model.vit.siglip import VisionTransformer
    torch.manual_seed(0)
    vit = VisionTransformer(img_size=56, patch_size=14, embed_dim=144, depth=4, num_heads=2, mlp_hidden=256)
    for p in vit.parameters():
        if p.dim() > 1:
            torch.nn.init.normal_(p, std=0.05)
    pix = torch.cat([torch.randn(3, 3, 56, 56), torch.randn(2046, 3, 56, 56)])
    sd = {k: v.detach().bfloat16().float() for k, v in vit.state_dict().items()}
    ref = ov.vit_intermediate_ref(sd, pix.bfloat16().float(), depth=4, num_heads=2, patch=14)
    yield vit.to(DEV).bfloat16(), pix.to(DEV).bfloat16(), ref.double()


@pytest.mark.parametrize("stream", ["1", "0"], ids=["stream", "fused"])
def test_vit_vs_oracle_many_rows_per_frame(monkeypatch, vit_many_frames, stream):
    """2 049 frames x 16 patches = 32 784 rows (4 098 waves of 8: the last block runs 2 of its 4 waves): in the stream
    form (TV_VIT_STREAM unset / 1) every LayerNorm runs on the many-row kernel with a row bias from the second one on;
    with TV_VIT_STREAM=0 the fused form's LayerNorms carry a residual and run on the wave kernel at the same row count.
    Judged per FRAME (a wrong row among 32 784 does not move a global relative error).  The first three frames are
    test_vit_vs_oracle's frames on the same weights.  Measured on an MI355X, worst per-frame relative error of those
    three: 4.94e-3 (stream), 4.88e-3 (TV_VIT_STREAM=0); of all 2 049: 5.38e-3 and 5.05e-3.  The bound of that test, 2e-2, is
    4.0 times the larger three-frame figure — more than the factor 2 asked of it — so it stands as the per-frame
    bound, and the test asserts that margin on what it measures."""
    monkeypatch.setenv("TV_VIT_STREAM", stream)
    vit, pix, ref = vit_many_frames
    with torch.no_grad():
        out = vit(pix)
    assert out.shape == (2049, 16, 144)
    err = (out.double().cpu() - ref).flatten(1).norm(dim=1) / ref.flatten(1).norm(dim=1)
    worst, three = int(err.argmax()), float(err[:3].max())
    print(f"vit per-frame relerr (TV_VIT_STREAM={stream}): worst {float(err[worst]):.3e} at frame {worst}, "
          f"first three frames {three:.3e}")
    assert VIT_FRAME_BOUND >= 2 * three, f"2e-2 is not twice the three-frame worst {three:.3e}"
    assert bool(torch.isfinite(err).all()) and float(err[worst]) < VIT_FRAME_BOUND, (worst, float(err[worst]))


@pytest.mark.parametrize("case,is_video", [("video", True), ("video_b2", True), ("images", False)])
def test_internvideo2_tower_vs_reference_golden(case, is_video):
    """InternVideo2 tower on the HIP operators (bf16) against the reference's own fp32
    output (tests/golden/internvideo2.npz); tolerance = bf16 round-off through 4 blocks."""
    from timeviper_amd.model.vit.internvideo2 import InternVideo2VisionConfig, InternVideo2VisionTower
    g = load_golden("internvideo2")
    cfg = InternVideo2VisionConfig(num_frames=4, hidden_size=64, num_hidden_layers=5,
                                   num_attention_heads=2, image_size=28, patch_size=14)
    tower = InternVideo2VisionTower(cfg).eval()
    tower.vision_tower.load_state_dict(golden_state_dict(g), strict=True)
    tower = tower.to(DEV).bfloat16()
    out = tower(torch.from_numpy(g[case]).to(DEV).bfloat16(), is_video=is_video)
    assert out.shape == g[case + "_out"].shape
    assert relerr(out, torch.from_numpy(g[case + "_out"])) < 3e-2


def test_internvideo2_full_width_block_runs():
    """Real InternVideo2-1B widths (1408 = 16 heads x 88, MLP 6144) for one 4-frame clip,
    2 blocks, against the oracle on the same bf16-rounded weights."""
    from timeviper_amd.model.vit.internvideo2 import InternVideo2VisionConfig, InternVideo2VisionTower
    torch.manual_seed(3)
    cfg = InternVideo2VisionConfig(num_hidden_layers=3)          # depth = 3 - 2 + 1 = 2
    tower = InternVideo2VisionTower(cfg).eval()
    with torch.no_grad():
        for n, p in tower.named_parameters():
            if n.endswith(("ls1.weight", "ls2.weight")):
                p.fill_(0.5)
            elif p.dim() > 1 and "pos_embed" not in n:
                p.normal_(0, 0.02)
    px = torch.randn(4, 1, 3, 224, 224)
    sd = {k: v.detach().bfloat16().float() for k, v in tower.vision_tower.state_dict().items()}
    ref = ov.internvideo2_tower_ref(sd, px.bfloat16().float(), 16, is_video=True)
    out = tower.to(DEV).bfloat16()(px.to(DEV).bfloat16(), is_video=True)
    assert out.shape == (1, 4 * 256, 1408)
    assert relerr(out, ref) < 2e-2


def test_vlm_end_to_end_tiny():
    """pixels -> ViT -> ToMe+MLP -> fusion -> hybrid LM with pdrop+TransV; composite oracle."""
    from timeviper_amd.model import build_synthetic_timeviper
    from timeviper_amd.model.llm.nano import NemotronHConfig
    cfg = NemotronHConfig(vocab_size=128, hidden_size=64, intermediate_size=96, num_hidden_layers=8,
                          hybrid_override_pattern="M-M*M-*M", num_attention_heads=4, head_dim=16,
                          num_key_value_heads=2, ssm_state_size=16, mamba_num_heads=8,
                          mamba_n_groups=2, mamba_head_dim=8, mamba_chunk_size=16)
    vlm = build_synthetic_timeviper(cfg, "siglip-vit-b16-224px", pdrop_type=PD,
                                    merge_module="CrossAttention", vit_depth=3, image_size=96)
    with torch.no_grad():   # separate the ranking scores (N(0,0.02) weights give near-uniform attention)
        for blk in vlm.llm_backbone.llm.backbone.layers:
            if blk.block_type == "attention":
                blk.mixer.q_proj.weight.mul_(40.0)
                blk.mixer.k_proj.weight.mul_(40.0)
    T = 5
    tok = vlm.default_token_id
    ids = torch.tensor([[5, 6, 7] + [tok] * T + [8, 9, 10, 11]], device=DEV)
    pix = torch.randn(T, 3, 96, 96, device=DEV, dtype=torch.bfloat16)
    with torch.no_grad():
        out = vlm(input_ids=ids, pixel_values_videos=pix)
        vis = vlm.encode_vision(pix, True)
    assert vis.shape == (T, 16, 64)
    assert out.logits.shape == (1, 1, 128) and torch.isfinite(out.logits).all()
    # oracle: same visual embeddings, LM stack on the CPU in fp32
    sd = {k: v.float().cpu() for k, v in vlm.llm_backbone.llm.state_dict().items()}
    ocfg = om.OracleConfig.from_hf(cfg, pdrop_type=PD, merge_module="CrossAttention")
    fused = om.fuse_embeddings_ref(ids.cpu(), vis.float().cpu(), sd["backbone.embeddings.weight"], tok)
    pa = om.pdrop_bookkeeping_ref(ids.cpu(), T, 16, tok)
    assert pa["num_vision_tokens"] == [80] and pa["text_prompt_lens"] == [7]
    col = {}
    om.causal_lm_ref(sd, ocfg, fused, pa, last_only=True, collect=col)
    trace = [t["kept"].cpu() for t in vlm.llm_backbone.llm.backbone.last_pdrop_trace]
    assert torch.equal(trace[0], col["kept"][0])          # "uni" stage: bit-exact
    # first "attn" stage: bf16 scores here, fp32 scores in the oracle -> mostly the same tokens
    # (later stages rank a different candidate set once one selection differs)
    inter = len(set(trace[1].tolist()) & set(col["kept"][1].tolist()))
    assert inter >= 0.6 * len(col["kept"][1]), (inter, len(col["kept"][1]))
    # same token selection -> logits comparable at bf16 tolerance
    ref = om.causal_lm_ref(sd, ocfg, fused, pa, last_only=True, forced_kept=trace)
    assert relerr(out.logits, ref) < 8e-2
    gen = vlm.generate(ids, pixel_values_videos=pix, max_new_tokens=4, return_ids=True)
    txt = vlm.generate(ids, pixel_values_videos=pix, max_new_tokens=4)      # reference contract: decoded text
    assert isinstance(txt, str) and txt == vlm.llm_tokenizer.decode(gen[0]).strip()
    assert gen.shape[0] == 1 and 1 <= gen.shape[1] <= 4
    assert int(gen[0, 0]) == int(out.logits[0, -1].argmax())


def test_vlm_with_internvideo2_backbone_runs_and_matches_parts():
    """InternVideo2 tower -> ToMe (4-frame clips, local_num_frames=4) -> fusion -> LM: the module
    wiring of generic_vlm.py:401-438 for the `internvideo2` identifier, checked against the same
    parts run one by one."""
    from timeviper_amd.model import build_synthetic_timeviper
    from timeviper_amd.model.llm.nano import NemotronHConfig
    from timeviper_amd.model.vit.internvideo2 import InternVideo2VisionConfig
    cfg = NemotronHConfig(vocab_size=128, hidden_size=64, intermediate_size=96, num_hidden_layers=4,
                          hybrid_override_pattern="M-*-", num_attention_heads=4, head_dim=16,
                          num_key_value_heads=2, ssm_state_size=16, mamba_num_heads=8,
                          mamba_n_groups=2, mamba_head_dim=8, mamba_chunk_size=16)
    vcfg = InternVideo2VisionConfig(num_frames=4, hidden_size=128, num_hidden_layers=4,
                                    num_attention_heads=4, image_size=112, patch_size=14)
    vlm = build_synthetic_timeviper(cfg, "internvideo2-1b-16-224px", image_size=112, vision_config=vcfg)
    T = 8
    tok = vlm.default_token_id
    ids = torch.tensor([[5, 6] + [tok] * T + [8, 9, 10]], device=DEV)
    pix = torch.randn(T, 1, 3, 112, 112, device=DEV).bfloat16()          # (T, B, C, H, W)
    with torch.no_grad():
        out = vlm(input_ids=ids, pixel_values_videos=pix).logits
        feats = vlm.vision_backbone(pix, is_video=True)                   # (2 clips, 4*64 patches, 128)
        assert feats.shape == (2, 4 * 64, 128)
        vis = vlm.projector_forward(feats, is_video=True)                 # (8 frames, 16 tokens, 64)
        assert vis.shape == (T, 16, 64)
        fused, _ = vlm.get_fused_data_nopacked(vis, ids)
        ref = vlm.llm_backbone(inputs_embeds=fused).logits
    assert out.shape[-1] == 128 and torch.isfinite(out.float()).all()
    assert relerr(out[:, -1], ref[:, -1]) < 3e-2


def test_vlm_with_qwen2_backbone_vs_oracle_and_generate():
    """BASELINE config 5's LM family behind the same VLM wiring: pixels -> ViT -> ToMe+MLP -> fusion ->
    Qwen2 with uniform pdrop + TransV (llm_registry.py:65-77 ids), against the pinned Qwen2 oracle on
    the same visual embeddings; greedy `generate` must continue from the prefill's argmax."""
    from oracle import qwen2 as oq
    from timeviper_amd.model import build_synthetic_timeviper
    from timeviper_amd.model.llm.qwen2 import Qwen2Config
    pd = "uni_1_0.75-uni_3_0.5"
    cfg = Qwen2Config(vocab_size=128, hidden_size=128, intermediate_size=256, num_hidden_layers=5,
                      num_attention_heads=2, num_key_value_heads=1, rope_theta=10000.0)
    vlm = build_synthetic_timeviper(cfg, "siglip-vit-b16-224px", pdrop_type=pd, merge_module="CrossAttention",
                                    vit_depth=3, image_size=96, llm_backbone_id="qwen2.5-7b-instruct")
    assert vlm.model_family == "qwen2" and vlm.use_pdrop
    T = 5
    tok = vlm.default_token_id
    ids = torch.tensor([[5, 6, 7] + [tok] * T + [8, 9, 10, 11]], device=DEV)
    pix = torch.randn(T, 3, 96, 96, device=DEV, dtype=torch.bfloat16)
    with torch.no_grad():
        out = vlm(input_ids=ids, pixel_values_videos=pix)
        vis = vlm.encode_vision(pix, True)
    assert out.logits.shape == (1, 1, 128) and torch.isfinite(out.logits).all()
    sd = {k: v.float().cpu() for k, v in vlm.llm_backbone.llm.state_dict().items()}
    fused = om.fuse_embeddings_ref(ids.cpu(), vis.float().cpu(), sd["model.embed_tokens.weight"], tok)
    pa = om.pdrop_bookkeeping_ref(ids.cpu(), T, 16, tok)
    ocfg = dict(num_hidden_layers=5, num_attention_heads=2, num_key_value_heads=1, head_dim=64,
                rope_theta=10000.0, rms_norm_eps=cfg.rms_norm_eps, pdrop_type=pd, merge_module="CrossAttention")
    ref = oq.causal_lm_ref(sd, ocfg, inputs_embeds=fused, pdrop_args=pa)
    assert relerr(out.logits[:, -1], ref[:, -1]) < 3e-2
    gen = vlm.generate(ids, pixel_values_videos=pix, max_new_tokens=4, return_ids=True)
    txt = vlm.generate(ids, pixel_values_videos=pix, max_new_tokens=4)      # reference contract: decoded text
    assert isinstance(txt, str) and txt == vlm.llm_tokenizer.decode(gen[0]).strip()
    assert gen.shape[0] == 1 and 1 <= gen.shape[1] <= 4
    assert int(gen[0, 0]) == int(out.logits[0, -1].argmax())


def test_vlm_dual_encoder_qwen2_matches_parts():
    """BASELINE config 4's wiring at toy size: DINOv2-L (frame-wise) + InternVideo2 (4-frame tubes)
    -> MultiToMe (16 + 16 tokens per frame, interleaved token-wise) -> fusion -> Qwen2 with pdrop +
    TransV.  The end-to-end forward must equal the same members run one by one, the interleave must
    be the reference's rule (projector/tome.py:214-231) and the LM stage must match the oracle."""
    from oracle import qwen2 as oq
    from timeviper_amd.model import build_synthetic_timeviper
    from timeviper_amd.model.llm.qwen2 import Qwen2Config
    from timeviper_amd.model.vit.internvideo2 import InternVideo2VisionConfig
    pd = "uni_1_0.75-uni_3_0.5"
    cfg = Qwen2Config(vocab_size=128, hidden_size=128, intermediate_size=256, num_hidden_layers=5,
                      num_attention_heads=2, num_key_value_heads=1, rope_theta=10000.0)
    vcfg = InternVideo2VisionConfig(num_frames=4, hidden_size=128, num_hidden_layers=4,
                                    num_attention_heads=4, image_size=112, patch_size=14)
    bid = "dinov2-vit-l+internvideo2-1b-16-224px"
    vlm = build_synthetic_timeviper(cfg, bid, pdrop_type=pd, merge_module="CrossAttention", image_size=112,
                                    llm_backbone_id="qwen2.5-7b-instruct", member_kwargs={
                                        "dinov2-vit-l": dict(depth_override=3, default_image_size=112),
                                        "internvideo2-1b-16-224px": dict(default_image_size=112, vision_config=vcfg)})
    T = 8
    tok = vlm.default_token_id
    ids = torch.tensor([[5, 6] + [tok] * T + [8, 9, 10]], device=DEV)
    pix = torch.randn(T, 3, 112, 112, device=DEV).bfloat16()
    with torch.no_grad():
        out = vlm(input_ids=ids, pixel_values_videos=pix).logits
        feats = vlm.vision_backbone(pix, is_video=True)
        assert feats["dinov2-vit-l"].shape == (T, 64, 1024)
        assert feats["internvideo2-1b-16-224px"].shape == (T // 4, 4 * 64, 128)
        vis = vlm.projector_forward(feats, is_video=True)
        assert vis.shape == (T, 32, 128)
        pj = vlm.projector.projectors
        a = pj["dinov2-vit-l"](feats["dinov2-vit-l"], compress=True, local_num_frames=1)
        b = pj["internvideo2-1b-16-224px"](feats["internvideo2-1b-16-224px"], compress=True, local_num_frames=4)
        assert torch.equal(vis[:, 0::2], a) and torch.equal(vis[:, 1::2], b.reshape(T, 16, 128))
    sd = {k: v.float().cpu() for k, v in vlm.llm_backbone.llm.state_dict().items()}
    fused = om.fuse_embeddings_ref(ids.cpu(), vis.float().cpu(), sd["model.embed_tokens.weight"], tok)
    pa = om.pdrop_bookkeeping_ref(ids.cpu(), T, 32, tok)
    ocfg = dict(num_hidden_layers=5, num_attention_heads=2, num_key_value_heads=1, head_dim=64,
                rope_theta=10000.0, rms_norm_eps=cfg.rms_norm_eps, pdrop_type=pd, merge_module="CrossAttention")
    ref = oq.causal_lm_ref(sd, ocfg, inputs_embeds=fused, pdrop_args=pa)
    assert relerr(out[:, -1], ref[:, -1]) < 3e-2


@pytest.mark.parametrize("tag,extra", [("wc_plain", {}), ("wc_pdrop_nomerge", dict(use_pdrop=True)),
                                       ("wc_pdrop_transv", dict(use_pdrop=True, merge_module="CrossAttention"))])
def test_qwen2_bf16_vs_reference_golden(tag, extra):
    """Qwen2 mirror on the HIP operators (bf16) against the REFERENCE's fp32 logits (`oracle/make_golden.py`, fixtures
    `qwen2_wc_*`: the reference's Qwen2ForCausalLM with well-conditioned projections and bf16-representable parameters, so
    the two runs differ by the rounding of bf16 activations only).  Bound 3e-2 of the logits' norm, as for the Nano toys.
    (The sharp `qwen2_{plain,pdrop_*}` fixtures amplify ANY bf16 run to ~ 14 %: they pin the fp32 oracle and the fp32
    mirror on the CPU — tests/test_oracle_golden.py, tests/test_model_cpu.py — and are not compared in bf16.)"""
    from timeviper_amd.model.llm.qwen2 import Qwen2Config, Qwen2ForCausalLM
    g = load_golden(f"qwen2_{tag}")
    cfg = Qwen2Config(vocab_size=64, hidden_size=64, intermediate_size=96, num_hidden_layers=6,
                      num_attention_heads=4, num_key_value_heads=2, rope_theta=10000.0,
                      pdrop_type="uni_1_0.75-uni_3_0.5-uni_4_0.25" if extra else None, **extra)
    model = Qwen2ForCausalLM(cfg).eval()
    model.load_state_dict(golden_state_dict(g), strict=True)
    model = model.to(DEV).bfloat16()
    args = {"train_pdrop_args": {"first_vision_token_positions": [3], "num_vision_tokens": [24],
                                 "text_prompt_lens": [19]}} if extra else {}
    with torch.no_grad():
        out = model(input_ids=torch.from_numpy(g["ids"]).long().to(DEV), use_cache=False, **args)
    assert out.logits.shape == g["logits"].shape
    e = relerr(out.logits, torch.from_numpy(g["logits"]))
    assert e < 3e-2, e


@pytest.mark.parametrize("merge", ["no_merge", "CrossAttention"])
def test_qwen2_bf16_vs_oracle_well_conditioned(merge):
    """Qwen2 mirror (bf16, HIP operators) against the pinned fp32 oracle on the same bf16-rounded
    weights: N(0, 0.05) weights, head_dim 64, uniform pdrop stages + TransV."""
    from oracle import qwen2 as oq
    from timeviper_amd.model.llm.qwen2 import Qwen2Config, Qwen2ForCausalLM
    pd = "uni_1_0.75-uni_3_0.5"
    torch.manual_seed(11)
    cfg = Qwen2Config(vocab_size=96, hidden_size=256, intermediate_size=512, num_hidden_layers=5,
                      num_attention_heads=4, num_key_value_heads=2, rope_theta=10000.0, use_pdrop=True,
                      pdrop_type=pd, merge_module=merge)
    model = Qwen2ForCausalLM(cfg).eval()
    with torch.no_grad():
        for n, p in model.named_parameters():
            if n.endswith("alpha"):
                p.fill_(0.5)
            elif p.dim() > 1:
                p.normal_(0, 0.05)
            elif n.endswith("bias"):
                p.normal_(0, 0.02)
    sd = {k: v.detach().bfloat16().float() for k, v in model.state_dict().items()}
    ids = torch.randint(0, 96, (1, 90))
    args = {"first_vision_token_positions": [4], "num_vision_tokens": [64], "text_prompt_lens": [26]}
    ocfg = dict(num_hidden_layers=5, num_attention_heads=4, num_key_value_heads=2, head_dim=64,
                rope_theta=10000.0, rms_norm_eps=1e-6, pdrop_type=pd, merge_module=merge)
    ref = oq.causal_lm_ref(sd, ocfg, input_ids=ids, pdrop_args=args)
    with torch.no_grad():
        out = model.to(DEV).bfloat16()(input_ids=ids.to(DEV), use_cache=False, train_pdrop_args=args)
    assert out.logits.shape == ref.shape
    e16 = relerr(out.logits, ref)
    assert e16 < 3e-2
    # The same forward with EVERY attention call on the e4m3 MFMA path (BASELINE config 5's switch, forced down to these
    # short sequences): pinned against the same fp32 oracle.  e4m3 carries 3 mantissa bits on q, k, v and P, so the bound
    # is wider than bf16's — stated here: logits within 8e-2 relative L2 (2.7 x the bf16 bound), the arg-max token of
    # every position whose oracle margin exceeds the fp8 error the same as the oracle's.
    from timeviper_amd import kernels as K
    with torch.no_grad(), K.fp8_attention(min_keys=1, min_queries=1):
        out8 = model(input_ids=ids.to(DEV), use_cache=False, train_pdrop_args=args)
    e8 = relerr(out8.logits, ref)
    assert e8 < 8e-2, (e8, e16)
    l8, lr = out8.logits.float().cpu()[0], ref.float()[0]
    top2 = lr.topk(2, dim=-1).values
    clear = (top2[:, 0] - top2[:, 1]) > 2 * (l8 - lr).abs().max(dim=-1).values
    assert (l8.argmax(-1)[clear] == lr.argmax(-1)[clear]).all()
    # (96 random-init logits lie close together: ~15 % of the positions have such a margin; the test needs some)
    assert int(clear.sum()) >= 5, int(clear.sum())


def test_qwen2_prefill_plus_decode_matches_full_prefill():
    from timeviper_amd.model.llm.qwen2 import Qwen2Config, Qwen2ForCausalLM
    torch.manual_seed(5)
    cfg = Qwen2Config(vocab_size=128, hidden_size=256, intermediate_size=384, num_hidden_layers=4,
                      num_attention_heads=4, num_key_value_heads=2, rope_theta=10000.0)
    model = Qwen2ForCausalLM(cfg).to(DEV).bfloat16().eval()
    ids = torch.randint(0, 128, (1, 70), device=DEV)
    with torch.no_grad():
        full = model(input_ids=ids, use_cache=False).logits
        cache = model.new_cache()
        model(input_ids=ids[:, :68], past_key_values=cache, use_cache=True)
        o1 = model(input_ids=ids[:, 68:69], past_key_values=cache, use_cache=True).logits
        o2 = model(input_ids=ids[:, 69:70], past_key_values=cache, use_cache=True).logits
    assert relerr(o1[:, -1], full[:, 68]) < 3e-2 and relerr(o2[:, -1], full[:, 69]) < 3e-2


def test_vit_mlp_fused_fc1_gelu_matches_the_two_pass_path(monkeypatch):
    """From 4 096 rows on the SigLIP / InternVideo2 MLPs run fc1 + bias + exact GELU as ONE kernel (tv_gemm_bf16_fwd,
    epilogue 1): same result as hipBLASLt + tv_gelu_fwd up to the accumulation order of the GEMM, and as the plain
    nn.Linear / nn.GELU modules (grad mode)."""
    from timeviper_amd.model.vit.siglip import Mlp
    from timeviper_amd.model.vit.internvideo2 import Mlp as IvMlp
    from timeviper_amd import kernels as K
    torch.manual_seed(3)
    for mlp, dim in ((Mlp(1152, 4304), 1152), (IvMlp(1408, 6144), 1408)):
        mlp = mlp.to(DEV).bfloat16().eval()
        with torch.no_grad():
            for p_ in mlp.parameters():
                p_.normal_(0, 0.03 if p_.dim() > 1 else 0.05)
        x = torch.randn(8, 729, dim, device=DEV).bfloat16()
        calls = []
        orig = K.linear_fused
        monkeypatch.setattr(K, "linear_fused", lambda *a, **kw: (calls.append(kw.get("epilogue")), orig(*a, **kw))[1])
        with torch.no_grad():
            fused = mlp(x)
        assert calls == [K.GEMM_BIAS_GELU], calls
        monkeypatch.setenv("TV_VIT_FUSED_FC1", "0")
        with torch.no_grad():
            two_pass = mlp(x)
        assert calls == [K.GEMM_BIAS_GELU]
        monkeypatch.delenv("TV_VIT_FUSED_FC1")
        monkeypatch.setattr(K, "linear_fused", orig)
        with torch.enable_grad():
            plain = mlp.fc2(torch.nn.functional.gelu(mlp.fc1(x))).detach()
        assert relerr(fused, two_pass) < 4e-3 and relerr(fused, plain) < 4e-3


def test_vit_zero_padded_gemms_match_plain_linears():
    """so400m widths (qkv N = 3456, MLP hidden 4304 — not multiples of the 256-wide GEMM tile): the
    inference path runs zero-padded weight copies; it must equal the plain nn.Linear path, follow
    in-place weight updates, and leave the checkpoint shapes alone."""
    from timeviper_amd.model.vit.siglip import Block
    torch.manual_seed(2)
    blk = Block(1152, 16, 4304).to(DEV).bfloat16().eval()
    with torch.no_grad():
        for p in blk.parameters():
            if p.dim() > 1:
                p.normal_(0, 0.03)
        for lin in (blk.attn.qkv, blk.attn.proj, blk.mlp.fc1, blk.mlp.fc2):
            lin.bias.normal_(0, 0.05)
    x = torch.randn(4, 729, 1152, device=DEV).bfloat16()
    with torch.enable_grad():                     # grad mode keeps the plain Linear path
        ref = blk(x).detach()
    with torch.no_grad():
        out = blk(x)
        assert blk.mlp._padded._val[0].shape == (4352, 1152) and blk.attn._padded._val[0].shape == (3584, 1152)
        assert relerr(out, ref) < 4e-3
        blk.mlp.fc1.weight.mul_(0.5)              # in-place update must invalidate the padded copy
        blk.attn.qkv.bias.add_(0.01)
        out2 = blk(x)
    with torch.enable_grad():
        ref2 = blk(x).detach()
    assert relerr(out2, ref2) < 4e-3 and relerr(out2, ref) > 1e-2
    assert blk.mlp.fc1.weight.shape == (4304, 1152) and set(blk.state_dict()) == {
        "norm1.weight", "norm1.bias", "attn.qkv.weight", "attn.qkv.bias", "attn.proj.weight", "attn.proj.bias",
        "norm2.weight", "norm2.bias", "mlp.fc1.weight", "mlp.fc1.bias", "mlp.fc2.weight", "mlp.fc2.bias"}


def test_internvideo2_fused_clips_equal_separate_clips():
    """`encode_vision` hands InternVideo2 (alone or inside a dual encoder) several 256-frame clips at
    once; the tower regroups each clip with the reference's clip-length-dependent reshape
    (model.py:178-182) and batches the tubes — the result must equal separate 256-frame calls, incl.
    a ragged last clip."""
    from timeviper_amd.model import build_synthetic_timeviper
    from timeviper_amd.model.llm.nano import NemotronHConfig
    from timeviper_amd.model.vit.internvideo2 import InternVideo2VisionConfig
    cfg = NemotronHConfig(vocab_size=128, hidden_size=64, intermediate_size=96, num_hidden_layers=2,
                          hybrid_override_pattern="M-", num_attention_heads=4, head_dim=16,
                          num_key_value_heads=2, ssm_state_size=16, mamba_num_heads=8,
                          mamba_n_groups=2, mamba_head_dim=8, mamba_chunk_size=16)
    vcfg = InternVideo2VisionConfig(num_frames=4, hidden_size=64, num_hidden_layers=3,
                                    num_attention_heads=2, image_size=112, patch_size=14)
    T = 2 * 256 + 8
    torch.manual_seed(4)
    pix4 = torch.randn(T, 3, 112, 112, device=DEV).bfloat16()
    for bid, kw in (("internvideo2-1b-16-224px", dict(vision_config=vcfg, image_size=112)),
                    ("dinov2-vit-l+internvideo2-1b-16-224px", dict(image_size=112, member_kwargs={
                        "dinov2-vit-l": dict(depth_override=2, default_image_size=112),
                        "internvideo2-1b-16-224px": dict(default_image_size=112, vision_config=vcfg)}))):
        vlm = build_synthetic_timeviper(cfg, bid, **kw)
        pix = pix4 if "+" in bid else pix4.unsqueeze(1)
        vb = vlm.vision_backbone
        with torch.no_grad():
            assert vlm.encode_vision(pix, True).shape == (T, 16 * (2 if "+" in bid else 1), 64)
            fused = vb(pix, is_video=True, clip_frames=256)                     # what encode_vision calls
            sep = [vb(c, is_video=True) for c in pix.split(256)]                # the reference's clips
            for key in (fused if isinstance(fused, dict) else {None: 0}):
                f = fused[key] if key is not None else fused
                r = torch.cat([c[key] if key is not None else c for c in sep])
                assert f.shape == r.shape and relerr(f, r) < 5e-3, (bid, key)
            # ToMe + MLP see tubes / frames one by one: same features -> same tokens for any batching
            # (features that differ by GEMM rounding may flip a near-tie in the discrete matching,
            # which is why the projector is compared on identical inputs)
            pf = vlm.projector_forward(fused, is_video=True)
            first = {k: v[: (64 if "internvideo2" in k else 256)] for k, v in fused.items()} \
                if isinstance(fused, dict) else fused[:64]
            assert relerr(pf[:256], vlm.projector_forward(first, is_video=True)) < 5e-3, bid


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
    return cfg, model


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


def test_realshape_prefill_bf16_vs_reference_golden():
    """Model-level parity at Nano-9B's real head shapes against numbers the REFERENCE produced (tests/golden/
    toy_realshape_g2.npz; the toy goldens above stop at the generic scan kernel and the small attention instance): the
    bf16 prefill runs ssd_head_kernel<5,4,2> (asserted) and the d-128 causal attention.  group_map "tile" = the
    reference CPU prefill's h % G (modeling_nano.py:781-782)."""
    from timeviper_amd import kernels as K
    cfg, model, g, L, _ = _realshape_model("g2", "tile")
    emb = torch.from_numpy(g["embeds"]).to(DEV).bfloat16()
    with torch.no_grad():
        out = model(inputs_embeds=emb, logits_to_keep=0).logits
    assert K.ssd_scan_last_impl() == 6, "the prefill did not run on the head-per-wave march"
    assert out.shape == (1, L, 96)
    assert relerr(out, g["logits"]) < 3e-2, relerr(out, g["logits"])


def test_realshape_prefill_plus_graphed_fused_decode_vs_reference_golden(monkeypatch):
    """... and the decode kernels at those shapes: a bf16 prefill of 300 tokens + four decode tokens through the fused
    decode step (TV_DECODE_FUSED=1: tv_gemv_bf16_fwd prologues, tv_selective_state_update at P 80 / N 128,
    tv_attn_decode_fwd at d 128) under GraphedDecodeStep reproduce positions 300 .. 303 of the reference's 304-token
    forward (tests/golden/toy_realshape_g1.npz; one B/C group, where the reference's prefill and decode group maps agree)."""
    from timeviper_amd import kernels as K
    from timeviper_amd.model.llm.decode_graph import GraphedDecodeStep
    from timeviper_amd.model.llm.nano import HybridMambaAttentionDynamicCache
    monkeypatch.setenv("TV_DECODE_FUSED", "1")
    cfg, model, g, L, ndec = _realshape_model("g1", "block")
    emb = torch.from_numpy(g["embeds"]).to(DEV).bfloat16()
    ref = torch.from_numpy(g["logits"])
    host_pos = torch.ones(1, dtype=torch.long)
    with torch.inference_mode():
        cache = HybridMambaAttentionDynamicCache(cfg, 1, dtype=torch.bfloat16, device=DEV)
        pre = model(inputs_embeds=emb[:, :L], past_key_values=cache, use_cache=True,
                    cache_position=torch.zeros(1, dtype=torch.long), logits_to_keep=0).logits
        assert K.ssd_scan_last_impl() == 6
        assert relerr(pre, ref[:, :L]) < 3e-2, relerr(pre, ref[:, :L])
        cache.begin_static_decode(ndec)
        cur = {}
        stepper = GraphedDecodeStep(
            lambda ids: model(inputs_embeds=cur["e"], past_key_values=cache, use_cache=True, cache_position=host_pos).logits,
            cache, 1, DEV)
        buf = torch.empty(1, 1, cfg.hidden_size, dtype=torch.bfloat16, device=DEV)     # static input of the captured step
        cur["e"] = buf
        for i in range(ndec):
            buf.copy_(emb[:, L + i:L + i + 1])
            stepper.step(torch.zeros(1, 1, dtype=torch.long, device=DEV))
            err = relerr(stepper.logits, ref[:, L + i])
            assert err < 3e-2, (i, err)
        assert stepper.graph is not None


def test_true_width_slice_vs_oracle():
    """The language model at Nano-9B's TRUE width (hidden 4 480, 128 Mamba heads of 80 in 8 groups, d_state 128, MLP 15 680,
    40 / 8 attention heads of 128): the first 16 layers of its pattern (8 Mamba, 7 MLP, the first attention layer) on 1 200
    tokens with a "uni" pdrop stage in front of layer 7 and an "attn" stage ranked by the attention layer (14), against the
    fp32 CPU oracle (oracle.model.causal_lm_ref) on the same random weights.  The bf16 run's kept indices are handed to the
    oracle for the "attn" stage (bf16 against fp32 scores: ties resolve differently; the exact ranking is checked in fp32 by
    test_pdrop_stage_indices_exact_vs_oracle_fp32); the "uni" stage must agree bit for bit.  Tolerance: relative L2 of the
    last-position logits < 5e-2 (bf16 activations through 16 residual layers)."""
    from timeviper_amd import kernels as K
    from timeviper_amd.model.llm.nano import NemotronHConfig, NemotronHForCausalLM
    pd = "uni_7_0.75-attn_14_0.5"
    full = NemotronHConfig.nemotron_nano_9b_v2()
    cfg = NemotronHConfig.nemotron_nano_9b_v2(vocab_size=2048, num_hidden_layers=16,
                                              hybrid_override_pattern=full.hybrid_override_pattern[:16],
                                              use_pdrop=True, pdrop_type=pd)
    assert cfg.hybrid_override_pattern.count("*") == 1 and cfg.hybrid_override_pattern[14] == "*"
    torch.manual_seed(16)
    model = NemotronHForCausalLM(cfg).eval()
    with torch.no_grad():          # separate the ranking scores (N(0, 0.02) weights give near-uniform attention)
        mix = model.backbone.layers[14].mixer
        mix.q_proj.weight.mul_(8.0)
        mix.k_proj.weight.mul_(8.0)
    sd = {k: v.detach().float() for k, v in model.state_dict().items()}
    model = model.to(DEV).bfloat16()
    tb, nv, ta = 20, 1100, 80
    L = tb + nv + ta
    g = torch.Generator().manual_seed(5)
    emb = (torch.randn(1, L, cfg.hidden_size, generator=g) * 0.5).bfloat16()
    pa = {"first_vision_token_positions": torch.tensor([tb]), "text_prompt_lens": [tb + ta], "num_vision_tokens": [nv],
          "is_interleaved": False}
    with torch.no_grad():
        out = model(inputs_embeds=emb.to(DEV), train_pdrop_args=pa).logits
    assert K.ssd_scan_last_impl() == 6, "the prefill did not run on the head-per-wave march"
    assert out.shape == (1, 1, 2048) and torch.isfinite(out).all()
    tr = [t["kept"].cpu() for t in model.backbone.last_pdrop_trace]
    assert [len(t) for t in tr] == [int(nv * 0.75), int(nv * 0.5)]
    assert torch.equal(tr[0], R.uniform_keep_indices_ref(nv, int(nv * 0.75)) + tb)          # "uni": exact integers
    ocfg = om.OracleConfig.from_hf(cfg, pdrop_type=pd, merge_module="no_merge")
    col = {}
    ref = om.causal_lm_ref(sd, ocfg, emb.float(), pa, last_only=True, forced_kept=tr, collect=col)
    e = relerr(out, ref)
    assert e < 5e-2, e
    # the oracle's own "attn" selection (fp32 scores) against the bf16 run's: mostly the same tokens
    own = {}
    om.causal_lm_ref(sd, ocfg, emb.float(), pa, last_only=True, collect=own)
    inter = len(set(tr[1].tolist()) & set(own["kept"][1].tolist()))
    assert inter >= 0.85 * len(tr[1]), (inter, len(tr[1]))


def test_kv_cache_grows_in_place_and_matches_concatenation():
    """`update` writes a token into spare capacity instead of re-concatenating the cache (modeling_nano.py:246-251):
    the views it hands out hold exactly what torch.cat would."""
    from timeviper_amd.model.llm.nano import HybridMambaAttentionDynamicCache
    cfg, _ = _toy_hybrid_d128("*")
    cache = HybridMambaAttentionDynamicCache(cfg, 2, dtype=torch.bfloat16, device=DEV, kv_reserve=4)
    g = torch.Generator(device=DEV).manual_seed(0)
    ks = [torch.randn(2, n, 2, 128, device=DEV, generator=g).bfloat16() for n in (300, 1, 1, 1, 1, 1, 7, 1)]
    vs = [torch.randn_like(k) for k in ks]
    for i, (k, v) in enumerate(zip(ks, vs)):
        kc, vc = cache.update(k, v, 0)
        assert torch.equal(kc, torch.cat(ks[:i + 1], 1)) and torch.equal(vc, torch.cat(vs[:i + 1], 1))
        assert cache.get_seq_length() == kc.shape[1] and cache.key_cache[0].data_ptr() == kc.data_ptr()
    ptrs = set()
    for _ in range(40):          # geometric growth: few re-allocations for many tokens
        cache.update(ks[1], vs[1], 0)
        ptrs.add(cache.kv_buffers(0)[0].data_ptr())
    assert len(ptrs) <= 3


@pytest.mark.parametrize("pattern", ["M-*M*-", "*M-"])
def test_graphed_decode_step_matches_the_eager_loop(pattern):
    """GraphedDecodeStep (static K / V buffers, device-side key count, one hipGraph launch per token) against the eager
    decode loop, teacher-forced with the same tokens: the logits of every step agree to bf16 round-off (the graph path
    runs tv_attn_decode_fwd, the eager one the prefill kernel with one query row)."""
    from timeviper_amd.model.llm.decode_graph import GraphedDecodeStep
    from timeviper_amd.model.llm.nano import HybridMambaAttentionDynamicCache
    cfg, model = _toy_hybrid_d128(pattern)
    g = torch.Generator(device=DEV).manual_seed(3)
    prompt = torch.randint(0, 256, (1, 300), device=DEV, generator=g)
    forced = torch.randint(0, 256, (10,), device=DEV, generator=g)
    host_pos = torch.ones(1, dtype=torch.long)
    with torch.inference_mode():
        eager_cache = HybridMambaAttentionDynamicCache(cfg, 1, dtype=torch.bfloat16, device=DEV)
        model(input_ids=prompt, past_key_values=eager_cache, use_cache=True, cache_position=torch.zeros(1, dtype=torch.long))
        eager = [model(input_ids=t.view(1, 1), past_key_values=eager_cache, use_cache=True,
                       cache_position=host_pos).logits[:, -1].clone() for t in forced]
        cache = HybridMambaAttentionDynamicCache(cfg, 1, dtype=torch.bfloat16, device=DEV)
        model(input_ids=prompt, past_key_values=cache, use_cache=True, cache_position=torch.zeros(1, dtype=torch.long))
        cache.begin_static_decode(len(forced))
        stepper = GraphedDecodeStep(
            lambda ids: model(input_ids=ids, past_key_values=cache, use_cache=True, cache_position=host_pos).logits,
            cache, 1, DEV)
        for i, t in enumerate(forced):
            nxt = stepper.step(t.view(1, 1))
            assert relerr(stepper.logits, eager[i]) < 3e-2, (i, relerr(stepper.logits, eager[i]))
            assert int(nxt) == int(stepper.logits.argmax(-1))
            assert cache.get_seq_length() == 300 + i + 1
        assert stepper.graph is not None          # steps 3.. were replays
        with pytest.raises(RuntimeError):         # the reservation is spent: the buffers must not move under the graph
            for _ in range(400):
                stepper.step(forced[0].view(1, 1))
        # ... and the cache it leaves is an ordinary one
        assert torch.equal(cache.key_cache[cache.attention_layers[0]][:, :310],
                           cache.kv_buffers(cache.attention_layers[0])[0][:, :310])


def raise_once_under_capture(fn):
    """`fn` as a step function whose first call under a stream capture fails: it runs the model — the host bookkeeping of
    the step has advanced, the launches were recorded, none executed — and then raises an ordinary Python exception inside
    the capture context.  No HIP call fails."""
    raised = []

    def step_fn(ids):
        out = fn(ids)
        if not raised and torch.cuda.is_current_stream_capturing():
            raised.append(True)
            raise RuntimeError("step function failed under capture (on purpose)")
        return out
    return step_fn, raised


def test_graphed_decode_step_falls_back_to_the_eager_step_when_the_capture_fails():
    """The capture of GraphedDecodeStep raises behind the model's forward: the step warns, puts the cache's host
    bookkeeping back (the capture advanced every attention layer's length and ran no kernel) and runs eagerly, as does
    every later one.  Teacher-forced against the eager loop, 8 tokens behind a 300-token prefill: the cache length after
    every step, and the logits of every step at the bound of test_graphed_decode_step_matches_the_eager_loop."""
    from timeviper_amd.model.llm.decode_graph import GraphedDecodeStep
    from timeviper_amd.model.llm.nano import HybridMambaAttentionDynamicCache
    cfg, model = _toy_hybrid_d128("M-*M*-")
    g = torch.Generator(device=DEV).manual_seed(3)
    prompt = torch.randint(0, 256, (1, 300), device=DEV, generator=g)
    forced = torch.randint(0, 256, (8,), device=DEV, generator=g)
    host_pos = torch.ones(1, dtype=torch.long)
    with torch.inference_mode():
        eager_cache = HybridMambaAttentionDynamicCache(cfg, 1, dtype=torch.bfloat16, device=DEV)
        model(input_ids=prompt, past_key_values=eager_cache, use_cache=True, cache_position=torch.zeros(1, dtype=torch.long))
        eager = [model(input_ids=t.view(1, 1), past_key_values=eager_cache, use_cache=True,
                       cache_position=host_pos).logits[:, -1].clone() for t in forced]
        cache = HybridMambaAttentionDynamicCache(cfg, 1, dtype=torch.bfloat16, device=DEV)
        model(input_ids=prompt, past_key_values=cache, use_cache=True, cache_position=torch.zeros(1, dtype=torch.long))
        cache.begin_static_decode(len(forced))
        room = cache.static_room()
        step_fn, raised = raise_once_under_capture(
            lambda ids: model(input_ids=ids, past_key_values=cache, use_cache=True, cache_position=host_pos).logits)
        stepper = GraphedDecodeStep(step_fn, cache, 1, DEV)
        for i, t in enumerate(forced):
            if i == stepper.warmup:              # the step that captures
                with pytest.warns(RuntimeWarning, match="graph capture failed"):
                    nxt = stepper.step(t.view(1, 1))
                assert raised and isinstance(stepper.capture_error, RuntimeError)
            else:
                nxt = stepper.step(t.view(1, 1))
            err = relerr(stepper.logits, eager[i])
            print(f"step {i}: relerr {err:.3e}, cache length {cache.get_seq_length()}")
            assert cache.get_seq_length() == 300 + i + 1, i
            assert err < 3e-2, (i, err)
            assert int(nxt) == int(stepper.logits.argmax(-1))
        assert stepper.capture_error is not None and stepper.graph is None and stepper.calls == len(forced)
        assert [cache._kv_len[i] for i in cache.attention_layers] == [308, 308] and cache.static_room() == room - 8


def test_fused_decode_step_matches_the_unfused_one(monkeypatch):
    """TV_DECODE_FUSED (default): the decode token's norms / activations run in the prologues of tv_gemv_bf16_fwd; =0:
    stand-alone kernels + torch.nn.Linear.  Same rounding points, so the logits agree to the products' accumulation
    order, token after token, and the caches end up equal to round-off."""
    from timeviper_amd import kernels as K
    from timeviper_amd.model.llm.nano import HybridMambaAttentionDynamicCache
    cfg, model = _toy_hybrid_d128("M-*M-*")
    g = torch.Generator(device=DEV).manual_seed(9)
    prompt = torch.randint(0, 256, (2, 270), device=DEV, generator=g)
    forced = torch.randint(0, 256, (6, 2), device=DEV, generator=g)
    host_pos = torch.ones(1, dtype=torch.long)
    runs = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("TV_DECODE_FUSED", mode)
        calls = []
        orig = K.gemv_fused
        monkeypatch.setattr(K, "gemv_fused", lambda *a, **kw: (calls.append(kw.get("prologue", a[3] if len(a) > 3 else 0)), orig(*a, **kw))[1])
        with torch.inference_mode():
            cache = HybridMambaAttentionDynamicCache(cfg, 2, dtype=torch.bfloat16, device=DEV)
            model(input_ids=prompt, past_key_values=cache, use_cache=True, cache_position=torch.zeros(1, dtype=torch.long))
            outs = [model(input_ids=t.view(2, 1), past_key_values=cache, use_cache=True, cache_position=host_pos).logits[:, -1].clone()
                    for t in forced]
        monkeypatch.setattr(K, "gemv_fused", orig)
        runs[mode] = (outs, cache, calls)
    assert runs["0"][2] == []
    assert runs["1"][2][0] == K.GEMV_NONE                  # the prefill's lm_head on its last position is one row too
    per_token = runs["1"][2][1:][:(len(runs["1"][2]) - 1) // 6]
    # M: rmsnorm-in_proj (conv update in its epilogue) + gated-out_proj; -: rmsnorm-up + relu2-down; *: rmsnorm-[q; k; v] + o;
    # the head
    blocks = [K.GEMV_RMSNORM, K.GEMV_GATED, K.GEMV_RMSNORM, K.GEMV_RELU2, K.GEMV_RMSNORM, K.GEMV_NONE]
    assert per_token == blocks + blocks + [K.GEMV_NONE], per_token
    for a, b in zip(runs["0"][0], runs["1"][0]):
        assert relerr(a, b) < 2e-2, relerr(a, b)
    c0, c1 = runs["0"][1], runs["1"][1]
    for i in range(cfg.num_hidden_layers):
        if c0.ssm_states[i].numel():
            assert relerr(c0.ssm_states[i], c1.ssm_states[i]) < 2e-2 and relerr(c0.conv_states[i], c1.conv_states[i]) < 2e-2


def test_generate_with_graphed_decode_step_continues_like_the_eager_loop(monkeypatch):
    """`generate()` on a Nemotron-H stack with attention head_dim 128, uniform token drop + TransV (attention layers
    behind a drop stage hold fewer tokens: one device-side key count per distinct length): the captured decode step
    (TV_DECODE_GRAPH, default) and the host-driven loop produce the same greedy continuation."""
    from timeviper_amd.model import build_synthetic_timeviper
    from timeviper_amd.model.llm import decode_graph
    from timeviper_amd.model.llm.nano import NemotronHConfig
    cfg = NemotronHConfig(vocab_size=128, hidden_size=256, intermediate_size=384, num_hidden_layers=8,
                          hybrid_override_pattern="M*-M*-M*", num_attention_heads=4, head_dim=128,
                          num_key_value_heads=2, ssm_state_size=16, mamba_num_heads=8,
                          mamba_n_groups=2, mamba_head_dim=16, mamba_chunk_size=16)
    vlm = build_synthetic_timeviper(cfg, "siglip-vit-b16-224px", pdrop_type="uni_2_0.75-uni_5_0.5",
                                    merge_module="CrossAttention", vit_depth=2, image_size=96)
    with torch.no_grad():       # spread the logits so that greedy decoding has no near-ties
        for blk in vlm.llm_backbone.llm.backbone.layers:
            if blk.block_type == "attention":
                blk.mixer.q_proj.weight.mul_(10.0)
                blk.mixer.k_proj.weight.mul_(10.0)
        vlm.llm_backbone.llm.lm_head.weight.mul_(20.0)
    T = 40                       # 40 frames x 16 tokens: every cache holds >= 256 keys (the split-KV kernel's range) after the drops
    tok = vlm.default_token_id
    ids = torch.tensor([[5, 6, 7] + [tok] * T + [8, 9, 10, 11]], device=DEV)
    pix = torch.randn(T, 3, 96, 96, device=DEV, dtype=torch.bfloat16)
    replays = []
    orig_step = decode_graph.GraphedDecodeStep.step

    def counting_step(self, t):
        out = orig_step(self, t)
        replays.append(self.graph is not None)
        return out
    monkeypatch.setattr(decode_graph.GraphedDecodeStep, "step", counting_step)
    graphed = vlm.generate(ids, pixel_values_videos=pix, max_new_tokens=12, return_ids=True, eos_token_id=-1)
    assert len(replays) == 12 and replays[:2] == [False, False] and all(replays[2:])
    monkeypatch.setenv("TV_DECODE_GRAPH", "0")
    replays.clear()
    eager = vlm.generate(ids, pixel_values_videos=pix, max_new_tokens=12, return_ids=True, eos_token_id=-1)
    assert replays == []
    assert graphed.shape == eager.shape == (1, 12)
    assert torch.equal(graphed, eager), (graphed.tolist(), eager.tolist())


@pytest.mark.parametrize("role,k", [("proj", 1152), ("fc2", 4352)])
def test_vit_residual_accumulate_repeats_bit_for_bit(role, k):
    """SigLIP-so400m's output projections accumulate into the residual stream (model/vit/siglip.py:_accumulate): at
    the forward's row counts the default path must give the same bits on every call of the same inputs, within bf16
    round-off of x + h W^T in fp32."""
    from timeviper_amd.model.vit import siglip
    assert role in siglip._OWN_ACCUM
    g = torch.Generator(device=DEV).manual_seed(0)
    M = 256 * 729
    x0 = torch.randn(M, 1152, device=DEV, generator=g).bfloat16()
    h = torch.randn(M, k, device=DEV, generator=g).bfloat16()
    w = (torch.randn(1152, k, device=DEV, generator=g) * 0.02).bfloat16()
    with torch.inference_mode():
        first = None
        for _ in range(40):
            x = x0.clone()
            siglip._accumulate(x, h, w, role)
            if first is None:
                first = x
            else:
                assert torch.equal(x, first)
        ref = torch.addmm(x0.float(), h.float(), w.float().t())
    assert relerr(first, ref) < 1e-2
