"""`GenericTimeViperVLM` / `HybridTimeViperVLM` — the outer drop-in boundary
(reference timeviper/model/generic_vlm.py:60-972, hybrid_vlm.py:28-50): same constructor,
attributes (`vision_backbone`, `projector`, `llm_backbone`, `arch_specifier`,
`llm_tokenizer`, `default_token_id`, `config`, `device`) and `forward` / `generate`
signatures, inference paths only.

forward (prefill) = ViT over 256-frame clips -> ToMe+MLP projector -> splice one
(tokens_per_frame, D) block per `<image>` placeholder -> hybrid LM (:221-399).
"""
from __future__ import annotations

import os

from typing import List, Optional, Union

import torch
import torch.nn as nn

from .llm import GenericLLMBackbone
from .llm.nano import CausalLMOutputWithPast
from .projector import MLPProjector, MultiMLPProjector, MultiToMe16_mlp_hd64, ToMe16_mlp_hd64
from .vit import VisionBackbone

IGNORE_INDEX = -100
DEFAULT_TOKEN = "<image>"


def _parse_compressed_tokens(arch_specifier: str) -> int:
    parts = arch_specifier.split("-")
    assert parts[-1].isdigit(), f"Cannot parse compressed tokens from {arch_specifier}"
    return int(parts[-1])


class GenericTimeViperVLM(nn.Module):
    supports_gradient_checkpointing = True
    _is_stateful = False

    def __init__(self, model_id: str, vision_backbone: VisionBackbone,
                 llm_backbone: GenericLLMBackbone, enable_mixed_precision_training: bool = True,
                 arch_specifier: str = "gelu_mlp", visual_token_order: str = "raw",
                 disable_data_packing: bool = False) -> None:
        super().__init__()
        self.model_family = f"{llm_backbone.llm_family}"
        self.model_id = model_id
        self.vision_backbone = vision_backbone
        self.llm_backbone = llm_backbone
        self.enable_mixed_precision_training = enable_mixed_precision_training
        self.main_input_name = "input_ids"
        self.arch_specifier = arch_specifier
        assert visual_token_order in ["raw", "ascending", "descending"]
        self._initialize_projector(visual_token_order)
        self.vision_backbone_requires_grad = False
        self.all_module_keys = ["vision_backbone", "llm_backbone", "projector"]
        self.eos_token_ids_to_use = getattr(llm_backbone, "terminators",
                                            [llm_backbone.tokenizer.eos_token_id])
        bb = self.llm_backbone.llm.backbone
        self.use_pdrop = bool(getattr(bb, "use_pdrop", False))
        self.pdrop_args = {"use_pdrop": self.use_pdrop}
        if self.use_pdrop:  # :105-126
            types = bb.pdrop_types
            self.pdrop_args.update({"pdrop_compress_types": [t[0] for t in types],
                                    "pdrop_layers": [int(t[1]) for t in types],
                                    "pdrop_ratios": [1] + [float(t[2]) for t in types]})
            self.llm_backbone.llm.set_pdrop_args(**self.pdrop_args)
        self.disable_data_packing = disable_data_packing
        self.vit_clip_frames = 256  # :274
        # The reference's 256-frame clips bound activation memory on 80 GB parts.  Towers that treat
        # every frame on its own (timm ViTs + frame-wise ToMe) give the same result for any clip
        # size, and larger GEMM / elementwise launches run ~6 % faster on MI355X (288 GB), so such
        # towers are fed `vit_clip_fuse` clips at a time.  InternVideo2 regroups frames into tubes
        # with a reshape that depends on the clip length (model.py:178-182): it regroups every 256 frames
        # as a separate call would, then runs the tubes of all fused clips as one batch.
        self.vit_clip_fuse = 8

    # ---- attributes read by callers (evaluate.py:223,392-393,619) ----
    @property
    def device(self) -> torch.device:
        return next(self.parameters()).device

    @property
    def dtype(self) -> torch.dtype:
        return torch.bfloat16

    @staticmethod
    def can_generate() -> bool:
        return True

    @property
    def llm_tokenizer(self):
        return self.llm_backbone.tokenizer

    @property
    def default_token_id(self):
        return self.llm_tokenizer.convert_tokens_to_ids(DEFAULT_TOKEN)

    @property
    def config(self):
        return self.llm_backbone.llm.config

    def _initialize_projector(self, visual_token_order):
        vdim, ldim = self.vision_backbone.embed_dim, self.llm_backbone.embed_dim
        multi = hasattr(self.vision_backbone, "backbone_ids") and \
            isinstance(self.vision_backbone.backbone_ids, list)
        if multi:
            dims = {bid: self.vision_backbone.backbones[bid.replace("-", "_")].embed_dim
                    for bid in self.vision_backbone.backbone_ids}
            if "gelu_mlp" in self.arch_specifier:
                self.projector = MultiMLPProjector(dims, ldim)
            elif "tome_mlp" in self.arch_specifier:
                self.num_compressed_tokens = _parse_compressed_tokens(self.arch_specifier)
                self.projector = MultiToMe16_mlp_hd64(
                    dims, ldim, mlp_type=self.arch_specifier.split("-")[0],
                    num_compressed_tokens=self.num_compressed_tokens, token_order=visual_token_order)
            else:
                raise ValueError(f"MultiViTBackbone only supports gelu_mlp or tome_mlp projector "
                                 f"for now, got {self.arch_specifier}")
        elif "gelu_mlp" in self.arch_specifier:
            self.projector = MLPProjector(vdim, ldim)
        elif "tome_mlp" in self.arch_specifier:
            self.num_compressed_tokens = _parse_compressed_tokens(self.arch_specifier)
            self.projector = ToMe16_mlp_hd64(
                vdim, ldim, mlp_type=self.arch_specifier.split("-")[0],
                num_compressed_tokens=self.num_compressed_tokens, token_order=visual_token_order)
        else:
            raise ValueError(f"GenericTimeViperVLM with projector architecture "
                             f"`{self.arch_specifier}` is not supported!")

    # ---- vision ----
    def projector_forward(self, patch_features, is_video=False):
        """:401-438."""
        ident = self.vision_backbone.get_identifier
        if "tome_mlp" in self.arch_specifier:
            if ident in ["siglip", "dinov2siglip", "dinov2"]:
                return self.projector(patch_features, compress=True, local_num_frames=1)
            if ident in ["internvideo2"]:
                lnf = 4 if is_video else 1
                ve = self.projector(patch_features, compress=True, local_num_frames=lnf)
                if is_video:
                    b, n, d = ve.shape
                    ve = ve.view(b * 4, n // 4, d)
                return ve
            if ident in ["multivit"]:
                lnf = {bid: (4 if ("internvideo2" in bid and is_video) else 1)
                       for bid in self.vision_backbone.backbone_ids}
                return self.projector(patch_features, compress=True, local_num_frames=lnf)
            raise ValueError(ident)
        ve = self.projector(patch_features)
        if ident in ["internvideo2"] and is_video:
            b, n, d = ve.shape
            ve = ve.view(b * 4, n // 4, d)
        self.num_compressed_tokens = ve.shape[1]
        return ve

    @torch.no_grad()
    def encode_vision(self, vision_inputs, is_video: bool):
        """eval branch of :266-281: clips of 256 frames through ViT + projector."""
        vb, n, kw = self.vision_backbone, self.vit_clip_frames, {}
        if getattr(vb, "frame_independent", False):
            n *= max(1, int(self.vit_clip_fuse))
        elif getattr(vb, "batched_clips", False) and is_video:
            # the backbone regroups every `vit_clip_frames` frames as a separate call would and runs
            # the tubes of `vit_clip_fuse` clips as one batch
            kw = {"clip_frames": n}
            n *= max(1, int(self.vit_clip_fuse))
        feats = [self.projector_forward(vb(clip, is_video=is_video, **kw), is_video=is_video)
                 for clip in vision_inputs.split(split_size=n)]
        return torch.cat(feats, dim=0)

    # ---- fusion ----
    def get_fused_data_nopacked(self, visual_embeddings, input_ids, labels=None):
        """:517-564, batch 1.  The reference walks the placeholders in a Python loop (one
        iteration per frame); here the common layout — one contiguous run of `<image>`
        tokens — is a single concatenation, and anything else takes the general walk."""
        if labels is not None:
            raise NotImplementedError("labels are a training feature")
        ids = input_ids[0]
        is_img = ids == self.default_token_id
        pos = is_img.nonzero(as_tuple=False).flatten()
        n = pos.numel()
        embed = self.llm_backbone.embed_input_ids
        first, last = int(pos[0]), int(pos[-1])
        vis = visual_embeddings
        if last - first + 1 == n and n == vis.shape[0]:
            parts = [embed(ids[None, :first]), vis.reshape(1, -1, vis.shape[-1]).to(self.dtype_of(embed))]
            if last + 1 < ids.shape[0]:
                parts.append(embed(ids[None, last + 1:]))
            return torch.cat(parts, dim=1), None
        plist = pos.tolist()
        out = [embed(ids[None, :plist[0]])]
        for i, s in enumerate(plist):
            out.append(vis[i:i + 1].to(out[0].dtype))
            start = s + 1
            end = plist[i + 1] if i < n - 1 else ids.shape[0]
            if start < ids.shape[0] and bool(is_img[start]):
                continue
            out.append(embed(ids[None, start:end]))
        return torch.cat(out, dim=1), None

    def dtype_of(self, embed):
        return self.llm_backbone.llm.get_input_embeddings().weight.dtype

    def pdrop_bookkeeping(self, input_ids, visual_embeddings):
        """:291-309."""
        is_img = input_ids.eq(self.default_token_id)
        return {"first_vision_token_positions": torch.argmax(is_img.int(), dim=1),
                "text_prompt_lens": [int(input_ids.shape[1] - int(is_img[0].sum()))],
                "num_vision_tokens": [visual_embeddings.size(0) * visual_embeddings.size(1)],
                "is_interleaved": False}

    # ---- forward / generate ----
    def forward(self, input_ids: Optional[torch.LongTensor] = None, attention_mask=None,
                pixel_values=None, pixel_values_videos=None, labels=None, inputs_embeds=None,
                past_key_values=None, use_cache=None, output_attentions=None,
                output_hidden_states=None, return_dict=None, position_ids=None,
                cache_position=None, inference_params=None, num_last_tokens: int = 0,
                answer_prompt: Optional[str] = None, logits_to_keep: Union[int, torch.Tensor, None] = None,
                image_grid_thw=None, video_grid_thw=None, logits_cache=None, txt_seq_lens=None,
                img_seq_lens=None, vid_seq_lens=None, multimodal_indices=None,
                visual_embeddings: Optional[torch.Tensor] = None) -> CausalLMOutputWithPast:
        if self.training:
            raise NotImplementedError("timeviper_amd implements the inference forward only")
        has_pixels = not (pixel_values is None and pixel_values_videos is None and visual_embeddings is None)
        if has_pixels and past_key_values is not None and cache_position is not None and int(cache_position[0]) > 0:
            raise NotImplementedError("a continuation (cache_position > 0) takes text only: new frames behind the "
                                      "token-drop stages of a finished prefill are not implemented")
        if not has_pixels:
            return self.llm_backbone(input_ids=input_ids, attention_mask=None,
                                     position_ids=position_ids, past_key_values=past_key_values,
                                     inputs_embeds=inputs_embeds, use_cache=use_cache,
                                     output_hidden_states=output_hidden_states,
                                     cache_position=cache_position, logits_to_keep=logits_to_keep,
                                     train_pdrop_args=self.pdrop_args if self.use_pdrop else None)
        if visual_embeddings is None:
            vin = pixel_values_videos if pixel_values_videos is not None else pixel_values
            visual_embeddings = self.encode_vision(vin, is_video=pixel_values_videos is not None)
        assert input_ids is not None and input_ids.shape[0] == 1
        train_pdrop_args = None
        if self.use_pdrop:
            train_pdrop_args = self.pdrop_bookkeeping(input_ids, visual_embeddings)
            self.pdrop_args.update(train_pdrop_args)
            train_pdrop_args = self.pdrop_args
        fused, _ = self.get_fused_data_nopacked(visual_embeddings, input_ids, None)
        L = fused.shape[1]
        # flash_attention_2 => mask None, positions = arange(L)   (:496-497, :512-514)
        position_ids = torch.arange(L, device=fused.device).unsqueeze(0)
        fused_cache_position = torch.arange(L, device=fused.device) if cache_position is not None else None
        return self.llm_backbone(input_ids=None, attention_mask=None, position_ids=position_ids,
                                 past_key_values=past_key_values, inputs_embeds=fused,
                                 use_cache=use_cache, output_hidden_states=output_hidden_states,
                                 cache_position=fused_cache_position, logits_to_keep=logits_to_keep,
                                 train_pdrop_args=train_pdrop_args)

    def prepare_inputs_for_generation(self, input_ids, past_key_values=None, attention_mask=None,
                                      inputs_embeds=None, cache_position=None, **kwargs):
        """generic_vlm.py:762-848 for the native greedy loop below.  Prefill (no cache yet, or more
        than one position): the tokenised `answer_prompt` is appended to the prompt (:772-785) and the
        pixels ride along (:793-795).  Decode step: no pixels; position = tokens the attention cache
        holds (:797-826; the reference reads layer 7 / 14's KV length, `get_seq_length()` here finds
        the first attention layer) and, under flash_attention_2, no mask (:828-832)."""
        is_prefill = past_key_values is None or cache_position is None or cache_position.shape[0] != 1
        if is_prefill:
            ap = kwargs.get("answer_prompt")
            if ap:
                ap_ids = self.llm_backbone.tokenizer(ap, add_special_tokens=False, return_tensors="pt").input_ids
                ap_ids = ap_ids.to(input_ids.device).expand(input_ids.shape[0], -1)
                input_ids = torch.cat([input_ids, ap_ids], dim=1)
                if attention_mask is not None:
                    attention_mask = torch.cat([attention_mask, torch.ones_like(ap_ids)], dim=1)
            if attention_mask is not None and not bool(attention_mask.all()):
                raise NotImplementedError("padded prompts (attention_mask with zeros) are not on the batch-1 "
                                          "evaluation path")
            return {"input_ids": input_ids, "attention_mask": None, "past_key_values": past_key_values,
                    "pixel_values": kwargs.get("pixel_values"),
                    "pixel_values_videos": kwargs.get("pixel_values_videos"), "use_cache": True,
                    "cache_position": torch.zeros(1, dtype=torch.long)}
        past_len = past_key_values.get_seq_length()
        cp = torch.tensor([max(past_len, 1)])          # host side: the mixers branch on it
        return {"input_ids": input_ids[:, -1:], "attention_mask": None, "past_key_values": past_key_values,
                "pixel_values": None, "pixel_values_videos": None, "use_cache": True, "cache_position": cp,
                "position_ids": cp.view(1, 1).to(input_ids.device)}

    @torch.inference_mode()
    def generate(self, *args, **kwargs):
        """Greedy decoding with the hybrid cache: what evaluate.py:507-525 asks of HF's
        GenerationMixin (`do_sample=False, use_cache=True, temperature=0, answer_prompt=...`), with
        the reference's return contract (generic_vlm.py:743-760): the DECODED text of the new tokens
        (prompt stripped, `.strip()`-ed), which evaluate.py:529 hands to `extract_answer`.
        `return_ids=True` (or HF's `return_dict_in_generate=True`, or a tokenizer without `decode`)
        returns the (1, n_new) id tensor instead.
        Conversations: `return_past_key_values=True` returns `(result, cache)`; the cache records in `pending_ids` the
        ids emitted but not yet run through the model.  `past_key_values=cache` with the next turn's `input_ids` (text
        only) feeds pending ids + new ids + `answer_prompt` through ONE continuation forward of that cache instead of
        a new prefill, then decodes as usual.
        Sampled decoding: `do_sample=True` with `temperature` (> 0; default 1), `top_k` (0: off), `top_p` (>= 1: off) —
        the arguments of the reference's second front-end (eval/vllm_inference/vllm_infer.py) — and `seed` (required:
        there is no hidden global random state) draws every token with ONE launch of `kernels.sample_logits` in the place
        of the argmax, inside the captured step where there is one.  The first new token is draw 0 of the stream
        `sample_stream` (default 0), the n-th draw n - 1: the same call returns the same ids, graphed or not.
        `do_sample=False` (any temperature) and `do_sample=True, temperature=0` decode greedily.  `speculative=D` with
        sampling decodes plainly; `repetition_penalty != 1` and `num_beams > 1` raise NotImplementedError."""
        input_ids = args[0] if args else kwargs.pop("input_ids", None)
        pixel_values = kwargs.pop("pixel_values", None)
        pixel_values_videos = kwargs.pop("pixel_values_videos", None)
        attention_mask = kwargs.pop("attention_mask", None)
        max_new_tokens = int(kwargs.pop("max_new_tokens", 128))
        return_ids = bool(kwargs.pop("return_ids", False)) or bool(kwargs.pop("return_dict_in_generate", False))
        from .llm.sampling import Sampler, sampling_arguments
        sampling = sampling_arguments(kwargs, "generate")      # None: greedy
        sample_stream = int(kwargs.pop("sample_stream", 0))
        eos = self._eos_set(kwargs.pop("eos_token_id", None))
        llm = self.llm_backbone.llm
        cache = kwargs.pop("past_key_values", None)
        return_cache = bool(kwargs.pop("return_past_key_values", False))
        speculative = kwargs.pop("speculative", None)
        draft_fn = kwargs.pop("draft_fn", None)
        mi = self.prepare_inputs_for_generation(input_ids, past_key_values=None, attention_mask=attention_mask,
                                                pixel_values=pixel_values, pixel_values_videos=pixel_values_videos,
                                                answer_prompt=kwargs.pop("answer_prompt", None))
        pdargs = self.pdrop_args if self.use_pdrop else None
        prompt_ids = mi["input_ids"]                       # (with the answer prompt: what the drafter looks drafts up in)
        if cache is None:
            cache = llm.new_cache(1, dtype=self.dtype, device=self.device)
            out = self.forward(input_ids=mi["input_ids"], pixel_values=mi["pixel_values"],
                               pixel_values_videos=mi["pixel_values_videos"], past_key_values=cache,
                               use_cache=True, cache_position=mi["cache_position"])
            # the drop bookkeeping of THIS prefill (tokens per stage: the position shift of every later token) travels
            # with its cache: the model object may prefill another video before the conversation goes on
            cache.pdrop_args = dict(pdargs) if pdargs is not None else None
        else:
            # the next turn of a conversation: the ids the last turn emitted but never fed + this turn's ids (+ the
            # answer prompt) go through ONE continuation forward of the cache the last turn left
            if mi["pixel_values"] is not None or mi["pixel_values_videos"] is not None:
                raise NotImplementedError("generate(past_key_values=...) continues with text only: new frames behind "
                                          "the token-drop stages of a finished prefill are not implemented")
            if hasattr(cache, "end_static_decode"):
                cache.end_static_decode()          # the last turn's fixed buffers: rows are appended again
            if getattr(cache, "attention_layers", None) and cache.get_seq_length() == 0:
                raise ValueError("generate(past_key_values=...): the cache holds no prefill")
            pdargs = getattr(cache, "pdrop_args", pdargs)
            ids = mi["input_ids"].to(self.device)
            pending = getattr(cache, "pending_ids", None)
            if pending is not None and pending.numel():
                ids = torch.cat([pending.to(ids.device).view(1, -1), ids], dim=1)
            # the position convention of the decode step (prepare_inputs_for_generation, reference :797-826): the tokens the
            # first attention layer holds — what T single steps would be given, so that the two stay interchangeable
            past_len = max(cache.get_seq_length(), 1)
            pos = (past_len + torch.arange(ids.shape[1], device=ids.device)).unsqueeze(0)
            out = self.llm_backbone(input_ids=ids, past_key_values=cache, use_cache=True,
                                    cache_position=torch.tensor([past_len]), position_ids=pos, train_pdrop_args=pdargs)
        new_tokens: List[int] = []
        fed = 0                               # how many of them went through the model
        # sampled decoding: the first token is draw 0 of the stream, the n-th new token draw n - 1 (llm/sampling.py)
        sampler = None if sampling is None else Sampler(self.device, streams=(sample_stream,), **sampling)
        pick = (lambda logits: logits.argmax(-1)) if sampler is None else sampler.sample
        tok = pick(out.logits[:, -1])
        self.last_generate_stats = {"speculative": False, "steps": 0, "drafted": 0, "accepted": 0, "emitted": 0,
                                    "graphed": False, "replays": 0, "graphs": 0, "capture_error": None,
                                    "fp8_weights": self._fp8_weights_on()}
        n_drafts = self._speculative_drafts(speculative, cache, max_new_tokens, sampled=sampler is not None)
        if n_drafts:
            history = [int(t) for t in prompt_ids.reshape(-1).tolist()]
            new_tokens, fed = self._speculative_decode(cache, int(tok), n_drafts, draft_fn, history, max_new_tokens, eos, pdargs)
            return self._finish_generate(new_tokens, fed, cache, return_ids, return_cache)
        stepper = self._graphed_decode_step(cache, max_new_tokens, pdargs, sampler)
        for _ in range(max_new_tokens):
            t = int(tok)
            new_tokens.append(t)
            if t in eos:
                break
            fed += 1
            if stepper is not None:            # the same step as below, replayed as one hipGraph launch
                tok = stepper.step(tok.view(1, 1))
                continue
            mi = self.prepare_inputs_for_generation(tok.view(1, 1), past_key_values=cache,
                                                    cache_position=torch.zeros(1, dtype=torch.long))
            out = self.llm_backbone(input_ids=mi["input_ids"], past_key_values=cache, use_cache=True,
                                    cache_position=mi["cache_position"], position_ids=mi["position_ids"],
                                    train_pdrop_args=pdargs)
            tok = pick(out.logits[:, -1])
        self.last_generate_stats.update(steps=fed, emitted=len(new_tokens), graphed=stepper is not None
                                        and stepper.graph is not None)
        return self._finish_generate(new_tokens, fed, cache, return_ids, return_cache)

    # ------------------------------------------------------------------ decode on e4m3 weights
    def quantize_llm_weights_e4m3(self) -> int:
        """`NemotronHForCausalLM.quantize_weights_e4m3` of the language model: its linear weights rounded to e4m3 with
        power-of-two row scales IN PLACE (the originals are gone), the 8-bit copies kept for the decode step's products.
        Opt-in; every decode mode (plain, speculative, branched, sampled, graphed) then runs on them unchanged."""
        llm = self.llm_backbone.llm
        if not hasattr(llm, "quantize_weights_e4m3"):
            raise NotImplementedError(f"e4m3 weights are implemented for the Nemotron-H hybrid only, not {type(llm).__name__}")
        return llm.quantize_weights_e4m3()

    def drop_llm_fp8_weights(self) -> None:
        """Free the 8-bit copies (the rounded bf16 weights stay)."""
        llm = self.llm_backbone.llm
        if not hasattr(llm, "drop_fp8_weights"):
            raise NotImplementedError(f"e4m3 weights are implemented for the Nemotron-H hybrid only, not {type(llm).__name__}")
        llm.drop_fp8_weights()

    def _fp8_weights_on(self) -> bool:
        """Whether the decode products of this call read e4m3 copies: quantized, not dropped, TV_FP8W not 0, on the GPU."""
        llm = self.llm_backbone.llm
        return bool(getattr(llm, "has_fp8_weights", lambda: False)() and os.environ.get("TV_FP8W", "1") != "0"
                    and self.device.type == "cuda")

    def _eos_set(self, eos_token_id) -> set:
        eos = self.eos_token_ids_to_use if eos_token_id is None else eos_token_id
        return set(int(t) for t in (eos if isinstance(eos, (list, tuple)) else [eos]))

    def _result(self, ids, return_ids):
        """New ids (1, n) as `generate` returns them: decoded and stripped, or the tensor itself."""
        tokenizer = self.llm_backbone.tokenizer
        if return_ids or not hasattr(tokenizer, "decode"):
            return ids
        return tokenizer.decode(ids[0], skip_special_tokens=False).strip()

    def _finish_generate(self, new_tokens, fed, cache, return_ids, return_cache):
        ids = torch.tensor([new_tokens], device=self.device)
        cache.pending_ids = ids[:, fed:].clone()
        result = self._result(ids, return_ids)
        return (result, cache) if return_cache else result

    def _step_fn(self, cache, batch_size, pdargs, logits_to_keep=None):
        """step_fn(ids) of the steppers of llm/decode_graph.py: one forward behind the prefill over ids (batch_size, T)
        against `cache` — the hybrid cache or a branch set — returning the logits of the last (`logits_to_keep`) positions."""
        host_pos = torch.ones(1, dtype=torch.long)              # "not the prefill" for the mixers' host-side branch
        dev_pos = torch.ones((batch_size, 1), dtype=torch.long, device=self.device)

        def step_fn(ids):
            return self.llm_backbone(input_ids=ids, past_key_values=cache, use_cache=True, cache_position=host_pos,
                                     position_ids=dev_pos, train_pdrop_args=pdargs, logits_to_keep=logits_to_keep).logits
        return step_fn

    def _hybrid_step_scope(self, cache, columns=None) -> bool:
        """What the captured decode step, the speculative step and the branched step ask alike: the Nemotron-H hybrid with
        its hybrid cache, attention layers in it, on the GPU head_dim 128 (the split-KV kernels).  `columns`: the tokens or
        branches that share one attention launch (tv_attn_append_fwd, tv_attn_branch_fwd) — then also no fp8 attention,
        bf16 (on the CPU fp32 too) and on the GPU columns x Hq / Hkv <= 128; None: the one-token step, bound by none of it."""
        from .llm.nano import HybridMambaAttentionDynamicCache, NemotronHForCausalLM
        from .. import kernels as K
        llm = self.llm_backbone.llm
        if (not isinstance(llm, NemotronHForCausalLM) or not isinstance(cache, HybridMambaAttentionDynamicCache)
                or not cache.attention_layers):
            return False
        on_gpu = self.device.type == "cuda"
        if on_gpu and cache.key_cache[cache.attention_layers[0]].shape[-1] != 128:
            return False
        if columns is None:
            return True
        cfg = llm.config
        return (not K._ATTN_FP8["on"] and llm.dtype in ((torch.bfloat16,) if on_gpu else (torch.bfloat16, torch.float32))
                and not (on_gpu and columns * (cfg.num_attention_heads // cfg.num_key_value_heads) > 128))

    def _speculative_drafts(self, speculative, cache, max_new_tokens, sampled: bool = False) -> int:
        """Drafts per step D for `generate(speculative=...)`, or 0 where the stack is out of the feature's scope and the
        tokens are decoded plainly: anything but the Nemotron-H hybrid with its hybrid cache (Qwen2's rotary positions),
        fp8 attention, on the GPU anything but bf16 with attention head_dim 128 and (D + 1) x Hq / Hkv <= 128 columns
        (tv_attn_append_fwd with a device-side key count), TV_DECODE_GRAPH=0 there (an eager step of ~400 launches loses
        more than the drafts win), sampled decoding (verifying drafts under a sampler is rejection sampling: not
        implemented; the tokens are sampled plainly)."""
        if speculative is None or speculative is False:
            return 0
        from .llm.nano import continue_t_seq
        from .llm.speculative import DEFAULT_DRAFTS
        D = DEFAULT_DRAFTS if speculative is True else int(speculative)
        if D < 1:
            raise ValueError("generate(speculative=D): D >= 1 drafts per step")
        if sampled or max_new_tokens < 2 or D + 1 > continue_t_seq() or not self._hybrid_step_scope(cache, columns=D + 1):
            return 0
        if self.device.type == "cuda" and os.environ.get("TV_DECODE_GRAPH", "1") == "0":
            return 0
        return D

    def _speculative_decode(self, cache, first, D, draft_fn, history, max_new_tokens, eos, pdargs):
        """The draft-and-verify loop behind `generate(speculative=D)` (llm/speculative.py, llm/decode_graph.py): per step
        ONE forward over [t0, d1 .. dD] against the cache in speculation mode — a captured graph on the GPU — and one read
        of (k, p1 .. pT): p1 .. pk are emitted, t0 and the k - 1 drafts that equal p1 .. p(k-1) stay in the cache.
        Returns (new ids, how many of them went through the model), the cache flushed and out of speculation mode."""
        from .llm.decode_graph import GraphedSpecStep
        from .llm.speculative import prompt_lookup_draft
        if draft_fn is None:
            placeholder = (int(self.default_token_id),)
            draft_fn = lambda ids, n: prompt_lookup_draft(ids, n, exclude_ids=placeholder)
        stats = self.last_generate_stats
        stats["speculative"] = True
        new_tokens, fed, T = [first], 0, D + 1
        if first in eos:
            stats["emitted"] = 1
            return new_tokens, fed
        cache.begin_speculation(T, max_new_tokens)
        step_fn = self._step_fn(cache, 1, pdargs, logits_to_keep=T)
        stepper = GraphedSpecStep(step_fn, cache, T, self.device, graphed=self.device.type == "cuda")
        done = False
        while not done:
            drafts = [int(t) for t in draft_fn(history + new_tokens, D)][:D]
            n_real = len(drafts)
            drafts += [0] * (D - n_real)                          # padding can only be rejected or be right
            k, p = stepper.step(new_tokens[-1], drafts)
            stats["steps"] += 1
            stats["drafted"] += n_real
            stats["accepted"] += min(k - 1, n_real)
            for m in range(1, k + 1):                             # p1 .. pk; t0 and d1 .. d(m-1) are fed and kept
                new_tokens.append(p[m - 1])
                fed += 1
                if p[m - 1] in eos or len(new_tokens) >= max_new_tokens:
                    if m < k:
                        cache.commit(m)
                    done = True
                    break
        if new_tokens[-1] not in eos:
            # the length limit: the plain loop runs its last token through the model too (nothing is left pending)
            with torch.inference_mode():
                step_fn(torch.tensor([[new_tokens[-1]]], device=self.device))
            cache.commit(1)
            fed += 1
        cache.end_speculation()
        stats.update(emitted=len(new_tokens), graphed=bool(stepper.graphs) and stepper.capture_error is None,
                     replays=stepper.replays, graphs=len(stepper.graphs),
                     capture_error=None if stepper.capture_error is None else repr(stepper.capture_error))
        return new_tokens, fed

    def _branch_scope(self, cache, n_branches: int) -> bool:
        """Whether `generate_branches` decodes its questions in lockstep (llm/branch.py): the Nemotron-H hybrid with its
        hybrid cache, 1..16 branches, no fp8 attention; on the GPU bf16, attention head_dim 128 and
        branches x Hq / Hkv <= 128 columns (tv_attn_branch_fwd).  Anything else runs question by question on clones."""
        from .llm.branch import MAX_BRANCHES
        return 1 <= n_branches <= MAX_BRANCHES and self._hybrid_step_scope(cache, columns=n_branches)

    @torch.inference_mode()
    def generate_branches(self, questions, past_key_values=None, max_new_tokens: int = 128, eos_token_id=None,
                          answer_prompt: Optional[str] = None, return_ids: bool = False, **sampling_kwargs) -> list:
        """Several questions about ONE prefilled video: `questions` is a list of 1..16 id tensors (1, T_b), text only,
        `past_key_values` the cache a `generate(..., return_past_key_values=True)` (or a prefill forward) left.  Result b
        is what `generate(questions[b], past_key_values=cache.clone(), ...)` with the same arguments returns; the cache
        itself is not modified.

        The questions are decoded in LOCKSTEP on `cache.branch(B)`: every step feeds ONE token per branch — the cache's
        pending ids, then the branch's question, then the tokenised `answer_prompt`, then the branch's own greedy tokens —
        as the B rows of one forward: the weights are read once per step for all branches, the K / V of the video is
        shared and read once per step and attention layer.  All branches hold the same number of rows at all times; a
        branch with a short question starts answering earlier, a finished one (end-of-sequence id, `max_new_tokens`)
        rides along as a padding row until the last one is done.  The step is one captured graph where plain `generate`
        would capture its step (`TV_DECODE_GRAPH`).  Out of scope (`_branch_scope`: Qwen2, fp32 on the GPU, more than
        16 questions, ...) the questions run one after the other on clones.  `last_generate_stats`: branched, branches,
        steps (forwards), graphed.

        Sampled decoding (`do_sample=True, temperature, top_k, top_p, seed`, as in `generate`): branch b draws from
        stream b, its n-th answer token is draw n - 1 — result b equals `generate(questions[b],
        past_key_values=cache.clone(), do_sample=True, seed=seed, sample_stream=b, ...)`.  `[q] * n` is n samples of one
        question for one prefill."""
        from .llm.sampling import Sampler, sampling_arguments
        sampling = sampling_arguments(sampling_kwargs, "generate_branches")
        if sampling_kwargs:
            raise TypeError(f"generate_branches: unexpected arguments {sorted(sampling_kwargs)}")
        cache = past_key_values
        if cache is None:
            raise ValueError("generate_branches: past_key_values (the prefilled cache the questions are about) is required")
        questions = [q.view(1, -1) for q in questions]
        B, max_new_tokens = len(questions), int(max_new_tokens)
        if B < 1 or any(q.numel() == 0 for q in questions):
            raise ValueError("generate_branches: at least one question, each of at least one id")
        if not self._branch_scope(cache, B):
            results, steps, graphed = [], 0, False
            for b, q in enumerate(questions):
                sample = {} if sampling is None else dict(sampling, do_sample=True, sample_stream=b)
                results.append(self.generate(q, past_key_values=cache.clone(), max_new_tokens=max_new_tokens,
                                             eos_token_id=eos_token_id, answer_prompt=answer_prompt, return_ids=return_ids,
                                             **sample))
                steps += self.last_generate_stats["steps"]
                graphed = graphed or bool(self.last_generate_stats["graphed"])
            self.last_generate_stats = {"branched": False, "branches": B, "steps": steps, "graphed": graphed,
                                        "fp8_weights": self._fp8_weights_on()}
            return results
        eos = self._eos_set(eos_token_id)
        if getattr(cache, "get_seq_length", None) and cache.get_seq_length() == 0:
            raise ValueError("generate_branches: the cache holds no prefill")
        tail: List[int] = []
        if answer_prompt:
            tail = self.llm_backbone.tokenizer(answer_prompt, add_special_tokens=False,
                                               return_tensors="pt").input_ids.reshape(-1).tolist()
        pending = getattr(cache, "pending_ids", None)
        head = [] if pending is None else pending.reshape(-1).tolist()
        feeds = [[int(t) for t in head + q.reshape(-1).tolist() + tail] for q in questions]
        n_steps = max(len(f) for f in feeds) + max(max_new_tokens - 1, 0)       # (the last emitted token is not fed)
        bs = cache.branch(B, suffix_cap=n_steps)
        bs.begin_static_decode(n_steps)
        pdargs = getattr(bs, "pdrop_args", self.pdrop_args if self.use_pdrop else None)      # (as `generate` reads the cache's)
        step_fn = self._step_fn(bs, B, pdargs)
        # branch b samples from stream b; its draw index (the tokens it has emitted) is written from the host every step
        sampler = None if sampling is None else Sampler(self.device, streams=range(B), advance=False, **sampling)
        pick = (lambda logits: logits.argmax(-1)) if sampler is None else sampler.sample
        stepper = None
        if (os.environ.get("TV_DECODE_GRAPH", "1") != "0" and self.device.type == "cuda" and max_new_tokens >= 8
                and self.dtype == torch.bfloat16):
            from .llm.decode_graph import GraphedDecodeStep
            stepper = GraphedDecodeStep(step_fn, bs, B, self.device, sampler=sampler)
        new_tokens: List[List[int]] = [[] for _ in range(B)]
        done = [max_new_tokens <= 0] * B
        steps = 0
        while not all(done):
            # branch b feeds its prompt, then its own last token; a finished branch rides along as a padding row
            row = [f[steps] if steps < len(f) else (t[-1] if t else 0) for f, t in zip(feeds, new_tokens)]
            ids = torch.tensor(row, dtype=torch.long, device=self.device).view(B, 1)
            if sampler is not None:
                sampler.set_draws([len(t) for t in new_tokens])
            if stepper is not None:
                nxt = stepper.step(ids)
            else:
                nxt = pick(step_fn(ids)[:, -1])
                bs.advance_static_device()
            steps += 1
            nxt = nxt.reshape(-1).tolist()
            for b in range(B):
                if done[b] or steps < len(feeds[b]):            # (still inside its prompt: the logits are not its answer's)
                    continue
                new_tokens[b].append(int(nxt[b]))
                done[b] = nxt[b] in eos or len(new_tokens[b]) >= max_new_tokens
        self.last_generate_stats = {"branched": True, "branches": B, "steps": steps,
                                    "graphed": stepper is not None and stepper.graph is not None,
                                    "fp8_weights": self._fp8_weights_on()}
        return [self._result(torch.tensor([t], device=self.device), return_ids) for t in new_tokens]

    def _graphed_decode_step(self, cache, max_new_tokens, pdargs, sampler=None):
        """The decode step behind `generate` as a captured graph (llm/decode_graph.py) where the stack allows it: the
        Nemotron-H hybrid (no positional encoding), bf16, attention head_dim 128 (tv_attn_decode_fwd), on the GPU, and
        enough tokens to pay for two eager warm-up steps and the capture.  TV_DECODE_GRAPH=0 keeps the eager loop."""
        from .llm.decode_graph import GraphedDecodeStep
        if (os.environ.get("TV_DECODE_GRAPH", "1") == "0" or self.device.type != "cuda" or max_new_tokens < 8
                or self.dtype != torch.bfloat16 or not self._hybrid_step_scope(cache)):
            return None
        cache.begin_static_decode(max_new_tokens)
        return GraphedDecodeStep(self._step_fn(cache, 1, pdargs), cache, 1, self.device, sampler=sampler)

    @classmethod
    def from_pretrained(cls, pretrained_checkpoint, model_id: str, vision_backbone: VisionBackbone,
                        llm_backbone: GenericLLMBackbone, enable_mixed_precision_training: bool = True,
                        arch_specifier: str = "gelu_mlp", visual_token_order: str = "raw"):
        """generic_vlm.py:874-910 (called at evaluate.py:198-214): build, `torch.load` the
        state dict, `load_state_dict(strict=True)`, freeze, eval, move to the GPU in bf16."""
        vlm = cls(model_id, vision_backbone, llm_backbone,
                  enable_mixed_precision_training=enable_mixed_precision_training,
                  arch_specifier=arch_specifier, visual_token_order=visual_token_order)
        pretrained_weights = torch.load(pretrained_checkpoint, map_location="cpu")
        vlm.load_state_dict(pretrained_weights, strict=True)
        vlm.requires_grad_(False)
        vlm.eval()
        device = torch.device("cuda") if torch.cuda.is_available() else torch.device("cpu")
        vlm.to(device, dtype=torch.bfloat16)
        return vlm


class HybridTimeViperVLM(GenericTimeViperVLM):
    """hybrid_vlm.py:28-50 only patches HF's cache preparation; with the native greedy
    `generate` above there is nothing left to patch."""
