"""Sampled decoding: the state a generation keeps around `kernels.sample_logits`.

The sampler sits where the decode step ends in `argmax` (llm/decode_graph.py): one launch per step, no host round trip,
replayable by the captured graph.  What changes from token to token — the draw index of every row — lives in device
memory at a fixed address; the seed and the parameters are launch constants of that generation's graph.  There is no
hidden global random state: token n of a generation is Philox4x32-10 at counter (n - 1, stream) under the key `seed`,
whatever ran before, graphed or not.
"""
from __future__ import annotations

from typing import Optional, Sequence

import torch

__all__ = ["Sampler", "sampling_arguments"]


def sampling_arguments(kwargs: dict, who: str) -> Optional[dict]:
    """Pops the decoding-strategy arguments of `generate` / `generate_branches` from kwargs.  Returns None for greedy
    decoding — `do_sample=False` with any temperature (what evaluate.py asks for), or `do_sample=True, temperature=0`
    (the vLLM convention of the reference's second front-end) — else the sampler's parameters."""
    do_sample = bool(kwargs.pop("do_sample", False))
    temperature = kwargs.pop("temperature", None)
    top_k, top_p = kwargs.pop("top_k", None), kwargs.pop("top_p", None)
    seed = kwargs.pop("seed", None)
    rp, nb = kwargs.pop("repetition_penalty", None), kwargs.pop("num_beams", None)
    if rp is not None and float(rp) != 1.0:
        raise NotImplementedError(f"{who}: repetition_penalty other than 1.0 is not implemented")
    if nb is not None and int(nb) > 1:
        raise NotImplementedError(f"{who}: num_beams > 1 (beam search) is not implemented")
    temperature = 1.0 if temperature is None else float(temperature)
    if temperature < 0.0:
        raise ValueError(f"{who}: temperature must not be negative")
    if not do_sample or temperature == 0.0:
        return None
    top_k = 0 if top_k is None else int(top_k)
    top_p = 1.0 if top_p is None else float(top_p)
    if top_k < 0 or not top_p > 0.0:
        raise ValueError(f"{who}: top_k >= 0 (0: off) and top_p > 0 (>= 1: off)")
    if seed is None:
        raise ValueError(f"{who}(do_sample=True) needs seed=...: there is no hidden global random state")
    return {"seed": int(seed), "temperature": temperature, "top_k": top_k, "top_p": top_p}


class Sampler:
    """`sample(logits)` -> (B,) ids for the B rows of one step.  Row b draws at (draws[b], streams[b]); `advance=True`
    (plain `generate`) bumps the draw indices on the device after every call — inside the graph when the step is
    captured —, `advance=False` leaves them to the caller (`generate_branches` writes them every step)."""

    def __init__(self, device, seed: int, temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0,
                 streams: Sequence[int] = (0,), advance: bool = True):
        self.seed, self.temperature, self.top_k, self.top_p = int(seed), float(temperature), int(top_k), float(top_p)
        self.advance = bool(advance)
        self.streams = torch.tensor([int(s) for s in streams], dtype=torch.int32, device=device)
        self.draws = torch.zeros(len(streams), dtype=torch.int64, device=device)

    def set_draws(self, draws: Sequence[int]) -> None:
        self.draws.copy_(torch.tensor([int(d) for d in draws], dtype=torch.int64))

    def sample(self, logits: torch.Tensor) -> torch.Tensor:
        from ... import kernels as K
        logits = logits[:, -1] if logits.dim() == 3 else logits
        if logits.dtype != torch.float32:
            logits = logits.float()
        ids = K.sample_logits(logits, self.draws, self.streams, self.seed, temperature=self.temperature,
                              top_k=self.top_k, top_p=self.top_p)
        if self.advance:
            self.draws.add_(1)
        return ids
