"""One decode step as ONE hipGraph launch.

A generated token of the hybrid stack is ~330 small launches (27 Mamba-2 mixers x {in_proj, conv update, state update,
gated norm, out_proj, norm}, 25 MLPs, 4 attention layers) that together move the 16.6 GB of weights once: ~2 ms of HBM
time at batch 1, against ~10 ms of host work when every launch is issued from Python (bench.py --config decode).  The
reference's loop (HF `generate`, evaluate.py:507-525 -> modeling_nano.py:484-546, 1666-1689) has the same shape and the
same problem.  On MI355X the answer is a captured graph rather than a tracing compiler: the step is made
launch-parameter-static — the K / V buffers have fixed capacity, the write slot and the key count live in device
memory (`HybridMambaAttentionDynamicCache.begin_static_decode`), the attention kernel reads the count there
(`tv_attn_decode_fwd(seqlens_k)`), the conv / SSM states are updated in place — captured once after two eager warm-up
tokens, and replayed per token with one `hipGraphLaunch`.

`_GraphedStep` warms up, captures, replays and falls back to the eager step, once for both steppers: `GraphedDecodeStep`
(one token per sequence: plain, sampled or branched decoding) and `GraphedSpecStep` (speculative decoding) say what a step
runs, which graph it belongs to and what the host does around a replay.

Valid for stacks whose decode step does not depend on the host-side position: the Nemotron-H hybrid has no positional
encoding (modeling_nano.py:1012-1220); a rotary backbone (Qwen2) would bake its angle in — `GraphedDecodeStep` is not
offered for it.
"""
from __future__ import annotations

from typing import Callable

import warnings

import torch

__all__ = ["GraphedDecodeStep", "GraphedSpecStep"]


class _GraphedStep:
    """`_launch()` runs one step: the first `warmup` calls eagerly (lazy initialisations: kernel attributes, cached
    constants, library workspaces), then one capture per graph key, then replays.  A subclass supplies `_run()` (the step),
    `_key()` (the graph the next step belongs to), `_before_replay()` / `_after_replay()` (the host checks and bookkeeping
    `_run` would have done).  If a capture raises, the cache's host bookkeeping — advanced without a kernel having run —
    goes back through `cache.host_state()` / `restore_host_state()` and this and every later step run eagerly; out of
    memory is re-raised instead (not a capture problem: the eager loop would only run out of memory later)."""
    what, unit = "decode", "token"          # the warning's wording

    def __init__(self, step_fn: Callable[[torch.Tensor], torch.Tensor], cache, ids_shape, device, warmup: int, graphed: bool):
        self.step_fn, self.cache, self.warmup = step_fn, cache, int(warmup)
        self.ids = torch.zeros(ids_shape, dtype=torch.int64, device=device)
        self.graphed = bool(graphed)      # False: every step eager (the CPU, or a caller that wants no capture)
        self.graphs, self.outs = {}, {}   # per graph key: the captured step and what its `_run` returned
        self.capture_error = None         # set when a capture failed: the stepper then runs every step eagerly
        self.calls, self.replays = 0, 0

    def _key(self):
        return 0

    def _before_replay(self):
        pass

    def _launch(self):
        self.calls += 1
        key = self._key()
        if key in self.graphs:
            self._before_replay()
            self.graphs[key].replay()
            self._after_replay()
            self.replays += 1
            return self.outs[key]
        if not self.graphed or self.calls <= self.warmup or self.capture_error is not None:
            return self._run()
        state = self.cache.host_state()
        try:
            side = torch.cuda.Stream(device=self.ids.device)
            side.wait_stream(torch.cuda.current_stream())
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                out = self._run()
            torch.cuda.current_stream().wait_stream(side)
        except Exception as e:  # a non-capturable op, a lazy library initialisation the warm-up did not reach, ...
            # nothing of the capture executed (the device-side position / key counts were not touched): the host
            # bookkeeping goes back, and the eager step, which works where the capture does not, runs from here on
            self.capture_error = e
            self.cache.restore_host_state(state)
            if isinstance(e, torch.cuda.OutOfMemoryError):
                raise
            warnings.warn(f"{self.what}: graph capture failed ({type(e).__name__}: {e}); every further {self.unit} runs as an "
                          f"eager sequence of launches (several times slower per {self.unit})", RuntimeWarning, stacklevel=3)
            torch.cuda.synchronize()
            return self._run()
        # the capture ran the host bookkeeping of one step and no kernel: this replay is that step
        self.graphs[key], self.outs[key] = graph, out
        graph.replay()
        self.replays += 1
        return out


class GraphedDecodeStep(_GraphedStep):
    """`step(token_ids)` -> next token ids — greedy, or drawn by `sampler` (llm/sampling.py: one launch of
    `kernels.sample_logits` in the place of the argmax, its draw indices in device memory) —, the same arithmetic as the
    eager loop.

    step_fn(ids) runs the language model on ONE token per sequence — ids is a (B, 1) int64 tensor that lives at a fixed
    address — against `cache` (already in static-decode mode; a `BranchSet` is one) and returns the logits of that token,
    (B, V) or (B, 1, V).  The first `warmup` calls run eagerly, the next one is captured, every later one replays; if the
    capture raises, the stepper keeps running the eager step (`capture_error` holds the reason)."""

    def __init__(self, step_fn: Callable[[torch.Tensor], torch.Tensor], cache, batch_size: int, device,
                 warmup: int = 2, sampler=None):
        if not getattr(cache, "static_decode", False):
            raise RuntimeError("GraphedDecodeStep: call cache.begin_static_decode(max_new_tokens) first")
        super().__init__(step_fn, cache, (batch_size, 1), device, warmup, graphed=True)
        self.sampler = sampler
        self.logits, self.next_ids = None, None

    @property
    def graph(self):
        return self.graphs.get(0)

    def _run(self):
        logits = self.step_fn(self.ids)
        logits = logits[:, -1] if logits.dim() == 3 else logits
        nxt = logits.argmax(-1) if self.sampler is None else self.sampler.sample(logits)
        self.cache.advance_static_device()
        return logits, nxt

    def _after_replay(self):
        self.cache.advance_static_host()

    @torch.inference_mode()
    def step(self, token_ids: torch.Tensor) -> torch.Tensor:
        if self.cache.static_room() < 1:
            raise RuntimeError("GraphedDecodeStep: the key / value buffers reserved by begin_static_decode are full")
        self.ids.copy_(token_ids.view(self.ids.shape))
        self.logits, self.next_ids = self._launch()
        return self.next_ids


class GraphedSpecStep(_GraphedStep):
    """One draft-and-verify step of speculative greedy decoding as ONE hipGraph launch.

    `step(t0, drafts)` feeds [t0, d1 .. dD] (T = D + 1 ids at a fixed address) through step_fn — a forward against
    `cache`, which is in speculation mode, returning the logits of the T positions, (1, T, V) — and computes on the device
    p = argmax, a = the number of leading drafts with d_i == p_i, k = a + 1, and `cache.commit(k)`.  It returns (k, p) to
    the host with one read.  The cache keeps two operand slots per Mamba layer and flips them every forward, so there are
    two graphs, one per slot parity: the first `warmup` calls run eagerly, the next two are captured, every later one
    replays the graph of its parity.  A failed capture falls back to the eager step for the rest of the generation
    (`capture_error` holds the reason; out of memory is raised)."""
    what, unit = "speculative decode", "step"

    def __init__(self, step_fn: Callable[[torch.Tensor], torch.Tensor], cache, n_tokens: int, device, warmup: int = 2,
                 graphed: bool = True):
        if not getattr(cache, "speculating", False):
            raise RuntimeError("GraphedSpecStep: call cache.begin_speculation(t_max, max_new_tokens) first")
        self.T = int(n_tokens)
        super().__init__(step_fn, cache, (1, self.T), device, warmup, graphed)

    def _run(self):
        logits = self.step_fn(self.ids)
        p = logits.reshape(self.T, -1).argmax(-1)                                   # (T,)
        k = self._accept(p)
        self.cache.commit(k)
        return torch.cat([k.reshape(1).to(torch.int64), p])

    def _accept(self, p):
        """k = 1 + the number of leading drafts that equal the model's own next token, on the device"""
        a = (self.ids[0, 1:] == p[:-1]).to(torch.int32).cumprod(0).sum()
        return (a + 1).to(torch.int32)

    def _key(self):
        return self.cache.spec_parity()

    def _before_replay(self):
        self.cache.spec_check(self.T)

    def _after_replay(self):
        self.cache.spec_replayed(self.T)

    @torch.inference_mode()
    def step(self, t0: int, drafts):
        """-> (k, [p1 .. pT]): k tokens of the forward are kept (t0 and k - 1 drafts), p1 .. pk are the tokens to emit."""
        host = torch.tensor([[int(t0)] + [int(d) for d in drafts]], dtype=torch.int64)
        if host.shape[1] != self.T:
            raise ValueError(f"GraphedSpecStep: {self.T - 1} drafts per step")
        self.ids.copy_(host)
        res = self._launch().tolist()
        k = res[0]
        self.cache.note_committed(k)
        return k, res[1:]
