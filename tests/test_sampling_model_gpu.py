"""Sampled decoding through `generate` / `generate_branches` on the GPU: the synthetic bf16 hybrid of
tests/test_speculative_gpu.py (head_dim 128, 16 new tokens: the decode step is captured), the sampler inside the graph.

There is deliberately no assertion that a sampled branch equals sampled `generate` on a clone: the B-row and 1-row linear
routes round differently in bf16, and a draw near a CDF boundary may then legitimately differ.  That equality is pinned on the
CPU (tests/test_sampling_cpu.py), where both sides run the same arithmetic."""
import pytest
import torch

from test_speculative_gpu import N_NEW, SEED_GRAPHED, _synthetic_vlm, spec_prompts

pytestmark = pytest.mark.gpu
DEV = "cuda"
HOT = 20.0          # undoes the lm_head x 20 spread: a distribution flat enough for seeds to matter
CASE = {}


def _case():
    """The model, its pixels, the prompt, the greedy ids and the cache that run left: computed once, never modified."""
    if not CASE:
        vlm = _synthetic_vlm(SEED_GRAPHED)
        pix = torch.randn(40, 3, 96, 96, generator=torch.Generator().manual_seed(SEED_GRAPHED)).to(DEV).bfloat16()
        ids = spec_prompts(vlm)["plain"]
        greedy, cache = vlm.generate(ids, pixel_values_videos=pix, max_new_tokens=N_NEW, return_ids=True, eos_token_id=-1,
                                     return_past_key_values=True)
        assert vlm.last_generate_stats["graphed"] is True
        CASE["case"] = (vlm, pix, ids, greedy, cache)
    return CASE["case"]


KW = dict(max_new_tokens=N_NEW, return_ids=True, eos_token_id=-1)


def test_top_k_1_is_greedy_inside_the_graph():
    vlm, pix, ids, greedy, _ = _case()
    got = vlm.generate(ids, pixel_values_videos=pix, do_sample=True, top_k=1, seed=5, **KW)
    st = vlm.last_generate_stats
    assert st["graphed"] is True and st["capture_error"] is None and st["emitted"] == N_NEW
    assert torch.equal(got, greedy), (got.tolist(), greedy.tolist())
    # temperature 0 is greedy decoding (no sampler, no seed needed)
    assert torch.equal(vlm.generate(ids, pixel_values_videos=pix, do_sample=True, temperature=0, **KW), greedy)


def test_same_seed_graphed_and_eager(monkeypatch):
    vlm, pix, ids, greedy, _ = _case()
    sk = dict(do_sample=True, temperature=HOT, top_k=50, top_p=0.95, seed=1234)
    graphed = vlm.generate(ids, pixel_values_videos=pix, **KW, **sk)
    assert vlm.last_generate_stats["graphed"] is True
    again = vlm.generate(ids, pixel_values_videos=pix, **KW, **sk)
    monkeypatch.setenv("TV_DECODE_GRAPH", "0")
    eager = vlm.generate(ids, pixel_values_videos=pix, **KW, **sk)
    assert vlm.last_generate_stats["graphed"] is False
    print("sampled:", graphed.tolist(), "greedy:", greedy.tolist())
    assert torch.equal(graphed, again) and torch.equal(graphed, eager), (graphed.tolist(), eager.tolist())
    assert not torch.equal(graphed, greedy)


def test_two_seeds_two_answers():
    vlm, _, _, _, cache = _case()
    q = torch.tensor([[12, 13, 14]], device=DEV)
    a, b = (vlm.generate(q, past_key_values=cache.clone(), do_sample=True, temperature=HOT, seed=s, **KW) for s in (1, 2))
    assert a.shape == b.shape == (1, N_NEW) and not torch.equal(a, b), a.tolist()
    c = vlm.generate(q, past_key_values=cache.clone(), do_sample=True, temperature=HOT, seed=1, sample_stream=1, **KW)
    assert not torch.equal(a, c)


def test_one_question_four_samples_for_one_prefill():
    vlm, _, _, _, cache = _case()
    q = torch.tensor([[12, 13, 14]], device=DEV)
    sk = dict(do_sample=True, temperature=HOT, top_p=0.98, seed=77)
    got = vlm.generate_branches([q] * 4, past_key_values=cache, **KW, **sk)
    st = vlm.last_generate_stats
    assert st["branched"] is True and st["graphed"] is True and st["branches"] == 4
    ans = [g[0].tolist() for g in got]
    print(ans)
    assert all(len(a) == N_NEW for a in ans) and len(set(map(tuple, ans))) > 1, ans
    again = vlm.generate_branches([q] * 4, past_key_values=cache, **KW, **sk)
    assert ans == [g[0].tolist() for g in again]
