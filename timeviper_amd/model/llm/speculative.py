"""Speculative greedy decoding: prompt-lookup drafts, verified by the model in one forward.

A decode token re-reads every weight for one row of output.  A draft-and-verify step feeds the last emitted token and D
drafted ones through ONE forward (a continuation of the hybrid cache in speculation mode), keeps the drafts the model's own
argmax agrees with and one more token — its correction, or its continuation when every draft was right.  Every emitted
token is the argmax of the model's logits: greedy output is unchanged by construction; what changes is how many weight
reads it costs.  The drafter needs no second model: it proposes what followed the most recent earlier occurrence of the
text's current tail (option letters, repeated phrases, quoted subtitles of a video QA prompt).
"""
from __future__ import annotations

from typing import Iterable, List, Sequence

__all__ = ["prompt_lookup_draft", "DEFAULT_DRAFTS"]

# `generate(speculative=True)`: the D with the lowest break-even acceptance a* in profiles/speculative_decode.json
# ("end_to_end" -> "best_drafts", written by devtools/bench_speculative.py): 2, at a* = 1.08 accepted drafts per step on
# an MI355X at 9B dims behind a 32 868-token cache (D = 1: a* = 1.06 > D, it can never pay; 3 / 4 / 8: 1.10 / 1.13 / 1.28).
DEFAULT_DRAFTS = 2


def prompt_lookup_draft(ids: Sequence[int], n_draft: int, ngram_max: int = 3, ngram_min: int = 1,
                        exclude_ids: Iterable[int] = ()) -> List[int]:
    """The longest suffix of `ids` (ngram_max down to ngram_min tokens) that also occurs earlier: the up to `n_draft` ids
    that followed its MOST RECENT earlier occurrence; [] if there is none.  Ids in `exclude_ids` (image placeholders) are
    never proposed: the continuation stops in front of the first one."""
    ids = list(ids)
    n = len(ids)
    if n_draft < 1:
        return []
    exclude = set(int(t) for t in exclude_ids)
    for g in range(min(int(ngram_max), n - 1), max(int(ngram_min), 1) - 1, -1):
        tail = ids[n - g:]
        for start in range(n - g - 1, -1, -1):                 # the most recent occurrence first
            if ids[start:start + g] == tail:
                out = []
                for t in ids[start + g:start + g + n_draft]:
                    if t in exclude:
                        break
                    out.append(int(t))
                if out:
                    return out
    return []
