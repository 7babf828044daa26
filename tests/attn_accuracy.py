"""Per-row judgement of an attention output against the fp32 oracle.

`close(o, o_ref, 2e-2, 1e-2)` has an absolute term; with q, k, v ~ randn and many keys the softmax averages V towards
zero, the output falls below that term and the check accepts almost anything (at 32 868 keys `o = o_ref / 2` passes on
98 % of the elements).  A relative error per OUTPUT ROW has no such floor:

    rowrel[b, q, h] = || o[b, q, h, :] - o_ref[b, q, h, :] ||_2 / || o_ref[b, q, h, :] ||_2          (fp64)

The bound is 2 eps of the I/O type (eps = 2^-8 for bf16, 2^-11 for fp16 — the values
test_flash_attention_streaming_row_sums_on_the_matrix_pipe uses):
  * rounding P to the I/O type perturbs each weight by at most eps / 2, independently per key;
  * one rounding of the output adds at most eps / 2 per element;
  * a CPU emulation of a correct kernel (fp32 scores, P rounded, fp32 accumulate, output rounded;
    tests/test_attn_accuracy_cpu.py) measures 0.77 eps for the sum of the two, at every shape and key count;
  * 2 eps leaves 2.6 x of headroom for what a real kernel adds (a split merge, exp2-based exponentials, P rounded
    relative to a lazy maximum) and stays 1.6 x below the smallest effect of a value-path mutation that the CPU test
    establishes (0.013: the last key dropped from an append at 3 000 keys).

A row whose reference is zero (no visible key: `attention_ref` returns zeros there) must be exactly zero."""
import torch

EPS = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}


def row_bound(dtype):
    return 2.0 * EPS[dtype]


def row_rel_err(o, o_ref):
    """One value per (batch, query, head) — the leading dimensions of `o`; fp64.  Rows with a zero reference: 0.0 if the
    output row is exactly zero, inf otherwise."""
    a, b = o.detach().double().cpu(), torch.as_tensor(o_ref).detach().double().cpu()
    assert a.shape == b.shape, (a.shape, b.shape)
    num, den = (a - b).norm(dim=-1), b.norm(dim=-1)
    rel = num / den.clamp_min(1e-300)
    zero = den == 0
    return torch.where(zero, torch.where(num == 0, torch.zeros_like(rel), torch.full_like(rel, float("inf"))), rel)


def assert_rows_close(o, o_ref, dtype, what="", bound=None):
    """Fails when any row's relative error exceeds `bound` (default: 2 eps of `dtype`) or is not finite; the message names
    the worst row.  Returns the largest row error (and prints it: the per-kernel table in DESIGN.md is read off a run)."""
    bound = row_bound(dtype) if bound is None else bound
    rel = row_rel_err(o, o_ref)
    rel = torch.where(torch.isnan(rel), torch.full_like(rel, float("inf")), rel)
    worst = int(rel.argmax())
    idx = tuple(int(i) for i in torch.unravel_index(torch.tensor(worst), rel.shape))
    mx = float(rel.flatten()[worst])
    print(f"rowrel {what}: max {mx:.3e} at (batch, query, head) {idx}, bound {bound:.3e}")
    assert mx <= bound, (f"{what}: row (batch, query, head) = {idx} has relative error {mx:.3e} > bound {bound:.3e} "
                         f"({int((rel > bound).sum())} of {rel.numel()} rows over the bound)")
    return mx
