"""tv_sample_logits_fwd on the GPU against the contract in numpy (tests/sampling_ref.py): the random word bit for bit, the
kept set (count and threshold) exactly, the returned id inside the CDF interval the random word falls in.

Inputs: `torch.manual_seed(seed); z = (torch.randn(V) * sigma).bfloat16().float()` — bf16 values widened to fp32, ~2 800
distinct values among 131 072 entries, so exact ties are everywhere and every rule is a value threshold.  The kept set may be
compared exactly because the reference's own top-p margin (how far, relative to the kept mass, its decision is from flipping)
is asserted to be >= 1e-4 for every case, while the kernel's masses are off by at most the device exp's 2 ulp plus
V * 2^-40 (the integer truncation), ~5e-7 relative: a 200-fold margin.  The id check allows eps = 2e-6 on the CDF (that
bound with a factor 4 for the device exp).  Every launch is one work-group per row, well under a second."""
import functools

import numpy as np
import pytest
import torch

import sampling_ref as SR

pytestmark = pytest.mark.gpu

CASES = [(64, 1.0, (0, 1, 2)), (1001, 3.0, (0, 1)), (131072, 3.0, (0, 1, 2)), (152064, 3.0, (0, 1, 2))]
INPUTS = [(V, sigma, seed) for V, sigma, seeds in CASES for seed in seeds]
PARAMS = [(1.0, 0, 0.9), (0.7, 50, 0.95), (1.3, 0, 0.5), (1.0, 40, 1.0), (1.0, 0, 1.0), (1.0, 1, 1.0)]
DRAWS = [0, 1, 2 ** 32 + 5]
SEED = 0x1234567890ABCDEF
MARGIN, EPS = 1e-4, 2e-6


@functools.lru_cache(maxsize=None)
def _row(V, sigma, seed):
    torch.manual_seed(seed)
    return (torch.randn(V) * sigma).bfloat16().float()


@functools.lru_cache(maxsize=None)
def _ref(V, sigma, seed, params):
    """computed once per (input, parameters), shared (a rolled row keeps the same values: the same kept set)"""
    r = SR.reference(_row(V, sigma, seed).numpy(), *params)
    return {k: r[k] for k in ("n_kept", "t_bits", "margin", "t")}


def _launch(logits, draws, streams, params, seed=SEED):
    from timeviper_amd import kernels as K
    B = logits.shape[0]
    d = torch.tensor(draws, dtype=torch.int64, device="cuda")
    s = torch.tensor(streams, dtype=torch.int32, device="cuda")
    diag = torch.full((B, 4), -1, dtype=torch.int32, device="cuda")
    ids = K.sample_logits(logits, d, s, seed, temperature=params[0], top_k=params[1], top_p=params[2], diag=diag)
    torch.cuda.synchronize()
    return ids.cpu().tolist(), (diag.cpu().numpy().astype(np.int64) & 0xFFFFFFFF).tolist()


def _check_row(z, want, params, draw, stream, got_id, got_diag, seed=SEED):
    """checks 1-3 of one row: z the row as launched (numpy), want = _ref(...) of its values"""
    n_kept, t_bits, u, zero = got_diag
    assert u == SR.random_word(seed, draw, stream) and zero == 0
    assert want["margin"] >= MARGIN, want["margin"]                     # the comparison below is exact only then
    print(f"V={z.shape[0]} params={params} kept={n_kept}/{want['n_kept']} margin={want['margin']:.3g}")
    assert (n_kept, t_bits) == (want["n_kept"], want["t_bits"])
    assert 0 <= got_id < z.shape[0]
    r = SR.reference(z, *params)
    assert r["keep"][got_id], "the returned id is not in the reference's kept set"
    F = SR.cdf(r)
    lo = F[got_id - 1] if got_id > 0 else 0.0
    x = u / 2.0 ** 32
    print(f"   id={got_id} F_(i-1)={lo:.9f} x={x:.9f} F_i={F[got_id]:.9f}")
    assert lo - EPS <= x <= F[got_id] + EPS


@pytest.mark.parametrize("pi", range(len(PARAMS)))
@pytest.mark.parametrize("V, sigma, seed", INPUTS)
def test_one_row_against_the_contract(V, sigma, seed, pi):
    params = PARAMS[pi]
    z = _row(V, sigma, seed)
    draw = DRAWS[(seed + pi) % 3]
    logits = z.cuda().view(1, V)
    ids, diag = _launch(logits, [draw], [0], params)
    _check_row(z.numpy(), _ref(V, sigma, seed, params), params, draw, 0, ids[0], diag[0])
    if params == (1.0, 1, 1.0):
        assert ids[0] == int(z.argmax()) and diag[0][0] == 1
    if params == (1.0, 40, 1.0) and V > 64:
        assert diag[0][0] >= 40                                          # ties at the 40th largest value are all kept
    # a second launch: bit for bit the same
    assert _launch(logits, [draw], [0], params) == (ids, diag)


def _batch(V, sigma, n_seeds, B):
    """B distinct rows: row b is the input of seed b % n_seeds rolled by b (the same values: the margins carry over)"""
    return torch.stack([_row(V, sigma, b % n_seeds).roll(b) for b in range(B)])


@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("B", [3, 16])
@pytest.mark.parametrize("V, sigma, n_seeds", [(1001, 3.0, 2), (131072, 3.0, 3), (152064, 3.0, 3)])
def test_rows_of_a_batch(V, sigma, n_seeds, B, strided):
    rows = _batch(V, sigma, n_seeds, B)
    if strided:                                                          # the view the model hands over: logits3d[:, -1]
        logits3d = torch.zeros(B, 2, V)
        logits3d[:, -1] = rows
        logits = logits3d.cuda()[:, -1]
        assert logits.stride(0) == 2 * V
    else:
        logits = rows.cuda()                                             # V = 1001: rows 1.. are not 16-byte aligned
    draws = [DRAWS[b % 3] for b in range(B)]
    streams = list(range(B))
    for params in (PARAMS[1], PARAMS[0]):
        ids, diag = _launch(logits, draws, streams, params)
        for b in range(B):
            _check_row(rows[b].numpy(), _ref(V, sigma, b % n_seeds, params), params, draws[b], b, ids[b], diag[b])
        assert _launch(logits, draws, streams, params) == (ids, diag)
        # row b does not depend on the other rows or on B
        for b in sorted({0, 1, B - 1}):
            one = _launch(rows[b:b + 1].cuda(), [draws[b]], [b], params)
            assert (one[0][0], one[1][0]) == (ids[b], diag[b]), b


def test_streams_and_draws_give_different_words_and_out_is_written_in_place():
    from timeviper_amd import kernels as K
    V = 1001
    logits = _row(V, 3.0, 0).cuda().view(1, V).expand(8, V)             # row stride 0: one row, eight draws
    assert logits.stride(0) == 0
    d = torch.tensor([0, 0, 1, 1, 2, 2, 3, 3], dtype=torch.int64, device="cuda")
    s = torch.tensor([0, 1, 0, 1, 0, 1, 0, 1], dtype=torch.int32, device="cuda")
    out = torch.full((8,), -1, dtype=torch.int64, device="cuda")
    diag = torch.zeros((8, 4), dtype=torch.int32, device="cuda")
    res = K.sample_logits(logits, d, s, 7, temperature=1.0, out=out, diag=diag)
    assert res.data_ptr() == out.data_ptr()
    words = (diag[:, 2].cpu().numpy().astype(np.int64) & 0xFFFFFFFF).tolist()
    assert words == [SR.random_word(7, int(a), int(b)) for a, b in zip(d.tolist(), s.tolist())] and len(set(words)) == 8
    F = SR.cdf(SR.reference(_row(V, 3.0, 0).numpy()))
    for i, w in zip(out.tolist(), words):
        assert 0 <= i < V and (F[i - 1] if i else 0.0) - EPS <= w / 2.0 ** 32 <= F[i] + EPS
    assert len(set(out.tolist())) > 1


@pytest.mark.parametrize("params", [PARAMS[1], PARAMS[4]])
def test_a_row_with_a_nan_still_gives_a_valid_id(params):
    V = 1001
    z = _row(V, 3.0, 1).clone()
    z[17] = float("nan")
    ids, _ = _launch(z.cuda().view(1, V), [3], [0], params)
    assert 0 <= ids[0] < V and ids[0] != 17
    allnan = torch.full((1, V), float("nan"), device="cuda")
    ids, _ = _launch(allnan, [3], [0], params)
    assert 0 <= ids[0] < V
    inf = _row(V, 3.0, 1).clone()
    inf[5] = float("inf")
    ids, _ = _launch(inf.cuda().view(1, V), [3], [0], params)
    assert 0 <= ids[0] < V
