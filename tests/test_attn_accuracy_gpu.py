"""The value path of every attention kernel on inputs whose answer is known in closed form — what the row metric on random
data does not pin down: WHICH V rows are read and for WHICH (query, head).

  * key identity    k = 0: every visible key weighs the same, v[j] is a signature of its key index that the I/O types
                    hold exactly; the output is the plain mean of V over the visible keys (fp64).  P is exactly 1 and the
                    fp32 sums of multiples of 1/128 are exact, so a correct kernel differs by one output rounding; a
                    wrong, duplicated or missing row shifts the mean.
  * one hot key     each (batch, query, head) has its own key j whose score beats the rest by > 17 (weight of all others
                    together < 1e-5): the output is v[j].  j sits on the first key, on the last visible key and on both
                    sides of every multiple of 32 (the split-KV kernel's 32-key steps and its splits, which are multiples
                    of 32; the prefill and ViT kernels' 96-key tiles).  GQA head mapping and bottom-right causal alignment
                    on the value side.
  * scale           v and v * 2^-6 give the same bits after rescaling: no absolute threshold or flush in the value path.

All judged with the 2 eps row bound of tests/attn_accuracy.py."""
import pytest
import torch

from attn_accuracy import assert_rows_close

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def K():
    from timeviper_amd import kernels
    return kernels


def visible_last(Lq, Lk, causal):
    """Index of the last key each query sees (bottom-right aligned causal mask)."""
    return torch.arange(Lq) + (Lk - Lq) if causal else torch.full((Lq,), Lk - 1)


# ------------------------------------------------------------------ key identity
def identity_case(B, Lq, Lk, Hq, Hkv, D, causal, dtype):
    g = torch.Generator().manual_seed(Lq * 7 + Lk + D)
    q = torch.randn(B, Lq, Hq, D, generator=g).to(dtype)
    k = torch.zeros(B, Lk, Hkv, D, dtype=dtype)
    j, h, d = torch.arange(Lk)[:, None, None], torch.arange(Hkv)[None, :, None], torch.arange(D)[None, None, :]
    sig = ((j * 131 + d * 17 + h * 29) % 251 - 125).double() / 128          # |.| <= 125 / 128: 8 significant bits
    v = sig[None].expand(B, Lk, Hkv, D).to(dtype)
    assert torch.equal(v.double(), sig[None].expand(B, Lk, Hkv, D))          # exact in the I/O type
    csum = torch.cumsum(sig, dim=0)                                          # (Lk, Hkv, D) fp64, exact
    last = visible_last(Lq, Lk, causal)
    mean = csum[last] / (last + 1)[:, None, None].double()                   # (Lq, Hkv, D)
    o_ref = mean.repeat_interleave(Hq // Hkv, dim=1)[None].expand(B, Lq, Hq, D)
    return q.to(DEV), k.to(DEV), v.to(DEV), o_ref


@pytest.mark.parametrize("Lk", [256, 257, 1000])
def test_key_identity_decode(K, Lk):
    q, k, v, o_ref = identity_case(2, 1, Lk, 32, 8, 128, True, torch.bfloat16)
    assert_rows_close(K.flash_attn_decode(q, k, v), o_ref, torch.bfloat16, f"decode identity Lk {Lk}")


@pytest.mark.parametrize("Lk", [37, 963, 1027])
@pytest.mark.parametrize("T", [2, 8])
def test_key_identity_append(K, T, Lk):
    q, k, v, o_ref = identity_case(1, T, Lk, 32, 8, 128, True, torch.bfloat16)
    calls = K.flash_attn_append_calls()
    o = K.flash_attn_append(q, k, v)
    assert K.flash_attn_append_calls() == calls + 1, "fell back to the prefill kernel"
    assert_rows_close(o, o_ref, torch.bfloat16, f"append identity T {T} Lk {Lk}")


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("L", [129, 300])
def test_key_identity_prefill(K, L, causal, dtype):
    q, k, v, o_ref = identity_case(2, L, L, 4, 2, 128, causal, dtype)
    assert_rows_close(K.flash_attn_func(q, k, v, causal=causal), o_ref, dtype, f"prefill identity L {L} causal {causal}")


# The streaming ViT kernels take a call only with >= 64 (batch, head) pairs and more query blocks per XCD than an eighth
# of the CUs (csrc/attention.hip launch_fa_d): 9 x 16 = 144 pairs x 2 query blocks = 36 per XCD.  A (2, 300, 300, 2 heads)
# batch runs on the prefill kernel whatever the variant: that is the second shape, which gives that kernel its head_dim
# 72 / 80 cases.
@pytest.mark.parametrize("variant", [3, 4, 5])
@pytest.mark.parametrize("B,Hq,Hkv,D", [(9, 16, 16, 72), (9, 16, 8, 80), (2, 2, 2, 72), (2, 2, 2, 80)])
def test_key_identity_vit_variants(K, B, Hq, Hkv, D, variant):
    q, k, v, o_ref = identity_case(B, 300, 300, Hq, Hkv, D, False, torch.bfloat16)
    K.flash_attn_set_variant(variant)
    try:
        o = K.flash_attn_func(q, k, v, causal=False)
    finally:
        K.flash_attn_set_variant(0)
    assert_rows_close(o, o_ref, torch.bfloat16, f"ViT variant {variant} identity B {B} H {Hq}/{Hkv} d {D}")


# ------------------------------------------------------------------ one hot key per query
def one_hot_case(B, Lq, Lk, Hq, Hkv, D, causal, dtype):
    """Keys are random sign vectors, q[b, i, h] = 4 k[b, j, h's kv-head] for its own key j = hot[b, i, h]: the hot score is
    4 sqrt(D) (>= 33.9), the others 4 N(0, 1) (the largest of a few thousand: < 4 x 4.2).  Returns the expected v[j]."""
    g = torch.Generator().manual_seed(Lq * 11 + Lk + D)
    rep = Hq // Hkv
    k = (torch.randint(0, 2, (B, Lk, Hkv, D), generator=g) * 2 - 1).to(dtype)
    v = torch.randn(B, Lk, Hkv, D, generator=g).to(dtype)
    last = visible_last(Lq, Lk, causal)
    cands = [0, -1] + [p for m in range(32, Lk, 32) for p in (m - 1, m)]           # -1: the last visible key
    hot = torch.empty(B, Lq, Hq, dtype=torch.long)
    r = 0
    for b in range(B):
        for i in range(Lq):
            vis = int(last[i])
            for h in range(Hq):
                # (causal, several tokens: one head of every token, another one each, takes its last visible key)
                c = -1 if (causal and Lq > 1 and h == i % Hq) else cands[r % len(cands)]
                hot[b, i, h] = vis if (c < 0 or c > vis) else c
                r += 1
    bi = torch.arange(B)[:, None, None].expand(B, Lq, Hq)
    hk = (torch.arange(Hq) // rep)[None, None, :].expand(B, Lq, Hq)
    q = (k[bi, hot, hk].float() * 4.0).to(dtype)
    o_ref = v[bi, hot, hk].double()
    return q.to(DEV), k.to(DEV), v.to(DEV), o_ref, hot


def test_one_hot_key_decode(K):
    # 2 x 32 rows: first key, last key and both sides of 31 step boundaries (the splits of 1 000 keys begin on some of them)
    q, k, v, o_ref, hot = one_hot_case(2, 1, 1000, 32, 8, 128, True, torch.bfloat16)
    assert len(set(hot.flatten().tolist())) == 64
    assert_rows_close(K.flash_attn_decode(q, k, v), o_ref, torch.bfloat16, "decode one-hot Lk 1000")


@pytest.mark.parametrize("T,Lk,Hq,Hkv", [(8, 963, 32, 8), (8, 1027, 32, 8), (5, 37, 12, 4), (3, 2500, 40, 2)])
def test_one_hot_key_append(K, T, Lk, Hq, Hkv):
    q, k, v, o_ref, hot = one_hot_case(1, T, Lk, Hq, Hkv, 128, True, torch.bfloat16)
    last = visible_last(T, Lk, True)
    assert all((hot[0, i] == last[i]).any() for i in range(T)), "every token has a head on its last visible key"
    calls = K.flash_attn_append_calls()
    o = K.flash_attn_append(q, k, v)
    assert K.flash_attn_append_calls() == calls + 1, "fell back to the prefill kernel"
    assert_rows_close(o, o_ref, torch.bfloat16, f"append one-hot T {T} Lk {Lk} H {Hq}/{Hkv}")


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("B,Lq,Lk,Hq,Hkv,D,causal", [
    (1, 300, 300, 4, 2, 128, True),
    (1, 50, 180, 8, 2, 128, True),       # bottom-right aligned: query i sees the keys <= i + 130
    (1, 129, 129, 5, 1, 64, True),       # five q-heads on one kv-head
    (1, 100, 333, 8, 2, 128, False),
    (2, 300, 300, 2, 2, 72, False),
    (1, 130, 200, 6, 3, 96, False),
])
def test_one_hot_key_prefill(K, B, Lq, Lk, Hq, Hkv, D, causal, dtype):
    q, k, v, o_ref, _ = one_hot_case(B, Lq, Lk, Hq, Hkv, D, causal, dtype)
    o = K.flash_attn_func(q, k, v, causal=causal)
    assert_rows_close(o, o_ref, dtype, f"prefill one-hot {Lq}x{Lk} H {Hq}/{Hkv} d {D} causal {causal}")


@pytest.mark.parametrize("variant", [3, 4, 5])
@pytest.mark.parametrize("B,Hq,Hkv,D", [(9, 16, 16, 72), (9, 16, 8, 80)])
def test_one_hot_key_vit_variants(K, B, Hq, Hkv, D, variant):
    q, k, v, o_ref, _ = one_hot_case(B, 300, 300, Hq, Hkv, D, False, torch.bfloat16)
    K.flash_attn_set_variant(variant)
    try:
        o = K.flash_attn_func(q, k, v, causal=False)
    finally:
        K.flash_attn_set_variant(0)
    assert_rows_close(o, o_ref, torch.bfloat16, f"ViT variant {variant} one-hot B {B} H {Hq}/{Hkv} d {D}")


# ------------------------------------------------------------------ scale invariance
def test_decode_value_scale_invariance(K):
    """Scaling V by a power of two is exact in bf16 and in every fp32 product and sum of the value path: same bits."""
    g = torch.Generator().manual_seed(1)
    q = torch.randn(1, 1, 32, 128, generator=g).bfloat16().to(DEV)
    k = torch.randn(1, 5000, 8, 128, generator=g).bfloat16().to(DEV)
    v = torch.randn(1, 5000, 8, 128, generator=g).bfloat16().to(DEV)
    vs = v * 2.0 ** -6
    assert torch.equal(vs.float() * 64, v.float())
    o = K.flash_attn_decode(q, k, v)
    os_ = K.flash_attn_decode(q, k, vs)
    assert torch.equal(os_.float() * 64, o.float()), (os_.float() * 64 - o.float()).abs().max().item()
