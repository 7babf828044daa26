// T3 (decode and continuation): a FEW query tokens per sequence against a long K / V cache, as one split-KV walk with two
// instantiations:
//   tv_attn_decode_fwd   ONE query token — the attention of a generate() step (modeling_nano.py:1198-1209 with q_len == 1;
//                        the cache layout of HybridMambaAttentionDynamicCache, :205-360);
//   tv_attn_append_fwd   the LAST T tokens of a sequence — the attention of a forward that continues a prefilled cache with
//                        a few tokens (a follow-up question, a tool result, a draft to verify).
//
// The prefill kernel (attention.hip) gives a (batch, q-head) pair to one work-group: with one query row that is
// Hq work-groups walking the whole cache one after the other (32 for Nemotron-Nano-9B: 1/8 of the chip, each streaming
// 32 868 keys serially, the four q-heads of a kv-head each fetching the same K / V).  Here the work is cut the other way:
//   * the q-heads that share a kv-head are the N columns of an MFMA tile, in blocks of 16 (`hblocks`): K and V are read
//     once per kv-head and column block;
//   * the keys are split over `nsplit` work-groups per kv-head and block (grid = nsplit x Hkv * hblocks x batch, >= one per
//     CU), each wave of a work-group walks every AD_NW-th 32-key step of its range, AD_NS - 1 steps of copies in flight;
//   * a second, tiny kernel merges the per-split (max, sum, O) partials (log-sum-exp combine).
// The key count can come from DEVICE memory (`seqlens_k`): a decode step captured in a hipGraph replays with a
// growing cache without re-capture — the grid is sized for the capacity, the ranges are cut in the kernel.
//
// Per 32-key step of a wave (v_mfma_f32_16x16x32_bf16, everything on the matrix pipe):
//   S^T[key][head] = K . Q^T     A = K rows (ds_read_b128 of the wave's 32 x 256-byte K tile), B = Q^T fragments held for
//                                the whole kernel;  2 tiles x 4 k-steps
//   online softmax               a lane owns one head (n = lane % 16) and 8 keys; running max per head, agreed between
//                                the 4 lanes of a head with two v_permlane swaps
//   O^T[d][head] += V^T . P      A = V^T: the V tile read with the transposing ds_read_b64_tr_b16; B = P, which the S^T accumulators are after a bf16 pack — the key
//                                order of the two S^T tiles is chosen so that no lane exchange is needed
// K and V tiles arrive by LDS-DMA (global_load_lds_dwordx4, 16 bytes a lane, no register round trip) into a ring of
// AD_NS stages PRIVATE to the wave, AD_NS - 1 steps ahead of the math behind counted vmcnt waits: no barrier in the
// loop; one at the end for the merge of the waves.  (K fragments as plain 16-byte global loads into registers would be
// the natural A operand, but a register ring filled by asynchronous loads does not survive the compiler: the copies it
// places on the loop's back edge read registers whose loads are still in flight.)
//
// What the continuation adds (APPEND; the decode instantiation contains none of it): the columns of a kv-head are its
// T * gq (token c / gq, head c % gq) pairs instead of its heads alone, with a token stride on Q, O and the partial slots.
// Query token i sees the keys < Lk - T + 1 + i (bottom-right causal): a per-column bound on the key index, which bites in
// the last step(s) of the last split only.  A column can therefore see NO key in a step, a wave or a split (T = Lk: token
// 0 sees key 0 alone): running maxima of -inf are kept out of the exponents, and a result is empty where its sum is 0.
// With one token every step holds a key of the range and wave 0 always has a step: the maxima are finite.
#include "ssd_common.hpp"

namespace {
using namespace ssdk;

#ifndef AD_NW
#define AD_NW 3                               // waves per work-group
#endif
#ifndef AD_NS
#define AD_NS 3                               // ring stages per wave (a stage: the K and the V tile of one step)
#endif
constexpr int AD_STEP = 32;                   // keys per wave step
constexpr int AD_D = 128;                     // head_dim of this kernel
constexpr int AD_ROWB = AD_D * 2;             // bytes of a K / V row in LDS
constexpr int AD_TILE = AD_STEP * AD_ROWB;    // 8 KiB
constexpr int AD_STAGE = 2 * AD_TILE;         // K tile, V tile
constexpr int AD_RING = AD_NW * AD_NS * AD_STAGE;                 // 144 KiB
constexpr int AD_MERGE = AD_NW * 32 * 64 * 4 + 2 * AD_NW * 64 * 4;     // [wave][ct * 4 + i][lane] fp32 O, [wave][lane] max, sum:
constexpr int AD_LDS = AD_RING > AD_MERGE ? AD_RING : AD_MERGE;        // written over the ring once the walk is over
constexpr int AD_OPS = 16;                    // copy instructions per step and wave
constexpr int AD_MAX_SPLIT = 256;
constexpr size_t AD_SLOT_BYTES = (AD_D + 2) * sizeof(float);      // workspace of a (column, split): fp32 O, max, sum
constexpr int AP_MAX_T = 64, AP_MAX_COLS = 128;      // continuation: T <= 64 query tokens, T * gq <= 128 columns

struct DecArgs {
  const bf16_t *q, *k, *v;
  bf16_t* o;
  float *lse, *part_o, *part_ml;
  const int* seqlens;                         // device, one per batch entry; nullptr: Lk for all
  int Lk, Hq, Hkv, gq, hblocks, nsplit, T, ncols;          // hblocks: blocks of 16 of the T * gq columns of a kv-head
  int64_t qsl, osl, qsb, qsh, ksb, ksl, ksh, vsb, vsl, vsh, osb, osh;       // (decode: T = 1, the token strides unused)
  float scale_log2;
};

// keys of a sequence and the keys per split (a multiple of the step), the same in both kernels
__device__ __forceinline__ void split_of(const DecArgs& a, int b, int& Lk, int& chunk) {
  Lk = a.seqlens ? min(max(a.seqlens[b], 0), a.Lk) : a.Lk;
  chunk = ((Lk + a.nsplit - 1) / a.nsplit + AD_STEP - 1) / AD_STEP * AD_STEP;
  if (chunk == 0) chunk = AD_STEP;
}

// first of the `nsplit` partial slots of a (batch entry, token, q-head)
template <bool APPEND>
__device__ __forceinline__ int64_t slot_of(const DecArgs& a, int b, int tok, int head) {
  return ((APPEND ? (int64_t)b * a.T + tok : (int64_t)b) * a.Hq + head) * a.nsplit;
}

template <bool APPEND>
__global__ __launch_bounds__(AD_NW * 64) void attn_splitkv_kernel(DecArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char ad_smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n = lane & 15, g = lane >> 4;                 // MFMA column (q-head / key row / d column) and k-quarter
  const int split = blockIdx.x, b = blockIdx.z;
  const int hk = blockIdx.y / a.hblocks, hb = blockIdx.y % a.hblocks;
  const int nh = min(16, (APPEND ? a.ncols : a.gq) - 16 * hb);        // columns of this block
  const int col = 16 * hb + min(n, nh - 1);               // this lane's column of the kv-head: (token, head)
  const int tok = APPEND ? col / a.gq : 0, head = hk * a.gq + (APPEND ? col % a.gq : col);
  int Lk, chunk;
  split_of(a, b, Lk, chunk);
  const int r0 = split * chunk, r1 = min(Lk, r0 + chunk);
  if (r0 >= r1) return;                                   // (the merge kernel skips the same splits)
  const int nsteps = (r1 - r0 + AD_STEP - 1) / AD_STEP;
  const int lim = APPEND ? Lk - a.T + tok - r0 : 0;       // APPEND: last key this lane's column sees, relative to r0
  const int nst = nsteps > wave ? (nsteps - wave + AD_NW - 1) / AD_NW : 0;      // steps wave, wave + AD_NW, ...

  const unsigned lds0 = lds_addr_of(ad_smem);
  const unsigned ring = lds0 + (unsigned)(wave * AD_NS * AD_STAGE);

  // ---- Q^T fragments (B operand): lane (n, g) holds Q[column n][32 ks + 8 g .. + 7]; columns past the block are zeros
  bf16x8 qf[4];
  {
    const bf16_t* qp = a.q + (int64_t)b * a.qsb + (APPEND ? (int64_t)tok * a.qsl : 0) + (int64_t)head * a.qsh + 8 * g;
    u32x4 raw[4];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) raw[ks] = gload16_async(qp + 32 * ks);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      settle(raw[ks]);
      const bf16x8 z = {};
      qf[ks] = n < nh ? __builtin_bit_cast(bf16x8, raw[ks]) : z;
    }
  }

  // ---- K rows (A operand of S^T): tile G row m = key kb + 8 (m >> 2) + 4 G + (m & 3), so that the accumulator rows
  // 4 g + i of tiles 0 / 1 are keys kb + 8 g + i and kb + 8 g + 4 + i: slots 0..7 of P's fragment for k-quarter g
  const bf16_t* kg = a.k + (int64_t)b * a.ksb + (int64_t)hk * a.ksh + (int64_t)r0 * a.ksl;
  const bf16_t* vg = a.v + (int64_t)b * a.vsb + (int64_t)hk * a.vsh + (int64_t)r0 * a.vsl;
  const int last = r1 - 1 - r0;                            // last key of the range, relative to r0
  // ---- copies: instruction i8 of a tile, lane l -> row 4 i8 + (l >> 4), physical 16-byte chunk l & 15, holding logical
  // chunk (l & 15) ^ f(row):  K: f = (row & 3) | ((row >> 1) & 12) (distinct over the 16 rows {0..3, 8..11, 16..19, 24..27} (+ 4)
  // that the 16 lanes of a ds_read_b128 group touch);
  // V: f = 2 ((row & 3) | ((row >> 1) & 4)) (the 32 lanes of one half of a transposing read — rows 8 kq + q4, kq in a
  // pair, 8-byte pieces p4 of the 32 bytes of d-tile ct — touch every bank once)
  const int crow = lane >> 4;
  const unsigned vchunk = (unsigned)((lane & 15) ^ (2 * (lane >> 4)));

  auto issue = [&](int i, int S) __attribute__((always_inline)) {
    const int kb = AD_STEP * (wave + AD_NW * i);           // relative to r0; rows past the range repeat its last key
    const void* kbp = uniform_ptr(kg);
    const void* vbp = uniform_ptr(vg);
    const unsigned dst = ring + (unsigned)(S * AD_STAGE);
#pragma unroll
    for (int i8 = 0; i8 < 8; ++i8) {
      const int row = 4 * i8 + crow, key = min(kb + row, last);
      const unsigned ch = (unsigned)((lane & 15) ^ ((row & 3) | ((row >> 1) & 12)));
      glds16(kbp, (unsigned)key * (unsigned)(a.ksl * 2) + ch * 16u, dst + (unsigned)(i8 * 1024));
    }
#pragma unroll
    for (int i8 = 0; i8 < 8; ++i8) {
      const int key = min(kb + 4 * i8 + crow, last);
      const unsigned ch = vchunk ^ (unsigned)(8 * ((i8 >> 1) & 1));
      glds16(vbp, (unsigned)key * (unsigned)(a.vsl * 2) + ch * 16u, dst + (unsigned)(AD_TILE + i8 * 1024));
    }
  };
  // K fragment reads: lane (m = n, kq = g), tile G, k-step ks: row 8 (m >> 2) + 4 G + (m & 3), logical chunk 4 ks + kq
  const int krow = 8 * (n >> 2) + (n & 3);
  unsigned k_rd[2];
#pragma unroll
  for (int G = 0; G < 2; ++G) {
    const int row = krow + 4 * G;
    k_rd[G] = (unsigned)(row * AD_ROWB + ((g ^ ((row & 3) | ((row >> 1) & 12))) << 4));
  }

  // transposing reads: lane (lc = n, kq = g) gets keys 8 kq + 0..7 of d column 16 ct + lc (two reads: rows 8 kq + q4 and + 4)
  const int q4 = n >> 2, p4 = n & 3;
  const unsigned tr_base = (unsigned)((8 * g + q4) * AD_ROWB + 16 * (p4 >> 1) + 8 * (p4 & 1)) | (unsigned)((q4 | (4 * (g & 1))) << 5);

  f32x4 oacc[8];
#pragma unroll
  for (int ct = 0; ct < 8; ++ct) oacc[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m_run = -INFINITY, l_run = 0.f;

  typedef __attribute__((address_space(3))) const bf16x8 lds_bf16x8;
  auto compute = [&](int i, int S) __attribute__((always_inline)) {
    const int kb = AD_STEP * (wave + AD_NW * i);
    asm volatile("s_waitcnt vmcnt(%0)" :: "n"(AD_OPS * (AD_NS - 1)) : "memory");     // the younger steps stay in flight
    const unsigned stage = ring + (unsigned)(S * AD_STAGE);
    f32x4 sacc[2];
#pragma unroll
    for (int G = 0; G < 2; ++G) {
      sacc[G] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        // (4 ks + g) ^ f = 4 ks ^ (g ^ f) for f < 16: the k-step flips bits 2..3 of the physical chunk
        const bf16x8 kf = *(lds_bf16x8*)(size_t)(stage + (k_rd[G] ^ (unsigned)(ks << 6)));
        sacc[G] = mfma16(kf, qf[ks], sacc[G]);
      }
    }
    float tmax = -INFINITY;
#pragma unroll
    for (int G = 0; G < 2; ++G)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bool ok = kb + 8 * g + 4 * G + j <= (APPEND ? min(last, lim) : last);
        sacc[G][j] = ok ? sacc[G][j] * a.scale_log2 : -INFINITY;
        tmax = fmaxf(tmax, sacc[G][j]);
      }
    tmax = xor32_max(xor16_max(tmax));
    const float m_new = fmaxf(m_run, tmax);                // APPEND: -inf while the column has seen no key
    const float m_ref = APPEND && m_new == -INFINITY ? 0.f : m_new;
    const float alpha = __builtin_amdgcn_exp2f(m_run - m_ref);
    float ps = 0.f;
    bf16x8 pf;
#pragma unroll
    for (int G = 0; G < 2; ++G)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float p = __builtin_amdgcn_exp2f(sacc[G][j] - m_ref);
        ps += p;
        pf[4 * G + j] = from_f32<bf16_t>(p);
      }
    l_run = l_run * alpha + ps;
    if (__builtin_amdgcn_ballot_w64(m_new > m_run)) {
#pragma unroll
      for (int ct = 0; ct < 8; ++ct) oacc[ct] *= alpha;
    }
    m_run = m_new;
    const unsigned st = stage + (unsigned)AD_TILE;
#pragma unroll
    for (int ct = 0; ct < 8; ++ct) {
      const unsigned p = st + (tr_base ^ (unsigned)(ct << 5));
      const bf16x8 vf = cat4(__builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_v4*)(size_t)p),
                             __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_v4*)(size_t)(p + 4 * AD_ROWB)));
      oacc[ct] = mfma16(vf, pf, oacc[ct]);
    }
  };

  {
#pragma unroll
    for (int j = 0; j < AD_NS - 1; ++j) issue(j, j);
    int S = 0;                                             // ring stage of step i
    for (int i = 0; i < nst; ++i) {
      const int Sn = S == 0 ? AD_NS - 1 : S - 1;           // (S + AD_NS - 1) % AD_NS: the stage step i - 1 has left
      issue(i + AD_NS - 1, Sn);
      compute(i, S);
      S = S == AD_NS - 1 ? 0 : S + 1;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // (copies of steps past the range)
  }

  // ---- merge the waves: [wave][ct * 4 + i][lane] partial O, per-lane max / sum (sum over the head's 4 lanes first);
  // the arrays lie over the ring, which every wave has left
  l_run = xor32_sum(xor16_sum(l_run));
  __syncthreads();
  float* mo = (float*)ad_smem;
  float* mm = mo + AD_NW * 32 * 64;
  float* ml = mm + AD_NW * 64;
#pragma unroll
  for (int ct = 0; ct < 8; ++ct)
#pragma unroll
    for (int j = 0; j < 4; ++j) mo[(wave * 32 + ct * 4 + j) * 64 + lane] = oacc[ct][j];
  mm[wave * 64 + lane] = m_run;
  ml[wave * 64 + lane] = l_run;
  __syncthreads();
  float m_tot = -INFINITY;
#pragma unroll
  for (int w = 0; w < AD_NW; ++w) m_tot = fmaxf(m_tot, mm[w * 64 + lane]);       // APPEND: -inf if the column sees no key of the split
  const float m_ref = APPEND && m_tot == -INFINITY ? 0.f : m_tot;
  float sc[AD_NW], l_tot = 0.f;
#pragma unroll
  for (int w = 0; w < AD_NW; ++w) {
    sc[w] = __builtin_amdgcn_exp2f(mm[w * 64 + lane] - m_ref);                    // exp2(-inf) = 0 for idle waves
    l_tot += sc[w] * ml[w * 64 + lane];
  }
  if (n < nh) {
    const int64_t slot = slot_of<APPEND>(a, b, tok, head) + split;
    for (int ct = wave; ct < 8; ct += AD_NW) {
      f32x4 r = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int w = 0; w < AD_NW; ++w)
#pragma unroll
        for (int j = 0; j < 4; ++j) r[j] += sc[w] * mo[(w * 32 + ct * 4 + j) * 64 + lane];
      *(f32x4*)(a.part_o + slot * AD_D + 16 * ct + 4 * g) = r;     // O^T rows d = 16 ct + 4 g + j of column n
    }
    if (wave == 0 && g == 0) {
      a.part_ml[slot * 2] = m_tot;
      a.part_ml[slot * 2 + 1] = l_tot;
    }
  }
}

// o[b][tok][h][d] = sum_s 2^(m_s - M) O_s[d] / sum_s 2^(m_s - M) l_s over the splits that hold keys; 128 threads,
// grid (Hq, batch), or (T * Hq, batch) with block x = token * Hq + head for the continuation.
// One pass with a running maximum, the loads of 8 splits issued before their first use (a split at a time the kernel was
// 32 dependent round trips to L2: 12 us for 1 MB).
template <bool APPEND>
__global__ __launch_bounds__(AD_D) void attn_splitkv_merge_kernel(DecArgs a) {
  constexpr int U = 8;
  typedef float f32x2 __attribute__((ext_vector_type(2)));
  const int tok = APPEND ? blockIdx.x / a.Hq : 0, h = APPEND ? blockIdx.x % a.Hq : blockIdx.x;
  const int b = blockIdx.y, d = threadIdx.x;
  int Lk, chunk;
  split_of(a, b, Lk, chunk);
  const int nvalid = (Lk + chunk - 1) / chunk;
  const int64_t slot0 = slot_of<APPEND>(a, b, tok, h);
  float M = -INFINITY, L = 0.f, O = 0.f;
  for (int s0 = 0; s0 < nvalid; s0 += U) {
    f32x2 ml[U];
    float o[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int sidx = min(s0 + u, nvalid - 1);        // (past the end: the last split again, weighted 0 below)
      ml[u] = *(const f32x2*)(a.part_ml + (slot0 + sidx) * 2);
      o[u] = a.part_o[(slot0 + sidx) * AD_D + d];
    }
    float mb = M;
#pragma unroll
    for (int u = 0; u < U; ++u) mb = s0 + u < nvalid ? fmaxf(mb, ml[u][0]) : mb;
    const float mr = APPEND && mb == -INFINITY ? 0.f : mb;       // (APPEND: no split so far holds a key this column sees)
    const float sc = __builtin_amdgcn_exp2f(M - mr);   // (M = -inf: 0)
    L *= sc;
    O *= sc;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const float w = s0 + u < nvalid ? __builtin_amdgcn_exp2f(ml[u][0] - mr) : 0.f;
      L = fmaf(w, ml[u][1], L);
      O = fmaf(w, o[u], O);
    }
    M = mb;
  }
  // (the two tests agree on finite partials; a NaN in them reaches a decode result and not a continuation's)
  const bool any = APPEND ? L > 0.f : nvalid > 0;
  a.o[(int64_t)b * a.osb + (APPEND ? (int64_t)tok * a.osl : 0) + (int64_t)h * a.osh + d] = from_f32<bf16_t>(any ? O / L : 0.f);
  if (a.lse && d == 0)          // (B, Hq), continuation (B, Hq, T)
    a.lse[APPEND ? ((int64_t)b * a.Hq + h) * a.T + tok : (int64_t)b * a.Hq + h] =
        any ? (M + __log2f(L)) * 0.6931471805599453f : -INFINITY;
}

int pick_splits(int batch, int nheads_kv, int hblocks, int seqlen_k) {
  const int per = batch * nheads_kv * hblocks;
  int want = (tv_cu_count() + per - 1) / per;                       // one work-group per CU
  const int most = (seqlen_k + AD_NW * AD_STEP - 1) / (AD_NW * AD_STEP);          // >= one step per wave
  if (want > most) want = most;
  if (want > AD_MAX_SPLIT) want = AD_MAX_SPLIT;
  return want < 1 ? 1 : want;
}

size_t workspace_bytes(int batch, int seqlen_q, int nheads_q, int nheads_kv, int seqlen_k) {
  if (batch <= 0 || seqlen_q <= 0 || nheads_q <= 0 || nheads_kv <= 0 || nheads_q % nheads_kv || seqlen_k < 0) return 0;
  const int hblocks = (seqlen_q * (nheads_q / nheads_kv) + 15) / 16;
  return (size_t)batch * seqlen_q * nheads_q * pick_splits(batch, nheads_kv, hblocks, seqlen_k) * AD_SLOT_BYTES;
}

int g_append_calls = 0;

// Both entry points; `name` prefixes the messages.  Decode: seqlen_q = 1 and token strides of 0.
template <bool APPEND>
int splitkv_fwd(const char* name, const void* q, const void* k, const void* v, void* o, void* lse, int batch, int seqlen_q,
                int seqlen_k, const int* seqlens_k, int nheads_q, int nheads_kv, int headdim, int64_t q_stride_b,
                int64_t q_stride_l, int64_t q_stride_h, int64_t k_stride_b, int64_t k_stride_l, int64_t k_stride_h,
                int64_t v_stride_b, int64_t v_stride_l, int64_t v_stride_h, int64_t o_stride_b, int64_t o_stride_l,
                int64_t o_stride_h, float softmax_scale, int dtype, void* workspace, size_t workspace_bytes,
                void* stream) {
  // decode on an empty cache (no k / v needed) runs the merge kernel alone; a continuation holds its own keys
  TV_CHECK_ARG(q && o && ((!APPEND && seqlen_k == 0) || (k && v)), "%s: null pointer", name);
  TV_CHECK_ARG(batch > 0 && seqlen_q > 0 && seqlen_k >= (APPEND ? seqlen_q : 0) && nheads_q > 0 && nheads_kv > 0 &&
                   nheads_q % nheads_kv == 0 && softmax_scale > 0.f,
               "%s: bad sizes or non-positive softmax scale%s", name,
               APPEND ? " (the queries are the last seqlen_q of the seqlen_k keys)" : "");
  if (dtype != TV_BF16) TV_UNSUPPORTED("%s: dtype must be bf16 (tv_flash_attn_fwd takes f16)", name);
  if (headdim != AD_D) TV_UNSUPPORTED("%s: headdim %d (this kernel: 128; tv_flash_attn_fwd takes the rest)", name, headdim);
  const int gq = nheads_q / nheads_kv, ncols = seqlen_q * gq, hblocks = (ncols + 15) / 16;
  if (APPEND && (seqlen_q > AP_MAX_T || ncols > AP_MAX_COLS))
    TV_UNSUPPORTED("%s: %d query tokens x %d q-heads per kv-head (this kernel: <= %d tokens, <= %d columns)", name,
                   seqlen_q, gq, AP_MAX_T, AP_MAX_COLS);
  const int64_t strides[] = {q_stride_b, q_stride_l, q_stride_h, k_stride_b, k_stride_l, k_stride_h, v_stride_b, v_stride_l, v_stride_h};
  for (int64_t s : strides)
    if (s % 8) TV_UNSUPPORTED("%s: q/k/v strides must be multiples of 8 elements", name);
  if (((uintptr_t)q & 15) || ((uintptr_t)k & 15) || ((uintptr_t)v & 15))
    TV_UNSUPPORTED("%s: q/k/v must be 16-byte aligned", name);
  if (k_stride_l < AD_D || v_stride_l < AD_D) TV_UNSUPPORTED("%s: k/v rows must not overlap", name);
  const int nsplit = pick_splits(batch, nheads_kv, hblocks, seqlen_k);
  // K and V rows are addressed with 32-bit byte offsets from the first key of a split
  if (((int64_t)seqlen_k / nsplit + 2 * AD_STEP) * v_stride_l * 2 >= (1ll << 31) ||
      ((int64_t)seqlen_k / nsplit + 2 * AD_STEP) * k_stride_l * 2 >= (1ll << 31))
    TV_UNSUPPORTED("%s: k / v row stride too large for a split of %d keys", name, seqlen_k / nsplit);
  const size_t slots = (size_t)batch * seqlen_q * nheads_q * nsplit;
  const size_t need = slots * AD_SLOT_BYTES;
  TV_CHECK_ARG(workspace && workspace_bytes >= need && ((uintptr_t)workspace & 15) == 0,
               "%s: workspace of %zu bytes (16-byte aligned) needed, got %zu", name, need, workspace_bytes);
  DecArgs a;
  a.q = (const bf16_t*)q; a.k = (const bf16_t*)k; a.v = (const bf16_t*)v; a.o = (bf16_t*)o; a.lse = (float*)lse;
  a.part_o = (float*)workspace;
  a.part_ml = a.part_o + slots * AD_D;
  a.seqlens = seqlens_k;
  a.Lk = seqlen_k; a.Hq = nheads_q; a.Hkv = nheads_kv; a.gq = gq; a.hblocks = hblocks; a.nsplit = nsplit;
  a.T = seqlen_q; a.ncols = ncols; a.qsl = q_stride_l; a.osl = o_stride_l;
  a.qsb = q_stride_b; a.qsh = q_stride_h; a.ksb = k_stride_b; a.ksl = k_stride_l; a.ksh = k_stride_h;
  a.vsb = v_stride_b; a.vsl = v_stride_l; a.vsh = v_stride_h; a.osb = o_stride_b; a.osh = o_stride_h;
  a.scale_log2 = softmax_scale * 1.4426950408889634f;
  hipStream_t st = (hipStream_t)stream;
  static const hipError_t attr = hipFuncSetAttribute((const void*)attn_splitkv_kernel<APPEND>,
                                                     hipFuncAttributeMaxDynamicSharedMemorySize, AD_LDS);
  if (attr != hipSuccess) {
    tv_set_error("%s: cannot reserve %d bytes of LDS: %s", name, AD_LDS, hipGetErrorString(attr));
    return TV_ERR_LAUNCH;
  }
  if (APPEND) ++g_append_calls;
  if (seqlen_k > 0)
    attn_splitkv_kernel<APPEND><<<dim3((unsigned)nsplit, (unsigned)(nheads_kv * hblocks), (unsigned)batch), AD_NW * 64, AD_LDS, st>>>(a);
  attn_splitkv_merge_kernel<APPEND><<<dim3((unsigned)(seqlen_q * nheads_q), (unsigned)batch), AD_D, 0, st>>>(a);
  TV_LAUNCH_CHECK();
}

}  // namespace

extern "C" size_t tv_attn_decode_workspace_bytes(int batch, int nheads_q, int nheads_kv, int seqlen_k) {
  return workspace_bytes(batch, 1, nheads_q, nheads_kv, seqlen_k);
}

extern "C" int tv_attn_decode_fwd(const void* q, const void* k, const void* v, void* o, void* lse, int batch,
                                  int seqlen_k, const int* seqlens_k, int nheads_q, int nheads_kv, int headdim,
                                  int64_t q_stride_b, int64_t q_stride_h, int64_t k_stride_b, int64_t k_stride_l,
                                  int64_t k_stride_h, int64_t v_stride_b, int64_t v_stride_l, int64_t v_stride_h,
                                  int64_t o_stride_b, int64_t o_stride_h, float softmax_scale, int dtype,
                                  void* workspace, size_t workspace_bytes, void* stream) {
  return splitkv_fwd<false>("attn_decode", q, k, v, o, lse, batch, 1, seqlen_k, seqlens_k, nheads_q, nheads_kv, headdim,
                            q_stride_b, 0, q_stride_h, k_stride_b, k_stride_l, k_stride_h, v_stride_b, v_stride_l,
                            v_stride_h, o_stride_b, 0, o_stride_h, softmax_scale, dtype, workspace, workspace_bytes, stream);
}

extern "C" size_t tv_attn_append_workspace_bytes(int batch, int seqlen_q, int nheads_q, int nheads_kv, int seqlen_k) {
  return workspace_bytes(batch, seqlen_q, nheads_q, nheads_kv, seqlen_k);
}

extern "C" int tv_attn_append_calls(void) { return g_append_calls; }

extern "C" int tv_attn_append_fwd(const void* q, const void* k, const void* v, void* o, void* lse, int batch,
                                  int seqlen_q, int seqlen_k, const int* seqlens_k, int nheads_q, int nheads_kv,
                                  int headdim, int64_t q_stride_b, int64_t q_stride_l, int64_t q_stride_h,
                                  int64_t k_stride_b, int64_t k_stride_l, int64_t k_stride_h, int64_t v_stride_b,
                                  int64_t v_stride_l, int64_t v_stride_h, int64_t o_stride_b, int64_t o_stride_l,
                                  int64_t o_stride_h, float softmax_scale, int dtype, void* workspace,
                                  size_t workspace_bytes, void* stream) {
  return splitkv_fwd<true>("attn_append", q, k, v, o, lse, batch, seqlen_q, seqlen_k, seqlens_k, nheads_q, nheads_kv,
                           headdim, q_stride_b, q_stride_l, q_stride_h, k_stride_b, k_stride_l, k_stride_h, v_stride_b,
                           v_stride_l, v_stride_h, o_stride_b, o_stride_l, o_stride_h, softmax_scale, dtype, workspace,
                           workspace_bytes, stream);
}
