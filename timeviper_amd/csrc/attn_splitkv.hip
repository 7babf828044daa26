// T3 (decode, continuation, branches): a FEW query tokens against a long K / V cache, as one split-KV walk with three
// instantiations:
//   tv_attn_decode_fwd   ONE query token — the attention of a generate() step (modeling_nano.py:1198-1209 with q_len == 1;
//                        the cache layout of HybridMambaAttentionDynamicCache, :205-360);
//   tv_attn_append_fwd   the LAST T tokens of a sequence — the attention of a forward that continues a prefilled cache with
//                        a few tokens (a follow-up question, a tool result, a draft to verify);
//   tv_attn_branch_fwd   ONE query token of each of B branches that share ONE prefix (a prefilled video asked several
//                        questions at once) and hold a short suffix each.
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
//
// What the branches add (BRANCH; the other two instantiations contain none of it): ONE launch holds two kinds of
// work-group.  A PREFIX work-group is the continuation's with the B branches in the place of the T tokens — the columns of a
// kv-head are its B * gq (branch c / gq, head c % gq) pairs, the prefix K / V is read once per kv-head and block of 16
// columns, never per branch — and without the causal bound: every branch sees the whole prefix.  A SUFFIX work-group is
// the decode step's: the gq heads of ONE branch over that branch's own n_b rows (device-side count, clamped to the
// capacity; n_b = 0: no work-group runs and the merge skips the slot).  A (branch, q-head) owns nsplit prefix slots followed
// by nsplit_s suffix slots; the merge kernel reduces the ones that hold keys.  Prefix_len >= 1, so a result is never empty.
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

constexpr int BR_MAX = 16, BR_SUFFIX_SPLIT_KEYS = 4 * AD_NW * AD_STEP, BR_MAX_SUFFIX_SPLIT = 16;

struct DecArgs {
  const bf16_t *q, *k, *v;
  bf16_t* o;
  float *lse, *part_o, *part_ml;
  const int* seqlens;                         // device, one per batch entry; nullptr: Lk for all
  int Lk, Hq, Hkv, gq, hblocks, nsplit, T, ncols;          // hblocks: blocks of 16 of the T * gq columns of a kv-head
  int64_t qsl, osl, qsb, qsh, ksb, ksl, ksh, vsb, vsl, vsh, osb, osh;       // (decode: T = 1, the token strides unused)
  float scale_log2;
  // the branch step alone: DecArgs describes the PREFIX (k / v one sequence, Lk = prefix_len, T = branches, the token strides
  // = the branch strides of q and o, nsplit / hblocks of the prefix walk, `seqlens` the SUFFIX counts), these the suffixes
  const bf16_t *ks, *vs;                      // (B, cap, Hkv, D)
  int cap, nsplit_s, nblk_p, hbq;             // suffix capacity and splits; prefix work-groups of the grid; blocks of 16 of gq
  int64_t kssb, kssl, kssh, vssb, vssl, vssh;
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

// The work of a BRANCH work-group (block x, uniform): the prefix work-groups first, split fastest, then the suffix ones.
struct BranchWork {
  bool sfx;
  int split, hk, hb, br, Lk, chunk;           // hb: block of 16 of the B * gq columns (prefix) / of the gq heads (suffix)
};
__device__ __forceinline__ BranchWork branch_work(const DecArgs& a, int x) {
  BranchWork w;
  w.sfx = x >= a.nblk_p;
  if (!w.sfx) {
    w.split = x % a.nsplit;
    x /= a.nsplit;
    w.hb = x % a.hblocks;
    w.hk = x / a.hblocks;
    w.br = 0;
    w.Lk = a.Lk;
    w.chunk = ((a.Lk + a.nsplit - 1) / a.nsplit + AD_STEP - 1) / AD_STEP * AD_STEP;
  } else {
    x -= a.nblk_p;
    w.split = x % a.nsplit_s;
    x /= a.nsplit_s;
    w.hb = x % a.hbq;
    x /= a.hbq;
    w.hk = x % a.Hkv;
    w.br = x / a.Hkv;
    w.Lk = a.seqlens ? min(max(a.seqlens[w.br], 0), a.cap) : a.cap;
    w.chunk = ((w.Lk + a.nsplit_s - 1) / a.nsplit_s + AD_STEP - 1) / AD_STEP * AD_STEP;
  }
  if (w.chunk == 0) w.chunk = AD_STEP;
  return w;
}

// The walk kernels share one body, attn_splitkv_walk.inc (`a`, APPEND and BRANCH are what it reads): it loads its Q
// fragments with ssdk::gload16_async and walks the keys behind hand-counted vmcnt waits, so none of them may use scratch.
template <bool APPEND>
__global__ __launch_bounds__(AD_NW * 64) void attn_splitkv_kernel(DecArgs a) {
  constexpr bool BRANCH = false;
#include "attn_splitkv_walk.inc"
}

__global__ __launch_bounds__(AD_NW * 64) void attn_branch_kernel(DecArgs a) {
  constexpr bool APPEND = false, BRANCH = true;
#include "attn_splitkv_walk.inc"
}

// o[b][tok][h][d] = sum_s 2^(m_s - M) O_s[d] / sum_s 2^(m_s - M) l_s over the splits that hold keys; 128 threads,
// grid (Hq, batch), or (T * Hq, batch) with block x = token * Hq + head for the continuation.
// One pass with a running maximum, the loads of 8 splits issued before their first use (a split at a time the kernel was
// 32 dependent round trips to L2: 12 us for 1 MB).
// BRANCH: grid (B * Hq), block x = branch * Hq + head; the prefix slots that hold keys, then the suffix ones.
template <bool APPEND>
__global__ __launch_bounds__(AD_D) void attn_splitkv_merge_kernel(DecArgs a) {
  constexpr bool BRANCH = false;
#include "attn_splitkv_merge.inc"
}

__global__ __launch_bounds__(AD_D) void attn_branch_merge_kernel(DecArgs a) {
  constexpr bool APPEND = false, BRANCH = true;
#include "attn_splitkv_merge.inc"
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
  DecArgs a = {};
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

// ---- the branch step
int g_branch_calls = 0;

int branch_suffix_splits(int suffix_cap) {
  const int want = (suffix_cap + BR_SUFFIX_SPLIT_KEYS - 1) / BR_SUFFIX_SPLIT_KEYS;
  return want < 1 ? 1 : want > BR_MAX_SUFFIX_SPLIT ? BR_MAX_SUFFIX_SPLIT : want;
}

// in the kernel's range: B <= 16 branches, B * gq <= 128 columns
bool branch_in_range(int branches, int nheads_q, int nheads_kv) {
  return branches <= BR_MAX && branches * (nheads_q / nheads_kv) <= AP_MAX_COLS;
}

}  // namespace

extern "C" size_t tv_attn_branch_workspace_bytes(int branches, int nheads_q, int nheads_kv, int prefix_len, int suffix_cap) {
  if (branches <= 0 || nheads_q <= 0 || nheads_kv <= 0 || nheads_q % nheads_kv || prefix_len < 1 || suffix_cap < 0 ||
      !branch_in_range(branches, nheads_q, nheads_kv))
    return 0;
  const int hblocks = (branches * (nheads_q / nheads_kv) + 15) / 16;
  return (size_t)branches * nheads_q * (pick_splits(1, nheads_kv, hblocks, prefix_len) + branch_suffix_splits(suffix_cap)) *
         AD_SLOT_BYTES;
}

extern "C" int tv_attn_branch_calls(void) { return g_branch_calls; }

extern "C" int tv_attn_branch_fwd(const void* q, const void* k_prefix, const void* v_prefix, const void* k_suffix,
                                  const void* v_suffix, void* o, void* lse, int branches, int prefix_len, int suffix_cap,
                                  const int* seqlens_suffix, int nheads_q, int nheads_kv, int headdim, int64_t q_stride_b,
                                  int64_t q_stride_h, int64_t kp_stride_l, int64_t kp_stride_h, int64_t vp_stride_l,
                                  int64_t vp_stride_h, int64_t ks_stride_b, int64_t ks_stride_l, int64_t ks_stride_h,
                                  int64_t vs_stride_b, int64_t vs_stride_l, int64_t vs_stride_h, int64_t o_stride_b,
                                  int64_t o_stride_h, float softmax_scale, int dtype, void* workspace,
                                  size_t workspace_bytes, void* stream) {
  const char* name = "attn_branch";
  TV_CHECK_ARG(q && o && k_prefix && v_prefix && (suffix_cap == 0 || (k_suffix && v_suffix)), "%s: null pointer", name);
  TV_CHECK_ARG(branches > 0 && prefix_len >= 1 && suffix_cap >= 0 && nheads_q > 0 && nheads_kv > 0 &&
                   nheads_q % nheads_kv == 0 && softmax_scale > 0.f,
               "%s: bad sizes or non-positive softmax scale (the shared prefix holds at least one key)", name);
  if (dtype != TV_BF16) TV_UNSUPPORTED("%s: dtype must be bf16", name);
  if (headdim != AD_D) TV_UNSUPPORTED("%s: headdim %d (this kernel: 128)", name, headdim);
  const int gq = nheads_q / nheads_kv, ncols = branches * gq, hblocks = (ncols + 15) / 16, hbq = (gq + 15) / 16;
  if (!branch_in_range(branches, nheads_q, nheads_kv))
    TV_UNSUPPORTED("%s: %d branches x %d q-heads per kv-head (this kernel: <= %d branches, <= %d columns)", name, branches,
                   gq, BR_MAX, AP_MAX_COLS);
  const int64_t strides[] = {q_stride_b, q_stride_h, kp_stride_l, kp_stride_h, vp_stride_l, vp_stride_h,
                             ks_stride_b, ks_stride_l, ks_stride_h, vs_stride_b, vs_stride_l, vs_stride_h};
  for (int64_t s : strides)
    if (s % 8) TV_UNSUPPORTED("%s: q/k/v strides must be multiples of 8 elements", name);
  if (((uintptr_t)q & 15) || ((uintptr_t)k_prefix & 15) || ((uintptr_t)v_prefix & 15) || ((uintptr_t)k_suffix & 15) ||
      ((uintptr_t)v_suffix & 15))
    TV_UNSUPPORTED("%s: q/k/v must be 16-byte aligned", name);
  if (kp_stride_l < AD_D || vp_stride_l < AD_D || (suffix_cap > 0 && (ks_stride_l < AD_D || vs_stride_l < AD_D)))
    TV_UNSUPPORTED("%s: k/v rows must not overlap", name);
  const int nsplit = pick_splits(1, nheads_kv, hblocks, prefix_len), nsplit_s = branch_suffix_splits(suffix_cap);
  // K and V rows are addressed with 32-bit byte offsets from the first key of a split
  const int64_t rows_p = (int64_t)prefix_len / nsplit + 2 * AD_STEP, rows_s = (int64_t)suffix_cap / nsplit_s + 2 * AD_STEP;
  if (rows_p * kp_stride_l * 2 >= (1ll << 31) || rows_p * vp_stride_l * 2 >= (1ll << 31) ||
      rows_s * ks_stride_l * 2 >= (1ll << 31) || rows_s * vs_stride_l * 2 >= (1ll << 31))
    TV_UNSUPPORTED("%s: k / v row stride too large for a split", name);
  const size_t slots = (size_t)branches * nheads_q * (nsplit + nsplit_s);
  const size_t need = slots * AD_SLOT_BYTES;
  TV_CHECK_ARG(workspace && workspace_bytes >= need && ((uintptr_t)workspace & 15) == 0,
               "%s: workspace of %zu bytes (16-byte aligned) needed, got %zu", name, need, workspace_bytes);
  DecArgs a = {};
  a.q = (const bf16_t*)q; a.k = (const bf16_t*)k_prefix; a.v = (const bf16_t*)v_prefix; a.o = (bf16_t*)o; a.lse = (float*)lse;
  a.part_o = (float*)workspace;
  a.part_ml = a.part_o + slots * AD_D;
  a.seqlens = seqlens_suffix;
  a.Lk = prefix_len; a.Hq = nheads_q; a.Hkv = nheads_kv; a.gq = gq; a.hblocks = hblocks; a.nsplit = nsplit;
  a.T = branches; a.ncols = ncols; a.qsl = q_stride_b; a.osl = o_stride_b;
  a.qsb = 0; a.qsh = q_stride_h; a.ksb = 0; a.ksl = kp_stride_l; a.ksh = kp_stride_h;
  a.vsb = 0; a.vsl = vp_stride_l; a.vsh = vp_stride_h; a.osb = 0; a.osh = o_stride_h;
  a.scale_log2 = softmax_scale * 1.4426950408889634f;
  a.ks = (const bf16_t*)k_suffix; a.vs = (const bf16_t*)v_suffix;
  a.cap = suffix_cap; a.nsplit_s = nsplit_s; a.nblk_p = nsplit * nheads_kv * hblocks; a.hbq = hbq;
  a.kssb = ks_stride_b; a.kssl = ks_stride_l; a.kssh = ks_stride_h;
  a.vssb = vs_stride_b; a.vssl = vs_stride_l; a.vssh = vs_stride_h;
  hipStream_t st = (hipStream_t)stream;
  static const hipError_t attr = hipFuncSetAttribute((const void*)attn_branch_kernel,
                                                     hipFuncAttributeMaxDynamicSharedMemorySize, AD_LDS);
  if (attr != hipSuccess) {
    tv_set_error("%s: cannot reserve %d bytes of LDS: %s", name, AD_LDS, hipGetErrorString(attr));
    return TV_ERR_LAUNCH;
  }
  ++g_branch_calls;
  // (suffix work-groups of a branch with no rows, or of a capacity of 0, leave at once)
  const unsigned nblk = (unsigned)(a.nblk_p + (suffix_cap > 0 ? branches * nheads_kv * hbq * nsplit_s : 0));
  attn_branch_kernel<<<dim3(nblk), AD_NW * 64, AD_LDS, st>>>(a);
  attn_branch_merge_kernel<<<dim3((unsigned)(branches * nheads_q)), AD_D, 0, st>>>(a);
  TV_LAUNCH_CHECK();
}

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
