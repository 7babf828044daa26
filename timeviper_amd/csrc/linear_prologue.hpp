// The prologue contract of the weight-streaming linear kernels (gemv.hip: 1 - 4 rows, linear_rows.hip: 1 - 16 rows),
// defined once: the operator f in front of the product y = f(x) W^T (+ bias), the device helpers both prologues are
// built from, and the host-side checks of the arguments both C entry points share.
//   PRO_NONE      f(x) = x
//   PRO_RMSNORM   s = bf16(x + delta) (written to `sum_out` by work-group 0: the new residual stream),
//                 f = bf16(w * (s * rsqrt(mean(s^2) + eps)))             NemotronHRMSNorm + block add, modeling_nano.py:897-903, :966
//   PRO_RELU2     f = bf16(relu(x)^2)                                    NemotronHMLP, :993-994
//   PRO_GATED     v = x * silu(z), f = bf16(w * (v * rsqrt(mean_group(v^2) + eps)))     MambaRMSNormGated, :371-380
// with the rounding points of the stand-alone kernels (norms.hip).  Everything here has internal linkage: each of the
// two translation units compiles its own copy.
#pragma once
#include "ssd_common.hpp"

namespace {

enum { PRO_NONE = 0, PRO_RMSNORM = 1, PRO_RELU2 = 2, PRO_GATED = 3 };
constexpr int PRO_RMSNORM_MAX_K = 8192;              // a row of the rmsnorm prologue (gemv: 8 channels x 256 threads x 4 pieces in registers)
constexpr int PRO_GATED_MAX_GROUP = 8 * 64 * 4;      // a group of the gated prologue: 8 channels x 64 lanes x 4 pieces in registers

// the 8 norm weights of one 16-byte piece of x: requested here (fp32 weights: two 16-byte loads, bf16: one), turned into
// floats by normw_get — AFTER every other request of the prologue is out: a conversion next to the load is a wait for it
struct NormW { f32x4 lo, hi; };
__device__ __forceinline__ NormW normw_load(const void* w, int f32, int i0) {
  // no branch: a value that arrives through one of two paths is copied where they join, and a copy is a wait for the load
  const char* base = (const char*)w + (size_t)i0 * (f32 ? 4 : 2);
  NormW r;
  r.lo = *(const f32x4*)base;
  r.hi = *(const f32x4*)(base + (f32 ? 16 : 0));       // (bf16 weights: the same 16 bytes again)
  return r;
}
__device__ __forceinline__ void normw_get(const NormW& r, int f32, float (&out)[8]) {
  if (f32) {
#pragma unroll
    for (int j = 0; j < 4; ++j) { out[j] = r.lo[j]; out[4 + j] = r.hi[j]; }
  } else {
    const bf16x8 v = __builtin_bit_cast(bf16x8, r.lo);
#pragma unroll
    for (int j = 0; j < 8; ++j) out[j] = (float)v[j];
  }
}

// 16 bytes of W; NT: non-temporal (a weight byte is used once a token: it should not displace x / the norm weights in L2)
template <bool NT>
__device__ __forceinline__ bf16x8 ldw8(const bf16_t* p) {
  return NT ? __builtin_nontemporal_load((const bf16x8*)p) : *(const bf16x8*)p;
}

// Host: the checks of the arguments tv_gemv_bf16_fwd and tv_linear_rows_bf16_fwd have in common, made before any HIP call,
// and the fields of GemvArgs / RowsArgs (`Args`: either, under its own name) they fill.  `name` starts the messages,
// `max_m` is the kernel's row limit.  Returns TV_OK, or the status to return with tv_last_error() set.
template <typename Args>
int linear_args_fill(Args& a, const char* name, int max_m, const void* x, const void* W, const void* bias, void* y, int M,
                     int N, int K, int64_t x_stride, int64_t ldw, int64_t y_stride, int prologue, const void* delta,
                     int64_t delta_stride, void* sum_out, int64_t sum_stride, const void* norm_weight,
                     int norm_weight_dtype, float eps, const void* gate, int64_t gate_stride, int group_size) {
  TV_CHECK_ARG(x && W && y, "%s: null pointer", name);
  TV_CHECK_ARG(M >= 1 && M <= max_m && N >= 1 && K >= 8, "%s: M %d must be 1..%d, N %d >= 1, K %d >= 8", name, M, max_m, N, K);
  if (K % 8 || ldw % 8 || x_stride % 8 || ((uintptr_t)x & 15) || ((uintptr_t)W & 15))
    TV_UNSUPPORTED("%s: K, the row strides of x and W must be multiples of 8 elements, x and W 16-byte aligned", name);
  TV_CHECK_ARG(prologue >= PRO_NONE && prologue <= PRO_GATED, "%s: prologue %d", name, prologue);
  // (a stride shorter than the row: rows that overlap — read, or written, past what the caller laid out)
  TV_CHECK_ARG(ldw >= K && (M == 1 || (x_stride >= K && y_stride >= N)),
               "%s: row strides (x %lld, W %lld, y %lld) shorter than the rows (K %d, N %d)", name, (long long)x_stride,
               (long long)ldw, (long long)y_stride, K, N);
  a.x = (const bf16_t*)x; a.W = (const bf16_t*)W; a.bias = (const bf16_t*)bias; a.y = (bf16_t*)y;
  a.delta = nullptr; a.gate = nullptr; a.norm_w = nullptr; a.sum_out = nullptr;
  a.M = M; a.N = N; a.K = K; a.group = K; a.norm_w_f32 = 0;
  a.xs = x_stride; a.ldw = ldw; a.ys = y_stride; a.ds = a.ss = a.gs = 0; a.eps = eps;
  if (prologue == PRO_RMSNORM || prologue == PRO_GATED) {
    TV_CHECK_ARG(norm_weight && (norm_weight_dtype == TV_F32 || norm_weight_dtype == TV_BF16), "%s: norm weight (fp32 or bf16) needed", name);
    a.norm_w = norm_weight; a.norm_w_f32 = norm_weight_dtype == TV_F32;
  }
  if (prologue == PRO_RMSNORM) {
    if (K > PRO_RMSNORM_MAX_K) TV_UNSUPPORTED("%s: rmsnorm prologue takes rows of <= %d channels", name, PRO_RMSNORM_MAX_K);
    if (delta && (delta_stride % 8 || ((uintptr_t)delta & 15))) TV_UNSUPPORTED("%s: delta must be 16-byte aligned rows", name);
    if (sum_out && (sum_stride % 8 || ((uintptr_t)sum_out & 15))) TV_UNSUPPORTED("%s: sum_out must be 16-byte aligned rows", name);
    TV_CHECK_ARG(M == 1 || ((!delta || delta_stride >= K) && (!sum_out || sum_stride >= K)),
                 "%s: delta / sum_out row strides shorter than K %d", name, K);
    TV_CHECK_ARG(!sum_out || (sum_out != x && sum_out != delta), "%s: sum_out must not alias x or delta", name);
    a.delta = (const bf16_t*)delta; a.ds = delta_stride; a.sum_out = (bf16_t*)sum_out; a.ss = sum_stride;
  }
  if (prologue == PRO_GATED) {
    TV_CHECK_ARG(group_size > 0 && K % group_size == 0 && group_size % 8 == 0, "%s: group size %d must divide K %d (multiple of 8)", name, group_size, K);
    if (group_size > PRO_GATED_MAX_GROUP) TV_UNSUPPORTED("%s: gated-norm prologue holds groups of <= %d channels", name, PRO_GATED_MAX_GROUP);
    if (gate && (gate_stride % 8 || ((uintptr_t)gate & 15))) TV_UNSUPPORTED("%s: gate must be 16-byte aligned rows", name);
    TV_CHECK_ARG(M == 1 || !gate || gate_stride >= K, "%s: gate row stride shorter than K %d", name, K);
    a.gate = (const bf16_t*)gate; a.gs = gate_stride; a.group = group_size;
  }
  return TV_OK;
}

}  // namespace
