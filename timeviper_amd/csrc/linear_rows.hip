// Few-token linear layers: y[m][n] = sum_k f(x)[m][k] W[n][k] (+ bias[n]) for 1 <= M <= 16 rows (a continuation or a
// speculative step of T tokens on one sequence).
//
// The weights are read once whether one token or sixteen use them, so this is gemv.hip's problem — stream W from HBM with
// 16-byte non-temporal loads, many in flight per wave, nothing but the loads in the stream — with the products on the
// matrix pipe: 16 rows of W are the A operand of v_mfma_f32_16x16x32_bf16, the (up to) 16 token rows the B operand.
// Lane l of a wave holds row (l & 15) of a 16-row tile of W and the 64 contiguous bytes [32 (l >> 4), 32 (l >> 4) + 32) of
// a 128-channel step: four loads, four MFMAs, 256 contiguous bytes of every row per wave and step.  The k order inside
// an MFMA is then not the memory order, which is free as long as the token operand uses the same one: lane l reads
// f(x)[min(l & 15, M - 1)][the same 4 x 8 channels] from LDS.  Columns M..15 of the result are copies of column M - 1 and
// are never stored; nothing is read for them.
//
// A work-group owns the tiles b, b + G, ... (at most 16: 4 accumulator registers each) and walks K in slices whose f(x)
// fits its 72 KiB of LDS (two work-groups a CU), keeping the accumulators across the slices.  Inside a slice its four
// waves split the steps into contiguous quarters; the four partial tiles meet in LDS once, after the last slice, and
// are added in wave order: deterministic, no atomics.  f is the prologue set of linear_prologue.hpp, with the rounding points and the
// order of the sums of squares of the stand-alone kernels in norms.hip (so the same rstd, bit for bit):
//   PRO_NONE / PRO_RELU2   elementwise, slice by slice
//   PRO_RMSNORM            one pass over x (+ delta) for the M sums of squares — work-group 0 writes all M rows of the new
//                          residual stream to `sum_out` there — then elementwise with the row's rstd; x lives in L2
//   PRO_GATED              slices are whole norm groups: a wave per (row, group), statistics inside the slice
#include "linear_prologue.hpp"

namespace {

constexpr int LR_THREADS = 256;
constexpr int LR_WAVES = LR_THREADS / 64;
constexpr int LR_MAXM = 16;
constexpr int LR_STEP = 128;                         // channels a wave takes per step (4 MFMAs of 32)
constexpr int LR_PAD = 8;                            // LDS row padding: a row stride of an odd number of 16-byte pieces
constexpr int LR_LDS = 72 * 1024;                    // dynamic LDS of a work-group
constexpr int LR_MAXT = 16;                          // tiles a work-group accumulates
constexpr int LR_FU = 4;                             // 16-byte pieces of x a thread requests before it converts the first

struct RowsArgs {
  const bf16_t *x, *W, *bias, *delta, *gate;
  const void* norm_w;
  bf16_t *y, *sum_out;
  int M, N, K, group, norm_w_f32;
  int KS, lds_stride;                                // channels a slice (multiple of LR_STEP, or of `group`); LDS row stride
  int64_t xs, ldw, ys, ds, ss, gs;
  float eps;
};

// PRO_RMSNORM, once a work-group: stat[m] = rsqrt(mean(bf16(x + delta)[m]^2) + eps); work-group 0 writes the sums.
// A thread's pieces and the order of the additions are rmsnorm_kernel's (norms.hip).
__device__ __forceinline__ void rows_rms_stats(const RowsArgs& a, float (*red)[LR_WAVES], float* stat) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nv = a.K / 8;
  for (int m = 0; m < a.M; ++m) {
    const bf16_t* xr = a.x + (int64_t)m * a.xs;
    const bf16_t* dr = a.delta ? a.delta + (int64_t)m * a.ds : xr;
    float ssq = 0.f;
#pragma unroll 4
    for (int iv = tid; iv < nv; iv += LR_THREADS) {
      bf16x8 v = *(const bf16x8*)(xr + 8 * iv);
      const bf16x8 d = *(const bf16x8*)(dr + 8 * iv);
      if (a.delta) {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = (bf16_t)((float)v[j] + (float)d[j]);
      }
      if (a.sum_out && blockIdx.x == 0) *(bf16x8*)(a.sum_out + (int64_t)m * a.ss + 8 * iv) = v;
#pragma unroll
      for (int j = 0; j < 8; ++j) ssq = fmaf((float)v[j], (float)v[j], ssq);
    }
    ssq = wave_sum_dpp(ssq);               // (norms.hip's order of the additions: the same rstd, bit for bit)
    if (lane == 0) red[m][wave] = ssq;
  }
  __syncthreads();
  if (tid < a.M) {
    float tot = 0.f;
#pragma unroll
    for (int i = 0; i < LR_WAVES; ++i) tot += red[tid][i];
    stat[tid] = rsqrtf(tot / (float)a.K + a.eps);
  }
  __syncthreads();
}

// f(x)[0..M)[k0, k0 + kl) -> fx (bf16, rows of a.lds_stride), zero up to `steps` whole steps.  The caller's barriers.
template <int PRO>
__device__ __forceinline__ void rows_fill(const RowsArgs& a, bf16_t* fx, const float* stat, int k0, int kl, int steps) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int PP = steps * (LR_STEP / 8);              // 16-byte pieces of a row of the slice
  const bf16x8 zero = {};
  if constexpr (PRO != PRO_GATED) {
    // LR_FU pieces a thread and round: every request first, the converts and the stores behind them (one round trip to
    // L2 a round, not one a piece).  A round's pieces past the end are the last piece again, request and store (the same
    // value to the same place): no branch, so the requests stay where they are.
    const int total = a.M * PP;
    for (int i0 = tid; i0 < total; i0 += LR_FU * LR_THREADS) {
      bf16x8 v[LR_FU], d[LR_FU];
      NormW wq[LR_FU];
      int mm[LR_FU], kk[LR_FU];
#pragma unroll
      for (int u = 0; u < LR_FU; ++u) {
        const int idx = min(i0 + u * LR_THREADS, total - 1);
        const int m = idx / PP, k = 8 * (idx - m * PP);
        const int kc = k0 + min(k, kl - 8);          // (pieces of the zero tail request the row's last piece again: no branch around a load)
        const bf16_t* xr = a.x + (int64_t)m * a.xs;
        v[u] = *(const bf16x8*)(xr + kc);
        if constexpr (PRO == PRO_RMSNORM) {
          d[u] = *(const bf16x8*)((a.delta ? a.delta + (int64_t)m * a.ds : xr) + kc);
          wq[u] = normw_load(a.norm_w, a.norm_w_f32, kc);
        }
        mm[u] = m, kk[u] = k;
      }
#pragma unroll
      for (int u = 0; u < LR_FU; ++u) {
        {
          bf16x8 o = v[u];
          if constexpr (PRO == PRO_RELU2) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
              const float r = fmaxf((float)o[j], 0.f);
              o[j] = (bf16_t)(r * r);
            }
          } else if constexpr (PRO == PRO_RMSNORM) {
            const float rstd = stat[mm[u]];
            float wv[8];
            normw_get(wq[u], a.norm_w_f32, wv);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
              const bf16_t sm = a.delta ? (bf16_t)((float)o[j] + (float)d[u][j]) : o[j];
              o[j] = (bf16_t)(wv[j] * ((float)sm * rstd));
            }
          }
          *(bf16x8*)(fx + (int64_t)mm[u] * a.lds_stride + kk[u]) = kk[u] < kl ? o : zero;
        }
      }
    }
  } else {
    // a wave per (row, group of the slice): rmsnorm_gated_kernel's arithmetic (norms.hip)
    constexpr int MAXV = 4, GPW = 1;                 // group <= 8 * 64 * 4 (launcher); a second pair in flight spills
    const int ngs = kl / a.group, gv = a.group / 8, npairs = a.M * ngs;
    for (int p0 = wave; p0 < npairs; p0 += GPW * LR_WAVES) {
      bf16x8 xv[GPW][MAXV], zv[GPW][MAXV];
      NormW wq[GPW][MAXV];
#pragma unroll
      for (int i = 0; i < GPW; ++i) {
        const int pr = min(p0 + i * LR_WAVES, npairs - 1), m = pr / ngs, g = pr - m * ngs;
        const bf16_t* xr = a.x + (int64_t)m * a.xs + k0 + (int64_t)g * a.group;
        const bf16_t* zr = a.gate ? a.gate + (int64_t)m * a.gs + k0 + (int64_t)g * a.group : xr;
#pragma unroll
        for (int k = 0; k < MAXV; ++k) {
          const int iv = min(lane + k * 64, gv - 1);
          xv[i][k] = *(const bf16x8*)(xr + 8 * iv);
          zv[i][k] = *(const bf16x8*)(zr + 8 * iv);
          wq[i][k] = normw_load(a.norm_w, a.norm_w_f32, k0 + g * a.group + 8 * iv);
        }
      }
#pragma unroll
      for (int i = 0; i < GPW; ++i) {
        const int pr = p0 + i * LR_WAVES;
        if (pr < npairs) {
          const int m = pr / ngs, g = pr - m * ngs;
          float vals[MAXV][8];
          float ssq = 0.f;
#pragma unroll
          for (int k = 0; k < MAXV; ++k) {
            if (lane + k * 64 < gv) {
#pragma unroll
              for (int j = 0; j < 8; ++j) {
                float f = (float)xv[i][k][j];
                if (a.gate) {
                  const float gt = (float)zv[i][k][j];
                  f *= gt * __builtin_amdgcn_rcpf(1.f + __expf(-gt));
                }
                vals[k][j] = f;
                ssq = fmaf(f, f, ssq);
              }
            }
          }
          ssq = wave_sum_dpp(ssq);               // (norms.hip's order of the additions: the same rstd, bit for bit)
          const float rstd = rsqrtf(ssq / (float)a.group + a.eps);
#pragma unroll
          for (int k = 0; k < MAXV; ++k) {
            const int iv = lane + k * 64;
            if (iv < gv) {
              bf16x8 o;
              float wv[8];
              normw_get(wq[i][k], a.norm_w_f32, wv);
#pragma unroll
              for (int j = 0; j < 8; ++j) o[j] = (bf16_t)(wv[j] * (vals[k][j] * rstd));
              *(bf16x8*)(fx + (int64_t)m * a.lds_stride + (int64_t)g * a.group + 8 * iv) = o;
            }
          }
        }
      }
    }
    const int tail = PP - kl / 8;                    // pieces of zeros behind the last group (last slice only)
    for (int idx = tid; idx < a.M * tail; idx += LR_THREADS) {
      const int m = idx / tail, p = idx - m * tail;
      *(bf16x8*)(fx + (int64_t)m * a.lds_stride + kl + 8 * p) = zero;
    }
  }
}

// TB tiles x SB steps are one batch of loads (4 TB SB load instructions, 16 with TB SB = 4), two batches in flight;
// NG groups of TB tiles a work-group.  Every load of W is unconditional: rows past N, steps past the wave's last and
// pieces past the end of K are clamped to an address inside the operand, and the steady-state loop holds nothing but
// batches of loads and batches of MFMAs, so the waits in front of the MFMAs count the batch behind (vmcnt(N), not 0).
template <int PRO, int TB, int SB, int NG>
__global__ __launch_bounds__(LR_THREADS, 2) void linear_rows_kernel(RowsArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lr_smem[];
  bf16_t* fx = (bf16_t*)lr_smem;                     // [M][lds_stride]; the partial tiles after the last slice
  __shared__ float red[LR_MAXM][LR_WAVES];
  __shared__ float stat[LR_MAXM];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);      // (a scalar: the step loops branch on scalars, not on exec)
  const int r = lane & 15, kq = lane >> 4;
  const int G = gridDim.x, ntiles = (a.N + 15) / 16;

  f32x4 acc[NG][TB];
#pragma unroll
  for (int g = 0; g < NG; ++g)
#pragma unroll
    for (int t = 0; t < TB; ++t) acc[g][t] = f32x4{0.f, 0.f, 0.f, 0.f};

  // the token operand: rows past M - 1 read row M - 1 again (their output columns are not stored)
  const bf16_t* fb = fx + (int64_t)min(r, a.M - 1) * a.lds_stride + kq * 32;

  // the lane's row of the TB tiles of group g (rows past N and tiles past the last: row N - 1 again, not stored)
  auto rows_of = [&](const bf16_t* (&wp)[TB], int g, int k0) __attribute__((always_inline)) {
#pragma unroll
    for (int t = 0; t < TB; ++t) {
      const int n = min((blockIdx.x + (g * TB + t) * G) * 16 + r, a.N - 1);
      wp[t] = a.W + (int64_t)n * a.ldw + k0;
    }
  };
  // one batch.  A step past se - 1 requests step se - 1 again (it is not multiplied); a piece past the end of K requests
  // the row's last piece again and meets the zeros behind f(x) in LDS.
  auto load = [&](bf16x8 (&dst)[TB][SB][4], const bf16_t* const (&wp)[TB], int s, int se, int kl) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < SB; ++i) {
      const int base = min(s + i, se - 1) * LR_STEP, lim = kl - 8 - base;
      int o[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) o[q] = base + min(kq * 32 + q * 8, lim);
#pragma unroll
      for (int t = 0; t < TB; ++t)
#pragma unroll
        for (int q = 0; q < 4; ++q) dst[t][i][q] = ldw8<true>(wp[t] + o[q]);
    }
  };
  auto mma = [&](const bf16x8 (&w)[TB][SB][4], f32x4 (&c)[TB], int s, int se, bool full) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < SB; ++i) {
      if (full || s + i < se) {                      // (wave uniform; `full` is a constant at every call)
        bf16x8 b[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) b[q] = *(const bf16x8*)(fb + (s + i) * LR_STEP + q * 8);
#pragma unroll
        for (int t = 0; t < TB; ++t)
#pragma unroll
          for (int q = 0; q < 4; ++q) c[t] = ssdk::mfma16(w[t][i][q], b[q], c[t]);
      }
    }
  };

  // The elementwise prologues ask for the slice's first batch of W in front of the fill, so that the weight stream does
  // not stand still behind it (gemv.hip does the same); the gated fill needs the registers for its group.
  constexpr bool PREFETCH = PRO != PRO_GATED;
  bf16x8 wa[TB][SB][4], wb[TB][SB][4];
  const bf16_t* wp[TB];
  if constexpr (PRO == PRO_RMSNORM) rows_rms_stats(a, red, stat);

  for (int k0 = 0; k0 < a.K; k0 += a.KS) {
    const int kl = min(a.KS, a.K - k0), steps = (kl + LR_STEP - 1) / LR_STEP;
    const int spw = (steps + LR_WAVES - 1) / LR_WAVES, sb = wave * spw, se = min(steps, sb + spw);
    if constexpr (PREFETCH) {
      rows_of(wp, 0, k0);
      load(wa, wp, sb, max(se, 1), kl);              // (a wave without a step of its own asks for step se - 1 >= 0: inside W)
    }
    if (k0) __syncthreads();                         // (the products of the slice in front are done with fx)
    rows_fill<PRO>(a, fx, stat, k0, kl, steps);
    // vmcnt(0): the gated fill leaves requests behind whose pieces it does not use (lanes past the end of a group); a
    // register of theirs met again in the step loop would put a wait for everything into every iteration.  Nothing else
    // is in flight here but the first batch, asked for in front of the fill.
    __builtin_amdgcn_s_waitcnt(0x0F70);
    __syncthreads();
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      if (blockIdx.x + g * TB * G < ntiles && sb < se) {      // (work-group uniform, wave uniform)
        if (!(PREFETCH && g == 0)) {
          rows_of(wp, g, k0);
          load(wa, wp, sb, se, kl);
        }
        int s = sb;
        for (; s + 2 * SB < se; s += 2 * SB) {       // steady state: both batches whole, a third one behind them
          load(wb, wp, s + SB, se, kl);
          __builtin_amdgcn_sched_barrier(0);         // (keeps a batch's requests in front of the products of the batch before:
          mma(wa, acc[g], s, se, true);              //  the scheduler otherwise gathers both batches and waits for all)
          __builtin_amdgcn_sched_barrier(0);
          load(wa, wp, s + 2 * SB, se, kl);
          __builtin_amdgcn_sched_barrier(0);
          mma(wb, acc[g], s + SB, se, true);
          __builtin_amdgcn_sched_barrier(0);
        }
        if (s + SB < se) {
          load(wb, wp, s + SB, se, kl);
          mma(wa, acc[g], s, se, true);
          mma(wb, acc[g], s + SB, se, false);
        } else {
          mma(wa, acc[g], s, se, false);
        }
      }
    }
  }

  // the four waves' partial tiles meet in LDS and are added in wave order
  __syncthreads();
  f32x4* part = (f32x4*)lr_smem;                     // [NG * TB][LR_WAVES][64]
#pragma unroll
  for (int g = 0; g < NG; ++g)
#pragma unroll
    for (int t = 0; t < TB; ++t) part[((g * TB + t) * LR_WAVES + wave) * 64 + lane] = acc[g][t];
  __syncthreads();
  for (int slot = wave; slot < NG * TB; slot += LR_WAVES) {
    const int tile = blockIdx.x + slot * G;
    if (tile < ntiles && r < a.M) {
      f32x4 v = part[(slot * LR_WAVES + 0) * 64 + lane];
#pragma unroll
      for (int w = 1; w < LR_WAVES; ++w) {
        const f32x4 p = part[(slot * LR_WAVES + w) * 64 + lane];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] += p[j];
      }
      // D of the MFMA: row (lane >> 4) * 4 + j is the row of W, column lane & 15 the token
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int n = tile * 16 + kq * 4 + j;
        if (n < a.N) a.y[(int64_t)r * a.ys + n] = (bf16_t)(v[j] + (a.bias ? (float)a.bias[n] : 0.f));
      }
    }
  }
}

template <int PRO, int TB, int SB, int NG>
int launch_rows_cfg(const RowsArgs& a, int wgs, size_t lds, hipStream_t st) {
  static const hipError_t attr = hipFuncSetAttribute((const void*)linear_rows_kernel<PRO, TB, SB, NG>,
                                                     hipFuncAttributeMaxDynamicSharedMemorySize, LR_LDS);
  if (attr != hipSuccess) {
    tv_set_error("linear_rows: cannot reserve %d KiB of LDS: %s", LR_LDS / 1024, hipGetErrorString(attr));
    return TV_ERR_LAUNCH;
  }
  linear_rows_kernel<PRO, TB, SB, NG><<<dim3((unsigned)wgs), LR_THREADS, lds, st>>>(a);
  TV_LAUNCH_CHECK();
}

template <int PRO>
int launch_rows(RowsArgs& a, hipStream_t st) {
  // a slice of f(x): whole norm groups (gated), else whole steps — four a wave where that many fit
  const int per_row = LR_LDS / (2 * a.M) - LR_PAD;
  if (PRO == PRO_GATED) {
    int g = per_row / a.group;                       // (the slice is stored in whole steps: >= 1 fits, group <= 2048)
    while (g > 1 && (g * a.group + LR_STEP - 1) / LR_STEP * LR_STEP > per_row) --g;
    a.KS = (g < 1 ? 1 : g) * a.group;
  } else {
    a.KS = per_row >= 4 * LR_WAVES * LR_STEP ? per_row / (LR_WAVES * LR_STEP) * (LR_WAVES * LR_STEP) : per_row / LR_STEP * LR_STEP;
  }
  const int longest = a.KS < a.K ? a.KS : a.K;
  a.lds_stride = (longest + LR_STEP - 1) / LR_STEP * LR_STEP + LR_PAD;
  // two work-groups a CU; tiles strided over them, at most LR_MAXT each
  const int ntiles = (a.N + 15) / 16;
  int wgs = 2 * tv_cu_count();
  if (wgs > ntiles) wgs = ntiles;
  // (the gated prologue's operands and 4 or 16 accumulator tiles do not fit 256 registers together: 2 tiles, more work-groups)
  constexpr int MAXT = PRO == PRO_GATED ? 2 : LR_MAXT;
  if ((ntiles + wgs - 1) / wgs > MAXT) wgs = (ntiles + MAXT - 1) / MAXT;
  const int tpw = (ntiles + wgs - 1) / wgs;
  const int slots = tpw <= 1 ? 1 : tpw <= 2 ? 2 : tpw <= 4 ? 4 : LR_MAXT;
  size_t lds = (size_t)a.M * a.lds_stride * sizeof(bf16_t);
  const size_t lds_part = (size_t)slots * LR_WAVES * 64 * sizeof(f32x4);
  if (lds < lds_part) lds = lds_part;
  if (tpw <= 1) return launch_rows_cfg<PRO, 1, 4, 1>(a, wgs, lds, st);
  if constexpr (PRO == PRO_GATED) {
    return launch_rows_cfg<PRO, 2, 2, 1>(a, wgs, lds, st);
  } else {
    if (tpw <= 2) return launch_rows_cfg<PRO, 2, 2, 1>(a, wgs, lds, st);
    if (tpw <= 4) return launch_rows_cfg<PRO, 4, 1, 1>(a, wgs, lds, st);
    return launch_rows_cfg<PRO, 2, 1, 8>(a, wgs, lds, st);    // (16 accumulator tiles: batches of 8 loads keep it within 256 registers)
  }
}
}  // namespace

extern "C" int tv_linear_rows_bf16_fwd(const void* x, const void* W, const void* bias, void* y, int M, int N, int K,
                                       int64_t x_stride, int64_t ldw, int64_t y_stride, int prologue, const void* delta,
                                       int64_t delta_stride, void* sum_out, int64_t sum_stride, const void* norm_weight,
                                       int norm_weight_dtype, float eps, const void* gate, int64_t gate_stride,
                                       int group_size, void* stream) {
  RowsArgs a;
  const int bad = linear_args_fill(a, "linear_rows", LR_MAXM, x, W, bias, y, M, N, K, x_stride, ldw, y_stride, prologue, delta,
                                   delta_stride, sum_out, sum_stride, norm_weight, norm_weight_dtype, eps, gate, gate_stride,
                                   group_size);
  if (bad != TV_OK) return bad;
  a.KS = a.lds_stride = 0;                           // (launch_rows)
  hipStream_t st = (hipStream_t)stream;
  switch (prologue) {
    case PRO_NONE: return launch_rows<PRO_NONE>(a, st);
    case PRO_RMSNORM: return launch_rows<PRO_RMSNORM>(a, st);
    case PRO_RELU2: return launch_rows<PRO_RELU2>(a, st);
    default: return launch_rows<PRO_GATED>(a, st);
  }
}
