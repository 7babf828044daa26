// What the decode-step matrix-vector kernels share (gemv.hip: bf16 weights, gemv_fp8w.hip: e4m3 weights): the arguments,
// the prologue that puts f(x) into LDS with the rounding points of linear_prologue.hpp, the wave reductions and the dev
// switches.  Everything here has internal linkage: each translation unit compiles its own copy.
#pragma once
#include "linear_prologue.hpp"

namespace {

constexpr int GV_THREADS = 256;
constexpr int GV_WAVES = GV_THREADS / 64;
constexpr int GV_MAXM = 4;

typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

struct GemvArgs {
  const bf16_t *x, *W, *bias, *delta, *gate;
  const void* norm_w;
  bf16_t *y, *sum_out;
  int M, N, K, group, norm_w_f32;
  int64_t xs, ldw, ys, ds, ss, gs;
  float eps;
  // epilogue (row-per-wave kernel): rows [conv_lo, conv_hi) of y pass through a width-4 causal-conv update + SiLU
  bf16_t* conv_state;              // (M, conv_hi - conv_lo, 4): shifted left, the new value appended
  const bf16_t *conv_w, *conv_b;   // (channels, 4), (channels) or NULL
  int conv_lo, conv_hi;
};

// sum over the 64 lanes, as a wave-uniform value (DPP row shifts / broadcasts + one readlane: no LDS crossbar)
__device__ __forceinline__ float wave_total(float v) {
  v = ssdk::wave_incl_scan_dpp(v);
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}

__device__ __forceinline__ float dot8(bf16x8 a, bf16x8 b, float acc) {
#pragma unroll
  for (int j = 0; j < 4; ++j)
    acc = __builtin_amdgcn_fdot2_f32_bf16(bf16x2{a[2 * j], a[2 * j + 1]}, bf16x2{b[2 * j], b[2 * j + 1]}, acc, false);
  return acc;
}

// f(x) -> LDS (bf16, [M][K]); ends with a barrier
template <int PRO, typename F>
__device__ __forceinline__ void gemv_prologue(const GemvArgs& a, bf16_t* fx, float* red, F&& after_loads) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int K = a.K, nv = K / 8;
  for (int m = 0; m < a.M; ++m) {
    const bf16_t* xr = a.x + (int64_t)m * a.xs;
    bf16_t* fr = fx + (int64_t)m * K;
    if (PRO == PRO_NONE || PRO == PRO_RELU2) {
      if (m == 0) after_loads();
      for (int iv = tid; iv < nv; iv += GV_THREADS) {
        bf16x8 v = *(const bf16x8*)(xr + 8 * iv);
        if (PRO == PRO_RELU2) {
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const float r = fmaxf((float)v[j], 0.f);
            v[j] = (bf16_t)(r * r);
          }
        }
        *(bf16x8*)(fr + 8 * iv) = v;
      }
    } else if (PRO == PRO_RMSNORM) {
      constexpr int MAXV = 4;                        // K <= 8 * 256 * 4 (PRO_RMSNORM_MAX_K)
      float vals[MAXV][8];
      NormW wq[MAXV];                                // (the weights are requested with x, not behind the reduction)
      float ssq = 0.f;
      bf16x8 xq[MAXV], dq[MAXV];
#pragma unroll
      for (int k = 0; k < MAXV; ++k) {               // (lanes past the end request the last piece again: no branch around a load)
        const int iv = min(tid + k * GV_THREADS, nv - 1);
        wq[k] = normw_load(a.norm_w, a.norm_w_f32, 8 * iv);
        xq[k] = *(const bf16x8*)(xr + 8 * iv);
        dq[k] = *(const bf16x8*)((a.delta ? a.delta + (int64_t)m * a.ds : xr) + 8 * iv);      // (no delta: x again, unused)
      }
      __builtin_amdgcn_sched_barrier(0);
      if (m == 0) after_loads();
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int k = 0; k < MAXV; ++k) {
        const int iv = tid + k * GV_THREADS;
        if (iv < nv) {
          bf16x8 v = xq[k];
          if (a.delta) {
            const bf16x8 d = dq[k];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = (bf16_t)((float)v[j] + (float)d[j]);     // the add rounds to bf16 (:966)
          }
          if (a.sum_out && blockIdx.x == 0) *(bf16x8*)(a.sum_out + (int64_t)m * a.ss + 8 * iv) = v;
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            vals[k][j] = (float)v[j];
            ssq = fmaf(vals[k][j], vals[k][j], ssq);
          }
        }
      }
      ssq = wave_sum(ssq);
      __syncthreads();                               // (red is reused by the next row)
      if (lane == 0) red[wave] = ssq;
      __syncthreads();
      float tot = 0.f;
#pragma unroll
      for (int i = 0; i < GV_WAVES; ++i) tot += red[i];
      const float rstd = rsqrtf(tot / (float)K + a.eps);
#pragma unroll
      for (int k = 0; k < MAXV; ++k) {
        const int iv = tid + k * GV_THREADS;
        if (iv < nv) {
          bf16x8 o;
          float wv[8];
          normw_get(wq[k], a.norm_w_f32, wv);
#pragma unroll
          for (int j = 0; j < 8; ++j) o[j] = (bf16_t)(wv[j] * (vals[k][j] * rstd));
          *(bf16x8*)(fr + 8 * iv) = o;
        }
      }
    } else {                                         // PRO_GATED: a wave per group of `group` channels
      constexpr int MAXV = 4, GPW = 1;               // group <= 8 * 64 * 4 (launcher)
      const int ngroups = K / a.group, gv = a.group / 8;
      if (m == 0 && wave >= ngroups) after_loads();
      for (int g0 = wave; g0 < ngroups; g0 += GPW * GV_WAVES) {
        bf16x8 xv[GPW][MAXV], zv[GPW][MAXV];
        NormW wq[GPW][MAXV];                         // (x, gate and weights of a group are requested together, the first group's in front of W)
#pragma unroll
        for (int i = 0; i < GPW; ++i) {
          const int g = min(g0 + i * GV_WAVES, ngroups - 1);
#pragma unroll
          for (int k = 0; k < MAXV; ++k) {
            const int iv = min(lane + k * 64, gv - 1);
            xv[i][k] = *(const bf16x8*)(xr + (int64_t)g * a.group + 8 * iv);
            zv[i][k] = *(const bf16x8*)((a.gate ? a.gate + (int64_t)m * a.gs : xr) + (int64_t)g * a.group + 8 * iv);
            wq[i][k] = normw_load(a.norm_w, a.norm_w_f32, g * a.group + 8 * iv);
          }
        }
        __builtin_amdgcn_sched_barrier(0);
        if (m == 0 && g0 == wave) after_loads();
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < GPW; ++i) {
          const int g = g0 + i * GV_WAVES;
          if (g < ngroups) {
            float vals[MAXV][8];
            float ssq = 0.f;
#pragma unroll
            for (int k = 0; k < MAXV; ++k) {
              const int iv = lane + k * 64;
              if (iv < gv) {
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
            ssq = wave_sum(ssq);
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
                *(bf16x8*)(fr + (int64_t)g * a.group + 8 * iv) = o;
              }
            }
          }
        }
      }
    }
  }
  __syncthreads();

}

// dev switches (A/B runs): TV_GEMV_NT = 0 plain loads of W; TV_GEMV_WGS = work-groups per CU (default 2)
int gemv_nt() { static const int v = [] { const char* e = getenv("TV_GEMV_NT"); return e ? atoi(e) : 1; }(); return v; }
int gemv_wgs() { static const int v = [] { const char* e = getenv("TV_GEMV_WGS"); return e ? atoi(e) : 2; }(); return v < 1 ? 1 : v; }

}  // namespace
