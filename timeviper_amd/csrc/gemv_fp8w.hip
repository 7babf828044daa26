// Decode-step linear layers on 8-bit weights: y[m][n] = w_scale[n] * sum_k f(x)[m][k] Q[n][k] (+ bias[n]) for M <= 4 rows,
// Q (N, K) in e4m3 (OCP float8_e4m3fn, one byte a weight) with one fp32 scale per output row.
//
// The decode step is bound by the bytes of W (gemv.hip); this is the same product streaming half of them.  A lane's 16-byte
// load now carries 16 weights: v_cvt_scalef32_pk_bf16_fp8 (scale 1.0: every e4m3 value is a bf16 value) turns each pair of
// bytes into the packed bf16 pair v_dot2c_f32_bf16 consumes, so the arithmetic, the fp32 accumulation and f(x) — bf16 in
// LDS, computed by the prologue of gemv_common.hpp with its rounding points — are those of the bf16 kernels; the row
// scale multiplies the finished sum once.  Where the scales are powers of two (kernels.quantize_rows_e4m3) diag(scale) Q is
// itself a bf16 matrix, and this kernel and tv_gemv_bf16_fwd on that matrix differ by the order of the additions only.
// Per 16 bytes of W: 8 conversions (once, shared by the rows of x) + 8 M dot2, against 4 M dot2 for bf16.
// The two routes of gemv.hip: a row of W per wave for K < 8192 (with the conv + SiLU epilogue), split-K for K >= 8192.
#include "gemv_common.hpp"

namespace {

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

struct GemvFp8Args : GemvArgs {                      // (W of the base: the e4m3 bytes, ldw in bytes)
  const float* w_scale;
};

int g_fp8w_calls = 0;

// 16 bytes of Q = 16 weights; NT as ldw8 (linear_prologue.hpp)
template <bool NT>
__device__ __forceinline__ u32x4 ldq16(const unsigned char* p) {
  return NT ? __builtin_nontemporal_load((const u32x4*)p) : *(const u32x4*)p;
}

// the 16 weights of a piece as 8 bf16 pairs, in the order of k (byte j of the piece is weight j)
__device__ __forceinline__ void cvt16(u32x4 q, bf16x2 (&w)[8]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    w[2 * j] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(q[j], 1.0f, false);
    w[2 * j + 1] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(q[j], 1.0f, true);
  }
}

__device__ __forceinline__ float dot16(const bf16x2 (&w)[8], bf16x8 x0, bf16x8 x1, float acc) {
#pragma unroll
  for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_fdot2_f32_bf16(w[j], bf16x2{x0[2 * j], x0[2 * j + 1]}, acc, false);
#pragma unroll
  for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_fdot2_f32_bf16(w[4 + j], bf16x2{x1[2 * j], x1[2 * j + 1]}, acc, false);
  return acc;
}

// Split-K (K >= 8 192): gemv_bf16_kernel of gemv.hip on pieces of 16 weights.  A work-group owns whole rows of Q, its four
// waves split K and meet in LDS every GB row groups; R rows at a time, NB load instructions per row and batch.
template <int PRO, int MT, int R, int NB, bool NT, bool PF>
__global__ __launch_bounds__(GV_THREADS) void gemv_fp8w_kernel(GemvFp8Args a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char gv_smem[];
  bf16_t* fx = (bf16_t*)gv_smem;                     // [M][K]
  __shared__ float red[GV_WAVES];
  constexpr int GB = 4;                              // row groups between two meetings of the waves
  __shared__ float part[2][GB][GV_WAVES][R][MT];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int K = a.K, nv = K / 16;
  const unsigned char* Q = (const unsigned char*)a.W;

  // this wave's share of K: 16-byte pieces [p0, p0 + np) of every row, 64 per load instruction
  const int G = gridDim.x;
  const int pw = (nv + GV_WAVES - 1) / GV_WAVES, p0 = wave * pw;
  const int np = min(nv - p0, pw);                   // (<= 0: nothing for this wave)
  const int nins = np > 0 ? (np + 63) / 64 : 0;
  auto load_batch = [&](u32x4 (&dst)[NB][R], int n0, int i0) __attribute__((always_inline)) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
      if (n0 + r * G < a.N) {                        // (work-group uniform)
        const unsigned char* wp = Q + (int64_t)(n0 + r * G) * a.ldw + 16 * (p0 + lane);
#pragma unroll
        for (int u = 0; u < NB; ++u) {
          const u32x4 z = {};
          dst[u][r] = 64 * (i0 + u) + lane < np ? ldq16<NT>(wp + 1024 * (i0 + u)) : z;
        }
      }
    }
  };
  u32x4 cur[NB][R];
  // the requests for the first rows of Q go out BEHIND those for the prologue's operands (a wave's loads return in order)
  gemv_prologue<PRO>(a, fx, red, [&]() __attribute__((always_inline)) { if ((int)blockIdx.x < a.N) load_batch(cur, blockIdx.x, 0); });

  const bf16_t* fl = fx + 16 * (p0 + lane);
  int par = 0, gi = 0, nflush = blockIdx.x;          // gi: groups since the last meeting; nflush: first row of the first of them
  for (int n0 = blockIdx.x; n0 < a.N; n0 += R * G) {
    float acc[R][MT];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int m = 0; m < MT; ++m) acc[r][m] = 0.f;
    auto fma_batch = [&](const u32x4 (&w)[NB][R], int i0) __attribute__((always_inline)) {
#pragma unroll
      for (int u = 0; u < NB; ++u)
        if (64 * (i0 + u) + lane < np) {
          bf16x2 wc[R][8];
#pragma unroll
          for (int r = 0; r < R; ++r)
            if (n0 + r * G < a.N) cvt16(w[u][r], wc[r]);
#pragma unroll
          for (int m = 0; m < MT; ++m)
            if (MT == 1 || m < a.M) {
              const bf16_t* xp = fl + (int64_t)m * K + 1024 * (i0 + u);
              const bf16x8 x0 = *(const bf16x8*)xp, x1 = *(const bf16x8*)(xp + 8);
#pragma unroll
              for (int r = 0; r < R; ++r)
                if (n0 + r * G < a.N) acc[r][m] = dot16(wc[r], x0, x1, acc[r][m]);
            }
        }
    };
    const bool more = n0 + R * G < a.N;
    u32x4 nxt[PF ? NB : 1][PF ? R : 1];
    if constexpr (PF) {
      if (more) load_batch(nxt, n0 + R * G, 0);
    } else {
      if (n0 != (int)blockIdx.x) load_batch(cur, n0, 0);
    }
    fma_batch(cur, 0);
    for (int i0 = NB; i0 < nins; i0 += NB) {
      u32x4 wv[NB][R];
      load_batch(wv, n0, i0);
      fma_batch(wv, i0);
    }
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int m = 0; m < MT; ++m) {
        const float sm = wave_total(acc[r][m]);
        if (lane == 0) part[par][gi][wave][r][m] = sm;
      }
    if (++gi == GB || !more) {
      __syncthreads();
      for (int i = tid; i < gi * R * MT; i += GV_THREADS) {
        const int j = i / (R * MT), r = (i / MT) % R, m = i % MT, n = nflush + (j * R + r) * G;
        if (n < a.N && (MT == 1 || m < a.M)) {
          float sm = 0.f;
#pragma unroll
          for (int w = 0; w < GV_WAVES; ++w) sm += part[par][j][w][r][m];
          a.y[(int64_t)m * a.ys + n] = (bf16_t)(sm * a.w_scale[n] + (a.bias ? (float)a.bias[n] : 0.f));
        }
      }
      par ^= 1; gi = 0; nflush = n0 + R * G;
    }
    if constexpr (PF) {
      if (more) {
#pragma unroll
        for (int u = 0; u < NB; ++u)
#pragma unroll
          for (int r = 0; r < R; ++r) cur[u][r] = nxt[u][r];
      }
    }
  }
}

// A ROW of Q per wave (K < 8 192): gemv_rows_kernel of gemv.hip on pieces of 16 weights, R rows at a time, with its
// width-4 conv + SiLU epilogue.  A row of K = 4 480 is 5 load instructions where the bf16 row is 9.
template <int PRO, int MT, bool NT, int R, int NB>
__global__ __launch_bounds__(GV_THREADS) void gemv_fp8w_rows_kernel(GemvFp8Args a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char gv_smem[];
  bf16_t* fx = (bf16_t*)gv_smem;                     // [M][K]
  __shared__ float red[GV_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int K = a.K, nv = K / 16;
  const unsigned char* Q = (const unsigned char*)a.W;
  const int TW = gridDim.x * GV_WAVES, gw = blockIdx.x * GV_WAVES + wave;
  const int nins = (nv + 63) / 64;
  auto load_batch = [&](u32x4 (&dst)[NB][R], int n0, int i0) __attribute__((always_inline)) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
      if (n0 + r * TW < a.N) {                       // (wave uniform)
        const unsigned char* wp = Q + (int64_t)(n0 + r * TW) * a.ldw + 16 * lane;
#pragma unroll
        for (int u = 0; u < NB; ++u) {
          const u32x4 z = {};
          dst[u][r] = 64 * (i0 + u) + lane < nv ? ldq16<NT>(wp + 1024 * (i0 + u)) : z;
        }
      }
    }
  };
  u32x4 cur[NB][R];
  // in flight while the prologue runs, requested behind the prologue's own operands (a wave's loads return in order)
  gemv_prologue<PRO>(a, fx, red, [&]() __attribute__((always_inline)) { if (gw < a.N) load_batch(cur, gw, 0); });

  const bf16_t* fl = fx + 16 * lane;
  for (int n0 = gw; n0 < a.N; n0 += R * TW) {
    float acc[R][MT];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int m = 0; m < MT; ++m) acc[r][m] = 0.f;
    auto fma_batch = [&](const u32x4 (&w)[NB][R], int i0) __attribute__((always_inline)) {
#pragma unroll
      for (int u = 0; u < NB; ++u)
        if (64 * (i0 + u) + lane < nv) {
          bf16x2 wc[R][8];
#pragma unroll
          for (int r = 0; r < R; ++r)
            if (n0 + r * TW < a.N) cvt16(w[u][r], wc[r]);
#pragma unroll
          for (int m = 0; m < MT; ++m)
            if (MT == 1 || m < a.M) {
              const bf16_t* xp = fl + (int64_t)m * K + 1024 * (i0 + u);
              const bf16x8 x0 = *(const bf16x8*)xp, x1 = *(const bf16x8*)(xp + 8);
#pragma unroll
              for (int r = 0; r < R; ++r)
                if (n0 + r * TW < a.N) acc[r][m] = dot16(wc[r], x0, x1, acc[r][m]);
            }
        }
    };
    if (n0 != gw) load_batch(cur, n0, 0);
    // lane r finishes row r of the group; its scale, bias and conv-update operands are requested now, behind the loads of Q
    const int nmine = n0 + min(lane, R - 1) * TW;
    const bool mine = lane < R && nmine < a.N;
    const bool conv_mine = MT == 1 && a.conv_state && mine && nmine >= a.conv_lo && nmine < a.conv_hi;
    const float sc = mine ? a.w_scale[nmine] : 0.f;
    bf16x4 c_old = {}, c_w = {};
    float c_b = 0.f;
    if (conv_mine) {
      const int c = nmine - a.conv_lo;
      c_old = *(const bf16x4*)(a.conv_state + (int64_t)c * 4);
      c_w = *(const bf16x4*)(a.conv_w + (int64_t)c * 4);
      if (a.conv_b) c_b = (float)a.conv_b[c];
    }
    fma_batch(cur, 0);
    for (int i0 = NB; i0 < nins; i0 += NB) {
      load_batch(cur, n0, i0);
      fma_batch(cur, i0);
    }
    float tot[R][MT];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int m = 0; m < MT; ++m) tot[r][m] = (MT == 1 || m < a.M) ? wave_total(acc[r][m]) : 0.f;
    if (mine) {
      const float bs = a.bias ? (float)a.bias[nmine] : 0.f;
#pragma unroll
      for (int m = 0; m < MT; ++m)
        if (MT == 1 || m < a.M) {
          float v = tot[0][m];
#pragma unroll
          for (int r = 1; r < R; ++r) v = lane == r ? tot[r][m] : v;
          bf16_t out = (bf16_t)(v * sc + bs);
          if (a.conv_state && nmine >= a.conv_lo && nmine < a.conv_hi) {
            // tv_causal_conv1d_update on this channel, with its arithmetic (conv1d.hip): window = state[1..3], out
            const int c = nmine - a.conv_lo;
            bf16_t* st = a.conv_state + ((int64_t)m * (a.conv_hi - a.conv_lo) + c) * 4;
            bf16x4 old = c_old, wv = c_w;
            float acc_c = c_b;
            if (MT != 1) {                           // (several rows of x: loaded here)
              old = *(const bf16x4*)st;
              wv = *(const bf16x4*)(a.conv_w + (int64_t)c * 4);
              acc_c = a.conv_b ? (float)a.conv_b[c] : 0.f;
            }
            const bf16x4 win = {old[1], old[2], old[3], out};
#pragma unroll
            for (int j = 0; j < 4; ++j) acc_c = fmaf((float)wv[j], (float)win[j], acc_c);
            *(bf16x4*)st = win;
            out = (bf16_t)silu_f(acc_c);
          }
          a.y[(int64_t)m * a.ys + nmine] = out;
        }
    }
  }
}

// dev switch (A/B runs): TV_FP8W_ROWS_R = rows of Q a wave of the row-per-wave kernel holds at a time, 2 (default) or 4.
// 4 keeps bf16's 20 loads a wave in flight with rows of half the bytes, and measured 0 - 18 % SLOWER on every role
// (profiles/fp8w_decode.json): the stream is not short of requests in flight.
int fp8w_rows_r() { static const int v = [] { const char* e = getenv("TV_FP8W_ROWS_R"); return e ? atoi(e) : 2; }(); return v == 4 ? 4 : 2; }

template <typename Kern>
int fp8w_reserve_lds(Kern kern) {
  const hipError_t attr = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024);
  if (attr != hipSuccess) {
    tv_set_error("gemv_fp8w: cannot reserve 128 KiB of LDS: %s", hipGetErrorString(attr));
    return TV_ERR_LAUNCH;
  }
  return TV_OK;
}
template <int PRO, int MT, int R, int NB, bool NT, bool PF>
int launch_fp8w_splitk(const GemvFp8Args& a, hipStream_t st) {
  static const int ok = fp8w_reserve_lds(gemv_fp8w_kernel<PRO, MT, R, NB, NT, PF>);
  if (ok != TV_OK) return ok;
  const size_t lds = (size_t)a.M * a.K * sizeof(bf16_t);
  int wgs = (a.N + R - 1) / R;                       // two work-groups per CU; fewer when there are not R rows for each
  const int most = gemv_wgs() * tv_cu_count();
  if (wgs > most) wgs = most;
  ++g_fp8w_calls;
  gemv_fp8w_kernel<PRO, MT, R, NB, NT, PF><<<dim3((unsigned)wgs), GV_THREADS, lds, st>>>(a);
  TV_LAUNCH_CHECK();
}
template <int PRO, int MT, bool NT, int R, int NB>
int launch_fp8w_rows(const GemvFp8Args& a, hipStream_t st) {
  static const int ok = fp8w_reserve_lds(gemv_fp8w_rows_kernel<PRO, MT, NT, R, NB>);
  if (ok != TV_OK) return ok;
  const size_t lds = (size_t)a.M * a.K * sizeof(bf16_t);
  int wgs = (a.N + R * GV_WAVES - 1) / (R * GV_WAVES);            // >= one row group per wave, two work-groups per CU
  const int most = gemv_wgs() * tv_cu_count();
  if (wgs > most) wgs = most;
  ++g_fp8w_calls;
  gemv_fp8w_rows_kernel<PRO, MT, NT, R, NB><<<dim3((unsigned)wgs), GV_THREADS, lds, st>>>(a);
  TV_LAUNCH_CHECK();
}
template <int PRO, int MT, bool NT>
int launch_fp8w_nt(const GemvFp8Args& a, hipStream_t st) {
  // (the conv epilogue is built into the row-per-wave kernel; the entry point refuses it for K >= 8192)
  constexpr bool PF = PRO != PRO_GATED;              // as gemv.hip: the gated prologue's operands leave no room for a second set of rows
  if (a.K >= 8192) return launch_fp8w_splitk<PRO, MT, 2, 4, NT, PF>(a, st);
  return fp8w_rows_r() == 2 ? launch_fp8w_rows<PRO, MT, NT, 2, 5>(a, st) : launch_fp8w_rows<PRO, MT, NT, 4, 5>(a, st);
}
template <int PRO>
int launch_fp8w(const GemvFp8Args& a, hipStream_t st) {
  if (a.M == 1) return gemv_nt() ? launch_fp8w_nt<PRO, 1, true>(a, st) : launch_fp8w_nt<PRO, 1, false>(a, st);
  return gemv_nt() ? launch_fp8w_nt<PRO, GV_MAXM, true>(a, st) : launch_fp8w_nt<PRO, GV_MAXM, false>(a, st);
}

}  // namespace

extern "C" int tv_gemv_fp8w_calls(void) { return g_fp8w_calls; }

extern "C" int tv_gemv_fp8w_fwd(const void* x, const void* W, const void* w_scale, const void* bias, void* y, int M, int N,
                                int K, int64_t x_stride, int64_t ldw, int64_t y_stride, int prologue, const void* delta,
                                int64_t delta_stride, void* sum_out, int64_t sum_stride, const void* norm_weight,
                                int norm_weight_dtype, float eps, const void* gate, int64_t gate_stride,
                                int group_size, void* conv_state, const void* conv_weight, const void* conv_bias,
                                int conv_row0, int conv_channels, void* stream) {
  GemvFp8Args a;
  TV_CHECK_ARG(w_scale, "gemv_fp8w: null pointer (w_scale)");
  if (K % 16 || ldw % 16) TV_UNSUPPORTED("gemv_fp8w: K %d and the row stride of W %lld must be multiples of 16", K, (long long)ldw);
  const int bad = linear_args_fill(a, "gemv_fp8w", GV_MAXM, x, W, bias, y, M, N, K, x_stride, ldw, y_stride, prologue, delta, delta_stride,
                                   sum_out, sum_stride, norm_weight, norm_weight_dtype, eps, gate, gate_stride, group_size);
  if (bad != TV_OK) return bad;
  if ((size_t)M * K * 2 > 128 * 1024) TV_UNSUPPORTED("gemv_fp8w: M x K = %d x %d does not fit the 128 KiB of LDS f(x) is held in", M, K);
  if ((uintptr_t)w_scale & 3) TV_UNSUPPORTED("gemv_fp8w: w_scale must be 4-byte aligned fp32");
  a.w_scale = (const float*)w_scale;
  a.conv_state = nullptr; a.conv_w = a.conv_b = nullptr; a.conv_lo = a.conv_hi = 0;
  if (conv_state) {
    TV_CHECK_ARG(conv_weight && conv_row0 >= 0 && conv_channels > 0 && conv_row0 + conv_channels <= N,
                 "gemv_fp8w: conv epilogue rows [%d, %d) outside the %d outputs", conv_row0, conv_row0 + conv_channels, N);
    if (K >= 8192) TV_UNSUPPORTED("gemv_fp8w: the conv epilogue is built into the row-per-wave kernel (K < 8192)");
    if (((uintptr_t)conv_state & 7) || ((uintptr_t)conv_weight & 7)) TV_UNSUPPORTED("gemv_fp8w: conv state / weight must be 8-byte aligned");
    a.conv_state = (bf16_t*)conv_state; a.conv_w = (const bf16_t*)conv_weight; a.conv_b = (const bf16_t*)conv_bias;
    a.conv_lo = conv_row0; a.conv_hi = conv_row0 + conv_channels;
  }
  hipStream_t st = (hipStream_t)stream;
  switch (prologue) {
    case PRO_NONE: return launch_fp8w<PRO_NONE>(a, st);
    case PRO_RMSNORM: return launch_fp8w<PRO_RMSNORM>(a, st);
    case PRO_RELU2: return launch_fp8w<PRO_RELU2>(a, st);
    default: return launch_fp8w<PRO_GATED>(a, st);
  }
}
