// S3 (generic path): Mamba-2 selective scan as the exact fp32 token recurrence
//   S_t = exp(dt_t A_h) S_{t-1} + dt_t x_t (x) B_t ;  y_t = S_t . C_t + D_h x_t
// for any dtype / head_dim / d_state (BASELINE config 1: fp32, N=16).  One
// workgroup owns (batch, head, 16 columns of P); a thread owns one column and
// every 16th state index n, keeps its state slice in registers for the whole
// sequence, and the 16 n-lanes of a column reduce y with DPP shuffles.  Token
// tiles are staged through LDS with coalesced loads.  The bf16 Nano-shape fast
// paths are the MFMA marches of ssd_head.hip / ssd_slice.hip; small d_state with a
// workspace goes to the chunk-parallel form in ssd_chunked.hip.
// Reference semantics: modeling_nano.py:639-653, CPU twin :775-851.
#include <type_traits>
#include "common.hpp"

namespace {

constexpr int GS_TT = 32;    // tokens staged per tile
constexpr int GS_PB = 16;    // P columns per workgroup
constexpr int GS_NL = 16;    // n-lanes per column
constexpr int GS_THREADS = GS_PB * GS_NL;

struct SsdArgs {
  const void *x, *dt, *Bm, *Cm;
  const float *A, *D, *dt_bias, *init;
  void* y;
  float *final_state, *total_decay;
  int L, H, P, G, N;
  int64_t xsb, xsl, dsb, dsl, bsb, bsl, bsg, csb, csl, csg, ysb, ysl;
  int softplus, group_map;
  float dt_min, dt_max;
};

template <typename T, int NPT>
__global__ __launch_bounds__(GS_THREADS) void ssd_generic_kernel(SsdArgs a) {
  extern __shared__ float smem[];
  const int N = a.N;
  float* sB = smem;                    // [TT][N]
  float* sC = sB + GS_TT * N;          // [TT][N]
  float* sX = sC + GS_TT * N;          // [TT][PB]
  float* sY = sX + GS_TT * GS_PB;      // [TT][PB]
  float* sDt = sY + GS_TT * GS_PB;     // [TT]
  float* sDa = sDt + GS_TT;            // [TT]

  const int pb = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
  const int tid = threadIdx.x;
  const int pl = tid / GS_NL, nl = tid % GS_NL;
  const int p = pb * GS_PB + pl;
  const int g = a.group_map ? (h % a.G) : (h / (a.H / a.G));
  const float Ah = a.A[h];
  const float Dh = a.D ? a.D[h] : 0.f;
  const float bias = a.dt_bias ? a.dt_bias[h] : 0.f;

  const T* xb = (const T*)a.x + (int64_t)b * a.xsb + (int64_t)h * a.P;
  const T* dtb = (const T*)a.dt + (int64_t)b * a.dsb + h;
  const T* Bb = (const T*)a.Bm + (int64_t)b * a.bsb + (int64_t)g * a.bsg;
  const T* Cb = (const T*)a.Cm + (int64_t)b * a.csb + (int64_t)g * a.csg;
  T* yb = (T*)a.y + (int64_t)b * a.ysb + (int64_t)h * a.P;

  float s[NPT];
#pragma unroll
  for (int j = 0; j < NPT; ++j) {
    const int n = nl + GS_NL * j;
    s[j] = (a.init && p < a.P && n < N)
               ? a.init[(((int64_t)b * a.H + h) * a.P + p) * N + n] : 0.f;
  }
  float decay_sum = 0.f;

  for (int t0 = 0; t0 < a.L; t0 += GS_TT) {
    const int tt = min(GS_TT, a.L - t0);
    __syncthreads();
    for (int i = tid; i < tt * N; i += GS_THREADS) {
      const int t = i / N, n = i % N;
      sB[i] = to_f32(Bb[(int64_t)(t0 + t) * a.bsl + n]);
      sC[i] = to_f32(Cb[(int64_t)(t0 + t) * a.csl + n]);
    }
    for (int i = tid; i < tt * GS_PB; i += GS_THREADS) {
      const int t = i / GS_PB, c = pb * GS_PB + i % GS_PB;
      sX[i] = c < a.P ? to_f32(xb[(int64_t)(t0 + t) * a.xsl + c]) : 0.f;
    }
    if (tid < tt) {
      float d = to_f32(dtb[(int64_t)(t0 + tid) * a.dsl]) + bias;
      if (a.softplus) d = softplus_f(d);
      d = fminf(fmaxf(d, a.dt_min), a.dt_max);
      sDt[tid] = d;
      sDa[tid] = d * Ah;
    }
    __syncthreads();
    for (int t = 0; t < tt; ++t) {
      const float dtv = sDt[t];
      const float da = sDa[t];
      const float dec = expf(da);
      const float xr = sX[t * GS_PB + pl];
      const float xv = dtv * xr;
      float acc = 0.f;
#pragma unroll
      for (int j = 0; j < NPT; ++j) {
        const int n = nl + GS_NL * j;
        if (n < N) {
          s[j] = fmaf(dec, s[j], xv * sB[t * N + n]);
          acc = fmaf(s[j], sC[t * N + n], acc);
        }
      }
      acc += __shfl_xor(acc, 8, 64);
      acc += __shfl_xor(acc, 4, 64);
      acc += __shfl_xor(acc, 2, 64);
      acc += __shfl_xor(acc, 1, 64);
      if (nl == 0) sY[t * GS_PB + pl] = fmaf(Dh, xr, acc);
      decay_sum += da;
    }
    __syncthreads();
    for (int i = tid; i < tt * GS_PB; i += GS_THREADS) {
      const int t = i / GS_PB, c = pb * GS_PB + i % GS_PB;
      if (c < a.P) yb[(int64_t)(t0 + t) * a.ysl + c] = from_f32<T>(sY[i]);
    }
  }
  if (a.final_state && p < a.P) {
#pragma unroll
    for (int j = 0; j < NPT; ++j) {
      const int n = nl + GS_NL * j;
      if (n < N) a.final_state[(((int64_t)b * a.H + h) * a.P + p) * N + n] = s[j];
    }
  }
  if (a.total_decay && pb == 0 && tid == 0) a.total_decay[(int64_t)b * a.H + h] = decay_sum;
}

template <typename T>
int launch_generic(const SsdArgs& a, int B, hipStream_t st) {
  const int npt = (a.N + GS_NL - 1) / GS_NL;
  dim3 grid((a.P + GS_PB - 1) / GS_PB, a.H, B);
  const size_t lds = (size_t)(2 * GS_TT * a.N + 2 * GS_TT * GS_PB + 2 * GS_TT) * sizeof(float);
#define TV_GS_CASE(NP)                                                                \
  if (npt <= NP) {                                                                    \
    ssd_generic_kernel<T, NP><<<grid, GS_THREADS, lds, st>>>(a);                      \
    TV_LAUNCH_CHECK();                                                                \
  }
  TV_GS_CASE(1)
  TV_GS_CASE(2)
  TV_GS_CASE(4)
  TV_GS_CASE(8)
  TV_GS_CASE(16)
#undef TV_GS_CASE
  TV_UNSUPPORTED("ssd_scan: d_state %d > 256", a.N);
}

// ---------------------------------------------------------------- decode
template <typename T>
__global__ void state_update_kernel(float* __restrict__ state, const T* __restrict__ x,
                                    const T* __restrict__ dt, const float* __restrict__ A,
                                    const T* __restrict__ Bm, const T* __restrict__ Cm,
                                    const float* __restrict__ D, const float* __restrict__ dt_bias,
                                    T* __restrict__ y, int H, int P, int G, int N, int softplus) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  const int h = blockIdx.y, b = blockIdx.z;
  if (p >= P) return;
  const int g = h / (H / G);
  float d = to_f32(dt[(int64_t)b * H + h]) + (dt_bias ? dt_bias[h] : 0.f);
  if (softplus) d = softplus_f(d);
  const float dec = expf(d * A[h]);
  const float xr = to_f32(x[((int64_t)b * H + h) * P + p]);
  const float xv = d * xr;
  float* s = state + (((int64_t)b * H + h) * P + p) * N;
  const T* Br = Bm + ((int64_t)b * G + g) * N;
  const T* Cr = Cm + ((int64_t)b * G + g) * N;
  float acc = 0.f;
  for (int n = 0; n < N; ++n) {
    const float v = fmaf(dec, s[n], xv * to_f32(Br[n]));
    s[n] = v;
    acc = fmaf(v, to_f32(Cr[n]), acc);
  }
  y[((int64_t)b * H + h) * P + p] = from_f32<T>(fmaf(D ? D[h] : 0.f, xr, acc));
}

// Decode step for d_state = 4 LPR (16 .. 256): LPR lanes share a state row (16 bytes = 4 fp32 each), a wave covers
// 64 / LPR rows per load — coalesced 512-byte rows instead of one thread walking its row with 4-byte loads at a 512-byte
// lane stride (36.7 us for the 2 x 5.2 MB of a Nano layer, round 4).  The launch is a latency chain, not a stream (a Nano
// layer is 10 240 rows = 5.2 MB, 20 KB a CU; an empty launch of this grid inside the decode graph takes 1.85 us):
// round 6 keeps ONE state row per lane group in flight per wave (5 120 waves; two and four rows a wave measured 4.7 and
// 5.6 us against 4.3), requests every scalar of the row (dt, dt_bias, A, D, x) and its B / C pieces in front of the state,
// reads and writes the state non-temporally (nothing re-reads it before the next token, 16.6 GB of weights later) and sums
// over d_state on DPP (row_shr inside a 16-lane row, row_bcast across rows: the group's last lane holds the sum) instead
// of five ds_bpermute round trips: 5.5 -> 4.3 us a launch back to back in a graph (devtools/bench_ssu.py), 7.9 -> 5.2 us
// inside the decode step.
template <int LPR>
__device__ __forceinline__ float group_sum_dpp(float v) {      // valid in the last lane of every LPR-lane group
  if (LPR >= 2) v = tv_dpp_add<0x111, 0xf>(v);                  // row_shr:1
  if (LPR >= 4) v = tv_dpp_add<0x112, 0xf>(v);                  // row_shr:2
  if (LPR >= 8) v = tv_dpp_add<0x114, 0xf>(v);                  // row_shr:4
  if (LPR >= 16) v = tv_dpp_add<0x118, 0xf>(v);                 // row_shr:8
  if (LPR >= 32) v = tv_dpp_add<0x142, 0xa>(v);                 // row_bcast:15 -> rows 1, 3
  if (LPR >= 64) v = tv_dpp_add<0x143, 0xc>(v);                 // row_bcast:31 -> rows 2, 3
  return v;
}

template <typename T, int LPR>
__global__ __launch_bounds__(256) void state_update_chain_kernel(float* __restrict__ state, const T* __restrict__ x,
                                                                        const T* __restrict__ dt, const float* __restrict__ A,
                                                                        const T* __restrict__ Bm, const T* __restrict__ Cm,
                                                                        const float* __restrict__ D,
                                                                        const float* __restrict__ dt_bias, T* __restrict__ y,
                                                                        int H, int P, int G, int softplus, int rows_total) {
  constexpr int N = 4 * LPR, RPW = 64 / LPR, IT = 1, WAVES = 4;      // IT: state rows per lane group in flight
  typedef typename std::conditional<std::is_same<T, float>::value, f32x4, typename std::conditional<std::is_same<T, bf16_t>::value, bf16x4, f16x4>::type>::type vec4_t;
  const int lane = threadIdx.x & 63;
  const int w = (int)blockIdx.x * WAVES + (threadIdx.x >> 6);
  const int sub = lane / LPR, ln = lane % LPR;
  const int hpg = H / G;
  int row[IT];
  f32x4 sv[IT];
  float dtv[IT], xr[IT], av[IT], bv[IT], dv[IT];
  vec4_t Bv[IT], Cv[IT];
#pragma unroll
  for (int it = 0; it < IT; ++it) {
    row[it] = (w * IT + it) * RPW + sub;                // (b, h, p) flattened
    const int rc = row[it] < rows_total ? row[it] : rows_total - 1;
    const int bh = (int)((unsigned)rc / (unsigned)P);
    const int b = (int)((unsigned)bh / (unsigned)H);
    const int h = bh - b * H;
    const int g = (int)((unsigned)h / (unsigned)hpg);
    sv[it] = __builtin_nontemporal_load((const f32x4*)(state + (int64_t)rc * N) + ln);
    dtv[it] = to_f32(dt[bh]);
    xr[it] = to_f32(x[rc]);
    av[it] = A[h];
    bv[it] = dt_bias ? dt_bias[h] : 0.f;
    dv[it] = D ? D[h] : 0.f;
    Bv[it] = *(const vec4_t*)(Bm + (int64_t)(b * G + g) * N + 4 * ln);
    Cv[it] = *(const vec4_t*)(Cm + (int64_t)(b * G + g) * N + 4 * ln);
  }
#pragma unroll
  for (int it = 0; it < IT; ++it) {
    const bool ok = row[it] < rows_total;
    float d = dtv[it] + bv[it];
    if (softplus) d = softplus_f(d);
    const float dec = expf(d * av[it]);
    const float xv = d * xr[it];
    float part = 0.f;
    f32x4 v;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      v[i] = fmaf(dec, sv[it][i], xv * to_f32(Bv[it][i]));
      part = fmaf(v[i], to_f32(Cv[it][i]), part);
    }
    if (ok) __builtin_nontemporal_store(v, (f32x4*)(state + (int64_t)row[it] * N) + ln);
    part = group_sum_dpp<LPR>(part);
    if (ok && ln == LPR - 1) y[row[it]] = from_f32<T>(fmaf(dv[it], xr[it], part));
  }
}

// ---------------------------------------------------------------- continuation: T tokens against a resident state
// The token recurrence of state_update_chain_kernel over T tokens of one launch (a continuation of a prefilled cache:
// a follow-up question, a tool result, a draft to verify).  Same lane layout (LPR lanes share a row, 16 bytes each) and,
// per token, the same arithmetic at the same rounding points — but the row is loaded once, stays in the lanes' registers
// over the T tokens and is stored once: 2 x 5.2 MB a Nano layer whatever T is, against T x that for T launches.  What
// streams per token is small (dt and x of the row, the lane's 4 entries of B and C: the rows of a head group read the
// same B / C lines out of L2) and is requested SQ_PF tokens ahead of its use, a batch of tokens at a time.
struct SeqArgs {
  float* state;
  const void *x, *dt, *Bm, *Cm;
  const float *A, *D, *dt_bias;
  void* y;
  int T, H, P, G, N;
  int64_t xsb, xsl, dsb, dsl, bsb, bsl, bsg, csb, csl, csg, ysb, ysl;
  int softplus, group_map, rows_total;
  float dt_min, dt_max;
};

constexpr int SQ_PF = 4;      // tokens whose operands are in flight while the previous SQ_PF are computed

// dt of a token as the recurrence uses it — one definition for every kernel below, so that a state carried by one of them
// and a state carried by another agree bit for bit
__device__ __forceinline__ float seq_dt(float raw, float bias, int softplus, float dt_min, float dt_max) {
  float d = raw + bias;
  if (softplus) d = softplus_f(d);
  return fminf(fmaxf(d, dt_min), dt_max);
}

// One token of the recurrence on a lane's 4 state entries.  WITH_Y: also the lane's part of y (before the sum over the
// row's lanes); without it (the commit phase of the speculative kernel) C is never touched and its loads fold away.
template <bool WITH_Y, typename V4>
__device__ __forceinline__ float seq_token_step(f32x4& sv, float d, float av, float xr, const V4& Bv, const V4& Cv) {
  const float dec = expf(d * av);
  const float xv = d * xr;
  float part = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    sv[i] = fmaf(dec, sv[i], xv * to_f32(Bv[i]));
    if (WITH_Y) part = fmaf(sv[i], to_f32(Cv[i]), part);
  }
  return part;
}

template <typename T, typename V4>
struct SeqBatch {
  T dt[SQ_PF], x[SQ_PF];
  V4 B[SQ_PF], C[SQ_PF];
};

// the per-row operand pointers of one token run (lane's piece of B / C, the row's x and dt) and their token strides
template <typename T>
struct SeqRun {
  const T *xp, *dp, *Bp, *Cp;
  int64_t xsl, dsl, bsl, csl;
};

struct SeqOps {               // one set of token operands as the entry points take them
  const void *x, *dt, *Bm, *Cm;
  int64_t xsb, xsl, dsb, dsl, bsb, bsl, bsg, csb, csl, csg;
};

template <typename T>
__device__ __forceinline__ SeqRun<T> seq_run_of(const SeqOps& o, int b, int h, int p, int g, int P, int ln4) {
  SeqRun<T> r;
  r.xp = (const T*)o.x + (int64_t)b * o.xsb + (int64_t)h * P + p;
  r.dp = (const T*)o.dt + (int64_t)b * o.dsb + h;
  r.Bp = (const T*)o.Bm + (int64_t)b * o.bsb + (int64_t)g * o.bsg + ln4;
  r.Cp = (const T*)o.Cm + (int64_t)b * o.csb + (int64_t)g * o.csg + ln4;
  r.xsl = o.xsl; r.dsl = o.dsl; r.bsl = o.bsl; r.csl = o.csl;
  return r;
}

// requests the operands of tokens t0 .. t0 + SQ_PF - 1 of a run of n >= 1 tokens (past the end: the last token again, never used)
template <bool WITH_Y, typename T, typename V4>
__device__ __forceinline__ void seq_load(SeqBatch<T, V4>& r, const SeqRun<T>& s, int t0, int n) {
#pragma unroll
  for (int j = 0; j < SQ_PF; ++j) {
    const int64_t t = min(t0 + j, n - 1);
    r.dt[j] = s.dp[t * s.dsl];
    r.x[j] = s.xp[t * s.xsl];
    r.B[j] = *(const V4*)(s.Bp + t * s.bsl);
    if (WITH_Y) r.C[j] = *(const V4*)(s.Cp + t * s.csl);
  }
}

struct SeqConsts {
  float av, bv, dv, dt_min, dt_max;
  int softplus;
};

// n >= 1 tokens against the row in `sv`; `cur` holds the operands of tokens 0 .. SQ_PF - 1 already.  Every branch on the
// token count is wave-uniform (n is a launch argument, or one value read by the whole grid).
template <bool WITH_Y, typename T, int LPR, typename V4>
__device__ __forceinline__ void seq_march(f32x4& sv, SeqBatch<T, V4>& cur, const SeqRun<T>& s, int n, const SeqConsts& c,
                                          T* yp, int64_t ysl, bool ok, int ln) {
  SeqBatch<T, V4> nxt;
  for (int t0 = 0; t0 < n; t0 += SQ_PF) {
    seq_load<WITH_Y>(nxt, s, t0 + SQ_PF, n);
#pragma unroll
    for (int j = 0; j < SQ_PF; ++j) {
      if (t0 + j < n) {                                 // wave-uniform
        const float d = seq_dt(to_f32(cur.dt[j]), c.bv, c.softplus, c.dt_min, c.dt_max);
        const float xr = to_f32(cur.x[j]);
        float part = seq_token_step<WITH_Y>(sv, d, c.av, xr, cur.B[j], cur.C[j]);
        if (WITH_Y) {
          part = group_sum_dpp<LPR>(part);
          if (ok && ln == LPR - 1) yp[(int64_t)(t0 + j) * ysl] = from_f32<T>(fmaf(c.dv, xr, part));
        }
      }
    }
#pragma unroll
    for (int j = 0; j < SQ_PF; ++j) {
      cur.dt[j] = nxt.dt[j];
      cur.x[j] = nxt.x[j];
      cur.B[j] = nxt.B[j];
      if (WITH_Y) cur.C[j] = nxt.C[j];
    }
  }
}

template <typename T> struct seq_vec4 { typedef f16x4 type; };
template <> struct seq_vec4<float> { typedef f32x4 type; };
template <> struct seq_vec4<bf16_t> { typedef bf16x4 type; };

__device__ __forceinline__ SeqOps seq_ops_of(const SeqArgs& a) {
  SeqOps o;
  o.x = a.x; o.dt = a.dt; o.Bm = a.Bm; o.Cm = a.Cm;
  o.xsb = a.xsb; o.xsl = a.xsl; o.dsb = a.dsb; o.dsl = a.dsl; o.bsb = a.bsb; o.bsl = a.bsl; o.bsg = a.bsg;
  o.csb = a.csb; o.csl = a.csl; o.csg = a.csg;
  return o;
}

template <typename T, int LPR>
__global__ __launch_bounds__(256) void state_update_seq_kernel(SeqArgs a) {
  constexpr int N = 4 * LPR, RPW = 64 / LPR, WAVES = 4;
  typedef typename seq_vec4<T>::type vec4_t;
  const int lane = threadIdx.x & 63;
  const int w = (int)blockIdx.x * WAVES + (threadIdx.x >> 6);
  const int sub = lane / LPR, ln = lane % LPR;
  const int row = w * RPW + sub;                        // (b, h, p) flattened
  const bool ok = row < a.rows_total;
  const int rc = ok ? row : a.rows_total - 1;
  const int bh = (int)((unsigned)rc / (unsigned)a.P);
  const int p = rc - bh * a.P;
  const int b = (int)((unsigned)bh / (unsigned)a.H);
  const int h = bh - b * a.H;
  const int g = a.group_map ? (h % a.G) : (int)((unsigned)h / (unsigned)(a.H / a.G));
  f32x4 sv = __builtin_nontemporal_load((const f32x4*)(a.state + (int64_t)rc * N) + ln);
  SeqConsts c;
  c.av = a.A[h];
  c.bv = a.dt_bias ? a.dt_bias[h] : 0.f;
  c.dv = a.D ? a.D[h] : 0.f;
  c.dt_min = a.dt_min; c.dt_max = a.dt_max; c.softplus = a.softplus;
  const SeqRun<T> s = seq_run_of<T>(seq_ops_of(a), b, h, p, g, a.P, 4 * ln);
  T* yp = (T*)a.y + (int64_t)b * a.ysb + (int64_t)h * a.P + p;
  SeqBatch<T, vec4_t> cur;
  seq_load<true>(cur, s, 0, a.T);
  seq_march<true, T, LPR>(sv, cur, s, a.T, c, yp, a.ysl, ok, ln);
  if (ok) __builtin_nontemporal_store(sv, (f32x4*)(a.state + (int64_t)row * N) + ln);
}

// any d_state: a thread per row, the row walked in memory once per token (it stays in the thread's cache lines)
template <typename T>
__global__ void state_update_seq_rows_kernel(SeqArgs a) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  const int h = blockIdx.y, b = blockIdx.z;
  if (p >= a.P) return;
  const int N = a.N;
  const int g = a.group_map ? (h % a.G) : h / (a.H / a.G);
  const float Ah = a.A[h], bias = a.dt_bias ? a.dt_bias[h] : 0.f, Dh = a.D ? a.D[h] : 0.f;
  float* s = a.state + (((int64_t)b * a.H + h) * a.P + p) * N;
  for (int t = 0; t < a.T; ++t) {
    const float d = seq_dt(to_f32(((const T*)a.dt)[(int64_t)b * a.dsb + (int64_t)t * a.dsl + h]), bias, a.softplus,
                           a.dt_min, a.dt_max);
    const float dec = expf(d * Ah);
    const float xr = to_f32(((const T*)a.x)[(int64_t)b * a.xsb + (int64_t)t * a.xsl + (int64_t)h * a.P + p]);
    const float xv = d * xr;
    const T* Br = (const T*)a.Bm + (int64_t)b * a.bsb + (int64_t)t * a.bsl + (int64_t)g * a.bsg;
    const T* Cr = (const T*)a.Cm + (int64_t)b * a.csb + (int64_t)t * a.csl + (int64_t)g * a.csg;
    float acc = 0.f;
    for (int n = 0; n < N; ++n) {
      const float v = fmaf(dec, s[n], xv * to_f32(Br[n]));
      s[n] = v;
      acc = fmaf(v, to_f32(Cr[n]), acc);
    }
    ((T*)a.y)[(int64_t)b * a.ysb + (int64_t)t * a.ysl + (int64_t)h * a.P + p] = from_f32<T>(fmaf(Dh, xr, acc));
  }
}

// ---------------------------------------------------------------- speculation: commit the kept tokens, look ahead
// One launch per Mamba layer and draft-and-verify step.  The state in memory is always the COMMITTED state: tokens fed
// provisionally (a draft that may be rejected) never reach it.
//   commit phase: the row advances by the first n_commit of the PREVIOUS step's tokens (their operands were kept by the
//                 caller) — the token step of the sequence kernel without y — and is stored iff n_commit > 0;
//   verify phase: the march goes on in registers over the T_new tokens of this step and writes their y; nothing of it
//                 is stored.
// A step therefore reads the state once and writes it at most once, as a decode step does.  n_commit is a launch
// argument or, for a captured graph, one int the whole grid reads (clamped to [0, T_prev]: a stale value cannot reach
// past the kept operands); every branch on it is wave-uniform.  The first operands of the verify phase are requested in
// front of the commit phase, beside the state row: their latency hides behind it.
struct SpecArgs {
  SeqArgs a;                  // the new tokens: operands, y, T = T_new, and everything per layer
  SeqOps prev;                // the previous step's operands
  int T_prev, n_commit;
  const int* n_commit_dev;
};

__device__ __forceinline__ int spec_n_commit(const SpecArgs& s) {
  return s.n_commit_dev ? min(max(*s.n_commit_dev, 0), s.T_prev) : s.n_commit;
}

template <typename T, int LPR>
__global__ __launch_bounds__(256) void state_update_spec_kernel(SpecArgs sa) {
  constexpr int N = 4 * LPR, RPW = 64 / LPR, WAVES = 4;
  typedef typename seq_vec4<T>::type vec4_t;
  const SeqArgs& a = sa.a;
  const int lane = threadIdx.x & 63;
  const int w = (int)blockIdx.x * WAVES + (threadIdx.x >> 6);
  const int sub = lane / LPR, ln = lane % LPR;
  const int row = w * RPW + sub;
  const bool ok = row < a.rows_total;
  const int rc = ok ? row : a.rows_total - 1;
  const int bh = (int)((unsigned)rc / (unsigned)a.P);
  const int p = rc - bh * a.P;
  const int b = (int)((unsigned)bh / (unsigned)a.H);
  const int h = bh - b * a.H;
  const int g = a.group_map ? (h % a.G) : (int)((unsigned)h / (unsigned)(a.H / a.G));
  f32x4 sv = __builtin_nontemporal_load((const f32x4*)(a.state + (int64_t)rc * N) + ln);
  const int nc = spec_n_commit(sa);
  SeqConsts c;
  c.av = a.A[h];
  c.bv = a.dt_bias ? a.dt_bias[h] : 0.f;
  c.dv = a.D ? a.D[h] : 0.f;
  c.dt_min = a.dt_min; c.dt_max = a.dt_max; c.softplus = a.softplus;
  SeqRun<T> sn = {};
  SeqBatch<T, vec4_t> curn = {};
  if (a.T > 0) {
    sn = seq_run_of<T>(seq_ops_of(a), b, h, p, g, a.P, 4 * ln);
    seq_load<true>(curn, sn, 0, a.T);
  }
  if (nc > 0) {
    const SeqRun<T> sp = seq_run_of<T>(sa.prev, b, h, p, g, a.P, 4 * ln);
    SeqBatch<T, vec4_t> curp;
    seq_load<false>(curp, sp, 0, nc);
    seq_march<false, T, LPR>(sv, curp, sp, nc, c, (T*)nullptr, 0, ok, ln);
    if (ok) __builtin_nontemporal_store(sv, (f32x4*)(a.state + (int64_t)row * N) + ln);
  }
  if (a.T > 0) {
    T* yp = (T*)a.y + (int64_t)b * a.ysb + (int64_t)h * a.P + p;
    seq_march<true, T, LPR>(sv, curn, sn, a.T, c, yp, a.ysl, ok, ln);
  }
}

// any d_state, a thread per row.  Commit: the row is walked in memory once per kept token, as the sequence kernel walks
// it.  Verify: the row must stay as committed, and a thread cannot hold a row of any length in registers: the loops are
// turned inside out — per state entry n the march over the tokens runs in one register, and y of SR_TC tokens at a time
// is accumulated over n in ascending order (the order, and so the rounding, of the sequence kernel's sum).  Tokens in
// front of the current SR_TC are marched again per entry: quadratic in T_new / SR_TC, on a path that exists for
// correctness at unusual d_state, not for speed.
constexpr int SR_TC = 8;

template <typename T>
__global__ void state_update_spec_rows_kernel(SpecArgs sa) {
  const SeqArgs& a = sa.a;
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  const int h = blockIdx.y, b = blockIdx.z;
  if (p >= a.P) return;
  const int N = a.N;
  const int g = a.group_map ? (h % a.G) : h / (a.H / a.G);
  const float Ah = a.A[h], bias = a.dt_bias ? a.dt_bias[h] : 0.f, Dh = a.D ? a.D[h] : 0.f;
  float* s = a.state + (((int64_t)b * a.H + h) * a.P + p) * N;
  const int nc = spec_n_commit(sa);
  const SeqOps& o = sa.prev;
  for (int t = 0; t < nc; ++t) {
    const float d = seq_dt(to_f32(((const T*)o.dt)[(int64_t)b * o.dsb + (int64_t)t * o.dsl + h]), bias, a.softplus,
                           a.dt_min, a.dt_max);
    const float dec = expf(d * Ah);
    const float xr = to_f32(((const T*)o.x)[(int64_t)b * o.xsb + (int64_t)t * o.xsl + (int64_t)h * a.P + p]);
    const float xv = d * xr;
    const T* Br = (const T*)o.Bm + (int64_t)b * o.bsb + (int64_t)t * o.bsl + (int64_t)g * o.bsg;
    for (int n = 0; n < N; ++n) s[n] = fmaf(dec, s[n], xv * to_f32(Br[n]));
  }
  const T* xb = (const T*)a.x + (int64_t)b * a.xsb + (int64_t)h * a.P + p;
  const T* db = (const T*)a.dt + (int64_t)b * a.dsb + h;
  const T* Bb = (const T*)a.Bm + (int64_t)b * a.bsb + (int64_t)g * a.bsg;
  const T* Cb = (const T*)a.Cm + (int64_t)b * a.csb + (int64_t)g * a.csg;
  for (int c0 = 0; c0 < a.T; c0 += SR_TC) {
    float dec[SR_TC], xv[SR_TC], xr[SR_TC], acc[SR_TC];
#pragma unroll
    for (int j = 0; j < SR_TC; ++j) {
      const int64_t t = min(c0 + j, a.T - 1);
      const float d = seq_dt(to_f32(db[t * a.dsl]), bias, a.softplus, a.dt_min, a.dt_max);
      dec[j] = expf(d * Ah);
      xr[j] = to_f32(xb[t * a.xsl]);
      xv[j] = d * xr[j];
      acc[j] = 0.f;
    }
    for (int n = 0; n < N; ++n) {
      float v = s[n];
      for (int t = 0; t < c0; ++t) {                    // the tokens in front of this batch, again
        const float d = seq_dt(to_f32(db[(int64_t)t * a.dsl]), bias, a.softplus, a.dt_min, a.dt_max);
        v = fmaf(expf(d * Ah), v, (d * to_f32(xb[(int64_t)t * a.xsl])) * to_f32(Bb[(int64_t)t * a.bsl + n]));
      }
#pragma unroll
      for (int j = 0; j < SR_TC; ++j) {
        if (c0 + j < a.T) {
          v = fmaf(dec[j], v, xv[j] * to_f32(Bb[(int64_t)(c0 + j) * a.bsl + n]));
          acc[j] = fmaf(v, to_f32(Cb[(int64_t)(c0 + j) * a.csl + n]), acc[j]);
        }
      }
    }
#pragma unroll
    for (int j = 0; j < SR_TC; ++j)
      if (c0 + j < a.T)
        ((T*)a.y)[(int64_t)b * a.ysb + (int64_t)(c0 + j) * a.ysl + (int64_t)h * a.P + p] = from_f32<T>(fmaf(Dh, xr[j], acc[j]));
  }
}

}  // namespace

// called from ssd_scan.hip (dispatcher)
int tv_ssd_generic_launch(const void* x, const void* dt, const void* A, const void* Bm,
                          const void* Cm, const void* D, const void* dt_bias,
                          const void* init_state, void* y, void* final_state, void* total_decay,
                          int batch, int seqlen, int nheads, int headdim, int ngroups, int dstate,
                          int64_t xsb, int64_t xsl, int64_t dsb, int64_t dsl, int64_t bsb,
                          int64_t bsl, int64_t bsg, int64_t csb, int64_t csl, int64_t csg, int64_t ysb, int64_t ysl,
                          int dtype, int dt_softplus, float dt_min, float dt_max, int group_map,
                          hipStream_t st) {
  SsdArgs a;
  a.x = x; a.dt = dt; a.Bm = Bm; a.Cm = Cm;
  a.A = (const float*)A; a.D = (const float*)D; a.dt_bias = (const float*)dt_bias;
  a.init = (const float*)init_state; a.y = y; a.final_state = (float*)final_state;
  a.total_decay = (float*)total_decay;
  a.L = seqlen; a.H = nheads; a.P = headdim; a.G = ngroups; a.N = dstate;
  a.xsb = xsb; a.xsl = xsl; a.dsb = dsb; a.dsl = dsl; a.bsb = bsb; a.bsl = bsl; a.bsg = bsg;
  a.csb = csb; a.csl = csl; a.csg = csg; a.ysb = ysb; a.ysl = ysl;
  a.softplus = dt_softplus; a.group_map = group_map; a.dt_min = dt_min; a.dt_max = dt_max;
  switch (dtype) {
    case TV_F32: return launch_generic<float>(a, batch, st);
    case TV_BF16: return launch_generic<bf16_t>(a, batch, st);
    case TV_F16: return launch_generic<f16_t>(a, batch, st);
  }
  TV_UNSUPPORTED("ssd_scan: dtype %d", dtype);
}

extern "C" int tv_selective_state_update(void* state, const void* x, const void* dt,
                                         const void* A, const void* Bm, const void* Cm,
                                         const void* D, const void* dt_bias, void* y, int batch,
                                         int nheads, int headdim, int ngroups, int dstate,
                                         int dtype, int dt_softplus, void* stream) {
  TV_CHECK_ARG(state && x && dt && A && Bm && Cm && y, "selective_state_update: null pointer");
  TV_CHECK_ARG(batch > 0 && nheads > 0 && headdim > 0 && ngroups > 0 && dstate > 0 &&
                   nheads % ngroups == 0,
               "selective_state_update: bad sizes");
  hipStream_t s = (hipStream_t)stream;
  // d_state 16 / 32 / 64 / 128 / 256 with 16-byte aligned rows: lanes share a row (coalesced); anything else: a thread per row
  const int lpr = dstate / 4;
  if (dstate % 4 == 0 && (lpr == 4 || lpr == 8 || lpr == 16 || lpr == 32 || lpr == 64) && (((uintptr_t)state) & 15) == 0 &&
      (((uintptr_t)Bm | (uintptr_t)Cm) & 15) == 0 && (int64_t)batch * nheads * headdim < (1ll << 31)) {
    const int64_t rows = (int64_t)batch * nheads * headdim;
    const int64_t rows_per_block = 4 * (64 / lpr);              // 4 waves x rows per wave-instruction
    const dim3 rgrid((unsigned)((rows + rows_per_block - 1) / rows_per_block));
#define TV_SUR(T, LPR)                                                                                        \
    state_update_chain_kernel<T, LPR><<<rgrid, 256, 0, s>>>((float*)state, (const T*)x, (const T*)dt,         \
        (const float*)A, (const T*)Bm, (const T*)Cm, (const float*)D, (const float*)dt_bias, (T*)y, nheads,   \
        headdim, ngroups, dt_softplus, (int)rows)
#define TV_SUR_T(T)                                                                                           \
    switch (lpr) { case 4: TV_SUR(T, 4); break; case 8: TV_SUR(T, 8); break; case 16: TV_SUR(T, 16); break;     \
                   case 32: TV_SUR(T, 32); break; default: TV_SUR(T, 64); break; }
    switch (dtype) {
      case TV_F32: TV_SUR_T(float); break;
      case TV_BF16: TV_SUR_T(bf16_t); break;
      case TV_F16: TV_SUR_T(f16_t); break;
      default: TV_UNSUPPORTED("selective_state_update: dtype %d", dtype);
    }
#undef TV_SUR_T
#undef TV_SUR
    TV_LAUNCH_CHECK();
  }
  dim3 grid((headdim + 63) / 64, nheads, batch);
#define TV_SU(T)                                                                              \
  state_update_kernel<T><<<grid, 64, 0, s>>>((float*)state, (const T*)x, (const T*)dt,        \
      (const float*)A, (const T*)Bm, (const T*)Cm, (const float*)D, (const float*)dt_bias,    \
      (T*)y, nheads, headdim, ngroups, dstate, dt_softplus)
  switch (dtype) {
    case TV_F32: TV_SU(float); break;
    case TV_BF16: TV_SU(bf16_t); break;
    case TV_F16: TV_SU(f16_t); break;
    default: TV_UNSUPPORTED("selective_state_update: dtype %d", dtype);
  }
#undef TV_SU
  TV_LAUNCH_CHECK();
}

static int g_seq_last_impl = 0;
extern "C" int tv_selective_state_update_seq_last_impl(void) { return g_seq_last_impl; }

extern "C" int tv_selective_state_update_seq(void* state, const void* x, const void* dt, const void* A,
                                             const void* Bm, const void* Cm, const void* D, const void* dt_bias,
                                             void* y, int batch, int seqlen, int nheads, int headdim, int ngroups,
                                             int dstate, int64_t xsb, int64_t xsl, int64_t dsb, int64_t dsl,
                                             int64_t bsb, int64_t bsl, int64_t bsg, int64_t csb, int64_t csl,
                                             int64_t csg, int64_t ysb, int64_t ysl, int dtype, int dt_softplus,
                                             float dt_min, float dt_max, int group_map, void* stream) {
  TV_CHECK_ARG(state && x && dt && A && Bm && Cm && y, "selective_state_update_seq: null pointer");
  TV_CHECK_ARG(batch > 0 && seqlen > 0 && nheads > 0 && headdim > 0 && ngroups > 0 && dstate > 0 &&
                   nheads % ngroups == 0,
               "selective_state_update_seq: bad sizes");
  TV_CHECK_ARG(xsl >= (int64_t)nheads * headdim && ysl >= (int64_t)nheads * headdim && dsl >= nheads,
               "selective_state_update_seq: x / y / dt rows overlap");
  if (dtype != TV_F32 && dtype != TV_BF16 && dtype != TV_F16) TV_UNSUPPORTED("selective_state_update_seq: dtype %d", dtype);
  hipStream_t s = (hipStream_t)stream;
  SeqArgs a;
  a.state = (float*)state; a.x = x; a.dt = dt; a.Bm = Bm; a.Cm = Cm;
  a.A = (const float*)A; a.D = (const float*)D; a.dt_bias = (const float*)dt_bias; a.y = y;
  a.T = seqlen; a.H = nheads; a.P = headdim; a.G = ngroups; a.N = dstate;
  a.xsb = xsb; a.xsl = xsl; a.dsb = dsb; a.dsl = dsl; a.bsb = bsb; a.bsl = bsl; a.bsg = bsg;
  a.csb = csb; a.csl = csl; a.csg = csg; a.ysb = ysb; a.ysl = ysl;
  a.softplus = dt_softplus; a.group_map = group_map; a.dt_min = dt_min; a.dt_max = dt_max;
  const int64_t rows = (int64_t)batch * nheads * headdim;
  a.rows_total = (int)(rows < (1ll << 31) ? rows : 0);
  // the lanes of a row read 4 entries of B / C as one vector: 16-byte aligned pieces for fp32, 8-byte for the 16-bit types
  const int lpr = dstate / 4;
  const int64_t bc = bsb | bsl | bsg | csb | csl | csg;
  const uintptr_t bc_align = dtype == TV_F32 ? 15 : 7;
  if (dstate % 4 == 0 && (lpr == 4 || lpr == 8 || lpr == 16 || lpr == 32 || lpr == 64) && (((uintptr_t)state) & 15) == 0 &&
      (((uintptr_t)Bm | (uintptr_t)Cm) & bc_align) == 0 && bc % 4 == 0 && rows < (1ll << 31)) {
    g_seq_last_impl = 1;
    const int64_t rows_per_block = 4 * (64 / lpr);
    const dim3 rgrid((unsigned)((rows + rows_per_block - 1) / rows_per_block));
#define TV_SQ(T, LPR) state_update_seq_kernel<T, LPR><<<rgrid, 256, 0, s>>>(a)
#define TV_SQ_T(T)                                                                                          \
    switch (lpr) { case 4: TV_SQ(T, 4); break; case 8: TV_SQ(T, 8); break; case 16: TV_SQ(T, 16); break;       \
                   case 32: TV_SQ(T, 32); break; default: TV_SQ(T, 64); break; }
    switch (dtype) {
      case TV_F32: TV_SQ_T(float); break;
      case TV_BF16: TV_SQ_T(bf16_t); break;
      default: TV_SQ_T(f16_t); break;
    }
#undef TV_SQ_T
#undef TV_SQ
    TV_LAUNCH_CHECK();
  }
  g_seq_last_impl = 2;
  dim3 grid((headdim + 63) / 64, nheads, batch);
  switch (dtype) {
    case TV_F32: state_update_seq_rows_kernel<float><<<grid, 64, 0, s>>>(a); break;
    case TV_BF16: state_update_seq_rows_kernel<bf16_t><<<grid, 64, 0, s>>>(a); break;
    default: state_update_seq_rows_kernel<f16_t><<<grid, 64, 0, s>>>(a); break;
  }
  TV_LAUNCH_CHECK();
}

static int g_spec_last_impl = 0;
extern "C" int tv_selective_state_update_spec_last_impl(void) { return g_spec_last_impl; }

extern "C" int tv_selective_state_update_spec(
    void* state, const void* A, const void* D, const void* dt_bias,
    const void* x_prev, const void* dt_prev, const void* B_prev, const void* C_prev, int t_prev, int n_commit,
    const int* n_commit_dev, int64_t pxsb, int64_t pxsl, int64_t pdsb, int64_t pdsl, int64_t pbsb, int64_t pbsl,
    int64_t pbsg, int64_t pcsb, int64_t pcsl, int64_t pcsg,
    const void* x, const void* dt, const void* Bm, const void* Cm, void* y, int t_new, int64_t xsb, int64_t xsl,
    int64_t dsb, int64_t dsl, int64_t bsb, int64_t bsl, int64_t bsg, int64_t csb, int64_t csl, int64_t csg, int64_t ysb,
    int64_t ysl, int batch, int nheads, int headdim, int ngroups, int dstate, int dtype, int dt_softplus, float dt_min,
    float dt_max, int group_map, void* stream) {
  TV_CHECK_ARG(state && A, "selective_state_update_spec: null pointer");
  TV_CHECK_ARG(batch > 0 && t_prev >= 0 && t_new >= 0 && nheads > 0 && headdim > 0 && ngroups > 0 && dstate > 0 &&
                   nheads % ngroups == 0,
               "selective_state_update_spec: bad sizes");
  TV_CHECK_ARG(t_prev == 0 || (x_prev && dt_prev && B_prev && C_prev), "selective_state_update_spec: null previous operands");
  TV_CHECK_ARG(t_new == 0 || (x && dt && Bm && Cm && y), "selective_state_update_spec: null operands");
  TV_CHECK_ARG(n_commit_dev || (n_commit >= 0 && n_commit <= t_prev),
               "selective_state_update_spec: n_commit outside [0, t_prev]");
  const int64_t hp = (int64_t)nheads * headdim;
  TV_CHECK_ARG(t_prev == 0 || (pxsl >= hp && pdsl >= nheads), "selective_state_update_spec: previous x / dt rows overlap");
  TV_CHECK_ARG(t_new == 0 || (xsl >= hp && ysl >= hp && dsl >= nheads), "selective_state_update_spec: x / y / dt rows overlap");
  if (dtype != TV_F32 && dtype != TV_BF16 && dtype != TV_F16) TV_UNSUPPORTED("selective_state_update_spec: dtype %d", dtype);
  if (t_new == 0 && (t_prev == 0 || (!n_commit_dev && n_commit == 0))) return TV_OK;      // nothing to commit, nothing to run
  hipStream_t s = (hipStream_t)stream;
  SpecArgs sa;
  SeqArgs& a = sa.a;
  a.state = (float*)state; a.x = x; a.dt = dt; a.Bm = Bm; a.Cm = Cm;
  a.A = (const float*)A; a.D = (const float*)D; a.dt_bias = (const float*)dt_bias; a.y = y;
  a.T = t_new; a.H = nheads; a.P = headdim; a.G = ngroups; a.N = dstate;
  a.xsb = xsb; a.xsl = xsl; a.dsb = dsb; a.dsl = dsl; a.bsb = bsb; a.bsl = bsl; a.bsg = bsg;
  a.csb = csb; a.csl = csl; a.csg = csg; a.ysb = ysb; a.ysl = ysl;
  a.softplus = dt_softplus; a.group_map = group_map; a.dt_min = dt_min; a.dt_max = dt_max;
  SeqOps& o = sa.prev;
  o.x = x_prev; o.dt = dt_prev; o.Bm = B_prev; o.Cm = C_prev;
  o.xsb = pxsb; o.xsl = pxsl; o.dsb = pdsb; o.dsl = pdsl; o.bsb = pbsb; o.bsl = pbsl; o.bsg = pbsg;
  o.csb = pcsb; o.csl = pcsl; o.csg = pcsg;
  sa.T_prev = t_prev; sa.n_commit = n_commit_dev ? 0 : n_commit; sa.n_commit_dev = n_commit_dev;
  const int64_t rows = (int64_t)batch * nheads * headdim;
  a.rows_total = (int)(rows < (1ll << 31) ? rows : 0);
  // as in the sequence entry point: the lanes of a row read 4 entries of B / C as one vector, of either operand set
  const int lpr = dstate / 4;
  int64_t bc = 0;
  uintptr_t ptrs = (uintptr_t)0;
  if (t_new > 0) { bc |= bsb | bsl | bsg | csb | csl | csg; ptrs |= (uintptr_t)Bm | (uintptr_t)Cm; }
  if (t_prev > 0) { bc |= pbsb | pbsl | pbsg; ptrs |= (uintptr_t)B_prev; }
  const uintptr_t bc_align = dtype == TV_F32 ? 15 : 7;
  if (dstate % 4 == 0 && (lpr == 4 || lpr == 8 || lpr == 16 || lpr == 32 || lpr == 64) && (((uintptr_t)state) & 15) == 0 &&
      (ptrs & bc_align) == 0 && bc % 4 == 0 && rows < (1ll << 31)) {
    g_spec_last_impl = 1;
    const int64_t rows_per_block = 4 * (64 / lpr);
    const dim3 rgrid((unsigned)((rows + rows_per_block - 1) / rows_per_block));
#define TV_SP(T, LPR) state_update_spec_kernel<T, LPR><<<rgrid, 256, 0, s>>>(sa)
#define TV_SP_T(T)                                                                                          \
    switch (lpr) { case 4: TV_SP(T, 4); break; case 8: TV_SP(T, 8); break; case 16: TV_SP(T, 16); break;       \
                   case 32: TV_SP(T, 32); break; default: TV_SP(T, 64); break; }
    switch (dtype) {
      case TV_F32: TV_SP_T(float); break;
      case TV_BF16: TV_SP_T(bf16_t); break;
      default: TV_SP_T(f16_t); break;
    }
#undef TV_SP_T
#undef TV_SP
    TV_LAUNCH_CHECK();
  }
  g_spec_last_impl = 2;
  dim3 grid((headdim + 63) / 64, nheads, batch);
  switch (dtype) {
    case TV_F32: state_update_spec_rows_kernel<float><<<grid, 64, 0, s>>>(sa); break;
    case TV_BF16: state_update_spec_rows_kernel<bf16_t><<<grid, 64, 0, s>>>(sa); break;
    default: state_update_spec_rows_kernel<f16_t><<<grid, 64, 0, s>>>(sa); break;
  }
  TV_LAUNCH_CHECK();
}
