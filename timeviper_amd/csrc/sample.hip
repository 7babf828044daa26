// Sampled decoding: temperature / top-k / top-p sampling of one token per row of fp32 logits in ONE launch, in the
// place of the decode step's argmax (llm/decode_graph.py), replayable by the captured graph: the draw index and the
// stream of every row live in device memory, the seed and the parameters are launch constants.
//
// The result is a pure function of (row, parameters, seed, draw index, stream): bitwise reproducible, independent of
// the other rows.  Everything is a VALUE threshold, never a sort order (bf16 logits widened to fp32 tie all the time):
//   s_i = z_i * (1/T) (one fp32 multiply), m = max s, w_i = exp(s_i - m), q_i = floor(w_i * 2^40) as an integer: every
//   mass below is an integer sum of q, so no sum depends on its order (V <= 2^18: all sums < 2^58);
//   top-k: t_k = the k-th largest s, keep s >= t_k (ties kept), W = the mass kept;
//   top-p (after top-k): keep i iff the mass of the kept tokens with s > s_i is < top_p * W;
//   u32 = Philox4x32-10(counter (draw_lo, draw_hi, stream, 0), key (seed_lo, seed_hi))[0], r = (W_kept * u32) >> 32;
//   the token is the smallest kept index whose inclusive prefix sum of q over the kept set exceeds r.
// One work-group of 1 024 threads per row.  s maps to an order-preserving 32-bit key; a threshold is found by a radix
// descent of 3 levels (11 + 11 + 10 bits) over integer LDS histograms (count for top-k, mass for top-p) filled with
// integer LDS atomics.  A descent whose filter is off is skipped.  The last pass sums q over the kept set per tile of
// 256 consecutive elements; one wave then walks the tile sums and the one tile that holds r.
#include "common.hpp"

namespace {

constexpr int kThreads = 1024;
constexpr int kWaves = kThreads / 64;
constexpr int kBins = 2048;
constexpr int kMaxVocab = 1 << 18;

typedef unsigned long long u64;
typedef unsigned int u32;

struct SampleSmem {
  u64 mass1[kBins];   // level-1 mass histogram: the top-k and the top-p descent both start from it
  u64 mass[kBins];    // level-2 / level-3 mass histogram; afterwards the kept mass per tile of 256 elements
  u32 cnt[kBins];     // count histogram of the current level
  u64 wave_m[kWaves];
  u32 wave_c[kWaves];
  float wave_f[2 * kWaves];
  u32 sel_bin;        // what pick_bin found
  u32 sel_above_c;
  u64 sel_above_m;
  u64 sel_target;
  u32 n_kept;
};

// order-preserving key of a float: a > b <=> key(a) > key(b); NaN sorts below everything (it carries no mass either)
__device__ __forceinline__ u32 key_of(float s) {
  const u32 b = __float_as_uint(s);
  if (s != s) return 0u;
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ u32 bits_of_key(u32 k) { return (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k; }

// q = floor(exp(s - m) * 2^40); NaN (a row outside the contract) carries no mass
__device__ __forceinline__ u64 mass_of(float s, float m) {
  const float d = s - m;
  const float x = expf(d) * 1099511627776.0f;
  return x >= 0.f ? (u64)x : 0ull;
}

// Elements [4g - shift, 4g - shift + 4) of the row, scaled: one 16-byte load where the group lies inside the row
// (shift = elements between the last 16-byte boundary and the row's start), element by element at the row's two ends.
// "+ 0.f" turns -0 into +0: equal values, one key.
__device__ __forceinline__ void load_group(const float* __restrict__ row, int V, int shift, int g, float inv_t,
                                           float s[4], bool ok[4]) {
  const int j0 = 4 * g - shift;
  if (j0 >= 0 && j0 + 3 < V) {
    const f32x4 x = *(const f32x4*)(row + j0);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      s[e] = x[e] * inv_t + 0.f;
      ok[e] = true;
    }
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int i = j0 + e;
      ok[e] = i >= 0 && i < V;
      s[e] = ok[e] ? row[i] * inv_t + 0.f : 0.f;
    }
  }
}

__device__ __forceinline__ u64 shfl_up_u64(u64 v, int o) {
  const u32 lo = __shfl_up((u32)v, o, 64), hi = __shfl_up((u32)(v >> 32), o, 64);
  return ((u64)hi << 32) | lo;
}
__device__ __forceinline__ u64 shfl_u64(u64 v, int src) {
  const u32 lo = __shfl((u32)v, src, 64), hi = __shfl((u32)(v >> 32), src, 64);
  return ((u64)hi << 32) | lo;
}

// sum over the wave of a 32-bit integer: DPP row shifts / row broadcasts (the pattern of wave_sum_dpp), lane 63 read back
template <int CTRL, int ROWMASK>
__device__ __forceinline__ u32 dpp_add_u32(u32 v) {
  return v + (u32)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROWMASK, 0xf, false);
}
__device__ __forceinline__ u32 wave_sum_u32(u32 v) {
  v = dpp_add_u32<0x111, 0xf>(v);
  v = dpp_add_u32<0x112, 0xf>(v);
  v = dpp_add_u32<0x114, 0xf>(v);
  v = dpp_add_u32<0x118, 0xf>(v);
  v = dpp_add_u32<0x142, 0xa>(v);
  v = dpp_add_u32<0x143, 0xc>(v);
  return (u32)__builtin_amdgcn_readlane((int)v, 63);
}

// One level of a descent: the histogram bin, counted from the TOP, whose inclusive cumulative count (by_mass false) or
// mass (by_mass true) first reaches the target.  frac >= 0: the target is ceil(frac * total mass) (top-p without top-k:
// W is the whole row's mass), else `target`; it is clamped to the total.  Leaves the bin, the count and the mass of
// the bins above it and the target in shared memory (bin 0, nothing above, where the histogram is empty).
__device__ void pick_bin(SampleSmem& sm, const u32* cnt, const u64* mass, bool by_mass, u64 target, double frac) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b0 = kBins - 1 - 2 * tid, b1 = b0 - 1;
  const u32 c0 = cnt ? cnt[b0] : 0u, c1 = cnt ? cnt[b1] : 0u;
  const u64 m0 = mass ? mass[b0] : 0ull, m1 = mass ? mass[b1] : 0ull;
  u32 ic = c0 + c1;
  u64 im = m0 + m1;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const u32 tc = __shfl_up(ic, o, 64);
    const u64 tm = shfl_up_u64(im, o);
    if (lane >= o) {
      ic += tc;
      im += tm;
    }
  }
  if (lane == 63) {
    sm.wave_c[wave] = ic;
    sm.wave_m[wave] = im;
  }
  if (tid == 0) {
    sm.sel_bin = 0u;
    sm.sel_above_c = 0u;
    sm.sel_above_m = 0ull;
    sm.sel_target = 0ull;
  }
  __syncthreads();
  u32 off_c = 0u, tot_c = 0u;
  u64 off_m = 0ull, tot_m = 0ull;
  for (int w = 0; w < kWaves; ++w) {
    const u32 wc = sm.wave_c[w];
    const u64 wm = sm.wave_m[w];
    if (w < wave) {
      off_c += wc;
      off_m += wm;
    }
    tot_c += wc;
    tot_m += wm;
  }
  if (frac >= 0.0) target = (u64)ceil(frac * (double)tot_m);
  const u64 total = by_mass ? tot_m : (u64)tot_c;
  if (target > total) target = total;
  const u32 ec = off_c + ic - (c0 + c1);      // count / mass of the bins above b0
  const u64 em = off_m + im - (m0 + m1);
  const u64 x0 = by_mass ? em : (u64)ec, v0 = by_mass ? m0 : (u64)c0, v1 = by_mass ? m1 : (u64)c1;
  if (x0 < target && target <= x0 + v0) {
    sm.sel_bin = (u32)b0;
    sm.sel_above_c = ec;
    sm.sel_above_m = em;
    sm.sel_target = target;
  } else if (x0 + v0 < target && target <= x0 + v0 + v1) {
    sm.sel_bin = (u32)b1;
    sm.sel_above_c = ec + c0;
    sm.sel_above_m = em + m0;
    sm.sel_target = target;
  }
  __syncthreads();
}

// One pass over the row: the elements whose key starts with `prefix` (all of them at level 1) go into the histograms of
// the level's digit.  cnt / mass null: that histogram is not needed.
__device__ void fill_level(const float* __restrict__ row, int V, int shift, int n_groups, float inv_t, float m,
                           int level, u32 prefix, u32* cnt, u64* mass) {
  const int p_shift = level == 2 ? 21 : 10;              // level 1: every key takes part
  const int b_shift = level == 1 ? 21 : (level == 2 ? 10 : 0);
  const u32 b_mask = level == 3 ? 1023u : 2047u;
#pragma unroll 2
  for (int g = threadIdx.x; g < n_groups; g += kThreads) {
    float s[4];
    bool ok[4];
    load_group(row, V, shift, g, inv_t, s, ok);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const u32 key = key_of(s[e]);
      if (ok[e] && (level == 1 || (key >> p_shift) == prefix)) {
        const u32 bin = (key >> b_shift) & b_mask;
        if (cnt) atomicAdd(&cnt[bin], 1u);
        if (mass) {
          const u64 q = mass_of(s[e], m);
          if (q) atomicAdd(&mass[bin], q);
        }
      }
    }
  }
}

__device__ __forceinline__ void zero_hist(u32* cnt, u64* mass) {
  for (int i = threadIdx.x; i < kBins; i += kThreads) {
    if (cnt) cnt[i] = 0u;
    if (mass) mass[i] = 0ull;
  }
}

__device__ __forceinline__ u32 philox4x32_10_first(u32 c0, u32 c1, u32 c2, u32 c3, u32 k0, u32 k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const u64 p0 = (u64)0xD2511F53u * c0, p1 = (u64)0xCD9E8D57u * c2;
    const u32 n0 = (u32)(p1 >> 32) ^ c1 ^ k0, n2 = (u32)(p0 >> 32) ^ c3 ^ k1;
    c1 = (u32)p1;
    c3 = (u32)p0;
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return c0;
}

__global__ __launch_bounds__(kThreads) void sample_logits_kernel(
    const float* __restrict__ logits, int64_t row_stride, int V, int64_t* __restrict__ out_ids,
    const int64_t* __restrict__ draws, const int* __restrict__ streams, int* __restrict__ diag, u64 seed, float inv_t,
    int top_k, float top_p) {
  __shared__ SampleSmem sm;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x;
  const float* __restrict__ row = logits + (int64_t)b * row_stride;
  const int shift = (int)(((uintptr_t)row & 15) >> 2);
  const int n_groups = (V + shift + 3) >> 2;
  const bool k_on = top_k > 0 && top_k < V, p_on = top_p < 1.f;

  // ---- the row's maximum (and minimum: the threshold reported when no filter is on)
  float mx = -INFINITY, mn = INFINITY;
#pragma unroll 2
  for (int g = tid; g < n_groups; g += kThreads) {
    float s[4];
    bool ok[4];
    load_group(row, V, shift, g, inv_t, s, ok);
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (ok[e]) {
        mx = fmaxf(mx, s[e]);
        mn = fminf(mn, s[e]);
      }
  }
  mx = wave_max(mx);
  mn = -wave_max(-mn);
  if (lane == 0) {
    sm.wave_f[wave] = mx;
    sm.wave_f[kWaves + wave] = mn;
  }
  __syncthreads();
  mx = sm.wave_f[0];
  mn = sm.wave_f[kWaves];
  for (int w = 1; w < kWaves; ++w) {
    mx = fmaxf(mx, sm.wave_f[w]);
    mn = fminf(mn, sm.wave_f[kWaves + w]);
  }
  const float m = mx;

  // ---- thresholds: keys >= key_t are kept
  u32 key_k = 0u, key_p = 0u;
  u64 W = 0ull;                                // the mass top-k keeps (needed by top-p only)
  if (k_on || p_on) {
    zero_hist(k_on ? sm.cnt : nullptr, p_on ? sm.mass1 : nullptr);
    __syncthreads();
    fill_level(row, V, shift, n_groups, inv_t, m, 1, 0u, k_on ? sm.cnt : nullptr, p_on ? sm.mass1 : nullptr);
    __syncthreads();
  }
  if (k_on) {
    u64 target = (u64)top_k;
    u32 prefix = 0u;
    for (int level = 1; level <= 3; ++level) {
      u64* mh = !p_on ? nullptr : (level == 1 ? sm.mass1 : sm.mass);
      if (level > 1) {
        zero_hist(sm.cnt, mh);
        __syncthreads();
        fill_level(row, V, shift, n_groups, inv_t, m, level, prefix, sm.cnt, mh);
        __syncthreads();
      }
      pick_bin(sm, sm.cnt, mh, false, target, -1.0);
      target -= sm.sel_above_c;               // what is still to be counted inside the chosen bin
      W += sm.sel_above_m;
      prefix = (prefix << (level == 3 ? 10 : 11)) | sm.sel_bin;
      if (level == 3 && p_on) W += sm.mass[sm.sel_bin];
      __syncthreads();                          // sel_* and the histograms are rewritten by the next level
    }
    key_k = prefix;
  }
  if (p_on) {
    u64 target = 0ull;
    u32 prefix = 0u;
    for (int level = 1; level <= 3; ++level) {
      u64* mh = level == 1 ? sm.mass1 : sm.mass;
      if (level > 1) {
        zero_hist(nullptr, mh);
        __syncthreads();
        fill_level(row, V, shift, n_groups, inv_t, m, level, prefix, nullptr, mh);
        __syncthreads();
      }
      if (level == 1) {
        // top_p * W: W is the mass top-k kept, or the whole row's (the total of the level-1 histogram)
        if (k_on) {
          target = (u64)ceil((double)top_p * (double)W);
          if (target > W) target = W;
        }
        pick_bin(sm, nullptr, mh, true, target, k_on ? -1.0 : (double)top_p);
        target = sm.sel_target;
      } else {
        pick_bin(sm, nullptr, mh, true, target, -1.0);
      }
      target -= sm.sel_above_m;
      prefix = (prefix << (level == 3 ? 10 : 11)) | sm.sel_bin;
      __syncthreads();
    }
    key_p = prefix;
  }
  const u32 key_t = key_k > key_p ? key_k : key_p;

  // ---- the kept mass per tile of 256 consecutive elements (tile = 16 * iteration + wave), the kept count
  const int n_tiles = (n_groups + 63) >> 6;
  u64* tile_sum = sm.mass;
  if (tid == 0) sm.n_kept = 0u;
  __syncthreads();
  u32 kept = 0u;
  for (int tile = wave; tile < n_tiles; tile += kWaves) {
    const int g = tile * 64 + lane;
    u64 ls = 0ull;
    u32 lk = 0u;
    if (g < n_groups) {
      float s[4];
      bool ok[4];
      load_group(row, V, shift, g, inv_t, s, ok);
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (ok[e] && key_of(s[e]) >= key_t) {
          ls += mass_of(s[e], m);
          ++lk;
        }
    }
    u64 ts = 0ull;
    if (__ballot(lk != 0u)) {
      // ls < 2^42: two 32-bit sums of 24-bit / 18-bit halves cannot overflow over 64 lanes
      const u32 lo = wave_sum_u32((u32)ls & 0xffffffu), hi = wave_sum_u32((u32)(ls >> 24));
      ts = ((u64)hi << 24) + lo;
      kept += wave_sum_u32(lk);
    }
    if (lane == 0) tile_sum[tile] = ts;
  }
  if (lane == 0 && kept) atomicAdd(&sm.n_kept, kept);
  __syncthreads();

  // ---- one wave: the random number, the tile that holds r, the element inside it
  if (wave != 0) return;
  const u64 draw = (u64)draws[b];
  const u32 u = philox4x32_10_first((u32)draw, (u32)(draw >> 32), (u32)streams[b], 0u, (u32)seed, (u32)(seed >> 32));
  const int per = (n_tiles + 63) >> 6;         // consecutive tiles per lane
  u64 mine = 0ull;
  for (int t = lane * per; t < min((lane + 1) * per, n_tiles); ++t) mine += tile_sum[t];
  u64 incl = mine;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const u64 t = shfl_up_u64(incl, o);
    if (lane >= o) incl += t;
  }
  const u64 w_kept = shfl_u64(incl, 63);
  const u64 r = __umul64hi(w_kept, (u64)u << 32);          // (w_kept * u) >> 32, exactly
  int64_t id = 0;                                          // a row without mass (outside the contract): a valid id
  const u64 in_lane = __ballot(incl > r);
  if (in_lane) {
    const int l0 = __ffsll((unsigned long long)in_lane) - 1;
    u64 base = shfl_u64(incl - mine, l0);
    int tile = l0 * per;
    const int t_end = min((l0 + 1) * per, n_tiles) - 1;
    while (tile < t_end && base + tile_sum[tile] <= r) base += tile_sum[tile++];
    const int g = tile * 64 + lane;
    u64 q[4] = {0ull, 0ull, 0ull, 0ull};
    if (g < n_groups) {
      float s[4];
      bool ok[4];
      load_group(row, V, shift, g, inv_t, s, ok);
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (ok[e] && key_of(s[e]) >= key_t) q[e] = mass_of(s[e], m);
    }
    const u64 lsum = q[0] + q[1] + q[2] + q[3];
    u64 li = lsum;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const u64 t = shfl_up_u64(li, o);
      if (lane >= o) li += t;
    }
    const u64 hit = __ballot(base + li > r);
    if (hit) {
      const int l1 = __ffsll((unsigned long long)hit) - 1;
      if (lane == l1) {
        u64 run = base + li - lsum;
        int e = 0;
        for (; e < 3; ++e) {
          run += q[e];
          if (run > r) break;
        }
        int i = 4 * g - shift + e;
        i = i < 0 ? 0 : (i >= V ? V - 1 : i);
        out_ids[b] = (int64_t)i;
      }
    } else if (lane == 0) {
      out_ids[b] = id;
    }
  } else if (lane == 0) {
    out_ids[b] = id;
  }
  if (diag && lane == 0) {
    diag[4 * b + 0] = (int)sm.n_kept;
    diag[4 * b + 1] = (int)(key_t ? bits_of_key(key_t) : __float_as_uint(mn));
    diag[4 * b + 2] = (int)u;
    diag[4 * b + 3] = 0;
  }
}

}  // namespace

extern "C" int tv_sample_logits_fwd(const void* logits, void* out_ids, const void* draws, const void* streams,
                                    void* diag, int batch, int vocab, int64_t row_stride, int64_t seed,
                                    float inv_temperature, int top_k, float top_p, void* stream) {
  TV_CHECK_ARG(logits && out_ids && draws && streams, "sample_logits: null pointer");
  TV_CHECK_ARG(batch >= 1 && vocab >= 1, "sample_logits: bad sizes (batch %d, vocab %d)", batch, vocab);
  TV_CHECK_ARG(inv_temperature > 0.f && inv_temperature < INFINITY, "sample_logits: the temperature must be positive");
  TV_CHECK_ARG(top_p > 0.f, "sample_logits: top_p must be positive (>= 1 switches it off)");
  TV_CHECK_ARG(top_k >= 0, "sample_logits: top_k must not be negative (0 switches it off)");
  TV_CHECK_ARG(((uintptr_t)logits & 3) == 0 && ((uintptr_t)out_ids & 7) == 0 && ((uintptr_t)draws & 7) == 0 &&
                   ((uintptr_t)streams & 3) == 0 && ((uintptr_t)diag & 3) == 0, "sample_logits: misaligned pointer");
  if (vocab > kMaxVocab) TV_UNSUPPORTED("sample_logits: vocab %d > 2^18 (the integer masses would overflow)", vocab);
  sample_logits_kernel<<<dim3((unsigned)batch), kThreads, 0, (hipStream_t)stream>>>(
      (const float*)logits, row_stride, vocab, (int64_t*)out_ids, (const int64_t*)draws, (const int*)streams,
      (int*)diag, (u64)seed, inv_temperature, top_k, top_p);
  TV_LAUNCH_CHECK();
}
