// The body of the merge kernels of attn_splitkv.hip (included into each: `a` the DecArgs, APPEND / BRANCH as in the walk).
  constexpr int U = 8;
  typedef float f32x2 __attribute__((ext_vector_type(2)));
  const int tok = APPEND || BRANCH ? blockIdx.x / a.Hq : 0, h = APPEND || BRANCH ? blockIdx.x % a.Hq : blockIdx.x;
  const int b = BRANCH ? 0 : blockIdx.y, d = threadIdx.x;
  int nvalid, nvalid_p = 0, skip = 0;                     // BRANCH: split s >= nvalid_p lies `skip` slots further on
  int64_t slot0;
  if constexpr (BRANCH) {
    const BranchWork wp = branch_work(a, 0), ws = branch_work(a, a.nblk_p + tok * a.Hkv * a.hbq * a.nsplit_s);
    nvalid_p = (wp.Lk + wp.chunk - 1) / wp.chunk;
    nvalid = nvalid_p + (ws.Lk + ws.chunk - 1) / ws.chunk;
    skip = a.nsplit - nvalid_p;
    slot0 = ((int64_t)tok * a.Hq + h) * (a.nsplit + a.nsplit_s);
  } else {
    int Lk, chunk;
    split_of(a, b, Lk, chunk);
    nvalid = (Lk + chunk - 1) / chunk;
    slot0 = slot_of<APPEND>(a, b, tok, h);
  }
  float M = -INFINITY, L = 0.f, O = 0.f;
  for (int s0 = 0; s0 < nvalid; s0 += U) {
    f32x2 ml[U];
    float o[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      int sidx = min(s0 + u, nvalid - 1);              // (past the end: the last split again, weighted 0 below)
      if (BRANCH && sidx >= nvalid_p) sidx += skip;
      ml[u] = *(const f32x2*)(a.part_ml + (slot0 + sidx) * 2);
      o[u] = a.part_o[(slot0 + sidx) * AD_D + d];
    }
    float mb = M;
#pragma unroll
    for (int u = 0; u < U; ++u) mb = s0 + u < nvalid ? fmaxf(mb, ml[u][0]) : mb;
    const float mr = (APPEND || BRANCH) && mb == -INFINITY ? 0.f : mb;       // (APPEND: no split so far holds a key this column sees)
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
  a.o[(int64_t)b * a.osb + (APPEND || BRANCH ? (int64_t)tok * a.osl : 0) + (int64_t)h * a.osh + d] = from_f32<bf16_t>(any ? O / L : 0.f);
  if (a.lse && d == 0)          // (B, Hq), continuation (B, Hq, T), branches (B, Hq)
    a.lse[APPEND ? ((int64_t)b * a.Hq + h) * a.T + tok : BRANCH ? (int64_t)blockIdx.x : (int64_t)b * a.Hq + h] =
        any ? (M + __log2f(L)) * 0.6931471805599453f : -INFINITY;
