// The body of the split-KV walk kernels of attn_splitkv.hip (included into each: `a` the DecArgs, APPEND and BRANCH what the
// kernel is instantiated for).
  extern __shared__ __attribute__((aligned(16))) unsigned char ad_smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n = lane & 15, g = lane >> 4;                 // MFMA column (q-head / key row / d column) and k-quarter
  int split, b, hk, hb, nh, col, tok, head, Lk, chunk;
  bool sfx = false;                                       // BRANCH: a suffix work-group
  if constexpr (BRANCH) {
    const BranchWork w = branch_work(a, (int)blockIdx.x);
    sfx = w.sfx; split = w.split; b = 0; hk = w.hk; hb = w.hb; Lk = w.Lk; chunk = w.chunk;
    nh = min(16, (sfx ? a.gq : a.ncols) - 16 * hb);
    col = 16 * hb + min(n, nh - 1);                       // prefix: (branch, head) of the kv-head; suffix: head alone
    tok = sfx ? w.br : col / a.gq;                        // the BRANCH, in the place of the continuation's token
    head = hk * a.gq + (sfx ? col : col % a.gq);
  } else {
    split = blockIdx.x, b = blockIdx.z;
    hk = blockIdx.y / a.hblocks, hb = blockIdx.y % a.hblocks;
    nh = min(16, (APPEND ? a.ncols : a.gq) - 16 * hb);     // columns of this block
    col = 16 * hb + min(n, nh - 1);                       // this lane's column of the kv-head: (token, head)
    tok = APPEND ? col / a.gq : 0, head = hk * a.gq + (APPEND ? col % a.gq : col);
    split_of(a, b, Lk, chunk);
  }
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
    const bf16_t* qp = a.q + (int64_t)b * a.qsb + (APPEND || BRANCH ? (int64_t)tok * a.qsl : 0) + (int64_t)head * a.qsh + 8 * g;
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
  const bf16_t *kg, *vg;
  if constexpr (BRANCH) {
    kg = sfx ? a.ks + (int64_t)tok * a.kssb + (int64_t)hk * a.kssh + (int64_t)r0 * a.kssl
             : a.k + (int64_t)hk * a.ksh + (int64_t)r0 * a.ksl;
    vg = sfx ? a.vs + (int64_t)tok * a.vssb + (int64_t)hk * a.vssh + (int64_t)r0 * a.vssl
             : a.v + (int64_t)hk * a.vsh + (int64_t)r0 * a.vsl;
  } else {
    kg = a.k + (int64_t)b * a.ksb + (int64_t)hk * a.ksh + (int64_t)r0 * a.ksl;
    vg = a.v + (int64_t)b * a.vsb + (int64_t)hk * a.vsh + (int64_t)r0 * a.vsl;
  }
  // bytes between two K / V rows
  auto krowb = [&]() __attribute__((always_inline)) {
    if constexpr (BRANCH) return (unsigned)((sfx ? a.kssl : a.ksl) * 2);
    else return (unsigned)(a.ksl * 2);
  };
  auto vrowb = [&]() __attribute__((always_inline)) {
    if constexpr (BRANCH) return (unsigned)((sfx ? a.vssl : a.vsl) * 2);
    else return (unsigned)(a.vsl * 2);
  };
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
      glds16(kbp, (unsigned)key * krowb() + ch * 16u, dst + (unsigned)(i8 * 1024));
    }
#pragma unroll
    for (int i8 = 0; i8 < 8; ++i8) {
      const int key = min(kb + 4 * i8 + crow, last);
      const unsigned ch = vchunk ^ (unsigned)(8 * ((i8 >> 1) & 1));
      glds16(vbp, (unsigned)key * vrowb() + ch * 16u, dst + (unsigned)(AD_TILE + i8 * 1024));
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
    const float m_ref = (APPEND || BRANCH) && m_new == -INFINITY ? 0.f : m_new;
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
  const float m_ref = (APPEND || BRANCH) && m_tot == -INFINITY ? 0.f : m_tot;
  float sc[AD_NW], l_tot = 0.f;
#pragma unroll
  for (int w = 0; w < AD_NW; ++w) {
    sc[w] = __builtin_amdgcn_exp2f(mm[w * 64 + lane] - m_ref);                    // exp2(-inf) = 0 for idle waves
    l_tot += sc[w] * ml[w * 64 + lane];
  }
  if (n < nh) {
    int64_t slot;
    if constexpr (BRANCH) slot = ((int64_t)tok * a.Hq + head) * (a.nsplit + a.nsplit_s) + (sfx ? a.nsplit : 0) + split;
    else slot = slot_of<APPEND>(a, b, tok, head) + split;
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
