// Body of the fused MLP kernels of mlp_fused.hip: included once per kernel, inside the kernel's braces, with D_, DBG, GS, PROJ, SPREAD, PITCH and
// PLAN visible as compile-time constants and the kernel's argument named a (MlpArgs).  Text, not a function: behind a __forceinline__
// function the argument struct is copied and every PROJ kernel spills (28-36 bytes of scratch); included, each kernel is the code it would be
// with the body written out in it.
  static_assert(PROJ || !PITCH, "the row pitch belongs to the PROJ variant");
  static_assert((PROJ && !PITCH) || !PLAN, "the row map belongs to the dense PROJ variant");
  constexpr int KS1 = D_ / BK;            // 12 k-steps of GEMM1
  constexpr int KQ = 4;                   // k-steps per GEMM1 stage
  constexpr int G1S = 2 * (KS1 / KQ);     // 6 GEMM1 stages per chunk: 2 pair-groups x 3 k-ranges
  constexpr int TH = D_ / RT;             // 3 output thirds of GEMM2
  constexpr int NT2 = D_ / 16;            // 24 output tiles per wave
  constexpr int G2S = (CH / BK) * TH;     // 6 GEMM2 stages per chunk: W2[128 outputs] x 32 hidden
  constexpr int SPC = G1S + G2S;          // ring stages per hidden chunk (12)
  constexpr int NG = NS / GS;             // groups in the ring: 1 being read, 1 cooling down, NG - 2 in flight
  constexpr int PD = (NG - 2) * GS;       // stages in flight after a refill
  static_assert(KS1 % KQ == 0 && D_ % RT == 0 && SPC % GS == 0 && NS % GS == 0 && NG >= 3, "layout");
  extern __shared__ __attribute__((aligned(16))) bf16_t sm[];
  float* sb1 = reinterpret_cast<float*>(sm + NS * TILE_EL);
  float* sb2 = sb1 + a.Hd;
  float* sgam = sb2 + D_;                 // LayerNorm affine, read per k-step in the prologue: 48 16-byte reads per lane that came from
  float* sbet = sgam + D_;                // L1 / L2 in groups of 8 behind a scheduling barrier = six exposed round trips per tile
  float* sbp = sbet + D_;                 // PROJ: bias of the attention projection
  float* sgn = sbp + D_;                  // PROJ + ln_next: the next block's norm1 affine
  float* sbn = sgn + D_;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);     // SGPR: LDS-DMA destinations (M0) stay scalar arithmetic
  const int l15 = lane & 15, lg = lane >> 4;
  const int nch = a.Hd / CH;
  for (int i = tid; i < a.Hd; i += 512) sb1[i] = a.b1[i];
  for (int i = tid; i < D_; i += 512) { sb2[i] = a.b2[i]; sgam[i] = a.gamma[i]; sbet[i] = a.beta[i]; }
  if constexpr (PROJ) {
    for (int i = tid; i < D_; i += 512) sbp[i] = a.bp[i];
    if (a.ln_next) for (int i = tid; i < D_; i += 512) { sgn[i] = a.gamma_n[i]; sbn[i] = a.beta_n[i]; }
  }
  __syncthreads();

  // ---- producer: one LDS-DMA instruction (16 LDS rows x 64 B) per wave and stage.  Buffer addressing: (SGPR resource
  // descriptor) + (32-bit per-lane byte offset) + (uniform byte offset in an SGPR); num_records = the weight's size, so an
  // offset of 2^31 is out of range: the load moves nothing but still counts in vmcnt.
  const int pr = 16 * wave + (lane >> 2);                        // LDS row of this lane's 16 B
  const int psl = ((lane & 3) ^ swz(pr)) * 8;
  // GEMM1 stage (u, kt): LDS row 32 s + h = W1[64 c + 32 u + h][32 (4 kt + s) ..],  s = k-step inside the stage, h < 32
  // GEMM2 stage (u, th): LDS row r = W2[128 th + r][64 c + 32 u ..]
  const int lo1 = ((pr & 31) * D_ + (pr >> 5) * BK + psl) * 2;
  const int lo2 = (pr * a.Hd + psl) * 2;
  const int pdst = 16 * wave * BK;
  const int wbytes = a.Hd * D_ * 2;
  const __amdgpu_buffer_rsrc_t r1 = __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16_t*>(a.W1), 0, wbytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t r2 = __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16_t*>(a.W2), 0, wbytes, 0x00020000);
  constexpr int OOB = 0x7ffffff0;
  // PROJ: the ring sequence starts with VOFF = 3 "virtual chunks" of SPC stages that carry the projection weight Wp: stage j of virtual
  // chunk v is the LDS tile  r -> Wp[128 v + r][32 j ..]  (the shape of a GEMM2 stage with row pitch D); chunk indices below are virtual
  // (MLP chunk c = virtual chunk c + VOFF) so that slot arithmetic and the look-ahead of the refills run straight through the seam
  constexpr int VOFF = PROJ ? TH : 0;
  int nchv = nch + VOFF;                  // (PLAN: per tile -- VOFF for a light tile, whose ring stages past the projection are the usual
                                          // out-of-range no-ops that still count in vmcnt)
  const __amdgpu_buffer_rsrc_t rp = __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16_t*>(PROJ ? a.Wp : a.W2), 0, D_ * D_ * 2, 0x00020000);
  const int lop = (pr * D_ + psl) * 2;
  auto issue = [&](int cv, int j, int slot) {                // stage j of virtual chunk cv (j is a compile-time constant at every call)
    if (DBG & 2) return;
    lds_void* dst = (lds_void*)(sm + slot * TILE_EL + pdst);
    const bool valid = cv < nchv;
    if (PROJ && cv < VOFF) {
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rp, dst, 16, lop, (cv * RT * D_ + j * BK) * 2, 0, 0);
      return;
    }
    const int c = cv - VOFF;
    if (j < G1S) {
      const int u = j / (KS1 / KQ), kt = j % (KS1 / KQ);
      __builtin_amdgcn_raw_ptr_buffer_load_lds(r1, dst, 16, valid ? lo1 : OOB, ((c * CH + 32 * u) * D_ + kt * KQ * BK) * 2, 0, 0);
    } else {
      const int jj = j - G1S, u = jj / TH, th = jj % TH;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(r2, dst, 16, valid ? lo2 : OOB, (th * RT * a.Hd + c * CH + u * BK) * 2, 0, 0);
    }
  };

  // ---- consumer fragment offsets (elements) inside a ring tile
  // GEMM2 (and any plain tile): row l15 of 16-row tile t: + t * 16 * BK
  const int fo2 = l15 * BK + ((lg ^ swz(l15)) << 3);
  // GEMM1: A-tile row i = l15 <- hidden 8 (i>>2) + (i&3) (+4 for tile Q) of the 32-row sub-tile of k-step s: + s * 32 * BK
  const int h1 = 8 * (l15 >> 2) + (l15 & 3);
  const int fo1p = h1 * BK + ((lg ^ swz(h1)) << 3);
  const int fo1q = (h1 + 4) * BK + ((lg ^ swz(h1 + 4)) << 3);

  const size_t rpitch = PITCH ? (size_t)a.pitch : (size_t)D_;      // elements between rows of x, xo and ao
  const int ntiles = (a.M + FBM - 1) / FBM;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int m = tile * FBM + wave * 16 + l15;
    const int mc = min(m, a.M - 1);
    // PLAN: physical row pm and sample si of virtual row mc; heavy is tile-uniform (scalar)
    int pm = mc, si = 0;
    bool heavy = true;
    if constexpr (PLAN) {
      const int q = mc / a.rows_per_sample;
      si = (int)min((unsigned)a.plan[1 + q], (unsigned)(a.nsamp - 1));        // (a table that is no permutation must not become an address)
      pm = si * a.rows_per_sample + (mc - q * a.rows_per_sample);
      heavy = (long long)tile * FBM < (long long)a.plan[0] * a.rows_per_sample;
      nchv = heavy ? nch + VOFF : VOFF;
    }
    MDBG_T(0);
    // ---- LayerNorm of the wave's 16 rows, straight into MFMA B-fragments: lane holds x[m][32 s + 8 g .. +7], s = 0..11
    u32x4_t xn[KS1];
    if constexpr (!PROJ) {
      const float* xr = a.x + (size_t)mc * D_ + 8 * lg;
      f32x4_t v[2 * KS1];
      float s = 0.f;
#pragma unroll
      for (int k = 0; k < KS1; ++k) {
        v[2 * k] = *reinterpret_cast<const f32x4_t*>(xr + 32 * k);
        v[2 * k + 1] = *reinterpret_cast<const f32x4_t*>(xr + 32 * k + 4);
      }
#pragma unroll
      for (int k = 0; k < 2 * KS1; ++k) s += (v[k][0] + v[k][1]) + (v[k][2] + v[k][3]);
      s += __shfl_xor(s, 16, 64);
      s += __shfl_xor(s, 32, 64);
      const float mu = s * (1.0f / D_);
      float q = 0.f;
#pragma unroll
      for (int k = 0; k < 2 * KS1; ++k) {
#pragma unroll
        for (int e = 0; e < 4; ++e) { const float d = v[k][e] - mu; q += d * d; }
      }
      q += __shfl_xor(q, 16, 64);
      q += __shfl_xor(q, 32, 64);
      const float rs = rsqrtf(q * (1.0f / D_) + a.eps);
      if (a.save_rows > 0 && m < a.save_rows && lg == 0) { a.s_mean[m] = mu; a.s_rstd[m] = rs; }
#pragma unroll
      for (int k = 0; k < KS1; ++k) {
        const f32x4_t g0 = *reinterpret_cast<const f32x4_t*>(sgam + 32 * k + 8 * lg);
        const f32x4_t g1 = *reinterpret_cast<const f32x4_t*>(sgam + 32 * k + 8 * lg + 4);
        const f32x4_t b0 = *reinterpret_cast<const f32x4_t*>(sbet + 32 * k + 8 * lg);
        const f32x4_t b1 = *reinterpret_cast<const f32x4_t*>(sbet + 32 * k + 8 * lg + 4);
        const f32x4_t p = v[2 * k], r = v[2 * k + 1];
        xn[k] = u32x4_t{pack_bf2((p[0] - mu) * rs * g0[0] + b0[0], (p[1] - mu) * rs * g0[1] + b0[1]),
                        pack_bf2((p[2] - mu) * rs * g0[2] + b0[2], (p[3] - mu) * rs * g0[3] + b0[3]),
                        pack_bf2((r[0] - mu) * rs * g1[0] + b1[0], (r[1] - mu) * rs * g1[1] + b1[1]),
                        pack_bf2((r[2] - mu) * rs * g1[2] + b1[2], (r[3] - mu) * rs * g1[3] + b1[3])};
        if (k & 1) __builtin_amdgcn_sched_barrier(0);     // keep the scheduler from hoisting all 48 affine loads (spills)
      }
    }
    const bool save_tile = !PROJ && a.save_rows > 0 && tile * FBM + wave * 16 < a.save_rows;      // wave-uniform
    if (save_tile && m < a.save_rows) {                                                     // norm2 output of the gradient rows
      bf16_t* lr = a.s_ln2 + (size_t)m * D_ + 8 * lg;
#pragma unroll
      for (int k = 0; k < KS1; ++k) *reinterpret_cast<u32x4_t*>(lr + 32 * k) = xn[k];
    }
    // PROJ: the attention output rows of the wave as MFMA B-fragments (lane holds ao[m][32 s + 8 g .. + 7])
    u32x4_t aof[PROJ ? KS1 : 1];
    if constexpr (PROJ) {
      const bf16_t* ar = a.ao + (size_t)pm * rpitch + 8 * lg;
#pragma unroll
      for (int k = 0; k < KS1; ++k) aof[k] = *reinterpret_cast<const u32x4_t*>(ar + 32 * k);
    }
    // PROJ: the residual stream never makes a round trip through memory inside the launch.  The rows' x enters as the START VALUE of the
    // output accumulators (lane (l15 = row, lg) holds columns 16 t + 4 lg + r), the projection accumulates on top of it, and the same
    // registers, then holding x1, are the start value of fc2.  The per-row drop-path factors (vit.py:163, :165; 0 or 1 / keep_prob) ride on
    // the B operands of the two products -- the bf16 attention-output fragments and the bf16 GELU output -- since a B column is one row:
    // a factor of 1 (block 0, eval) is exact, 0 leaves x untouched, any other means bf16(rs * value) instead of rs * bf16(value): for GELU
    // the ONE rounding of the operand either way; for ao a second one unless the attention launch applied rs1 before ITS rounding
    // (ao_scaled: srhip_attn_block_fused out_scale).
    float rs1v = 1.0f, rs2v = 1.0f;
    f32x4_t acc2[NT2];
    if constexpr (PROJ) {
      if (a.row_scale1) rs1v = a.row_scale1[PLAN ? si : mc / a.rows_per_sample];
      if (a.row_scale) rs2v = a.row_scale[PLAN ? si : mc / a.rows_per_sample];
      const float* xr = a.x + (size_t)pm * rpitch + 4 * lg;
#pragma unroll
      for (int t = 0; t < NT2; ++t) acc2[t] = *reinterpret_cast<const f32x4_t*>(xr + 16 * t);
      if (rs1v != 1.0f && !a.ao_scaled) {
#pragma unroll
        for (int k = 0; k < KS1; ++k)
#pragma unroll
          for (int e = 0; e < 4; ++e)
            aof[k][e] = pack_bf2(rs1v * __builtin_bit_cast(float, aof[k][e] << 16), rs1v * __builtin_bit_cast(float, aof[k][e] & 0xffff0000u));
      }
    }
    __syncthreads();                       // previous tile's ring reads are over (and sb1/sb2 are written)
    MDBG_T(1);
#pragma unroll
    for (int p = 0; p < PD; ++p) issue(p / SPC, p % SPC, p);   // groups 0 .. NG-3

    __builtin_amdgcn_sched_barrier(0);     // the accumulators must not become live (zeroed early) across the LayerNorm above
    if constexpr (!PROJ) {
#pragma unroll
      for (int t = 0; t < NT2; ++t) acc2[t] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    } else {                               // + rs1 * bp while the first ring stages are in flight
#pragma unroll
      for (int t = 0; t < NT2; ++t) {
        const f32x4_t bb = *reinterpret_cast<const f32x4_t*>(sbp + 16 * t + 4 * lg);
        acc2[t][0] += rs1v * bb[0]; acc2[t][1] += rs1v * bb[1]; acc2[t][2] += rs1v * bb[2]; acc2[t][3] += rs1v * bb[3];
      }
    }
    f32x4_t acc1[4];                       // [2 u + {P, Q}], started at the fc1 bias of the tile's hidden units
    u32x4_t hf[2];
    u32x4_t fa0[4], fa1[4];                // A fragments of half-stage h of stage j in fa[h]: 4 fragments = 4 MFMAs

    // Group sync before the first read of group (c * SPC + j) / GS: own DMA parts of the group have landed (counted vmcnt:
    // the NG - 3 younger groups may still be in flight), barrier (everybody's parts have), then refill the group that was
    // consumed two syncs ago.
    auto sync_group = [&](auto jc, int c) __attribute__((always_inline)) {
      constexpr int j = decltype(jc)::value;
      static_assert(j % GS == 0, "group start");
      if constexpr ((DBG & 2) == 0) wait_vm<GS*(NG - 3)>();
      __builtin_amdgcn_s_barrier();
      if constexpr (!SPREAD) {
#pragma unroll
        for (int i = 0; i < GS; ++i) {
          const int jn = (j + PD + i) % SPC, cn = c + (j + PD + i) / SPC;
          issue(cn, jn, (c * SPC + j + PD + i) & (NS - 1));
        }
      }
    };
    // SPREAD: stage j of (virtual) chunk c asks for stage j + PD (its slot held stage j + PD - NS, consumed before the last group barrier)
    auto issue_ahead = [&](auto jc, int c, bool late) __attribute__((always_inline)) {
      constexpr int j = decltype(jc)::value;
      // (tried: the SIMD partners -- waves 4-7 -- issuing behind the stage's second MFMA half instead: 30 spilled registers, not built)
      if constexpr (SPREAD == 1) { if (!late) issue(c + (j + PD) / SPC, (j + PD) % SPC, (c * SPC + j + PD) & (NS - 1)); }
    };
    // half-stage (j, h): GEMM1: k-steps 2h, 2h+1 of the stage x tiles P, Q; GEMM2: output tiles 4h .. 4h+3 of the third
    auto read_half = [&](auto jc, auto hc, int c) __attribute__((always_inline)) {
      constexpr int j = decltype(jc)::value, h = decltype(hc)::value;
      u32x4_t(&fa)[4] = h ? fa1 : fa0;
      const bf16_t* st = sm + ((c * SPC + j) & (NS - 1)) * TILE_EL;
      if constexpr ((DBG & 4) != 0) {
#pragma unroll
        for (int t = 0; t < 4; ++t) fa[t] = u32x4_t{(unsigned)(c + t), 1u, 2u, (unsigned)j};
      } else if constexpr (j < G1S) {
#pragma unroll
        for (int s_ = 0; s_ < 2; ++s_) {
          fa[2 * s_] = *reinterpret_cast<const u32x4_t*>(st + fo1p + (2 * h + s_) * 32 * BK);
          fa[2 * s_ + 1] = *reinterpret_cast<const u32x4_t*>(st + fo1q + (2 * h + s_) * 32 * BK);
        }
      } else {
#pragma unroll
        for (int t = 0; t < 4; ++t) fa[t] = *reinterpret_cast<const u32x4_t*>(st + fo2 + (4 * h + t) * 16 * BK);
      }
    };
    // bias + GELU + bf16 pack, ONE element at a time so that it can be threaded between MFMAs: element e = 4 X + r of
    // pair-group u is hidden unit 64 c + 32 u + 8 g + e (X = 0: tile P, 1: tile Q; r = accumulator register).
    float gcarry = 0.f, pcarry = 0.f;
    // accumulator start = fc1 bias: lane (g) holds hidden 64 c + 32 u + 8 g + 4 X + r in register r of tile X
    auto acc1_start = [&](auto uc, auto xc, int c) __attribute__((always_inline)) {
      constexpr int u = decltype(uc)::value, X = decltype(xc)::value;
      acc1[2 * u + X] = *reinterpret_cast<const f32x4_t*>(sb1 + min(c - VOFF, nch - 1) * CH + 32 * u + 8 * lg + 4 * X);
    };
    auto gelu_elem = [&](auto uc, auto ec, int c) __attribute__((always_inline)) {
      constexpr int u = decltype(uc)::value, e = decltype(ec)::value, X = e >> 2, r = e & 3;
      const float v = acc1[2 * u + X][r];
      if constexpr (PROJ && (DBG & 1) == 0) {
        // rows without a backward: the two values of a bf16 pair together, packed fp32 math, no transcendentals (gelu_poly2); the row's
        // drop-path factor (lane column of the B fragment) rides on the result before its rounding
        if constexpr ((e & 1) == 1) {
          const f32x2_t g2 = gelu_poly2(f32x2_t{acc1[2 * u + X][r - 1], v}) * f32x2_t{rs2v, rs2v};
          hf[u][e >> 1] = pack_bf2(g2[0], g2[1]);
        }
      } else {
      float gv;
      if constexpr ((DBG & 1) != 0) gv = v; else gv = gelu_erf(v);
      if constexpr (PROJ) gv *= rs2v;          // drop-path factor of the row (lane column of the B fragment)
      if constexpr ((e & 1) == 0) { gcarry = gv; pcarry = v; } else hf[u][e >> 1] = pack_bf2(gcarry, gv);
      }
      if constexpr ((e & 1) == 1) {
        // gradient rows: keep the fc1 pre-activation and the GELU output (bf16, as the unfused path saves them); rare (8 % of the
        // tiles) and conservative for the counted vmcnt waits (extra younger stores can only make a wait longer)
        if (save_tile && m < a.save_rows) {
          const size_t o = (size_t)m * a.Hd + (c - VOFF) * CH + 32 * u + 8 * lg + (e - 1);
          *reinterpret_cast<uint32_t*>(a.s_pre + o) = pack_bf2(pcarry, v);
          *reinterpret_cast<uint32_t*>(a.s_h + o) = hf[u][e >> 1];
        }
      }
      if constexpr (r == 3) acc1_start(uc, std::integral_constant<int, X>{}, c + 1);     // restart for the next chunk
    };
    // Which GELU elements ride behind half-stage (j, h): group 0 (complete after stage 2) behind stages 3-5, group 1
    // (complete after stage 5, needed by stage 9) behind stages 6-8; 2,1,1,2,1,1 elements per half-stage.
    auto gelu_slot = [&](auto jc, auto hc, auto pc, int c) __attribute__((always_inline)) {
      constexpr int j = decltype(jc)::value, h = decltype(hc)::value, part = decltype(pc)::value;
      if constexpr (j >= 3 && j <= 8 && (DBG & 8) == 0) {
        constexpr int u = (j - 3) / 3, q = 2 * ((j - 3) % 3) + h;           // q = 0..5
        constexpr int first[7] = {0, 2, 3, 4, 6, 7, 8};
        constexpr int e0 = first[q], n = first[q + 1] - first[q];
        if constexpr (part < n) gelu_elem(std::integral_constant<int, u>{}, std::integral_constant<int, e0 + part>{}, c);
      }
    };
    auto mfma_one = [&](auto jc, auto hc, auto tc) __attribute__((always_inline)) {
      constexpr int j = decltype(jc)::value, h = decltype(hc)::value, t = decltype(tc)::value;
      u32x4_t(&fa)[4] = h ? fa1 : fa0;
      if constexpr ((DBG & 8) != 0) {
        asm volatile("" ::"v"(fa[t]));
        if constexpr (j == G1S - 1) { hf[0] = fa[0]; hf[1] = fa[1]; }
      } else if constexpr (j < G1S) {
        constexpr int u = j / (KS1 / KQ), kt = j % (KS1 / KQ);
        acc1[2 * u + (t & 1)] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            __builtin_bit_cast(bf16x8_t, fa[t]), __builtin_bit_cast(bf16x8_t, xn[kt * KQ + 2 * h + (t >> 1)]), acc1[2 * u + (t & 1)],
            0, 0, 0);
      } else {
        constexpr int u = (j - G1S) / TH, th = (j - G1S) % TH;
        acc2[th * 8 + 4 * h + t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            __builtin_bit_cast(bf16x8_t, fa[t]), __builtin_bit_cast(bf16x8_t, hf[u]), acc2[th * 8 + 4 * h + t], 0, 0, 0);
      }
    };
    // half-stage (j, h): 4 MFMAs with up to two GELU elements threaded between them (VALU work in the shadow of the matrix
    // pipe; in one lump it left the pipe idle ~25 % of the time because both waves of a SIMD reach it together)
    auto mfma_half = [&](auto jc, auto hc, int c) __attribute__((always_inline)) {     // c = chunk the stage belongs to
      using T0 = std::integral_constant<int, 0>;
      using T1 = std::integral_constant<int, 1>;
      using T2 = std::integral_constant<int, 2>;
      using T3 = std::integral_constant<int, 3>;
      mfma_one(jc, hc, T0{});
      mfma_one(jc, hc, T1{});
      __builtin_amdgcn_sched_barrier(0);
      gelu_slot(jc, hc, T0{}, c);
      __builtin_amdgcn_sched_barrier(0);
      mfma_one(jc, hc, T2{});
      mfma_one(jc, hc, T3{});
      __builtin_amdgcn_sched_barrier(0);
      gelu_slot(jc, hc, T1{}, c);
      __builtin_amdgcn_sched_barrier(0);
    };
    using H0 = std::integral_constant<int, 0>;
    using H1 = std::integral_constant<int, 1>;
    if constexpr (PROJ) {
      // ---- attention output projection: VOFF virtual chunks of SPC stages, stage (v, j) = Wp rows 128 v .. x k-step j, the GEMM2 stage
      // shape: 8 MFMAs acc2[8 v + t] += Wp tile t . ao fragment j, same software pipeline as below
      auto read_half_p = [&](auto jc, auto hc, int cv) __attribute__((always_inline)) {
        constexpr int j = decltype(jc)::value, h = decltype(hc)::value;
        u32x4_t(&fa)[4] = h ? fa1 : fa0;
        const bf16_t* st = sm + ((cv * SPC + j) & (NS - 1)) * TILE_EL;
#pragma unroll
        for (int t = 0; t < 4; ++t) fa[t] = *reinterpret_cast<const u32x4_t*>(st + fo2 + (4 * h + t) * 16 * BK);
      };
      sync_group(H0{}, 0);
      read_half_p(H0{}, H0{}, 0);
      static_for<VOFF>([&](auto vc) __attribute__((always_inline)) {
        constexpr int v = decltype(vc)::value;
        static_for<SPC>([&](auto jc) __attribute__((always_inline)) {
          constexpr int j = decltype(jc)::value;
          constexpr int jn = (j + 1) % SPC, vn = v + (j + 1) / SPC;
          read_half_p(jc, H1{}, v);
#pragma unroll
          for (int t = 0; t < 4; ++t)
            acc2[v * 8 + t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, fa0[t]), __builtin_bit_cast(bf16x8_t, aof[j]),
                                                                       acc2[v * 8 + t], 0, 0, 0);
          __builtin_amdgcn_sched_barrier(0);
          issue_ahead(jc, v, false);
          if constexpr (jn % GS == 0) sync_group(std::integral_constant<int, jn>{}, vn);
          if constexpr (vn == VOFF) read_half(std::integral_constant<int, 0>{}, H0{}, vn);       // the seam: first MLP stage (GEMM1 fragments)
          else read_half_p(std::integral_constant<int, jn>{}, H0{}, vn);
#pragma unroll
          for (int t = 0; t < 4; ++t)
            acc2[v * 8 + 4 + t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, fa1[t]), __builtin_bit_cast(bf16x8_t, aof[j]),
                                                                           acc2[v * 8 + 4 + t], 0, 0, 0);
          __builtin_amdgcn_sched_barrier(0);
          issue_ahead(jc, v, true);
        });
      });
      MDBG_T(4);
      // ---- first residual + LayerNorm, from the accumulator layout: lane (l15 = row, lg) holds columns 16 t + 4 lg + r of its row.
      //   acc2 = x + rs1 * (ao Wp^T + bp) = x1 (vit.py:163) stays in the accumulators as the start value of fc2 and is normalised from
      //   there; the bf16 pairs are moved into the B-fragment layout (lane holds columns 32 s + 8 lg .. + 7) by two row
      //   swaps per register: for the tile pair (2 s, 2 s + 1)
      //   permlane32_swap(P, Q) = {P0 P1 Q0 Q1, P2 P3 Q2 Q3} (rows = lane groups), then permlane16_swap of those two
      //   = {P0 P2 Q0 Q2, P1 P3 Q1 Q3}: exactly columns 8 lg .. + 3 and 8 lg + 4 .. + 7 of the k-step for lane group lg.
      // (PLAN, light tile: x1 is the rows' result -- nothing below runs until the epilogue)
      if (PLAN && !heavy) goto epilogue;
      {
        float sum = 0.f;
#pragma unroll
        for (int t = 0; t < NT2; ++t) sum += (acc2[t][0] + acc2[t][1]) + (acc2[t][2] + acc2[t][3]);
        const float mu = rows_sum4(sum) * (1.0f / D_);
        float q = 0.f;
#pragma unroll
        for (int t = 0; t < NT2; ++t)
#pragma unroll
          for (int e = 0; e < 4; ++e) { const float d = acc2[t][e] - mu; q += d * d; }
        const float rs = rsqrtf(rows_sum4(q) * (1.0f / D_) + a.eps);
        // (the 48 affine reads must not all be issued up front: 192 live registers = spills whose reloads stall the weight ring; the offset
        // of every k-step is made to depend on the fragment the previous one produced)
        int ko = 4 * lg;
        asm volatile("" : "+v"(ko) : "v"(rs));
#pragma unroll
        for (int sI = 0; sI < KS1; ++sI) {
          if (sI > 0) asm volatile("" : "+v"(ko) : "v"(xn[sI - 1][3]));
          unsigned pk[2][2];                         // [tile of the pair][dword]
#pragma unroll
          for (int e = 0; e < 2; ++e) {
            const int t = 2 * sI + e;
            const f32x4_t g4 = *reinterpret_cast<const f32x4_t*>(sgam + 16 * t + ko);
            const f32x4_t b4 = *reinterpret_cast<const f32x4_t*>(sbet + 16 * t + ko);
            pk[e][0] = pack_bf2((acc2[t][0] - mu) * rs * g4[0] + b4[0], (acc2[t][1] - mu) * rs * g4[1] + b4[1]);
            pk[e][1] = pack_bf2((acc2[t][2] - mu) * rs * g4[2] + b4[2], (acc2[t][3] - mu) * rs * g4[3] + b4[3]);
          }
          unsigned out4[4];
#pragma unroll
          for (int d = 0; d < 2; ++d) {
            const auto w32 = __builtin_amdgcn_permlane32_swap(pk[0][d], pk[1][d], false, false);
            const auto w16 = __builtin_amdgcn_permlane16_swap(w32[0], w32[1], false, false);
            out4[d] = w16[0];                        // columns 8 lg + 2 d, + 1
            out4[2 + d] = w16[1];                    // columns 8 lg + 4 + 2 d, + 1
          }
          xn[sI] = u32x4_t{out4[0], out4[1], out4[2], out4[3]};
          if (sI & 1) __builtin_amdgcn_sched_barrier(0);
        }
      }
      MDBG_T(5);
      // fc2 accumulates on x1 + rs2 * b2: the block's output needs no epilogue arithmetic
#pragma unroll
      for (int t = 0; t < NT2; ++t) {
        const f32x4_t bb = *reinterpret_cast<const f32x4_t*>(sb2 + 16 * t + 4 * lg);
        acc2[t][0] += rs2v * bb[0]; acc2[t][1] += rs2v * bb[1]; acc2[t][2] += rs2v * bb[2]; acc2[t][3] += rs2v * bb[3];
      }
    }
    {
      using I0 = std::integral_constant<int, 0>;
      using I1 = std::integral_constant<int, 1>;
      acc1_start(I0{}, I0{}, VOFF); acc1_start(I0{}, I1{}, VOFF); acc1_start(I1{}, I0{}, VOFF); acc1_start(I1{}, I1{}, VOFF);
    }
    if constexpr (!PROJ) {
      sync_group(H0{}, 0);
      read_half(H0{}, H0{}, 0);
    }
    for (int c = VOFF; c < nchv; ++c)
      static_for<SPC>([&](auto jc) __attribute__((always_inline)) {
        constexpr int j = decltype(jc)::value;
        constexpr int jn = (j + 1) % SPC;
        const int cn = c + (j + 1) / SPC;
        read_half(jc, H1{}, c);
        mfma_half(jc, H0{}, c);
        issue_ahead(jc, c, false);
        if constexpr (jn % GS == 0) sync_group(std::integral_constant<int, jn>{}, cn);
        read_half(std::integral_constant<int, jn>{}, H0{}, cn);  // (one stage past the end: a stale slot, never multiplied)
        mfma_half(jc, H1{}, c);
        issue_ahead(jc, c, true);
      });
  epilogue:
    MDBG_T(2);
    // ---- epilogue: lane holds y[m][16 t + 4 g + r]
    int pme = mc;
    if constexpr (PLAN) {
      // the physical row again, from a lane id read HERE: carried across the main loop it would be one live register more than the kernel has
      int ln_;
      asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(ln_));
      const int me = min(tile * FBM + wave * 16 + (ln_ & 15), a.M - 1), q = me / a.rows_per_sample;
      const int se = (int)min((unsigned)a.plan[1 + q], (unsigned)(a.nsamp - 1));
      pme = se * a.rows_per_sample + (me - q * a.rows_per_sample);
    }
    if (PROJ && a.ln_next) {                // wave-uniform: the rows leave as fp32 (residual stream) AND normalised for the next block
      float* xw = a.xo + (size_t)pme * rpitch + 4 * lg;
      float sum = 0.f;
#pragma unroll
      for (int t = 0; t < NT2; ++t) {
        const f32x4_t xv = acc2[t];
        if (m < a.M) *reinterpret_cast<f32x4_t*>(xw + 16 * t) = xv;
        sum += (xv[0] + xv[1]) + (xv[2] + xv[3]);
      }
      const float mu = rows_sum4(sum) * (1.0f / D_);
      float q = 0.f;
#pragma unroll
      for (int t = 0; t < NT2; ++t)
#pragma unroll
        for (int e = 0; e < 4; ++e) { const float d = acc2[t][e] - mu; q += d * d; }
      const float rs = rsqrtf(rows_sum4(q) * (1.0f / D_) + a.eps);
      bf16_t* lw = a.ln_next + (size_t)pme * D_ + 8 * lg;
      int ko = 4 * lg;
      asm volatile("" : "+v"(ko) : "v"(rs));
      unsigned chain = 0;
#pragma unroll
      for (int sI = 0; sI < KS1; ++sI) {     // same re-layout as after the projection: 16 bytes per lane and k-step leave
        if (sI > 0) asm volatile("" : "+v"(ko) : "v"(chain));
        unsigned pk[2][2];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          const int t = 2 * sI + e;
          const f32x4_t g4 = *reinterpret_cast<const f32x4_t*>(sgn + 16 * t + ko);
          const f32x4_t b4 = *reinterpret_cast<const f32x4_t*>(sbn + 16 * t + ko);
          pk[e][0] = pack_bf2((acc2[t][0] - mu) * rs * g4[0] + b4[0], (acc2[t][1] - mu) * rs * g4[1] + b4[1]);
          pk[e][1] = pack_bf2((acc2[t][2] - mu) * rs * g4[2] + b4[2], (acc2[t][3] - mu) * rs * g4[3] + b4[3]);
        }
        unsigned out4[4];
#pragma unroll
        for (int d = 0; d < 2; ++d) {
          const auto w32 = __builtin_amdgcn_permlane32_swap(pk[0][d], pk[1][d], false, false);
          const auto w16 = __builtin_amdgcn_permlane16_swap(w32[0], w32[1], false, false);
          out4[d] = w16[0];
          out4[2 + d] = w16[1];
        }
        chain = out4[3];
        if (m < a.M) *reinterpret_cast<u32x4_t*>(lw + 32 * sI) = u32x4_t{out4[0], out4[1], out4[2], out4[3]};
      }
    } else if (PROJ) {
      float* xw = a.xo + (size_t)pme * rpitch + 4 * lg;
      if (m < a.M) {
#pragma unroll
        for (int t = 0; t < NT2; ++t) *reinterpret_cast<f32x4_t*>(xw + 16 * t) = acc2[t];
      }
    } else if (m < a.M) {
      const float rsc = a.row_scale ? a.row_scale[m / a.rows_per_sample] : 1.0f;
      const float* xr = a.x + (size_t)m * D_ + 4 * lg;
      float* xw = a.xo + (size_t)m * D_ + 4 * lg;
#pragma unroll
      for (int t = 0; t < NT2; ++t) {
        const f32x4_t bb = *reinterpret_cast<const f32x4_t*>(sb2 + 16 * t + 4 * lg);
        f32x4_t xv = *reinterpret_cast<const f32x4_t*>(xr + 16 * t);
        xv[0] += rsc * (acc2[t][0] + bb[0]); xv[1] += rsc * (acc2[t][1] + bb[1]);
        xv[2] += rsc * (acc2[t][2] + bb[2]); xv[3] += rsc * (acc2[t][3] + bb[3]);
        *reinterpret_cast<f32x4_t*>(xw + 16 * t) = xv;
      }
    }
#ifdef SRHIP_TUNING
    __builtin_amdgcn_s_waitcnt(0);          // stores issued AND acknowledged
    __syncthreads();
    MDBG_T(3);
#endif
  }
