// Body of the head-dim-64 attention backward kernels, included by attention.hip inside each
// __global__ definition (never on its own).  The including function provides the argument
// `AttnBwdArgs a` and the compile-time constants DROP, CAUSAL, MULTI, GL and REL; the design
// notes are in front of attn_bwd_d64_kernel in attention.hip.  It is a textual include and not a
// device function because a function call, even inlined, changes how the kernel arguments are
// loaded and with that the register allocation of the existing kernels.
  // LDS: Q tiles R x 4K | dO tiles R x 4K | K block 16K | V block 16K | dS^T 2 x 8K | lse, delta
  // (R = 2 register-staged: 2 x 32 rows each; R = 3 with GL: all <= 128 rows each)
  // The per-q-tile inputs (Q, dO, lse, delta) and dS^T are multi-buffered, so one barrier per
  // q-tile orders everything: tile t+2 is staged into the buffers tile t (t - 1 with GL) has
  // released, and dQ needs no cross-wave reduction (each wave owns 16 queries x 32 d of the
  // tile's dQ and sums over all 128 keys itself).
  static_assert(!(GL && MULTI), "GL: single key block only");
  static_assert(!(GL && REL), "REL: register-staged forms only");
  constexpr int QR = GL ? 3 : 2;
  constexpr int QB = QR * 4096;
  __shared__ __attribute__((aligned(16))) char smem[2 * QB + 16384 + 16384 + 16384 + (GL ? 1024 : 512)];
  char* Qs = smem;
  char* dOs = smem + QB;
  char* Ks = smem + 2 * QB;
  char* Vs = Ks + 16384;
  char* dSs = Vs + 16384;
  float* lse_s = reinterpret_cast<float*>(dSs + 16384);       // [2][32] or [128]
  float* delta_s = lse_s + (GL ? 128 : 64);                   // [2][32] or [128]
  // REL: the two windows interleaved (dynamic LDS, 8 W bytes): [2 i] the log2-scaled bias of
  // window offset i, [2 i + 1] the fp32 d_rel sum -- one address register serves both, every
  // register's offset from it is an immediate, and a 32-lane half still covers 32 banks
  extern __shared__ float bwd_rel_dyn[];

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 31, hh = lane >> 5;
  const int bh = blockIdx.y, b = bh / a.H, h = bh % a.H;
  const int k0 = blockIdx.x * 128;
  const int key_l = k0 + w * 32 + r;  // this lane's key (MFMA column)
  const bool kvalid = key_l < a.Sk;
  const float LOG2E = 1.4426950408889634f;

  const bf16_t* kp = a.k + b * a.k_sb + h * a.k_sh;
  const bf16_t* vp = a.v + b * a.v_sb + h * a.v_sh;
  // K and V blocks (128 keys) into LDS: row reads give the B operands of S = Q K^T and
  // dP = dO V^T (re-read per q-tile instead of pinning 32 VGPRs), transposed reads of K
  // give dQ's operand
  if constexpr (GL) {
    // wave w DMAs rows 32 w + 8 i + (lane >> 3); lane l lands at physical chunk l & 7, so it
    // fetches logical chunk (l & 7) ^ rev3(((row >> 1) & 7)) = (l & 7) ^ rev3((4 i + (l >> 4)) & 7).
    // Rows past Sk read row Sk - 1 (finite; their -inf key bias zeroes them)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = 32 * w + 8 * i + (lane >> 3);
      const unsigned key = (unsigned)min(k0 + row, a.Sk - 1);
      const unsigned c = (unsigned)((lane & 7) ^ rev3((4 * i + (lane >> 4)) & 7));
      at_glds16s(kp, (key * (unsigned)a.k_ss + c * 8u) * 2u, Ks + (32 * w + 8 * i) * 128);
      at_glds16s(vp, (key * (unsigned)a.v_ss + c * 8u) * 2u, Vs + (32 * w + 8 * i) * 128);
    }
  } else {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c = tid + 256 * i;
    const int row = c >> 3, ch = c & 7;
    const int key = k0 + row;
    const bool ok = key < a.Sk;
    const u16x8 kv = ok ? *reinterpret_cast<const u16x8*>(kp + (long)key * a.k_ss + ch * 8) : u16x8(0);
    const u16x8 vv = ok ? *reinterpret_cast<const u16x8*>(vp + (long)key * a.v_ss + ch * 8) : u16x8(0);
    *reinterpret_cast<u16x8*>(Ks + swz(row, ch)) = kv;
    *reinterpret_cast<u16x8*>(Vs + swz(row, ch)) = vv;
  }
  }
  const int krow = w * 32 + r;   // this lane's key row inside the block
  float kb2 = 0.f;
  if (a.kbias && kvalid) kb2 = a.kbias[b * a.kb_sb + key_l] * LOG2E;
  if (!kvalid) kb2 = -INFINITY;

  f32x16 dV0, dV1, dK0, dK1;
#pragma unroll
  for (int i = 0; i < 16; ++i) { dV0[i] = 0.f; dV1[i] = 0.f; dK0[i] = 0.f; dK1[i] = 0.f; }

  const bf16_t* qbase = a.q + b * a.q_sb + h * a.q_sh;
  const bf16_t* dobase = a.dO + b * a.do_sb + h * a.do_sh;
  const bf16_t* obase = a.o + b * a.o_sb + h * a.o_sh;
  bf16_t* dqbase = a.dq + b * a.dq_sb + h * a.dq_sh;
  const int trow = (lane >> 2) & 3;
  const int tcol = ((lane >> 4) & 1) * 16 + (lane & 3) * 4;
  const int nq = (a.Sq + 31) / 32;
  if constexpr (REL) {
    // both windows; the barrier before the q-tile loop publishes them
    const int W = 32 * nq + 127, win0 = k0 - 32 * nq + 1 + a.rel_base;
    const float* relh = a.relb + h * a.relb_sh;
    for (int i = tid; i < W; i += 256) {
      const int gi = win0 + i;
      bwd_rel_dyn[2 * i] = (gi >= 0 && gi < a.relb_len) ? relh[gi] * LOG2E : 0.f;
      bwd_rel_dyn[2 * i + 1] = 0.f;
    }
  }
  // MULTI: Sk > 128, several key blocks per (batch, head) -> dQ summed by fp32 atomics
  constexpr bool single_block = !MULTI;
  // 16-byte dQ stores need 8-element strides and a 16-byte aligned base
  const bool dq16 = ((a.dq_ss | a.dq_sb | a.dq_sh) & 7) == 0 && (((uintptr_t)a.dq) & 15) == 0;
  // this wave's share of the tile's dQ: queries 16 (w & 1) .. +16, d 32 (w >> 1) .. +32
  const int dq_q0 = 16 * (w & 1), dq_d0 = 32 * (w >> 1);
  // 16x16x32 fragment lane roles (transposing reads): g = lane >> 4 picks 8 keys, q4 / p4 a
  // row / 4-column group inside them
  const int fg = lane >> 4, fq = (lane & 15) >> 2, fp = lane & 3;

  // Q / dO / lse / delta tiles are register-prefetched two q-tiles ahead (issued before the
  // tile's MFMAs, written to LDS after its barrier into the buffer it has just released)
  const int prow = tid >> 3, pch = tid & 7;
  // delta = rowsum(dO * O) is computed here (no separate kernel): each thread prefetches
  // the O chunk matching its dO chunk; the 8 threads of a row reduce at staging time
  u16x8 pQ, pdO, pO;
  float pL = INFINITY;
#define BWD_PREFETCH(qb_)                                                                   \
  {                                                                                         \
    const int q_ = (qb_) + prow;                                                            \
    const bool ok_ = q_ < a.Sq;                                                             \
    pQ = ok_ ? *reinterpret_cast<const u16x8*>(qbase + (q_ * (int)a.q_ss + pch * 8)) : u16x8(0); \
    pdO = ok_ ? *reinterpret_cast<const u16x8*>(dobase + (q_ * (int)a.do_ss + pch * 8)) : u16x8(0); \
    pO = ok_ ? *reinterpret_cast<const u16x8*>(obase + (q_ * (int)a.o_ss + pch * 8)) : u16x8(0); \
    if (tid < 32) {                                                                         \
      const bool ok2_ = (qb_) + tid < a.Sq;                                                 \
      pL = ok2_ ? a.lse[(long)bh * a.Sq + (qb_) + tid] : INFINITY;                          \
    }                                                                                       \
  }
#define BWD_STAGE(buf_)                                                                     \
  {                                                                                         \
    *reinterpret_cast<u16x8*>(Qs + (buf_) * 4096 + swz(prow, pch)) = pQ;                    \
    *reinterpret_cast<u16x8*>(dOs + (buf_) * 4096 + swz(prow, pch)) = pdO;                  \
    if (tid < 32) lse_s[(buf_) * 32 + tid] = pL;                                            \
    float dd_ = 0.f;                                                                        \
    _Pragma("unroll") for (int j_ = 0; j_ < 8; ++j_) dd_ += bf2f(pdO[j_]) * bf2f(pO[j_]);  \
    dd_ += __shfl_xor(dd_, 1, 64);                                                          \
    dd_ += __shfl_xor(dd_, 2, 64);                                                          \
    dd_ += __shfl_xor(dd_, 4, 64);                                                          \
    if (pch == 0) delta_s[(buf_) * 32 + prow] = dd_;                                        \
  }
  // GL: Q / dO tile t (32 rows) into ring slot `slot_`: wave w DMAs rows 8 w + (lane >> 3) of
  // each (one 1 KB instruction per operand); rows past Sq read row Sq - 1 (finite; their
  // +inf lse zeroes every product they enter)
#define BWD_GLDS(qb_, slot_)                                                                \
  {                                                                                         \
    const unsigned q_ = (unsigned)min((qb_) + 8 * w + (lane >> 3), a.Sq - 1);               \
    const unsigned c_ = (unsigned)((lane & 7) ^ rev3((4 * w + (lane >> 4)) & 7));           \
    at_glds16s(qbase, (q_ * (unsigned)a.q_ss + c_ * 8u) * 2u, Qs + (slot_) * 4096 + w * 1024); \
    at_glds16s(dobase, (q_ * (unsigned)a.do_ss + c_ * 8u) * 2u, dOs + (slot_) * 4096 + w * 1024); \
  }
  if constexpr (GL) {
    BWD_GLDS(0, 0);
    if (nq > 1) BWD_GLDS(32, 1);
    // lse and delta of all rows: thread (row tid >> 1, half tid & 1) dots 32 d of dO and O
    {
      const int row = tid >> 1, hf = tid & 1;
      float dd = 0.f;
      if (row < a.Sq) {
        const bf16_t* dr = dobase + row * (int)a.do_ss + 32 * hf;
        const bf16_t* orow = obase + row * (int)a.o_ss + 32 * hf;
        u16x8 dv[4], ov[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          dv[j] = *reinterpret_cast<const u16x8*>(dr + 8 * j);
          ov[j] = *reinterpret_cast<const u16x8*>(orow + 8 * j);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int e = 0; e < 8; ++e) dd += bf2f(dv[j][e]) * bf2f(ov[j][e]);
      }
      dd += __shfl_xor(dd, 1, 64);
      if (hf == 0 && row < 128) delta_s[row] = dd;
      if (tid < 128) lse_s[tid] = tid < a.Sq ? a.lse[(long)bh * a.Sq + tid] : INFINITY;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  } else {
  BWD_PREFETCH(0);
  BWD_STAGE(0);
  if (nq > 1) {
    BWD_PREFETCH(32);
    BWD_STAGE(1);
  }
  }
  __syncthreads();

  int slot = 0;      // GL: ring slot of tile qt
  for (int qt = 0; qt < nq; ++qt) {
    const int qb = qt * 32;
    const int buf = qt & 1;
    if constexpr (GL) {
      // slot of tile qt + 2 == slot of tile qt - 1 (released at tile qt - 1's barrier)
      if (qt + 2 < nq) { const int s2 = slot == 0 ? 2 : slot - 1; BWD_GLDS(qb + 64, s2); }
    } else {
      if (qt + 2 < nq) BWD_PREFETCH(qb + 64);
    }
    const char* Qt = Qs + (GL ? slot : buf) * 4096;
    const char* dOt = dOs + (GL ? slot : buf) * 4096;
    const float* lse_t = lse_s + (GL ? qb : buf * 32);
    const float* delta_t = delta_s + (GL ? qb : buf * 32);
    char* dSt = dSs + buf * 8192;
    f32x16 S, dP;
#pragma unroll
    for (int i = 0; i < 16; ++i) { S[i] = 0.f; dP[i] = 0.f; }
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      S = mfma32(lds_b128(Qt + swz(r, 2 * s + hh)), lds_b128(Ks + swz(krow, 2 * s + hh)), S);
      dP = mfma32(lds_b128(dOt + swz(r, 2 * s + hh)), lds_b128(Vs + swz(krow, 2 * s + hh)), dP);
    }
    // dropout keep bits: the pair (even key, odd key) shares one hash; the two lanes of a
    // pair (lane ^ 1) each hash 8 of the 16 query rows and swap halves with one DPP move
    // packed into one register: bit i = keep decision of register i
    uint32_t keepbits = 0xFFFFu;
    if (DROP) {
      const uint32_t T0 = (uint32_t)(((uint64_t)bh * a.Sq + qb) * (uint64_t)(a.Sk >> 1));
      const uint32_t half_sk = (uint32_t)(a.Sk >> 1);
      const int hsel = r & 1;                // == key_l & 1 (k0, w*32 even)
      uint32_t mine = 0, theirs = 0;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int i = 8 * hsel + j;
        const int qrow = (i & 3) + 8 * (i >> 2) + 4 * hh;
        const uint32_t rr = hash_u32((T0 + (uint32_t)qrow * half_sk + (uint32_t)(key_l >> 1)) ^ a.hash_base);
        const uint32_t klo = (rr & 0xFFFFu) >= a.thr16, khi = (rr >> 16) >= a.thr16;
        mine |= (hsel ? khi : klo) << i;
        theirs |= (hsel ? klo : khi) << i;
      }
      keepbits = mine | (uint32_t)__builtin_amdgcn_update_dpp(0, (int)theirs, 0xB1, 0xF, 0xF, false);
    }
    // reg i <-> query row qrow(i) = (i&3) + 8(i>>2) + 4hh of this tile; column = key_l
    // REL: window index of (qrow(i), this lane's key) = krow + 32 nq - 1 - qb - qrow(i), in
    // [0, W); relp points at the pair of the tile's last row (8 g + j = 27)
    [[maybe_unused]] float* relp = bwd_rel_dyn + 2 * (krow + 32 * nq - 1 - qb - 4 * hh - 27);
    if constexpr (REL) {                  // the forward's order: fma, then the bias
#pragma unroll
      for (int i = 0; i < 16; ++i)
        S[i] = fmaf(S[i], a.scale_log2, kb2) + relp[2 * (27 - 8 * (i >> 2) - (i & 3))];
    }
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const f32x4 L4 = *reinterpret_cast<const f32x4*>(lse_t + 8 * g + 4 * hh);
      const f32x4 D4 = *reinterpret_cast<const f32x4*>(delta_t + 8 * g + 4 * hh);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int i = 4 * g + j;
        float x;
        if constexpr (REL) x = S[i];      // scaled and biased above
        else x = fmaf(S[i], a.scale_log2, kb2);
        if (CAUSAL && key_l > qb + 8 * g + 4 * hh + j) x = -INFINITY;
        const float p = __builtin_amdgcn_exp2f(x - L4[j]);
        float pd = p, dpv = dP[i];
        if (DROP) {
          const bool keep = (keepbits >> i) & 1u;
          pd = keep ? p * a.inv_keep : 0.f;
          dpv = keep ? dpv * a.inv_keep : 0.f;
        }
        S[i] = pd;                        // P (after dropout) for dV
        dP[i] = p * (dpv - D4[j]);        // dS (unscaled) for dK, dQ
      }
    }
    if constexpr (REL) {                  // d_rel: the fp32 dS, before its bf16 rounding
#pragma unroll
      for (int i = 0; i < 16; ++i)
        __hip_atomic_fetch_add(relp + 2 * (27 - 8 * (i >> 2) - (i & 3)) + 1, dP[i], __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    bf16x8_t pf[2], dsf[2];
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
      for (int j = 0; j < 8; ++j) { pf[s2][j] = (__bf16)S[8 * s2 + j]; dsf[s2][j] = (__bf16)dP[8 * s2 + j]; }
    // dV^T += dO^T . P ; dK^T += Q^T . dS   (A operands by transposed reads of the tiles)
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
      const int qr = 16 * s2 + 4 * hh + trow;
      const bf16x8_t ado0 = cat_tr(lds_tr(dOt + swz_e(qr, tcol)), lds_tr(dOt + swz_e(qr + 8, tcol)));
      const bf16x8_t ado1 = cat_tr(lds_tr(dOt + swz_e(qr, 32 + tcol)), lds_tr(dOt + swz_e(qr + 8, 32 + tcol)));
      const bf16x8_t aq0 = cat_tr(lds_tr(Qt + swz_e(qr, tcol)), lds_tr(Qt + swz_e(qr + 8, tcol)));
      const bf16x8_t aq1 = cat_tr(lds_tr(Qt + swz_e(qr, 32 + tcol)), lds_tr(Qt + swz_e(qr + 8, 32 + tcol)));
      dV0 = mfma32(ado0, pf[s2], dV0);
      dV1 = mfma32(ado1, pf[s2], dV1);
      dK0 = mfma32(aq0, dsf[s2], dK0);
      dK1 = mfma32(aq1, dsf[s2], dK1);
    }
    // dS^T -> LDS [128 keys][32 q] (64-byte rows, 8-byte chunks XOR dsw(key), below):
    // each lane owns one key row and 4 runs of 4 consecutive queries -> 4 ds_write_b64
    {
      const int key = w * 32 + r;
      char* rowp = dSt + key * 64;
      const int sw = dsw(key);
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int c = 2 * g + hh;     // 8-byte chunk = queries 8g + 4hh .. +3
        u16x4 v = {f2bf(dP[4 * g]), f2bf(dP[4 * g + 1]), f2bf(dP[4 * g + 2]), f2bf(dP[4 * g + 3])};
        *reinterpret_cast<u16x4*>(rowp + ((c ^ sw) << 3)) = v;
      }
    }
    if constexpr (GL) {
      // tile qt + 1's DMA (issued a tile and a half ago) must have landed before this barrier;
      // only tile qt + 2's two pieces may stay in flight
      if (qt + 2 < nq) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      slot = slot == 2 ? 0 : slot + 1;
    }
    __syncthreads();   // the ONLY barrier of the tile: dS^T complete; this tile's Q / dO / lse /
                       // delta buffers free; tile t+1's staged buffers visible
    // tile qt + 2's inputs into the buffers tile qt released at this barrier (staging after the
    // dQ stores instead measured slower: its vmcnt wait then covers those stores too)
    if constexpr (!GL) {
      if (qt + 2 < nq) BWD_STAGE(buf);
    }
    // dQ[q][d] = sum over the 128 keys of dS[q][key] K[key][d], 16x16x32 MFMAs issued as
    // (K^T fragment, dS fragment): the lane ends up with 4 consecutive d of one query.  Both
    // fragments (8 consecutive keys per lane) come from transposing reads of [key][.] images.
    // The key rows a lane reads are a permutation of the natural 8 fg + 4 j + fq (bits 2 and 3
    // swapped: 16 (fg >> 1) + 8 j + 4 (fg & 1) + fq), the same for both operands, so the sum
    // over keys is unchanged: each 32-lane half of a transposing read then covers 8
    // consecutive rows, whose swizzled chunks of K (swz) and of dS^T (dsw) fill all 64 banks
    // (with the natural order rows r and r + 8 of K shared banks: a 2-way conflict on every
    // K^T read).
    f32x4 dq0 = {0.f, 0.f, 0.f, 0.f}, dq1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const int kr0 = 32 * ks + 16 * (fg >> 1) + 4 * (fg & 1) + fq, kr1 = kr0 + 8;
      const int qc = (dq_q0 >> 2) + fp;        // 8-byte chunk of queries dq_q0 + 4 fp .. + 3
      const bf16x8_t sf = cat_tr(lds_tr(dSt + kr0 * 64 + ((qc ^ dsw(kr0)) << 3)),
                                 lds_tr(dSt + kr1 * 64 + ((qc ^ dsw(kr1)) << 3)));
      const bf16x8_t kf0 = cat_tr(lds_tr(Ks + swz_e(kr0, dq_d0 + 4 * fp)), lds_tr(Ks + swz_e(kr1, dq_d0 + 4 * fp)));
      const bf16x8_t kf1 = cat_tr(lds_tr(Ks + swz_e(kr0, dq_d0 + 16 + 4 * fp)),
                                  lds_tr(Ks + swz_e(kr1, dq_d0 + 16 + 4 * fp)));
      dq0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf0, sf, dq0, 0, 0, 0);
      dq1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf1, sf, dq1, 0, 0, 0);
    }
    // dq0[rr] = dQ[q = dq_q0 + (lane & 15)][d = dq_d0 + 4 (lane >> 4) + rr], dq1 the same +16
    const int q = qb + dq_q0 + (lane & 15);
    if (single_block && dq16 && qb + 32 <= a.Sq) {
      const u16x4 o0 = {f2bf(dq0[0] * a.scale), f2bf(dq0[1] * a.scale), f2bf(dq0[2] * a.scale), f2bf(dq0[3] * a.scale)};
      const u16x4 o1 = {f2bf(dq1[0] * a.scale), f2bf(dq1[1] * a.scale), f2bf(dq1[2] * a.scale), f2bf(dq1[3] * a.scale)};
      // permlane16 swap of the two d blocks: lane group g gets 8 consecutive d
      const uint2 xv = __builtin_bit_cast(uint2, o0), yv = __builtin_bit_cast(uint2, o1);
      const auto s0 = __builtin_amdgcn_permlane16_swap(xv.x, yv.x, false, false);
      const auto s1 = __builtin_amdgcn_permlane16_swap(xv.y, yv.y, false, false);
      const uint4 v = {s0[0], s1[0], s0[1], s1[1]};
      const int d = dq_d0 + 16 * (fg & 1) + 8 * (fg >> 1);
      *reinterpret_cast<uint4*>(dqbase + q * (int)a.dq_ss + d) = v;
    } else if (!single_block) {
      // Sk > 128: the wave's [16 q][32 d] fp32 share goes through LDS so that each atomic
      // wave-instruction adds two contiguous 128-byte row segments (the memory-side atomic
      // unit's full-rate shape) instead of 16 rows x 4 scattered dwords (~10x slower: the
      // backward took 883 us at B 32, S 512 before, 326 after).  Scratch: this wave's own key
      // rows of the OTHER dS^T buffer (tile qt - 1's, read by every wave's dQ before this
      // tile's barrier; rewritten only by this wave, at tile qt + 1); 128-byte rows, 16-byte
      // chunks XOR (q & 7).  Every lane takes part; rows past Sq only skip their atomics.
      char* xw = dSs + (buf ^ 1) * 8192 + w * 2048;
      const int xq = lane & 15;
      *reinterpret_cast<f32x4*>(xw + xq * 128 + ((fg ^ (xq & 7)) << 4)) = dq0;
      *reinterpret_cast<f32x4*>(xw + xq * 128 + (((4 + fg) ^ (xq & 7)) << 4)) = dq1;
      __builtin_amdgcn_wave_barrier();
      const int xd = lane & 31;
      float* accp = a.dq_acc + ((long)bh * a.Sq + qb + dq_q0) * 64 + dq_d0 + xd;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int qr = 2 * i + (lane >> 5);
        const float val = *reinterpret_cast<const float*>(xw + qr * 128 + (((xd >> 2) ^ (qr & 7)) << 4) + ((xd & 3) << 2)) * a.scale;
        if (qb + dq_q0 + qr < a.Sq) atomicAdd(accp + qr * 64, val);
      }
      __builtin_amdgcn_wave_barrier();
    } else if (q < a.Sq) {
#pragma unroll
      for (int t2 = 0; t2 < 2; ++t2)
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
          const int d = dq_d0 + 16 * t2 + 4 * fg + rr;
          dqbase[q * (int)a.dq_ss + d] = f2bf((t2 ? dq1[rr] : dq0[rr]) * a.scale);
        }
    }
  }
#undef BWD_PREFETCH
#undef BWD_STAGE
#undef BWD_GLDS
  {
    const long kl = kvalid ? key_l : 0;
    store_row64(a.dk + b * a.dk_sb + h * a.dk_sh + kl * a.dk_ss, dK0, dK1, a.scale, hh, kvalid);
    store_row64(a.dv + b * a.dv_sb + h * a.dv_sh + kl * a.dv_ss, dV0, dV1, 1.f, hh, kvalid);
  }
  if constexpr (REL) {
    // the whole window, zeros included, so the reduce kernel needs no memset
    __syncthreads();
    const int W = 32 * nq + 127;
    float* wsp = a.drel_ws + (((long)b * gridDim.x + blockIdx.x) * a.H + h) * W;
    for (int i = tid; i < W; i += 256) wsp[i] = bwd_rel_dyn[2 * i + 1];
  }
