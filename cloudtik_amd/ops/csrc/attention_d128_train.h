// Head-dim-128 training kernels (T5-3B / T5-11B fine-tuning: d_kv = 128), included by
// attention.hip inside namespace ct after the d64 kernels (never on its own): the forward with
// dropout and the backward.  A p = 0 training forward is attn_fwd_d128_kernel with an lse buffer.

// attn_fwd_d128_kernel with attention-prob dropout: the same structure, LDS image and semantics
// (its header comment states them), under a name of its own so that attn_fwd_d128_kernel<CAUSAL,
// REL> keeps the name tests and profiles match on.  The dropout stream is the d64 kernels': one
// hash_u32 per (even key, odd key) pair indexed by (bh, query, key >> 1), so it drops exactly the
// elements ops.reference.attn_dropout_keep names; dropped probabilities are zeroed in place and
// 1 / (1 - p) is folded into the final 1 / l, l being the pre-dropout row sum, so lse is that
// of the undropped softmax.
template <bool CAUSAL, bool REL>
__global__ __launch_bounds__(256, 2) void attn_fwd_d128_drop_kernel(AttnFwdArgs a) {
  __shared__ __attribute__((aligned(16))) char smem[2 * 4 * 64 * 128 + 2 * 64 * 4];
  float* kbias_lds = reinterpret_cast<float*>(smem + 65536);
  extern __shared__ float relb_dyn[];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 31, hh = lane >> 5;
  const int bh = blockIdx.y, b = bh / a.H, h = bh % a.H;
  const int qi = blockIdx.x * 128 + w * 32 + r;
  const bool qvalid = qi < a.Sq;
  const bool wactive = (int)blockIdx.x * 128 + w * 32 < a.Sq;   // wave-uniform
  const float LOG2E = 1.4426950408889634f;
  if (REL)
    for (int i = tid; i < a.relb_len; i += 256) relb_dyn[i] = a.relb[h * a.relb_sh + i] * LOG2E;

  const bf16_t* qp = a.q + b * a.q_sb + h * a.q_sh + (long)qi * a.q_ss;
  bf16x8_t qf[8];
#pragma unroll
  for (int s = 0; s < 8; ++s) qf[s] = gload_frag(qp + 16 * s + 8 * hh, qvalid);

  const bf16_t* kp = a.k + b * a.k_sb + h * a.k_sh;
  const bf16_t* vp = a.v + b * a.v_sb + h * a.v_sh;
  const float* kbp = a.kbias ? a.kbias + b * a.kb_sb : nullptr;
  float stB = 0.f;
  // element pair index base of this lane's query row (dropout stream); Sk even
  const uint32_t rb2 = (uint32_t)((((uint64_t)bh * a.Sq + qi) * (uint64_t)a.Sk) >> 1);

  f32x16 O[4];
#pragma unroll
  for (int ob = 0; ob < 4; ++ob)
#pragma unroll
    for (int i = 0; i < 16; ++i) O[ob][i] = 0.f;
  float m = -INFINITY, l = 0.f;
  const int nt = (a.Sk + 63) / 64;
  const bool resident = nt == 2;

#define FWD128_GLDS(kt_, buf_)                                                                 \
  _Pragma("unroll") for (int hf_ = 0; hf_ < 2; ++hf_)                                          \
  _Pragma("unroll") for (int i_ = 0; i_ < 2; ++i_) {                                           \
    const int row_ = 16 * w + 8 * i_ + (lane >> 3);                                            \
    const unsigned key_ = (unsigned)min((kt_) * 64 + row_, a.Sk - 1);                          \
    const unsigned c_ = (unsigned)((lane & 7) ^ rev3((4 * i_ + (lane >> 4)) & 7));             \
    char* dst_ = smem + (buf_) * 32768 + hf_ * 8192 + (16 * w + 8 * i_) * 128;                 \
    at_glds16s_pad(kp, (key_ * (unsigned)a.k_ss + 64u * hf_ + c_ * 8u) * 2u, dst_);                \
    at_glds16s_pad(vp, (key_ * (unsigned)a.v_ss + 64u * hf_ + c_ * 8u) * 2u, dst_ + 16384);        \
  }
  FWD128_GLDS(0, 0);
  if (resident) {
    FWD128_GLDS(1, 1);
    if (tid < 128) stB = tid < a.Sk ? (kbp ? kbp[tid] * LOG2E : 0.f) : -INFINITY;
  } else if (tid < 64) {
    stB = tid < a.Sk ? (kbp ? kbp[tid] * LOG2E : 0.f) : -INFINITY;
  }
  if (tid < (resident ? 128 : 64)) kbias_lds[tid] = stB;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  const int trow = (lane >> 2) & 3;
  const int tcol = ((lane >> 4) & 1) * 16 + (lane & 3) * 4;

  for (int kt = 0; kt < nt; ++kt) {
    const int buf = kt & 1;
    if (!resident && kt + 1 < nt) {
      FWD128_GLDS(kt + 1, buf ^ 1);
      if (tid < 64) {
        const int kk = (kt + 1) * 64 + tid;
        stB = kk < a.Sk ? (kbp ? kbp[kk] * LOG2E : 0.f) : -INFINITY;
      }
    }
    if (wactive) {
      const char* Kb = smem + buf * 32768;
      const char* Vb = Kb + 16384;
      f32x16 S0, S1;
#pragma unroll
      for (int i = 0; i < 16; ++i) { S0[i] = 0.f; S1[i] = 0.f; }
#pragma unroll
      for (int s = 0; s < 8; ++s) {
        const char* Kh = Kb + (s >> 2) * 8192;
        S0 = mfma32(lds_b128(Kh + swz(r, 2 * (s & 3) + hh)), qf[s], S0);
        S1 = mfma32(lds_b128(Kh + swz(32 + r, 2 * (s & 3) + hh)), qf[s], S1);
      }
      const float* kbt = kbias_lds + buf * 64 + 4 * hh;
      float mx = -INFINITY;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const f32x4 b0 = *reinterpret_cast<const f32x4*>(kbt + 8 * g);
        const f32x4 b1 = *reinterpret_cast<const f32x4*>(kbt + 32 + 8 * g);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int i = 4 * g + j;
          float x0 = fmaf(S0[i], a.scale_log2, b0[j]);
          float x1 = fmaf(S1[i], a.scale_log2, b1[j]);
          if (REL) {
            const int ri = kt * 64 + 8 * g + 4 * hh + j - qi + a.rel_base;
            x0 += relb_dyn[min(max(ri, 0), a.relb_len - 1)];
            x1 += relb_dyn[min(max(ri + 32, 0), a.relb_len - 1)];
          }
          if (CAUSAL) {
            const int key0 = kt * 64 + 8 * g + 4 * hh + j;
            if (key0 > qi) x0 = -INFINITY;
            if (key0 + 32 > qi) x1 = -INFINITY;
          }
          S0[i] = x0; S1[i] = x1;
          mx = fmaxf(mx, fmaxf(x0, x1));
        }
      }
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      const float m_new = fmaxf(m, mx);
      const float msub = m_new == -INFINITY ? 0.f : m_new;
      const float alpha = __builtin_amdgcn_exp2f(m - msub);
      m = m_new;
      float ps = 0.f;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        S0[i] = __builtin_amdgcn_exp2f(S0[i] - msub);
        S1[i] = __builtin_amdgcn_exp2f(S1[i] - msub);
        ps += S0[i] + S1[i];
      }
      l = l * alpha + ps;
#pragma unroll
      for (int ob = 0; ob < 4; ++ob)
#pragma unroll
        for (int i = 0; i < 16; ++i) O[ob][i] *= alpha;
      // dropout, element for element the d64 forward's (see attn_fwd_d64_kernel)
      {
        const uint32_t pbase = rb2 + (uint32_t)(kt * 32 + 2 * hh);
        const uint32_t thi = a.thr16 << 16;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
#pragma unroll
          for (int i = 0; i < 16; i += 2) {  // (i&3) in {0,2}: an even key and its odd partner
            const uint32_t pair = pbase + (uint32_t)(t * 16 + 4 * (i >> 2) + ((i & 3) >> 1));
            const uint32_t rr = hash_u32(pair ^ a.hash_base);
            const bool k0 = (rr << 16) >= thi, k1 = rr >= thi;
            if (t == 0) { S0[i] = k0 ? S0[i] : 0.f; S0[i + 1] = k1 ? S0[i + 1] : 0.f; }
            else { S1[i] = k0 ? S1[i] : 0.f; S1[i + 1] = k1 ? S1[i + 1] : 0.f; }
          }
        }
      }
      bf16x8_t pf[2][2];
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          pf[0][s2][j] = (__bf16)S0[8 * s2 + j];
          pf[1][s2][j] = (__bf16)S1[8 * s2 + j];
        }
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
          const int kb = t * 32 + 16 * s2 + 4 * hh + trow;
#pragma unroll
          for (int ob = 0; ob < 4; ++ob) {
            const char* Vh = Vb + (ob >> 1) * 8192;
            const int col = 32 * (ob & 1) + tcol;
            const bf16x8_t av = cat_tr(lds_tr(Vh + swz_e(kb, col)), lds_tr(Vh + swz_e(kb + 8, col)));
            O[ob] = mfma32(av, pf[t][s2], O[ob]);
          }
        }
    }
    if (!resident) {
      if (kt + 1 < nt && tid < 64) kbias_lds[(buf ^ 1) * 64 + tid] = stB;
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
    }
  }
#undef FWD128_GLDS
  if (!wactive) return;
  l += __shfl_xor(l, 32, 64);
  const float inv = l > 0.f ? a.inv_keep / l : 0.f;
  bf16_t* op = a.o + b * a.o_sb + h * a.o_sh + (long)(qvalid ? qi : 0) * a.o_ss;
  store_row64(op, O[0], O[1], inv, hh, qvalid);
  store_row64(op + 64, O[2], O[3], inv, hh, qvalid);
  if (qvalid) {
    if (hh == 0 && a.lse) a.lse[(long)bh * a.Sq + qi] = l > 0.f ? m + log2f(l) : INFINITY;
  }
}

// Head-dim-128 backward: the register-staged d64 backward (attention_bwd_d64_body.h; design notes
// in front of attn_bwd_d64_kernel) widened to 128 columns, with the same semantics -- key on the
// lane, P and dS rounded to bf16 before their MFMAs, delta = rowsum(dO . O) from the bf16 O
// computed here, d_rel summed in fp32 from the unrounded dS into the workgroup's LDS window and
// stored whole into drel_ws (REL), dQ summed by fp32 atomics into dq_acc when Sk > 128 (MULTI).
//   * every 128-wide tile is two 64-column halves, each the d64 swz() image (as in the d128
//     forward), so all row reads and transposing reads keep the d64 bank pattern;
//   * S and dP take 8 k-steps; dK^T and dV^T are four f32x16 blocks each (d 0..31, .. 96..127);
//   * dQ: a wave owns 16 queries x 64 d of the q-tile (d half w >> 1, four 16x16 blocks); MULTI
//     stages that fp32 share through its 2 KB of the other dS^T buffer in two 32-column passes.
// LDS: Q tiles 2 x 8K | dO tiles 2 x 8K | K block 32K | V block 32K | dS^T 2 x 8K | lse, delta
// = kBwd128Static bytes, so ONE workgroup per CU (160 KiB), and the unified 512-entry register
// file at one wave per SIMD holds the eight accumulators plus S and dP.  The REL windows are the
// d64 kernel's (W = 32 nq + 127, same index arithmetic: 128 keys per workgroup, 32-row
// q-tiles), 8 W bytes of dynamic LDS.  Loads of rows past Sq / keys past Sk are predicated off
// (zeros), their +inf lse / -inf key bias make every product they enter exactly zero, and
// their stores are skipped.
constexpr int kBwd128Static = 2 * 16384 + 2 * 32768 + 16384 + 512;

template <bool DROP, bool CAUSAL, bool MULTI, bool REL>
__global__ __launch_bounds__(256, 1) void attn_bwd_d128_kernel(AttnBwdArgs a) {
  __shared__ __attribute__((aligned(16))) char smem[kBwd128Static];
  char* Qs = smem;                 // [buf][half][32 rows][128 B]
  char* dOs = smem + 16384;
  char* Ks = smem + 32768;         // [half][128 rows][128 B]
  char* Vs = Ks + 32768;
  char* dSs = Vs + 32768;          // [buf][128 keys][64 B]
  float* lse_s = reinterpret_cast<float*>(dSs + 16384);       // [2][32]
  float* delta_s = lse_s + 64;                                // [2][32]
  // REL: [2 i] the log2-scaled bias of window offset i, [2 i + 1] the fp32 d_rel sum
  extern __shared__ float bwd_rel_dyn[];

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 31, hh = lane >> 5;
  const int bh = blockIdx.y, b = bh / a.H, h = bh % a.H;
  const int k0 = blockIdx.x * 128;
  const int key_l = k0 + w * 32 + r;  // this lane's key (MFMA column)
  const bool kvalid = key_l < a.Sk;
  const float LOG2E = 1.4426950408889634f;

  const bf16_t* kp = a.k + b * a.k_sb + h * a.k_sh;
  const bf16_t* vp = a.v + b * a.v_sb + h * a.v_sh;
  // K and V blocks (128 keys x 256 B): 16 consecutive threads fetch one row
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int c = tid + 256 * i;
    const int row = c >> 4, hf = (c >> 3) & 1, ch = c & 7;
    const int key = k0 + row;
    const bool ok = key < a.Sk;
    const u16x8 kv = ok ? *reinterpret_cast<const u16x8*>(kp + (long)key * a.k_ss + 64 * hf + ch * 8) : u16x8(0);
    const u16x8 vv = ok ? *reinterpret_cast<const u16x8*>(vp + (long)key * a.v_ss + 64 * hf + ch * 8) : u16x8(0);
    *reinterpret_cast<u16x8*>(Ks + hf * 16384 + swz(row, ch)) = kv;
    *reinterpret_cast<u16x8*>(Vs + hf * 16384 + swz(row, ch)) = vv;
  }
  const int krow = w * 32 + r;   // this lane's key row inside the block
  float kb2 = 0.f;
  if (a.kbias && kvalid) kb2 = a.kbias[b * a.kb_sb + key_l] * LOG2E;
  if (!kvalid) kb2 = -INFINITY;

  f32x16 dV[4], dK[4];
#pragma unroll
  for (int ob = 0; ob < 4; ++ob)
#pragma unroll
    for (int i = 0; i < 16; ++i) { dV[ob][i] = 0.f; dK[ob][i] = 0.f; }

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
  // 16-byte dQ stores need 8-element strides and a 16-byte aligned base
  const bool dq16 = ((a.dq_ss | a.dq_sb | a.dq_sh) & 7) == 0 && (((uintptr_t)a.dq) & 15) == 0;
  // this wave's share of the tile's dQ: queries 16 (w & 1) .. +16, d 64 (w >> 1) .. +64
  const int dq_q0 = 16 * (w & 1), dq_d0 = 64 * (w >> 1);
  const char* Kdq = Ks + (w >> 1) * 16384;
  // 16x16x32 fragment lane roles (transposing reads), as in the d64 body
  const int fg = lane >> 4, fq = (lane & 15) >> 2, fp = lane & 3;

  // Q / dO / O / lse tiles are register-prefetched two q-tiles ahead: thread (prow, pch) takes
  // 16-byte chunk pch of both halves of row prow; the 8 threads of a row reduce delta
  const int prow = tid >> 3, pch = tid & 7;
  u16x8 pQ[2], pdO[2], pO[2];
  float pL = INFINITY;
#define BWD128_PREFETCH(qb_)                                                                \
  {                                                                                         \
    const int q_ = (qb_) + prow;                                                            \
    const bool ok_ = q_ < a.Sq;                                                             \
    _Pragma("unroll") for (int hf_ = 0; hf_ < 2; ++hf_) {                                   \
      const int e_ = 64 * hf_ + pch * 8;                                                    \
      pQ[hf_] = ok_ ? *reinterpret_cast<const u16x8*>(qbase + (q_ * (int)a.q_ss + e_)) : u16x8(0);   \
      pdO[hf_] = ok_ ? *reinterpret_cast<const u16x8*>(dobase + (q_ * (int)a.do_ss + e_)) : u16x8(0); \
      pO[hf_] = ok_ ? *reinterpret_cast<const u16x8*>(obase + (q_ * (int)a.o_ss + e_)) : u16x8(0);   \
    }                                                                                       \
    if (tid < 32) {                                                                         \
      const bool ok2_ = (qb_) + tid < a.Sq;                                                 \
      pL = ok2_ ? a.lse[(long)bh * a.Sq + (qb_) + tid] : INFINITY;                          \
    }                                                                                       \
  }
#define BWD128_STAGE(buf_)                                                                  \
  {                                                                                         \
    float dd_ = 0.f;                                                                        \
    _Pragma("unroll") for (int hf_ = 0; hf_ < 2; ++hf_) {                                   \
      *reinterpret_cast<u16x8*>(Qs + (buf_) * 8192 + hf_ * 4096 + swz(prow, pch)) = pQ[hf_];   \
      *reinterpret_cast<u16x8*>(dOs + (buf_) * 8192 + hf_ * 4096 + swz(prow, pch)) = pdO[hf_]; \
      _Pragma("unroll") for (int j_ = 0; j_ < 8; ++j_) dd_ += bf2f(pdO[hf_][j_]) * bf2f(pO[hf_][j_]); \
    }                                                                                       \
    if (tid < 32) lse_s[(buf_) * 32 + tid] = pL;                                            \
    dd_ += __shfl_xor(dd_, 1, 64);                                                          \
    dd_ += __shfl_xor(dd_, 2, 64);                                                          \
    dd_ += __shfl_xor(dd_, 4, 64);                                                          \
    if (pch == 0) delta_s[(buf_) * 32 + prow] = dd_;                                        \
  }
  BWD128_PREFETCH(0);
  BWD128_STAGE(0);
  if (nq > 1) {
    BWD128_PREFETCH(32);
    BWD128_STAGE(1);
  }
  __syncthreads();

  for (int qt = 0; qt < nq; ++qt) {
    const int qb = qt * 32;
    const int buf = qt & 1;
    if (qt + 2 < nq) BWD128_PREFETCH(qb + 64);
    const char* Qt = Qs + buf * 8192;
    const char* dOt = dOs + buf * 8192;
    const float* lse_t = lse_s + buf * 32;
    const float* delta_t = delta_s + buf * 32;
    char* dSt = dSs + buf * 8192;
    f32x16 S, dP;
#pragma unroll
    for (int i = 0; i < 16; ++i) { S[i] = 0.f; dP[i] = 0.f; }
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      const int hf = s >> 2, c = 2 * (s & 3) + hh;
      S = mfma32(lds_b128(Qt + hf * 4096 + swz(r, c)), lds_b128(Ks + hf * 16384 + swz(krow, c)), S);
      dP = mfma32(lds_b128(dOt + hf * 4096 + swz(r, c)), lds_b128(Vs + hf * 16384 + swz(krow, c)), dP);
    }
    // dropout keep bits, the d64 body's: the pair (even key, odd key) shares one hash; the two
    // lanes of a pair each hash 8 of the 16 query rows and swap halves with one DPP move
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
#pragma unroll
      for (int ob = 0; ob < 4; ++ob) {
        const int ho = (ob >> 1) * 4096, col = 32 * (ob & 1) + tcol;
        const bf16x8_t ado = cat_tr(lds_tr(dOt + ho + swz_e(qr, col)), lds_tr(dOt + ho + swz_e(qr + 8, col)));
        const bf16x8_t aq = cat_tr(lds_tr(Qt + ho + swz_e(qr, col)), lds_tr(Qt + ho + swz_e(qr + 8, col)));
        dV[ob] = mfma32(ado, pf[s2], dV[ob]);
        dK[ob] = mfma32(aq, dsf[s2], dK[ob]);
      }
    }
    // dS^T -> LDS [128 keys][32 q] (64-byte rows, 8-byte chunks XOR dsw(key))
    {
      char* rowp = dSt + krow * 64;
      const int sw = dsw(krow);
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int c = 2 * g + hh;     // 8-byte chunk = queries 8g + 4hh .. +3
        u16x4 v = {f2bf(dP[4 * g]), f2bf(dP[4 * g + 1]), f2bf(dP[4 * g + 2]), f2bf(dP[4 * g + 3])};
        *reinterpret_cast<u16x4*>(rowp + ((c ^ sw) << 3)) = v;
      }
    }
    __syncthreads();   // the ONLY barrier of the tile: dS^T complete; this tile's Q / dO / lse /
                       // delta buffers free; tile t+1's staged buffers visible
    if (qt + 2 < nq) BWD128_STAGE(buf);
    // dQ[q][d] = sum over the 128 keys of dS[q][key] K[key][d]: the d64 body's 16x16x32 scheme
    // (same permuted key rows for both operands) over four 16-column blocks of this wave's d half
    f32x4 dq[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) dq[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const int kr0 = 32 * ks + 16 * (fg >> 1) + 4 * (fg & 1) + fq, kr1 = kr0 + 8;
      const int qc = (dq_q0 >> 2) + fp;        // 8-byte chunk of queries dq_q0 + 4 fp .. + 3
      const bf16x8_t sf = cat_tr(lds_tr(dSt + kr0 * 64 + ((qc ^ dsw(kr0)) << 3)),
                                 lds_tr(dSt + kr1 * 64 + ((qc ^ dsw(kr1)) << 3)));
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bf16x8_t kf = cat_tr(lds_tr(Kdq + swz_e(kr0, 16 * j + 4 * fp)), lds_tr(Kdq + swz_e(kr1, 16 * j + 4 * fp)));
        dq[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, sf, dq[j], 0, 0, 0);
      }
    }
    // dq[j][rr] = dQ[q = dq_q0 + (lane & 15)][d = dq_d0 + 16 j + 4 (lane >> 4) + rr]
    const int q = qb + dq_q0 + (lane & 15);
    if (!MULTI && dq16 && qb + 32 <= a.Sq) {
#pragma unroll
      for (int pr = 0; pr < 2; ++pr) {
        const f32x4 &x = dq[2 * pr], &y = dq[2 * pr + 1];
        const u16x4 o0 = {f2bf(x[0] * a.scale), f2bf(x[1] * a.scale), f2bf(x[2] * a.scale), f2bf(x[3] * a.scale)};
        const u16x4 o1 = {f2bf(y[0] * a.scale), f2bf(y[1] * a.scale), f2bf(y[2] * a.scale), f2bf(y[3] * a.scale)};
        // permlane16 swap of the two d blocks: lane group g gets 8 consecutive d
        const uint2 xv = __builtin_bit_cast(uint2, o0), yv = __builtin_bit_cast(uint2, o1);
        const auto s0 = __builtin_amdgcn_permlane16_swap(xv.x, yv.x, false, false);
        const auto s1 = __builtin_amdgcn_permlane16_swap(xv.y, yv.y, false, false);
        const uint4 v = {s0[0], s1[0], s0[1], s1[1]};
        const int d = dq_d0 + 32 * pr + 16 * (fg & 1) + 8 * (fg >> 1);
        *reinterpret_cast<uint4*>(dqbase + q * (int)a.dq_ss + d) = v;
      }
    } else if (MULTI) {
      // Sk > 128: the wave's fp32 share goes through LDS so that each atomic wave-instruction
      // adds two contiguous 128-byte row segments (see the d64 body).  Scratch: this wave's own
      // key rows of the OTHER dS^T buffer, 2 KB = [16 q][32 d] fp32, so the 64 d go in two passes
      // of 32; 128-byte rows, 16-byte chunks XOR (q & 7).  Every lane takes part; rows past Sq
      // only skip their atomics.
      char* xw = dSs + (buf ^ 1) * 8192 + w * 2048;
      const int xq = lane & 15, xd = lane & 31;
#pragma unroll
      for (int pr = 0; pr < 2; ++pr) {
        *reinterpret_cast<f32x4*>(xw + xq * 128 + ((fg ^ (xq & 7)) << 4)) = dq[2 * pr];
        *reinterpret_cast<f32x4*>(xw + xq * 128 + (((4 + fg) ^ (xq & 7)) << 4)) = dq[2 * pr + 1];
        __builtin_amdgcn_wave_barrier();
        float* accp = a.dq_acc + ((long)bh * a.Sq + qb + dq_q0) * 128 + dq_d0 + 32 * pr + xd;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const int qr = 2 * i + (lane >> 5);
          const float val = *reinterpret_cast<const float*>(xw + qr * 128 + (((xd >> 2) ^ (qr & 7)) << 4) + ((xd & 3) << 2)) * a.scale;
          if (qb + dq_q0 + qr < a.Sq) atomicAdd(accp + qr * 128, val);
        }
        __builtin_amdgcn_wave_barrier();
      }
    } else if (q < a.Sq) {
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int rr = 0; rr < 4; ++rr)
          dqbase[q * (int)a.dq_ss + dq_d0 + 16 * j + 4 * fg + rr] = f2bf(dq[j][rr] * a.scale);
    }
  }
#undef BWD128_PREFETCH
#undef BWD128_STAGE
  {
    const long kl = kvalid ? key_l : 0;
    bf16_t* dkp = a.dk + b * a.dk_sb + h * a.dk_sh + kl * a.dk_ss;
    bf16_t* dvp = a.dv + b * a.dv_sb + h * a.dv_sh + kl * a.dv_ss;
    store_row64(dkp, dK[0], dK[1], a.scale, hh, kvalid);
    store_row64(dkp + 64, dK[2], dK[3], a.scale, hh, kvalid);
    store_row64(dvp, dV[0], dV[1], 1.f, hh, kvalid);
    store_row64(dvp + 64, dV[2], dV[3], 1.f, hh, kvalid);
  }
  if constexpr (REL) {
    // the whole window, zeros included, so the reduce kernel needs no memset
    __syncthreads();
    const int W = 32 * nq + 127;
    float* wsp = a.drel_ws + (((long)b * gridDim.x + blockIdx.x) * a.H + h) * W;
    for (int i = tid; i < W; i += 256) wsp[i] = bwd_rel_dyn[2 * i + 1];
  }
}
