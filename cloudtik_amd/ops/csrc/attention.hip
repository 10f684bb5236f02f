// Fused multi-head attention on CDNA4 MFMA, bf16 I/O: forward + backward at head_dim 64 and at
// head_dim 128 (T5-3B / T5-11B, d_kv = 128: attn_fwd_d128_kernel, whose header comment states its
// LDS plan, for inference and the p = 0 training forward; attn_fwd_d128_drop_kernel and
// attn_bwd_d128_kernel in attention_d128_train.h for training).
//
// Hot op of the reference's BERT-large pretraining: HF BertSelfAttention, 16 heads x 64,
// S = 128 (phase-1 shards) / 512, padding mask + attention-prob dropout 0.1
// (run_pretrain_mlperf.py:449-471).  There is no attention kernel in the reference tree --
// it reaches this through PyTorch/IPEX -- so this is designed for MI355X from scratch:
//
// Forward (flash-style, never materialises S x S):
//   * workgroup = 4 waves = 128 queries of one (batch, head); each wave owns 32 queries.
//   * S^T = K . Q^T with v_mfma_f32_32x32x16_bf16: the query sits on the MFMA lane and the
//     keys in the 16 accumulator registers, so a query's softmax row is lane-local except
//     for one xor-32 shuffle (no LDS round trip for the softmax).
//   * the P^T accumulator feeds the next MFMA directly as its B operand
//     (O^T += V^T . P^T, cdna_hip_programming.md §3 "accumulator as next operand"); V^T
//     fragments come from ds_read_b64_tr_b16 transposed LDS reads of the row-major V tile.
//   * K/V tiles of 64 keys, double-buffered in LDS, register-staged (global loads for tile
//     t+1 issued before the MFMAs of tile t, LDS write after: T14).
//   * every 128-byte LDS row is XOR-swizzled at 16-byte granularity with
//     rev3((row >> 1) & 7): conflict-free for both the ds_read_b128 row reads and the
//     ds_read_b64_tr_b16 column reads (see swz()).
//   * online softmax in the exp2 domain; stores O and the per-row log2-sum-exp.
// Backward (FlashAttention-2 structure, "key on the lane"):
//   * workgroup = 4 waves = 128 keys; each wave keeps K, V fragments of its 32 keys in
//     VGPRs and accumulates dK^T, dV^T in registers over all query tiles.
//   * S = Q.K^T and dP = dO.V^T are computed with the key on the lane, so P and dS are
//     already the B operands of dV^T += dO^T.P and dK^T += Q^T.dS (Q^T, dO^T by
//     transposed LDS reads); only dS crosses LDS (once) for dQ = dS.K.
//   * dQ: each wave owns 16 queries x 32 d of the q-tile and sums over all 128 keys itself
//     (16x16x32 MFMAs on transposed reads of dS^T and K: no cross-wave reduction); the
//     q-tile inputs and dS^T are double-buffered, so each q-tile takes ONE barrier.  Stored
//     directly (bf16, 16-byte stores after a permlane16 swap) when one workgroup covers all
//     keys (S <= 128, the BERT phase-1 case), otherwise accumulated with fp32 atomics and
//     converted by a tiny kernel.
//   * attention-prob dropout regenerated from a counter hash (nothing stored).
//   * the kernel body is attention_bwd_d64_body.h, included by attn_bwd_d64_kernel and by
//     attn_bwd_d64_rel_kernel (T5 training: relative-position bias in the score, its gradient
//     out through LDS float adds and attn_drel_reduce_kernel; notes in front of the kernels).
// Head dim 128 (attn_fwd_d128_kernel<CAUSAL, REL>): the forward above with 8 k-steps for S^T and
// four O^T blocks; a K/V tile is two 64-column halves in the d64 LDS image; K/V by
// global_load_lds into a two-deep ring; the relative-bias stage is dynamic LDS sized to the
// vector, so two workgroups share a CU.  Its training kernels (the forward with dropout, and the
// backward: the d64 backward widened to 128 columns, one workgroup per CU) are in
// attention_d128_train.h.
#include "common.h"
#include "attention_api.h"
#include <cstdlib>
#include <type_traits>

namespace ct {

typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((address_space(3))) s16x4 lds_s16x4;

__device__ __forceinline__ int rev3(int x) { return ((x & 1) << 2) | (x & 2) | ((x >> 2) & 1); }
// byte offset of 16-byte chunk c of `row` inside a [rows][64 x bf16] LDS tile
__device__ __forceinline__ int swz(int row, int c) { return row * 128 + ((c ^ rev3((row >> 1) & 7)) << 4); }
__device__ __forceinline__ int swz_e(int row, int col) { return swz(row, col >> 3) + ((col & 7) << 1); }
// 8-byte chunk XOR of key row `key` in the backward's dS^T image ([keys][32 q], 64-byte rows).
// Writes (ds_write_b64, 16-lane groups over 32 banks): 16 consecutive keys hit distinct
// (parity, chunk) slots.  Transposing reads (32-lane halves over 64 banks, 8 consecutive rows
// 8a .. 8a + 7, 4 chunks each): rows r and r + 4 share a 64-byte window and their chunk sets
// differ in bit 2.
__device__ __forceinline__ int dsw(int key) { return ((key >> 1) & 7) ^ (key & 4); }

__device__ __forceinline__ bf16x8_t lds_b128(const char* p) {
  return __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const u16x8*>(p));
}
__device__ __forceinline__ s16x4 lds_tr(const char* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(p));
}
__device__ __forceinline__ bf16x8_t cat_tr(s16x4 lo, s16x4 hi) {
  typedef __attribute__((ext_vector_type(8))) short s16x8;
  s16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(bf16x8_t, v);
}
__device__ __forceinline__ bf16x8_t gload_frag(const bf16_t* p, bool valid) {
  u16x8 v = valid ? *reinterpret_cast<const u16x8*>(p) : u16x8(0);
  return __builtin_bit_cast(bf16x8_t, v);
}
__device__ __forceinline__ f32x16 mfma32(bf16x8_t a, bf16x8_t b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}
typedef __attribute__((address_space(3))) void at_lds_void;
// global_load_lds_dwordx4: lane l's 16 bytes at sbase + voff land at LDS wave_base + 16 l (one
// 1 KB wave instruction, no staging registers).  sbase must be wave-uniform.  The compiler does
// not count these in vmcnt: callers wait with s_waitcnt vmcnt(0) before the barrier.
__device__ __forceinline__ void at_glds16s(const void* sbase, unsigned voff, const char* lds_wave_base) {
  const unsigned la = __builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)(at_lds_void*)lds_wave_base);
  const uint64_t sb = (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)sbase) |
                      ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((unsigned)((uintptr_t)sbase >> 32)) << 32);
  asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" ::"v"(voff), "s"(sb), "s"(la)
               : "memory", "m0");
}
// Store a 64-wide row held as two 32x32 MFMA accumulators in the "row on the lane" layout:
// lane (r, hh) holds columns d = 8 g + 4 hh .. + 3 of row r (A0: d < 32, A1: d + 32).  A
// v_permlane32_swap of the (g, g + 1) pair between the lane halves leaves each lane 8
// consecutive columns (hh = 0: block g, hh = 1: block g + 1), so the row goes out as 16-byte
// stores, 4 per lane instead of 8 of 8 bytes (the store tail of these short kernels is
// issue-bound).  Every lane must take part (the swap); `valid` only gates the stores.
__device__ __forceinline__ void store_row64(bf16_t* p, const f32x16& A0, const f32x16& A1, float mul, int hh,
                                            bool valid) {
  u16x8 ov[4];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int gp = 0; gp < 2; ++gp) {
      const f32x16& A = t ? A1 : A0;
      const int g0 = 2 * gp, g1 = g0 + 1;
      const u16x4 x = {f2bf(A[4 * g0] * mul), f2bf(A[4 * g0 + 1] * mul), f2bf(A[4 * g0 + 2] * mul),
                       f2bf(A[4 * g0 + 3] * mul)};
      const u16x4 y = {f2bf(A[4 * g1] * mul), f2bf(A[4 * g1 + 1] * mul), f2bf(A[4 * g1 + 2] * mul),
                       f2bf(A[4 * g1 + 3] * mul)};
      const uint2 xv = __builtin_bit_cast(uint2, x), yv = __builtin_bit_cast(uint2, y);
      const auto s0 = __builtin_amdgcn_permlane32_swap(xv.x, yv.x, false, false);
      const auto s1 = __builtin_amdgcn_permlane32_swap(xv.y, yv.y, false, false);
      // s*[0] = the new x (hh = 1 lanes: the partner's y), s*[1] = the new y
      const uint4 v = {s0[0], s1[0], s0[1], s1[1]};
      ov[2 * t + gp] = __builtin_bit_cast(u16x8, v);
    }
  if (!valid) return;
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int gp = 0; gp < 2; ++gp) *reinterpret_cast<u16x8*>(p + 32 * t + 8 * (2 * gp + hh)) = ov[2 * t + gp];
}

__device__ __forceinline__ uint32_t hash_u32(uint32_t x) {
  x ^= x >> 16; x *= 0x7FEB352Du; x ^= x >> 15; x *= 0x846CA68Bu; x ^= x >> 16;
  return x;
}
// 16-bit uniform pair for element pair `pair` (elements 2*pair, 2*pair+1)
__device__ __forceinline__ uint32_t drop_pair(uint32_t base, uint64_t pair) {
  return hash_u32((uint32_t)pair ^ base);
}

struct AttnFwdArgs {
  const bf16_t* q; const bf16_t* k; const bf16_t* v; bf16_t* o;
  long q_sb, q_ss, q_sh, k_sb, k_ss, k_sh, v_sb, v_ss, v_sh, o_sb, o_ss, o_sh;
  const float* kbias; long kb_sb;  // additive per-key bias [B, Sk] (natural-log units)
  float* lse;                      // [B*H, Sq] log2-domain log-sum-exp
  int B, H, Sq, Sk;
  float scale_log2;                // softmax scale * log2(e)
  uint32_t thr16; float inv_keep; uint32_t hash_base; int causal;
  // relative-position bias (T5): score(q, k) += relb[h][k - q + rel_base] (natural-log units)
  const float* relb; long relb_sh; int relb_len; int rel_base;
};

constexpr int kRelBiasMax = 4096;   // LDS floats for one head's relative-offset bias vector

// WPE: waves per SIMD the register budget must allow (256 threads = 1 wave per SIMD per
// workgroup).  The compiler's default budget (236 VGPR + 32 AGPR) allowed ONE resident
// workgroup per CU, so a workgroup's Q/K/V loads never overlapped another's MFMAs; at 2 the
// kernel fits in ~170 VGPRs without spills.
// GL: K/V tiles go global -> LDS by global_load_lds (at_glds16s) instead of through the
// stK/stV (+ k1/v1) staging registers: wave w DMAs rows 16 w .. 16 w + 15 of the K and the V
// tile (two 1 KB wave instructions each).  Lane l lands at physical chunk l & 7 of row
// 16 w + 8 i + (l >> 3), so it fetches logical chunk (l & 7) ^ rev3(((row >> 1) & 7)) =
// (l & 7) ^ rev3((4 i + (l >> 4)) & 7) -- the same swizzled image the register path writes.
// Keys past Sk read key Sk - 1 (finite data; their -inf key bias zeroes them), so no load is
// out of bounds and no zero fill is needed.
template <bool DROP, bool CAUSAL, bool REL = false, int WPE = 2, bool GL = false>
__global__ __launch_bounds__(256, WPE) void attn_fwd_d64_kernel(AttnFwdArgs a) {
  // [buf][K,V][64 rows][128 B] then [buf][64] fp32 log2-domain key bias (-inf past Sk)
  __shared__ __attribute__((aligned(16))) char smem[2 * 2 * 64 * 128 + 2 * 64 * 4];
  float* kbias_lds = reinterpret_cast<float*>(smem + 32768);
  // one head's relative-position bias vector, log2-scaled (REL variant only; the first
  // K/V tile's barrier below publishes it)
  __shared__ float relb_lds[REL ? kRelBiasMax : 1];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 31, hh = lane >> 5;
  const int bh = blockIdx.y, b = bh / a.H, h = bh % a.H;
  const int qi = blockIdx.x * 128 + w * 32 + r;
  const bool qvalid = qi < a.Sq;
  const float LOG2E = 1.4426950408889634f;
  if (REL)
    for (int i = tid; i < a.relb_len; i += 256) relb_lds[i] = a.relb[h * a.relb_sh + i] * LOG2E;

  const bf16_t* qp = a.q + b * a.q_sb + h * a.q_sh + (long)qi * a.q_ss;
  bf16x8_t qf[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) qf[s] = gload_frag(qp + 16 * s + 8 * hh, qvalid);

  const bf16_t* kp = a.k + b * a.k_sb + h * a.k_sh;
  const bf16_t* vp = a.v + b * a.v_sb + h * a.v_sh;
  const float* kbp = a.kbias ? a.kbias + b * a.kb_sb : nullptr;
  const int srow = tid >> 3, sch = tid & 7;
  u16x8 stK[2], stV[2];
  float stB = 0.f;
  // element pair index base of this lane's query row (dropout stream); Sk even
  const uint32_t rb2 = (uint32_t)((((uint64_t)bh * a.Sq + qi) * (uint64_t)a.Sk) >> 1);

  f32x16 O0, O1;
#pragma unroll
  for (int i = 0; i < 16; ++i) { O0[i] = 0.f; O1[i] = 0.f; }
  float m = -INFINITY, l = 0.f;
  const int nt = (a.Sk + 63) / 64;

#define FWD_GLOAD(kt_)                                                               \
  _Pragma("unroll") for (int i_ = 0; i_ < 2; ++i_) {                                 \
    const int key_ = (kt_) * 64 + srow + 32 * i_;                                    \
    const bool ok_ = key_ < a.Sk;                                                    \
    stK[i_] = ok_ ? *reinterpret_cast<const u16x8*>(kp + (key_ * (int)a.k_ss + sch * 8)) : u16x8(0); \
    stV[i_] = ok_ ? *reinterpret_cast<const u16x8*>(vp + (key_ * (int)a.v_ss + sch * 8)) : u16x8(0); \
  }                                                                                  \
  if (tid < 64) {                                                                    \
    const int kk_ = (kt_) * 64 + tid;                                                \
    stB = kk_ < a.Sk ? (kbp ? kbp[kk_] * LOG2E : 0.f) : -INFINITY;                   \
  }
#define FWD_SWRITE(buf_)                                                             \
  _Pragma("unroll") for (int i_ = 0; i_ < 2; ++i_) {                                 \
    char* kb_ = smem + (buf_) * 16384;                                               \
    *reinterpret_cast<u16x8*>(kb_ + swz(srow + 32 * i_, sch)) = stK[i_];             \
    *reinterpret_cast<u16x8*>(kb_ + 8192 + swz(srow + 32 * i_, sch)) = stV[i_];      \
  }                                                                                  \
  if (tid < 64) kbias_lds[(buf_) * 64 + tid] = stB;

  // Sk <= 128 (BERT phase 1): both K/V tiles are loaded up front (a second staging set; the
  // accumulators are not live yet, so it costs no occupancy) and sit in the two LDS buffers
  // before the first MFMA -- one memory latency per workgroup instead of two in series, and
  // no barrier inside the loop
  const bool resident = nt == 2;
#define FWD_GLDS(kt_, buf_)                                                                    \
  _Pragma("unroll") for (int i_ = 0; i_ < 2; ++i_) {                                           \
    const int row_ = 16 * w + 8 * i_ + (lane >> 3);                                            \
    const unsigned key_ = (unsigned)min((kt_) * 64 + row_, a.Sk - 1);                          \
    const unsigned c_ = (unsigned)((lane & 7) ^ rev3((4 * i_ + (lane >> 4)) & 7));             \
    char* dst_ = smem + (buf_) * 16384 + (16 * w + 8 * i_) * 128;                              \
    at_glds16s(kp, (key_ * (unsigned)a.k_ss + c_ * 8u) * 2u, dst_);                            \
    at_glds16s(vp, (key_ * (unsigned)a.v_ss + c_ * 8u) * 2u, dst_ + 8192);                     \
  }
  if constexpr (GL) {
    FWD_GLDS(0, 0);
    if (resident) {
      FWD_GLDS(1, 1);
      if (tid < 128) stB = tid < a.Sk ? (kbp ? kbp[tid] * LOG2E : 0.f) : -INFINITY;
    } else if (tid < 64) {
      stB = tid < a.Sk ? (kbp ? kbp[tid] * LOG2E : 0.f) : -INFINITY;
    }
    if (tid < (resident ? 128 : 64)) kbias_lds[tid] = stB;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  } else {
  FWD_GLOAD(0);
  if (resident) {
    u16x8 k1[2], v1[2];
    float b1 = 0.f;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int key = 64 + srow + 32 * i;
      const bool ok = key < a.Sk;
      k1[i] = ok ? *reinterpret_cast<const u16x8*>(kp + (key * (int)a.k_ss + sch * 8)) : u16x8(0);
      v1[i] = ok ? *reinterpret_cast<const u16x8*>(vp + (key * (int)a.v_ss + sch * 8)) : u16x8(0);
    }
    if (tid < 64) {
      const int kk = 64 + tid;
      b1 = kk < a.Sk ? (kbp ? kbp[kk] * LOG2E : 0.f) : -INFINITY;
    }
    FWD_SWRITE(0);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      *reinterpret_cast<u16x8*>(smem + 16384 + swz(srow + 32 * i, sch)) = k1[i];
      *reinterpret_cast<u16x8*>(smem + 16384 + 8192 + swz(srow + 32 * i, sch)) = v1[i];
    }
    if (tid < 64) kbias_lds[64 + tid] = b1;
  } else {
    FWD_SWRITE(0);
  }
  }
  __syncthreads();

  const int trow = (lane >> 2) & 3;
  const int tcol = ((lane >> 4) & 1) * 16 + (lane & 3) * 4;

  for (int kt = 0; kt < nt; ++kt) {
    const int buf = kt & 1;
    if (!resident && kt + 1 < nt) {
      if constexpr (GL) {
        // buf ^ 1 was last read in tile kt - 1, which ended with a barrier
        FWD_GLDS(kt + 1, buf ^ 1);
        if (tid < 64) {
          const int kk = (kt + 1) * 64 + tid;
          stB = kk < a.Sk ? (kbp ? kbp[kk] * LOG2E : 0.f) : -INFINITY;
        }
      } else {
        FWD_GLOAD(kt + 1);
      }
    }
    const char* Kb = smem + buf * 16384;
    const char* Vb = Kb + 8192;
    f32x16 S0, S1;
#pragma unroll
    for (int i = 0; i < 16; ++i) { S0[i] = 0.f; S1[i] = 0.f; }
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      S0 = mfma32(lds_b128(Kb + swz(r, 2 * s + hh)), qf[s], S0);
      S1 = mfma32(lds_b128(Kb + swz(32 + r, 2 * s + hh)), qf[s], S1);
    }
    // reg i <-> key kt*64 + t*32 + 8(i>>2) + 4hh + (i&3): 4 consecutive keys per group,
    // so the bias comes in as float4 LDS reads; -inf bias masks keys past Sk
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
          x0 += relb_lds[min(max(ri, 0), a.relb_len - 1)];
          x1 += relb_lds[min(max(ri + 32, 0), a.relb_len - 1)];
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
    for (int i = 0; i < 16; ++i) { O0[i] *= alpha; O1[i] *= alpha; }
    // dropout: one 32-bit hash per (even, odd) key pair, one 16-bit uniform each.  Dropped
    // probabilities are zeroed in place (compare + select); the 1/(1-p) rescale is folded
    // into the final 1/l normalisation (l is the pre-dropout row sum), so no per-element
    // multiply.  (r >> 16) >= t16  <=>  r >= t16 << 16; (r & 0xFFFF) >= t16  <=>
    // (r << 16) >= t16 << 16: one compare per element.
    if (DROP) {
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
    // P^T registers -> bf16 B fragments (k-step s2 of tile t = registers 8*s2 .. 8*s2+7)
    bf16x8_t pf[2][2];
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        pf[0][s2][j] = (__bf16)S0[8 * s2 + j];
        pf[1][s2][j] = (__bf16)S1[8 * s2 + j];
      }
    // O^T[d][q] += V^T[d][key] . P^T[key][q]; V^T fragments by transposed LDS reads
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        const int kb = t * 32 + 16 * s2 + 4 * hh + trow;
        const bf16x8_t a0 = cat_tr(lds_tr(Vb + swz_e(kb, tcol)), lds_tr(Vb + swz_e(kb + 8, tcol)));
        const bf16x8_t a1 = cat_tr(lds_tr(Vb + swz_e(kb, 32 + tcol)), lds_tr(Vb + swz_e(kb + 8, 32 + tcol)));
        O0 = mfma32(a0, pf[t][s2], O0);
        O1 = mfma32(a1, pf[t][s2], O1);
      }
    if (!resident) {
      if constexpr (GL) {
        if (kt + 1 < nt && tid < 64) kbias_lds[(buf ^ 1) * 64 + tid] = stB;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      } else {
        if (kt + 1 < nt) { FWD_SWRITE(buf ^ 1); }
      }
      __syncthreads();
    }
  }
#undef FWD_GLOAD
#undef FWD_SWRITE
#undef FWD_GLDS
  l += __shfl_xor(l, 32, 64);
  const float inv = l > 0.f ? (DROP ? a.inv_keep : 1.f) / l : 0.f;
  bf16_t* op = a.o + b * a.o_sb + h * a.o_sh + (long)(qvalid ? qi : 0) * a.o_ss;
  store_row64(op, O0, O1, inv, hh, qvalid);
  if (qvalid) {
    if (hh == 0 && a.lse) a.lse[(long)bh * a.Sq + qi] = l > 0.f ? m + log2f(l) : INFINITY;
  }
}


// Pipelined persistent forward (no relative bias): a workgroup walks work items blockIdx.x,
// + gridDim.x, ... (item = q-block + nqb * (batch * H + head)) and runs ONE flat loop over the
// K/V tiles of all of them.  The K/V (+ key bias) of flat tile f + 2 are loaded into one of two
// register staging sets at step f and written to LDS at the end of step f + 1, so every load
// has two tile computations to land (the one-set kernel above gives it one).  Measured SLOWER
// than the one-item kernel (75.5 vs 65.9 us on BERT-large shapes): the hardware dispatcher
// already overlaps one workgroup's loads with another's MFMAs, and the persistent walk only
// adds loop-carried state (199 VGPRs, 2 waves/SIMD).  Kept as an opt-in (CLOUDTIK_AMD_ATTN_FWD_PIPE=1)
// for long sequences, where items have many tiles.  The next item's Q fragments
// are loaded at the first tile of the current item.  The loop is unrolled by two so the
// staging set is a compile-time choice (a runtime index would put the sets in scratch).
template <bool DROP, bool CAUSAL>
__global__ __launch_bounds__(256, 2) void attn_fwd_pipe_kernel(AttnFwdArgs a) {
  __shared__ __attribute__((aligned(16))) char smem[2 * 2 * 64 * 128 + 2 * 64 * 4];
  float* kbias_lds = reinterpret_cast<float*>(smem + 32768);
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 31, hh = lane >> 5;
  const int nqb = (a.Sq + 127) / 128;
  const int nitems = nqb * a.B * a.H;
  const int G = gridDim.x;
  if ((int)blockIdx.x >= nitems) return;
  const float LOG2E = 1.4426950408889634f;
  const int srow = tid >> 3, sch = tid & 7;
  const int nt = (a.Sk + 63) / 64;
  const int my_items = (nitems - (int)blockIdx.x + G - 1) / G;
  const int nflat = my_items * nt;
  const int trow = (lane >> 2) & 3;
  const int tcol = ((lane >> 4) & 1) * 16 + (lane & 3) * 4;

  u16x8 k0s[2], v0s[2], k1s[2], v1s[2];
  float b0s = 0.f, b1s = 0.f;
  auto gload = [&](int f, u16x8 (&K)[2], u16x8 (&V)[2], float& Bv) {
    const int it = (int)blockIdx.x + (f / nt) * G, kt = f % nt;
    const int bh = it / nqb, b = bh / a.H, h = bh % a.H;
    const bf16_t* kp = a.k + b * a.k_sb + h * a.k_sh;
    const bf16_t* vp = a.v + b * a.v_sb + h * a.v_sh;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int key = kt * 64 + srow + 32 * i;
      const bool ok = key < a.Sk;
      K[i] = ok ? *reinterpret_cast<const u16x8*>(kp + (key * (int)a.k_ss + sch * 8)) : u16x8(0);
      V[i] = ok ? *reinterpret_cast<const u16x8*>(vp + (key * (int)a.v_ss + sch * 8)) : u16x8(0);
    }
    if (tid < 64) {
      const int kk = kt * 64 + tid;
      Bv = kk < a.Sk ? (a.kbias ? a.kbias[b * a.kb_sb + kk] * LOG2E : 0.f) : -INFINITY;
    }
  };
  auto swrite = [&](int buf, const u16x8 (&K)[2], const u16x8 (&V)[2], float Bv) {
    char* kb = smem + buf * 16384;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      *reinterpret_cast<u16x8*>(kb + swz(srow + 32 * i, sch)) = K[i];
      *reinterpret_cast<u16x8*>(kb + 8192 + swz(srow + 32 * i, sch)) = V[i];
    }
    if (tid < 64) kbias_lds[buf * 64 + tid] = Bv;
  };
  auto qload = [&](int it, bf16x8_t (&Q)[4]) {
    const int bh = it / nqb, b = bh / a.H, h = bh % a.H;
    const int qi = (it % nqb) * 128 + w * 32 + r;
    const bf16_t* qp = a.q + b * a.q_sb + h * a.q_sh + (long)qi * a.q_ss;
#pragma unroll
    for (int s = 0; s < 4; ++s) Q[s] = gload_frag(qp + 16 * s + 8 * hh, qi < a.Sq);
  };

  bf16x8_t qf[4], qn[4];
  qload(blockIdx.x, qf);
  gload(0, k0s, v0s, b0s);
  if (nflat > 1) gload(1, k1s, v1s, b1s);
  swrite(0, k0s, v0s, b0s);
  __syncthreads();

  f32x16 O0, O1;
  float m = -INFINITY, l = 0.f;

  // one flat step: compute tile f from LDS buffer P (f % 2 == P), K/V of tile f + 2 into
  // staging set P, tile f + 1 (staging set 1 - P) into buffer 1 - P at the end
  auto step = [&](int f, u16x8 (&Kp)[2], u16x8 (&Vp)[2], float& Bp, const u16x8 (&Kq)[2],
                  const u16x8 (&Vq)[2], const float& Bq, int P) {
    if (f + 2 < nflat) gload(f + 2, Kp, Vp, Bp);
    const int fi = f / nt, kt = f - fi * nt;
    const int item = (int)blockIdx.x + fi * G;
    const int bh = item / nqb;
    const int qi = (item % nqb) * 128 + w * 32 + r;
    if (kt == 0) {
#pragma unroll
      for (int i = 0; i < 16; ++i) { O0[i] = 0.f; O1[i] = 0.f; }
      m = -INFINITY;
      l = 0.f;
      if (fi + 1 < my_items) qload(item + G, qn);
    }
    const char* Kb = smem + P * 16384;
    const char* Vb = Kb + 8192;
    f32x16 S0, S1;
#pragma unroll
    for (int i = 0; i < 16; ++i) { S0[i] = 0.f; S1[i] = 0.f; }
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      S0 = mfma32(lds_b128(Kb + swz(r, 2 * s + hh)), qf[s], S0);
      S1 = mfma32(lds_b128(Kb + swz(32 + r, 2 * s + hh)), qf[s], S1);
    }
    const float* kbt = kbias_lds + P * 64 + 4 * hh;
    float mx = -INFINITY;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const f32x4 bb0 = *reinterpret_cast<const f32x4*>(kbt + 8 * g);
      const f32x4 bb1 = *reinterpret_cast<const f32x4*>(kbt + 32 + 8 * g);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int i = 4 * g + j;
        float x0 = fmaf(S0[i], a.scale_log2, bb0[j]);
        float x1 = fmaf(S1[i], a.scale_log2, bb1[j]);
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
    for (int i = 0; i < 16; ++i) { O0[i] *= alpha; O1[i] *= alpha; }
    if (DROP) {   // the dropout stream of the one-item kernel above, element for element
      const uint32_t rb2 = (uint32_t)((((uint64_t)bh * a.Sq + qi) * (uint64_t)a.Sk) >> 1);
      const uint32_t pbase = rb2 + (uint32_t)(kt * 32 + 2 * hh);
      const uint32_t thi = a.thr16 << 16;
#pragma unroll
      for (int t = 0; t < 2; ++t) {
#pragma unroll
        for (int i = 0; i < 16; i += 2) {
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
        const bf16x8_t a0 = cat_tr(lds_tr(Vb + swz_e(kb, tcol)), lds_tr(Vb + swz_e(kb + 8, tcol)));
        const bf16x8_t a1 = cat_tr(lds_tr(Vb + swz_e(kb, 32 + tcol)), lds_tr(Vb + swz_e(kb + 8, 32 + tcol)));
        O0 = mfma32(a0, pf[t][s2], O0);
        O1 = mfma32(a1, pf[t][s2], O1);
      }
    if (kt == nt - 1) {
      float lt = l + __shfl_xor(l, 32, 64);
      const float inv = lt > 0.f ? (DROP ? a.inv_keep : 1.f) / lt : 0.f;
      if (qi < a.Sq) {
        const int b = bh / a.H, h = bh % a.H;
        bf16_t* op = a.o + b * a.o_sb + h * a.o_sh + (long)qi * a.o_ss;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int d = 8 * g + 4 * hh;
          u16x4 v0 = {f2bf(O0[4 * g] * inv), f2bf(O0[4 * g + 1] * inv), f2bf(O0[4 * g + 2] * inv), f2bf(O0[4 * g + 3] * inv)};
          u16x4 v1 = {f2bf(O1[4 * g] * inv), f2bf(O1[4 * g + 1] * inv), f2bf(O1[4 * g + 2] * inv), f2bf(O1[4 * g + 3] * inv)};
          *reinterpret_cast<u16x4*>(op + d) = v0;
          *reinterpret_cast<u16x4*>(op + 32 + d) = v1;
        }
        if (hh == 0 && a.lse) a.lse[(long)bh * a.Sq + qi] = lt > 0.f ? m + log2f(lt) : INFINITY;
      }
#pragma unroll
      for (int s = 0; s < 4; ++s) qf[s] = qn[s];
    }
    if (f + 1 < nflat) swrite(1 - P, Kq, Vq, Bq);
    __syncthreads();
  };
  for (int f = 0; f < nflat; f += 2) {
    step(f, k0s, v0s, b0s, k1s, v1s, b1s, 0);
    if (f + 1 < nflat) step(f + 1, k1s, v1s, b1s, k0s, v0s, b0s, 1);
  }
}

// at_glds16s for the d128 kernel.  Its REL instantiations keep the K/V base pointers in VGPRs, so
// the readfirstlanes below are real VALU writes of the SGPR pair the load reads as its scalar
// base, and the compiler does not pad that hazard around inline asm (5 wait states; what
// scripts/isa_audit.py checks): s_mov + s_nop 3 are the 5.
__device__ __forceinline__ void at_glds16s_pad(const void* sbase, unsigned voff, const char* lds_wave_base) {
  const unsigned la = __builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)(at_lds_void*)lds_wave_base);
  const uint64_t sb = (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)sbase) |
                      ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((unsigned)((uintptr_t)sbase >> 32)) << 32);
  asm volatile("s_mov_b32 m0, %2\n\ts_nop 3\n\tglobal_load_lds_dwordx4 %0, %1" ::"v"(voff), "s"(sb), "s"(la)
               : "memory", "m0");
}

// Head-dim-128 inference forward (T5-3B / T5-11B: d_kv = 128): forward only, no dropout.
// Semantics of attn_fwd_d64_kernel<false, CAUSAL, REL>: fp32 key bias, optional relative-bias
// vector, top-left causal mask, exp2-domain online softmax, o bf16 + lse fp32 (log2 domain),
// a fully masked row gives o = 0 and lse = +inf.  Same query-on-the-lane structure:
// 4 waves x 32 queries, S^T = K . Q^T in 8 k-steps (qf[8]), the P^T accumulators feed
// O^T += V^T . P^T, O^T is four f32x16 blocks (d 0..31, 32..63, 64..95, 96..127).
//
// LDS image: a 64-key x 128-d tile is two 64-column halves, each the d64 kernel's
// [64 rows][128 B] image under the same swz(): k-steps 0..3 / O blocks 0, 1 read half 0,
// k-steps 4..7 / O blocks 2, 3 read half 1, so the ds_read_b128 row reads and the
// ds_read_tr16_b64 column reads keep the d64 kernel's conflict-free pattern.
//
// LDS plan: 64-key tiles, K and V both double-buffered (2 x (16 KB + 16 KB) = 64 KB) plus
// 512 B of key bias, and the relative-bias stage sized to relb_len at launch (dynamic LDS,
// 4 relb_len bytes) instead of a fixed kRelBiasMax x 4 = 16 KB.  Why: with the fixed stage a
// workgroup takes 80.5 KB and ONE fits in a CU's 160 KB, so its tile loads overlap nobody's
// MFMAs; T5's vectors are Sq + Sk - 1 floats (a few hundred to ~1 K), and at
// relb_len <= 3968 a workgroup stays under 80 KB and TWO fit, which is also all the
// 2-waves-per-SIMD register budget allows.  The ring keeps the d64 kernel's one barrier per
// tile (a single-buffered V needs a second one) and its 64-key softmax step (32-key tiles
// double the number of rescales and barriers).  Cost: one workgroup per CU for the non-T5
// case 3968 < relb_len <= 4096, and never the three per CU the d64 kernel reaches.
//
// K/V tiles go global -> LDS by global_load_lds (at_glds16s_pad), wave w rows 16 w .. 16 w + 15
// of both halves of K and V (eight 1 KB wave instructions a tile), no staging registers.
// Keys past Sk re-read key Sk - 1 and are killed by their -inf key bias: no load is out of
// bounds.  Both tiles of an Sk <= 128 call are loaded up front (no barrier in the loop).
// A wave none of whose 32 queries exists (the decode shape: Sq = 1) still loads its share of
// every tile and meets every barrier, but skips the MFMAs and the softmax.
template <bool CAUSAL, bool REL>
__global__ __launch_bounds__(256, 2) void attn_fwd_d128_kernel(AttnFwdArgs a) {
  // [buf][K half 0, K half 1, V half 0, V half 1][64 rows][128 B], then [buf][64] fp32
  // log2-domain key bias (-inf past Sk)
  __shared__ __attribute__((aligned(16))) char smem[2 * 4 * 64 * 128 + 2 * 64 * 4];
  float* kbias_lds = reinterpret_cast<float*>(smem + 65536);
  // one head's relative-position bias vector, log2-scaled: relb_len floats of dynamic LDS
  // (REL only; the first K/V tile's barrier below publishes it)
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

  f32x16 O[4];
#pragma unroll
  for (int ob = 0; ob < 4; ++ob)
#pragma unroll
    for (int i = 0; i < 16; ++i) O[ob][i] = 0.f;
  float m = -INFINITY, l = 0.f;
  const int nt = (a.Sk + 63) / 64;
  const bool resident = nt == 2;

  // lane l lands at physical chunk l & 7 of row 16 w + 8 i + (l >> 3) of the half, so it
  // fetches logical chunk (l & 7) ^ rev3((4 i + (l >> 4)) & 7): the swz() image
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
      // buf ^ 1 was last read in tile kt - 1, which ended with a barrier
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
      // reg i <-> key kt*64 + t*32 + 8(i>>2) + 4hh + (i&3), as in the d64 kernel
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
      // P^T registers -> bf16 B fragments (k-step s2 of tile t = registers 8*s2 .. 8*s2+7)
      bf16x8_t pf[2][2];
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          pf[0][s2][j] = (__bf16)S0[8 * s2 + j];
          pf[1][s2][j] = (__bf16)S1[8 * s2 + j];
        }
      // O^T[d][q] += V^T[d][key] . P^T[key][q]; V^T fragments by transposed LDS reads
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
  const float inv = l > 0.f ? 1.f / l : 0.f;
  bf16_t* op = a.o + b * a.o_sb + h * a.o_sh + (long)(qvalid ? qi : 0) * a.o_ss;
  store_row64(op, O[0], O[1], inv, hh, qvalid);
  store_row64(op + 64, O[2], O[3], inv, hh, qvalid);
  if (qvalid) {
    if (hh == 0 && a.lse) a.lse[(long)bh * a.Sq + qi] = l > 0.f ? m + log2f(l) : INFINITY;
  }
}

struct AttnBwdArgs {
  const bf16_t* q; const bf16_t* k; const bf16_t* v; const bf16_t* dO; const bf16_t* o;
  long o_sb, o_ss, o_sh;
  bf16_t* dq; bf16_t* dk; bf16_t* dv; float* dq_acc;
  long q_sb, q_ss, q_sh, k_sb, k_ss, k_sh, v_sb, v_ss, v_sh, do_sb, do_ss, do_sh;
  long dq_sb, dq_ss, dq_sh, dk_sb, dk_ss, dk_sh, dv_sb, dv_ss, dv_sh;
  const float* kbias; long kb_sb;
  const float* lse; const float* delta;
  int B, H, Sq, Sk;
  float scale_log2, scale;
  uint32_t thr16; float inv_keep; uint32_t hash_base; int causal;
  // the relative-bias backward only (REL): score(q, k) += relb[h][k - q + rel_base] (natural-log
  // units); drel_ws [B, nkb, H, W] fp32 takes each workgroup's window of the bias gradient
  const float* relb; long relb_sh; int relb_len; int rel_base;
  float* drel_ws;
};

// GL (single key block and Sq <= 128 only): every LDS tile arrives by global_load_lds -- K, V
// and the first two Q / dO tiles in the prologue, tile t + 2's Q / dO at the top of tile t into
// a THREE-deep ring (the slot tile t - 1 released at its barrier), waited for by a counted
// vmcnt just before tile t + 1's barrier: one and a half tiles of compute cover each load
// (the register-staged form gives half a tile and stalls on it: 47 % of wave cycles parked in
// s_waitcnt / barrier).  lse and delta = rowsum(dO * O) are computed for all (<= 128) rows
// once in the prologue instead of per tile, so the loop issues no register-destined loads.
//
// REL (relative-position bias, T5 training): the score gets rel[h][key - query + rel_base] and the
// kernel also produces the gradient of that vector.  A workgroup owns keys k0 .. k0 + 127 and
// walks query rows 0 .. 32 nq - 1, so the offsets it touches form ONE window of
// W = 32 nq + 127 entries starting at win0 = k0 - (32 nq - 1) + rel_base; window index
// (key - k0) - query + 32 nq - 1 lies in [0, W) for every (query, key) of the padded tiles, rows
// past Sq and keys past Sk included, so no LDS address can leave the window.  Two windows of
// dynamic LDS (sized at launch): the bias, log2-scaled, zero where win0 + i is outside [0, L)
// (only padded rows / keys land there, and their P is 0), and the fp32 sum of dS per offset.
// dS is taken in fp32 before its bf16 rounding and added with LDS float adds (in register i
// consecutive lanes hold consecutive keys: consecutive addresses per 32-lane half).  The window
// is then stored whole, with plain stores, into a [B, nkb, H, W] workspace that
// attn_drel_reduce_kernel sums in a fixed order.  The LDS adds of one workgroup land in an
// order the hardware picks, so d_rel is NOT bitwise reproducible from run to run (the sum
// across workgroups is).  REL has no GL form: Sq <= 128 runs the register-staged kernel.
// The REL kernels have a name of their own, attn_bwd_d64_rel_kernel<DROP, CAUSAL, MULTI>, so
// that attn_bwd_d64_kernel<DROP, CAUSAL, MULTI, GL> keeps the name tests and profiles match on;
// both include the one body (attention_bwd_d64_body.h) with REL as a compile-time constant.
template <bool DROP, bool CAUSAL, bool MULTI, bool GL = false>
__global__ __launch_bounds__(256, 2) void attn_bwd_d64_kernel(AttnBwdArgs a) {
  constexpr bool REL = false;
#include "attention_bwd_d64_body.h"
}

template <bool DROP, bool CAUSAL, bool MULTI>
__global__ __launch_bounds__(256, 2) void attn_bwd_d64_rel_kernel(AttnBwdArgs a) {
  constexpr bool GL = false, REL = true;
#include "attention_bwd_d64_body.h"
}

#include "attention_d128_train.h"

// d_rel[h][i] (fp32, strided) = the sum over (batch, key block), in that fixed order, of the
// workspace windows that hold offset i; every entry is written, an offset in no window as 0.
__global__ void attn_drel_reduce_kernel(const float* __restrict__ ws, float* __restrict__ drel, long d_sh, long d_si,
                                        int B, int nkb, int H, int W, int L, int win00) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= H * L) return;
  const int h = t / L, i = t - h * L;
  float acc = 0.f;
  for (int b = 0; b < B; ++b)
    for (int kb = 0; kb < nkb; ++kb) {
      const int li = i - (win00 + 128 * kb);       // window of key block kb starts at win00 + 128 kb
      if (li >= 0 && li < W) acc += ws[(((long)b * nkb + kb) * H + h) * W + li];
    }
  drel[h * d_sh + i * d_si] = acc;
}

// dq (bf16, strided) = dq_acc (fp32 [B*H, Sq, D]), D = 1 << dshift
__global__ void attn_dq_convert_kernel(const float* __restrict__ acc, bf16_t* __restrict__ dq,
                                       long sb, long ss, long sh, int B, int H, int Sq, int dshift) {
  const long t = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (t >= ((long)B * H * Sq) << dshift) return;
  const int d = t & ((1 << dshift) - 1);
  const long row = t >> dshift;
  const int q = row % Sq;
  const int bh = row / Sq;
  const int b = bh / H, h = bh % H;
  dq[b * sb + h * sh + (long)q * ss + d] = f2bf(acc[t]);
}

}  // namespace ct

using namespace ct;

static_assert(kRelBiasMax == kCtAttnRelBiasMax, "the kernels' LDS stage is the interface's limit");

static uint32_t host_hash_u32(uint32_t x) {
  x ^= x >> 16; x *= 0x7FEB352Du; x ^= x >> 15; x *= 0x846CA68Bu; x ^= x >> 16;
  return x;
}
static void drop_params(float p, uint64_t seed, uint64_t offset, uint32_t* thr16, float* inv_keep,
                        uint32_t* base) {
  long t = (long)(p * 65536.0f + 0.5f);
  *thr16 = (uint32_t)(t > 65535 ? 65535 : t);
  *inv_keep = p > 0.f ? 1.f / (1.f - p) : 1.f;
  const uint32_t s_lo = (uint32_t)seed, s_hi = (uint32_t)(seed >> 32), o_lo = (uint32_t)offset;
  *base = host_hash_u32(s_lo ^ (s_hi * 0x85EBCA6Bu) ^ (o_lo * 0xC2B2AE35u));
}

// Multiprocessor count of the current device (cached per device id).
static int attn_cu_count() {
  static int cache[64] = {0};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
  if (!cache[dev]) {
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
    cache[dev] = n;
  }
  return cache[dev];
}

// an environment knob; every caller keeps the value in a function-local static (read once per process)
static int env_int(const char* name, int dflt) {
  const char* e = getenv(name);
  return e ? atoi(e) : dflt;
}

// Persistent grid of a kernel with `per_cu` resident workgroups per CU over `nitems` work
// items: every workgroup takes ceil(nitems / slots) items and the grid is the fewest
// workgroups that need no more rounds than that.  CLOUDTIK_AMD_ATTN_PERSIST=0: one
// workgroup per item.
static int attn_persistent_grid(long nitems, int per_cu) {
  static const int on = env_int("CLOUDTIK_AMD_ATTN_PERSIST", 1);
  if (!on || nitems <= 0) return (int)nitems;
  const long slots = (long)attn_cu_count() * per_cu;
  if (nitems <= slots) return (int)nitems;
  const long rounds = (nitems + slots - 1) / slots;
  return (int)((nitems + rounds - 1) / rounds);
}

// Relative-bias backward.  W = 32 ceil(Sq / 32) + 127 offsets per workgroup window (see
// attn_bwd_d64_kernel); the kernel keeps two windows (8 W bytes) of dynamic LDS next to its
// 66,048 static bytes, and two workgroups per CU (what __launch_bounds__(256, 2) and the
// register budget are for) leave 160 KiB / 2 - 66,048 = 15,872 bytes: W <= 1984, Sq <= 1856.
// The D = 128 backward has one workgroup per CU: 160 KiB - kBwd128Static (115,200) = 48,640 bytes,
// W <= 6080, which every call with relb_len <= kCtAttnRelBiasMax meets (W <= Sq + 158 there).
constexpr int kBwdRelMaxWindow = (160 * 1024 / 2 - 66048) / 8;
constexpr int kBwd128RelMaxWindow = (160 * 1024 - kBwd128Static) / 8;
extern "C" int ct_attn_bwd_relbias_window(int Sq) { return 32 * ((Sq + 31) / 32) + 127; }
extern "C" int ct_attn_bwd_relbias_max_window() { return kBwdRelMaxWindow; }
extern "C" int ct_attn_bwd_relbias_max_window_d(int D) { return D == 128 ? kBwd128RelMaxWindow : kBwdRelMaxWindow; }

// the kernels index rows inside one (batch, head) slice with 32-bit offsets; a row is D elements
static bool fits32(const CtAttnView& t, long rows, int D) { return rows * t.ss + D < (1L << 31); }
// 16-byte stores: o (the forwards' epilogue), dk / dv (store_row64)
static bool aligned16(const CtAttnView& t) { return !(((uintptr_t)t.p & 15) || t.sb % 8 || t.ss % 8 || t.sh % 8); }

// The refusals of ct_attn_fwd / ct_attn_bwd, in the order the codes are listed; every one comes
// before the first memset or launch, so a refused call has written nothing.
//    -1  a non-positive size, a D other than 64 or 128, or a missing pointer: lse for the d64
//        relative-bias forward, d_rel / drel_ws for the relative-bias backward; relb with
//        relb_len <= 0
//    -2  p > 0 with odd Sk (the dropout stream is drawn per element pair)
//    -4  relb_len > kCtAttnRelBiasMax
//   -10  backward: relb does not cover every (key - query) offset
//    -5  a tensor's rows do not fit 32-bit offsets
//    -7  o (forward) or dk / dv (backward) not 16-byte aligned
//    -9  relative-bias backward: the windows do not fit next to the kernel's static LDS (D 64: two
//        workgroups per CU; D 128: one)
//    -3  backward: Sk > 128 without dq_acc (float[B H Sq D])
//    -6  forward, CLOUDTIK_AMD_ATTN_FWD_PIPE route only: item count (refused by ct_attn_fwd itself)
//    -8  a launch or the memset failed (not a refusal: the stream may hold part of the call)
static int attn_refusal(const CtAttnCall& c, bool bwd) {
  const bool rel = c.relb != nullptr;
  if (c.B <= 0 || c.H <= 0 || c.Sq <= 0 || c.Sk <= 0 || (rel && c.relb_len <= 0)) return -1;
  if (c.D != 64 && c.D != 128) return -1;
  if (rel && (bwd ? !c.d_rel || !c.drel_ws : c.D == 64 && !c.lse)) return -1;
  if (c.p_drop > 0.f && (c.Sk % 2)) return -2;
  if (rel && c.relb_len > kCtAttnRelBiasMax) return -4;
  if (bwd && rel && (c.rel_base < c.Sq - 1 || (long)c.rel_base + c.Sk > c.relb_len)) return -10;
  if (!fits32(c.q, c.Sq, c.D) || !fits32(c.k, c.Sk, c.D) || !fits32(c.v, c.Sk, c.D) || !fits32(c.o, c.Sq, c.D))
    return -5;
  if (bwd && (!fits32(c.dO, c.Sq, c.D) || !fits32(c.dq, c.Sq, c.D))) return -5;
  if (bwd ? !aligned16(c.dk) || !aligned16(c.dv) : !aligned16(c.o)) return -7;
  if (bwd && rel && ct_attn_bwd_relbias_window(c.Sq) > ct_attn_bwd_relbias_max_window_d(c.D)) return -9;
  if (bwd && c.Sk > 128 && !c.dq_acc) return -3;
  return 0;
}

// one tensor's pointer and strides into the kernel arguments, together
template <class P>
static void put(const CtAttnView& t, P*& p, long& sb, long& ss, long& sh) { p = (P*)t.p; sb = t.sb; ss = t.ss; sh = t.sh; }
// The fields AttnFwdArgs and AttnBwdArgs share (two structs because each is its kernels' kernarg
// layout).  Without relb its fields are zero; at p = 0 the dropout fields are drop_params(0, ..)'s.
template <class Args>
static void fill_shared(Args& a, const CtAttnCall& c) {
  put(c.q, a.q, a.q_sb, a.q_ss, a.q_sh);
  put(c.k, a.k, a.k_sb, a.k_ss, a.k_sh);
  put(c.v, a.v, a.v_sb, a.v_ss, a.v_sh);
  put(c.o, a.o, a.o_sb, a.o_ss, a.o_sh);
  a.kbias = c.kbias; a.kb_sb = c.kb_sb; a.lse = c.lse;
  a.B = c.B; a.H = c.H; a.Sq = c.Sq; a.Sk = c.Sk;
  a.scale_log2 = c.scale * 1.4426950408889634f;
  drop_params(c.p_drop, c.seed, c.offset, &a.thr16, &a.inv_keep, &a.hash_base);
  a.causal = c.causal;
  const bool rel = c.relb != nullptr;
  a.relb = c.relb; a.relb_sh = rel ? c.relb_sh : 0; a.relb_len = rel ? c.relb_len : 0; a.rel_base = rel ? c.rel_base : 0;
}

// f(std::bool_constant<x>{}, std::bool_constant<y>{}): two runtime flags as template arguments
// (masking and dropout are template parameters of every kernel: no per-element test of a runtime
// flag in the non-causal, BERT, kernels)
template <class F>
static void with_bools(bool x, bool y, F&& f) {
  if (x && y) f(std::true_type{}, std::true_type{});
  else if (x) f(std::true_type{}, std::false_type{});
  else if (y) f(std::false_type{}, std::true_type{});
  else f(std::false_type{}, std::false_type{});
}
template <int N> using int_c = std::integral_constant<int, N>;

static int launch_rc() { return hipGetLastError() == hipSuccess ? 0 : -8; }

// Forward: writes o and lse (lse may be null without relb).  Dispatch:
//   D 128           attn_fwd_d128_kernel<CAUSAL, REL> at p = 0 (inference, and training when given lse),
//                   attn_fwd_d128_drop_kernel<CAUSAL, REL> at p > 0; the relative-bias stage in dynamic LDS
//   D 64, relb      attn_fwd_d64_kernel<DROP, CAUSAL, REL = true>, two workgroups per CU (T5: inference at
//                   p = 0, training with the dropout stream of the plain forward)
//   D 64            attn_fwd_d64_kernel<DROP, CAUSAL, false, WPE, GL>, or attn_fwd_pipe_kernel, by the knobs
extern "C" int ct_attn_fwd(const CtAttnCall* call, hipStream_t stream) {
  const CtAttnCall& c = *call;
  if (const int rc = attn_refusal(c, false)) return rc;
  AttnFwdArgs a;
  fill_shared(a, c);
  const dim3 grid((c.Sq + 127) / 128, c.B * c.H);
  const bool drop = c.p_drop > 0.f, causal = c.causal != 0, rel = c.relb != nullptr;
  if (c.D == 128) {
    const size_t dyn = rel ? (size_t)c.relb_len * sizeof(float) : 0;
    with_bools(causal, rel, [&](auto CA, auto RE) {
      if (drop) attn_fwd_d128_drop_kernel<CA.value, RE.value><<<grid, 256, dyn, stream>>>(a);
      else attn_fwd_d128_kernel<CA.value, RE.value><<<grid, 256, dyn, stream>>>(a);
    });
    return launch_rc();
  }
  if (rel) {
    with_bools(drop, causal, [&](auto DR, auto CA) {
      attn_fwd_d64_kernel<DR.value, CA.value, true><<<grid, 256, 0, stream>>>(a);
    });
    return launch_rc();
  }
  // default: 2 waves/SIMD.  (r3: 3 with dropout, 168 VGPRs, 74-75 vs 77-78 us per BERT-large
  // layer; since both K/V tiles of an S <= 128 item load up front the 3-wave build spills one
  // register and the BERT-large step is 0.03-0.06 ms faster at 2 in three interleaved rounds:
  // 72.63 / 72.60 / 72.36 vs 72.57 / 72.55 / 72.34 ms)
  static const int wpe_env = env_int("CLOUDTIK_AMD_ATTN_FWD_WPE", 0);
  static const int gl = env_int("CLOUDTIK_AMD_ATTN_FWD_GLDS", 1);
  const int wpe = (wpe_env >= 1 && wpe_env <= 4) ? wpe_env : (gl ? 3 : 2);
  // opt-in: measured slower than the one-item kernel on BERT-large shapes (B 256, S 128,
  // p 0.1: 75.5 us persistent / 84.9 us one item per workgroup vs 65.9 us;
  // profiles/r3/attention_persistent_ab.md)
  static const int pipe = env_int("CLOUDTIK_AMD_ATTN_FWD_PIPE", 0);
  if (pipe) {
    const long nitems = (long)grid.x * c.B * c.H;
    if (nitems > (1L << 30)) return -6;
    const int g1 = attn_persistent_grid(nitems, 2);
    with_bools(drop, causal, [&](auto DR, auto CA) {
      attn_fwd_pipe_kernel<DR.value, CA.value><<<g1, 256, 0, stream>>>(a);
    });
    return launch_rc();
  }
  auto launch = [&](auto W, auto G) {
    with_bools(drop, causal, [&](auto DR, auto CA) {
      attn_fwd_d64_kernel<DR.value, CA.value, false, W.value, G.value><<<grid, 256, 0, stream>>>(a);
    });
  };
  if (gl) {
    if (wpe == 4) launch(int_c<4>{}, std::true_type{});
    else if (wpe == 3) launch(int_c<3>{}, std::true_type{});
    else launch(int_c<2>{}, std::true_type{});
  } else {
    if (wpe == 3) launch(int_c<3>{}, std::false_type{});
    else if (wpe == 1) launch(int_c<1>{}, std::false_type{});
    else launch(int_c<2>{}, std::false_type{});
  }
  return launch_rc();
}

// Backward: writes dq, dk, dv and, with relb, every entry of d_rel.  Dispatch at D 64:
//   no relb   attn_bwd_d64_kernel<DROP, CAUSAL, MULTI, GL>: Sk > 128 -> MULTI (dQ summed in dq_acc, zeroed
//             here, then attn_dq_convert_kernel); otherwise one key block, by LDS DMA (GL) when Sq <= 128
//             and CLOUDTIK_AMD_ATTN_BWD_GL is not 0
//   relb      attn_bwd_d64_rel_kernel<DROP, CAUSAL, MULTI>: the register-staged single-block form for
//             every Sq when Sk <= 128 (REL has no LDS-DMA form); two windows of dynamic LDS; then
//             attn_drel_reduce_kernel sums the windows in drel_ws into d_rel
// At D 128 every call runs attn_bwd_d128_kernel<DROP, CAUSAL, MULTI, REL> (register-staged, one workgroup
// per CU), followed by the same convert (Sk > 128) and reduce (relb) kernels.
extern "C" int ct_attn_bwd(const CtAttnCall* call, hipStream_t stream) {
  const CtAttnCall& c = *call;
  if (const int rc = attn_refusal(c, true)) return rc;
  const bool drop = c.p_drop > 0.f, causal = c.causal != 0, rel = c.relb != nullptr;
  AttnBwdArgs a;
  fill_shared(a, c);
  put(c.dO, a.dO, a.do_sb, a.do_ss, a.do_sh);
  put(c.dq, a.dq, a.dq_sb, a.dq_ss, a.dq_sh);
  put(c.dk, a.dk, a.dk_sb, a.dk_ss, a.dk_sh);
  put(c.dv, a.dv, a.dv_sb, a.dv_ss, a.dv_sh);
  a.dq_acc = c.dq_acc; a.scale = c.scale;
  a.delta = rel ? nullptr : c.delta; a.drel_ws = rel ? c.drel_ws : nullptr;
  const long rows = (long)c.B * c.H * c.Sq;
  const int nkb = (c.Sk + 127) / 128, W = ct_attn_bwd_relbias_window(c.Sq);
  const bool multi = nkb > 1;
  if (multi && hipMemsetAsync(c.dq_acc, 0, sizeof(float) * rows * c.D, stream) != hipSuccess) return -8;
  const dim3 grid(nkb, c.B * c.H);
  if (c.D == 128) {
    const size_t dyn = rel ? (size_t)W * 2 * sizeof(float) : 0;
    auto launch = [&](auto MU, auto RE) {
      with_bools(drop, causal, [&](auto DR, auto CA) {
        attn_bwd_d128_kernel<DR.value, CA.value, MU.value, RE.value><<<grid, 256, dyn, stream>>>(a);
      });
    };
    with_bools(multi, rel, launch);
  } else if (rel) {
    const size_t dyn = (size_t)W * 2 * sizeof(float);
    auto launch = [&](auto MU) {
      with_bools(drop, causal, [&](auto DR, auto CA) {
        attn_bwd_d64_rel_kernel<DR.value, CA.value, MU.value><<<grid, 256, dyn, stream>>>(a);
      });
    };
    if (multi) launch(std::true_type{}); else launch(std::false_type{});
  } else {
    static const int bwd_gl = env_int("CLOUDTIK_AMD_ATTN_BWD_GL", 1);
    auto launch = [&](auto MU, auto G) {
      with_bools(drop, causal, [&](auto DR, auto CA) {
        attn_bwd_d64_kernel<DR.value, CA.value, MU.value, G.value><<<grid, 256, 0, stream>>>(a);
      });
    };
    if (multi) launch(std::true_type{}, std::false_type{});
    else if (bwd_gl && c.Sq <= 128) launch(std::false_type{}, std::true_type{});
    else launch(std::false_type{}, std::false_type{});
  }
  if (launch_rc()) return -8;
  if (multi)
    attn_dq_convert_kernel<<<(int)((rows * c.D + 255) / 256), 256, 0, stream>>>(
        c.dq_acc, a.dq, a.dq_sb, a.dq_ss, a.dq_sh, c.B, c.H, c.Sq, c.D == 128 ? 7 : 6);
  // window of key block 0 starts at offset 1 - 32 nq + rel_base = rel_base + 128 - W
  if (rel)
    attn_drel_reduce_kernel<<<(c.H * c.relb_len + 255) / 256, 256, 0, stream>>>(
        c.drel_ws, c.d_rel, c.d_sh, c.d_si, c.B, nkb, c.H, W, c.relb_len, c.rel_base + 128 - W);
  return launch_rc();
}

