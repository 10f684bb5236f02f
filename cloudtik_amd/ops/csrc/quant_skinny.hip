// Int8 kernels for the decode step of a quantized encoder-decoder (gfx950): the RMS norm that also
// emits its output quantized per row, and the int8 GEMM for M <= 64 activation rows.  Number
// format and rounding rule: quant.hip (symmetric int8, one fp32 scale per activation row and per
// weight output channel, exact int32 accumulation on v_mfma_i32_16x16x64_i8).
//
// A decode step multiplies batch x beams rows against every weight matrix, so each weight byte
// is used once and the step is bound by its launches and by how fast the weights stream in, not
// by the matrix cores.  Hence (a) the norm in front of a GEMM writes the GEMM's int8 operand and
// its row scales itself (no separate quantize launch), (b) the GEMM's epilogue carries the ReLU
// or the residual add that follows it, and (c) the GEMM is a weight-streaming kernel, not a
// shrunken tile: see gemm_i8_skinny_kernel.
#include "common.h"

namespace ct {
namespace {

typedef __attribute__((ext_vector_type(4))) int i32x4;
typedef __attribute__((ext_vector_type(2))) int i32x2;

// quant.hip's rule: ONE fp32 multiply, round-half-to-even, clamp
__device__ __forceinline__ int sk_quant1(bf16_t e, float inv) {
  const float r = rintf(bf2f(e) * inv);
  return (int)fminf(fmaxf(r, -127.f), 127.f);
}
__device__ __forceinline__ int sk_quant4(bf16_t e0, bf16_t e1, bf16_t e2, bf16_t e3, float inv) {
  return (sk_quant1(e0, inv) & 0xFF) | ((sk_quant1(e1, inv) & 0xFF) << 8) | ((sk_quant1(e2, inv) & 0xFF) << 16) |
         ((sk_quant1(e3, inv) & 0xFF) << 24);
}

// ------------------------------------------------------------------ RMS norm + row quantization
// y = RMSNorm(x + res) * gamma with the structure and the arithmetic of ln_fwd_kernel<MAXV, true>
// (layernorm.hip: one wave per row, the row in registers, the bf16-rounded sum normalised), then
// (q, scale) = quant_rows_i8 of the ROUNDED bf16 y, so the pair equals what the unfused chain
// (norm, then quant_rows_i8) produces.  Y may be null (the consumer takes int8 only).
template <int MAXV>
__global__ __launch_bounds__(256) void rmsnorm_quant_rows_kernel(const bf16_t* __restrict__ X,
                                                                 const bf16_t* __restrict__ res,
                                                                 const bf16_t* __restrict__ gamma,
                                                                 bf16_t* __restrict__ Y, int8_t* __restrict__ Q,
                                                                 float* __restrict__ S, int M, int N, float eps) {
  const int lane = threadIdx.x & 63;
  const int wpb = blockDim.x >> 6;
  const int nvec = N >> 3;
  const bool has_res = res != nullptr;
  for (int row = blockIdx.x * wpb + (threadIdx.x >> 6); row < M; row += gridDim.x * wpb) {
    const u16x8* xr = reinterpret_cast<const u16x8*>(X + (size_t)row * N);
    const u16x8* rr = reinterpret_cast<const u16x8*>(res + (size_t)row * N);
    float v[MAXV][8];
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
      const int c = lane + i * 64;
      if (c < nvec) {
        const u16x8 xv = xr[c];
        u16x8 rv = u16x8(0);
        if (has_res) rv = rr[c];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          float t = bf2f(xv[j]) + 0.f;          // the (absent) bias of the LayerNorm kernel
          t += bf2f(rv[j]);
          v[i][j] = bf2f(f2bf(t));
        }
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[i][j] = 0.f;
      }
    }
    float var = 0.f;
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
      if (lane + i * 64 < nvec) {
#pragma unroll
        for (int j = 0; j < 8; ++j) { const float d = v[i][j]; var += d * d; }
      }
    }
    var = wave_sum(var) / N;
    const float rstd = rsqrtf(var + eps);
    const u16x8* g8 = reinterpret_cast<const u16x8*>(gamma);
    u16x8 o[MAXV];
    float amax = 0.f;
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
      const int c = lane + i * 64;
      if (c < nvec) {
        const u16x8 g = g8[c];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          o[i][j] = f2bf(v[i][j] * rstd * bf2f(g[j]) + 0.f);
          amax = fmaxf(amax, fabsf(bf2f(o[i][j])));
        }
        if (Y) reinterpret_cast<u16x8*>(Y + (size_t)row * N)[c] = o[i];
      }
    }
    amax = wave_max(amax);
    const float inv = amax > 0.f ? 127.0f / amax : 0.f;
    if (lane == 0) S[row] = amax / 127.0f;
    i32x2* qr = reinterpret_cast<i32x2*>(Q + (size_t)row * N);
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
      const int c = lane + i * 64;
      if (c < nvec) {
        i32x2 p;
        p[0] = sk_quant4(o[i][0], o[i][1], o[i][2], o[i][3], inv);
        p[1] = sk_quant4(o[i][4], o[i][5], o[i][6], o[i][7], inv);
        qr[c] = p;
      }
    }
  }
}

// ------------------------------------------------------------------------------ the skinny GEMM
// D[M <= 64, N] = epilogue(A[M, K] . W[N, K]^T), both int8 and K-contiguous, in one launch.
//
// A workgroup of four waves owns 16 output channels (one MFMA fragment of W rows) over ALL of K
// and every activation row; its waves split K: in iteration `it` wave w multiplies the 64-byte K
// step at k = 256 it + 64 w.  With 16 channels per workgroup even N = 768 gives 48 workgroups of
// four waves, each streaming its own bytes; the four int32 partials are added through LDS after
// the loop (integers: any order is exact), so nothing crosses workgroups and there is no second
// pass.
//
// Weights: used by exactly one wave, so they go from global memory straight to VGPRs as 16-byte
// loads (a lane's 16 bytes are k = 64 s + 16 (lane >> 4) .. + 15 of row lane & 15: the fragment the
// MFMA takes), kSkDepth K steps in flight per wave in a register ring -- the load of step
// s + kSkDepth is issued as soon as step s has been multiplied, and nothing waits for it until
// its turn comes.
//
// Activations: the [16 MT rows][256 bytes] K slab of an iteration is read from global memory in
// full 256-byte row pieces by the whole workgroup (consecutive lanes, consecutive 16-byte slots)
// and staged in LDS, double-buffered with one barrier per iteration; each wave reads its
// fragments out of it.  Slot s of row r is stored at slot s ^ (r & 15), so the 16 rows one
// ds_read_b128 group serves fall on 16 different slots.  Rows >= M and bytes >= K are zero.
//
// As in gemm_i8_nt_kernel W is the MFMA's A operand and the activations its B operand, so a lane
// holds four consecutive n of one m (col = lane & 15 -> m, row = 4 (lane >> 4) + reg -> n) and
// stores them as one vector.
//
// Epilogue (RAW false), in the order ops.reference.dequant_epilogue states: f = acc * (sa[m] * sw[n])
// as two separate fp32 multiplies, + bias[n], ReLU, y = bf16(f), and with a residual
// y = bf16(float(y) + float(res[m, n])) -- rounded BEFORE the add, so the fused op equals the
// unfused chain.  A lane reads its four residual values before it stores, so D may alias res.
// RAW true stores the int32 accumulators.
constexpr int kSkBK = 256;      // bytes of K per workgroup iteration: one MFMA step per wave
constexpr int kSkWaves = 4;
constexpr int kSkDepth = 4;     // weight K steps in flight per wave

template <int MT, bool RAW>
__global__ __launch_bounds__(64 * kSkWaves) void gemm_i8_skinny_kernel(
    const int8_t* __restrict__ A, const int8_t* __restrict__ W, const float* __restrict__ sa,
    const float* __restrict__ sw, const bf16_t* __restrict__ bias, const bf16_t* res, void* Dv, int M, int N, int K,
    int relu) {
  constexpr int ROWS = 16 * MT, T = 64 * kSkWaves;
  static_assert(ROWS * 16 == MT * T, "one 16-byte slot of the slab per thread and MT");
  static_assert(kSkWaves * MT * 64 * 16 <= 2 * ROWS * kSkBK, "the partial sums reuse the slabs");
  __shared__ __attribute__((aligned(16))) int8_t lds[2 * ROWS * kSkBK];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int n0 = blockIdx.x * 16;
  const int nit = (K + kSkBK - 1) / kSkBK;

  // tails read a clamped (valid) address and are zeroed: no branch per load
  const int8_t* wp = W + (size_t)(n0 + (lane & 15)) * K + 16 * (lane >> 4);
  auto wload = [&](int it) -> i32x4 {
    const int k = it * kSkBK + 64 * wid;
    const i32x4 v = *reinterpret_cast<const i32x4*>(wp + min(k, K - 64));
    return k < K ? v : (i32x4)(0);
  };
  i32x4 ra[MT];
  auto gload = [&](int it) {
#pragma unroll
    for (int i = 0; i < MT; ++i) {
      const int c = tid + T * i, gm = c >> 4, k = it * kSkBK + (c & 15) * 16;
      const i32x4 v = *reinterpret_cast<const i32x4*>(A + (size_t)min(gm, M - 1) * K + min(k, K - 16));
      ra[i] = (gm < M && k < K) ? v : (i32x4)(0);
    }
  };
  auto lstore = [&](int buf) {
#pragma unroll
    for (int i = 0; i < MT; ++i) {
      const int c = tid + T * i, row = c >> 4, slot = c & 15;
      *reinterpret_cast<i32x4*>(lds + buf * (ROWS * kSkBK) + row * kSkBK + ((slot ^ (row & 15)) << 4)) = ra[i];
    }
  };

  i32x4 acc[MT];
#pragma unroll
  for (int i = 0; i < MT; ++i) acc[i] = (i32x4)(0);
  i32x4 wr[kSkDepth];
#pragma unroll
  for (int d = 0; d < kSkDepth; ++d) wr[d] = wload(d);       // steps past K come back zero

  gload(0);
  lstore(0);
  __syncthreads();
  for (int it0 = 0; it0 < nit; it0 += kSkDepth) {
#pragma unroll
    for (int d = 0; d < kSkDepth; ++d) {
      const int it = it0 + d;
      if (it < nit) {                              // uniform over the workgroup
        const bool more = it + 1 < nit;
        if (more) gload(it + 1);
        const int8_t* slab = lds + (it & 1) * (ROWS * kSkBK);
        const int slot = 4 * wid + (lane >> 4);
#pragma unroll
        for (int i = 0; i < MT; ++i) {
          const int r = i * 16 + (lane & 15);
          const i32x4 fa = *reinterpret_cast<const i32x4*>(slab + r * kSkBK + ((slot ^ (r & 15)) << 4));
          acc[i] = __builtin_amdgcn_mfma_i32_16x16x64_i8(wr[d], fa, acc[i], 0, 0, 0);
        }
        wr[d] = wload(it + kSkDepth);
        if (more) lstore((it + 1) & 1);            // the slab iteration it - 1 read: all waves are past it
        __syncthreads();
      }
    }
  }

  // the waves' partial sums, through the (now idle) slabs; wave w then finishes fragments w, w + 4, ..
  int* red = reinterpret_cast<int*>(lds);
#pragma unroll
  for (int i = 0; i < MT; ++i)
    *reinterpret_cast<i32x4*>(red + ((wid * MT + i) * 64 + lane) * 4) = acc[i];
  __syncthreads();
#pragma unroll
  for (int i = 0; i < MT; ++i) {
    if ((i % kSkWaves) != wid) continue;           // uniform over the wave
    i32x4 a = (i32x4)(0);
#pragma unroll
    for (int w = 0; w < kSkWaves; ++w) a += *reinterpret_cast<const i32x4*>(red + ((w * MT + i) * 64 + lane) * 4);
    const int m = i * 16 + (lane & 15);
    if (m >= M) continue;
    const int n = n0 + 4 * (lane >> 4);            // N % 16 == 0 and n % 4 == 0: n + 3 < N
    const size_t o = (size_t)m * N + n;
    if constexpr (RAW) {
      *reinterpret_cast<i32x4*>(reinterpret_cast<int*>(Dv) + o) = a;
    } else {
      const float sam = sa[m];
      const f32x4 s = *reinterpret_cast<const f32x4*>(sw + n);
      u16x4 b = {0, 0, 0, 0}, rv = {0, 0, 0, 0}, y;
      if (bias) b = *reinterpret_cast<const u16x4*>(bias + n);
      if (res) rv = *reinterpret_cast<const u16x4*>(res + o);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        // the reference's operation order with every step rounded: contraction is switched off
        // for this block, which therefore uses plain operators (__fmul_rn / __fadd_rn are inline
        // functions compiled with contraction on, and their results still fuse).  A product
        // fused into the bias add breaks bf16 ties the other way.
#pragma clang fp contract(off)
        float f = (float)a[r] * (sam * s[r]);
        if (bias) f = f + bf2f(b[r]);
        if (relu) f = f < 0.f ? 0.f : f;           // keeps a NaN, as the reference does
        y[r] = f2bf(f);
        if (res) y[r] = f2bf(bf2f(y[r]) + bf2f(rv[r]));
      }
      *reinterpret_cast<u16x4*>(reinterpret_cast<bf16_t*>(Dv) + o) = y;
    }
  }
}

}  // namespace
}  // namespace ct

extern "C" {

// (Y bf16 [M, N] unless null, Q int8 [M, N], S fp32 [M]) = RMSNorm(X + res) * gamma and its row
// quantization.  res optional.  N % 16 == 0, N <= 2048.
int ct_rmsnorm_quant_rows(const void* X, const void* res, const void* gamma, void* Y, void* Q, float* S, int M, int N,
                          float eps, hipStream_t stream) {
  if (M <= 0 || N <= 0 || N % 16 || N > 2048 || !X || !gamma || !Q || !S) return 1;
  auto* x = reinterpret_cast<const ct::bf16_t*>(X);
  auto* r = reinterpret_cast<const ct::bf16_t*>(res);
  auto* g = reinterpret_cast<const ct::bf16_t*>(gamma);
  auto* y = reinterpret_cast<ct::bf16_t*>(Y);
  auto* q = reinterpret_cast<int8_t*>(Q);
  const int mv = (N / 8 + 63) / 64;
  int grid = ct::ceil_div(M, 4);
  if (grid > 16384) grid = 16384;
#define CT_RQ(MV) case MV: ct::rmsnorm_quant_rows_kernel<MV><<<grid, 256, 0, stream>>>(x, r, g, y, q, S, M, N, eps); break;
  switch (mv) {
    CT_RQ(1) CT_RQ(2) CT_RQ(3) CT_RQ(4)
    default: return 1;
  }
#undef CT_RQ
  return 0;
}

// raw 0: bf16 D = act((A W^T) * sa[m] * sw[n] + bias[n]) (+ res), act 0 none / 2 ReLU; raw 1: int32
// D = A W^T.  1 <= M <= 64, K % 64 == 0, K <= 8192, N % 64 == 0.
int ct_gemm_i8_skinny(const void* A, const void* W, const float* sa, const float* sw, const void* bias,
                      const void* res, void* D, int M, int N, int K, int act, int raw, hipStream_t stream) {
  if (M <= 0 || M > 64 || N <= 0 || K <= 0 || K % 64 || N % 64 || K > 8192 || !A || !W || !D) return 1;
  if (!raw && (!sa || !sw || (act != 0 && act != 2))) return 1;
  auto* a = reinterpret_cast<const int8_t*>(A);
  auto* w = reinterpret_cast<const int8_t*>(W);
  auto* b = reinterpret_cast<const ct::bf16_t*>(bias);
  auto* r = reinterpret_cast<const ct::bf16_t*>(res);
  const int grid = N / 16, threads = 64 * ct::kSkWaves, relu = act == 2;
#define CT_SK(MT) case MT: \
    if (raw) ct::gemm_i8_skinny_kernel<MT, true><<<grid, threads, 0, stream>>>(a, w, nullptr, nullptr, nullptr, nullptr, \
                                                                              D, M, N, K, 0); \
    else ct::gemm_i8_skinny_kernel<MT, false><<<grid, threads, 0, stream>>>(a, w, sa, sw, b, r, D, M, N, K, relu); \
    break;
  switch ((M + 15) / 16) {
    CT_SK(1) CT_SK(2) CT_SK(3) CT_SK(4)
    default: return 1;
  }
#undef CT_SK
  return 0;
}

}  // extern "C"
