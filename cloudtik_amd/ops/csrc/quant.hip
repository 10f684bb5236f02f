// Int8 post-training quantization kernels for gfx950: dynamic per-row symmetric quantization
// of a bf16 activation matrix, and the int8 x int8 -> int32 NT GEMM on the i8 matrix cores
// with a fp32 dequantize (+ bias, + GELU) epilogue.  Inference only.
//
// Number format: symmetric, no zero point.  A row's scale is amax / 127 (fp32, IEEE divide);
// elements are q = clamp(rne(x * (127 / amax)), -127, 127) with ONE fp32 multiply (nothing to
// contract into an fma) and round-half-to-even, so a host implementation of the same formula
// is bit-equal.  An all-zero row has scale 0 and q 0.
//
// Static quantization uses the same rule with a calibrated range in place of the row maximum:
// the host computes scale = amax / 127 and inv = 127 / amax once and passes them by value, so
// the cast is elementwise (values beyond the range saturate) and sits in whatever kernel writes
// the tensor: a plain cast (quant_static_i8_kernel), the LayerNorm (ln_quant_fwd_kernel) and
// the GEMM epilogue (MODE 5 / 6 below).  Each of them quantizes the ROUNDED bf16 value it
// would have stored, so a fused producer and the unfused chain agree bit for bit.
#include "common.h"

namespace ct {

typedef __attribute__((ext_vector_type(4))) int i32x4;

// ------------------------------------------------------------------------- row quantization
// Each thread owns up to two 16-element chunks of its row (two 16-byte loads in, one 16-byte
// store out per chunk).  WAVE: one row per wave, four rows per block (K <= 2048); otherwise
// one row per 256-thread block (K <= 8192) with the maximum combined through LDS.
__device__ __forceinline__ int quant1(bf16_t e, float inv) {
  const float r = rintf(bf2f(e) * inv);
  return (int)fminf(fmaxf(r, -127.f), 127.f);
}

template <bool WAVE>
__global__ __launch_bounds__(256) void quant_rows_i8_kernel(const bf16_t* __restrict__ X, int8_t* __restrict__ Q,
                                                            float* __restrict__ S, int M, int K) {
  __shared__ float red[4];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int row = WAVE ? blockIdx.x * 4 + wid : blockIdx.x;
  const int t = WAVE ? lane : (int)threadIdx.x;
  constexpr int kStride = WAVE ? 64 : 256;
  const bool live = row < M;                       // uniform over the wave (WAVE) / the block
  if (WAVE && !live) return;
  const int nch = K >> 4;
  const bf16_t* x = X + (size_t)(live ? row : 0) * K;
  u16x8 v[2][2];
  float amax = 0.f;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int c = t + i * kStride;
    if (live && c < nch) {
      v[i][0] = *reinterpret_cast<const u16x8*>(x + c * 16);
      v[i][1] = *reinterpret_cast<const u16x8*>(x + c * 16 + 8);
#pragma unroll
      for (int j = 0; j < 8; ++j)
        amax = fmaxf(amax, fmaxf(fabsf(bf2f(v[i][0][j])), fabsf(bf2f(v[i][1][j]))));
    }
  }
  amax = wave_max(amax);
  if (!WAVE) {
    if (lane == 0) red[wid] = amax;
    __syncthreads();
    amax = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    if (!live) return;
  }
  const float inv = amax > 0.f ? 127.0f / amax : 0.f;
  if (t == 0) S[row] = amax / 127.0f;
  int8_t* q = Q + (size_t)row * K;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int c = t + i * kStride;
    if (c < nch) {
      i32x4 o;
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        const u16x8& s = v[i][w >> 1];
        const int b = (w & 1) * 4;
        o[w] = (quant1(s[b], inv) & 0xFF) | ((quant1(s[b + 1], inv) & 0xFF) << 8) |
               ((quant1(s[b + 2], inv) & 0xFF) << 16) | ((quant1(s[b + 3], inv) & 0xFF) << 24);
      }
      *reinterpret_cast<i32x4*>(q + c * 16) = o;
    }
  }
}

// ------------------------------------------------------------------- static quantization
__device__ __forceinline__ int quant4(bf16_t e0, bf16_t e1, bf16_t e2, bf16_t e3, float inv) {
  return (quant1(e0, inv) & 0xFF) | ((quant1(e1, inv) & 0xFF) << 8) | ((quant1(e2, inv) & 0xFF) << 16) |
         ((quant1(e3, inv) & 0xFF) << 24);
}

// Elementwise bf16 -> int8 with one given inv: a thread owns one 16-element chunk.
__global__ __launch_bounds__(256) void quant_static_i8_kernel(const bf16_t* __restrict__ X, int8_t* __restrict__ Q,
                                                              float inv, long nch) {
  const long c = (long)blockIdx.x * 256 + threadIdx.x;
  if (c >= nch) return;
  const u16x8 v0 = *reinterpret_cast<const u16x8*>(X + c * 16);
  const u16x8 v1 = *reinterpret_cast<const u16x8*>(X + c * 16 + 8);
  i32x4 o;
  o[0] = quant4(v0[0], v0[1], v0[2], v0[3], inv);
  o[1] = quant4(v0[4], v0[5], v0[6], v0[7], inv);
  o[2] = quant4(v1[0], v1[1], v1[2], v1[3], inv);
  o[3] = quant4(v1[4], v1[5], v1[6], v1[7], inv);
  *reinterpret_cast<i32x4*>(Q + c * 16) = o;
}

// Inference forward of y = LN(res + (x + bias)) * gamma + beta that also writes q = quant(y):
// the structure and the arithmetic of ln_fwd_kernel (layernorm.hip; one wave per row, the row
// in registers, N % 8 == 0, N <= 2048) without dropout, the saved sum and the statistics.
// QOUT false writes y alone (the consumer of this LayerNorm is not an int8 site).
typedef __attribute__((ext_vector_type(2))) int i32x2;

template <int MAXV, bool QOUT>
__global__ __launch_bounds__(256) void ln_quant_fwd_kernel(const bf16_t* __restrict__ X, const bf16_t* __restrict__ bias,
                                                           const bf16_t* __restrict__ res,
                                                           const bf16_t* __restrict__ gamma,
                                                           const bf16_t* __restrict__ beta, bf16_t* __restrict__ Y,
                                                           int8_t* __restrict__ Q, int M, int N, float eps, float inv) {
  const int lane = threadIdx.x & 63;
  const int wpb = blockDim.x >> 6;
  const int nvec = N >> 3;
  const bool has_bias = bias != nullptr, has_res = res != nullptr;
  for (int row = blockIdx.x * wpb + (threadIdx.x >> 6); row < M; row += gridDim.x * wpb) {
    const u16x8* xr = reinterpret_cast<const u16x8*>(X + (size_t)row * N);
    const u16x8* rr = reinterpret_cast<const u16x8*>(res + (size_t)row * N);
    const u16x8* br = reinterpret_cast<const u16x8*>(bias);
    float v[MAXV][8];
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
      const int c = lane + i * 64;
      if (c < nvec) {
        const u16x8 xv = xr[c];
        u16x8 bv = u16x8(0), rv = u16x8(0);
        if (has_bias) bv = br[c];
        if (has_res) rv = rr[c];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          float t = bf2f(xv[j]) + bf2f(bv[j]);
          t += bf2f(rv[j]);
          v[i][j] = bf2f(f2bf(t));  // the rounded sum, as the training kernel normalises it
          sum += v[i][j];
        }
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[i][j] = 0.f;
      }
    }
    sum = wave_sum(sum);
    const float mean = sum / N;
    float var = 0.f;
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
      if (lane + i * 64 < nvec) {
#pragma unroll
        for (int j = 0; j < 8; ++j) { const float d = v[i][j] - mean; var += d * d; }
      }
    }
    var = wave_sum(var) / N;
    const float rstd = rsqrtf(var + eps);
    u16x8* yr = reinterpret_cast<u16x8*>(Y + (size_t)row * N);
    i32x2* qr = reinterpret_cast<i32x2*>(Q + (size_t)row * N);
    const u16x8* g8 = reinterpret_cast<const u16x8*>(gamma);
    const u16x8* b8 = reinterpret_cast<const u16x8*>(beta);
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
      const int c = lane + i * 64;
      if (c < nvec) {
        const u16x8 g = g8[c];
        u16x8 bb = u16x8(0);
        if (beta) bb = b8[c];
        u16x8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = f2bf((v[i][j] - mean) * rstd * bf2f(g[j]) + bf2f(bb[j]));
        yr[c] = o;
        if constexpr (QOUT) {
          i32x2 p;
          p[0] = quant4(o[0], o[1], o[2], o[3], inv);
          p[1] = quant4(o[4], o[5], o[6], o[7], inv);
          qr[c] = p;
        }
      }
    }
  }
}

// --------------------------------------------------------------------------------- the GEMM
// D[M,N] = A[M,K] . W[N,K]^T, both int8 and K-contiguous, exact int32 accumulation on
// v_mfma_i32_16x16x64_i8.  A block of 2 x WN waves, each owning MF x 4 fragments of 16 x 16,
// computes one (32 MF) x (64 WN) output tile in 128-byte K steps.  The next K tile is fetched
// into registers while the current one is multiplied out of LDS; with OCC blocks per CU the
// other blocks' MFMAs cover a block's wait for that fetch (one K tile of MFMAs is much shorter
// than the load latency, so occupancy is what sets the speed here: 2 -> 3 blocks per CU took
// the M = 8192, N = 3072, K = 1024 GEMM from 72 to 55 us).
//
// LDS image: [rows][128 bytes] per operand, the 16-byte slot s of row r stored at slot
// s ^ (r & 7): the 16 lanes that one ds_read_b128 group serves (rows r .. r + 15 of a fragment,
// slots 4 ks + (lane >> 4)) then fall on 16 different 4-bank slots.
//
// Fragments: a lane's 16 bytes are k = 64 ks + 16 (lane >> 4) .. + 15 of its row for BOTH
// operands, so whatever order the instruction takes the k values of a fragment in, it is the
// same for both and cancels in the sum.  W is the MFMA's A operand (rows of the result), the
// activations its B operand (columns), so a lane holds four consecutive n of one m
// (col = lane & 15 -> m, row = 4 (lane >> 4) + reg -> n) and stores them as one vector.
//
// MODE 0: bf16 out, y = acc * (sa[m] * sw[n]) + bias[n];  MODE 1: the same through GELU (erf);
// MODE 2: the raw int32 accumulators.  MODE 3 / 4: MODE 0 / 1 with one by-value activation scale
// sa_s in place of sa[m] (static quantization);  MODE 5 / 6: the same, the bf16 result quantized
// with inv_out and written as int8 (a lane's four n are one 32-bit store).
constexpr int kBK = 128;

template <int MODE, int MF, int WN, int OCC>
__global__ __launch_bounds__(128 * WN, OCC) void gemm_i8_nt_kernel(const int8_t* __restrict__ A, const int8_t* __restrict__ W,
                                                         const float* __restrict__ sa, const float* __restrict__ sw,
                                                         const bf16_t* __restrict__ bias, void* __restrict__ Dv,
                                                         int M, int N, int K, float sa_s, float inv_out) {
  constexpr bool kRaw = MODE == 2, kStatic = MODE >= 3, kGelu = MODE == 1 || MODE == 4 || MODE == 6, kI8 = MODE >= 5;
  // 2 x WN waves, each MF x 4 fragments: the block's tile is (32 MF) x (64 WN)
  constexpr int T = 128 * WN, BM = 32 * MF, BN = 64 * WN;
  constexpr int CA = BM * 8 / T, CW = BN * 8 / T;       // 16-byte chunks per thread and K tile
  __shared__ __attribute__((aligned(16))) int8_t lds[(BM + BN) * kBK];
  int8_t* lA = lds;
  int8_t* lW = lds + BM * kBK;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wm = wid / WN, wn = wid % WN;
  // consecutive tiles (n fastest) run on one XCD, so its L2 holds one A panel for them (walking
  // 8 M-tiles per N-tile instead measured the same within noise)
  const int tiles_n = (N + BN - 1) / BN;
  const int L = xcd_remap(blockIdx.x, gridDim.x);
  const int m0 = (L / tiles_n) * BM, n0 = (L % tiles_n) * BN;

  i32x4 ra[CA], rw[CW];
  auto gload = [&](int k0) {
#pragma unroll
    for (int i = 0; i < CA; ++i) {
      // tail rows / the K tail read a clamped (valid) address and are zeroed: no branch per load
      const int c = tid + T * i, gm = m0 + (c >> 3), k = k0 + (c & 7) * 16;
      const i32x4 v = *reinterpret_cast<const i32x4*>(A + (size_t)min(gm, M - 1) * K + min(k, K - 16));
      ra[i] = (gm < M && k < K) ? v : (i32x4)(0);
    }
#pragma unroll
    for (int i = 0; i < CW; ++i) {
      const int c = tid + T * i, gn = n0 + (c >> 3), k = k0 + (c & 7) * 16;
      const i32x4 v = *reinterpret_cast<const i32x4*>(W + (size_t)min(gn, N - 1) * K + min(k, K - 16));
      rw[i] = (gn < N && k < K) ? v : (i32x4)(0);
    }
  };
  auto lstore = [&]() {
#pragma unroll
    for (int i = 0; i < CA; ++i) {
      const int c = tid + T * i, row = c >> 3, slot = c & 7;
      *reinterpret_cast<i32x4*>(lA + row * kBK + ((slot ^ (row & 7)) << 4)) = ra[i];
    }
#pragma unroll
    for (int i = 0; i < CW; ++i) {
      const int c = tid + T * i, row = c >> 3, slot = c & 7;
      *reinterpret_cast<i32x4*>(lW + row * kBK + ((slot ^ (row & 7)) << 4)) = rw[i];
    }
  };

  i32x4 acc[MF][4];
#pragma unroll
  for (int i = 0; i < MF; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = (i32x4)(0);

  gload(0);
  lstore();
  __syncthreads();
  for (int k0 = 0; k0 < K; k0 += kBK) {
    const bool more = k0 + kBK < K;
    if (more) gload(k0 + kBK);
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const int slot = ks * 4 + (lane >> 4);
      i32x4 fa[MF], fw[4];
#pragma unroll
      for (int i = 0; i < MF; ++i) {
        const int r = wm * (16 * MF) + i * 16 + (lane & 15);
        fa[i] = *reinterpret_cast<const i32x4*>(lA + r * kBK + ((slot ^ (r & 7)) << 4));
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int r = wn * 64 + j * 16 + (lane & 15);
        fw[j] = *reinterpret_cast<const i32x4*>(lW + r * kBK + ((slot ^ (r & 7)) << 4));
      }
#pragma unroll
      for (int i = 0; i < MF; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(fw[j], fa[i], acc[i][j], 0, 0, 0);
    }
    __syncthreads();
    if (more) {
      lstore();
      __syncthreads();
    }
  }

#pragma unroll
  for (int i = 0; i < MF; ++i) {
    const int m = m0 + wm * (16 * MF) + i * 16 + (lane & 15);
    if (m >= M) continue;
    float sam = 0.f;
    if constexpr (kStatic) sam = sa_s;
    else if constexpr (!kRaw) sam = sa[m];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int n = n0 + wn * 64 + j * 16 + 4 * (lane >> 4);
      if (n >= N) continue;                      // N % 64 == 0 and n % 4 == 0: n + 3 < N
      const size_t o = (size_t)m * N + n;
      if constexpr (kRaw) {
        *reinterpret_cast<i32x4*>(reinterpret_cast<int*>(Dv) + o) = acc[i][j];
      } else {
        const f32x4 s = *reinterpret_cast<const f32x4*>(sw + n);
        u16x4 b = {0, 0, 0, 0}, y;
        if (bias) b = *reinterpret_cast<const u16x4*>(bias + n);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          // the reference's operation order, kept out of fma contraction: where the bias
          // cancels the product a fused add would differ by far more than a rounding
          float f = __fmul_rn((float)acc[i][j][r], __fmul_rn(sam, s[r]));
          if (bias) f = __fadd_rn(f, bf2f(b[r]));
          if constexpr (kGelu) f = gelu_erf(f);
          y[r] = f2bf(f);
        }
        if constexpr (kI8)
          *reinterpret_cast<int*>(reinterpret_cast<int8_t*>(Dv) + o) = quant4(y[0], y[1], y[2], y[3], inv_out);
        else
          *reinterpret_cast<u16x4*>(reinterpret_cast<bf16_t*>(Dv) + o) = y;
      }
    }
  }
}

}  // namespace ct

// The tile in use: 2 x 2 waves of 4 x 4 fragments (128 x 128), three blocks per CU (154 VGPRs,
// 32 KiB of LDS each).  On M = 8192 BERT shapes the 256 x 256 tile (2 x 4 waves of 8 x 4
// fragments, one block per CU) was slower at every N <= 3072 and equal at N = 4096, and
// 256 x 128 with four waves slower everywhere (profiles/quant/SUMMARY.md).
namespace {
constexpr int kMF = 4, kWN = 2, kOCC = 3;
constexpr int kBM = 32 * kMF, kBN = 64 * kWN, kThreads = 128 * kWN;
}  // namespace

extern "C" {

// X bf16 [M, K] -> Q int8 [M, K], S fp32 [M].  K % 16 == 0, K <= 8192.
int ct_quant_rows_i8(const void* X, void* Q, float* S, int M, int K, hipStream_t stream) {
  if (M <= 0 || K <= 0 || K % 16 || K > 8192) return 1;
  auto* x = reinterpret_cast<const ct::bf16_t*>(X);
  auto* q = reinterpret_cast<int8_t*>(Q);
  if (K <= 2048)
    ct::quant_rows_i8_kernel<true><<<ct::ceil_div(M, 4), 256, 0, stream>>>(x, q, S, M, K);
  else
    ct::quant_rows_i8_kernel<false><<<M, 256, 0, stream>>>(x, q, S, M, K);
  return 0;
}

// mode 0: bf16 D = A W^T scaled (+ bias); 1: the same through GELU; 2: int32 D = A W^T.
// K % 64 == 0, K <= 8192, N % 64 == 0, M >= 1.
int ct_gemm_i8_nt(const void* A, const void* W, const float* sa, const float* sw, const void* bias, void* D,
                  int M, int N, int K, int mode, hipStream_t stream) {
  if (M <= 0 || N <= 0 || K <= 0 || K % 64 || N % 64 || K > 8192 || mode < 0 || mode > 2) return 1;
  if (mode != 2 && (!sa || !sw)) return 1;
  if ((long)ct::ceil_div(M, kBM) * ct::ceil_div(N, kBN) > 0x7FFFFFFFL) return 1;
  auto* a = reinterpret_cast<const int8_t*>(A);
  auto* w = reinterpret_cast<const int8_t*>(W);
  auto* b = reinterpret_cast<const ct::bf16_t*>(bias);
  const int grid = ct::ceil_div(M, kBM) * ct::ceil_div(N, kBN);
  if (mode == 0)
    ct::gemm_i8_nt_kernel<0, kMF, kWN, kOCC><<<grid, kThreads, 0, stream>>>(a, w, sa, sw, b, D, M, N, K, 0.f,
                                                                           0.f);
  else if (mode == 1)
    ct::gemm_i8_nt_kernel<1, kMF, kWN, kOCC><<<grid, kThreads, 0, stream>>>(a, w, sa, sw, b, D, M, N, K, 0.f,
                                                                           0.f);
  else
    ct::gemm_i8_nt_kernel<2, kMF, kWN, kOCC><<<grid, kThreads, 0, stream>>>(a, w, nullptr, nullptr, nullptr, D, M, N,
                                                                           K, 0.f, 0.f);
  return 0;
}

// X bf16 [n] -> Q int8 [n], q = clamp(rne(x * inv)); n % 16 == 0.
int ct_quant_static_i8(const void* X, void* Q, long n, float inv, hipStream_t stream) {
  if (n <= 0 || n % 16 || n / 16 > 0x7FFFFFFFL || !(inv >= 0.f) || inv > 3.4e38f) return 1;
  const long nch = n / 16;
  ct::quant_static_i8_kernel<<<(unsigned)((nch + 255) / 256), 256, 0, stream>>>(
      reinterpret_cast<const ct::bf16_t*>(X), reinterpret_cast<int8_t*>(Q), inv, nch);
  return 0;
}

// Y bf16 [M, N] = LN(res + (X + bias)) * gamma + beta, and Q int8 [M, N] = quant(Y, inv) unless Q
// is null.  bias, res, beta optional.  N % 8 == 0, N <= 2048.
int ct_layernorm_quant_i8(const void* X, const void* bias, const void* res, const void* gamma, const void* beta,
                          void* Y, void* Q, int M, int N, float eps, float inv, hipStream_t stream) {
  if (M <= 0 || N <= 0 || N % 8 || N > 2048 || !(inv >= 0.f) || inv > 3.4e38f) return 1;
  auto* x = reinterpret_cast<const ct::bf16_t*>(X);
  auto* bi = reinterpret_cast<const ct::bf16_t*>(bias);
  auto* r = reinterpret_cast<const ct::bf16_t*>(res);
  auto* g = reinterpret_cast<const ct::bf16_t*>(gamma);
  auto* be = reinterpret_cast<const ct::bf16_t*>(beta);
  auto* y = reinterpret_cast<ct::bf16_t*>(Y);
  auto* q = reinterpret_cast<int8_t*>(Q);
  const int mv = (N / 8 + 63) / 64;
  int grid = ct::ceil_div(M, 4);
  if (grid > 16384) grid = 16384;
#define CT_LNQ(MV) case MV: \
    if (q) ct::ln_quant_fwd_kernel<MV, true><<<grid, 256, 0, stream>>>(x, bi, r, g, be, y, q, M, N, eps, inv); \
    else ct::ln_quant_fwd_kernel<MV, false><<<grid, 256, 0, stream>>>(x, bi, r, g, be, y, q, M, N, eps, inv); \
    break;
  switch (mv) {
    CT_LNQ(1) CT_LNQ(2) CT_LNQ(3) CT_LNQ(4)
    default: return 1;
  }
#undef CT_LNQ
  return 0;
}

// ct_gemm_i8_nt with one activation scale sa for every row: D = act((A W^T) * (sa * sw[n]) + bias),
// act 0 none / 1 GELU, written as bf16 (out_i8 == 0) or quantized with inv_out to int8.
int ct_gemm_i8_nt_static(const void* A, const void* W, float sa, const float* sw, const void* bias, void* D, int M,
                         int N, int K, int act, int out_i8, float inv_out, hipStream_t stream) {
  if (M <= 0 || N <= 0 || K <= 0 || K % 64 || N % 64 || K > 8192 || act < 0 || act > 1 || !sw) return 1;
  if (!(sa >= 0.f) || sa > 3.4e38f || !(inv_out >= 0.f) || inv_out > 3.4e38f) return 1;
  if ((long)ct::ceil_div(M, kBM) * ct::ceil_div(N, kBN) > 0x7FFFFFFFL) return 1;
  auto* a = reinterpret_cast<const int8_t*>(A);
  auto* w = reinterpret_cast<const int8_t*>(W);
  auto* b = reinterpret_cast<const ct::bf16_t*>(bias);
  const int grid = ct::ceil_div(M, kBM) * ct::ceil_div(N, kBN);
#define CT_GS(MODE) ct::gemm_i8_nt_kernel<MODE, kMF, kWN, kOCC><<<grid, kThreads, 0, stream>>>( \
      a, w, nullptr, sw, b, D, M, N, K, sa, inv_out)
  if (!out_i8) { if (act) CT_GS(4); else CT_GS(3); }
  else { if (act) CT_GS(6); else CT_GS(5); }
#undef CT_GS
  return 0;
}

}  // extern "C"
