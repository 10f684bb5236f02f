// Int8 post-training quantization kernels for gfx950: dynamic per-row symmetric quantization
// of a bf16 activation matrix, and the int8 x int8 -> int32 NT GEMM on the i8 matrix cores
// with a fp32 dequantize (+ bias, + GELU) epilogue.  Inference only.
//
// Number format: symmetric, no zero point.  A row's scale is amax / 127 (fp32, IEEE divide);
// elements are q = clamp(rne(x * (127 / amax)), -127, 127) with ONE fp32 multiply (nothing to
// contract into an fma) and round-half-to-even, so a host implementation of the same formula
// is bit-equal.  An all-zero row has scale 0 and q 0.
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
// MODE 2: the raw int32 accumulators.
constexpr int kBK = 128;

template <int MODE, int MF, int WN, int OCC>
__global__ __launch_bounds__(128 * WN, OCC) void gemm_i8_nt_kernel(const int8_t* __restrict__ A, const int8_t* __restrict__ W,
                                                         const float* __restrict__ sa, const float* __restrict__ sw,
                                                         const bf16_t* __restrict__ bias, void* __restrict__ Dv,
                                                         int M, int N, int K) {
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
    if constexpr (MODE != 2) sam = sa[m];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int n = n0 + wn * 64 + j * 16 + 4 * (lane >> 4);
      if (n >= N) continue;                      // N % 64 == 0 and n % 4 == 0: n + 3 < N
      const size_t o = (size_t)m * N + n;
      if constexpr (MODE == 2) {
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
          if constexpr (MODE == 1) f = gelu_erf(f);
          y[r] = f2bf(f);
        }
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
    ct::gemm_i8_nt_kernel<0, kMF, kWN, kOCC><<<grid, kThreads, 0, stream>>>(a, w, sa, sw, b, D, M, N, K);
  else if (mode == 1)
    ct::gemm_i8_nt_kernel<1, kMF, kWN, kOCC><<<grid, kThreads, 0, stream>>>(a, w, sa, sw, b, D, M, N, K);
  else
    ct::gemm_i8_nt_kernel<2, kMF, kWN, kOCC><<<grid, kThreads, 0, stream>>>(a, w, nullptr, nullptr, nullptr, D, M, N,
                                                                           K);
  return 0;
}

}  // extern "C"
