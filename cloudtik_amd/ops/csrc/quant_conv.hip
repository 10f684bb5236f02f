// Int8 forward convolution for gfx950 as an implicit GEMM on v_mfma_i32_16x16x64_i8: the tile,
// the 128-byte K step, the swizzled LDS image and the fragment convention of gemm_i8_nt_kernel
// (quant.hip), with the activation operand gathered from an NHWC (channels_last) int8 image
// instead of read from a matrix.  Inference only; BatchNorm is folded into the weights and the
// fp32 bias offline, so the epilogue is the whole rest of a ResNet layer: dequantize, bias,
// int8 residual, ReLU, and the cast to the next layer's int8 range.
//
// GEMM view: M = N Ho Wo output pixels, N = Co, K = R S Ci with tap-major weight rows
// ([Co][R][S][Ci], what conv.weight_rows gives).  A 16-byte chunk of the activation tile is 16
// channels of one tap of one pixel; Ci % 64 == 0 keeps a chunk inside one tap and K a multiple
// of 64.  A K tile (128 bytes) may straddle two taps (Ci = 64: every second one does), so tap and
// channel are tracked per chunk; the slot of a thread's chunks (tid & 7) is the same for all of
// them, so ONE (tap, channel) pair per thread advances with the K tile.  A row's (n, ho, wo) does
// not change with K: it is decoded once, before the loop.
//
// A chunk outside the image (padding), in a tail row or past K reads a clamped, valid address
// and is zeroed -- the GEMM's rule -- so no load is predicated.
//
// Epilogue, in this order and with every operation kept out of fma contraction, so that
// reference.conv_i8_static is bit-equal:
//   f = fmul(float(acc), fmul(a_scale, w_scale[n]));  f = fadd(f, bias[n]);
//   if res:  f = fadd(f, fmul(float(res[m, n]), res_scale));   if relu: f = max(f, 0);
//   y = bf16(f);  out = y (bf16)  or  quant4(y, inv_out) (int8, from the ROUNDED bf16).
#include "common.h"

// The compiler's default is -ffp-contract=fast, and the __fmul_rn / __fadd_rn of this toolchain's
// headers are plain * and + compiled under that default, so they fuse into v_fma_f32 once inlined.
// The epilogue below is therefore written with * and + under this pragma, which is what keeps its
// multiplies and adds separate roundings (no v_fma in this file's code object).
#pragma clang fp contract(off)

namespace ct {

typedef __attribute__((ext_vector_type(4))) int i32x4;

namespace {

constexpr int kBK = 128;

struct ConvGeo {
  int H, W, Ci, Ho, Wo, Co, R, stride, pad, M, K;
};

__device__ __forceinline__ int cq1(bf16_t e, float inv) {
  const float r = rintf(bf2f(e) * inv);
  return (int)fminf(fmaxf(r, -127.f), 127.f);
}
__device__ __forceinline__ int cq4(const u16x4& y, float inv) {
  return (cq1(y[0], inv) & 0xFF) | ((cq1(y[1], inv) & 0xFF) << 8) | ((cq1(y[2], inv) & 0xFF) << 16) |
         ((cq1(y[3], inv) & 0xFF) << 24);
}

}  // namespace

// 2 x WN waves of MF x 4 fragments: a (32 MF) x (64 WN) tile of [pixels] x [channels].
template <bool I8OUT, int MF, int WN, int OCC>
__global__ __launch_bounds__(128 * WN, OCC) void conv_i8_fwd_kernel(
    const int8_t* __restrict__ X, const int8_t* __restrict__ Wq, const float* __restrict__ sw,
    const float* __restrict__ bias, const int8_t* __restrict__ res, void* __restrict__ Yv, ConvGeo g, float a_scale,
    float res_scale, float inv_out, int relu) {
  constexpr int T = 128 * WN, BM = 32 * MF, BN = 64 * WN;
  constexpr int CA = BM * 8 / T, CW = BN * 8 / T;       // 16-byte chunks per thread and K tile
  __shared__ __attribute__((aligned(16))) int8_t lds[(BM + BN) * kBK];
  int8_t* lA = lds;
  int8_t* lW = lds + BM * kBK;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wm = wid / WN, wn = wid % WN;
  const int M = g.M, N = g.Co, K = g.K;
  const int tiles_n = (N + BN - 1) / BN;
  const int L = xcd_remap(blockIdx.x, gridDim.x);
  const int m0 = (L / tiles_n) * BM, n0 = (L % tiles_n) * BN;

  // this thread's CA pixels: image base (in pixels) and the input coordinate of tap (0, 0)
  int pbase[CA], hi0[CA], wi0[CA];
  bool live[CA];
#pragma unroll
  for (int i = 0; i < CA; ++i) {
    const int gm = m0 + ((tid + T * i) >> 3);
    const int m = min(gm, M - 1);
    const int n = m / (g.Ho * g.Wo), rem = m - n * (g.Ho * g.Wo);
    const int ho = rem / g.Wo, wo = rem - ho * g.Wo;
    pbase[i] = n * g.H * g.W;
    hi0[i] = ho * g.stride - g.pad;
    wi0[i] = wo * g.stride - g.pad;
    live[i] = gm < M;
  }
  // (tap, channel) of this thread's slot in the K tile being fetched; advances by 128 per tile
  const int slot = tid & 7;
  int tap = (slot * 16) / g.Ci, ch = (slot * 16) % g.Ci;

  i32x4 ra[CA], rw[CW];
  auto gload = [&](int k0) {
    const int k = k0 + slot * 16;
    const bool kin = k < K;
    const int t = kin ? tap : g.R * g.R - 1, c = kin ? ch : g.Ci - 16;   // the clamped chunk is K - 16
    const int r = g.R == 3 ? t / 3 : 0, s = t - 3 * r;                   // R == 1: t == 0
#pragma unroll
    for (int i = 0; i < CA; ++i) {
      const int hi = hi0[i] + r, wi = wi0[i] + s;
      const bool in = kin && live[i] && hi >= 0 && hi < g.H && wi >= 0 && wi < g.W;
      const int hc = min(max(hi, 0), g.H - 1), wc = min(max(wi, 0), g.W - 1);
      const i32x4 v = *reinterpret_cast<const i32x4*>(X + ((size_t)(pbase[i] + hc * g.W + wc) * g.Ci + c));
      ra[i] = in ? v : (i32x4)(0);
    }
#pragma unroll
    for (int i = 0; i < CW; ++i) {
      const int gn = n0 + ((tid + T * i) >> 3);
      const i32x4 v = *reinterpret_cast<const i32x4*>(Wq + (size_t)min(gn, N - 1) * K + min(k, K - 16));
      rw[i] = (gn < N && kin) ? v : (i32x4)(0);
    }
    ch += kBK;
    while (ch >= g.Ci) { ch -= g.Ci; ++tap; }            // Ci >= 64: at most two steps
  };
  auto lstore = [&]() {
#pragma unroll
    for (int i = 0; i < CA; ++i) {
      const int row = (tid + T * i) >> 3;
      *reinterpret_cast<i32x4*>(lA + row * kBK + ((slot ^ (row & 7)) << 4)) = ra[i];
    }
#pragma unroll
    for (int i = 0; i < CW; ++i) {
      const int row = (tid + T * i) >> 3;
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
      const int fs = ks * 4 + (lane >> 4);
      i32x4 fa[MF], fw[4];
#pragma unroll
      for (int i = 0; i < MF; ++i) {
        const int r = wm * (16 * MF) + i * 16 + (lane & 15);
        fa[i] = *reinterpret_cast<const i32x4*>(lA + r * kBK + ((fs ^ (r & 7)) << 4));
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int r = wn * 64 + j * 16 + (lane & 15);
        fw[j] = *reinterpret_cast<const i32x4*>(lW + r * kBK + ((fs ^ (r & 7)) << 4));
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

  // W is the MFMA's A operand: a lane holds four consecutive channels n of one pixel m.  A bf16
  // result goes out as the lane's 8-byte vector.  An int8 one would be 4 bytes per lane (a store
  // instruction covering 16 pixels x 16 bytes), so the int8 tile is staged through LDS -- free
  // after the K loop's last barrier, in the operands' swizzle -- and written as 16-byte chunks,
  // eight consecutive threads covering the 128 contiguous bytes of a pixel's channels.
#pragma unroll
  for (int i = 0; i < MF; ++i) {
    const int ml = wm * (16 * MF) + i * 16 + (lane & 15), m = m0 + ml;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int nl = wn * 64 + j * 16 + 4 * (lane >> 4), n = n0 + nl;
      const bool in = m < M && n < N;              // Co % 64 == 0 and n % 4 == 0: n + 3 < Co
      const size_t o = (size_t)m * N + n;          // channels_last: pixel-major, channel-minor
      u16x4 y = {0, 0, 0, 0};
      if (in) {
        const f32x4 s = *reinterpret_cast<const f32x4*>(sw + n);
        const f32x4 b = *reinterpret_cast<const f32x4*>(bias + n);
        int rq = 0;
        if (res) rq = *reinterpret_cast<const int*>(res + o);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          // plain * and + under contract(off): one rounding each
          float f = (float)acc[i][j][r] * (a_scale * s[r]);
          f = f + b[r];
          if (res) f = f + (float)(int8_t)(rq >> (8 * r)) * res_scale;
          if (relu) f = fmaxf(f, 0.f);
          y[r] = f2bf(f);
        }
      }
      if constexpr (I8OUT)
        *reinterpret_cast<int*>(lds + ml * BN + (((nl >> 4) ^ (ml & 7)) << 4) + (nl & 15)) = cq4(y, inv_out);
      else if (in)
        *reinterpret_cast<u16x4*>(reinterpret_cast<bf16_t*>(Yv) + o) = y;
    }
  }
  if constexpr (I8OUT) {
    static_assert(BN % 128 == 0 && BM * BN <= (BM + BN) * kBK, "the int8 tile must fit the operands' LDS");
    __syncthreads();
    constexpr int CPR = BN / 16;                   // 16-byte chunks per tile row
    for (int c = tid; c < BM * CPR; c += T) {
      const int row = c / CPR, ch = c % CPR, m = m0 + row, n = n0 + ch * 16;
      if (m < M && n < N)                          // n % 16 == 0 and Co % 64 == 0: n + 15 < Co
        *reinterpret_cast<i32x4*>(reinterpret_cast<int8_t*>(Yv) + (size_t)m * N + n) =
            *reinterpret_cast<const i32x4*>(lds + row * BN + ((ch ^ (row & 7)) << 4));
    }
  }
}

}  // namespace ct

// The GEMM's tile for every shape: 2 x 2 waves of 4 x 4 fragments (128 x 128), three blocks per CU
// (160 VGPRs, 32 KiB of LDS each).  At Co = 64 half of it is idle, but the 128 x 64 tile (WN = 1,
// eight activation chunks per thread: 168 VGPRs and 23 spilled) was not faster on the ResNet-50
// layer-1 shapes at batch 64: 23.2 against 23.2 us (64 -> 64, 1x1), 39.5 against 27.7 us
// (256 -> 64, 1x1), 55.5 against 39.5 us (64 -> 64, 3x3), both with direct stores;
// profiles/quant_conv/SUMMARY.md.
namespace {
constexpr int kMF = 4, kWN = 2, kOCC = 3;
constexpr int kBM = 32 * kMF, kBN = 64 * kWN, kThreads = 128 * kWN;
bool factor_ok(float v) { return v >= 0.f && v <= 3.4e38f; }       // finite, non-negative (NaN fails)
}  // namespace

extern "C" {

// Y[N, Co, Ho, Wo] (channels_last; bf16, or int8 quantized with inv_out) =
//   act(conv(X int8 [N, Ci, H, W] channels_last, Wq int8 [Co, R*R*Ci]) * (a_scale * sw[co]) + bias[co]
//       + res * res_scale).
// Ci % 64 == 0, Co % 64 == 0, R in {1, 3}, stride in {1, 2}, pad == R / 2, R*R*Ci <= 32768.
// Returns 1 for anything else.
int ct_conv_i8_fwd(const void* X, const void* Wq, const float* sw, const float* bias, const void* res, void* Y, int N,
                   int H, int W, int Ci, int Co, int R, int stride, int pad, float a_scale, float res_scale,
                   float inv_out, int relu, int out_i8, hipStream_t stream) {
  if (N <= 0 || H <= 0 || W <= 0 || Ci <= 0 || Co <= 0 || Ci % 64 || Co % 64 || !X || !Wq || !sw || !bias || !Y)
    return 1;
  if ((R != 1 && R != 3) || (stride != 1 && stride != 2) || pad != R / 2) return 1;
  if ((long)R * R * Ci > 32768) return 1;
  if (!factor_ok(a_scale) || !factor_ok(res_scale) || !factor_ok(inv_out)) return 1;
  const int Ho = (H + 2 * pad - R) / stride + 1, Wo = (W + 2 * pad - R) / stride + 1;
  if (Ho <= 0 || Wo <= 0) return 1;
  const long M = (long)N * Ho * Wo;
  if (M > 65535L * 128 || (long)N * H * W > 0x7FFFFFFFL) return 1;
  if ((long)ct::ceil_div(M, kBM) * ct::ceil_div(Co, kBN) > 0x7FFFFFFFL) return 1;
  const ct::ConvGeo g{H, W, Ci, Ho, Wo, Co, R, stride, pad, (int)M, R * R * Ci};
  const int grid = ct::ceil_div(M, kBM) * ct::ceil_div(Co, kBN);
  auto* x = reinterpret_cast<const int8_t*>(X);
  auto* w = reinterpret_cast<const int8_t*>(Wq);
  auto* r = reinterpret_cast<const int8_t*>(res);
  if (out_i8)
    ct::conv_i8_fwd_kernel<true, kMF, kWN, kOCC><<<grid, kThreads, 0, stream>>>(x, w, sw, bias, r, Y, g, a_scale,
                                                                                res_scale, inv_out, relu);
  else
    ct::conv_i8_fwd_kernel<false, kMF, kWN, kOCC><<<grid, kThreads, 0, stream>>>(x, w, sw, bias, r, Y, g, a_scale,
                                                                                 res_scale, inv_out, relu);
  return 0;
}

}  // extern "C"
