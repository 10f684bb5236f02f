// Gated-GELU feed-forward activation of T5 v1.1 / Flan-T5 (bf16, 16-byte vectors per lane):
//   h  = dropout_p(gelu_tanh(g) * u)                      forward, one rounding at the store
//   dg = dh * keep * s * u * gelu_tanh'(g)                backward, one pass over dh, g, u;
//   du = dh * keep * s * gelu_tanh(g)                     s = 1 / (1 - p)
// g and u are rows of F elements at their own row strides (the two halves of a stacked [M, 2F]
// GEMM output go in as they are); h, dh, dg and du are contiguous.  The keep bits are those of
// dropout_kernel over the contiguous output (vector number row * F/8 + column vector), regenerated
// in the backward from (seed, offset): nothing is stored.
//
// gelu_tanh(g) = 0.5 g (1 + tanh(z/2)) = g * sigmoid(z) with z = 2c (g + 0.044715 g^3), c = sqrt(2/pi).
// With e = exp(-|z|) and r = 1 / (1 + e): sigmoid(|z|) = r and 1 - sigmoid(|z|) = e r, and z has the
// sign of g, so one v_exp and one v_rcp per element give the sigmoid and its complement with
// neither overflow nor cancellation in either tail (libm tanhf per element would make the kernel
// VALU-bound).
#include "common.h"

namespace ct {

constexpr float kGeluC2 = 2.f * 0.7978845608028654f;                    // 2 sqrt(2/pi)
constexpr float kGeluA = 0.044715f;
constexpr float kLog2e = 1.4426950408889634f;

// sigmoid(z(g)) in `sig`, 1 - sigmoid(z(g)) in `oms`
__device__ __forceinline__ void gelu_tanh_sigmoid(float g, float& sig, float& oms) {
  const float z = kGeluC2 * g * fmaf(kGeluA * g, g, 1.f);
  const float e = __builtin_amdgcn_exp2f(-kLog2e * fabsf(z));
  const float r = __builtin_amdgcn_rcpf(1.f + e);
  const float er = e * r;
  sig = g >= 0.f ? r : er;
  oms = g >= 0.f ? er : r;
}
__device__ __forceinline__ float gelu_tanh(float g) {
  float sig, oms;
  gelu_tanh_sigmoid(g, sig, oms);
  return g * sig;
}
// gelu_tanh(g) in `y`, its derivative sig (1 + g (1 - sig) z'(g)) in `dy`
__device__ __forceinline__ void gelu_tanh_both(float g, float& y, float& dy) {
  float sig, oms;
  gelu_tanh_sigmoid(g, sig, oms);
  const float dz = kGeluC2 * fmaf(3.f * kGeluA * g, g, 1.f);
  y = g * sig;
  dy = sig * fmaf(g * oms, dz, 1.f);
}

// 2-D mapping of bias_act_fwd_kernel: blockIdx.x / lane pick a column vector, the 4 waves of the
// block and blockIdx.y stride over rows, ROWS rows per step, so 2 * ROWS independent 16-byte loads
// are in flight per lane.  gs / us: row strides of g / u in vectors.
constexpr int kGgFwdRows = 4;
constexpr int kGgBwdRows = 2;

template <bool DROP>
__global__ __launch_bounds__(256) void gated_gelu_fwd_kernel(const bf16_t* __restrict__ g,
                                                             const bf16_t* __restrict__ u,
                                                             bf16_t* __restrict__ h, long M, int nvec_row,
                                                             long gs, long us, uint32_t thresh, float scale,
                                                             uint64_t seed, uint64_t offset) {
  constexpr int R = kGgFwdRows;
  const int c = blockIdx.x * 64 + (threadIdx.x & 63);
  if (c >= nvec_row) return;
  const long rstride = (long)gridDim.y * 4 * R;
  const u16x8* gr = reinterpret_cast<const u16x8*>(g);
  const u16x8* ur = reinterpret_cast<const u16x8*>(u);
  u16x8* hr = reinterpret_cast<u16x8*>(h);
  for (long r0 = ((long)blockIdx.y * 4 + (threadIdx.x >> 6)) * R; r0 < M; r0 += rstride) {
    u16x8 gv[R], uv[R];
#pragma unroll
    for (int k = 0; k < R; ++k) {
      const bool in = r0 + k < M;
      gv[k] = in ? gr[(r0 + k) * gs + c] : u16x8(0);
      uv[k] = in ? ur[(r0 + k) * us + c] : u16x8(0);
    }
#pragma unroll
    for (int k = 0; k < R; ++k) {
      if (r0 + k >= M) break;
      const long v = (r0 + k) * nvec_row + c;
      uint32_t keep = 0xFFu;
      if (DROP) keep = dropout_bits8(seed, offset, (uint64_t)v, thresh);
      u16x8 o;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float y = gelu_tanh(bf2f(gv[k][j])) * bf2f(uv[k][j]);
        o[j] = DROP ? (((keep >> j) & 1u) ? f2bf(y * scale) : (bf16_t)0) : f2bf(y);
      }
      hr[v] = o;
    }
  }
}

template <bool DROP>
__global__ __launch_bounds__(256) void gated_gelu_bwd_kernel(const bf16_t* __restrict__ dh,
                                                             const bf16_t* __restrict__ g,
                                                             const bf16_t* __restrict__ u,
                                                             bf16_t* __restrict__ dg, bf16_t* __restrict__ du,
                                                             long M, int nvec_row, long gs, long us,
                                                             uint32_t thresh, float scale, uint64_t seed,
                                                             uint64_t offset) {
  constexpr int R = kGgBwdRows;
  const int c = blockIdx.x * 64 + (threadIdx.x & 63);
  if (c >= nvec_row) return;
  const long rstride = (long)gridDim.y * 4 * R;
  const u16x8* dr = reinterpret_cast<const u16x8*>(dh);
  const u16x8* gr = reinterpret_cast<const u16x8*>(g);
  const u16x8* ur = reinterpret_cast<const u16x8*>(u);
  for (long r0 = ((long)blockIdx.y * 4 + (threadIdx.x >> 6)) * R; r0 < M; r0 += rstride) {
    u16x8 dv[R], gv[R], uv[R];
#pragma unroll
    for (int k = 0; k < R; ++k) {
      const bool in = r0 + k < M;
      dv[k] = in ? dr[(r0 + k) * nvec_row + c] : u16x8(0);
      gv[k] = in ? gr[(r0 + k) * gs + c] : u16x8(0);
      uv[k] = in ? ur[(r0 + k) * us + c] : u16x8(0);
    }
#pragma unroll
    for (int k = 0; k < R; ++k) {
      if (r0 + k >= M) break;
      const long v = (r0 + k) * nvec_row + c;
      uint32_t keep = 0xFFu;
      if (DROP) keep = dropout_bits8(seed, offset, (uint64_t)v, thresh);
      u16x8 og, ou;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float y, dy;
        gelu_tanh_both(bf2f(gv[k][j]), y, dy);
        float d = bf2f(dv[k][j]);
        if (DROP) d = ((keep >> j) & 1u) ? d * scale : 0.f;
        og[j] = f2bf(d * bf2f(uv[k][j]) * dy);
        ou[j] = f2bf(d * y);
      }
      reinterpret_cast<u16x8*>(dg)[v] = og;
      reinterpret_cast<u16x8*>(du)[v] = ou;
    }
  }
}

// column blocks x row blocks, about 2048 workgroups at the most (8 waves per SIMD over 256 CUs);
// the rows beyond are covered by the grid-stride loop
static inline dim3 gated_gelu_grid(long M, int nvec, int rows_per_wave) {
  const int gx = (nvec + 63) / 64;
  long gy = (M + 4 * rows_per_wave - 1) / (4 * rows_per_wave);
  const long want = (2048 + gx - 1) / gx;
  if (gy > want) gy = want;
  if (gy < 1) gy = 1;
  return dim3((unsigned)gx, (unsigned)gy);
}

// rows of F elements, F % 8 == 0, 16-byte-aligned bases, row strides (elements) multiples of 8
static inline bool gated_gelu_args_ok(long M, int F, long gs, long us, const void* a, const void* b,
                                      const void* c, const void* d, const void* e) {
  if (M < 0 || F <= 0 || F % 8 || gs % 8 || us % 8 || gs < F || us < F) return false;
  const uintptr_t bits = (uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d | (uintptr_t)e;
  return (bits & 15) == 0;
}

}  // namespace ct

using namespace ct;

extern "C" int ct_gated_gelu_fwd(const void* g, const void* u, void* h, long M, int F, long g_stride,
                                 long u_stride, float p, uint64_t seed, uint64_t offset, hipStream_t stream) {
  if (!gated_gelu_args_ok(M, F, g_stride, u_stride, g, u, h, nullptr, nullptr) || !(p >= 0.f && p < 1.f)) return -1;
  if (M == 0) return 0;
  const int nvec = F / 8;
  const dim3 grid = gated_gelu_grid(M, nvec, kGgFwdRows);
  if (p > 0.f)
    gated_gelu_fwd_kernel<true><<<grid, 256, 0, stream>>>((const bf16_t*)g, (const bf16_t*)u, (bf16_t*)h, M, nvec,
                                                          g_stride / 8, u_stride / 8, dropout_threshold(p),
                                                          1.f / (1.f - p), seed, offset);
  else
    gated_gelu_fwd_kernel<false><<<grid, 256, 0, stream>>>((const bf16_t*)g, (const bf16_t*)u, (bf16_t*)h, M, nvec,
                                                           g_stride / 8, u_stride / 8, 0u, 1.f, 0, 0);
  return 0;
}

extern "C" int ct_gated_gelu_bwd(const void* dh, const void* g, const void* u, void* dg, void* du, long M,
                                 int F, long g_stride, long u_stride, float p, uint64_t seed, uint64_t offset,
                                 hipStream_t stream) {
  if (!gated_gelu_args_ok(M, F, g_stride, u_stride, dh, g, u, dg, du) || !(p >= 0.f && p < 1.f)) return -1;
  if (M == 0) return 0;
  const int nvec = F / 8;
  const dim3 grid = gated_gelu_grid(M, nvec, kGgBwdRows);
  if (p > 0.f)
    gated_gelu_bwd_kernel<true><<<grid, 256, 0, stream>>>((const bf16_t*)dh, (const bf16_t*)g, (const bf16_t*)u,
                                                          (bf16_t*)dg, (bf16_t*)du, M, nvec, g_stride / 8,
                                                          u_stride / 8, dropout_threshold(p), 1.f / (1.f - p),
                                                          seed, offset);
  else
    gated_gelu_bwd_kernel<false><<<grid, 256, 0, stream>>>((const bf16_t*)dh, (const bf16_t*)g, (const bf16_t*)u,
                                                           (bf16_t*)dg, (bf16_t*)du, M, nvec, g_stride / 8,
                                                           u_stride / 8, 0u, 1.f, 0, 0);
  return 0;
}
