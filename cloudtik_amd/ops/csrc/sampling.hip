// Token sampling for graph-replayed decoding on gfx950 (ops/sampling.py states the rule;
// `sample_step_reference` there is the specification this kernel is tested against).
//
// One decode step leaves logits [R, V].  Two launches follow on the caller's stream, neither
// reading anything back to the host:
//
//   sample_step_kernel     one workgroup of 1024 threads per row.  The processed row (repetition
//                          penalty, temperature, NaN -> -inf) is staged once as fp32, in LDS when
//                          V <= kSampCap and in a caller-provided workspace otherwise, and every
//                          later pass reads that copy.  Thresholds come from radix selects over
//                          order-preserving uint32 keys, 8 bits a level: by count for top-k, by
//                          mass for top-p.  With top-k on, the survivors (at most kSampSurv unless
//                          ties say otherwise) are compacted in token order and top-p and the draw
//                          run over them alone.  The draw is a block-wide prefix sum in token order.
//   sample_advance_kernel  one thread: the step counter moves once every row has read it.
//
// Reproducibility: a weight is exp(x - max) in fp32, truncated to a multiple of 2^-sbits and
// held as a 64-bit integer (sbits = 62 - ceil(log2 V), so a row's sum stays below 2^62).  All
// sums of weights are integer sums, which commute: histogram atomics, scans and the draw give
// the same bits in any order.  No floating-point atomic is used.
#include "common.h"
#include <limits.h>
#include <math.h>

namespace ct {

typedef unsigned long long u64;

constexpr int kSampThreads = 1024;
constexpr int kSampWaves = kSampThreads / 64;
constexpr int kSampCap = 32768;        // fp32 row staged in LDS: 128 KiB of the CU's 160 KiB
constexpr int kSampSurv = 1024;        // compacted top-k survivors

struct SampShared {
  u64 hmass[256];
  unsigned hcnt[256];
  float sx[kSampSurv];
  int si[kSampSurv];
  u64 wsum[kSampWaves];
  float wred[kSampWaves];
  u64 b_mass;
  unsigned b_cnt, b_cnt_incl, b_k;
  int b_digit, b_tok;
};

// order-preserving key of a non-NaN float; -0 and +0 share one key
__device__ __forceinline__ uint32_t samp_key(float x) {
  if (x == 0.f) x = 0.f;
  const uint32_t b = __float_as_uint(x);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float samp_unkey(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}
__device__ __forceinline__ u64 samp_weight(float x, float m, double scale) {
  return (u64)((double)expf(x - m) * scale);
}
__device__ __forceinline__ float samp_clean(float v) { return v == v ? v : -INFINITY; }

__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                              uint32_t k1, uint32_t (&o)[4]) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  o[0] = c0; o[1] = c1; o[2] = c2; o[3] = c3;
}

template <typename V>
__device__ __forceinline__ V samp_wave_incl(V v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const V t = __shfl_up(v, o, 64);
    if (lane >= o) v += t;
  }
  return v;
}

// exclusive prefix of `local` over the block in thread order, and the block's total
__device__ __forceinline__ void samp_block_scan(u64 local, u64& excl, u64& total, SampShared& S) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const u64 incl = samp_wave_incl(local, lane);
  __syncthreads();
  if (lane == 63) S.wsum[wid] = incl;
  __syncthreads();
  u64 before = 0, all = 0;
#pragma unroll
  for (int w = 0; w < kSampWaves; ++w) {
    const u64 s = S.wsum[w];
    if (w < wid) before += s;
    all += s;
  }
  excl = before + incl - local;
  total = all;
}

template <bool MAX>
__device__ __forceinline__ float samp_block_minmax(float v, SampShared& S) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float t = __shfl_xor(v, o, 64);
    v = MAX ? fmaxf(v, t) : fminf(v, t);
  }
  __syncthreads();
  if (lane == 0) S.wred[wid] = v;
  __syncthreads();
  float r = S.wred[0];
#pragma unroll
  for (int w = 1; w < kSampWaves; ++w) r = MAX ? fmaxf(r, S.wred[w]) : fminf(r, S.wred[w]);
  return r;
}

template <typename T>
struct SampLoad;
template <>
struct SampLoad<bf16_t> {
  static constexpr int N = 8;
  __device__ static __forceinline__ void load(const bf16_t* p, float (&o)[8]) {
    const u16x8 v = *reinterpret_cast<const u16x8*>(p);
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = bf2f(v[j]);
  }
};
template <>
struct SampLoad<float> {
  static constexpr int N = 4;
  __device__ static __forceinline__ void load(const float* p, float (&o)[4]) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(p);
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = v[j];
  }
};

// LDS: the row is staged in shared memory (V <= kSampCap); else in ws [R, V] fp32
template <typename T, bool LDS>
__global__ __launch_bounds__(kSampThreads) void sample_step_kernel(
    const T* __restrict__ X, float* __restrict__ ws, long* out, uint8_t* done, long* cur, const long* pos,
    const long* seed, const float* __restrict__ u_in, float* __restrict__ u_out, float* __restrict__ thr_out,
    int* __restrict__ keep_out, int V, int Tn, int start_token, int eos, int pad, float temperature, int top_k,
    float top_p, float rp, int sbits) {
  __shared__ float row_lds[LDS ? kSampCap : 1];
  __shared__ SampShared S;
  constexpr int N = SampLoad<T>::N;
  const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const long t = *pos;
  if (t < 0 || t >= Tn) {                      // a replay past the last step changes nothing
    if (tid == 0) { u_out[row] = 0.f; thr_out[row] = 0.f; keep_out[row] = 0; }
    return;
  }
  const T* x = X + (size_t)row * V;
  float* xs = LDS ? row_lds : ws + (size_t)row * V;
  const double scale = (double)(1ull << sbits);

  // ---- stage: x = l / temperature, NaN -> -inf
  {
    const int mis = (int)((reinterpret_cast<uintptr_t>(x) / sizeof(T)) % N);
    const int head = min(V, (N - mis) % N);
    const int nvec = (V - head) / N;
    const int tail0 = head + nvec * N;
    if (tid < head) xs[tid] = samp_clean(__fdiv_rn(to_f<T>(x[tid]), temperature));
    for (int c = tid; c < nvec; c += kSampThreads) {
      float v[N];
      SampLoad<T>::load(x + head + c * N, v);
#pragma unroll
      for (int j = 0; j < N; ++j) xs[head + c * N + j] = samp_clean(__fdiv_rn(v[j], temperature));
    }
    if (tail0 + tid < V) xs[tail0 + tid] = samp_clean(__fdiv_rn(to_f<T>(x[tail0 + tid]), temperature));
  }
  __syncthreads();
  // ---- repetition penalty on the start token and the tokens written so far, from the original
  // value: a token seen twice is written twice with the same bits
  if (rp != 1.f) {
    for (long j = tid; j <= t; j += kSampThreads) {
      const long tok = j == 0 ? (long)start_token : out[(size_t)row * Tn + (j - 1)];
      if (tok >= 0 && tok < V) {
        const float l = to_f<T>(x[tok]);
        const float p = l < 0.f ? l * rp : __fdiv_rn(l, rp);
        xs[tok] = samp_clean(__fdiv_rn(p, temperature));
      }
    }
    __syncthreads();
  }

  // ---- the uniform
  float u;
  if (u_in != nullptr) {
    u = u_in[row];
    u = u >= 0.f ? fminf(u, 0.99999994f) : 0.f;
  } else {
    const u64 sd = (u64)*seed;
    uint32_t r4[4];
    philox4x32_10((uint32_t)row, (uint32_t)t, 0u, 0u, (uint32_t)sd, (uint32_t)(sd >> 32), r4);
    u = (float)(r4[0] >> 8) * 5.9604644775390625e-08f;
  }

  // ---- row maximum
  float m = -INFINITY;
  for (int i = tid; i < V; i += kSampThreads) m = fmaxf(m, xs[i]);
  m = samp_block_minmax<true>(m, S);

  // the working set: n elements, value val(i), token tokof(i), taking part when val >= lo
  bool surv = false;
  int n = V;
  float lo = -INFINITY;
  auto val = [&](int i) -> float { return surv ? S.sx[i] : xs[i]; };
  auto tokof = [&](int i) -> int { return surv ? S.si[i] : i; };

  float thr = m;
  unsigned n_keep = 0;
  int token = 0;
  const bool finite = m > -INFINITY && m < INFINITY;

  if (!finite) {
    // no finite logit (or a +inf): token 0; thr is the maximum
    u64 c = 0, ex, tot;
    for (int i = tid; i < V; i += kSampThreads) c += xs[i] >= m ? 1 : 0;
    samp_block_scan(c, ex, tot, S);
    n_keep = (unsigned)tot;
  } else {
    // one level of a radix select: histogram the digit at `shift` of the keys under `prefix`
    auto histogram = [&](int level, uint32_t prefix, bool mass) {
      const int shift = 24 - 8 * level;
      __syncthreads();
      if (tid < 256) { S.hcnt[tid] = 0; S.hmass[tid] = 0; }
      __syncthreads();
      int cd = -1;
      unsigned cc = 0;
      u64 cm = 0;
      for (int i = tid; i < n; i += kSampThreads) {
        const float v = val(i);
        if (!(v >= lo)) continue;
        const uint32_t key = samp_key(v);
        if (level > 0 && (key >> (shift + 8)) != prefix) continue;
        const int d = (int)((key >> shift) & 255u);
        if (d != cd) {                        // runs of one digit cost one atomic
          if (cc) {
            atomicAdd(&S.hcnt[cd], cc);
            if (mass) atomicAdd(&S.hmass[cd], cm);
          }
          cd = d; cc = 0; cm = 0;
        }
        ++cc;
        if (mass) cm += samp_weight(v, m, scale);
      }
      if (cc) {
        atomicAdd(&S.hcnt[cd], cc);
        if (mass) atomicAdd(&S.hmass[cd], cm);
      }
      __syncthreads();
    };

    // ---- top-k: the k-th largest key by count
    if (top_k > 0 && top_k < V) {
      uint32_t prefix = 0;
      unsigned k = (unsigned)top_k, above_all = 0, n_ge = 0;
      for (int level = 0; level < 4; ++level) {
        histogram(level, prefix, false);
        if (tid < 64) {                       // lane owns bins 255 - 4 * lane - j, j = 0..3, top first
          unsigned c[4], loc = 0;
#pragma unroll
          for (int j = 0; j < 4; ++j) { c[j] = S.hcnt[255 - (4 * lane + j)]; loc += c[j]; }
          unsigned above = samp_wave_incl(loc, lane) - loc;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            if (above < k && k <= above + c[j]) {
              S.b_digit = 255 - (4 * lane + j);
              S.b_k = k - above;
              S.b_cnt = above;
              S.b_cnt_incl = above + c[j];
            }
            above += c[j];
          }
        }
        __syncthreads();
        prefix = (prefix << 8) | (uint32_t)S.b_digit;
        k = S.b_k;
        n_ge = above_all + S.b_cnt_incl;
        above_all += S.b_cnt;
      }
      thr = samp_unkey(prefix);
      n_keep = n_ge;
      lo = thr;
      if (n_ge <= (unsigned)kSampSurv) {
        // compact the survivors in token order
        int chunk = (V + kSampThreads - 1) / kSampThreads;
        chunk |= 1;
        const long b0 = (long)tid * chunk;
        const int i0 = (int)(b0 < V ? b0 : V), i1 = (int)(b0 + chunk < V ? b0 + chunk : V);
        u64 c = 0, ex, tot;
        for (int i = i0; i < i1; ++i) c += xs[i] >= thr ? 1 : 0;
        samp_block_scan(c, ex, tot, S);
        int w = (int)ex;
        for (int i = i0; i < i1; ++i) {
          const float v = xs[i];
          if (v >= thr && w < kSampSurv) { S.sx[w] = v; S.si[w] = i; ++w; }
        }
        __syncthreads();
        surv = true;
        n = (int)n_ge;
        lo = -INFINITY;
      }
    }

    // ---- top-p: the lowest key whose mass above it stays below top_p * Z
    if (top_p < 1.f) {
      uint32_t prefix = 0;
      u64 base = 0, target = 1;
      unsigned above_all = 0, n_ge = 0;
      for (int level = 0; level < 4; ++level) {
        histogram(level, prefix, true);
        if (tid < 64) {
          unsigned c[4], cl = 0;
          u64 ms[4], ml = 0;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            c[j] = S.hcnt[255 - (4 * lane + j)];
            ms[j] = S.hmass[255 - (4 * lane + j)];
            cl += c[j]; ml += ms[j];
          }
          const unsigned ci = samp_wave_incl(cl, lane);
          const u64 mi = samp_wave_incl(ml, lane);
          if (level == 0) {                   // the first wave keeps the target across the levels
            const u64 z = __shfl(mi, 63, 64);
            const double pz = ceil((double)top_p * (double)z);
            target = pz < 1.0 ? 1ull : (u64)pz;
          }
          unsigned ca = ci - cl;
          u64 ma = base + (mi - ml);
          int best = -1;
          unsigned bc = 0, bci = 0;
          u64 bm = 0, bmi = 0;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            if (c[j] > 0 && ma < target) { best = 4 * lane + j; bc = ca; bci = ca + c[j]; bm = ma; bmi = ma + ms[j]; }
            ca += c[j]; ma += ms[j];
          }
          int top = best;
#pragma unroll
          for (int o = 32; o > 0; o >>= 1) top = max(top, __shfl_xor(top, o, 64));
          if (best == top && top >= 0) {
            S.b_digit = 255 - top;
            S.b_mass = bm;
            S.b_cnt = bc;
            S.b_cnt_incl = bci;
          }
        }
        __syncthreads();
        prefix = (prefix << 8) | (uint32_t)S.b_digit;
        base = S.b_mass;
        n_ge = above_all + S.b_cnt_incl;
        above_all += S.b_cnt;
        __syncthreads();
      }
      thr = samp_unkey(prefix);
      n_keep = n_ge;
    } else if (!(top_k > 0 && top_k < V)) {
      float mn = INFINITY;
      for (int i = tid; i < V; i += kSampThreads) mn = fminf(mn, xs[i]);
      thr = samp_block_minmax<false>(mn, S);
      n_keep = (unsigned)V;
    }

    // ---- the draw: lowest kept token, in token order, whose inclusive mass exceeds u * Z
    {
      int chunk = (n + kSampThreads - 1) / kSampThreads;
      chunk |= 1;
      const long b0 = (long)tid * chunk;
      const int i0 = (int)(b0 < n ? b0 : n), i1 = (int)(b0 + chunk < n ? b0 + chunk : n);
      u64 loc = 0, ex, z;
      for (int i = i0; i < i1; ++i) {
        const float v = val(i);
        if (v >= thr) loc += samp_weight(v, m, scale);
      }
      samp_block_scan(loc, ex, z, S);
      u64 want = (u64)floor((double)u * (double)z);
      if (want >= z) want = z - 1;             // z >= 2^sbits: the maximum is kept
      if (tid == 0) S.b_tok = 0;
      __syncthreads();
      if (ex <= want && want < ex + loc) {
        u64 c = ex;
        int found = -1;
        for (int i = i0; i < i1 && found < 0; ++i) {
          const float v = val(i);
          if (v >= thr) {
            c += samp_weight(v, m, scale);
            if (c > want) found = tokof(i);
          }
        }
        S.b_tok = found < 0 ? 0 : found;
      }
      __syncthreads();
      token = S.b_tok;
    }
  }

  // ---- bookkeeping
  if (tid == 0) {
    u_out[row] = u;
    thr_out[row] = thr;
    keep_out[row] = (int)n_keep;
    const bool was_done = done[row] != 0;
    const long tok = was_done ? (long)pad : (long)token;
    out[(size_t)row * Tn + t] = tok;
    cur[row] = tok;
    if (tok == (long)eos) done[row] = 1;
  }
}

__global__ void sample_advance_kernel(long* pos, int Tn) {
  if (threadIdx.x == 0) {
    const long t = *pos;
    if (t >= 0 && t < Tn) *pos = t + 1;
  }
}

}  // namespace ct

extern "C" {

int ct_sample_capacity() { return ct::kSampCap; }

// X [R, V] bf16 (is_bf16) or fp32, contiguous; ws [R, V] fp32 when V > ct_sample_capacity(), else
// unused; out [R, T]; done [R]; cur [R]; pos, seed [1]; u_in [R] or null; diagnostics [R] each
int ct_sample_step(const void* X, int is_bf16, float* ws, long* out, uint8_t* done, long* cur, long* pos,
                   const long* seed, const float* u_in, float* u_out, float* thr_out, int* keep_out, int R, int V,
                   int T, int start_token, int eos, int pad, float temperature, int top_k, float top_p, float rp,
                   hipStream_t stream) {
  if (R <= 0 || V < 1 || V > (1 << 27) || T < 1 || start_token < 0 || start_token >= V || top_k < 0) return 1;
  if (!(temperature > 0.f) || !(rp > 0.f) || !(top_p > 0.f) || top_p > 1.f) return 1;
  const bool lds = V <= ct::kSampCap;
  if (!lds && ws == nullptr) return 1;
  int lg = 0;
  while ((1l << lg) < V) ++lg;
  const int sbits = 62 - lg;
#define CT_SAMPLE(T_, LDS_)                                                                                     \
  hipLaunchKernelGGL((ct::sample_step_kernel<T_, LDS_>), dim3(R), dim3(ct::kSampThreads), 0, stream,            \
                     (const T_*)X, ws, out, done, cur, pos, seed, u_in, u_out, thr_out, keep_out, V, T,        \
                     start_token, eos, pad, temperature, top_k, top_p, rp, sbits)
  if (is_bf16) {
    if (lds) CT_SAMPLE(ct::bf16_t, true); else CT_SAMPLE(ct::bf16_t, false);
  } else {
    if (lds) CT_SAMPLE(float, true); else CT_SAMPLE(float, false);
  }
#undef CT_SAMPLE
  if (hipGetLastError() != hipSuccess) return 2;
  hipLaunchKernelGGL(ct::sample_advance_kernel, dim3(1), dim3(64), 0, stream, pos, T);
  return hipGetLastError() == hipSuccess ? 0 : 2;
}

}  // extern "C"
