// Beam-search bookkeeping for graph-replayed decoding on gfx950 (ops/beam.py states the rules;
// `beam_step_reference` there is the specification these kernels are tested against).
//
// One decode step at batch B * K leaves logits [B * K, V].  Three launches follow, all on the
// caller's stream, none of them reading anything back to the host:
//
//   beam_topk_kernel      one workgroup per row: one pass over the row with 16-byte loads, an
//                         online max / sum-exp, and a private top-2K per thread; the row's top-2K
//                         comes out of 2K block-wide arg-max rounds (wave shuffles, then LDS
//                         across the four waves).  Writes log-sum-exp and 2K (logit, token).
//   beam_update_kernel    one wave per batch item: ranks the K * 2K candidates (the item's top
//                         2K over K * V is contained in them), then applies the stop, running-set,
//                         finished-set and early-stop rules and rewrites the state in place.
//                         The last workgroup to arrive advances the step counter.
//   cache_reorder_kernel  gathers every self-attention cache row by beam_idx from the ping to
//                         the pong buffers, all layers in one launch through a pointer table,
//                         copying only the slots written so far.
//
// Order is total everywhere: a candidate beats another when its score is larger, or equal with
// the lower flat index k * V + token.  A NaN logit ranks as -inf.
#include "common.h"
#include <limits.h>
#include <math.h>

namespace ct {

constexpr float kBeamNeg = -1.0e9f;
constexpr int kBeamMaxK = 8;

__device__ __forceinline__ bool beats(float a, int ai, float b, int bi) { return a > b || (a == b && ai < bi); }

template <typename T>
struct BeamLoad;
template <>
struct BeamLoad<bf16_t> {
  static constexpr int N = 8;
  __device__ static __forceinline__ void load(const bf16_t* p, float (&o)[8]) {
    const u16x8 v = *reinterpret_cast<const u16x8*>(p);
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = bf2f(v[j]);
  }
};
template <>
struct BeamLoad<float> {
  static constexpr int N = 4;
  __device__ static __forceinline__ void load(const float* p, float (&o)[4]) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(p);
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = v[j];
  }
};

// ------------------------------------------------------------------------------- row top-2K
// KK: the private list length, 2K rounded up to a power of two; k2 = 2K entries are written.
template <typename T, int KK>
__global__ __launch_bounds__(256) void beam_topk_kernel(const T* __restrict__ X, float* __restrict__ lse,
                                                        float* __restrict__ top_val, int* __restrict__ top_tok,
                                                        int V, int k2) {
  constexpr int N = BeamLoad<T>::N;
  __shared__ float red_m[4], red_s[4];
  __shared__ float win_v[2][4];
  __shared__ int win_i[2][4], win_t[2][4];
  const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const T* x = X + (size_t)row * V;

  float tv[KK];
  int ti[KK];
#pragma unroll
  for (int j = 0; j < KK; ++j) { tv[j] = -INFINITY; ti[j] = INT_MAX; }
  float m = -INFINITY, s = 0.f;

  auto rank = [&](float v, int idx) {
    if (beats(v, idx, tv[KK - 1], ti[KK - 1])) {
      tv[KK - 1] = v; ti[KK - 1] = idx;
#pragma unroll
      for (int j = KK - 1; j > 0; --j) {
        if (beats(tv[j], ti[j], tv[j - 1], ti[j - 1])) {
          const float fv = tv[j]; tv[j] = tv[j - 1]; tv[j - 1] = fv;
          const int fi = ti[j]; ti[j] = ti[j - 1]; ti[j - 1] = fi;
        }
      }
    }
  };
  auto one = [&](float v, int idx) {
    if (!(v == v)) v = -INFINITY;
    const float nm = fmaxf(m, v);
    if (nm > -INFINITY) { s = s * expf(m - nm) + expf(v - nm); m = nm; }
    rank(v, idx);
  };

  // scalar head up to the first 16-byte boundary of this row, vector body, scalar tail
  const int mis = (int)((reinterpret_cast<uintptr_t>(x) / sizeof(T)) % N);
  const int head = min(V, (N - mis) % N);
  const int nvec = (V - head) / N;
  const int tail0 = head + nvec * N;
  if (tid < head) one(to_f<T>(x[tid]), tid);
  for (int c = tid; c < nvec; c += 256) {
    float v[N];
    BeamLoad<T>::load(x + head + c * N, v);
    float cm = -INFINITY;
#pragma unroll
    for (int j = 0; j < N; ++j) {
      if (!(v[j] == v[j])) v[j] = -INFINITY;
      cm = fmaxf(cm, v[j]);
    }
    const float nm = fmaxf(m, cm);
    if (nm > -INFINITY) {
      float add = 0.f;
#pragma unroll
      for (int j = 0; j < N; ++j) add += expf(v[j] - nm);
      s = s * expf(m - nm) + add;
      m = nm;
    }
#pragma unroll
    for (int j = 0; j < N; ++j) rank(v[j], head + c * N + j);
  }
  if (tail0 + tid < V) one(to_f<T>(x[tail0 + tid]), tail0 + tid);      // fewer than N <= 8 elements

  // log-sum-exp of the row
  {
    float bm = wave_max(m);
    float bs = wave_sum(bm > -INFINITY ? s * expf(m - bm) : 0.f);
    if (lane == 0) { red_m[wid] = bm; red_s[wid] = bs; }
    __syncthreads();
    if (tid == 0) {
      const float gm = fmaxf(fmaxf(red_m[0], red_m[1]), fmaxf(red_m[2], red_m[3]));
      float gs = 0.f;
      for (int w = 0; w < 4; ++w) gs += red_m[w] > -INFINITY ? red_s[w] * expf(red_m[w] - gm) : 0.f;
      lse[row] = gm + logf(gs);
    }
  }

  // 2K rounds: every thread offers the head of its list, the block picks the best, its owner pops
  for (int r = 0; r < k2; ++r) {
    float bv = tv[0];
    int bi = ti[0], bt = tid;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(bv, o, 64);
      const int oi = __shfl_xor(bi, o, 64), ot = __shfl_xor(bt, o, 64);
      if (beats(ov, oi, bv, bi) || (ov == bv && oi == bi && ot < bt)) { bv = ov; bi = oi; bt = ot; }
    }
    const int buf = r & 1;             // two buffers: one barrier per round is enough
    if (lane == 0) { win_v[buf][wid] = bv; win_i[buf][wid] = bi; win_t[buf][wid] = bt; }
    __syncthreads();
    bv = win_v[buf][0]; bi = win_i[buf][0]; bt = win_t[buf][0];
#pragma unroll
    for (int w = 1; w < 4; ++w) {
      const float ov = win_v[buf][w];
      const int oi = win_i[buf][w], ot = win_t[buf][w];
      if (beats(ov, oi, bv, bi) || (ov == bv && oi == bi && ot < bt)) { bv = ov; bi = oi; bt = ot; }
    }
    if (tid == 0) {
      top_val[(size_t)row * k2 + r] = bv;
      top_tok[(size_t)row * k2 + r] = min(bi, V - 1);       // V >= 2K: never the empty-slot mark
    }
    if (tid == bt) {
#pragma unroll
      for (int j = 0; j < KK - 1; ++j) { tv[j] = tv[j + 1]; ti[j] = ti[j + 1]; }
      tv[KK - 1] = -INFINITY; ti[KK - 1] = INT_MAX;
    }
  }
}

// ------------------------------------------------------------------------------ state update
// State of batch item b (ops/beam.py): run_seq / fin_seq [K, T] int64, run_score / fin_score
// [K] fp32, fin_flag [K] and unsat as bytes.  64 threads; K <= 8, so at most 128 candidates.
__global__ __launch_bounds__(64) void beam_update_kernel(
    const float* __restrict__ lse, const float* __restrict__ top_val, const int* __restrict__ top_tok,
    long* run_seq, float* run_score, long* fin_seq, float* fin_score, uint8_t* fin_flag, uint8_t* unsat,
    const float* __restrict__ len_pen, long* pos, unsigned* arrive, long* __restrict__ beam_idx,
    long* __restrict__ cur, float* __restrict__ cand_score, long* __restrict__ cand_idx,
    int K, int V, int T, int eos, int early) {
  __shared__ float c_s[kBeamMaxK * 2 * kBeamMaxK];
  __shared__ int c_id[kBeamMaxK * 2 * kBeamMaxK];
  __shared__ float top_s[2 * kBeamMaxK];
  __shared__ int top_id[2 * kBeamMaxK];
  __shared__ float m_s[2 * kBeamMaxK];
  __shared__ int run_r[kBeamMaxK], fin_src[kBeamMaxK];
  __shared__ float run_new[kBeamMaxK], fin_new[kBeamMaxK];
  __shared__ uint8_t flag_new[kBeamMaxK];

  const int b = blockIdx.x, lane = threadIdx.x;
  const int k2 = 2 * K, n = K * k2;
  const long t = *pos;
  const bool valid = t >= 0 && t < T;            // a replay past the last step changes nothing
  if (valid) {
    const bool last = t == T - 1;
    for (int i = lane; i < n; i += 64) {
      const int k = i / k2, row = b * K + k;
      float sc = (top_val[(size_t)row * k2 + (i - k * k2)] - lse[row]) + run_score[row];
      if (!(sc == sc)) sc = -INFINITY;
      const int tok = min(max(top_tok[(size_t)row * k2 + (i - k * k2)], 0), V - 1);
      c_s[i] = sc;
      c_id[i] = k * V + tok;
    }
    __syncthreads();
    for (int i = lane; i < n; i += 64) {
      const float sc = c_s[i];
      const int id = c_id[i];
      int rank = 0;
      for (int j = 0; j < n; ++j) rank += beats(c_s[j], c_id[j], sc, id) ? 1 : 0;
      if (rank < k2) { top_s[rank] = sc; top_id[rank] = id; }
    }
    __syncthreads();
    const float L = len_pen[t];
    bool full = early != 0;
    for (int k = 0; k < K; ++k) full = full && fin_flag[b * K + k] != 0;
    const bool open = unsat[b] != 0;
    if (lane < k2) {
      cand_score[b * k2 + lane] = top_s[lane];
      cand_idx[b * k2 + lane] = top_id[lane];
    }
    // rule 3: running slot `lane` takes the lane-th candidate that does not stop, in rank order;
    // when fewer than K go on (the last step) the stopped ones follow, marked with -1e9
    if (lane < K) {
      int sel = -1, seen = 0;
      for (int r = 0; r < k2; ++r) {
        const bool stop = last || (top_id[r] % V) == eos;
        if (!stop) { if (seen == lane) sel = r; ++seen; }
      }
      if (sel < 0) {
        int want = lane - seen;
        for (int r = 0; r < k2; ++r) {
          const bool stop = last || (top_id[r] % V) == eos;
          if (stop) { if (want == 0) sel = r; --want; }
        }
      }
      const bool stop = last || (top_id[sel] % V) == eos;
      run_r[lane] = sel;
      run_new[lane] = stop ? top_s[sel] + kBeamNeg : top_s[sel];
    }
    // rule 4: merged list = K finished hypotheses, then the K best candidates
    if (lane < k2) {
      float ms;
      if (lane < K) {
        ms = fin_score[b * K + lane];
      } else {
        const int r = lane - K;
        const bool stop = last || (top_id[r] % V) == eos;
        ms = (stop && !full && open) ? top_s[r] / L : -INFINITY;
      }
      if (!(ms == ms)) ms = -INFINITY;            // keeps the ranks below a permutation
      m_s[lane] = ms;
    }
    __syncthreads();
    if (lane < k2) {
      const float ms = m_s[lane];
      int rank = 0;
      for (int j = 0; j < k2; ++j) rank += (m_s[j] > ms || (m_s[j] == ms && j < lane)) ? 1 : 0;
      if (rank < K) {
        fin_src[rank] = lane;
        fin_new[rank] = ms;
        flag_new[rank] = lane < K ? fin_flag[b * K + lane] : (uint8_t)1;
      }
    }
    __syncthreads();                              // every read of the old scores and flags is done
    // sequences: position p of every old row is read before position p of any row is written
    int rbeam[kBeamMaxK], rtok[kBeamMaxK], fsrc[kBeamMaxK], fbeam[kBeamMaxK], ftok[kBeamMaxK];
#pragma unroll
    for (int j = 0; j < kBeamMaxK; ++j) {
      if (j < K) {
        const int id = top_id[run_r[j]];
        rbeam[j] = id / V; rtok[j] = id % V;
        fsrc[j] = fin_src[j];
        const int fid = top_id[max(fsrc[j] - K, 0)];
        fbeam[j] = fid / V; ftok[j] = fid % V;
      }
    }
    long* rs = run_seq + (size_t)b * K * T;
    long* fs = fin_seq + (size_t)b * K * T;
    for (int p = lane; p < T; p += 64) {
      long rv[kBeamMaxK], fv[kBeamMaxK];
#pragma unroll
      for (int j = 0; j < kBeamMaxK; ++j) {
        if (j < K) {
          rv[j] = p == t ? (long)rtok[j] : rs[(size_t)rbeam[j] * T + p];
          fv[j] = fsrc[j] < K ? fs[(size_t)fsrc[j] * T + p]
                              : (p == t ? (long)ftok[j] : rs[(size_t)fbeam[j] * T + p]);
        }
      }
#pragma unroll
      for (int j = 0; j < kBeamMaxK; ++j) {
        if (j < K) {
          rs[(size_t)j * T + p] = rv[j];
          fs[(size_t)j * T + p] = fv[j];
        }
      }
    }
    if (lane < K) {
      const int row = b * K + lane;
      run_score[row] = run_new[lane];
      fin_score[row] = fin_new[lane];
      fin_flag[row] = flag_new[lane];
      const int id = top_id[run_r[lane]];
      beam_idx[row] = (long)b * K + id / V;
      cur[row] = id % V;
    }
    if (lane == 0) {
      // rule 5
      float worst = fin_new[0];
      for (int k = 1; k < K; ++k) worst = fminf(worst, fin_new[k]);
      const float best = run_new[0] / L;
      bool any = false;
      for (int k = 0; k < K; ++k) any = any || best > (flag_new[k] ? worst : kBeamNeg);
      unsat[b] = (open && any) ? 1 : 0;
    }
  }
  // the step counter moves once every workgroup has read it: the last one to arrive advances it
  __syncthreads();
  if (lane == 0) {
    __threadfence();
    const unsigned old = atomicAdd(arrive, 1u);
    if (old == gridDim.x - 1) {
      atomicExch(arrive, 0u);
      if (valid) *pos = t + 1;
    }
  }
}

// ----------------------------------------------------------------------------- cache reorder
// table: n source pointers, then n destination pointers; every tensor [R, T, H, D] bf16, a row
// of row_chunks 16-byte chunks, slot_chunks of them per time slot.  Copies slots < *pos.
__global__ __launch_bounds__(256) void cache_reorder_kernel(const long* __restrict__ table, int n,
                                                            const long* __restrict__ beam_idx,
                                                            const long* __restrict__ pos, int R, int T,
                                                            long row_chunks, int slot_chunks) {
  const long c = (long)blockIdx.x * 256 + threadIdx.x;
  const int r = blockIdx.y, z = blockIdx.z;
  long count = *pos;
  count = count < 0 ? 0 : (count > T ? T : count);
  if (c >= count * slot_chunks) return;
  const long src_row = beam_idx[r];
  if (src_row < 0 || src_row >= R) return;
  const u16x8* src = reinterpret_cast<const u16x8*>(table[z]);
  u16x8* dst = reinterpret_cast<u16x8*>(table[n + z]);
  dst[(size_t)r * row_chunks + c] = src[(size_t)src_row * row_chunks + c];
}

}  // namespace ct

extern "C" {

// X [R, V] bf16 (is_bf16) or fp32, contiguous -> lse [R], top_val / top_tok [R, k2]; 2 <= k2 <= 16
int ct_beam_topk(const void* X, int is_bf16, float* lse, float* top_val, int* top_tok, int R, int V, int k2,
                 hipStream_t stream) {
  if (R <= 0 || k2 < 2 || k2 > 2 * ct::kBeamMaxK || V < k2) return 1;
  const int kk = k2 <= 2 ? 2 : k2 <= 4 ? 4 : k2 <= 8 ? 8 : 16;
#define CT_BEAM_TOPK(T_, KK_)                                                                          \
  hipLaunchKernelGGL((ct::beam_topk_kernel<T_, KK_>), dim3(R), dim3(256), 0, stream, (const T_*)X, lse, \
                     top_val, top_tok, V, k2)
#define CT_BEAM_TOPK_T(T_)                                  \
  switch (kk) {                                             \
    case 2: CT_BEAM_TOPK(T_, 2); break;                     \
    case 4: CT_BEAM_TOPK(T_, 4); break;                     \
    case 8: CT_BEAM_TOPK(T_, 8); break;                     \
    default: CT_BEAM_TOPK(T_, 16); break;                   \
  }
  if (is_bf16) { CT_BEAM_TOPK_T(ct::bf16_t) } else { CT_BEAM_TOPK_T(float) }
#undef CT_BEAM_TOPK_T
#undef CT_BEAM_TOPK
  return hipGetLastError() == hipSuccess ? 0 : 2;
}

int ct_beam_update(const float* lse, const float* top_val, const int* top_tok, long* run_seq, float* run_score,
                   long* fin_seq, float* fin_score, uint8_t* fin_flag, uint8_t* unsat, const float* len_pen,
                   long* pos, unsigned* arrive, long* beam_idx, long* cur, float* cand_score, long* cand_idx, int B,
                   int K, int V, int T, int eos, int early, hipStream_t stream) {
  if (B <= 0 || K < 1 || K > ct::kBeamMaxK || V < 2 * K || T < 1 || (long)K * V > INT_MAX) return 1;
  hipLaunchKernelGGL(ct::beam_update_kernel, dim3(B), dim3(64), 0, stream, lse, top_val, top_tok, run_seq,
                     run_score, fin_seq, fin_score, fin_flag, unsat, len_pen, pos, arrive, beam_idx, cur,
                     cand_score, cand_idx, K, V, T, eos, early);
  return hipGetLastError() == hipSuccess ? 0 : 2;
}

// n tensor pairs of [R, T, slot_elems] bf16 (slot_elems = H * D, a multiple of 8)
int ct_cache_reorder(const long* table, int n, const long* beam_idx, const long* pos, int R, int T, int slot_elems,
                     hipStream_t stream) {
  if (n <= 0 || n > 65535 || R <= 0 || R > 65535 || T <= 0 || slot_elems <= 0 || slot_elems % 8) return 1;
  const int slot_chunks = slot_elems / 8;
  const long row_chunks = (long)T * slot_chunks;
  const long gx = (row_chunks + 255) / 256;
  if (gx > INT_MAX) return 1;
  hipLaunchKernelGGL(ct::cache_reorder_kernel, dim3((unsigned)gx, R, n), dim3(256), 0, stream, table, n, beam_idx,
                     pos, R, T, row_chunks, slot_chunks);
  return hipGetLastError() == hipSuccess ? 0 : 2;
}

}  // extern "C"
