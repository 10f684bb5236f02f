// History-dependent token bans for graph-replayed decoding on gfx950 (ops/constrain.py states the
// rule; `constrain_reference` there is the specification this kernel is tested against).
//
// One decode step leaves logits [R, V].  One launch follows on the caller's stream and reads
// nothing back to the host: the step `t` comes from the device.
//
//   logits_constrain_kernel  one workgroup of one wave per row.  The row's decoder input
//                            h = [start] + hist[r, :t] is staged in LDS as int32 (a token outside
//                            [0, V) becomes -1, which matches nothing and bans nothing).  Lanes test
//                            the n-gram match positions, then the bad words, with stride 64, and
//                            append the banned tokens to an LDS list by ballot and prefix count, so
//                            the list is in a fixed order: history index, word index, EOS.
//                            Phase A loads the original logit of every list entry into LDS; a
//                            workgroup barrier follows; phase B stores -inf.  No original value is
//                            loaded after the barrier, so a token that is in the list twice cannot
//                            be read back as -inf, and it enters ban_lse once: an entry whose token
//                            stands earlier in the list contributes nothing.
//
// Reproducibility: the list order is fixed, every lane sums its entries in list order and the wave
// reduces with a fixed butterfly, so ban_lse and the row come out bit-identical on every launch.
// Cost: O(t) match tests and O(L^2 / 64) LDS compares for a list of L entries; L is the number of
// banned occurrences, a handful for n >= 2 and t + 1 for n = 1.
#include "common.h"
#include <math.h>

namespace ct {

constexpr int kConMaxT = 1024;                                 // steps of history a row may hold
constexpr int kConMaxWords = 1024;
constexpr int kConMaxWordTokens = 2048;
constexpr int kConList = kConMaxT + kConMaxWords + 1;          // n-gram hits + words + EOS

template <typename T>
__device__ __forceinline__ T con_neg_inf();
template <>
__device__ __forceinline__ float con_neg_inf<float>() { return -INFINITY; }
template <>
__device__ __forceinline__ bf16_t con_neg_inf<bf16_t>() { return (bf16_t)0xFF80u; }

// appends `tok` of every lane with `hit` to list[count ..] in lane order; returns the new count
__device__ __forceinline__ int con_append(int* list, int count, bool hit, int tok, int lane) {
  const unsigned long long mask = __ballot(hit);
  if (hit) list[count + __popcll(mask & ((1ull << lane) - 1ull))] = tok;
  return count + __popcll(mask);
}

template <typename T>
__global__ __launch_bounds__(64) void logits_constrain_kernel(
    T* __restrict__ X, const long* __restrict__ hist, const long* __restrict__ pos, const int* __restrict__ wtok,
    const int* __restrict__ woff, float* __restrict__ ban_lse, int V, int Tn, int start_token, int n, int min_new,
    int eos, int n_words, int n_wtok) {
  __shared__ int h[kConMaxT];
  __shared__ int list[kConList];
  __shared__ float val[kConList];
  const int row = blockIdx.x, lane = threadIdx.x;
  const long t64 = pos[0];
  if (t64 < 0 || t64 >= Tn) {                    // no step to constrain: nothing is read or written
    if (ban_lse != nullptr && lane == 0) ban_lse[row] = -INFINITY;
    return;
  }
  const int t = (int)t64, len = t + 1;           // len <= Tn <= kConMaxT entries of h
  const long* hr = hist + (size_t)row * Tn;
  T* x = X + (size_t)row * V;

  for (int j = lane; j < len; j += 64) {         // slots >= t of hist are never read
    const long tok = j == 0 ? (long)start_token : hr[j - 1];
    h[j] = (tok >= 0 && tok < V) ? (int)tok : -1;
  }
  __syncthreads();

  int count = 0;
  // n-gram: position i in 0 .. len - n bans h[i + n - 1] when h[i .. i + n - 2] equals the last
  // n - 1 tokens of h
  if (n >= 1 && len >= n) {
    const int cnt = len - n + 1, suf = len - (n - 1);
    for (int base = 0; base < cnt; base += 64) {
      const int i = base + lane;
      bool hit = i < cnt;
      for (int j = 0; hit && j < n - 1; ++j) hit = h[suf + j] >= 0 && h[i + j] == h[suf + j];
      const int tok = hit ? h[i + n - 1] : -1;
      count = con_append(list, count, hit && tok >= 0, tok, lane);
    }
  }
  // bad words: word w bans its last token when its first m - 1 tokens end h
  for (int base = 0; base < n_words; base += 64) {
    const int w = base + lane;
    bool hit = w < n_words;
    int tok = -1;
    if (hit) {
      const int o0 = woff[w], o1 = woff[w + 1];
      const bool table_ok = o0 >= 0 && o1 > o0 && o1 <= n_wtok;      // a broken table entry bans nothing
      const int m = table_ok ? o1 - o0 : 1;
      hit = table_ok && m - 1 <= len;
      for (int j = 0; hit && j < m - 1; ++j) {
        const int a = h[len - (m - 1) + j];
        hit = a >= 0 && a == wtok[o0 + j];
      }
      if (hit) tok = wtok[o1 - 1];
      hit = hit && tok >= 0 && tok < V;
    }
    count = con_append(list, count, hit, tok, lane);
  }
  // minimum length
  if (t < min_new && eos >= 0 && eos < V) {
    if (lane == 0) list[count] = eos;
    ++count;
  }
  __syncthreads();

  // phase A: every original value, and the entries that repeat an earlier token
  float m = -INFINITY;
  if (ban_lse != nullptr) {
    for (int k = lane; k < count; k += 64) {
      const int tok = list[k];
      float v = to_f<T>(x[tok]);
      for (int e = 0; e < k; ++e)
        if (list[e] == tok) { v = -INFINITY; break; }
      if (!(v == v)) v = -INFINITY;                // a NaN logit counts as -inf, as in the beam kernels
      val[k] = v;
      m = fmaxf(m, v);
    }
    m = wave_max(m);
  }
  __syncthreads();                                 // read before write: no load of x follows

  // phase B
  for (int k = lane; k < count; k += 64) x[list[k]] = con_neg_inf<T>();
  if (ban_lse != nullptr) {
    float s = 0.f;
    if (m > -INFINITY && m < INFINITY)
      for (int k = lane; k < count; k += 64) s += expf(val[k] - m);
    s = wave_sum(s);
    if (lane == 0) ban_lse[row] = (m > -INFINITY && m < INFINITY) ? m + logf(s) : m;
  }
}

}  // namespace ct

extern "C" {

int ct_constrain_max_steps() { return ct::kConMaxT; }
int ct_constrain_max_words() { return ct::kConMaxWords; }
int ct_constrain_max_word_tokens() { return ct::kConMaxWordTokens; }

// X [R, V] bf16 (is_bf16) or fp32, contiguous, in place; hist [R, T]; pos [1]; wtok [n_wtok] and
// woff [n_words + 1] (null when n_words = 0); ban_lse [R] or null
int ct_logits_constrain(void* X, int is_bf16, const long* hist, const long* pos, const int* wtok, const int* woff,
                        float* ban_lse, int R, int V, int T, int start_token, int n, int min_new, int eos,
                        int n_words, int n_wtok, hipStream_t stream) {
  if (R <= 0 || V < 1 || T < 1 || T > ct::kConMaxT || n < 0 || min_new < 0) return 1;
  if (n_words < 0 || n_words > ct::kConMaxWords || n_wtok < 0 || n_wtok > ct::kConMaxWordTokens) return 1;
  if (n_words > 0 && (wtok == nullptr || woff == nullptr)) return 1;
  if (is_bf16)
    hipLaunchKernelGGL((ct::logits_constrain_kernel<ct::bf16_t>), dim3(R), dim3(64), 0, stream, (ct::bf16_t*)X, hist,
                       pos, wtok, woff, ban_lse, V, T, start_token, n, min_new, eos, n_words, n_wtok);
  else
    hipLaunchKernelGGL((ct::logits_constrain_kernel<float>), dim3(R), dim3(64), 0, stream, (float*)X, hist, pos, wtok,
                       woff, ban_lse, V, T, start_token, n, min_new, eos, n_words, n_wtok);
  return hipGetLastError() == hipSuccess ? 0 : 2;
}

}  // extern "C"
