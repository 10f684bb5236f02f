// The host interface of attention.hip: one call descriptor and two entry points.  Included by
// attention.hip (so the definitions are checked against these declarations) and by bindings.cpp
// (compiled by g++), so a field or a parameter has one type for both compilers.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <type_traits>

// longest relative-position bias vector per head (the kernels stage one head's vector in LDS)
constexpr int kCtAttnRelBiasMax = 4096;

// a [B, S, H, D] bf16 view with unit stride on D; strides in elements
struct CtAttnView { const void* p; long sb, ss, sh; };

// One attention call.  Callers value-initialise it (CtAttnCall c{}) and set what the call uses:
// an unused pointer stays null and an unused number zero.
struct CtAttnCall {
  CtAttnView q, k, v, o;              // o: written by the forward, read by the backward
  CtAttnView dO, dq, dk, dv;          // backward only
  const float* kbias; long kb_sb;     // additive key bias [B, Sk] fp32 (row stride kb_sb); null: none
  // relative-position bias [H, relb_len] fp32 (row stride relb_sh): score(q, k) +=
  // relb[h][k - q + rel_base]; null: none
  const float* relb; long relb_sh; int relb_len, rel_base;
  float* d_rel; long d_sh, d_si;      // backward with relb: its gradient [H, relb_len], any strides
  float* lse;                         // [B * H, Sq] log2-domain; the forward writes, the backward reads
  // backward workspaces: delta float[B H Sq] (without relb); dq_acc float[B H Sq D] when Sk > 128;
  // drel_ws float[B ceil(Sk / 128) H ct_attn_bwd_relbias_window(Sq)] (with relb).  None needs clearing.
  float *delta, *dq_acc, *drel_ws;
  int B, H, Sq, Sk, D;                // D: 64 or 128
  float scale, p_drop; uint64_t seed, offset;
  int causal;
};
static_assert(std::is_standard_layout<CtAttnCall>::value && std::is_trivially_copyable<CtAttnCall>::value,
              "CtAttnCall crosses two compilers");

// 0, or a negative refusal code (the table is in front of the definitions); a refused call
// has written nothing and launched nothing.
extern "C" int ct_attn_fwd(const CtAttnCall* c, hipStream_t stream);
extern "C" int ct_attn_bwd(const CtAttnCall* c, hipStream_t stream);
// offsets in one workgroup's window of the bias gradient, and the most the LDS budget takes: at
// head dim 64, and at head dim D (64 or 128)
extern "C" int ct_attn_bwd_relbias_window(int Sq);
extern "C" int ct_attn_bwd_relbias_max_window();
extern "C" int ct_attn_bwd_relbias_max_window_d(int D);
