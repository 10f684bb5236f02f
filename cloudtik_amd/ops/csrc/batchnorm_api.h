// The host interface of batchnorm.hip: one forward and one backward call descriptor, the
// launchers with a short argument list, and the workspace sizes.  Included by batchnorm.hip (so
// the definitions are checked against these declarations) and by bindings_bn.cpp (compiled by
// g++), so a field or a parameter has one type for both compilers.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <type_traits>

// most partial blocks of a reduction pass (ct_bn_max_blocks()), tiles per first-level merge /
// sum group, most channels of the reductions
constexpr int kCtBnMaxBlocks = 2048;
constexpr int kCtBnGroup = 64;
constexpr int kCtBnMaxC = 2048;

// Workspace sizes in floats, stated once for the launchers, the bindings and (through
// bn_given_part_floats) ops/conv.py.
// block partials of a statistics or backward-reduce pass
inline long ct_bn_block_part_floats(long C) { return 2L * kCtBnMaxBlocks * C; }
// first-level groups of `tiles` tile partials
inline long ct_bn_groups(long tiles) { return (tiles + kCtBnGroup - 1) / kCtBnGroup; }
// producer (mean, M2) partials [2][tiles][C] with the tail the forward merges into.  The launcher
// merges above max(2 * kCtBnGroup, CLOUDTIK_AMD_BN_DIRECT_TILES) tiles, so the tail from
// 2 * kCtBnGroup on covers every setting of the knob (0 included).
inline long ct_bn_given_part_floats(long tiles, long C) {
  return 2 * (tiles + (tiles > 2 * kCtBnGroup ? ct_bn_groups(tiles) : 0)) * C;
}
// backward with given sums: their first-level sums q1, q2 [groups][C], then coef
inline long ct_bn_bwd_work_floats(long tiles, long C) { return 2 * ct_bn_groups(tiles) * C + 3 * C; }
// (ca, c1, c0) of dx = ca dy' + c1 x + c0
inline long ct_bn_coef_floats(long C) { return 3 * C; }

// One BatchNorm of a call.  Callers value-initialise the call (CtBnFwd c{}) and set what it
// uses: an unused pointer stays null and an unused number zero.
struct CtBnSide {
  const void* x;                      // bf16 [M, C]
  const void *gamma, *beta;           // bf16, or fp32 with param_f32 / param_flags bit 0 (beta: forward only)
  float *run_mean, *run_var;          // forward: updated in place
  float* stat;                        // float[4C] save_mean, save_invstd, a, b: the forward writes, the backward reads
  // tiles == 0: the call runs its own reduction pass over x into part = float[ct_bn_block_part_floats(C)].
  // tiles > 0, forward: part = the producer's (mean, M2) partials, ct_bn_given_part_floats(tiles, C),
  // rows_per_tile rows each, the last one short.
  float* part;
  int tiles, rows_per_tile;
  // backward
  void *dx, *dgamma, *dbeta;          // dgamma / dbeta in gamma's dtype
  float* coef;                        // own reduction: float[ct_bn_coef_floats(C)] scratch
  // tiles > 0, backward: the producer's per-tile sums p1 [tiles][C] and p2 = p1 + p2off, and
  // work = float[ct_bn_bwd_work_floats(tiles, C)], whose last 3C floats receive coef
  const float* p1; long p2off; float* work;
};

// y = [relu](bn(a.x) [+ res]) [+ ReLU bitmask]; with b.x, y = relu(bn(a.x) + bn(b.x)) + bitmask;
// with arg, the ResNet stem y = maxpool3x3/s2/p1(relu(bn(a.x))) + byte argmax.
struct CtBnFwd {
  CtBnSide a, b;
  const void* res;                    // bf16 [M, C] or null
  void* y;
  void* mask;                         // uint8 [M C / 8] or null (the pair always writes it)
  int relu;
  void* arg;                          // stem pool: uint8 [N, OH, OW, C], x = [N, H, W, C], M = N H W
  int N, H, W, OH, OW;
  int M, C;
  float eps, momentum;
  int param_f32;
};

struct CtBnBwd {
  const void* dy;                     // with given sums: already ReLU-masked
  // relu_mode (own reduction only): 0 none, 1 mask from y (bf16), 2 recomputed from x and stat,
  // 3 y is the forward's ReLU bitmask
  const void* y; int relu_mode;
  void* dres;                         // own reduction: the masked gradient, or null
  // a alone with its own reduction or with given sums (a null a.dx then: coefficients only); a
  // with given sums and b with its own reduction: one apply pass writes a.dx and b.dx
  CtBnSide a, b;
  int param_flags;                    // bit 0: fp32 parameters, bit 1: accumulate into dgamma / dbeta
  int M, C;
};
static_assert(std::is_standard_layout<CtBnFwd>::value && std::is_trivially_copyable<CtBnFwd>::value &&
              std::is_standard_layout<CtBnBwd>::value && std::is_trivially_copyable<CtBnBwd>::value,
              "the BatchNorm call descriptors cross two compilers");

// 0, a negative refusal code (the table is in front of the definitions; a refused call has
// launched nothing), or 7: a launch failed
extern "C" int ct_bn_fwd(const CtBnFwd* c, hipStream_t stream);
extern "C" int ct_bn_bwd(const CtBnBwd* c, hipStream_t stream);
// inference-mode forward with given affine coefficients a, b (float[C] each)
extern "C" int ct_bn_apply(const void* x, const void* res, const float* a, const float* b, void* y, int M, int C,
                           int relu, hipStream_t stream);
extern "C" int ct_bn_max_blocks();
// gradient of maxpool3x3/s2/p1 from the byte argmax
extern "C" int ct_maxpool3s2_bwd(const void* dy, const void* arg, void* dx, int N, int H, int W, int C, int OH,
                                 int OW, hipStream_t stream);
// the same + the stem BatchNorm's backward reduction: dxm = the masked gradient, part =
// float[2 * ct_maxpool3s2_bwd_bn_rows(N, H) * C] (p1 rows then p2 rows), stat = the forward's
extern "C" int ct_maxpool3s2_bwd_bn(const void* dy, const void* arg, const void* x, const float* stat, void* dxm,
                                    float* part, int N, int H, int W, int C, int OH, int OW, hipStream_t stream);
extern "C" long ct_maxpool3s2_bwd_bn_rows(int N, int H);
