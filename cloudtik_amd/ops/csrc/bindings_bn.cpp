// Bindings for the NHWC BatchNorm kernels (csrc/batchnorm.hip).  Every training forward fills one
// CtBnFwd and every backward one CtBnBwd (batchnorm_api.h); shapes, dtypes and workspace sizes
// are validated here, and the launchers refuse what is left before they launch anything.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <hip/hip_runtime.h>
#include <initializer_list>
#include <vector>
#include "batchnorm_api.h"

#define CHECK_F32(x) TORCH_CHECK((x).scalar_type() == at::kFloat, #x " must be fp32")
#define CHECK_IN(x) TORCH_CHECK((x).is_cuda() && (x).is_contiguous(), #x " must be a contiguous GPU tensor")

using OptTensor = c10::optional<at::Tensor>;

static inline hipStream_t cur_stream() { return at::hip::getCurrentHIPStream().stream(); }
static inline bool given(const OptTensor& t) { return t.has_value() && t->defined(); }
static at::Tensor f32_empty(const at::Tensor& like, long n) { return at::empty({n}, like.options().dtype(at::kFloat)); }

static void check_nhwc(const at::Tensor& x, const char* name) {
  TORCH_CHECK(x.is_cuda(), name, " must be a GPU tensor");
  TORCH_CHECK(x.scalar_type() == at::kBFloat16, name, " must be bf16");
  TORCH_CHECK(x.dim() == 4 ? x.is_contiguous(at::MemoryFormat::ChannelsLast) : x.is_contiguous(),
              name, " must be channels_last (4-D) or contiguous [M, C]");
}
static int64_t nhwc_rows(const at::Tensor& x) { return x.numel() / x.size(1); }

// optional ReLU bitmask output of the training forwards: uint8, one byte per 8 channels
static void* mask_ptr(const OptTensor& mask, const at::Tensor& x) {
  if (!given(mask)) return nullptr;
  TORCH_CHECK(mask->is_cuda() && mask->scalar_type() == at::kByte && mask->is_contiguous() &&
              mask->numel() * 8 == x.numel(), "ReLU mask: uint8 [numel / 8]");
  return mask->data_ptr();
}

// gamma / beta (and the gamma of a backward) arrive in bf16 or in fp32 -- BatchNorm parameters kept
// in fp32 beside bf16 activations -- and the kernels read them in that dtype: 1 when fp32
static int bn_param_f32(const at::Tensor& gamma, const char* name) {
  TORCH_CHECK(gamma.is_cuda() && (gamma.scalar_type() == at::kBFloat16 || gamma.scalar_type() == at::kFloat), name,
              ": BatchNorm parameters must be bf16 or fp32 CUDA tensors");
  return gamma.scalar_type() == at::kFloat ? 1 : 0;
}

// ---------------------------------------------------------------- the forward call
// One forward side: its tensors, and what fill() allocates for it.  Statistics source: with
// `part`, the per-tile partials of x's producer (conv epilogue) -- means [tiles][C] then M2
// [tiles][C], tiles = ceil(M / rows_per_tile), then the tail of the first-level merge; without,
// the side's own pass, whose block partials go to `ws`.
struct FwdSide {
  const at::Tensor &x, &gamma, &beta, &run_mean, &run_var;
  const at::Tensor* part;
  int64_t rows_per_tile;
  at::Tensor stat, ws;   // stat = float[4C]: save_mean, save_invstd, a, b (y = x * a + b ...)
};

// checks the side's tensors, allocates and fills s; returns param_f32
static int fill(CtBnSide& s, FwdSide& t, const char* name) {
  const long C = t.x.size(1);
  TORCH_CHECK(t.gamma.numel() == C && t.beta.numel() == C && t.run_mean.numel() == C && t.run_var.numel() == C, name,
              ": per-channel tensors");
  TORCH_CHECK(t.run_mean.scalar_type() == at::kFloat && t.run_var.scalar_type() == at::kFloat, name,
              ": running statistics must be fp32");
  TORCH_CHECK(t.beta.is_cuda() && t.beta.scalar_type() == t.gamma.scalar_type(), name,
              ": gamma and beta must share a dtype");
  const int pf32 = bn_param_f32(t.gamma, name);
  if (t.part) {
    CHECK_IN(*t.part); CHECK_F32(*t.part);
    TORCH_CHECK(t.rows_per_tile > 0, name, ": rows per tile");
    const long tiles = (nhwc_rows(t.x) + t.rows_per_tile - 1) / t.rows_per_tile;
    TORCH_CHECK(t.part->numel() >= ct_bn_given_part_floats(tiles, C), name, ": part buffer");
    s.tiles = (int)tiles; s.rows_per_tile = (int)t.rows_per_tile;
  } else {
    t.ws = f32_empty(t.x, ct_bn_block_part_floats(C));
  }
  t.stat = f32_empty(t.x, 4 * C);
  s.x = t.x.data_ptr(); s.gamma = t.gamma.data_ptr(); s.beta = t.beta.data_ptr();
  s.run_mean = t.run_mean.data_ptr<float>(); s.run_var = t.run_var.data_ptr<float>();
  s.stat = t.stat.data_ptr<float>(); s.part = (t.part ? *t.part : t.ws).data_ptr<float>();
  return pf32;
}

static void launch(CtBnFwd& c, const at::Tensor& x, double eps, double momentum, const char* name) {
  c.M = (int)nhwc_rows(x); c.C = (int)x.size(1);
  c.eps = (float)eps; c.momentum = (float)momentum;
  const int rc = ct_bn_fwd(&c, cur_stream());
  TORCH_CHECK(rc == 0, name, ": unsupported shape (C=", c.C, ", M=", c.M, "), rc=", rc);
}

// bn_fwd_train (part null) and bn_fwd_train_given: returns (y, stat); mask_out (optional, uint8
// [numel / 8]) receives the ReLU bitmask (bit j of byte v: y > 0)
static std::vector<at::Tensor> fwd_plain(FwdSide a, const OptTensor& res, double eps, double momentum, bool relu,
                                         const OptTensor& mask_out, const char* name) {
  const at::Tensor& x = a.x;
  check_nhwc(x, "x");
  TORCH_CHECK(a.part || x.size(1) <= kCtBnMaxC, name, ": C <= 2048");
  if (given(res)) { check_nhwc(*res, "residual"); TORCH_CHECK(res->sizes() == x.sizes()); }
  CtBnFwd c{};
  c.param_f32 = fill(c.a, a, name);
  auto y = at::empty_like(x);
  c.res = given(res) ? res->data_ptr() : nullptr;
  c.y = y.data_ptr(); c.mask = mask_ptr(mask_out, x); c.relu = relu ? 1 : 0;
  launch(c, x, eps, momentum, name);
  return {y, a.stat};
}
std::vector<at::Tensor> bn_fwd_train(at::Tensor x, OptTensor res, at::Tensor gamma, at::Tensor beta,
                                     at::Tensor run_mean, at::Tensor run_var, double eps, double momentum, bool relu,
                                     OptTensor mask_out) {
  return fwd_plain({x, gamma, beta, run_mean, run_var, nullptr, 0}, res, eps, momentum, relu, mask_out, "bn_fwd_train");
}
std::vector<at::Tensor> bn_fwd_train_given(at::Tensor x, OptTensor res, at::Tensor gamma, at::Tensor beta,
                                           at::Tensor run_mean, at::Tensor run_var, at::Tensor part,
                                           int64_t rows_per_tile, double eps, double momentum, bool relu,
                                           OptTensor mask_out) {
  return fwd_plain({x, gamma, beta, run_mean, run_var, &part, rows_per_tile}, res, eps, momentum, relu, mask_out,
                   "bn_fwd_train_given");
}

// y = relu(bn(x) + bn2(x2)) with both BatchNorms' statistics from their producers' partials (the
// ResNet downsample block: bn3(conv3) + down_bn(down)): returns (y, mask bytes, stat, stat2)
std::vector<at::Tensor> bn_fwd_train_given2(at::Tensor x, at::Tensor gamma, at::Tensor beta, at::Tensor run_mean,
                                            at::Tensor run_var, at::Tensor part, int64_t rows_per_tile,
                                            at::Tensor x2, at::Tensor gamma2, at::Tensor beta2,
                                            at::Tensor run_mean2, at::Tensor run_var2, at::Tensor part2,
                                            int64_t rows_per_tile2, double eps, double momentum) {
  const char* name = "bn_fwd_train_given2";
  check_nhwc(x, "x");
  check_nhwc(x2, "x2");
  TORCH_CHECK(x2.sizes() == x.sizes() && x2.strides() == x.strides(), name, ": x2 layout");
  FwdSide a{x, gamma, beta, run_mean, run_var, &part, rows_per_tile};
  FwdSide b{x2, gamma2, beta2, run_mean2, run_var2, &part2, rows_per_tile2};
  CtBnFwd c{};
  c.param_f32 = fill(c.a, a, name);
  TORCH_CHECK(fill(c.b, b, name) == c.param_f32, name, ": parameter dtypes");
  auto y = at::empty_like(x);
  auto mask = at::empty({x.numel() / 8}, x.options().dtype(at::kByte));
  c.y = y.data_ptr(); c.mask = mask.data_ptr();
  launch(c, x, eps, momentum, name);
  return {y, mask, a.stat, b.stat};
}

// ResNet stem, bn_fwd_train_pool (part null) and bn_fwd_train_pool_given (part, rows per tile:
// conv_fwd(..., partials=True)): returns (y_pool [N, C, OH, OW] channels_last, argmax bytes
// [N, OH, OW, C] uint8, stat)
static std::vector<at::Tensor> fwd_pool(FwdSide a, double eps, double momentum, const char* name) {
  const at::Tensor& x = a.x;
  check_nhwc(x, "x");
  TORCH_CHECK(x.dim() == 4, name, ": 4-D NHWC input");
  TORCH_CHECK(x.size(1) % 8 == 0 && x.size(1) <= kCtBnMaxC, name, ": C % 8 == 0, C <= 2048");
  CtBnFwd c{};
  c.param_f32 = fill(c.a, a, name);
  c.N = x.size(0); c.H = x.size(2); c.W = x.size(3);
  c.OH = (c.H - 1) / 2 + 1; c.OW = (c.W - 1) / 2 + 1;
  auto y = at::empty({c.N, x.size(1), c.OH, c.OW}, x.options().memory_format(at::MemoryFormat::ChannelsLast));
  auto arg = at::empty({c.N, c.OH, c.OW, x.size(1)}, x.options().dtype(at::kByte));
  c.y = y.data_ptr(); c.arg = arg.data_ptr();
  launch(c, x, eps, momentum, name);
  return {y, arg, a.stat};
}
std::vector<at::Tensor> bn_fwd_train_pool(at::Tensor x, at::Tensor gamma, at::Tensor beta, at::Tensor run_mean,
                                          at::Tensor run_var, double eps, double momentum) {
  return fwd_pool({x, gamma, beta, run_mean, run_var, nullptr, 0}, eps, momentum, "bn_fwd_train_pool");
}
std::vector<at::Tensor> bn_fwd_train_pool_given(at::Tensor x, at::Tensor gamma, at::Tensor beta,
                                                at::Tensor run_mean, at::Tensor run_var, at::Tensor part,
                                                int64_t rows_per_tile, double eps, double momentum) {
  return fwd_pool({x, gamma, beta, run_mean, run_var, &part, rows_per_tile}, eps, momentum, "bn_fwd_train_pool_given");
}

at::Tensor bn_apply(at::Tensor x, OptTensor res, at::Tensor a, at::Tensor b, bool relu) {
  check_nhwc(x, "x");
  const int C = x.size(1);
  CHECK_F32(a); CHECK_F32(b); TORCH_CHECK(a.numel() == C && b.numel() == C);
  auto y = at::empty_like(x);
  int rc = ct_bn_apply(x.data_ptr(), given(res) ? res->data_ptr() : nullptr, a.data_ptr<float>(), b.data_ptr<float>(),
                       y.data_ptr(), (int)nhwc_rows(x), C, relu ? 1 : 0, cur_stream());
  TORCH_CHECK(rc == 0, "bn_apply: unsupported C");
  return y;
}

// ---------------------------------------------------------------- the backward call
// One backward side: gamma, the forward's stat and the optional accumulate targets (views of the
// flat gradient buffer, wanted when dgamma_acc is given), and what fill() allocates for it.  Sums:
// with `part`, the per-tile sums of the gradient's producer, float[2 * rows * C] with the first
// `tiles` rows of each half used; without, the side's own reduction.
struct BwdSide {
  const at::Tensor &gamma, &stat;
  const OptTensor &dgamma_acc, &dbeta_acc;
  const at::Tensor* part;
  int64_t tiles, rows;
  at::Tensor dgamma, dbeta, ws, coef;   // the targets or new tensors like gamma; workspace; (ca, c1, c0)
};

// checks the side's tensors over C channels, allocates and fills s; returns param_flags
static int fill(CtBnSide& s, BwdSide& t, long C, const char* name) {
  TORCH_CHECK(C <= kCtBnMaxC && t.stat.numel() == 4 * C, name, ": stat must be float[4C], C <= 2048");
  CHECK_F32(t.stat);
  TORCH_CHECK(t.gamma.numel() == C, name, ": gamma must have C elements");
  const int pf32 = bn_param_f32(t.gamma, name);
  const bool acc = given(t.dgamma_acc);
  if (acc) {
    TORCH_CHECK(given(t.dbeta_acc), name, ": dgamma_acc needs dbeta_acc");
    for (const at::Tensor* g : {&*t.dgamma_acc, &*t.dbeta_acc})
      TORCH_CHECK(g->is_contiguous() && g->numel() == C && g->scalar_type() == t.gamma.scalar_type(), name,
                  ": bad accumulate targets");
  }
  t.dgamma = acc ? *t.dgamma_acc : at::empty_like(t.gamma);
  t.dbeta = acc ? *t.dbeta_acc : at::empty_like(t.gamma);
  if (t.part) {
    CHECK_F32(*t.part);
    TORCH_CHECK(t.tiles > 0 && t.tiles <= t.rows && t.part->numel() >= 2 * t.rows * C, name, ": part buffer");
    t.ws = f32_empty(t.gamma, ct_bn_bwd_work_floats(t.tiles, C));
    t.coef = t.ws.narrow(0, t.ws.numel() - ct_bn_coef_floats(C), ct_bn_coef_floats(C));
    s.p1 = t.part->data_ptr<float>(); s.p2off = t.rows * C; s.tiles = (int)t.tiles; s.work = t.ws.data_ptr<float>();
  } else {
    t.ws = f32_empty(t.gamma, ct_bn_block_part_floats(C));
    t.coef = f32_empty(t.gamma, ct_bn_coef_floats(C));
    s.part = t.ws.data_ptr<float>(); s.coef = t.coef.data_ptr<float>();
  }
  s.gamma = t.gamma.data_ptr(); s.stat = t.stat.data_ptr<float>();
  s.dgamma = t.dgamma.data_ptr(); s.dbeta = t.dbeta.data_ptr();
  return pf32 | (acc ? 2 : 0);
}

static void launch(CtBnBwd& c, long M, long C, const char* name) {
  c.M = (int)M; c.C = (int)C;
  const int rc = ct_bn_bwd(&c, cur_stream());
  TORCH_CHECK(rc == 0, name, ": unsupported shape (C=", c.C, ", M=", c.M, "), rc=", rc);
}

// returns (dx, dres, dgamma, dbeta).  relu_mode: 0 no ReLU, 1 mask from y (forward had a
// residual), 2 mask recomputed from x and the forward's (a, b) -- y may be undefined then,
// 3 y is the forward's ReLU bitmask (uint8 [numel / 8]).
std::vector<at::Tensor> bn_bwd(at::Tensor dy, OptTensor y, at::Tensor x, at::Tensor gamma, at::Tensor stat,
                               int64_t relu_mode, bool need_dres, OptTensor dgamma_acc, OptTensor dbeta_acc) {
  check_nhwc(x, "x");
  at::Tensor dyc = dy.dim() == 4 ? dy.contiguous(at::MemoryFormat::ChannelsLast) : dy.contiguous();
  check_nhwc(dyc, "dy");
  TORCH_CHECK(relu_mode >= 0 && relu_mode <= 3, "bn_bwd: relu_mode 0/1/2/3");
  if (relu_mode == 1) {
    TORCH_CHECK(given(y), "bn_bwd: relu_mode 1 needs y");
    check_nhwc(*y, "y");
    TORCH_CHECK(y->sizes() == x.sizes(), "bn_bwd: y shape");
  }
  if (relu_mode == 3) {
    TORCH_CHECK(given(y), "bn_bwd: relu_mode 3 needs the mask");
    mask_ptr(y, x);
  }
  TORCH_CHECK(dyc.sizes() == x.sizes(), "bn_bwd: dy shape");
  BwdSide a{gamma, stat, dgamma_acc, dbeta_acc, nullptr, 0, 0};
  CtBnBwd c{};
  c.param_flags = fill(c.a, a, x.size(1), "bn_bwd");
  at::Tensor dx = at::empty_like(x), dres = need_dres ? at::empty_like(x) : at::Tensor();
  c.dy = dyc.data_ptr();
  c.y = (relu_mode == 1 || relu_mode == 3) ? y->data_ptr() : nullptr;
  c.relu_mode = (int)relu_mode;
  c.dres = need_dres ? dres.data_ptr() : nullptr;
  c.a.x = x.data_ptr(); c.a.dx = dx.data_ptr();
  launch(c, nhwc_rows(x), x.size(1), "bn_bwd");
  return {dx, dres, a.dgamma, a.dbeta};
}

// BatchNorm (+ ReLU) backward from the reduction done by the conv that produced dy
// (conv_igemm_bn): dym = the masked gradient, part as in BwdSide.  Returns (dx, dgamma, dbeta).
std::vector<at::Tensor> bn_bwd_given(at::Tensor dym, at::Tensor x, at::Tensor gamma, at::Tensor stat, at::Tensor part,
                                     int64_t tiles, int64_t rows, OptTensor dgamma_acc, OptTensor dbeta_acc) {
  check_nhwc(x, "x");
  check_nhwc(dym, "dym");
  TORCH_CHECK(dym.sizes() == x.sizes() && dym.strides() == x.strides(), "bn_bwd_given: dym / x layout");
  BwdSide a{gamma, stat, dgamma_acc, dbeta_acc, &part, tiles, rows};
  CtBnBwd c{};
  c.param_flags = fill(c.a, a, x.size(1), "bn_bwd_given");
  auto dx = at::empty_like(x);
  c.dy = dym.data_ptr();
  c.a.x = x.data_ptr(); c.a.dx = dx.data_ptr();
  launch(c, nhwc_rows(x), x.size(1), "bn_bwd_given");
  return {dx, a.dgamma, a.dbeta};
}

// backward of bn_fwd_train_given2 with the masked gradient and bn's partials from the consuming
// conv's epilogue: [dx, dx2, dgamma, dbeta, dgamma2, dbeta2] (accumulated into the *_acc targets,
// all four or none, when given)
std::vector<at::Tensor> bn_bwd_given_pair(at::Tensor dym, at::Tensor x, at::Tensor gamma, at::Tensor stat,
                                          at::Tensor part, int64_t tiles, int64_t rows, at::Tensor x2,
                                          at::Tensor gamma2, at::Tensor stat2, OptTensor dgamma_acc,
                                          OptTensor dbeta_acc, OptTensor dgamma2_acc, OptTensor dbeta2_acc) {
  const char* name = "bn_bwd_given_pair";
  check_nhwc(x, "x");
  check_nhwc(x2, "x2");
  check_nhwc(dym, "dym");
  TORCH_CHECK(dym.sizes() == x.sizes() && dym.strides() == x.strides() && x2.sizes() == x.sizes() &&
              x2.strides() == x.strides(), name, ": layouts");
  TORCH_CHECK(gamma2.scalar_type() == gamma.scalar_type(), name, ": parameter dtypes");
  for (const OptTensor* t : {&dbeta_acc, &dgamma2_acc, &dbeta2_acc})
    TORCH_CHECK(given(*t) == given(dgamma_acc), name, ": accumulate targets: all or none");
  BwdSide a{gamma, stat, dgamma_acc, dbeta_acc, &part, tiles, rows};
  BwdSide b{gamma2, stat2, dgamma2_acc, dbeta2_acc, nullptr, 0, 0};
  CtBnBwd c{};
  c.param_flags = fill(c.a, a, x.size(1), name);
  fill(c.b, b, x.size(1), name);
  auto dx = at::empty_like(x), dx2 = at::empty_like(x2);
  c.dy = dym.data_ptr();
  c.a.x = x.data_ptr(); c.a.dx = dx.data_ptr();
  c.b.x = x2.data_ptr(); c.b.dx = dx2.data_ptr();
  launch(c, nhwc_rows(x), x.size(1), name);
  return {dx, dx2, a.dgamma, a.dbeta, b.dgamma, b.dbeta};
}

// The BatchNorm backward's per-channel results WITHOUT the apply pass: (dgamma, dbeta, coef) from
// the producer's per-tile sums, coef = float[3C] = (ca, c1, c0) with dx = ca dym + c1 x + c0.  For
// a BatchNorm whose input gradient only feeds a weight gradient (the ResNet stem: dW = ca G1 +
// c1 G2 + c0 G0 over the conv's im2col columns, ops/functional.py _StemBlockFn).
std::vector<at::Tensor> bn_bwd_coefs_given(int64_t M, at::Tensor gamma, at::Tensor stat, at::Tensor part,
                                           int64_t tiles, int64_t rows, OptTensor dgamma_acc, OptTensor dbeta_acc) {
  const long C = gamma.numel();
  TORCH_CHECK(gamma.is_cuda() && C % 8 == 0 && M > 0, "bn_bwd_coefs_given: gamma, M");
  BwdSide a{gamma, stat, dgamma_acc, dbeta_acc, &part, tiles, rows};
  CtBnBwd c{};
  c.param_flags = fill(c.a, a, C, "bn_bwd_coefs_given");
  launch(c, M, C, "bn_bwd_coefs_given");
  return {a.dgamma, a.dbeta, a.coef};
}

// ---------------------------------------------------------------- stem max-pool backward
// gradient of maxpool3x3/s2/p1 from the byte argmax: dx [N, C, H, W] channels_last
at::Tensor maxpool3s2_bwd(at::Tensor dy, at::Tensor arg, int64_t H, int64_t W) {
  at::Tensor dyc = dy.contiguous(at::MemoryFormat::ChannelsLast);
  check_nhwc(dyc, "dy");
  const int N = dyc.size(0), C = dyc.size(1), OH = dyc.size(2), OW = dyc.size(3);
  TORCH_CHECK(arg.scalar_type() == at::kByte && arg.is_contiguous() && arg.numel() == dyc.numel(),
              "maxpool3s2_bwd: argmax bytes");
  TORCH_CHECK(OH == (H - 1) / 2 + 1 && OW == (W - 1) / 2 + 1 && C % 8 == 0, "maxpool3s2_bwd: shape");
  auto dx = at::empty({N, C, (long)H, (long)W}, dyc.options().memory_format(at::MemoryFormat::ChannelsLast));
  int rc = ct_maxpool3s2_bwd(dyc.data_ptr(), arg.data_ptr(), dx.data_ptr(), N, (int)H, (int)W, C, OH, OW,
                             cur_stream());
  TORCH_CHECK(rc == 0, "maxpool3s2_bwd: unsupported shape");
  return dx;
}

// stem backward: the max-pool gradient gather + the BatchNorm's ReLU mask and backward sums in one
// pass; returns the masked gradient (at x's shape) and fills part (float[2 * rows * C]: p1 rows
// then p2 rows, rows = maxpool3s2_bwd_bn_rows(N, H) tiles) for bn_bwd_given
at::Tensor maxpool3s2_bwd_bn(at::Tensor dy, at::Tensor arg, at::Tensor x, at::Tensor stat, at::Tensor part) {
  at::Tensor dyc = dy.contiguous(at::MemoryFormat::ChannelsLast);
  check_nhwc(dyc, "dy");
  check_nhwc(x, "x");
  CHECK_F32(stat);
  CHECK_F32(part);
  const int N = dyc.size(0), C = dyc.size(1), OH = dyc.size(2), OW = dyc.size(3);
  const int H = x.size(2), W = x.size(3);
  TORCH_CHECK(x.size(0) == N && x.size(1) == C && stat.numel() == 4 * (long)C, "maxpool3s2_bwd_bn: shapes");
  TORCH_CHECK(arg.scalar_type() == at::kByte && arg.is_contiguous() && arg.numel() == dyc.numel(),
              "maxpool3s2_bwd_bn: argmax bytes");
  TORCH_CHECK(part.is_contiguous() && part.numel() >= 2L * ct_maxpool3s2_bwd_bn_rows(N, H) * C,
              "maxpool3s2_bwd_bn: part buffer");
  auto dxm = at::empty_like(x);
  int rc = ct_maxpool3s2_bwd_bn(dyc.data_ptr(), arg.data_ptr(), x.data_ptr(), stat.data_ptr<float>(), dxm.data_ptr(),
                                part.data_ptr<float>(), N, H, W, C, OH, OW, cur_stream());
  TORCH_CHECK(rc == 0, "maxpool3s2_bwd_bn: unsupported shape");
  return dxm;
}

void register_bn(pybind11::module& m) {
  m.def("bn_fwd_train", &bn_fwd_train, pybind11::arg("x"), pybind11::arg("res"), pybind11::arg("gamma"),
        pybind11::arg("beta"), pybind11::arg("run_mean"), pybind11::arg("run_var"), pybind11::arg("eps"),
        pybind11::arg("momentum"), pybind11::arg("relu"), pybind11::arg("mask_out") = pybind11::none());
  m.def("bn_fwd_train_given", &bn_fwd_train_given, pybind11::arg("x"), pybind11::arg("res"), pybind11::arg("gamma"),
        pybind11::arg("beta"), pybind11::arg("run_mean"), pybind11::arg("run_var"), pybind11::arg("part"),
        pybind11::arg("rows_per_tile"), pybind11::arg("eps"), pybind11::arg("momentum"), pybind11::arg("relu"),
        pybind11::arg("mask_out") = pybind11::none());
  m.def("bn_fwd_train_given2", &bn_fwd_train_given2);
  m.def("bn_fwd_train_pool", &bn_fwd_train_pool);
  m.def("bn_fwd_train_pool_given", &bn_fwd_train_pool_given);
  m.def("bn_apply", &bn_apply);
  m.def("bn_bwd", &bn_bwd);
  m.def("bn_bwd_given", &bn_bwd_given);
  m.def("bn_bwd_given_pair", &bn_bwd_given_pair);
  m.def("bn_bwd_coefs_given", &bn_bwd_coefs_given);
  m.def("maxpool3s2_bwd", &maxpool3s2_bwd);
  m.def("maxpool3s2_bwd_bn", &maxpool3s2_bwd_bn);
  m.def("maxpool3s2_bwd_bn_rows", [](int64_t N, int64_t H) { return (int64_t)ct_maxpool3s2_bwd_bn_rows((int)N, (int)H); });
  // floats of a producer-partials buffer with its merge tail (ops/conv.py allocates it)
  m.def("bn_given_part_floats", [](int64_t tiles, int64_t C) { return (int64_t)ct_bn_given_part_floats(tiles, C); });
}
