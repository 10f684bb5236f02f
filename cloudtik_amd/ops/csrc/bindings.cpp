// Thin PyTorch bindings for the cloudtik_amd CDNA4 op library.
// Every function validates shapes/dtypes on the host (a mis-shaped launch of a hand-written
// kernel can fault the GPU), fetches the current HIP stream and calls the extern "C"
// launcher.  No allocation happens inside the launchers; workspaces come from the caller.
#include <torch/extension.h>
#include <map>
#include <mutex>
#include <ATen/hip/HIPContext.h>
#include <hip/hip_runtime.h>
#include "attention_api.h"   // the attention entries: declared once, for attention.hip too

extern "C" {
int ct_layernorm_fwd(const void*, const void*, const void*, const void*, const void*, void*, void*,
                     float*, float*, int, int, float, int, float, uint64_t, uint64_t, hipStream_t);
int ct_layernorm_bwd_grid(int M, int N);
int ct_layernorm_bwd(const void*, const void*, const void*, const float*, const float*,
                     const void*, void*, void*, float*, void*, void*, void*, int, int, int, int,
                     int, float, uint64_t, uint64_t, hipStream_t);
int ct_layernorm_bwd2(const void*, const void*, const void*, const float*, const float*,
                      const void*, void*, void*, float*, void*, void*, void*, int, int, int, int,
                      int, float, uint64_t, uint64_t, int, const void*, hipStream_t);
int ct_colsum(const float*, void*, int, int, int, int, hipStream_t);
int ct_bias_act_fwd(const void*, const void*, void*, long, int, int, hipStream_t);
int ct_bias_act_bwd_grid(long M);
int ct_bias_act_bwd(const void*, const void*, const void*, void*, float*, void*, long, int, int,
                    int, int, hipStream_t);
int ct_dropout(const void*, void*, long, float, uint64_t, uint64_t, hipStream_t);
int ct_embed3_fwd(const int64_t*, const int64_t*, const void*, const void*, const void*, void*, int,
                  int, int, hipStream_t);
int ct_embed3_bwd(const int64_t*, const int64_t*, const void*, float*, float*, float*, int, int, int, int, hipStream_t);
int ct_cast(const void*, int, void*, int, long, float, int, hipStream_t);
int ct_splitk_reduce(const float*, int, long, void*, int, hipStream_t);
int ct_splitk_reduce_clear(float*, int, long, void*, int, hipStream_t);
int ct_splitk_reduce2(const float*, int, long, void*, const float*, int, long, void*, int, hipStream_t);
int ct_splitk_reduce_group(int, const float* const*, const int*, const long*, void* const*, int, hipStream_t);
int ct_lamb(const void*, int, float*, float*, float*, void*, int, const int*, const long*,
            const int*, int, const int*, int, const float*, const float*, float, float, float, int,
            int, float*, float*, int, hipStream_t);
int ct_adam(const void*, int, float*, float*, float*, void*, int, const int*, const long*,
            const int*, int, const float*, const float*, float, float, float, int, hipStream_t);
int ct_sgd(const void*, int, float*, float*, void*, int, const int*, const long*, const int*, int,
           const float*, const float*, float, float, int, hipStream_t);
int ct_sumsq(const void*, int, long, float*, float*, hipStream_t);
int ct_clip_coef(const float*, float*, float, float, hipStream_t);
int ct_xent_fwd(const void*, void*, int, int, const int64_t*, float*, float*, const float*, int, int,
                float, hipStream_t);
}

#define CHECK_CUDA(x) TORCH_CHECK((x).is_cuda(), #x " must be a GPU tensor")
#define CHECK_CONTIG(x) TORCH_CHECK((x).is_contiguous(), #x " must be contiguous")
#define CHECK_BF16(x) TORCH_CHECK((x).scalar_type() == at::kBFloat16, #x " must be bf16")
#define CHECK_F32(x) TORCH_CHECK((x).scalar_type() == at::kFloat, #x " must be fp32")
#define CHECK_IN(x) do { CHECK_CUDA(x); CHECK_CONTIG(x); } while (0)

static inline hipStream_t cur_stream() { return at::hip::getCurrentHIPStream().stream(); }
static inline const void* optr(const c10::optional<at::Tensor>& t) {
  return (t.has_value() && t->defined()) ? t->data_ptr() : nullptr;
}
static inline void* optr_mut(const c10::optional<at::Tensor>& t) {
  return (t.has_value() && t->defined()) ? t->data_ptr() : nullptr;
}
static inline int dt_code(const at::Tensor& t) {
  if (t.scalar_type() == at::kFloat) return 0;
  if (t.scalar_type() == at::kBFloat16) return 1;
  TORCH_CHECK(false, "only fp32 / bf16 supported");
  return -1;
}

// ---------------------------------------------------------------- layernorm
// returns (y, s, mean, rstd); s is undefined when no bias/residual/dropout was applied
std::vector<at::Tensor> layernorm_fwd(at::Tensor x, c10::optional<at::Tensor> bias,
                                      c10::optional<at::Tensor> res, at::Tensor gamma,
                                      c10::optional<at::Tensor> beta, double eps, bool rms,
                                      double p_drop, int64_t seed, int64_t offset, bool keep_sum) {
  CHECK_IN(x); CHECK_BF16(x); CHECK_IN(gamma); CHECK_BF16(gamma);
  const int N = x.size(-1);
  const int M = x.numel() / N;
  TORCH_CHECK(gamma.numel() == N, "gamma size");
  if (bias.has_value() && bias->defined()) { CHECK_IN(*bias); CHECK_BF16(*bias); TORCH_CHECK(bias->numel() == N); }
  if (res.has_value() && res->defined()) { CHECK_IN(*res); CHECK_BF16(*res); TORCH_CHECK(res->numel() == x.numel()); }
  if (beta.has_value() && beta->defined()) { CHECK_IN(*beta); CHECK_BF16(*beta); TORCH_CHECK(beta->numel() == N); }
  auto y = at::empty_like(x);
  // keep_sum = false: the caller's backward runs from y (layernorm_bwd_into from_y), so the
  // normalised input sum s is not written
  const bool need_s = keep_sum && (optr(bias) || optr(res) || p_drop > 0.0);
  at::Tensor s = need_s ? at::empty_like(x) : at::Tensor();
  auto fo = x.options().dtype(at::kFloat);
  auto mean = at::empty({M}, fo);
  auto rstd = at::empty({M}, fo);
  int rc = ct_layernorm_fwd(x.data_ptr(), optr(bias), optr(res), gamma.data_ptr(), optr(beta),
                            y.data_ptr(), need_s ? s.data_ptr() : nullptr, mean.data_ptr<float>(),
                            rstd.data_ptr<float>(), M, N, (float)eps, rms ? 1 : 0, (float)p_drop,
                            (uint64_t)seed, (uint64_t)offset, cur_stream());
  TORCH_CHECK(rc == 0, "layernorm_fwd: unsupported shape N=", N);
  return {y, s, mean, rstd};
}

// returns (ds, dx, dgamma, dbeta, dbias)
std::vector<at::Tensor> layernorm_bwd(at::Tensor dy, at::Tensor s, at::Tensor gamma, at::Tensor mean,
                                      at::Tensor rstd, c10::optional<at::Tensor> dextra, bool rms,
                                      bool has_beta, bool has_bias, bool need_dx, double p_drop,
                                      int64_t seed, int64_t offset) {
  CHECK_IN(dy); CHECK_BF16(dy); CHECK_IN(s); CHECK_BF16(s); CHECK_IN(gamma);
  const int N = s.size(-1);
  const int M = s.numel() / N;
  TORCH_CHECK(dy.numel() == s.numel());
  auto ds = at::empty_like(s);
  at::Tensor dx = need_dx ? at::empty_like(s) : at::Tensor();
  auto dgamma = at::empty_like(gamma);
  at::Tensor dbeta = has_beta ? at::empty_like(gamma) : at::Tensor();
  at::Tensor dbias = has_bias ? at::empty_like(gamma) : at::Tensor();
  const int grid = ct_layernorm_bwd_grid(M, N);
  auto part = at::empty({3 * (long)grid * N}, s.options().dtype(at::kFloat));
  int rc = ct_layernorm_bwd(dy.data_ptr(), s.data_ptr(), gamma.data_ptr(), mean.data_ptr<float>(),
                            rstd.data_ptr<float>(), optr(dextra), ds.data_ptr(),
                            need_dx ? dx.data_ptr() : nullptr, part.data_ptr<float>(),
                            dgamma.data_ptr(), has_beta ? dbeta.data_ptr() : nullptr,
                            has_bias ? dbias.data_ptr() : nullptr, M, N, rms ? 1 : 0,
                            gamma.scalar_type() == at::kFloat ? 1 : 0, 0, (float)p_drop,
                            (uint64_t)seed, (uint64_t)offset, cur_stream());
  TORCH_CHECK(rc == 0, "layernorm_bwd: unsupported shape N=", N);
  return {ds, dx, dgamma, dbeta, dbias};
}

// Same as layernorm_bwd but parameter grads are ACCUMULATED into caller-provided tensors
// (views of the flat gradient buffer) and the activation grads may go to given outputs.
// returns (ds, dx); dx is undefined when need_dx is false.
std::vector<at::Tensor> layernorm_bwd_into(at::Tensor dy, at::Tensor s, at::Tensor gamma,
                                           at::Tensor mean, at::Tensor rstd, bool rms,
                                           at::Tensor dgamma, c10::optional<at::Tensor> dbeta,
                                           c10::optional<at::Tensor> dbias, bool need_dx,
                                           double p_drop, int64_t seed, int64_t offset,
                                           c10::optional<at::Tensor> beta_y) {
  CHECK_IN(dy); CHECK_BF16(dy); CHECK_IN(s); CHECK_BF16(s); CHECK_IN(gamma); CHECK_IN(dgamma);
  const int N = s.size(-1);
  const int M = s.numel() / N;
  TORCH_CHECK(dy.numel() == s.numel() && dgamma.numel() == N);
  if (dbeta.has_value() && dbeta->defined()) { CHECK_IN(*dbeta); TORCH_CHECK(dbeta->numel() == N && dbeta->scalar_type() == dgamma.scalar_type()); }
  if (dbias.has_value() && dbias->defined()) { CHECK_IN(*dbias); TORCH_CHECK(dbias->numel() == N && dbias->scalar_type() == dgamma.scalar_type()); }
  auto ds = at::empty_like(s);
  at::Tensor dx = need_dx ? at::empty_like(s) : at::Tensor();
  const int grid = ct_layernorm_bwd_grid(M, N);
  auto part = at::empty({3 * (long)grid * N}, s.options().dtype(at::kFloat));
  // beta_y given: s is the forward's OUTPUT y (its keep_sum = false form), xhat = (y - beta) / gamma
  const bool from_y = beta_y.has_value() && beta_y->defined();
  if (from_y) { CHECK_IN(*beta_y); CHECK_BF16(*beta_y); CHECK_BF16(gamma); TORCH_CHECK(beta_y->numel() == N && !rms); }
  int rc = ct_layernorm_bwd2(dy.data_ptr(), s.data_ptr(), gamma.data_ptr(), mean.data_ptr<float>(),
                             rstd.data_ptr<float>(), nullptr, ds.data_ptr(),
                             need_dx ? dx.data_ptr() : nullptr, part.data_ptr<float>(),
                             dgamma.data_ptr(), optr_mut(dbeta), optr_mut(dbias), M, N, rms ? 1 : 0,
                             dgamma.scalar_type() == at::kFloat ? 1 : 0, 1, (float)p_drop,
                             (uint64_t)seed, (uint64_t)offset, from_y ? 1 : 0, optr(beta_y), cur_stream());
  TORCH_CHECK(rc == 0, "layernorm_bwd_into: unsupported shape N=", N);
  return {ds, dx};
}

// ---------------------------------------------------------------- bias + activation
at::Tensor bias_act_fwd(at::Tensor z, c10::optional<at::Tensor> bias, int64_t act) {
  CHECK_IN(z); CHECK_BF16(z);
  const int N = z.size(-1);
  auto y = at::empty_like(z);
  int rc = ct_bias_act_fwd(z.data_ptr(), optr(bias), y.data_ptr(), z.numel() / N, N, (int)act, cur_stream());
  TORCH_CHECK(rc == 0, "bias_act_fwd: N % 8 != 0");
  return y;
}

std::vector<at::Tensor> bias_act_bwd(at::Tensor dy, at::Tensor z, c10::optional<at::Tensor> bias,
                                     int64_t act, bool need_dbias) {
  CHECK_IN(dy); CHECK_IN(z); CHECK_BF16(z); CHECK_BF16(dy);
  const int N = z.size(-1);
  const long M = z.numel() / N;
  auto dz = at::empty_like(z);
  at::Tensor dbias, part;
  if (need_dbias) {
    dbias = at::empty({N}, z.options());
    part = at::empty({(long)ct_bias_act_bwd_grid(M) * N}, z.options().dtype(at::kFloat));
  }
  int rc = ct_bias_act_bwd(dy.data_ptr(), z.data_ptr(), optr(bias), dz.data_ptr(),
                           need_dbias ? part.data_ptr<float>() : nullptr,
                           need_dbias ? dbias.data_ptr() : nullptr, M, N, (int)act, 0, 0, cur_stream());
  TORCH_CHECK(rc == 0, "bias_act_bwd: N % 8 != 0");
  return {dz, dbias};
}

// dz = dy * act'(z + bias) (skipped when want_dz is false: pure bias-gradient reduction);
// d(bias) accumulated into `dbias` (a view of the flat gradient buffer).
at::Tensor bias_act_bwd_into(at::Tensor dy, at::Tensor z, c10::optional<at::Tensor> bias, int64_t act,
                             at::Tensor dbias, bool want_dz) {
  CHECK_IN(dy); CHECK_IN(z); CHECK_BF16(z); CHECK_BF16(dy); CHECK_IN(dbias);
  const int N = z.size(-1);
  const long M = z.numel() / N;
  TORCH_CHECK(dbias.numel() == N && dy.numel() == z.numel());
  at::Tensor dz = want_dz ? at::empty_like(z) : at::Tensor();
  auto part = at::empty({(long)ct_bias_act_bwd_grid(M) * N}, z.options().dtype(at::kFloat));
  int rc = ct_bias_act_bwd(dy.data_ptr(), z.data_ptr(), optr(bias), want_dz ? dz.data_ptr() : nullptr,
                           part.data_ptr<float>(), dbias.data_ptr(), M, N, (int)act,
                           dbias.scalar_type() == at::kFloat ? 1 : 0, 1, cur_stream());
  TORCH_CHECK(rc == 0, "bias_act_bwd_into: N % 8 != 0");
  return dz;
}

at::Tensor dropout_fwd(at::Tensor x, double p, int64_t seed, int64_t offset) {
  CHECK_IN(x); CHECK_BF16(x);
  auto y = at::empty_like(x);
  int rc = ct_dropout(x.data_ptr(), y.data_ptr(), x.numel(), (float)p, (uint64_t)seed, (uint64_t)offset, cur_stream());
  TORCH_CHECK(rc == 0, "dropout: numel % 8 != 0");
  return y;
}

// ---------------------------------------------------------------- embeddings
at::Tensor embed3_fwd(at::Tensor ids, c10::optional<at::Tensor> tt, at::Tensor W,
                      c10::optional<at::Tensor> P, c10::optional<at::Tensor> T) {
  CHECK_IN(ids); CHECK_IN(W); CHECK_BF16(W);
  TORCH_CHECK(ids.scalar_type() == at::kLong, "ids must be int64");
  TORCH_CHECK(ids.dim() == 2, "ids must be [B, S]");
  const int S = ids.size(1), N = W.size(1), ntok = ids.numel();
  if (P.has_value() && P->defined()) TORCH_CHECK(P->size(0) >= S && P->size(1) == N);
  if (tt.has_value() && tt->defined()) TORCH_CHECK(tt->numel() == ntok && tt->scalar_type() == at::kLong);
  auto out = at::empty({ids.size(0), S, N}, W.options());
  int rc = ct_embed3_fwd(ids.data_ptr<int64_t>(),
                         (tt.has_value() && tt->defined()) ? tt->data_ptr<int64_t>() : nullptr,
                         W.data_ptr(), optr(P), optr(T), out.data_ptr(), ntok, S, N, cur_stream());
  TORCH_CHECK(rc == 0, "embed3_fwd: N % 8 != 0");
  return out;
}

void embed3_bwd(at::Tensor ids, c10::optional<at::Tensor> tt, at::Tensor g,
                c10::optional<at::Tensor> dW, c10::optional<at::Tensor> dP,
                c10::optional<at::Tensor> dT) {
  CHECK_IN(ids); CHECK_IN(g); CHECK_BF16(g);
  const int S = ids.size(1), N = g.size(-1), ntok = ids.numel();
  TORCH_CHECK(ids.dim() == 2 && g.numel() == (int64_t)ntok * N, "embed3_bwd: g must be [ids.numel(), N]");
  if (tt.has_value() && tt->defined()) TORCH_CHECK(tt->numel() == ntok, "embed3_bwd: token types shape");
  if (dP.has_value() && dP->defined()) TORCH_CHECK(dP->size(0) >= S, "embed3_bwd: position table too short");
  for (auto* t : {&dW, &dP, &dT}) if (t->has_value() && (*t)->defined()) { CHECK_F32(**t); CHECK_IN(**t); TORCH_CHECK((*t)->size(1) == N); }
  ct_embed3_bwd(ids.data_ptr<int64_t>(), (tt.has_value() && tt->defined()) ? tt->data_ptr<int64_t>() : nullptr,
                g.data_ptr(), (float*)optr_mut(dW), (float*)optr_mut(dP), (float*)optr_mut(dT), ntok, S,
                N, (dT.has_value() && dT->defined()) ? (int)dT->size(0) : 0, cur_stream());
}

void cast_into(at::Tensor x, at::Tensor y, double scale, bool accumulate) {
  CHECK_IN(x); CHECK_IN(y);
  TORCH_CHECK(x.numel() == y.numel());
  ct_cast(x.data_ptr(), dt_code(x), y.data_ptr(), dt_code(y), x.numel(), (float)scale, accumulate ? 1 : 0, cur_stream());
}

// one (partials [S, ...] fp32, g bf16) pair of a split-K reduce entry
static void check_reduce_pair(const char* who, const at::Tensor& partials, const at::Tensor& g) {
  CHECK_IN(partials); CHECK_F32(partials); CHECK_IN(g); CHECK_BF16(g);
  TORCH_CHECK(partials.dim() >= 2 && partials[0].numel() == g.numel(), who, ": shape mismatch");
  TORCH_CHECK(g.numel() % 8 == 0, who, ": numel must be a multiple of 8");
}

void splitk_reduce(at::Tensor partials, at::Tensor g, bool accumulate) {
  check_reduce_pair("splitk_reduce", partials, g);
  TORCH_CHECK(ct_splitk_reduce(partials.data_ptr<float>(), (int)partials.size(0), g.numel(), g.data_ptr(),
                               accumulate ? 1 : 0, cur_stream()) == 0);
}

// two (partials, g) reductions in one launch (see ct_splitk_reduce2)
void splitk_reduce2(at::Tensor p1, at::Tensor g1, at::Tensor p2, at::Tensor g2, bool accumulate) {
  check_reduce_pair("splitk_reduce2", p1, g1);
  check_reduce_pair("splitk_reduce2", p2, g2);
  TORCH_CHECK(ct_splitk_reduce2(p1.data_ptr<float>(), (int)p1.size(0), g1.numel(), g1.data_ptr(),
                                p2.data_ptr<float>(), (int)p2.size(0), g2.numel(), g2.data_ptr(),
                                accumulate ? 1 : 0, cur_stream()) == 0);
}

// up to 4 (partials, g) reductions in one launch (see ct_splitk_reduce_group)
void splitk_reduce_group(std::vector<at::Tensor> partials, std::vector<at::Tensor> gs, bool accumulate) {
  const size_t n = partials.size();
  TORCH_CHECK(n >= 1 && n <= 4 && gs.size() == n, "splitk_reduce_group: 1..4 (partials, g) pairs");
  std::vector<const float*> P(n);
  std::vector<void*> g(n);
  std::vector<int> S(n);
  std::vector<long> len(n);
  for (size_t i = 0; i < n; ++i) {
    check_reduce_pair("splitk_reduce_group", partials[i], gs[i]);
    TORCH_CHECK(gs[i].numel() > 0, "splitk_reduce_group: empty tensor");
    P[i] = partials[i].data_ptr<float>();
    g[i] = gs[i].data_ptr();
    S[i] = (int)partials[i].size(0);
    len[i] = gs[i].numel();
  }
  TORCH_CHECK(ct_splitk_reduce_group((int)n, P.data(), S.data(), len.data(), g.data(), accumulate ? 1 : 0,
                                     cur_stream()) == 0, "splitk_reduce_group: misaligned tensor");
}

// splitk_reduce, and the partials are zeroed once read (persistent accumulation buffers)
void splitk_reduce_clear(at::Tensor partials, at::Tensor g, bool accumulate) {
  check_reduce_pair("splitk_reduce_clear", partials, g);
  TORCH_CHECK(ct_splitk_reduce_clear(partials.data_ptr<float>(), (int)partials.size(0), g.numel(), g.data_ptr(),
                                     accumulate ? 1 : 0, cur_stream()) == 0, "splitk_reduce_clear failed");
}

// ---------------------------------------------------------------- optimizers
void lamb_step(at::Tensor g, at::Tensor m, at::Tensor v, at::Tensor w, c10::optional<at::Tensor> w_model,
               at::Tensor seg_tensor, at::Tensor seg_start, at::Tensor seg_len, at::Tensor tensor_first_seg,
               at::Tensor tensor_wd, at::Tensor dyn, double beta1, double beta2, double eps,
               bool bias_corr, bool trust_all, at::Tensor seg_part, at::Tensor tensor_part, int64_t stage) {
  for (auto* t : {&g, &m, &v, &w, &seg_tensor, &seg_start, &seg_len, &tensor_first_seg, &tensor_wd, &dyn, &seg_part, &tensor_part}) CHECK_IN(*t);
  CHECK_F32(m); CHECK_F32(v); CHECK_F32(w);
  TORCH_CHECK(g.numel() >= w.numel() && m.numel() == w.numel() && v.numel() == w.numel());
  const int nseg = seg_len.numel(), T = tensor_wd.numel();
  TORCH_CHECK(seg_part.numel() >= 2 * nseg && tensor_part.numel() >= 2 * T && tensor_first_seg.numel() == T + 1);
  TORCH_CHECK(dyn.numel() >= 4, "lamb_step: dyn holds lr, grad scale and two bias corrections");
  int pdt = 0;
  if (w_model.has_value() && w_model->defined()) { CHECK_IN(*w_model); pdt = dt_code(*w_model); TORCH_CHECK(w_model->numel() >= w.numel()); }
  ct_lamb(g.data_ptr(), dt_code(g), m.data_ptr<float>(), v.data_ptr<float>(), w.data_ptr<float>(),
          optr_mut(w_model), pdt, seg_tensor.data_ptr<int>(), seg_start.data_ptr<int64_t>(),
          seg_len.data_ptr<int>(), nseg, tensor_first_seg.data_ptr<int>(), T,
          tensor_wd.data_ptr<float>(), dyn.data_ptr<float>(), (float)beta1, (float)beta2, (float)eps,
          bias_corr ? 1 : 0, trust_all ? 1 : 0, seg_part.data_ptr<float>(), tensor_part.data_ptr<float>(),
          (int)stage, cur_stream());
}

void adam_step(at::Tensor g, at::Tensor m, at::Tensor v, at::Tensor w, c10::optional<at::Tensor> w_model,
               at::Tensor seg_tensor, at::Tensor seg_start, at::Tensor seg_len, at::Tensor tensor_wd,
               at::Tensor dyn, double beta1, double beta2, double eps, bool adamw) {
  for (auto* t : {&g, &m, &v, &w, &seg_tensor, &seg_start, &seg_len, &tensor_wd, &dyn}) CHECK_IN(*t);
  CHECK_F32(m); CHECK_F32(v); CHECK_F32(w);
  TORCH_CHECK(g.numel() >= w.numel() && m.numel() == w.numel() && v.numel() == w.numel());
  TORCH_CHECK(dyn.numel() >= 4, "adam_step: dyn holds lr, grad scale and two bias corrections");
  int pdt = 0;
  if (w_model.has_value() && w_model->defined()) {
    CHECK_IN(*w_model); pdt = dt_code(*w_model);
    TORCH_CHECK(w_model->numel() >= w.numel(), "adam_step: w_model is shorter than w");
  }
  ct_adam(g.data_ptr(), dt_code(g), m.data_ptr<float>(), v.data_ptr<float>(), w.data_ptr<float>(),
          optr_mut(w_model), pdt, seg_tensor.data_ptr<int>(), seg_start.data_ptr<int64_t>(),
          seg_len.data_ptr<int>(), seg_len.numel(), tensor_wd.data_ptr<float>(), dyn.data_ptr<float>(),
          (float)beta1, (float)beta2, (float)eps, adamw ? 1 : 0, cur_stream());
}

void sgd_step(at::Tensor g, c10::optional<at::Tensor> buf, at::Tensor w, c10::optional<at::Tensor> w_model,
              at::Tensor seg_tensor, at::Tensor seg_start, at::Tensor seg_len, at::Tensor tensor_wd,
              at::Tensor dyn, double momentum, double dampening, bool nesterov) {
  for (auto* t : {&g, &w, &seg_tensor, &seg_start, &seg_len, &tensor_wd, &dyn}) CHECK_IN(*t);
  CHECK_F32(w);
  TORCH_CHECK(g.numel() >= w.numel());
  TORCH_CHECK(dyn.numel() >= 3, "sgd_step: dyn holds lr, grad scale and the first-step flag");
  if (momentum != 0.0) {
    TORCH_CHECK(buf.has_value() && buf->defined() && buf->numel() == w.numel(), "momentum buffer");
    CHECK_IN(*buf); CHECK_F32(*buf);
  }
  int pdt = 0;
  if (w_model.has_value() && w_model->defined()) {
    CHECK_IN(*w_model); pdt = dt_code(*w_model);
    TORCH_CHECK(w_model->numel() >= w.numel(), "sgd_step: w_model is shorter than w");
  }
  // momentum == 0: the kernel never touches buf
  ct_sgd(g.data_ptr(), dt_code(g), momentum != 0.0 ? (float*)optr_mut(buf) : nullptr, w.data_ptr<float>(),
         optr_mut(w_model), pdt, seg_tensor.data_ptr<int>(), seg_start.data_ptr<int64_t>(),
         seg_len.data_ptr<int>(), seg_len.numel(), tensor_wd.data_ptr<float>(), dyn.data_ptr<float>(),
         (float)momentum, (float)dampening, nesterov ? 1 : 0, cur_stream());
}

void sumsq_into(at::Tensor x, at::Tensor out) {
  CHECK_IN(x); CHECK_IN(out); CHECK_F32(out);
  TORCH_CHECK(x.numel() % 4 == 0, "sumsq: numel % 4");
  auto part = at::empty({2048}, out.options());
  ct_sumsq(x.data_ptr(), dt_code(x), x.numel(), out.data_ptr<float>(), part.data_ptr<float>(), cur_stream());
}

void clip_coef(at::Tensor sumsq, at::Tensor dyn, double base_scale, double max_norm) {
  CHECK_IN(sumsq); CHECK_IN(dyn); CHECK_F32(sumsq); CHECK_F32(dyn);
  TORCH_CHECK(sumsq.numel() >= 1 && dyn.numel() >= 4, "clip_coef: sumsq [1], dyn [>= 4]");
  ct_clip_coef(sumsq.data_ptr<float>(), dyn.data_ptr<float>(), (float)base_scale, (float)max_norm, cur_stream());
}

// ---------------------------------------------------------------- cross entropy
// logits [R, ld] bf16 (ld % 8 == 0); gradient written into `dlogits` (may be logits itself)
std::vector<at::Tensor> xent_fwd(at::Tensor logits, at::Tensor dlogits, int64_t V, at::Tensor labels,
                                 c10::optional<at::Tensor> scale, int64_t ignore_index,
                                 double label_smoothing) {
  CHECK_IN(logits); CHECK_BF16(logits); CHECK_IN(dlogits); CHECK_BF16(dlogits); CHECK_IN(labels);
  TORCH_CHECK(logits.dim() == 2 && dlogits.sizes() == logits.sizes());
  TORCH_CHECK(labels.scalar_type() == at::kLong && labels.numel() == logits.size(0));
  const int R = logits.size(0), ld = logits.size(1);
  TORCH_CHECK(V <= ld && ld % 8 == 0, "xent: ld must be a multiple of 8 and >= V");
  auto fo = logits.options().dtype(at::kFloat);
  auto loss = at::empty({R}, fo), lse = at::empty({R}, fo);
  const float* sp = nullptr;
  if (scale.has_value() && scale->defined()) { CHECK_F32(*scale); sp = scale->data_ptr<float>(); }
  ct_xent_fwd(logits.data_ptr(), dlogits.data_ptr(), ld, (int)V, labels.data_ptr<int64_t>(),
              loss.data_ptr<float>(), lse.data_ptr<float>(), sp, R, (int)ignore_index,
              (float)label_smoothing, cur_stream());
  return {loss, lse};
}

// ---------------------------------------------------------------- attention (head_dim 64 / 128)
// q, k, v, o: 4-D [B, S, H, D] views with unit stride on the last dim (e.g. slices of a
// packed [B, S, 3, H, D] QKV projection output); key_bias: fp32 [B, Sk] additive.
// attn_fwd takes D = 64, or D = 128 without dropout, and attn_bwd D = 64 (the entries of the packed
// BERT / GPT path and of ops.attention); the training pairs attn_fwd_train / attn_bwd_train and
// attn_fwd_relbias_train / attn_bwd_relbias take D = 64 or 128.  Every function fills one CtAttnCall (attention_api.h) through the helpers
// below, each tensor's pointer and strides together, and calls ct_attn_fwd or ct_attn_bwd.
static CtAttnView attn_view(const at::Tensor& t, const char* name, bool d128) {
  TORCH_CHECK(t.dim() == 4 && (t.size(3) == 64 || (d128 && t.size(3) == 128)) && t.stride(3) == 1, name,
              d128 ? " must be [B,S,H,64] or [B,S,H,128] with unit last stride"
                   : " must be [B,S,H,64] with unit last stride (head dim 128 is forward only through this entry: "
                     "attn_bwd_train / attn_bwd_relbias take it)");
  CHECK_CUDA(t); CHECK_BF16(t);
  return {t.data_ptr(), t.stride(0), t.stride(1), t.stride(2)};
}
// The views and sizes of a call: q, k, v, o (D = 128 allowed when d128) and, for a backward, their
// gradients dO, dq, dk, dv.  Everything else in the descriptor is left null / zero.
static CtAttnCall attn_call(const at::Tensor& q, const at::Tensor& k, const at::Tensor& v, const at::Tensor& o,
                            bool d128, const at::Tensor* dO = nullptr, const at::Tensor* dq = nullptr,
                            const at::Tensor* dk = nullptr, const at::Tensor* dv = nullptr) {
  CtAttnCall c{};
  c.q = attn_view(q, "q", d128); c.k = attn_view(k, "k", d128); c.v = attn_view(v, "v", d128); c.o = attn_view(o, "o", d128);
  if (dO) {
    c.dO = attn_view(*dO, "dO", d128); c.dq = attn_view(*dq, "dq", d128);
    c.dk = attn_view(*dk, "dk", d128); c.dv = attn_view(*dv, "dv", d128);
  }
  // the head dim the forward dispatches on: q, k, v and o must agree
  const long D = q.size(3);
  TORCH_CHECK(k.size(3) == D && v.size(3) == D && o.size(3) == D, "q, k, v and o must have the same head dim, got ",
              D, ", ", k.size(3), ", ", v.size(3), ", ", o.size(3));
  if (dO) {
    TORCH_CHECK(dO->sizes() == o.sizes() && dq->sizes() == q.sizes() && dk->sizes() == k.sizes() && dv->sizes() == v.sizes());
  }
  c.B = q.size(0); c.Sq = q.size(1); c.H = q.size(2); c.Sk = k.size(1); c.D = (int)D;
  TORCH_CHECK(k.size(0) == c.B && v.size(0) == c.B && k.size(2) == c.H && v.size(2) == c.H && v.size(1) == c.Sk);
  TORCH_CHECK(o.size(0) == c.B && o.size(1) == c.Sq && o.size(2) == c.H);
  return c;
}
static void key_bias_checked(const c10::optional<at::Tensor>& key_bias, CtAttnCall& c) {
  if (!(key_bias.has_value() && key_bias->defined())) return;
  CHECK_F32(*key_bias); CHECK_CUDA(*key_bias);
  TORCH_CHECK(key_bias->dim() == 2 && key_bias->size(0) == c.B && key_bias->size(1) == c.Sk && key_bias->stride(1) == 1);
  c.kbias = key_bias->data_ptr<float>(); c.kb_sb = key_bias->stride(0);
}
// T5-style relative-position bias vector relb [H, L]; returns L
static long relb_checked(const at::Tensor& relb, int64_t rel_base, CtAttnCall& c) {
  CHECK_F32(relb); CHECK_CUDA(relb);
  TORCH_CHECK(relb.dim() == 2 && relb.size(0) == c.H && (relb.stride(1) == 1 || relb.size(1) == 1),
              "relb must be [H, L] fp32");
  const long L = relb.size(1);
  TORCH_CHECK(rel_base >= c.Sq - 1 && rel_base + c.Sk <= L, "relb does not cover every (key - query) offset");
  c.relb = relb.data_ptr<float>(); c.relb_sh = relb.stride(0); c.rel_base = (int)rel_base;
  c.relb_len = (int)std::min<long>(L, 1 << 20);   // past the limit either way: the entry answers rc=-4
  return L;
}
// the kernels read lse as a dense fp32 [B*H, Sq]
static void lse_checked(const at::Tensor& lse, CtAttnCall& c) {
  CHECK_F32(lse); CHECK_CUDA(lse);
  TORCH_CHECK(lse.is_contiguous() && lse.numel() == (long)c.B * c.H * c.Sq, "lse must be contiguous fp32 [B*H, Sq]");
  c.lse = lse.data_ptr<float>();
}
static void attn_params(CtAttnCall& c, double scale, double p, int64_t seed, int64_t offset, bool causal) {
  c.scale = (float)scale; c.p_drop = (float)p; c.seed = (uint64_t)seed; c.offset = (uint64_t)offset;
  c.causal = causal ? 1 : 0;
}
// allocates lse, runs the forward; returns lse
static at::Tensor attn_fwd_run(CtAttnCall& c, const at::Tensor& q, const char* who) {
  auto lse = at::empty({(long)c.B * c.H, c.Sq}, q.options().dtype(at::kFloat));
  c.lse = lse.data_ptr<float>();
  int rc = ct_attn_fwd(&c, cur_stream());
  TORCH_CHECK(rc == 0, who, c.D == 128 ? " (head dim 128)" : "", " failed rc=", rc);
  return lse;
}

at::Tensor attn_fwd(at::Tensor q, at::Tensor k, at::Tensor v, at::Tensor o,
                    c10::optional<at::Tensor> key_bias, double scale, double p, int64_t seed,
                    int64_t offset, bool causal) {
  CtAttnCall c = attn_call(q, k, v, o, true);
  key_bias_checked(key_bias, c);
  TORCH_CHECK(c.D == 64 || p == 0.0, "attn_fwd: head dim 128 has no dropout through this entry (p must be 0; "
              "attn_fwd_train / attn_fwd_relbias_train take p > 0)");
  // D = 128: no dropout stream, so no seed either
  attn_params(c, scale, p, c.D == 64 ? seed : 0, c.D == 64 ? offset : 0, causal);
  return attn_fwd_run(c, q, "attn_fwd");
}

// inference forward with a T5-style relative-position bias vector relb [H, L]
at::Tensor attn_fwd_relbias(at::Tensor q, at::Tensor k, at::Tensor v, at::Tensor o,
                            c10::optional<at::Tensor> key_bias, at::Tensor relb, int64_t rel_base, double scale,
                            bool causal) {
  CtAttnCall c = attn_call(q, k, v, o, true);
  relb_checked(relb, rel_base, c);
  key_bias_checked(key_bias, c);
  attn_params(c, scale, 0.0, 0, 0, causal);
  return attn_fwd_run(c, q, "attn_fwd_relbias");
}

void attn_bwd(at::Tensor q, at::Tensor k, at::Tensor v, at::Tensor o, at::Tensor dO, at::Tensor dq,
              at::Tensor dk, at::Tensor dv, c10::optional<at::Tensor> key_bias, at::Tensor lse,
              double scale, double p, int64_t seed, int64_t offset, bool causal) {
  CtAttnCall c = attn_call(q, k, v, o, false, &dO, &dq, &dk, &dv);
  lse_checked(lse, c);
  key_bias_checked(key_bias, c);
  attn_params(c, scale, p, seed, offset, causal);
  auto fo = q.options().dtype(at::kFloat);
  auto delta = at::empty({(long)c.B * c.H * c.Sq}, fo);
  at::Tensor dq_acc;
  if (c.Sk > 128) dq_acc = at::empty({(long)c.B * c.H * c.Sq * 64}, fo);
  c.delta = delta.data_ptr<float>();
  c.dq_acc = c.Sk > 128 ? dq_acc.data_ptr<float>() : nullptr;
  int rc = ct_attn_bwd(&c, cur_stream());
  TORCH_CHECK(rc == 0, "attn_bwd failed rc=", rc);
}

// ---- relative-bias attention for training (T5, head dim 64 or 128): forward with dropout + lse,
// and a backward that also returns the gradient of the bias vector
at::Tensor attn_fwd_relbias_train(at::Tensor q, at::Tensor k, at::Tensor v, at::Tensor o,
                                  c10::optional<at::Tensor> key_bias, at::Tensor relb, int64_t rel_base,
                                  double scale, double p, int64_t seed, int64_t offset, bool causal) {
  CtAttnCall c = attn_call(q, k, v, o, true);
  relb_checked(relb, rel_base, c);
  key_bias_checked(key_bias, c);
  attn_params(c, scale, p, seed, offset, causal);
  return attn_fwd_run(c, q, "attn_fwd_relbias_train");
}

// d_rel: fp32 [H, L] in any strides (the gradient in the layout of the caller's bias view); every
// entry is written.  rc=-9: Sq too long for the kernel's LDS windows (callers fall back).
void attn_bwd_relbias(at::Tensor q, at::Tensor k, at::Tensor v, at::Tensor o, at::Tensor dO, at::Tensor dq,
                      at::Tensor dk, at::Tensor dv, at::Tensor d_rel, c10::optional<at::Tensor> key_bias,
                      at::Tensor relb, int64_t rel_base, at::Tensor lse, double scale, double p, int64_t seed,
                      int64_t offset, bool causal) {
  CtAttnCall c = attn_call(q, k, v, o, true, &dO, &dq, &dk, &dv);
  lse_checked(lse, c);
  const long L = relb_checked(relb, rel_base, c);
  key_bias_checked(key_bias, c);
  attn_params(c, scale, p, seed, offset, causal);
  CHECK_F32(d_rel); CHECK_CUDA(d_rel);
  TORCH_CHECK(d_rel.dim() == 2 && d_rel.size(0) == c.H && d_rel.size(1) == L, "d_rel must be fp32 [H, L] like relb");
  TORCH_CHECK(L <= 1 || c.H <= 1 || (d_rel.stride(0) != 0 && d_rel.stride(1) != 0), "d_rel must not be an expanded view");
  c.d_rel = d_rel.data_ptr<float>(); c.d_sh = d_rel.stride(0); c.d_si = d_rel.stride(1);
  auto fo = q.options().dtype(at::kFloat);
  const int nkb = (c.Sk + 127) / 128;
  const long W = ct_attn_bwd_relbias_window(c.Sq);
  at::Tensor dq_acc, ws;
  // the C entry refuses a longer L and windows past the LDS budget before it touches a workspace
  const bool sized = L <= kCtAttnRelBiasMax && W <= ct_attn_bwd_relbias_max_window_d(c.D);
  if (c.Sk > 128 && sized) dq_acc = at::empty({(long)c.B * c.H * c.Sq * c.D}, fo);
  ws = at::empty({sized ? (long)c.B * nkb * c.H * W : 1L}, fo);
  c.dq_acc = dq_acc.defined() ? dq_acc.data_ptr<float>() : nullptr;
  c.drel_ws = ws.data_ptr<float>();
  int rc = ct_attn_bwd(&c, cur_stream());
  TORCH_CHECK(rc == 0, "attn_bwd_relbias failed rc=", rc);
}

// ---- attention without a bias vector for training, head dim 64 or 128 (T5 cross-attention at
// d_kv = 128; at 64 the kernels of attn_fwd / attn_bwd): forward with dropout + lse, and the backward
at::Tensor attn_fwd_train(at::Tensor q, at::Tensor k, at::Tensor v, at::Tensor o,
                          c10::optional<at::Tensor> key_bias, double scale, double p, int64_t seed,
                          int64_t offset, bool causal) {
  CtAttnCall c = attn_call(q, k, v, o, true);
  key_bias_checked(key_bias, c);
  attn_params(c, scale, p, seed, offset, causal);
  return attn_fwd_run(c, q, "attn_fwd_train");
}

void attn_bwd_train(at::Tensor q, at::Tensor k, at::Tensor v, at::Tensor o, at::Tensor dO, at::Tensor dq,
                    at::Tensor dk, at::Tensor dv, c10::optional<at::Tensor> key_bias, at::Tensor lse,
                    double scale, double p, int64_t seed, int64_t offset, bool causal) {
  CtAttnCall c = attn_call(q, k, v, o, true, &dO, &dq, &dk, &dv);
  lse_checked(lse, c);
  key_bias_checked(key_bias, c);
  attn_params(c, scale, p, seed, offset, causal);
  at::Tensor dq_acc;
  if (c.Sk > 128) dq_acc = at::empty({(long)c.B * c.H * c.Sq * c.D}, q.options().dtype(at::kFloat));
  c.dq_acc = dq_acc.defined() ? dq_acc.data_ptr<float>() : nullptr;
  int rc = ct_attn_bwd(&c, cur_stream());
  TORCH_CHECK(rc == 0, "attn_bwd_train failed rc=", rc);
}

void register_ext(pybind11::module& m);   // bindings_ext.cpp
void register_graph(pybind11::module& m); // bindings_graph.cpp
void register_deform(pybind11::module& m); // bindings_deform.cpp
void register_p2p(pybind11::module& m);    // bindings_p2p.cpp
void register_lt(pybind11::module& m);     // bindings_lt.cpp
void register_conv(pybind11::module& m);   // bindings_conv.cpp
void register_quant(pybind11::module& m);  // bindings_quant.cpp
void register_beam(pybind11::module& m);   // bindings_beam.cpp
void register_sampling(pybind11::module& m); // bindings_sampling.cpp
void register_constrain(pybind11::module& m); // bindings_constrain.cpp
void register_quant_skinny(pybind11::module& m); // bindings_quant_skinny.cpp
void register_bn(pybind11::module& m);     // bindings_bn.cpp
void register_gated_act(pybind11::module& m); // bindings_gated_act.cpp

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "cloudtik_amd CDNA4 (gfx950) op library";
  register_ext(m);
  register_graph(m);
  register_deform(m);
  register_p2p(m);
  register_lt(m);
  register_conv(m);
  register_quant(m);
  register_beam(m);
  register_sampling(m);
  register_constrain(m);
  register_quant_skinny(m);
  register_bn(m);
  register_gated_act(m);
  m.def("layernorm_fwd", &layernorm_fwd, pybind11::arg("x"), pybind11::arg("bias"), pybind11::arg("res"),
        pybind11::arg("gamma"), pybind11::arg("beta"), pybind11::arg("eps"), pybind11::arg("rms"),
        pybind11::arg("p_drop"), pybind11::arg("seed"), pybind11::arg("offset"), pybind11::arg("keep_sum") = true);
  m.def("layernorm_bwd", &layernorm_bwd);
  m.def("bias_act_fwd", &bias_act_fwd);
  m.def("bias_act_bwd", &bias_act_bwd);
  m.def("bias_act_bwd_into", &bias_act_bwd_into);
  m.def("layernorm_bwd_into", &layernorm_bwd_into, pybind11::arg("dy"), pybind11::arg("s"), pybind11::arg("gamma"),
        pybind11::arg("mean"), pybind11::arg("rstd"), pybind11::arg("rms"), pybind11::arg("dgamma"),
        pybind11::arg("dbeta"), pybind11::arg("dbias"), pybind11::arg("need_dx"), pybind11::arg("p_drop"),
        pybind11::arg("seed"), pybind11::arg("offset"), pybind11::arg("beta_y") = pybind11::none());
  m.def("dropout_fwd", &dropout_fwd);
  m.def("embed3_fwd", &embed3_fwd);
  m.def("embed3_bwd", &embed3_bwd);
  m.def("cast_into", &cast_into);
  m.def("splitk_reduce", &splitk_reduce);
  m.def("splitk_reduce_clear", &splitk_reduce_clear);
  m.def("splitk_reduce2", &splitk_reduce2);
  m.def("splitk_reduce_group", &splitk_reduce_group);
  m.def("lamb_step", &lamb_step);
  m.def("adam_step", &adam_step);
  m.def("sgd_step", &sgd_step);
  m.def("sumsq_into", &sumsq_into);
  m.def("clip_coef", &clip_coef);
  m.def("xent_fwd", &xent_fwd);
  m.def("attn_fwd_relbias", &attn_fwd_relbias);
  m.def("attn_fwd", &attn_fwd);
  m.def("attn_bwd", &attn_bwd);
  m.def("attn_fwd_relbias_train", &attn_fwd_relbias_train);
  m.def("attn_bwd_relbias", &attn_bwd_relbias);
  m.def("attn_bwd_relbias_window", [](int64_t Sq) { return (int64_t)ct_attn_bwd_relbias_window((int)Sq); });
  m.def("attn_bwd_relbias_max_window", []() { return (int64_t)ct_attn_bwd_relbias_max_window(); });
  m.def("attn_bwd_relbias_max_window_d", [](int64_t D) { return (int64_t)ct_attn_bwd_relbias_max_window_d((int)D); });
  m.def("attn_fwd_train", &attn_fwd_train);
  m.def("attn_bwd_train", &attn_bwd_train);
}
