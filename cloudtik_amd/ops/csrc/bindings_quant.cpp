// Bindings for the int8 quantization kernels (quant.hip, quant_conv.hip).  Every constraint the kernels rely
// on (dtype, contiguity, 16-byte alignment, K / N multiples, K range, matching sizes) is
// checked here; a violated one raises and nothing is launched.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <hip/hip_runtime.h>
#include <cmath>

extern "C" {
int ct_quant_rows_i8(const void*, void*, float*, int, int, hipStream_t);
int ct_gemm_i8_nt(const void*, const void*, const float*, const float*, const void*, void*, int, int, int, int,
                  hipStream_t);
int ct_quant_static_i8(const void*, void*, long, float, hipStream_t);
int ct_layernorm_quant_i8(const void*, const void*, const void*, const void*, const void*, void*, void*, int, int,
                          float, float, hipStream_t);
int ct_gemm_i8_nt_static(const void*, const void*, float, const float*, const void*, void*, int, int, int, int, int,
                         float, hipStream_t);
int ct_conv_i8_fwd(const void*, const void*, const float*, const float*, const void*, void*, int, int, int, int, int,
                   int, int, int, float, float, float, int, int, hipStream_t);
}

namespace {

#define QCHECK(x) TORCH_CHECK((x).is_cuda() && (x).is_contiguous(), #x " must be a contiguous GPU tensor")
#define QDT(x, d, name) TORCH_CHECK((x).scalar_type() == (d), #x " must be " name)
#define QALIGN(x) TORCH_CHECK(reinterpret_cast<uintptr_t>((x).data_ptr()) % 16 == 0, #x " must be 16-byte aligned")

hipStream_t stream() { return at::hip::getCurrentHIPStream().stream(); }

// x bf16 [..., K] -> (q int8 [..., K], scale fp32 [...])
std::vector<at::Tensor> quant_rows_i8(at::Tensor x) {
  QCHECK(x); QDT(x, at::kBFloat16, "bf16"); QALIGN(x);
  TORCH_CHECK(x.dim() >= 1 && x.numel() > 0, "quant_rows_i8: empty input");
  const int64_t K = x.size(-1), M = x.numel() / K;
  TORCH_CHECK(K % 16 == 0 && K <= 8192, "quant_rows_i8: K must be a multiple of 16 and <= 8192, got ", K);
  TORCH_CHECK(M <= INT32_MAX, "quant_rows_i8: too many rows");
  auto q = at::empty(x.sizes(), x.options().dtype(at::kChar));
  auto lead = x.sizes().vec();
  lead.pop_back();
  auto scale = at::empty(lead, x.options().dtype(at::kFloat));
  int rc = ct_quant_rows_i8(x.data_ptr(), q.data_ptr(), scale.data_ptr<float>(), (int)M, (int)K, stream());
  TORCH_CHECK(rc == 0, "ct_quant_rows_i8 failed: ", rc);
  return {q, scale};
}

// shapes of an NT int8 product: a_q [M, K], w_q [N, K], out [M, N]
void check_operands(const at::Tensor& a_q, const at::Tensor& w_q, const at::Tensor& out, int64_t& M, int64_t& N,
                    int64_t& K) {
  QCHECK(a_q); QCHECK(w_q); QCHECK(out);
  QDT(a_q, at::kChar, "int8"); QDT(w_q, at::kChar, "int8");
  QALIGN(a_q); QALIGN(w_q); QALIGN(out);
  TORCH_CHECK(a_q.dim() == 2 && w_q.dim() == 2 && out.dim() == 2, "gemm_i8_nt: operands must be 2-D");
  M = a_q.size(0); K = a_q.size(1); N = w_q.size(0);
  TORCH_CHECK(w_q.size(1) == K, "gemm_i8_nt: a_q [M, K] and w_q [N, K] disagree on K");
  TORCH_CHECK(out.size(0) == M && out.size(1) == N, "gemm_i8_nt: out must be [M, N]");
  TORCH_CHECK(M >= 1 && M <= 65535 * 128, "gemm_i8_nt: M out of range");
  TORCH_CHECK(K >= 64 && K % 64 == 0 && K <= 8192, "gemm_i8_nt: K must be a multiple of 64 and <= 8192, got ", K);
  TORCH_CHECK(N >= 64 && N % 64 == 0, "gemm_i8_nt: N must be a multiple of 64, got ", N);
  TORCH_CHECK(M * N <= (int64_t)INT32_MAX * 64, "gemm_i8_nt: output too large");
}

// out bf16 [M, N] = act((a_q . w_q^T) * a_scale[m] * w_scale[n] + bias[n]); act 0 none, 1 GELU
void gemm_i8_nt(at::Tensor a_q, at::Tensor a_scale, at::Tensor w_q, at::Tensor w_scale,
                c10::optional<at::Tensor> bias, int64_t act, at::Tensor out) {
  int64_t M, N, K;
  check_operands(a_q, w_q, out, M, N, K);
  QDT(out, at::kBFloat16, "bf16");
  QCHECK(a_scale); QCHECK(w_scale);
  QDT(a_scale, at::kFloat, "fp32"); QDT(w_scale, at::kFloat, "fp32");
  QALIGN(w_scale);
  TORCH_CHECK(a_scale.numel() == M && w_scale.numel() == N, "gemm_i8_nt: scales must be [M] and [N]");
  TORCH_CHECK(act == 0 || act == 1, "gemm_i8_nt: act must be 0 (none) or 1 (GELU)");
  const void* b = nullptr;
  if (bias.has_value() && bias->defined()) {
    QCHECK(*bias); QDT(*bias, at::kBFloat16, "bf16");
    TORCH_CHECK(bias->numel() == N, "gemm_i8_nt: bias must be [N]");
    TORCH_CHECK(reinterpret_cast<uintptr_t>(bias->data_ptr()) % 8 == 0, "bias must be 8-byte aligned");
    b = bias->data_ptr();
  }
  int rc = ct_gemm_i8_nt(a_q.data_ptr(), w_q.data_ptr(), a_scale.data_ptr<float>(), w_scale.data_ptr<float>(), b,
                         out.data_ptr(), (int)M, (int)N, (int)K, (int)act, stream());
  TORCH_CHECK(rc == 0, "ct_gemm_i8_nt failed: ", rc);
}

// out int32 [M, N] = a_q . w_q^T, the exact accumulators
void gemm_i8_nt_raw(at::Tensor a_q, at::Tensor w_q, at::Tensor out) {
  int64_t M, N, K;
  check_operands(a_q, w_q, out, M, N, K);
  QDT(out, at::kInt, "int32");
  int rc = ct_gemm_i8_nt(a_q.data_ptr(), w_q.data_ptr(), nullptr, nullptr, nullptr, out.data_ptr(), (int)M, (int)N,
                         (int)K, 2, stream());
  TORCH_CHECK(rc == 0, "ct_gemm_i8_nt failed: ", rc);
}

// ------------------------------------------------------------------ static quantization
// A by-value scale / inverse scale computed on the host from a calibrated range: finite, >= 0,
// and exactly representable in fp32 (the kernels take a float).
float checked_factor(double v, const char* name) {
  TORCH_CHECK(std::isfinite(v) && v >= 0.0, name, " must be finite and non-negative, got ", v);
  TORCH_CHECK((double)(float)v == v, name, " must be an fp32 value, got ", v);
  return (float)v;
}

const void* optional_bf16(const c10::optional<at::Tensor>& t, int64_t numel, size_t align, const char* name) {
  if (!t.has_value() || !t->defined()) return nullptr;
  TORCH_CHECK(t->is_cuda() && t->is_contiguous(), name, " must be a contiguous GPU tensor");
  TORCH_CHECK(t->scalar_type() == at::kBFloat16, name, " must be bf16");
  TORCH_CHECK(t->numel() == numel, name, " has the wrong size");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t->data_ptr()) % align == 0, name, " must be ", align, "-byte aligned");
  return t->data_ptr();
}

// x bf16 [...] -> q int8 [...], q = clamp(rne(x * inv), -127, 127)
at::Tensor quant_static_i8(at::Tensor x, double inv) {
  QCHECK(x); QDT(x, at::kBFloat16, "bf16"); QALIGN(x);
  const float finv = checked_factor(inv, "quant_static_i8: inv");
  const int64_t n = x.numel();
  TORCH_CHECK(n > 0, "quant_static_i8: empty input");
  TORCH_CHECK(n % 16 == 0 && n / 16 <= INT32_MAX, "quant_static_i8: the element count must be a multiple of 16, got ",
              n);
  auto q = at::empty(x.sizes(), x.options().dtype(at::kChar));
  int rc = ct_quant_static_i8(x.data_ptr(), q.data_ptr(), (long)n, finv, stream());
  TORCH_CHECK(rc == 0, "ct_quant_static_i8 failed: ", rc);
  return q;
}

// (y bf16, q int8 or None) = LN(res + (x + bias)) * gamma + beta and its quantization with inv;
// emit_q false writes y alone
std::vector<c10::optional<at::Tensor>> layernorm_quant_i8(at::Tensor x, c10::optional<at::Tensor> bias,
                                                          c10::optional<at::Tensor> res, at::Tensor gamma,
                                                          c10::optional<at::Tensor> beta, double eps, double inv,
                                                          bool emit_q) {
  QCHECK(x); QDT(x, at::kBFloat16, "bf16"); QALIGN(x);
  TORCH_CHECK(x.dim() >= 1 && x.numel() > 0, "layernorm_quant_i8: empty input");
  const int64_t N = x.size(-1), M = x.numel() / N;
  TORCH_CHECK(N % 8 == 0 && N <= 2048, "layernorm_quant_i8: N must be a multiple of 8 and <= 2048, got ", N);
  TORCH_CHECK(M <= INT32_MAX, "layernorm_quant_i8: too many rows");
  TORCH_CHECK(std::isfinite(eps) && eps >= 0.0, "layernorm_quant_i8: eps must be finite and non-negative");
  const float finv = checked_factor(inv, "layernorm_quant_i8: inv");
  const void* g = optional_bf16(gamma, N, 16, "gamma");
  const void* bi = optional_bf16(bias, N, 16, "bias");
  const void* be = optional_bf16(beta, N, 16, "beta");
  const void* r = optional_bf16(res, x.numel(), 16, "residual");
  auto y = at::empty_like(x);
  c10::optional<at::Tensor> q;
  if (emit_q) q = at::empty(x.sizes(), x.options().dtype(at::kChar));
  int rc = ct_layernorm_quant_i8(x.data_ptr(), bi, r, g, be, y.data_ptr(), emit_q ? q->data_ptr() : nullptr, (int)M,
                                 (int)N, (float)eps, finv, stream());
  TORCH_CHECK(rc == 0, "ct_layernorm_quant_i8 failed: ", rc);
  return {y, q};
}

// out [M, N] = act((a_q . w_q^T) * a_scale * w_scale[n] + bias[n]) with ONE activation scale; a bf16
// out takes the result, an int8 out its quantization with out_inv
void gemm_i8_nt_static(at::Tensor a_q, double a_scale, at::Tensor w_q, at::Tensor w_scale,
                       c10::optional<at::Tensor> bias, int64_t act, at::Tensor out, double out_inv) {
  int64_t M, N, K;
  check_operands(a_q, w_q, out, M, N, K);
  const bool i8 = out.scalar_type() == at::kChar;
  TORCH_CHECK(i8 || out.scalar_type() == at::kBFloat16, "gemm_i8_nt_static: out must be bf16 or int8");
  QCHECK(w_scale); QDT(w_scale, at::kFloat, "fp32"); QALIGN(w_scale);
  TORCH_CHECK(w_scale.numel() == N, "gemm_i8_nt_static: w_scale must be [N]");
  TORCH_CHECK(act == 0 || act == 1, "gemm_i8_nt_static: act must be 0 (none) or 1 (GELU)");
  const float sa = checked_factor(a_scale, "gemm_i8_nt_static: a_scale");
  const float inv = checked_factor(out_inv, "gemm_i8_nt_static: out_inv");
  const void* b = optional_bf16(bias, N, 8, "bias");
  int rc = ct_gemm_i8_nt_static(a_q.data_ptr(), w_q.data_ptr(), sa, w_scale.data_ptr<float>(), b, out.data_ptr(),
                                (int)M, (int)N, (int)K, (int)act, i8 ? 1 : 0, inv, stream());
  TORCH_CHECK(rc == 0, "ct_gemm_i8_nt_static failed: ", rc);
}

// ------------------------------------------------------------------ int8 convolution
#define QCL(x) TORCH_CHECK((x).is_cuda() && (x).dim() == 4 && (x).is_contiguous(at::MemoryFormat::ChannelsLast), \
                           #x " must be a 4-D channels_last GPU tensor")

// out [N, Co, Ho, Wo] = act(conv(x_q, w_q) * a_scale * w_scale[co] + bias[co] + res_q * res_scale), all
// image tensors channels_last; a bf16 out takes the result, an int8 out its quantization with out_inv.
// w_q [Co, R*R*Ci] has tap-major rows.
void conv2d_i8_static(at::Tensor x_q, double a_scale, at::Tensor w_q, at::Tensor w_scale, at::Tensor bias,
                      int64_t stride, int64_t padding, bool relu, c10::optional<at::Tensor> res_q, double res_scale,
                      at::Tensor out, double out_inv) {
  QCL(x_q); QCL(out); QCHECK(w_q); QCHECK(w_scale); QCHECK(bias);
  QDT(x_q, at::kChar, "int8"); QDT(w_q, at::kChar, "int8");
  QDT(w_scale, at::kFloat, "fp32"); QDT(bias, at::kFloat, "fp32");
  QALIGN(x_q); QALIGN(w_q); QALIGN(out); QALIGN(w_scale); QALIGN(bias);
  const bool i8 = out.scalar_type() == at::kChar;
  TORCH_CHECK(i8 || out.scalar_type() == at::kBFloat16, "conv2d_i8_static: out must be bf16 or int8");
  const int64_t N = x_q.size(0), Ci = x_q.size(1), H = x_q.size(2), W = x_q.size(3);
  TORCH_CHECK(x_q.numel() > 0, "conv2d_i8_static: empty input");
  TORCH_CHECK(w_q.dim() == 2, "conv2d_i8_static: w_q must be [Co, R*R*Ci]");
  const int64_t Co = w_q.size(0), K = w_q.size(1);
  TORCH_CHECK(Ci % 64 == 0 && Co >= 64 && Co % 64 == 0,
              "conv2d_i8_static: Ci and Co must be multiples of 64, got ", Ci, " and ", Co);
  TORCH_CHECK(K == Ci || K == 9 * Ci, "conv2d_i8_static: the filter must be 1x1 or 3x3 over all ", Ci,
              " input channels (groups = 1), got rows of ", K);
  const int64_t R = K == Ci ? 1 : 3;
  TORCH_CHECK(K <= 32768, "conv2d_i8_static: R*S*Ci must be <= 32768, got ", K);
  TORCH_CHECK(stride == 1 || stride == 2, "conv2d_i8_static: stride must be 1 or 2, got ", stride);
  TORCH_CHECK(padding == R / 2, "conv2d_i8_static: padding must be R / 2 = ", R / 2, ", got ", padding);
  TORCH_CHECK(w_scale.numel() == Co && bias.numel() == Co, "conv2d_i8_static: w_scale and bias must be [Co]");
  const int64_t Ho = (H + 2 * padding - R) / stride + 1, Wo = (W + 2 * padding - R) / stride + 1;
  TORCH_CHECK(out.size(0) == N && out.size(1) == Co && out.size(2) == Ho && out.size(3) == Wo,
              "conv2d_i8_static: out must be [", N, ", ", Co, ", ", Ho, ", ", Wo, "]");
  TORCH_CHECK(N * Ho * Wo <= 65535 * 128 && N * H * W <= INT32_MAX, "conv2d_i8_static: too many pixels");
  const float sa = checked_factor(a_scale, "conv2d_i8_static: a_scale");
  const float sr = checked_factor(res_scale, "conv2d_i8_static: res_scale");
  const float inv = checked_factor(out_inv, "conv2d_i8_static: out_inv");
  const void* r = nullptr;
  if (res_q.has_value() && res_q->defined()) {
    QCL(*res_q); QDT(*res_q, at::kChar, "int8"); QALIGN(*res_q);
    TORCH_CHECK(res_q->sizes() == out.sizes(), "conv2d_i8_static: the residual must have the output's shape");
    r = res_q->data_ptr();
  }
  int rc = ct_conv_i8_fwd(x_q.data_ptr(), w_q.data_ptr(), w_scale.data_ptr<float>(), bias.data_ptr<float>(), r,
                          out.data_ptr(), (int)N, (int)H, (int)W, (int)Ci, (int)Co, (int)R, (int)stride, (int)padding,
                          sa, sr, inv, relu ? 1 : 0, i8 ? 1 : 0, stream());
  TORCH_CHECK(rc == 0, "ct_conv_i8_fwd failed: ", rc);
}

}  // namespace

void register_quant(pybind11::module& m) {
  m.def("quant_static_i8", &quant_static_i8, pybind11::arg("x"), pybind11::arg("inv"));
  m.def("layernorm_quant_i8", &layernorm_quant_i8, pybind11::arg("x"), pybind11::arg("bias"),
        pybind11::arg("residual"), pybind11::arg("gamma"), pybind11::arg("beta"), pybind11::arg("eps"),
        pybind11::arg("inv"), pybind11::arg("emit_q"));
  m.def("gemm_i8_nt_static", &gemm_i8_nt_static, pybind11::arg("a_q"), pybind11::arg("a_scale"),
        pybind11::arg("w_q"), pybind11::arg("w_scale"), pybind11::arg("bias"), pybind11::arg("act"),
        pybind11::arg("out"), pybind11::arg("out_inv"));
  m.def("conv2d_i8_static", &conv2d_i8_static, pybind11::arg("x_q"), pybind11::arg("a_scale"), pybind11::arg("w_q"),
        pybind11::arg("w_scale"), pybind11::arg("bias"), pybind11::arg("stride"), pybind11::arg("padding"),
        pybind11::arg("relu"), pybind11::arg("res_q"), pybind11::arg("res_scale"), pybind11::arg("out"),
        pybind11::arg("out_inv"));
  m.def("quant_rows_i8", &quant_rows_i8);
  m.def("gemm_i8_nt", &gemm_i8_nt, pybind11::arg("a_q"), pybind11::arg("a_scale"), pybind11::arg("w_q"),
        pybind11::arg("w_scale"), pybind11::arg("bias"), pybind11::arg("act"), pybind11::arg("out"));
  m.def("gemm_i8_nt_raw", &gemm_i8_nt_raw);
}
