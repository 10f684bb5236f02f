// Bindings for the int8 decode kernels (quant_skinny.hip).  Every constraint the kernels rely on
// (dtype, contiguity, 16-byte alignment, M / K / N ranges and multiples, matching sizes) is
// checked here; a violated one raises and nothing is launched.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <hip/hip_runtime.h>
#include <cmath>

extern "C" {
int ct_rmsnorm_quant_rows(const void*, const void*, const void*, void*, void*, float*, int, int, float, hipStream_t);
int ct_gemm_i8_skinny(const void*, const void*, const float*, const float*, const void*, const void*, void*, int, int,
                      int, int, int, hipStream_t);
}

namespace {

#define SCHECK(x) TORCH_CHECK((x).is_cuda() && (x).is_contiguous(), #x " must be a contiguous GPU tensor")
#define SDT(x, d, name) TORCH_CHECK((x).scalar_type() == (d), #x " must be " name)
#define SALIGN(x) TORCH_CHECK(reinterpret_cast<uintptr_t>((x).data_ptr()) % 16 == 0, #x " must be 16-byte aligned")

hipStream_t stream() { return at::hip::getCurrentHIPStream().stream(); }

// (y bf16 or None, q int8, scale fp32 [...]) = RMSNorm(x + residual) * gamma and its row quantization
std::vector<c10::optional<at::Tensor>> rmsnorm_quant_rows(at::Tensor x, c10::optional<at::Tensor> residual,
                                                          at::Tensor gamma, double eps, bool emit_y) {
  SCHECK(x); SDT(x, at::kBFloat16, "bf16"); SALIGN(x);
  SCHECK(gamma); SDT(gamma, at::kBFloat16, "bf16"); SALIGN(gamma);
  TORCH_CHECK(x.dim() >= 1 && x.numel() > 0, "rmsnorm_quant_rows: empty input");
  const int64_t N = x.size(-1), M = x.numel() / N;
  TORCH_CHECK(N % 16 == 0 && N <= 2048, "rmsnorm_quant_rows: N must be a multiple of 16 and <= 2048, got ", N);
  TORCH_CHECK(M <= INT32_MAX, "rmsnorm_quant_rows: too many rows");
  TORCH_CHECK(gamma.numel() == N, "rmsnorm_quant_rows: gamma must be [N]");
  TORCH_CHECK(std::isfinite(eps) && eps >= 0.0, "rmsnorm_quant_rows: eps must be finite and non-negative");
  const void* r = nullptr;
  if (residual.has_value() && residual->defined()) {
    SCHECK(*residual); SDT(*residual, at::kBFloat16, "bf16"); SALIGN(*residual);
    TORCH_CHECK(residual->sizes() == x.sizes(), "rmsnorm_quant_rows: the residual must have x's shape");
    r = residual->data_ptr();
  }
  c10::optional<at::Tensor> y;
  if (emit_y) y = at::empty_like(x);
  auto q = at::empty(x.sizes(), x.options().dtype(at::kChar));
  auto lead = x.sizes().vec();
  lead.pop_back();
  auto scale = at::empty(lead, x.options().dtype(at::kFloat));
  int rc = ct_rmsnorm_quant_rows(x.data_ptr(), r, gamma.data_ptr(), emit_y ? y->data_ptr() : nullptr, q.data_ptr(),
                                 scale.data_ptr<float>(), (int)M, (int)N, (float)eps, stream());
  TORCH_CHECK(rc == 0, "ct_rmsnorm_quant_rows failed: ", rc);
  return {y, q, scale};
}

// shapes of a skinny NT int8 product: a_q [M <= 64, K], w_q [N, K], out [M, N]
void check_skinny(const at::Tensor& a_q, const at::Tensor& w_q, const at::Tensor& out, int64_t& M, int64_t& N,
                  int64_t& K) {
  SCHECK(a_q); SCHECK(w_q); SCHECK(out);
  SDT(a_q, at::kChar, "int8"); SDT(w_q, at::kChar, "int8");
  SALIGN(a_q); SALIGN(w_q); SALIGN(out);
  TORCH_CHECK(a_q.dim() == 2 && w_q.dim() == 2 && out.dim() == 2, "gemm_i8_skinny: operands must be 2-D");
  M = a_q.size(0); K = a_q.size(1); N = w_q.size(0);
  TORCH_CHECK(w_q.size(1) == K, "gemm_i8_skinny: a_q [M, K] and w_q [N, K] disagree on K");
  TORCH_CHECK(out.size(0) == M && out.size(1) == N, "gemm_i8_skinny: out must be [M, N]");
  TORCH_CHECK(M >= 1 && M <= 64, "gemm_i8_skinny: M must be in 1 .. 64, got ", M,
              " (larger products belong to gemm_i8_nt)");
  TORCH_CHECK(K >= 64 && K % 64 == 0 && K <= 8192, "gemm_i8_skinny: K must be a multiple of 64 and <= 8192, got ", K);
  TORCH_CHECK(N >= 64 && N % 64 == 0 && N <= INT32_MAX / 64, "gemm_i8_skinny: N must be a multiple of 64, got ", N);
}

// out bf16 [M, N] = act((a_q . w_q^T) * a_scale[m] * w_scale[n] + bias[n]) (+ residual); act 0 none,
// 2 ReLU.  out may be the residual.
void gemm_i8_skinny(at::Tensor a_q, at::Tensor a_scale, at::Tensor w_q, at::Tensor w_scale,
                    c10::optional<at::Tensor> bias, int64_t act, c10::optional<at::Tensor> residual, at::Tensor out) {
  int64_t M, N, K;
  check_skinny(a_q, w_q, out, M, N, K);
  SDT(out, at::kBFloat16, "bf16");
  SCHECK(a_scale); SCHECK(w_scale);
  SDT(a_scale, at::kFloat, "fp32"); SDT(w_scale, at::kFloat, "fp32");
  SALIGN(w_scale);
  TORCH_CHECK(a_scale.numel() == M && w_scale.numel() == N, "gemm_i8_skinny: scales must be [M] and [N]");
  TORCH_CHECK(act == 0 || act == 2, "gemm_i8_skinny: act must be 0 (none) or 2 (ReLU)");
  const void* b = nullptr;
  if (bias.has_value() && bias->defined()) {
    SCHECK(*bias); SDT(*bias, at::kBFloat16, "bf16");
    TORCH_CHECK(bias->numel() == N, "gemm_i8_skinny: bias must be [N]");
    TORCH_CHECK(reinterpret_cast<uintptr_t>(bias->data_ptr()) % 8 == 0, "bias must be 8-byte aligned");
    b = bias->data_ptr();
  }
  const void* r = nullptr;
  if (residual.has_value() && residual->defined()) {
    SCHECK(*residual); SDT(*residual, at::kBFloat16, "bf16"); SALIGN(*residual);
    TORCH_CHECK(residual->dim() == 2 && residual->size(0) == M && residual->size(1) == N,
                "gemm_i8_skinny: the residual must be [M, N]");
    r = residual->data_ptr();
    // the same tensor or a disjoint one: a lane reads exactly the elements it then writes
    const char* r0 = static_cast<const char*>(r);
    const char* o0 = static_cast<const char*>(out.data_ptr());
    const int64_t bytes = M * N * 2;
    TORCH_CHECK(r0 == o0 || r0 + bytes <= o0 || o0 + bytes <= r0,
                "gemm_i8_skinny: out must be the residual itself or not overlap it");
  }
  int rc = ct_gemm_i8_skinny(a_q.data_ptr(), w_q.data_ptr(), a_scale.data_ptr<float>(), w_scale.data_ptr<float>(), b,
                             r, out.data_ptr(), (int)M, (int)N, (int)K, (int)act, 0, stream());
  TORCH_CHECK(rc == 0, "ct_gemm_i8_skinny failed: ", rc);
}

// out int32 [M, N] = a_q . w_q^T, the exact accumulators
void gemm_i8_skinny_raw(at::Tensor a_q, at::Tensor w_q, at::Tensor out) {
  int64_t M, N, K;
  check_skinny(a_q, w_q, out, M, N, K);
  SDT(out, at::kInt, "int32");
  int rc = ct_gemm_i8_skinny(a_q.data_ptr(), w_q.data_ptr(), nullptr, nullptr, nullptr, nullptr, out.data_ptr(),
                             (int)M, (int)N, (int)K, 0, 1, stream());
  TORCH_CHECK(rc == 0, "ct_gemm_i8_skinny failed: ", rc);
}

}  // namespace

void register_quant_skinny(pybind11::module& m) {
  m.def("rmsnorm_quant_rows", &rmsnorm_quant_rows, pybind11::arg("x"), pybind11::arg("residual"),
        pybind11::arg("gamma"), pybind11::arg("eps"), pybind11::arg("emit_y"));
  m.def("gemm_i8_skinny", &gemm_i8_skinny, pybind11::arg("a_q"), pybind11::arg("a_scale"), pybind11::arg("w_q"),
        pybind11::arg("w_scale"), pybind11::arg("bias"), pybind11::arg("act"), pybind11::arg("residual"),
        pybind11::arg("out"));
  m.def("gemm_i8_skinny_raw", &gemm_i8_skinny_raw);
}
