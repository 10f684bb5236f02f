// Binding for the sampling kernel (sampling.hip).  Every shape, dtype, stride, alignment and
// device the kernel relies on is checked here; a violated one raises and nothing is launched.
// Nothing here reads device memory or synchronises, so the call can be captured into a graph.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <hip/hip_runtime.h>

#include <cmath>

extern "C" {
int ct_sample_capacity();
int ct_sample_step(const void*, int, float*, long*, uint8_t*, long*, long*, const long*, const float*, float*, float*,
                   int*, int, int, int, int, int, int, float, int, float, float, hipStream_t);
}

namespace {

static_assert(sizeof(long) == 8, "int64 tensors are passed as long");

void check(const at::Tensor& t, const char* name, at::ScalarType dt, at::IntArrayRef shape, const at::Tensor& like) {
  TORCH_CHECK(t.is_cuda() && t.is_contiguous(), "sample_step: ", name, " must be a contiguous GPU tensor");
  TORCH_CHECK(t.device() == like.device(), "sample_step: ", name, " must be on the device of logits");
  TORCH_CHECK(t.scalar_type() == dt, "sample_step: ", name, " must be ", dt, ", got ", t.scalar_type());
  TORCH_CHECK(t.sizes() == shape, "sample_step: ", name, " must have shape ", shape, ", got ", t.sizes());
}

// One step of the rule in ops/sampling.py, in place on out / done / cur / pos; returns the row
// diagnostics (u fp32 [R], thr fp32 [R], n_keep int32 [R]).
std::vector<at::Tensor> sample_step(at::Tensor logits, at::Tensor out, at::Tensor done, at::Tensor cur, at::Tensor pos,
                                    at::Tensor seed, int64_t start_token, int64_t eos, int64_t pad,
                                    double temperature, int64_t top_k, double top_p, double repetition_penalty,
                                    c10::optional<at::Tensor> u) {
  TORCH_CHECK(logits.is_cuda() && logits.dim() == 2, "sample_step: logits must be a 2-D GPU tensor");
  TORCH_CHECK(logits.scalar_type() == at::kBFloat16 || logits.scalar_type() == at::kFloat,
              "sample_step: logits must be bf16 or fp32, got ", logits.scalar_type());
  const int64_t R = logits.size(0), V = logits.size(1);
  TORCH_CHECK(R >= 1 && R <= INT32_MAX, "sample_step: logits row count out of range");
  TORCH_CHECK(V >= 1 && V <= (1 << 27), "sample_step: logits must hold 1 .. 2^27 tokens a row, got ", V);
  TORCH_CHECK(logits.stride(1) == 1 && logits.stride(0) == V && logits.is_contiguous(),
              "sample_step: logits must be contiguous");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(logits.data_ptr()) % logits.element_size() == 0,
              "sample_step: logits must be element-aligned");
  TORCH_CHECK(out.dim() == 2, "sample_step: out must be [R, T]");
  const int64_t T = out.size(1);
  TORCH_CHECK(T >= 1 && T <= INT32_MAX, "sample_step: out step count out of range");
  check(out, "out", at::kLong, {R, T}, logits);
  check(done, "done", at::kBool, {R}, logits);
  check(cur, "cur", at::kLong, {R, 1}, logits);
  check(pos, "pos", at::kLong, {1}, logits);
  check(seed, "seed", at::kLong, {1}, logits);
  const float* u_in = nullptr;
  if (u.has_value()) {
    check(*u, "u", at::kFloat, {R}, logits);
    u_in = u->data_ptr<float>();
  }
  TORCH_CHECK(start_token >= 0 && start_token < V, "sample_step: start_token must be a token of the row, got ", start_token);
  TORCH_CHECK(eos >= INT32_MIN && eos <= INT32_MAX && pad >= INT32_MIN && pad <= INT32_MAX,
              "sample_step: eos and pad must fit 32 bits");
  TORCH_CHECK(std::isfinite(temperature) && temperature > 0 && (float)temperature > 0.f && std::isfinite((float)temperature),
              "sample_step: temperature must be finite and > 0, got ", temperature);
  TORCH_CHECK(std::isfinite(repetition_penalty) && repetition_penalty > 0 && (float)repetition_penalty > 0.f &&
                  std::isfinite((float)repetition_penalty),
              "sample_step: repetition_penalty must be finite and > 0, got ", repetition_penalty);
  TORCH_CHECK(top_p > 0 && top_p <= 1 && (float)top_p > 0.f, "sample_step: top_p must be in (0, 1], got ", top_p);
  TORCH_CHECK(top_k >= 0, "sample_step: top_k must be >= 0, got ", top_k);
  const int k = (int)std::min<int64_t>(top_k, V);                // any top_k >= V is off
  auto f32 = logits.options().dtype(at::kFloat);
  auto u_out = at::empty({R}, f32);
  auto thr = at::empty({R}, f32);
  auto n_keep = at::empty({R}, logits.options().dtype(at::kInt));
  at::Tensor ws;                                                  // rows beyond the on-chip capacity
  if (V > ct_sample_capacity()) ws = at::empty({R, V}, f32);
  int rc = ct_sample_step(logits.data_ptr(), logits.scalar_type() == at::kBFloat16,
                          ws.defined() ? ws.data_ptr<float>() : nullptr, (long*)out.data_ptr(),
                          (uint8_t*)done.data_ptr(), (long*)cur.data_ptr(), (long*)pos.data_ptr(),
                          (const long*)seed.data_ptr(), u_in, u_out.data_ptr<float>(), thr.data_ptr<float>(),
                          n_keep.data_ptr<int>(), (int)R, (int)V, (int)T, (int)start_token, (int)eos, (int)pad,
                          (float)temperature, k, (float)top_p, (float)repetition_penalty,
                          at::hip::getCurrentHIPStream().stream());
  TORCH_CHECK(rc == 0, "ct_sample_step failed: ", rc);
  return {u_out, thr, n_keep};
}

}  // namespace

void register_sampling(pybind11::module& m) {
  m.def("sample_step", &sample_step, pybind11::arg("logits"), pybind11::arg("out"), pybind11::arg("done"),
        pybind11::arg("cur"), pybind11::arg("pos"), pybind11::arg("seed"), pybind11::arg("start_token"),
        pybind11::arg("eos"), pybind11::arg("pad"), pybind11::arg("temperature"), pybind11::arg("top_k"),
        pybind11::arg("top_p"), pybind11::arg("repetition_penalty"), pybind11::arg("u") = pybind11::none());
}
