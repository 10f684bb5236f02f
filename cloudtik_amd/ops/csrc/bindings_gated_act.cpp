// Bindings for the gated-GELU kernels (gated_act.hip).  Every dtype, shape, stride and alignment
// the kernels rely on is checked here; a violated one raises and nothing is launched.  Nothing here
// reads device memory or synchronises, so the calls can be captured into a graph.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <hip/hip_runtime.h>

extern "C" {
int ct_gated_gelu_fwd(const void*, const void*, void*, long, int, long, long, float, uint64_t, uint64_t, hipStream_t);
int ct_gated_gelu_bwd(const void*, const void*, const void*, void*, void*, long, int, long, long, float, uint64_t,
                      uint64_t, hipStream_t);
}

namespace {

// `t` as M rows of F bf16 elements; returns the row stride in elements
int64_t rows_of(const at::Tensor& t, const char* name, int64_t M, int64_t F, const at::Tensor& like) {
  TORCH_CHECK(t.is_cuda() && t.device() == like.device(), "gated_gelu: ", name, " must be a GPU tensor on one device");
  TORCH_CHECK(t.scalar_type() == at::kBFloat16, "gated_gelu: ", name, " must be bf16, got ", t.scalar_type());
  TORCH_CHECK(t.dim() == 2 && t.size(0) == M && t.size(1) == F, "gated_gelu: ", name, " must be [", M, ", ", F,
              "], got ", t.sizes());
  TORCH_CHECK(F == 1 || t.stride(1) == 1, "gated_gelu: the last dimension of ", name, " must be contiguous");
  const int64_t stride = M > 1 ? t.stride(0) : F;
  TORCH_CHECK(stride >= F && stride % 8 == 0, "gated_gelu: the row stride of ", name,
              " must be a multiple of 8 elements and at least F, got ", stride);
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0, "gated_gelu: ", name,
              " must start at a 16-byte-aligned address");
  const int64_t end = t.storage_offset() + (M > 0 ? (M - 1) * stride + F : 0);
  TORCH_CHECK(end * 2 <= (int64_t)t.storage().nbytes(), "gated_gelu: ", name, " reaches beyond its storage");
  return stride;
}

void shape_of(const at::Tensor& g, int64_t& M, int64_t& F) {
  TORCH_CHECK(g.dim() == 2, "gated_gelu: g must be [M, F]");
  M = g.size(0);
  F = g.size(1);
  TORCH_CHECK(F >= 8 && F % 8 == 0 && F <= INT32_MAX, "gated_gelu: F must be a positive multiple of 8, got ", F);
}

// h [M, F] contiguous = dropout_p(gelu_tanh(g) * u), the keep bits of (seed, offset)
at::Tensor gated_gelu_fwd(at::Tensor g, at::Tensor u, double p, int64_t seed, int64_t offset) {
  int64_t M, F;
  shape_of(g, M, F);
  TORCH_CHECK(p >= 0.0 && p < 1.0, "gated_gelu: p must be in [0, 1), got ", p);
  const int64_t gs = rows_of(g, "g", M, F, g), us = rows_of(u, "u", M, F, g);
  auto h = at::empty({M, F}, g.options());
  int rc = ct_gated_gelu_fwd(g.data_ptr(), u.data_ptr(), h.data_ptr(), M, (int)F, gs, us, (float)p, (uint64_t)seed,
                             (uint64_t)offset, at::hip::getCurrentHIPStream().stream());
  TORCH_CHECK(rc == 0, "ct_gated_gelu_fwd refused its arguments");
  return h;
}

// (dg, du) [M, F] contiguous from dh [M, F] contiguous and the forward's g, u, (p, seed, offset)
std::vector<at::Tensor> gated_gelu_bwd(at::Tensor dh, at::Tensor g, at::Tensor u, double p, int64_t seed,
                                       int64_t offset) {
  int64_t M, F;
  shape_of(g, M, F);
  TORCH_CHECK(p >= 0.0 && p < 1.0, "gated_gelu: p must be in [0, 1), got ", p);
  const int64_t gs = rows_of(g, "g", M, F, g), us = rows_of(u, "u", M, F, g);
  TORCH_CHECK(dh.is_contiguous(), "gated_gelu: dh must be contiguous");
  rows_of(dh, "dh", M, F, g);
  auto dg = at::empty({M, F}, g.options()), du = at::empty({M, F}, g.options());
  int rc = ct_gated_gelu_bwd(dh.data_ptr(), g.data_ptr(), u.data_ptr(), dg.data_ptr(), du.data_ptr(), M, (int)F, gs, us,
                             (float)p, (uint64_t)seed, (uint64_t)offset, at::hip::getCurrentHIPStream().stream());
  TORCH_CHECK(rc == 0, "ct_gated_gelu_bwd refused its arguments");
  return {dg, du};
}

}  // namespace

void register_gated_act(pybind11::module& m) {
  m.def("gated_gelu_fwd", &gated_gelu_fwd, pybind11::arg("g"), pybind11::arg("u"), pybind11::arg("p"),
        pybind11::arg("seed"), pybind11::arg("offset"));
  m.def("gated_gelu_bwd", &gated_gelu_bwd, pybind11::arg("dh"), pybind11::arg("g"), pybind11::arg("u"),
        pybind11::arg("p"), pybind11::arg("seed"), pybind11::arg("offset"));
}
