// Binding for the token-ban kernel (constrain.hip).  Every shape, dtype, stride and device the
// kernel relies on is checked here; a violated one raises and nothing is launched.  Nothing here
// reads device memory, allocates or synchronises, so the call can be captured into a graph.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <hip/hip_runtime.h>

extern "C" {
int ct_constrain_max_steps();
int ct_constrain_max_words();
int ct_constrain_max_word_tokens();
int ct_logits_constrain(void*, int, const long*, const long*, const int*, const int*, float*, int, int, int, int, int,
                        int, int, int, int, hipStream_t);
}

namespace {

static_assert(sizeof(long) == 8, "int64 tensors are passed as long");

void check(const at::Tensor& t, const char* name, at::ScalarType dt, at::IntArrayRef shape, const at::Tensor& like) {
  TORCH_CHECK(t.is_cuda() && t.is_contiguous(), "logits_constrain: ", name, " must be a contiguous GPU tensor");
  TORCH_CHECK(t.device() == like.device(), "logits_constrain: ", name, " must be on the device of logits");
  TORCH_CHECK(t.scalar_type() == dt, "logits_constrain: ", name, " must be ", dt, ", got ", t.scalar_type());
  TORCH_CHECK(t.sizes() == shape, "logits_constrain: ", name, " must have shape ", shape, ", got ", t.sizes());
}

// The rule of ops/constrain.py, in place on logits [R, V]; ban_lse fp32 [R] is written when given.
void logits_constrain(at::Tensor logits, at::Tensor hist, at::Tensor pos, int64_t start_token, int64_t n,
                      int64_t min_new, int64_t eos, c10::optional<at::Tensor> word_tok,
                      c10::optional<at::Tensor> word_off, c10::optional<at::Tensor> ban_lse) {
  TORCH_CHECK(logits.is_cuda() && logits.dim() == 2, "logits_constrain: logits must be a 2-D GPU tensor");
  TORCH_CHECK(logits.scalar_type() == at::kBFloat16 || logits.scalar_type() == at::kFloat,
              "logits_constrain: logits must be bf16 or fp32, got ", logits.scalar_type());
  const int64_t R = logits.size(0), V = logits.size(1);
  TORCH_CHECK(R >= 1 && R <= INT32_MAX, "logits_constrain: logits row count out of range");
  TORCH_CHECK(V >= 1 && V <= (1 << 27), "logits_constrain: logits must hold 1 .. 2^27 tokens a row, got ", V);
  TORCH_CHECK(logits.stride(1) == 1 && logits.stride(0) == V && logits.is_contiguous(),
              "logits_constrain: logits must be contiguous");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(logits.data_ptr()) % logits.element_size() == 0,
              "logits_constrain: logits must be element-aligned");
  TORCH_CHECK(hist.dim() == 2, "logits_constrain: hist must be [R, T]");
  const int64_t T = hist.size(1);
  TORCH_CHECK(T >= 1 && T <= ct_constrain_max_steps(), "logits_constrain: hist must hold 1 .. ",
              ct_constrain_max_steps(), " steps, got ", T);
  check(hist, "hist", at::kLong, {R, T}, logits);
  check(pos, "pos", at::kLong, {1}, logits);
  TORCH_CHECK(start_token >= 0 && start_token < V, "logits_constrain: start_token must be a token of the row, got ",
              start_token);
  TORCH_CHECK(n >= 0 && n <= INT32_MAX, "logits_constrain: n must be >= 0, got ", n);
  TORCH_CHECK(min_new >= 0 && min_new <= INT32_MAX, "logits_constrain: min_new must be >= 0, got ", min_new);
  TORCH_CHECK(eos >= INT32_MIN && eos <= INT32_MAX, "logits_constrain: eos must fit 32 bits");
  TORCH_CHECK(word_tok.has_value() == word_off.has_value(),
              "logits_constrain: word_tok and word_off come together");
  const int* wtok = nullptr;
  const int* woff = nullptr;
  int64_t n_words = 0, n_wtok = 0;
  if (word_tok.has_value()) {
    TORCH_CHECK(word_tok->dim() == 1 && word_off->dim() == 1, "logits_constrain: the word tables must be 1-D");
    n_wtok = word_tok->size(0);
    n_words = word_off->size(0) - 1;
    TORCH_CHECK(n_words >= 1 && n_words <= ct_constrain_max_words(), "logits_constrain: 1 .. ",
                ct_constrain_max_words(), " words are supported, got ", n_words);
    TORCH_CHECK(n_wtok >= n_words && n_wtok <= ct_constrain_max_word_tokens(), "logits_constrain: the words may hold ",
                ct_constrain_max_word_tokens(), " tokens in all and one each at least, got ", n_wtok);
    check(*word_tok, "word_tok", at::kInt, {n_wtok}, logits);
    check(*word_off, "word_off", at::kInt, {n_words + 1}, logits);
    wtok = word_tok->data_ptr<int>();
    woff = word_off->data_ptr<int>();
  }
  float* lse = nullptr;
  if (ban_lse.has_value()) {
    check(*ban_lse, "ban_lse", at::kFloat, {R}, logits);
    lse = ban_lse->data_ptr<float>();
  }
  int rc = ct_logits_constrain(logits.data_ptr(), logits.scalar_type() == at::kBFloat16, (const long*)hist.data_ptr(),
                               (const long*)pos.data_ptr(), wtok, woff, lse, (int)R, (int)V, (int)T, (int)start_token,
                               (int)n, (int)min_new, (int)eos, (int)n_words, (int)n_wtok,
                               at::hip::getCurrentHIPStream().stream());
  TORCH_CHECK(rc == 0, "ct_logits_constrain failed: ", rc);
}

}  // namespace

void register_constrain(pybind11::module& m) {
  m.def("logits_constrain", &logits_constrain, pybind11::arg("logits"), pybind11::arg("hist"), pybind11::arg("pos"),
        pybind11::arg("start_token"), pybind11::arg("n"), pybind11::arg("min_new"), pybind11::arg("eos"),
        pybind11::arg("word_tok") = pybind11::none(), pybind11::arg("word_off") = pybind11::none(),
        pybind11::arg("ban_lse") = pybind11::none());
  m.def("constrain_caps", []() {
    return std::make_tuple(ct_constrain_max_steps(), ct_constrain_max_words(), ct_constrain_max_word_tokens());
  });
}
