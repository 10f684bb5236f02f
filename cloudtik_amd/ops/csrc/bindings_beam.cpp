// Bindings for the beam-search kernels (beam.hip).  Every shape, dtype, stride and alignment the
// kernels rely on is checked here; a violated one raises and nothing is launched.  Nothing here
// reads device memory or synchronises, so the calls can be captured into a graph.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <hip/hip_runtime.h>

extern "C" {
int ct_beam_topk(const void*, int, float*, float*, int*, int, int, int, hipStream_t);
int ct_beam_update(const float*, const float*, const int*, long*, float*, long*, float*, uint8_t*, uint8_t*,
                   const float*, long*, unsigned*, long*, long*, float*, long*, int, int, int, int, int, int,
                   hipStream_t);
int ct_cache_reorder(const long*, int, const long*, const long*, int, int, int, hipStream_t);
}

namespace {

static_assert(sizeof(long) == 8, "int64 tensors are passed as long");

hipStream_t stream() { return at::hip::getCurrentHIPStream().stream(); }

void check(const at::Tensor& t, const char* name, at::ScalarType dt, at::IntArrayRef shape) {
  TORCH_CHECK(t.is_cuda() && t.is_contiguous(), name, " must be a contiguous GPU tensor");
  TORCH_CHECK(t.scalar_type() == dt, name, " must be ", dt, ", got ", t.scalar_type());
  TORCH_CHECK(t.sizes() == shape, name, " must have shape ", shape, ", got ", t.sizes());
}

// logits [R, V] bf16 | fp32 -> (lse fp32 [R], top_val fp32 [R, 2K], top_tok int32 [R, 2K])
std::vector<at::Tensor> beam_topk(at::Tensor logits, int64_t num_beams) {
  TORCH_CHECK(logits.is_cuda() && logits.dim() == 2, "beam_topk: logits must be a 2-D GPU tensor");
  TORCH_CHECK(logits.scalar_type() == at::kBFloat16 || logits.scalar_type() == at::kFloat,
              "beam_topk: logits must be bf16 or fp32, got ", logits.scalar_type());
  TORCH_CHECK(num_beams >= 1 && num_beams <= 8, "beam_topk: num_beams must be in 1..8, got ", num_beams);
  const int64_t R = logits.size(0), V = logits.size(1), k2 = 2 * num_beams;
  TORCH_CHECK(R >= 1 && R <= INT32_MAX, "beam_topk: row count out of range");
  TORCH_CHECK(V >= k2 && V <= (1 << 27), "beam_topk: the vocabulary must hold 2 * num_beams .. 2^27 tokens, got ", V);
  TORCH_CHECK(logits.stride(1) == 1 && logits.stride(0) == V, "beam_topk: logits must be contiguous");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(logits.data_ptr()) % logits.element_size() == 0,
              "beam_topk: logits must be element-aligned");
  auto f32 = logits.options().dtype(at::kFloat);
  auto lse = at::empty({R}, f32);
  auto val = at::empty({R, k2}, f32);
  auto tok = at::empty({R, k2}, logits.options().dtype(at::kInt));
  int rc = ct_beam_topk(logits.data_ptr(), logits.scalar_type() == at::kBFloat16, lse.data_ptr<float>(),
                        val.data_ptr<float>(), tok.data_ptr<int>(), (int)R, (int)V, (int)k2, stream());
  TORCH_CHECK(rc == 0, "ct_beam_topk failed: ", rc);
  return {lse, val, tok};
}

// One step of the rules in ops/beam.py on the device state; returns (cand_score fp32 [B, 2K],
// cand_idx int64 [B, 2K]), the step's candidates in rank order (idx = beam * V + token).
std::vector<at::Tensor> beam_update(at::Tensor lse, at::Tensor top_val, at::Tensor top_tok, at::Tensor run_seq,
                                    at::Tensor run_score, at::Tensor fin_seq, at::Tensor fin_score,
                                    at::Tensor fin_flag, at::Tensor unsat, at::Tensor len_pen, at::Tensor pos,
                                    at::Tensor arrive, at::Tensor beam_idx, at::Tensor cur, int64_t vocab,
                                    int64_t eos, bool early_stopping) {
  TORCH_CHECK(run_seq.dim() == 3, "beam_update: run_seq must be [B, K, T]");
  const int64_t B = run_seq.size(0), K = run_seq.size(1), T = run_seq.size(2), k2 = 2 * K;
  TORCH_CHECK(B >= 1 && B <= 65535 * 64, "beam_update: batch out of range");
  TORCH_CHECK(K >= 1 && K <= 8, "beam_update: num_beams must be in 1..8, got ", K);
  TORCH_CHECK(T >= 1 && T <= INT32_MAX, "beam_update: step count out of range");
  TORCH_CHECK(vocab >= k2 && vocab <= (1 << 27), "beam_update: vocab must be in 2 * num_beams .. 2^27");
  TORCH_CHECK(B * K <= INT32_MAX / 16, "beam_update: too many rows");
  check(lse, "lse", at::kFloat, {B * K});
  check(top_val, "top_val", at::kFloat, {B * K, k2});
  check(top_tok, "top_tok", at::kInt, {B * K, k2});
  check(run_seq, "run_seq", at::kLong, {B, K, T});
  check(fin_seq, "fin_seq", at::kLong, {B, K, T});
  check(run_score, "run_score", at::kFloat, {B, K});
  check(fin_score, "fin_score", at::kFloat, {B, K});
  check(fin_flag, "fin_flag", at::kBool, {B, K});
  check(unsat, "unsat", at::kBool, {B});
  check(len_pen, "len_pen", at::kFloat, {T});
  check(pos, "pos", at::kLong, {1});
  check(arrive, "arrive", at::kInt, {1});
  check(beam_idx, "beam_idx", at::kLong, {B * K});
  check(cur, "cur", at::kLong, {B * K, 1});
  for (const at::Tensor* t : {&lse, &top_val, &top_tok, &fin_seq, &run_score, &fin_score, &fin_flag, &unsat, &len_pen,
                              &pos, &arrive, &beam_idx, &cur})
    TORCH_CHECK(t->device() == run_seq.device(), "beam_update: every tensor must be on run_seq's device");
  auto cand_score = at::empty({B, k2}, lse.options());
  auto cand_idx = at::empty({B, k2}, lse.options().dtype(at::kLong));
  int rc = ct_beam_update(lse.data_ptr<float>(), top_val.data_ptr<float>(), top_tok.data_ptr<int>(),
                          (long*)run_seq.data_ptr(), run_score.data_ptr<float>(), (long*)fin_seq.data_ptr(),
                          fin_score.data_ptr<float>(), (uint8_t*)fin_flag.data_ptr(), (uint8_t*)unsat.data_ptr(),
                          len_pen.data_ptr<float>(), (long*)pos.data_ptr(), (unsigned*)arrive.data_ptr(),
                          (long*)beam_idx.data_ptr(), (long*)cur.data_ptr(), cand_score.data_ptr<float>(),
                          (long*)cand_idx.data_ptr(), (int)B, (int)K, (int)vocab, (int)T, (int)eos,
                          early_stopping ? 1 : 0, stream());
  TORCH_CHECK(rc == 0, "ct_beam_update failed: ", rc);
  return {cand_score, cand_idx};
}

// The pointer table of one set of ping (src) and pong (dst) caches, built once from checked
// tensors and kept with them, so a launch can never see a pointer that was not validated.
class BeamCachePlan {
 public:
  BeamCachePlan(std::vector<at::Tensor> src, std::vector<at::Tensor> dst) : src_(std::move(src)), dst_(std::move(dst)) {
    TORCH_CHECK(!src_.empty() && src_.size() == dst_.size() && src_.size() <= 65535,
                "BeamCachePlan: need as many destination as source tensors (1..65535)");
    const auto& f = src_[0];
    TORCH_CHECK(f.dim() == 4, "BeamCachePlan: caches must be [R, T, H, D]");
    rows_ = f.size(0); slots_ = f.size(1); slot_elems_ = f.size(2) * f.size(3);
    TORCH_CHECK(rows_ >= 1 && rows_ <= 65535, "BeamCachePlan: 1..65535 rows, got ", rows_);
    TORCH_CHECK(slots_ >= 1 && slots_ <= INT32_MAX, "BeamCachePlan: slot count out of range");
    TORCH_CHECK(slot_elems_ >= 8 && slot_elems_ % 8 == 0 && slot_elems_ <= INT32_MAX,
                "BeamCachePlan: H * D must be a multiple of 8, got ", slot_elems_);
    std::vector<int64_t> ptrs;
    for (const auto* set : {&src_, &dst_})
      for (const auto& t : *set) {
        check(t, "cache", at::kBFloat16, f.sizes());
        TORCH_CHECK(t.device() == f.device(), "BeamCachePlan: caches must share one device");
        TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0, "BeamCachePlan: caches must be 16-byte aligned");
        ptrs.push_back(reinterpret_cast<int64_t>(t.data_ptr()));
      }
    for (size_t i = 0; i < src_.size(); ++i)
      for (size_t j = 0; j < dst_.size(); ++j)
        TORCH_CHECK(src_[i].data_ptr() != dst_[j].data_ptr(), "BeamCachePlan: a cache cannot be reordered in place");
    table_ = at::tensor(ptrs, at::TensorOptions().dtype(at::kLong)).to(f.device());
  }

  // dst[i][r, :pos] = src[i][beam_idx[r], :pos] for every pair i
  void run(at::Tensor beam_idx, at::Tensor pos) {
    check(beam_idx, "beam_idx", at::kLong, {rows_});
    check(pos, "pos", at::kLong, {1});
    TORCH_CHECK(beam_idx.device() == table_.device() && pos.device() == table_.device(),
                "cache_reorder: beam_idx and pos must be on the caches' device");
    int rc = ct_cache_reorder((const long*)table_.data_ptr(), (int)src_.size(), (const long*)beam_idx.data_ptr(),
                              (const long*)pos.data_ptr(), (int)rows_, (int)slots_, (int)slot_elems_, stream());
    TORCH_CHECK(rc == 0, "ct_cache_reorder failed: ", rc);
  }

 private:
  std::vector<at::Tensor> src_, dst_;
  at::Tensor table_;
  int64_t rows_ = 0, slots_ = 0, slot_elems_ = 0;
};

}  // namespace

void register_beam(pybind11::module& m) {
  m.def("beam_topk", &beam_topk, pybind11::arg("logits"), pybind11::arg("num_beams"));
  m.def("beam_update", &beam_update, pybind11::arg("lse"), pybind11::arg("top_val"), pybind11::arg("top_tok"),
        pybind11::arg("run_seq"), pybind11::arg("run_score"), pybind11::arg("fin_seq"), pybind11::arg("fin_score"),
        pybind11::arg("fin_flag"), pybind11::arg("unsat"), pybind11::arg("len_pen"), pybind11::arg("pos"),
        pybind11::arg("arrive"), pybind11::arg("beam_idx"), pybind11::arg("cur"), pybind11::arg("vocab"),
        pybind11::arg("eos"), pybind11::arg("early_stopping"));
  pybind11::class_<BeamCachePlan>(m, "BeamCachePlan")
      .def(pybind11::init<std::vector<at::Tensor>, std::vector<at::Tensor>>(), pybind11::arg("src"),
           pybind11::arg("dst"))
      .def("run", &BeamCachePlan::run, pybind11::arg("beam_idx"), pybind11::arg("pos"));
}
