"""Int8 quantization kernels (csrc/quant.hip) against the CPU reference: the quantized tensors
and the int32 accumulators bit for bit, the bf16 epilogue within one ulp, the binding checks,
the quantized BERT end to end and a graph replay."""
import pytest
import torch

from cloudtik_amd import ops
from cloudtik_amd.models.bert import BertConfig, BertLayer
from cloudtik_amd.models.bert_quant import QuantBertClassifier, QuantBertLayer
from cloudtik_amd.modeling.transfer_learning.text_classification import BertClassifier
from cloudtik_amd.ops import reference as ref

pytestmark = pytest.mark.gpu


def _rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


# ----------------------------------------------------------------------------- quant_rows_i8
# (1, 64): one row, the smallest K the GEMM takes; (67, 128): row tail of the 4-rows-per-block
# kernel; (130, 1024): the model's width; (3, 2048) / (3, 2064): either side of the switch from
# one row per wave to one row per block; (5, 8192): the widest row allowed
@pytest.mark.parametrize("M,K", [(1, 64), (67, 128), (130, 1024), (3, 2048), (3, 2064), (5, 8192)])
def test_quant_rows_bit_equal(cuda, M, K):
    g = torch.Generator().manual_seed(M * 10007 + K)
    x = (torch.randn(M, K, generator=g) * 3).to(torch.bfloat16)
    if M > 4:
        x[1] = 0                                         # a zero row: scale 0, q 0
        x[2] = 0
        x[2, :6] = torch.tensor([127.0, 0.5, 1.5, -2.5, -0.5, 126.5])   # inv == 1: exact ties
        x[3] = -x[3].abs() - 0.25                        # the maximum is negative
    q_ref, s_ref = ref.quantize_rows(x)
    q, s = ops.quantize_rows(x.to(cuda))
    assert q.dtype == torch.int8 and s.dtype == torch.float32 and q.is_cuda
    assert torch.equal(s.cpu(), s_ref)
    assert torch.equal(q.cpu(), q_ref)
    if M > 4:
        assert s_ref[1] == 0 and not q_ref[1].any()
        assert q_ref[2, :6].tolist() == [127, 0, 2, -2, 0, 126]


def test_quant_rows_leading_dims(cuda):
    x = torch.randn(3, 5, 128).to(torch.bfloat16)
    q, s = ops.quantize_rows(x.to(cuda))
    q_ref, s_ref = ref.quantize_rows(x)
    assert q.shape == (3, 5, 128) and s.shape == (3, 5)
    assert torch.equal(q.cpu(), q_ref) and torch.equal(s.cpu(), s_ref)


# ----------------------------------------------------------------------------- gemm_i8_nt_raw
def _rand_i8(g, *shape):
    return torch.randint(-127, 128, shape, generator=g, dtype=torch.int32).to(torch.int8)


def _raw(cuda, a, w):
    out = torch.full((a.shape[0], w.shape[0]), -7, device=cuda, dtype=torch.int32)
    ops.require_native().gemm_i8_nt_raw(a.to(cuda), w.to(cuda), out)
    return out.cpu()


RAW_CASES = ([(m, 128, 128) for m in (16, 64, 128)] +          # one block, aligned M
             [(m, 64, 64) for m in (1, 17, 131)] +             # M tail, a single 64-wide K step
             [(m, 192, 192) for m in (1, 17, 131)] +           # N no multiple of 128, 3 K steps of 64
             [(m, 128, 320) for m in (1, 17, 131)] +           # 5 K steps of 64
             [(1155, 192, 64)])                                # 10 x 2 tiles: more blocks than XCDs


@pytest.mark.parametrize("M,N,K", RAW_CASES)
def test_gemm_i8_raw_exact(cuda, M, N, K):
    g = torch.Generator().manual_seed(M * 1000003 + N * 1009 + K)
    a, w = _rand_i8(g, M, K), _rand_i8(g, N, K)
    assert torch.equal(_raw(cuda, a, w), ref.gemm_i8_nt_raw(a, w))


@pytest.mark.parametrize("M,N,K", [(64, 128, 128), (131, 192, 192), (17, 128, 320)])
def test_gemm_i8_raw_identity(cuda, M, N, K):
    """A = I (padded with zeros) against an asymmetric W returns W's columns: catches a swapped
    or mis-strided C write whatever the k order inside the instruction."""
    a = torch.zeros(M, K, dtype=torch.int8)
    d = min(M, K)
    a[torch.arange(d), torch.arange(d)] = 1
    n, k = torch.arange(N).view(N, 1), torch.arange(K).view(1, K)
    w = ((3 * n + 7 * k) % 251 - 125).to(torch.int8)
    want = torch.zeros(M, N, dtype=torch.int32)
    want[:d] = w[:, :d].t().to(torch.int32)
    assert torch.equal(_raw(cuda, a, w), want)


def test_gemm_i8_raw_extreme_accumulator(cuda):
    M, N, K = 16, 64, 8192
    a = torch.full((M, K), 127, dtype=torch.int8)
    w = torch.full((N, K), -127, dtype=torch.int8)
    out = _raw(cuda, a, w)
    assert out.dtype == torch.int32 and torch.equal(out, torch.full((M, N), -127 * 127 * K, dtype=torch.int32))


# ----------------------------------------------------------------------------- gemm_i8_nt (bf16)
def _ordered(t):
    """bf16 -> integers whose difference is the distance in bf16 ulps (sign-magnitude unfolded)."""
    b = t.contiguous().view(torch.int16).to(torch.int32)
    return torch.where(b < 0, -(b & 0x7FFF), b)


@pytest.mark.parametrize("M,N,K", [(64, 128, 128), (131, 192, 192)])
@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("act", [ops.ACT_NONE, ops.ACT_GELU])
def test_gemm_i8_bf16_epilogue(cuda, M, N, K, with_bias, act):
    g = torch.Generator().manual_seed(M + N + K)
    x = torch.randn(M, K, generator=g).to(torch.bfloat16)
    w = torch.randn(N, K, generator=g) * K ** -0.5
    bias = torch.randn(N, generator=g).to(torch.bfloat16) if with_bias else None
    a_q, a_s = ref.quantize_rows(x)
    w_q, w_s = ops.quantize_weight(w)
    # the oracle: the reference epilogue on the exact accumulators, cast to bf16
    want = ref.dequant_epilogue(ref.gemm_i8_nt_raw(a_q, w_q), a_s, w_s, bias, act, torch.bfloat16)
    got = ops.linear_i8((a_q.to(cuda), a_s.to(cuda)), w_q.to(cuda), w_s.to(cuda),
                        bias.to(cuda) if with_bias else None, act)
    assert got.dtype == torch.bfloat16 and got.shape == (M, N)
    got = got.cpu()
    if act == ops.ACT_NONE:
        ulps = (_ordered(got) - _ordered(want)).abs().max().item()
        print(f"max bf16 ulp distance {ulps}")
        assert ulps <= 1
    else:
        r = _rel(got, want)
        print(f"gelu rel {r:.2e}")
        assert r < 1e-2
    # quantizing inside linear_i8 is the same computation
    assert torch.equal(ops.linear_i8(x.to(cuda), w_q.to(cuda), w_s.to(cuda),
                                     bias.to(cuda) if with_bias else None, act).cpu(), got)


# ----------------------------------------------------------------------------- binding checks
def test_bindings_reject_bad_operands(cuda):
    C = ops.require_native()
    i8 = lambda *s: torch.zeros(*s, device=cuda, dtype=torch.int8)
    i32 = lambda *s: torch.zeros(*s, device=cuda, dtype=torch.int32)
    f32 = lambda *s: torch.ones(*s, device=cuda, dtype=torch.float32)
    bf = lambda *s: torch.zeros(*s, device=cuda, dtype=torch.bfloat16)
    bad_raw = [
        (i8(16, 96), i8(64, 96), i32(16, 64)),                    # K = 96
        (i8(16, 64), i8(32, 64), i32(16, 32)),                    # N = 32
        (i8(16, 128)[:, ::2], i8(64, 64), i32(16, 64)),           # a non-contiguous operand
        (i8(16, 64), i8(64, 128)[:, ::2], i32(16, 64)),
        (i8(16, 64), i8(64, 64), i32(16, 128)[:, ::2]),
        (i8(16, 64).to(torch.uint8), i8(64, 64), i32(16, 64)),    # wrong dtypes
        (i8(16, 64), bf(64, 64), i32(16, 64)),
        (i8(16, 64), i8(64, 64), f32(16, 64)),
        (i8(16, 64), i8(64, 128), i32(16, 64)),                   # K mismatch
        (i8(16, 64), i8(64, 64), i32(17, 64)),                    # out shape
        (i8(16, 64).cpu(), i8(64, 64), i32(16, 64)),              # not on the GPU
    ]
    for args in bad_raw:
        with pytest.raises(RuntimeError):
            C.gemm_i8_nt_raw(*args)
    ok = (i8(16, 64), f32(16), i8(64, 64), f32(64), None, 0, bf(16, 64))
    C.gemm_i8_nt(*ok)
    for idx, val in [(1, f32(15)), (3, f32(63)), (1, bf(16)), (4, bf(32)), (4, f32(64)), (5, 2), (6, i32(16, 64)),
                     (0, i8(16, 96)), (2, i8(32, 64))]:
        args = list(ok)
        args[idx] = val
        with pytest.raises(RuntimeError):
            C.gemm_i8_nt(*args)
    for x in (bf(4, 24), bf(4, 8208), f32(4, 64), bf(4, 128)[:, ::2]):   # K % 16, K > 8192, dtype, strides
        with pytest.raises(RuntimeError):
            C.quant_rows_i8(x)
    with pytest.raises(TypeError):
        ops.quantize_rows(f32(4, 64))                              # no silent cast on the GPU path


# ----------------------------------------------------------------------------- end to end
def test_quant_bert_end_to_end(cuda):
    """bert-tiny (hidden 128, 2 heads of 64, 2 layers), batch 3 x 128 with a padding mask:
    rel(q_gpu, f_cpu) <= rel(q_cpu, f_cpu) + 2 rel(f_gpu, f_cpu) on the logits -- the GPU int8
    model may differ from the fp32 model by the quantization error the CPU reference shows plus
    the bf16 kernels' noise, which enters once directly and once by flipping int8 roundings."""
    torch.manual_seed(0)
    cfg = BertConfig.tiny()
    assert (cfg.hidden_size, cfg.num_attention_heads, cfg.num_hidden_layers) == (128, 2, 2)
    f_cpu = BertClassifier(cfg, 16, device="cpu", dtype=torch.float32).eval()
    f_gpu = BertClassifier(cfg, 16, device=cuda, dtype=torch.bfloat16).eval()
    f_gpu.load_state_dict({k: v.to(torch.bfloat16) for k, v in f_cpu.state_dict().items()})
    q_cpu = QuantBertClassifier.from_float(f_cpu)
    q_gpu = QuantBertClassifier.from_float(f_gpu)
    assert q_gpu.bert.layers[0].qkv_weight_q.dtype == torch.int8 and q_gpu.bert.layers[0].qkv_weight_q.is_cuda
    ids = torch.randint(1, cfg.vocab_size, (3, 128))
    mask = torch.ones(3, 128, dtype=torch.long)
    mask[1, 90:] = 0
    mask[2, 17:] = 0
    with torch.no_grad():
        want = f_cpu(ids, mask)
        out = {"q_cpu": q_cpu(ids, mask), "f_gpu": f_gpu(ids.to(cuda), mask.to(cuda)),
               "q_gpu": q_gpu(ids.to(cuda), mask.to(cuda))}
    r = {k: _rel(v, want) for k, v in out.items()}
    print("rel to fp32 CPU logits:", {k: f"{v:.4e}" for k, v in r.items()})
    assert out["q_gpu"].dtype == torch.bfloat16 and torch.isfinite(out["q_gpu"]).all()
    assert r["q_gpu"] <= r["q_cpu"] + 2 * r["f_gpu"]


def test_quant_layer_graph_replay(cuda):
    """A captured layer replays to the eager result bit for bit: no launcher allocates or
    synchronises behind the stream's back."""
    torch.manual_seed(1)
    cfg = BertConfig.tiny()
    layer = QuantBertLayer.from_float(BertLayer(cfg, device=cuda, dtype=torch.bfloat16))
    x = torch.randn(2, 128, cfg.hidden_size, device=cuda).to(torch.bfloat16)
    kb = torch.zeros(2, 128, device=cuda)
    kb[1, 100:] = -10000.0
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            layer(x, kb)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = layer(x, kb)
    x.copy_(torch.randn(2, 128, cfg.hidden_size, device=cuda).to(torch.bfloat16))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(y, layer(x, kb))
