"""Static int8 quantization kernels (csrc/quant.hip) against the CPU reference: the cast, the
LayerNorm that emits int8 and the int8-out GEMM epilogue bit for bit, the binding checks, the
static BERT end to end, fused against unfused, and a graph replay."""
import pytest
import torch

from cloudtik_amd import ops
from cloudtik_amd.models.bert import BertConfig, BertLayer
from cloudtik_amd.models.bert_quant import SITES, QuantBertClassifier, QuantBertLayer, calibrate
from cloudtik_amd.modeling.transfer_learning.text_classification import BertClassifier
from cloudtik_amd.ops import reference as ref

pytestmark = pytest.mark.gpu


def _rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def _ordered(t):
    """bf16 -> integers whose difference is the distance in bf16 ulps (sign-magnitude unfolded)."""
    b = t.contiguous().view(torch.int16).to(torch.int32)
    return torch.where(b < 0, -(b & 0x7FFF), b)


# ----------------------------------------------------------------------------- quant_static_i8
# (1, 16): one chunk, one live thread; (67, 128): a partial last block; (3, 2064) and (5, 8192):
# row widths on either side of the row kernel's switch (this kernel is flat); 3-D: leading dims
@pytest.mark.parametrize("shape", [(1, 16), (67, 128), (3, 2064), (5, 8192), (3, 5, 128)])
def test_quantize_static_bit_equal(cuda, shape):
    g = torch.Generator().manual_seed(sum(shape) * 10007 + len(shape))
    x = (torch.randn(*shape, generator=g) * 3).to(torch.bfloat16)
    flat = x.view(-1)
    flat[:8] = torch.tensor([127.0, 0.5, 1.5, -2.5, -0.5, 126.5, 300.0, -300.0])   # amax 127: exact ties
    xg = x.to(cuda)
    q = ops.quantize_static(xg, 127.0)
    assert q.dtype == torch.int8 and q.is_cuda and q.shape == x.shape
    assert torch.equal(q.cpu(), ref.quantize_static(x, 127.0))
    assert q.view(-1)[:8].tolist() == [127, 0, 2, -2, 0, 126, 127, -127]
    for amax in (2.9375, 7.3, 0.1):                       # saturated values on both signs
        amax = float(torch.tensor(amax, dtype=torch.float32))
        want = ref.quantize_static(x, amax)
        assert (want == 127).any() and (want == -127).any()
        assert torch.equal(ops.quantize_static(xg, amax).cpu(), want)
    assert not ops.quantize_static(xg, 0.0).any()         # amax = 0: q 0


# ----------------------------------------------------------------------------- layer_norm_quant
# M: one row, a partial block of four waves, a grid tail; N: fewer 8-element chunks than lanes,
# then one, two and four chunks per lane
@pytest.mark.parametrize("M", [1, 5, 67])
@pytest.mark.parametrize("N", [64, 128, 1024, 2048])
@pytest.mark.parametrize("fused_in", [False, True])
def test_layer_norm_quant(cuda, M, N, fused_in):
    g = torch.Generator().manual_seed(M * 10007 + N + fused_in)
    bf = lambda t: t.to(torch.bfloat16).to(cuda)
    x = bf(torch.randn(M, N, generator=g) * 2)
    gamma, beta = bf(torch.rand(N, generator=g) + 0.5), bf(torch.randn(N, generator=g) * 0.2)
    bias = bf(torch.randn(N, generator=g) * 0.2) if fused_in else None
    res = bf(torch.randn(M, N, generator=g)) if fused_in else None
    amax = 1.5                                            # a normalised row reaches about 3: some saturate
    y, q = ops.layer_norm_quant(x, gamma, beta, 1e-12, bias=bias, residual=res, amax=amax)
    assert y.dtype == torch.bfloat16 and q.dtype == torch.int8 and y.shape == q.shape == (M, N)
    want_q = ref.quantize_static(y.cpu(), amax)
    assert torch.equal(q.cpu(), want_q)                   # from the stored, rounded y
    assert N < 128 or ((want_q.abs() == 127).any() and (want_q.abs() < 127).any())
    y0 = ops.layer_norm(x, gamma, beta, 1e-12, bias=bias, residual=res, training=False)
    diff = (y != y0).sum().item()
    print(f"elements differing from ops.layer_norm: {diff}")
    assert torch.equal(y, y0)
    y1, none = ops.layer_norm_quant(x, gamma, beta, 1e-12, bias=bias, residual=res)   # int8 output off
    assert none is None and torch.equal(y1, y)
    # no beta, 3-D input
    if M == 5:
        x3 = x.view(1, M, N)
        y3, q3 = ops.layer_norm_quant(x3, gamma, None, 1e-12, amax=amax)
        assert y3.shape == q3.shape == (1, M, N)
        assert torch.equal(y3.view(M, N), ops.layer_norm(x, gamma, None, 1e-12, training=False))
        assert torch.equal(q3.cpu(), ref.quantize_static(y3.cpu(), amax))


# ----------------------------------------------------------------------------- gemm_i8_nt_static
@pytest.mark.parametrize("M,N,K", [(1, 64, 64), (64, 128, 128), (131, 192, 192), (17, 128, 320)])
@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("act", [ops.ACT_NONE, ops.ACT_GELU])
def test_linear_i8_static(cuda, M, N, K, with_bias, act):
    g = torch.Generator().manual_seed(M + N + K)
    x = torch.randn(M, K, generator=g).to(torch.bfloat16)
    w = torch.randn(N, K, generator=g) * K ** -0.5
    bias = torch.randn(N, generator=g).to(torch.bfloat16) if with_bias else None
    a_amax = 2.5                                          # inputs beyond 2.5 sigma saturate
    a_q = ref.quantize_static(x, a_amax)
    w_q, w_s = ops.quantize_weight(w)
    # the oracle: the reference epilogue on the exact accumulators, cast to bf16
    a_s = torch.full((M,), ref.static_scales(a_amax)[0])
    want = ref.dequant_epilogue(ref.gemm_i8_nt_raw(a_q, w_q), a_s, w_s, bias, act, torch.bfloat16)
    dev = lambda t: None if t is None else t.to(cuda)
    got_g = ops.linear_i8_static(dev(a_q), a_amax, dev(w_q), dev(w_s), dev(bias), act)
    assert got_g.dtype == torch.bfloat16 and got_g.shape == (M, N)
    got = got_g.cpu()
    if act == ops.ACT_NONE:
        ulps = (_ordered(got) - _ordered(want)).abs().max().item()
        print(f"max bf16 ulp distance {ulps}")
        assert ulps <= 1
    else:
        r = _rel(got, want)
        print(f"gelu rel {r:.2e}")
        assert r < 1e-2
    # quantizing inside linear_i8_static is the same computation
    assert torch.equal(ops.linear_i8_static(dev(x), a_amax, dev(w_q), dev(w_s), dev(bias), act).cpu(), got)
    # int8 out: exactly the quantization of the same call's bf16 output
    out_amax = float(got.float().abs().max()) * 0.5
    want_q = ref.quantize_static(got, out_amax)
    assert (want_q.abs() == 127).sum() >= 1
    q = ops.linear_i8_static(dev(a_q), a_amax, dev(w_q), dev(w_s), dev(bias), act, out_amax=out_amax)
    assert q.dtype == torch.int8 and q.shape == (M, N)
    assert torch.equal(q.cpu(), want_q)
    assert torch.equal(q, ops.quantize_static(got_g, out_amax))   # and what the unfused chain gives


@pytest.mark.parametrize("M,N,K", [(64, 128, 128), (131, 192, 192), (17, 128, 320)])
def test_linear_i8_static_identity(cuda, M, N, K):
    """A = I (padded with zeros) against an asymmetric W, all scales 1: the int8 output is W's
    columns.  Catches a swapped or mis-strided 32-bit store."""
    a = torch.zeros(M, K, dtype=torch.int8)
    d = min(M, K)
    a[torch.arange(d), torch.arange(d)] = 1
    n, k = torch.arange(N).view(N, 1), torch.arange(K).view(1, K)
    w = ((3 * n + 7 * k) % 251 - 125).to(torch.int8)
    want = torch.zeros(M, N, dtype=torch.int8)
    want[:d] = w[:, :d].t()
    # a_amax = out_amax = 127: scale and inv are exactly 1
    q = torch.full((M, N), -7, device=cuda, dtype=torch.int8)
    ops.require_native().gemm_i8_nt_static(a.to(cuda), 1.0, w.to(cuda), torch.ones(N, device=cuda), None, 0, q, 1.0)
    assert torch.equal(q.cpu(), want)
    assert torch.equal(ops.linear_i8_static(a.to(cuda), 127.0, w.to(cuda), torch.ones(N, device=cuda),
                                            out_amax=127.0).cpu(), want)


# ----------------------------------------------------------------------------- binding checks
def test_static_bindings_reject_bad_operands(cuda):
    C = ops.require_native()
    i8 = lambda *s: torch.zeros(*s, device=cuda, dtype=torch.int8)
    f32 = lambda *s: torch.ones(*s, device=cuda, dtype=torch.float32)
    bf = lambda *s: torch.zeros(*s, device=cuda, dtype=torch.bfloat16)
    bad_factors = (-1.0, float("inf"), float("nan"), 0.1)      # 0.1 is no fp32 value

    assert C.quant_static_i8(bf(4, 64), 1.0).shape == (4, 64)
    for x in (f32(4, 64), bf(4, 128)[:, ::2], bf(3, 8), bf(4, 64).cpu(), bf(80)[4:68], bf(0, 16)):
        with pytest.raises(RuntimeError):                  # dtype, strides, % 16, CPU, alignment, empty
            C.quant_static_i8(x, 1.0)
    for v in bad_factors:
        with pytest.raises(RuntimeError):
            C.quant_static_i8(bf(4, 64), v)

    ok = (bf(4, 64), bf(64), bf(4, 64), bf(64), bf(64), 1e-12, 1.0, True)
    y, q = C.layernorm_quant_i8(*ok)
    assert y.shape == q.shape == (4, 64) and q.dtype == torch.int8
    assert C.layernorm_quant_i8(*ok[:-1], False)[1] is None
    for idx, val in [(0, bf(4, 60)), (0, bf(4, 2056)), (0, f32(4, 64)), (0, bf(4, 128)[:, ::2]), (0, bf(4, 64).cpu()),
                     (1, bf(32)), (1, f32(64)), (2, bf(3, 64)), (2, bf(4, 128)[:, ::2]), (3, bf(32)), (3, f32(64)),
                     (3, bf(68)[4:]), (4, bf(65)), (4, bf(64).cpu()), (5, -1.0), (5, float("nan"))]:
        args = list(ok)
        args[idx] = val
        with pytest.raises(RuntimeError):
            C.layernorm_quant_i8(*args)
    for v in bad_factors:
        with pytest.raises(RuntimeError):
            C.layernorm_quant_i8(*ok[:6], v, True)

    ok = (i8(16, 64), 1.0, i8(64, 64), f32(64), None, 0, bf(16, 64), 0.0)
    C.gemm_i8_nt_static(*ok)
    C.gemm_i8_nt_static(*ok[:6], i8(16, 64), 1.0)
    for idx, val in [(0, i8(16, 96)), (2, i8(32, 64)), (0, i8(16, 128)[:, ::2]), (2, i8(64, 128)[:, ::2]),
                     (6, bf(16, 128)[:, ::2]), (6, i8(16, 128)[:, ::2]), (0, bf(16, 64)), (2, i8(64, 128)),
                     (3, f32(63)), (3, bf(64)), (4, bf(32)), (4, f32(64)), (5, 2), (6, f32(16, 64)),
                     (6, i8(17, 64)), (0, i8(16, 64).cpu()), (6, bf(16, 64).cpu())]:
        args = list(ok)
        args[idx] = val
        with pytest.raises(RuntimeError):
            C.gemm_i8_nt_static(*args)
    for v in bad_factors:
        with pytest.raises(RuntimeError):
            C.gemm_i8_nt_static(*ok[:1], v, *ok[2:])
        with pytest.raises(RuntimeError):
            C.gemm_i8_nt_static(*ok[:6], i8(16, 64), v)

    # the dispatchers: a bad range is a ValueError before anything is launched; no silent cast
    for amax in (-1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            ops.quantize_static(bf(4, 64), amax)
        with pytest.raises(ValueError):
            ops.layer_norm_quant(bf(4, 64), bf(64), bf(64), amax=amax)
        with pytest.raises(ValueError):
            ops.linear_i8_static(i8(16, 64), amax, i8(64, 64), f32(64))
        with pytest.raises(ValueError):
            ops.linear_i8_static(i8(16, 64), 1.0, i8(64, 64), f32(64), out_amax=amax)
    with pytest.raises(TypeError):
        ops.quantize_static(f32(4, 64), 1.0)
    with pytest.raises(TypeError):
        ops.layer_norm_quant(f32(4, 64), bf(64), bf(64), amax=1.0)
    with pytest.raises(RuntimeError):
        ops.layer_norm_quant(bf(4, 2056), bf(2056), bf(2056), amax=1.0)    # outside the tiling: no fall-back


# ----------------------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def tiny(cuda):
    """bert-tiny (hidden 128, 2 heads of 64, 2 layers) as fp32 on the CPU and bf16 on the GPU, a
    3 x 128 batch with a padding mask, and the ranges calibrated on the fp32 CPU model."""
    torch.manual_seed(0)
    cfg = BertConfig.tiny()
    assert (cfg.hidden_size, cfg.num_attention_heads, cfg.num_hidden_layers) == (128, 2, 2)
    f_cpu = BertClassifier(cfg, 16, device="cpu", dtype=torch.float32).eval()
    f_gpu = BertClassifier(cfg, 16, device=cuda, dtype=torch.bfloat16).eval()
    f_gpu.load_state_dict({k: v.to(torch.bfloat16) for k, v in f_cpu.state_dict().items()})
    ids = torch.randint(1, cfg.vocab_size, (3, 128))
    mask = torch.ones(3, 128, dtype=torch.long)
    mask[1, 90:] = 0
    mask[2, 17:] = 0
    amax = calibrate(f_cpu, [(ids, mask)])
    with torch.no_grad():
        want = f_cpu(ids, mask)
    return f_cpu, f_gpu, ids, mask, amax, want


def test_static_bert_end_to_end(cuda, tiny):
    """rel(q_gpu, f_cpu) <= rel(q_cpu, f_cpu) + 2 rel(f_gpu, f_cpu) on the logits -- the GPU int8
    model may differ from the fp32 model by the quantization error the CPU reference shows plus
    the bf16 kernels' noise, which enters once directly and once by flipping int8 roundings."""
    f_cpu, f_gpu, ids, mask, amax, want = tiny
    q_cpu = QuantBertClassifier.from_float(f_cpu, act_amax=amax)
    q_gpu = QuantBertClassifier.from_float(f_gpu, act_amax=amax)
    assert q_gpu.act_amax == amax and q_gpu.bert.layers[0].qkv_weight_q.is_cuda
    with torch.no_grad():
        out = {"q_cpu": q_cpu(ids, mask), "f_gpu": f_gpu(ids.to(cuda), mask.to(cuda)),
               "q_gpu": q_gpu(ids.to(cuda), mask.to(cuda))}
    r = {k: _rel(v, want) for k, v in out.items()}
    print("rel to fp32 CPU logits:", {k: f"{v:.4e}" for k, v in r.items()})
    assert out["q_gpu"].dtype == torch.bfloat16 and torch.isfinite(out["q_gpu"]).all()
    assert r["q_gpu"] <= r["q_cpu"] + 2 * r["f_gpu"]


@pytest.mark.parametrize("sites", [SITES, ("qkv", "out", "ffn1"), ("qkv", "ffn1")])
def test_static_fused_equals_unfused(cuda, tiny, sites):
    _, f_gpu, ids, mask, amax, _ = tiny
    fused = QuantBertClassifier.from_float(f_gpu, sites, act_amax=amax, fuse=True)
    plain = QuantBertClassifier.from_float(f_gpu, sites, act_amax=amax, fuse=False)
    with torch.no_grad():
        a, b = fused(ids.to(cuda), mask.to(cuda)), plain(ids.to(cuda), mask.to(cuda))
    assert torch.isfinite(a).all() and torch.equal(a, b)


def test_static_layer_graph_replay(cuda):
    """A captured static layer replays to the eager result bit for bit: the ranges reach the
    kernels by value, nothing allocates or synchronises behind the stream's back."""
    torch.manual_seed(1)
    cfg = BertConfig.tiny()
    layer = QuantBertLayer.from_float(BertLayer(cfg, device=cuda, dtype=torch.bfloat16), SITES,
                                      act_amax=[4.0, 0.5, 4.0, 1.0])
    x = torch.randn(2, 128, cfg.hidden_size, device=cuda).to(torch.bfloat16)
    kb = torch.zeros(2, 128, device=cuda)
    kb[1, 100:] = -10000.0
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            layer(x, kb, out_amax=4.0)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y, y_q = layer(x, kb, out_amax=4.0)
    x.copy_(torch.randn(2, 128, cfg.hidden_size, device=cuda).to(torch.bfloat16))
    graph.replay()
    torch.cuda.synchronize()
    y2, y2_q = layer(x, kb, out_amax=4.0)
    assert torch.equal(y, y2) and torch.equal(y_q, y2_q)
    assert torch.equal(y_q.cpu(), ref.quantize_static(y.cpu(), 4.0))
    assert torch.equal(layer(x, kb), y2)                 # without an int8 output the same y
