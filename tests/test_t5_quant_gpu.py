"""Int8 T5 on the GPU: the decode GEMM for M <= 64 (csrc/quant_skinny.hip) against the CPU reference
bit for bit -- accumulators and bf16 epilogue --, the RMS norm that emits int8 against the unfused
chain, the fused decode step against the module path, graph replay of all three generation modes
and the end-to-end error of the logits."""
import pytest
import torch

from cloudtik_amd import ops
from cloudtik_amd.models.t5 import T5Config, T5ForConditionalGeneration
from cloudtik_amd.models.t5_quant import QuantT5ForConditionalGeneration
from cloudtik_amd.ops import constrain as C
from cloudtik_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

BF = torch.bfloat16

# (1, 64, 64): one K step, fewer steps than waves; (17, 192, 320): one row past an MFMA tile, N not a
# multiple of 128, a K tail inside the 256-byte slab; (33, 64, 8192): the largest K; (64, 192, 1024): the
# largest M; (48, 32128, 128): the head's width
SHAPES = [(1, 64, 64), (5, 128, 192), (16, 64, 128), (17, 192, 320), (33, 64, 8192), (64, 192, 1024),
          (48, 32128, 128)]
GUARD = 3                                                     # rows behind M that must stay untouched


def _case(M, N, K):
    """Asymmetric operands (a sign or operand swap changes the sums), scales and a residual."""
    g = torch.Generator().manual_seed(M * 1000003 + N * 101 + K)
    a = torch.randint(-127, 128, (M, K), generator=g, dtype=torch.int32).to(torch.int8)
    w = torch.randint(-30, 128, (N, K), generator=g, dtype=torch.int32).to(torch.int8)   # A alone has zero mean
    sa = torch.rand(M, generator=g) * 0.02 + 1e-3
    sw = torch.rand(N, generator=g) * 2e-3 + 1e-4
    bias = torch.randn(N, generator=g).to(BF)
    res = (torch.randn(M, N, generator=g) * 4).to(BF)
    return a, w, sa, sw, bias, res


_CACHE = {}


def _shared(M, N, K):
    """The operands and the reference accumulators of a shape, computed once for every test."""
    key = (M, N, K)
    if key not in _CACHE:
        case = _case(M, N, K)
        _CACHE[key] = case + (ref.gemm_i8_nt_raw(case[0], case[1]),)
    return _CACHE[key]


def _raw(cuda, a, w):
    M, N = a.shape[0], w.shape[0]
    buf = torch.full((M + GUARD, N), -7, device=cuda, dtype=torch.int32)
    ops.require_native().gemm_i8_skinny_raw(a.to(cuda), w.to(cuda), buf[:M])
    assert bool((buf[M:] == -7).all())
    return buf[:M].cpu()


# ----------------------------------------------------------------------------- raw accumulators
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_skinny_raw_exact(cuda, M, N, K):
    a, w, *_, acc = _shared(M, N, K)
    assert torch.equal(_raw(cuda, a, w), acc)


def test_skinny_raw_identity_weight(cuda):
    """W = identity puts A's column n on output column n: a row / column swap cannot pass."""
    M, K = 17, 128
    g = torch.Generator().manual_seed(5)
    a = torch.randint(-127, 128, (M, K), generator=g, dtype=torch.int32).to(torch.int8)
    w = torch.eye(K, dtype=torch.int8)
    assert torch.equal(_raw(cuda, a, w), a.to(torch.int32))


def test_skinny_raw_extreme_accumulator(cuda):
    M, N, K = 3, 64, 8192
    a = torch.full((M, K), 127, dtype=torch.int8)
    a[1] = -127
    w = torch.full((N, K), 127, dtype=torch.int8)
    w[1::2] = -127
    got = _raw(cuda, a, w)
    assert torch.equal(got, ref.gemm_i8_nt_raw(a, w))
    assert got.abs().min().item() == 127 * 127 * 8192


# ----------------------------------------------------------------------------- the epilogue
@pytest.mark.parametrize("mode", ["none", "relu", "bias_relu", "residual", "bias_residual", "alias"])
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_skinny_epilogue_bit_equal(cuda, M, N, K, mode):
    a, w, sa, sw, bias, res, acc = _shared(M, N, K)
    act = ops.ACT_RELU if "relu" in mode else ops.ACT_NONE
    b = bias if "bias" in mode else None
    r = res if ("residual" in mode or mode == "alias") else None
    want = ref.dequant_epilogue(acc, sa, sw, b, act, BF, r)
    buf = torch.full((M + GUARD, N), 777.0, device=cuda, dtype=BF)
    r_gpu = None
    if mode == "alias":
        buf[:M] = res.to(cuda)
        r_gpu = buf[:M]
    elif r is not None:
        r_gpu = r.to(cuda)
    ops.require_native().gemm_i8_skinny(a.to(cuda), sa.to(cuda), w.to(cuda), sw.to(cuda),
                                        b.to(cuda) if b is not None else None, act, r_gpu, buf[:M])
    assert torch.equal(buf[:M].cpu(), want)
    assert bool((buf[M:] == 777.0).all())
    if "relu" in mode:
        assert bool((want == 0).any()) and bool((want > 0).any())
    if r is not None and mode != "alias":
        assert torch.equal(r_gpu.cpu(), res)                  # a separate residual is only read


def test_linear_i8_routes_agree(cuda, monkeypatch):
    """ops.linear_i8: the decode kernel, the tiled kernel forced by CLOUDTIK_AMD_I8_SKINNY=0 and, past 64
    rows, the tiled kernel with PyTorch's ReLU / residual give the reference's bits."""
    M, N, K = 80, 192, 320
    a, w, sa, sw, _, res = _case(M, N, K)
    acc = ref.gemm_i8_nt_raw(a, w)
    for rows in (17, 80):
        pair = (a[:rows].to(cuda), sa[:rows].to(cuda))
        for act, r in ((ops.ACT_NONE, None), (ops.ACT_RELU, None), (ops.ACT_NONE, res[:rows])):
            want = ref.dequant_epilogue(acc[:rows], sa[:rows], sw, None, act, BF, r)
            for env in ("1", "0"):
                monkeypatch.setenv("CLOUDTIK_AMD_I8_SKINNY", env)
                got = ops.linear_i8(pair, w.to(cuda), sw.to(cuda), None, act,
                                    residual=r.to(cuda) if r is not None else None)
                assert torch.equal(got.cpu(), want), (rows, act, env)
    with pytest.raises(ValueError):
        ops.linear_i8(pair, w.to(cuda), sw.to(cuda), None, ops.ACT_RELU, residual=res.to(cuda))


def test_skinny_binding_refusals(cuda):
    Cx = ops.require_native()

    def call(M=4, N=64, K=64, a=None, w=None, out=None, res=None, act=0):
        a = torch.zeros(M, K, device=cuda, dtype=torch.int8) if a is None else a
        w = torch.zeros(N, K, device=cuda, dtype=torch.int8) if w is None else w
        out = torch.zeros(a.shape[0], w.shape[0], device=cuda, dtype=BF) if out is None else out
        Cx.gemm_i8_skinny(a, torch.ones(a.shape[0], device=cuda), w, torch.ones(w.shape[0], device=cuda), None, act,
                          res, out)

    call()                                                    # the accepted baseline
    with pytest.raises(RuntimeError, match="M must be in 1 .. 64"):
        call(M=65)
    with pytest.raises(RuntimeError, match="K must be a multiple of 64"):
        call(K=96)
    with pytest.raises(RuntimeError, match="K must be a multiple of 64"):
        call(K=8256)
    with pytest.raises(RuntimeError, match="N must be a multiple of 64"):
        call(N=96)
    with pytest.raises(RuntimeError, match="act must be"):
        call(act=1)
    raw = torch.zeros(4 * 64 + 16, device=cuda, dtype=torch.int8)
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        call(a=raw[1:1 + 4 * 64].view(4, 64))
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        call(w=torch.zeros(64 * 64 + 16, device=cuda, dtype=torch.int8)[8:8 + 64 * 64].view(64, 64))
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        call(out=torch.zeros(4 * 64 + 8, device=cuda, dtype=BF)[1:1 + 4 * 64].view(4, 64))
    with pytest.raises(RuntimeError, match="contiguous"):
        call(a=torch.zeros(4, 128, device=cuda, dtype=torch.int8)[:, :64])
    both = torch.zeros(6, 64, device=cuda, dtype=BF)
    with pytest.raises(RuntimeError, match="overlap"):
        call(res=both[:4], out=both[2:6][:4])
    with pytest.raises(RuntimeError, match="int32"):
        Cx.gemm_i8_skinny_raw(torch.zeros(4, 64, device=cuda, dtype=torch.int8),
                              torch.zeros(64, 64, device=cuda, dtype=torch.int8), torch.zeros(4, 64, device=cuda, dtype=BF))
    with pytest.raises(RuntimeError, match="multiple of 16"):
        ops.rms_norm_quant(torch.zeros(2, 24, device=cuda, dtype=BF), torch.ones(24, device=cuda, dtype=BF), 1e-6)
    with pytest.raises(RuntimeError, match="multiple of 16"):
        ops.rms_norm_quant(torch.zeros(2, 2064, device=cuda, dtype=BF), torch.ones(2064, device=cuda, dtype=BF), 1e-6)


# ----------------------------------------------------------------------------- rmsnorm_quant_rows
# (67, 768): a row tail of the four-rows-per-block grid; 512 .. 2048: one to four vectors per lane, (1, 128) lanes
# without any
@pytest.mark.parametrize("zero_row", [False, True])
@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("M,N", [(1, 128), (5, 512), (67, 768), (3, 1024), (2, 2048)])
def test_rmsnorm_quant_rows_bit_equal(cuda, M, N, with_res, zero_row):
    g = torch.Generator().manual_seed(M * 4099 + N)
    x = (torch.randn(M, N, generator=g) * 3).to(BF)
    res = (torch.randn(M, N, generator=g) * 2).to(BF) if with_res else None
    gamma = (1 + 0.2 * torch.randn(N, generator=g)).to(BF)
    if zero_row:
        x[M - 1] = 0
        if with_res:
            res[M - 1] = 0
    xg, rg, gg = x.to(cuda), (res.to(cuda) if with_res else None), gamma.to(cuda)
    y_want = ops.layer_norm(xg, gg, None, eps=1e-6, residual=rg, training=False, rms=True)
    y, (q, s) = ops.rms_norm_quant(xg, gg, 1e-6, rg)
    assert y.dtype == BF and q.dtype == torch.int8 and s.dtype == torch.float32 and s.shape == (M,)
    assert torch.equal(y, y_want)
    q_want, s_want = ref.quantize_rows(y.cpu())
    assert torch.equal(q.cpu(), q_want) and torch.equal(s.cpu(), s_want)
    if zero_row:
        assert s_want[M - 1] == 0 and not q_want[M - 1].any()
    y2, (q2, s2) = ops.rms_norm_quant(xg, gg, 1e-6, rg, emit_y=False)
    assert y2 is None and torch.equal(q2, q) and torch.equal(s2, s)


# ----------------------------------------------------------------------------- the model
def _config(gated):
    return T5Config(vocab_size=192, d_model=128, d_kv=64, num_heads=2, d_ff=256, num_layers=2, num_decoder_layers=2,
                    relative_attention_num_buckets=8, dropout_rate=0.0, gated_gelu=gated)


@pytest.fixture(scope="module")
def models(cuda):
    """Per FF type: the fp32 model on the CPU with bf16-representable weights, its bf16 copy on the GPU and the
    int8 models of both."""
    out = {}
    for gated in (False, True):
        torch.manual_seed(11 + gated)
        f32 = T5ForConditionalGeneration(_config(gated), dtype=torch.float32).eval()
        with torch.no_grad():
            for p in f32.parameters():
                p.copy_(p.bfloat16().float())
        bf = T5ForConditionalGeneration(_config(gated), device=cuda).eval()
        bf.load_state_dict({k: v.bfloat16() for k, v in f32.state_dict().items()})
        out[gated] = dict(f32=f32, bf=bf, q_cpu=f32.quantize_dynamic(), q=bf.quantize_dynamic())
    return out


def _sources(B, S, cuda, seed=3):
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(2, 192, (B, S), generator=g)
    mask = torch.ones(B, S, dtype=torch.long)
    mask[B // 2, S - 3:] = 0
    return x.to(cuda), mask.to(cuda)


@pytest.mark.parametrize("gated", [False, True])
@pytest.mark.parametrize("rows", [3, 64])
def test_fused_step_equals_module_path(cuda, models, rows, gated):
    """Three steps of the fused ``_decode_step_static`` against the float model's step run on the
    int8 modules: caches and logits bit for bit.  64 rows = batch 16 x 4 beams."""
    qm = models[gated]["q"]
    assert isinstance(qm, QuantT5ForConditionalGeneration)
    cfg, S, T = qm.cfg, 9, 5
    x, mask = _sources(rows, S, cuda)
    with torch.no_grad():
        enc, _ = qm.encoder(x, mask)
        cross = [(b.ca._split(b.ca.k(enc)), b.ca._split(b.ca.v(enc))) for b in qm.decoder.blocks]
        enc_bias = (1.0 - mask.float()) * -1e9
        slots = torch.arange(T, device=cuda)

        def run(step_fn):
            kc = [torch.zeros(rows, T, cfg.num_heads, cfg.d_kv, dtype=BF, device=cuda) for _ in qm.decoder.blocks]
            vc = [torch.zeros_like(k) for k in kc]
            cur = torch.full((rows, 1), cfg.decoder_start_token_id, dtype=torch.long, device=cuda)
            outs = []
            for t in range(3):
                pos = torch.tensor([t], device=cuda)
                h = step_fn(cur, pos, slots, kc, vc, cross, enc_bias)
                logits = qm.logits(h[:, -1])
                outs.append(logits)
                cur = logits.float().argmax(-1)[:, None]
            return outs, kc, vc

        fused, kf, vf = run(qm._decode_step_static)
        plain, kp, vp = run(lambda *a: T5ForConditionalGeneration._decode_step_static(qm, *a))
    for t in range(3):
        assert fused[t].shape == (rows, cfg.vocab_size) and fused[t].dtype == BF
        assert torch.equal(fused[t], plain[t]), t
    for a, b in zip(kf + vf, kp + vp):
        assert torch.equal(a, b)
    assert fused[2].float().abs().max() > 0


STEPS = 8


def _eager_static_greedy(qm, key):
    st = qm._graphs[key]
    st["reset"]()
    for _ in range(STEPS):
        st["step"]()
    return st["out"].clone()


@pytest.mark.parametrize("gated", [False, True])
def test_graph_replay_matches_eager_static_step(cuda, models, gated):
    qm = models[gated]["q"]
    x, mask = _sources(3, 9, cuda, seed=5)
    V, eos = qm.cfg.vocab_size, qm.cfg.eos_token_id
    # greedy with an n-gram ban
    cons = C.check_constrain_args(2, 0, 0, None, V, eos, 1, STEPS)
    got = qm.generate(x, mask, max_new_tokens=STEPS, no_repeat_ngram_size=2)
    assert got.shape == (3, STEPS)
    keys = [k for k in qm._graphs if k[0] == 3 and k[-1] == cons]
    assert len(keys) == 1
    assert torch.equal(got, _eager_static_greedy(qm, keys[0]))
    n = len(qm._graphs)
    assert torch.equal(qm.generate(x, mask, max_new_tokens=STEPS, no_repeat_ngram_size=2), got) and len(qm._graphs) == n
    # four beams, two returned
    got, score = qm.generate(x, mask, max_new_tokens=STEPS, num_beams=4, num_return_sequences=2, return_scores=True)
    assert got.shape == (6, STEPS) and score.shape == (6,)
    n = len(qm._graphs)
    again = qm.generate(x, mask, max_new_tokens=STEPS, num_beams=4, num_return_sequences=2)
    assert torch.equal(again, got) and len(qm._graphs) == n
    eager, e_score = qm._generate_beam_static(x, mask, STEPS, 4, 1.0, False, graph=False, num_return=2)
    assert torch.equal(got, eager)
    torch.testing.assert_close(score, e_score, rtol=1e-5, atol=0)
    # sampling with a seed
    rule = dict(do_sample=True, seed=7, top_k=20, temperature=0.9)
    got = qm.generate(x, mask, max_new_tokens=STEPS, **rule)
    n = len(qm._graphs)
    assert torch.equal(qm.generate(x, mask, max_new_tokens=STEPS, **rule), got) and len(qm._graphs) == n
    assert torch.equal(got, qm._generate_sample_static(x, mask, STEPS, 1, 7, temperature=0.9, top_k=20, graph=False))


@pytest.mark.parametrize("gated", [False, True])
def test_end_to_end_logits_error(cuda, models, gated):
    """e(A, B): relative L2 error of teacher-forced logits.  The int8 model on the GPU may be as far from
    the fp32 model as the int8 reference arithmetic is (x 1.5 for quantization flips that the bf16 norms
    and attention cause) plus what bf16 alone costs."""
    m = models[gated]
    g = torch.Generator().manual_seed(9)
    x = torch.randint(2, 192, (3, 11), generator=g)
    dec_ids = torch.randint(2, 192, (3, 7), generator=g)

    @torch.no_grad()
    def logits(model, dev):
        enc, _ = model.encoder(x.to(dev))
        d, _ = model.decoder(dec_ids.to(dev), enc=enc)
        return model.logits(d).float().cpu()

    want = logits(m["f32"], "cpu")

    def e(a):
        return ((a - want).norm() / want.norm()).item()

    e_int8_gpu, e_int8_cpu, e_bf16_gpu = e(logits(m["q"], cuda)), e(logits(m["q_cpu"], "cpu")), e(logits(m["bf"], cuda))
    print(f"gated={gated}: e_int8_gpu {e_int8_gpu:.5f}  e_int8_cpu {e_int8_cpu:.5f}  e_bf16_gpu {e_bf16_gpu:.5f}")
    assert e_int8_cpu > 0 and e_bf16_gpu > 0
    assert e_int8_gpu <= 1.5 * e_int8_cpu + e_bf16_gpu
