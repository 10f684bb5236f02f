"""Int8 T5 on the CPU reference arithmetic: the error of the logits and the tokens against the fp32
float model, the stacked weights and the folded head against the per-matrix forms bit for bit, the
ReLU / residual epilogue rule, every generation mode, the state dict and the refusals."""
import pytest
import torch
import torch.nn.functional as F

from cloudtik_amd import ops
from cloudtik_amd.models.t5 import T5Config, T5ForConditionalGeneration
from cloudtik_amd.models.t5_quant import QuantLinear, QuantT5ForConditionalGeneration, RowQuantized
from cloudtik_amd.ops import reference as ref

SEEDS = (0, 1, 2)


def _config(gated):
    return T5Config(vocab_size=192, d_model=128, d_kv=64, num_heads=2, d_ff=256, num_layers=2, num_decoder_layers=2,
                    relative_attention_num_buckets=8, dropout_rate=0.0, gated_gelu=gated)


_MODELS = {}


def _pair(gated, seed):
    """(float fp32 model, its int8 model, source ids, decoder ids), built once per (FF type, seed)."""
    key = (gated, seed)
    if key not in _MODELS:
        torch.manual_seed(seed)
        m = T5ForConditionalGeneration(_config(gated), dtype=torch.float32).eval()
        g = torch.Generator().manual_seed(100 + seed)
        ids = torch.randint(2, 192, (3, 9), generator=g)
        dec_ids = torch.randint(2, 192, (3, 7), generator=g)
        _MODELS[key] = (m, m.quantize_dynamic(), ids, dec_ids)
    return _MODELS[key]


@torch.no_grad()
def _teacher_forced(model, ids, dec_ids):
    enc, _ = model.encoder(ids)
    d, _ = model.decoder(dec_ids, enc=enc)
    return model.logits(d).float()


# ----------------------------------------------------------------------------- accuracy
@pytest.mark.parametrize("gated", [False, True])
@pytest.mark.parametrize("seed", SEEDS)
def test_logits_error_and_greedy_tokens(gated, seed):
    """Relative L2 error of the teacher-forced logits below 0.02: twice the 0.0101 - 0.0112 measured with the
    reference arithmetic at this config over these seeds and both FF types; and the same greedy tokens."""
    m, q, ids, dec_ids = _pair(gated, seed)
    assert isinstance(q, QuantT5ForConditionalGeneration) and not isinstance(m, QuantT5ForConditionalGeneration)
    a, b = _teacher_forced(q, ids, dec_ids), _teacher_forced(m, ids, dec_ids)
    rel = ((a - b).norm() / b.norm()).item()
    print(f"gated={gated} seed={seed}: rel {rel:.5f}")
    assert 0 < rel < 0.02
    assert torch.equal(q.generate(ids, max_new_tokens=12), m.generate(ids, max_new_tokens=12))


# ----------------------------------------------------------------------------- bit-equality
@pytest.mark.parametrize("gated", [False, True])
def test_stacked_forms_equal_per_matrix(gated):
    m, q, ids, _ = _pair(gated, 0)
    x = torch.randn(2, 5, 128, generator=torch.Generator().manual_seed(3))
    fa, qa = m.decoder.blocks[1].sa, q.decoder.blocks[1].sa
    stacked = qa.qkv(x)
    assert stacked.shape == (2, 5, 3 * 128)
    for j, name in enumerate("qkv"):
        alone = QuantLinear(128, 128).load_weight(getattr(fa, name).weight)
        assert torch.equal(getattr(qa, name)(x), alone(x))                        # the module path's slice
        assert torch.equal(stacked[..., j * 128:(j + 1) * 128], alone(x))         # the fused path's GEMM
    ff, qf = m.encoder.blocks[0].ff, q.encoder.blocks[0].ff
    if gated:
        stacked = qf.wi_stack(x)
        for j, name in enumerate(("wi", "wi_1")):
            alone = QuantLinear(128, 256).load_weight(getattr(ff, name).weight)
            assert torch.equal(getattr(qf, name)(x), alone(x))
            assert torch.equal(stacked[..., j * 256:(j + 1) * 256], alone(x))
    else:
        assert isinstance(qf.wi, QuantLinear) and not hasattr(qf, "wi_stack")
        assert torch.equal(qf.wi(x, act=ops.ACT_RELU), F.relu(qf.wi(x)))


def test_folded_head():
    m, q, _, _ = _pair(False, 0)
    d = torch.randn(4, 128, generator=torch.Generator().manual_seed(4))
    w_q, w_scale = ops.quantize_weight(m.shared.weight)
    assert torch.equal(q.head.w_q, w_q)
    want = ops.linear_i8(d, w_q, w_scale * m.cfg.d_model ** -0.5)
    assert torch.equal(q.logits(d), want)
    # the fused step hands the head int8 rows: the same bits as quantizing the tensor
    y, (qq, s) = ops.rms_norm_quant(d[:, None], q.decoder.final.weight, 1e-6)
    assert torch.equal(q.logits(RowQuantized(qq, s)[:, -1]), q.logits(y[:, -1]))
    # what stays in the model dtype
    assert q.shared.weight.dtype == torch.float32 and torch.equal(q.shared.weight, m.shared.weight)
    assert torch.equal(q.decoder.blocks[0].sa.rel.weight, m.decoder.blocks[0].sa.rel.weight)


@pytest.mark.parametrize("gated", [False, True])
def test_fused_step_equals_module_path_on_the_reference(gated):
    """``_decode_step_static`` of the int8 model (fused ops) against the float model's step run on the
    int8 modules, on the reference arithmetic."""
    _, q, ids, _ = _pair(gated, 1)
    cfg, T, B = q.cfg, 4, ids.shape[0]
    with torch.no_grad():
        enc, _ = q.encoder(ids)
        cross = [(b.ca._split(b.ca.k(enc)), b.ca._split(b.ca.v(enc))) for b in q.decoder.blocks]
        slots = torch.arange(T)

        def run(step_fn):
            kc = [torch.zeros(B, T, cfg.num_heads, cfg.d_kv) for _ in q.decoder.blocks]
            vc = [torch.zeros_like(k) for k in kc]
            cur, outs = torch.zeros(B, 1, dtype=torch.long), []
            for t in range(2):
                h = step_fn(cur, torch.tensor([t]), slots, kc, vc, cross, None)
                outs.append(q.logits(h[:, -1]))
                cur = outs[-1].argmax(-1)[:, None]
            return outs

        fused = run(q._decode_step_static)
        plain = run(lambda *a: T5ForConditionalGeneration._decode_step_static(q, *a))
    for a, b in zip(fused, plain):
        assert torch.equal(a, b)


# ----------------------------------------------------------------------------- the written rule
def test_epilogue_relu_and_residual_rule():
    """Hand-built accumulators: f = acc * (sa * sw) as two fp32 multiplies, + bias, the activation, the
    rounding to dtype, then the residual added to the ROUNDED value and rounded again."""
    bf = torch.bfloat16
    acc = torch.tensor([[3, -5, 257, 0], [100, -100, 1, 2]], dtype=torch.int32)
    sa, sw = torch.tensor([0.5, 0.25]), torch.tensor([1.0, 2.0, 1.0, 3.0])
    bias = torch.tensor([0.0, 1.0, 0.0, -1.0])
    f = torch.tensor([[1.5, -5.0, 128.5, 0.0], [25.0, -50.0, 0.25, 1.5]]) + bias
    assert torch.equal(ref.dequant_epilogue(acc, sa, sw, bias), f)
    assert torch.equal(ref.dequant_epilogue(acc, sa, sw, bias, ops.ACT_RELU), f.clamp(min=0))
    assert torch.equal(ref.dequant_epilogue(acc, sa, sw, bias, ops.ACT_RELU, bf), f.clamp(min=0).to(bf))
    # 128.5 rounds to 128 in bf16 (ulp 1) BEFORE the residual 0.5 is added: 128.5 -> 128 (ties to even), where
    # adding first would give 129
    res = torch.tensor([[0.5, 0.5, 0.5, 0.5], [1.0, 1.0, 1.0, 1.0]], dtype=bf)
    got = ref.dequant_epilogue(acc, sa, sw, None, ops.ACT_NONE, bf, res)
    assert got.dtype == bf and got[0, 2].item() == 128.0
    assert ((f - bias)[0, 2] + 0.5).to(bf).item() == 129.0
    assert torch.equal(got, ((f - bias).to(bf).float() + res.float()).to(bf))
    # the op: equal to the linear followed by the add, and to relu of the linear
    x = torch.randn(5, 64, generator=torch.Generator().manual_seed(0)).to(bf)
    w_q, w_s = ops.quantize_weight(torch.randn(64, 64, generator=torch.Generator().manual_seed(1)))
    r = torch.randn(5, 64, generator=torch.Generator().manual_seed(2)).to(bf)
    h = ops.linear_i8(x, w_q, w_s)
    assert h.dtype == bf
    assert torch.equal(ops.linear_i8(x, w_q, w_s, residual=r), r + h)
    assert torch.equal(ops.linear_i8(x, w_q, w_s, act=ops.ACT_RELU), F.relu(h))
    with pytest.raises(ValueError):
        ops.linear_i8(x, w_q, w_s, act=ops.ACT_RELU, residual=r)
    with pytest.raises(ValueError):                       # the op's ReLU is the bias-free one
        ops.linear_i8(x, w_q, w_s, torch.zeros(64, dtype=bf), ops.ACT_RELU)
    with pytest.raises(ValueError):
        ref.dequant_epilogue(acc, sa, sw, None, ops.ACT_RELU, bf, res)
    with pytest.raises(ValueError):
        ops.linear_i8(x, w_q, w_s, residual=r[:4])
    with pytest.raises(ValueError):
        ref.dequant_epilogue(acc, sa, sw, None, ops.ACT_NONE, torch.float32, res)     # a residual of another dtype


def test_rms_norm_quant_reference():
    g = torch.Generator().manual_seed(6)
    x, r = torch.randn(3, 4, 64, generator=g).bfloat16(), torch.randn(3, 4, 64, generator=g).bfloat16()
    gamma = (1 + 0.1 * torch.randn(64, generator=g)).bfloat16()
    x[1, 2], r[1, 2] = 0, 0
    y, (q, s) = ops.rms_norm_quant(x, gamma, 1e-6, r)
    assert torch.equal(y, ops.layer_norm(x, gamma, None, eps=1e-6, residual=r, training=False, rms=True))
    q_want, s_want = ref.quantize_rows(y)
    assert torch.equal(q, q_want) and torch.equal(s, s_want) and s.shape == (3, 4)
    assert s[1, 2] == 0 and not q[1, 2].any()
    assert ops.rms_norm_quant(x, gamma, 1e-6, emit_y=False)[0] is None


# ----------------------------------------------------------------------------- the model's interface
@pytest.mark.parametrize("gated", [False, True])
def test_generation_modes_and_state_dict_round_trip(gated):
    _, q, ids, _ = _pair(gated, 2)
    mask = torch.ones_like(ids)
    mask[1, 6:] = 0
    greedy = q.generate(ids, mask, max_new_tokens=6, no_repeat_ngram_size=2)
    beam, score = q.generate(ids, mask, max_new_tokens=6, num_beams=3, num_return_sequences=2, return_scores=True)
    sample = q.generate(ids, mask, max_new_tokens=6, do_sample=True, seed=5, top_k=10, num_return_sequences=2)
    assert greedy.shape == (3, 6) and beam.shape == (6, 6) and score.shape == (6,) and sample.shape == (6, 6)
    assert torch.equal(sample, q.generate(ids, mask, max_new_tokens=6, do_sample=True, seed=5, top_k=10,
                                          num_return_sequences=2))
    sd = q.state_dict()
    assert sd["decoder.blocks.0.sa.qkv.w_q"].dtype == torch.int8 and sd["head.w_scale"].dtype == torch.float32
    assert not any(k.endswith((".q.weight", ".wi.weight", ".sa.q.w_q")) for k in sd)
    skeleton = QuantT5ForConditionalGeneration(_config(gated), dtype=torch.float32)
    assert not skeleton.head.w_q.any()
    skeleton.load_state_dict(sd)
    assert torch.equal(skeleton.generate(ids, mask, max_new_tokens=6, no_repeat_ngram_size=2), greedy)
    assert torch.equal(skeleton.generate(ids, mask, max_new_tokens=6, num_beams=3, num_return_sequences=2), beam)


def test_refusals():
    m, q, ids, dec_ids = _pair(False, 0)
    with pytest.raises(RuntimeError, match="inference-only"):
        q(ids, dec_ids)
    with pytest.raises(RuntimeError, match="inference-only"):
        q.train()
    assert q.eval() is q and not q.training and q.quantize_dynamic() is q
    assert not any(p.requires_grad for p in q.parameters())
    assert m.training is False and isinstance(m.decoder.blocks[0].sa.q, torch.nn.Linear)      # the float model is untouched
