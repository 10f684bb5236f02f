"""Static int8 post-training quantization on the CPU path: the rounding rule against a given
range, the static linear, calibration, the config with two approaches, quantize -> load ->
predict with a static config and the trial ladder."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F
import yaml

from cloudtik_amd import ops
from cloudtik_amd.models import bert_quant
from cloudtik_amd.models.bert import BertConfig
from cloudtik_amd.models.bert_quant import SITES, QuantBertClassifier, calibrate
from cloudtik_amd.modeling.transfer_learning import (HashTokenizer, TextClassificationDataset, get_model,
                                                     load_model)
from cloudtik_amd.modeling.transfer_learning import quantization as Q
from cloudtik_amd.modeling.transfer_learning.text_classification import BertClassifier
from cloudtik_amd.ops import reference as ref

STATIC, DYNAMIC = "post_training_static_quant", "post_training_dynamic_quant"


# ----------------------------------------------------------------------------- the rule
def _formula(x, amax):
    """The rule written out element by element in numpy fp32."""
    x = x.float().numpy().astype(np.float32)
    amax = np.float32(amax)
    inv = np.float32(127.0) / amax if amax > 0 else np.float32(0.0)      # one division
    q = np.zeros(x.shape, np.int8)
    for i, v in enumerate(x.reshape(-1)):
        r = np.rint(np.float32(v * inv))                 # one fp32 multiply, round half to even
        q.reshape(-1)[i] = np.int8(min(max(r, -127.0), 127.0))
    return torch.from_numpy(q)


def test_static_scales_are_single_divisions():
    for amax in (3.0, 0.1, 2.9375, 1e-3, 7.3, 511.0):
        a = np.float32(amax)
        scale, inv = ref.static_scales(float(a))
        assert isinstance(scale, float) and isinstance(inv, float)
        assert scale == float(a / np.float32(127.0)) and inv == float(np.float32(127.0) / a)
        assert float(np.float32(scale)) == scale and float(np.float32(inv)) == inv    # exact fp32 values
    assert ref.static_scales(0.0) == (0.0, 0.0)
    for bad in (-1.0, float("inf"), float("nan"), 1e-44):
        with pytest.raises(ValueError):
            ref.static_scales(bad)


@pytest.mark.parametrize("fn", [ops.quantize_static, ref.quantize_static])
def test_quantize_static_matches_formula(fn):
    torch.manual_seed(0)
    x = (torch.randn(6, 32) * 2).to(torch.bfloat16).float()
    x[0, :4] = torch.tensor([9.0, -9.0, 3.0, -3.0])     # beyond and at the range, both signs
    q = fn(x, 3.0)
    assert q.dtype == torch.int8 and q.shape == x.shape
    assert torch.equal(q, _formula(x, 3.0))
    assert q[0, :4].tolist() == [127, -127, 127, -127]
    assert (x.abs() > 3.0).sum() > 4 and q.abs().max() == 127          # values beyond amax saturate
    # amax = 127 makes inv 1: exact .5 ties go to the even neighbour
    t = torch.tensor([127.0, 0.5, 1.5, -2.5, -0.5, 126.5, 300.0, -128.0])
    assert fn(t, 127.0).tolist() == [127, 0, 2, -2, 0, 126, 127, -127]
    # amax = 0: q 0 (and scale 0)
    assert not fn(x, 0.0).any() and ref.static_scales(0.0)[0] == 0.0
    # a negative-only tensor
    n = -x.abs() - 0.5
    qn = fn(n, 2.0)
    assert torch.equal(qn, _formula(n, 2.0)) and qn.max() < 0 and qn.min() == -127
    # many ranges: 127 / amax must be ONE division (reciprocal-then-multiply rounds twice)
    g = torch.Generator().manual_seed(67 * 10007 + 128)
    y = (torch.randn(67, 128, generator=g) * 3).to(torch.bfloat16)
    for row in y[:24]:
        amax = float(row.float().abs().max())
        assert torch.equal(fn(row, amax), _formula(row, amax))
        assert torch.equal(fn(row, amax), ref.quantize_rows(row[None])[0][0])   # the row rule at its own maximum
    for bad in (-1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            fn(x, bad)


def test_linear_i8_static_forms():
    torch.manual_seed(1)
    M, N, K = 24, 64, 128
    x, w, b = torch.randn(M, K), torch.randn(N, K) * K ** -0.5, torch.randn(N)
    wq, ws = ops.quantize_weight(w)
    a_amax = float(x.abs().max()) * 0.75                 # some inputs saturate
    y = ops.linear_i8_static(x, a_amax, wq, ws, b)
    assert y.dtype == torch.float32 and y.shape == (M, N)
    # the pre-quantized form is the same computation
    xq = ops.quantize_static(x, a_amax)
    assert torch.equal(ops.linear_i8_static(xq, a_amax, wq, ws, b), y)
    assert torch.equal(ref.linear_i8_static(xq, a_amax, wq, ws, b), y)
    # it is dequant_epilogue with the scalar scale
    scale = torch.full((M,), ref.static_scales(a_amax)[0])
    assert torch.equal(y, ref.dequant_epilogue(ref.gemm_i8_nt_raw(xq, wq), scale, ws, b))
    # close to the float linear of the clipped input (2/127 as for the dynamic linear)
    yr = F.linear(x.clamp(-a_amax, a_amax), w)
    y0 = ops.linear_i8_static(x, a_amax, wq, ws)
    assert ((y0 - yr).norm() / yr.norm()).item() < 2 / 127
    # int8 out is quantize_static of the result rounded to dtype first
    for act in (ops.ACT_NONE, ops.ACT_GELU):
        for dt in (torch.float32, torch.bfloat16):
            yb = ops.linear_i8_static(xq, a_amax, wq, ws, b, act, dtype=dt)
            assert yb.dtype == dt
            out_amax = float(yb.float().abs().max()) * 0.5
            q = ops.linear_i8_static(xq, a_amax, wq, ws, b, act, out_amax=out_amax, dtype=dt)
            assert q.dtype == torch.int8 and torch.equal(q, ref.quantize_static(yb, out_amax))
            assert (q.abs() == 127).sum() > 0
    torch.testing.assert_close(ops.linear_i8_static(xq, a_amax, wq, ws, b, ops.ACT_GELU), F.gelu(y))
    with pytest.raises(ValueError):
        ops.linear_i8_static(xq, a_amax, wq, ws, b, ops.ACT_RELU)
    with pytest.raises(ValueError):
        ops.linear_i8_static(xq, -1.0, wq, ws, b)


def test_layer_norm_quant_cpu():
    torch.manual_seed(2)
    x, r = torch.randn(5, 64), torch.randn(5, 64)
    g, b, bias = torch.rand(64) + 0.5, torch.randn(64) * 0.1, torch.randn(64) * 0.1
    y, q = ops.layer_norm_quant(x, g, b, 1e-12, bias=bias, residual=r, amax=1.5)
    assert torch.equal(y, ops.layer_norm(x, g, b, 1e-12, bias=bias, residual=r, training=False))
    assert torch.equal(q, ref.quantize_static(y, 1.5)) and (q.abs() == 127).any()
    y2, none = ops.layer_norm_quant(x, g, b, 1e-12, bias=bias, residual=r)
    assert none is None and torch.equal(y2, y)


# ----------------------------------------------------------------------------- calibration
def test_calibrate_matches_hooks():
    """The ranges equal a brute-force maximum over the inputs of the four linears, taken from the
    float model itself: forward hooks give every layer's input and output, and the tensors in
    between are recomputed from the layer's own weights."""
    torch.manual_seed(3)
    cfg = BertConfig.tiny()
    f = BertClassifier(cfg, 4, device="cpu", dtype=torch.float32).eval()
    batches = []
    for n in (3, 2):
        ids = torch.randint(1, cfg.vocab_size, (n, 32))
        mask = torch.ones(n, 32, dtype=torch.long)
        mask[0, 20:] = 0
        batches.append({"input_ids": ids, "attention_mask": mask})
    want = torch.zeros(cfg.num_hidden_layers, 4)

    def hook(i):
        def fn(layer, args, out):
            x, key_bias = args
            qkv = F.linear(x, layer.qkv_weight, layer.qkv_bias)
            ctx = ops.attention_packed(qkv, cfg.num_attention_heads, key_bias, p=0.0, training=False)
            a = F.linear(ctx, layer.out_weight)
            x1 = ops.layer_norm(a, layer.ln1_weight, layer.ln1_bias, cfg.layer_norm_eps, bias=layer.out_bias,
                                residual=x, training=False)
            h = F.gelu(F.linear(x1, layer.ffn1_weight, layer.ffn1_bias))
            y = ops.layer_norm(F.linear(h, layer.ffn2_weight), layer.ln2_weight, layer.ln2_bias,
                               cfg.layer_norm_eps, bias=layer.ffn2_bias, residual=x1, training=False)
            torch.testing.assert_close(y, out)           # the recomputation is the layer
            for k, t in enumerate((x, ctx, x1, h)):
                want[i, k] = max(want[i, k], t.abs().max())
        return fn

    handles = [l.register_forward_hook(hook(i)) for i, l in enumerate(f.bert.layers)]
    with torch.no_grad():
        for b in batches:
            f(b["input_ids"], b["attention_mask"])
    for h in handles:
        h.remove()
    got = calibrate(f, batches)
    assert len(got) == cfg.num_hidden_layers and all(len(r) == 4 and all(isinstance(v, float) for v in r) for r in got)
    torch.testing.assert_close(torch.tensor(got), want, rtol=1e-5, atol=0)
    # the qkv range of layer 0 is the embedding LayerNorm's output: exactly the hook's value
    assert got[0][0] == want[0, 0].item()
    assert got == calibrate(f, [(b["input_ids"], b["attention_mask"]) for b in batches])   # tuples too
    with pytest.raises(ValueError):
        calibrate(f, [])


def test_static_model_sites_and_fuse():
    """Producers emit int8 only for int8 consumers; fused and unfused agree bit for bit."""
    torch.manual_seed(4)
    cfg = BertConfig.tiny()
    f = BertClassifier(cfg, 4, device="cpu", dtype=torch.float32).eval()
    ids = torch.randint(1, cfg.vocab_size, (2, 32))
    mask = torch.ones(2, 32, dtype=torch.long)
    mask[1, 9:] = 0
    amax = calibrate(f, [(ids, mask)])
    want = f(ids, mask)
    for sites in (SITES, ("qkv", "out", "ffn1"), ("qkv", "ffn1"), ("ffn2",), ()):
        a = QuantBertClassifier.from_float(f, sites, act_amax=amax)
        b = QuantBertClassifier.from_float(f, sites, act_amax=amax, fuse=False)
        assert a.act_amax == amax and a.sites_per_layer == [[s for s in SITES if s in sites]] * 2
        ya, yb = a(ids, mask), b(ids, mask)
        assert torch.equal(ya, yb)
        assert ((ya - want).norm() / want.norm()).item() < 0.05
    assert "act_amax" not in " ".join(a.state_dict())     # the ranges are not tensors of the model
    assert QuantBertClassifier.from_float(f).act_amax is None
    with pytest.raises(ValueError):
        QuantBertClassifier.from_float(f, SITES, act_amax=amax[:1])
    with pytest.raises(ValueError):
        QuantBertClassifier.from_float(f, SITES, act_amax=[[1.0, -1.0, 1.0, 1.0]] * 2)


# ----------------------------------------------------------------------------- the model API
def _keyword_data(n=400, seed=0):
    rng = np.random.default_rng(seed)
    pos, neg = ["great", "good", "excellent", "love"], ["bad", "awful", "terrible", "hate"]
    filler = ["the", "movie", "was", "plot", "acting", "really", "quite"]
    texts, labels = [], []
    for _ in range(n):
        y = int(rng.integers(0, 2))
        words = list(rng.choice(filler, 6)) + [rng.choice(pos if y else neg)]
        rng.shuffle(words)
        texts.append(" ".join(words))
        labels.append(y)
    tok = HashTokenizer(vocab_size=512, max_length=16)
    return (TextClassificationDataset(texts[:320], labels[:320], tok),
            TextClassificationDataset(texts[320:], labels[320:], tok))


@pytest.fixture(scope="module")
def trained(tmp_path_factory):
    """(model, eval dataset, export dir, static config path): bert-tiny trained on the keyword task."""
    torch.manual_seed(0)
    ds, ev = _keyword_data()
    m = get_model("bert-tiny", use_case="text_classification", num_classes=2, device="cpu")
    m.train(ds, epochs=4, batch_size=32, lr=1e-3, log_every=0)
    root = tmp_path_factory.mktemp("quant_static")
    saved = str(root / "fp32")
    m.export(saved)
    cfg = str(root / "conf" / "static.yaml")
    m.export_quantization_config(cfg, ev, batch_size=16, approach=STATIC, calibration_sampling_size=48)
    return m, ev, saved, cfg


def test_config_approaches(trained, tmp_path, monkeypatch):
    m, ev, _, cfg_path = trained
    monkeypatch.delenv("OUTPUT_DIR", raising=False)
    cfg = Q.read_config(cfg_path)
    assert cfg["quantization"] == {"approach": STATIC, "calibration": {"sampling_size": 48}}
    with open(cfg_path) as f:
        assert yaml.safe_load(f) == cfg and yaml.safe_load(yaml.safe_dump(cfg)) == cfg
    # the alias takes the two as trailing keyword arguments; the default sampling size is 100
    p = str(tmp_path / "alias.yaml")
    m.export_neural_compressor_config(p, ev, 8, approach=STATIC)
    assert Q.read_config(p)["quantization"] == {"approach": STATIC, "calibration": {"sampling_size": 100}}
    # a dynamic config is what build_config gives, key for key and in the same order
    d = str(tmp_path / "dyn.yaml")
    m.export_quantization_config(d, ev, 8)
    want = Q.build_config(m.model_name, ev, 8, 0.01, 0, 50, 9527, '')
    got = Q.read_config(d)
    assert got == want and got["quantization"] == {"approach": DYNAMIC}
    with open(d) as f:
        assert f.read() == yaml.safe_dump(want, sort_keys=False)
    m.export_quantization_config(d, ev, 8, overwrite=True, approach=DYNAMIC, calibration_sampling_size=7)
    assert Q.read_config(d) == want                      # the sampling size is a static setting
    # bad values raise and write nothing
    p = str(tmp_path / "bad.yaml")
    bad = [dict(approach="post_training_weight_only"), dict(approach="static"), dict(approach=None),
           dict(approach=STATIC, calibration_sampling_size=0), dict(approach=STATIC, calibration_sampling_size=-3),
           dict(approach=STATIC, calibration_sampling_size=2.5), dict(approach=STATIC, calibration_sampling_size="9"),
           dict(approach=STATIC, calibration_sampling_size=None), dict(approach=STATIC, calibration_sampling_size=True),
           dict(calibration_sampling_size=0)]
    for kw in bad:
        with pytest.raises(ValueError):
            m.export_quantization_config(p, ev, 8, **kw)
        assert not os.path.exists(p)
        with pytest.raises(ValueError):
            m.export_neural_compressor_config(p, ev, 8, **kw)
        assert not os.path.exists(p)
    # read_config still rejects other approaches
    with open(p, "w") as f:
        yaml.safe_dump(dict(want, quantization={"approach": "quant_aware_training"}), f)
    with pytest.raises(ValueError):
        Q.read_config(p)


def test_static_quantize_reload_predict(trained, tmp_path):
    """Measured on the CPU: float accuracy 1.0, static int8 accuracy 1.0.  One range per tensor
    may move the logits further than per-token scales do (a property of the format, not a
    defect), so the outputs are compared by argmax and accuracy, with no bound on their distance."""
    from safetensors.torch import load_file
    m, ev, saved, cfg = trained
    acc_fp = m.evaluate(ev)["accuracy"]
    assert acc_fp > 0.85
    out = str(tmp_path / "int8")
    path = m.quantize(saved, out, cfg, dataset=ev)
    assert path == os.path.join(out, "model.safetensors") and os.path.isfile(path)
    L = m.cfg.num_hidden_layers

    with open(os.path.join(out, "model_config.json")) as f:
        block = json.load(f)["quantization"]
    assert block["approach"] == STATIC and block["trial"] == 1
    assert block["sites"] == [list(SITES)] * L
    assert block["calibration"] == {"sampling_size": 48, "num_examples": 48}
    amax = block["act_amax"]
    assert len(amax) == L and all(len(r) == 4 for r in amax)
    assert all(isinstance(v, float) and v > 0 and float(np.float32(v)) == v for r in amax for v in r)
    assert block["accuracy"]["fp32"] == pytest.approx(acc_fp)
    # the ranges are those of the first 48 examples at the config's batch size
    sub = [{"input_ids": ev.ids[i:i + 16], "attention_mask": ev.mask[i:i + 16]} for i in range(0, 48, 16)]
    assert amax == calibrate(m.model, sub)

    # the int8 weights are what the dynamic approach saves
    sd = load_file(path)
    dyn_cfg, dyn_out = str(tmp_path / "dyn.yaml"), str(tmp_path / "dyn")
    m.export_quantization_config(dyn_cfg, ev, batch_size=16)
    dyn = load_file(m.quantize(saved, dyn_out, dyn_cfg, dataset=ev))
    assert set(sd) == set(dyn) and all(torch.equal(sd[k], dyn[k]) for k in sd)
    assert sd["bert.layers.0.qkv_weight_q"].dtype == torch.int8 and "bert.layers.0.qkv_weight" not in sd
    with open(os.path.join(dyn_out, "model_config.json")) as f:
        dyn_block = json.load(f)["quantization"]
    assert list(dyn_block) == ["approach", "sites", "accuracy", "accuracy_criterion_relative", "trial", "trials"]
    assert dyn_block["approach"] == DYNAMIC

    q = load_model(out, device="cpu")
    assert isinstance(q.model, QuantBertClassifier) and q.quantization == block
    assert q.model.act_amax == amax
    # the reloaded model computes what the model that was exported computed, bit for bit
    pre = QuantBertClassifier.from_float(m.model, SITES, act_amax=amax)
    with torch.no_grad():
        assert torch.equal(q.model(ev.ids[:32], ev.mask[:32]), pre(ev.ids[:32], ev.mask[:32]))
    acc_q = q.evaluate(ev)["accuracy"]
    assert acc_q == pytest.approx(block["accuracy"]["int8"])
    print(f"accuracy: float {acc_fp}, static int8 {acc_q}")
    assert (acc_fp - acc_q) / acc_fp <= 0.01             # the config's criterion
    p_q, p_fp = q.predict(ev.ids[:8], ev.mask[:8]), m.predict(ev.ids[:8], ev.mask[:8])
    print(f"largest probability distance {(p_q - p_fp).abs().max().item():.3f}")
    assert p_q.shape == p_fp.shape and torch.equal(p_q.argmax(-1), p_fp.argmax(-1))
    with pytest.raises(RuntimeError):
        q.train(ev)

    # export of the loaded model round-trips; benchmark accepts it as an int8 model
    again = str(tmp_path / "again")
    q.export(again)
    q2 = load_model(again, device="cpu")
    assert q2.quantization == block and torch.equal(q2.predict(ev.ids[:8], ev.mask[:8]), p_q)
    acc = m.benchmark(out, cfg, mode="accuracy", model_type="int8", dataset=ev)
    assert acc == {"accuracy": pytest.approx(acc_q)}
    res = m.benchmark(out, cfg, mode="performance", model_type="int8", warmup=1, iters=2)
    assert res["batch_size"] == 16 and res["latency_ms"] > 0
    with pytest.raises(ValueError):
        m.benchmark(out, cfg, model_type="fp32")          # it is an int8 model
    with pytest.raises(ValueError):
        m.quantize(out, str(tmp_path / "twice"), cfg, dataset=ev)     # already quantized


def test_static_needs_dataset(trained, tmp_path):
    m, ev, saved, cfg = trained
    out = tmp_path / "o"
    with pytest.raises(ValueError, match="dataset"):
        m.quantize(saved, str(out), cfg)
    assert not out.exists()


def test_static_trial_ladder(trained, tmp_path, monkeypatch):
    m, ev, saved, cfg = trained
    calls, calibrations = [], []
    real = bert_quant.calibrate

    def counting(model, batches):
        batches = list(batches)
        calibrations.append((type(model).__name__, sum(len(b["input_ids"]) for b in batches)))
        return real(model, batches)

    def fails_all_four(self, wrapper, dataset, batch_size):
        sites = wrapper.model.sites_per_layer[0] if wrapper.quantization else None
        calls.append(sites)
        if sites is not None:                            # every trial carries the same ranges
            assert wrapper.model.act_amax is not None and wrapper.quantization["approach"] == STATIC
        return 0.5 if sites == list(SITES) else 1.0

    monkeypatch.setattr(bert_quant, "calibrate", counting)
    monkeypatch.setattr(type(m), "_trial_accuracy", fails_all_four)
    out = str(tmp_path / "t2")
    assert m.quantize(saved, out, cfg, dataset=ev)
    assert calls == [None, list(SITES), ["qkv", "out", "ffn1"]]
    assert calibrations == [("BertClassifier", 48)]       # once, on the float model, 48 examples
    with open(os.path.join(out, "model_config.json")) as f:
        block = json.load(f)["quantization"]
    assert block["trial"] == 2 and block["sites"] == [["qkv", "out", "ffn1"]] * m.cfg.num_hidden_layers
    assert [t["relative_loss"] for t in block["trials"]] == [0.5, 0.0]
    assert len(block["act_amax"]) == m.cfg.num_hidden_layers and len(block["act_amax"][0]) == 4
    q = load_model(out, device="cpu")
    assert q.model.bert.layers[0].ffn2_weight.dtype == torch.float32
    assert q.model.bert.layers[0].ffn1_weight_q.dtype == torch.int8
    assert q.predict(ev.ids[:4], ev.mask[:4]).shape == (4, 2)

    monkeypatch.setattr(type(m), "_trial_accuracy",
                        lambda self, wrapper, dataset, batch_size: 0.5 if wrapper.quantization else 1.0)
    none = str(tmp_path / "none")
    assert m.quantize(saved, none, cfg, dataset=ev) is None
    assert not os.path.exists(os.path.join(none, "model.safetensors"))
    assert not os.path.exists(os.path.join(none, "model_config.json"))
    assert len(calibrations) == 2

    # a sampling size beyond the dataset calibrates on all of it
    big = str(tmp_path / "big.yaml")
    m.export_quantization_config(big, ev, 16, approach=STATIC, calibration_sampling_size=1000)
    monkeypatch.setattr(type(m), "_trial_accuracy", lambda self, wrapper, dataset, batch_size: 1.0)
    assert m.quantize(saved, str(tmp_path / "all"), big, dataset=ev)
    assert calibrations[-1] == ("BertClassifier", len(ev))
    with open(os.path.join(str(tmp_path / "all"), "model_config.json")) as f:
        assert json.load(f)["quantization"]["calibration"] == {"sampling_size": 1000, "num_examples": len(ev)}
