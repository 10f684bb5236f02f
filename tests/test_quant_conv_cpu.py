"""The static int8 convolution on the CPU: the reference op against independent formulations,
BatchNorm folding, the quantized ResNet and the image quantization workflow."""
import json
import os

import pytest
import torch
import torch.nn.functional as F

from cloudtik_amd import ops
from cloudtik_amd.modeling.transfer_learning import image_quantization as iq
from cloudtik_amd.modeling.transfer_learning.datasets import (HashTokenizer, TextClassificationDataset,
                                                              synthetic_image_dataset)
from cloudtik_amd.modeling.transfer_learning.image_classification import ImageClassificationModel
from cloudtik_amd.modeling.transfer_learning.model_factory import load_model
from cloudtik_amd.models import resnet_quant as rq
from cloudtik_amd.models.resnet import BasicBlock, Bottleneck, ResNet
from cloudtik_amd.ops import reference as ref

from quant_conv_util import conv_case, one_hot_rows, randomize_bn, shifted, tiny_images, tiny_resnet


# ----------------------------------------------------------------------------- 1. the reference op
@pytest.mark.parametrize("case", [(2, 7, 7, 64, 64, 3, 1), (1, 14, 14, 128, 128, 3, 2), (2, 7, 7, 256, 64, 1, 1),
                                  (2, 14, 14, 64, 128, 1, 2), (1, 9, 5, 64, 64, 3, 1)],
                         ids=lambda c: "x".join(map(str, c)))
@pytest.mark.parametrize("relu,with_res,out_amax,dtype", [(False, False, None, torch.float32),
                                                          (True, True, None, torch.bfloat16),
                                                          (True, True, 1.5, torch.bfloat16),
                                                          (False, True, 1.5, torch.float32)])
def test_reference_against_fp64_conv(case, relu, with_res, out_amax, dtype):
    N, H, W, ci, co, R, stride = case
    x, w_q, w_s, bias = conv_case(N, H, W, ci, co, R, seed=sum(case))
    a_amax, res_amax = 2.0, 3.0
    # independent: F.conv2d in fp64 on the integer values (exact: |acc| < 2^53), same epilogue
    w4 = w_q.view(co, R, R, ci).permute(0, 3, 1, 2).double()
    acc = F.conv2d(x.double(), w4, stride=stride, padding=R // 2)
    assert torch.equal(acc, ref.conv_i8_acc(x, w_q, stride, R // 2).double())
    sa = torch.tensor(ref.static_scales(a_amax)[0], dtype=torch.float32)
    f = acc.float() * (sa * w_s).view(1, -1, 1, 1)
    f = f + bias.view(1, -1, 1, 1)
    res = None
    if with_res:
        res = torch.randint(-127, 128, f.shape, generator=torch.Generator().manual_seed(1), dtype=torch.int8)
        f = f + res.float() * torch.tensor(ref.static_scales(res_amax)[0], dtype=torch.float32)
    if relu:
        f = torch.relu(f)
    want = f.to(dtype)
    if out_amax is not None:
        want = ref.quantize_static(want, out_amax)
    got = ops.conv2d_i8_static(x, a_amax, w_q, w_s, bias, stride, R // 2, relu, res, res_amax if with_res else None,
                               out_amax, dtype=dtype)
    assert got.dtype == want.dtype and torch.equal(got, want)
    assert ops.conv2d_i8_static(x, a_amax, w_q, w_s, bias, stride, R // 2, relu, res, res_amax if with_res else None,
                                out_amax).dtype == (torch.float32 if out_amax is None else torch.int8)


def test_reference_rejects():
    x, w_q, w_s, bias = conv_case(1, 6, 6, 64, 64, 3, seed=1)
    with pytest.raises(ValueError):
        ops.conv2d_i8_static(x, 1.0, w_q, w_s, bias, 1, 1, False, dilation=2)
    with pytest.raises(ValueError):
        ops.conv2d_i8_static(x, 1.0, w_q, w_s, bias, 1, 1, False, groups=2)
    with pytest.raises(ValueError):
        ops.conv2d_i8_static(x, 1.0, w_q[:, :288], w_s, bias, 1, 1, False)      # a grouped weight's rows
    with pytest.raises(ValueError):
        ops.conv2d_i8_static(x, float("inf"), w_q, w_s, bias, 1, 1, False)
    with pytest.raises(ValueError):
        ops.conv2d_i8_static(x, 1.0, w_q, w_s, bias, 1, 1, False, res_q=torch.zeros(1, 64, 6, 6, dtype=torch.int8))
    with pytest.raises(TypeError):
        ops.conv2d_i8_static(x.float(), 1.0, w_q, w_s, bias, 1, 1, False)


# ----------------------------------------------------------------------------- 2. one-hot taps
@pytest.mark.parametrize("stride", [1, 2])
def test_one_hot_taps(stride):
    x = torch.randint(-127, 128, (2, 64, 7, 5), generator=torch.Generator().manual_seed(3), dtype=torch.int8)
    one, zero = torch.ones(64), torch.zeros(64)
    for r in range(3):
        for s in range(3):
            y = ops.conv2d_i8_static(x, 127.0, one_hot_rows(64, 3, r, s), one, zero, stride, 1, False)
            assert torch.equal(y, shifted(x, r, s, 3, stride).float()), (r, s)


# ----------------------------------------------------------------------------- 3. fold_bn
@pytest.mark.parametrize("k,stride", [(1, 1), (3, 2)])
def test_fold_bn(k, stride):
    torch.manual_seed(k)
    b = randomize_bn(Bottleneck(64, 64, stride, downsample=True, dtype=torch.float32),
                     torch.Generator().manual_seed(9)).eval()
    conv, bn = (b.conv1, b.bn1) if k == 1 else (b.conv2, b.bn2)
    x = torch.randn(2, 64, 9, 9)
    with torch.no_grad():
        z = F.conv2d(x, conv.weight, stride=conv.stride, padding=conv.padding)
        want = F.batch_norm(z, bn.running_mean, bn.running_var, bn.weight, bn.bias, False, 0.0, bn.eps)
        rows, bias = ops.fold_bn(conv.weight, bn)
        assert rows.shape == (64, k * k * 64) and rows.dtype == bias.dtype == torch.float32
        w = rows.view(64, k, k, 64).permute(0, 3, 1, 2)
        got = F.conv2d(x, w, bias, stride=conv.stride, padding=conv.padding)
    # fp32 throughout: the two differ by the order of a few roundings of O(1) values
    assert (got - want).abs().max() < 1e-4 * want.abs().max()
    assert torch.equal(rows, ops.conv.weight_rows(w).contiguous())             # tap-major, as the GPU conv has them


# ----------------------------------------------------------------------------- 4. the model
@pytest.fixture(scope="module")
def tiny():
    m = tiny_resnet(0)
    x = tiny_images()
    with torch.no_grad():
        y = m(x)
    return m, rq.calibrate(m, [x]), x, y


def test_calibrate_sites(tiny):
    m, amax, x, _ = tiny
    want = {"stem"} | {f"layer{i}.0.{s}" for i in range(1, 5) for s in ("bn1", "bn2", "down_bn", "out")}
    assert set(amax) == want and all(isinstance(v, float) and v > 0 for v in amax.values())
    with torch.no_grad():
        assert amax["stem"] == m.stem(x).abs().max().item()
        assert amax["layer1.0.out"] == m.layer1(m.stem(x)).abs().max().item()
    two = rq.calibrate(m, [x[:4], (x[4:], None)])                             # maxima over batches; (x, y) pairs
    assert two == pytest.approx(amax, rel=1e-5)
    with pytest.raises(ValueError):
        rq.calibrate(m, [])
    assert not m.training


@pytest.mark.parametrize("sites", list(rq.TRIALS) + [("layer1", "layer3")])
def test_from_float_sites_and_joins(tiny, sites):
    m, amax, x, y = tiny
    q = rq.QuantResNet.from_float(m, sites, amax)
    assert q.sites == list(sites) and not q.training
    prev_int8, entries = False, {}
    for i, name in enumerate(rq.STAGES):
        blk = getattr(q, name)[0]
        if name in sites:
            assert isinstance(blk, rq.QuantBottleneck) and blk.conv3_weight_q.any()
            nxt = i + 1 < 4 and rq.STAGES[i + 1] in sites
            assert blk.float_out == (not nxt)                                 # bf16 / fp32 in front of a float consumer
            if not prev_int8:                                                 # a float tensor enters: one cast
                entries[name] = amax["stem" if i == 0 else f"layer{i}.0.out"]
            assert blk.ranges["in"] == amax["stem" if i == 0 else f"layer{i}.0.out"]
            prev_int8 = nxt
        else:
            assert isinstance(blk, Bottleneck) and blk is getattr(m, name)[0]
            prev_int8 = False
    assert q._entry == entries
    outs = q.trunk(q.stem(x))
    for name, o in zip(rq.STAGES, outs):
        nxt = rq.STAGES.index(name) + 1
        want_i8 = name in sites and nxt < 4 and rq.STAGES[nxt] in sites
        assert o.dtype == (torch.int8 if want_i8 else torch.float32)
    yq = q(x)
    assert yq.shape == y.shape and torch.isfinite(yq).all()
    q.train()
    assert not q.training                                                     # inference only


def test_state_dict_round_trip(tiny):
    m, amax, x, _ = tiny
    q = rq.QuantResNet.from_float(m, ("layer2", "layer3", "layer4"), amax)
    sd = q.state_dict()
    assert sd["layer2.0.conv2_weight_q"].dtype == torch.int8 and sd["layer2.0.conv2_weight_q"].shape == (128, 9 * 128)
    assert sd["layer2.0.down_weight_scale"].dtype == sd["layer2.0.down_bias"].dtype == torch.float32
    assert "layer2.0.conv1.weight" not in sd and "layer1.0.conv1.weight" in sd and "fc.weight" in sd
    q2 = rq.QuantResNet.from_float(tiny_resnet(5), ("layer2", "layer3", "layer4"), amax)
    assert not torch.equal(q2(x), q(x))
    q2.load_state_dict(sd)
    assert torch.equal(q2(x), q(x))


def test_unsupported_models(tiny):
    _, amax, _, _ = tiny
    basic = ResNet((1, 1, 1, 1), 10, dtype=torch.float32, block=BasicBlock)
    grouped = ResNet((1, 1, 1, 1), 10, dtype=torch.float32, groups=2, width_per_group=64)
    for bad in (basic, grouped):
        with pytest.raises(NotImplementedError):
            rq.QuantResNet.from_float(bad, rq.STAGES, amax)
    with pytest.raises(NotImplementedError):
        rq.calibrate(basic, [tiny_images(2)])
    m = tiny_resnet(0)
    with pytest.raises(ValueError):
        rq.QuantResNet.from_float(m, ("layer5",), amax)
    with pytest.raises(ValueError):
        rq.QuantResNet.from_float(m, rq.STAGES, {"stem": 1.0})                # a missing range
    with pytest.raises(ValueError):
        rq.QuantResNet.from_float(m, rq.STAGES, None)


# ----------------------------------------------------------------------------- 7. the error on the CPU
def test_full_model_error_cpu(tiny):
    """d_cpu, the figure tests/test_quant_conv_gpu.py takes its bound from (D_CPU there)."""
    m, amax, x, y = tiny
    yq = rq.QuantResNet.from_float(m, rq.STAGES, amax)(x)
    d = ((yq - y).abs().max() / y.abs().max()).item()
    print(f"d_cpu = {d:.4f}")
    assert d == pytest.approx(0.0277, abs=0.003)       # recorded there; fp32 conv order moves it in the 4th digit


# ----------------------------------------------------------------------------- 5. the workflow
@pytest.fixture(scope="module")
def exported(tmp_path_factory):
    torch.manual_seed(0)
    m = ImageClassificationModel("resnet_tiny", num_classes=4, device="cpu")
    randomize_bn(m.model, torch.Generator().manual_seed(1))
    ds = synthetic_image_dataset(16, 4, image_size=32, seed=0)
    d = tmp_path_factory.mktemp("img")
    saved, cfg = str(d / "fp"), str(d / "q.yaml")
    m.export(saved)
    iq.export_quantization_config(m, cfg, ds, 8, accuracy_criterion_relative=1.0, calibration_sampling_size=8)
    return m, ds, saved, cfg


def test_float_export_unchanged(exported, tmp_path):
    from safetensors.torch import save_file
    m, _, saved, _ = exported
    # what the export wrote before int8 models existed: the state dict and these four keys
    ref_path = str(tmp_path / "ref.safetensors")
    save_file({k: v.detach().contiguous().cpu() for k, v in m.model.state_dict().items()}, ref_path)
    with open(ref_path, "rb") as a, open(os.path.join(saved, "model.safetensors"), "rb") as b:
        assert a.read() == b.read()
    with open(os.path.join(saved, "model_config.json")) as f:
        assert f.read() == json.dumps({"use_case": "image_classification", "model_name": "resnet_tiny",
                                       "num_classes": 4, "classes": None})
    assert sorted(os.listdir(saved)) == ["model.safetensors", "model_config.json"]
    assert load_model(saved, device="cpu").quantization is None


def test_config_export(exported, tmp_path):
    import yaml
    m, ds, _, cfg = exported
    with open(cfg) as f:
        c = yaml.safe_load(f)
    assert c["quantization"] == {"approach": "post_training_static_quant", "calibration": {"sampling_size": 8}}
    loader = {"batch_size": 8, "dataset": {"image_classification": {"num_examples": 16, "image_size": 32}}}
    assert c["evaluation"]["accuracy"]["dataloader"] == c["evaluation"]["performance"]["dataloader"] == loader
    assert c["model"] == {"name": "resnet_tiny", "framework": "cloudtik_amd"}
    assert c["tuning"]["accuracy_criterion"] == {"relative": 1.0}
    with pytest.raises(FileExistsError):
        iq.export_quantization_config(m, cfg, ds, 8)
    iq.export_quantization_config(m, cfg, ds, 8, overwrite=True, accuracy_criterion_relative=1.0,
                                  calibration_sampling_size=8)
    new = str(tmp_path / "sub" / "n.yaml")
    text = TextClassificationDataset(["a b", "c d"], [0, 1], HashTokenizer(max_length=8))
    for bad in (text, [1, 2, 3], None):
        with pytest.raises(NotImplementedError):
            iq.export_quantization_config(m, new, bad, 8)
    with pytest.raises(ValueError, match="static-only"):
        iq.export_quantization_config(m, new, ds, 8, approach="post_training_dynamic_quant")
    for kw in (dict(batch_size=0), dict(batch_size=True), dict(accuracy_criterion_relative=2.0),
               dict(accuracy_criterion_relative=1), dict(exit_policy_timeout=-1), dict(exit_policy_max_trials=0),
               dict(tuning_random_seed=-1), dict(tuning_workspace=3), dict(approach="qat"),
               dict(calibration_sampling_size=0)):
        args = dict(batch_size=8)
        args.update(kw)
        with pytest.raises(ValueError):
            iq.export_quantization_config(m, new, ds, **args)
    assert not os.path.exists(new)


def test_text_config_unchanged():
    """The generalised dataloader block: a text config is, byte for byte, what it was."""
    import yaml
    from cloudtik_amd.modeling.transfer_learning.quantization import build_config
    text = TextClassificationDataset(["a b", "c d"], [0, 1], HashTokenizer(max_length=8))
    got = yaml.safe_dump(build_config("bert-tiny", text, 4, 0.01, 0, 50, 9527, ""), sort_keys=False)
    loader = lambda: {"batch_size": 4, "dataset": {"text_classification": {"num_examples": 2, "max_length": 8}}}
    was = {"version": 1.0, "model": {"name": "bert-tiny", "framework": "cloudtik_amd"},
           "quantization": {"approach": "post_training_dynamic_quant"},
           "evaluation": {"accuracy": {"metric": {"topk": 1}, "dataloader": loader()},
                          "performance": {"configs": {"num_of_instance": 1}, "dataloader": loader()}},
           "tuning": {"accuracy_criterion": {"relative": 0.01}, "exit_policy": {"timeout": 0, "max_trials": 50},
                      "random_seed": 9527}}
    assert got == yaml.safe_dump(was, sort_keys=False)
    assert "&id" not in got                                 # two separate blocks, no YAML anchors


def test_quantize_load_predict_cpu(exported, tmp_path, capsys):
    from safetensors.torch import load_file
    m, ds, saved, cfg = exported
    out = str(tmp_path / "int8")
    path = iq.quantize(m, saved, out, cfg, ds)
    assert path == os.path.join(out, "model.safetensors") and os.path.isfile(path)
    sd = load_file(path)
    for name in rq.STAGES:
        for conv in ("conv1", "conv2", "conv3", "down"):
            assert sd[f"{name}.0.{conv}_weight_q"].dtype == torch.int8
            assert sd[f"{name}.0.{conv}_weight_scale"].dtype == sd[f"{name}.0.{conv}_bias"].dtype == torch.float32
        assert f"{name}.0.conv1.weight" not in sd and f"{name}.0.bn1.weight" not in sd
    fp = load_file(os.path.join(saved, "model.safetensors"))
    for k in ("conv1.weight", "bn1.running_var", "fc.weight", "fc.bias"):
        assert torch.equal(sd[k], fp[k])                    # the stem and the head are unchanged
    with open(os.path.join(out, "model_config.json")) as f:
        block = json.load(f)["quantization"]
    assert block["approach"] == "post_training_static_quant" and block["trial"] == 1
    assert block["sites"] == list(rq.STAGES) and len(block["act_amax"]) == 17
    assert block["calibration"] == {"sampling_size": 8, "num_examples": 8}
    assert block["accuracy"]["fp32"] == pytest.approx(m.evaluate(ds)["accuracy"])
    assert [t["sites"] for t in block["trials"]] == [list(rq.STAGES)]

    q = load_model(out, device="cpu")
    assert isinstance(q, ImageClassificationModel) and isinstance(q.model, rq.QuantResNet)
    assert q.quantization == block and q.model.act_amax == block["act_amax"]
    assert q.evaluate(ds)["accuracy"] == pytest.approx(block["accuracy"]["int8"])
    x = torch.stack([ds[i][0] for i in range(4)])
    p_q, p_f = q.predict(x), m.predict(x)
    assert p_q.shape == p_f.shape == (4, 4) and torch.isfinite(p_q).all()
    with pytest.raises(RuntimeError):
        q.train(ds)

    acc = iq.benchmark(m, out, cfg, mode="accuracy", model_type="int8", dataset=ds)
    assert acc == {"accuracy": pytest.approx(block["accuracy"]["int8"])}
    res = iq.benchmark(m, saved, cfg, model_type="fp32", image_size=32, warmup=1, iters=1)
    assert set(res) == {"latency_ms", "throughput", "batch_size", "image_size", "warmup", "iters"}
    assert res["batch_size"] == 8 and res["latency_ms"] > 0
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["model_type"] == "fp32" and line["model_name"] == "resnet_tiny"
    for kw in (dict(mode="speed"), dict(model_type="int4"), dict(model_type="fp32"),        # it is an int8 model
               dict(mode="accuracy", model_type="int8")):                                   # no dataset
        with pytest.raises(ValueError):
            iq.benchmark(m, out, cfg, **kw)
    with pytest.raises(NotADirectoryError):
        iq.benchmark(m, str(tmp_path / "missing"))
    with pytest.raises(FileNotFoundError):
        iq.benchmark(m, out, str(tmp_path / "no.yaml"))
    with pytest.raises(ValueError):
        iq.quantize(m, out, str(tmp_path / "again"), cfg, ds)                # already quantized


def test_quantize_errors(exported, tmp_path):
    m, ds, saved, cfg = exported
    with pytest.raises(NotADirectoryError):
        iq.quantize(m, str(tmp_path / "missing"), str(tmp_path / "o"), cfg, ds)
    empty = tmp_path / "empty"
    empty.mkdir()
    with pytest.raises(FileNotFoundError):
        iq.quantize(m, str(empty), str(tmp_path / "o"), cfg, ds)
    with pytest.raises(FileNotFoundError):
        iq.quantize(m, saved, str(tmp_path / "o"), str(tmp_path / "no.yaml"), ds)
    with pytest.raises(FileExistsError):
        iq.quantize(m, saved, saved, cfg, ds)               # output_dir already holds a model
    with pytest.raises(ValueError):
        iq.quantize(m, saved, str(tmp_path / "o"), cfg, None)
    with pytest.raises(NotImplementedError):
        iq.quantize(m, saved, str(tmp_path / "o"), cfg, [1, 2])
    dyn = str(tmp_path / "dyn.yaml")
    with open(cfg) as f, open(dyn, "w") as g:
        g.write(f.read().replace("post_training_static_quant", "post_training_dynamic_quant"))
    with pytest.raises(ValueError, match="static-only"):
        iq.quantize(m, saved, str(tmp_path / "o"), dyn, ds)
    other = str(tmp_path / "other.yaml")
    with open(cfg) as f, open(other, "w") as g:
        g.write(f.read().replace("post_training_static_quant", "quant_aware_training"))
    with pytest.raises(ValueError):
        iq.quantize(m, saved, str(tmp_path / "o"), other, ds)
    assert not (tmp_path / "o").exists()


def test_trial_ladder(exported, tmp_path, monkeypatch):
    m, ds, saved, _ = exported
    strict = str(tmp_path / "strict.yaml")
    iq.export_quantization_config(m, strict, ds, 8, accuracy_criterion_relative=0.0, calibration_sampling_size=8)
    calls = []

    def fails_with_layer1(wrapper, dataset, batch_size):
        sites = wrapper.model.sites if wrapper.quantization else None
        calls.append(sites)
        return 0.5 if sites and "layer1" in sites else 1.0

    monkeypatch.setattr(iq, "_trial_accuracy", fails_with_layer1)
    out = str(tmp_path / "t2")
    assert iq.quantize(m, saved, out, strict, ds)
    assert calls == [None, list(rq.TRIALS[0]), list(rq.TRIALS[1])]
    with open(os.path.join(out, "model_config.json")) as f:
        block = json.load(f)["quantization"]
    assert block["trial"] == 2 and block["sites"] == ["layer2", "layer3", "layer4"]
    assert [t["relative_loss"] for t in block["trials"]] == [0.5, 0.0]
    q = load_model(out, device="cpu")
    assert isinstance(q.model.layer1[0], Bottleneck) and isinstance(q.model.layer2[0], rq.QuantBottleneck)
    assert q.predict(torch.stack([ds[0][0]])).shape == (1, 4)

    # criterion 0.0 and an int8 accuracy below the float one in every trial: None, nothing written
    calls.clear()
    monkeypatch.setattr(iq, "_trial_accuracy", lambda w, d, b: calls.append(1) or (0.5 if w.quantization else 1.0))
    none = str(tmp_path / "none")
    assert iq.quantize(m, saved, none, strict, ds) is None
    assert len(calls) == 1 + len(rq.TRIALS) and not os.path.exists(none)

    # the exit policy's trial count ends the ladder early
    one = str(tmp_path / "one.yaml")
    iq.export_quantization_config(m, one, ds, 8, accuracy_criterion_relative=0.0, exit_policy_max_trials=1)
    calls.clear()
    monkeypatch.setattr(iq, "_trial_accuracy", fails_with_layer1)
    assert iq.quantize(m, saved, str(tmp_path / "t1"), one, ds) is None
    assert calls == [None, list(rq.TRIALS[0])]


# ----------------------------------------------------------------------------- 6. the hooks
def test_hooks_point_at_the_functions():
    m = ImageClassificationModel.__new__(ImageClassificationModel)
    for call in (lambda: m.quantize("a", "b", "c"), lambda: m.export_quantization_config("c", None, 8),
                 lambda: m.export_neural_compressor_config("c", None, 8), lambda: m.benchmark("a"),
                 lambda: m.benchmark_neural_compressor("a", "c")):
        with pytest.raises(NotImplementedError, match="image classification") as e:
            call()
        msg = str(e.value)
        assert "image_quantization" in msg
        assert all(f in msg for f in ("export_quantization_config(", ".quantize(", ".benchmark("))
        assert "no int8 convolution" not in msg
    for f in ("export_quantization_config", "quantize", "benchmark"):
        assert callable(getattr(iq, f))
