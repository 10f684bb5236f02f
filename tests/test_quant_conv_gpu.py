"""The int8 convolution kernel (csrc/quant_conv.hip) and the int8 ResNet on the GPU.  Every
comparison of int8 / bf16 tensors is ``torch.equal`` against the CPU reference
(``ops.reference.conv_i8_static``): the accumulation is exact and the epilogue's arithmetic
is fixed, so nothing is left to a tolerance."""
import copy
import json
import os

import pytest
import torch

from cloudtik_amd import ops
from cloudtik_amd.models import resnet_quant as rq
from cloudtik_amd.models.resnet import Bottleneck, ResNet
from cloudtik_amd.ops import reference as ref

from quant_conv_util import conv_case, one_hot_rows, randomize_bn, shifted, tiny_images, tiny_resnet

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16

# d_cpu = max|logits_int8 - logits_float| / max|logits_float| of tiny_resnet(seed 0) on
# tiny_images(8, 32, seed 2), all four stages in int8, fp32 on the CPU, as
# tests/test_quant_conv_cpu.py::test_full_model_error_cpu measures it: 0.0277
D_CPU = 0.0277


def _dev(t, cuda):
    return None if t is None else t.to(cuda)


# ----------------------------------------------------------------------------- 1. the op
# (N, H, W, Ci, Co, R, stride): see the issue for the hazard each shape carries
CASES = [
    (2, 7, 7, 64, 64, 3, 1),        # M = 98: M tail inside one tile; Co = 64: N tail; K = 576: K tail, straddling taps
    (1, 14, 14, 128, 128, 3, 2),    # strided 3x3
    (2, 7, 7, 256, 64, 1, 1),       # 1x1
    (2, 14, 14, 256, 512, 1, 2),    # strided 1x1 (the downsample branch), four N tiles
    (3, 10, 10, 64, 128, 3, 1),     # M = 300: three tiles, a tail of 44, tiles that straddle images
    (1, 9, 5, 64, 64, 3, 1),        # H != W
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("out_i8", [False, True])
def test_conv_bit_equal(cuda, case, relu, with_res, out_i8):
    N, H, W, ci, co, R, stride = case
    x, w_q, w_s, bias = conv_case(N, H, W, ci, co, R, seed=sum(case) * 131 + R)
    a_amax, res_amax = 2.0, 3.0
    out_amax = 1.5 if out_i8 else None                     # results reach about 3: some saturate
    Ho, Wo = (H + 2 * (R // 2) - R) // stride + 1, (W + 2 * (R // 2) - R) // stride + 1
    res = None
    if with_res:
        g = torch.Generator().manual_seed(7)
        res = torch.randint(-127, 128, (N, co, Ho, Wo), generator=g, dtype=torch.int8).contiguous(
            memory_format=torch.channels_last)
    want = ref.conv_i8_static(x, a_amax, w_q, w_s, bias, stride, R // 2, relu, res, res_amax if with_res else None,
                              out_amax, dtype=BF16)
    got = ops.conv2d_i8_static(_dev(x, cuda), a_amax, _dev(w_q, cuda), _dev(w_s, cuda), _dev(bias, cuda), stride,
                               R // 2, relu, _dev(res, cuda), res_amax if with_res else None, out_amax)
    assert got.is_cuda and got.shape == (N, co, Ho, Wo) and got.dtype == (torch.int8 if out_i8 else BF16)
    assert got.is_contiguous(memory_format=torch.channels_last)
    bad = (got.cpu() != want).sum().item()
    print(f"elements differing from the reference: {bad} of {want.numel()}")
    assert torch.equal(got.cpu(), want)
    if out_i8:
        assert (want.abs() == 127).any() and (want.abs() < 127).any()


# ----------------------------------------------------------------------------- 2. one-hot taps
@pytest.mark.parametrize("stride", [1, 2])
def test_one_hot_taps(cuda, stride):
    g = torch.Generator().manual_seed(3)
    x = torch.randint(-127, 128, (2, 64, 7, 5), generator=g, dtype=torch.int8).contiguous(
        memory_format=torch.channels_last)
    xg = x.to(cuda)
    one, zero = torch.ones(64, device=cuda), torch.zeros(64, device=cuda)
    for r in range(3):
        for s in range(3):
            w = one_hot_rows(64, 3, r, s).to(cuda)
            want = shifted(x, r, s, 3, stride)
            y = ops.conv2d_i8_static(xg, 127.0, w, one, zero, stride, 1, False)          # scale 1: y == acc
            assert torch.equal(y.cpu().float(), want.float()), (r, s)
            q = ops.conv2d_i8_static(xg, 127.0, w, one, zero, stride, 1, False, out_amax=127.0)
            assert torch.equal(q.cpu(), want), (r, s)


# ----------------------------------------------------------------------------- 3. saturation
def test_saturation_and_zero_scales(cuda):
    x, w_q, w_s, bias = conv_case(2, 7, 7, 64, 64, 3, seed=11)
    args = lambda *t: [_dev(v, cuda) for v in t]
    # a range far below the results: both clamps
    want = ref.conv_i8_static(x, 2.0, w_q, w_s, bias, 1, 1, False, out_amax=0.25, dtype=BF16)
    assert (want == 127).any() and (want == -127).any()
    xg, wg, sg, bg = args(x, w_q, w_s, bias)
    assert torch.equal(ops.conv2d_i8_static(xg, 2.0, wg, sg, bg, 1, 1, False, out_amax=0.25).cpu(), want)
    # a_amax = 0: the activation scale is 0, so without a bias everything is 0
    zero = torch.zeros_like(bg)
    assert not ops.conv2d_i8_static(xg, 0.0, wg, sg, zero, 1, 1, False).any()
    assert not ops.conv2d_i8_static(xg, 0.0, wg, sg, zero, 1, 1, False, out_amax=1.0).any()
    # an all-zero weight row quantizes to scale 0: that channel is its bias
    w = torch.randn(64, 576, generator=torch.Generator().manual_seed(5)) / 24
    w[5] = 0
    w_q, w_s = ops.quantize_weight(w)
    assert w_s[5] == 0 and not w_q[5].any()
    y = ops.conv2d_i8_static(xg, 2.0, w_q.to(cuda), w_s.to(cuda), bg, 1, 1, False)
    assert torch.equal(y.cpu(), ref.conv_i8_static(x, 2.0, w_q, w_s, bias, 1, 1, False, dtype=BF16))
    assert torch.equal(y[:, 5].cpu(), bias[5].to(BF16).expand(2, 7, 7))


# ----------------------------------------------------------------------------- 4. rejections
def test_rejections_leave_output_untouched(cuda):
    C = ops.require_native()
    cl = lambda t: t.contiguous(memory_format=torch.channels_last)
    i8 = lambda *s: torch.ones(*s, device=cuda, dtype=torch.int8)
    f32 = lambda n: torch.ones(n, device=cuda)

    def rejected(x, w, out_shape, a_scale=1.0, w_scale=None, bias=None, stride=1, padding=None, res=None,
                 res_scale=0.0, out_inv=0.0, out_dtype=BF16, out_cl=True):
        co = w.shape[0]
        out = torch.full(out_shape, 77, device=cuda, dtype=out_dtype)
        out = cl(out) if out_cl else out
        before = out.clone()
        if padding is None:
            padding = 1 if w.shape[1] == 9 * x.shape[1] else 0
        with pytest.raises((RuntimeError, TypeError, ValueError)):
            C.conv2d_i8_static(x, a_scale, w, f32(co) if w_scale is None else w_scale,
                               f32(co) if bias is None else bias, stride, padding, False, res, res_scale, out, out_inv)
        torch.cuda.synchronize()
        assert torch.equal(out, before)

    x64 = cl(i8(1, 64, 6, 6))
    ok_out = (1, 64, 6, 6)
    rejected(cl(i8(1, 32, 6, 6)), i8(64, 32), ok_out)                         # Ci % 64
    rejected(x64, i8(32, 64), (1, 32, 6, 6))                                  # Co % 64
    rejected(x64, i8(64, 25 * 64), ok_out, padding=2)                         # 5x5
    rejected(x64, i8(64, 32), ok_out)                                         # groups = 2: rows of Ci / 2
    rejected(x64, i8(64, 64), (1, 64, 2, 2), stride=3)                        # stride 3
    rejected(x64, i8(64, 9 * 64), (1, 64, 4, 4), padding=0)                   # padding != R // 2
    rejected(i8(1, 64, 6, 6), i8(64, 64), ok_out)                             # NCHW-contiguous input
    rejected(x64, i8(64, 64), ok_out, out_cl=False)                           # NCHW-contiguous output
    rejected(x64.to(BF16), i8(64, 64), ok_out)                                # dtypes
    rejected(x64, i8(64, 64).to(BF16), ok_out)
    rejected(x64, i8(64, 64), ok_out, w_scale=f32(64).to(BF16))
    rejected(x64, i8(64, 64), ok_out, bias=f32(64).to(BF16))
    rejected(x64, i8(64, 64), ok_out, out_dtype=torch.float32)
    rejected(x64, i8(64, 64), ok_out, res=cl(i8(1, 64, 3, 3)), res_scale=1.0)   # residual shape
    rejected(x64, i8(64, 64), ok_out, res=cl(i8(1, 64, 6, 6)).to(BF16), res_scale=1.0)
    rejected(x64, i8(64, 64), (1, 64, 5, 6))                                  # output shape
    for bad in (float("inf"), float("nan"), -1.0):                            # scales
        rejected(x64, i8(64, 64), ok_out, a_scale=bad)
        rejected(x64, i8(64, 64), ok_out, out_inv=bad)
        rejected(x64, i8(64, 64), ok_out, res=cl(i8(1, 64, 6, 6)), res_scale=bad)
    # the op itself: dilation, groups and ranges are checked before anything is allocated
    w, s = i8(64, 9 * 64), f32(64)
    with pytest.raises(ValueError):
        ops.conv2d_i8_static(x64, 1.0, w, s, s, 1, 1, False, dilation=2)
    with pytest.raises(ValueError):
        ops.conv2d_i8_static(x64, 1.0, w, s, s, 1, 1, False, groups=2)
    with pytest.raises(ValueError):
        ops.conv2d_i8_static(x64, 1.0, w, s, s, (1, 2), 1, False)
    for bad in (float("inf"), float("nan"), -1.0):
        with pytest.raises(ValueError):
            ops.conv2d_i8_static(x64, bad, w, s, s, 1, 1, False)
        with pytest.raises(ValueError):
            ops.conv2d_i8_static(x64, 1.0, w, s, s, 1, 1, False, out_amax=bad)
    with pytest.raises(TypeError):
        ops.conv2d_i8_static(x64, 1.0, w, s, s, 1, 1, False, dtype=torch.float32)
    # and a good call still works afterwards
    assert ops.conv2d_i8_static(x64, 127.0, w, s, s, 1, 1, False).shape == ok_out


# ----------------------------------------------------------------------------- 5. a block
def _block(cin, width, stride, down, seed):
    torch.manual_seed(seed)
    b = Bottleneck(cin, width, stride, downsample=down, dtype=torch.float32)
    return randomize_bn(b, torch.Generator().manual_seed(seed + 1)).to(BF16).eval()


def _x_q(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-127, 128, shape, generator=g, dtype=torch.int8).contiguous(memory_format=torch.channels_last)


RANGES = {"in": 2.0, "bn1": 3.0, "bn2": 2.5, "down_bn": 3.5, "out": 4.0}


@pytest.mark.parametrize("down", [False, True])
@pytest.mark.parametrize("float_out", [False, True])
def test_quant_bottleneck(cuda, down, float_out):
    b = _block(64, 64, 2, True, 21) if down else _block(256, 64, 1, False, 22)
    q = rq.QuantBottleneck.from_float(b, RANGES, float_out)
    assert q.conv3_weight_q.any()                          # bn3 is not the zero-initialised one
    x = _x_q((2, 64 if down else 256, 8, 8), 23)
    want = q(x)
    got = copy.deepcopy(q).to(cuda)(x.to(cuda))
    assert got.dtype == (BF16 if float_out else torch.int8) and got.shape == want.shape == (2, 256, 4 if down else 8,
                                                                                            4 if down else 8)
    assert torch.equal(got.cpu(), want)
    assert want.float().abs().max() > 0


# ----------------------------------------------------------------------------- 6. the trunk
@pytest.fixture(scope="module")
def tiny():
    """(float fp32 CPU model, ranges, images)."""
    m = tiny_resnet(0)
    x = tiny_images()
    return m, rq.calibrate(m, [x]), x


def test_trunk_every_stage(cuda, tiny):
    m, amax, _ = tiny
    q = rq.QuantResNet.from_float(copy.deepcopy(m).to(BF16), rq.STAGES, amax)
    qg = copy.deepcopy(q).to(cuda)
    x = _x_q((2, 64, 8, 8), 31)
    xc, xg = x, x.to(cuda)
    for name in rq.STAGES:
        xc, xg = getattr(q, name)(xc), getattr(qg, name)(xg)
        assert xc.dtype == (BF16 if name == "layer4" else torch.int8)
        assert xc.float().abs().max() > 0
        assert torch.equal(xg.cpu(), xc), name
    assert xc.shape == (2, 2048, 1, 1)


# ----------------------------------------------------------------------------- 7. the model
def test_full_model_against_bf16(cuda, tiny):
    m, amax, x = tiny
    fg = ResNet((1, 1, 1, 1), 10, device=cuda, dtype=BF16)
    fg.load_state_dict({k: v.to(BF16) if v.is_floating_point() and "running" not in k else v
                        for k, v in m.state_dict().items()})
    fg.eval()
    xg = x.to(cuda, BF16).contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        y_f = fg(xg).float()
        y_q = rq.QuantResNet.from_float(fg, rq.STAGES, amax)(xg).float()
    d = ((y_q - y_f).abs().max() / y_f.abs().max()).item()
    print(f"d_gpu = {d:.4f} (d_cpu = {D_CPU}, bound {2 * D_CPU:.4f})")
    assert d <= 2 * D_CPU


# ----------------------------------------------------------------------------- 8. graph replay
def test_bottleneck_graph_replay(cuda):
    q = rq.QuantBottleneck.from_float(_block(64, 64, 2, True, 41), RANGES).to(cuda)
    x = _x_q((2, 64, 8, 8), 42).to(cuda)
    eager = q(x).clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        q(x)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = q(x)
    x.copy_(_x_q((2, 64, 8, 8), 43))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(y, q(x)) and not torch.equal(y, eager)


# ----------------------------------------------------------------------------- 9. the workflow
def test_quantize_load_predict(cuda, tmp_path):
    from cloudtik_amd.modeling.transfer_learning import image_quantization as iq
    from cloudtik_amd.modeling.transfer_learning.datasets import synthetic_image_dataset
    from cloudtik_amd.modeling.transfer_learning.image_classification import ImageClassificationModel
    from cloudtik_amd.modeling.transfer_learning.model_factory import load_model
    torch.manual_seed(0)
    m = ImageClassificationModel("resnet_tiny", num_classes=4, device=cuda)
    randomize_bn(m.model, torch.Generator().manual_seed(1))
    ds = synthetic_image_dataset(64, 4, image_size=32, seed=0)
    saved, out, cfg = str(tmp_path / "fp"), str(tmp_path / "int8"), str(tmp_path / "q.yaml")
    m.export(saved)
    iq.export_quantization_config(m, cfg, ds, 32, accuracy_criterion_relative=1.0, calibration_sampling_size=32)
    path = iq.quantize(m, saved, out, cfg, ds)
    assert path == os.path.join(out, "model.safetensors") and os.path.isfile(path)
    with open(os.path.join(out, "model_config.json")) as f:
        block = json.load(f)["quantization"]
    assert block["trial"] == 1 and block["sites"] == list(rq.STAGES)
    q = load_model(out, device=cuda)
    assert isinstance(q.model, rq.QuantResNet) and q.quantization == block
    assert q.model.layer1[0].conv1_weight_q.is_cuda and q.model.layer1[0].conv1_weight_q.dtype == torch.int8
    x = torch.stack([ds[i][0] for i in range(8)])
    p_q, p_f = q.predict(x), m.predict(x)
    assert p_q.shape == p_f.shape == (8, 4) and torch.isfinite(p_q).all()
    assert torch.allclose(p_q.sum(-1), torch.ones(8, device=p_q.device), atol=1e-5)
    assert q.evaluate(ds)["accuracy"] == pytest.approx(block["accuracy"]["int8"])
