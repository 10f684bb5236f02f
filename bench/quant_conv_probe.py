"""Time the static int8 convolution (csrc/quant_conv.hip) against the bf16 eval path, in one
process:

    python bench/quant_conv_probe.py layers [batch] [iters] [rounds]
        every convolution shape of a ResNet-50 bottleneck trunk at ``batch`` (default 64): the int8
        kernel with ReLU and int8 output against the bf16 implicit-GEMM convolution followed by the
        eval BatchNorm + ReLU pass it replaces.  conv3 shapes carry the residual in both.
    python bench/quant_conv_probe.py model [iters] [rounds] [batch ...]
        ResNet-50 forward (eval), bf16 against int8 with all four stages quantized, at each
        ``batch`` (default 64 256) x 3 x 224 x 224.  Random weights, random BatchNorm statistics,
        ranges calibrated on one random batch: a timing, not an accuracy figure.  Eager calls, host
        launch cost included.

The variants of a group alternate ``rounds`` times; each figure is the fastest round (all rounds
are printed too).  A ``layers`` timing replays a captured graph of ``iters`` calls (HIP events around three
replays, warm-up excluded), so it is device time without the host's launch cost.  One JSON line per
group."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# (stage, name, Ci, Co, R, stride, input H = W, blocks that run it)
SHAPES = [
    ("layer1", "conv1.first", 64, 64, 1, 1, 56, 1), ("layer1", "conv1", 256, 64, 1, 1, 56, 2),
    ("layer1", "conv2", 64, 64, 3, 1, 56, 3), ("layer1", "conv3", 64, 256, 1, 1, 56, 3),
    ("layer1", "down", 64, 256, 1, 1, 56, 1),
    ("layer2", "conv1.first", 256, 128, 1, 1, 56, 1), ("layer2", "conv2.first", 128, 128, 3, 2, 56, 1),
    ("layer2", "down", 256, 512, 1, 2, 56, 1), ("layer2", "conv1", 512, 128, 1, 1, 28, 3),
    ("layer2", "conv2", 128, 128, 3, 1, 28, 3), ("layer2", "conv3", 128, 512, 1, 1, 28, 4),
    ("layer3", "conv1.first", 512, 256, 1, 1, 28, 1), ("layer3", "conv2.first", 256, 256, 3, 2, 28, 1),
    ("layer3", "down", 512, 1024, 1, 2, 28, 1), ("layer3", "conv1", 1024, 256, 1, 1, 14, 5),
    ("layer3", "conv2", 256, 256, 3, 1, 14, 5), ("layer3", "conv3", 256, 1024, 1, 1, 14, 6),
    ("layer4", "conv1.first", 1024, 512, 1, 1, 14, 1), ("layer4", "conv2.first", 512, 512, 3, 2, 14, 1),
    ("layer4", "down", 1024, 2048, 1, 2, 14, 1), ("layer4", "conv1", 2048, 512, 1, 1, 7, 2),
    ("layer4", "conv2", 512, 512, 3, 1, 7, 2), ("layer4", "conv3", 512, 2048, 1, 1, 7, 3),
]


def _time(fn, iters, warmup=5):
    """Microseconds per call: ``iters`` calls captured into one graph and replayed, so the figure
    is the kernels back to back without the host's launch cost (which at batch 64 exceeds most of
    these kernels); the first replay is warm-up."""
    for _ in range(warmup):
        fn()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(iters):
            fn()
    graph.replay()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(3):
        graph.replay()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) * 1e3 / (3 * iters)


def _time_eager(fn, iters, warmup=3):
    """Microseconds per eager call, host launch cost included: what a user's loop sees."""
    for _ in range(warmup):
        fn()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) * 1e3 / iters


def _group(head, variants, iters, rounds, time=_time):
    runs = {k: [] for k in variants}
    for _ in range(rounds):                                  # a, b, c, a, b, c: the variants alternate
        for k, fn in variants.items():
            runs[k].append(round(time(fn, iters), 1))
    best = {k: min(v) for k, v in runs.items()}
    print(json.dumps(dict(head, us=best, rounds_us=runs, iters=iters)), flush=True)
    return best


def layers(argv):
    batch = int(argv[0]) if argv else 64
    iters = int(argv[1]) if len(argv) > 1 else 30
    rounds = int(argv[2]) if len(argv) > 2 else 3
    from cloudtik_amd import ops
    from cloudtik_amd.models.resnet import BatchNormAct, _conv
    from cloudtik_amd.ops import conv as igemm
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(0)
    cl = lambda t: t.contiguous(memory_format=torch.channels_last)
    total = {}
    for stage, name, ci, co, R, stride, H, count in SHAPES:
        Ho = (H + 2 * (R // 2) - R) // stride + 1
        x = cl(torch.randint(-127, 128, (batch, ci, H, H), generator=g, dtype=torch.int8)).to(dev)
        w_q, w_s = ops.quantize_weight(torch.randn(co, R * R * ci, generator=g) * (R * R * ci) ** -0.5)
        w_q, w_s, bias = w_q.to(dev), w_s.to(dev), (torch.randn(co, generator=g) * 0.3).to(dev)
        is3 = name.startswith("conv3")
        res = cl(torch.randint(-127, 128, (batch, co, Ho, Ho), generator=g, dtype=torch.int8)).to(dev) if is3 else None
        relu = name != "down"
        i8 = lambda: ops.conv2d_i8_static(x, 2.0, w_q, w_s, bias, stride, R // 2, relu, res, 3.0 if is3 else None, 2.0)
        conv = _conv(ci, co, R, stride, device=dev, dtype=torch.bfloat16).to(memory_format=torch.channels_last)
        bn = BatchNormAct(co, relu=relu, device=dev, dtype=torch.bfloat16).eval()
        xb = cl(torch.randn(batch, ci, H, H, generator=g).to(torch.bfloat16)).to(dev)
        rb = cl(torch.randn(batch, co, Ho, Ho, generator=g).to(torch.bfloat16)).to(dev) if is3 else None
        variants = {"int8": i8}
        with torch.no_grad():
            variants["bf16_conv+bn"] = lambda: bn(igemm.conv2d(xb, conv), residual=rb)
            variants["bf16_conv"] = lambda: igemm.conv2d(xb, conv)
            best = _group({"group": "layer", "stage": stage, "conv": name, "batch": batch, "Ci": ci, "Co": co, "R": R,
                           "stride": stride, "H": H, "M": batch * Ho * Ho, "K": R * R * ci, "blocks": count,
                           "gflop": round(2e-9 * batch * Ho * Ho * co * R * R * ci, 2)}, variants, iters, rounds)
        for k, v in best.items():
            total[k] = total.get(k, 0.0) + v * count
    print(json.dumps({"group": "trunk_sum", "batch": batch, "us": {k: round(v, 1) for k, v in total.items()}}),
          flush=True)


def model(argv):
    iters = int(argv[0]) if argv else 10
    rounds = int(argv[1]) if len(argv) > 1 else 3
    batches = [int(b) for b in argv[2:]] or [64, 256]
    from cloudtik_amd import ops
    from cloudtik_amd.models import resnet_quant as rq
    from cloudtik_amd.models.resnet import resnet50
    ops.require_native()
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    m = resnet50(device=dev).eval()
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for mod in m.modules():                              # random statistics: bn3's zero init folds conv3 to 0
            if hasattr(mod, "running_var"):
                c = mod.weight.shape[0]
                mod.weight.copy_(torch.rand(c, generator=g) + 0.5)
                mod.bias.copy_(torch.randn(c, generator=g) * 0.2)
                mod.running_mean.copy_(torch.randn(c, generator=g) * 0.2)
                mod.running_var.copy_(torch.rand(c, generator=g) * 1.5 + 0.5)
    img = lambda n: torch.randn(n, 3, 224, 224, generator=g).to(dev, torch.bfloat16).contiguous(
        memory_format=torch.channels_last)
    amax = rq.calibrate(m, [img(16)])
    q = rq.QuantResNet.from_float(m, rq.STAGES, amax)
    try:
        clock = torch.cuda.clock_rate()
    except Exception:  # noqa: BLE001 - needs the SMI Python package; the timing does not
        clock = None
    print(json.dumps({"group": "device", "name": torch.cuda.get_device_name(0), "clock_mhz": clock}), flush=True)
    with torch.no_grad():
        for b in batches:
            x = img(b)
            yf, yq = m(x).float(), q(x).float()
            d = ((yq - yf).abs().max() / yf.abs().max()).item()
            best = _group({"group": "resnet50_forward", "batch": b, "image": 224,
                           "max_logit_diff_over_max_logit": round(d, 4)},
                          {"bf16": lambda: m(x), "int8": lambda: q(x)}, iters, rounds, time=_time_eager)
            print(json.dumps({"group": "resnet50_forward_img_s", "batch": b,
                              "img_s": {k: round(b * 1e6 / v, 1) for k, v in best.items()}}), flush=True)


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "layers"
    {"layers": layers, "model": model}[what](sys.argv[2:])
