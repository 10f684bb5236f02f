#!/usr/bin/env python3
"""Post-training static int8 quantization of an image classifier, end to end: fine-tune on a
synthetic dataset (class-dependent mean colour + noise), export, write the quantization config,
quantize (BatchNorm folded into int8 convolutions on the i8 matrix cores, int8 activations between
them, ranges calibrated on the dataset), reload, and benchmark the float export against the int8
one in the same process.

    python examples/ai/image_classification_quantize.py                      # resnet_tiny, trains
    python examples/ai/image_classification_quantize.py --model resnet50 --epochs 0 \
        --image-size 224 --batch 64                                          # latency only

The workflow is in ``cloudtik_amd.modeling.transfer_learning.image_quantization`` (functions that
take the model object); the stem, the pooling head and ``fc`` stay in the model's own type.

With ``--epochs 0`` the model keeps its random initialisation -- the BatchNorm statistics are
randomised so that the zero-initialised last BatchNorm of a block does not fold its convolution
to zero -- and there is no accuracy to preserve: any accuracy is accepted and only the latency
comparison means something.  Prints one JSON line per benchmark and a final summary line.
"""
import argparse
import json
import os
import sys
import tempfile

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--model", default="resnet_tiny", choices=["resnet_tiny", "resnet50", "resnet101"])
    ap.add_argument("--classes", type=int, default=4)
    ap.add_argument("--examples", type=int, default=256)
    ap.add_argument("--image-size", type=int, default=64)
    ap.add_argument("--epochs", type=int, default=2)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--batch", type=int, default=64, help="benchmark batch size")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--workdir", default=None)
    ap.add_argument("--device", default=None)
    a = ap.parse_args()

    from cloudtik_amd.modeling.transfer_learning import get_model, image_quantization as iq, load_model
    from cloudtik_amd.modeling.transfer_learning.datasets import synthetic_image_dataset
    work = a.workdir or tempfile.mkdtemp(prefix="ct_quant_img_")
    torch.manual_seed(0)
    m = get_model(a.model, use_case="image_classification", num_classes=a.classes, device=a.device,
                  freeze_backbone=False)
    train = synthetic_image_dataset(a.examples, a.classes, a.image_size, seed=0)
    ev = synthetic_image_dataset(max(a.examples // 4, a.classes), a.classes, a.image_size, seed=1)
    if a.epochs > 0:
        m.train(train, epochs=a.epochs, batch_size=32, lr=a.lr, log_every=0)
        print(json.dumps({"float_accuracy": m.evaluate(ev)["accuracy"], "data": "synthetic"}), flush=True)
    else:
        g = torch.Generator().manual_seed(1)
        with torch.no_grad():
            for mod in m.model.modules():
                if hasattr(mod, "running_var"):
                    c = mod.weight.shape[0]
                    mod.weight.copy_(torch.rand(c, generator=g) + 0.5)
                    mod.running_mean.copy_(torch.randn(c, generator=g) * 0.2)
                    mod.running_var.copy_(torch.rand(c, generator=g) * 1.5 + 0.5)

    saved, out, cfg = os.path.join(work, "fp32"), os.path.join(work, "int8"), os.path.join(work, "quant.yaml")
    m.export(saved)
    iq.export_quantization_config(m, cfg, ev, batch_size=a.batch, overwrite=True,
                                  accuracy_criterion_relative=1.0 if a.epochs == 0 else 0.01,
                                  calibration_sampling_size=min(100, len(ev)))
    if iq.quantize(m, saved, out, cfg, ev) is None:
        print("no trial met the accuracy criterion; nothing written")
        return 1
    q = load_model(out, device=a.device)
    block = q.quantization
    x = torch.stack([ev[i][0] for i in range(4)])
    print(json.dumps({"approach": block["approach"], "int8_sites": block["sites"], "trial": block["trial"],
                      "accuracy": block["accuracy"], "data": "synthetic",
                      "weights": "fine-tuned" if a.epochs > 0 else "random initialisation",
                      "predictions": q.predict(x).argmax(-1).tolist(),
                      "labels": [int(ev[i][1]) for i in range(4)]}), flush=True)

    kw = dict(batch_size=a.batch, image_size=a.image_size, warmup=a.warmup, iters=a.iters)
    res = {}
    for rnd in range(2):                       # float, int8, float, int8: the variants repeat on the same box
        for name, path in (("fp32", saved), ("int8", out)):
            res.setdefault(name, []).append(iq.benchmark(m, path, cfg, model_type=name, **kw)["latency_ms"])
    fp, i8 = min(res["fp32"]), min(res["int8"])
    print(json.dumps({"model": a.model, "batch_size": a.batch, "image_size": a.image_size,
                      "float_latency_ms": res["fp32"], "int8_latency_ms": res["int8"],
                      "int8_over_float": round(i8 / fp, 3)}), flush=True)
    if a.epochs > 0:
        iq.benchmark(m, out, cfg, mode="accuracy", model_type="int8", dataset=ev)       # prints its JSON line
    return 0


if __name__ == "__main__":
    sys.exit(main())
