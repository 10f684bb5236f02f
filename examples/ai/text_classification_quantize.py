#!/usr/bin/env python3
"""Post-training int8 quantization of a text classifier, end to end: fine-tune on a synthetic
keyword-sentiment task, export, write the quantization config, quantize (int8 weights, per-call
activation quantization on the i8 matrix cores), reload, and benchmark the float export against
the int8 one in the same process.

    python examples/ai/text_classification_quantize.py                       # bert-tiny, trains
    python examples/ai/text_classification_quantize.py --model bert-large-uncased --epochs 0 \
        --batch 64 --seq-len 128                                             # latency only
    python examples/ai/text_classification_quantize.py --approach static     # calibrated ranges

``--approach static`` calibrates one activation range per site and layer on the evaluation
dataset (``post_training_static_quant``): the int8 activations then come out of the LayerNorm and
GEMM epilogues instead of per-token quantize passes.  It also quantizes the same export with the
dynamic approach and times float, dynamic int8 and static int8 in turn, in this one process.

With ``--epochs 0`` the model keeps its random initialisation and there is no accuracy to
preserve: the dynamic approach quantizes without an evaluation, the static one still needs the
dataset to calibrate on and accepts any accuracy; the latency comparison is unaffected.
Prints one JSON line per benchmark and a final summary line.
"""
import argparse
import json
import os
import sys
import tempfile

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def keyword_dataset(tokenizer, n=800, seed=0):
    from cloudtik_amd.modeling.transfer_learning import TextClassificationDataset
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
    cut = n * 4 // 5
    return (TextClassificationDataset(texts[:cut], labels[:cut], tokenizer),
            TextClassificationDataset(texts[cut:], labels[cut:], tokenizer))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--model", default="bert-tiny", choices=["bert-tiny", "bert-base-uncased", "bert-large-uncased"])
    ap.add_argument("--epochs", type=int, default=4)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--batch", type=int, default=64, help="benchmark batch size")
    ap.add_argument("--seq-len", type=int, default=128)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--approach", default="dynamic", choices=["dynamic", "static"])
    ap.add_argument("--workdir", default=None)
    ap.add_argument("--device", default=None)
    a = ap.parse_args()

    from cloudtik_amd.modeling.transfer_learning import HashTokenizer, get_model, load_model
    work = a.workdir or tempfile.mkdtemp(prefix="ct_quant_")
    torch.manual_seed(0)
    m = get_model(a.model, use_case="text_classification", num_classes=2, device=a.device)
    tok = HashTokenizer(vocab_size=m.cfg.vocab_size, max_length=16)
    train, ev = keyword_dataset(tok)
    if a.epochs > 0:
        m.train(train, epochs=a.epochs, batch_size=32, lr=a.lr, log_every=0)
        print(json.dumps({"float_accuracy": m.evaluate(ev)["accuracy"]}), flush=True)

    saved, out, cfg = os.path.join(work, "fp32"), os.path.join(work, "int8"), os.path.join(work, "quant.yaml")
    m.export(saved)
    static = a.approach == "static"
    m.export_quantization_config(cfg, ev, batch_size=a.batch, overwrite=True,
                                 approach=f"post_training_{a.approach}_quant",
                                 accuracy_criterion_relative=1.0 if static and a.epochs == 0 else 0.01)
    if m.quantize(saved, out, cfg, dataset=ev if a.epochs > 0 or static else None) is None:
        print("no trial met the accuracy criterion; nothing written")
        return 1
    variants = {"fp32": (saved, "fp32"), "int8": (out, "int8")}
    if static:                                 # the dynamic model of the same export, to time beside it
        dyn, dyn_cfg = os.path.join(work, "int8_dynamic"), os.path.join(work, "quant_dynamic.yaml")
        m.export_quantization_config(dyn_cfg, ev, batch_size=a.batch, overwrite=True)
        if m.quantize(saved, dyn, dyn_cfg, dataset=ev if a.epochs > 0 else None) is not None:
            variants = {"fp32": (saved, "fp32"), "int8_dynamic": (dyn, "int8"), "int8": (out, "int8")}
    q = load_model(out, device=a.device)
    with open(os.path.join(out, "model_config.json")) as f:
        block = json.load(f)["quantization"]
    probs = q.predict(ev.ids[:4], ev.mask[:4])
    print(json.dumps({"approach": block["approach"], "int8_sites": block["sites"][0], "trial": block["trial"],
                      "accuracy": block["accuracy"],
                      "predictions": probs.argmax(-1).tolist(), "labels": ev.y[:4].tolist()}), flush=True)

    kw = dict(batch_size=a.batch, seq_len=a.seq_len, warmup=a.warmup, iters=a.iters)
    res = {}
    for rnd in range(2):                       # float, int8, float, int8: the variants repeat on the same box
        for name, (path, model_type) in variants.items():
            res.setdefault(name, []).append(m.benchmark(path, cfg, model_type=model_type, **kw)["latency_ms"])
    fp, i8 = min(res["fp32"]), min(res["int8"])
    summary = {"model": a.model, "approach": a.approach, "batch_size": a.batch, "seq_len": a.seq_len,
               "float_latency_ms": res["fp32"], "int8_latency_ms": res["int8"], "int8_over_float": round(i8 / fp, 3)}
    if "int8_dynamic" in res:
        summary.update(int8_dynamic_latency_ms=res["int8_dynamic"],
                       static_over_dynamic=round(i8 / min(res["int8_dynamic"]), 3))
    print(json.dumps(summary), flush=True)
    if a.epochs > 0:
        m.benchmark(out, cfg, mode="accuracy", model_type="int8", dataset=ev)      # prints its JSON line
    return 0


if __name__ == "__main__":
    sys.exit(main())
