"""T5-base training step on the MFMA attention kernels against the routing they replace.

T5-base, random init, dropout 0.1, forward + backward of ``model(input_ids, labels, mask)`` at
16 x 128 -> 128 tokens and 8 x 512 -> 128 tokens.  The two routes are the same model object:
``CLOUDTIK_AMD_T5_TRAIN_ATTN`` is read per call, so ``1`` (the relative-bias forward / backward
kernels and dropout inside ``ops.attention``) and ``0`` (the parent commit's path:
``F.scaled_dot_product_attention`` with the materialised [1, H, S, S] bias) alternate inside one
process, ``rounds`` times, after a warm-up of both.  Each round times ``iters`` steps with device
events; every figure is the median round with the min and max next to it (the run-to-run spread).
``torch.cuda.max_memory_allocated`` is reset before and read after a round of each route.  The
loss of both routes on the same batch (dropout off for that one comparison) is printed too.

    python bench/t5_train_probe.py [rounds] [iters] [--trace] [--xl]

``--xl``: the d_kv = 128 topology instead of T5-base: a SLICE of t5-3b, its width (d_model 1024,
32 heads x 128, d_ff 16384) with 2 + 2 layers instead of 24 + 24, so every layer has the 3B
model's shapes and the step fits a short run; the figures are per-slice, not a 3B step time.

``--trace``: no timing; three steps of the kernel route at each shape, for a separate
``rocprofv3 --kernel-trace --stats -- python bench/t5_train_probe.py --trace`` run.

One JSON line per shape, written as it is measured."""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SWITCH = "CLOUDTIK_AMD_T5_TRAIN_ATTN"
SHAPES = [(16, 128, 128), (8, 512, 128)]         # batch, source tokens, target tokens


def _batch(B, S, T, vocab, dev):
    g = torch.Generator().manual_seed(B * 1000 + S)
    ids = torch.randint(2, vocab, (B, S), generator=g)
    mask = torch.ones(B, S, dtype=torch.long)
    ids[B - 1, S - S // 8:], mask[B - 1, S - S // 8:] = 0, 0        # one padded source
    labels = torch.randint(2, vocab, (B, T), generator=g)
    labels[0, T - T // 8:] = -100
    return ids.to(dev), labels.to(dev), mask.to(dev)


def _step(model, batch):
    model.zero_grad(set_to_none=True)
    loss = model(*batch)
    loss.backward()
    return loss


def _ms(model, batch, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        _step(model, batch)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def _set_dropout(model, rate):
    """The attention reads cfg.dropout_rate; the stacks and feed-forwards keep a copy in ``p``."""
    model.cfg.dropout_rate = rate
    for m in model.modules():
        if isinstance(getattr(m, "p", None), float):
            m.p = rate


def _summary(v):
    return {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    rounds = int(args[0]) if args else 5
    iters = int(args[1]) if len(args) > 1 else 10
    trace = "--trace" in sys.argv
    xl = "--xl" in sys.argv
    from cloudtik_amd import ops
    from cloudtik_amd.models.t5 import T5Config, T5ForConditionalGeneration
    ops.require_native()
    dev = torch.device("cuda", 0)
    props = torch.cuda.get_device_properties(dev)
    print(json.dumps({"device": props.name, "cus": props.multi_processor_count, "rounds": rounds, "iters": iters,
                      "trace": trace}), flush=True)
    torch.manual_seed(0)
    ops.manual_seed(0)
    if xl:
        import dataclasses
        cfg = dataclasses.replace(T5Config.xl(dropout_rate=0.1), num_layers=2, num_decoder_layers=2)
        label = "t5-3b slice, 2 + 2 layers"
    else:
        cfg, label = T5Config.base(dropout_rate=0.1), "t5-base"
    model = T5ForConditionalGeneration(cfg, device=dev).train()
    routes = {"kernels": "1", "sdpa": "0"}
    for B, S, T in SHAPES:
        batch = _batch(B, S, T, model.cfg.vocab_size, dev)
        if trace:
            os.environ[SWITCH] = "1"
            for _ in range(3):
                _step(model, batch)
            torch.cuda.synchronize()
            continue
        # the two routes compute the same loss (dropout off: their dropout streams differ)
        losses = {}
        _set_dropout(model, 0.0)
        for name, sw in routes.items():
            os.environ[SWITCH] = sw
            losses[name] = round(float(_step(model, batch)), 5)
        _set_dropout(model, 0.1)
        for name, sw in routes.items():                      # warm-up of both routes at this shape
            os.environ[SWITCH] = sw
            for _ in range(3):
                _step(model, batch)
        torch.cuda.synchronize()
        runs = {k: [] for k in routes}
        peak = {}
        for _ in range(rounds):                              # the routes alternate
            for name, sw in routes.items():
                os.environ[SWITCH] = sw
                model.zero_grad(set_to_none=True)
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats(dev)
                runs[name].append(_ms(model, batch, iters))
                peak[name] = round(torch.cuda.max_memory_allocated(dev) / 2 ** 20, 1)
        res = {k: _summary(v) for k, v in runs.items()}
        print(json.dumps({"model": label + " (random init, dropout 0.1)", "d_kv": cfg.d_kv, "batch": B, "source": S, "target": T,
                          "step_ms": res, "peak_mib": peak, "loss_no_dropout": losses,
                          "speedup_median": round(res["sdpa"]["median"] / res["kernels"]["median"], 3)}), flush=True)
    os.environ.pop(SWITCH, None)


if __name__ == "__main__":
    main()
