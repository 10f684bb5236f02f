"""What beam search adds to a graph-replayed T5 decode step: T5-base, 16 sources x 128 tokens,
32 new tokens, 4 beams, against greedy decoding at batch 64 (the same decoder work per step).

Three beam variants share the captured decoder step and differ in the bookkeeping after the
logits: the HIP kernels (``fused``), ``beam_step_reference`` taking its 2K candidates with
``torch.topk`` as the library does (``torch_topk``), and the same with the full stable sort the
rule is written with (``torch_sort``).  Only the replays are timed (state reset + one replay per
token; the encoder and the capture are outside), variants alternate ``rounds`` times, and each
figure is the fastest round, in microseconds per token (host clock around synchronised work).

    python bench/t5_beam_probe.py [rounds] [reps]

One JSON line: per-token times, the surplus of each beam variant over greedy, whether the three
beam variants returned the same tokens, and the device kernels per decode step of each beam variant
(counted by the profiler over an eager run of the same step; null if it cannot count)."""
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

B, S, T, K = 16, 128, 32, 4


def _replays(st, greedy):
    st["reset"]()
    if greedy:
        for _ in range(T):
            st["graph"].replay()
    else:
        for t in range(T):
            st["steps"][t & 1]()


def _time(st, greedy, reps):
    _replays(st, greedy)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        _replays(st, greedy)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / (reps * T)


def _kernels_per_step(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)
        return round(n / T, 1) if n else None
    except Exception:  # noqa: BLE001 - the count is a side figure
        return None


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    from cloudtik_amd import ops
    from cloudtik_amd.models.t5 import T5Config, T5ForConditionalGeneration
    ops.require_native()
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = T5ForConditionalGeneration(T5Config.base(dropout_rate=0.0), device=dev).eval()
    g = torch.Generator().manual_seed(1)
    x = torch.randint(2, 32128, (B * K, S), generator=g).to(dev)
    mask = torch.ones(B * K, S, dtype=torch.long, device=dev)
    mask[::3, S - 17:] = 0

    beam = lambda **kw: model._generate_beam_static(x[:B], mask[:B], T, K, 1.0, False, **kw)
    outs = {"fused": beam(), "torch_topk": beam(fused=False, select="topk"), "torch_sort": beam(fused=False)}
    model.generate(x, mask, max_new_tokens=T)
    states = {"greedy_b64": next(v for k, v in model._graphs.items() if k[0] != "beam")}
    for k, v in model._graphs.items():
        if k[0] == "beam":
            states["fused" if k[9] else "torch_" + k[11]] = v
    runs = {k: [] for k in states}
    for _ in range(rounds):                                   # the variants alternate
        for k, st in states.items():
            runs[k].append(round(_time(st, k == "greedy_b64", reps), 1))
    us = {k: min(v) for k, v in runs.items()}
    kernels = {
        "fused": _kernels_per_step(lambda: beam(graph=False)),
        "torch_topk": _kernels_per_step(lambda: beam(fused=False, graph=False, select="topk")),
        "torch_sort": _kernels_per_step(lambda: beam(fused=False, graph=False)),
    }
    print(json.dumps({
        "model": "t5-base", "sources": B, "source_len": S, "new_tokens": T, "num_beams": K,
        "us_per_token": us, "surplus_us_per_token": {k: round(v - us["greedy_b64"], 1) for k, v in us.items()
                                                     if k != "greedy_b64"},
        "same_tokens": bool(all(torch.equal(outs["fused"][0], o[0]) for o in outs.values())),
        "kernels_per_step_eager": kernels, "rounds_us": runs, "reps": reps}), flush=True)


if __name__ == "__main__":
    main()
