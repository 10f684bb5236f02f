"""What the token bans add to a graph-replayed T5 decode step: T5-base, 16 sources x 128 tokens, 32
and 200 new tokens, for greedy decoding, 4-beam search and top-k sampling, each with
``no_repeat_ngram_size=3, min_length=30`` (the stock summarisation settings) against the same mode
without constraints, which is the graph the parent commit captures.

The constrained graph is the plain one with one launch of the ban kernel after the logits (and, for
beam search, one elementwise ``logaddexp`` on [64] that restores the log-sum-exp).  Only the replays
are timed (state reset + one replay per token; the encoder and the capture are outside), variants
alternate ``rounds`` times, and each figure is the fastest round, in microseconds per token (host
clock around synchronised work).

    python bench/t5_constrain_probe.py [rounds] [reps at 32 tokens] [reps at 200 tokens]

Every constrained variant is captured right after its plain twin.  Two captures of one graph can
replay tens of microseconds apart (profiles/t5_constrain/SUMMARY.md), so a surplus of a few
microseconds is an order of magnitude, not a figure.

One JSON line: per-token times, the surplus of each constrained variant over its plain twin, every
round's figure, and the share of distinct tokens in each output.

The rule's PyTorch ops captured in a graph are not measured: nothing here runs a reference in a
captured graph on the GPU (profiles/t5_sample/SUMMARY.md records why)."""
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

B, S, K = 16, 128, 4
STEPS = (32, 200)
BANS = dict(no_repeat_ngram_size=3, min_length=30)
TOP_K = 50
SEED = 1234


def _replays(st, mode, T):
    if mode == "greedy":
        st["reset"]()
        for _ in range(T):
            st["graph"].replay()
    elif mode == "beam":
        st["reset"]()
        for t in range(T):
            st["steps"][t & 1]()
    else:
        st["reset"](SEED)
        for _ in range(T):
            st["run"]()


def _time(st, mode, T, reps):
    _replays(st, mode, T)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        _replays(st, mode, T)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / (reps * T)


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    reps = {32: int(sys.argv[2]) if len(sys.argv) > 2 else 5, 200: int(sys.argv[3]) if len(sys.argv) > 3 else 2}
    from cloudtik_amd import ops
    from cloudtik_amd.models.t5 import T5Config, T5ForConditionalGeneration
    ops.require_native()
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = T5ForConditionalGeneration(T5Config.base(dropout_rate=0.0), device=dev).eval()
    with torch.no_grad():
        model.shared.weight.mul_(0.05)     # tied N(0, 1) embeddings put all mass on one token: flatten the rows
    g = torch.Generator().manual_seed(1)
    x = torch.randint(2, 32128, (B, S), generator=g).to(dev)
    mask = torch.ones(B, S, dtype=torch.long, device=dev)
    mask[::3, S - 17:] = 0

    calls = {"greedy": dict(), "beam": dict(num_beams=K), "sample": dict(do_sample=True, top_k=TOP_K, seed=SEED)}
    states, distinct = {}, {}
    for T in STEPS:
        for mode, kw in calls.items():
            for name, bans in (("plain", {}), ("bans", BANS)):
                before = set(model._graphs) if hasattr(model, "_graphs") else set()
                out = model.generate(x, mask, max_new_tokens=T, **kw, **bans)
                new = set(model._graphs) - before
                assert len(new) == 1, new                      # this call's capture
                states[f"{mode}_{name}_t{T}"] = (model._graphs[new.pop()], mode, T)
                distinct[f"{mode}_{name}_t{T}"] = round(out.unique().numel() / out.numel(), 3)
                print(f"captured {mode}_{name}_t{T}", file=sys.stderr, flush=True)
    runs = {k: [] for k in states}
    for _ in range(rounds):                                   # the variants alternate
        for k, (st, mode, T) in states.items():
            runs[k].append(round(_time(st, mode, T, reps[T]), 1))
        print("round done", file=sys.stderr, flush=True)
    us = {k: min(v) for k, v in runs.items()}
    surplus = {k: round(v - us[k.replace("_bans_", "_plain_")], 1) for k, v in us.items() if "_bans_" in k}
    print(json.dumps({"model": "t5-base", "sources": B, "source_len": S, "num_beams": K, "top_k": TOP_K, "bans": BANS,
                      "us_per_token": us, "surplus_us_per_token": surplus, "distinct_token_share": distinct,
                      "rounds_us": runs, "reps": reps}), flush=True)


if __name__ == "__main__":
    main()
