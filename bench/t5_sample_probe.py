"""What sampling adds to a graph-replayed T5 decode step: T5-base, 16 sources x 128 tokens, 32 new
tokens, N = 1 and 4 samples per source, against greedy decoding at the same batch (16 and 64 rows:
the same decoder work per step).

The sampling graph is the greedy one with the sampling kernel in place of the arg-max tail.  It is
measured for three settings: top_k 50; top_p 0.9; top_k 50 with top_p 0.95 and repetition_penalty
1.2.  Only the replays are timed (state reset + one replay per token; the encoder and the capture
are outside), variants alternate ``rounds`` times, and each figure is the fastest round, in
microseconds per token (host clock around synchronised work).

    python bench/t5_sample_probe.py [rounds] [reps]

One JSON line: per-token times, the surplus of each setting over greedy at the same batch, and the
share of distinct tokens in each output (a model that repeats one token would measure an easy row).

The rule's PyTorch ops captured in the same graph are not measured: that variant faulted on the GPU
inside the library's sort and was taken out (profiles/t5_sample/SUMMARY.md)."""
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

B, S, T = 16, 128, 32
SETTINGS = {"k50": dict(top_k=50), "p0.9": dict(top_p=0.9),
            "k50_p0.95_rp1.2": dict(top_k=50, top_p=0.95, repetition_penalty=1.2)}
SEED = 1234


def _replays(st, greedy):
    if greedy:
        st["reset"]()
        for _ in range(T):
            st["graph"].replay()
    else:
        st["reset"](SEED)
        for _ in range(T):
            st["run"]()


def _time(st, greedy, reps):
    _replays(st, greedy)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        _replays(st, greedy)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / (reps * T)


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    from cloudtik_amd import ops
    from cloudtik_amd.models.t5 import T5Config, T5ForConditionalGeneration
    ops.require_native()
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = T5ForConditionalGeneration(T5Config.base(dropout_rate=0.0), device=dev).eval()
    with torch.no_grad():
        model.shared.weight.mul_(0.05)     # tied N(0, 1) embeddings put all mass on one token: flatten the rows
    g = torch.Generator().manual_seed(1)
    x = torch.randint(2, 32128, (4 * B, S), generator=g).to(dev)
    mask = torch.ones(4 * B, S, dtype=torch.long, device=dev)
    mask[::3, S - 17:] = 0

    states, distinct = {}, {}
    for N in (1, 4):
        model.generate(x[:B * N], mask[:B * N], max_new_tokens=T)
        states[f"greedy_b{B * N}"] = next(v for k, v in model._graphs.items() if k[0] == B * N)
        for name, rule in SETTINGS.items():
            out = model._generate_sample_static(x[:B], mask[:B], T, N, SEED, **rule)
            states[f"kernel_n{N}_{name}"] = next(
                v for k, v in model._graphs.items()
                if k[0] == "sample" and k[1] == B * N and k[-1] and
                k[6:10] == (1.0, rule.get("top_k", 0), rule.get("top_p", 1.0), rule.get("repetition_penalty", 1.0)))
            distinct[f"n{N}_{name}"] = round(out.unique().numel() / out.numel(), 3)
            print(f"captured n{N}_{name}", file=sys.stderr, flush=True)
    runs = {k: [] for k in states}
    for _ in range(rounds):                                   # the variants alternate
        for k, st in states.items():
            runs[k].append(round(_time(st, k.startswith("greedy"), reps), 1))
        print("round done", file=sys.stderr, flush=True)
    us = {k: min(v) for k, v in runs.items()}
    surplus = {k: round(v - us[f"greedy_b{B * int(k.split('_n')[1][0])}"], 1) for k, v in us.items()
               if not k.startswith("greedy")}
    print(json.dumps({"model": "t5-base", "sources": B, "source_len": S, "new_tokens": T, "us_per_token": us,
                      "surplus_us_per_token": surplus, "distinct_token_share": distinct, "rounds_us": runs, "reps": reps}),
          flush=True)


if __name__ == "__main__":
    main()
