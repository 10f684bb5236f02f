"""The fused gated-GELU feed-forward of T5 v1.1 (``ops.gated_gelu``) against the PyTorch composition it
replaces: the op alone, a v1.1-base training step and greedy graph decoding.

The two routes alternate inside one process, ``rounds`` times, after a warm-up of both; a round times
``iters`` calls with device events; every figure is the median round with the min and max next to it
(the round-to-round spread).

* ``op``: forward and backward at rows 2048 / 4096 x F 2048 / 2816 / 5120 / 10240, dropout 0.1.  The
  composition is ``F.dropout(F.gelu(g, approximate="tanh") * u, 0.1)`` and its autograd.  Calls walk a ring
  of input sets of at least 1 GiB, so no call finds its inputs in the 256 MiB Infinity Cache.  Bytes/s from
  the bytes the algorithm needs (forward 3 M F 2, backward 5 M F 2) and their share of the HBM rate a
  copy reaches (6.29 TB/s).
* ``train``: forward + backward of a v1.1-base model (random init, dropout 0.1) at 16 x 128 -> 128 and
  8 x 512 -> 128 tokens, ``CLOUDTIK_AMD_T5_FUSED_FF=1`` against ``0`` (read per call), with the peak memory
  of a round of each.
* ``decode``: one replay of the captured greedy decode step at 1 and 16 sources of 128 tokens, bf16 and
  int8; the switch is read at capture, so each setting has its own capture and the replays alternate.

    python bench/t5_ff_probe.py [rounds] [iters] [--only op|train|decode]

One JSON line per measurement, written as it is measured."""
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SWITCH = "CLOUDTIK_AMD_T5_FUSED_FF"
HBM_BYTES_PER_S = 6.29e12                    # measured float4 copy, MI355X
OP_ROWS, OP_F = (2048, 4096), (2048, 2816, 5120, 10240)
TRAIN_SHAPES = [(16, 128, 128), (8, 512, 128)]         # batch, source tokens, target tokens
DECODE_BATCHES, DECODE_SOURCE, DECODE_STEPS = (1, 16), 128, 32
P = 0.1


def _summary(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def _timed(fn, iters):
    """Milliseconds per call of ``fn(i)`` over ``iters`` calls."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for i in range(iters):
        fn(i)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def _alternate(routes, rounds, iters, before=None):
    """{route: [ms per call, one per round]}, the routes taking turns."""
    runs = {k: [] for k in routes}
    for _ in range(rounds):
        for name, fn in routes.items():
            if before is not None:
                before(name)
            runs[name].append(_timed(fn, iters))
    return runs


# ------------------------------------------------------------------------------------- the op
def probe_op(ops, dev, rounds, iters):
    def composed(g, u):
        return F.dropout(F.gelu(g, approximate="tanh") * u, P)

    def fused(g, u):
        return ops.gated_gelu(g, u, P)

    for M in OP_ROWS:
        for Fd in OP_F:
            one = M * Fd * 2
            nset = max(2, -(-2 ** 30 // (3 * one)))
            gen = torch.Generator(device=dev).manual_seed(M + Fd)
            sets = [tuple((torch.randn(M, Fd, device=dev, generator=gen) * s).bfloat16().requires_grad_(r)
                          for s, r in ((2, True), (2, True), (1, False))) for _ in range(nset)]
            res = {}
            for direction, need in (("fwd", 3 * one), ("bwd", 5 * one)):
                routes = {}
                for name, fn in (("fused", fused), ("composed", composed)):
                    if direction == "fwd":
                        routes[name] = lambda i, fn=fn: fn(*sets[i % nset][:2])
                    else:
                        outs = [fn(g, u) for g, u, _ in sets]          # one autograd graph per input set
                        routes[name] = lambda i, outs=outs: torch.autograd.grad(
                            outs[i % nset], sets[i % nset][:2], sets[i % nset][2], retain_graph=True)
                for fn in routes.values():                             # warm-up of both
                    for i in range(nset + 2):
                        fn(i)
                runs = _alternate(routes, rounds, iters)
                res[direction] = {}
                for name, v in runs.items():
                    s = _summary(v)
                    rate = need / (s["median"] * 1e-3)
                    res[direction][name] = {"ms": s, "tb_per_s": round(rate / 1e12, 3),
                                            "hbm_share": round(rate / HBM_BYTES_PER_S, 3)}
                res[direction]["speedup_median"] = round(
                    res[direction]["composed"]["ms"]["median"] / res[direction]["fused"]["ms"]["median"], 3)
                del routes
            print(json.dumps({"probe": "op", "rows": M, "F": Fd, "p": P, "input_sets": nset, **res}), flush=True)
            del sets
            torch.cuda.empty_cache()


# ----------------------------------------------------------------------------------- training
def _batch(B, S, T, vocab, dev):
    g = torch.Generator().manual_seed(B * 1000 + S)
    ids = torch.randint(2, vocab, (B, S), generator=g)
    mask = torch.ones(B, S, dtype=torch.long)
    ids[B - 1, S - S // 8:], mask[B - 1, S - S // 8:] = 0, 0        # one padded source
    labels = torch.randint(2, vocab, (B, T), generator=g)
    labels[0, T - T // 8:] = -100
    return ids.to(dev), labels.to(dev), mask.to(dev)


def probe_train(model, dev, rounds, iters):
    model.train()

    def step(_):
        model.zero_grad(set_to_none=True)
        model(*batch).backward()

    routes = {"fused": step, "composed": step}
    switch = {"fused": "1", "composed": "0"}
    for B, S, T in TRAIN_SHAPES:
        batch = _batch(B, S, T, model.cfg.vocab_size, dev)
        for name in routes:                                         # warm-up of both routes at this shape
            os.environ[SWITCH] = switch[name]
            for i in range(3):
                step(i)
        peak = {}

        def before(name):
            if before.last is not None:
                peak[before.last] = round(torch.cuda.max_memory_allocated(dev) / 2 ** 20, 1)
            os.environ[SWITCH] = switch[name]
            model.zero_grad(set_to_none=True)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats(dev)
            before.last = name

        before.last = None
        runs = _alternate(routes, rounds, iters, before)
        before("fused")                                             # closes the last round's peak
        res = {k: _summary(v) for k, v in runs.items()}
        print(json.dumps({"probe": "train", "model": "t5-v1.1-base (random init, dropout 0.1)", "batch": B, "source": S,
                          "target": T, "step_ms": res, "peak_mib": peak,
                          "speedup_median": round(res["composed"]["median"] / res["fused"]["median"], 3)}), flush=True)
    os.environ.pop(SWITCH, None)
    model.zero_grad(set_to_none=True)


# ------------------------------------------------------------------------------------- decode
def probe_decode(model, label, dev, rounds, iters):
    model.eval()
    T = DECODE_STEPS
    for B in DECODE_BATCHES:
        ids, _, mask = _batch(max(B, 2), DECODE_SOURCE, 8, model.cfg.vocab_size, dev)
        ids, mask = ids[:B], mask[:B]
        states, tokens = {}, {}
        for name, sw in (("fused", "1"), ("composed", "0")):
            os.environ[SWITCH] = sw
            model._graphs = {}                                      # the switch is read at capture
            tokens[name] = model.generate(ids, mask, max_new_tokens=T)
            (states[name],) = model._graphs.values()
        model._graphs = {}

        def replays(st):
            def run(_):
                st["reset"]()
                for _ in range(T):
                    st["graph"].replay()
            return run

        routes = {k: replays(st) for k, st in states.items()}
        for fn in routes.values():
            fn(0)
        runs = _alternate(routes, rounds, max(1, iters // 2))
        res = {k: _summary([ms / T for ms in v]) for k, v in runs.items()}
        same = int((tokens["fused"] == tokens["composed"]).sum())
        print(json.dumps({"probe": "decode", "model": "t5-v1.1-base " + label, "sources": B, "source_tokens": DECODE_SOURCE,
                          "steps": T, "token_ms": res, "tokens_equal": f"{same} / {tokens['fused'].numel()}",
                          "speedup_median": round(res["composed"]["median"] / res["fused"]["median"], 3)}), flush=True)
        del states, routes
    os.environ.pop(SWITCH, None)


def main():
    argv = sys.argv[1:]
    only = None
    if "--only" in argv:
        at = argv.index("--only")
        only = argv[at + 1]
        if only not in ("op", "train", "decode"):
            raise SystemExit(f"--only takes op, train or decode, got {only!r}")
        del argv[at:at + 2]
    rounds = int(argv[0]) if argv else 5
    iters = int(argv[1]) if len(argv) > 1 else 10
    from cloudtik_amd import ops
    from cloudtik_amd.models.t5 import T5Config, T5ForConditionalGeneration
    ops.require_native()
    dev = torch.device("cuda", 0)
    props = torch.cuda.get_device_properties(dev)
    print(json.dumps({"device": props.name, "cus": props.multi_processor_count, "rounds": rounds, "iters": iters}),
          flush=True)
    torch.manual_seed(0)
    ops.manual_seed(0)
    if only in (None, "op"):
        probe_op(ops, dev, rounds, iters)
    if only in (None, "train", "decode"):
        model = T5ForConditionalGeneration(T5Config.v1_1("base", dropout_rate=0.1), device=dev)
        if only in (None, "train"):
            probe_train(model, dev, rounds, iters)
        if only in (None, "decode"):
            with torch.no_grad():
                probe_decode(model, "bf16", dev, rounds, iters)
                probe_decode(model.eval().quantize_dynamic(), "int8", dev, rounds, iters)


if __name__ == "__main__":
    main()
