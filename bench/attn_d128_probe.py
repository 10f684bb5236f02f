"""The head-dim-128 attention kernel against the path the parent commit took for the same call, at
T5-3B's shapes (H = 32, D = 128), and the per-token time of a T5-3B greedy graph decode.

The parent path is built here, not read back from the library: with d_kv = 128 every inference
call fell to
* prefill: ``F.scaled_dot_product_attention`` with the materialised [B, H, Sq, Sk] bias
  (``T5Attention.full_bias``, built per call as the model did),
* decode self-attention (``attention_relbias``): two fp32 einsums, a gather of the bias, a softmax,
* decode cross-attention (``ops.attention``): fp32 matmul, softmax, matmul.

Kernel shapes: ``iters`` calls are captured into one graph per variant and the replays are timed
with device events (device time, no host launch cost: the decode step runs inside a graph too).
Model: ``T5Config.xl()`` random-init, source length 128, 32 new tokens; one captured decode step
per variant (the parent one captured with the two wrappers swapped for the functions above); only
the replays are timed (state reset + one replay per token, host clock around synchronised work).
Variants alternate ``rounds`` times; every figure is the median round with the min and max next
to it (the run-to-run spread).

    python bench/attn_d128_probe.py [rounds] [iters] [--no-model]

One JSON line per shape, written as it is measured."""
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

H, D = 32, 128


# ------------------------------------------------------------------ the parent commit's paths
def parent_relbias(q, k, v, rel_bias, rel_base, key_bias=None, scale=1.0, causal=False):
    """q/k/v [B, S, H, D]: the einsum fallback."""
    Sq, Sk = q.shape[1], k.shape[1]
    idx = (torch.arange(Sk, device=q.device)[None, :] - torch.arange(Sq, device=q.device)[:, None] + rel_base)
    bias = rel_bias.float()[:, idx.clamp(0, rel_bias.shape[1] - 1)][None]
    if key_bias is not None:
        bias = bias + key_bias.float()[:, None, None, :]
    s = torch.einsum("bqhd,bkhd->bhqk", q.float(), k.float()) * scale + bias
    if causal:
        s = s.masked_fill(torch.ones(Sq, Sk, dtype=torch.bool, device=q.device).triu(1), float("-inf"))
    return torch.einsum("bhqk,bkhd->bqhd", torch.softmax(s, -1), v.float()).to(q.dtype)


def parent_attention(q, k, v, key_bias=None, p=0.0, scale=None, causal=False):
    """q/k/v [B, H, S, D]: the fp32 reference."""
    s = torch.matmul(q.float(), k.float().transpose(-1, -2)) * scale
    if key_bias is not None:
        s = s + key_bias.float()[:, None, None, :]
    return torch.matmul(torch.softmax(s, -1), v.float()).to(q.dtype)


def parent_prefill(q, k, v, relvec, rel_base, key_bias, causal):
    """q/k/v [B, S, H, D]: the materialised bias + SDPA branch of T5Attention.forward."""
    Sq, Sk = q.shape[1], k.shape[1]
    dev = q.device
    idx = torch.arange(Sk, device=dev)[None, :] - torch.arange(Sq, device=dev)[:, None] + rel_base
    bias = relvec[:, idx][None]
    if causal:
        bias = bias.masked_fill(~torch.ones(Sq, Sk, dtype=torch.bool, device=dev).tril(0), float("-inf"))
    bias = bias + key_bias[:, None, None, :]
    return F.scaled_dot_product_attention(q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2),
                                          attn_mask=bias.to(q.dtype), scale=1.0).transpose(1, 2)


# ------------------------------------------------------------------ timing
def _graph_of(fn, iters):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(iters):
            fn()
    return g


def _us(g, iters, reps=3):
    g.replay()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        g.replay()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / (reps * iters)


def _summary(v):
    return {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)}


def compare(name, new, old, rounds, iters, meta):
    out_new, out_old = new(), old()
    diff = (out_new.float() - out_old.float()).abs().max().item()
    gs = {"new": _graph_of(new, iters), "parent": _graph_of(old, iters)}
    runs = {k: [] for k in gs}
    for _ in range(rounds):                                   # the variants alternate
        for k, g in gs.items():
            runs[k].append(_us(g, iters))
    res = {k: _summary(v) for k, v in runs.items()}
    print(json.dumps({"shape": name, **meta, "us_per_call": res,
                      "speedup_median": round(res["parent"]["median"] / res["new"]["median"], 2),
                      "max_abs_diff": round(diff, 5)}), flush=True)


def kernel_shapes(dev, rounds, iters):
    from cloudtik_amd import ops
    g = torch.Generator().manual_seed(0)

    def rnd(*shape):
        return (torch.randn(*shape, generator=g) * 0.25).to(dev, torch.bfloat16)

    for B in (1, 16):
        S = 128
        q, k, v = rnd(B, S, H, D), rnd(B, S, H, D), rnd(B, S, H, D)
        relvec = (torch.randn(H, 2 * S - 1, generator=g) * 0.5).to(dev)
        kb = torch.zeros(B, S, device=dev)
        kb[B - 1, S - 17:] = -1e9
        for causal in (False, True):
            compare("prefill", lambda: ops.attention_relbias(q, k, v, relvec, S - 1, kb, scale=1.0, causal=causal),
                    lambda: parent_prefill(q, k, v, relvec, S - 1, kb, causal), rounds, iters,
                    dict(B=B, Sq=S, Sk=S, causal=causal, parent="sdpa+bias"))
        for Sk in (32, 200):
            q1, kc, vc = rnd(B, 1, H, D), rnd(B, Sk, H, D), rnd(B, Sk, H, D)
            rv = (torch.randn(H, Sk, generator=g) * 0.5).to(dev)
            kb1 = torch.zeros(B, Sk, device=dev)
            kb1[:, Sk - 5:] = -1e9                               # slots the decode has not reached
            compare("decode_self", lambda: ops.attention_relbias(q1, kc, vc, rv, 0, kb1, scale=1.0, causal=False),
                    lambda: parent_relbias(q1, kc, vc, rv, 0, kb1, 1.0, False), rounds, iters,
                    dict(B=B, Sq=1, Sk=Sk, causal=False, parent="einsum"))
        q1, ck, cv = rnd(B, 1, H, D), rnd(B, S, H, D), rnd(B, S, H, D)
        compare("decode_cross",
                lambda: ops.attention(q1.transpose(1, 2), ck.transpose(1, 2), cv.transpose(1, 2), key_bias=kb,
                                      scale=1.0).transpose(1, 2),
                lambda: parent_attention(q1.transpose(1, 2), ck.transpose(1, 2), cv.transpose(1, 2), key_bias=kb,
                                         scale=1.0).transpose(1, 2), rounds, iters,
                dict(B=B, Sq=1, Sk=S, causal=False, parent="matmul+softmax"))


def model_decode(dev, rounds, reps):
    from cloudtik_amd import ops
    from cloudtik_amd.models.t5 import T5Config, T5ForConditionalGeneration
    S, T = 128, 32
    torch.manual_seed(0)
    model = T5ForConditionalGeneration(T5Config.xl(dropout_rate=0.0), device=dev).eval()
    for B in (1, 16):
        with torch.no_grad():
            states = {"new": model._capture_decode(B, S, T, torch.bfloat16, dev, True)}
            keep = ops.attention_relbias, ops.attention
            ops.attention_relbias, ops.attention = parent_relbias, parent_attention
            try:
                states["parent"] = model._capture_decode(B, S, T, torch.bfloat16, dev, True)
            finally:
                ops.attention_relbias, ops.attention = keep
        g = torch.Generator().manual_seed(B)
        for st in states.values():
            g.manual_seed(B)
            for ck, cv in st["cross"]:
                ck.copy_((torch.randn(ck.shape, generator=g) * 0.25).to(dev, torch.bfloat16))
                cv.copy_((torch.randn(cv.shape, generator=g) * 0.25).to(dev, torch.bfloat16))

        def tokens(st):
            st["reset"]()
            for _ in range(T):
                st["graph"].replay()

        for st in states.values():
            tokens(st)
        torch.cuda.synchronize()
        same = bool(torch.equal(states["new"]["out"], states["parent"]["out"]))
        runs = {k: [] for k in states}
        for _ in range(rounds):
            for k, st in states.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(reps):
                    tokens(st)
                torch.cuda.synchronize()
                runs[k].append((time.perf_counter() - t0) * 1e6 / (reps * T))
        res = {k: _summary(v) for k, v in runs.items()}
        print(json.dumps({"model": "t5-3b (random init)", "B": B, "source_len": S, "new_tokens": T,
                          "us_per_token": res, "speedup_median": round(res["parent"]["median"] / res["new"]["median"], 3),
                          "same_tokens": same}), flush=True)
        del states


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    rounds = int(args[0]) if args else 5
    iters = int(args[1]) if len(args) > 1 else 50
    from cloudtik_amd import ops
    ops.require_native()
    dev = torch.device("cuda", 0)
    props = torch.cuda.get_device_properties(dev)
    print(json.dumps({"device": props.name, "cus": props.multi_processor_count,
                      "clock_rate_khz": getattr(props, "clock_rate", None), "rounds": rounds, "iters": iters}), flush=True)
    with torch.no_grad():
        kernel_shapes(dev, rounds, iters)
    if "--no-model" not in sys.argv:
        model_decode(dev, rounds, 3)


if __name__ == "__main__":
    main()
