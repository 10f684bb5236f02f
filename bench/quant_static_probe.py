"""Time the static-quantization producers against what they replace, per site and per layer, at
M = 8192 tokens (64 x 128) and the BERT-base and BERT-large widths, in one process:

- ``layer_norm`` alone against ``layer_norm_quant`` (bias + residual folded in, as in a layer);
- the ``ffn1`` GEMM with bias + GELU writing bf16 against the same writing int8;
- the ``ffn2`` GEMM fed by static int8 against the dynamic one with per-token scales;
- ``quantize_static`` against ``quantize_rows`` at both widths of a layer;
- a layer's linears, LayerNorms and casts (everything but attention) chained as the dynamic
  model, the static unfused model, the static fused model and the bf16 model run them.

    python bench/quant_static_probe.py [iters] [rounds]

The variants of a group alternate ``rounds`` times; each figure is the fastest round (all rounds
are printed too).  One JSON line per group, times in microseconds, HIP events, warm-up excluded."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WIDTHS = {"bert-base": (768, 3072), "bert-large": (1024, 4096)}
M = 8192


def _time(fn, iters, warmup=5):
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


def _group(name, model, variants, iters, rounds):
    runs = {k: [] for k in variants}
    for _ in range(rounds):                                  # a, b, c, a, b, c: the variants alternate
        for k, fn in variants.items():
            runs[k].append(round(_time(fn, iters), 1))
    print(json.dumps({"group": name, "model": model, "M": M, "us": {k: min(v) for k, v in runs.items()},
                      "rounds_us": runs, "iters": iters}), flush=True)


def main():
    iters = int(sys.argv[1]) if len(sys.argv) > 1 else 50
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    from cloudtik_amd import ops
    ops.require_native()
    g = torch.Generator(device="cuda").manual_seed(0)
    bf = lambda *s, std=1.0: (torch.randn(*s, device="cuda", generator=g) * std).to(torch.bfloat16)
    for model, (H, I) in WIDTHS.items():
        x, res, ctx, act = bf(M, H), bf(M, H), bf(M, H, std=0.3), bf(M, I, std=0.5)
        gamma, beta, bias_h, bias_i = bf(H, std=0.1) + 1, bf(H, std=0.1), bf(H, std=0.1), bf(I, std=0.1)
        w = {"qkv": bf(3 * H, H, std=H ** -0.5), "out": bf(H, H, std=H ** -0.5),
             "ffn1": bf(I, H, std=H ** -0.5), "ffn2": bf(H, I, std=I ** -0.5)}
        bias_qkv = bf(3 * H, std=0.1)
        wq = {k: ops.quantize_weight(v) for k, v in w.items()}
        # ranges as calibration would give them: the largest value of each site's input
        amax = {"qkv": 4.5, "out": float(ctx.float().abs().max()), "ffn1": 4.5, "ffn2": float(act.float().abs().max())}
        ln = lambda t, r: ops.layer_norm(t, gamma, beta, 1e-12, bias=bias_h, residual=r, training=False)
        lnq = lambda t, r, a: ops.layer_norm_quant(t, gamma, beta, 1e-12, bias=bias_h, residual=r, amax=a)
        lin = lambda s, t, b=None, a=ops.ACT_NONE: ops.linear_i8(t, *wq[s], b, a)
        slin = lambda s, t, b=None, a=ops.ACT_NONE, o=None: ops.linear_i8_static(t, amax[s], *wq[s], b, a, out_amax=o)

        _group("layer_norm", model, {"layer_norm": lambda: ln(x, res), "layer_norm_quant": lambda: lnq(x, res, 4.5),
                                     "layer_norm+quantize_static": lambda: ops.quantize_static(ln(x, res), 4.5)},
               iters, rounds)
        x_q = ops.quantize_static(x, amax["ffn1"])
        _group("ffn1", model, {"bf16_out": lambda: slin("ffn1", x_q, bias_i, ops.ACT_GELU),
                               "int8_out": lambda: slin("ffn1", x_q, bias_i, ops.ACT_GELU, amax["ffn2"]),
                               "bf16_out+quantize_static": lambda: ops.quantize_static(
                                   slin("ffn1", x_q, bias_i, ops.ACT_GELU), amax["ffn2"])}, iters, rounds)
        h_q, h_rows = ops.quantize_static(act, amax["ffn2"]), ops.quantize_rows(act)
        _group("ffn2", model, {"static": lambda: slin("ffn2", h_q), "dynamic": lambda: lin("ffn2", h_rows),
                               "addmm_bf16": lambda: torch.mm(act, w["ffn2"].t())}, iters, rounds)
        _group("quantize", model, {f"quantize_static_K{H}": lambda: ops.quantize_static(x, 4.5),
                                   f"quantize_rows_K{H}": lambda: ops.quantize_rows(x),
                                   f"quantize_static_K{I}": lambda: ops.quantize_static(act, amax["ffn2"]),
                                   f"quantize_rows_K{I}": lambda: ops.quantize_rows(act)}, iters, rounds)

        # a layer without its attention: ctx is a fixed tensor standing for the attention output
        def dynamic():
            lin("qkv", ops.quantize_rows(x), bias_qkv)
            x1 = ln(lin("out", ops.quantize_rows(ctx)), x)
            h = lin("ffn1", ops.quantize_rows(x1), bias_i, ops.ACT_GELU)
            return ln(lin("ffn2", ops.quantize_rows(h)), x1)

        def static_unfused():
            slin("qkv", ops.quantize_static(x, amax["qkv"]), bias_qkv)
            x1 = ln(slin("out", ops.quantize_static(ctx, amax["out"])), x)
            h = slin("ffn1", ops.quantize_static(x1, amax["ffn1"]), bias_i, ops.ACT_GELU)
            y = ln(slin("ffn2", ops.quantize_static(h, amax["ffn2"])), x1)
            return y, ops.quantize_static(y, amax["qkv"])            # the next layer's qkv input

        def static_fused(x_q=ops.quantize_static(x, amax["qkv"])):
            slin("qkv", x_q, bias_qkv)
            x1, x1_q = lnq(slin("out", ops.quantize_static(ctx, amax["out"])), x, amax["ffn1"])
            h_q = slin("ffn1", x1_q, bias_i, ops.ACT_GELU, amax["ffn2"])
            return lnq(slin("ffn2", h_q), x1, amax["qkv"])

        def bf16():
            torch.addmm(bias_qkv, x, w["qkv"].t())
            x1 = ln(torch.mm(ctx, w["out"].t()), x)
            h = ops.bias_gelu(torch.mm(x1, w["ffn1"].t()), bias_i)
            return ln(torch.mm(h, w["ffn2"].t()), x1)

        a, b = static_unfused(), static_fused()
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), "fused and unfused disagree"
        _group("layer_without_attention", model, {"dynamic": dynamic, "static_unfused": static_unfused,
                                                  "static_fused": static_fused, "bf16": bf16}, iters, rounds)


if __name__ == "__main__":
    main()
