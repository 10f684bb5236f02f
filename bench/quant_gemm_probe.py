"""Time the int8 linear against the bf16 one on the BERT-large encoder shapes, in one process:
``linear_i8`` alone (activations already quantized), ``quantize_rows + linear_i8`` (what a
layer pays per site) and ``torch.addmm`` in bf16, at M = 8192 tokens (64 x 128).

    python bench/quant_gemm_probe.py [iters]

Prints one JSON line per shape (times in microseconds, HIP events, warm-up excluded)."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(3072, 1024), (1024, 1024), (4096, 1024), (1024, 4096)]   # (N, K): qkv, out, ffn1, ffn2
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


def main():
    iters = int(sys.argv[1]) if len(sys.argv) > 1 else 50
    from cloudtik_amd import ops
    ops.require_native()
    g = torch.Generator(device="cuda").manual_seed(0)
    for N, K in SHAPES:
        x = torch.randn(M, K, device="cuda", generator=g).to(torch.bfloat16)
        w = (torch.randn(N, K, device="cuda", generator=g) * K ** -0.5).to(torch.bfloat16)
        b = torch.randn(N, device="cuda", generator=g).to(torch.bfloat16)
        w_q, w_s = ops.quantize_weight(w)
        xq = ops.quantize_rows(x)
        t_gemm = _time(lambda: ops.linear_i8(xq, w_q, w_s, b), iters)
        t_quant = _time(lambda: ops.quantize_rows(x), iters)
        t_both = _time(lambda: ops.linear_i8(ops.quantize_rows(x), w_q, w_s, b), iters)
        t_bf16 = _time(lambda: torch.addmm(b, x, w.t()), iters)
        err = ((ops.linear_i8(xq, w_q, w_s, b).float() - torch.addmm(b, x, w.t()).float()).norm()
               / torch.addmm(b, x, w.t()).float().norm()).item()
        ops_ = 2.0 * M * N * K
        print(json.dumps({"M": M, "N": N, "K": K, "linear_i8_us": round(t_gemm, 1),
                          "quantize_rows_us": round(t_quant, 1), "quantize_plus_linear_i8_us": round(t_both, 1),
                          "addmm_bf16_us": round(t_bf16, 1), "linear_i8_tops": round(ops_ / t_gemm / 1e6, 1),
                          "addmm_bf16_tflops": round(ops_ / t_bf16 / 1e6, 1), "rel_vs_bf16": round(err, 5),
                          "iters": iters}), flush=True)


if __name__ == "__main__":
    main()
