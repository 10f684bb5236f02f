"""Int8 against bf16 T5 on one GPU, same process, same weights, the variants alternating.

    python bench/t5_quant_probe.py model  [base|large] [rounds] [reps]
    python bench/t5_quant_probe.py gemm   [rounds] [reps]
    python bench/t5_quant_probe.py launches [base|large]

``model``: graph-replayed decode time per token at 1 x 1, 16 x 1 and 16 x 4 beams (source length 128,
32 new tokens; only the replays are timed, the encoder and the captures are outside) and the
encoder time at 16 x 128, for the bf16 model and its ``quantize_dynamic()`` copy.  Each figure is the
fastest of ``rounds`` alternating rounds of ``reps`` repetitions (host clock around synchronised work).

``gemm``: the decode GEMM (``gemm_i8_skinny``, one launch, int8 rows in: what follows a fused norm)
against what it replaces (``quant_rows_i8`` + ``gemm_i8_nt``, two launches, bf16 rows in: the route
``CLOUDTIK_AMD_I8_SKINNY=0`` takes) and against the skinny kernel behind the same ``quant_rows_i8``
(what follows attention and the ReLU), at M = 1, 16, 64 on the four decode shapes of T5-base and its
32128-wide head.  Each variant is captured as a graph of 20 calls;
microseconds per call.

``launches``: kernels per eager static decode step (16 rows), counted by the profiler in a run of
its own; per decoder layer = (the step of a three-layer decoder - that of a one-layer decoder) / 2.

One JSON line each."""
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

S, T = 128, 32


def _models(size, dev):
    from cloudtik_amd.models.t5 import T5Config, T5ForConditionalGeneration
    torch.manual_seed(0)
    bf = T5ForConditionalGeneration(getattr(T5Config, size)(dropout_rate=0.0), device=dev).eval()
    with torch.no_grad():
        bf.shared.weight.mul_(0.05)        # tied N(0, 1) embeddings put all mass on one token: flatten the rows
    return {"bf16": bf, "int8": bf.quantize_dynamic()}


def _sources(B, dev):
    g = torch.Generator().manual_seed(1)
    x = torch.randint(2, 32128, (B, S), generator=g).to(dev)
    mask = torch.ones(B, S, dtype=torch.long, device=dev)
    mask[::3, S - 17:] = 0
    return x, mask


def _timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / reps


def run_model(size, rounds, reps):
    dev = torch.device("cuda", 0)
    models = _models(size, dev)
    runs, agree = {}, {}
    fns = {}
    for B, K in ((1, 1), (16, 1), (16, 4)):
        x, mask = _sources(B, dev)
        outs = {}
        for name, m in models.items():
            outs[name] = m.generate(x, mask, max_new_tokens=T, num_beams=K)
            if K == 1:
                st = next(v for k, v in m._graphs.items() if k[0] == B and k[1] == S)

                def replay(st=st):
                    st["reset"]()
                    for _ in range(T):
                        st["graph"].replay()
            else:
                st = next(v for k, v in m._graphs.items() if k[0] == "beam" and k[1] == B and k[6] == K)

                def replay(st=st):
                    st["reset"]()
                    for t in range(T):
                        st["steps"][t & 1]()
            fns[f"decode_{B}x{K}_{name}"] = (replay, T)
        agree[f"{B}x{K}"] = round((outs["bf16"] == outs["int8"]).float().mean().item(), 3)
        print(f"captured {B}x{K}", file=sys.stderr, flush=True)
    x, mask = _sources(16, dev)
    for name, m in models.items():
        fns[f"encoder_16x{S}_{name}"] = ((lambda m=m: m.encoder(x, mask)), 1)
    with torch.no_grad():
        for _ in range(rounds):
            for k, (fn, per) in fns.items():
                runs.setdefault(k, []).append(round(_timed(fn, reps) / per, 1))
            print("round done", file=sys.stderr, flush=True)
    us = {k: min(v) for k, v in runs.items()}
    ratio = {k[:-5]: round(us[k] / us[k[:-5] + "_bf16"], 3) for k in us if k.endswith("_int8")}
    print(json.dumps({"probe": "model", "model": f"t5-{size}", "source_len": S, "new_tokens": T,
                      "us_per_token_or_call": us, "int8_over_bf16": ratio, "token_agreement_with_bf16": agree,
                      "rounds_us": runs, "reps": reps}), flush=True)


GEMM_SHAPES = {"qkv": (2304, 768), "o": (768, 768), "wi": (3072, 768), "wo": (768, 3072), "head": (32128, 768)}
CALLS = 20


def run_gemm(rounds, reps):
    from cloudtik_amd import ops
    C = ops.require_native()
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(0)
    graphs, keep = {}, []
    for site, (N, K) in GEMM_SHAPES.items():
        w_q, w_s = ops.quantize_weight(torch.randn(N, K, generator=g) * K ** -0.5)
        w_q, w_s = w_q.to(dev), w_s.to(dev)
        for M in (1, 16, 64):
            x = torch.randn(M, K, generator=g).to(torch.bfloat16).to(dev)
            q, s = ops.quantize_rows(x)
            out = torch.empty(M, N, device=dev, dtype=torch.bfloat16)

            # the operands are default arguments: a graph replays over the addresses it captured, and
            # torch.cuda.graph() empties the allocator's cache on entry, so a tensor the next iteration
            # let go of would be unmapped under the graphs captured before; `keep` holds them all
            def skinny(q=q, s=s, w_q=w_q, w_s=w_s, out=out):
                C.gemm_i8_skinny(q, s, w_q, w_s, None, 0, None, out)

            def quant_skinny(x=x, w_q=w_q, w_s=w_s, out=out):
                q2, s2 = C.quant_rows_i8(x)
                C.gemm_i8_skinny(q2, s2, w_q, w_s, None, 0, None, out)

            def quant_tiled(x=x, w_q=w_q, w_s=w_s, out=out):
                q2, s2 = C.quant_rows_i8(x)
                C.gemm_i8_nt(q2, s2, w_q, w_s, None, 0, out)

            keep.append((x, q, s, w_q, w_s, out))
            for name, fn in (("skinny", skinny), ("quant+skinny", quant_skinny), ("quant+tiled", quant_tiled)):
                fn()
                torch.cuda.synchronize()
                gr = torch.cuda.CUDAGraph()
                with torch.cuda.graph(gr):
                    for _ in range(CALLS):
                        fn()
                graphs[f"{site}_M{M}_{name}"] = gr
    runs = {}
    for _ in range(rounds):
        for k, gr in graphs.items():
            runs.setdefault(k, []).append(round(_timed(gr.replay, reps) / CALLS, 2))
    us = {k: min(v) for k, v in runs.items()}
    print(json.dumps({"probe": "gemm", "shapes_N_K": GEMM_SHAPES, "calls_per_graph": CALLS, "us_per_call": us,
                      "reps": reps, "rounds": rounds}), flush=True)


def run_launches(size):
    from torch.profiler import ProfilerActivity, profile
    from cloudtik_amd.models.t5 import T5Config, T5ForConditionalGeneration
    dev = torch.device("cuda", 0)
    B = 16
    x, mask = _sources(B, dev)
    counts = {}
    for layers in (1, 3):
        torch.manual_seed(0)
        cfg = getattr(T5Config, size)(dropout_rate=0.0)
        cfg.num_layers, cfg.num_decoder_layers = 1, layers
        bf = T5ForConditionalGeneration(cfg, device=dev).eval()
        for name, m in (("bf16", bf), ("int8", bf.quantize_dynamic())):
            m.generate(x, mask, max_new_tokens=4)
            st = next(v for k, v in m._graphs.items() if k[0] == B)
            st["reset"]()
            st["step"]()
            torch.cuda.synchronize()
            with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
                st["step"]()
                torch.cuda.synchronize()
            kernels = [e.name for e in prof.events()
                       if str(e.device_type).endswith("CUDA") and "emcpy" not in e.name and "emset" not in e.name]
            counts[f"{name}_layers{layers}"] = len(kernels)
            if layers == 3:
                counts[f"{name}_names"] = sorted(set(kernels))
    per_layer = {n: (counts[f"{n}_layers3"] - counts[f"{n}_layers1"]) / 2 for n in ("bf16", "int8")}
    print(json.dumps({"probe": "launches", "model": f"t5-{size}", "rows": B, "kernels_per_step": counts,
                      "kernels_per_decoder_layer": per_layer}), flush=True)


def main():
    from cloudtik_amd import ops
    ops.require_native()
    if not torch.cuda.is_available():
        raise SystemExit("t5_quant_probe needs a GPU")
    what = sys.argv[1] if len(sys.argv) > 1 else "model"
    if what == "model":
        run_model(sys.argv[2] if len(sys.argv) > 2 else "base", int(sys.argv[3]) if len(sys.argv) > 3 else 5,
                  int(sys.argv[4]) if len(sys.argv) > 4 else 3)
    elif what == "gemm":
        run_gemm(int(sys.argv[2]) if len(sys.argv) > 2 else 5, int(sys.argv[3]) if len(sys.argv) > 3 else 20)
    elif what == "launches":
        run_launches(sys.argv[2] if len(sys.argv) > 2 else "base")
    else:
        raise SystemExit(__doc__)


if __name__ == "__main__":
    main()
