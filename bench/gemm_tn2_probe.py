"""Weight-gradient GEMM dW = dY^T X on the BERT-large shapes (tokens 32768): the MFMA kernel's
TN layout (ct_gemm_tn2, split-K into fp32 slabs) vs hipBLASLt's batched split-K GEMM (the
current wgrad path), each followed by the same splitk_reduce into a bf16 gradient.

    python bench/gemm_tn2_probe.py [--tokens 32768]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timeit(fn, iters=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(True), torch.cuda.Event(True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e3


def group_mode(C, T):
    """Each BERT-large pair as one grouped launch + one grouped reduce against the two separate
    gemm_tn2(_bias) + splitk_reduce(2) calls it replaces (what wgrad_accumulate issues)."""
    from cloudtik_amd.ops.linear import tn2_group_splits, tn2_splits
    g = torch.Generator(device="cuda").manual_seed(0)
    bf = torch.bfloat16
    pairs = [("wo+qkv", (1024, 1024, False), (3072, 1024, True)), ("ffn2+ffn1", (1024, 4096, False), (4096, 1024, True))]
    for name, *shapes in pairs:
        ops_ = []
        for N, K, bias in shapes:
            dy = torch.randn(T, N, device="cuda", generator=g).to(bf)
            x = (torch.randn(T, K, device="cuda", generator=g) * T ** -0.5).to(bf)
            ops_.append((dy, x, torch.zeros(N, K, device="cuda", dtype=bf),
                         torch.zeros(N, device="cuda", dtype=bf) if bias else None, tn2_splits(T, N, K)))
        Sg = tn2_group_splits(T, [(N, K) for N, K, _ in shapes])
        Ps = [torch.empty(S, dy.shape[1], x.shape[1], device="cuda") for dy, x, _g, _b, S in ops_]
        bs = [torch.empty(S, dy.shape[1], device="cuda") if b is not None else None for dy, _x, _g, b, S in ops_]
        Pg = [torch.empty(Sg, dy.shape[1], x.shape[1], device="cuda") for dy, x, _g, _b, _S in ops_]
        bg = [torch.empty(Sg, dy.shape[1], device="cuda") if b is not None else None for dy, _x, _g, b, _S in ops_]

        def sep_gemm():
            for (dy, x, _g, b, S), P, bP in zip(ops_, Ps, bs):
                C.gemm_tn2_bias(dy, x, P, S, False, bP) if b is not None else C.gemm_tn2(dy, x, P, S, False)

        def sep_reduce():
            for (_dy, _x, gr, b, _S), P, bP in zip(ops_, Ps, bs):
                C.splitk_reduce2(P, gr, bP, b, True) if b is not None else C.splitk_reduce(P, gr, True)

        def grp_gemm():
            assert C.gemm_tn_group([o[0] for o in ops_], [o[1] for o in ops_], Pg, bg, Sg)

        red_p = Pg + [b for b in bg if b is not None]
        red_g = [o[2] for o in ops_] + [o[3] for o in ops_ if o[3] is not None]

        def grp_reduce():
            C.splitk_reduce_group(red_p, red_g, True)

        def both(a, b):
            return lambda: (a(), b())

        row = {"pair": name, "tokens": T, "separate_splits": [o[4] for o in ops_], "group_splits": Sg}
        # interleaved: separate, grouped, separate, grouped
        for rnd in range(2):
            row[f"separate_gemm_us_{rnd}"] = round(timeit(sep_gemm), 1)
            row[f"group_gemm_us_{rnd}"] = round(timeit(grp_gemm), 1)
            row[f"separate_reduce_us_{rnd}"] = round(timeit(sep_reduce), 1)
            row[f"group_reduce_us_{rnd}"] = round(timeit(grp_reduce), 1)
            row[f"separate_total_us_{rnd}"] = round(timeit(both(sep_gemm, sep_reduce)), 1)
            row[f"group_total_us_{rnd}"] = round(timeit(both(grp_gemm, grp_reduce)), 1)
        for o in ops_:
            o[2].zero_()
        grp_gemm()
        grp_reduce()
        errs = []
        for dy, x, gr, _b, _S in ops_:
            ref = dy.float().t() @ x.float()
            errs.append(float(f"{((gr.float() - ref).norm() / ref.norm()).item():.1e}"))
        row["group_relerr"] = errs
        print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=32768)
    ap.add_argument("--group", action="store_true",
                    help="time each BERT-large pair grouped (one launch + one reduce) against the two separate calls")
    a = ap.parse_args()
    from cloudtik_amd import ops
    from cloudtik_amd.ops.linear import splitk_factor, tn2_splits
    C = ops.require_native()
    T = a.tokens
    if a.group:
        group_mode(C, T)
        return
    g = torch.Generator(device="cuda").manual_seed(0)
    for name, N, K in [("qkv", 3072, 1024), ("proj", 1024, 1024), ("ffn1", 4096, 1024), ("ffn2", 1024, 4096)]:
        dy = torch.randn(T, N, device="cuda", generator=g).to(torch.bfloat16)
        x = torch.randn(T, K, device="cuda", generator=g).to(torch.bfloat16)
        ref = dy.float().t() @ x.float()
        fl = 2 * T * N * K
        row = {"case": name, "N": N, "K": K}
        row["tn2_splits_chosen"] = tn2_splits(T, N, K)
        for S in sorted({splitk_factor(T, N, K), tn2_splits(T, N, K), 2, 4, 5, 6, 8, 16}):
            if T // 64 < S:
                continue
            P = torch.empty(S, N, K, device="cuda")
            t_gemm = timeit(lambda: C.gemm_tn2(dy, x, P, S, False))
            gr = torch.zeros(N, K, device="cuda", dtype=torch.bfloat16)
            C.gemm_tn2(dy, x, P, S, False)
            C.splitk_reduce(P, gr, True)
            err = ((gr.float() - ref).norm() / ref.norm()).item()
            t_red = timeit(lambda: C.splitk_reduce(P, gr, True))
            row[f"tn2_S{S}_us"] = round(t_gemm, 1)
            row[f"tn2_S{S}_tflops"] = round(fl / t_gemm / 1e6)
            row[f"reduce_S{S}_us"] = round(t_red, 1)
            row[f"tn2_S{S}_relerr"] = float(f"{err:.1e}")
        S = splitk_factor(T, N, K)
        t_bmm = timeit(lambda: torch.bmm(dy.view(S, T // S, N).transpose(1, 2), x.view(S, T // S, K),
                                         out_dtype=torch.float32))
        row["hipblaslt_bmm_S"] = S
        row["hipblaslt_bmm_us"] = round(t_bmm, 1)
        row["hipblaslt_bmm_tflops"] = round(fl / t_bmm / 1e6)
        gr = torch.zeros(N, K, device="cuda", dtype=torch.bfloat16)
        t_acc = timeit(lambda: gr.addmm_(dy.t(), x))
        row["hipblaslt_addmm_us"] = round(t_acc, 1)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
