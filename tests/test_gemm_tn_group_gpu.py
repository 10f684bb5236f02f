"""Grouped weight-gradient GEMM (csrc/gemm_nt.hip ct_gemm_tn_group): several TN problems that
share the token count K and one slice count in one launch, their fp32 slabs and bias partials
against fp32 PyTorch references per slice; the grouped split-K reduce (csrc/elementwise.hip
ct_splitk_reduce_group); and ``wgrad_accumulate_group`` against the per-problem path.

Operands are drawn as in test_gemm_nt_gpu.py (B scaled by K ** -0.5) and the slab tolerances
are that file's for gemm_tn2: rtol 2e-3, atol 2e-3 * max |ref|; bias partials rtol 1e-3,
atol 1e-2.  Slabs and partials are NaN-filled before every call, so an unwritten tile shows."""
import pytest
import torch

pytestmark = pytest.mark.gpu

NAN = float("nan")


def _C():
    from cloudtik_amd import ops
    return ops.require_native()


def _rand(*shape, scale=1.0, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.randn(*shape, device="cuda", generator=g) * scale).to(torch.bfloat16)


def _split_ranges(K, S):
    """K range of each slice: the K / 64 K-tiles dealt out, the first (K / 64) % S slices one
    K-tile longer."""
    q, r = divmod(K // 64, S)
    out, k = [], 0
    for s in range(S):
        n = (q + (1 if s < r else 0)) * 64
        out.append((k, k + n))
        k += n
    return out


def _problems(shapes, K, seed=0):
    """[(A [K, M], B [K, N])] for shapes [(M, N)]."""
    return [(_rand(K, M, seed=seed + 10 * i + 1), _rand(K, N, seed=seed + 10 * i + 2, scale=K ** -0.5))
            for i, (M, N) in enumerate(shapes)]


def _run_group(probs, S, bias):
    """Calls gemm_tn_group on NaN-filled outputs; returns (ok, slabs, bias partials)."""
    P = [torch.full((S, A.shape[1], B.shape[1]), NAN, device="cuda") for A, B in probs]
    bP = [torch.full((S, A.shape[1]), NAN, device="cuda") if b else None for (A, _), b in zip(probs, bias)]
    ok = _C().gemm_tn_group([A for A, _ in probs], [B for _, B in probs], P, bP, S)
    return ok, P, bP


def _check_group(probs, S, bias, K):
    ok, P, bP = _run_group(probs, S, bias)
    assert ok
    ranges = _split_ranges(K, S)
    for (A, B), p, bp in zip(probs, P, bP):
        ref = A.float().t() @ B.float()
        atol = 2e-3 * ref.abs().max().item()
        torch.testing.assert_close(p.sum(0), ref, rtol=2e-3, atol=atol)
        for s_, (k0, k1) in enumerate(ranges):          # each slab is its own K range
            torch.testing.assert_close(p[s_], A[k0:k1].float().t() @ B[k0:k1].float(), rtol=2e-3, atol=atol)
        if bp is not None:
            want = torch.stack([A[k0:k1].float().sum(0) for k0, k1 in ranges])
            torch.testing.assert_close(bp, want, rtol=1e-3, atol=1e-2)
    return P, bP


def test_two_shapes_one_ktile_per_slice():
    K, S = 128, 2
    _check_group(_problems([(256, 256), (512, 256)], K), S, [False, False], K)


def test_nine_workgroups_uneven_slices():
    """1 + 2 tiles, 3 slices of 2 / 2 / 1 K-tiles: 9 workgroups, not a multiple of the 8 XCDs."""
    K, S = 320, 3
    _check_group(_problems([(256, 256), (256, 512)], K, seed=3), S, [False, False], K)


@pytest.mark.parametrize("bias", [(True, False), (False, True), (True, True), (False, False)])
def test_bias_per_problem(bias):
    """The biased problems have N = 512 (two column tiles), so only their tn == 0 tiles sum."""
    K, S = 256, 2
    _check_group(_problems([(256, 512), (512, 512)], K, seed=5), S, list(bias), K)


def test_column_slice_operand():
    """A is a column slice of a wider tensor (lda > M), B likewise."""
    K, S = 192, 3
    wideA, wideB = _rand(K, 640, seed=31), _rand(K, 768, seed=32, scale=K ** -0.5)
    probs = [(wideA[:, 128:384], _rand(K, 256, seed=33, scale=K ** -0.5)),
             (_rand(K, 256, seed=34), wideB[:, 256:768])]
    _check_group(probs, S, [True, False], K)


def test_four_problems():
    K, S = 192, 2
    _check_group(_problems([(256, 256), (512, 256), (256, 768), (768, 512)], K, seed=7), S,
                 [False, True, False, True], K)


def test_bert_width_pair():
    """Wo (1024 x 1024) + Wqkv (3072 x 1024) at reduced tokens, bias on the second; two runs are
    bitwise equal."""
    K, S = 2048, 4
    probs = _problems([(1024, 1024), (3072, 1024)], K, seed=9)
    P, bP = _check_group(probs, S, [False, True], K)
    ok, P2, bP2 = _run_group(probs, S, [False, True])
    assert ok
    for a, b in zip(P + [bP[1]], P2 + [bP2[1]]):
        assert torch.equal(a, b)


def test_refusals_leave_outputs_untouched():
    C = _C()

    def refused(As, Bs, S, shapes=None):
        shapes = shapes or [(A.shape[1], B.shape[1]) for A, B in zip(As, Bs)]
        P = [torch.full((S, M, N), NAN, device="cuda") for M, N in shapes]
        bP = [torch.full((S, M), NAN, device="cuda") for M, _ in shapes]
        assert not C.gemm_tn_group(As, Bs, P, bP, S)
        torch.cuda.synchronize()
        assert all(t.isnan().all() for t in P + bP)

    K = 128
    A, B = _rand(K, 256, seed=41), _rand(K, 256, seed=42)
    refused([A] * 5, [B] * 5, 2)                                          # more than 4 problems
    refused([A, _rand(K, 128, seed=43)], [B, B], 2)                       # M % 256
    refused([A, A], [B, _rand(K, 384, seed=44)], 2)                       # N % 256
    refused([_rand(96, 256, seed=45)] * 2, [_rand(96, 256, seed=46)] * 2, 2)   # K % 64
    refused([A, A], [B, B], 3)                                            # K / 64 = 2 < splits
    refused([A, A], [B, B], 1)                                            # splits < 2
    flat = _rand(K * 256 + 8, seed=47)
    refused([A, flat[4:4 + K * 256].view(K, 256)], [B, B], 2)             # pointer not 16-byte aligned
    wide = _rand(K, 260, seed=48)
    refused([A, A], [B, wide[:, :256]], 2)                                # leading dimension % 8


def _ascending_sum(P, g0):
    """bf16(g0 + P[0] + P[1] + ...): P.sum(0) in fp32 with the slice order pinned to ascending,
    as the kernel sums (so the comparison is exact)."""
    acc = g0.float().clone() if g0 is not None else torch.zeros_like(P[0])
    for s_ in range(P.shape[0]):
        acc += P[s_]
    return acc.to(torch.bfloat16)


@pytest.mark.parametrize("count", [3, 4])
@pytest.mark.parametrize("accumulate", [False, True])
def test_splitk_reduce_group_exact(count, accumulate):
    C = _C()
    dims = [(4, 256, 512), (2, 256), (3, 512, 256), (5, 1024)][:count]     # (S, *shape of g)
    gen = torch.Generator(device="cuda").manual_seed(count)
    Ps = [torch.randn(*d, device="cuda", generator=gen) for d in dims]
    g0 = [_rand(*d[1:], seed=50 + i) for i, d in enumerate(dims)]
    gs = [g.clone() for g in g0]
    C.splitk_reduce_group(Ps, gs, accumulate)
    for P, g, base in zip(Ps, gs, g0):
        assert torch.equal(g, _ascending_sum(P, base if accumulate else None))


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("numel", [8, 8 * 257])         # one vector; one vector past a full workgroup
@pytest.mark.parametrize("S", [1, 3, 4, 5])             # around the slice loop's unroll of 4
def test_reduce_kernels_agree_bit_for_bit(S, numel, accumulate):
    """splitk_reduce, splitk_reduce2 (as either half), splitk_reduce_group (as any entry) and
    splitk_reduce_clear on one (P, g): each equals the ascending-order fp32 sum exactly, and the
    clear form leaves P all zero."""
    C = _C()
    gen = torch.Generator(device="cuda").manual_seed(100 * S + numel)
    P = torch.randn(S, numel, device="cuda", generator=gen)
    g0 = _rand(numel, seed=70 + S)
    want = _ascending_sum(P, g0 if accumulate else None)
    other_P = torch.randn(2, 16, device="cuda", generator=gen)      # the launch's other entries
    fresh = lambda: (g0.clone(), _rand(16, seed=71))

    g, _ = fresh()
    C.splitk_reduce(P, g, accumulate)
    assert torch.equal(g, want)
    for first in (True, False):
        g, o = fresh()
        C.splitk_reduce2(*((P, g, other_P, o) if first else (other_P, o, P, g)), accumulate)
        assert torch.equal(g, want)
    for slot in range(4):
        g, _ = fresh()
        Ps, gs = [other_P.clone() for _ in range(4)], [fresh()[1] for _ in range(4)]
        Ps[slot], gs[slot] = P, g
        C.splitk_reduce_group(Ps, gs, accumulate)
        assert torch.equal(g, want)
    g, _ = fresh()
    Pc = P.clone()
    C.splitk_reduce_clear(Pc, g, accumulate)
    assert torch.equal(g, want)
    assert Pc.count_nonzero().item() == 0


def test_wgrad_accumulate_group_matches_separate_calls():
    """The grouped accumulate and the two per-problem calls are both within the slab tolerance
    of the fp32 reference (not bitwise equal: the partial counts differ); the grouped call is
    bitwise reproducible."""
    from cloudtik_amd.ops.linear import tn2_group_splits, wgrad_accumulate, wgrad_accumulate_group
    T = 2048
    dy_a, x_a = _rand(T, 256, seed=61), _rand(T, 256, seed=62, scale=T ** -0.5)
    dy_b, x_b = _rand(T, 512, seed=63), _rand(T, 256, seed=64, scale=T ** -0.5)
    assert tn2_group_splits(T, [(256, 256), (512, 256)]) >= 2            # the grouped path runs
    base = [_rand(256, 256, seed=65), _rand(512, 256, seed=66), _rand(512, seed=67)]

    def grouped():
        g = [t.clone() for t in base]
        wgrad_accumulate_group([(g[0], dy_a, x_a, None), (g[1], dy_b, x_b, g[2])])
        return g

    g1, g2 = grouped(), grouped()
    sep = [t.clone() for t in base]
    wgrad_accumulate(sep[0], dy_a, x_a)
    wgrad_accumulate(sep[1], dy_b, x_b, sep[2])
    refs = [base[0].float() + dy_a.float().t() @ x_a.float(), base[1].float() + dy_b.float().t() @ x_b.float(),
            base[2].float() + dy_b.float().sum(0)]
    # the outputs are bf16: one rounding of the fp32 sum, at most half an ulp = 2 ** -8 relative,
    # on top of the fp32 tolerances (slabs: 2e-3, 2e-3 * max |ref|; bias partials: 1e-3, 1e-2)
    tols = [dict(rtol=2e-3 + 2 ** -8, atol=2e-3 * refs[0].abs().max().item()),
            dict(rtol=2e-3 + 2 ** -8, atol=2e-3 * refs[1].abs().max().item()),
            dict(rtol=1e-3 + 2 ** -8, atol=1e-2)]
    for got, other, again, ref, tol in zip(g1, sep, g2, refs, tols):
        assert torch.equal(got, again)
        torch.testing.assert_close(got.float(), ref, **tol)
        torch.testing.assert_close(other.float(), ref, **tol)
