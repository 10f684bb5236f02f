"""ops.attention_relbias on the CPU (the PyTorch reference every call the kernels cannot take goes
to): dropout on the kernels' stream, gradients for q, k, v and the bias vector, and p = 0 unchanged."""
import torch

from cloudtik_amd import ops
from cloudtik_amd.ops import reference as ref

B, H, SQ, SK, D = 2, 3, 20, 26, 16
REL_BASE, L = SQ + 1, SQ + SK + 3          # two spare offsets on each side
SCALE = 0.3
SEED = 5


def _inputs(dtype=torch.float32):
    g = torch.Generator().manual_seed(3)
    q = torch.randn(B, SQ, H, D, generator=g).to(dtype)
    k = torch.randn(B, SK, H, D, generator=g).to(dtype)
    v = torch.randn(B, SK, H, D, generator=g).to(dtype)
    rel = (torch.randn(H, L, generator=g) * 0.5).to(dtype)
    kb = torch.randn(B, SK, generator=g) * 0.5
    kb[1, SK - 5:] = -10000.0
    do = torch.randn(B, SQ, H, D, generator=g).to(dtype)
    return q, k, v, rel, kb, do


def _independent64(q, k, v, rel, kb, causal, keep, p):
    """An fp64 computation that shares no code with the front end: explicit loops over the bias."""
    q, k, v, rel = (t.double() for t in (q, k, v, rel))
    s = torch.empty(B, H, SQ, SK, dtype=torch.float64)
    for i in range(SQ):
        for j in range(SK):
            s[:, :, i, j] = (q[:, i] * k[:, j]).sum(-1) * SCALE + rel[:, j - i + REL_BASE][None] + kb[:, j, None].double()
            if causal and j > i:
                s[:, :, i, j] = float("-inf")
    pr = torch.softmax(s, -1)
    if keep is not None:
        pr = pr * keep.double() / (1.0 - p)
    return torch.einsum("bhqk,bkhd->bqhd", pr, v)


def _stream(p):
    ops.manual_seed(SEED)
    seed, off = ops._rng.next(B * H * SQ * SK)
    return ref.attn_dropout_keep(B, H, SQ, SK, p, seed, off)


def test_dropout_uses_the_kernels_stream():
    q, k, v, rel, kb, _ = _inputs()
    for causal in (False, True):
        keep = _stream(0.1)
        ops.manual_seed(SEED)
        got = ops.attention_relbias(q, k, v, rel, REL_BASE, kb, scale=SCALE, causal=causal, p=0.1)
        want = _independent64(q, k, v, rel, kb, causal, keep, 0.1)
        assert got.dtype == torch.float32
        # fp32 against fp64: a few ulps of sums of <= 26 products of O(1) numbers
        assert (got.double() - want).abs().max() <= 1e-5 * want.abs().max()
        dropped = _independent64(q, k, v, rel, kb, causal, None, 0.0)
        assert (want - dropped).abs().max() > 1e-2 * want.abs().max()      # the mask matters


def test_gradients_match_fp64_autograd():
    q, k, v, rel, kb, do = _inputs()
    keep = _stream(0.1)
    leaves = [t.clone().requires_grad_() for t in (q, k, v, rel)]
    ops.manual_seed(SEED)
    ops.attention_relbias(*leaves, REL_BASE, kb, scale=SCALE, causal=True, p=0.1).backward(do)
    leaves64 = [t.double().requires_grad_() for t in (q, k, v, rel)]
    _independent64(*leaves64, kb, True, keep, 0.1).backward(do.double())
    for name, a, b in zip("q k v rel".split(), leaves, leaves64):
        assert a.grad is not None and a.grad.shape == a.shape, name
        assert (a.grad.double() - b.grad).abs().max() <= 1e-5 * b.grad.abs().max(), name
    # the gradient comes back in the layout of the bias that was passed: a transposed view
    relt = rel.t().contiguous().t().requires_grad_()
    ops.manual_seed(SEED)
    ops.attention_relbias(q, k, v, relt, REL_BASE, kb, scale=SCALE, causal=True, p=0.1).backward(do)
    assert torch.allclose(relt.grad, leaves[3].grad, rtol=1e-6, atol=1e-7)
    # spare offsets get no gradient
    assert (leaves[3].grad[:, :REL_BASE - SQ + 1] == 0).all() and (leaves[3].grad[:, REL_BASE + SK:] == 0).all()


def test_p0_is_the_former_fallback_bit_for_bit():
    for dtype in (torch.float32, torch.bfloat16):
        q, k, v, rel, kb, _ = _inputs(dtype)
        for causal in (False, True):
            got = ops.attention_relbias(q, k, v, rel, REL_BASE, kb, scale=SCALE, causal=causal, p=0.0)
            idx = torch.arange(SK)[None, :] - torch.arange(SQ)[:, None] + REL_BASE
            bias = rel.float()[:, idx.clamp(0, L - 1)][None] + kb.float()[:, None, None, :]
            s = torch.einsum("bqhd,bkhd->bhqk", q.float(), k.float()) * SCALE + bias
            if causal:
                s = s.masked_fill(torch.ones(SQ, SK, dtype=torch.bool).triu(1), float("-inf"))
            want = torch.einsum("bhqk,bkhd->bqhd", torch.softmax(s, -1), v.float()).to(dtype)
            assert torch.equal(got, want)
            assert torch.equal(got, ops.attention_relbias(q, k, v, rel, REL_BASE, kb, scale=SCALE, causal=causal))
