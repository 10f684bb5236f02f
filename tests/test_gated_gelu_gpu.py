"""``ops.gated_gelu`` on the GPU (csrc/gated_act.hip): h, dg and du per element against fp64 computed
from the same bf16 inputs, on shapes that each exercise another part of the grid; the dropout mask
against ``ref.dropout_keep_mask``; the refusals; graph capture.

TOLERANCE, per element: one bf16 ulp of the reference value, 2^-8 |ref| (the single rounding at the
store, a whole ulp so that an fp32 error which flips the rounding is allowed), plus 2^-20 of the
product of the inputs that the value is linear in (|g u| for h, |dh u| for dg, |dh g| for du, times
the keep scale): the absolute error fp32 arithmetic leaves where the terms of the value cancel.  The
kernel's sigmoid form (one exp, one rcp on |z|) has no cancellation in either tail, so nothing wider
is needed."""
import math

import pytest
import torch

from cloudtik_amd import ops
from cloudtik_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
C = math.sqrt(2.0 / math.pi)

# [1, 8]: one vector; [3, 64]: fewer rows than a row step; [5, 2816]: 352 vectors = 5.5 column blocks
# of 64; [257, 1024]: a row tail against 4 waves x 4 rows (forward) and 4 x 2 (backward); [2, 7, 64]: 3-D
SHAPES = [(1, 8), (3, 64), (5, 2816), (257, 1024), (2, 7, 64)]


def _fp64(g, u, dh=None, keep=None, p=0.0):
    """h, and with ``dh`` also dg and du, in fp64.  0.5 (1 + tanh z) = sigmoid(2 z) and its complement
    sigmoid(-2 z) are evaluated as such, so the reference keeps its relative accuracy in both tails
    (fp64's own 1 + tanh z is exactly 0 below g = -4.4)."""
    g, u = g.double().cpu(), u.double().cpu()
    s = 1.0 / (1.0 - p)
    k = torch.ones_like(g) if keep is None else keep.view(g.shape).double()
    z2 = 2.0 * C * (g + 0.044715 * g ** 3)
    sig, oms = torch.sigmoid(z2), torch.sigmoid(-z2)
    gelu = g * sig
    h = gelu * u * k * s
    if dh is None:
        return h
    dgelu = sig + g * sig * oms * 2.0 * C * (1.0 + 3 * 0.044715 * g * g)
    d = dh.double().cpu() * k * s
    return h, d * u * dgelu, d * gelu


def _inputs(shape, seed):
    gen = torch.Generator().manual_seed(seed)
    g = torch.randn(shape, generator=gen) * 2
    u = torch.randn(shape, generator=gen) * 2
    dh = torch.randn(shape, generator=gen)
    flat, n = g.view(-1), g.numel()
    tail = torch.tensor([-9.0, -6.5, -4.0, 4.0, 7.25, 9.0, -5.0, 8.0])
    flat[torch.arange(8) * (n // 8)] = tail                    # planted over the whole tensor
    return g.to(BF), u.to(BF), dh.to(BF)


def _close(got, want, lin, what):
    tol = 2.0 ** -8 * want.abs() + 2.0 ** -20 * lin.abs()
    err = (got.double().cpu() - want).abs()
    bad = err > tol
    assert not bool(bad.any()), (what, int(bad.sum()), float((err / tol.clamp_min(1e-300)).max()))


def _check(g, u, dh, p, cuda):
    """Forward and backward of (g, u) on the GPU at dropout ``p`` against fp64; returns h."""
    gg, ug = g.detach().requires_grad_(True), u.detach().requires_grad_(True)
    state = ops.rng_state()
    h = ops.gated_gelu(gg, ug, p)
    assert h.shape == g.shape and h.dtype == BF and h.is_contiguous()
    keep = ref.dropout_keep_mask(g.numel(), p, state["seed"], state["offset"]) if p > 0 else None
    dg, du = torch.autograd.grad(h, (gg, ug), dh)
    assert dg.shape == g.shape and du.shape == g.shape
    want_h, want_dg, want_du = _fp64(g, u, dh, keep, p)
    s = 1.0 / (1.0 - p)
    g64, u64, d64 = g.double().cpu(), u.double().cpu(), dh.double().cpu()
    _close(h, want_h, s * g64 * u64, "h")
    _close(dg, want_dg, s * d64 * u64, "dg")
    _close(du, want_du, s * d64 * g64, "du")
    if keep is not None:
        k = keep.view(g.shape)
        assert 0 < int(k.sum()) < k.numel()
        # where no factor is zero; below g = -10 the sigmoid itself underflows fp32
        live = (d64 != 0) & (u64 != 0) & (g64 != 0) & (g64 > -9.5)
        assert torch.equal((dg.cpu() == 0) & live, ~k & live)   # backward zeros: exactly the dropped
        assert torch.equal((du.cpu() == 0) & live, ~k & live)
        assert bool((h.cpu()[~k] == 0).all())
    return h


@pytest.mark.parametrize("p", [0.0, 0.1, 0.5])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_against_fp64(cuda, shape, p):
    g, u, dh = (t.to(cuda) for t in _inputs(shape, sum(shape)))
    ops.manual_seed(1234)
    ops.dropout(torch.ones(64, device=cuda, dtype=BF), 0.5)     # a non-zero offset
    _check(g, u, dh, p, cuda)


@pytest.mark.parametrize("p", [0.0, 0.1])
def test_strided_halves_of_a_stacked_tensor(cuda, p):
    """The halves of a [33, 2 * 256] tensor: row stride 2 F, the second base offset by F; no copy is
    made and the result is that of the contiguous halves, bit for bit."""
    F = 256
    g, u, dh = _inputs((33, F), 9)
    stacked = torch.cat([g, u], 1).to(cuda)
    gs, us = stacked.split(F, -1)
    assert not gs.is_contiguous() and us.data_ptr() == stacked.data_ptr() + 2 * F
    ops.manual_seed(7)
    h = _check(gs, us, dh.to(cuda), p, cuda)
    ops.manual_seed(7)
    assert torch.equal(h, ops.gated_gelu(g.to(cuda), u.to(cuda), p))
    # gradients reach the stacked tensor through the split
    st = stacked.clone().requires_grad_(True)
    a, b = st.split(F, -1)
    ops.gated_gelu(a, b).sum().backward()
    assert st.grad.shape == stacked.shape and bool((st.grad[:, F:] != 0).any())


def test_dropout_is_seeded(cuda):
    g, u, _ = (t.to(cuda) for t in _inputs((5, 2816), 3))
    ops.manual_seed(99)
    a, b = ops.gated_gelu(g, u, 0.5), ops.gated_gelu(g, u, 0.5)
    ops.manual_seed(99)
    c = ops.gated_gelu(g, u, 0.5)
    assert torch.equal(a, c)
    assert not torch.equal(a == 0, b == 0)                      # the next call draws another mask
    assert torch.equal(ops.gated_gelu(g, u, 0.5, training=False), ops.gated_gelu(g, u))


def test_saves_the_inputs_only(cuda):
    g, u, _ = (t.to(cuda).requires_grad_(True) for t in _inputs((3, 64), 4))
    saved = []
    with torch.autograd.graph.saved_tensors_hooks(lambda t: saved.append(t) or t, lambda t: t):
        ops.gated_gelu(g, u, 0.1)
    assert sorted(t.data_ptr() for t in saved) == sorted((g.data_ptr(), u.data_ptr()))


def test_refusals(cuda):
    ok = torch.zeros(4, 16, device=cuda, dtype=BF)
    ops.gated_gelu(ok, ok)
    with pytest.raises(ValueError, match="bf16"):
        ops.gated_gelu(ok.float(), ok.float())
    with pytest.raises(ValueError, match="multiple of 8"):
        ops.gated_gelu(ok[:, :12].contiguous(), ok[:, :12].contiguous())
    raw = torch.zeros(4 * 16 + 8, device=cuda, dtype=BF)
    off = raw[1:1 + 4 * 16].view(4, 16)                         # base 2 bytes past a 16-byte boundary
    with pytest.raises(ValueError, match="16-byte"):
        ops.gated_gelu(off, ok)
    with pytest.raises(ValueError, match="16-byte"):
        ops.gated_gelu(ok, off)
    # the binding checks on its own: nothing misaligned, strided by odd rows or of another dtype launches
    Cx = ops.require_native()
    with pytest.raises(RuntimeError, match="16-byte-aligned"):
        Cx.gated_gelu_fwd(off, ok, 0.0, 0, 0)
    with pytest.raises(RuntimeError, match="bf16"):
        Cx.gated_gelu_fwd(ok.float(), ok.float(), 0.0, 0, 0)
    with pytest.raises(RuntimeError, match="multiple of 8"):
        Cx.gated_gelu_fwd(ok[:, :12], ok[:, :12], 0.0, 0, 0)
    with pytest.raises(RuntimeError, match="row stride"):
        Cx.gated_gelu_fwd(torch.zeros(4, 20, device=cuda, dtype=BF)[:, :16], ok, 0.0, 0, 0)


def test_graph_capture(cuda):
    g, u, _ = (t.to(cuda) for t in _inputs((257, 1024), 6))
    want = ops.gated_gelu(g, u)
    out = torch.zeros_like(want)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        out.copy_(ops.gated_gelu(g, u))
    torch.cuda.current_stream().wait_stream(side)
    out.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out.copy_(ops.gated_gelu(g, u))
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, want)
