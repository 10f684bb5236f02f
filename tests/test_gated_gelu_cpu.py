"""``ops.gated_gelu`` on the CPU: the reference against an fp64 evaluation, its dropout mask against
``ref.dropout_keep_mask``, and its autograd against ``gradcheck``."""
import math

import pytest
import torch

from cloudtik_amd import ops
from cloudtik_amd.ops import reference as ref

C = math.sqrt(2.0 / math.pi)


def gated_gelu_fp64(g, u):
    """gelu_tanh(g) * u in fp64, from the tanh form of the definition."""
    g, u = g.double(), u.double()
    return 0.5 * g * (1.0 + torch.tanh(C * (g + 0.044715 * g ** 3))) * u


def _inputs(shape, seed, dtype):
    gen = torch.Generator().manual_seed(seed)
    g = torch.randn(shape, generator=gen) * 2
    u = torch.randn(shape, generator=gen) * 2
    flat = g.view(-1)
    tail = torch.tensor([-9.0, -6.5, -4.0, 4.0, 7.25, 9.0])
    flat[:min(6, flat.numel())] = tail[:min(6, flat.numel())]
    return g.to(dtype), u.to(dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64, torch.bfloat16])
def test_reference_against_fp64(dtype):
    g, u = _inputs((5, 24), 0, dtype)
    got = ref.gated_gelu(g, u)
    assert got.dtype == dtype and got.shape == g.shape
    want = gated_gelu_fp64(g, u)
    # the input dtype rounds the activation and the product once each; fp32's 1 + tanh cancels in the
    # negative tail, which costs eps * |g u| absolute
    eps = {torch.float32: 2.0 ** -23, torch.float64: 2.0 ** -52, torch.bfloat16: 2.0 ** -7}[dtype]
    tol = 2 * eps * want.abs() + 2 * eps * (g.double() * u.double()).abs()
    assert bool(((got.double() - want).abs() <= tol).all())
    assert torch.equal(ops.gated_gelu(g, u), got)              # the CPU dispatch is the reference
    assert torch.equal(ops.gated_gelu(g, u, 0.3, training=False), got)


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_dropout_mask_is_the_hash_mask(p):
    g, u = _inputs((3, 7, 16), 1, torch.float32)
    ops.manual_seed(77)
    ops.dropout(torch.ones(8), 0.5)                             # move the offset off zero
    state = ops.rng_state()
    got = ops.gated_gelu(g, u, p)
    keep = ref.dropout_keep_mask(g.numel(), p, state["seed"], state["offset"]).view(g.shape)
    assert 0 < int(keep.sum()) < keep.numel()
    plain = ref.gated_gelu(g, u)
    assert torch.equal(got, torch.where(keep, plain * (1.0 / (1.0 - p)), torch.zeros_like(plain)))
    assert ops.rng_state()["offset"] == state["offset"] + g.numel() // 8
    # the mask ops.dropout draws for a tensor of this shape at the same (seed, offset)
    ops.set_rng_state(state)
    assert torch.equal(ops.dropout(torch.ones_like(g), p) != 0, keep)
    # the same state gives the same bits, the next call another mask
    ops.set_rng_state(state)
    again, other = ops.gated_gelu(g, u, p), ops.gated_gelu(g, u, p)
    assert torch.equal(again, got) and not torch.equal(other != 0, got != 0)


def test_reference_autograd():
    g, u = _inputs((2, 8), 2, torch.float64)
    g.requires_grad_(True)
    u.requires_grad_(True)
    assert torch.autograd.gradcheck(lambda a, b: ref.gated_gelu(a, b), (g, u))
    ops.manual_seed(5)
    state = ops.rng_state()

    def dropped(a, b):                                          # one fixed mask for every evaluation
        return ref.gated_gelu(a, b, 0.5, state["seed"], state["offset"])

    assert torch.autograd.gradcheck(dropped, (g, u))


def test_argument_checks():
    g = torch.zeros(2, 8)
    with pytest.raises(ValueError, match="agree"):
        ops.gated_gelu(g, torch.zeros(2, 16))
    with pytest.raises(ValueError, match="p must be"):
        ops.gated_gelu(g, g, 1.0)
