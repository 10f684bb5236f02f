"""Whole-step hipGraph capture (train/graph_step.py): a small ResNet trained through captured
replays follows the eager run step for step (weights, loss, BN running stats), with the
gradient side stream on; LAMB's per-step bias corrections reach the replays through the
optimizer's graph slot."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _setup(seed=0):
    from cloudtik_amd.models.resnet import ResNetTrainStep, resnet18_like_small
    from cloudtik_amd.train.optim import FlatParamSpace, FusedSGD
    torch.manual_seed(seed)
    m = resnet18_like_small(device="cuda")
    m.train()
    named = list(m.named_parameters())
    sp = FlatParamSpace([p for _, p in named], names=[n for n, _ in named])
    opt = FusedSGD(sp, lr=0.05, momentum=0.9, weight_decay=1e-4, space=sp)
    g = torch.Generator().manual_seed(3)
    dt = next(m.parameters()).dtype
    x = torch.randn(8, 3, 32, 32, generator=g).to("cuda", dt).contiguous(memory_format=torch.channels_last)
    y = torch.randint(0, 10, (8,), generator=g).cuda()
    return m, sp, opt, ResNetTrainStep(m, opt), x, y


def test_graphed_resnet_step_matches_eager():
    from cloudtik_amd.train.graph_step import GraphedStep
    m0, sp0, _, ts0, x, y = _setup()
    losses0 = [float(ts0(x, y).detach()) for _ in range(7)]
    m1, sp1, opt1, ts1, x1, y1 = _setup()
    step = GraphedStep(lambda: ts1(x1, y1), optimizers=[opt1], warmup=2)
    losses1 = [float(step().detach()) for _ in range(7)]
    assert step.graph is not None
    torch.testing.assert_close(torch.tensor(losses1), torch.tensor(losses0), rtol=2e-2, atol=2e-2)
    torch.testing.assert_close(sp1.model.float(), sp0.model.float(), rtol=5e-2, atol=5e-3)
    bn0 = [b for n, b in m0.named_buffers() if n.endswith("running_mean")]
    bn1 = [b for n, b in m1.named_buffers() if n.endswith("running_mean")]
    for a, b in zip(bn1, bn0):
        torch.testing.assert_close(a.float(), b.float(), rtol=5e-2, atol=5e-3)


def test_graph_slot_carries_per_step_bias_corrections():
    from cloudtik_amd.train.graph_step import GraphedStep
    from cloudtik_amd.train.optim import FlatParamSpace, FusedLAMB
    torch.manual_seed(1)
    w = torch.nn.Parameter(torch.randn(4096, device="cuda"))
    sp = FlatParamSpace([w], names=["w"])
    opt = FusedLAMB(sp, lr=1e-2, space=sp)
    target = torch.randn(4096, device="cuda")

    def body():
        loss = ((w - target) ** 2).sum()
        loss.backward()
        opt.step()
        opt.zero_grad()
        return loss

    w_ref = torch.nn.Parameter(w.detach().clone())
    sp_ref = FlatParamSpace([w_ref], names=["w"])
    opt_ref = FusedLAMB(sp_ref, lr=1e-2, space=sp_ref)
    for _ in range(8):
        ((w_ref - target) ** 2).sum().backward()
        opt_ref.step()
        opt_ref.zero_grad()
    step = GraphedStep(body, optimizers=[opt], warmup=2)
    for _ in range(8):
        step()
    torch.cuda.synchronize()
    assert opt.step_count == opt_ref.step_count == 8
    torch.testing.assert_close(w.detach(), w_ref.detach(), rtol=1e-5, atol=1e-6)


def _graphed_sgd_follows_fp64(dampening, warmup):
    """FusedSGD(momentum=0.9) on one 4096-element parameter for 4 steps under GraphedStep, a new
    gradient copied into the static buffer before every call; after each step the weights are
    compared with an fp64 SGD (PyTorch rule: buf = g on the first step, then
    buf = 0.9 buf + (1 - dampening) g; w -= lr buf).  Tolerance: 4 steps of fp32 rounding, one
    ulp (1.2e-7) of the value each: rtol 1e-6; where the terms cancel the error is an ulp of
    the terms, which stay below 8 (ulp 4.8e-7) here: atol 1e-6.  A momentum that is not
    accumulated is off by lr x 0.9 x |buf|, about 5e-2."""
    from cloudtik_amd.train.graph_step import GraphedStep
    from cloudtik_amd.train.optim import FlatParamSpace, FusedSGD
    n, lr, mom, steps = 4096, 0.05, 0.9, 4
    gen = torch.Generator().manual_seed(11)
    w0 = torch.randn(n, generator=gen)
    grads = [torch.randn(n, generator=gen) for _ in range(steps)]
    w = torch.nn.Parameter(w0.clone().cuda())
    sp = FlatParamSpace([w], names=["w"])
    opt = FusedSGD(sp, lr=lr, momentum=mom, dampening=dampening, space=sp)
    step = GraphedStep(opt.step, optimizers=[opt], warmup=warmup)
    ref, buf = w0.double(), None
    for i, g in enumerate(grads):
        sp.grad[:n].copy_(g.cuda())
        step()
        torch.cuda.synchronize()
        g = g.double()
        buf = g.clone() if buf is None else mom * buf + (1 - dampening) * g
        ref = ref - lr * buf
        torch.testing.assert_close(w.detach().double().cpu(), ref, rtol=1e-6, atol=1e-6,
                                   msg=lambda m: "step %d: %s" % (i + 1, m))
        torch.testing.assert_close(opt.momentum_buffer[:n].double().cpu(), buf, rtol=1e-6, atol=1e-6,
                                   msg=lambda m: "momentum buffer, step %d: %s" % (i + 1, m))
    assert step.graph is not None and opt.step_count == steps


def test_graphed_sgd_captured_at_first_step_accumulates_momentum():
    """warmup=0 captures at step_count == 1: the first-step rule (buf = g) must hold for the
    first replay only, so the flag may not be a captured kernel argument."""
    _graphed_sgd_follows_fp64(dampening=0.0, warmup=0)


def test_graphed_sgd_with_dampening_after_warmup():
    _graphed_sgd_follows_fp64(dampening=0.3, warmup=2)
