"""Head-dim-128 attention for training (ops/csrc/attention_d128_train.h): the forward with dropout
and lse, and the backward with dQ, dK, dV and the gradient of the bias vector, through the
relative-bias pair (attn_fwd_relbias_train / attn_bwd_relbias) and the plain pair
(attn_fwd_train / attn_bwd_train), on every dispatch path and edge.

Method of tests/test_attention_relbias_bwd_gpu.py (read its docstring first); what does not depend
on the head dim is imported from it, the rest has a D = 128 copy here.  Every case compares the
HIP kernels with an fp64 autograd reference computed from the same bf16 inputs (``_ref64``), in
which the bias vector ``rel`` is a leaf, so ``rel.grad`` is the wanted ``d_rel``; a case without a
bias vector uses the same reference with ``rel`` = 0 and has no ``d_rel``.

* ``o``, ``dq``, ``dk``, ``dv``: per (batch, head, row), max |kernel - ref| over the 128 columns /
  (max |ref| over that row + 1e-3 x the tensor's max |ref|); ``lse``: absolute, log2 units.
* ``d_rel``, per (head, offset i): |kernel - ref| / (A[h, i] + 1e-3 x max_i A[h, .]) with
  A[h, i] = the sum of |dS_ref| over the diagonal key - query + rel_base = i and all batches.

BOUNDS.  Not taken from the kernel.  ``_model`` (imported) is the rounding model: fp32 scores in
the log2 domain, P and dS rounded to bf16 before their MFMAs, delta from the bf16 O, bf16 outputs,
``d_rel`` summed in fp32 from the unrounded dS.  Its worst figures against ``_ref64`` at D = 128
over the whole case matrix below (measured on a CPU: ``model_table()``), and the bounds, 4 x each
(the factor of both existing attention test files):

    | quantity                                              | model worst | bound (4 x) |
    |-------------------------------------------------------|-------------|-------------|
    | o                                                     | 6.17e-03    | 2.47e-02    |
    | lse (absolute, log2 units)                            | 8.71e-07    | 3.48e-06    |
    | dq                                                    | 7.03e-03    | 2.81e-02    |
    | dk                                                    | 1.44e-02    | 5.76e-02    |
    | dv                                                    | 6.34e-03    | 2.54e-02    |
    | dq, causal rows 0..7, p = 0        (``dq_short``)       | 1.25e-01    | 5.00e-01    |
    | dq, causal rows 0..7, p > 0        (``dq_short_drop``)  | 6.57e+00    | 2.63e+01    |
    | dk with Sq = 1                     (``dk_single``)      | 1.02e-01    | 4.08e-01    |
    | d_rel                                                 | 1.89e-03    | 7.56e-03    |
    | d_rel with Sq = 1                  (``d_rel_single``)   | 4.42e-02    | 1.77e-01    |

The ill-conditioned classes (``dq_short``, ``dq_short_drop``, ``dk_single``, ``d_rel_single``) are
those of the d64 file, same cause (dS = P (dP - delta) with delta from the bf16 O, where
dP - delta cancels), each bounded by its own model figure.  ``d_rel`` is not bitwise reproducible
(LDS float adds in an order the hardware picks), so repeated runs are compared within the bound.

CASE MATRIX (B = 2, H = 3, D = 128, inputs randn * 0.5, scale 1/sqrt(128), rel_base = Sq - 1,
L = Sq + Sk - 1, rel = randn * 0.5), crossed with causal x p in {0, 0.1 (even Sk only)} x key
bias {none, present} x bias vector {none, present}:

| path                                                                      | (Sq, Sk)             |
|---------------------------------------------------------------------------|----------------------|
| one key block, full q-tiles                                               | (64, 72), (128, 128) |
| partial q-tile / single row                                               | (33, 128), (1, 40)   |
| one key block, Sq > 128                                                   | (160, 72)            |
| several key blocks (atomics + convert; windows meet in the reduce; keys   | (33, 130), (160, 264)|
|   past Sk in the last block)                                              |                      |
| odd Sk, p = 0                                                             | (96, 63)             |

Kernels: a p = 0 forward is ``attn_fwd_d128_kernel<CAUSAL, REL>``, a p > 0 forward
``attn_fwd_d128_drop_kernel<CAUSAL, REL>``, every backward ``attn_bwd_d128_kernel<DROP, CAUSAL,
MULTI, REL>`` (MULTI: Sk > 128, then ``attn_dq_convert_kernel``; REL: then
``attn_drel_reduce_kernel``); ``test_d128_kernels_selected`` reads the names from the profiler.
"""
import functools
import math

import pytest
import torch

from cloudtik_amd import ops
from cloudtik_amd.ops.attention import _relbias_reference
from test_attention_relbias_bwd_gpu import (SEED, _back, _bshd, _errors, _is_sentinel, _keep_mask, _key_bias, _model,
                                            _ref64, _rel_vec, _same_bits, _sentinel_like)

D = 128
B0, H0 = 2, 3
SCALE = 1.0 / math.sqrt(128.0)
SENTINEL = 0x7FA5

# worst error of _model against _ref64 over the whole matrix (see the module docstring)
MODEL_WORST = {"o": 6.17e-3, "lse": 8.71e-7, "dq": 7.03e-3, "dk": 1.44e-2, "dv": 6.34e-3,
               "dq_short": 1.25e-1, "dq_short_drop": 6.57, "dk_single": 1.02e-1,
               "d_rel": 1.89e-3, "d_rel_single": 4.42e-2}
BOUND = {k: 4.0 * v for k, v in MODEL_WORST.items()}

SHAPES = [(64, 72), (128, 128), (33, 128), (1, 40), (160, 72), (33, 130), (160, 264), (96, 63)]
# one shape per row of the table
ROW_SHAPES = [(64, 72), (33, 128), (160, 72), (160, 264), (96, 63)]


def _cases(shapes):
    out = []
    for Sq, Sk in shapes:
        for causal in (False, True):
            for p in (0.0, 0.1):
                if p > 0 and Sk % 2:
                    continue       # routed to the PyTorch reference: test_front_end_routes_to_reference
                for bias in ("none", "present"):
                    for relv in ("norel", "rel"):
                        out.append((Sq, Sk, causal, p, bias, relv))
    return out


def _id(c):
    return "%dx%d-%s-p%g-%s-%s" % (c[0], c[1], "causal" if c[2] else "full", c[3], c[4], c[5])


@functools.lru_cache(maxsize=None)
def _inputs(B, H, Sq, Sk, amp=0.5):
    g = torch.Generator().manual_seed(3000 * Sq + Sk)
    q = (torch.randn(B, H, Sq, D, generator=g) * amp).bfloat16()
    k = (torch.randn(B, H, Sk, D, generator=g) * amp).bfloat16()
    v = (torch.randn(B, H, Sk, D, generator=g) * amp).bfloat16()
    do = torch.randn(B, H, Sq, D, generator=g).bfloat16()
    return {"q": q, "k": k, "v": v, "do": do}


@functools.lru_cache(maxsize=None)
def _expected(case):
    """Inputs, key bias, bias vector (zeros for a case without one), keep mask and the fp64
    reference of one case: computed once, shared by every test that needs it, never modified."""
    Sq, Sk, causal, p, bias, relv = case
    inp = _inputs(B0, H0, Sq, Sk)
    kb = _key_bias(B0, Sk, bias)
    rel_base, L = Sq - 1, Sq + Sk - 1
    rel = _rel_vec(H0, L) if relv == "rel" else torch.zeros(H0, L)
    keep, seed, off = _keep_mask(B0, H0, Sq, Sk, p)
    want = _ref64(inp, rel, rel_base, kb, causal, keep, p, SCALE)
    if relv != "rel":
        want = {n: t for n, t in want.items() if n not in ("d_rel", "A")}
    return inp, kb, rel, rel_base, keep, (seed, off), want


def _check(got, want, kb=None, tag="", causal=False, p=0.0, rel_base=None):
    """Finite outputs, every quantity within its bound, exactly zero dk / dv at keys that carry a
    -10000 bias, and under the causal mask exactly zero d_rel at every offset past rel_base."""
    errs = _errors(got, want, causal, p)
    print("d128-err %s %s" % (tag, " ".join("%s=%.3e" % kv for kv in sorted(errs.items()))))
    for n, t in got.items():
        ok = torch.isfinite(t.double()) | (torch.isinf(want[n]) & (t.double() == want[n]))
        assert ok.all(), "%s: %s has %d non-finite values" % (tag, n, int((~ok).sum()))
    for n, e in errs.items():
        assert e <= BOUND[n], "%s: %s worst error %.3e > bound %.3e" % (tag, n, e, BOUND[n])
    if kb is not None:
        dead = kb <= -5000.0                                             # [B, Sk]
        for n in ("dk", "dv"):
            if n in got and dead.any():
                stray = got[n].double().abs().amax(-1).amax(1)[dead]
                assert (stray == 0).all(), "%s: %s is non-zero at a masked key (max %.3e)" % (tag, n, stray.max())
    if causal and "d_rel" in got:
        assert (got["d_rel"][:, rel_base + 1:] == 0).all(), "%s: d_rel non-zero past the causal diagonal" % tag
    return errs


def _model_of(case):
    inp, kb, rel, rel_base, keep, _, want = _expected(case)
    got = _model(inp, rel, rel_base, kb, case[2], keep, case[3], SCALE)
    if case[5] != "rel":
        del got["d_rel"]
    return got, want


def model_table(shapes=SHAPES):
    """Worst error of the rounding model per quantity over the cases of ``shapes``."""
    worst = {}
    for case in _cases(shapes):
        got, want = _model_of(case)
        for n, e in _errors(got, want, case[2], case[3]).items():
            worst[n] = max(worst.get(n, 0.0), e)
    return worst


# ------------------------------------------------------------------ GPU runners
def _run_direct(dev, inp, rel, rel_base, kb, causal, p, seed, off, with_rel):
    """The bindings called as the autograd functions call them."""
    C = ops.require_native()
    q, k, v, do = (_bshd(inp[n], dev) for n in ("q", "k", "v", "do"))
    B, Sq, H, _ = q.shape
    kbd = kb.to(dev) if kb is not None else None
    o = torch.empty_like(q)
    dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    if with_rel:
        reld = rel.to(dev)
        d_rel = torch.empty_like(reld)
        lse = C.attn_fwd_relbias_train(q, k, v, o, kbd, reld, rel_base, SCALE, p, seed, off, causal)
        C.attn_bwd_relbias(q, k, v, o, do, dq, dk, dv, d_rel, kbd, reld, rel_base, lse, SCALE, p, seed, off, causal)
    else:
        lse = C.attn_fwd_train(q, k, v, o, kbd, SCALE, p, seed, off, causal)
        C.attn_bwd_train(q, k, v, o, do, dq, dk, dv, kbd, lse, SCALE, p, seed, off, causal)
    out = {"o": _back(o), "lse": lse.view(B, H, Sq).cpu(), "dq": _back(dq), "dk": _back(dk), "dv": _back(dv)}
    if with_rel:
        out["d_rel"] = d_rel.cpu()
    return out


def _run_front(dev, inp, rel, rel_base, kb, causal, p, with_rel):
    """ops.attention_relbias under autograd, on the stream of ops.manual_seed(SEED)."""
    q, k, v = (_bshd(inp[n], dev).detach().requires_grad_() for n in ("q", "k", "v"))
    reld = rel.to(dev).requires_grad_() if with_rel else None
    ops.manual_seed(SEED)
    o = ops.attention_relbias(q, k, v, reld, rel_base, kb.to(dev) if kb is not None else None, scale=SCALE,
                              causal=causal, p=p)
    o.backward(_bshd(inp["do"], dev))
    out = {"o": _back(o.detach()), "dq": _back(q.grad), "dk": _back(k.grad), "dv": _back(v.grad)}
    if with_rel:
        out["d_rel"] = reld.grad.cpu()
    return out


# ------------------------------------------------------------------ 1. the case matrix
@pytest.mark.gpu
@pytest.mark.parametrize("case", _cases(SHAPES), ids=_id)
def test_d128_forward_backward(cuda, case):
    """Raw bindings against the fp64 reference; ops.attention_relbias under autograd returns what
    the raw bindings return (bit for bit where the kernels are deterministic, d_rel within its bound)."""
    Sq, Sk, causal, p, bias, relv = case
    inp, kb, rel, rel_base, keep, (seed, off), want = _expected(case)
    raw = _run_direct(cuda, inp, rel, rel_base, kb, causal, p, seed, off, relv == "rel")
    _check(raw, want, kb, "direct " + _id(case), causal, p, rel_base)
    front = _run_front(cuda, inp, rel, rel_base, kb, causal, p, relv == "rel")
    _same_bits(front, raw, ("o", "dk", "dv") + (("dq",) if Sk <= 128 else ()), "front " + _id(case))
    _check(front, want, kb, "front " + _id(case), causal, p, rel_base)


# ------------------------------------------------------------------ 2. extra cases
PAD_HS = {"q": 136, "k": 144, "v": 152, "do": 160, "o": 168, "dq": 176, "dk": 184, "dv": 200}


def _padded(dev, B, S, H, hs, fill_bits=SENTINEL, data=None):
    """A [B, S, H, 128] view into a larger buffer: 3 extra rows after S, head stride hs (a multiple
    of 8, not 128), a 16-element gap between batches, an 8-element (16-byte) offset from the base.
    Returns (buffer, view, mask of the buffer elements the view covers)."""
    ss = H * hs
    sb = (S + 3) * ss + 16
    n = 8 + B * sb + 8
    buf = torch.full((n,), fill_bits, dtype=torch.int16, device=dev).view(torch.bfloat16)
    geom = ((B, S, H, D), (sb, ss, hs, 1), 8)
    view = buf.as_strided(*geom)
    mask = torch.zeros(n, dtype=torch.bool, device=dev)
    mask.as_strided(*geom).fill_(True)
    if data is not None:
        view.copy_(data)
    return buf, view, mask


@pytest.mark.gpu
@pytest.mark.parametrize("Sq,Sk", [(33, 128), (160, 264)])
def test_padded_views_write_nothing_outside(cuda, Sq, Sk):
    """q, k, v, dO, o, dq, dk, dv are padded views with eight different head strides, the inputs'
    padding NaN, the outputs' a sentinel that must survive; d_rel is a transposed [L, H] view inside
    a sentinel-filled buffer.  Strides of one tensor used for another read NaN or hit a sentinel."""
    case = (Sq, Sk, True, 0.1, "present", "rel")
    inp, kb, rel, rel_base, keep, (seed, off), want = _expected(case)
    C = ops.require_native()
    t = {}
    for n, S in (("q", Sq), ("k", Sk), ("v", Sk), ("do", Sq)):
        _, t[n], _ = _padded(cuda, B0, S, H0, PAD_HS[n], 0x7FC0, _bshd(inp[n], cuda))
    out = {n: _padded(cuda, B0, S, H0, PAD_HS[n]) for n, S in (("o", Sq), ("dq", Sq), ("dk", Sk), ("dv", Sk))}
    kbd, reld = kb.to(cuda), rel.to(cuda)
    L = rel.shape[1]
    dbuf = _sentinel_like(torch.empty(L + 2, H0 + 1, device=cuda))
    d_rel = dbuf[1:L + 1, :H0].t()
    lse = C.attn_fwd_relbias_train(t["q"], t["k"], t["v"], out["o"][1], kbd, reld, rel_base, SCALE, 0.1, seed, off, True)
    C.attn_bwd_relbias(t["q"], t["k"], t["v"], out["o"][1], t["do"], out["dq"][1], out["dk"][1], out["dv"][1], d_rel,
                       kbd, reld, rel_base, lse, SCALE, 0.1, seed, off, True)
    torch.cuda.synchronize()
    for n, (buf, _, mask) in out.items():
        assert bool((buf.view(torch.int16)[~mask] == SENTINEL).all()), "%s: written outside its valid region" % n
    assert _is_sentinel(dbuf[0]) and _is_sentinel(dbuf[L + 1]) and _is_sentinel(dbuf[:, H0])
    got = {n: _back(view) for n, (_, view, _) in out.items()}
    got.update(lse=lse.view(B0, H0, Sq).cpu(), d_rel=d_rel.cpu())
    _check(got, want, kb, "padded " + _id(case), True, 0.1, rel_base)


@pytest.mark.gpu
@pytest.mark.parametrize("Sq,Sk", [(33, 128), (160, 264)])
def test_fully_masked_batch(cuda, Sq, Sk):
    """-inf on every key of batch 0: nothing is NaN, batch 0's o, dq, dk, dv are exactly zero (lse
    +inf), and d_rel equals the reference, to which batch 0 contributes nothing."""
    case = (Sq, Sk, False, 0.0, "inf0", "rel")
    inp, kb, rel, rel_base, keep, _, want = _expected(case)
    got = _run_direct(cuda, inp, rel, rel_base, kb, False, 0.0, 0, 0, True)
    assert (got["o"][0] == 0).all() and (got["lse"][0] == float("inf")).all()
    for n in ("dq", "dk", "dv"):
        assert torch.isfinite(got[n].float()).all() and (got[n][0] == 0).all(), n
    assert torch.isfinite(got["d_rel"]).all()
    alone = _ref64({n: t[1:] for n, t in inp.items()}, rel, rel_base, kb[1:], scale=SCALE)
    assert torch.allclose(alone["d_rel"], want["d_rel"], rtol=1e-12, atol=0)     # batch 0 adds nothing
    rest = {n: (t if n in ("d_rel", "A") else t[1:]) for n, t in want.items()}
    _check({n: (t if n == "d_rel" else t[1:]) for n, t in got.items()}, rest, None, "masked " + _id(case))


@pytest.mark.gpu
@pytest.mark.parametrize("Sq,Sk", [(33, 128), (160, 264)])
def test_same_seed_same_bits(cuda, Sq, Sk):
    """Two runs from one seed: bit-equal o, lse, dk, dv, and dq for Sk <= 128 (Sk > 128 sums dQ with
    fp32 atomics); d_rel within its bound of the reference both times.  Another seed: another o."""
    case = (Sq, Sk, True, 0.1, "present", "rel")
    inp, kb, rel, rel_base, keep, (seed, off), want = _expected(case)
    a = _run_direct(cuda, inp, rel, rel_base, kb, True, 0.1, seed, off, True)
    b = _run_direct(cuda, inp, rel, rel_base, kb, True, 0.1, seed, off, True)
    _same_bits(a, b, ("o", "lse", "dk", "dv") + (("dq",) if Sk <= 128 else ()), "rerun " + _id(case))
    for r in (a, b):
        _check({"d_rel": r["d_rel"]}, want, None, "rerun d_rel " + _id(case), True, 0.1, rel_base)
    other = _run_direct(cuda, inp, rel, rel_base, kb, True, 0.1, seed + 1, off, True)
    assert not torch.equal(other["o"], a["o"])


@pytest.mark.gpu
def test_long_query_windows(cuda):
    """Sq = 2048 (past the d64 kernels' limit of 1856): W = 2175 offsets, 17.4 KB of dynamic LDS
    next to the backward's 115,200 static bytes; the D = 128 budget takes it and the kernels run it
    (ops.attention_relbias under autograd).  The rounding model's figures at this shape (o 5.15e-3,
    lse 6.24e-7, dq 6.95e-3, dk 4.65e-3, dv 4.08e-3, d_rel 4.76e-4) are within the table's, so
    the table's bounds hold here."""
    C = ops.require_native()
    Sq, Sk = 2048, 96
    assert C.attn_bwd_relbias_window(Sq) > C.attn_bwd_relbias_max_window()
    assert C.attn_bwd_relbias_window(Sq) <= C.attn_bwd_relbias_max_window_d(128)
    inp = _inputs(1, 1, Sq, Sk)
    rel = _rel_vec(1, Sq + Sk - 1)
    want = _ref64(inp, rel, Sq - 1, None, False, None, 0.0, SCALE)
    names = _attn_kernels(lambda: _run_front(cuda, inp, rel, Sq - 1, None, False, 0.0, True))
    assert any("attn_bwd_d128" in n for n in names) and any("attn_drel_reduce_kernel" in n for n in names), names
    _check(_run_front(cuda, inp, rel, Sq - 1, None, False, 0.0, True), want, None, "long Sq", False, 0.0, Sq - 1)


# ------------------------------------------------------------------ 3. the kernels that ran
def _attn_kernels(fn):
    from torch.profiler import ProfilerActivity, profile
    fn()                                                       # warm: module load, allocations
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "attn_" in e.name]


@pytest.mark.gpu
@pytest.mark.parametrize("with_rel", [True, False], ids=["rel", "norel"])
def test_d128_kernels_selected(cuda, with_rel):
    """The kernels that actually ran, by name from the profiler, one shape per row of the table."""
    for Sq, Sk in ROW_SHAPES:
        for p in ((0.0, 0.1) if Sk % 2 == 0 else (0.0,)):
            inp = _inputs(B0, H0, Sq, Sk)
            rel = _rel_vec(H0, Sq + Sk - 1)
            names = _attn_kernels(lambda: _run_direct(cuda, inp, rel, Sq - 1, None, True, p, SEED, 0, with_rel))
            tag = (Sq, Sk, p, names)
            fwd = [n for n in names if "attn_fwd" in n]
            bwd = [n for n in names if "attn_bwd" in n]
            assert len(fwd) == 1 and len(bwd) == 1, tag
            if p > 0:
                assert "attn_fwd_d128_drop" in fwd[0], tag
            else:
                assert "attn_fwd_d128_kernel<true, %s>" % ("true" if with_rel else "false") in fwd[0], tag
            assert "attn_bwd_d128" in bwd[0], tag
            assert sum("attn_drel_reduce_kernel" in n for n in names) == (1 if with_rel else 0), tag
            assert any("attn_dq_convert_kernel" in n for n in names) == (Sk > 128), tag


# ------------------------------------------------------------------ 4. the front end
@pytest.mark.gpu
@pytest.mark.parametrize("how", ["odd_sk_dropout", "long_rel"])
def test_front_end_routes_to_reference(cuda, how):
    """Calls the kernels cannot take go to the PyTorch reference, on the stream the front end drew:
    odd Sk with p > 0, and a bias vector longer than 4096."""
    if how == "odd_sk_dropout":
        B, H, Sq, Sk, p = B0, H0, 96, 63, 0.1
    else:
        B, H, Sq, Sk, p = 1, 1, 2100, 2000, 0.0
    inp = _inputs(B, H, Sq, Sk)
    rel_base, L = Sq - 1, Sq + Sk - 1
    rel = _rel_vec(H, L).to(cuda)
    q, k, v, do = (_bshd(inp[n], cuda) for n in ("q", "k", "v", "do"))
    leaves = [t.detach().requires_grad_() for t in (q, k, v, rel)]
    ops.manual_seed(SEED)
    names = _attn_kernels(lambda: ops.attention_relbias(*leaves, rel_base, None, scale=SCALE, causal=False, p=p))
    assert not names, names
    ops.manual_seed(SEED)
    got = ops.attention_relbias(*leaves, rel_base, None, scale=SCALE, causal=False, p=p)
    got.backward(do)
    ops.manual_seed(SEED)
    seed, off = ops._rng.next(B * H * Sq * Sk) if p > 0 else (0, 0)
    leaves2 = [t.detach().requires_grad_() for t in (q, k, v, rel)]
    want = _relbias_reference(*leaves2, rel_base, None, SCALE, False, p, seed, off)
    want.backward(do)
    assert torch.equal(got, want)
    for a, b in zip(leaves, leaves2):
        assert torch.isfinite(a.grad).all()
        assert (a.grad.float() - b.grad.float()).abs().max() <= 1e-3 * b.grad.float().abs().max()


@pytest.mark.gpu
def test_front_end_plain_training_kernels(cuda):
    """attention_relbias(rel_bias=None) at D = 128 with a gradient runs the plain training kernels
    (no reduce kernel), at p = 0 and p > 0; without a gradient and dropout, the inference call."""
    Sq, Sk = 64, 72
    inp = _inputs(B0, H0, Sq, Sk)
    do = _bshd(inp["do"], cuda)
    for p in (0.0, 0.1):
        def step():
            q, k, v = (_bshd(inp[n], cuda).detach().requires_grad_() for n in ("q", "k", "v"))
            ops.attention_relbias(q, k, v, None, scale=SCALE, p=p).backward(do)
        names = _attn_kernels(step)
        assert len(names) == 2, names
        assert ("attn_fwd_d128_drop" if p > 0 else "attn_fwd_d128_kernel<false, false>") in names[0], names
        assert "attn_bwd_d128_kernel<%s, false, false, false>" % ("true" if p > 0 else "false") in names[1], names
    q, k, v = (_bshd(inp[n], cuda) for n in ("q", "k", "v"))
    names = _attn_kernels(lambda: ops.attention_relbias(q, k, v, None, scale=SCALE))
    assert len(names) == 1 and "attn_fwd_d128_kernel<false, false>" in names[0], names


@pytest.mark.gpu
def test_window_budget_and_old_entries(cuda):
    """The D-aware window query: the d64 figure at 64, and at 128 room for every L <= 4096 call;
    the older entries still refuse D = 128 training calls and write nothing."""
    C = ops.require_native()
    assert C.attn_bwd_relbias_max_window_d(64) == C.attn_bwd_relbias_max_window()
    assert C.attn_bwd_relbias_max_window_d(128) >= C.attn_bwd_relbias_window(4096)
    inp = _inputs(B0, H0, 64, 72)
    q, k, v, do = (_bshd(inp[n], cuda) for n in ("q", "k", "v", "do"))
    o = _sentinel_like(q)
    with pytest.raises(RuntimeError, match="no dropout"):
        C.attn_fwd(q, k, v, o, None, SCALE, 0.1, 3, 0, False)
    outs = [_sentinel_like(q), _sentinel_like(k), _sentinel_like(v)]
    with pytest.raises(RuntimeError, match="forward only"):
        C.attn_bwd(q, k, v, q, do, outs[0], outs[1], outs[2], None, torch.zeros(B0 * H0, 64, device=cuda), SCALE, 0.0,
                   0, 0, False)
    torch.cuda.synchronize()
    assert all(_is_sentinel(t) for t in [o] + outs)
