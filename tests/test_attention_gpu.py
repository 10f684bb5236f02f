"""Attention kernels (ops/csrc/attention.hip): per-row checks on every dispatch path and edge.

Every case compares the HIP kernels with an fp64 reference computed from the same bf16 inputs
(``_ref64``), row by row:

* ``o``, ``dq``, ``dk``, ``dv``: for every (batch, head, row), max |kernel - ref| over the 64
  columns divided by (max |ref| over that row + 1e-3 x the tensor's max |ref|); the assertion is
  on the worst row.
* ``lse`` (log2 domain, what the backward consumes): absolute difference per row.

BOUNDS.  Not taken from the kernel.  ``_model`` is a CPU model of the kernels' arithmetic that
rounds only where they round -- fp32 scores and accumulation, P and dS rounded to bf16 before
their MFMAs, delta = rowsum(dO * O) from the bf16 O, and O, dQ, dK, dV rounded to bf16.  Its worst
per-row error against the fp64 reference over the whole case matrix below (default dispatch
matrix plus the relative-bias cases; measured on a CPU) is

    | quantity                                             | model worst | bound (4 x) |
    |------------------------------------------------------|-------------|-------------|
    | o                                                    | 5.87e-3     | 2.35e-2     |
    | lse (absolute, log2 units)                           | 8.11e-7     | 3.24e-6     |
    | dq                                                   | 7.84e-3     | 3.14e-2     |
    | dk                                                   | 1.38e-2     | 5.52e-2     |
    | dv                                                   | 6.63e-3     | 2.65e-2     |
    | dq, causal rows 0..7, p = 0        (``dq_short``)      | 2.10e-1     | 8.40e-1     |
    | dq, causal rows 0..7, p > 0        (``dq_short_drop``) | 5.18        | 2.07e+1     |
    | dk with Sq = 1                     (``dk_single``)     | 1.50e-1     | 6.00e-1     |

and each bound is 4 x that (``BOUND``): the factor covers accumulation order, the exp2-domain
online-softmax rescaling and the hardware exp2.  ``test_rounding_model_meets_bounds`` re-runs
the model over the matrix.

ILL-CONDITIONED ROWS.  One bound per quantity over the whole matrix would be 2.07e+1 for dq and
6.00e-1 for dk, which checks nothing, so the rows that cause it have bounds of their own and every
other row keeps a tight one (each bound is at most the single whole-matrix one).  The cause is
in the arithmetic, not in a kernel: dS = P (dP - delta) with delta = rowsum(dO * O) taken from
the bf16 O, so delta carries an absolute error of about 2^-9 |dO . O| that does not shrink
where dP - delta cancels.
* Under the causal mask query row q sees q + 1 keys.  Row 0 sees one: its exact dq is zero,
  while 1 / (1 - p) scaled O = V[0] / 0.9 no longer rounds to bf16 exactly, so the computed dq is
  about 2.5e-3 against a floor of 1e-3 x max |dq| = 5e-4.  The model's error per row falls from
  5.2 (row 0, p = 0.1) and 0.21 (row 1, p = 0) to the regular 6e-3 by row 8.
* With Sq = 1 a dk row is dS[key] x q: there is no sum over queries to absorb a key whose
  dP - delta nearly cancels.
* A tensor whose reference is identically zero (dq and dk when the only query sees one key) has
  no scale of its own; its error is taken in absolute units (relative to 1, the scale of dO).
The dS of those rows is still checked tightly through dk (which sums over all queries) and
their dQ store paths through the non-causal cases of the same shapes.

CASE MATRIX (B = 2, H = 3, D = 64, inputs randn * 0.5, scale 1/8), crossed with causal x
p in {0, 0.1} (0.1 only for even Sk) x key bias {none, present}:

| path                                                                      | (Sq, Sk)                          |
|---------------------------------------------------------------------------|-----------------------------------|
| forward, one K/V tile                                                     | (40, 40), (1, 64)                 |
| forward resident (two tiles) + LDS-DMA backward (Sq <= 128, one key       | (128, 128), (64, 72)              |
|   block), full q-tiles                                                    |                                   |
| same, partial q-tile -> scalar dQ stores                                  | (100, 72), (33, 128), (1, 40)     |
| backward, register-staged single block (Sq > 128, Sk <= 128)              | (160, 72), (129, 128), (200, 40)  |
| backward MULTI (Sk > 128), fp32 atomics + convert                         | (33, 130), (200, 200), (160, 264) |
| odd Sk, p = 0 only                                                        | (96, 63), (128, 129)              |

KERNEL INSTANTIATIONS -> CASES.  {DROP, CAUSAL} is covered everywhere by the causal x p cross.

* forward ``attn_fwd_d64_kernel<DROP, CAUSAL, false, 3, GL=true>`` (default): every case of
  ``test_default_dispatch``; one tile Sk <= 64, resident 65..128, streamed >= 129.
* forward ``<.., 2, GL=false>`` (register-staged): ``test_variant_subset`` in the child with
  ``CLOUDTIK_AMD_ATTN_FWD_GLDS=0``; ``<.., 2, GL=true>``: the child with ``..._FWD_WPE=2``.
* forward ``attn_fwd_pipe_kernel<DROP, CAUSAL>``: the children with ``..._FWD_PIPE=1`` (persistent
  grid) and ``..._FWD_PIPE=1 ..._PERSIST=0`` (one workgroup per item); ``test_variant_persistent_walk``
  gives every workgroup several items there.
* forward ``<false, CAUSAL, REL=true>``: ``test_relbias_forward``.
* backward ``attn_bwd_d64_kernel<DROP, CAUSAL, MULTI=false, GL=true>``: Sq <= 128 and Sk <= 128 rows.
* backward ``<.., MULTI=false, GL=false>``: the Sq > 128, Sk <= 128 row; every single-block case
  in the child with ``CLOUDTIK_AMD_ATTN_BWD_GL=0``.
* backward ``<.., MULTI=true, GL=false>`` + ``attn_dq_convert_kernel``: the Sk > 128 rows.
* dQ stores: 16-byte (full 32-query tile, one key block) (128, 128), (64, 72), (160, 72);
  scalar (partial tile, one key block) (100, 72), (33, 128), (1, 40), (129, 128), (200, 40), and
  every tile of a dq that is not 16-byte addressable (``test_unaligned_dq_takes_scalar_stores``);
  fp32 atomics + convert (33, 130), (200, 200), (160, 264), (128, 129).
* dK / dV tail store (``store_row64`` with rows past Sk gated off): every Sk that is no multiple
  of 128; the canary test shows nothing lands past Sk.
* ``test_variant_kernels_selected`` reads the names of the kernels that ran from the profiler and
  compares them with the dispatcher's rule, in this process and in every child process.
* p > 0 with odd Sk is routed by the wrapper to the PyTorch reference;
  ``test_odd_sk_dropout_routes_to_reference`` asserts that routing (the kernel refuses: rc -2).

The causal mask is top-left aligned (key index > query index is masked), also when Sq != Sk, as
in ``ops.reference.attention`` and both kernels.
"""
import functools
import math
import os
import subprocess
import sys

import pytest
import torch

from cloudtik_amd import ops
from cloudtik_amd.ops import reference as ref

D = 64
B0, H0 = 2, 3
SCALE = 0.125
SEED = 11
LN2 = math.log(2.0)
LOG2E = 1.0 / LN2

# worst per-row error of _model against _ref64 over the whole matrix (see the module docstring)
MODEL_WORST = {"o": 5.87e-3, "lse": 8.11e-7, "dq": 7.84e-3, "dk": 1.38e-2, "dv": 6.63e-3,
               "dq_short": 2.10e-1, "dq_short_drop": 5.18, "dk_single": 1.50e-1}
BOUND = {k: 4.0 * v for k, v in MODEL_WORST.items()}

SHAPES = [(40, 40), (1, 64),
          (128, 128), (64, 72),
          (100, 72), (33, 128), (1, 40),
          (160, 72), (129, 128), (200, 40),
          (33, 130), (200, 200), (160, 264),
          (96, 63), (128, 129)]
REL_SHAPES = [(1, 200), (33, 130), (129, 65), (96, 63)]
# one shape per row of the table, for the non-default kernels
VARIANT_SHAPES = [(40, 40), (64, 72), (100, 72), (160, 72), (200, 200), (96, 63)]


def _cases(shapes, biases=("none", "present")):
    out = []
    for Sq, Sk in shapes:
        for causal in (False, True):
            for p in (0.0, 0.1):
                if p > 0 and Sk % 2:
                    continue       # routed to the PyTorch reference: test_odd_sk_dropout_routes_to_reference
                for bias in biases:
                    out.append((Sq, Sk, causal, p, bias))
    return out


def _id(c):
    return "%dx%d-%s-p%g-%s" % (c[0], c[1], "causal" if c[2] else "full", c[3], c[4])


# ------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=None)
def _inputs(B, H, Sq, Sk):
    g = torch.Generator().manual_seed(1000 * Sq + Sk)
    q = (torch.randn(B, H, Sq, D, generator=g) * 0.5).bfloat16()
    k = (torch.randn(B, H, Sk, D, generator=g) * 0.5).bfloat16()
    v = (torch.randn(B, H, Sk, D, generator=g) * 0.5).bfloat16()
    do = torch.randn(B, H, Sq, D, generator=g).bfloat16()
    return {"q": q, "k": k, "v": v, "do": do}


def _key_bias(B, Sk, kind):
    """none | present: a small finite bias on every key plus -10000 on the last quarter of the keys
    of batch 1 only (so batch indexing matters) | inf0: -inf on every key of batch 0."""
    if kind == "none":
        return None
    g = torch.Generator().manual_seed(77 + Sk)
    kb = torch.randn(B, Sk, generator=g) * 0.5
    if kind == "present":
        kb[1, Sk - Sk // 4:] = -10000.0
    else:
        kb[0] = float("-inf")
    return kb


def _rel_matrix(rel, rel_base, Sq, Sk):
    idx = torch.arange(Sk)[None, :] - torch.arange(Sq)[:, None] + rel_base
    return rel[:, idx]                                                   # [H, Sq, Sk]


def _keep_mask(B, H, Sq, Sk, p):
    """The keep mask of the stream the wrappers draw after ops.manual_seed(SEED)."""
    if p == 0:
        return None, 0, 0
    ops.manual_seed(SEED)
    seed, off = ops._rng.next(B * H * Sq * Sk)
    return ref.attn_dropout_keep(B, H, Sq, Sk, p, seed, off), seed, off


# ------------------------------------------------------------------ fp64 reference
def _ref64(inp, kb=None, causal=False, keep=None, p=0.0, relm=None, masked=None):
    """fp64 forward + autograd backward from the bf16 inputs ([B, H, S, 64]).  ``masked``
    ([.., Sq, Sk] bool) overrides the causal mask (the checker tests shift it).  Rows with every
    key masked get P = 0: O = 0, lse = +inf, zero gradients (what the kernels define)."""
    q, k, v = (inp[n].double().requires_grad_() for n in ("q", "k", "v"))
    Sq, Sk = q.shape[2], k.shape[2]
    s = q @ k.transpose(-1, -2) * SCALE
    if kb is not None:
        s = s + kb.double()[:, None, None, :]
    if relm is not None:
        s = s + relm.double()[None]
    if masked is None and causal:
        # top-left aligned, also when Sq != Sk: key index > query index is masked
        masked = torch.ones(Sq, Sk, dtype=torch.bool).triu(1)
    if masked is not None:
        s = s.masked_fill(masked, float("-inf"))
    m = s.detach().amax(-1, keepdim=True)
    m = torch.where(torch.isinf(m), torch.zeros_like(m), m)
    e = torch.exp(s - m)
    l = e.sum(-1, keepdim=True)
    pr = e / torch.where(l > 0, l, torch.ones_like(l))
    lse = torch.where(l > 0, m + torch.log(torch.where(l > 0, l, torch.ones_like(l))),
                      torch.full_like(l, float("inf"))).squeeze(-1) / LN2
    if keep is not None:
        w = keep if keep.dtype != torch.bool else keep.double() / (1.0 - p)
        pr = pr * w
    o = pr @ v
    o.backward(inp["do"].double())
    return {"o": o.detach(), "lse": lse.detach(), "dq": q.grad, "dk": k.grad, "dv": v.grad}


# ------------------------------------------------------------------ CPU rounding model of the kernels
def _bf(x):
    return x.bfloat16().float()


def _model(inp, kb=None, causal=False, keep=None, p=0.0, relm=None):
    """What the kernels compute, with their rounding steps and nothing else: fp32 scores in the
    log2 domain, l = the pre-dropout fp32 row sum, P rounded to bf16 before P.V, O rounded to
    bf16, delta from that bf16 O, P (x 1/keep) and dS rounded to bf16 before their MFMAs, fp32
    accumulation, dQ / dK / dV rounded to bf16."""
    q, k, v, do = (inp[n].float() for n in ("q", "k", "v", "do"))
    Sq, Sk = q.shape[2], k.shape[2]
    sl2 = torch.tensor(SCALE, dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32)
    s = (q @ k.transpose(-1, -2)) * sl2
    if kb is not None:
        s = s + (kb.float() * LOG2E)[:, None, None, :]
    if relm is not None:
        s = s + (relm.float() * LOG2E)[None]
    if causal:
        s = s.masked_fill(torch.ones(Sq, Sk, dtype=torch.bool).triu(1), float("-inf"))
    m = s.amax(-1, keepdim=True)
    msub = torch.where(torch.isinf(m), torch.zeros_like(m), m)
    pu = torch.exp2(s - msub)
    l = pu.sum(-1, keepdim=True)
    inv_keep = 1.0 / (1.0 - p) if p > 0 else 1.0
    kf = keep.float() if keep is not None else torch.ones_like(pu)
    inv = torch.where(l > 0, inv_keep / torch.where(l > 0, l, torch.ones_like(l)), torch.zeros_like(l))
    o = _bf((_bf(pu * kf) @ v) * inv)
    lse = torch.where(l > 0, m + torch.log2(torch.where(l > 0, l, torch.ones_like(l))),
                      torch.full_like(l, float("inf")))
    delta = (do * o).sum(-1, keepdim=True)
    pn = torch.exp2(s - lse)
    pd = pn * kf * inv_keep
    dpv = (do @ v.transpose(-1, -2)) * kf * inv_keep
    ds = _bf(pn * (dpv - delta))
    dv = _bf(_bf(pd).transpose(-1, -2) @ do)
    dk = _bf((ds.transpose(-1, -2) @ q) * SCALE)
    dq = _bf((ds @ k) * SCALE)
    return {"o": o, "lse": lse.squeeze(-1), "dq": dq, "dk": dk, "dv": dv}


# ------------------------------------------------------------------ metric and checker
SHORT = 8      # causal query rows with fewer than SHORT visible keys: see "ILL-CONDITIONED ROWS"


def _rows(x, want):
    """Per-row error [..., S]: max |x - want| over the 64 columns / (max |want| over the row + 1e-3
    of the tensor's max |want|).  A reference that is identically zero (dq and dk of a single
    visible key: a one-key softmax has no gradient) has no scale; the error is then absolute,
    that is relative to 1, the scale of dO."""
    x, want = x.double(), want.double()
    d = (x - want).abs().amax(-1)
    top = want.abs().max()
    if top == 0:
        return d
    return d / (want.abs().amax(-1) + 1e-3 * top)


def _lse_err(x, want):
    x, want = x.double(), want.double()
    same_inf = torch.isinf(want) & (x == want)
    d = torch.where(same_inf, torch.zeros_like(want), (x - want).abs())
    return d.max().item()


def _errors(got, want, causal=False, p=0.0):
    """Worst row per quantity, keyed like BOUND."""
    out = {}
    for n, t in got.items():
        if n == "lse":
            out[n] = _lse_err(t, want[n])
            continue
        e = _rows(t, want[n])                                            # [B, H, S]
        if n == "dq" and causal:
            out["dq_short_drop" if p > 0 else "dq_short"] = e[..., :SHORT].max().item()
            if e.shape[-1] > SHORT:
                out[n] = e[..., SHORT:].max().item()
        elif n == "dk" and want["o"].shape[2] == 1:
            out["dk_single"] = e.max().item()
        else:
            out[n] = e.max().item()
    return out


def _check(got, want, kb=None, tag="", causal=False, p=0.0):
    """The assertions of every case: finite outputs, every quantity within its bound on its worst
    row, and exactly zero dk / dv at keys that carry a -10000 bias."""
    errs = _errors(got, want, causal, p)
    print("attn-err %s %s" % (tag, " ".join("%s=%.3e" % kv for kv in sorted(errs.items()))))
    for n, t in got.items():
        ok = torch.isfinite(t.double()) | (torch.isinf(want[n]) & (t.double() == want[n]))
        assert ok.all(), "%s: %s has %d non-finite values" % (tag, n, int((~ok).sum()))
    for n, e in errs.items():
        assert e <= BOUND[n], "%s: %s worst row error %.3e > bound %.3e" % (tag, n, e, BOUND[n])
    if kb is not None:
        dead = kb <= -5000.0                                             # [B, Sk]
        for n in ("dk", "dv"):
            if n in got and dead.any():
                stray = got[n].double().abs().amax(-1).amax(1)[dead]     # [B, Sk] -> masked keys
                assert (stray == 0).all(), "%s: %s is non-zero at a masked key (max %.3e)" % (tag, n, stray.max())
    return errs


def _rel(a, b):
    """The whole-tensor criterion of the older attention tests."""
    a, b = a.double(), b.double()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


@functools.lru_cache(maxsize=None)
def _expected(case, B=B0, H=H0):
    """Inputs, key bias, keep mask and the fp64 reference of one case: computed once, shared by
    every test that needs it, never modified."""
    Sq, Sk, causal, p, bias = case
    inp = _inputs(B, H, Sq, Sk)
    kb = _key_bias(B, Sk, bias)
    keep, seed, off = _keep_mask(B, H, Sq, Sk, p)
    return inp, kb, keep, (seed, off), _ref64(inp, kb, causal, keep, p)


@functools.lru_cache(maxsize=None)
def _expected_rel(Sq, Sk, causal, bias):
    inp = _inputs(B0, H0, Sq, Sk)
    kb = _key_bias(B0, Sk, bias)
    g = torch.Generator().manual_seed(5 + Sq)
    rel = torch.randn(H0, Sq + Sk - 1, generator=g) * 0.5
    relm = _rel_matrix(rel, Sq - 1, Sq, Sk)
    return inp, kb, rel, relm, _ref64(inp, kb, causal, relm=relm)


# ------------------------------------------------------------------ the checker itself, on the CPU
def test_rounding_model_meets_bounds():
    """The model that the bounds come from passes them (by a factor of 4) on every case of the
    matrix, relative-bias cases included; prints its worst error per quantity."""
    worst = {n: 0.0 for n in BOUND}
    for case in _cases(SHAPES):
        inp, kb, keep, _, want = _expected(case)
        got = _model(inp, kb, case[2], keep, case[3])
        for n, e in _errors(got, want, case[2], case[3]).items():
            worst[n] = max(worst[n], e)
        _check(got, want, kb, "model " + _id(case), case[2], case[3])
    for Sq, Sk in REL_SHAPES:
        for causal in (False, True):
            for bias in ("none", "present"):
                inp, kb, _, relm, want = _expected_rel(Sq, Sk, causal, bias)
                got = _model(inp, kb, causal, relm=relm)
                got = {n: got[n] for n in ("o", "lse")}
                for n, e in _errors(got, want).items():
                    worst[n] = max(worst[n], e)
                _check(got, want, None, "model rel %dx%d" % (Sq, Sk))
    print("model worst:", " ".join("%s=%.3e" % kv for kv in sorted(worst.items())))
    for n in BOUND:     # the recorded figures are the model's, give or take another CPU's summation order
        assert MODEL_WORST[n] / 2 <= worst[n] <= MODEL_WORST[n] * 2, (n, worst[n], MODEL_WORST[n])


def _fails(got, want, kb=None, tag="", causal=False, p=0.0):
    with pytest.raises(AssertionError):
        _check(got, want, kb, tag, causal, p)


def test_checker_catches_zeroed_output_row():
    """One output row zeroed.  At the largest shape of test_attention_packed (B 2, H 4, S 512) it
    is 1 / sqrt(4096) = 1.6e-2 of the tensor norm: inside the old 2e-2, outside the per-row bound."""
    inp = _inputs(2, 4, 512, 512)
    want = _ref64(inp)
    got = {n: t.clone() for n, t in want.items()}
    got["o"][1, 2, 300] = 0
    assert _rel(got["o"], want["o"]) < 2e-2
    _fails(got, want, tag="zeroed row")


def test_checker_catches_shifted_causal_diagonal():
    """The causal diagonal shifted by one (key q + 1 admitted) for one 32-row tile of one head."""
    case = (200, 200, True, 0.0, "none")
    inp, kb, _, _, want = _expected(case)
    masked = torch.ones(200, 200, dtype=torch.bool).triu(1).expand(B0, H0, 200, 200).clone()
    masked[1, 2, 160:192] = torch.ones(200, 200, dtype=torch.bool).triu(2)[160:192]
    got = _ref64(inp, kb, True, masked=masked)
    assert _rel(got["o"], want["o"]) < 2e-2
    _fails(got, want, tag="shifted diagonal", causal=True)
    _fails({"o": got["o"]}, want, tag="shifted diagonal, o alone", causal=True)


def test_checker_catches_key_past_sk():
    """One key past Sk admitted with a zero score (zero-filled K and V rows that the -inf tail
    bias failed to mask): every row of O shrinks by about 1 / (Sk + 1), inside the old 2e-2; the
    row sums, hence lse, move by log2(1 + 1 / Sk)."""
    case = (96, 63, False, 0.0, "none")
    inp, kb, _, _, want = _expected(case)
    z = torch.zeros(B0, H0, 1, D, dtype=torch.bfloat16)
    ghost = {"q": inp["q"], "do": inp["do"], "k": torch.cat([inp["k"], z], 2), "v": torch.cat([inp["v"], z], 2)}
    got = _ref64(ghost)
    got["dk"], got["dv"] = got["dk"][:, :, :63], got["dv"][:, :, :63]
    assert _rel(got["o"], want["o"]) < 2e-2
    _fails(got, want, tag="key past Sk")
    _fails({"lse": got["lse"]}, want, tag="key past Sk, lse alone")


def test_checker_catches_missing_dropout_rescale():
    """The 1 / (1 - p) rescale missing on one 64-key tile of one head."""
    case = (200, 200, False, 0.1, "none")
    inp, kb, keep, _, want = _expected(case)
    w = keep.double() / 0.9
    w[0, 1, :, 64:128] = keep[0, 1, :, 64:128].double()
    got = _ref64(inp, kb, False, w, 0.1)
    _fails(got, want, tag="dropout rescale", p=0.1)
    _fails({"o": got["o"]}, want, tag="dropout rescale, o alone", p=0.1)


def test_checker_catches_gradient_at_masked_key():
    """dk of one masked key non-zero, by far less than any norm would notice."""
    case = (64, 72, False, 0.0, "present")
    inp, kb, _, _, want = _expected(case)
    got = {n: t.clone() for n, t in want.items()}
    _check(got, want, kb, "reference against itself")
    got["dk"][1, 0, 71, 5] = 1e-30
    _fails(got, want, kb, tag="masked key")


# ------------------------------------------------------------------ GPU runners
def _bshd(t, dev):
    """[B, H, S, 64] (CPU, contiguous) -> the [B, S, H, 64] view of a device copy."""
    return t.to(dev).transpose(1, 2)


def _back(t):
    """[B, S, H, 64] device view -> [B, H, S, 64] on the CPU."""
    return t.transpose(1, 2).cpu()


def _run_direct(dev, inp, kb, causal, p, seed, off, backward=True):
    """attn_fwd / attn_bwd called as the autograd functions call them; returns lse too."""
    C = ops.require_native()
    q, k, v, do = (_bshd(inp[n], dev) for n in ("q", "k", "v", "do"))
    B, Sq, H, _ = q.shape
    kbd = kb.to(dev) if kb is not None else None
    o = torch.empty_like(q)
    lse = C.attn_fwd(q, k, v, o, kbd, SCALE, p, seed, off, causal)
    got = {"o": _back(o), "lse": lse.view(B, H, Sq).cpu()}
    if backward:
        dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        C.attn_bwd(q, k, v, o, do, dq, dk, dv, kbd, lse, SCALE, p, seed, off, causal)
        got.update(dq=_back(dq), dk=_back(dk), dv=_back(dv))
    return got


def _run_bhsd(dev, inp, kb, causal, p):
    q, k, v = (inp[n].to(dev).requires_grad_() for n in ("q", "k", "v"))
    ops.manual_seed(SEED)
    o = ops.attention(q, k, v, kb.to(dev) if kb is not None else None, p=p, scale=SCALE, causal=causal)
    o.backward(inp["do"].to(dev))
    return {"o": o.detach().cpu(), "dq": q.grad.cpu(), "dk": k.grad.cpu(), "dv": v.grad.cpu()}


def _run_packed(dev, inp, kb, causal, p):
    B, H, S, _ = inp["q"].shape
    qkv = torch.stack([inp[n].permute(0, 2, 1, 3) for n in ("q", "k", "v")], 2)      # [B, S, 3, H, 64]
    qkv = qkv.reshape(B, S, 3 * H * D).to(dev).requires_grad_()
    ops.manual_seed(SEED)
    o = ops.attention_packed(qkv, H, kb.to(dev) if kb is not None else None, p=p, training=True, scale=SCALE,
                             causal=causal)
    o.backward(inp["do"].permute(0, 2, 1, 3).reshape(B, S, H * D).to(dev))
    g = qkv.grad.view(B, S, 3, H, D).permute(2, 0, 3, 1, 4).cpu()
    return {"o": o.detach().view(B, S, H, D).permute(0, 2, 1, 3).cpu(), "dq": g[0], "dk": g[1], "dv": g[2]}


# ------------------------------------------------------------------ 2. default dispatch
@pytest.mark.gpu
@pytest.mark.parametrize("case", _cases(SHAPES), ids=_id)
def test_default_dispatch(cuda, case):
    """ops.attention (any Sq, Sk) and, for self-attention shapes, ops.attention_packed against the
    fp64 reference, plus lse from the direct attn_fwd call the autograd functions make."""
    Sq, Sk, causal, p, bias = case
    inp, kb, keep, (seed, off), want = _expected(case)
    _check(_run_direct(cuda, inp, kb, causal, p, seed, off), want, kb, "direct " + _id(case), causal, p)
    _check(_run_bhsd(cuda, inp, kb, causal, p), want, kb, "bhsd " + _id(case), causal, p)
    if Sq == Sk:
        _check(_run_packed(cuda, inp, kb, causal, p), want, kb, "packed " + _id(case), causal, p)


@pytest.mark.gpu
@pytest.mark.parametrize("Sq,Sk", [(96, 63), (128, 129)])
def test_odd_sk_dropout_routes_to_reference(cuda, Sq, Sk):
    """p > 0 with odd Sk: the kernel refuses (rc -2) and the wrapper computes exactly what
    ops.reference.attention computes with the stream it drew."""
    inp = _inputs(B0, H0, Sq, Sk)
    C = ops.require_native()
    q, k, v = (_bshd(inp[n], cuda) for n in ("q", "k", "v"))
    o = torch.zeros_like(q)
    with pytest.raises(RuntimeError, match="rc=-2"):
        C.attn_fwd(q, k, v, o, None, SCALE, 0.1, SEED, 0, False)
    assert not o.any()
    qd, kd, vd = (inp[n].to(cuda) for n in ("q", "k", "v"))
    ops.manual_seed(SEED)
    got = ops.attention(qd, kd, vd, p=0.1, scale=SCALE)
    ops.manual_seed(SEED)
    seed, off = ops._rng.next(B0 * H0 * Sq * Sk)
    assert torch.equal(got, ref.attention(qd, kd, vd, None, 0.1, seed, off, SCALE))


# ------------------------------------------------------------------ 3. views, padding, refusals
SENTINEL = 0x7FA5      # a bf16 NaN bit pattern no kernel produces
# head strides of the padded-view tests: all different, multiples of 8 (16-byte rows), none 64
PAD_HS = {"q": 72, "k": 80, "v": 88, "do": 96, "o": 104, "dq": 112, "dk": 120, "dv": 136}


def _padded(dev, B, S, H, hs, fill_bits=SENTINEL, data=None):
    """A [B, S, H, 64] view into a larger buffer: 3 extra rows after S, head stride hs (a multiple
    of 8, not 64), a 16-element gap between batches, an 8-element (16-byte) offset from the base.
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


def _untouched(buf, mask, bits=SENTINEL):
    return bool((buf.view(torch.int16)[~mask] == bits).all())


@pytest.mark.gpu
@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("Sq,Sk", [(100, 72), (160, 264)])
def test_padded_views_write_nothing_outside(cuda, Sq, Sk, causal):
    """Every tensor is a padded view (rows after S, gaps between heads and batches); the inputs'
    padding is NaN, the outputs' a sentinel that must survive bit for bit.  The eight tensors have
    eight different head strides (PAD_HS), hence eight different stride triples: a launch that
    takes one tensor's strides for another's reads NaN padding or writes over a sentinel."""
    case = (Sq, Sk, causal, 0.1, "present")
    inp, kb, keep, (seed, off), want = _expected(case)
    C = ops.require_native()
    nan = 0x7FC0
    t = {}
    for n, S in (("q", Sq), ("k", Sk), ("v", Sk), ("do", Sq)):
        _, t[n], _ = _padded(cuda, B0, S, H0, PAD_HS[n], nan, inp[n].to(cuda).transpose(1, 2))
    out = {n: _padded(cuda, B0, S, H0, PAD_HS[n]) for n, S in (("o", Sq), ("dq", Sq), ("dk", Sk), ("dv", Sk))}
    kbd = kb.to(cuda)
    lse = C.attn_fwd(t["q"], t["k"], t["v"], out["o"][1], kbd, SCALE, 0.1, seed, off, causal)
    C.attn_bwd(t["q"], t["k"], t["v"], out["o"][1], t["do"], out["dq"][1], out["dk"][1], out["dv"][1], kbd, lse,
               SCALE, 0.1, seed, off, causal)
    torch.cuda.synchronize()
    for n, (buf, _, mask) in out.items():
        assert _untouched(buf, mask), "%s: written outside its valid region" % n
    got = {n: _back(view) for n, (_, view, _) in out.items()}
    got["lse"] = lse.view(B0, H0, Sq).cpu()
    _check(got, want, kb, "padded " + _id(case), causal, 0.1)


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["misaligned", "odd_stride"])
def test_unaligned_dq_takes_scalar_stores(cuda, how):
    """dq, unlike o / dk / dv, may sit at any 2-byte offset: a base that is not 16-byte aligned
    or a stride that is no multiple of 8 sends every tile of a single key block (full ones too:
    Sq = 64) through the scalar dQ stores.  Same bounds, nothing written outside."""
    case = (64, 72, True, 0.1, "present")
    Sq, Sk, causal, p, _ = case
    inp, kb, keep, (seed, off), want = _expected(case)
    C = ops.require_native()
    q, k, v, do = (_bshd(inp[n], cuda) for n in ("q", "k", "v", "do"))
    kbd = kb.to(cuda)
    o = torch.empty_like(q)
    lse = C.attn_fwd(q, k, v, o, kbd, SCALE, p, seed, off, causal)
    hs, base = (64, 4) if how == "misaligned" else (68, 0)
    ss = H0 * hs
    sb = Sq * ss + 12
    buf = torch.full((base + B0 * sb + 8,), SENTINEL, dtype=torch.int16, device=cuda).view(torch.bfloat16)
    geom = ((B0, Sq, H0, D), (sb, ss, hs, 1), base)
    dq = buf.as_strided(*geom)
    mask = torch.zeros(buf.numel(), dtype=torch.bool, device=cuda)
    mask.as_strided(*geom).fill_(True)
    dk, dv = torch.empty_like(k), torch.empty_like(v)
    C.attn_bwd(q, k, v, o, do, dq, dk, dv, kbd, lse, SCALE, p, seed, off, causal)
    torch.cuda.synchronize()
    assert _untouched(buf, mask)
    got = {"o": _back(o), "lse": lse.view(B0, H0, Sq).cpu(), "dq": _back(dq), "dk": _back(dk), "dv": _back(dv)}
    _check(got, want, kb, "unaligned dq " + how, causal, p)


@pytest.mark.gpu
@pytest.mark.parametrize("Sq,Sk", [(100, 72), (160, 264)])
def test_fully_masked_rows(cuda, Sq, Sk):
    """-inf on every key of batch 0: O == 0, lse == +inf, zero gradients there; batch 1 matches
    the reference.  One single-key-block shape and one MULTI shape."""
    case = (Sq, Sk, False, 0.0, "inf0")
    inp, kb, _, _, want = _expected(case)
    got = _run_direct(cuda, inp, kb, False, 0.0, 0, 0)
    assert (got["o"][0] == 0).all()
    assert (got["lse"][0] == float("inf")).all()
    for n in ("dq", "dk", "dv"):
        assert torch.isfinite(got[n].float()).all(), n
        assert (got[n][0] == 0).all(), n
    _check({n: t[1:] for n, t in got.items()}, {n: t[1:] for n, t in want.items()}, None, "masked " + _id(case))
    bh = _run_bhsd(cuda, inp, kb, False, 0.0)
    assert (bh["o"][0] == 0).all() and (bh["dq"][0] == 0).all()
    _check({n: t[1:] for n, t in bh.items()}, {n: t[1:] for n, t in want.items()}, None, "masked bhsd " + _id(case))


def _small(dev, Sq=40, Sk=40):
    inp = _inputs(B0, H0, Sq, Sk)
    return tuple(_bshd(inp[n], dev) for n in ("q", "k", "v", "do"))


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["misaligned", "odd_stride"])
def test_forward_refuses_unaligned_output(cuda, how):
    """The forward's 16-byte stores need a 16-byte aligned o with strides that are multiples of 8."""
    C = ops.require_native()
    q, k, v, _ = _small(cuda)
    buf = torch.full((8 + B0 * 40 * H0 * 68,), SENTINEL, dtype=torch.int16, device=cuda).view(torch.bfloat16)
    if how == "misaligned":
        o = buf.as_strided((B0, 40, H0, D), (40 * H0 * 64, H0 * 64, 64, 1), 4)
    else:
        o = buf.as_strided((B0, 40, H0, D), (40 * H0 * 68, H0 * 68, 68, 1), 0)
    with pytest.raises(RuntimeError, match="rc=-7"):
        C.attn_fwd(q, k, v, o, None, SCALE, 0.0, 0, 0, False)
    rel = torch.zeros(H0, 79, device=cuda)
    with pytest.raises(RuntimeError, match="rc=-7"):
        C.attn_fwd_relbias(q, k, v, o, None, rel, 39, SCALE, False)
    torch.cuda.synchronize()
    assert bool((buf.view(torch.int16) == SENTINEL).all())


@pytest.mark.gpu
def test_relbias_refusals(cuda):
    """relb longer than the kernel's LDS vector (4096), and relb that does not cover every
    (key - query) offset, raise and write nothing."""
    C = ops.require_native()
    q, k, v, _ = _small(cuda)
    o = torch.full_like(q, float("nan"))
    o.view(torch.int16).fill_(SENTINEL)
    with pytest.raises(RuntimeError, match="rc=-4"):
        C.attn_fwd_relbias(q, k, v, o, None, torch.zeros(H0, 4097, device=cuda), 39, SCALE, False)
    with pytest.raises(RuntimeError, match="does not cover"):
        C.attn_fwd_relbias(q, k, v, o, None, torch.zeros(H0, 79, device=cuda), 38, SCALE, False)   # rel_base < Sq - 1
    with pytest.raises(RuntimeError, match="does not cover"):
        C.attn_fwd_relbias(q, k, v, o, None, torch.zeros(H0, 78, device=cuda), 39, SCALE, False)   # rel_base + Sk > L
    torch.cuda.synchronize()
    assert bool((o.view(torch.int16) == SENTINEL).all())


_BAD_KB = {
    "bf16": lambda kb: kb.bfloat16(),
    "cpu": lambda kb: kb.cpu(),
    "longer": lambda kb: torch.cat([kb, kb[:, :1]], 1),
    "one_batch": lambda kb: kb[:1],
    "flat": lambda kb: kb.reshape(-1),
    "strided": lambda kb: torch.cat([kb, kb], 1)[:, ::2],
}
_BAD_LSE = {
    "fp64": lambda l: l.double(),
    "cpu": lambda l: l.cpu(),
    "strided": lambda l: torch.cat([l, l], 1)[:, ::2],
    "short": lambda l: l[:-1],
}


def _bwd_refusal(dev, kb_fn=None, lse_fn=None):
    C = ops.require_native()
    q, k, v, do = _small(dev)
    kb = torch.zeros(B0, 40, device=dev)
    o = torch.empty_like(q)
    lse = C.attn_fwd(q, k, v, o, kb, SCALE, 0.0, 0, 0, False)
    outs = [torch.empty_like(q) for _ in range(3)]
    for t in outs:
        t.view(torch.int16).fill_(SENTINEL)
    with pytest.raises(RuntimeError):
        C.attn_bwd(q, k, v, o, do, outs[0], outs[1], outs[2], kb_fn(kb) if kb_fn else kb,
                   lse_fn(lse) if lse_fn else lse, SCALE, 0.0, 0, 0, False)
    torch.cuda.synchronize()
    for t in outs:
        assert bool((t.view(torch.int16) == SENTINEL).all())
    C.attn_bwd(q, k, v, o, do, outs[0], outs[1], outs[2], kb, lse, SCALE, 0.0, 0, 0, False)   # the good call runs
    assert all(torch.isfinite(t.float()).all() for t in outs)


@pytest.mark.gpu
@pytest.mark.parametrize("bad", sorted(_BAD_KB))
def test_backward_refuses_bad_key_bias(cuda, bad):
    """attn_bwd checks key_bias as attn_fwd does: fp32, on the device, [B, Sk], unit last stride."""
    _bwd_refusal(cuda, kb_fn=_BAD_KB[bad])


@pytest.mark.gpu
@pytest.mark.parametrize("bad", sorted(_BAD_LSE))
def test_backward_refuses_bad_lse(cuda, bad):
    """attn_bwd checks lse: fp32, on the device, contiguous, B * H * Sq values."""
    _bwd_refusal(cuda, lse_fn=_BAD_LSE[bad])


# ------------------------------------------------------------------ 4. relative-bias forward
@pytest.mark.gpu
@pytest.mark.parametrize("bias", ["none", "present"])
@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("Sq,Sk", REL_SHAPES)
def test_relbias_forward(cuda, Sq, Sk, causal, bias):
    """attn_fwd_relbias (rel_base = Sq - 1, L = Sq + Sk - 1), o and lse per row."""
    inp, kb, rel, relm, want = _expected_rel(Sq, Sk, causal, bias)
    C = ops.require_native()
    q, k, v = (_bshd(inp[n], cuda) for n in ("q", "k", "v"))
    o = torch.empty_like(q)
    lse = C.attn_fwd_relbias(q, k, v, o, kb.to(cuda) if kb is not None else None, rel.to(cuda), Sq - 1, SCALE, causal)
    tag = "rel %dx%d %s %s" % (Sq, Sk, "causal" if causal else "full", bias)
    _check({"o": _back(o), "lse": lse.view(B0, H0, Sq).cpu()}, want, None, tag)
    front = ops.attention_relbias(q, k, v, rel.to(cuda), Sq - 1, kb.to(cuda) if kb is not None else None,
                                  scale=SCALE, causal=causal)
    assert torch.equal(front, o)


# ------------------------------------------------------------------ 5. non-default kernels
_VARIANT_CASES = [c for c in _cases(VARIANT_SHAPES, ("present",))]


@pytest.mark.gpu
@pytest.mark.parametrize("case", _VARIANT_CASES, ids=_id)
def test_variant_subset(cuda, case):
    """One shape per row of the table, causal x p: the subset that the child processes below
    re-run under each kernel-selecting variable (here it runs the default kernels)."""
    Sq, Sk, causal, p, bias = case
    inp, kb, keep, (seed, off), want = _expected(case)
    _check(_run_direct(cuda, inp, kb, causal, p, seed, off), want, kb, "variant " + _id(case), causal, p)


@pytest.mark.gpu
@pytest.mark.parametrize("causal,p", [(False, 0.1), (True, 0.0)], ids=["full-p0.1", "causal-p0"])
def test_variant_persistent_walk(cuda, causal, p):
    """More work items than the persistent forward has resident slots (B * H * ceil(Sq / 128) >
    2 x CUs), so under CLOUDTIK_AMD_ATTN_FWD_PIPE=1 every workgroup walks several items and hands
    the next item's Q over; B 9, H 32, Sq 200, Sk 72 on 256 CUs is 576 items."""
    cus = torch.cuda.get_device_properties(cuda).multi_processor_count
    H, Sq, Sk = 32, 200, 72
    B = (2 * cus) // (2 * H) + 1
    assert B * H * 2 > 2 * cus
    inp, kb, keep, (seed, off), want = _expected((Sq, Sk, causal, p, "present"), B, H)
    got = _run_direct(cuda, inp, kb, causal, p, seed, off, backward=False)
    _check(got, want, None, "walk B%d %s p%g" % (B, "causal" if causal else "full", p))


def _dispatch_names():
    """The kernel instantiations ct_attn_fwd / ct_attn_bwd pick for DROP, CAUSAL under this
    process's variables: (forward, {(Sq, Sk): backward})."""
    def env(name, default):
        return int(os.environ.get("CLOUDTIK_AMD_ATTN_" + name, default))
    gl, wpe, bgl = env("FWD_GLDS", 1), env("FWD_WPE", 0), env("BWD_GL", 1)
    if env("FWD_PIPE", 0):
        fwd = "attn_fwd_pipe_kernel<true, true>"
    else:
        if not 1 <= wpe <= 4:
            wpe = 3 if gl else 2
        wpe = wpe if wpe in ((3, 4) if gl else (1, 3)) else 2
        fwd = "attn_fwd_d64_kernel<true, true, false, %d, %s>" % (wpe, "true" if gl else "false")
    bwd = "attn_bwd_d64_kernel<true, true, %s, %s>"
    return fwd, {(64, 72): bwd % ("false", "true" if bgl else "false"),     # one key block, Sq <= 128
                 (160, 72): bwd % ("false", "false"),                        # one key block, Sq > 128
                 (160, 264): bwd % ("true", "false")}                        # MULTI


@pytest.mark.gpu
def test_variant_kernels_selected(cuda):
    """The kernels that actually ran, by name from the profiler, are the ones the dispatcher is
    documented to pick under this process's variables -- so a child process below cannot pass by
    quietly running the default kernels."""
    from torch.profiler import ProfilerActivity, profile
    fwd, bwds = _dispatch_names()
    for (Sq, Sk), bwd in bwds.items():
        inp = _inputs(B0, H0, Sq, Sk)
        _run_direct(cuda, inp, None, True, 0.1, SEED, 0)                     # warm: module load, allocations
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            _run_direct(cuda, inp, None, True, 0.1, SEED, 0)
            torch.cuda.synchronize()
        names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "attn_" in e.name]
        assert any(fwd in n for n in names), (Sq, Sk, fwd, names)
        assert any(bwd in n for n in names), (Sq, Sk, bwd, names)
        assert sum("attn_fwd" in n for n in names) == 1 and sum("attn_bwd" in n for n in names) == 1, names
        assert any("attn_dq_convert_kernel" in n for n in names) == (Sk > 128), names


_VARIANTS = [
    {"CLOUDTIK_AMD_ATTN_FWD_GLDS": "0"},
    {"CLOUDTIK_AMD_ATTN_FWD_WPE": "2"},
    {"CLOUDTIK_AMD_ATTN_BWD_GL": "0"},
    {"CLOUDTIK_AMD_ATTN_FWD_PIPE": "1"},
    {"CLOUDTIK_AMD_ATTN_FWD_PIPE": "1", "CLOUDTIK_AMD_ATTN_PERSIST": "0"},
]


@pytest.mark.gpu
@pytest.mark.parametrize("knobs", _VARIANTS, ids=lambda d: ",".join("%s=%s" % (k[18:], v) for k, v in d.items()))
def test_nondefault_kernels_in_child_process(cuda, knobs):
    """The kernels selected by environment variable -- the register-staged forward, the previous
    2-waves default, the register-staged backward, the persistent forward in both grid shapes --
    on the variant subset above, in a child process with the variables set (the library reads
    them once per process)."""
    env = {k: v for k, v in os.environ.items() if not k.startswith("CLOUDTIK_AMD_ATTN_")}
    env.update(knobs)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-s", __file__, "-m", "gpu", "-k", "test_variant_",
                        "-p", "no:cacheprovider"], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and "skipped" not in r.stdout, r.stdout[-2000:]
    worst = {}
    for line in r.stdout.splitlines():
        if "attn-err " in line:
            for kv in line.split():
                if "=" in kv:
                    n, e = kv.split("=")
                    worst[n] = max(worst.get(n, 0.0), float(e))
    print("attn-err-child %s %s" % (knobs, " ".join("%s=%.3e" % kv for kv in sorted(worst.items()))))
