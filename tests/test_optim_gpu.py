"""Fused optimizer kernels (ops/csrc/optim.hip: LAMB stage 1 / 2, Adam / AdamW, SGD, sumsq_into,
clip_coef): per-element and per-tensor fp64 checks on every dispatch path, segment-table shape
and option; the CPU paths of train/optim.py and ``FlatParamSpace._build_segments`` beside them.

REFERENCE.  ``_lamb_stage1`` / ``_lamb_stage2``, ``_adam``, ``_sgd``, ``_sumsq`` and ``_clip`` are plain
PyTorch transcriptions of the update rules, parameterised by a dtype ``dt``; ``dt = F64`` is the
reference.  They read the same fp32 / bf16 tensors the kernel gets (gradients, state, the
per-tensor weight decay and the ``dyn`` vector) and call nothing of cloudtik_amd.train.optim.  The
fp64 ``_adam`` / ``_sgd`` are pinned to ``torch.optim.Adam`` / ``AdamW`` / ``SGD`` run in fp64 (1e-12), and
``FusedLAMB._step_torch`` (pinned to the reference LAMB in test_model_parity.py) is held to ``_lamb``.
The kernels are called through the bindings (``C.lamb_step`` ...), with segment tables and ``dyn``
built here; a second group goes through ``FlatParamSpace`` + ``FusedLAMB`` / ``FusedAdam`` /
``FusedSGD``, on the GPU and on the CPU path.

METRIC.  Per tensor, worst element; tensors are never pooled (the printed figures are one per
tensor, ``a/b/c``).
* ``m``, ``v``, ``buf``: |k - ref| / (sum of |terms| of that element + 1e-3 x the tensor's largest such
  sum), the terms being beta x old, (1 - beta) x g x scale and, where decay enters the gradient,
  (1 - beta) x wd x w.  The moments cancel, so |ref| is no scale for them.
* fp32 ``w``: |k - ref| / (|w_old| + |applied update of the reference|), elementwise.
* LAMB ``tensor_part`` after stage 1 (per tensor ||w||^2, ||u||^2) and ``sumsq_into`` (the previous
  value of ``out`` among the terms): |k - ref| / ref; all terms are positive.
* ``clip_coef``: ``dyn[1]`` relative.

BOUNDS.  Not taken from a kernel.  The same functions with ``dt = F32`` are a CPU model that rounds
only where the kernels round: fp32 ``m``, ``v``, ``w``, ``buf``, sums (per segment, then per tensor) and
``dyn``, the hyper-parameters as fp32 kernel arguments; bf16 only for the model copy and for bf16
gradients on input.  Its worst error against the fp64 reference over the whole case matrix below
(measured on a CPU) and the bound, 4 x that (summation order, fused multiply-add contraction,
``sqrtf``):

    | quantity                                   | model worst | bound (4 x) |
    |--------------------------------------------|-------------|-------------|
    | ``lamb_m``: LAMB exp_avg                     | 1.55e-07    | 6.20e-07    |
    | ``lamb_v``: LAMB exp_avg_sq                  | 2.87e-07    | 1.15e-06    |
    | ``lamb_part``: LAMB per-tensor sums          | 1.74e-07    | 6.96e-07    |
    | ``lamb_w``: LAMB fp32 weights                | 2.26e-06    | 9.04e-06    |
    | ``adam_m``: Adam exp_avg                     | 1.57e-07    | 6.28e-07    |
    | ``adam_v``: Adam exp_avg_sq                  | 3.20e-07    | 1.28e-06    |
    | ``adam_w``: Adam fp32 weights                | 2.60e-05    | 1.04e-04    |
    | ``sgd_buf``: SGD momentum buffer             | 1.43e-07    | 5.72e-07    |
    | ``sgd_w``: SGD fp32 weights                  | 1.28e-06    | 5.12e-06    |
    | ``sumsq``: sumsq_into                        | 1.15e-07    | 4.60e-07    |
    | ``clip``: clip_coef dyn[1]                   | 4.63e-08    | 1.85e-07    |

Hyper-parameters put the applied update at roughly 0.3 .. 30 % of |w| for most elements (lr 0.05,
gradients ~0.1, moments ~0.05, weights ~0.5), so a trust ratio or a decay that is 1 % off sits two
orders of magnitude above the ``w`` bounds.  ``test_rounding_model_meets_bounds`` re-runs the model.
The hyper-parameters (betas, eps, momentum, dampening, max_norm) are fp32 kernel arguments, and the
reference takes them as such: ``1.f - 0.999f`` is 1.3e-5 from 0.001, and the operation under test is
the one with the fp32 beta (the CPU paths of train/optim.py form 1 - beta the same way).
The ``w`` figures are set by a few ill-conditioned elements out of millions (the model's median
element is at 2e-8): the scale |w_old| + |update| does not hold the terms that cancel inside the
update.  ``lamb_w``, ``sgd_w``: the momentum terms (beta x m and (1 - beta) x g; g and momentum x buf)
cancel to ~1 % of their size at an element whose weight is ~1e-5.  ``adam_w``: the first L2 step from
zero state is lr x gr / (|gr| + eps') with gr = g x scale + wd x w; where these two cancel (0.00499795
- 0.00499825) the rounding of gr is divided by a denominator of ~1e-6.

EXACT RESULTS (``torch.equal``).
* The model copy (bf16 or fp32) equals the kernel's own fp32 ``w`` after the step converted to its
  dtype (round to nearest even), at every element of every segment.
* Every element of ``w``, ``w_model``, ``m``, ``v``, ``buf`` outside the segments -- a 64-element margin
  before and after each buffer, one 64-element gap between two tensors, the range of a tensor
  without a segment -- keeps its bits; ``g`` is never written; a buffer the call does not take
  (``buf`` at momentum 0: ``None`` is passed) cannot be written.
* LAMB stage 3 equals stage 1 then stage 2 in two calls, bit for bit.
* LAMB ratio exactly 1 (compared with a reference whose ratio is 1 by construction, finite): a
  tensor with wd 0 and trust_all 0; a tensor of zero weights; a tensor whose u is zero.
* ``clip_coef`` leaves ``dyn[0]``, ``dyn[2]``, ``dyn[3]`` bit-unchanged; ``sumsq_into`` of zeros adds
  exactly 0.

CASE MATRIX.
* Segment tables (``LAYOUTS``), shared by the three optimizers: tensors of padded lengths 64, 128,
  8192, 8192 + 64, 3 x 8192, 65 x 8192 + 64 in one flat space, the first T of them for T in {1, 3,
  4, 5, 6} (blocks of 4 tensors in ``seg_to_tensor_kernel`` with and without a partial last block;
  at T 6 a tensor of 66 segments wraps its lane loop), T >= 5 with a 64-element gap that no
  segment covers; ``T5-empty``: tensor 3 without a segment; ``rank0`` / ``rank1``: the shard-local
  tables of two ranks that own alternate 4096-element pieces of the T 5 space (ZeRO-1 buckets of
  8192 and a last one of 128), rank 1 without a segment for tensors 0 and 1.  Every start and
  length is a multiple of 64; segments are at most 8192 long with short tails.
* LAMB: gradient {fp32, bf16} x model copy {none, fp32, bf16} x bias correction {off, on at step 1
  from zero state, on at step 7} x trust_all {0, 1} x ``dyn[1]`` {1, 0.37}: all 72 on T5, every
  sixth on the other tables (each gradient / copy pair twice); wd per tensor 0.01 / 0 mixed.  The
  two-rank emulation (stage 1 per rank, the ``tensor_part`` s added, stage 2 per rank) against the
  unsharded reference, six combinations.
* Adam: adamw {0, 1} x gradient x model copy x step {1 from zero state, 7} x ``dyn[1]`` {1, 0.37}:
  all 48 on T5, every fourth elsewhere; zero gradient with zero state (adamw: m = v = 0 exactly
  and the update is the decay term).
* SGD: (momentum, dampening, nesterov) in {(0, 0, 0), (0.9, 0, 0), (0.9, 0.3, 0), (0.9, 0, 1)} x
  first {0, 1} x gradient x model copy x ``dyn[1]``: all 96 on T5, every eighth elsewhere.
* ``dyn`` read on the device: each optimizer called twice with ``dyn`` rewritten (lr halved) between.
* ``sumsq_into``: n in {4, 252, 1024, 1028, 4 x (2048 x 256 + 3)} x {fp32, bf16}, ``out`` preset, two
  calls into one ``out``, all-zero input.  ``clip_coef``: norm below / equal to / above max_norm,
  sumsq 0, base_scale {1, 1/8}.
* End to end (``E2E``): three parameters (24 x 16, 24, 24) in bf16 and fp32 through ``FlatParamSpace``
  for 3 steps, each step compared with the reference applied to the state before it:
  ``FusedLAMB(max_grad_norm=1)`` clipping at step 1 and not at step 3, with grad_scale 1 and 0.25;
  LAMB with trust_all and bias correction; ``FusedAdam(adamw=False)``; AdamW with grad_scale 0.25;
  ``FusedSGD(nesterov=True)``; ``FusedSGD(dampening=0.3)`` with grad_scale 0.25; SGD without momentum.
* ``_build_segments``: numels {1, 63, 64, 65, 8192, 8193, 64 x 8192 + 1}, world 1..4, plain shards
  and ZeRO-1 pieces.

KERNEL INSTANTIATIONS -> CASES.
* ``lamb_stage1_kernel<float / unsigned short>`` (fp32 / bf16 gradient), ``lamb_stage2_kernel<float /
  unsigned short>`` (no or fp32 copy / bf16 copy; ``w_model == nullptr``: no copy),
  ``seg_to_tensor_kernel``: ``test_variant_lamb*`` in this process.
* ``lamb_stage1_v8_kernel<.>``, ``lamb_stage2_v8_kernel<.>``: the same tests in the child process with
  ``CLOUDTIK_AMD_LAMB_V8=1`` (``test_nondefault_kernels_in_child_process``); a bf16 gradient that starts
  4 elements (8 bytes) into its buffer takes the 4-wide kernels there too
  (``test_variant_lamb_offset_gradient``).
* ``adam_kernel<GT, PT>``, ``sgd_kernel<GT, PT>``, GT, PT in {float, unsigned short}: ``test_adam``,
  ``test_sgd`` (PT = float with ``w_model == nullptr`` and with an fp32 copy).
* ``sumsq_kernel<float / unsigned short>`` (the grid-stride loop at n = 4 x (2048 x 256 + 3)),
  ``sumsq_finish_kernel``: ``test_sumsq``; ``clip_coef_kernel``: ``test_clip_coef``.
* ``test_variant_kernels_selected`` reads the kernel names from the profiler in this process and in
  the child and compares them with the rules of ``ct_lamb`` / ``ct_adam`` / ``ct_sgd`` / ``ct_sumsq``.
"""
import functools
import itertools
import os
import subprocess
import sys
import types
import zlib

import pytest
import torch

from cloudtik_amd import ops

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
MARGIN = 64          # canary elements before and after every flat buffer
GAP = 64             # uncovered elements between two tensors
SEG = 8192
LENS = (64, 128, 8192, 8192 + 64, 3 * 8192, 65 * 8192 + 64)
WD = (0.01, 0.0, 0.01, 0.0, 0.01, 0.01)
LR = 0.05

# worst error of the F32 model against the F64 reference over the whole matrix (module docstring)
MODEL_WORST = {
    "lamb_m": 1.55e-07,
    "lamb_v": 2.87e-07,
    "lamb_part": 1.74e-07,
    "lamb_w": 2.26e-06,
    "adam_m": 1.57e-07,
    "adam_v": 3.20e-07,
    "adam_w": 2.60e-05,
    "sgd_buf": 1.43e-07,
    "sgd_w": 1.28e-06,
    "sumsq": 1.15e-07,
    "clip": 4.63e-08,
}
BOUND = {k: 4.0 * v for k, v in MODEL_WORST.items()}


def HP(**kw):
    d = dict(b1=0.9, b2=0.999, eps=1e-6, bias_corr=False, trust_all=False, adamw=True, momentum=0.0,
             dampening=0.0, nesterov=False, max_grad_norm=None)
    d.update(kw)
    return types.SimpleNamespace(**d)


# ------------------------------------------------------------------ segment tables
class Layout:
    """A flat space of ``n`` elements and a segment table over it.  ``segs``: (tensor, start, len),
    grouped by tensor in tensor order; ``gidx``: for a rank's shard-local table, the index of each
    local element in the unsharded space."""

    def __init__(self, name, n, T, segs, gidx=None):
        self.name, self.n, self.T, self.segs, self.gidx = name, n, T, segs, gidx
        assert [t for t, _, _ in segs] == sorted(t for t, _, _ in segs)
        self.first = [sum(1 for t, _, _ in segs if t < k) for k in range(T + 1)]
        tid = torch.full((n,), -1, dtype=torch.long)
        for t, s, l in segs:
            assert s % 64 == 0 and l % 64 == 0 and 0 < l <= SEG and 0 <= s and s + l <= n
            assert (tid[s:s + l] == -1).all()
            tid[s:s + l] = t
        self._tid = tid
        self._dev = {}

    def on(self, dev):
        key = str(dev)
        if key not in self._dev:
            i32 = lambda v: torch.tensor(v or [0], dtype=torch.int32, device=dev)  # noqa: E731
            tid = self._tid.to(dev)
            self._dev[key] = types.SimpleNamespace(
                seg_tensor=i32([t for t, _, _ in self.segs]),
                seg_start=torch.tensor([s for _, s, _ in self.segs], dtype=torch.int64, device=dev),
                seg_len=i32([l for _, _, l in self.segs]),
                first=torch.tensor(self.first, dtype=torch.int32, device=dev),
                tid=tid, cov=tid >= 0, tid0=tid.clamp_min(0),
                idx=[(tid == t).nonzero().flatten() for t in range(self.T)])
        return self._dev[key]


def _split(t, a, b, shift=0):
    return [(t, shift + s, min(SEG, b - s)) for s in range(a, b, SEG)]


def _plain(name, lens, gap_after=None, empty=None):
    segs, off = [], 0
    for t, n in enumerate(lens):
        if t != empty:
            segs += _split(t, off, off + n)
        off += n + (GAP if t == gap_after else 0)
    return Layout(name, off, len(lens), segs)


def _rank_layouts(lens, world=2, cap=8192):
    """The unsharded table and one shard-local table per rank: buckets of ``cap`` elements (the last
    one shorter), rank r owns chunk r of each, packed back to back -- the 64-aligned pieces
    GradBucketer._build_uniform_buckets makes."""
    total = sum(lens)
    assert total % (64 * world) == 0 and cap % (64 * world) == 0
    offs = [sum(lens[:t]) for t in range(len(lens))]
    out = [_plain("T%d-global" % len(lens), lens)]
    for r in range(world):
        pieces, lo, loc = [], 0, 0
        while lo < total:
            hi = min(lo + cap, total)
            c = (hi - lo) // world
            pieces.append((lo + r * c, lo + (r + 1) * c, loc))
            loc, lo = loc + c, hi
        segs = []
        for t, (o, n) in enumerate(zip(offs, lens)):
            for plo, phi, ploc in pieces:
                a, b = max(o, plo), min(o + n, phi)
                if a < b:
                    segs += _split(t, a, b, ploc - plo)
        gidx = torch.cat([torch.arange(plo, phi) for plo, phi, _ in pieces])
        out.append(Layout("rank%d" % r, loc, len(lens), segs, gidx))
    return out


@functools.lru_cache(None)
def _layouts():
    lays = [_plain("T%d" % T, LENS[:T], gap_after=1 if T >= 5 else None) for T in (1, 3, 4, 5, 6)]
    lays.append(_plain("T5-empty", LENS[:5], gap_after=1, empty=3))
    lays += _rank_layouts(LENS[:5])[1:]
    return {l.name: l for l in lays}


LAYOUTS = ("T1", "T3", "T4", "T5", "T6", "T5-empty", "rank0", "rank1")
FULL = "T5"          # the table that takes the whole option matrix


# ------------------------------------------------------------------ inputs
def _gen(tag):
    g = torch.Generator()
    g.manual_seed(zlib.crc32(tag.encode()))
    return g


@functools.lru_cache(None)
def _base(n, tag):
    """fp32 CPU buffers of n + 2 x MARGIN elements; the same values for every case of a table."""
    gen = _gen("optim-%s-%d" % (tag, n))
    r = lambda: torch.randn(n + 2 * MARGIN, generator=gen)  # noqa: E731
    return {"W": 0.5 * r(), "G": 0.1 * r(), "M": 0.05 * r(), "B": 0.3 * r(),
            "V": 0.01 * (0.25 + torch.rand(n + 2 * MARGIN, generator=gen))}


def _make(lay, dev, gdt=F32, wmdt=None, state="rand", dyn=(LR, 1.0, 1.0, 1.0), goff=0, base=None, wd=None):
    """Device buffers for one call.  ``x[k]`` (g, m, v, w, buf, wm): the views the kernel gets;
    ``x['full']``: the buffers with their margins; ``x['ref']``: clones the reference reads."""
    n = lay.n
    base = base or _base(n, lay.name)
    full = {k: v.clone() for k, v in base.items()}
    inner = slice(MARGIN, MARGIN + n)
    if state in ("zero", "zero-grad"):
        for k in ("M", "V", "B"):
            full[k][inner] = 0
    if state == "zero-grad":
        full["G"][inner] = 0
    full["G"] = torch.cat([full["G"], full["G"][:8]]).to(gdt)      # room for an offset view
    full["WM"] = full["W"].to(wmdt) if wmdt is not None else None
    full = {k: (v.to(dev) if v is not None else None) for k, v in full.items()}
    x = {"full": full, "goff": goff, "n": n,
         "wd": torch.tensor((wd or WD)[:lay.T], dtype=F32, device=dev),
         "dyn": torch.tensor(dyn, dtype=F32, device=dev)}
    _views(x, full)
    _snapshot(x)
    return x


def _views(x, full, into=None):
    n, goff = x["n"], x["goff"]
    into = x if into is None else into
    for k, name in (("W", "w"), ("M", "m"), ("V", "v"), ("B", "buf"), ("WM", "wm")):
        into[name] = full[k][MARGIN:MARGIN + n] if full[k] is not None else None
    into["g"] = full["G"][MARGIN + goff:MARGIN + goff + n]
    return into


def _snapshot(x):
    """Keep the current buffers as the reference's inputs (and as the 'before' of the bit checks)."""
    x["orig"] = {k: (v.clone() if v is not None else None) for k, v in x["full"].items()}
    x["ref"] = _views(x, x["orig"], {"wd": x["wd"], "dyn": x["dyn"].clone()})


def _dyn(step, gs, hp, lr=LR, first=None):
    if first is not None:                       # SGD: slot 2 is the first-step flag
        return (lr, gs, float(first), 1.0)
    return (lr, gs, 1.0 / (1.0 - hp.b1 ** step), 1.0 / (1.0 - hp.b2 ** step))


# ------------------------------------------------------------------ reference (dt = F64) / model (dt = F32)
def _sc(v, dt, dev):
    """A hyper-parameter as the kernel gets it: an fp32 argument (1 - float(0.999) is 1.3e-5 from
    0.001; the operation under test is the one with the fp32 beta)."""
    return torch.tensor(v, dtype=F32, device=dev).to(dt)


def _f32(v):
    return float(torch.tensor(v, dtype=F32))


def _tensor_sums(x, lay, dt):
    """Per-tensor sums of x as the kernels form them: one sum per segment, then one per tensor."""
    seg = [x[s:s + l].sum() for _, s, l in lay.segs]
    out = torch.zeros(lay.T, dtype=dt, device=x.device)
    for t in range(lay.T):
        a, b = lay.first[t], lay.first[t + 1]
        if b > a:
            out[t] = torch.stack(seg[a:b]).sum()
    return out


def _lamb_u(m, v, w, wd, dyn, hp, dt):
    one = _sc(1.0, dt, w.device)
    bc1, bc2 = (dyn[2], dyn[3]) if hp.bias_corr else (one, one)
    return (m * bc1) / ((v * bc2).sqrt() + _sc(hp.eps, dt, w.device)) + wd * w


def _lamb_stage1(x, lay, hp, dt):
    L = lay.on(x["w"].device)
    dev = x["w"].device
    g, m0, v0, w = (x[k].to(dt) for k in ("g", "m", "v", "w"))
    dyn, wd = x["dyn"].to(dt), x["wd"].to(dt)[L.tid0]
    b1, b2, one = _sc(hp.b1, dt, dev), _sc(hp.b2, dt, dev), _sc(1.0, dt, dev)
    gr = g * dyn[1]
    m1, m2 = b1 * m0, (one - b1) * gr
    v1, v2 = b2 * v0, (one - b2) * gr * gr
    m, v = m1 + m2, v1 + v2
    u = _lamb_u(m, v, w, wd, dyn, hp, dt)
    zero = torch.zeros_like(w)
    part = torch.stack([_tensor_sums(torch.where(L.cov, w * w, zero), lay, dt),
                        _tensor_sums(torch.where(L.cov, u * u, zero), lay, dt)], 1)
    return {"m": torch.where(L.cov, m, m0), "v": torch.where(L.cov, v, v0), "part": part,
            "m_terms": m1.abs() + m2.abs(), "v_terms": v1.abs() + v2.abs()}


def _lamb_stage2(x, m, v, part, lay, hp, dt, ratio_one=()):
    """``part`` [T, 2]: the per-tensor sums the ratio is taken from (stage 1's, or the sum over
    ranks).  ``ratio_one``: tensors whose ratio is 1 by construction (the exact-ratio cases)."""
    L = lay.on(x["w"].device)
    w = x["w"].to(dt)
    dyn, wdt = x["dyn"].to(dt), x["wd"].to(dt)
    u = _lamb_u(m.to(dt), v.to(dt), w, wdt[L.tid0], dyn, hp, dt)
    wn, un = part[:, 0].to(dt).sqrt(), part[:, 1].to(dt).sqrt()
    one = torch.ones_like(wn)
    ratio = torch.where((wn > 0) & (un > 0), wn / un, one)
    if not hp.trust_all:
        ratio = torch.where(wdt != 0, ratio, one)
    for t in ratio_one:
        ratio[t] = 1.0
    upd = (dyn[0] * ratio)[L.tid0] * u
    return {"w": torch.where(L.cov, w - upd, w), "upd": upd.abs(), "ratio": ratio}


def _adam(x, lay, hp, dt):
    dev = x["w"].device
    L = lay.on(dev)
    g, m0, v0, w = (x[k].to(dt) for k in ("g", "m", "v", "w"))
    dyn, wd = x["dyn"].to(dt), x["wd"].to(dt)[L.tid0]
    b1, b2, one = _sc(hp.b1, dt, dev), _sc(hp.b2, dt, dev), _sc(1.0, dt, dev)
    gr = g * dyn[1]
    mass = gr.abs()
    if not hp.adamw:
        mass = mass + (wd * w).abs()
        gr = gr + wd * w
    m1, m2 = b1 * m0, (one - b1) * gr
    v1, v2 = b2 * v0, (one - b2) * gr * gr
    m, v = m1 + m2, v1 + v2
    upd = (m * dyn[2]) / ((v * dyn[3]).sqrt() + _sc(hp.eps, dt, dev))
    if hp.adamw:
        upd = upd + wd * w
    upd = dyn[0] * upd
    return {"m": torch.where(L.cov, m, m0), "v": torch.where(L.cov, v, v0), "w": torch.where(L.cov, w - upd, w),
            "upd": upd.abs(), "m_terms": m1.abs() + (one - b1) * mass, "v_terms": v1.abs() + v2.abs()}


def _sgd(x, lay, hp, dt):
    """PyTorch's rule; the first step (buf = g) is flagged by dyn[2] != 0."""
    dev = x["w"].device
    L = lay.on(dev)
    g, w = x["g"].to(dt), x["w"].to(dt)
    dyn, wd = x["dyn"].to(dt), x["wd"].to(dt)[L.tid0]
    gr = g * dyn[1] + wd * w
    mass = (g * dyn[1]).abs() + (wd * w).abs()
    out = {}
    if hp.momentum != 0:
        b0 = x["buf"].to(dt)
        mom, damp, one = _sc(hp.momentum, dt, dev), _sc(hp.dampening, dt, dev), _sc(1.0, dt, dev)
        if bool(dyn[2] != 0):
            buf, terms = gr, mass
        else:
            buf, terms = mom * b0 + (one - damp) * gr, (mom * b0).abs() + (one - damp) * mass
        gr = gr + mom * buf if hp.nesterov else buf
        out.update(buf=torch.where(L.cov, buf, b0), buf_terms=terms)
    upd = dyn[0] * gr
    out.update(w=torch.where(L.cov, w - upd, w), upd=upd.abs())
    return out


def _sumsq(x, prev, dt):
    """prev + sum x^2; returns the result and the sum of the terms."""
    s = x.to(dt).pow(2).sum()
    return prev.to(dt) + s, prev.to(dt).abs() + s


def _clip(sumsq, base_scale, max_norm, dt):
    dev = sumsq.device
    bs = _sc(base_scale, dt, dev)
    norm = sumsq.to(dt).sqrt() * bs
    c = _sc(max_norm, dt, dev) / (norm + _sc(1e-6, dt, dev))
    return bs * torch.minimum(c, _sc(1.0, dt, dev))


# ------------------------------------------------------------------ metric
def _worst(e):
    """max that keeps a NaN (a NaN anywhere fails every bound)."""
    if e.numel() == 0:
        return 0.0
    return float("nan") if torch.isnan(e).any() else e.max().item()


def _err_terms(k, want, terms, lay):
    L = lay.on(k.device)
    d = (k.double() - want.double()).abs()
    out = []
    for idx in L.idx:
        tt = terms[idx].double()
        top = tt.max() if idx.numel() else 0
        out.append(_worst(d[idx] / (tt + 1e-3 * top) if top > 0 else d[idx]))
    return out


def _err_w(k, want, w_old, upd, lay):
    L = lay.on(k.device)
    d = (k.double() - want.double()).abs()
    e = d / (w_old.double().abs() + upd.double())
    e = torch.where(d == 0, torch.zeros_like(e), e)          # 0 / 0 where nothing moved
    return [_worst(e[idx]) for idx in L.idx]


def _err_rel(k, want):
    d = (k.double() - want.double()).abs()
    e = d / want.double().abs()
    return torch.where(d == 0, torch.zeros_like(e), e)


def _note(errs, key, per_tensor):
    n = max(len(per_tensor), len(errs.get(key, ())))
    old, new = (list(v) + [0.0] * (n - len(v)) for v in (errs.get(key, ()), per_tensor))
    errs[key] = [b if (b != b or b > a) else a for a, b in zip(old, new)]


def _top(v):
    return float("nan") if any(e != e for e in v) else max(v)


def _assert_bounds(errs, tag):
    print("optim-err %s %s" % (tag, " ".join("%s=%s" % (k, "/".join("%.2e" % e for e in v)) for k, v in sorted(errs.items()))))
    for k, v in errs.items():
        for t, e in enumerate(v):
            assert e <= BOUND[k], "%s: %s tensor %d worst error %.3e > bound %.3e" % (tag, k, t, e, BOUND[k])


def _gather(ref, lay):
    """A global-layout result seen from a rank (``lay.gidx``)."""
    if lay.gidx is None:
        return ref
    g = lay.gidx.to(next(iter(ref.values())).device)
    return {k: (v[g] if v.dim() == 1 and v.numel() > lay.T * 2 else v) for k, v in ref.items()}


# ------------------------------------------------------------------ exact checks on the kernels' buffers
def _check_bits(x, lay, wrote, tag):
    """Outside the segments nothing moved; buffers the call may not write did not move at all; the
    model copy is the fp32 result rounded to its dtype."""
    full, orig = x["full"], x["orig"]
    dev = full["W"].device
    cov = torch.zeros(lay.n + 2 * MARGIN, dtype=torch.bool, device=dev)
    cov[MARGIN:MARGIN + lay.n] = lay.on(dev).cov
    for k in ("W", "M", "V", "B", "WM"):
        if full[k] is None:
            continue
        if k in wrote:
            assert torch.equal(full[k][~cov], orig[k][~cov]), "%s: %s written outside the segments" % (tag, k)
        else:
            assert torch.equal(full[k], orig[k]), "%s: %s written" % (tag, k)
    assert torch.equal(full["G"], orig["G"]), "%s: the gradient was written" % tag
    if x["wm"] is not None:
        c = lay.on(dev).cov
        assert torch.equal(x["wm"][c], x["w"][c].to(x["wm"].dtype)), "%s: model copy != rounded fp32 weights" % tag
    for k in ("w", "m", "v", "buf"):
        assert torch.isfinite(x[k]).all(), "%s: %s not finite" % (tag, k)


# ------------------------------------------------------------------ kernel calls
def _k_lamb(x, lay, hp, stage=3, part=None):
    C = ops.require_native()
    L = lay.on(x["w"].device)
    seg_part = torch.full((2 * len(lay.segs) + 2,), -7.5, dtype=F32, device=x["w"].device)
    part = torch.full((2 * lay.T,), -7.5, dtype=F32, device=x["w"].device) if part is None else part
    C.lamb_step(x["g"], x["m"], x["v"], x["w"], x["wm"], L.seg_tensor, L.seg_start, L.seg_len, L.first, x["wd"],
                x["dyn"], hp.b1, hp.b2, hp.eps, hp.bias_corr, hp.trust_all, seg_part, part, stage)
    assert seg_part[-2:].eq(-7.5).all()
    return part


def _k_adam(x, lay, hp):
    L = lay.on(x["w"].device)
    ops.require_native().adam_step(x["g"], x["m"], x["v"], x["w"], x["wm"], L.seg_tensor, L.seg_start, L.seg_len,
                                   x["wd"], x["dyn"], hp.b1, hp.b2, hp.eps, hp.adamw)


def _k_sgd(x, lay, hp):
    L = lay.on(x["w"].device)
    ops.require_native().sgd_step(x["g"], x["buf"] if hp.momentum != 0 else None, x["w"], x["wm"], L.seg_tensor,
                                  L.seg_start, L.seg_len, x["wd"], x["dyn"], hp.momentum, hp.dampening, hp.nesterov)


# ------------------------------------------------------------------ one case = inputs, reference, kernel or model, errors
def _lamb_errors(errs, got, r1, r2, x, lay):
    _note(errs, "lamb_m", _err_terms(got["m"], r1["m"], r1["m_terms"], lay))
    _note(errs, "lamb_v", _err_terms(got["v"], r1["v"], r1["v_terms"], lay))
    _note(errs, "lamb_w", _err_w(got["w"], r2["w"], x["ref"]["w"], r2["upd"], lay))
    if "part" in got:
        _note(errs, "lamb_part", [_worst(e) for e in _err_rel(got["part"].view(-1, 2), r1["part"])])


def _lamb_case(lay, dev, run, errs, hp, gdt, wmdt, step, gs, goff=0, tag=""):
    x = _make(lay, dev, gdt, wmdt, "zero" if step == 1 else "rand", _dyn(step or 7, gs, hp), goff)
    r1 = _lamb_stage1(x["ref"], lay, hp, F64)
    r2 = _lamb_stage2(x["ref"], r1["m"], r1["v"], r1["part"], lay, hp, F64)
    if run == "kernel":
        part = _k_lamb(x, lay, hp)
        _check_bits(x, lay, {"W", "M", "V", "WM"}, tag)
        got = {"m": x["m"], "v": x["v"], "w": x["w"], "part": part}
    else:
        got = _lamb_stage1(x["ref"], lay, hp, F32)
        got.update(_lamb_stage2(x["ref"], got["m"], got["v"], got["part"], lay, hp, F32))
    _lamb_errors(errs, got, r1, r2, x, lay)


def _adam_case(lay, dev, run, errs, hp, gdt, wmdt, step, gs, state=None, tag=""):
    x = _make(lay, dev, gdt, wmdt, state or ("zero" if step == 1 else "rand"), _dyn(step, gs, hp))
    ref = _adam(x["ref"], lay, hp, F64)
    if run == "kernel":
        _k_adam(x, lay, hp)
        _check_bits(x, lay, {"W", "M", "V", "WM"}, tag)
        got = x
    else:
        got = _adam(x["ref"], lay, hp, F32)
    _note(errs, "adam_m", _err_terms(got["m"], ref["m"], ref["m_terms"], lay))
    _note(errs, "adam_v", _err_terms(got["v"], ref["v"], ref["v_terms"], lay))
    _note(errs, "adam_w", _err_w(got["w"], ref["w"], x["ref"]["w"], ref["upd"], lay))
    return x, ref


def _sgd_case(lay, dev, run, errs, hp, gdt, wmdt, first, gs, tag=""):
    x = _make(lay, dev, gdt, wmdt, "rand", _dyn(None, gs, hp, first=first))
    ref = _sgd(x["ref"], lay, hp, F64)
    if run == "kernel":
        _k_sgd(x, lay, hp)
        _check_bits(x, lay, {"W", "B", "WM"} if hp.momentum != 0 else {"W", "WM"}, tag)
        got = x
    else:
        got = _sgd(x["ref"], lay, hp, F32)
    if hp.momentum != 0:
        _note(errs, "sgd_buf", _err_terms(got["buf"], ref["buf"], ref["buf_terms"], lay))
    _note(errs, "sgd_w", _err_w(got["w"], ref["w"], x["ref"]["w"], ref["upd"], lay))


GDT = (F32, BF16)
WMDT = (None, F32, BF16)
LAMB_OPTS = list(itertools.product(GDT, WMDT, ((False, None), (True, 1), (True, 7)), (False, True), (1.0, 0.37)))
ADAM_OPTS = list(itertools.product((False, True), GDT, WMDT, (1, 7), (1.0, 0.37)))
SGD_MODES = ((0.0, 0.0, False), (0.9, 0.0, False), (0.9, 0.3, False), (0.9, 0.0, True))
SGD_OPTS = list(itertools.product(SGD_MODES, (0, 1), GDT, WMDT, (1.0, 0.37)))


def _thin(opts, name, every, at):
    """The whole matrix on the FULL table; elsewhere one combination in ``every``, the same number for
    each gradient / model-copy pair (``o[at]``, ``o[at + 1]``), a different choice per table."""
    if name == FULL:
        return opts
    picked = []
    for pair in itertools.product(GDT, WMDT):
        group = sorted((o for o in opts if (o[at], o[at + 1]) == pair), key=lambda o: zlib.crc32((name + repr(o)).encode()))
        picked += group[:max(1, len(group) // every)]
    return picked


def _lamb_matrix(name, dev, run, errs):
    lay = _layouts()[name]
    for gdt, wmdt, (bc, step), ta, gs in _thin(LAMB_OPTS, name, 6, 0):
        _lamb_case(lay, dev, run, errs, HP(bias_corr=bc, trust_all=ta), gdt, wmdt, step, gs,
                   tag="lamb %s g=%s wm=%s bc=%s step=%s ta=%d gs=%g" % (name, gdt, wmdt, bc, step, ta, gs))


def _adam_matrix(name, dev, run, errs):
    lay = _layouts()[name]
    for aw, gdt, wmdt, step, gs in _thin(ADAM_OPTS, name, 4, 1):
        _adam_case(lay, dev, run, errs, HP(adamw=aw), gdt, wmdt, step, gs,
                   tag="adam %s adamw=%d g=%s wm=%s step=%d gs=%g" % (name, aw, gdt, wmdt, step, gs))


def _sgd_matrix(name, dev, run, errs):
    lay = _layouts()[name]
    for (mom, damp, nes), first, gdt, wmdt, gs in _thin(SGD_OPTS, name, 8, 2):
        _sgd_case(lay, dev, run, errs, HP(momentum=mom, dampening=damp, nesterov=nes), gdt, wmdt, first, gs,
                  tag="sgd %s mom=%g damp=%g nes=%d first=%d g=%s wm=%s gs=%g" % (name, mom, damp, nes, first, gdt, wmdt, gs))


RANK_OPTS = [(F32, None, False, None, False, 1.0), (BF16, BF16, False, None, False, 0.37), (F32, BF16, True, 7, True, 1.0),
             (BF16, F32, True, 1, False, 1.0), (BF16, None, False, None, True, 0.37), (F32, F32, True, 7, False, 0.37)]


def _lamb_ranks(dev, run, errs):
    """ZeRO-1's norm all-reduce: stage 1 on each rank's table, the two tensor_parts added, stage 2
    on each rank -- against the reference on the unsharded space."""
    glob, r0, r1 = _rank_layouts(LENS[:5])
    gbase = _base(glob.n, glob.name)
    for gdt, wmdt, bc, step, ta, gs in RANK_OPTS:
        hp = HP(bias_corr=bc, trust_all=ta)
        state, dyn = "zero" if step == 1 else "rand", _dyn(step or 7, gs, hp)
        xg = _make(glob, dev, gdt, wmdt, state, dyn)
        g1 = _lamb_stage1(xg["ref"], glob, hp, F64)
        g2 = _lamb_stage2(xg["ref"], g1["m"], g1["v"], g1["part"], glob, hp, F64)
        xs = []
        for lay in (r0, r1):
            canary = lambda k: gbase[k][:MARGIN]  # noqa: E731
            base = {k: torch.cat([canary(k), v[MARGIN:MARGIN + glob.n][lay.gidx], canary(k)]) for k, v in gbase.items()}
            xs.append(_make(lay, dev, gdt, wmdt, state, dyn, base=base))
        if run == "kernel":
            parts = [_k_lamb(x, lay, hp, stage=1) for x, lay in zip(xs, (r0, r1))]
            total = parts[0] + parts[1]
            for x, lay in zip(xs, (r0, r1)):
                _k_lamb(x, lay, hp, stage=2, part=total.clone())
                _check_bits(x, lay, {"W", "M", "V", "WM"}, "ranks %s" % lay.name)
            gots = [{"m": x["m"], "v": x["v"], "w": x["w"]} for x in xs]
        else:
            s1 = [_lamb_stage1(x["ref"], lay, hp, F32) for x, lay in zip(xs, (r0, r1))]
            total = s1[0]["part"] + s1[1]["part"]
            gots = [dict(a, **_lamb_stage2(x["ref"], a["m"], a["v"], total, lay, hp, F32)) for a, x, lay in zip(s1, xs, (r0, r1))]
            gots = [{k: v for k, v in g.items() if k != "part"} for g in gots]
        _note(errs, "lamb_part", [_worst(e) for e in _err_rel(total.view(-1, 2), g1["part"])])
        for got, x, lay in zip(gots, xs, (r0, r1)):
            _lamb_errors(errs, got, _gather(g1, lay), _gather(g2, lay), x, lay)


# ------------------------------------------------------------------ sumsq / clip cases
SUMSQ_N = (4, 252, 1024, 1028, 4 * (2048 * 256 + 3))
CLIP_CASES = [(ss, bs) for bs in (1.0, 0.125) for ss in (0.25, 1.0, 9.0, 0.0)]      # x 1 / bs^2; max_norm 1


def _sumsq_cases(dev, run, errs):
    C = ops.require_native() if run == "kernel" else None
    for n in SUMSQ_N:
        for dt in GDT:
            x = (0.3 * torch.randn(n, generator=_gen("sumsq-%d" % n))).to(dt).to(dev)
            zeros = torch.zeros_like(x)
            for prev in (0.0, 3.25):
                out = torch.tensor([prev], dtype=F32, device=dev)
                want, mass = _sumsq(x, out[0], F64)
                want2, _ = _sumsq(x, want, F64)
                if run == "kernel":
                    C.sumsq_into(x, out)
                    one = out.clone()
                    C.sumsq_into(x, out)                 # a second call adds to the same out
                    two = out.clone()
                    C.sumsq_into(zeros, out)
                    assert torch.equal(out, two), "sumsq of zeros changed out (n %d)" % n
                    one, two = one[0], two[0]
                else:
                    one, _ = _sumsq(x, out[0], F32)
                    two, _ = _sumsq(x, one, F32)
                _note(errs, "sumsq", [_worst(_err_rel(one, want).reshape(1)), _worst(_err_rel(two, want2).reshape(1))])


def _clip_cases(dev, run, errs):
    C = ops.require_native() if run == "kernel" else None
    for ss, bs in CLIP_CASES:
        sumsq = torch.tensor([ss / (bs * bs)], dtype=F32, device=dev)
        dyn = torch.tensor([LR, 77.0, 1.25, 3.5], dtype=F32, device=dev)
        want = _clip(sumsq[0], bs, 1.0, F64)
        if run == "kernel":
            before = dyn.clone()
            C.clip_coef(sumsq, dyn, bs, 1.0)
            assert torch.equal(dyn[[0, 2, 3]], before[[0, 2, 3]]), "clip_coef wrote beside dyn[1]"
            got = dyn[1]
            if ss == 0.0:
                assert got.item() == bs
        else:
            got = _clip(sumsq[0], bs, 1.0, F32)
        assert (want < bs) == (ss >= 1.0)
        _note(errs, "clip", [_worst(_err_rel(got, want).reshape(1))])


# ------------------------------------------------------------------ end to end through FlatParamSpace
E2E = [
    ("lamb-clip", "lamb", dict(max_grad_norm=1.0), 1.0),
    ("lamb-clip-gs", "lamb", dict(max_grad_norm=1.0), 0.25),
    ("lamb-trustall-bc", "lamb", dict(trust_all=True, bias_correction=True), 1.0),
    ("adam-l2", "adam", dict(adamw=False), 1.0),
    ("adamw-gs", "adam", dict(adamw=True), 0.25),
    ("sgd-nesterov", "sgd", dict(momentum=0.9, nesterov=True), 1.0),
    ("sgd-damp-gs", "sgd", dict(momentum=0.9, dampening=0.3), 0.25),
    ("sgd-plain", "sgd", dict(momentum=0.0), 1.0),
]
E2E_IDS = [c[0] for c in E2E]
E2E_NORMS = (6.0, 1.7, 0.4)        # ||g x grad_scale|| per step: clipped, clipped, not clipped
E2E_SHAPES = ((24, 16), (24,), (24,))
E2E_NAMES = ("fc.weight", "fc.bias", "ln.weight")


def _space_layout(sp):
    """The table a FlatParamSpace of world size 1 should hold, built here from its offsets."""
    segs = []
    for t, (o, n) in enumerate(zip(sp.offsets, sp.numels)):
        segs += _split(t, o, o + (n + 63) // 64 * 64)
    return Layout("space", sp.total, len(sp.offsets), segs)


def _step_ref(kind, x, lay, hp, gs, dt):
    """One optimizer step on the flat state ``x``: (new state, the reference's terms, dyn[1])."""
    if hp.max_grad_norm:
        ss, _ = _sumsq(x["g"], torch.zeros((), dtype=F32, device=x["g"].device), dt)
        coef = _clip(ss, gs, hp.max_grad_norm, dt)
        dyn = x["dyn"].to(dt).clone()
        dyn[1] = coef
        x = dict(x, dyn=dyn)
    if kind == "lamb":
        out = _lamb_stage1(x, lay, hp, dt)
        out.update(_lamb_stage2(x, out["m"], out["v"], out["part"], lay, hp, dt))
    else:
        out = (_adam if kind == "adam" else _sgd)(x, lay, hp, dt)
    out["dyn1"] = x["dyn"][1]
    return out


def _e2e(case, mdt, dev, impl, errs):
    """3 steps; each compared with the fp64 reference applied to the state before that step.
    impl 'fused': the optimizer classes (HIP kernels on a GPU, their PyTorch path on the CPU);
    impl 'model': the F32 rounding model."""
    from cloudtik_amd.train.optim import FlatParamSpace, FusedAdam, FusedLAMB, FusedSGD
    name, kind, kw, gs = case
    gen = _gen("e2e-" + name)
    params = [torch.nn.Parameter(((1.0 if i == 2 else 0.0) + 0.5 * torch.randn(s, generator=gen)).to(mdt).to(dev))
              for i, s in enumerate(E2E_SHAPES)]
    sp = FlatParamSpace(params, names=list(E2E_NAMES))
    lay = _space_layout(sp)
    real = torch.zeros(sp.total, dtype=torch.bool)
    for o, n in zip(sp.offsets, sp.numels):
        real[o:o + n] = True
    wd = torch.tensor([0.0 if n.endswith("bias") else 0.01 for n in sp.names], dtype=F32, device=dev)
    eps = 1e-8 if kind == "adam" else 1e-6
    hp = HP(eps=eps, bias_corr=kw.get("bias_correction", False), trust_all=kw.get("trust_all", False),
            adamw=kw.get("adamw", True), momentum=kw.get("momentum", 0.0), dampening=kw.get("dampening", 0.0),
            nesterov=kw.get("nesterov", False), max_grad_norm=kw.get("max_grad_norm"))
    zeros = lambda: torch.zeros(sp.total, dtype=F32, device=dev)  # noqa: E731
    if impl == "fused":
        cls = {"lamb": FusedLAMB, "adam": FusedAdam, "sgd": FusedSGD}[kind]
        opt = cls(sp, lr=LR, weight_decay=0.01, no_decay=lambda n: n.endswith("bias"), space=sp,
                  **(dict(kw, eps=eps) if kind != "sgd" else kw))
        opt.grad_scale = gs
        state = lambda: {"w": sp.shard_params, "wm": sp.shard_model if sp.master is not None else None,  # noqa: E731
                         "m": getattr(opt, "exp_avg", None), "v": getattr(opt, "exp_avg_sq", None),
                         "buf": getattr(opt, "momentum_buffer", None)}
    else:
        st = {"w": sp.model.float().clone(), "wm": sp.model.clone() if mdt != F32 else None,
              "m": zeros(), "v": zeros(), "buf": zeros() if hp.momentum else None}
        state = lambda: st  # noqa: E731
    clipped = []
    for step in (1, 2, 3):
        g = torch.randn(sp.total, generator=gen) * real
        g = (g * (E2E_NORMS[step - 1] / gs / g.norm())).to(mdt).to(dev)
        sp.grad.copy_(g)
        dyn = _dyn(step, gs, hp, first=(step == 1) if kind == "sgd" else None)
        if kind == "lamb" and not hp.bias_corr:
            dyn = (LR, gs, 1.0, 1.0)
        x = {k: (v.clone() if v is not None else None) for k, v in state().items()}
        x.update(g=g.clone(), wd=wd, dyn=torch.tensor(dyn, dtype=F32, device=dev))
        x["ref"] = x
        ref = _step_ref(kind, x, lay, hp, gs, F64)
        if impl == "fused":
            opt.step()
            got = state()
            assert torch.equal(sp.grad, g), "the optimizer wrote the gradient"
            if got["wm"] is not None:
                assert torch.equal(got["wm"], got["w"].to(mdt)), "model copy != rounded master weights"
            if hp.max_grad_norm and dev.type == "cuda":
                _note(errs, "clip", [_worst(_err_rel(opt.dyn[1], ref["dyn1"]).reshape(1))])
        else:
            got = _step_ref(kind, x, lay, hp, gs, F32)
            st.update({k: got[k].to(F32) for k in ("w", "m", "v", "buf") if k in got})
            if st["wm"] is not None:
                st["wm"] = st["w"].to(mdt)
        clipped.append(bool(ref["dyn1"] < gs))
        pre = kind
        if kind != "sgd":
            _note(errs, pre + "_m", _err_terms(got["m"], ref["m"], ref["m_terms"], lay))
            _note(errs, pre + "_v", _err_terms(got["v"], ref["v"], ref["v_terms"], lay))
        elif hp.momentum:
            _note(errs, "sgd_buf", _err_terms(got["buf"], ref["buf"], ref["buf_terms"], lay))
        _note(errs, pre + "_w", _err_w(got["w"], ref["w"], x["w"], ref["upd"], lay))
    if hp.max_grad_norm:
        assert clipped == [True, True, False], clipped
    # the parameters are views of the flat buffers: the update is visible through them
    for p, o, n in zip(sp.params, sp.offsets, sp.numels):
        assert torch.equal(p.detach().reshape(-1), sp.model[o:o + n])


# ------------------------------------------------------------------ the model the bounds come from (CPU)
def _model_matrix():
    errs, cpu = {}, torch.device("cpu")
    for name in LAYOUTS:
        _lamb_matrix(name, cpu, "model", errs)
        _adam_matrix(name, cpu, "model", errs)
        _sgd_matrix(name, cpu, "model", errs)
    _lamb_ranks(cpu, "model", errs)
    _zero_grad_adam(cpu, "model", errs)
    _dyn_reread(cpu, "model", errs)
    _sumsq_cases(cpu, "model", errs)
    _clip_cases(cpu, "model", errs)
    for case in E2E:
        for mdt in (BF16, F32):
            _e2e(case, mdt, cpu, "model", errs)
    return {k: _top(v) for k, v in errs.items()}


def test_rounding_model_meets_bounds():
    """The model that the bounds come from meets them (by the factor of 4) on every case of the
    matrix, and the recorded figures are the model's; prints its worst error per quantity."""
    worst = _model_matrix()
    print("model worst:\n" + "\n".join('    "%s": %.2e,' % kv for kv in sorted(worst.items())))
    assert set(worst) == set(MODEL_WORST)
    for n in BOUND:      # give or take another CPU's summation order
        assert MODEL_WORST[n] * 0.75 <= worst[n] <= MODEL_WORST[n] * 1.25, (n, worst[n], MODEL_WORST[n])


def test_checker_catches_one_percent_on_a_small_tensor():
    """A trust ratio 1 % off on the 128-element tensor of T5, and a decay applied to a tensor that
    has none, vanish in the whole-buffer 2e-2 norm of the older tests and fail here."""
    lay, hp = _layouts()["T5"], HP(trust_all=True)
    x = _make(lay, torch.device("cpu"))
    r1 = _lamb_stage1(x["ref"], lay, hp, F64)
    r2 = _lamb_stage2(x["ref"], r1["m"], r1["v"], r1["part"], lay, hp, F64)
    part = r1["part"].clone()
    part[1, 0] *= 1.02                                   # ||w||^2 of tensor 1: ratio x 1.01
    bad = _lamb_stage2(x["ref"], r1["m"], r1["v"], part, lay, hp, F64)
    assert ((bad["w"] - r2["w"]).norm() / r2["w"].norm()).item() < 2e-2
    with pytest.raises(AssertionError):
        errs = {}
        _note(errs, "lamb_w", _err_w(bad["w"], r2["w"], x["ref"]["w"], r2["upd"], lay))
        _assert_bounds(errs, "ratio 1 % off")
    x2 = dict(x["ref"], wd=torch.full_like(x["wd"], 0.01))
    a, b = _adam(x["ref"], lay, HP(), F64), _adam(x2, lay, HP(), F64)
    assert ((a["w"] - b["w"]).norm() / a["w"].norm()).item() < 2e-2
    with pytest.raises(AssertionError):
        errs = {}
        _note(errs, "adam_w", _err_w(b["w"], a["w"], x["ref"]["w"], a["upd"], lay))
        _assert_bounds(errs, "decay on the wrong tensor")


# ------------------------------------------------------------------ CPU: the reference pinned to torch.optim
def _torch_optim_case(kind, hp, steps=3):
    """``_adam`` / ``_sgd`` in fp64 on three tensors against torch.optim on per-tensor parameters."""
    hp = HP(**dict(vars(hp), **{k: _f32(getattr(hp, k)) for k in ("b1", "b2", "eps", "momentum", "dampening")}))
    lay = _plain("pin", (64, 128, 192))
    gen = _gen("pin-%s" % kind)
    wds = (0.01, 0.0, 0.01)
    x = {"w": 0.5 * torch.randn(lay.n, generator=gen, dtype=F64), "m": torch.zeros(lay.n, dtype=F64),
         "v": torch.zeros(lay.n, dtype=F64), "buf": torch.zeros(lay.n, dtype=F64),
         "wd": torch.tensor(wds, dtype=F64)}
    cuts = [(s, s + l) for _, s, l in lay.segs]
    ps = [torch.nn.Parameter(x["w"][a:b].clone()) for a, b in cuts]
    groups = [{"params": [p], "weight_decay": wd} for p, wd in zip(ps, wds)]
    if kind == "adam":       # hp: the hyper-parameters as _sc hands them to the reference (fp32 values)
        topt = (torch.optim.AdamW if hp.adamw else torch.optim.Adam)(groups, lr=LR, betas=(hp.b1, hp.b2), eps=hp.eps)
    else:
        topt = torch.optim.SGD(groups, lr=LR, momentum=hp.momentum, dampening=hp.dampening, nesterov=hp.nesterov)
    worst = 0.0
    for step in range(1, steps + 1):
        gs = 0.37 if step == 2 else 1.0
        g = 0.1 * torch.randn(lay.n, generator=gen, dtype=F64)
        dyn = _dyn(step, gs, hp, first=(step == 1) if kind == "sgd" else None)
        x.update(g=g, dyn=torch.tensor(dyn, dtype=F64))
        out = (_adam if kind == "adam" else _sgd)(x, lay, hp, F64)
        for p, (a, b) in zip(ps, cuts):
            p.grad = (g[a:b] * gs).clone()
        topt.step()
        want = torch.cat([p.detach() for p in ps])
        worst = max(worst, _top(_err_w(out["w"], want, x["w"], out["upd"], lay)))
        x.update({k: out[k] for k in ("w", "m", "v", "buf") if k in out})
    return worst


@pytest.mark.parametrize("adamw", [False, True])
def test_reference_adam_is_torch_optim(adamw):
    assert _torch_optim_case("adam", HP(adamw=adamw, eps=1e-8)) <= 1e-12


@pytest.mark.parametrize("mode", SGD_MODES, ids=lambda m: "mom%g-damp%g-nes%d" % m)
def test_reference_sgd_is_torch_optim(mode):
    assert _torch_optim_case("sgd", HP(momentum=mode[0], dampening=mode[1], nesterov=mode[2])) <= 1e-12


# ------------------------------------------------------------------ CPU: the optimizers' PyTorch path
@pytest.mark.parametrize("mdt", [BF16, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("case", E2E, ids=E2E_IDS)
def test_cpu_path_follows_reference(case, mdt):
    """FusedLAMB._step_torch and the CPU branches of FusedAdam / FusedSGD, fp32 PyTorch on the flat
    buffers, stay within the fp32 model bounds of the fp64 reference: max_grad_norm, trust_all,
    bias_correction, adamw=False, nesterov, dampening, grad_scale."""
    errs = {}
    _e2e(case, mdt, torch.device("cpu"), "fused", errs)
    _assert_bounds(errs, "cpu-path %s %s" % (case[0], mdt))


# ------------------------------------------------------------------ CPU: FlatParamSpace._build_segments
SEG_NUMELS = (1, 63, 64, 65, 8192, 8193, 64 * 8192 + 1)


def _zero_pieces(total, world, rank, cap):
    pieces, lo, loc = [], 0, 0
    while lo < total:
        hi = min(lo + cap, total)
        c = (hi - lo) // world
        pieces.append((lo + rank * c, lo + (rank + 1) * c, loc))
        loc, lo = loc + c, hi
    return pieces


@pytest.mark.parametrize("zero", [False, True], ids=["plain", "zero1"])
@pytest.mark.parametrize("world", [1, 2, 3, 4])
def test_build_segments_properties(world, zero):
    from cloudtik_amd.train.optim import ALIGN, SEG as SEG_, FlatParamSpace
    assert (ALIGN, SEG_) == (64, SEG)
    seen = None
    for rank in range(world):
        params = [torch.nn.Parameter(torch.zeros(n)) for n in SEG_NUMELS]
        sp = FlatParamSpace(params, shard=(rank, world))
        if zero:
            sp.set_shard_pieces(_zero_pieces(sp.total, world, rank, 64 * world * 37), F32, None, None, None)
        T = len(sp.params)
        st, ss, sl = sp._seg_cpu
        first = sp.tensor_first_seg.tolist()
        assert len(first) == T + 1 and first[0] == 0 and first[-1] == len(st) == sp.nseg
        assert all(a <= b for a, b in zip(first, first[1:]))
        assert sp.seg_tensor.tolist()[:sp.nseg] == st and sp.seg_start.tolist()[:sp.nseg] == ss
        assert sp.seg_len.tolist()[:sp.nseg] == sl
        mine = torch.zeros(sp.total, dtype=torch.bool)
        for lo, hi, _ in sp.pieces:
            mine[lo:hi] = True
        count = torch.zeros(sp.total, dtype=torch.int32)      # global elements covered by a segment
        owner = torch.full((sp.total,), -1, dtype=torch.long)
        for i, (t, s, l) in enumerate(zip(st, ss, sl)):
            assert first[t] <= i < first[t + 1]
            assert s % 64 == 0 and l % 64 == 0 and 0 < l <= SEG and s + l <= sp.shard_size
            (lo, hi, loc), = [p for p in sp.pieces if p[2] <= s < p[2] + p[1] - p[0]]
            assert s + l <= loc + hi - lo, "a segment crosses two pieces"
            a = lo + s - loc
            count[a:a + l] += 1
            owner[a:a + l] = t
        want = torch.full((sp.total,), -1, dtype=torch.long)
        for t, (o, n) in enumerate(zip(sp.offsets, sp.numels)):
            want[o:o + (n + 63) // 64 * 64] = t
        want[~mine] = -1
        assert count.max() <= 1, "segments overlap"
        assert torch.equal(owner, want), "segments do not tile (padded tensor range x this rank's pieces)"
        seen = count if seen is None else seen + count
        used = sp.used
    assert (seen[:used] == 1).all() and (seen[used:] == 0).all()


# ------------------------------------------------------------------ GPU: LAMB
@pytest.mark.gpu
@pytest.mark.parametrize("name", LAYOUTS)
def test_variant_lamb(cuda, name):
    errs = {}
    _lamb_matrix(name, cuda, "kernel", errs)
    _assert_bounds(errs, "lamb %s" % name)


@pytest.mark.gpu
def test_variant_lamb_two_rank_norm_allreduce(cuda):
    errs = {}
    _lamb_ranks(cuda, "kernel", errs)
    _assert_bounds(errs, "lamb ranks")


@pytest.mark.gpu
@pytest.mark.parametrize("wmdt", WMDT, ids=["nocopy", "fp32copy", "bf16copy"])
def test_variant_lamb_stage3_is_stage1_then_stage2(cuda, wmdt):
    lay, hp = _layouts()["T6"], HP(bias_corr=True, trust_all=True)
    a = _make(lay, cuda, BF16, wmdt, "rand", _dyn(7, 0.37, hp))
    b = _make(lay, cuda, BF16, wmdt, "rand", _dyn(7, 0.37, hp))
    pa = _k_lamb(a, lay, hp, 3)
    pb = _k_lamb(b, lay, hp, 1)
    mid = b["w"].clone()
    assert torch.equal(mid, b["ref"]["w"]), "stage 1 wrote the weights"
    _k_lamb(b, lay, hp, 2, part=pb)
    assert torch.equal(pa, pb)
    for k in ("W", "M", "V", "WM"):
        if a["full"][k] is not None:
            assert torch.equal(a["full"][k], b["full"][k]), k


@pytest.mark.gpu
def test_variant_lamb_ratio_exactly_one(cuda):
    """wd 0 without trust_all; all-zero weights; all-zero u (zero gradient and moments, wd 0, with
    trust_all): ratio 1, compared with a reference whose ratio is 1 by construction."""
    lay = _layouts()["T4"]
    for ta, ones in ((False, (0, 1)), (True, (1, 2))):
        hp = HP(trust_all=ta)
        base = {k: v.clone() for k, v in _base(lay.n, lay.name).items()}
        (_, s1, l1), (_, s2, l2) = lay.segs[1], lay.segs[2]
        base["W"][MARGIN + s1:MARGIN + s1 + l1] = 0                       # tensor 1: zero weights
        for k in ("G", "M", "V"):
            base[k][MARGIN + s2:MARGIN + s2 + l2] = 0                     # tensor 2: zero u at wd 0
        x = _make(lay, cuda, F32, BF16, "rand", _dyn(7, 1.0, hp), base=base, wd=(0.0, 0.01, 0.0, 0.01))
        r1 = _lamb_stage1(x["ref"], lay, hp, F64)
        r2 = _lamb_stage2(x["ref"], r1["m"], r1["v"], r1["part"], lay, hp, F64, ratio_one=ones)
        assert r1["part"][1, 0] == 0 and r1["part"][2, 1] == 0 and (r1["part"][0] > 0).all()
        part = _k_lamb(x, lay, hp)
        _check_bits(x, lay, {"W", "M", "V", "WM"}, "ratio one")
        errs = {}
        _lamb_errors(errs, {"m": x["m"], "v": x["v"], "w": x["w"], "part": part}, r1, r2, x, lay)
        _assert_bounds(errs, "lamb ratio-one trust_all=%d" % ta)
        if ta:
            assert torch.equal(x["w"][s2:s2 + l2], x["ref"]["w"][s2:s2 + l2])     # u = 0: the weights stay


@pytest.mark.gpu
def test_variant_lamb_offset_gradient(cuda):
    """A bf16 gradient that starts 4 elements (8 bytes) into its buffer: 8-byte aligned, so the
    8-wide kernels (16-byte accesses) step aside for the 4-wide ones, and the result is right."""
    lay, hp, errs = _layouts()["T5"], HP(trust_all=True), {}
    _lamb_case(lay, cuda, "kernel", errs, hp, BF16, BF16, 7, 0.37, goff=4, tag="lamb offset")
    _assert_bounds(errs, "lamb offset-gradient")


# ------------------------------------------------------------------ GPU: Adam, SGD, dyn
@pytest.mark.gpu
@pytest.mark.parametrize("name", LAYOUTS)
def test_adam(cuda, name):
    errs = {}
    _adam_matrix(name, cuda, "kernel", errs)
    _assert_bounds(errs, "adam %s" % name)


def _zero_grad_adam(dev, run, errs):
    lay = _layouts()["T4"]
    for aw in (False, True):
        x, ref = _adam_case(lay, dev, run, errs, HP(adamw=aw), F32, BF16, 1, 1.0, state="zero-grad", tag="adam zero")
        if aw and run == "kernel":
            c = lay.on(dev).cov
            assert not x["m"][c].any() and not x["v"][c].any()
            decay = x["ref"]["w"].double() * (1 - LR * x["wd"].double()[lay.on(dev).tid0])
            assert ((x["w"].double() - decay).abs() <= BOUND["adam_w"] * x["ref"]["w"].double().abs())[c].all()


@pytest.mark.gpu
def test_adam_zero_gradient_is_the_decay_term(cuda):
    errs = {}
    _zero_grad_adam(cuda, "kernel", errs)
    _assert_bounds(errs, "adam zero-gradient")


@pytest.mark.gpu
@pytest.mark.parametrize("name", LAYOUTS)
def test_sgd(cuda, name):
    errs = {}
    _sgd_matrix(name, cuda, "kernel", errs)
    _assert_bounds(errs, "sgd %s" % name)


def _dyn_reread(dev, run, errs):
    """Two calls with the same arguments, dyn rewritten on the device in between (lr halved, other
    slots moved): the second follows the new values -- what a graph replay relies on."""
    lay = _layouts()["T4"]
    hl, ha, hs = HP(bias_corr=True, trust_all=True), HP(adamw=False), HP(momentum=0.9, dampening=0.3)
    calls = (("lamb", hl, _dyn(6, 1.0, hl), _dyn(7, 0.37, hl, lr=LR / 2)),
             ("adam", ha, _dyn(6, 1.0, ha), _dyn(7, 0.37, ha, lr=LR / 2)),
             ("sgd", hs, _dyn(None, 1.0, hs, first=1), _dyn(None, 0.37, hs, lr=LR / 2, first=0)))
    for kind, hp, d0, d1 in calls:
        x = _make(lay, dev, BF16, BF16, "rand", d0)
        for d in (d0, d1):
            x["dyn"].copy_(torch.tensor(d, dtype=F32))
            _snapshot(x)
            ref = _step_ref(kind, x["ref"], lay, hp, 1.0, F64)
            if run == "kernel":
                {"lamb": _k_lamb, "adam": _k_adam, "sgd": _k_sgd}[kind](x, lay, hp)
                _check_bits(x, lay, {"W", "M", "V", "B", "WM"} - ({"B"} if kind != "sgd" else {"M", "V"}), "dyn " + kind)
                got = x
            else:
                got = _step_ref(kind, x["ref"], lay, hp, 1.0, F32)
                for k, name in (("w", "W"), ("m", "M"), ("v", "V"), ("buf", "B")):
                    if k in got:
                        x["full"][name][MARGIN:MARGIN + lay.n] = got[k].to(F32)
            _note(errs, kind + "_w", _err_w(got["w"], ref["w"], x["ref"]["w"], ref["upd"], lay))
            if kind == "sgd":
                _note(errs, "sgd_buf", _err_terms(got["buf"], ref["buf"], ref["buf_terms"], lay))
            else:
                _note(errs, kind + "_m", _err_terms(got["m"], ref["m"], ref["m_terms"], lay))
                _note(errs, kind + "_v", _err_terms(got["v"], ref["v"], ref["v_terms"], lay))


@pytest.mark.gpu
def test_dyn_is_read_on_the_device(cuda):
    errs = {}
    _dyn_reread(cuda, "kernel", errs)
    _assert_bounds(errs, "dyn reread")


# ------------------------------------------------------------------ GPU: sumsq, clip, bindings, end to end
@pytest.mark.gpu
def test_sumsq(cuda):
    errs = {}
    _sumsq_cases(cuda, "kernel", errs)
    _assert_bounds(errs, "sumsq")


@pytest.mark.gpu
def test_clip_coef(cuda):
    errs = {}
    _clip_cases(cuda, "kernel", errs)
    _assert_bounds(errs, "clip")


@pytest.mark.gpu
def test_bindings_refuse_short_or_foreign_tensors(cuda):
    """Host-side argument checks (nothing is launched): a model copy shorter than the weights, and
    clip_coef's device, dtype and length."""
    C = ops.require_native()
    lay = _layouts()["T3"]
    L = lay.on(cuda)
    x = _make(lay, cuda, F32, BF16)
    short = x["wm"][:lay.n - 64].contiguous()
    with pytest.raises(RuntimeError):
        C.adam_step(x["g"], x["m"], x["v"], x["w"], short, L.seg_tensor, L.seg_start, L.seg_len, x["wd"], x["dyn"],
                    0.9, 0.999, 1e-8, True)
    with pytest.raises(RuntimeError):
        C.sgd_step(x["g"], x["buf"], x["w"], short, L.seg_tensor, L.seg_start, L.seg_len, x["wd"], x["dyn"], 0.9, 0.0, False)
    with pytest.raises(RuntimeError):
        C.lamb_step(x["g"], x["m"], x["v"], x["w"], short, L.seg_tensor, L.seg_start, L.seg_len, L.first, x["wd"], x["dyn"],
                    0.9, 0.999, 1e-6, False, False, torch.zeros(2 * len(lay.segs), device=cuda),
                    torch.zeros(2 * lay.T, device=cuda), 3)
    ss, dyn = torch.ones(1, device=cuda), torch.ones(4, device=cuda)
    for bad_ss, bad_dyn in ((ss.cpu(), dyn), (ss, dyn.cpu()), (ss.double(), dyn), (ss, dyn.bfloat16()), (ss, dyn[:3]),
                            (ss[:0], dyn)):
        with pytest.raises(RuntimeError):
            C.clip_coef(bad_ss, bad_dyn, 1.0, 1.0)
    torch.cuda.synchronize()
    assert torch.equal(dyn, torch.ones(4, device=cuda))
    _check_bits(x, lay, set(), "refused calls")


@pytest.mark.gpu
@pytest.mark.parametrize("mdt", [BF16, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("case", E2E, ids=E2E_IDS)
def test_end_to_end_through_flat_space(cuda, case, mdt):
    errs = {}
    _e2e(case, mdt, cuda, "fused", errs)
    _assert_bounds(errs, "e2e %s %s" % (case[0], mdt))


# ------------------------------------------------------------------ GPU: which kernels ran
def _v8():
    e = os.environ.get("CLOUDTIK_AMD_LAMB_V8")
    return bool(e) and e.strip().lstrip("+-").isdigit() and int(e) != 0      # the library's atoi(e) != 0


@pytest.mark.gpu
def test_variant_kernels_selected(cuda):
    """The kernels that ran, by name from the profiler, are the ones ct_lamb / ct_adam / ct_sgd /
    ct_sumsq are documented to pick under this process's variable: a child process cannot pass by
    quietly running the default kernels."""
    from torch.profiler import ProfilerActivity, profile
    lay = _layouts()["T3"]
    tn = {F32: "float", BF16: "unsignedshort", None: "float"}
    keys = ("lamb_stage", "seg_to_tensor", "adam_kernel", "sgd_kernel", "sumsq", "clip_coef")

    def names_of(fn):
        fn()                                            # warm: module load, allocations
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return [e.name.replace(" ", "") for e in prof.events()
                if e.device_type == torch.autograd.DeviceType.CUDA and any(k in e.name for k in keys)]

    def has(names, want):
        assert len(names) == len(want) and all(any(w in n for n in names) for w in want), (names, want)

    for gdt, wmdt in itertools.product(GDT, WMDT):
        for goff in (0, 4) if gdt == BF16 else (0,):
            v8 = "_v8" if (_v8() and goff == 0) else ""
            x = _make(lay, cuda, gdt, wmdt, goff=goff)
            has(names_of(lambda: _k_lamb(x, lay, HP())),
                ["lamb_stage1%s_kernel<%s>" % (v8, tn[gdt]), "seg_to_tensor_kernel", "lamb_stage2%s_kernel<%s>" % (v8, tn[wmdt])])
        x = _make(lay, cuda, gdt, wmdt)
        has(names_of(lambda: _k_adam(x, lay, HP())), ["adam_kernel<%s,%s>" % (tn[gdt], tn[wmdt])])
        has(names_of(lambda: _k_sgd(x, lay, HP(momentum=0.9))), ["sgd_kernel<%s,%s>" % (tn[gdt], tn[wmdt])])
    C = ops.require_native()
    for dt in GDT:
        v, out = torch.ones(1024, device=cuda, dtype=dt), torch.zeros(1, device=cuda)
        has(names_of(lambda: C.sumsq_into(v, out)), ["sumsq_kernel<%s>" % tn[dt], "sumsq_finish_kernel"])
    dyn = torch.ones(4, device=cuda)
    has(names_of(lambda: C.clip_coef(out, dyn, 1.0, 1.0)), ["clip_coef_kernel"])


@pytest.mark.gpu
def test_nondefault_kernels_in_child_process(cuda):
    """The 8-wide LAMB kernels (CLOUDTIK_AMD_LAMB_V8=1, read once per process) on the
    ``test_variant_*`` subset in one child process."""
    env = dict(os.environ, CLOUDTIK_AMD_LAMB_V8="1")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-s", __file__, "-m", "gpu", "-k", "test_variant_",
                        "-p", "no:cacheprovider"], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and "skipped" not in r.stdout, r.stdout[-2000:]
    worst = {}
    for line in r.stdout.splitlines():
        if line.startswith("optim-err "):
            for kv in line.split():
                if "=" in kv and kv.split("=")[0] in BOUND:
                    n, e = kv.split("=")
                    worst[n] = max([worst.get(n, 0.0)] + [float(v) for v in e.split("/")])
    assert worst, r.stdout[-2000:]
    print("optim-err-child V8=1 %s" % " ".join("%s=%.2e" % kv for kv in sorted(worst.items())))
