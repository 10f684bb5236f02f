"""Relative-bias attention for training (ops/csrc/attention.hip): forward with dropout and lse,
backward with dQ, dK, dV and the gradient of the bias vector, on every dispatch path and edge.

Method of tests/test_attention_gpu.py (read its docstring first), with helpers of its own.  Every
case compares the HIP kernels with an fp64 autograd reference computed from the same bf16 inputs
(``_ref64``), in which the bias vector ``rel`` is a leaf, so ``rel.grad`` is the wanted ``d_rel``:

* ``o``, ``dq``, ``dk``, ``dv``: per (batch, head, row), max |kernel - ref| over the 64 columns /
  (max |ref| over that row + 1e-3 x the tensor's max |ref|); ``lse``: absolute, log2 units.
* ``d_rel``, per (head, offset i): |kernel - ref| / (A[h, i] + 1e-3 x max_i A[h, .]) with
  A[h, i] = the sum of |dS_ref| over the diagonal key - query + rel_base = i and all batches (fp64).
  The denominator is the sum of magnitudes, not the magnitude of the sum, so cancellation on a
  diagonal does not fail a correct kernel.

BOUNDS.  Not taken from the kernel.  ``_model`` is the rounding model of test_attention_gpu.py
(fp32 scores in the log2 domain, P and dS rounded to bf16 before their MFMAs, delta from the bf16
O, bf16 outputs) plus ``d_rel`` summed in fp32 from the UNROUNDED fp32 dS, which is what the
kernel adds.  Its worst figures against ``_ref64`` over the whole case matrix below, the extra
cases included (measured on a CPU), and the bounds, 4 x each (the factor of test_attention_gpu.py:
accumulation order, the exp2-domain rescaling, the hardware exp2):

    | quantity                                              | model worst | bound (4 x) |
    |-------------------------------------------------------|-------------|-------------|
    | o                                                     | 6.11e-03    | 2.44e-02    |
    | lse (absolute, log2 units)                            | 8.71e-07    | 3.48e-06    |
    | dq                                                    | 7.87e-03    | 3.15e-02    |
    | dk                                                    | 1.60e-02    | 6.40e-02    |
    | dv                                                    | 6.12e-03    | 2.45e-02    |
    | dq, causal rows 0..7, p = 0        (``dq_short``)       | 9.20e-02    | 3.68e-01    |
    | dq, causal rows 0..7, p > 0        (``dq_short_drop``)  | 7.16e+00    | 2.86e+01    |
    | dk with Sq = 1                     (``dk_single``)      | 4.34e-02    | 1.74e-01    |
    | d_rel                                                 | 3.47e-03    | 1.39e-02    |
    | d_rel with Sq = 1                  (``d_rel_single``)   | 1.76e-02    | 7.04e-02    |

ILL-CONDITIONED ENTRIES.  ``dq_short``, ``dq_short_drop`` and ``dk_single`` are the classes of
test_attention_gpu.py, same cause: dS = P (dP - delta) with delta from the bf16 O, whose absolute
error of about 2^-9 |dO . O| does not shrink where dP - delta cancels (causal rows that see one
or a few keys; Sq = 1).  ``d_rel_single`` is ``dk_single`` seen from the bias: with Sq = 1 every
offset holds ONE dS per batch, no sum over queries absorbs a key whose dP - delta nearly
cancels, and the model is 5 x worse there (1.76e-2) than anywhere else (3.47e-3, and below 2e-3
under the causal mask, where the short rows' error lands on the well-populated main diagonal).
Each class bound is at most the whole-matrix figure.

``d_rel`` is NOT bitwise reproducible (the workgroup sums its window with LDS float adds in an
order the hardware picks; only the sum across workgroups is order-fixed), so repeated runs are
compared within the bound, never bit for bit.

CASE MATRIX (B = 2, H = 3, D = 64, inputs randn * 0.5, scale 1/8, rel_base = Sq - 1,
L = Sq + Sk - 1, rel = randn * 0.5), crossed with causal x p in {0, 0.1 (even Sk only)} x key
bias {none, present}:

| path                                                              | (Sq, Sk)                          |
|-------------------------------------------------------------------|-----------------------------------|
| forward one tile; backward single block, Sq <= 128, full q-tiles  | (40, 40), (128, 128), (64, 72)    |
| partial q-tile (rows past Sq enter the window arithmetic)         | (100, 72), (33, 128), (1, 40)     |
| single block, Sq > 128                                            | (160, 72), (129, 128)             |
| MULTI, Sk > 128 (several windows per head meet in the reduce;     | (33, 130), (200, 200), (160, 264) |
|   keys past Sk in the last block)                                 |                                   |
| odd Sk, p = 0                                                     | (96, 63), (128, 129)              |

KERNEL INSTANTIATIONS -> CASES.  {DROP, CAUSAL} is covered everywhere by the causal x p cross.

* forward ``attn_fwd_d64_kernel<DROP, CAUSAL, REL=true, 2, GL=false>``: every case.
* backward ``attn_bwd_d64_rel_kernel<DROP, CAUSAL, MULTI=false>``: every Sk <= 128 row.  REL has
  NO LDS-DMA (GL) form: Sq <= 128 runs this register-staged single-block kernel too.
* backward ``attn_bwd_d64_rel_kernel<DROP, CAUSAL, MULTI=true>`` + ``attn_dq_convert_kernel``: the
  Sk > 128 rows.
* ``attn_drel_reduce_kernel``: every case; several key-block windows per head in the MULTI rows.
* ``test_rel_kernels_selected`` reads the kernel names from the profiler, one shape per row.
* p > 0 with odd Sk, and an Sq whose windows exceed the LDS budget (Sq > 1856), are routed by
  the front end to the PyTorch reference (``test_front_end_routes_to_reference``).
"""
import functools
import math

import pytest
import torch

from cloudtik_amd import ops
from cloudtik_amd.ops import reference as ref
from cloudtik_amd.ops.attention import _relbias_reference
from test_attention_gpu import PAD_HS, _padded, _untouched

D = 64
B0, H0 = 2, 3
SCALE = 0.125
SEED = 11
LN2 = math.log(2.0)
LOG2E = 1.0 / LN2
SHORT = 8      # causal query rows with fewer than SHORT visible keys

# worst error of _model against _ref64 over the whole matrix (see the module docstring)
MODEL_WORST = {"o": 6.11e-3, "lse": 8.71e-7, "dq": 7.87e-3, "dk": 1.60e-2, "dv": 6.12e-3,
               "dq_short": 9.20e-2, "dq_short_drop": 7.16, "dk_single": 4.34e-2,
               "d_rel": 3.47e-3, "d_rel_single": 1.76e-2}
BOUND = {k: 4.0 * v for k, v in MODEL_WORST.items()}

SHAPES = [(40, 40), (128, 128), (64, 72),
          (100, 72), (33, 128), (1, 40),
          (160, 72), (129, 128),
          (33, 130), (200, 200), (160, 264),
          (96, 63), (128, 129)]
# one shape per row of the table
ROW_SHAPES = [(64, 72), (100, 72), (160, 72), (160, 264), (96, 63)]


def _cases(shapes, biases=("none", "present")):
    out = []
    for Sq, Sk in shapes:
        for causal in (False, True):
            for p in (0.0, 0.1):
                if p > 0 and Sk % 2:
                    continue       # routed to the PyTorch reference: test_front_end_routes_to_reference
                for bias in biases:
                    out.append((Sq, Sk, causal, p, bias))
    return out


def _id(c):
    return "%dx%d-%s-p%g-%s" % (c[0], c[1], "causal" if c[2] else "full", c[3], c[4])


# ------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=None)
def _inputs(B, H, Sq, Sk, amp=0.5):
    g = torch.Generator().manual_seed(2000 * Sq + Sk)
    q = (torch.randn(B, H, Sq, D, generator=g) * amp).bfloat16()
    k = (torch.randn(B, H, Sk, D, generator=g) * amp).bfloat16()
    v = (torch.randn(B, H, Sk, D, generator=g) * amp).bfloat16()
    do = torch.randn(B, H, Sq, D, generator=g).bfloat16()
    return {"q": q, "k": k, "v": v, "do": do}


def _key_bias(B, Sk, kind):
    """none | present: a small finite bias on every key plus -10000 on the last quarter of the keys
    of batch 1 only | inf0: -inf on every key of batch 0."""
    if kind == "none":
        return None
    g = torch.Generator().manual_seed(177 + Sk)
    kb = torch.randn(B, Sk, generator=g) * 0.5
    if kind == "present":
        kb[1, Sk - Sk // 4:] = -10000.0
    else:
        kb[0] = float("-inf")
    return kb


@functools.lru_cache(maxsize=None)
def _rel_vec(H, L, salt=0):
    g = torch.Generator().manual_seed(31 + L + 1000 * salt)
    return torch.randn(H, L, generator=g) * 0.5


def _diag_index(Sq, Sk, rel_base):
    return torch.arange(Sk)[None, :] - torch.arange(Sq)[:, None] + rel_base      # [Sq, Sk]


def _diag_sum(x, idx, L):
    """[B, H, Sq, Sk] -> [H, L]: the sum over batches and over each diagonal key - query + rel_base = i."""
    H = x.shape[1]
    return torch.zeros(H, L, dtype=x.dtype).index_add_(1, idx.reshape(-1), x.sum(0).reshape(H, -1))


def _keep_mask(B, H, Sq, Sk, p):
    """The keep mask of the stream the front end draws after ops.manual_seed(SEED)."""
    if p == 0:
        return None, 0, 0
    ops.manual_seed(SEED)
    seed, off = ops._rng.next(B * H * Sq * Sk)
    return ref.attn_dropout_keep(B, H, Sq, Sk, p, seed, off), seed, off


# ------------------------------------------------------------------ fp64 reference
def _ref64(inp, rel, rel_base, kb=None, causal=False, keep=None, p=0.0, scale=SCALE):
    """fp64 forward + autograd backward from the bf16 inputs ([B, H, S, 64]); ``rel`` [H, L] is a
    leaf.  Rows with every key masked get P = 0: O = 0, lse = +inf, zero gradients.  Also returns
    ``A`` [H, L], the sum of |dS| per offset (the d_rel metric's denominator)."""
    q, k, v = (inp[n].double().requires_grad_() for n in ("q", "k", "v"))
    relv = rel.double().requires_grad_()
    Sq, Sk, L = q.shape[2], k.shape[2], rel.shape[1]
    idx = _diag_index(Sq, Sk, rel_base)
    s0 = q @ k.transpose(-1, -2) * scale + relv[:, idx][None]
    if kb is not None:
        s0 = s0 + kb.double()[:, None, None, :]
    s0.retain_grad()
    s = s0
    if causal:
        s = s.masked_fill(torch.ones(Sq, Sk, dtype=torch.bool).triu(1), float("-inf"))
    m = s.detach().amax(-1, keepdim=True)
    m = torch.where(torch.isinf(m), torch.zeros_like(m), m)
    e = torch.exp(s - m)
    l = e.sum(-1, keepdim=True)
    pr = e / torch.where(l > 0, l, torch.ones_like(l))
    lse = torch.where(l > 0, m + torch.log(torch.where(l > 0, l, torch.ones_like(l))),
                      torch.full_like(l, float("inf"))).squeeze(-1) / LN2
    if keep is not None:
        pr = pr * (keep.double() / (1.0 - p))
    o = pr @ v
    o.backward(inp["do"].double())
    return {"o": o.detach(), "lse": lse.detach(), "dq": q.grad, "dk": k.grad, "dv": v.grad, "d_rel": relv.grad,
            "A": _diag_sum(s0.grad.abs(), idx, L)}


# ------------------------------------------------------------------ CPU rounding model of the kernels
def _bf(x):
    return x.bfloat16().float()


def _model(inp, rel, rel_base, kb=None, causal=False, keep=None, p=0.0, scale=SCALE, drel_keys=None):
    """What the kernels compute, with their rounding steps and nothing else (the model of
    test_attention_gpu.py), plus d_rel: the fp32 sum over each diagonal and all batches of the
    fp32 dS BEFORE its bf16 rounding.  ``drel_keys``: only these keys enter d_rel (a checker test
    leaves a key block out with it)."""
    q, k, v, do = (inp[n].float() for n in ("q", "k", "v", "do"))
    Sq, Sk, L = q.shape[2], k.shape[2], rel.shape[1]
    idx = _diag_index(Sq, Sk, rel_base)
    sl2 = torch.tensor(scale, dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32)
    s = (q @ k.transpose(-1, -2)) * sl2
    if kb is not None:
        s = s + (kb.float() * LOG2E)[:, None, None, :]
    s = s + (rel.float() * LOG2E)[:, idx][None]
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
    ds32 = pn * (dpv - delta)
    ds = _bf(ds32)
    dv = _bf(_bf(pd).transpose(-1, -2) @ do)
    dk = _bf((ds.transpose(-1, -2) @ q) * scale)
    dq = _bf((ds @ k) * scale)
    if drel_keys is not None:
        gate = torch.zeros(Sk)
        gate[drel_keys] = 1.0
        ds32 = ds32 * gate
    return {"o": o, "lse": lse.squeeze(-1), "dq": dq, "dk": dk, "dv": dv, "d_rel": _diag_sum(ds32, idx, L)}


# ------------------------------------------------------------------ metric and checker
def _rows(x, want):
    x, want = x.double(), want.double()
    d = (x - want).abs().amax(-1)
    top = want.abs().max()
    if top == 0:
        return d
    return d / (want.abs().amax(-1) + 1e-3 * top)


def _lse_err(x, want):
    x, want = x.double(), want.double()
    same_inf = torch.isinf(want) & (x == want)
    return torch.where(same_inf, torch.zeros_like(want), (x - want).abs()).max().item()


def _drel_err(x, want, A):
    """Per (h, i): |x - want| / (A[h, i] + 1e-3 max_i A[h, .]); a head whose A is identically zero
    (a single visible key everywhere: no gradient) has no scale, the error is then absolute."""
    den = A + 1e-3 * A.amax(1, keepdim=True)
    den = torch.where(den > 0, den, torch.ones_like(den))
    return ((x.double() - want.double()).abs() / den)


def _errors(got, want, causal=False, p=0.0):
    """Worst row / entry per quantity, keyed like BOUND."""
    out = {}
    for n, t in got.items():
        if n == "lse":
            out[n] = _lse_err(t, want[n])
        elif n == "d_rel":
            out["d_rel_single" if want["o"].shape[2] == 1 else "d_rel"] = _drel_err(t, want[n], want["A"]).max().item()
        else:
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


def _check(got, want, kb=None, tag="", causal=False, p=0.0, rel_base=None):
    """The assertions of every case: finite outputs, every quantity within its bound, exactly zero
    dk / dv at keys that carry a -10000 bias, and under the causal mask exactly zero d_rel at every
    offset past rel_base (key > query)."""
    errs = _errors(got, want, causal, p)
    print("relattn-err %s %s" % (tag, " ".join("%s=%.3e" % kv for kv in sorted(errs.items()))))
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
        assert rel_base is not None
        assert (got["d_rel"][:, rel_base + 1:] == 0).all(), "%s: d_rel non-zero past the causal diagonal" % tag
    return errs


@functools.lru_cache(maxsize=None)
def _expected(case, slack=0, amp=0.5, scale=SCALE):
    """Inputs, key bias, bias vector, keep mask and the fp64 reference of one case: computed once,
    shared by every test that needs it, never modified.  ``slack``: rel_base = Sq - 1 + slack and
    L = Sq + Sk - 1 + 2 slack."""
    Sq, Sk, causal, p, bias = case
    inp = _inputs(B0, H0, Sq, Sk, amp)
    kb = _key_bias(B0, Sk, bias)
    rel_base, L = Sq - 1 + slack, Sq + Sk - 1 + 2 * slack
    rel = _rel_vec(H0, L)
    keep, seed, off = _keep_mask(B0, H0, Sq, Sk, p)
    return inp, kb, rel, rel_base, keep, (seed, off), _ref64(inp, rel, rel_base, kb, causal, keep, p, scale)


T5_CASE = (64, 64, True, 0.1, "present")       # scale 1.0, inputs randn * 0.25: the call T5 makes


def _t5_expected():
    return _expected(T5_CASE, 0, 0.25, 1.0)


# ------------------------------------------------------------------ the checker itself, on the CPU
def test_rounding_model_meets_bounds():
    """The model that the bounds come from passes them (by a factor of 4) on every case of the
    matrix and on the extra cases; prints its worst error per quantity."""
    worst = {n: 0.0 for n in BOUND}

    def one(exp, case, tag, scale=SCALE):
        inp, kb, rel, rel_base, keep, _, want = exp
        got = _model(inp, rel, rel_base, kb, case[2], keep, case[3], scale)
        for n, e in _check(got, want, kb, tag, case[2], case[3], rel_base).items():
            worst[n] = max(worst[n], e)

    for case in _cases(SHAPES):
        one(_expected(case), case, "model " + _id(case))
    slack_case = (100, 72, False, 0.1, "present")
    one(_expected(slack_case, 5), slack_case, "model slack")
    one(_t5_expected(), T5_CASE, "model t5", 1.0)
    print("model worst:", " ".join("%s=%.3e" % kv for kv in sorted(worst.items())))
    for n in BOUND:     # the recorded figures are the model's, give or take another CPU's summation order
        assert MODEL_WORST[n] / 2 <= worst[n] <= MODEL_WORST[n] * 2, (n, worst[n], MODEL_WORST[n])


def _fails(got, want, **kw):
    with pytest.raises(AssertionError):
        _check(got, want, **kw)


def test_checker_catches_shifted_d_rel():
    """d_rel shifted by one offset (the bias indexed at key - query + rel_base + 1)."""
    case = (100, 72, False, 0.0, "none")
    inp, kb, rel, rel_base, keep, _, want = _expected(case)
    got = _model(inp, rel, rel_base, kb)
    _check(got, want, kb, "model, unbroken")
    got["d_rel"] = torch.roll(got["d_rel"], 1, dims=1)
    _fails({"d_rel": got["d_rel"]}, want, tag="shifted d_rel")


def test_checker_catches_missing_batch():
    """d_rel without batch 1's share."""
    case = (100, 72, False, 0.0, "none")
    inp, kb, rel, rel_base, keep, _, want = _expected(case)
    one = {n: t[:1] for n, t in inp.items()}
    got = _model(one, rel, rel_base, None)
    _fails({"d_rel": got["d_rel"]}, want, tag="d_rel of batch 0 alone")


def test_checker_catches_missing_key_block():
    """d_rel without the second key block's share (keys 128 .. 255) at (160, 264)."""
    case = (160, 264, False, 0.0, "none")
    inp, kb, rel, rel_base, keep, _, want = _expected(case)
    _check(_model(inp, rel, rel_base, kb), want, kb, "model, unbroken")
    got = _model(inp, rel, rel_base, kb, drel_keys=[k for k in range(264) if not 128 <= k < 256])
    _fails({"d_rel": got["d_rel"]}, want, tag="d_rel without key block 1")


def test_checker_catches_missing_dropout_rescale():
    """d_rel without the 1 / (1 - p) factor at p = 0.1."""
    case = (100, 72, False, 0.1, "none")
    inp, kb, rel, rel_base, keep, _, want = _expected(case)
    got = _model(inp, rel, rel_base, kb, False, keep, 0.1)
    _check(got, want, kb, "model, unbroken", p=0.1)
    _fails({"d_rel": got["d_rel"] * 0.9}, want, tag="d_rel without the rescale", p=0.1)


# ------------------------------------------------------------------ GPU runners
def _bshd(t, dev):
    return t.to(dev).transpose(1, 2)


def _back(t):
    return t.transpose(1, 2).cpu()


def _run_direct(dev, inp, rel, rel_base, kb, causal, p, seed, off, scale=SCALE, rel_dev=None):
    """attn_fwd_relbias_train / attn_bwd_relbias called as the autograd function calls them."""
    C = ops.require_native()
    q, k, v, do = (_bshd(inp[n], dev) for n in ("q", "k", "v", "do"))
    B, Sq, H, _ = q.shape
    kbd = kb.to(dev) if kb is not None else None
    reld = rel.to(dev) if rel_dev is None else rel_dev
    o = torch.empty_like(q)
    lse = C.attn_fwd_relbias_train(q, k, v, o, kbd, reld, rel_base, scale, p, seed, off, causal)
    dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    d_rel = torch.empty_like(reld)
    C.attn_bwd_relbias(q, k, v, o, do, dq, dk, dv, d_rel, kbd, reld, rel_base, lse, scale, p, seed, off, causal)
    return {"o": _back(o), "lse": lse.view(B, H, Sq).cpu(), "dq": _back(dq), "dk": _back(dk), "dv": _back(dv),
            "d_rel": d_rel.cpu()}


def _run_front(dev, inp, rel, rel_base, kb, causal, p, scale=SCALE, rel_dev=None):
    """ops.attention_relbias under autograd, on the stream of ops.manual_seed(SEED)."""
    q, k, v = (_bshd(inp[n], dev).detach().requires_grad_() for n in ("q", "k", "v"))
    reld = (rel.to(dev) if rel_dev is None else rel_dev).detach().requires_grad_()
    ops.manual_seed(SEED)
    o = ops.attention_relbias(q, k, v, reld, rel_base, kb.to(dev) if kb is not None else None, scale=scale,
                              causal=causal, p=p)
    o.backward(_bshd(inp["do"], dev))
    return {"o": _back(o.detach()), "dq": _back(q.grad), "dk": _back(k.grad), "dv": _back(v.grad),
            "d_rel": reld.grad.cpu()}, reld.grad


def _same_bits(a, b, names, tag):
    for n in names:
        assert torch.equal(a[n], b[n]), "%s: %s differs" % (tag, n)


# ------------------------------------------------------------------ 1. the case matrix
@pytest.mark.gpu
@pytest.mark.parametrize("case", _cases(SHAPES), ids=_id)
def test_relbias_forward_backward(cuda, case):
    """Raw bindings against the fp64 reference; ops.attention_relbias under autograd returns what
    the raw bindings return (bit for bit where the kernels are deterministic, d_rel within its bound)."""
    Sq, Sk, causal, p, bias = case
    inp, kb, rel, rel_base, keep, (seed, off), want = _expected(case)
    raw = _run_direct(cuda, inp, rel, rel_base, kb, causal, p, seed, off)
    _check(raw, want, kb, "direct " + _id(case), causal, p, rel_base)
    front, _ = _run_front(cuda, inp, rel, rel_base, kb, causal, p)
    _same_bits(front, raw, ("o", "dk", "dv") + (("dq",) if Sk <= 128 else ()), "front " + _id(case))
    _check(front, want, kb, "front " + _id(case), causal, p, rel_base)


# ------------------------------------------------------------------ 2. extra cases
@pytest.mark.gpu
@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
def test_slack_in_rel(cuda, causal):
    """rel longer than the offsets need (rel_base = Sq + 4, L = Sq + Sk + 9): every d_rel entry
    outside [rel_base - Sq + 1, rel_base + Sk - 1] is exactly 0 (written, not left over)."""
    case = (100, 72, causal, 0.1, "present")
    inp, kb, rel, rel_base, keep, (seed, off), want = _expected(case, 5)
    assert rel_base == 104 and rel.shape[1] == 181
    got = _run_direct(cuda, inp, rel, rel_base, kb, causal, 0.1, seed, off)
    _check(got, want, kb, "slack " + _id(case), causal, 0.1, rel_base)
    assert (got["d_rel"][:, :rel_base - 100 + 1] == 0).all() and (got["d_rel"][:, rel_base + 72:] == 0).all()
    assert (want["d_rel"][:, :rel_base - 100 + 1] == 0).all() and (want["d_rel"][:, rel_base + 72:] == 0).all()


@pytest.mark.gpu
def test_t5_call(cuda):
    """The call the T5 model makes: scale 1.0, inputs randn * 0.25, (64, 64), causal, p 0.1, key bias."""
    inp, kb, rel, rel_base, keep, (seed, off), want = _t5_expected()
    got = _run_direct(cuda, inp, rel, rel_base, kb, True, 0.1, seed, off, scale=1.0)
    _check(got, want, kb, "t5 call", True, 0.1, rel_base)


@pytest.mark.gpu
@pytest.mark.parametrize("Sq,Sk", [(100, 72), (160, 264)])
def test_fully_masked_batch(cuda, Sq, Sk):
    """-inf on every key of batch 0: every output is finite (lse +inf there), batch 0's o and
    gradients are zero, and d_rel equals the reference, to which batch 0 contributes nothing."""
    case = (Sq, Sk, False, 0.0, "inf0")
    inp, kb, rel, rel_base, keep, _, want = _expected(case)
    got = _run_direct(cuda, inp, rel, rel_base, kb, False, 0.0, 0, 0)
    assert (got["o"][0] == 0).all() and (got["lse"][0] == float("inf")).all()
    for n in ("dq", "dk", "dv"):
        assert torch.isfinite(got[n].float()).all() and (got[n][0] == 0).all(), n
    assert torch.isfinite(got["d_rel"]).all()
    one = {n: t[1:] for n, t in inp.items()}
    alone = _ref64(one, rel, rel_base, kb[1:])
    assert torch.allclose(alone["d_rel"], want["d_rel"], rtol=1e-12, atol=0)     # batch 0 adds nothing
    rest = {n: (t if n in ("d_rel", "A") else t[1:]) for n, t in want.items()}
    _check({n: (t if n == "d_rel" else t[1:]) for n, t in got.items()}, rest, None, "masked " + _id(case))


@pytest.mark.gpu
@pytest.mark.parametrize("Sq,Sk", [(64, 72), (160, 264)])
def test_transposed_rel_view(cuda, Sq, Sk):
    """rel passed as the transpose of a contiguous [L, H] tensor (what the T5 model passes): the same
    d_rel, returned in that view's layout."""
    case = (Sq, Sk, True, 0.1, "present")
    inp, kb, rel, rel_base, keep, (seed, off), want = _expected(case)
    view = rel.t().contiguous().to(cuda).t()
    assert not view.is_contiguous()
    front, grad = _run_front(cuda, inp, rel, rel_base, kb, True, 0.1, rel_dev=view)
    assert grad.shape == view.shape and grad.stride() == view.stride()
    _check(front, want, kb, "transposed rel " + _id(case), True, 0.1, rel_base)
    # the raw binding writes a strided d_rel too
    C = ops.require_native()
    q, k, v, do = (_bshd(inp[n], cuda) for n in ("q", "k", "v", "do"))
    o = torch.empty_like(q)
    relc = rel.to(cuda)
    lse = C.attn_fwd_relbias_train(q, k, v, o, kb.to(cuda), relc, rel_base, SCALE, 0.1, seed, off, True)
    outs = [torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)]
    d_t = torch.full((rel.shape[1], H0), float("nan"), device=cuda).t()
    C.attn_bwd_relbias(q, k, v, o, do, outs[0], outs[1], outs[2], d_t, kb.to(cuda), relc, rel_base, lse, SCALE, 0.1,
                       seed, off, True)
    _check({"d_rel": d_t.cpu()}, want, None, "strided d_rel " + _id(case), True, 0.1, rel_base)


@pytest.mark.gpu
@pytest.mark.parametrize("Sq,Sk", [(100, 72), (160, 264)])
def test_padded_views_distinct_strides(cuda, Sq, Sk):
    """test_attention_gpu.py's test_padded_views_write_nothing_outside for the relative-bias pair:
    q, k, v, dO, o, dq, dk, dv are padded views with eight different head strides (PAD_HS), the
    inputs' padding NaN, the outputs' a sentinel that must survive; d_rel is a transposed [L, H]
    view filled with NaN.  Strides of one tensor used for another read NaN or hit a sentinel."""
    case = (Sq, Sk, True, 0.1, "present")
    inp, kb, rel, rel_base, keep, (seed, off), want = _expected(case)
    C = ops.require_native()
    t = {}
    for n, S in (("q", Sq), ("k", Sk), ("v", Sk), ("do", Sq)):
        _, t[n], _ = _padded(cuda, B0, S, H0, PAD_HS[n], 0x7FC0, _bshd(inp[n], cuda))
    out = {n: _padded(cuda, B0, S, H0, PAD_HS[n]) for n, S in (("o", Sq), ("dq", Sq), ("dk", Sk), ("dv", Sk))}
    assert len({v.stride()[:3] for v in list(t.values()) + [view for _, view, _ in out.values()]}) == 8
    kbd, reld = kb.to(cuda), rel.to(cuda)
    d_rel = torch.full((rel.shape[1], H0), float("nan"), device=cuda).t()
    lse = C.attn_fwd_relbias_train(t["q"], t["k"], t["v"], out["o"][1], kbd, reld, rel_base, SCALE, 0.1, seed, off, True)
    C.attn_bwd_relbias(t["q"], t["k"], t["v"], out["o"][1], t["do"], out["dq"][1], out["dk"][1], out["dv"][1], d_rel,
                       kbd, reld, rel_base, lse, SCALE, 0.1, seed, off, True)
    torch.cuda.synchronize()
    for n, (buf, _, mask) in out.items():
        assert _untouched(buf, mask), "%s: written outside its valid region" % n
    got = {n: _back(view) for n, (_, view, _) in out.items()}
    got.update(lse=lse.view(B0, H0, Sq).cpu(), d_rel=d_rel.cpu())
    _check(got, want, kb, "padded " + _id(case), True, 0.1, rel_base)


@pytest.mark.gpu
@pytest.mark.parametrize("Sq,Sk", [(100, 72), (160, 264)])
def test_same_seed_same_bits(cuda, Sq, Sk):
    """Two runs from the same seed: bit-equal o, lse, dk, dv, and dq for Sk <= 128 (Sk > 128 sums dQ
    with fp32 atomics); d_rel within its bound of the reference both times, no bit test on it."""
    case = (Sq, Sk, True, 0.1, "present")
    inp, kb, rel, rel_base, keep, (seed, off), want = _expected(case)
    a = _run_direct(cuda, inp, rel, rel_base, kb, True, 0.1, seed, off)
    b = _run_direct(cuda, inp, rel, rel_base, kb, True, 0.1, seed, off)
    _same_bits(a, b, ("o", "lse", "dk", "dv") + (("dq",) if Sk <= 128 else ()), "rerun " + _id(case))
    for r in (a, b):
        _check({"d_rel": r["d_rel"]}, want, None, "rerun d_rel " + _id(case), True, 0.1, rel_base)
    other = _run_direct(cuda, inp, rel, rel_base, kb, True, 0.1, seed + 1, off)
    assert not torch.equal(other["o"], a["o"])


@pytest.mark.gpu
@pytest.mark.parametrize("Sq,Sk", [(64, 72), (160, 264)])
def test_no_grad_p0_is_the_inference_call(cuda, Sq, Sk):
    """Without a gradient and without dropout the front end still makes the inference call:
    bit-equal to attn_fwd_relbias; and the training forward at p = 0 computes the same bits."""
    case = (Sq, Sk, True, 0.0, "present")
    inp, kb, rel, rel_base, _, _, want = _expected(case)
    C = ops.require_native()
    q, k, v = (_bshd(inp[n], cuda) for n in ("q", "k", "v"))
    o = torch.empty_like(q)
    C.attn_fwd_relbias(q, k, v, o, kb.to(cuda), rel.to(cuda), rel_base, SCALE, True)
    front = ops.attention_relbias(q, k, v, rel.to(cuda), rel_base, kb.to(cuda), scale=SCALE, causal=True)
    assert torch.equal(front, o)
    with torch.no_grad():
        front = ops.attention_relbias(q.clone().requires_grad_(), k, v, rel.to(cuda), rel_base, kb.to(cuda),
                                      scale=SCALE, causal=True, p=0.0)
    assert torch.equal(front, o)
    o2 = torch.empty_like(q)
    C.attn_fwd_relbias_train(q, k, v, o2, kb.to(cuda), rel.to(cuda), rel_base, SCALE, 0.0, 0, 0, True)
    assert torch.equal(o2, o)


# ------------------------------------------------------------------ 3. refusals and routing
SENTINEL = 0x7FA5      # a bf16 NaN bit pattern no kernel produces
SENTINEL32 = 0x7FA55AA5


def _sentinel_like(t):
    out = torch.empty_like(t)
    if t.dtype == torch.bfloat16:
        out.view(torch.int16).fill_(SENTINEL)
    else:
        out.view(torch.int32).fill_(SENTINEL32)
    return out


def _is_sentinel(t):
    if t.dtype == torch.bfloat16:
        return bool((t.view(torch.int16) == SENTINEL).all())
    return bool((t.view(torch.int32) == SENTINEL32).all())


_REFUSALS = {
    # name: (Sq, Sk, L, rel_base, p, misaligned o, message)
    "L4097": (40, 40, 4097, 39, 0.0, False, "rc=-4"),
    "rel_base_short": (40, 40, 79, 38, 0.0, False, "does not cover"),
    "L_short": (40, 40, 78, 39, 0.0, False, "does not cover"),
    "odd_sk_dropout": (96, 63, 158, 95, 0.1, False, "rc=-2"),
    "misaligned_o": (40, 40, 79, 39, 0.0, True, "rc=-7"),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(_REFUSALS))
def test_refusals_write_nothing(cuda, name):
    """Calls the new bindings refuse raise and leave sentinel-filled outputs untouched: L = 4097, a
    rel that does not cover every offset, odd Sk with p > 0, a misaligned o (forward) / dk (backward)."""
    Sq, Sk, L, rel_base, p, misaligned, msg = _REFUSALS[name]
    C = ops.require_native()
    inp = _inputs(B0, H0, Sq, Sk)
    q, k, v, do = (_bshd(inp[n], cuda) for n in ("q", "k", "v", "do"))
    rel = torch.zeros(H0, L, device=cuda)
    if misaligned:
        buf = torch.full((8 + B0 * Sq * H0 * 64,), SENTINEL, dtype=torch.int16, device=cuda).view(torch.bfloat16)
        o = buf.as_strided((B0, Sq, H0, D), (Sq * H0 * 64, H0 * 64, 64, 1), 4)
    else:
        o = _sentinel_like(q)
    with pytest.raises(RuntimeError, match=msg):
        C.attn_fwd_relbias_train(q, k, v, o, None, rel, rel_base, SCALE, p, SEED, 0, False)
    torch.cuda.synchronize()
    assert _is_sentinel(buf if misaligned else o)
    # the backward refuses the same call (a misaligned dk stands in for the misaligned o)
    good_o = torch.zeros_like(q)
    lse = torch.zeros(B0 * H0, Sq, device=cuda)
    dq, dv, d_rel = _sentinel_like(q), _sentinel_like(v), _sentinel_like(rel)
    if misaligned:
        kbuf = torch.full((8 + B0 * Sk * H0 * 64,), SENTINEL, dtype=torch.int16, device=cuda).view(torch.bfloat16)
        dk = kbuf.as_strided((B0, Sk, H0, D), (Sk * H0 * 64, H0 * 64, 64, 1), 4)
    else:
        dk = _sentinel_like(k)
    with pytest.raises(RuntimeError, match=msg):
        C.attn_bwd_relbias(q, k, v, good_o, do, dq, dk, dv, d_rel, None, rel, rel_base, lse, SCALE, p, SEED, 0, False)
    torch.cuda.synchronize()
    for t in (dq, kbuf if misaligned else dk, dv, d_rel):
        assert _is_sentinel(t)


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["odd_sk_dropout", "long_sq"])
def test_front_end_routes_to_reference(cuda, how):
    """Calls the kernels cannot take go to the PyTorch reference, on the stream the front end drew:
    odd Sk with p > 0, and an Sq whose backward windows exceed the LDS budget (the binding refuses
    it with rc=-9 and writes nothing)."""
    C = ops.require_native()
    if how == "odd_sk_dropout":
        B, H, Sq, Sk, p = B0, H0, 96, 63, 0.1
    else:
        B, H, Sq, Sk, p = 1, 1, 1860, 8, 0.0
        assert C.attn_bwd_relbias_window(Sq) > C.attn_bwd_relbias_max_window() >= C.attn_bwd_relbias_window(1856)
    inp = _inputs(B, H, Sq, Sk)
    rel_base, L = Sq - 1, Sq + Sk - 1
    rel = _rel_vec(H, L).to(cuda)
    q, k, v, do = (_bshd(inp[n], cuda) for n in ("q", "k", "v", "do"))
    if how == "long_sq":
        o = torch.empty_like(q)
        lse = C.attn_fwd_relbias_train(q, k, v, o, None, rel, rel_base, SCALE, 0.0, 0, 0, False)   # the forward runs
        outs = [_sentinel_like(q), _sentinel_like(k), _sentinel_like(v), _sentinel_like(rel)]
        with pytest.raises(RuntimeError, match="rc=-9"):
            C.attn_bwd_relbias(q, k, v, o, do, outs[0], outs[1], outs[2], outs[3], None, rel, rel_base, lse, SCALE, 0.0,
                               0, 0, False)
        torch.cuda.synchronize()
        assert all(_is_sentinel(t) for t in outs)
    leaves = [t.detach().requires_grad_() for t in (q, k, v, rel)]
    ops.manual_seed(SEED)
    got = ops.attention_relbias(*leaves, rel_base, None, scale=SCALE, causal=False, p=p)
    got.backward(do)
    ops.manual_seed(SEED)
    seed, off = ops._rng.next(B * H * Sq * Sk) if p > 0 else (0, 0)
    leaves2 = [t.detach().requires_grad_() for t in (q, k, v, rel)]
    want = _relbias_reference(*leaves2, rel_base, None, SCALE, False, p, seed, off)
    want.backward(do)
    assert torch.equal(got, want)
    # the same computation twice; only the order of PyTorch's own atomic adds (the bias gather's
    # backward) may differ between the two
    for a, b in zip(leaves, leaves2):
        assert torch.isfinite(a.grad).all()
        assert (a.grad.float() - b.grad.float()).abs().max() <= 1e-3 * b.grad.float().abs().max()


# ------------------------------------------------------------------ 4. the kernels that ran
@pytest.mark.gpu
def test_rel_kernels_selected(cuda):
    """The kernels that actually ran, by name from the profiler, are the REL instantiations the
    dispatcher documents, for one shape per row of the table."""
    from torch.profiler import ProfilerActivity, profile
    for Sq, Sk in ROW_SHAPES:
        p = 0.1 if Sk % 2 == 0 else 0.0
        drop = "true" if p > 0 else "false"
        fwd = "attn_fwd_d64_kernel<%s, true, true, 2, false>" % drop
        bwd = "attn_bwd_d64_rel_kernel<%s, true, %s>" % (drop, "true" if Sk > 128 else "false")
        inp = _inputs(B0, H0, Sq, Sk)
        rel = _rel_vec(H0, Sq + Sk - 1)
        _run_direct(cuda, inp, rel, Sq - 1, None, True, p, SEED, 0)              # warm: module load, allocations
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            _run_direct(cuda, inp, rel, Sq - 1, None, True, p, SEED, 0)
            torch.cuda.synchronize()
        names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "attn_" in e.name]
        assert any(fwd in n for n in names), (Sq, Sk, fwd, names)
        assert any(bwd in n for n in names), (Sq, Sk, bwd, names)
        assert sum("attn_fwd" in n for n in names) == 1 and sum("attn_bwd" in n for n in names) == 1, names
        assert sum("attn_drel_reduce_kernel" in n for n in names) == 1, names
        assert any("attn_dq_convert_kernel" in n for n in names) == (Sk > 128), names
