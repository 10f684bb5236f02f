"""Head-dim-128 inference attention (``attn_fwd_d128_kernel`` in ops/csrc/attention.hip).

Method of tests/test_attention_gpu.py, with helpers of its own.  Every case compares the kernel
with an fp64 reference computed from the same bf16 inputs (``_ref64``), per (batch, head, row):

* ``o``: max |kernel - ref| over the 128 columns divided by (max |ref| over that row + 1e-3 x
  the tensor's max |ref|); the assertion is on the worst row.
* ``lse`` (log2 domain): absolute difference per row.

BOUNDS.  Not taken from the kernel.  ``_model`` is a CPU model of the kernel's arithmetic that
rounds only where it rounds: fp32 scores (log2 domain) and accumulation, P rounded to bf16 before
its MFMA, O rounded to bf16.  Its worst per-row error against the fp64 reference over the whole
case matrix below (measured on a CPU) is

    | quantity                   | model worst | bound (4 x) |
    |----------------------------|-------------|-------------|
    | o                          | 5.83e-3     | 2.33e-2     |
    | lse (absolute, log2 units) | 6.86e-7     | 2.74e-6     |

and each bound is 4 x that (``BOUND``), the factor of the d64 file: it covers accumulation order,
the exp2-domain online-softmax rescaling and the hardware exp2.
``test_rounding_model_meets_bounds`` re-runs the model over the matrix.

CASE MATRIX (B = 2, H = 3, D = 128, inputs randn * 0.5, scale 1/sqrt(128)), crossed with causal x
key bias {none, present, inf0 = one batch row fully masked} x {plain, REL with rel_base = Sq - 1,
L = Sq + Sk - 1}.  The kernel's K/V tile is 64 keys in a two-deep ring, as in the d64 kernel, so
the tile and ring boundaries are those of the issue's table:

| (Sq, Sk)            | what it reaches                                                    |
|---------------------|--------------------------------------------------------------------|
| (1, 64), (40, 40)   | one K/V tile, full and partial; a lone query (three idle waves)     |
| (128, 128), (64, 72)| two tiles loaded up front (no barrier in the loop), full q-block    |
| (1, 200), (33, 130) | streamed ring, a tail tile of 8 and of 2 keys; the decode shape     |
| (129, 65)           | a second q-block holding one query                                 |
| (96, 63)            | odd Sk                                                             |

plus one REL case at scale 1.0 on inputs randn * 0.25 ((33, 130), key bias present): how T5 calls
the kernel.  Every case also calls the front end (``ops.attention_relbias`` / ``ops.attention``)
and asserts that it returns the kernel's bits.

The causal mask is top-left aligned (key index > query index is masked), also when Sq != Sk.
"""
import functools
import math

import pytest
import torch

from cloudtik_amd import ops
from cloudtik_amd.ops import reference as ref

D = 128
B0, H0 = 2, 3
SCALE = 1.0 / math.sqrt(128.0)
LN2 = math.log(2.0)
LOG2E = 1.0 / LN2

# worst per-row error of _model against _ref64 over the whole matrix (see the module docstring)
MODEL_WORST = {"o": 5.83e-3, "lse": 6.86e-7}
BOUND = {k: 4.0 * v for k, v in MODEL_WORST.items()}

SHAPES = [(1, 64), (40, 40), (128, 128), (64, 72), (1, 200), (33, 130), (129, 65), (96, 63)]
BIASES = ("none", "present", "inf0")
# (Sq, Sk, causal, bias, rel, t5): t5 = scale 1.0 on inputs randn * 0.25
CASES = [(Sq, Sk, causal, bias, rel, False) for Sq, Sk in SHAPES for causal in (False, True) for bias in BIASES
         for rel in (False, True)] + [(33, 130, False, "present", True, True)]


def _id(c):
    return "%dx%d-%s-%s-%s%s" % (c[0], c[1], "causal" if c[2] else "full", c[3], "rel" if c[4] else "plain",
                                 "-t5" if c[5] else "")


# ------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=None)
def _inputs(B, H, Sq, Sk, amp=0.5):
    g = torch.Generator().manual_seed(2000 * Sq + Sk)
    q = (torch.randn(B, H, Sq, D, generator=g) * amp).bfloat16()
    k = (torch.randn(B, H, Sk, D, generator=g) * amp).bfloat16()
    v = (torch.randn(B, H, Sk, D, generator=g) * amp).bfloat16()
    return {"q": q, "k": k, "v": v}


def _key_bias(B, Sk, kind):
    """none | present: a small finite bias on every key plus -10000 on the last quarter of the keys
    of batch 1 only (so batch indexing matters) | inf0: -inf on every key of batch 0."""
    if kind == "none":
        return None
    g = torch.Generator().manual_seed(177 + Sk)
    kb = torch.randn(B, Sk, generator=g) * 0.5
    if kind == "present":
        kb[1, Sk - Sk // 4:] = -10000.0
    else:
        kb[0] = float("-inf")
    return kb


def _rel_matrix(rel, rel_base, Sq, Sk):
    idx = torch.arange(Sk)[None, :] - torch.arange(Sq)[:, None] + rel_base
    return rel[:, idx]                                                   # [H, Sq, Sk]


# ------------------------------------------------------------------ fp64 reference
def _ref64(inp, kb=None, causal=False, relm=None, masked=None, scale=SCALE):
    """fp64 forward from the bf16 inputs ([B, H, S, 128]).  ``masked`` ([.., Sq, Sk] bool) overrides
    the causal mask (the checker tests shift it).  Rows with every key masked get P = 0: O = 0,
    lse = +inf (what the kernel defines)."""
    q, k, v = (inp[n].double() for n in ("q", "k", "v"))
    Sq, Sk = q.shape[2], k.shape[2]
    s = q @ k.transpose(-1, -2) * scale
    if kb is not None:
        s = s + kb.double()[:, None, None, :]
    if relm is not None:
        s = s + relm.double()[None]
    if masked is None and causal:
        masked = torch.ones(Sq, Sk, dtype=torch.bool).triu(1)
    if masked is not None:
        s = s.masked_fill(masked, float("-inf"))
    m = s.amax(-1, keepdim=True)
    m = torch.where(torch.isinf(m), torch.zeros_like(m), m)
    e = torch.exp(s - m)
    l = e.sum(-1, keepdim=True)
    one = torch.ones_like(l)
    pr = e / torch.where(l > 0, l, one)
    lse = torch.where(l > 0, m + torch.log(torch.where(l > 0, l, one)), torch.full_like(l, float("inf"))).squeeze(-1)
    return {"o": pr @ v, "lse": lse / LN2}


# ------------------------------------------------------------------ CPU rounding model of the kernel
def _bf(x):
    return x.bfloat16().float()


def _model(inp, kb=None, causal=False, relm=None, scale=SCALE):
    """What the kernel computes, with its rounding steps and nothing else: fp32 scores in the log2
    domain, fp32 row sum, P rounded to bf16 before P.V, fp32 accumulation, O rounded to bf16."""
    q, k, v = (inp[n].float() for n in ("q", "k", "v"))
    Sq, Sk = q.shape[2], k.shape[2]
    sl2 = torch.tensor(scale, dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32)
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
    one = torch.ones_like(l)
    inv = torch.where(l > 0, 1.0 / torch.where(l > 0, l, one), torch.zeros_like(l))
    o = _bf((_bf(pu) @ v) * inv)
    lse = torch.where(l > 0, m + torch.log2(torch.where(l > 0, l, one)), torch.full_like(l, float("inf")))
    return {"o": o, "lse": lse.squeeze(-1)}


# ------------------------------------------------------------------ metric and checker
def _rows(x, want):
    """Per-row error [..., S]: max |x - want| over the 128 columns / (max |want| over the row +
    1e-3 of the tensor's max |want|)."""
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


def _errors(got, want):
    return {n: _lse_err(t, want[n]) if n == "lse" else _rows(t, want[n]).max().item() for n, t in got.items()}


def _check(got, want, tag=""):
    """The assertions of every case: finite outputs (lse = +inf where the reference has it) and
    every quantity within its bound on its worst row."""
    errs = _errors(got, want)
    print("attn128-err %s %s" % (tag, " ".join("%s=%.3e" % kv for kv in sorted(errs.items()))))
    for n, t in got.items():
        ok = torch.isfinite(t.double()) | (torch.isinf(want[n]) & (t.double() == want[n]))
        assert ok.all(), "%s: %s has %d non-finite values" % (tag, n, int((~ok).sum()))
    for n, e in errs.items():
        assert e <= BOUND[n], "%s: %s worst row error %.3e > bound %.3e" % (tag, n, e, BOUND[n])
    return errs


@functools.lru_cache(maxsize=None)
def _expected(case):
    """Inputs, key bias, relative-bias vector and the fp64 reference of one case: computed once,
    shared by every test that needs it, never modified."""
    Sq, Sk, causal, bias, rel, t5 = case
    inp = _inputs(B0, H0, Sq, Sk, 0.25 if t5 else 0.5)
    kb = _key_bias(B0, Sk, bias)
    relv = relm = None
    if rel:
        g = torch.Generator().manual_seed(15 + Sq)
        relv = torch.randn(H0, Sq + Sk - 1, generator=g) * 0.5
        relm = _rel_matrix(relv, Sq - 1, Sq, Sk)
    scale = 1.0 if t5 else SCALE
    return inp, kb, relv, relm, scale, _ref64(inp, kb, causal, relm, scale=scale)


# ------------------------------------------------------------------ the checker itself, on the CPU
def test_rounding_model_meets_bounds():
    """The model that the bounds come from passes them (by a factor of 4) on every case of the
    matrix; prints its worst error per quantity."""
    worst = {n: 0.0 for n in BOUND}
    for case in CASES:
        inp, kb, _, relm, scale, want = _expected(case)
        got = _model(inp, kb, case[2], relm, scale)
        for n, e in _check(got, want, "model " + _id(case)).items():
            worst[n] = max(worst[n], e)
    print("model worst:", " ".join("%s=%.3e" % kv for kv in sorted(worst.items())))
    for n in BOUND:     # the recorded figures are the model's, give or take another CPU's summation order
        assert MODEL_WORST[n] / 2 <= worst[n] <= MODEL_WORST[n] * 2, (n, worst[n], MODEL_WORST[n])


def _fails(got, want, tag=""):
    with pytest.raises(AssertionError):
        _check(got, want, tag)


def test_checker_catches_zeroed_output_row():
    case = (128, 128, False, "none", False, False)
    want = _expected(case)[-1]
    got = {n: t.clone() for n, t in want.items()}
    _check(got, want, "reference against itself")
    got["o"][1, 2, 100] = 0
    _fails(got, want, "zeroed row")


def test_checker_catches_shifted_causal_diagonal():
    """The causal diagonal shifted by one (key q + 1 admitted) for one 32-row tile of one head."""
    case = (128, 128, True, "none", False, False)
    inp, kb, _, _, _, want = _expected(case)
    masked = torch.ones(128, 128, dtype=torch.bool).triu(1).expand(B0, H0, 128, 128).clone()
    masked[1, 2, 64:96] = torch.ones(128, 128, dtype=torch.bool).triu(2)[64:96]
    got = _ref64(inp, kb, True, masked=masked)
    _fails(got, want, "shifted diagonal")
    _fails({"o": got["o"]}, want, "shifted diagonal, o alone")


def test_checker_catches_key_past_sk():
    """One key past Sk admitted with a zero score (a tail key that the -inf bias failed to mask):
    every row of O shrinks by about 1 / (Sk + 1); lse moves by about log2(1 + 1 / Sk)."""
    case = (96, 63, False, "none", False, False)
    inp, kb, _, _, _, want = _expected(case)
    z = torch.zeros(B0, H0, 1, D, dtype=torch.bfloat16)
    ghost = {"q": inp["q"], "k": torch.cat([inp["k"], z], 2), "v": torch.cat([inp["v"], z], 2)}
    got = _ref64(ghost)
    _fails(got, want, "key past Sk")
    _fails({"lse": got["lse"]}, want, "key past Sk, lse alone")


# ------------------------------------------------------------------ GPU runners
def _bshd(t, dev):
    """[B, H, S, 128] (CPU, contiguous) -> the [B, S, H, 128] view of a device copy."""
    return t.to(dev).transpose(1, 2)


def _back(t):
    return t.transpose(1, 2).cpu()


def _call(C, q, k, v, o, kbd, reld, rel_base, scale, causal):
    if reld is not None:
        return C.attn_fwd_relbias(q, k, v, o, kbd, reld, rel_base, scale, causal)
    return C.attn_fwd(q, k, v, o, kbd, scale, 0.0, 0, 0, causal)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_d128_forward(cuda, case):
    """attn_fwd / attn_fwd_relbias at D = 128: o and lse per row against the fp64 reference; a
    fully masked batch gives o == 0 and lse == +inf; the front end returns the same bits."""
    Sq, Sk, causal, bias, rel, t5 = case
    inp, kb, relv, relm, scale, want = _expected(case)
    C = ops.require_native()
    q, k, v = (_bshd(inp[n], cuda) for n in ("q", "k", "v"))
    kbd = kb.to(cuda) if kb is not None else None
    reld = relv.to(cuda) if rel else None
    o = torch.empty_like(q)
    lse = _call(C, q, k, v, o, kbd, reld, Sq - 1, scale, causal)
    got = {"o": _back(o), "lse": lse.view(B0, H0, Sq).cpu()}
    _check(got, want, _id(case))
    if bias == "inf0":
        assert (got["o"][0] == 0).all() and (got["lse"][0] == float("inf")).all()
    if rel:
        front = ops.attention_relbias(q, k, v, reld, Sq - 1, kbd, scale=scale, causal=causal)
        assert torch.equal(front, o)
    else:
        front = ops.attention(q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2), kbd, scale=scale, causal=causal)
        assert torch.equal(front.transpose(1, 2), o)


# ------------------------------------------------------------------ strided views
SENTINEL = 0x7FA5      # a bf16 NaN bit pattern no kernel produces


def _sentinel(dev, *shape):
    return torch.full(shape, SENTINEL, dtype=torch.int16, device=dev).view(torch.bfloat16)


def _untouched(buf, mask):
    return bool((buf.view(torch.int16)[~mask] == SENTINEL).all())


def _padded_out(dev, B, S, H, hs):
    """A [B, S, H, 128] view into a larger buffer: 3 extra rows after S, head stride hs (136, not
    128), a 16-element gap between batches, an 8-element (16-byte) offset from the base."""
    ss = H * hs
    sb = (S + 3) * ss + 16
    n = 8 + B * sb + 8
    buf = _sentinel(dev, n)
    geom = ((B, S, H, D), (sb, ss, hs, 1), 8)
    mask = torch.zeros(n, dtype=torch.bool, device=dev)
    mask.as_strided(*geom).fill_(True)
    return buf, buf.as_strided(*geom), mask


@pytest.mark.gpu
@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("Sq,Sk", [(100, 72), (33, 130)])
def test_strided_views(cuda, Sq, Sk, causal):
    """K and V are slices of two caches of different lengths and head counts, q comes out of a
    packed [B, Sq, 3, H, D] projection, o is a padded view.  Everything outside the views holds a NaN sentinel: results
    stay within bounds (so no padding was read into them) and no sentinel changes."""
    inp = _inputs(B0, H0, Sq, Sk)
    kb = _key_bias(B0, Sk, "present")
    g = torch.Generator().manual_seed(15 + Sq)
    relv = torch.randn(H0, Sq + Sk - 1, generator=g) * 0.5
    C = ops.require_native()
    # the V cache is longer and has one head more than the K cache, so q, k, v and o have four
    # different (batch, row, head) stride triples: one tensor's strides used for another show
    kc, vc = _sentinel(cuda, B0, Sk + 5, H0, D), _sentinel(cuda, B0, Sk + 9, H0 + 1, D)
    kc[:, :Sk] = _bshd(inp["k"], cuda)
    vc[:, :Sk, :H0] = _bshd(inp["v"], cuda)
    packed = _sentinel(cuda, B0, Sq, 3, H0, D)
    packed[:, :, 0] = _bshd(inp["q"], cuda)
    q, k, v = packed.view(B0, Sq, 3 * H0 * D).view(B0, Sq, 3, H0, D)[:, :, 0], kc[:, :Sk], vc[:, :Sk, :H0]
    snap = [t.clone() for t in (kc, vc, packed)]
    for rel in (False, True):
        want = _ref64(inp, kb, causal, _rel_matrix(relv, Sq - 1, Sq, Sk) if rel else None)
        buf, o, mask = _padded_out(cuda, B0, Sq, H0, 136)
        assert len({t.stride()[:3] for t in (q, k, v, o)}) == 4
        lse = _call(C, q, k, v, o, kb.to(cuda), relv.to(cuda) if rel else None, Sq - 1, SCALE, causal)
        torch.cuda.synchronize()
        assert _untouched(buf, mask), "o: written outside its valid region"
        for t, s in zip((kc, vc, packed), snap):
            assert torch.equal(t.view(torch.int16), s.view(torch.int16))
        _check({"o": _back(o), "lse": lse.view(B0, H0, Sq).cpu()}, want,
               "views %dx%d %s %s" % (Sq, Sk, "causal" if causal else "full", "rel" if rel else "plain"))


# ------------------------------------------------------------------ dispatch
def _attn_kernels(fn):
    from torch.profiler import ProfilerActivity, profile
    fn()                                                                  # warm: module load, allocations
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "attn_" in e.name]


@pytest.mark.gpu
def test_kernels_selected(cuda):
    """By name from the profiler: a D = 128 call runs attn_fwd_d128_kernel<CAUSAL, REL>, and a
    D = 64 call in the same process still runs attn_fwd_d64_kernel."""
    C = ops.require_native()
    inp = _inputs(B0, H0, 40, 40)
    q, k, v = (_bshd(inp[n], cuda) for n in ("q", "k", "v"))
    o = torch.empty_like(q)
    reld = torch.zeros(H0, 79, device=cuda)
    for causal in (False, True):
        for rel in (False, True):
            names = _attn_kernels(lambda: _call(C, q, k, v, o, None, reld if rel else None, 39, SCALE, causal))
            want = "attn_fwd_d128_kernel<%s, %s>" % ("true" if causal else "false", "true" if rel else "false")
            assert len(names) == 1 and want in names[0], (want, names)
    q64, k64, v64 = (t[..., :64].contiguous() for t in (q, k, v))
    o64 = torch.empty_like(q64)
    names = _attn_kernels(lambda: C.attn_fwd(q64, k64, v64, o64, None, 0.125, 0.0, 0, 0, False))
    assert len(names) == 1 and "attn_fwd_d64_kernel<false, false, false" in names[0], names
    names = _attn_kernels(lambda: C.attn_fwd_relbias(q64, k64, v64, o64, None, reld, 39, 0.125, True))
    assert len(names) == 1 and "attn_fwd_d64_kernel<false, true, true" in names[0], names


# ------------------------------------------------------------------ refusals and routing
@pytest.mark.gpu
def test_refusals(cuda):
    """Each a Python exception, nothing launched (the sentinel in o survives)."""
    C = ops.require_native()
    inp = _inputs(B0, H0, 40, 40)
    q, k, v = (_bshd(inp[n], cuda) for n in ("q", "k", "v"))
    o = _sentinel(cuda, B0, 40, H0, D)
    o64 = _sentinel(cuda, B0, 40, H0, 64)
    rel = torch.zeros(H0, 79, device=cuda)
    # mixed last dimensions
    for args in ((q[..., :64], k, v, o), (q, k[..., :64], v, o), (q, k, v[..., :64], o), (q, k, v, o64)):
        with pytest.raises(RuntimeError, match="same head dim"):
            C.attn_fwd(*args, None, SCALE, 0.0, 0, 0, False)
        with pytest.raises(RuntimeError, match="same head dim"):
            C.attn_fwd_relbias(*args, None, rel, 39, SCALE, False)
    # dropout
    with pytest.raises(RuntimeError, match="no dropout"):
        C.attn_fwd(q, k, v, o, None, SCALE, 0.1, 3, 0, False)
    # backward
    lse = torch.zeros(B0 * H0, 40, device=cuda)
    outs = [_sentinel(cuda, B0, 40, H0, D) for _ in range(3)]
    with pytest.raises(RuntimeError, match="forward only"):
        C.attn_bwd(q, k, v, q, q, outs[0], outs[1], outs[2], None, lse, SCALE, 0.0, 0, 0, False)
    # an output that is not 16-byte addressable
    buf = _sentinel(cuda, 8 + B0 * 40 * H0 * 132)
    for geom in (((B0, 40, H0, D), (40 * H0 * 128, H0 * 128, 128, 1), 4),
                 ((B0, 40, H0, D), (40 * H0 * 132, H0 * 132, 132, 1), 0)):
        bad = buf.as_strided(*geom)
        with pytest.raises(RuntimeError, match="rc=-7"):
            C.attn_fwd(q, k, v, bad, None, SCALE, 0.0, 0, 0, False)
        with pytest.raises(RuntimeError, match="rc=-7"):
            C.attn_fwd_relbias(q, k, v, bad, None, rel, 39, SCALE, False)
    # relb longer than 4096; rel_base < Sq - 1
    with pytest.raises(RuntimeError, match="rc=-4"):
        C.attn_fwd_relbias(q, k, v, o, None, torch.zeros(H0, 4097, device=cuda), 39, SCALE, False)
    with pytest.raises(RuntimeError, match="does not cover"):
        C.attn_fwd_relbias(q, k, v, o, None, rel, 38, SCALE, False)
    torch.cuda.synchronize()
    for t in [o, o64, buf] + outs:
        assert bool((t.view(torch.int16) == SENTINEL).all())


@pytest.mark.gpu
def test_attention_routes_gradient_calls_to_reference(cuda):
    """ops.attention at D = 128 with inputs that require grad, under grad mode: the reference's
    result, and it backpropagates.  Under no_grad the same tensors take the kernel."""
    inp = _inputs(B0, H0, 40, 40)
    q, k, v = (inp[n].to(cuda).requires_grad_() for n in ("q", "k", "v"))
    got = ops.attention(q, k, v, scale=SCALE, causal=True)
    assert torch.equal(got, ref.attention(q, k, v, None, 0.0, 0, 0, SCALE, True))
    got.float().sum().backward()
    assert all(t.grad is not None and torch.isfinite(t.grad.float()).all() for t in (q, k, v))
    with torch.no_grad():
        names = _attn_kernels(lambda: ops.attention(q, k, v, scale=SCALE, causal=True))
    assert len(names) == 1 and "attn_fwd_d128_kernel<true, false>" in names[0], names


@pytest.mark.gpu
def test_attention_routes_dropout_to_reference(cuda):
    """ops.attention at D = 128 with p > 0: exactly what ops.reference.attention computes with the
    stream the wrapper drew."""
    inp = _inputs(B0, H0, 40, 40)
    q, k, v = (inp[n].to(cuda) for n in ("q", "k", "v"))
    ops.manual_seed(11)
    got = ops.attention(q, k, v, p=0.1, scale=SCALE)
    ops.manual_seed(11)
    seed, off = ops._rng.next(B0 * H0 * 40 * 40)
    assert torch.equal(got, ref.attention(q, k, v, None, 0.1, seed, off, SCALE))
