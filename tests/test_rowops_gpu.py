"""LayerNorm / RMSNorm, bias + activation, dropout, embedding3 and cross-entropy kernels
(ops/csrc/layernorm.hip, elementwise.hip, xent.hip): per-row and per-column fp64 checks on every
dispatch path and tail.

REFERENCE.  Every case compares the HIP kernels with an fp64 reference of the same operation
computed in plain PyTorch from the same bf16 inputs (``_ln_fwd`` / ``_ln_bwd`` / ``_ba`` /
``_emb`` with ``dt = F64``).  Where a kernel normalises a rounded intermediate the reference takes
the same definition: the kernel normalises the rounded ``s = bf16(res + dropout(x + bias))``, so ``s``
is checked on its own (below) and the reference normalises that same bf16 ``s`` in fp64.
The backward kernels are handed the reference's own ``s`` (bf16), ``mean`` / ``rstd`` (rounded to
fp32) and, for the output form, ``bf16(y)``, so forward and backward are checked apart.  The
output-form backward (FROMY, xhat = (y - beta) / gamma) is compared with the true gradient at
``s``; a channel whose gamma is exactly 0 has xhat 0 by the kernel's definition, and the
reference takes that definition for that channel.

METRIC (that of test_attention_gpu.py).
* row tensors (``y``, ``ds``, ``dx``, ``dz``, embedding table gradients): per row,
  max |kernel - ref| / (max |ref| over the row + 1e-3 x the tensor's max |ref|); worst row.
* column sums (``dgamma``, ``dbeta``, ``dbias``): per column, |kernel - ref| /
  (sum of |terms| of that column, the buffer's previous value included, + 1e-3 x the largest such
  sum); worst column.  The sums cancel, so max |ref| is no scale for them.
* ``mean``, ``rstd``: |kernel - ref| / max(1, |ref|) per row (absolute below 1, relative above).

BOUNDS.  Not taken from a kernel.  The same functions with ``dt = F32`` are a CPU model that
rounds only where the kernels round: fp32 sums and statistics, bf16 ``s``, ``y``, ``ds``, ``dx``,
``dz``, parameter gradients in the dtype of their buffer.  Its worst error against the fp64
reference over the whole case matrix below (measured on a CPU) and the bound, 4 x that
(accumulation order, ``rsqrtf`` / ``__expf``, the kernels' erf approximation):

    | quantity                                   | model worst | bound (4 x) |
    |--------------------------------------------|-------------|-------------|
    | ``y``: LayerNorm / RMSNorm y               | 3.89e-03    | 1.56e-02    |
    | ``mean``: mean                             | 2.98e-08    | 1.19e-07    |
    | ``rstd``: rstd                             | 2.25e-07    | 9.00e-07    |
    | ``ds``: ds                                 | 3.88e-03    | 1.55e-02    |
    | ``dx``: dx                                 | 3.89e-03    | 1.56e-02    |
    | ``dgamma_f32``                             | 1.76e-07    | 7.04e-07    |
    | ``dgamma_bf16``                            | 3.81e-03    | 1.52e-02    |
    | ``dbeta_f32``                              | 5.87e-08    | 2.35e-07    |
    | ``dbeta_bf16``                             | 3.88e-03    | 1.55e-02    |
    | ``dbias_f32``                              | 1.55e-07    | 6.20e-07    |
    | ``dbias_bf16``                             | 3.87e-03    | 1.55e-02    |
    | ``ds_y``: ds, output form                  | 8.58e-03    | 3.43e-02    |
    | ``dx_y``: dx, output form                  | 1.09e-02    | 4.36e-02    |
    | ``dgamma_y_f32``                           | 2.04e-02    | 8.16e-02    |
    | ``dgamma_y_bf16``                          | 3.23e-02    | 1.29e-01    |
    | ``dbias_y_f32``                            | 9.90e-04    | 3.96e-03    |
    | ``dbias_y_bf16``                           | 4.05e-03    | 1.62e-02    |
    | ``ba_y``: bias_act y (GELU)                | 3.86e-03    | 1.54e-02    |
    | ``ba_dz``: bias_act dz (GELU)              | 3.88e-03    | 1.55e-02    |
    | ``ba_dbias_f32``                           | 1.25e-06    | 5.00e-06    |
    | ``ba_dbias_bf16``                          | 3.89e-03    | 1.56e-02    |
    | ``emb_dW``: embedding3 dW (bf16)           | 3.89e-03    | 1.56e-02    |
    | ``emb_dP``: embedding3 dP (bf16)           | 3.88e-03    | 1.55e-02    |
    | ``emb_dT``: embedding3 dT (bf16)           | 3.47e-03    | 1.39e-02    |

``_y`` lines: the output-form (FROMY) backward, which divides by gamma (its xhat carries the
bf16 rounding of y over gamma); the common lines are not widened for it.  ``_f32`` / ``_bf16``: the
dtype of the accumulation buffer.  ``test_rounding_model_meets_bounds`` re-runs the model.

EXACT RESULTS (``torch.equal`` with the model: one or two fp32 operations, no fused multiply-add
possible): dropout kept values ``bf16(float(x) * float32(1 / (1 - p)))`` and zeros, forward and
backward; bias_act forward and dz for ReLU and NONE; embedding3 forward ``(W + P) + T``;
LayerNorm ``s`` when p = 0.  With p > 0 the compiler may contract ``t * scale + r``: ``s`` is then
within one bf16 step of ``s``, plus 2^-23 x the larger operand for the product's skipped fp32
rounding, of the model.  ``dx`` is exactly 0 wherever the mask drops, ``ds`` is not.

CASE MATRIX.
* LayerNorm forward: N in {8, 504, 512, 520, 1024, 1032, 1536, 1544, 2048} x M in {1, 5, 333} and
  (M 65541, N 8); configurations plain, bias, residual, bias + residual, bias + residual + p 0.1,
  p 0.1 alone, no beta, RMSNorm, RMSNorm + residual, keep_sum = False; ``C.layernorm_fwd`` per row
  and ``ops.layer_norm`` bit-equal to it.  N = 12, 2056: refused, wrapper = reference.
* LayerNorm backward: the same N x M in {5, 333}; (M in {1, 5, 513, 3073, 6145, 9217}, N 520) and
  (M in {2049, 4097, 6145}, N 1544): 1..4 rows per wave, P = 1, 2, 129, 768 partial rows.  Forms
  (``FORMS``): saved sum x dbias on / off x p 0 / 0.1; RMSNorm (dbias off; on with p 0.1); output
  form with dbias on / off (gamma in [0.3, 1.7], gamma[5] = 0); dextra on two saved-sum and two
  RMSNorm forms.  Parameter gradients accumulate into non-zero fp32 and bf16 slices of a larger
  buffer whose other elements must not change (``layernorm_bwd_into``); the dextra forms go through
  ``layernorm_bwd`` (bf16, no accumulation).  The M sweeps run every form too.
* bias_act: act {NONE, GELU, RELU} x bias {present, absent} x N {8, 512, 520, 4096} x
  M {1, 3, 4, 5, 64, 65, 193, 1025, 2049, 3073}; forward M 2064 x N 32768; want_dz = False; dbias
  fp32 and bf16 accumulated into non-zero values, and bf16 not accumulated (``bias_act_bwd``).
* dropout: n {8, 8000, 8 x (4096 x 256 + 3)} x p {0.1, 0.5}.
* embedding3: (T, B, S, H) {(2, 4, 64, 256), (3, 16, 32, 320), (1, 64, 16, 1024), (2, 1, 7, 8),
  (1, 5, 1, 264), (2, 3, 65536, 8)} x tables {all, no P, no T, T without tt} x ids down the batch
  {equal, alternating, random, random with id 0}.
* xent: (V, ld) {(16390, 16392), (1001, 1024), (64, 64)} x smoothing {0, 0.1}, labels on every
  thread / register boundary, V and -5 invalid, in place / out of place, scale given / None; R 8200.

KERNEL INSTANTIATIONS -> CASES.
* ``ln_fwd_kernel<MAXV, RMS>``: MAXV 1 N <= 512, 2 N 520..1024, 3 N 1032..1536, 4 N 1544..2048
  (``test_ln_forward`` at every N, RMS false and true); the row loop past 16384 blocks: M 65541.
* ``ln_bwd_kernel<MAXV, RMS, EXTRA, DBIAS, FROMY, PF2>``, MAXV as above (``test_ln_backward`` at
  every N):
  - ``<., false, false, true / false, false, true>`` (PF2, default): forms sum-db-p, sum-db /
    sum-nodb-p, sum-nodb; rows per wave 1..4: ``test_ln_backward_row_sweep``.
  - ``<., false, true, true / false, false, true>``: sum-db-p-extra / sum-nodb-extra.
  - ``<., false, false / true, true / false, false, false>`` (PF2 = false): the same forms in the
    child process with ``CLOUDTIK_AMD_LN_BWD_PF2=0`` (``test_variant_ln_backward``).
  - ``<., true, false, false / true>``: rms / rms-db-p; ``<., true, true, false / true>``:
    rms-extra / rms-db-p-extra.  The dispatcher never pairs RMS with PF2.
  - ``<., false, false, true / false, true, false>``: y-db-p / y-nodb.  FROMY never runs with PF2,
    and FROMY with EXTRA is reachable by no binding (``layernorm_bwd_into`` takes no dextra).
* ``colsum3_kernel<float / bf16>``: every backward case; P (the grid) 1, 2, 84 and 129, 513, 768
  (N 520) / 512 (N 1544): tail only, one 128-row step + tail, several steps.
* ``bias_act_fwd_kernel``: ``test_bias_act``, M 1..5 the 4-row tail; the row loop past the grid
  cap: ``test_bias_act_forward_past_grid_cap``.  ``bias_act_bwd_kernel``: M <= 1024 single loop,
  1025, 2049, 3073 the paired loop without / with a tail row; ``part == nullptr``:
  ``bias_act_bwd`` without a bias.  ``colsum_kernel<float / bf16>``: P 1, 2, 16, 17, 49, 256.
* ``dropout_kernel``: ``test_dropout``; the grid-stride loop at n = 8 x (4096 x 256 + 3).
* ``embed3_fwd_kernel``, ``embed3_bwd_seq_kernel`` (S <= 65535; nT <= 2 registers, nT 3 atomics),
  ``embed3_bwd_kernel`` (S 65536): ``test_embedding3``.
* ``xent_fwd_reg_kernel<4>`` ld 64 and 1024, ``<12>`` ld 16392 (``<8>``, ``<16>``:
  test_ops_gpu.py, ld 12000 / 30720); ``xent_fwd_kernel`` at these ld: the child process with
  ``CLOUDTIK_AMD_XENT_REG=0``; the row loop past 8192 blocks: ``test_variant_xent_many_rows``.
* ``test_variant_kernels_selected`` reads the kernel names from the profiler in this process and
  in each child and compares them with the dispatchers' rules.
"""
import collections
import functools
import math
import os
import subprocess
import sys
import zlib

import pytest
import torch

from cloudtik_amd import ops
from cloudtik_amd.ops import reference as ref

F32, F64 = torch.float32, torch.float64
BF16 = torch.bfloat16
SEED = 7
PAD = 8         # guard elements around every parameter-gradient slice

# worst error of the F32 model against the F64 reference over the whole matrix (module docstring)
MODEL_WORST = {
    "y": 3.89e-03,
    "mean": 2.98e-08,
    "rstd": 2.25e-07,
    "ds": 3.88e-03,
    "dx": 3.89e-03,
    "dgamma_f32": 1.76e-07,
    "dgamma_bf16": 3.81e-03,
    "dbeta_f32": 5.87e-08,
    "dbeta_bf16": 3.88e-03,
    "dbias_f32": 1.55e-07,
    "dbias_bf16": 3.87e-03,
    "ds_y": 8.58e-03,
    "dx_y": 1.09e-02,
    "dgamma_y_f32": 2.04e-02,
    "dgamma_y_bf16": 3.23e-02,
    "dbias_y_f32": 9.90e-04,
    "dbias_y_bf16": 4.05e-03,
    "ba_y": 3.86e-03,
    "ba_dz": 3.88e-03,
    "ba_dbias_f32": 1.25e-06,
    "ba_dbias_bf16": 3.89e-03,
    "emb_dW": 3.89e-03,
    "emb_dP": 3.88e-03,
    "emb_dT": 3.47e-03,
}
BOUND = {k: 4.0 * v for k, v in MODEL_WORST.items()}


# ------------------------------------------------------------------ metric
def _rows(x, want):
    x, want = x.double(), want.double()
    d = (x - want).abs().amax(-1)
    top = want.abs().max()
    if top == 0:
        return d
    return d / (want.abs().amax(-1) + 1e-3 * top)


def _cols(x, want, mass):
    d = (x.double() - want.double()).abs()
    top = mass.max()
    if top == 0:
        return d
    return d / (mass.double() + 1e-3 * top)


def _stat(x, want):
    want = want.double()
    return (x.double() - want).abs() / want.abs().clamp_min(1.0)


def _worst(e):
    """max that keeps a NaN (a NaN anywhere fails every bound)."""
    return float("nan") if torch.isnan(e).any() else e.max().item()


def _assert_bounds(errs, tag):
    print("rowops-err %s %s" % (tag, " ".join("%s=%.3e" % kv for kv in sorted(errs.items()))))
    for n, e in errs.items():
        assert e <= BOUND[n], "%s: %s worst error %.3e > bound %.3e" % (tag, n, e, BOUND[n])


def _one_ulp(a, b, mag):
    """|a - b| <= one bf16 step of the larger of the two results + 2^-23 x ``mag``, the largest
    operand of the sum that was rounded: a contracted multiply-add skips the fp32 rounding of the
    product (half an fp32 step of ``mag``), which is what moves the result where the sum cancels."""
    a, b = a.double(), b.double()
    exp = torch.frexp(torch.maximum(a.abs(), b.abs()))[1]          # |v| in [2^(e-1), 2^e): step 2^(e-8)
    step = torch.ldexp(torch.ones_like(a), exp - 8)
    return bool(((a - b).abs() <= step + 2.0 ** -23 * mag.double()).all())


def _rnd(t, dt):
    """bf16 rounding where the kernels round (model); the reference keeps fp64."""
    return t.bfloat16().to(dt) if dt == F32 else t


def _scale(p, dev):
    """The kernels' keep scale: float32(1) / (float32(1) - float32(p))."""
    one = torch.ones((), dtype=F32, device=dev)
    return one / (one - torch.tensor(p, dtype=F32, device=dev))


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


@functools.lru_cache(maxsize=4)
def _keep(n, p):
    """Keep mask of the stream (SEED, offset 0): what ops.manual_seed(SEED) hands the first site."""
    return ref.dropout_keep_mask(n, p, SEED, 0)


# ------------------------------------------------------------------ LayerNorm: reference and model
LnCfg = collections.namedtuple("LnCfg", "name bias res p rms beta keep_sum", defaults=(True, True))
FWD_CFGS = [LnCfg("plain", False, False, 0.0, False), LnCfg("bias", True, False, 0.0, False),
            LnCfg("res", False, True, 0.0, False), LnCfg("bias-res", True, True, 0.0, False),
            LnCfg("bias-res-p", True, True, 0.1, False), LnCfg("p", False, False, 0.1, False),
            LnCfg("nobeta", False, False, 0.0, False, False), LnCfg("rms", False, False, 0.0, True),
            LnCfg("rms-res", False, True, 0.0, True),
            LnCfg("bias-res-p-nosum", True, True, 0.1, False, True, False)]
LN_N = [8, 504, 512, 520, 1024, 1032, 1536, 1544, 2048]
EPS = {False: 1e-12, True: 1e-6}     # LayerNorm (BERT), RMSNorm (T5)

Form = collections.namedtuple("Form", "name kind dbias p extra", defaults=(False,))
FORMS = [Form("sum-db-p", "sum", True, 0.1), Form("sum-db", "sum", True, 0.0),
         Form("sum-nodb-p", "sum", False, 0.1), Form("sum-nodb", "sum", False, 0.0),
         Form("rms", "rms", False, 0.0), Form("rms-db-p", "rms", True, 0.1),
         Form("y-db-p", "y", True, 0.1), Form("y-nodb", "y", False, 0.0),
         Form("sum-db-p-extra", "sum", True, 0.1, True), Form("sum-nodb-extra", "sum", False, 0.0, True),
         Form("rms-extra", "rms", False, 0.0, True), Form("rms-db-p-extra", "rms", True, 0.1, True)]
SWEEPS = [(M, 520) for M in (1, 5, 513, 3073, 6145, 9217)] + [(M, 1544) for M in (2049, 4097, 6145)]


@functools.lru_cache(maxsize=2)
def _ln_inputs(M, N, spread):
    """bf16 inputs on the CPU; ``spread``: gamma over [0.3, 1.7] with gamma[5] = 0 and beta over
    [-1, 1] (the output-form cases), else gamma near 1 and beta near 0."""
    g = _gen("ln", M, N, spread)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    inp = {"x": r(M, N), "res": r(M, N), "bias": 0.1 * r(N), "dy": r(M, N), "dextra": 0.5 * r(M, N)}
    if spread:
        inp["gamma"] = 0.3 + 1.4 * torch.rand(N, generator=g)
        inp["gamma"][5] = 0
        inp["beta"] = 2 * torch.rand(N, generator=g) - 1
    else:
        inp["gamma"] = 1 + 0.1 * r(N)
        inp["beta"] = 0.1 * r(N)
    return {k: v.bfloat16() for k, v in inp.items()}


def _ln_fwd(inp, c, keep, dt, s16=None):
    """s = bf16(res + dropout(x + bias)) in the kernels' fp32 order (that IS the definition of s:
    exact at p = 0), or the ``s16`` given; then its statistics and y.  dt F64: reference; F32: model."""
    t = inp["x"].float()
    if c.bias:
        t = t + inp["bias"].float()
    if c.p > 0:
        t = torch.where(keep, t * _scale(c.p, t.device), torch.zeros_like(t))
    mag = t.abs()
    if c.res:
        t = t + inp["res"].float()
        mag = torch.maximum(mag, inp["res"].float().abs())
    if s16 is None:
        s16 = t.bfloat16()
    s = s16.to(dt)
    N = s.shape[1]
    mean = torch.zeros_like(s[:, 0]) if c.rms else s.sum(1) / N
    var = ((s - mean[:, None]) ** 2).sum(1) / N
    rstd = torch.rsqrt(var + torch.tensor(EPS[c.rms], dtype=F32).to(dt))
    y = (s - mean[:, None]) * rstd[:, None] * inp["gamma"].to(dt)
    if c.beta and not c.rms:
        y = y + inp["beta"].to(dt)
    return {"y": _rnd(y, dt), "s": s16, "mean": mean, "rstd": rstd, "mag": mag}


def _ln_bwd(inp, f, keep, fwd, dt, from_y=False):
    """Backward of LN / RMSNorm at the reference forward's s (bf16), mean and rstd (fp32).
    ``from_y`` (model only): the kernels' output form, xhat = (bf16(y) - beta) / gamma.  The
    reference of those cases is the gradient at s with xhat = 0 where gamma == 0.  Returns row
    tensors, column sums and the columns' sums of |terms|."""
    dy, g = inp["dy"].to(dt), inp["gamma"].to(dt)
    mean, rstd = fwd["mean"].float().to(dt)[:, None], fwd["rstd"].float().to(dt)[:, None]
    N = dy.shape[1]
    live = (g != 0).to(dt)
    if from_y:
        u = fwd["y"].bfloat16().to(dt) - inp["beta"].to(dt)
        rg = torch.where(g != 0, 1.0 / g, torch.zeros_like(g))
        xhat = u * rg
        s2 = (dy * u).sum(1, keepdim=True) / N
        gterms = dy * u * rg
    else:
        xhat = (fwd["s"].to(dt) - mean) * rstd
        if f.kind == "y":
            xhat = xhat * live
        s2 = (dy * g * xhat).sum(1, keepdim=True) / N
        gterms = dy * xhat
    dgv = dy * g
    s1 = 0.0 if f.kind == "rms" else dgv.sum(1, keepdim=True) / N
    t = rstd * (dgv - s1 - xhat * s2)
    if f.extra:
        t = t + inp["dextra"].to(dt)
    tx = torch.where(keep, t * _scale(f.p, t.device).to(dt), torch.zeros_like(t)) if f.p > 0 else t
    out = {"ds": _rnd(t, dt), "dx": _rnd(tx, dt),
           "cols": {"dgamma": gterms.sum(0)}, "mass": {"dgamma": gterms.abs().sum(0)}}
    if f.kind != "rms":
        out["cols"]["dbeta"], out["mass"]["dbeta"] = dy.sum(0), dy.abs().sum(0)
    if f.dbias:
        out["cols"]["dbias"], out["mass"]["dbias"] = tx.sum(0), tx.abs().sum(0)
    return out


def _fwd_cfg_of(f):
    return LnCfg(f.name, f.dbias, True, f.p, f.kind == "rms")


def _accumulate(col, init, dtype, dt):
    """What a column-sum kernel leaves in a buffer of ``dtype`` that held ``init``."""
    v = col + init.to(dt)
    return v.to(dtype).to(dt) if dt == F32 else v


def _ln_fwd_errors(got, want):
    return {"y": _worst(_rows(got["y"], want["y"])), "mean": _worst(_stat(got["mean"], want["mean"])),
            "rstd": _worst(_stat(got["rstd"], want["rstd"]))}


def _ln_bwd_errors(got, want, f, init, dtype):
    """got["cols"]: finished buffers (dtype); want: reference sums before the buffer's value."""
    sfx = "_y" if f.kind == "y" else ""
    out = {"ds" + sfx: _worst(_rows(got["ds"], want["ds"])), "dx" + sfx: _worst(_rows(got["dx"], want["dx"]))}
    for n, col in want["cols"].items():
        i0 = init[n].double() if init is not None else torch.zeros_like(col)
        key = n + (sfx if n != "dbeta" else "") + ("_f32" if dtype == F32 else "_bf16")
        out[key] = _worst(_cols(got["cols"][n], col + i0, want["mass"][n] + i0.abs()))
    return out


def _param_init(N, dtype, names):
    """A buffer with one N-element slice per name, PAD guard elements around each, all non-zero."""
    g = _gen("param", N, str(dtype))
    big = torch.randn(len(names) * (N + PAD) + PAD, generator=g).to(dtype)
    big[big == 0] = 1
    at = {n: PAD + i * (N + PAD) for i, n in enumerate(names)}
    return big, at


# ------------------------------------------------------------------ bias_act: reference and model
def _ba(z, bias, act, dy, dt):
    t = z.to(dt)
    if bias is not None:
        t = t + bias.to(dt)
    if act == ops.ACT_GELU:
        cdf = 0.5 * (1 + torch.erf(t * math.sqrt(0.5)))
        y, g = t * cdf, cdf + t * torch.exp(-0.5 * t * t) * 0.3989422804014327
    elif act == ops.ACT_RELU:
        y, g = t.clamp_min(0), (t > 0).to(dt)
    else:
        y, g = t, torch.ones_like(t)
    out = {"y": _rnd(y, dt)}
    if dy is not None:
        d = dy.to(dt) * g
        out.update(dz=_rnd(d, dt), col=d.sum(0), mass=d.abs().sum(0))
    return out


BA_M = [1, 3, 4, 5, 64, 65, 193, 1025, 2049, 3073]
BA_N = [8, 512, 520, 4096]
ACTS = {"none": ops.ACT_NONE, "gelu": ops.ACT_GELU, "relu": ops.ACT_RELU}


@functools.lru_cache(maxsize=2)
def _ba_inputs(M, N):
    g = _gen("ba", M, N)
    return {"z": torch.randn(M, N, generator=g).bfloat16(), "dy": torch.randn(M, N, generator=g).bfloat16(),
            "bias": (0.1 * torch.randn(N, generator=g)).bfloat16()}


def _ba_errors(got, want, act, init=None, dtype=None):
    """GELU: bounds.  ReLU and NONE are exact: asserted apart, nothing to bound."""
    out = {}
    if act == ops.ACT_GELU:
        out["ba_y"] = _worst(_rows(got["y"], want["y"]))
        if "dz" in got:
            out["ba_dz"] = _worst(_rows(got["dz"], want["dz"]))
    if "col" in got:
        i0 = init.double() if init is not None else torch.zeros_like(want["col"])
        key = "ba_dbias" + ("_f32" if dtype == F32 else "_bf16")
        out[key] = _worst(_cols(got["col"], want["col"] + i0, want["mass"] + i0.abs()))
    return out


# ------------------------------------------------------------------ embedding3: reference and model
EMB_SHAPES = [(2, 4, 64, 256), (3, 16, 32, 320), (1, 64, 16, 1024), (2, 1, 7, 8), (1, 5, 1, 264), (2, 3, 65536, 8)]
EMB_TABLES = ["all", "noP", "noT", "T-without-tt"]
EMB_IDS = ["equal", "alternating", "random", "random0"]
EMB_V = 1000


@functools.lru_cache(maxsize=2)
def _emb_inputs(T, B, S, H, ids_kind):
    g = _gen("emb", T, B, S, H, ids_kind)
    r = lambda *s: torch.randn(*s, generator=g).bfloat16()  # noqa: E731
    a, b = torch.randint(1, EMB_V, (S,), generator=g), torch.randint(1, EMB_V, (S,), generator=g)
    if ids_kind == "equal":
        ids = a[None].expand(B, S).clone()
    elif ids_kind == "alternating":         # the run-merging register resets at every token
        b = torch.where(b == a, (a % (EMB_V - 1)) + 1, b)
        ids = torch.where((torch.arange(B) % 2 == 0)[:, None], a[None], b[None]).clone()
    else:
        ids = torch.randint(1 if ids_kind == "random" else 0, EMB_V, (B, S), generator=g)
        if ids_kind == "random0":
            ids[torch.rand(B, S, generator=g) < 0.01] = 0      # few: same-address atomics serialise
            ids[0, 0] = ids[B // 2, S // 2] = 0
    return {"ids": ids, "tt": torch.randint(0, T, (B, S), generator=g), "W": r(EMB_V, H), "P": r(S + 3, H),
            "T": r(T, H), "dy": r(B, S, H)}


def _emb(inp, tables, dt):
    """Forward (W + P) + T and the three table gradients."""
    ids, S = inp["ids"], inp["ids"].shape[1]
    H = inp["W"].shape[1]
    o = inp["W"].to(dt)[ids]
    if tables != "noP":
        o = o + inp["P"].to(dt)[:S][None]
    if tables != "noT":
        tt = inp["tt"] if tables != "T-without-tt" else torch.zeros_like(ids)
        o = o + inp["T"].to(dt)[tt]
    dy = inp["dy"].to(dt).reshape(-1, H)
    out = {"y": _rnd(o, dt), "dW": _rnd(torch.zeros_like(inp["W"], dtype=dt).index_add_(0, ids.reshape(-1), dy), dt)}
    if tables != "noP":
        dP = torch.zeros_like(inp["P"], dtype=dt)
        dP[:S] = inp["dy"].to(dt).sum(0)
        out["dP"] = _rnd(dP, dt)
    if tables != "noT":
        out["dT"] = _rnd(torch.zeros_like(inp["T"], dtype=dt).index_add_(0, tt.reshape(-1), dy), dt)
    return out


def _emb_errors(got, want):
    return {"emb_" + n: _worst(_rows(got[n], want[n])) for n in want if n != "y"}


# ------------------------------------------------------------------ the model over the matrix (CPU)
def _model_matrix():
    """Worst error of the model per quantity over the whole case matrix."""
    worst = collections.defaultdict(float)

    def note(errs):
        for n, e in errs.items():
            assert e == e, n
            worst[n] = max(worst[n], e)

    for N in LN_N:
        for M in (1, 5, 333):
            _model_ln_fwd(M, N, note)
        for M in (5, 333):
            for f in FORMS:
                _model_ln_bwd(M, N, f, note)
    _model_ln_fwd(65541, 8, note)
    for M, N in SWEEPS:
        for f in FORMS:
            _model_ln_bwd(M, N, f, note)
    for N in BA_N:
        for M in BA_M:
            inp = _ba_inputs(M, N)
            for act in ACTS.values():
                for bias in (inp["bias"], None):
                    want = _ba(inp["z"], bias, act, inp["dy"], F64)
                    got = _ba(inp["z"], bias, act, inp["dy"], F32)
                    for dtype in (F32, BF16):
                        init = torch.randn(N, generator=_gen("bainit", N)).to(dtype)
                        fin = dict(got, col=_accumulate(got["col"], init, dtype, F32))
                        note(_ba_errors(fin, want, act, init, dtype))
                    note(_ba_errors(dict(got, col=got["col"].bfloat16()), want, act, None, BF16))
    inp = _ba_inputs(2064, 32768)
    note(_ba_errors(_ba(inp["z"], inp["bias"], ops.ACT_GELU, None, F32), _ba(inp["z"], inp["bias"], ops.ACT_GELU, None, F64),
                    ops.ACT_GELU))
    for shape in EMB_SHAPES:
        for kind in EMB_IDS:
            inp = _emb_inputs(*shape, kind)
            for tables in EMB_TABLES:
                note(_emb_errors(_emb(inp, tables, F32), _emb(inp, tables, F64)))
    return dict(worst)


def _model_ln_fwd(M, N, note):
    inp = _ln_inputs(M, N, False)
    for c in FWD_CFGS:
        keep = _keep(M * N, c.p).view(M, N) if c.p > 0 else None
        want, got = _ln_fwd(inp, c, keep, F64), _ln_fwd(inp, c, keep, F32)
        note(_ln_fwd_errors(got, want))


def _model_ln_bwd(M, N, f, note):
    inp = _ln_inputs(M, N, f.kind == "y")
    keep = _keep(M * N, f.p).view(M, N) if f.p > 0 else None
    fwd = _ln_fwd(inp, _fwd_cfg_of(f), keep, F64)
    want, got = _ln_bwd(inp, f, keep, fwd, F64), _ln_bwd(inp, f, keep, fwd, F32, from_y=f.kind == "y")
    for dtype in (BF16,) if f.extra else (F32, BF16):
        big, at = _param_init(N, dtype, sorted(want["cols"]))
        init = None if f.extra else {n: big[at[n]:at[n] + N] for n in at}
        cols = {n: _accumulate(c, init[n] if init else torch.zeros(N), dtype, F32) for n, c in got["cols"].items()}
        note(_ln_bwd_errors(dict(got, cols=cols), want, f, init, dtype))


def test_rounding_model_meets_bounds():
    """The model that the bounds come from meets them (by the factor of 4) on every case of the
    matrix, and the recorded figures are the model's; prints its worst error per quantity."""
    worst = _model_matrix()
    print("model worst:\n" + "\n".join('    "%s": %.2e,' % kv for kv in sorted(worst.items())))
    assert set(worst) == set(MODEL_WORST)
    for n in BOUND:      # give or take another CPU's summation order
        assert MODEL_WORST[n] * 0.75 <= worst[n] <= MODEL_WORST[n] * 1.25, (n, worst[n], MODEL_WORST[n])


def test_checker_catches_one_wrong_row_and_one_short_column():
    """One row of 333 scaled by 1.05 and one dgamma column that misses 32 of its 333 terms stay
    inside the whole-tensor 2e-2 of the older tests and fail here."""
    M, N = 333, 1024
    f = FORMS[0]
    inp = _ln_inputs(M, N, False)
    keep = _keep(M * N, f.p).view(M, N)
    c = _fwd_cfg_of(f)
    want = _ln_fwd(inp, c, keep, F64)
    got = {k: v.clone() for k, v in want.items()}
    got["y"][200] *= 1.05
    assert ((got["y"] - want["y"]).norm() / want["y"].norm()).item() < 2e-2
    with pytest.raises(AssertionError):
        _assert_bounds(_ln_fwd_errors(got, want), "wrong row")
    bw = _ln_bwd(inp, f, keep, want, F64)
    cols = {n: v.clone() for n, v in bw["cols"].items()}
    xhat = (want["s"].double() - want["mean"][:, None]) * want["rstd"][:, None]
    cols["dgamma"][77] -= (inp["dy"].double() * xhat)[:32, 77].sum()
    assert ((cols["dgamma"] - bw["cols"]["dgamma"]).norm() / bw["cols"]["dgamma"].norm()).item() < 2e-2
    with pytest.raises(AssertionError):
        _assert_bounds(_ln_bwd_errors(dict(bw, cols=cols), bw, f, None, F32), "short column")


# ------------------------------------------------------------------ GPU: LayerNorm forward
def _dev(inp, dev):
    return {k: v.to(dev) for k, v in inp.items()}


def _run_ln_fwd(d, c):
    C = ops.require_native()
    y, s, mean, rstd = C.layernorm_fwd(d["x"], d["bias"] if c.bias else None, d["res"] if c.res else None, d["gamma"],
                                       d["beta"] if (c.beta and not c.rms) else None, EPS[c.rms], c.rms, c.p, SEED, 0,
                                       keep_sum=c.keep_sum)
    return {"y": y, "s": s, "mean": mean, "rstd": rstd}


def _check_ln_fwd(dev, M, N):
    inp = _ln_inputs(M, N, False)
    d = _dev(inp, dev)
    kept = {}
    for c in FWD_CFGS:
        keep = _keep(M * N, c.p).view(M, N).to(dev) if c.p > 0 else None
        model = _ln_fwd(d, c, keep, F32)
        got = _run_ln_fwd(d, c)
        tag = "ln-fwd %dx%d %s" % (M, N, c.name)
        if not c.keep_sum:           # the same call with keep_sum: same y and statistics, and its s
            sib = kept[c.name[:-6]]
            assert got["s"] is None and all(torch.equal(got[n], sib[n]) for n in ("y", "mean", "rstd")), tag
            s16 = sib["s"]
        elif c.bias or c.res or c.p > 0:
            s16 = got["s"]
            if c.p == 0:
                assert torch.equal(s16, model["s"]), tag
            else:
                assert _one_ulp(s16, model["s"], model["mag"]), tag
                base = d["res"] if c.res else torch.zeros_like(s16)
                assert torch.equal(s16[~keep], base[~keep]), tag + ": s at a dropped element is not the residual"
        else:
            assert got["s"] is None, tag
            s16 = d["x"]
        kept[c.name] = got
        # the kernel normalises its rounded s (checked above): the reference normalises the same s
        _assert_bounds(_ln_fwd_errors(got, _ln_fwd(d, c, keep, F64, s16)), tag)
        ops.manual_seed(SEED)
        front = ops.layer_norm(d["x"], d["gamma"], d["beta"] if (c.beta and not c.rms) else None, EPS[c.rms],
                               bias=d["bias"] if c.bias else None, residual=d["res"] if c.res else None, p=c.p,
                               training=True, rms=c.rms)
        assert torch.equal(front, got["y"]), tag


@pytest.mark.gpu
@pytest.mark.parametrize("M", [1, 5, 333])
@pytest.mark.parametrize("N", LN_N)
def test_ln_forward(cuda, N, M):
    _check_ln_fwd(cuda, M, N)


@pytest.mark.gpu
def test_ln_forward_more_rows_than_the_grid(cuda):
    """65541 rows: more than 16384 blocks x 4 waves, every wave walks the row loop."""
    _check_ln_fwd(cuda, 65541, 8)


@pytest.mark.gpu
@pytest.mark.parametrize("N", [12, 2056])
def test_ln_refused_widths_route_to_reference(cuda, N):
    C = ops.require_native()
    g = _gen("refuse", N)
    x = torch.randn(5, N, generator=g).bfloat16().to(cuda)
    gamma, beta = (torch.randn(N, generator=g).bfloat16().to(cuda) for _ in range(2))
    with pytest.raises(RuntimeError, match="unsupported shape"):
        C.layernorm_fwd(x, None, None, gamma, beta, 1e-12, False, 0.0, 0, 0)
    assert torch.equal(ops.layer_norm(x, gamma, beta, 1e-12), ref.layer_norm(x, gamma, beta, 1e-12)[0])


# ------------------------------------------------------------------ GPU: LayerNorm backward
def _check_ln_bwd(dev, M, N, f):
    C = ops.require_native()
    inp = _ln_inputs(M, N, f.kind == "y")
    d = _dev(inp, dev)
    keep = _keep(M * N, f.p).view(M, N).to(dev) if f.p > 0 else None
    fwd = _ln_fwd(d, _fwd_cfg_of(f), keep, F64)
    want = _ln_bwd(d, f, keep, fwd, F64)
    rms = f.kind == "rms"
    src = fwd["y"].bfloat16() if f.kind == "y" else fwd["s"]
    mean, rstd = fwd["mean"].float(), fwd["rstd"].float()
    tag = "ln-bwd %dx%d %s" % (M, N, f.name)
    names = sorted(want["cols"])
    runs = []
    if f.extra:
        ds, dx, dg, db, dbi = C.layernorm_bwd(d["dy"], src, d["gamma"], mean, rstd, d["dextra"], rms, not rms, f.dbias,
                                              True, f.p, SEED, 0)
        assert (db is None) == rms and (dbi is None) == (not f.dbias), tag
        runs.append((BF16, None, ds, dx, {"dgamma": dg, "dbeta": db, "dbias": dbi}))
    else:
        for dtype in (F32, BF16):
            big, at = _param_init(N, dtype, names)
            dbig = big.to(dev)
            view = {n: dbig[at[n]:at[n] + N] for n in names}
            ds, dx = C.layernorm_bwd_into(d["dy"], src, d["gamma"], mean, rstd, rms, view["dgamma"], view.get("dbeta"),
                                          view.get("dbias"), True, f.p, SEED, 0, beta_y=d["beta"] if f.kind == "y" else None)
            guard = torch.ones(big.numel(), dtype=torch.bool)
            for n in names:
                guard[at[n]:at[n] + N] = False
            assert torch.equal(dbig.cpu()[guard], big[guard]), tag + ": written outside the gradient slices"
            runs.append((dtype, {n: big[at[n]:at[n] + N].to(dev) for n in names}, ds, dx, view))
    for dtype, init, ds, dx, cols in runs:
        got = {"ds": ds, "dx": dx, "cols": {n: cols[n] for n in names}}
        _assert_bounds(_ln_bwd_errors(got, want, f, init, dtype), tag + (" f32" if dtype == F32 else " bf16"))
        if f.p > 0:
            assert not dx[~keep].any(), tag + ": dx is not 0 at a dropped element"
            masked = (ds == 0) & ~keep & (want["ds"].abs() > 1e-3 * want["ds"].abs().amax(1, keepdim=True))
            assert not masked.any(), tag + ": ds is 0 at a dropped element"
        else:
            assert torch.equal(dx, ds), tag
        if f.kind == "y":
            assert cols["dgamma"][5].item() == (init["dgamma"][5].item() if init else 0.0), tag


def _form_id(f):
    return f.name


@pytest.mark.gpu
@pytest.mark.parametrize("f", FORMS, ids=_form_id)
@pytest.mark.parametrize("M", [5, 333])
@pytest.mark.parametrize("N", LN_N)
def test_ln_backward(cuda, N, M, f):
    _check_ln_bwd(cuda, M, N, f)


@pytest.mark.gpu
@pytest.mark.parametrize("f", FORMS, ids=_form_id)
@pytest.mark.parametrize("M,N", SWEEPS)
def test_ln_backward_row_sweep(cuda, M, N, f):
    """1, 2, 3 and 4 rows per wave on the 768-block grid (N 520) and the 512-block grid (N 1544):
    the prefetch loop ends on either register set; P = 1, 2, 129, 768 / 512 partial rows."""
    _check_ln_bwd(cuda, M, N, f)


VARIANT_BWD = [(333, 1536), (5, 8), (3073, 520), (9217, 520), (4097, 1544)]


@pytest.mark.gpu
@pytest.mark.parametrize("f", [f for f in FORMS if f.kind == "sum"] + [FORMS[4], FORMS[6]], ids=_form_id)
@pytest.mark.parametrize("M,N", VARIANT_BWD)
def test_variant_ln_backward(cuda, M, N, f):
    """One shape per line of the backward matrix, every saved-sum form (the ones the prefetch
    variable switches) and one RMSNorm and one output form: re-run in the child processes."""
    _check_ln_bwd(cuda, M, N, f)


# ------------------------------------------------------------------ GPU: bias_act
def _check_ba(dev, M, N, act, has_bias):
    C = ops.require_native()
    inp = _dev(_ba_inputs(M, N), dev)
    z, dy, bias = inp["z"], inp["dy"], inp["bias"] if has_bias else None
    want, model = _ba(z, bias, act, dy, F64), _ba(z, bias, act, dy, F32)
    tag = "bias_act %dx%d act%d %s" % (M, N, act, "bias" if has_bias else "nobias")
    exact = act != ops.ACT_GELU
    y = C.bias_act_fwd(z, bias, act)
    dz, dbias = C.bias_act_bwd(dy, z, bias, act, has_bias)
    assert (dbias is None) == (not has_bias), tag
    got = {"y": y, "dz": dz}
    if has_bias:
        got["col"] = dbias
    _assert_bounds(_ba_errors(got, want, act, None, BF16), tag)
    if exact:
        assert torch.equal(y.float(), model["y"]) and torch.equal(dz.float(), model["dz"]), tag
    for dtype in (F32, BF16):
        init = torch.randn(N, generator=_gen("bainit", N)).to(dtype)
        big = torch.cat([init[:PAD], init, init[:PAD]]).to(dev)
        buf = big[PAD:PAD + N]
        dz2 = C.bias_act_bwd_into(dy, z, bias, act, buf, True)
        assert torch.equal(dz2, dz), tag
        assert torch.equal(big[:PAD].cpu(), init[:PAD]) and torch.equal(big[-PAD:].cpu(), init[:PAD]), tag
        _assert_bounds(_ba_errors({"y": y, "col": buf}, want, act, init.to(dev), dtype), tag + " into " + str(dtype))
        if dtype == F32:
            buf2 = init.to(dev)
            assert C.bias_act_bwd_into(dy, z, bias, act, buf2, False) is None, tag
            assert torch.equal(buf2, buf), tag + ": want_dz=False changes the bias gradient"


@pytest.mark.gpu
@pytest.mark.parametrize("has_bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("act", sorted(ACTS))
@pytest.mark.parametrize("N", BA_N)
def test_bias_act(cuda, N, act, has_bias):
    for M in BA_M:
        _check_ba(cuda, M, N, ACTS[act], has_bias)


@pytest.mark.gpu
def test_bias_act_forward_past_grid_cap(cuda):
    """M 2064, N 32768: 129 row blocks wanted, 128 launched -- the forward's row loop runs twice."""
    C = ops.require_native()
    inp = _dev(_ba_inputs(2064, 32768), cuda)
    want = _ba(inp["z"], inp["bias"], ops.ACT_GELU, None, F64)
    got = {"y": C.bias_act_fwd(inp["z"], inp["bias"], ops.ACT_GELU)}
    _assert_bounds(_ba_errors(got, want, ops.ACT_GELU), "bias_act cap gelu")
    model = _ba(inp["z"], inp["bias"], ops.ACT_RELU, None, F32)
    assert torch.equal(C.bias_act_fwd(inp["z"], inp["bias"], ops.ACT_RELU).float(), model["y"])


# ------------------------------------------------------------------ GPU: dropout
@pytest.mark.gpu
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("n", [8, 8 * 1000, 8 * (4096 * 256 + 3)])
def test_dropout(cuda, n, p):
    """Forward and backward bit-equal to bf16(float(x) * float32(1 / (1 - p))) under the reference
    mask; the last n is past the 4096 x 256 grid, so the grid-stride loop runs."""
    g = _gen("drop", n)
    x = torch.randn(n, generator=g).bfloat16().to(cuda).requires_grad_()
    dy = torch.randn(n, generator=g).bfloat16().to(cuda)
    keep = _keep(n, p).to(cuda)
    ops.manual_seed(SEED)
    y = ops.dropout(x, p, True)
    y.backward(dy)
    for got, src in ((y.detach(), x.detach()), (x.grad, dy)):
        model = torch.where(keep, (src.float() * _scale(p, cuda)).bfloat16(), torch.zeros_like(src))
        assert torch.equal(got, model)
    q = (ref.dropout_threshold(p) >> 16) / 65536.0
    live = x.detach() != 0                     # a zero of y there is a dropped element
    m, dropped = live.sum().item(), (y.detach()[live] == 0).sum().item()
    assert abs(dropped - m * q) <= 4 * math.sqrt(m * q * (1 - q))


# ------------------------------------------------------------------ GPU: embedding3
@pytest.mark.gpu
@pytest.mark.parametrize("ids_kind", EMB_IDS)
@pytest.mark.parametrize("shape", EMB_SHAPES, ids=lambda s: "T%d-B%d-S%d-H%d" % s)
def test_embedding3(cuda, shape, ids_kind):
    """Forward bit-equal to bf16((W + P) + T); dW, dP, dT per row.  S = 65536 takes the per-token
    atomic backward, every other shape the per-position one."""
    inp = _dev(_emb_inputs(*shape, ids_kind), cuda)
    for tables in EMB_TABLES:
        want, model = _emb(inp, tables, F64), _emb(inp, tables, F32)
        W, P, T = (inp[n].clone().requires_grad_() for n in ("W", "P", "T"))
        y = ops.embedding3(inp["ids"], None if tables == "T-without-tt" else inp["tt"], W,
                           None if tables == "noP" else P, None if tables == "noT" else T)
        y.backward(inp["dy"])
        tag = "embedding3 %s %s %s" % (shape, ids_kind, tables)
        assert torch.equal(y.detach().float(), model["y"]), tag
        got = {"dW": W.grad, "dP": P.grad, "dT": T.grad}
        assert (P.grad is None) == (tables == "noP") and (T.grad is None) == (tables == "noT"), tag
        _assert_bounds(_emb_errors({n: got[n] for n in want if n != "y"}, want), tag)


# ------------------------------------------------------------------ GPU: xent
XENT_SHAPES = [(16390, 16392), (1001, 1024), (64, 64)]


def _xent_labels(V, ld):
    nv = -(-(ld // 8) // 256)
    nv = 4 if nv <= 4 else 8 if nv <= 8 else 12 if nv <= 12 else 16
    cols = {0, 7, 8, 2047, 2048, V - 1} | {2048 * k - 1 for k in range(1, nv)} | {2048 * k for k in range(1, nv)}
    valid = sorted(c for c in cols if 0 <= c < V)
    return torch.tensor(valid + [V, -5, -100, V // 2, 1], dtype=torch.int64)


def _check_xent(dev, V, ld, smooth, labels, in_place, with_scale, tag):
    """The assertions of test_xent_kernel_matches_fp32, against fp64, on every row."""
    C = ops.require_native()
    R = labels.numel()
    logits = (3 * torch.randn(R, ld, generator=_gen("xent", V, ld, R))).bfloat16().to(dev)
    labels = labels.to(dev)
    r64 = logits.double()[:, :V]
    lse_ref = torch.logsumexp(r64, 1)
    valid = (labels >= 0) & (labels < V) & (labels != -100)
    scale = torch.tensor([1.0 / valid.sum().item()], device=dev) if with_scale else None
    src = logits.clone()
    out = src if in_place else torch.full_like(logits, float("nan"))
    loss, lse = C.xent_fwd(src, out, V, labels, scale, -100, smooth)
    if not in_place:
        assert torch.equal(src, logits), tag + ": logits changed by an out-of-place call"
    logp = r64 - lse_ref[:, None]
    safe = torch.where(valid, labels, torch.zeros_like(labels))
    nll = -logp.gather(1, safe[:, None])[:, 0]
    want_loss = torch.where(valid, (1 - smooth) * nll - smooth * logp.mean(1), torch.zeros_like(nll))
    torch.testing.assert_close(lse.double(), lse_ref, rtol=1e-4, atol=1e-3, msg=tag)
    torch.testing.assert_close(loss.double(), want_loss, rtol=1e-3, atol=2e-3, msg=tag)
    assert (loss[~valid] == 0).all(), tag
    onehot = torch.nn.functional.one_hot(safe, V).double()
    g = (logp.exp() - smooth / V - (1 - smooth) * onehot) * (scale.double() if with_scale else 1.0) * valid[:, None].double()
    torch.testing.assert_close(out.double()[:, :V], g, rtol=2e-2, atol=2e-4, msg=tag)
    assert not out[~valid].any(), tag + ": gradient row of an invalid label is not zero"
    assert not out[:, V:].any(), tag + ": padded columns are not zero"


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["inplace-scale", "outofplace-scale", "inplace-noscale"])
@pytest.mark.parametrize("smooth", [0.0, 0.1])
@pytest.mark.parametrize("V,ld", XENT_SHAPES)
def test_variant_xent(cuda, V, ld, smooth, how):
    """Labels at 0, 7, 8, 2047, 2048, V - 1 and on both sides of every register boundary of the
    register kernel; labels V and -5 (invalid, not ignore_index) and -100 give zero loss and a zero
    gradient row.  Runs the register kernels here and the two-pass kernel in the child process."""
    labels = _xent_labels(V, ld)
    _check_xent(cuda, V, ld, smooth, labels, how.startswith("inplace"), how.endswith("-scale"),
                "xent V%d ld%d s%g %s" % (V, ld, smooth, how))


@pytest.mark.gpu
def test_variant_xent_many_rows(cuda):
    """8200 rows at ld 64: more rows than the 8192 blocks, so blocks 0..7 take a second row."""
    labels = torch.randint(0, 64, (8200,), generator=_gen("xent-rows"))
    labels[::5] = -100
    labels[8195], labels[8199], labels[3] = 64, -5, 63
    _check_xent(cuda, 64, 64, 0.1, labels, True, True, "xent R8200")


# ------------------------------------------------------------------ GPU: which kernels ran
def _expected_kernels():
    """Kernel names the dispatchers of layernorm.hip and xent.hip pick in this process."""
    pf2 = os.environ.get("CLOUDTIK_AMD_LN_BWD_PF2", "1")[:1] != "0"
    reg = os.environ.get("CLOUDTIK_AMD_XENT_REG")
    reg = reg is None or (reg.strip().lstrip("+-").isdigit() and int(reg) != 0)      # the library's atoi(e) != 0
    t = lambda b: "true" if b else "false"  # noqa: E731
    # (N, form) -> <MAXV, RMS, EXTRA, DBIAS, FROMY, PF2>
    ln = {(520, "sum-db-p"): "ln_bwd_kernel<2, false, false, true, false, %s>" % t(pf2),
          (1536, "sum-nodb-extra"): "ln_bwd_kernel<3, false, true, false, false, %s>" % t(pf2),
          (8, "rms"): "ln_bwd_kernel<1, true, false, false, false, false>",
          (2048, "y-db-p"): "ln_bwd_kernel<4, false, false, true, true, false>"}
    xent = {1024: "xent_fwd_reg_kernel<4>" if reg else "xent_fwd_kernel",
            16392: "xent_fwd_reg_kernel<12>" if reg else "xent_fwd_kernel"}
    return ln, xent


@pytest.mark.gpu
def test_variant_kernels_selected(cuda):
    """The kernels that ran, by name from the profiler, are the ones the dispatchers are
    documented to pick under this process's variables: a child process cannot pass by quietly
    running the default kernels."""
    from torch.profiler import ProfilerActivity, profile
    ln, xent = _expected_kernels()
    forms = {f.name: f for f in FORMS}

    def names_of(fn, key):
        fn()                                            # warm: module load, allocations
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and key in e.name]

    for (N, form), want in ln.items():
        names = names_of(lambda: _check_ln_bwd(cuda, 5, N, forms[form]), "ln_bwd_kernel")
        assert names and all(want in n for n in names), (N, form, want, names)
    for ld, want in xent.items():
        V = ld - 2
        labels = _xent_labels(V, ld)
        names = names_of(lambda: _check_xent(cuda, V, ld, 0.0, labels, True, True, "names"), "xent_fwd")
        assert len(names) == 1 and want in names[0], (ld, want, names)


_VARIANTS = [{"CLOUDTIK_AMD_LN_BWD_PF2": "0"}, {"CLOUDTIK_AMD_XENT_REG": "0"}]


@pytest.mark.gpu
@pytest.mark.parametrize("knobs", _VARIANTS, ids=lambda d: ",".join("%s=%s" % (k[13:], v) for k, v in d.items()))
def test_nondefault_kernels_in_child_process(cuda, knobs):
    """The one-row-in-flight LayerNorm backward and the two-pass cross entropy at small ld, on the
    ``test_variant_*`` subset, in a child process with the variable set (read once per process)."""
    env = {k: v for k, v in os.environ.items() if k not in ("CLOUDTIK_AMD_LN_BWD_PF2", "CLOUDTIK_AMD_XENT_REG")}
    env.update(knobs)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-s", __file__, "-m", "gpu", "-k", "test_variant_",
                        "-p", "no:cacheprovider"], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and "skipped" not in r.stdout, r.stdout[-2000:]
    worst = {}
    for line in r.stdout.splitlines():
        if line.startswith("rowops-err "):
            for kv in line.split():
                if "=" in kv:
                    n, e = kv.split("=")
                    worst[n] = max(worst.get(n, 0.0), float(e))
    print("rowops-err-child %s %s" % (knobs, " ".join("%s=%.3e" % kv for kv in sorted(worst.items()))))
