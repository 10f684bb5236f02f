"""Linear layer with the weight-gradient GEMM accumulating straight into the flat gradient
buffer ("gradient-accumulation fusion").

With PyTorch's stock ``F.linear`` backward, dW is produced into a fresh tensor and then
``AccumulateGrad`` adds it into ``param.grad`` -- one extra read-read-write pass over every
weight per step (the flat buffer of train.optim.FlatParamSpace is pre-set as ``.grad``).
Here the backward calls ``issue_wgrads`` instead, the one entry every weight gradient goes
through (this layer's and the transformer blocks'): on the side stream or in line, a lone
gradient through ``wgrad_accumulate`` -- the MFMA TN kernel, split-K fp32 slabs and a reduce
that adds them into the bf16 gradient; hipBLASLt where a shape is outside its tiling -- and the
gradients of one block through ``wgrad_accumulate_group``, one launch for all.  Because autograd
then never sees a weight gradient, the data-parallel bucketer is notified explicitly
(``param._ct_grad_ready``, installed by parallel.ddp.GradBucketer).
"""
from __future__ import annotations

import os
from typing import Optional

import torch
import torch.nn.functional as F

# bias gradients out of the MFMA weight-gradient GEMM (extra all-ones MFMA; ops/csrc/gemm_nt.hip)
_WGRAD_BIAS_FUSE = os.environ.get("CLOUDTIK_AMD_WGRAD_BIAS_FUSE", "1") == "1"
# split-K for weight-gradient GEMMs: 0 disables, otherwise the maximum split factor
_SPLITK_MAX = int(os.environ.get("CLOUDTIK_AMD_WGRAD_SPLITK", "8"))

# Weight-gradient GEMMs on a side HIP stream: they depend only on (dY, X) and write disjoint
# slices of the flat gradient buffer, so they can run concurrently with the dgrad chain of the
# backward pass (filling the CUs the dgrad GEMM's last wave leaves idle).  Consumers of the
# gradients -- the bucketed all-reduce and the optimizer -- order themselves after this
# stream via ``sync_grad_stream()``.
#
# The choice is a property of each weight (``param._ct_wgrad_side``, set per model by
# ``use_wgrad_side_stream``), read by the backward that produces its gradient: two models in
# one process keep their own routing, and nothing a model builder does changes another
# model's backward.  CLOUDTIK_AMD_WGRAD_STREAM (0 / 1) pins it for every model.
_WGRAD_STREAM_ENV = os.environ.get("CLOUDTIK_AMD_WGRAD_STREAM")
_DEFAULT_SIDE = (_WGRAD_STREAM_ENV or "1") == "1"
# weight-gradient GEMMs through the MFMA kernel's TN layout (csrc/gemm_nt.hip, ct_gemm_tn2)
# instead of hipBLASLt's batched split-K GEMM: 13-17 % faster per BERT-large layer
# (bench/gemm_tn2_probe.py); "blas" restores hipBLASLt
_HIP_WGRAD = os.environ.get("CLOUDTIK_AMD_WGRAD_KERNEL", "hip") == "hip"
# split-K partial GEMMs through the binding's strided-batched hipBLASLt call whose algorithm is
# chosen by timing every solution once per shape (torch.bmm's heuristic pick is not tuned:
# TunableOp skips bf16 -> fp32 batched GEMMs)
_LT_WGRAD = os.environ.get("CLOUDTIK_AMD_WGRAD_LT", "0") == "1"
# The two weight gradients of one transformer block (Wo + Wqkv, W2 + W1) as ONE grouped split-K
# launch (csrc/gemm_nt.hip ct_gemm_tn_group) + ONE grouped reduce: together they fill the CUs
# with half the slices, so half the fp32 slab bytes are written and read back, and four launches
# per block become two.  BERT-large, one MI355X, interleaved rounds on one box
# (profiles/wgrad_group/SUMMARY.md): in line 70.85-70.93 -> 69.96-70.10 ms/step, on the side
# stream 70.19-70.39 -> 69.66-69.92, so it is on for both routings.  CLOUDTIK_AMD_WGRAD_GROUP
# (0 / 1) pins it; with 0 the issue order and the kernels are those of the ungrouped path.
_WGRAD_GROUP_ENV = os.environ.get("CLOUDTIK_AMD_WGRAD_GROUP")
_WGRAD_GROUP_INLINE_DEFAULT = True
_WGRAD_GROUP_SIDE_DEFAULT = True
_streams = {}


def wgrad_group_enabled(side: bool, pair: str = "") -> bool:
    """Whether a block's weight gradients are issued as one grouped launch; ``side``: the
    weights' routing (side stream or in line); ``pair``: "attn" (Wo + Wqkv) or "ffn" (W2 + W1)
    -- CLOUDTIK_AMD_WGRAD_GROUP=attn / ffn groups that pair alone (for measuring them apart)."""
    if _WGRAD_GROUP_ENV is not None:
        return _WGRAD_GROUP_ENV == "1" or (pair != "" and _WGRAD_GROUP_ENV == pair)
    return _WGRAD_GROUP_SIDE_DEFAULT if side else _WGRAD_GROUP_INLINE_DEFAULT


def grad_stream():
    """The side stream used for weight-gradient GEMMs on the current device (or None
    without a GPU).  Created on first use; cached per device."""
    if not torch.cuda.is_available():
        return None
    dev = torch.cuda.current_device()
    s = _streams.get(dev)
    if s is None:
        s = _streams[dev] = torch.cuda.Stream(device=dev)
    return s


def use_wgrad_side_stream(params, enabled: Optional[bool]) -> bool:
    """A model's weight-gradient routing: ``params`` (an ``nn.Module`` or an iterable of
    parameters) get their gradients on the side stream when ``enabled`` (None: the process
    default), unless CLOUDTIK_AMD_WGRAD_STREAM pins it.  Worth it where the backward's
    critical path is memory-bound (ResNet-50: BatchNorm passes; the side stream saves 2.0 ms
    of 24.0 per step), not where it is two compute-bound GEMM streams competing for the
    matrix cores (BERT-large: 71.3 ms with it, 70.6 without; profiles/r4/bert_rejected_r4.md).
    Returns the setting in force."""
    val = _DEFAULT_SIDE if (_WGRAD_STREAM_ENV is not None or enabled is None) else bool(enabled)
    it = params.parameters() if hasattr(params, "parameters") else params
    for p in it:
        p._ct_wgrad_side = val
    return val


def wgrad_side(p) -> bool:
    """Whether parameter ``p``'s weight gradient goes to the side stream."""
    v = getattr(p, "_ct_wgrad_side", None)
    return _DEFAULT_SIDE if v is None else bool(v)


def sync_grad_stream() -> None:
    """Make the current stream wait for every weight gradient issued so far."""
    s = _streams.get(torch.cuda.current_device()) if torch.cuda.is_available() else None
    if s is not None:
        torch.cuda.current_stream().wait_stream(s)


_end_of_backward_sync_queued = False


def _join_grad_stream():
    """Autograd final callback: the streams that read gradients after ``backward()`` returns
    wait (on the GPU, no host sync) for every weight gradient issued on the side stream, so a
    plain ``param.grad`` read -- clipping, logging, a test -- never races the side stream."""
    global _end_of_backward_sync_queued
    _end_of_backward_sync_queued = False
    s = _streams.get(torch.cuda.current_device())
    if s is None:
        return
    cur = torch.cuda.current_stream()
    cur.wait_stream(s)
    default = torch.cuda.default_stream()
    if default != cur and not torch.cuda.is_current_stream_capturing():
        default.wait_stream(s)


def side_grad_stream():
    """``grad_stream()`` for work issued from inside a backward pass: the first call of a
    backward also queues the end-of-backward join (``_join_grad_stream``)."""
    global _end_of_backward_sync_queued
    s = grad_stream()
    if s is not None and not _end_of_backward_sync_queued and torch._C._current_graph_task_id() != -1:
        torch.autograd.Variable._execution_engine.queue_callback(_join_grad_stream)
        _end_of_backward_sync_queued = True
    return s


def _on_side_stream(issue, operands, enabled: bool) -> bool:
    """Run ``issue()`` on the gradient side stream, after everything queued on the current
    stream (dY / X produced, grad zeroed), and keep ``operands`` alive until it has run there;
    False (nothing issued) when ``enabled`` is False or there is no GPU."""
    s = side_grad_stream() if enabled else None
    if s is None:
        return False
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        issue()
    for t in operands:
        t.record_stream(s)
    return True


def wgrad_on_side_stream(g: torch.Tensor, dy2: torch.Tensor, x2: torch.Tensor,
                         dbias: Optional[torch.Tensor] = None, enabled: bool = True) -> bool:
    """Issue ``g += dy2^T x2`` (and ``dbias += column sums of dy2``) on the gradient side
    stream; False (nothing issued) when ``enabled`` is False or there is no GPU."""
    return _on_side_stream(lambda: wgrad_accumulate(g, dy2, x2, dbias), (dy2, x2), g.is_cuda and enabled)


def wgrad_group_on_side_stream(items, enabled: bool = True) -> bool:
    """``wgrad_accumulate_group(items)`` on the gradient side stream; False (nothing issued)
    when ``enabled`` is False or there is no GPU."""
    return _on_side_stream(lambda: wgrad_accumulate_group(items), [t for it in items for t in it[1:3]],
                           enabled and all(it[0].is_cuda for it in items))


def grad_ready(*params) -> None:
    """Tell the data-parallel bucketer that these parameters' gradients have been issued."""
    for p in params:
        cb = getattr(p, "_ct_grad_ready", None)
        if cb is not None:
            cb(p)


def issue_wgrads(items) -> None:
    """Accumulate the weight gradient of every ``(param, dy2, x2, bias_param_or_None)`` of
    ``items`` into ``param.grad`` (flat, one routing for all) and, with a bias, the column sums
    of dy2 into ``bias.grad``: on the side stream when the weights are routed there, else in
    line; one item through ``wgrad_accumulate``, several (one block's, same tokens) through
    ``wgrad_accumulate_group``.  Then every weight and bias is reported ready, in order."""
    args = [(p.grad, dy2, x2, b.grad if b is not None else None) for p, dy2, x2, b in items]
    side = wgrad_side(items[0][0])
    if len(args) == 1:
        if not wgrad_on_side_stream(*args[0], enabled=side):
            wgrad_accumulate(*args[0])
    elif not wgrad_group_on_side_stream(args, enabled=side):
        wgrad_accumulate_group(args)
    for p, _dy2, _x2, b in items:
        grad_ready(p)
        if b is not None:
            grad_ready(b)


def splitk_factor(T: int, N: int, K: int) -> int:
    """Split factor for dW[N,K] = dY[T,N]^T X[T,K].  hipBLASLt's 256x256 macro-tiles give only
    ceil(N/256)*ceil(K/256) workgroups (16..192 for BERT-large), far fewer than the 256 CUs;
    splitting the T reduction S ways multiplies the workgroup count (measured on MI355X,
    bench/gemm_bench.py: 1024x1024 wgrad 0.51 -> 0.81 PF/s at S=8, 3072x1024 0.67 -> 0.89)."""
    tiles = -(-N // 256) * -(-K // 256)
    S = 1
    while tiles * S < 256 and S < _SPLITK_MAX:
        S *= 2
    while S > 1 and (T % S or T // S < 2048):
        S //= 2
    return S


def _tn2_choose(T: int, tiles: int, nk: int, cus: int) -> int:
    """The MFMA wgrad kernel's slice count for ``tiles`` 256 x 256 output tiles holding ``nk``
    elements in all (any S: the kernel deals the T / 64 K-tiles out over the slices).
    Modelled time = K loop + fp32 slab round trip:
      loop(S) = t_full * waves(S) * cus / (tiles * S), waves = ceil(tiles * S / cus), with
      t_full the loop time at a perfect spread (2 nk T at ~1.3 PF/s, measured K-loop rate);
      slab(S) = S * tiles * 256 KiB * 2 (written, read back by the reduce) at ~5 TB/s (0 at S=1).
    >= 512 tokens per slice."""
    if tiles <= 0 or T % 64:
        return 1
    t_full = 2.0 * nk * T / 1.3e15
    best, best_cost = 1, None
    for S in range(1, 33):
        if S > 1 and (T // S < 512 or T // 64 < S):
            continue
        waves = -(-tiles * S // cus)
        cost = t_full * waves * cus / (tiles * S) + (S * tiles * 262144 * 2 / 5e12 if S > 1 else 0.0)
        if best_cost is None or cost < best_cost * (1 - 1e-9):
            best, best_cost = S, cost
    return best


def tn2_splits(T: int, N: int, K: int, cus: int = 256) -> int:
    """Split factor for one weight gradient dW[N, K] on the MFMA wgrad kernel (``_tn2_choose``).
    BERT-large: qkv 48 tiles -> 5 (240 workgroups, one wave; 16 power-of-two slices cost 3x the
    slab bytes), proj 16 tiles -> 16, FFN 64 tiles -> 4.  Counts whole tiles only: the caller
    checks N and K against the tiling."""
    return _tn2_choose(T, (N // 256) * (K // 256), N * K, cus)


def tn2_group_splits(T: int, shapes, cus: int = 256) -> int:
    """Slice count shared by several weight gradients dW_i[N_i, K_i] issued as one grouped
    launch: the ``tn2_splits`` cost model over the summed tile count and the summed FLOPs.
    BERT-large (T = 32768): Wo + Wqkv 64 tiles -> 4, W2 + W1 128 tiles -> 2.  1 when a shape is
    outside the kernel's tiling."""
    shapes = list(shapes)
    if not shapes or any(N <= 0 or K <= 0 or N % 256 or K % 256 for N, K in shapes):
        return 1
    return _tn2_choose(T, sum((N // 256) * (K // 256) for N, K in shapes), sum(N * K for N, K in shapes), cus)


_GROUP_MAX = 4      # problems per grouped GEMM launch, entries per grouped reduce launch


def _mfma_tn_ok(g: torch.Tensor, dy2: torch.Tensor, x2: torch.Tensor) -> bool:
    """Whether ``g += dy2^T x2`` takes the MFMA TN kernel: bf16 on a GPU, widths in whole
    256 x 256 tiles, tokens in whole 64-row K-tiles."""
    return (_HIP_WGRAD and g.is_cuda and g.dtype == torch.bfloat16 and dy2.dtype == torch.bfloat16
            and dy2.shape[1] % 256 == 0 and x2.shape[1] % 256 == 0 and dy2.shape[0] % 64 == 0)


def _bias_fused(dbias: Optional[torch.Tensor]) -> bool:
    """Whether this bias gradient comes out of the weight-gradient GEMM (all-ones MFMA)."""
    return (_WGRAD_BIAS_FUSE and dbias is not None and dbias.dtype == torch.bfloat16
            and dbias.is_contiguous())


def _group_qualifies(items) -> bool:
    """``_mfma_tn_ok`` for every problem, over one token count and on one device.  On top of
    it, what only the grouped entries need: a group always ends in the grouped reduce, which
    takes each g as a raw pointer to a dense [N, K] array and refuses one that is not 16-byte
    aligned (a lone gradient may be unsplit, written by the GEMM itself through g's stride);
    and a bad x2 dtype falls back here, to raise from the lone entry as it always has."""
    if not 2 <= len(items) <= _GROUP_MAX:
        return False
    T, dev = items[0][1].shape[0], items[0][0].device
    for g, dy2, x2, _db in items:
        if dy2.dim() != 2 or x2.dim() != 2 or dy2.shape[0] != T or x2.shape[0] != T:
            return False
        if not (_mfma_tn_ok(g, dy2, x2) and g.device == dev and x2.dtype == torch.bfloat16):
            return False
        if tuple(g.shape) != (dy2.shape[1], x2.shape[1]) or not g.is_contiguous() or g.data_ptr() % 16:
            return False
    return True


def wgrad_accumulate_group(items) -> None:
    """``wgrad_accumulate(g, dy2, x2, dbias)`` for every ``(g, dy2, x2, dbias)`` of ``items``
    (weight gradients over the same tokens, e.g. the two of one transformer block) as one
    grouped split-K GEMM into one fp32 workspace and one grouped reduce.  Falls back to the
    per-problem calls when the slice chooser returns 1, a tensor does not qualify or the
    native entry refuses."""
    items = list(items)
    S = 1
    if _group_qualifies(items):
        S = tn2_group_splits(items[0][1].shape[0], [(dy2.shape[1], x2.shape[1]) for _g, dy2, x2, _db in items])
    if S < 2:
        for it in items:
            wgrad_accumulate(*it)
        return
    from cloudtik_amd import ops
    C = ops.require_native()
    # the grouped reduce refuses a misaligned bias gradient: that one takes the column-sum kernel
    fuse = [_bias_fused(db) and db.data_ptr() % 16 == 0 for _g, _dy2, _x2, db in items]
    sizes = [S * dy2.shape[1] * x2.shape[1] for _g, dy2, x2, _db in items]
    bsizes = [S * it[1].shape[1] if f else 0 for it, f in zip(items, fuse)]
    ws = torch.empty(sum(sizes) + sum(bsizes), device=items[0][0].device, dtype=torch.float32)
    A, B, P, bP, off = [], [], [], [], 0
    for (_g, dy2, x2, _db), n in zip(items, sizes):
        A.append(dy2.contiguous())
        B.append(x2.contiguous())
        P.append(ws[off:off + n].view(S, dy2.shape[1], x2.shape[1]))
        off += n
    for (_g, dy2, _x2, _db), n in zip(items, bsizes):
        bP.append(ws[off:off + n].view(S, dy2.shape[1]) if n else None)
        off += n
    if not C.gemm_tn_group(A, B, P, bP, S):
        for it in items:
            wgrad_accumulate(*it)
        return
    red = [(p, it[0]) for p, it in zip(P, items)] + [(b, it[3]) for b, it in zip(bP, items) if b is not None]
    for i in range(0, len(red), _GROUP_MAX):
        C.splitk_reduce_group([p for p, _ in red[i:i + _GROUP_MAX]], [g for _, g in red[i:i + _GROUP_MAX]], True)
    for (_g, dy2, _x2, db), f in zip(items, fuse):
        if db is not None and not f:
            _bias_colsum(db, dy2)


def _bias_colsum(dbias: torch.Tensor, dy2: torch.Tensor) -> None:
    """dbias += column sums of dy2 (fp32 accumulation)."""
    if dbias.is_cuda and dbias.dtype == torch.bfloat16 and dbias.is_contiguous() and dy2.shape[1] % 8 == 0:
        from cloudtik_amd import ops
        ops.require_native().bias_act_bwd_into(dy2.contiguous(), dy2.contiguous(), None, 0, dbias, False)
    else:
        dbias.add_(dy2.float().sum(0).to(dbias.dtype))


def wgrad_accumulate(g: torch.Tensor, dy2: torch.Tensor, x2: torch.Tensor,
                     dbias: Optional[torch.Tensor] = None) -> None:
    """g += dy2^T x2 (bf16 g, fp32 accumulation); with ``dbias``, also dbias += column sums of
    dy2 (the bias gradient).  The MFMA kernel's TN layout with split-K fp32 slabs + one fused
    reduce-accumulate kernel (or, unsplit, accumulating straight into g), the bias sums coming
    out of the same kernel (one extra MFMA per A fragment against an all-ones operand);
    otherwise hipBLASLt's batched split-K GEMM, or its beta=1 epilogue when one split fills
    the GPU, plus a column-sum kernel for the bias."""
    T, N = dy2.shape
    K = x2.shape[1]
    if _mfma_tn_ok(g, dy2, x2):
        from cloudtik_amd import ops
        C = ops.require_native()
        S = tn2_splits(T, N, K)
        dy2c, x2c = dy2.contiguous(), x2.contiguous()
        fuse_bias = _bias_fused(dbias)
        bP = torch.empty(S, N, device=g.device, dtype=torch.float32) if fuse_bias else None
        out = g if S == 1 else torch.empty(S, N, K, device=g.device, dtype=torch.float32)
        ok = (C.gemm_tn2_bias(dy2c, x2c, out, S, S == 1, bP) if fuse_bias
              else C.gemm_tn2(dy2c, x2c, out, S, S == 1))
        if ok:
            if S > 1 and fuse_bias:
                C.splitk_reduce2(out, g, bP, dbias, True)     # slabs + bias partials, one launch
            elif S > 1:
                C.splitk_reduce(out, g, True)
            elif fuse_bias:
                C.splitk_reduce(bP, dbias, True)
            if dbias is not None and not fuse_bias:
                _bias_colsum(dbias, dy2)
            return
    if dbias is not None:
        _bias_colsum(dbias, dy2)
    S = splitk_factor(T, N, K) if (g.is_cuda and g.dtype == torch.bfloat16 and g.is_contiguous()) else 1
    if S == 1:
        g.addmm_(dy2.t(), x2)
        return
    from cloudtik_amd import ops
    dy2 = dy2.contiguous()
    x2 = x2.contiguous()
    if _LT_WGRAD:
        C = ops.require_native()
        Ts = T // S
        P = torch.empty(S, N, K, device=g.device, dtype=torch.float32)
        # P[s] = dy2[s*Ts:(s+1)*Ts]^T @ x2[s*Ts:(s+1)*Ts]
        if C.lt_bmm_tuned(dy2[:Ts], x2[:Ts], P[0], True, False, S, Ts * N, Ts * K, N * K, 0) >= 0:
            C.splitk_reduce(P, g, True)
            return
    P = torch.bmm(dy2.view(S, T // S, N).transpose(1, 2), x2.view(S, T // S, K), out_dtype=torch.float32)
    ops.require_native().splitk_reduce(P, g, True)


class _LinearFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias):
        ctx.save_for_backward(x, weight)
        ctx.weight_param = weight
        ctx.has_bias = bias is not None
        return F.linear(x, weight, bias)

    @staticmethod
    def backward(ctx, dy):
        x, W = ctx.saved_tensors
        Wp = ctx.weight_param
        out_f, in_f = W.shape
        dy2 = dy.reshape(-1, out_f)
        x2 = x.reshape(-1, in_f)
        dx = torch.matmul(dy, W) if ctx.needs_input_grad[0] else None
        dW = None
        if ctx.needs_input_grad[1]:
            g = Wp.grad
            if g is not None and getattr(Wp, "_ct_flat_grad", False) and g.dtype == dy.dtype:
                issue_wgrads([(Wp, dy2, x2, None)])
            else:
                dW = torch.matmul(dy2.t(), x2)
        db = dy2.sum(0) if ctx.has_bias and ctx.needs_input_grad[2] else None
        return dx, dW, db


def linear(x, weight, bias=None):
    """y = x @ weight^T + bias with flat-buffer weight-gradient accumulation on GPU.

    Assumes ``weight`` is used by exactly one ``linear`` call per backward pass (its
    readiness is reported to the gradient bucketer when this GEMM has been issued); use
    ``F.linear`` for shared/tied weights."""
    if x.is_cuda and weight.requires_grad and torch.is_grad_enabled():
        return _LinearFn.apply(x, weight, bias)
    return F.linear(x, weight, bias)
