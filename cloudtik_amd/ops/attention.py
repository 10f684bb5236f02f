"""Fused attention front-end (HIP MFMA kernels in csrc/attention.hip).

Two entry points:

* :func:`attention_packed` -- BERT/GPT path: takes the packed QKV projection output
  ``[B, S, 3*H*64]`` (no permute/contiguous copies: the kernel reads Q, K, V through
  strides), returns ``[B, S, H*64]`` ready for the output projection, and its backward
  writes dQ, dK, dV into ONE packed ``[B, S, 3*H*64]`` gradient so the QKV projection's
  backward is a single GEMM.
* :func:`attention` -- generic ``[B, H, S, D]`` tensors (torch SDPA layout).  D = 64 trains;
  D = 128 takes the inference kernel when the call needs neither a gradient nor dropout.
* :func:`attention_relbias` -- ``[B, S, H, D]`` tensors with a T5 relative-position bias vector
  (or none: ``rel_bias=None``); D = 64 and D = 128 both train.

``key_bias`` is an additive fp32 ``[B, Sk]`` per-key bias (HF BERT: ``(1 - mask) * -10000``).
"""
from __future__ import annotations

import math

import torch

from . import reference as ref


def _ops():
    from cloudtik_amd import ops
    return ops


class _AttnPackedFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, H, key_bias, scale, p, seed, offset, causal):
        B, S, W = qkv.shape
        D = W // (3 * H)
        v5 = qkv.view(B, S, 3, H, D)
        q, k, v = v5[:, :, 0], v5[:, :, 1], v5[:, :, 2]
        o = torch.empty(B, S, H, D, dtype=qkv.dtype, device=qkv.device)
        lse = _ops().require_native().attn_fwd(q, k, v, o, key_bias, scale, p, seed, offset, causal)
        ctx.save_for_backward(qkv, o, lse, key_bias if key_bias is not None else torch.empty(0))
        ctx.cfg = (H, scale, p, seed, offset, causal, key_bias is not None)
        return o.view(B, S, H * D)

    @staticmethod
    def backward(ctx, do):
        qkv, o, lse, kb = ctx.saved_tensors
        H, scale, p, seed, offset, causal, has_kb = ctx.cfg
        B, S, W = qkv.shape
        D = W // (3 * H)
        v5 = qkv.view(B, S, 3, H, D)
        dqkv = torch.empty_like(qkv)
        d5 = dqkv.view(B, S, 3, H, D)
        do4 = do.contiguous().view(B, S, H, D)
        _ops().require_native().attn_bwd(v5[:, :, 0], v5[:, :, 1], v5[:, :, 2], o, do4,
                                         d5[:, :, 0], d5[:, :, 1], d5[:, :, 2],
                                         kb if has_kb else None, lse, scale, p, seed, offset, causal)
        return dqkv, None, None, None, None, None, None, None


class _AttnFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, key_bias, scale, p, seed, offset, causal):
        # q, k, v: [B, S, H, D] views
        B, Sq, H, D = q.shape
        o = torch.empty(B, Sq, H, D, dtype=q.dtype, device=q.device)
        lse = _ops().require_native().attn_fwd(q, k, v, o, key_bias, scale, p, seed, offset, causal)
        ctx.save_for_backward(q, k, v, o, lse, key_bias if key_bias is not None else torch.empty(0))
        ctx.cfg = (scale, p, seed, offset, causal, key_bias is not None)
        return o

    @staticmethod
    def backward(ctx, do):
        q, k, v, o, lse, kb = ctx.saved_tensors
        scale, p, seed, offset, causal, has_kb = ctx.cfg
        dq = torch.empty(q.shape, dtype=q.dtype, device=q.device)
        dk = torch.empty(k.shape, dtype=k.dtype, device=k.device)
        dv = torch.empty(v.shape, dtype=v.dtype, device=v.device)
        _ops().require_native().attn_bwd(q, k, v, o, do.contiguous(), dq, dk, dv,
                                         kb if has_kb else None, lse, scale, p, seed, offset, causal)
        return dq, dk, dv, None, None, None, None, None, None


def _native_ok(t, D):
    return t.is_cuda and t.dtype == torch.bfloat16 and D == 64


def _fwd_only_d128(q, k, v, p):
    """A D = 128 call :func:`attention` sends to the inference kernel: bf16 on the GPU, no dropout,
    and nothing autograd would record."""
    return (q.is_cuda and q.dtype == torch.bfloat16 and p == 0
            and not (torch.is_grad_enabled() and (q.requires_grad or k.requires_grad or v.requires_grad)))


def attention_packed(qkv, num_heads, key_bias=None, p=0.0, training=True, scale=None,
                     causal=False):
    """qkv: [B, S, 3*H*D] -> [B, S, H*D]."""
    B, S, W = qkv.shape
    D = W // (3 * num_heads)
    scale = float(scale if scale is not None else 1.0 / math.sqrt(D))
    p = float(p) if training else 0.0
    ops = _ops()
    seed, offset = ops._rng.next(B * num_heads * S * S) if p > 0 else (0, 0)
    if key_bias is not None:
        key_bias = key_bias.float().contiguous()
    if ops._use_native(qkv) and _native_ok(qkv, D) and (p == 0 or S % 2 == 0):
        return _AttnPackedFn.apply(qkv.contiguous(), num_heads, key_bias, scale, p, seed, offset, bool(causal))
    v5 = qkv.view(B, S, 3, num_heads, D).permute(2, 0, 3, 1, 4)
    o = ref.attention(v5[0], v5[1], v5[2], key_bias, p, seed, offset, scale, causal)
    return o.permute(0, 2, 1, 3).reshape(B, S, num_heads * D)


def attention(q, k, v, key_bias=None, p=0.0, scale=None, causal=False):
    """q, k, v: [B, H, S, D] -> [B, H, Sq, D].  At D = 128 a call with a gradient or with p > 0
    returns exactly the PyTorch reference's result here; the D = 128 training kernels are reached
    through ``attention_relbias(..., rel_bias=None)`` in the ``[B, S, H, D]`` layout."""
    B, H, Sq, D = q.shape
    Sk = k.shape[2]
    scale = float(scale if scale is not None else 1.0 / math.sqrt(D))
    ops = _ops()
    seed, offset = ops._rng.next(B * H * Sq * Sk) if p > 0 else (0, 0)
    if key_bias is not None:
        key_bias = key_bias.float().contiguous()
    if D == 128 and _fwd_only_d128(q, k, v, p) and ops._use_native(q):
        # head dim 128: the inference call only (training: attention_relbias), so not through _AttnFn
        qt = q.transpose(1, 2)
        o = torch.empty(qt.shape, dtype=q.dtype, device=q.device)
        ops.require_native().attn_fwd(qt, k.transpose(1, 2), v.transpose(1, 2), o, key_bias, scale, 0.0, 0, 0,
                                      bool(causal))
        return o.transpose(1, 2)
    if ops._use_native(q) and _native_ok(q, D) and (p == 0 or Sk % 2 == 0):
        o = _AttnFn.apply(q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2), key_bias, scale,
                          float(p), seed, offset, bool(causal))
        return o.transpose(1, 2)
    return ref.attention(q, k, v, key_bias, p, seed, offset, scale, causal)




class _AttnRelFn(torch.autograd.Function):
    """Relative-bias attention at head dim 64 or 128: attn_fwd_relbias_train / attn_bwd_relbias."""

    @staticmethod
    def forward(ctx, q, k, v, rel_bias, key_bias, rel_base, scale, p, seed, offset, causal):
        # q, k, v: [B, S, H, D]; rel_bias: [H, L] in any layout and dtype
        relc = rel_bias.detach().float().contiguous()
        o = torch.empty(q.shape, dtype=q.dtype, device=q.device)
        lse = _ops().require_native().attn_fwd_relbias_train(q, k, v, o, key_bias, relc, rel_base, scale, p, seed,
                                                             offset, causal)
        ctx.save_for_backward(q, k, v, o, lse, relc, rel_bias, key_bias if key_bias is not None else torch.empty(0))
        ctx.cfg = (rel_base, scale, p, seed, offset, causal, key_bias is not None)
        return o

    @staticmethod
    def backward(ctx, do):
        q, k, v, o, lse, relc, rel_bias, kb = ctx.saved_tensors
        rel_base, scale, p, seed, offset, causal, has_kb = ctx.cfg
        dq = torch.empty(q.shape, dtype=q.dtype, device=q.device)
        dk = torch.empty(k.shape, dtype=k.dtype, device=k.device)
        dv = torch.empty(v.shape, dtype=v.dtype, device=v.device)
        # the gradient in the layout of the bias that was passed (the T5 model passes the
        # transpose of an [L, H] gather, so its backward gets a contiguous [L, H])
        d_rel = torch.empty_like(rel_bias, dtype=torch.float32)
        _ops().require_native().attn_bwd_relbias(q, k, v, o, do.contiguous(), dq, dk, dv, d_rel,
                                                 kb if has_kb else None, relc, rel_base, lse, scale, p, seed, offset,
                                                 causal)
        return dq, dk, dv, d_rel.to(rel_bias.dtype), None, None, None, None, None, None, None


class _AttnTrainFn(torch.autograd.Function):
    """Attention without a bias vector on [B, S, H, D] views, head dim 64 or 128: attn_fwd_train /
    attn_bwd_train."""

    @staticmethod
    def forward(ctx, q, k, v, key_bias, scale, p, seed, offset, causal):
        o = torch.empty(q.shape, dtype=q.dtype, device=q.device)
        lse = _ops().require_native().attn_fwd_train(q, k, v, o, key_bias, scale, p, seed, offset, causal)
        ctx.save_for_backward(q, k, v, o, lse, key_bias if key_bias is not None else torch.empty(0))
        ctx.cfg = (scale, p, seed, offset, causal, key_bias is not None)
        return o

    @staticmethod
    def backward(ctx, do):
        q, k, v, o, lse, kb = ctx.saved_tensors
        scale, p, seed, offset, causal, has_kb = ctx.cfg
        dq = torch.empty(q.shape, dtype=q.dtype, device=q.device)
        dk = torch.empty(k.shape, dtype=k.dtype, device=k.device)
        dv = torch.empty(v.shape, dtype=v.dtype, device=v.device)
        _ops().require_native().attn_bwd_train(q, k, v, o, do.contiguous(), dq, dk, dv, kb if has_kb else None, lse,
                                               scale, p, seed, offset, causal)
        return dq, dk, dv, None, None, None, None, None, None


def _relbias_reference(q, k, v, rel_bias, rel_base, key_bias, scale, causal, p, seed, offset):
    """PyTorch fallback of attention_relbias: fp32, differentiable; p > 0 drops the elements the
    kernels drop (ref.attn_dropout_keep).  Without a bias vector it is ref.attention on the
    transposed layout."""
    if rel_bias is None:
        return ref.attention(q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2), key_bias, p, seed, offset,
                             scale, causal).transpose(1, 2)
    B, Sq, H, D = q.shape
    Sk = k.shape[1]
    idx = (torch.arange(Sk, device=q.device)[None, :] - torch.arange(Sq, device=q.device)[:, None] + rel_base)
    bias = rel_bias.float()[:, idx.clamp(0, rel_bias.shape[1] - 1)][None]            # [1, H, Sq, Sk]
    if key_bias is not None:
        bias = bias + key_bias.float()[:, None, None, :]
    s = torch.einsum("bqhd,bkhd->bhqk", q.float(), k.float()) * scale + bias
    if causal:
        s = s.masked_fill(torch.ones(Sq, Sk, dtype=torch.bool, device=q.device).triu(1), float("-inf"))
    pr = torch.softmax(s, -1)
    if p > 0.0:
        keep = ref.attn_dropout_keep(B, H, Sq, Sk, p, seed, offset).to(q.device)
        pr = torch.where(keep, pr / (1.0 - p), torch.zeros_like(pr))
    return torch.einsum("bhqk,bkhd->bqhd", pr, v.float()).to(q.dtype)


def attention_relbias(q, k, v, rel_bias, rel_base: int = 0, key_bias=None, scale: float = 1.0, causal: bool = False,
                      p: float = 0.0):
    """Attention with a relative-position bias (T5): q/k/v ``[B, S, H, D]``, ``rel_bias [H, L]``
    adds ``rel_bias[h, k - q + rel_base]`` to every score (natural-log units), ``key_bias
    [B, Sk]`` masks keys, ``p`` is attention-probability dropout (the stream of
    :func:`attention`).  ``rel_bias=None`` is plain attention in this layout: no bias, no bias
    gradient (T5 cross-attention).  HIP MFMA kernels on the GPU in bf16 at D = 64 and D = 128,
    both differentiable in q, k, v and ``rel_bias`` (the gradient of ``rel_bias`` sums fp32 dS with
    LDS float adds and is not bitwise reproducible).  Everything else -- CPU or fp32 tensors, odd
    Sk with p > 0, L > 4096, a query length whose backward windows do not fit the kernel's LDS
    budget (D = 64: Sq > 1856; none at D = 128 within L <= 4096) -- takes the differentiable
    PyTorch reference."""
    B, Sq, H, D = q.shape
    Sk = k.shape[1]
    p = float(p)
    ops = _ops()
    seed, offset = ops._rng.next(B * H * Sq * Sk) if p > 0 else (0, 0)
    rel = rel_bias is not None
    native = (q.is_cuda and q.dtype == torch.bfloat16 and D in (64, 128) and (not rel or rel_bias.shape[1] <= 4096)
              and ops.native_available())
    grad = torch.is_grad_enabled() and (q.requires_grad or k.requires_grad or v.requires_grad
                                        or (rel and rel_bias.requires_grad))
    kb = key_bias.float().contiguous() if (native and key_bias is not None) else None
    if native and not grad and p == 0:
        o = torch.empty_like(q)
        if rel:
            ops.require_native().attn_fwd_relbias(q, k, v, o, kb, rel_bias.float().contiguous(), int(rel_base),
                                                  float(scale), bool(causal))
        else:
            ops.require_native().attn_fwd(q, k, v, o, kb, float(scale), 0.0, 0, 0, bool(causal))
        return o
    if native and (p == 0 or Sk % 2 == 0):
        if not rel:
            return _AttnTrainFn.apply(q, k, v, kb, float(scale), p, seed, offset, bool(causal))
        C = ops.require_native()
        if not grad or C.attn_bwd_relbias_window(Sq) <= C.attn_bwd_relbias_max_window_d(D):
            return _AttnRelFn.apply(q, k, v, rel_bias, kb, int(rel_base), float(scale), p, seed, offset,
                                    bool(causal))
    return _relbias_reference(q, k, v, rel_bias, rel_base, key_bias, float(scale), causal, p, seed, offset)
