"""Plain-PyTorch reference implementations of every cloudtik_amd HIP op.

Used (a) as the CPU execution path and (b) as the fp32 oracle in the GPU numerics
tests.  The dropout masks are bit-identical to the kernels': both evaluate the same
counter-based hash stream (``common.h: dropout_bits8``), so a CPU run and a GPU run of the
same model with the same seed drop the same elements.
"""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as F

M32 = np.uint64(0xFFFFFFFF)
ACT_NONE, ACT_GELU, ACT_RELU = 0, 1, 2


def _mix32(x):
    """common.h mix32 on uint64 arrays holding uint32 values."""
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7FEB352D)) & M32
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846CA68B)) & M32
    return x ^ (x >> np.uint64(16))


def _dropout_key(seed: int, offset: int) -> int:
    def m(x):
        return int(_mix32(np.array([x & 0xFFFFFFFF], dtype=np.uint64))[0])
    k = m(((offset >> 32) + 0x632BE5AB) & 0xFFFFFFFF)
    k = m(k ^ (offset & 0xFFFFFFFF))
    k = m(k ^ ((seed >> 32) & 0xFFFFFFFF))
    return m(k ^ (seed & 0xFFFFFFFF))


def dropout_threshold(p: float) -> int:
    t = float(p) * 4294967296.0
    return 0xFFFFFFFF if t >= 4294967295.0 else int(t)


def dropout_keep_mask(n: int, p: float, seed: int, offset: int) -> torch.Tensor:
    """Boolean keep-mask of ``n`` elements (n % 8 == 0), identical to the HIP kernels
    (common.h dropout_bits8: one 16-bit uniform per element from a hash of the pair counter)."""
    assert n % 8 == 0
    seed &= 0xFFFFFFFFFFFFFFFF
    offset &= 0xFFFFFFFFFFFFFFFF
    v = np.arange(n // 8, dtype=np.uint64)
    key = np.uint64(_dropout_key(seed, offset)) ^ _mix32((v >> np.uint64(30)) & M32)
    t16 = np.uint64(dropout_threshold(p) >> 16)
    out = np.empty((n // 8, 8), dtype=bool)
    for j in range(4):
        ctr = ((v << np.uint64(2)) | np.uint64(j)) & M32
        r = _mix32(((((ctr + key) & M32) * np.uint64(0x9E3779B1)) & M32) ^ key)
        out[:, 2 * j] = (r & np.uint64(0xFFFF)) >= t16
        out[:, 2 * j + 1] = (r >> np.uint64(16)) >= t16
    return torch.from_numpy(out.reshape(-1))


def dropout(x: torch.Tensor, p: float, seed: int, offset: int) -> torch.Tensor:
    if p <= 0.0:
        return x
    keep = dropout_keep_mask(x.numel(), p, seed, offset).to(x.device).view_as(x)
    return torch.where(keep, x * (1.0 / (1.0 - p)), torch.zeros_like(x))


def _round(x: torch.Tensor, like: torch.Tensor) -> torch.Tensor:
    return x.to(like.dtype).to(torch.float32) if like.dtype != torch.float32 else x


def layer_norm(x, gamma, beta=None, eps=1e-12, bias=None, residual=None, p=0.0, seed=0,
               offset=0, rms=False):
    """y = LN(residual + dropout(x + bias)); returns (y, s) with s the LN input."""
    xf = x.float()
    if bias is not None:
        xf = xf + bias.float()
    if p > 0.0:
        xf = dropout(xf, p, seed, offset)
    if residual is not None:
        xf = xf + residual.float()
    s = _round(xf, x)
    if rms:
        var = (s * s).mean(-1, keepdim=True)
        y = s * torch.rsqrt(var + eps) * gamma.float()
    else:
        mean = s.mean(-1, keepdim=True)
        var = ((s - mean) ** 2).mean(-1, keepdim=True)
        y = (s - mean) * torch.rsqrt(var + eps) * gamma.float()
        if beta is not None:
            y = y + beta.float()
    return y.to(x.dtype), s.to(x.dtype)


def bias_act(z, bias=None, act=ACT_GELU):
    t = z.float()
    if bias is not None:
        t = t + bias.float()
    if act == ACT_GELU:
        t = F.gelu(t)
    elif act == ACT_RELU:
        t = F.relu(t)
    return t.to(z.dtype)


def gated_gelu(g, u, p=0.0, seed=0, offset=0):
    """h = dropout_p(gelu_tanh(g) * u) in the input dtype, the hash mask of (seed, offset) over
    the contiguous output (T5 v1.1 feed-forward)."""
    return dropout(F.gelu(g, approximate="tanh") * u, p, seed, offset)


def embedding3(ids, tt, W, P=None, T=None):
    out = W.float()[ids]
    if P is not None:
        out = out + P.float()[: ids.shape[1]].unsqueeze(0)
    if T is not None:
        out = out + T.float()[tt if tt is not None else torch.zeros_like(ids)]
    return out.to(W.dtype)


def cross_entropy(logits, labels, V=None, ignore_index=-100, label_smoothing=0.0):
    """Mean CE over valid rows of logits[:, :V] (fp32 math)."""
    V = V or logits.shape[-1]
    return F.cross_entropy(logits[:, :V].float(), labels, ignore_index=ignore_index,
                           label_smoothing=label_smoothing)


def _hash_u32(x):
    x = x ^ (x >> 16)
    x = (x * 0x7FEB352D) & 0xFFFFFFFF
    x = x ^ (x >> 15)
    x = (x * 0x846CA68B) & 0xFFFFFFFF
    x = x ^ (x >> 16)
    return x


def attn_dropout_keep(B, H, Sq, Sk, p, seed, offset):
    """Keep mask [B, H, Sq, Sk] identical to the attention kernels' hash-based stream."""
    idx = np.arange(B * H * Sq * Sk, dtype=np.uint64).reshape(B, H, Sq, Sk)
    pair = idx >> np.uint64(1)
    half = (idx & np.uint64(1)).astype(np.uint64)
    s_lo = np.uint64(seed & 0xFFFFFFFF)
    s_hi = np.uint64((seed >> 32) & 0xFFFFFFFF)
    off = np.uint64(offset & 0xFFFFFFFF)
    base = _hash_u32((s_lo ^ (s_hi * np.uint64(0x85EBCA6B) & M32) ^ (off * np.uint64(0xC2B2AE35) & M32)) & M32)
    r = _hash_u32(((pair & M32) ^ base) & M32)
    r16 = (r >> (half * np.uint64(16))) & np.uint64(0xFFFF)
    thr = np.uint64(min(65535, int(round(p * 65536.0))))
    return torch.from_numpy(r16 >= thr)


def attention(q, k, v, key_bias=None, p=0.0, seed=0, offset=0, scale=None, causal=False):
    """q,k,v: [B, H, S, D]; key_bias: additive [B, Sk] (fp32). Returns [B, H, Sq, D]."""
    D = q.shape[-1]
    scale = scale if scale is not None else 1.0 / math.sqrt(D)
    s = torch.matmul(q.float(), k.float().transpose(-1, -2)) * scale
    if key_bias is not None:
        s = s + key_bias.float()[:, None, None, :]
    if causal:
        Sq, Sk = s.shape[-2:]
        m = torch.ones(Sq, Sk, dtype=torch.bool, device=s.device).triu(1)
        s = s.masked_fill(m, float("-inf"))
    pr = torch.softmax(s, -1)
    if p > 0.0:
        keep = attn_dropout_keep(*s.shape, p, seed, offset).to(s.device)
        pr = torch.where(keep, pr / (1.0 - p), torch.zeros_like(pr))
    return torch.matmul(pr, v.float()).to(q.dtype)


# ------------------------------------------------------------------ int8 quantization
def quantize_rows(x):
    """Symmetric per-row int8 quantization, the arithmetic of csrc/quant.hip: amax over the last
    dimension in fp32, scale = amax / 127, q = clamp(rne(x * (127 / amax)), -127, 127) with one
    fp32 multiply; an all-zero row gives scale 0 and q 0.  Returns (q int8, scale fp32)."""
    xf = x.float()
    amax = xf.abs().amax(-1, keepdim=True)
    # tensor / tensor: one IEEE division each (``127.0 / amax`` is reciprocal-then-multiply in
    # PyTorch, two roundings; a tensor divided by a Python scalar is too on some devices)
    c127 = torch.full_like(amax, 127.0)
    scale = amax / c127
    inv = torch.where(amax > 0, c127 / amax, torch.zeros_like(amax))
    q = torch.clamp(torch.round(xf * inv), -127.0, 127.0).to(torch.int8)
    return q, scale.squeeze(-1)


def gemm_i8_nt_raw(a_q, w_q):
    """The exact int32 accumulators of a_q [M, K] . w_q [N, K]^T."""
    return torch.matmul(a_q.to(torch.int32), w_q.to(torch.int32).t())


def dequant_epilogue(acc, a_scale, w_scale, bias=None, act=ACT_NONE, dtype=torch.float32, residual=None):
    """y = act(acc * (a_scale[m] * w_scale[n]) + bias[n]) in fp32, rounded to ``dtype``; with a
    ``residual`` [M, N] of ``dtype`` then y = round(float(y) + float(residual)) -- rounded BEFORE
    the add, so the fused op equals the unfused chain (the linear, then ``x + h`` in ``dtype``).
    ``act`` is ACT_NONE, ACT_GELU or ACT_RELU; ReLU together with a residual raises."""
    y = acc.to(torch.float32) * (a_scale.float().unsqueeze(-1) * w_scale.float().unsqueeze(0))
    if bias is not None:
        y = y + bias.float()
    if act == ACT_GELU:
        y = F.gelu(y)
    elif act == ACT_RELU:
        if residual is not None:
            raise ValueError("linear_i8: ACT_RELU together with a residual is not supported")
        y = F.relu(y)
    elif act != ACT_NONE:
        raise ValueError(f"linear_i8: unsupported activation {act}")
    y = y.to(dtype)
    if residual is not None:
        if residual.dtype != dtype or residual.shape != y.shape:
            raise ValueError(f"linear_i8: the residual must be {dtype} of shape {tuple(y.shape)}")
        y = (y.float() + residual.float()).to(dtype)
    return y


def linear_i8(a_q, a_scale, w_q, w_scale, bias=None, act=ACT_NONE, dtype=torch.float32, residual=None):
    """a_q [M, K] int8 with per-row scales against w_q [N, K] int8 with per-channel scales."""
    return dequant_epilogue(gemm_i8_nt_raw(a_q, w_q), a_scale, w_scale, bias, act, dtype, residual)


def rms_norm_quant(x, gamma, eps, residual=None):
    """(y, (q, scale)): y = RMSNorm(x + residual) * gamma exactly as ``layer_norm(..., rms=True)``
    returns it, and ``quantize_rows`` of that ROUNDED y."""
    y, _ = layer_norm(x, gamma, None, eps, None, residual, rms=True)
    return y, quantize_rows(y)


# ------------------------------------------------------------------ static int8 quantization
def _check_amax(amax) -> float:
    amax = float(amax)
    if not (0.0 <= amax < float("inf")):
        raise ValueError(f"a quantization range must be finite and non-negative, got {amax}")
    return amax


def static_scales(amax):
    """(scale, inv) of a calibrated range: scale = amax / 127 and inv = 127 / amax (0 for a zero
    range), each ONE IEEE fp32 division, returned as Python floats that hold the fp32 values
    exactly -- what the kernels receive by value."""
    import numpy as np
    a, c127 = np.float32(_check_amax(amax)), np.float32(127.0)
    if not np.isfinite(a):
        raise ValueError(f"a quantization range must fit fp32, got {amax}")
    with np.errstate(over="ignore"):
        inv = c127 / a if a > 0 else np.float32(0.0)
    if not np.isfinite(inv):
        raise ValueError(f"a quantization range this small has no fp32 inverse scale: {amax}")
    return float(a / c127), float(inv)


def quantize_static(x, amax):
    """Symmetric int8 quantization against a given range instead of the row maximum:
    q = clamp(rne(x * inv), -127, 127) with one fp32 multiply; values beyond ``amax`` saturate,
    ``amax == 0`` gives q == 0."""
    _, inv = static_scales(amax)
    xf = x.float()
    return torch.clamp(torch.round(xf * torch.full((), inv, dtype=torch.float32, device=xf.device)),
                       -127.0, 127.0).to(torch.int8)


def linear_i8_static(a_q, a_amax, w_q, w_scale, bias=None, act=ACT_NONE, out_amax=None, dtype=torch.float32):
    """``linear_i8`` with one activation scale for the whole tensor.  With ``out_amax`` the
    result, rounded to ``dtype`` first, is quantized against that range and returned as int8."""
    scale, _ = static_scales(a_amax)
    a_scale = torch.full((a_q.shape[0],), scale, dtype=torch.float32, device=a_q.device)
    y = dequant_epilogue(gemm_i8_nt_raw(a_q, w_q), a_scale, w_scale, bias, act, dtype)
    return y if out_amax is None else quantize_static(y, out_amax)


# ------------------------------------------------------------------ static int8 convolution
def _square(v, what) -> int:
    if isinstance(v, (tuple, list)):
        if len(v) != 2 or v[0] != v[1]:
            raise ValueError(f"conv_i8_static: {what} must be the same in both directions, got {tuple(v)}")
        v = v[0]
    return int(v)


def conv_geometry(x_shape, w_rows_shape, stride, padding, dilation=1, groups=1):
    """(R, stride, padding, Ho, Wo) of a square convolution given by its tap-major weight rows
    [Co, R*R*Ci]; raises ValueError for rows that are no whole square filter over all Ci channels
    (a grouped weight is not), and for a dilation or a group count other than 1."""
    if _square(dilation, "dilation") != 1 or int(groups) != 1:
        raise ValueError(f"conv_i8_static: dilation and groups must be 1, got {dilation} and {groups}")
    stride, padding = _square(stride, "stride"), _square(padding, "padding")
    if len(x_shape) != 4 or len(w_rows_shape) != 2:
        raise ValueError("conv_i8_static: expected x [N, Ci, H, W] and weight rows [Co, R*R*Ci]")
    ci, K = x_shape[1], w_rows_shape[1]
    R = math.isqrt(K // ci) if ci > 0 and K % ci == 0 else 0
    if R < 1 or R * R * ci != K:
        raise ValueError(f"conv_i8_static: rows of {K} are no square filter over {ci} input channels")
    if stride < 1 or padding < 0:
        raise ValueError(f"conv_i8_static: bad stride {stride} / padding {padding}")
    Ho, Wo = (x_shape[2] + 2 * padding - R) // stride + 1, (x_shape[3] + 2 * padding - R) // stride + 1
    if Ho < 1 or Wo < 1:
        raise ValueError("conv_i8_static: the filter does not fit the image")
    return R, stride, padding, Ho, Wo


def conv_i8_acc(x_q, w_q, stride, padding):
    """The exact int32 accumulators [N, Co, Ho, Wo] of an int8 convolution: x_q [N, Ci, H, W],
    w_q [Co, R*R*Ci] tap-major rows ([Co][R][S][Ci]).  int64 unfold + matmul (fp32 is not exact:
    one K = 4608 dot product of int8 products passes 2^24)."""
    R, stride, padding, Ho, Wo = conv_geometry(x_q.shape, w_q.shape, stride, padding)
    N, ci, H, W = x_q.shape
    co = w_q.shape[0]
    xp = F.pad(x_q.to(torch.int64), (padding, padding, padding, padding))
    cols = []
    for r in range(R):                                    # tap-major, channel-minor: the rows' order
        for s in range(R):
            cols.append(xp[:, :, r:r + (Ho - 1) * stride + 1:stride, s:s + (Wo - 1) * stride + 1:stride])
    a = torch.stack(cols, 1).reshape(N, R * R * ci, Ho * Wo)          # [N, K, P]
    acc = torch.matmul(w_q.to(torch.int64).unsqueeze(0), a)           # [N, Co, P]
    return acc.reshape(N, co, Ho, Wo).to(torch.int32)


def conv_i8_static(x_q, a_amax, w_q, w_scale, bias, stride, padding, relu, res_q=None, res_amax=None,
                   out_amax=None, dtype=torch.float32, dilation=1, groups=1):
    """Static int8 convolution with the epilogue of csrc/quant_conv.hip, one fp32 operation at a
    time and in its order:

        f = acc * (a_scale * w_scale[co]);  f = f + bias[co];  f = f + res_q * res_scale;
        f = max(f, 0) if relu;  y = f rounded to ``dtype``

    and, with ``out_amax``, ``quantize_static(y, out_amax)`` (int8) in place of y.  ``x_q`` is
    int8 [N, Ci, H, W], ``w_q`` int8 [Co, R*R*Ci] tap-major rows, ``w_scale`` and ``bias`` fp32
    [Co] (the bias carries the folded BatchNorm shift), ``res_q`` int8 of the output's shape with
    its range ``res_amax``."""
    conv_geometry(x_q.shape, w_q.shape, stride, padding, dilation, groups)
    if x_q.dtype != torch.int8 or w_q.dtype != torch.int8:
        raise TypeError("conv_i8_static: x_q and w_q must be int8")
    if (res_q is None) != (res_amax is None):
        raise ValueError("conv_i8_static: a residual needs its range, and a range its residual")
    a_scale, _ = static_scales(a_amax)
    acc = conv_i8_acc(x_q, w_q, stride, padding)
    one = lambda v: torch.full((), v, dtype=torch.float32, device=acc.device)
    f = acc.to(torch.float32) * (one(a_scale) * w_scale.float()).view(1, -1, 1, 1)
    f = f + bias.float().view(1, -1, 1, 1)
    if res_q is not None:
        if res_q.dtype != torch.int8 or res_q.shape != f.shape:
            raise ValueError("conv_i8_static: the residual must be int8 and have the output's shape")
        f = f + res_q.to(torch.float32) * one(static_scales(res_amax)[0])
    if relu:
        f = torch.clamp_min(f, 0.0)
    y = f.to(dtype)
    if x_q.is_contiguous(memory_format=torch.channels_last):
        y = y.contiguous(memory_format=torch.channels_last)
    return y if out_amax is None else quantize_static(y, out_amax)


def fold_bn(conv_weight, bn):
    """Fold an eval-mode BatchNorm into the bias-free convolution in front of it:
    (w_folded fp32 [Co, R*S*Ci] tap-major rows, bias fp32 [Co]) with
    bn(conv(x, w)) == conv(x, w_folded) + bias.  fp32 on the host, from the running statistics;
    ``bn`` is anything with weight, bias, running_mean, running_var and eps."""
    w = conv_weight.detach().float().cpu()
    g = bn.weight.detach().float().cpu() * torch.rsqrt(bn.running_var.detach().float().cpu() + bn.eps)
    rows = w.permute(0, 2, 3, 1).reshape(w.shape[0], -1) * g.unsqueeze(1)
    bias = bn.bias.detach().float().cpu() - bn.running_mean.detach().float().cpu() * g
    return rows.contiguous(), bias.contiguous()
