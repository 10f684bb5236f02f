"""Int8 post-training quantization ops (inference only): dynamic per-row activation
quantization and the int8 linear on the i8 matrix cores (csrc/quant.hip).

Number format: symmetric int8, no zero point; activations get one fp32 scale per row (token),
computed per call, weights one per output channel, computed once offline.  The rounding rule
is fixed (``reference.quantize_rows``), so the GPU kernel and the CPU reference agree bit for
bit on the quantized tensors, and the int32 accumulation is exact on both.

Static quantization (``quantize_static``, ``layer_norm_quant``, ``linear_i8_static``) applies the
same rule against one calibrated range per tensor, so the cast is elementwise and fused into
the kernel that produces the tensor.  ``conv2d_i8_static`` (csrc/quant_conv.hip) is the static int8
convolution, with BatchNorm folded into its weights and bias (``fold_bn``).

GPU tensors go to the HIP kernels (required; shapes outside their tiling raise), CPU tensors
to ``ops.reference``.
"""
from __future__ import annotations

from typing import Optional, Tuple, Union

import torch

from . import reference as ref

ACT_NONE, ACT_GELU = ref.ACT_NONE, ref.ACT_GELU

Quantized = Tuple[torch.Tensor, torch.Tensor]


def _pkg():
    from cloudtik_amd import ops
    return ops


def quantize_rows(x: torch.Tensor) -> Quantized:
    """x [..., K] -> (q int8 [..., K], scale fp32 [...]); x ~= q * scale[..., None]."""
    if _pkg()._use_native(x):
        if x.dtype != torch.bfloat16:
            raise TypeError(f"quantize_rows: GPU input must be bf16, got {x.dtype}")
        q, s = _pkg().require_native().quant_rows_i8(x.contiguous())
        return q, s
    return ref.quantize_rows(x)


def quantize_weight(w: torch.Tensor) -> Quantized:
    """w [N, K] -> (int8 [N, K], fp32 scale [N]), one scale per output channel; the arithmetic
    of ``quantize_rows``.  Offline, so plain PyTorch on the host (one implementation of the
    rounding rule, whatever device ``w`` lives on); the result is returned on ``w``'s device."""
    if w.dim() != 2:
        raise ValueError("quantize_weight: expected a [N, K] matrix")
    q, s = ref.quantize_rows(w.detach().cpu())
    return q.contiguous().to(w.device), s.contiguous().to(w.device)


def linear_i8(x: Union[torch.Tensor, Quantized], w_q: torch.Tensor, w_scale: torch.Tensor,
              bias: Optional[torch.Tensor] = None, act: int = ACT_NONE,
              dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    """act(x @ dequant(w_q)^T + bias) with int8 operands and exact int32 accumulation.

    ``x`` is a floating tensor [..., K] (quantized per row here) or the ``(q, scale)`` pair
    ``quantize_rows`` returned.  ``dtype`` is the output type; it defaults to the input's type
    (a quantized pair: bf16 on the GPU, fp32 on the CPU)."""
    if act not in (ACT_NONE, ACT_GELU):
        raise ValueError(f"linear_i8: act must be ACT_NONE or ACT_GELU, got {act}")
    if isinstance(x, torch.Tensor):
        if dtype is None:
            dtype = x.dtype
        a_q, a_s = quantize_rows(x)
    else:
        a_q, a_s = x
    lead = a_q.shape[:-1]
    K = a_q.shape[-1]
    N = w_q.shape[0]
    a2, s1 = a_q.reshape(-1, K), a_s.reshape(-1)
    if _pkg()._use_native(a_q, w_q):
        if dtype not in (None, torch.bfloat16):
            raise TypeError(f"linear_i8: the GPU kernel writes bf16, not {dtype}")
        out = torch.empty(a2.shape[0], N, device=a_q.device, dtype=torch.bfloat16)
        _pkg().require_native().gemm_i8_nt(a2.contiguous(), s1.contiguous(), w_q, w_scale, bias, int(act), out)
    else:
        out = ref.linear_i8(a2, s1, w_q, w_scale, bias, act, dtype or torch.float32)
    return out.view(*lead, N)


# ------------------------------------------------------------------ static (calibrated) ranges
# One fp32 range ``amax`` per site in place of the per-row maximum.  ``amax`` is a Python float:
# scale and inv are computed on the host (``reference.static_scales``) and reach the kernels by
# value, so nothing here reads a device scalar or synchronises.
def quantize_static(x: torch.Tensor, amax: float) -> torch.Tensor:
    """x [...] -> q int8 [...], q = clamp(rne(x * (127 / amax)), -127, 127); x ~= q * amax / 127."""
    _, inv = ref.static_scales(amax)
    if _pkg()._use_native(x):
        if x.dtype != torch.bfloat16:
            raise TypeError(f"quantize_static: GPU input must be bf16, got {x.dtype}")
        return _pkg().require_native().quant_static_i8(x.contiguous(), inv)
    return ref.quantize_static(x, amax)


def layer_norm_quant(x: torch.Tensor, gamma: torch.Tensor, beta: Optional[torch.Tensor] = None, eps: float = 1e-12,
                     bias: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None,
                     amax: Optional[float] = None) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """Inference LayerNorm that also emits its output quantized against ``amax``:
    y = LN(residual + (x + bias)) * gamma + beta, q = quantize_static(y, amax).  Returns (y, q);
    q is None when ``amax`` is None (the int8 output is switched off)."""
    inv = 0.0 if amax is None else ref.static_scales(amax)[1]
    if _pkg()._use_native(x):
        if x.dtype != torch.bfloat16:
            raise TypeError(f"layer_norm_quant: GPU input must be bf16, got {x.dtype}")
        y, q = _pkg().require_native().layernorm_quant_i8(
            x.contiguous(), bias, residual.contiguous() if residual is not None else None, gamma, beta,
            float(eps), inv, amax is not None)
        return y, q
    y, _ = ref.layer_norm(x, gamma, beta, eps, bias, residual)
    return y, (None if amax is None else ref.quantize_static(y, amax))


def linear_i8_static(x: torch.Tensor, a_amax: float, w_q: torch.Tensor, w_scale: torch.Tensor,
                     bias: Optional[torch.Tensor] = None, act: int = ACT_NONE, out_amax: Optional[float] = None,
                     dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    """``linear_i8`` with the calibrated activation range ``a_amax``.  ``x`` [..., K] is floating
    (quantized here) or already int8.  With ``out_amax`` the result -- rounded to ``dtype`` first
    -- comes back as int8 quantized against that range, ready for the next int8 linear."""
    if act not in (ACT_NONE, ACT_GELU):
        raise ValueError(f"linear_i8_static: act must be ACT_NONE or ACT_GELU, got {act}")
    a_scale, _ = ref.static_scales(a_amax)
    out_inv = 0.0 if out_amax is None else ref.static_scales(out_amax)[1]
    if x.dtype != torch.int8:
        if dtype is None:
            dtype = x.dtype
        x = quantize_static(x, a_amax)
    lead, K, N = x.shape[:-1], x.shape[-1], w_q.shape[0]
    a2 = x.reshape(-1, K)
    if _pkg()._use_native(x, w_q):
        if dtype not in (None, torch.bfloat16):
            raise TypeError(f"linear_i8_static: the GPU kernel computes bf16, not {dtype}")
        out = torch.empty(a2.shape[0], N, device=x.device, dtype=torch.bfloat16 if out_amax is None else torch.int8)
        _pkg().require_native().gemm_i8_nt_static(a2.contiguous(), a_scale, w_q, w_scale, bias, int(act), out, out_inv)
    else:
        out = ref.linear_i8_static(a2, a_amax, w_q, w_scale, bias, act, out_amax, dtype or torch.float32)
    return out.view(*lead, N)


# ------------------------------------------------------------------ static int8 convolution
fold_bn = ref.fold_bn


def conv2d_i8_static(x_q: torch.Tensor, a_amax: float, w_q: torch.Tensor, w_scale: torch.Tensor, bias: torch.Tensor,
                     stride, padding, relu: bool, res_q: Optional[torch.Tensor] = None,
                     res_amax: Optional[float] = None, out_amax: Optional[float] = None,
                     dtype: Optional[torch.dtype] = None, dilation=1, groups=1) -> torch.Tensor:
    """relu(conv(x_q, w_q) dequantized + bias + residual) with int8 operands and exact int32
    accumulation.  ``x_q`` int8 [N, Ci, H, W] (channels_last on the GPU) holds values of range
    ``a_amax``; ``w_q`` int8 [Co, R*R*Ci] are tap-major rows (``conv.weight_rows`` order) with fp32
    ``w_scale`` [Co]; ``bias`` is fp32 [Co] (with ``fold_bn`` it carries the BatchNorm shift);
    ``res_q`` int8 of the output's shape has range ``res_amax``.  The result is ``dtype`` (bf16 on
    the GPU, fp32 by default on the CPU), or with ``out_amax`` that result quantized against the
    range: int8, ready for the next convolution.

    The GPU kernel takes Ci and Co multiples of 64, 1x1 and 3x3 filters, stride 1 or 2, padding
    R // 2, groups = dilation = 1 and R*R*Ci <= 32768; anything else raises."""
    if _pkg()._use_native(x_q, w_q):
        R, stride, padding, Ho, Wo = ref.conv_geometry(x_q.shape, w_q.shape, stride, padding, dilation, groups)
        if dtype not in (None, torch.bfloat16):
            raise TypeError(f"conv2d_i8_static: the GPU kernel computes bf16, not {dtype}")
        if (res_q is None) != (res_amax is None):
            raise ValueError("conv2d_i8_static: a residual needs its range, and a range its residual")
        a_scale, _ = ref.static_scales(a_amax)
        res_scale = 0.0 if res_amax is None else ref.static_scales(res_amax)[0]
        out_inv = 0.0 if out_amax is None else ref.static_scales(out_amax)[1]
        out = torch.empty((x_q.shape[0], w_q.shape[0], Ho, Wo), device=x_q.device,
                          dtype=torch.bfloat16 if out_amax is None else torch.int8,
                          memory_format=torch.channels_last)
        _pkg().require_native().conv2d_i8_static(x_q, a_scale, w_q, w_scale, bias, stride, padding, bool(relu), res_q,
                                                 res_scale, out, out_inv)
        return out
    return ref.conv_i8_static(x_q, a_amax, w_q, w_scale, bias, stride, padding, relu, res_q, res_amax, out_amax,
                              dtype or torch.float32, dilation, groups)
