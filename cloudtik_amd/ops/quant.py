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

Decoding (csrc/quant_skinny.hip): ``linear_i8`` with up to ``SKINNY_MAX_M`` rows runs in a one-launch
weight-streaming kernel whose epilogue also carries a ReLU or a residual add, and ``rms_norm_quant``
is the RMS norm that emits the int8 rows and scales of the linear behind it.

GPU tensors go to the HIP kernels (required; shapes outside their tiling raise), CPU tensors
to ``ops.reference``.
"""
from __future__ import annotations

import os
from typing import Optional, Tuple, Union

import torch

from . import reference as ref

ACT_NONE, ACT_GELU, ACT_RELU = ref.ACT_NONE, ref.ACT_GELU, ref.ACT_RELU

SKINNY_MAX_M = 64         # rows the decode GEMM (csrc/quant_skinny.hip) takes

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


def skinny_enabled() -> bool:
    """``CLOUDTIK_AMD_I8_SKINNY=0`` sends every ``linear_i8`` to the tiled kernel (A/B runs)."""
    return os.environ.get("CLOUDTIK_AMD_I8_SKINNY", "1") != "0"


def linear_i8(x: Union[torch.Tensor, Quantized], w_q: torch.Tensor, w_scale: torch.Tensor,
              bias: Optional[torch.Tensor] = None, act: int = ACT_NONE,
              dtype: Optional[torch.dtype] = None, residual: Optional[torch.Tensor] = None,
              out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """act(x @ dequant(w_q)^T + bias) (+ residual) with int8 operands and exact int32 accumulation.

    ``x`` is a floating tensor [..., K] (quantized per row here) or the ``(q, scale)`` pair
    ``quantize_rows`` returned.  ``dtype`` is the output type; it defaults to the input's type
    (a quantized pair: bf16 on the GPU, fp32 on the CPU).  ``act`` is ACT_NONE, ACT_GELU or
    ACT_RELU.  ``residual`` [..., N] of the output type is added to the ROUNDED result
    (``reference.dequant_epilogue`` states the rule), so the call equals the linear followed by
    ``residual + h``; it does not combine with ACT_RELU.  ACT_RELU is the bias-free epilogue T5's
    feed-forward needs: together with a ``bias`` it raises, as every ReLU call did before this
    activation existed here (``reference.dequant_epilogue`` and the kernel take both).  ``out``
    (GPU) receives the result and may be the residual itself.

    On the GPU up to ``SKINNY_MAX_M`` rows without a bias, with ACT_NONE / ACT_RELU, run in the
    one-launch decode kernel, epilogue included; everything else (more rows, GELU, and calls with
    a bias: the classifier's, which keep the kernel they had) runs in the tiled kernel, with ReLU
    and the residual applied by PyTorch ops after it."""
    if act not in (ACT_NONE, ACT_GELU, ACT_RELU):
        raise ValueError(f"linear_i8: act must be ACT_NONE, ACT_GELU or ACT_RELU, got {act}")
    if act == ACT_RELU and residual is not None:
        raise ValueError("linear_i8: ACT_RELU together with a residual is not supported")
    if act == ACT_RELU and bias is not None:
        raise ValueError("linear_i8: ACT_RELU together with a bias is not supported")
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
    r2 = None
    if residual is not None:
        if residual.shape != (*lead, N):
            raise ValueError(f"linear_i8: the residual must have shape {(*lead, N)}, got {tuple(residual.shape)}")
        r2 = residual.reshape(-1, N)
    if _pkg()._use_native(a_q, w_q):
        if dtype not in (None, torch.bfloat16):
            raise TypeError(f"linear_i8: the GPU kernel writes bf16, not {dtype}")
        M = a2.shape[0]
        if out is None:
            o2 = torch.empty(M, N, device=a_q.device, dtype=torch.bfloat16)
        else:
            if out.shape != (*lead, N) or out.dtype != torch.bfloat16 or not out.is_contiguous():
                raise ValueError(f"linear_i8: out must be a contiguous bf16 tensor of shape {(*lead, N)}")
            o2 = out.view(M, N)
        C = _pkg().require_native()
        if M <= SKINNY_MAX_M and bias is None and act != ACT_GELU and skinny_enabled():
            C.gemm_i8_skinny(a2.contiguous(), s1.contiguous(), w_q, w_scale, bias, int(act),
                             r2.contiguous() if r2 is not None else None, o2)
        else:
            # the tiled kernel has no ReLU / residual epilogue: the same arithmetic as PyTorch ops
            # (ReLU commutes with the rounding; the bf16 add rounds the sum of the rounded result)
            tiled = o2 if r2 is None else torch.empty_like(o2)
            C.gemm_i8_nt(a2.contiguous(), s1.contiguous(), w_q, w_scale, bias,
                         int(ACT_GELU if act == ACT_GELU else ACT_NONE), tiled)
            if act == ACT_RELU:
                torch.relu_(tiled)
            if r2 is not None:
                torch.add(tiled, r2, out=o2)
        res = o2
    else:
        if out is not None:
            raise ValueError("linear_i8: out belongs to the GPU path")
        res = ref.linear_i8(a2, s1, w_q, w_scale, bias, act, dtype or torch.float32, r2)
    return res.view(*lead, N)


def rms_norm_quant(x: torch.Tensor, gamma: torch.Tensor, eps: float, residual: Optional[torch.Tensor] = None,
                   emit_y: bool = True) -> Tuple[Optional[torch.Tensor], Quantized]:
    """RMS norm that also emits its output quantized per row: ``(y, (q, scale))`` with
    y = RMSNorm(x + residual) * gamma exactly what ``ops.layer_norm(..., rms=True)`` returns and
    ``(q, scale) = quantize_rows(y)``, computed from the rounded y.  One kernel on the GPU (bf16,
    last dimension a multiple of 16 up to 2048); ``emit_y=False`` skips writing y there and
    returns None for it (the consumer is an int8 linear alone)."""
    if _pkg()._use_native(x):
        if x.dtype != torch.bfloat16:
            raise TypeError(f"rms_norm_quant: GPU input must be bf16, got {x.dtype}")
        y, q, s = _pkg().require_native().rmsnorm_quant_rows(
            x.contiguous(), residual.contiguous() if residual is not None else None, gamma, float(eps), bool(emit_y))
        return y, (q, s)
    y, qs = ref.rms_norm_quant(x, gamma, eps, residual)
    return (y if emit_y else None), qs


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
