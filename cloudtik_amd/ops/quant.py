"""Int8 post-training quantization ops (inference only): dynamic per-row activation
quantization and the int8 linear on the i8 matrix cores (csrc/quant.hip).

Number format: symmetric int8, no zero point; activations get one fp32 scale per row (token),
computed per call, weights one per output channel, computed once offline.  The rounding rule
is fixed (``reference.quantize_rows``), so the GPU kernel and the CPU reference agree bit for
bit on the quantized tensors, and the int32 accumulation is exact on both.

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
