"""Inference-only T5 with int8 linears (post-training dynamic quantization; the reference
workload's ``PRECISION=int8``, which runs ``torch.quantization.quantize_dynamic`` over every
``nn.Linear`` of ``T5ForConditionalGeneration``, the output head included).

Number format (``cloudtik_amd.ops.quant``): symmetric int8, weights with one fp32 scale per output
channel computed once, activations with one per row (token) computed on every call, exact int32
accumulation.  That is this project's format, not torch's per-tensor affine one, so the tokens of
the reference's int8 model are not reproduced bit for bit.

What is quantized: every linear of both stacks and the output head (an int8 copy of the tied
embedding with the d_model^-0.5 folded into its channel scales; of ``lm_head`` with factor 1 for the
untied unscaled head of T5 v1.1).  The embedding lookup table, the
norms' weights, the relative-bias table and attention stay in the model dtype.  ``q`` / ``k`` /
``v`` of self-attention are one stacked [3 inner, d_model] weight and ``wi_0`` / ``wi_1`` of the gated
feed-forward one [2 d_ff, d_model] weight; the per-matrix modules the float code calls (``sa.q``,
``ff.wi_1``, ..) are row slices of the stack and give the same bits.

The module path (block ``forward``, the encoder, the eager loops, the CPU) runs the float model's
code on those modules.  The graph-captured decode step of all three generation modes
(``_decode_step_static``, ``logits``) runs fused: every norm emits the int8 operand of the linear
behind it (``ops.rms_norm_quant``), QKV is one GEMM, ``o`` / cross ``o`` / ``wo`` carry the residual add
and ``wi`` the ReLU in their epilogues, and the head takes the final norm's int8 output directly: 16
launches per decoder layer where the bf16 step has 19 (``profiles/t5_quant/SUMMARY.md``).  Both
paths give the same bits.

State dict: ``shared.weight``, the norms and the relative-bias tables under the float model's
names; per linear ``<name>.w_q`` (int8) and ``<name>.w_scale`` (fp32), the stacks as ``sa.qkv`` and
``ff.wi_stack``, the head as ``head``.
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn

from cloudtik_amd import ops
from cloudtik_amd.models.t5 import T5Config, T5ForConditionalGeneration, T5Norm, relative_position_bucket
from cloudtik_amd.ops import quant


class QuantLinear(nn.Module):
    """A bias-free int8 linear: ``w_q`` int8 [N, K], ``w_scale`` fp32 [N]."""

    def __init__(self, in_features: int, out_features: int, device=None):
        super().__init__()
        self.in_features, self.out_features = in_features, out_features
        self.register_buffer("w_q", torch.zeros(out_features, in_features, device=device, dtype=torch.int8))
        self.register_buffer("w_scale", torch.zeros(out_features, device=device, dtype=torch.float32))

    @torch.no_grad()
    def load_weight(self, w: torch.Tensor, scale_factor: Optional[float] = None):
        """Quantize the float weight ``w`` [N, K] into this module; ``scale_factor`` is folded into
        the channel scales (one fp32 multiply)."""
        wq, ws = quant.quantize_weight(w)
        if scale_factor is not None:
            ws = ws * scale_factor
        self.w_q.copy_(wq)
        self.w_scale.copy_(ws)
        return self

    def forward(self, x, act: int = quant.ACT_NONE, residual=None, out=None, dtype=None):
        """``x``: a floating tensor or the ``(q, scale)`` pair a fused norm produced."""
        return quant.linear_i8(x, self.w_q, self.w_scale, None, act, dtype=dtype, residual=residual, out=out)

    def extra_repr(self):
        return f"in_features={self.in_features}, out_features={self.out_features}, int8"


class QuantLinearSlice(nn.Module):
    """Output channels [lo, hi) of a stacked ``QuantLinear`` as a linear of its own: no tensors
    of its own (the parent is held unregistered), the same bits as a separate int8 linear over
    those rows, because an output channel depends on its own weight row and scale alone."""

    def __init__(self, parent: QuantLinear, lo: int, hi: int):
        super().__init__()
        self._parent = (parent,)
        self.lo, self.hi = lo, hi

    def forward(self, x):
        p = self._parent[0]
        return quant.linear_i8(x, p.w_q[self.lo:self.hi], p.w_scale[self.lo:self.hi])


class RowQuantized:
    """Hidden states that exist only as int8 rows and their scales (the fused final norm's
    output); indexing applies to both, so ``x[:, -1]`` works as on the float tensor."""

    def __init__(self, q: torch.Tensor, scale: torch.Tensor):
        self.q, self.scale = q, scale

    def __getitem__(self, idx):
        return RowQuantized(self.q[idx], self.scale[idx])


class QuantT5ForConditionalGeneration(T5ForConditionalGeneration):
    """``T5ForConditionalGeneration`` for inference with int8 linears; ``generate`` is inherited
    unchanged.  ``QuantT5ForConditionalGeneration(cfg)`` is a skeleton for ``load_state_dict``;
    ``from_float`` (or ``T5ForConditionalGeneration.quantize_dynamic``) quantizes a float model."""

    def __init__(self, cfg: T5Config = None, device=None, dtype=torch.bfloat16):
        # the float structure without storage, then int8 linears in place of its nn.Linear and
        # real tensors for what stays in the model dtype
        super().__init__(cfg, device="meta", dtype=dtype)
        cfg = self.cfg
        inner = cfg.num_heads * cfg.d_kv
        for stack in (self.encoder, self.decoder):
            for blk in stack.blocks:
                a = blk.sa
                a.qkv = QuantLinear(cfg.d_model, 3 * inner, device)
                a.q, a.k, a.v = (QuantLinearSlice(a.qkv, j * inner, (j + 1) * inner) for j in range(3))
                a.o = QuantLinear(inner, cfg.d_model, device)
                if blk.decoder:
                    c = blk.ca
                    c.q, c.k, c.v = (QuantLinear(cfg.d_model, inner, device) for _ in range(3))
                    c.o = QuantLinear(inner, cfg.d_model, device)
                ff = blk.ff
                if ff.gated:
                    ff.wi_stack = QuantLinear(cfg.d_model, 2 * cfg.d_ff, device)
                    ff.wi = QuantLinearSlice(ff.wi_stack, 0, cfg.d_ff)
                    ff.wi_1 = QuantLinearSlice(ff.wi_stack, cfg.d_ff, 2 * cfg.d_ff)
                else:
                    ff.wi = QuantLinear(cfg.d_model, cfg.d_ff, device)
                ff.wo = QuantLinear(cfg.d_ff, cfg.d_model, device)
        self.head = QuantLinear(cfg.d_model, cfg.vocab_size, device)
        if not cfg.tie_word_embeddings:
            del self.lm_head                   # the untied float head lives on as `head` alone
        for m in self.modules():
            for name, p in list(m._parameters.items()):
                if p is not None and p.is_meta:
                    fill = torch.ones if isinstance(m, T5Norm) else torch.zeros
                    m._parameters[name] = nn.Parameter(fill(p.shape, device=device, dtype=p.dtype), requires_grad=False)
        super().train(False)

    # ------------------------------------------------------------------------- construction
    @classmethod
    @torch.no_grad()
    def from_float(cls, model: T5ForConditionalGeneration) -> "QuantT5ForConditionalGeneration":
        """Quantize a float model: weights are quantized per output channel on the host, everything
        else is copied; the result lives on the model's device in its dtype."""
        w = model.shared.weight
        q = cls(model.cfg, device=w.device, dtype=model.dtype)
        q.shared.weight.copy_(w)
        q.head.load_weight(model.head_weight(), model.cfg.d_model ** -0.5 if model.cfg.scales_outputs else None)
        for qs, fs in ((q.encoder, model.encoder), (q.decoder, model.decoder)):
            qs.final.weight.copy_(fs.final.weight)
            for qb, fb in zip(qs.blocks, fs.blocks):
                qb.ln_sa.weight.copy_(fb.ln_sa.weight)
                qb.ln_ff.weight.copy_(fb.ln_ff.weight)
                if fb.sa.rel is not None:
                    qb.sa.rel.weight.copy_(fb.sa.rel.weight)
                qb.sa.qkv.load_weight(torch.cat([fb.sa.q.weight, fb.sa.k.weight, fb.sa.v.weight], 0))
                qb.sa.o.load_weight(fb.sa.o.weight)
                if fb.decoder:
                    qb.ln_ca.weight.copy_(fb.ln_ca.weight)
                    for name in "qkvo":
                        getattr(qb.ca, name).load_weight(getattr(fb.ca, name).weight)
                if fb.ff.gated:
                    qb.ff.wi_stack.load_weight(torch.cat([fb.ff.wi.weight, fb.ff.wi_1.weight], 0))
                else:
                    qb.ff.wi.load_weight(fb.ff.wi.weight)
                qb.ff.wo.load_weight(fb.ff.wo.weight)
        return q

    def train(self, mode: bool = True):
        if mode:
            raise RuntimeError("QuantT5ForConditionalGeneration is inference-only: it has no training mode")
        return super().train(False)

    def forward(self, *args, **kwargs):
        raise RuntimeError("QuantT5ForConditionalGeneration is inference-only: train the float model and "
                           "quantize it (T5ForConditionalGeneration.quantize_dynamic)")

    def quantize_dynamic(self):
        return self

    def load_hf_state_dict(self, state_dict):
        raise RuntimeError("load the checkpoint into the float model and quantize that (quantize_dynamic)")

    # ------------------------------------------------------------------------------ the head
    def logits(self, dec):
        """[..., vocab] from the final norm's output, a tensor or the fused norm's int8 rows; the
        d_model^-0.5 of a scaled head lives in the head's channel scales."""
        if isinstance(dec, RowQuantized):
            return self.head((dec.q, dec.scale), dtype=self.dtype)
        return self.head(dec)

    # ---------------------------------------------------------------------- the fused step
    def _decode_step_static(self, cur, pos, slots, kc, vc, cross, enc_bias):
        """The float model's static decode step with every linear fused with its neighbours: per
        layer three norm + quantize kernels, the stacked QKV GEMM, and ``o`` / cross ``o`` / ``wo`` with
        the residual add (``wi`` with the ReLU) in their epilogues.  Returns the final norm's output
        as ``RowQuantized`` [B, 1, d_model] for ``logits``.  The same bits as the module path."""
        cfg, dec, dt = self.cfg, self.decoder, self.dtype
        B, T = cur.shape[0], slots.shape[0]
        inner = cfg.num_heads * cfg.d_kv
        x = dec.embed(cur)
        inplace = x.is_cuda                                  # x is this step's own tensor
        bucket = relative_position_bucket(slots - pos, False, cfg.relative_attention_num_buckets,
                                          cfg.relative_attention_max_distance)
        relvec = dec.blocks[0].sa.rel(bucket).t().float().contiguous()     # query at `pos`, keys 0..T-1
        key_bias = torch.where(slots <= pos, 0.0, -1e9).float()[None].expand(B, T).contiguous()

        def add_into(lin, h, x):                             # x + lin(h), the add in the GEMM's epilogue
            return lin(h, residual=x, out=x if inplace else None, dtype=dt)

        for i, blk in enumerate(dec.blocks):
            a, c, ff = blk.sa, blk.ca, blk.ff
            _, h = quant.rms_norm_quant(x, blk.ln_sa.weight, blk.ln_sa.eps, emit_y=False)
            q, k, v = (a._split(t) for t in a.qkv(h, dtype=dt).split(inner, -1))
            kc[i].index_copy_(1, pos, k)
            vc[i].index_copy_(1, pos, v)
            o = ops.attention_relbias(q, kc[i], vc[i], relvec, 0, key_bias, scale=1.0, causal=False)
            x = add_into(a.o, o.reshape(B, 1, -1), x)
            _, h = quant.rms_norm_quant(x, blk.ln_ca.weight, blk.ln_ca.eps, emit_y=False)
            q = c._split(c.q(h, dtype=dt))
            o = ops.attention(q.transpose(1, 2), cross[i][0].transpose(1, 2), cross[i][1].transpose(1, 2),
                              key_bias=enc_bias, scale=1.0).transpose(1, 2)
            x = add_into(c.o, o.reshape(B, 1, -1), x)
            _, h = quant.rms_norm_quant(x, blk.ln_ff.weight, blk.ln_ff.eps, emit_y=False)
            if ff.gated:
                g, u = ff.wi_stack(h, dtype=dt).split(cfg.d_ff, -1)
                h = ff.gate(g, u)
            else:
                h = ff.wi(h, act=quant.ACT_RELU, dtype=dt)
            x = add_into(ff.wo, h, x)
        _, (q, s) = quant.rms_norm_quant(x, dec.final.weight, dec.final.eps, emit_y=False)
        return RowQuantized(q, s)
