"""Inference-only BERT encoder / classifier with int8 linears (post-training dynamic
quantization: int8 weights with one fp32 scale per output channel, activations quantized per
token on every call; ``cloudtik_amd.ops.quant``).

Built from a trained ``BertClassifier``; the training modules (``models.bert.BertLayer``,
``ops.transformer``) are not involved.  Per layer a set ``int8_sites`` of
{"qkv", "out", "ffn1", "ffn2"} says which of the four linears run in int8; a site left out
keeps its original weight and runs ``F.linear``.  Embeddings, LayerNorms, attention, the
pooler and the classifier head stay in the model dtype.

State dict: the tensors of the float model under their own names, except that a quantized
site's ``<site>_weight`` is replaced by ``<site>_weight_q`` (int8) and ``<site>_weight_scale``
(fp32).

Static quantization (``act_amax`` given: per layer one calibrated fp32 range for the input of
each of the four sites, from ``calibrate``) replaces the per-token scales of an int8 site by that
constant, so the int8 activations are produced where the bf16 ones are: the LayerNorm in front
of ``qkv`` / ``ffn1`` and the bias + GELU epilogue of ``ffn1`` emit int8 next to / instead of
bf16, and only the attention context goes through a cast of its own.  A producer emits int8 only
when its consumer is an int8 site.  ``fuse=False`` runs the same arithmetic as separate kernels
(LayerNorm, then cast; bf16 GEMM, then cast); the two agree bit for bit.  The ranges are plain
Python floats (they reach the kernels by value) and are not part of the state dict.
"""
from __future__ import annotations

from typing import Dict, Iterable, List, Optional, Sequence

import torch
import torch.nn as nn
import torch.nn.functional as F

from cloudtik_amd import ops
from cloudtik_amd.models.bert import BertConfig
from cloudtik_amd.ops import quant

SITES = ("qkv", "out", "ffn1", "ffn2")


def _check_sites(sites: Iterable[str]) -> List[str]:
    sites = list(sites)
    bad = [s for s in sites if s not in SITES]
    if bad:
        raise ValueError(f"unknown int8 site(s) {bad}; choose from {list(SITES)}")
    return [s for s in SITES if s in sites]


def _check_amax(act_amax, what="act_amax") -> Optional[Dict[str, float]]:
    """One layer's ranges, as a {site: float} dict or four floats in ``SITES`` order."""
    if act_amax is None:
        return None
    if isinstance(act_amax, dict):
        act_amax = [act_amax[s] for s in SITES]
    vals = [float(v) for v in act_amax]
    if len(vals) != len(SITES):
        raise ValueError(f"{what}: expected one range for each of {list(SITES)}, got {len(vals)}")
    for v in vals:
        quant.ref.static_scales(v)                      # finite, non-negative, fp32
    return dict(zip(SITES, vals))


def _site_shapes(cfg: BertConfig):
    H, I = cfg.hidden_size, cfg.intermediate_size
    return {"qkv": (3 * H, H), "out": (H, H), "ffn1": (I, H), "ffn2": (H, I)}


class QuantBertLayer(nn.Module):
    """One post-LN encoder layer; every tensor is a buffer (nothing here trains)."""

    def __init__(self, cfg: BertConfig, int8_sites: Iterable[str] = SITES, device=None, dtype=torch.bfloat16,
                 act_amax=None, fuse: bool = True):
        super().__init__()
        self.cfg = cfg
        self.int8_sites = _check_sites(int8_sites)
        self.act_amax = _check_amax(act_amax)           # None: dynamic per-token scales
        self.fuse = bool(fuse)
        self._observer = None                           # calibrate(): called with (site, input)
        kw = dict(device=device, dtype=dtype)
        for site, (n, k) in _site_shapes(cfg).items():
            if site in self.int8_sites:
                self.register_buffer(f"{site}_weight_q", torch.zeros(n, k, device=device, dtype=torch.int8))
                self.register_buffer(f"{site}_weight_scale", torch.zeros(n, device=device, dtype=torch.float32))
            else:
                self.register_buffer(f"{site}_weight", torch.zeros(n, k, **kw))
            self.register_buffer(f"{site}_bias", torch.zeros(n, **kw))
        for ln in ("ln1", "ln2"):
            self.register_buffer(f"{ln}_weight", torch.ones(cfg.hidden_size, **kw))
            self.register_buffer(f"{ln}_bias", torch.zeros(cfg.hidden_size, **kw))

    @classmethod
    def from_float(cls, layer: nn.Module, int8_sites: Iterable[str] = SITES, act_amax=None,
                   fuse: bool = True) -> "QuantBertLayer":
        w = layer.qkv_weight
        q = cls(layer.cfg, int8_sites, device=w.device, dtype=w.dtype, act_amax=act_amax, fuse=fuse)
        for name, t in layer.state_dict().items():
            site = name[:-len("_weight")] if name.endswith("_weight") else None
            if site in q.int8_sites:
                wq, ws = quant.quantize_weight(t)
                getattr(q, f"{site}_weight_q").copy_(wq)
                getattr(q, f"{site}_weight_scale").copy_(ws)
            else:
                getattr(q, name).copy_(t)
        return q

    def _linear(self, site: str, x, bias=None, act=quant.ACT_NONE):
        if self._observer is not None:
            self._observer(site, x)
        if site in self.int8_sites:
            return quant.linear_i8(quant.quantize_rows(x), getattr(self, f"{site}_weight_q"),
                                   getattr(self, f"{site}_weight_scale"), bias, act, dtype=x.dtype)
        y = F.linear(x, getattr(self, f"{site}_weight"))
        if act == quant.ACT_GELU:
            return ops.bias_gelu(y, bias)
        return y if bias is None else y + bias

    # ------------------------------------------------------------------ static path
    def _emits(self, site: str) -> bool:
        """Whether the producer of ``site``'s input writes int8 (static ranges, an int8 site)."""
        return self.act_amax is not None and site in self.int8_sites

    def _cast(self, site: str, x):
        return quant.quantize_static(x, self.act_amax[site])

    def _norm(self, x, ln: str, bias, residual, amax: Optional[float]):
        """(y, q): the LayerNorm and, with a range, its int8 output -- one kernel (its int8 output
        switched off without a range) or the training LayerNorm's forward and a cast."""
        g, b, eps = getattr(self, f"{ln}_weight"), getattr(self, f"{ln}_bias"), self.cfg.layer_norm_eps
        if self.fuse:
            return quant.layer_norm_quant(x, g, b, eps, bias=bias, residual=residual, amax=amax)
        y = ops.layer_norm(x, g, b, eps, bias=bias, residual=residual, training=False)
        return y, (None if amax is None else quant.quantize_static(y, amax))

    def _linear_static(self, site: str, x_q, bias=None, act=quant.ACT_NONE, out_amax=None, dtype=None):
        w_q, w_s = getattr(self, f"{site}_weight_q"), getattr(self, f"{site}_weight_scale")
        if out_amax is not None and not self.fuse:
            y = quant.linear_i8_static(x_q, self.act_amax[site], w_q, w_s, bias, act, dtype=dtype)
            return quant.quantize_static(y, out_amax)
        return quant.linear_i8_static(x_q, self.act_amax[site], w_q, w_s, bias, act, out_amax, dtype=dtype)

    def _forward_static(self, x, key_bias, x_q, out_amax):
        cfg, dt = self.cfg, x.dtype
        if self._emits("qkv"):
            qkv = self._linear_static("qkv", self._cast("qkv", x) if x_q is None else x_q, self.qkv_bias, dtype=dt)
        else:
            qkv = self._linear("qkv", x, self.qkv_bias)
        ctx = ops.attention_packed(qkv, cfg.num_attention_heads, key_bias, p=0.0, training=False)
        a = self._linear_static("out", self._cast("out", ctx), dtype=dt) if self._emits("out") \
            else self._linear("out", ctx)
        x1, x1_q = self._norm(a, "ln1", self.out_bias, x, self.act_amax["ffn1"] if self._emits("ffn1") else None)
        to_ffn2 = self.act_amax["ffn2"] if self._emits("ffn2") else None
        if self._emits("ffn1"):     # int8 straight out of the bias + GELU epilogue when ffn2 takes int8
            h = self._linear_static("ffn1", x1_q, self.ffn1_bias, quant.ACT_GELU, to_ffn2, dtype=dt)
        else:
            h = self._linear("ffn1", x1, self.ffn1_bias, quant.ACT_GELU)
            if to_ffn2 is not None:
                h = self._cast("ffn2", h)
        f = self._linear_static("ffn2", h, dtype=dt) if self._emits("ffn2") else self._linear("ffn2", h)
        return self._norm(f, "ln2", self.ffn2_bias, x1, out_amax)

    @torch.no_grad()
    def forward(self, x, key_bias, x_q=None, out_amax: Optional[float] = None):
        """The layer's output.  Static ranges only: ``x_q`` is ``x`` already quantized against this
        layer's ``qkv`` range (by the producer of ``x``); with ``out_amax`` -- the next layer's
        ``qkv`` range -- the result is the pair (y, y_q)."""
        if self.act_amax is not None:
            y, y_q = self._forward_static(x, key_bias, x_q, out_amax)
            return y if out_amax is None else (y, y_q)
        if x_q is not None or out_amax is not None:
            raise ValueError("int8 inputs / outputs between layers need static ranges (act_amax)")
        cfg = self.cfg
        qkv = self._linear("qkv", x, self.qkv_bias)
        ctx = ops.attention_packed(qkv, cfg.num_attention_heads, key_bias, p=0.0, training=False)
        a = self._linear("out", ctx)
        x1 = ops.layer_norm(a, self.ln1_weight, self.ln1_bias, cfg.layer_norm_eps, bias=self.out_bias,
                            residual=x, training=False)
        h = self._linear("ffn1", x1, self.ffn1_bias, quant.ACT_GELU)
        f = self._linear("ffn2", h)
        return ops.layer_norm(f, self.ln2_weight, self.ln2_bias, cfg.layer_norm_eps, bias=self.ffn2_bias,
                              residual=x1, training=False)


class QuantBertModel(nn.Module):
    def __init__(self, cfg: BertConfig, sites_per_layer: Sequence[Iterable[str]], device=None, dtype=torch.bfloat16,
                 act_amax=None, fuse: bool = True):
        super().__init__()
        if len(sites_per_layer) != cfg.num_hidden_layers:
            raise ValueError("one int8 site set per encoder layer is required")
        if act_amax is not None and len(act_amax) != cfg.num_hidden_layers:
            raise ValueError("act_amax: one set of ranges per encoder layer is required")
        self.fuse = bool(fuse)
        self.cfg = cfg
        H = cfg.hidden_size
        kw = dict(device=device, dtype=dtype)
        self.register_buffer("word_embeddings", torch.zeros(cfg.padded_vocab, H, **kw))
        self.register_buffer("position_embeddings", torch.zeros(cfg.max_position_embeddings, H, **kw))
        self.register_buffer("token_type_embeddings", torch.zeros(cfg.type_vocab_size, H, **kw))
        self.register_buffer("emb_ln_weight", torch.ones(H, **kw))
        self.register_buffer("emb_ln_bias", torch.zeros(H, **kw))
        amax = act_amax if act_amax is not None else [None] * cfg.num_hidden_layers
        self.layers = nn.ModuleList([QuantBertLayer(cfg, s, act_amax=a, fuse=fuse, **kw)
                                     for s, a in zip(sites_per_layer, amax)])
        self.register_buffer("pooler_weight", torch.zeros(H, H, **kw))
        self.register_buffer("pooler_bias", torch.zeros(H, **kw))

    def _emb_norm(self, emb, amax: Optional[float]):
        eps = self.cfg.layer_norm_eps
        if self.fuse:
            return quant.layer_norm_quant(emb, self.emb_ln_weight, self.emb_ln_bias, eps, amax=amax)
        x = ops.layer_norm(emb, self.emb_ln_weight, self.emb_ln_bias, eps, training=False)
        return x, (None if amax is None else quant.quantize_static(x, amax))

    @torch.no_grad()
    def forward(self, input_ids, token_type_ids=None, attention_mask=None):
        cfg = self.cfg
        emb = ops.embedding3(input_ids, token_type_ids, self.word_embeddings, self.position_embeddings,
                             self.token_type_embeddings)
        key_bias = None
        if attention_mask is not None:
            key_bias = (1.0 - attention_mask.to(torch.float32)) * -10000.0
        if self.layers[0].act_amax is not None:
            # static ranges: whatever writes a layer's input also writes it as int8 for qkv
            ranges = [l.act_amax["qkv"] if l._emits("qkv") else None for l in self.layers] + [None]
            x, x_q = self._emb_norm(emb, ranges[0])
            for layer, nxt in zip(self.layers, ranges[1:]):
                x, x_q = layer._forward_static(x, key_bias, x_q, nxt)
        else:
            x = ops.layer_norm(emb, self.emb_ln_weight, self.emb_ln_bias, cfg.layer_norm_eps, training=False)
            for layer in self.layers:
                x = layer(x, key_bias)
        pooled = torch.tanh(F.linear(x[:, 0], self.pooler_weight, self.pooler_bias))
        return x, pooled


class QuantBertClassifier(nn.Module):
    """``BertClassifier`` for inference with int8 encoder linears; same call signature."""

    def __init__(self, cfg: BertConfig, num_classes: int, sites_per_layer: Optional[Sequence[Iterable[str]]] = None,
                 device=None, dtype=torch.bfloat16, act_amax=None, fuse: bool = True):
        super().__init__()
        if sites_per_layer is None:
            sites_per_layer = [SITES] * cfg.num_hidden_layers
        self.bert = QuantBertModel(cfg, sites_per_layer, device=device, dtype=dtype, act_amax=act_amax, fuse=fuse)
        self.classifier = nn.Linear(cfg.hidden_size, num_classes, device=device, dtype=dtype)
        self.classifier.requires_grad_(False)
        self.eval()

    @property
    def sites_per_layer(self) -> List[List[str]]:
        return [list(l.int8_sites) for l in self.bert.layers]

    @property
    def act_amax(self) -> Optional[List[List[float]]]:
        """The static ranges, [layers][4] in ``SITES`` order, or None for a dynamic model."""
        if self.bert.layers[0].act_amax is None:
            return None
        return [[l.act_amax[s] for s in SITES] for l in self.bert.layers]

    @classmethod
    def from_float(cls, model: nn.Module, int8_sites=SITES, act_amax=None, fuse: bool = True) -> "QuantBertClassifier":
        """Quantize a trained ``BertClassifier``.  ``int8_sites``: one site set for every layer,
        or a sequence with one set per layer.  ``act_amax`` (from ``calibrate``) selects static
        activation ranges, ``fuse`` the fused or the unfused kernels for them."""
        cfg = model.bert.cfg
        sites = list(int8_sites)
        if all(isinstance(s, str) for s in sites):
            sites = [sites] * cfg.num_hidden_layers
        w = model.classifier.weight
        q = cls(cfg, model.classifier.out_features, sites, device=w.device, dtype=w.dtype, act_amax=act_amax,
                fuse=fuse)
        q.classifier.load_state_dict(model.classifier.state_dict())
        for name, t in model.bert.state_dict().items():
            if not name.startswith("layers."):
                getattr(q.bert, name).copy_(t)
        amax = act_amax if act_amax is not None else [None] * cfg.num_hidden_layers
        q.bert.layers = nn.ModuleList([QuantBertLayer.from_float(l, s, a, fuse)
                                       for l, s, a in zip(model.bert.layers, sites, amax)])
        return q

    @torch.no_grad()
    def forward(self, input_ids, attention_mask=None, token_type_ids=None):
        _, pooled = self.bert(input_ids, token_type_ids, attention_mask)
        return self.classifier(pooled)


@torch.no_grad()
def calibrate(float_model: nn.Module, batches) -> List[List[float]]:
    """Activation ranges for static quantization: run the float model (its weights in this
    module's inference forward, no site in int8) over ``batches`` and return, per layer, the
    largest ``abs()`` seen at the input of each of ``SITES`` -- [layers][4] Python floats holding
    fp32 values.  A batch is a dict with ``input_ids`` / ``attention_mask`` (/ ``token_type_ids``)
    or a tuple ``(input_ids, attention_mask)``.  The running maxima stay on the device
    (``torch.maximum``) and are read back once, at the end."""
    m = QuantBertClassifier.from_float(float_model, ())
    dev = m.classifier.weight.device
    seen = torch.zeros(len(m.bert.layers), len(SITES), device=dev, dtype=torch.float32)

    def observer(i):
        def note(site, x):
            k = SITES.index(site)
            seen[i, k] = torch.maximum(seen[i, k], x.abs().amax().float())
        return note

    for i, layer in enumerate(m.bert.layers):
        layer._observer = observer(i)
    n = 0
    for b in batches:
        if isinstance(b, dict):
            ids, mask, tt = b["input_ids"], b.get("attention_mask"), b.get("token_type_ids")
        else:
            ids, mask, tt = b[0], (b[1] if len(b) > 1 else None), None
        to = lambda t: None if t is None else t.to(dev)
        m(to(ids), to(mask), to(tt))
        n += 1
    if n == 0:
        raise ValueError("calibrate: no batches")
    return seen.cpu().tolist()
