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
"""
from __future__ import annotations

from typing import Iterable, List, Optional, Sequence

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


def _site_shapes(cfg: BertConfig):
    H, I = cfg.hidden_size, cfg.intermediate_size
    return {"qkv": (3 * H, H), "out": (H, H), "ffn1": (I, H), "ffn2": (H, I)}


class QuantBertLayer(nn.Module):
    """One post-LN encoder layer; every tensor is a buffer (nothing here trains)."""

    def __init__(self, cfg: BertConfig, int8_sites: Iterable[str] = SITES, device=None, dtype=torch.bfloat16):
        super().__init__()
        self.cfg = cfg
        self.int8_sites = _check_sites(int8_sites)
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
    def from_float(cls, layer: nn.Module, int8_sites: Iterable[str] = SITES) -> "QuantBertLayer":
        w = layer.qkv_weight
        q = cls(layer.cfg, int8_sites, device=w.device, dtype=w.dtype)
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
        if site in self.int8_sites:
            return quant.linear_i8(quant.quantize_rows(x), getattr(self, f"{site}_weight_q"),
                                   getattr(self, f"{site}_weight_scale"), bias, act, dtype=x.dtype)
        y = F.linear(x, getattr(self, f"{site}_weight"))
        if act == quant.ACT_GELU:
            return ops.bias_gelu(y, bias)
        return y if bias is None else y + bias

    @torch.no_grad()
    def forward(self, x, key_bias):
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
    def __init__(self, cfg: BertConfig, sites_per_layer: Sequence[Iterable[str]], device=None, dtype=torch.bfloat16):
        super().__init__()
        if len(sites_per_layer) != cfg.num_hidden_layers:
            raise ValueError("one int8 site set per encoder layer is required")
        self.cfg = cfg
        H = cfg.hidden_size
        kw = dict(device=device, dtype=dtype)
        self.register_buffer("word_embeddings", torch.zeros(cfg.padded_vocab, H, **kw))
        self.register_buffer("position_embeddings", torch.zeros(cfg.max_position_embeddings, H, **kw))
        self.register_buffer("token_type_embeddings", torch.zeros(cfg.type_vocab_size, H, **kw))
        self.register_buffer("emb_ln_weight", torch.ones(H, **kw))
        self.register_buffer("emb_ln_bias", torch.zeros(H, **kw))
        self.layers = nn.ModuleList([QuantBertLayer(cfg, s, **kw) for s in sites_per_layer])
        self.register_buffer("pooler_weight", torch.zeros(H, H, **kw))
        self.register_buffer("pooler_bias", torch.zeros(H, **kw))

    @torch.no_grad()
    def forward(self, input_ids, token_type_ids=None, attention_mask=None):
        cfg = self.cfg
        emb = ops.embedding3(input_ids, token_type_ids, self.word_embeddings, self.position_embeddings,
                             self.token_type_embeddings)
        x = ops.layer_norm(emb, self.emb_ln_weight, self.emb_ln_bias, cfg.layer_norm_eps, training=False)
        key_bias = None
        if attention_mask is not None:
            key_bias = (1.0 - attention_mask.to(torch.float32)) * -10000.0
        for layer in self.layers:
            x = layer(x, key_bias)
        pooled = torch.tanh(F.linear(x[:, 0], self.pooler_weight, self.pooler_bias))
        return x, pooled


class QuantBertClassifier(nn.Module):
    """``BertClassifier`` for inference with int8 encoder linears; same call signature."""

    def __init__(self, cfg: BertConfig, num_classes: int, sites_per_layer: Optional[Sequence[Iterable[str]]] = None,
                 device=None, dtype=torch.bfloat16):
        super().__init__()
        if sites_per_layer is None:
            sites_per_layer = [SITES] * cfg.num_hidden_layers
        self.bert = QuantBertModel(cfg, sites_per_layer, device=device, dtype=dtype)
        self.classifier = nn.Linear(cfg.hidden_size, num_classes, device=device, dtype=dtype)
        self.classifier.requires_grad_(False)
        self.eval()

    @property
    def sites_per_layer(self) -> List[List[str]]:
        return [list(l.int8_sites) for l in self.bert.layers]

    @classmethod
    def from_float(cls, model: nn.Module, int8_sites=SITES) -> "QuantBertClassifier":
        """Quantize a trained ``BertClassifier``.  ``int8_sites``: one site set for every layer,
        or a sequence with one set per layer."""
        cfg = model.bert.cfg
        sites = list(int8_sites)
        if all(isinstance(s, str) for s in sites):
            sites = [sites] * cfg.num_hidden_layers
        w = model.classifier.weight
        q = cls(cfg, model.classifier.out_features, sites, device=w.device, dtype=w.dtype)
        q.classifier.load_state_dict(model.classifier.state_dict())
        for name, t in model.bert.state_dict().items():
            if not name.startswith("layers."):
                getattr(q.bert, name).copy_(t)
        q.bert.layers = nn.ModuleList([QuantBertLayer.from_float(l, s) for l, s in zip(model.bert.layers, sites)])
        return q

    @torch.no_grad()
    def forward(self, input_ids, attention_mask=None, token_type_ids=None):
        _, pooled = self.bert(input_ids, token_type_ids, attention_mask)
        return self.classifier(pooled)
