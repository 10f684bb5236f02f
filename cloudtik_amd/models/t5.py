"""T5 encoder-decoder: the v1.0 checkpoints (t5-small / base / large / 3b / 11b; 3b and 11b have
d_kv = 128) and T5 v1.1 / Flan-T5 (``T5Config.v1_1``: small .. xxl, gated-GELU feed-forward, untied
output head).

Reference workload: the quickstart T5 inference (applications/ai/quickstart, HF
``T5ForConditionalGeneration``).  Random-init weights or a local HF
checkpoint directory (``from_pretrained``; or ``from_hf_config`` + ``load_hf_state_dict``), same
architecture: pre-norm blocks with RMS LayerNorm (no mean, no bias), un-scaled attention with a
learned bucketed relative-position bias shared by all layers of a stack, ReLU (v1.0) or gated-GELU
(v1.1) feed-forward, and an output head that is either the input embedding scaled by d_model^-0.5
(v1.0, ``tie_word_embeddings``) or a matrix of its own applied unscaled (v1.1, ``lm_head``).

MI355X mapping: RMS norms run in the HIP LayerNorm kernel (``rms=True``); the relative
position bias is carried as one [H, Sq + Sk - 1] vector per stack (bias depends only on
key - query) and added inside the MFMA flash-attention kernel (``ops.attention_relbias``),
so neither inference nor d_kv-64 training materialises an [H, Sq, Sk] bias: the kernels'
backward returns the gradient of that vector (not bitwise reproducible: fp32 LDS adds) and both
directions take attention dropout, at d_kv 64 and 128 alike; cross-attention uses the MFMA kernel
with the per-key padding mask; the gated-GELU feed-forward runs ``gelu_tanh(wi_0 x) * wi_1 x`` and its
dropout as one kernel forward and one backward (``ops.gated_gelu``, ``csrc/gated_act.hip``: only the two
GEMM outputs are kept for the backward; ``CLOUDTIK_AMD_T5_FUSED_FF=0`` restores the PyTorch
composition); the training loss is the fused linear + cross-entropy HIP kernel over the
32128-token vocabulary, on ``lm_head`` when the head is untied; generation keeps a per-layer KV
cache and replays the decode step as a HIP graph, greedy, with beam search (``ops/beam.py``, ``csrc/beam.hip``) or
sampling (``ops/sampling.py``, ``csrc/sampling.hip``), each with the history-dependent token bans of
``no_repeat_ngram_size``, ``min_length`` and ``bad_words_ids`` (``ops/constrain.py``,
``csrc/constrain.hip``).
"""
from __future__ import annotations

import logging
import math
import os
from dataclasses import dataclass
from typing import List, Optional, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from cloudtik_amd import ops
from cloudtik_amd.ops import beam as beam_ops
from cloudtik_amd.ops import constrain as constrain_ops
from cloudtik_amd.ops import sampling as sample_ops

logger = logging.getLogger(__name__)

@dataclass
class T5Config:
    vocab_size: int = 32128
    d_model: int = 768
    d_kv: int = 64
    d_ff: int = 3072
    num_layers: int = 12
    num_decoder_layers: int = 12
    num_heads: int = 12
    relative_attention_num_buckets: int = 32
    relative_attention_max_distance: int = 128
    dropout_rate: float = 0.1
    layer_norm_epsilon: float = 1e-6
    gated_gelu: bool = False          # T5 v1.1 feed-forward
    pad_token_id: int = 0
    decoder_start_token_id: int = 0
    eos_token_id: int = 1
    tie_word_embeddings: bool = True  # False: an output head of its own, ``lm_head`` (T5 v1.1)
    scale_decoder_outputs: Optional[bool] = None   # d_model^-0.5 before the head; None: as tie_word_embeddings

    @property
    def scales_outputs(self) -> bool:
        return self.tie_word_embeddings if self.scale_decoder_outputs is None else bool(self.scale_decoder_outputs)

    @classmethod
    def small(cls, **kw):
        return cls(d_model=512, d_ff=2048, num_layers=6, num_decoder_layers=6, num_heads=8, **kw)

    @classmethod
    def base(cls, **kw):
        return cls(**kw)

    @classmethod
    def large(cls, **kw):
        return cls(d_model=1024, d_ff=4096, num_layers=24, num_decoder_layers=24, num_heads=16, **kw)

    @classmethod
    def xl(cls, **kw):
        """t5-3b."""
        return cls(d_model=1024, d_kv=128, d_ff=16384, num_layers=24, num_decoder_layers=24, num_heads=32, **kw)

    @classmethod
    def xxl(cls, **kw):
        """t5-11b."""
        return cls(d_model=1024, d_kv=128, d_ff=65536, num_layers=24, num_decoder_layers=24, num_heads=128, **kw)

    @classmethod
    def v1_1(cls, size: str, **kw):
        """T5 v1.1 / Flan-T5 ``small`` .. ``xxl``: gated-GELU feed-forward, untied unscaled head."""
        if size not in _V1_1_SIZES:
            raise ValueError(f"unknown T5 v1.1 size {size!r} (known: {', '.join(_V1_1_SIZES)})")
        d_model, d_ff, layers, heads = _V1_1_SIZES[size]
        base = dict(d_model=d_model, d_kv=64, d_ff=d_ff, num_layers=layers, num_decoder_layers=layers, num_heads=heads,
                    gated_gelu=True, tie_word_embeddings=False)
        base.update(kw)
        return cls(**base)

    @classmethod
    def tiny(cls, **kw):
        base = dict(vocab_size=64, d_model=32, d_kv=8, d_ff=64, num_layers=2, num_decoder_layers=2, num_heads=4,
                    relative_attention_num_buckets=8, relative_attention_max_distance=16, dropout_rate=0.0)
        base.update(kw)
        return cls(**base)


# T5 v1.1 / Flan-T5: (d_model, d_ff, layers per stack, heads); d_kv is 64 throughout
_V1_1_SIZES = {"small": (512, 1024, 8, 6), "base": (768, 2048, 12, 12), "large": (1024, 2816, 24, 16),
               "xl": (2048, 5120, 24, 32), "xxl": (4096, 10240, 24, 64)}

_TASK_PASS_THROUGH = ("min_length", "no_repeat_ngram_size", "num_beams", "length_penalty", "early_stopping")


def generate_kwargs_for_task(config, task: str):
    """The generation settings a HF T5 config ships for ``task`` (``task_specific_params[task]``, such as
    "summarization"), as ``(kwargs, prefix)``: keyword arguments of ``T5ForConditionalGeneration.generate``
    and the text the task puts in front of its source.  ``config`` is a config of the library, a
    dict, or the path of a local ``config.json``.  ``max_length`` counts the start token, so it
    becomes ``max_new_tokens = max_length - 1``; ``min_length``, ``no_repeat_ngram_size``,
    ``num_beams``, ``length_penalty`` and ``early_stopping`` pass through; a setting ``generate``
    does not have raises ValueError."""
    if isinstance(config, (str, os.PathLike)):
        import json
        with open(config) as f:
            config = json.load(f)
    elif not isinstance(config, dict):
        config = config.to_dict()
    tasks = config.get("task_specific_params") or {}
    if task not in tasks:
        raise KeyError(f"the config has no task_specific_params[{task!r}] (it has {sorted(tasks)})")
    kwargs, prefix = {}, ""
    for name, value in tasks[task].items():
        if name == "prefix":
            prefix = value
        elif name == "max_length":
            kwargs["max_new_tokens"] = int(value) - 1
        elif name in _TASK_PASS_THROUGH:
            kwargs[name] = value
        else:
            raise ValueError(f"task_specific_params[{task!r}] sets {name!r}, which generate does not support")
    return kwargs, prefix


def _read_checkpoint(path: str):
    """The state dict of a local HF checkpoint directory, single file or sharded."""
    import json

    def load(name):
        f = os.path.join(path, name)
        if name.endswith(".safetensors"):
            from safetensors.torch import load_file
            return load_file(f)
        return torch.load(f, map_location="cpu", weights_only=True)

    for single, index in (("model.safetensors", "model.safetensors.index.json"),
                          ("pytorch_model.bin", "pytorch_model.bin.index.json")):
        if os.path.exists(os.path.join(path, single)):
            return load(single)
        if os.path.exists(os.path.join(path, index)):
            with open(os.path.join(path, index)) as f:
                weight_map = json.load(f)["weight_map"]
            sd = {}
            for shard in sorted(set(weight_map.values())):
                if os.path.basename(shard) != shard:
                    raise ValueError(f"{index} names a shard outside the checkpoint directory: {shard!r}")
                part = load(shard)
                sd.update({k: v for k, v in part.items() if weight_map.get(k) == shard})
            missing = sorted(set(weight_map) - set(sd))
            if missing:
                raise KeyError(f"{index} lists tensors its shards do not hold: {missing}")
            return sd
    raise FileNotFoundError(f"no model.safetensors, pytorch_model.bin or sharded index in {path!r}")


def relative_position_bucket(rel: torch.Tensor, bidirectional: bool, num_buckets: int, max_distance: int):
    """T5 bucketing of (key - query) offsets: exact buckets for small offsets, log-spaced
    buckets up to ``max_distance``, one shared bucket beyond."""
    ret = torch.zeros_like(rel)
    if bidirectional:
        num_buckets //= 2
        ret = ret + (rel > 0).long() * num_buckets
        n = rel.abs()
    else:
        n = (-rel).clamp(min=0)
    max_exact = num_buckets // 2
    small = n < max_exact
    large = max_exact + (torch.log(n.float().clamp(min=1) / max_exact) / math.log(max_distance / max_exact)
                         * (num_buckets - max_exact)).long()
    large = large.clamp(max=num_buckets - 1)
    return ret + torch.where(small, n, large)


def train_attention_kernels() -> bool:
    """Whether d_kv 64 / 128 attention takes the HIP kernels in grad mode and under dropout (default);
    ``CLOUDTIK_AMD_T5_TRAIN_ATTN=0`` keeps those calls on ``F.scaled_dot_product_attention`` with
    a materialised bias, the earlier routing (the A/B switch of bench/t5_train_probe.py)."""
    return os.environ.get("CLOUDTIK_AMD_T5_TRAIN_ATTN", "1") != "0"


def fused_ff_kernels() -> bool:
    """Whether the gated-GELU feed-forward takes ``ops.gated_gelu`` on the GPU in bf16 (default);
    ``CLOUDTIK_AMD_T5_FUSED_FF=0`` keeps the PyTorch composition, the earlier routing (the A/B switch
    of bench/t5_ff_probe.py).  Read per call."""
    return os.environ.get("CLOUDTIK_AMD_T5_FUSED_FF", "1") != "0"


class T5Norm(nn.Module):
    def __init__(self, d, eps, device=None, dtype=None):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(d, device=device, dtype=dtype))
        self.eps = eps

    def forward(self, x, residual=None):
        return ops.layer_norm(x, self.weight, None, eps=self.eps, residual=residual, rms=True)


class T5Attention(nn.Module):
    def __init__(self, cfg: T5Config, relative_bias: bool, causal: bool, device=None, dtype=None):
        super().__init__()
        inner = cfg.num_heads * cfg.d_kv
        kw = dict(bias=False, device=device, dtype=dtype)
        self.q, self.k, self.v = nn.Linear(cfg.d_model, inner, **kw), nn.Linear(cfg.d_model, inner, **kw), \
            nn.Linear(cfg.d_model, inner, **kw)
        self.o = nn.Linear(inner, cfg.d_model, **kw)
        self.h, self.dk = cfg.num_heads, cfg.d_kv
        self.causal = causal
        self.cfg = cfg
        self.rel = nn.Embedding(cfg.relative_attention_num_buckets, cfg.num_heads, device=device, dtype=dtype) \
            if relative_bias else None

    def relative_vector(self, sq: int, sk: int, device, offset: int = 0):
        """Per-head bias for every (key - query) offset: ``relvec [H, sq + sk - 1]`` with
        ``score(q, k) += relvec[h, k - q + rel_base]``, ``rel_base = sq - 1``; query
        positions start at ``offset`` (decoding with a KV cache)."""
        rel_base = sq - 1
        rel = torch.arange(sq + sk - 1, device=device) - rel_base - offset
        bucket = relative_position_bucket(rel, not self.causal, self.cfg.relative_attention_num_buckets,
                                          self.cfg.relative_attention_max_distance)
        return self.rel(bucket).t().float(), rel_base

    @staticmethod
    def full_bias(relvec, rel_base, sq, sk, causal_offset=None, key_bias=None):
        """Materialised [B|1, H, sq, sk] additive bias (the SDPA path)."""
        dev = relvec.device
        idx = torch.arange(sk, device=dev)[None, :] - torch.arange(sq, device=dev)[:, None] + rel_base
        bias = relvec[:, idx][None]
        if causal_offset is not None:
            allowed = torch.ones(sq, sk, dtype=torch.bool, device=dev).tril(causal_offset)
            bias = bias.masked_fill(~allowed, float("-inf"))
        if key_bias is not None:
            bias = bias + key_bias[:, None, None, :]
        return bias

    def _split(self, x):
        B, S, _ = x.shape
        return x.view(B, S, self.h, self.dk)

    def forward(self, x, kv=None, rel=None, key_bias=None, cache=None, offset: int = 0):
        """``kv``: encoder states for cross-attention; ``rel``: (relvec, rel_base) of the stack;
        ``key_bias`` [B, Sk] additive key mask; ``cache``: (k, v) of earlier decoder steps."""
        from cloudtik_amd import ops
        B, S, _ = x.shape
        q = self._split(self.q(x))                                    # [B, S, H, D]
        src = x if kv is None else kv
        if kv is not None and cache is not None:
            k, v = cache                                              # cross-attention K/V computed once
        else:
            k, v = self._split(self.k(src)), self._split(self.v(src))
            if cache is not None:
                k, v = torch.cat([cache[0], k], 1), torch.cat([cache[1], v], 1)
        Sk = k.shape[1]
        grad = torch.is_grad_enabled() and self.training
        kernel_ok = q.is_cuda and q.dtype == torch.bfloat16 and self.dk in (64, 128)
        # causal masking in the kernel is top-left aligned: exact for prefill (offset 0) and for
        # single-token decode steps (every cached key is visible)
        causal = self.causal and S > 1
        # d_kv 64 and 128 train on the kernels: self-attention with the bias gradient and dropout
        # (ops.attention_relbias), cross-attention with dropout (ops.attention at d_kv 64,
        # ops.attention_relbias(rel_bias=None) at 128, where ops.attention has no training kernels).
        # CLOUDTIK_AMD_T5_TRAIN_ATTN=0 sends grad-mode and dropout calls back to SDPA below.
        train_kernels = train_attention_kernels()
        needs_grad = torch.is_grad_enabled() and (q.requires_grad or k.requires_grad or v.requires_grad)
        if self.dk == 128 and not train_kernels and needs_grad:
            kernel_ok = False
        p = self.cfg.dropout_rate if (self.training and train_kernels) else 0.0
        if rel is not None and kernel_ok and (train_kernels or not grad) and (offset == 0 or not causal):
            relvec, rel_base = rel
            o = ops.attention_relbias(q, k, v, relvec, rel_base, key_bias, scale=1.0, causal=causal, p=p)
        elif rel is None and kernel_ok and (train_kernels or not (self.training and self.cfg.dropout_rate)):
            if self.dk == 128 and (needs_grad or p > 0):
                o = ops.attention_relbias(q, k, v, None, 0, key_bias, scale=1.0, causal=causal, p=p)
            else:
                o = ops.attention(q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2), key_bias=key_bias, p=p,
                                  scale=1.0, causal=causal).transpose(1, 2)      # T5 folds the scale into init
        else:
            bias = None
            if rel is not None:
                bias = self.full_bias(rel[0], rel[1], S, Sk, offset if causal else None, key_bias)
            elif key_bias is not None:
                bias = key_bias[:, None, None, :]
            o = F.scaled_dot_product_attention(
                q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2),
                attn_mask=bias.to(q.dtype) if bias is not None else None,
                dropout_p=self.cfg.dropout_rate if self.training else 0.0,
                is_causal=causal and bias is None, scale=1.0).transpose(1, 2)
        return self.o(o.reshape(B, S, -1)), (k, v)


class T5FF(nn.Module):
    def __init__(self, cfg: T5Config, device=None, dtype=None):
        super().__init__()
        kw = dict(bias=False, device=device, dtype=dtype)
        self.gated = cfg.gated_gelu
        self.wi = nn.Linear(cfg.d_model, cfg.d_ff, **kw)
        if self.gated:
            self.wi_1 = nn.Linear(cfg.d_model, cfg.d_ff, **kw)
        self.wo = nn.Linear(cfg.d_ff, cfg.d_model, **kw)
        self.p = cfg.dropout_rate
        self.d_ff = cfg.d_ff

    def fused(self, x) -> bool:
        """Whether ``x`` takes the gated-GELU kernel: a gated feed-forward on the GPU in bf16.  One row
        through the float linears in inference (greedy decoding of one source) stays on the composition:
        the kernel measured 0.5 % slower per token there and faster everywhere else
        (profiles/t5_v11/SUMMARY.md).  The int8 linears take the kernel at every row count, in the module
        path and in the fused decode step alike."""
        if not (self.gated and x.is_cuda and x.dtype == torch.bfloat16 and self.d_ff % 8 == 0 and fused_ff_kernels()):
            return False
        one_row = x.numel() == x.shape[-1]
        return not (one_row and not self.training and isinstance(self.wi, nn.Linear))

    def gate(self, g, u):
        """gelu_tanh(g) * u without dropout: the activation of the inference steps (the int8 decode
        step calls it on the halves of its stacked GEMM output, so both paths give the same bits)."""
        if self.fused(g):
            return ops.gated_gelu(g, u, 0.0, False)
        return F.gelu(g, approximate="tanh") * u

    def forward(self, x):
        if self.fused(x):
            return self.wo(ops.gated_gelu(self.wi(x), self.wi_1(x), self.p, self.training))
        h = F.gelu(self.wi(x), approximate="tanh") * self.wi_1(x) if self.gated else F.relu(self.wi(x))
        if self.training and self.p:
            h = F.dropout(h, self.p)
        return self.wo(h)


class T5Block(nn.Module):
    def __init__(self, cfg: T5Config, decoder: bool, relative_bias: bool, device=None, dtype=None):
        super().__init__()
        kw = dict(device=device, dtype=dtype)
        self.ln_sa = T5Norm(cfg.d_model, cfg.layer_norm_epsilon, **kw)
        self.sa = T5Attention(cfg, relative_bias, causal=decoder, **kw)
        self.decoder = decoder
        if decoder:
            self.ln_ca = T5Norm(cfg.d_model, cfg.layer_norm_epsilon, **kw)
            self.ca = T5Attention(cfg, False, causal=False, **kw)
        self.ln_ff = T5Norm(cfg.d_model, cfg.layer_norm_epsilon, **kw)
        self.ff = T5FF(cfg, **kw)
        self.p = cfg.dropout_rate

    def _drop(self, x):
        return F.dropout(x, self.p) if (self.training and self.p) else x

    def forward(self, x, rel, key_bias=None, enc=None, enc_bias=None, cache=None, offset: int = 0):
        new_cache = {}
        h, new_cache["self"] = self.sa(self.ln_sa(x), rel=rel, key_bias=key_bias,
                                       cache=cache.get("self") if cache else None, offset=offset)
        x = x + self._drop(h)
        if self.decoder:
            h, new_cache["cross"] = self.ca(self.ln_ca(x), kv=enc, key_bias=enc_bias,
                                            cache=cache.get("cross") if cache else None)
            x = x + self._drop(h)
        x = x + self._drop(self.ff(self.ln_ff(x)))
        return x, new_cache


class T5Stack(nn.Module):
    def __init__(self, cfg: T5Config, decoder: bool, embed: nn.Embedding, device=None, dtype=None):
        super().__init__()
        n = cfg.num_decoder_layers if decoder else cfg.num_layers
        self.embed = embed
        self.blocks = nn.ModuleList([T5Block(cfg, decoder, i == 0, device, dtype) for i in range(n)])
        self.final = T5Norm(cfg.d_model, cfg.layer_norm_epsilon, device, dtype)
        self.decoder = decoder
        self.p = cfg.dropout_rate

    def forward(self, ids, mask=None, enc=None, enc_mask=None, caches=None, offset: int = 0):
        x = self.embed(ids)
        if self.training and self.p:
            x = F.dropout(x, self.p)
        B, S = ids.shape
        sk = S + offset
        rel = self.blocks[0].sa.relative_vector(S, sk, ids.device, offset)
        key_bias = (1.0 - mask.float()) * -1e9 if mask is not None else None
        enc_bias = (1.0 - enc_mask.float()) * -1e9 if enc_mask is not None else None
        new_caches = []
        for i, blk in enumerate(self.blocks):
            x, c = blk(x, rel, key_bias, enc, enc_bias, caches[i] if caches else None, offset)
            new_caches.append(c)
        x = self.final(x)
        if self.training and self.p:
            x = F.dropout(x, self.p)
        return x, new_caches


class T5ForConditionalGeneration(nn.Module):
    def __init__(self, cfg: T5Config = None, device=None, dtype=torch.bfloat16):
        super().__init__()
        cfg = cfg or T5Config()
        self.cfg = cfg
        self.shared = nn.Embedding(cfg.vocab_size, cfg.d_model, device=device, dtype=dtype)
        nn.init.normal_(self.shared.weight, std=1.0)
        self.encoder = T5Stack(cfg, False, self.shared, device, dtype)
        self.decoder = T5Stack(cfg, True, self.shared, device, dtype)
        if not cfg.tie_word_embeddings:
            self.lm_head = nn.Linear(cfg.d_model, cfg.vocab_size, bias=False, device=device, dtype=dtype)
            nn.init.normal_(self.lm_head.weight, std=1.0)      # the library's init of an untied head
        self.dtype = dtype

    def head_weight(self):
        """The output head [vocab, d_model]: ``lm_head`` of an untied model, else the embedding."""
        return self.shared.weight if self.cfg.tie_word_embeddings else self.lm_head.weight

    def _shift_right(self, labels):
        start = torch.full_like(labels[:, :1], self.cfg.decoder_start_token_id)
        ids = torch.cat([start, labels[:, :-1]], 1)
        return ids.masked_fill(ids == -100, self.cfg.pad_token_id)

    def forward(self, input_ids, labels, attention_mask=None, decoder_input_ids=None):
        """Training: mean token cross-entropy (the tied head scaled by d_model^-0.5, or the untied
        ``lm_head`` unscaled: ``cfg.scales_outputs``)."""
        enc, _ = self.encoder(input_ids, attention_mask)
        dec_ids = decoder_input_ids if decoder_input_ids is not None else self._shift_right(labels)
        dec, _ = self.decoder(dec_ids, enc=enc, enc_mask=attention_mask)
        if self.cfg.scales_outputs:
            dec = dec * (self.cfg.d_model ** -0.5)
        x = dec.reshape(-1, self.cfg.d_model)
        return ops.cross_entropy_fused(x, self.head_weight(), None, labels.reshape(-1), ignore_index=-100)

    def logits(self, dec):
        if self.cfg.scales_outputs:
            dec = dec * (self.cfg.d_model ** -0.5)
        return F.linear(dec, self.head_weight())

    def quantize_dynamic(self):
        """The int8 inference model of this one (``models.t5_quant``; the reference's
        ``torch.quantization.quantize_dynamic`` step): every linear and the output head in int8,
        ``generate`` with all its modes unchanged.  This model is left as it is."""
        from cloudtik_amd.models.t5_quant import QuantT5ForConditionalGeneration
        return QuantT5ForConditionalGeneration.from_float(self)

    @torch.no_grad()
    def generate(self, input_ids, attention_mask=None, max_new_tokens: int = 32,
                 use_graph: Optional[bool] = None, num_beams: int = 1, length_penalty: float = 1.0,
                 early_stopping: bool = False, return_scores: bool = False, trace: Optional[list] = None,
                 do_sample: bool = False, temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0,
                 repetition_penalty: float = 1.0, num_return_sequences: int = 1, seed: Optional[int] = None,
                 no_repeat_ngram_size: int = 0, min_new_tokens: int = 0, min_length: int = 0,
                 bad_words_ids: Optional[List[List[int]]] = None):
        """Greedy decoding with a KV cache (self-attention K/V grow; cross K/V computed once).

        On the GPU the decode step is captured once into a HIP graph over a static KV cache
        of ``max_new_tokens`` slots and replayed per token (``_generate_graph``): a decode step
        is ~15 small kernels per layer, so launch overhead, not math, bounds eager decoding.

        ``num_beams`` > 1 searches with that many beams (``ops.beam`` states the rules: the
        tensor-only beam search of HF ``generate``, every step run) and returns the best
        finished hypothesis [B, max_new_tokens], pad after EOS; with ``return_scores`` also its
        score, sum of log-probabilities / length**``length_penalty``, fp32 [B].  On the GPU the
        step runs at batch B * num_beams inside the same kind of graph, with the bookkeeping
        in the beam kernels (``_generate_beam_static``); ``use_graph=False``, a ``trace`` list and
        the CPU run the eager reference loop, which appends every step's 2K candidate scores
        [B, 2K] to ``trace``.  ``num_return_sequences`` = N <= ``num_beams`` returns the N best
        finished hypotheses [B * N, max_new_tokens], item-major (rows b * N .. b * N + N - 1 belong
        to input b), and their scores [B * N].

        ``do_sample`` draws every token instead (``ops.sampling`` states the rule: repetition
        penalty, temperature, top-k, top-p as the HF logits processors apply them, then one draw
        per row and step from a Philox stream keyed by ``seed``).  It needs ``num_beams`` = 1 and
        returns N = ``num_return_sequences`` independent samples per input, [B * N,
        max_new_tokens], item-major, pad after EOS.  ``top_k`` = 0 (or >= the vocabulary) and
        ``top_p`` = 1 are off.  ``seed`` is an int in [0, 2**63); None draws one from torch's
        default CPU generator, so ``torch.manual_seed`` makes a program reproducible.  The same
        seed, arguments and model give the same tokens replayed, eager on the static step, or
        called again.  On the GPU the step runs at batch B * N inside a graph that ends in the
        sampling kernel (``_generate_sample_static``) and reads the seed from the device, so one
        capture per (temperature, top_k, top_p, repetition_penalty) serves every seed;
        ``use_graph=False`` runs the eager loop on the growing-cache decoder, ended by the same
        kernel on the GPU and by the reference on the CPU.  Without ``do_sample`` the sampling
        arguments must be at their defaults.

        ``no_repeat_ngram_size``, ``min_new_tokens``, ``min_length`` (the library's: it counts the
        start token, so the minimum is ``max(min_new_tokens, min_length - 1)`` new tokens) and
        ``bad_words_ids`` ban tokens by the row's history (``ops.constrain`` states the rule: the HF
        logits processors of the same names) in all three modes and on every path: one kernel launch
        per step inside the graph or the eager loop on the GPU, the reference on the CPU.  Beam
        search masks after the log-softmax, as the library does.  At their defaults nothing is
        launched and the captures and their keys are what they were; otherwise the frozen rule
        joins the key."""
        if use_graph is None:
            use_graph = input_ids.is_cuda and os.environ.get("CLOUDTIK_AMD_T5_GRAPH", "1") == "1"
        beam_ops.check_beam_args(num_beams, self.cfg.vocab_size, early_stopping)
        sample_ops.check_sample_args(temperature, top_k, top_p, repetition_penalty, num_return_sequences, seed)
        cons = constrain_ops.check_constrain_args(no_repeat_ngram_size, min_new_tokens, min_length, bad_words_ids,
                                                  self.cfg.vocab_size, self.cfg.eos_token_id, num_beams, max_new_tokens)
        N = num_return_sequences
        if do_sample:
            if num_beams != 1:
                raise ValueError("do_sample needs num_beams = 1 (beam sampling is not supported)")
            if return_scores or trace is not None:
                raise ValueError("return_scores and trace belong to beam search (num_beams > 1)")
            if seed is None:
                seed = int(torch.randint(0, 2 ** 63 - 1, (1,), dtype=torch.int64).item())
            if use_graph and input_ids.is_cuda:
                return self._generate_sample_static(input_ids, attention_mask, max_new_tokens, N, seed, temperature,
                                                    top_k, top_p, repetition_penalty, cons=cons)
            return self._generate_sample_eager(input_ids, attention_mask, max_new_tokens, N, seed, temperature,
                                               top_k, top_p, repetition_penalty, cons=cons)
        if temperature != 1.0 or top_k != 0 or top_p != 1.0 or repetition_penalty != 1.0 or seed is not None:
            raise ValueError("temperature, top_k, top_p, repetition_penalty and seed belong to sampling (do_sample=True)")
        if N > num_beams:
            raise ValueError(f"num_return_sequences = {N} needs do_sample=True or num_beams >= {N}, got num_beams = {num_beams}")
        if num_beams > 1:
            if use_graph and input_ids.is_cuda and trace is None:
                seq, score = self._generate_beam_static(input_ids, attention_mask, max_new_tokens, num_beams,
                                                        length_penalty, early_stopping, num_return=N, cons=cons)
            else:
                seq, score = self._generate_beam_eager(input_ids, attention_mask, max_new_tokens, num_beams,
                                                       length_penalty, early_stopping, trace, num_return=N, cons=cons)
            return (seq, score) if return_scores else seq
        if return_scores or trace is not None:
            raise ValueError("return_scores and trace belong to beam search (num_beams > 1)")
        if use_graph and input_ids.is_cuda:
            try:
                return self._generate_graph(input_ids, attention_mask, max_new_tokens, cons)
            except RuntimeError as e:          # capture unsupported by some op: eager fallback
                logger.warning("T5 graph decoding unavailable (%s); decoding eagerly", e)
        enc, _ = self.encoder(input_ids, attention_mask)
        B = input_ids.shape[0]
        cur = torch.full((B, 1), self.cfg.decoder_start_token_id, dtype=torch.long, device=input_ids.device)
        out, caches = [], None
        done = torch.zeros(B, dtype=torch.bool, device=input_ids.device)
        con, hist = self._constrainer(cons, input_ids.device), None
        if con is not None:                    # the row's history as the ban rule reads it: pad after EOS
            hist = torch.full((B, max_new_tokens), self.cfg.pad_token_id, dtype=torch.long, device=input_ids.device)
        for step in range(max_new_tokens):
            dec, caches = self.decoder(cur, enc=enc, enc_mask=attention_mask, caches=caches, offset=step)
            logits = self.logits(dec[:, -1])
            if con is not None:
                logits = con(logits, hist, torch.tensor([step], dtype=torch.long, device=input_ids.device))
            nxt = logits.float().argmax(-1)
            nxt = torch.where(done, torch.full_like(nxt, self.cfg.pad_token_id), nxt)
            if con is not None:
                hist[:, step] = nxt
            out.append(nxt)
            done |= nxt == self.cfg.eos_token_id
            cur = nxt[:, None]
        return torch.stack(out, 1)

    def _constrainer(self, cons, dev):
        """The frozen ban rule of ``generate`` bound to this model's tokens and a device, or None."""
        if cons is None:
            return None
        return constrain_ops.Constrainer(cons, self.cfg.decoder_start_token_id, self.cfg.eos_token_id, dev)

    def _generate_graph(self, input_ids, attention_mask, max_new: int, cons=None) -> torch.Tensor:
        """Graph-replayed greedy decoding.  The captured graph and its static buffers are cached
        per (batch, source length, steps, masked) and, when one is on, the ban rule ``cons``: a later
        call only runs the encoder, copies the cross-attention K/V and the source mask into the
        static buffers and replays."""
        cfg = self.cfg
        dev = input_ids.device
        B, S, T = input_ids.shape[0], input_ids.shape[1], max_new
        dec = self.decoder
        enc, _ = self.encoder(input_ids, attention_mask)
        key = (B, S, T, attention_mask is not None, str(dev)) + ((cons,) if cons is not None else ())
        cache = getattr(self, "_graphs", None)
        if cache is None:
            cache = self._graphs = {}
        st = cache.get(key)
        if st is None:
            st = cache[key] = self._capture_decode(B, S, T, enc.dtype, dev, attention_mask is not None, cons)
        for i, b in enumerate(dec.blocks):
            st["cross"][i][0].copy_(b.ca._split(b.ca.k(enc)))
            st["cross"][i][1].copy_(b.ca._split(b.ca.v(enc)))
        if attention_mask is not None:
            st["enc_bias"].copy_((1.0 - attention_mask.float()) * -1e9)
        st["reset"]()
        for _ in range(T):
            st["graph"].replay()
        return st["out"].clone()

    def _decode_step_static(self, cur, pos, slots, kc, vc, cross, enc_bias):
        """One decoder step over static buffers, free of host decisions (capturable): embeds
        ``cur`` [B, 1], writes each layer's self-attention K/V into slot ``pos`` of ``kc`` / ``vc``
        [B, T, H, D] and returns the final hidden states [B, 1, d_model]."""
        cfg, dec = self.cfg, self.decoder
        B, T = cur.shape[0], slots.shape[0]
        x = dec.embed(cur)
        bucket = relative_position_bucket(slots - pos, False, cfg.relative_attention_num_buckets,
                                          cfg.relative_attention_max_distance)
        relvec = dec.blocks[0].sa.rel(bucket).t().float().contiguous()     # query at `pos`, keys 0..T-1
        key_bias = torch.where(slots <= pos, 0.0, -1e9).float()[None].expand(B, T).contiguous()
        for i, blk in enumerate(dec.blocks):
            h = blk.ln_sa(x)
            a = blk.sa
            q, k, v = a._split(a.q(h)), a._split(a.k(h)), a._split(a.v(h))
            kc[i].index_copy_(1, pos, k)
            vc[i].index_copy_(1, pos, v)
            o = ops.attention_relbias(q, kc[i], vc[i], relvec, 0, key_bias, scale=1.0, causal=False)
            x = x + a.o(o.reshape(B, 1, -1))
            h = blk.ln_ca(x)
            c = blk.ca
            q = c._split(c.q(h))
            o = ops.attention(q.transpose(1, 2), cross[i][0].transpose(1, 2), cross[i][1].transpose(1, 2),
                              key_bias=enc_bias, scale=1.0).transpose(1, 2)
            x = x + c.o(o.reshape(B, 1, -1))
            x = x + blk.ff(blk.ln_ff(x))
        return dec.final(x)

    def _capture_decode(self, B, S, T, dtype, dev, masked: bool, cons=None):
        cfg = self.cfg
        H, D = cfg.num_heads, cfg.d_kv
        dec = self.decoder
        kc = [torch.zeros(B, T, H, D, dtype=dtype, device=dev) for _ in dec.blocks]
        vc = [torch.zeros(B, T, H, D, dtype=dtype, device=dev) for _ in dec.blocks]
        cross = [(torch.zeros(B, S, H, D, dtype=dtype, device=dev), torch.zeros(B, S, H, D, dtype=dtype, device=dev))
                 for _ in dec.blocks]
        enc_bias = torch.zeros(B, S, device=dev) if masked else None
        cur = torch.full((B, 1), cfg.decoder_start_token_id, dtype=torch.long, device=dev)
        pos = torch.zeros(1, dtype=torch.long, device=dev)
        out = torch.full((B, T), cfg.pad_token_id, dtype=torch.long, device=dev)
        done = torch.zeros(B, dtype=torch.bool, device=dev)
        slots = torch.arange(T, device=dev)
        pad = torch.full((B,), cfg.pad_token_id, dtype=torch.long, device=dev)
        con = self._constrainer(cons, dev)         # holds the bad-word tables the captured kernel reads

        def step():
            x = self._decode_step_static(cur, pos, slots, kc, vc, cross, enc_bias)
            logits = self.logits(x[:, -1])
            if con is not None:                    # `out` is the history: slots < pos, pad after EOS
                con(logits, out, pos)
            nxt = logits.float().argmax(-1)
            nxt = torch.where(done, pad, nxt)
            out.index_copy_(1, pos, nxt[:, None])
            done.logical_or_(nxt == cfg.eos_token_id)
            cur.copy_(nxt[:, None])
            pos.add_(1)

        def reset():
            cur.fill_(cfg.decoder_start_token_id)
            pos.zero_()
            out.fill_(cfg.pad_token_id)
            done.zero_()

        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):          # warm up (lazy inits, library handles) off the capture
            step()
        torch.cuda.current_stream().wait_stream(side)
        reset()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            step()
        # "step" keeps the buffers only the captured kernels still use (the caches) allocated
        return {"graph": graph, "cross": cross, "enc_bias": enc_bias, "out": out, "reset": reset, "step": step}

    # ------------------------------------------------------------------------- beam search
    @torch.no_grad()
    def _generate_beam_eager(self, input_ids, attention_mask, max_new, K, length_penalty, early_stopping, trace=None,
                             num_return: int = 1, cons=None):
        """The reference beam loop, any device and dtype: the growing-cache decoder at batch
        B * K and ``beam_step_reference`` / ``cache_reorder_reference`` after every step."""
        cfg, dev = self.cfg, input_ids.device
        B, T = input_ids.shape[0], max_new
        enc, _ = self.encoder(input_ids, attention_mask)
        enc = enc.repeat_interleave(K, 0)
        mask = attention_mask.repeat_interleave(K, 0) if attention_mask is not None else None
        state = beam_ops.new_state(B, K, T, cfg.pad_token_id, dev)
        len_pen = beam_ops.length_penalty_table(T, length_penalty, dev)
        cur = torch.full((B * K, 1), cfg.decoder_start_token_id, dtype=torch.long, device=dev)
        caches = None
        con = self._constrainer(cons, dev)
        for t in range(T):
            dec, caches = self.decoder(cur, enc=enc, enc_mask=mask, caches=caches, offset=t)
            logits, ban = self.logits(dec[:, -1]), None
            if con is not None:                    # row b * K + k has the history run_seq[b, k]
                ban = con.ban_mask(logits, state["run_seq"].reshape(B * K, T),
                                   torch.tensor([t], dtype=torch.long, device=dev))
            state, beam_idx, nxt, cand, _ = beam_ops.beam_step_reference(
                logits, state, t, len_pen, cfg.eos_token_id, early_stopping, ban=ban)
            if trace is not None:
                trace.append(cand)
            for c in caches:                       # cross K/V are the same for every beam of an item
                c["self"] = tuple(beam_ops.cache_reorder_reference(c["self"], beam_idx))
            cur = nxt[:, None]
        return self._best_finished(state, num_return)

    @staticmethod
    def _best_finished(state, n: int):
        """The n best finished hypotheses and their scores: [B, T] and [B] for n = 1, else flattened
        item-major to [B * n, T] and [B * n]."""
        seq, score = state["fin_seq"], state["fin_score"]
        if n == 1:
            return seq[:, 0].clone(), score[:, 0].clone()
        return seq[:, :n].reshape(-1, seq.shape[2]).clone(), score[:, :n].reshape(-1).clone()

    @torch.no_grad()
    def _generate_beam_static(self, input_ids, attention_mask, max_new, K, length_penalty=1.0, early_stopping=False,
                              fused: bool = True, graph: bool = True, trace=None, select: str = "sort",
                              num_return: int = 1, cons=None):
        """Beam search over the static-cache decode step at batch B * K.  ``fused``: the beam
        kernels do the bookkeeping (else the PyTorch reference does, on the same step, so both
        see the same logits); ``graph``: two captured graphs, one per cache parity, are replayed
        in turn (else the same step runs eagerly and fills ``trace``).  Captures are cached like
        the greedy ones, additionally by (K, length_penalty, early_stopping) and, when one is on, the
        ban rule ``cons``."""
        dev = input_ids.device
        B, S, T = input_ids.shape[0], input_ids.shape[1], max_new
        if trace is not None and graph:
            raise ValueError("trace needs graph=False")
        enc, _ = self.encoder(input_ids, attention_mask)
        masked = attention_mask is not None
        key = ("beam", B, S, T, masked, str(dev), K, float(length_penalty), bool(early_stopping), fused, graph, select)
        if cons is not None:
            key = key + (cons,)
        cache = getattr(self, "_graphs", None)
        if cache is None:
            cache = self._graphs = {}
        st = cache.get(key)
        if st is None:
            st = cache[key] = self._capture_beam_decode(B, S, T, enc.dtype, dev, masked, K, length_penalty,
                                                        early_stopping, fused, graph, select, cons)
        for i, b in enumerate(self.decoder.blocks):     # cross K/V: expanded to B * K rows once per call
            st["cross"][i][0].copy_(b.ca._split(b.ca.k(enc)).repeat_interleave(K, 0))
            st["cross"][i][1].copy_(b.ca._split(b.ca.v(enc)).repeat_interleave(K, 0))
        if masked:
            st["enc_bias"].copy_(((1.0 - attention_mask.float()) * -1e9).repeat_interleave(K, 0))
        st["reset"]()
        st["trace"][0] = trace
        for t in range(T):
            st["steps"][t & 1]()
        st["trace"][0] = None
        return self._best_finished(st["state"], num_return)

    def _capture_beam_decode(self, B, S, T, dtype, dev, masked, K, length_penalty, early_stopping, fused, graph,
                             select, cons=None):
        cfg = self.cfg
        H, D, R = cfg.num_heads, cfg.d_kv, B * K
        n = len(self.decoder.blocks)

        def zeros(*shape):
            return torch.zeros(*shape, dtype=dtype, device=dev)

        # self-attention caches in two sets: step t reads and extends set t & 1, and the reorder
        # gathers its rows by source beam into the other set, which step t + 1 uses
        kc = [[zeros(R, T, H, D) for _ in range(n)] for _ in range(2)]
        vc = [[zeros(R, T, H, D) for _ in range(n)] for _ in range(2)]
        cross = [(zeros(R, S, H, D), zeros(R, S, H, D)) for _ in range(n)]
        enc_bias = torch.zeros(R, S, device=dev) if masked else None
        cur = torch.full((R, 1), cfg.decoder_start_token_id, dtype=torch.long, device=dev)
        pos = torch.zeros(1, dtype=torch.long, device=dev)
        arrive = torch.zeros(1, dtype=torch.int32, device=dev)
        beam_idx = torch.zeros(R, dtype=torch.long, device=dev)
        slots = torch.arange(T, device=dev)
        state = beam_ops.new_state(B, K, T, cfg.pad_token_id, dev)
        len_pen = beam_ops.length_penalty_table(T, length_penalty, dev)
        reorder = [beam_ops.CacheReorder(kc[p] + vc[p], kc[1 - p] + vc[1 - p]) for p in range(2)] if fused else None
        trace = [None]
        con = self._constrainer(cons, dev)         # holds the bad-word tables the captured kernel reads
        hist = state["run_seq"].view(R, T)         # row b * K + k: gathered by source beam in every update
        ban_lse = torch.empty(R, dtype=torch.float32, device=dev) if con is not None and fused else None

        def step(p):
            x = self._decode_step_static(cur, pos, slots, kc[p], vc[p], cross, enc_bias)
            logits = self.logits(x[:, -1])
            if fused:
                if con is not None:
                    con(logits, hist, pos, ban_lse)
                beam_ops.beam_step(logits, state, pos, arrive, len_pen, beam_idx, cur, cfg.eos_token_id, early_stopping,
                                   ban_lse=ban_lse)
                reorder[p](beam_idx, pos)
                return
            ban = con.ban_mask(logits, hist, pos) if con is not None else None
            new, src, nxt, cand, _ = beam_ops.beam_step_reference(logits, state, pos, len_pen, cfg.eos_token_id,
                                                                  early_stopping, select=select, ban=ban)
            if trace[0] is not None:
                trace[0].append(cand)
            for name, v in new.items():
                state[name].copy_(v)
            cur.copy_(nxt[:, None])
            beam_ops.cache_reorder_reference(kc[p] + vc[p], src, out=kc[1 - p] + vc[1 - p])
            pos.add_(1)

        def reset():
            cur.fill_(cfg.decoder_start_token_id)
            pos.zero_()
            arrive.zero_()
            beam_ops.reset_state(state, cfg.pad_token_id)

        steps = [lambda: step(0), lambda: step(1)]
        if graph:
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):      # warm up (lazy inits, library handles) off the capture
                for p in range(2):
                    reset()
                    step(p)
            torch.cuda.current_stream().wait_stream(side)
            reset()
            graphs = [torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()]
            for p in range(2):
                with torch.cuda.graph(graphs[p]):
                    step(p)
            steps = [graphs[0].replay, graphs[1].replay]
        # "step" keeps what only the captured kernels still use (caches, pointer tables) allocated
        return {"steps": steps, "cross": cross, "enc_bias": enc_bias, "state": state, "reset": reset, "trace": trace,
                "step": step}

    # ---------------------------------------------------------------------------- sampling
    @torch.no_grad()
    def _generate_sample_eager(self, input_ids, attention_mask, max_new, N, seed, temperature=1.0, top_k=0, top_p=1.0,
                               repetition_penalty=1.0, cons=None):
        """The eager sampling loop, any device and dtype: the growing-cache decoder at batch B * N,
        and after every step ``sample_step_reference`` on the CPU or the sampling kernel on the GPU."""
        cfg, dev = self.cfg, input_ids.device
        R, T = input_ids.shape[0] * N, max_new
        enc, _ = self.encoder(input_ids, attention_mask)
        enc = enc.repeat_interleave(N, 0)
        mask = attention_mask.repeat_interleave(N, 0) if attention_mask is not None else None
        out = torch.full((R, T), cfg.pad_token_id, dtype=torch.long, device=dev)
        done = torch.zeros(R, dtype=torch.bool, device=dev)
        cur = torch.full((R, 1), cfg.decoder_start_token_id, dtype=torch.long, device=dev)
        pos = torch.zeros(1, dtype=torch.long, device=dev)
        seed_t = torch.tensor([seed], dtype=torch.long, device=dev)
        rule = (cfg.decoder_start_token_id, cfg.eos_token_id, cfg.pad_token_id, temperature, top_k, top_p,
                repetition_penalty)
        caches = None
        con = self._constrainer(cons, dev)
        for t in range(T):
            dec, caches = self.decoder(cur, enc=enc, enc_mask=mask, caches=caches, offset=t)
            logits = self.logits(dec[:, -1])
            if con is not None:                    # the bans first: `out` is the history
                logits = con(logits.contiguous(), out, pos)
            if dev.type == "cuda":
                sample_ops.sample_step(logits.contiguous(), out, done, cur, pos, seed_t, *rule)
            else:
                out, done, cur, pos = sample_ops.sample_step_reference(logits, out, done, cur, pos, seed_t, *rule)[:4]
        return out

    @torch.no_grad()
    def _generate_sample_static(self, input_ids, attention_mask, max_new, N, seed, temperature=1.0, top_k=0,
                                top_p=1.0, repetition_penalty=1.0, graph: bool = True, cons=None):
        """Sampling over the static-cache decode step at batch R = B * N, ended by the sampling
        kernel.  ``graph``: the captured step is replayed (else the same step runs eagerly).
        Captures are cached like the greedy ones, additionally by the sampling parameters, which
        are launch arguments, and, when one is on, the ban rule ``cons``; the seed is a device tensor
        ``reset`` rewrites, so it is not in the key."""
        dev = input_ids.device
        B, S, T = input_ids.shape[0], input_ids.shape[1], max_new
        R = B * N
        enc, _ = self.encoder(input_ids, attention_mask)
        masked = attention_mask is not None
        key = ("sample", R, S, T, masked, str(dev), float(temperature), int(top_k), float(top_p),
               float(repetition_penalty)) + ((cons,) if cons is not None else ()) + (graph,)
        cache = getattr(self, "_graphs", None)
        if cache is None:
            cache = self._graphs = {}
        st = cache.get(key)
        if st is None:
            st = cache[key] = self._capture_sample_decode(R, S, T, enc.dtype, dev, masked, float(temperature),
                                                          int(top_k), float(top_p), float(repetition_penalty), graph,
                                                          cons)
        for i, b in enumerate(self.decoder.blocks):     # cross K/V: expanded to B * N rows once per call
            st["cross"][i][0].copy_(b.ca._split(b.ca.k(enc)).repeat_interleave(N, 0))
            st["cross"][i][1].copy_(b.ca._split(b.ca.v(enc)).repeat_interleave(N, 0))
        if masked:
            st["enc_bias"].copy_(((1.0 - attention_mask.float()) * -1e9).repeat_interleave(N, 0))
        st["reset"](seed)
        for _ in range(T):
            st["run"]()
        return st["out"].clone()

    def _capture_sample_decode(self, R, S, T, dtype, dev, masked, temperature, top_k, top_p, repetition_penalty,
                               graph, cons=None):
        cfg = self.cfg
        H, D = cfg.num_heads, cfg.d_kv
        dec = self.decoder
        kc = [torch.zeros(R, T, H, D, dtype=dtype, device=dev) for _ in dec.blocks]
        vc = [torch.zeros(R, T, H, D, dtype=dtype, device=dev) for _ in dec.blocks]
        cross = [(torch.zeros(R, S, H, D, dtype=dtype, device=dev), torch.zeros(R, S, H, D, dtype=dtype, device=dev))
                 for _ in dec.blocks]
        enc_bias = torch.zeros(R, S, device=dev) if masked else None
        cur = torch.full((R, 1), cfg.decoder_start_token_id, dtype=torch.long, device=dev)
        pos = torch.zeros(1, dtype=torch.long, device=dev)
        seed = torch.zeros(1, dtype=torch.long, device=dev)
        out = torch.full((R, T), cfg.pad_token_id, dtype=torch.long, device=dev)
        done = torch.zeros(R, dtype=torch.bool, device=dev)
        slots = torch.arange(T, device=dev)
        rule = (cfg.decoder_start_token_id, cfg.eos_token_id, cfg.pad_token_id, temperature, top_k, top_p,
                repetition_penalty)
        con = self._constrainer(cons, dev)         # holds the bad-word tables the captured kernel reads

        def step():
            x = self._decode_step_static(cur, pos, slots, kc, vc, cross, enc_bias)
            logits = self.logits(x[:, -1])
            if con is not None:                    # the bans first: `out` is the history
                con(logits, out, pos)
            sample_ops.sample_step(logits, out, done, cur, pos, seed, *rule)

        def reset(seed_value=0):
            seed.fill_(seed_value)
            cur.fill_(cfg.decoder_start_token_id)
            pos.zero_()
            out.fill_(cfg.pad_token_id)
            done.zero_()

        run = step
        if graph:
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):      # warm up (lazy inits, library handles) off the capture
                step()
            torch.cuda.current_stream().wait_stream(side)
            reset()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                step()
            run = g.replay
        # "step" keeps the buffers only the captured kernels still use (the caches) allocated
        return {"run": run, "cross": cross, "enc_bias": enc_bias, "out": out, "reset": reset, "step": step}

    # --------------------------------------------------------------------- pretrained weights
    @classmethod
    def from_pretrained(cls, path, device=None, dtype=torch.bfloat16):
        """The model of a local HF checkpoint directory (nothing is ever downloaded): ``config.json`` and
        the weights in ``model.safetensors``, ``pytorch_model.bin``, or the shards that
        ``model.safetensors.index.json`` / ``pytorch_model.bin.index.json`` list.  The head is untied when
        the config says ``tie_word_embeddings: false`` or the weights hold an ``lm_head.weight`` that differs
        from ``shared.weight`` (newer versions of the library save an untied model as ``tie_word_embeddings:
        true, scale_decoder_outputs: false`` plus that tensor); ``scale_decoder_outputs`` is the config's
        when it has one, else that of a tied head exactly."""
        import json
        path = os.fspath(path)
        if not os.path.isdir(path):
            raise FileNotFoundError(f"from_pretrained takes a local checkpoint directory, got {path!r}")
        with open(os.path.join(path, "config.json")) as f:
            config = json.load(f)
        sd = _read_checkpoint(path)
        head, shared = sd.get("lm_head.weight"), sd.get("shared.weight")
        differs = head is not None and shared is not None and (head.shape != shared.shape or not torch.equal(head, shared))
        tie = config.get("tie_word_embeddings")
        untied = differs or (tie is not None and not tie)
        model = cls.from_hf_config({**config, "tie_word_embeddings": not untied}, device=device, dtype=dtype,
                                   untied_head=untied)
        return model.load_hf_state_dict(sd)

    @classmethod
    def from_hf_config(cls, config, device=None, dtype=torch.bfloat16, untied_head: bool = False):
        """A model with the topology of a HF T5 config: a ``T5Config`` of the library, a dict, or
        the path of a local ``config.json``.  ``untied_head``: an output head of its own (``lm_head``,
        T5 v1.1 / Flan-T5), whatever the config's ``tie_word_embeddings``; without it such a config is
        refused, since the weights decide too (``from_pretrained`` looks at both).  A
        ``scale_decoder_outputs`` key is honoured; absent, a tied head scales and an untied one does not."""
        if isinstance(config, (str, os.PathLike)):
            import json
            with open(config) as f:
                config = json.load(f)
        elif not isinstance(config, dict):
            config = config.to_dict()
        def get(name, default):                    # a key saved as null counts as absent
            v = config.get(name)
            return default if v is None else v

        act = get("feed_forward_proj", "relu")
        if act not in ("relu", "gated-gelu"):
            raise ValueError(f"unsupported feed_forward_proj {act!r} (relu and gated-gelu are)")
        if not get("tie_word_embeddings", True):
            if not untied_head:
                raise ValueError("the config has an untied output head (tie_word_embeddings=False): load the checkpoint "
                                 "directory with from_pretrained, or pass untied_head=True")
        eos = get("eos_token_id", 1)
        if isinstance(eos, (list, tuple)):
            if len(eos) != 1:
                raise ValueError(f"one eos_token_id is supported, got {eos}")
            eos = eos[0]
        cfg = T5Config(
            vocab_size=config["vocab_size"], d_model=config["d_model"], d_kv=config["d_kv"], d_ff=config["d_ff"],
            num_layers=config["num_layers"], num_decoder_layers=get("num_decoder_layers", config["num_layers"]),
            num_heads=config["num_heads"],
            relative_attention_num_buckets=get("relative_attention_num_buckets", 32),
            relative_attention_max_distance=get("relative_attention_max_distance", 128),
            dropout_rate=get("dropout_rate", 0.1), layer_norm_epsilon=get("layer_norm_epsilon", 1e-6),
            gated_gelu=act == "gated-gelu", pad_token_id=get("pad_token_id", 0),
            decoder_start_token_id=get("decoder_start_token_id", 0), eos_token_id=eos,
            tie_word_embeddings=not untied_head, scale_decoder_outputs=config.get("scale_decoder_outputs"))
        return cls(cfg, device=device, dtype=dtype)

    def _hf_name_map(self):
        """{our parameter name: HF state-dict key}."""
        names = {"shared.weight": "shared.weight"}
        if not self.cfg.tie_word_embeddings:
            names["lm_head.weight"] = "lm_head.weight"
        for stack, blocks in (("encoder", self.encoder.blocks), ("decoder", self.decoder.blocks)):
            names[f"{stack}.final.weight"] = f"{stack}.final_layer_norm.weight"
            ff = 2 if stack == "decoder" else 1
            for i, _ in enumerate(blocks):
                ours, hf = f"{stack}.blocks.{i}", f"{stack}.block.{i}.layer"
                for w in "qkvo":
                    names[f"{ours}.sa.{w}.weight"] = f"{hf}.0.SelfAttention.{w}.weight"
                if i == 0:
                    names[f"{ours}.sa.rel.weight"] = f"{hf}.0.SelfAttention.relative_attention_bias.weight"
                names[f"{ours}.ln_sa.weight"] = f"{hf}.0.layer_norm.weight"
                if stack == "decoder":
                    for w in "qkvo":
                        names[f"{ours}.ca.{w}.weight"] = f"{hf}.1.EncDecAttention.{w}.weight"
                    names[f"{ours}.ln_ca.weight"] = f"{hf}.1.layer_norm.weight"
                names[f"{ours}.ln_ff.weight"] = f"{hf}.{ff}.layer_norm.weight"
                if self.cfg.gated_gelu:
                    names[f"{ours}.ff.wi.weight"] = f"{hf}.{ff}.DenseReluDense.wi_0.weight"
                    names[f"{ours}.ff.wi_1.weight"] = f"{hf}.{ff}.DenseReluDense.wi_1.weight"
                else:
                    names[f"{ours}.ff.wi.weight"] = f"{hf}.{ff}.DenseReluDense.wi.weight"
                names[f"{ours}.ff.wo.weight"] = f"{hf}.{ff}.DenseReluDense.wo.weight"
        return names

    @torch.no_grad()
    def load_hf_state_dict(self, state_dict):
        """Copy the weights of a HF ``T5ForConditionalGeneration`` state dict (a dict, or the path
        of a local ``.bin`` / ``.pt`` / ``.safetensors`` file) into this model, cast to its dtype.
        Every parameter must be present with its shape, and no key may be left over: the tied
        copies of the embedding are accepted when they equal it; a model with an untied head requires
        ``lm_head.weight`` and copies it, a tied one refuses an ``lm_head.weight`` that differs."""
        if isinstance(state_dict, (str, os.PathLike)):
            path = os.fspath(state_dict)
            if path.endswith(".safetensors"):
                from safetensors.torch import load_file
                state_dict = load_file(path)
            else:
                state_dict = torch.load(path, map_location="cpu", weights_only=True)
        sd = dict(state_dict)
        shared = sd.get("shared.weight")
        tied_keys = ("encoder.embed_tokens.weight", "decoder.embed_tokens.weight") + \
            (("lm_head.weight",) if self.cfg.tie_word_embeddings else ())
        for tied in tied_keys:
            w = sd.pop(tied, None)
            if w is not None and (shared is None or w.shape != shared.shape or not torch.equal(w, shared.to(w.device))):
                raise ValueError(f"{tied} differs from shared.weight: untied embeddings / output heads are not supported")
        params = dict(self.named_parameters())
        names = self._hf_name_map()
        assert set(names) == set(params), sorted(set(names) ^ set(params))
        missing = sorted(hf for hf in names.values() if hf not in sd)
        extra = sorted(set(sd) - set(names.values()))
        if missing or extra:
            raise KeyError(f"load_hf_state_dict: missing keys {missing}, unknown keys {extra}")
        for ours, hf in names.items():
            if params[ours].shape != sd[hf].shape:
                raise ValueError(f"load_hf_state_dict: {hf} has shape {tuple(sd[hf].shape)}, "
                                 f"expected {tuple(params[ours].shape)}")
        for ours, hf in names.items():
            params[ours].copy_(sd[hf])
        return self                 # in place: graphs captured earlier read the new weights
