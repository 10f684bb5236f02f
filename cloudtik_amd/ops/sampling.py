"""Token sampling with fixed shapes and no host decision, so a decode step that ends in it can be
replayed as a graph: the rule as plain PyTorch (``sample_step_reference``; any device, the
specification) and the HIP kernel that applies the same rule on the GPU (``sample_step``;
csrc/sampling.hip).

The rule, for one row of logits ``l[0..V)`` (bf16 or fp32, taken to fp32), the row's earlier decoder
input (the start token and the tokens written so far) and a uniform ``u`` in [0, 1):

1. Repetition penalty: for every distinct token v of the decoder input, ``x[v] = l[v] * rp`` if
   ``l[v] < 0`` else ``l[v] / rp``, from the original value, so a token seen twice is penalised
   once.  The start token counts, and so does a pad written after EOS, as in HF ``generate``.
2. Temperature: ``x = x / temperature``, one IEEE fp32 division.  NaN ranks as -inf from here on.
3. Top-k: with ``0 < top_k < V`` keep ``x[v] >= (k-th largest x)``; everything tied with the k-th
   value stays.  ``top_k = 0`` and ``top_k >= V`` are off.
4. Top-p: with ``top_p < 1``, let ``w[v] = exp(x[v] - max)`` over the kept tokens and Z their sum;
   keep v iff ``A(x[v]) < top_p``, where A(t) is the sum of w over kept tokens with ``x > t``,
   divided by Z.  The best token has A = 0, so one token always stays.  This is the nucleus rule
   of HF ``TopPLogitsWarper`` written as a threshold, and it is symmetric in ties: a tie group
   that straddles the boundary stays whole, where the library splits it in sort order.
   ``top_p = 1`` is off.  (The reference evaluates A in fp32 the way the library does: ascending
   sort, softmax, running sum, compared with ``1 - top_p``; on untied fp32 rows it keeps the
   library's set.)
5. Draw: over the kept tokens in ascending token id, with inclusive cumulative weights C, the
   result is the lowest v with ``C[v] > u * Z``.
6. Bookkeeping: a row whose ``done`` flag is set emits pad; the token is written at slot ``pos`` of
   ``out`` and into the decoder's next input ``cur``; ``done |= token == eos``; ``pos`` advances
   once per step.  A row whose maximum is not finite (no finite logit) emits token 0.

``u`` comes from Philox4x32-10 with key ``(seed & 0xffffffff, seed >> 32)`` and counter
``(row, step, 0, 0)``: ``u = (word0 >> 8) * 2**-24`` (``philox_uniform_reference``).

Error model of the kernel.  The reference sums weights in floating point; the kernel truncates
every fp32 weight ``exp(x - max)`` to a multiple of ``2**-weight_bits(V)`` and sums the results as
64-bit integers, so its sums are exact and independent of order, and differ from the exact rule by
the rounding of ``exp`` (a few 2**-24, relative, per weight) and at most ``V * 2**-weight_bits(V)``
of truncation.  ``tests/test_t5_sample_gpu.py`` turns this into its tolerance.
"""
from __future__ import annotations

import math
from typing import Optional, Tuple

import torch

M32 = 0xFFFFFFFF


def _pkg():
    from cloudtik_amd import ops
    return ops


def weight_bits(vocab: int) -> int:
    """Fraction bits of the kernel's fixed-point weights: a row's sum stays below 2**62."""
    return 62 - max(int(vocab) - 1, 0).bit_length()


def check_sample_args(temperature=1.0, top_k=0, top_p=1.0, repetition_penalty=1.0, num_return_sequences=1,
                      seed=None) -> None:
    def number(v):
        return isinstance(v, (int, float)) and not isinstance(v, bool) and math.isfinite(v)

    if not number(temperature) or not temperature > 0:
        raise ValueError(f"temperature must be finite and > 0, got {temperature!r}")
    if not number(repetition_penalty) or not repetition_penalty > 0:
        raise ValueError(f"repetition_penalty must be finite and > 0, got {repetition_penalty!r}")
    if not number(top_p) or not 0 < top_p <= 1:
        raise ValueError(f"top_p must be in (0, 1], got {top_p!r}")
    if not isinstance(top_k, int) or isinstance(top_k, bool) or top_k < 0:
        raise ValueError(f"top_k must be an integer >= 0, got {top_k!r}")
    if not isinstance(num_return_sequences, int) or isinstance(num_return_sequences, bool) or num_return_sequences < 1:
        raise ValueError(f"num_return_sequences must be an integer >= 1, got {num_return_sequences!r}")
    if seed is not None and (not isinstance(seed, int) or isinstance(seed, bool) or not 0 <= seed < 2 ** 63):
        raise ValueError(f"seed must be None or an integer in [0, 2**63), got {seed!r}")


# ------------------------------------------------------------------------------------- Philox
def _mulhilo(a: int, b):
    """(high, low) 32-bit words of a * b for a constant a < 2**32 and b < 2**32, in arithmetic that
    stays below 2**63: Python ints and int64 tensors both take it."""
    bl, bh = b & 0xFFFF, b >> 16
    pl, ph = a * bl, a * bh
    hi = (ph + (pl >> 16)) >> 16
    lo = (pl + ((ph & 0xFFFF) << 16)) & M32
    return hi, lo


def philox4x32(counter, key):
    """Philox4x32-10 of a 4-word counter and a 2-word key: four 32-bit words, as Python ints or as
    int64 tensors, whichever came in."""
    c0, c1, c2, c3 = counter
    k0, k1 = key
    for _ in range(10):
        hi0, lo0 = _mulhilo(0xD2511F53, c0)
        hi1, lo1 = _mulhilo(0xCD9E8D57, c2)
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


def uniform_of_word(word: int) -> float:
    """A 32-bit word as a multiple of 2**-24 in [0, 1): its top 24 bits."""
    return (word >> 8) * 2.0 ** -24


def philox_uniform_reference(seed: int, row: int, step: int) -> float:
    """The uniform of (seed, row, step) in pure integer arithmetic."""
    return uniform_of_word(philox4x32((row & M32, step & M32, 0, 0), (seed & M32, (seed >> 32) & M32))[0])


def philox_uniform(seed: torch.Tensor, rows: int, step: torch.Tensor) -> torch.Tensor:
    """The same uniforms for rows 0..rows-1 as fp32 [rows], from device tensors ``seed`` [1] and
    ``step`` (nothing is read back)."""
    dev = seed.device
    r = torch.arange(rows, dtype=torch.long, device=dev)
    zero = torch.zeros_like(r)
    s = seed.reshape(()).long()
    t = torch.as_tensor(step, dtype=torch.long, device=dev).reshape(())
    word = philox4x32((r, (t & M32) + zero, zero, zero), ((s & M32) + zero, ((s >> 32) & M32) + zero))[0]
    return (word >> 8).to(torch.float32) * (2.0 ** -24)


# ----------------------------------------------------------------------------------- the rule
def process_logits_reference(logits: torch.Tensor, seen: Optional[torch.Tensor], temperature: float = 1.0,
                             top_k: int = 0, top_p: float = 1.0, repetition_penalty: float = 1.0
                             ) -> Tuple[torch.Tensor, torch.Tensor]:
    """Steps 1-4 on logits [R, V]: (processed logits x fp32 [R, V], kept mask bool [R, V]).
    ``seen`` is a bool mask [R, V] of the tokens of the decoder input, or None."""
    V = logits.shape[-1]
    x = logits.float()
    if seen is not None and repetition_penalty != 1.0:
        x = torch.where(seen, torch.where(x < 0, x * repetition_penalty, x / repetition_penalty), x)
    x = x / temperature
    x = torch.where(torch.isnan(x), torch.full_like(x, float("-inf")), x)
    keep = torch.ones_like(x, dtype=torch.bool)
    if 0 < top_k < V:
        keep = x >= torch.topk(x, top_k, dim=-1)[0][..., -1, None]
    if top_p < 1.0:
        s = torch.sort(x.masked_fill(~keep, float("-inf")), dim=-1, descending=False)[0]
        remove = s.softmax(dim=-1).cumsum(dim=-1) <= (1 - top_p)
        remove[..., -1] = False
        thr = torch.where(remove, torch.full_like(s, float("inf")), s).min(-1, keepdim=True)[0]
        keep = keep & (x >= thr)
    return x, keep


def draw_reference(x: torch.Tensor, keep: torch.Tensor, u: torch.Tensor) -> torch.Tensor:
    """Step 5 on processed logits [R, V] and their kept mask, weights in fp64: tokens int64 [R]."""
    V = x.shape[-1]
    m = x.max(-1, keepdim=True)[0]
    ok = torch.isfinite(m)
    w = torch.where(keep & ok, torch.exp((x - m).double()), torch.zeros((), dtype=torch.float64, device=x.device))
    w = torch.where(torch.isnan(w), torch.zeros_like(w), w)
    C = w.cumsum(-1)
    tok = torch.searchsorted(C, u.double()[:, None] * C[:, -1:], right=True)[:, 0].clamp(max=V - 1)
    return torch.where(ok[:, 0], tok, torch.zeros_like(tok))


def seen_mask(out: torch.Tensor, pos: torch.Tensor, start_token: int, vocab: int) -> torch.Tensor:
    """bool [R, V]: the start token and the tokens in slots < pos of ``out`` [R, T]."""
    R, T = out.shape
    dev = out.device
    t = torch.as_tensor(pos, dtype=torch.long, device=dev).reshape(())
    ids = torch.cat([torch.full((R, 1), int(start_token), dtype=torch.long, device=dev), out], 1).clamp(0, vocab - 1)
    valid = (torch.arange(T + 1, device=dev) <= t).to(torch.int32)[None].expand(R, T + 1)
    return torch.zeros(R, vocab, dtype=torch.int32, device=dev).scatter_add_(1, ids, valid) > 0


def sample_step_reference(logits: torch.Tensor, out: torch.Tensor, done: torch.Tensor, cur: torch.Tensor,
                          pos: torch.Tensor, seed: torch.Tensor, start_token: int, eos: int, pad: int,
                          temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0,
                          repetition_penalty: float = 1.0, u: Optional[torch.Tensor] = None):
    """One step of the rule above.  Returns (out, done, cur, pos, u [R], thr [R], n_keep [R]) as new
    tensors; the arguments are left as they are.  ``pos`` and ``seed`` may live on the device
    (nothing here reads them back)."""
    check_sample_args(temperature, top_k, top_p, repetition_penalty)
    R, V = logits.shape
    T = out.shape[1]
    dev = logits.device
    t = torch.as_tensor(pos, dtype=torch.long, device=dev).reshape(())
    if u is None:
        u = philox_uniform(torch.as_tensor(seed, dtype=torch.long, device=dev).reshape(1), R, t)
    seen = seen_mask(out, t, start_token, V) if repetition_penalty != 1.0 else None
    x, keep = process_logits_reference(logits, seen, temperature, top_k, top_p, repetition_penalty)
    tok = draw_reference(x, keep, u)
    tok = torch.where(done, torch.full_like(tok, int(pad)), tok)
    at_t = torch.arange(T, device=dev) == t
    new_out = torch.where(at_t[None], tok[:, None], out)
    thr = torch.where(keep, x, torch.full_like(x, float("inf"))).min(-1)[0]
    return (new_out, done | (tok == eos), tok[:, None], torch.as_tensor(pos, device=dev) + 1, u.float(), thr,
            keep.sum(-1).to(torch.int32))


# --------------------------------------------------------------------------------- HIP kernel
def sample_step(logits: torch.Tensor, out: torch.Tensor, done: torch.Tensor, cur: torch.Tensor, pos: torch.Tensor,
                seed: torch.Tensor, start_token: int, eos: int, pad: int, temperature: float = 1.0, top_k: int = 0,
                top_p: float = 1.0, repetition_penalty: float = 1.0, u: Optional[torch.Tensor] = None):
    """The fused form of ``sample_step_reference`` on the GPU, in place on the caller's stream:
    reads step ``pos[0]`` and ``seed[0]`` on the device, writes the token into ``out`` [R, T] and
    ``cur`` [R, 1], updates ``done`` [R] and advances ``pos``.  An fp32 ``u`` [R] overrides Philox.
    Returns the row diagnostics (u fp32 [R], thr fp32 [R] the smallest kept processed logit,
    n_keep int32 [R] the count of processed logits >= thr)."""
    if not _pkg()._use_native(logits):
        raise RuntimeError("sample_step is a GPU kernel; use sample_step_reference on the CPU")
    check_sample_args(temperature, top_k, top_p, repetition_penalty)
    return _pkg().require_native().sample_step(logits, out, done, cur, pos, seed, int(start_token), int(eos), int(pad),
                                               float(temperature), int(top_k), float(top_p),
                                               float(repetition_penalty), u)
