"""History-dependent token bans with fixed shapes and no host decision, so a decode step that uses
them can be replayed as a graph: the rule as plain PyTorch (``constrain_reference``; any device, the
specification) and the HIP kernel that applies the same rule on the GPU (``logits_constrain``;
csrc/constrain.hip).  They are the ``no_repeat_ngram_size``, ``bad_words_ids`` and ``min_length`` /
``min_new_tokens`` logits processors of HF ``generate``.

The rule, for one row at step ``t`` (0-based) with logits ``l[0..V)`` (bf16 or fp32) and the row's
decoder input so far ``h = [start_token] + hist[r, :t]``, of length ``t + 1``.  The start token
counts, and so does a pad written after EOS, as in HF ``generate``, which works on the same
``input_ids``.  The ban set S is the union of

* n-gram, ``no_repeat_ngram_size = n >= 1``: for every i in 0 .. t + 1 - n, if
  ``h[i : i+n-1] == h[t+2-n : t+1]`` (the last n - 1 tokens), ban ``h[i+n-1]``.  The range is empty
  while ``t + 1 < n``; ``n = 1`` bans every token of h.
* bad words: a word w of m >= 1 tokens bans ``w[-1]`` if ``m - 1 <= t + 1`` and
  ``h[t+2-m : t+1] == w[:-1]``.  A one-token word is always banned.  (With ``m - 1 == t + 1`` the
  whole of h, start token included, is the word's prefix; the library skips that one case.)
* minimum length: if ``t < min_new``, ban EOS.

A history token outside [0, V) equals nothing, itself included, and bans nothing.

Outputs: ``x[v] = -inf`` for v in S and ``l[v]`` unchanged otherwise (the library's mask value),
and ``ban_lse = log(sum over the distinct v in S of exp(l[v]))`` in fp32, from the values before
masking: -inf for an empty S, and a token banned for two reasons counts once.

Use.  Greedy decoding takes the arg-max of x.  Sampling takes x as the row of the sampling rule
(``ops/sampling.py``): the bans depend on the history only and a penalised or scaled -inf stays
-inf, so banning first gives what the library's processor order gives.  Beam search masks after
``log_softmax`` as the library does: rule 1 of ``ops/beam.py`` becomes ``log_softmax(l)[v] +
run_score`` for v outside S and -inf inside, the log-sum-exp still over the whole row; the fused
path takes the top 2K of x and restores that log-sum-exp as ``logaddexp(lse(x), ban_lse)``.  The
history of beam row ``b * K + k`` is ``run_seq[b, k]``, already gathered by source beam.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import torch

MAX_STEPS = 1024              # the kernel's caps (csrc/constrain.hip): history slots of a row,
MAX_WORDS = 1024              # bad words,
MAX_WORD_TOKENS = 2048        # and their tokens in all

Rule = Tuple[int, int, Tuple[Tuple[int, ...], ...]]     # (n, min_new, words)


def _pkg():
    from cloudtik_amd import ops
    return ops


def _count(v, name):
    if not isinstance(v, int) or isinstance(v, bool) or v < 0:
        raise ValueError(f"{name} must be an integer >= 0, got {v!r}")
    return v


def check_constrain_args(no_repeat_ngram_size=0, min_new_tokens=0, min_length=0, bad_words_ids=None,
                         vocab: Optional[int] = None, eos: Optional[int] = None, num_beams: int = 1,
                         max_new_tokens: Optional[int] = None) -> Optional[Rule]:
    """Raises ValueError for arguments the rule does not take.  Returns the frozen rule
    ``(n, min_new, words)``, hashable, with ``min_new = max(min_new_tokens, min_length - 1)``
    (``min_length`` counts the start token, as in the library), or None when nothing is on."""
    n = _count(no_repeat_ngram_size, "no_repeat_ngram_size")
    min_new = max(_count(min_new_tokens, "min_new_tokens"), _count(min_length, "min_length") - 1)
    words = []
    if bad_words_ids is not None:
        if not isinstance(bad_words_ids, (list, tuple)):
            raise ValueError(f"bad_words_ids must be a list of non-empty lists of token ids, got {bad_words_ids!r}")
        for w in bad_words_ids:
            if not isinstance(w, (list, tuple)) or len(w) == 0 or \
                    not all(isinstance(v, int) and not isinstance(v, bool) for v in w):
                raise ValueError(f"bad_words_ids must be a list of non-empty lists of token ids, got {w!r}")
            if vocab is not None and not all(0 <= v < vocab for v in w):
                raise ValueError(f"bad_words_ids holds a token outside the vocabulary [0, {vocab}): {list(w)!r}")
            if eos is not None and list(w) == [eos]:
                raise ValueError(f"bad_words_ids bans the EOS token {[eos]!r} for good: use min_new_tokens")
            words.append(tuple(w))
        if len(words) > MAX_WORDS:
            raise ValueError(f"bad_words_ids holds {len(words)} words; at most {MAX_WORDS} are supported")
        if sum(len(w) for w in words) > MAX_WORD_TOKENS:
            raise ValueError(f"bad_words_ids holds {sum(len(w) for w in words)} tokens in all; at most "
                             f"{MAX_WORD_TOKENS} are supported")
    if n == 0 and min_new == 0 and not words:
        return None
    if max_new_tokens is not None and max_new_tokens > MAX_STEPS:
        raise ValueError(f"no_repeat_ngram_size, min_length and bad_words_ids support max_new_tokens <= {MAX_STEPS}, "
                         f"got {max_new_tokens}")
    if num_beams > 1 and vocab is not None and max_new_tokens is not None:
        # a row bans at most t + 1 <= max_new_tokens history tokens, one per word and EOS, so it keeps
        # 2K finite candidates and no rank is decided by a tie among -inf
        need = 2 * num_beams + max_new_tokens + 1 + len(words)
        if vocab < need:
            raise ValueError(f"beam search with no_repeat_ngram_size, min_length or bad_words_ids needs a vocabulary "
                             f"of at least 2 * num_beams + max_new_tokens + 1 + len(bad_words_ids) = {need} tokens, "
                             f"got {vocab}")
    return n, min_new, tuple(words)


# ----------------------------------------------------------------------------------- the rule
def ban_mask_reference(hist: torch.Tensor, pos, vocab: int, start_token: int, no_repeat_ngram_size: int = 0,
                       min_new: int = 0, eos: int = -1, bad_words: Sequence[Sequence[int]] = ()) -> torch.Tensor:
    """The ban set of every row as bool [R, V].  ``hist`` [R, T] int64 holds the tokens written so
    far in slots < ``pos``; later slots are not looked at.  ``pos`` is read on the host."""
    R, T = hist.shape
    dev = hist.device
    V, n = int(vocab), int(no_repeat_ngram_size)
    t = int(pos)
    hits = torch.zeros(R, V, dtype=torch.int32, device=dev)
    if not 0 <= t < T:
        return hits > 0
    h = torch.cat([torch.full((R, 1), int(start_token), dtype=torch.long, device=dev), hist[:, :t].long()], 1)
    valid = (h >= 0) & (h < V)
    L = t + 1
    if n >= 1 and L >= n:
        cnt = L - n + 1
        if n == 1:
            hit = torch.ones(R, cnt, dtype=torch.bool, device=dev)
        else:
            suffix, ok = h[:, L - (n - 1):], valid[:, L - (n - 1):].all(1)
            hit = (h.unfold(1, n - 1, 1)[:, :cnt] == suffix[:, None, :]).all(-1) & ok[:, None]
        hit = hit & valid[:, n - 1:]
        hits.scatter_add_(1, h[:, n - 1:].clamp(0, V - 1), hit.to(torch.int32))
    for w in bad_words:
        m = len(w)
        last = int(w[-1])
        if m - 1 > L or not 0 <= last < V:
            continue
        if m == 1:
            hits[:, last] += 1
        else:
            prefix = torch.tensor(list(w[:-1]), dtype=torch.long, device=dev)
            tail = h[:, L - (m - 1):]
            hits[:, last] += ((tail == prefix[None]) & valid[:, L - (m - 1):]).all(1).to(torch.int32)
    if t < int(min_new) and 0 <= int(eos) < V:
        hits[:, int(eos)] += 1
    return hits > 0


def constrain_reference(logits: torch.Tensor, hist: torch.Tensor, pos, start_token: int,
                        no_repeat_ngram_size: int = 0, min_new: int = 0, eos: int = -1,
                        bad_words: Sequence[Sequence[int]] = ()) -> Tuple[torch.Tensor, torch.Tensor]:
    """The rule above on logits [R, V]: (x in the dtype of ``logits``, ban_lse fp32 [R]) as new
    tensors."""
    ban = ban_mask_reference(hist, pos, logits.shape[-1], start_token, no_repeat_ngram_size, min_new, eos, bad_words)
    neg = torch.full((), float("-inf"), dtype=torch.float32, device=logits.device)
    ban_lse = torch.logsumexp(torch.where(ban, logits.float(), neg), -1)
    return logits.masked_fill(ban, float("-inf")), ban_lse


# --------------------------------------------------------------------------------- HIP kernel
def word_tables(bad_words: Sequence[Sequence[int]], device) -> Tuple[Optional[torch.Tensor], Optional[torch.Tensor]]:
    """The kernel's form of the bad words, built once: (tokens int32 [sum m], offsets int32
    [words + 1]) on ``device``, or (None, None) without words."""
    if not bad_words:
        return None, None
    tok = [int(v) for w in bad_words for v in w]
    off = [0]
    for w in bad_words:
        off.append(off[-1] + len(w))
    if len(bad_words) > MAX_WORDS or len(tok) > MAX_WORD_TOKENS or any(len(w) == 0 for w in bad_words):
        raise ValueError(f"at most {MAX_WORDS} non-empty words of {MAX_WORD_TOKENS} tokens in all are supported")
    return (torch.tensor(tok, dtype=torch.int32, device=device), torch.tensor(off, dtype=torch.int32, device=device))


def logits_constrain(logits: torch.Tensor, hist: torch.Tensor, pos: torch.Tensor, start_token: int,
                     no_repeat_ngram_size: int = 0, min_new: int = 0, eos: int = -1,
                     tables: Tuple[Optional[torch.Tensor], Optional[torch.Tensor]] = (None, None),
                     ban_lse: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The kernel form of ``constrain_reference`` on the GPU, in place on the caller's stream:
    reads step ``pos[0]`` on the device, stores -inf into the banned entries of ``logits`` [R, V]
    (contiguous bf16 or fp32) and, when given, writes ``ban_lse`` fp32 [R].  ``tables`` comes from
    ``word_tables``.  One launch, no host read, no allocation.  Returns ``logits``."""
    if not _pkg()._use_native(logits):
        raise RuntimeError("logits_constrain is a GPU kernel; use constrain_reference on the CPU")
    _pkg().require_native().logits_constrain(logits, hist, pos, int(start_token), int(no_repeat_ngram_size),
                                             int(min_new), int(eos), tables[0], tables[1], ban_lse)
    return logits


class Constrainer:
    """A frozen rule (``check_constrain_args``) bound to a model's start and EOS tokens and a device:
    the kernel on the GPU, the reference on the CPU.  The bad-word tables are built once, here, and
    live as long as this object, which a captured graph's owner keeps."""

    def __init__(self, rule: Rule, start_token: int, eos: int, device):
        self.n, self.min_new, self.words = rule
        self.start_token, self.eos = int(start_token), int(eos)
        self.tables = word_tables(self.words, device) if torch.device(device).type == "cuda" else (None, None)

    def __call__(self, logits: torch.Tensor, hist: torch.Tensor, pos, ban_lse: Optional[torch.Tensor] = None):
        """The masked logits [R, V]: ``logits`` itself, masked in place, on the GPU (``pos`` is an
        int64 [1] tensor there), a new tensor on the CPU.  ``ban_lse`` fp32 [R] is filled when given."""
        if logits.is_cuda:
            return logits_constrain(logits, hist, pos, self.start_token, self.n, self.min_new, self.eos, self.tables,
                                    ban_lse)
        x, lse = constrain_reference(logits, hist, pos, self.start_token, self.n, self.min_new, self.eos, self.words)
        if ban_lse is not None:
            ban_lse.copy_(lse)
        return x

    def ban_mask(self, logits: torch.Tensor, hist: torch.Tensor, pos) -> torch.Tensor:
        """The ban set as bool [R, V], for ``beam_step_reference``; ``logits`` is left as it is.  On
        the GPU it is read off a copy the kernel masked."""
        if logits.is_cuda:
            masked = self(logits.clone(), hist, pos)
            return torch.isneginf(masked) & ~torch.isneginf(logits)
        return ban_mask_reference(hist, pos, logits.shape[-1], self.start_token, self.n, self.min_new, self.eos,
                                  self.words)
