"""Beam-search bookkeeping with fixed shapes and no host decision, so a decode step that ends in
it can be replayed as a graph: the rules as plain PyTorch (``beam_step_reference``,
``cache_reorder_reference``; any device, the specification) and the HIP kernels that apply the
same rules on the GPU (``beam_step``, ``CacheReorder``; csrc/beam.hip).

State of a batch of B items searched with K beams over T steps (``new_state``):

    run_seq   [B, K, T] int64   running hypotheses, pad beyond the current step
    run_score [B, K]    fp32    their summed log-probabilities; starts [0, -1e9, ...]
    fin_seq   [B, K, T] int64   finished hypotheses, best first, pad after the last token
    fin_score [B, K]    fp32    score / length**length_penalty; -1e9 for an empty slot
    fin_flag  [B, K]    bool    the slot holds a hypothesis
    unsat     [B]       bool    a running beam could still beat the worst finished one

Step t = 0 .. T-1 (L = t + 1) on logits [B * K, V]:

1. candidates log_softmax(logits)[k, v] + run_score[k] in fp32; the top 2K over (k, v) in
   descending order, a tie going to the lower flat index k * V + v;
2. candidate r continues beam idx // V with token idx % V at position t and stops when the
   token is EOS or L == T;
3. the next running set is the first K candidates that do not stop, in rank order (if fewer
   than K go on, which happens at the last step only, stopped ones follow with -1e9 added);
4. a stopped candidate of rank < K joins the finished set with score / L**length_penalty unless
   ``early_stopping`` and every slot is taken, or ``unsat`` is off; the finished set keeps the
   best K of old and new, an old entry before a new one of the same score;
5. ``unsat &= any_k(run_score[0] / L**length_penalty > (fin_flag[k] ? min(fin_score) : -1e9))``.

After T steps ``fin_seq[:, 0]`` is the result.  Once an item is blocked by rule 4 it stays
blocked, so running all T steps gives what a loop that leaves early gives.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple, Union

import torch

NEG = -1.0e9
MAX_BEAMS = 8

State = Dict[str, torch.Tensor]


def _pkg():
    from cloudtik_amd import ops
    return ops


def check_beam_args(num_beams: int, vocab: int, early_stopping=False) -> None:
    if not isinstance(num_beams, int) or not 1 <= num_beams <= MAX_BEAMS:
        raise ValueError(f"num_beams must be an integer in 1..{MAX_BEAMS}, got {num_beams!r}")
    if vocab < 2 * num_beams:
        raise ValueError(f"beam search needs a vocabulary of at least 2 * num_beams = {2 * num_beams} tokens, got {vocab}")
    if not isinstance(early_stopping, bool):
        raise ValueError(f"early_stopping must be True or False ('never' is not supported), got {early_stopping!r}")


def new_state(batch: int, num_beams: int, steps: int, pad: int, device=None) -> State:
    B, K, T = batch, num_beams, steps
    st = {
        "run_seq": torch.full((B, K, T), pad, dtype=torch.long, device=device),
        "run_score": torch.full((B, K), NEG, dtype=torch.float32, device=device),
        "fin_seq": torch.full((B, K, T), pad, dtype=torch.long, device=device),
        "fin_score": torch.full((B, K), NEG, dtype=torch.float32, device=device),
        "fin_flag": torch.zeros(B, K, dtype=torch.bool, device=device),
        "unsat": torch.ones(B, dtype=torch.bool, device=device),
    }
    st["run_score"][:, 0] = 0.0
    return st


def reset_state(st: State, pad: int) -> None:
    st["run_seq"].fill_(pad)
    st["fin_seq"].fill_(pad)
    st["run_score"].fill_(NEG)
    st["run_score"][:, 0] = 0.0
    st["fin_score"].fill_(NEG)
    st["fin_flag"].zero_()
    st["unsat"].fill_(True)


def length_penalty_table(steps: int, length_penalty: float, device=None) -> torch.Tensor:
    """[T] fp32, entry t = (t + 1) ** length_penalty computed in double and rounded once: the
    divisor of rules 4 and 5, the same number for the reference and the kernel."""
    return torch.tensor([float(L) ** float(length_penalty) for L in range(1, steps + 1)], dtype=torch.float32,
                        device=device)


def beam_step_reference(logits: torch.Tensor, state: State, t: Union[int, torch.Tensor], len_pen: torch.Tensor,
                        eos: int, early_stopping: bool = False, select: str = "sort",
                        ban: Optional[torch.Tensor] = None) -> Tuple[State, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """One step of the rules above.  Returns (new state, beam_idx [B * K] with the batch offset
    b * K added, next_tok [B * K], cand_score [B, 2K], cand_idx [B, 2K]); ``state`` is left as it
    is.  ``t`` may be a device tensor (nothing here reads it back).  ``select="topk"`` takes the
    2K candidates with ``torch.topk``, which is faster and leaves a tie across rank 2K to the
    library; "sort" is the rule.  ``ban`` bool [B * K, V] (``ops/constrain.py``) sets the candidates of
    banned tokens to -inf after the log-softmax, which still normalises over the whole row."""
    run_seq, run_score = state["run_seq"], state["run_score"]
    fin_seq, fin_score, fin_flag, unsat = state["fin_seq"], state["fin_score"], state["fin_flag"], state["unsat"]
    B, K, T = run_seq.shape
    V = logits.shape[-1]
    dev = logits.device
    t = torch.as_tensor(t, dtype=torch.long, device=dev).reshape(())
    last = t == T - 1
    at_t = torch.arange(T, device=dev) == t                                           # [T]
    L = len_pen.to(dev).index_select(0, t.reshape(1)).reshape(())       # no host read: t may live on the device

    logp = torch.log_softmax(logits.float(), -1)
    if ban is not None:
        logp = logp.masked_fill(ban, float("-inf"))
    flat = (logp.view(B, K, V) + run_score[:, :, None]).view(B, K * V)
    if select == "topk":
        s, idx = torch.topk(flat, 2 * K, dim=1)
        idx, o = torch.sort(idx, dim=1)                                               # ties inside the set
        s, o = torch.sort(s.gather(1, o), dim=1, descending=True, stable=True)
        idx = idx.gather(1, o)
    else:
        s, idx = torch.sort(flat, dim=1, descending=True, stable=True)
        s, idx = s[:, :2 * K].contiguous(), idx[:, :2 * K].contiguous()
    beam, tok = idx // V, idx % V
    stop = (tok == eos) | last
    cseq = run_seq.gather(1, beam[:, :, None].expand(B, 2 * K, T))
    cseq = torch.where(at_t, tok[:, :, None], cseq)

    # rule 3
    order = torch.sort(stop.long(), dim=1, stable=True)[1][:, :K]
    new_run_score = (s + stop.float() * NEG).gather(1, order)
    new_run_seq = cseq.gather(1, order[:, :, None].expand(B, K, T))
    beam_idx = beam.gather(1, order) + torch.arange(B, device=dev)[:, None] * K
    next_tok = tok.gather(1, order)

    # rule 4
    full = fin_flag.all(1, keepdim=True) & bool(early_stopping)
    elig = stop[:, :K] & ~full & unsat[:, None]
    merged = torch.cat([fin_score, torch.where(elig, s[:, :K] / L, torch.full_like(s[:, :K], float("-inf")))], 1)
    o = torch.sort(merged, dim=1, descending=True, stable=True)[1][:, :K]
    new_fin_score = merged.gather(1, o)
    new_fin_seq = torch.cat([fin_seq, cseq[:, :K]], 1).gather(1, o[:, :, None].expand(B, K, T))
    new_fin_flag = torch.cat([fin_flag, elig], 1).gather(1, o)

    # rule 5
    worst = torch.where(new_fin_flag, new_fin_score.min(1, keepdim=True)[0], torch.full_like(new_fin_score, NEG))
    new_unsat = unsat & (new_run_score[:, :1] / L > worst).any(1)

    new = {"run_seq": new_run_seq, "run_score": new_run_score, "fin_seq": new_fin_seq, "fin_score": new_fin_score,
           "fin_flag": new_fin_flag, "unsat": new_unsat}
    return new, beam_idx.reshape(-1), next_tok.reshape(-1), s, idx


def cache_reorder_reference(caches: Sequence[torch.Tensor], beam_idx: torch.Tensor, count: Optional[int] = None,
                            out: Optional[Sequence[torch.Tensor]] = None) -> List[torch.Tensor]:
    """Row r of every cache [R, T, ...] becomes row ``beam_idx[r]``.  With ``out`` the rows are
    written there, and with ``count`` only their first ``count`` time slots (the rest of ``out``
    is left alone)."""
    res = []
    for i, c in enumerate(caches):
        g = c.index_select(0, beam_idx)
        if out is None:
            res.append(g)
            continue
        if count is None:
            out[i].copy_(g)
        else:
            out[i][:, :count].copy_(g[:, :count])
        res.append(out[i])
    return res


# ------------------------------------------------------------------------------ HIP kernels
def beam_topk(logits: torch.Tensor, num_beams: int):
    """logits [R, V] bf16 | fp32 on the GPU -> (log-sum-exp fp32 [R], the 2K largest logits
    fp32 [R, 2K], their tokens int32 [R, 2K]) of every row, read once."""
    if not _pkg()._use_native(logits):
        raise RuntimeError("beam_topk is a GPU kernel; use beam_step_reference on the CPU")
    return _pkg().require_native().beam_topk(logits.contiguous(), int(num_beams))


def beam_step(logits: torch.Tensor, state: State, pos: torch.Tensor, arrive: torch.Tensor, len_pen: torch.Tensor,
              beam_idx: torch.Tensor, cur: torch.Tensor, eos: int, early_stopping: bool = False,
              ban_lse: Optional[torch.Tensor] = None):
    """The fused form of ``beam_step_reference`` on the GPU, in place: reads step ``pos[0]``,
    rewrites ``state``, ``beam_idx`` [B * K] and the decoder's next input ``cur`` [B * K, 1], and
    advances ``pos``.  ``arrive`` is an int32 [1] zero the kernel uses to find its last workgroup.
    Returns the step's candidates (cand_score [B, 2K], cand_idx [B, 2K]).  With ``ban_lse`` fp32
    [B * K], ``logits`` are rows masked by ``ops.constrain.logits_constrain`` and ``ban_lse`` the
    log-sum-exp of what it masked: the whole row's log-sum-exp is restored from the two."""
    if not _pkg()._use_native(logits):
        raise RuntimeError("beam_step is a GPU kernel; use beam_step_reference on the CPU")
    C = _pkg().require_native()
    K = state["run_seq"].shape[1]
    lse, val, tok = C.beam_topk(logits.contiguous(), K)
    if ban_lse is not None:
        lse = torch.logaddexp(lse, ban_lse)
    return C.beam_update(lse, val, tok, state["run_seq"], state["run_score"], state["fin_seq"], state["fin_score"],
                         state["fin_flag"], state["unsat"], len_pen, pos, arrive, beam_idx, cur,
                         int(logits.shape[-1]), int(eos), bool(early_stopping))


class CacheReorder:
    """``dst[i][r, :pos] = src[i][beam_idx[r], :pos]`` for every cache pair in one launch.  The
    caches are [R, T, H, D] bf16; their pointer table is built once, here."""

    def __init__(self, src: Sequence[torch.Tensor], dst: Sequence[torch.Tensor]):
        if not _pkg()._use_native(*src):
            raise RuntimeError("CacheReorder is a GPU kernel; use cache_reorder_reference on the CPU")
        self._plan = _pkg().require_native().BeamCachePlan(list(src), list(dst))

    def __call__(self, beam_idx: torch.Tensor, pos: torch.Tensor) -> None:
        self._plan.run(beam_idx, pos)
