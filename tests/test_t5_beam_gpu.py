"""Beam-search kernels (csrc/beam.hip) against the PyTorch rules (ops/beam.py): the fused step on
synthetic states, the cache reorder bit for bit, and graph-replayed ``generate(num_beams=K)``
against the reference loop on the same static-cache step."""
import pytest
import torch

from cloudtik_amd.models.t5 import T5Config, T5ForConditionalGeneration
from cloudtik_amd.ops import beam as beam_ops

pytestmark = pytest.mark.gpu

EOS, PAD, T = 1, 0, 6
KINDS = ("step0", "middle", "full_early", "unsat_false", "last")
MARGIN = 1e-3


def make_case(V, K, B, dtype, kind, seed):
    """(logits [B * K, V], state, t, early_stopping) on the CPU.  Logits: N(0, 0.5) with 2K + 1
    tokens per row lifted to distinct multiples of 0.25 above it, so a row's best candidates are
    apart by construction and rows differ by their real-valued score offsets."""
    g = torch.Generator().manual_seed(seed)
    R, nb = B * K, min(2 * K + 1, V)
    c0 = 3.0 if V > 64 else -2.0                    # a small vocabulary: keep log-sum-exp, and so the scores, O(1)
    logits = torch.randn(R, V, generator=g) * 0.5 + (0.0 if V > 64 else -6.0)
    for r in range(R):
        toks = torch.randperm(V - 2, generator=g)[:nb] + 2 if V - 2 >= nb else torch.randperm(V, generator=g)[:nb]
        logits[r, toks] = c0 + 0.25 * torch.randperm(nb, generator=g).float()
    t = {"step0": 0, "middle": 2, "full_early": 3, "unsat_false": 3, "last": T - 1}[kind]
    st = beam_ops.new_state(B, K, T, PAD)
    if kind != "step0":
        st["run_seq"][:, :, :t] = torch.randint(2, V, (B, K, t), generator=g)
        st["run_score"] = -(3 + 0.5 * torch.rand(B, K, generator=g)).sort(1)[0]
        # EOS first in every other beam and second in the rest, between the lifted levels
        for r in range(R):
            logits[r, EOS] = c0 + 0.125 + 0.25 * (nb if r % 2 == 0 else nb - 2)
        n_fin = K if kind in ("full_early", "unsat_false") else K // 2
        for b in range(B):
            for k in range(n_fin):
                n = int(torch.randint(1, t + 1, (1,), generator=g))
                st["fin_seq"][b, k, :n] = torch.randint(2, V, (n,), generator=g)
                st["fin_seq"][b, k, n - 1] = EOS
            st["fin_score"][b, :n_fin] = -(1 + 4 * torch.rand(n_fin, generator=g)).sort()[0]
            st["fin_flag"][b, :n_fin] = True
        if kind == "unsat_false":
            st["unsat"][:] = False
            if B > 1:
                st["unsat"][B - 1] = True          # one item still open next to closed ones
    return logits.to(dtype), st, t, kind == "full_early"


def _close(got, want):
    got, want = got.float().cpu(), want.float().cpu()
    assert ((got - want).abs() <= 1e-5 * want.abs()).all(), (got, want)


def _margin(logits, st, K):
    """Smallest gap between adjacent candidates among the reference's top 2K + 1."""
    B, V = st["run_score"].shape[0], logits.shape[-1]
    flat = (torch.log_softmax(logits.float(), -1).view(B, K, V) + st["run_score"][:, :, None]).view(B, -1)
    top = flat.topk(min(2 * K + 1, flat.shape[1]), dim=1)[0]
    return float((top[:, :-1] - top[:, 1:]).min())


def _preconditions(logits, st, K, kind, want, w_cs, w_ci):
    """What a case must show, judged on the reference alone: no two of the best 2K + 1 candidates
    within the margin (a tie would let either order pass), scores away from 0 (where a relative
    bound means nothing), and the situation the case is named after."""
    V = logits.shape[-1]
    ok = _margin(logits, st, K) > MARGIN and float(w_cs.abs().min()) > 0.5
    if kind == "middle" and K >= 2:
        stop = (w_ci % V) == EOS
        ok = ok and bool(stop[:, :K].any() and stop[:, K:].any())      # EOS below and at or above rank K
    if kind == "last":
        ok = ok and bool((want["fin_flag"].sum(1) > st["fin_flag"].sum(1)).all())
    return ok


# V: the T5 vocabulary; an odd size, so rows start off the 16-byte grid and end in a tail; 2K at K = 8
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("K", [1, 2, 4, 8])
@pytest.mark.parametrize("V", [32128, 1003, 16])
def test_fused_step_matches_reference(cuda, V, K, B, dtype):
    len_pen = beam_ops.length_penalty_table(T, 0.6, cuda)
    for kind in KINDS:
        for attempt in range(40):                  # the first seed whose reference meets the preconditions
            logits, st, t, early = make_case(V, K, B, dtype, kind, 1000 * KINDS.index(kind) + V + 10 * K + B + attempt)
            logits = logits.to(cuda)
            st = {k: v.to(cuda) for k, v in st.items()}
            want, w_idx, w_tok, w_cs, w_ci = beam_ops.beam_step_reference(logits, st, t, len_pen, EOS, early)
            if _preconditions(logits, st, K, kind, want, w_cs, w_ci):
                break
        assert _preconditions(logits, st, K, kind, want, w_cs, w_ci), (kind, _margin(logits, st, K))
        assert _margin(logits, st, K) > MARGIN

        pos = torch.tensor([t], device=cuda)
        arrive = torch.zeros(1, dtype=torch.int32, device=cuda)
        beam_idx = torch.full((B * K,), -1, device=cuda)
        cur = torch.full((B * K, 1), -1, device=cuda)
        got = {k: v.clone() for k, v in st.items()}
        cs, ci = beam_ops.beam_step(logits, got, pos, arrive, len_pen, beam_idx, cur, EOS, early)
        assert int(pos) == t + 1 and int(arrive) == 0
        assert torch.equal(ci, w_ci), kind
        assert torch.equal(beam_idx, w_idx) and torch.equal(cur[:, 0], w_tok), kind
        for name in ("run_seq", "fin_seq", "fin_flag", "unsat"):
            assert torch.equal(got[name], want[name]), (kind, name)
        _close(cs, w_cs)
        _close(got["run_score"], want["run_score"])
        _close(got["fin_score"], want["fin_score"])


def test_topk_rows(cuda):
    """``beam_topk`` alone: rows off the 16-byte grid, a row shorter than one vector, -inf entries,
    and exact ties (plenty in bf16), which go to the lower token."""
    g = torch.Generator().manual_seed(7)
    for dtype, V in ((torch.bfloat16, 1003), (torch.float32, 1001), (torch.bfloat16, 17), (torch.float32, 8)):
        x = torch.randn(5, V, generator=g).to(dtype)
        x[2, 5] = float("-inf")
        x[3, V - 1] = x[3].max()                                   # a tie for first place, the later one in the tail
        lse, val, tok = beam_ops.beam_topk(x.to(cuda), 4)
        torch.testing.assert_close(lse.cpu(), torch.logsumexp(x.float(), 1), rtol=1e-5, atol=1e-6)
        w_val, w_tok = torch.sort(x.float(), dim=1, descending=True, stable=True)
        assert torch.equal(tok.cpu().long(), w_tok[:, :8]), (dtype, V)
        assert torch.equal(val.cpu(), w_val[:, :8])


def test_binding_checks(cuda):
    x = torch.zeros(4, 32, device=cuda)
    with pytest.raises(RuntimeError, match="num_beams"):
        beam_ops.beam_topk(x, 9)
    with pytest.raises(RuntimeError, match="vocabulary"):
        beam_ops.beam_topk(x[:, :6].contiguous(), 4)
    with pytest.raises(RuntimeError, match="bf16 or fp32"):
        beam_ops.beam_topk(x.half(), 2)
    st = {k: v.to(cuda) for k, v in beam_ops.new_state(2, 2, T, PAD).items()}
    args = dict(pos=torch.zeros(1, dtype=torch.long, device=cuda), arrive=torch.zeros(1, dtype=torch.int32, device=cuda),
                len_pen=beam_ops.length_penalty_table(T, 1.0, cuda), beam_idx=torch.zeros(4, dtype=torch.long, device=cuda),
                cur=torch.zeros(4, 1, dtype=torch.long, device=cuda), eos=EOS)
    with pytest.raises(RuntimeError, match="beam_idx"):
        beam_ops.beam_step(x, st, **{**args, "beam_idx": args["beam_idx"][:3]})
    with pytest.raises(RuntimeError, match="len_pen"):
        beam_ops.beam_step(x, st, **{**args, "len_pen": args["len_pen"][:3]})
    with pytest.raises(RuntimeError, match="lse"):
        beam_ops.beam_step(x[:2], st, **args)
    a = [torch.zeros(6, 10, 8, 64, dtype=torch.bfloat16, device=cuda) for _ in range(2)]
    with pytest.raises(RuntimeError, match="in place"):
        beam_ops.CacheReorder(a, a)
    with pytest.raises(RuntimeError, match="cache"):
        beam_ops.CacheReorder(a, [t.float() for t in a])


# ------------------------------------------------------------------------------ cache reorder
@pytest.mark.parametrize("count", [0, 9])
@pytest.mark.parametrize("index", ["identity", "permutation", "duplicates"])
def test_cache_reorder_bit_equal(cuda, index, count):
    R, Tc, H, D = 6, 10, 8, 64
    g = torch.Generator().manual_seed(11)
    src = [torch.randn(R, Tc, H, D, generator=g).to(torch.bfloat16).to(cuda) for _ in range(4)]   # 2 layers, K and V
    dst = [torch.randn(R, Tc, H, D, generator=g).to(torch.bfloat16).to(cuda) for _ in range(4)]
    before = [d.clone() for d in dst]
    idx = {"identity": [0, 1, 2, 3, 4, 5], "permutation": [4, 2, 5, 0, 1, 3], "duplicates": [1, 1, 1, 3, 3, 5]}[index]
    idx = torch.tensor(idx, device=cuda)
    beam_ops.CacheReorder(src, dst)(idx, torch.tensor([count], device=cuda))
    want = beam_ops.cache_reorder_reference(src, idx, count=count, out=[b.clone() for b in before])
    for d, w, b, s in zip(dst, want, before, src):
        assert torch.equal(d.view(torch.int16), w.view(torch.int16))
        assert torch.equal(d[:, count:].view(torch.int16), b[:, count:].view(torch.int16))     # later slots untouched
        assert torch.equal(d[:, :count].view(torch.int16), s.index_select(0, idx)[:, :count].view(torch.int16))


# --------------------------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def small(cuda):
    torch.manual_seed(0)
    return T5ForConditionalGeneration(T5Config.small(dropout_rate=0.0), device=cuda).eval()


def _batch(seed, cuda):
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(2, 32128, (3, 24), generator=g).to(cuda)
    mask = torch.ones(3, 24, dtype=torch.long, device=cuda)
    mask[1, 17:] = 0
    return x, mask


def _trace_margin(trace):
    return min(float((c[:, :-1] - c[:, 1:]).min()) for c in trace)


# inputs for which the reference loop's candidates stay apart at every step; measured on the MI355X.
# Few do: a row of bf16 logits repeats values near its top (a quarter of the seeds pass at K = 2, one
# in a hundred at K = 4).  The test re-checks the margin and moves on to the next seed if it fails.
E2E_SEEDS = {2: (0, 3, 4, 7, 8, 12), 4: (128, 216, 532, 543, 591, 636, 733)}


@pytest.mark.parametrize("early", [True, False])
@pytest.mark.parametrize("K", [2, 4])
def test_graph_generate_matches_reference_loop(cuda, small, K, early):
    steps, calls = 10, 0
    for seed in E2E_SEEDS[K]:
        x, mask = _batch(seed, cuda)
        trace = []
        w_seq, w_score = small._generate_beam_static(x, mask, steps, K, 1.0, early, fused=False, graph=False, trace=trace)
        assert len(trace) == steps and trace[0].shape == (3, 2 * K)
        if _trace_margin(trace) <= MARGIN:         # two candidates too close: not an input for this test
            continue
        seq, score = small.generate(x, mask, max_new_tokens=steps, num_beams=K, early_stopping=early, return_scores=True)
        assert seq.shape == (3, steps) and seq.dtype == torch.long and score.shape == (3,)
        assert torch.equal(seq, w_seq), seed
        torch.testing.assert_close(score, w_score, rtol=1e-4, atol=0)
        graphs = [k for k in small._graphs if k[0] == "beam" and k[6] == K and k[8] == early and k[9] and k[10]]
        assert len(graphs) == 1                    # a later call replays the first call's capture
        calls += 1
        if calls == 2:
            break
    assert calls == 2, "fewer than two inputs with candidates apart by the margin"
