"""The token-ban kernel (csrc/constrain.hip) against the PyTorch rule (ops/constrain.py) computed
on the CPU: every dispatch edge of the grid bit for bit, the duplicate-ban log-sum-exp, canaries
around what it may read and write, launches repeated and replayed in a graph; the beam and sampling
kernels on the masked rows it leaves; and ``generate`` with constraints, graph against eager, on the
small bf16 model."""
import pytest
import torch

from cloudtik_amd.models.t5 import T5Config, T5ForConditionalGeneration
from cloudtik_amd.ops import beam as beam_ops
from cloudtik_amd.ops import constrain as C
from cloudtik_amd.ops import sampling as sample_ops

from test_t5_beam_gpu import MARGIN, _close

pytestmark = pytest.mark.gpu

START, EOS, PAD = 0, 1, 0
NEG_INF = float("-inf")
WORDS = ((7,), (2, 3), (3, 2, 4), (5, 5, 2, 9))        # lengths 1 .. 4; (2, 3) ends in a token n-grams ban too
TOP = 10                                               # tokens TOP .. TOP + 4 hold the rows' arg-max; nothing bans them
DEVIATION = [0.0]                                      # the largest relative ban_lse deviation seen, printed


def _bits(x):
    return x.view(torch.int16) if x.dtype == torch.bfloat16 else x.view(torch.int32)


def _case(V, R, T, t, dtype, seed):
    """(logits [R + 2, V] with a guard row at either end, hist [R, T]) on the CPU.  Logits N(-6, 0.5):
    a ban_lse of a few of them stays away from 0, where a relative bound means nothing.  History from
    4 symbols so n-grams recur; every slot >= t holds the row's arg-max token, which nothing bans:
    a kernel that read one would ban it with n = 1.  Slots < t hold an out-of-range token in two rows."""
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(R + 2, V, generator=g) * 0.5 - 6.0
    top = TOP + torch.arange(R + 2) % 5
    logits[torch.arange(R + 2), top] = 3.0
    hist = torch.randint(2, 6, (R, T), generator=g)
    hist[:, t:] = top[1:R + 1, None]
    if t >= 2:
        hist[0, 0] = -1
        hist[R - 1, 1] = V
    return logits.to(dtype), hist


def _check_lse(got, want):
    got, want = got.float().cpu(), want.float().cpu()
    empty = torch.isneginf(want)
    assert torch.equal(torch.isneginf(got), empty), (got, want)
    if bool((~empty).any()):
        _close(got[~empty], want[~empty])
        DEVIATION[0] = max(DEVIATION[0], float(((got[~empty] - want[~empty]).abs() / want[~empty].abs()).max()))


def _run(cuda, logits, hist, t, n, min_new, words, with_lse=True):
    """One launch on rows 1 .. R of ``logits``: (all rows back on the CPU, ban_lse)."""
    R = hist.shape[0]
    buf = logits.to(cuda)
    lse = torch.full((R,), float("nan"), device=cuda) if with_lse else None
    got = C.logits_constrain(buf[1:R + 1], hist.to(cuda), torch.tensor([t], device=cuda), START, n, min_new, EOS,
                             C.word_tables(words, cuda), lse)
    assert got.data_ptr() == buf[1:R + 1].data_ptr()
    return buf.cpu(), (lse.cpu() if with_lse else None)


# V: below a wave and below beam_topk's 256 threads; odd row strides; the T5 vocabulary
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("V", [24, 1003, 32128])
def test_kernel_matches_reference(cuda, V, dtype):
    cases = 0
    for R in (1, 5, 64):
        for T in (1, 8, 200):
            for n in (0, 1, 3):
                steps = sorted({min(max(t, 0), T - 1) for t in (0, n - 2, n - 1, n, T // 2, T - 1)})
                for t in steps:
                    min_new = T // 2 + 1                   # EOS is banned in the first half of the steps
                    words = WORDS if (R + T + n + t) % 2 == 0 else ()
                    logits, hist = _case(V, R, T, t, dtype, 7 * V + 31 * R + T + 1000 * n + t)
                    x, lse = C.constrain_reference(logits[1:R + 1], hist, t, START, n, min_new, EOS, words)
                    assert torch.equal(x.argmax(-1), logits[1:R + 1].argmax(-1))      # the canary token stays
                    got, got_lse = _run(cuda, logits, hist, t, n, min_new, words)
                    assert torch.equal(_bits(got[1:R + 1]), _bits(x)), (R, T, n, t)
                    assert torch.equal(_bits(got[0]), _bits(logits[0])) and torch.equal(_bits(got[-1]), _bits(logits[-1]))
                    _check_lse(got_lse, lse)
                    again, again_lse = _run(cuda, logits, hist, t, n, min_new, words)
                    assert torch.equal(_bits(again), _bits(got)) and torch.equal(again_lse.view(torch.int32),
                                                                                got_lse.view(torch.int32))
                    cases += 1
    print(f"V={V} {dtype}: {cases} launches checked, largest relative ban_lse deviation so far {DEVIATION[0]:.3e}")


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("V", [24, 1003])
def test_rule_parts_and_every_word_length(cuda, V, dtype):
    """Each part alone and all together on hand-built histories where every word bites."""
    T = 8
    hist = torch.tensor([[2, 3, 2, 4, 5, 5, 2, 2],          # t = 3: (3, 2, 4) bites; t = 7: (5, 5, 2, 9)
                         [3, 2, 3, 2, 3, 2, 3, 2],          # (2, 3) bites wherever the last token is 2
                         [0, 4, 0, 4, 0, 4, 0, 4]])         # interior start tokens
    g = torch.Generator().manual_seed(V)
    logits = (torch.randn(5, V, generator=g) * 0.5 - 6.0).to(dtype)
    bitten = set()
    for t in range(T):
        for n, min_new, words in ((2, 0, ()), (0, 0, WORDS), (0, 5, ()), (3, 5, WORDS), (1, 0, WORDS)):
            x, lse = C.constrain_reference(logits[1:4], hist, t, START, n, min_new, EOS, words)
            got, got_lse = _run(cuda, logits, hist, t, n, min_new, words)
            assert torch.equal(_bits(got[1:4]), _bits(x)), (t, n, min_new)
            assert torch.equal(_bits(got[0]), _bits(logits[0])) and torch.equal(_bits(got[4]), _bits(logits[4]))
            _check_lse(got_lse, lse)
            no_lse, _ = _run(cuda, logits, hist, t, n, min_new, words, with_lse=False)
            assert torch.equal(_bits(no_lse), _bits(got))
            if n == 0 and min_new == 0:
                for w in WORDS:
                    if bool(torch.isneginf(x[:, w[-1]].float()).any()):
                        bitten.add(len(w))
    assert bitten == {1, 2, 3, 4}


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("V", [24, 1003, 32128])
def test_token_banned_three_times_counts_once(cuda, V, dtype):
    """EOS banned by the n-gram rule, a word and the minimum length at once, on rows where it holds
    nearly all the mass: counted twice, ban_lse would be off by log 2."""
    hist = torch.tensor([[7, EOS, 7, 9], [7, EOS, 7, 9]])
    logits = torch.full((4, V), -6.0)
    logits[:, EOS] = 5.0
    logits[2, 7] = 4.0                                         # row 1 of the call: two tokens of weight
    logits = logits.to(dtype)
    words = ((7, EOS), (8,))
    x, lse = C.constrain_reference(logits[1:3], hist, 3, START, 2, 10, EOS, words)
    assert torch.isneginf(x[:, EOS].float()).all() and torch.isneginf(x[:, 8].float()).all()
    exact = torch.logsumexp(torch.stack([logits[1:3, EOS], logits[1:3, 8]], 1).double(), 1)
    assert (lse.double() - exact).abs().max() < 1e-5 and float(lse[0]) < 5.01
    got, got_lse = _run(cuda, logits, hist, 3, 2, 10, words)
    assert torch.equal(_bits(got[1:3]), _bits(x))
    _check_lse(got_lse, lse)
    # n = 1: every occurrence of 7 is listed, and counted once
    x, lse = C.constrain_reference(logits[1:3], hist, 3, START, 1, 10, EOS, words)
    got, got_lse = _run(cuda, logits, hist, 3, 1, 10, words)
    assert torch.equal(_bits(got[1:3]), _bits(x))
    _check_lse(got_lse, lse)


def test_empty_set_and_step_out_of_range(cuda):
    logits = torch.randn(3, 40)
    hist = torch.full((1, 4), 5)
    got, lse = _run(cuda, logits, hist, 2, 3, 0, ())           # (5, 5) has not been followed by anything yet
    want, want_lse = C.constrain_reference(logits[1:2], hist, 2, START, 3, 0, EOS, ())
    assert torch.equal(got[1:2], want) and torch.equal(got, logits) and float(lse[0]) == NEG_INF == float(want_lse[0])
    for t in (4, 5, -1):                                       # no such step: nothing is read or written
        got, lse = _run(cuda, logits, hist, t, 1, 9, WORDS)
        assert torch.equal(got, logits) and float(lse[0]) == NEG_INF


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("V,T", [(24, 8), (1003, 8), (32128, 200)])
def test_graph_replay_is_bit_identical(cuda, V, T, dtype):
    """The launch captured once and replayed for t = 0 .. T - 1, the step read from the device, gives
    the bits of the one-shot launches, which are the reference's."""
    R, n, min_new = 5, 3, T // 2
    g = torch.Generator().manual_seed(V + T)
    src = (torch.randn(R, V, generator=g) * 0.5 - 6.0).to(dtype)
    hist = torch.randint(2, 6, (R, T), generator=g)
    one_shot = []
    for t in range(T):
        x, lse = C.constrain_reference(src, hist, t, START, n, min_new, EOS, WORDS)
        got, got_lse = _run(cuda, torch.cat([src[:1], src, src[:1]]), hist, t, n, min_new, WORDS)
        assert torch.equal(_bits(got[1:R + 1]), _bits(x)), t
        _check_lse(got_lse, lse)
        one_shot.append((got[1:R + 1], got_lse))

    src_d, hist_d = src.to(cuda), hist.to(cuda)
    work = torch.empty_like(src_d)
    lse_d = torch.empty(R, device=cuda)
    pos = torch.zeros(1, dtype=torch.long, device=cuda)
    tables = C.word_tables(WORDS, cuda)

    def step():
        work.copy_(src_d)
        C.logits_constrain(work, hist_d, pos, START, n, min_new, EOS, tables, lse_d)
        pos.add_(1)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    pos.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    pos.zero_()
    for t in range(T):
        graph.replay()
        assert torch.equal(_bits(work.cpu()), _bits(one_shot[t][0])), t
        assert torch.equal(lse_d.cpu().view(torch.int32), one_shot[t][1].view(torch.int32)), t
    assert int(pos) == T


def test_binding_checks(cuda):
    x = torch.zeros(4, 32, device=cuda)
    hist = torch.zeros(4, 6, dtype=torch.long, device=cuda)
    pos = torch.zeros(1, dtype=torch.long, device=cuda)
    C.logits_constrain(x, hist, pos, START, 2, 0, EOS)
    with pytest.raises(RuntimeError, match="bf16 or fp32"):
        C.logits_constrain(x.half(), hist, pos, START, 2, 0, EOS)
    with pytest.raises(RuntimeError, match="contiguous"):
        C.logits_constrain(x.t().contiguous().t(), hist, pos, START, 2, 0, EOS)
    with pytest.raises(RuntimeError, match="hist"):
        C.logits_constrain(x, hist[:3], pos, START, 2, 0, EOS)
    with pytest.raises(RuntimeError, match="hist"):
        C.logits_constrain(x, hist.int(), pos, START, 2, 0, EOS)
    with pytest.raises(RuntimeError, match="steps"):
        C.logits_constrain(x, torch.zeros(4, C.MAX_STEPS + 1, dtype=torch.long, device=cuda), pos, START, 2, 0, EOS)
    with pytest.raises(RuntimeError, match="pos"):
        C.logits_constrain(x, hist, pos.cpu(), START, 2, 0, EOS)
    with pytest.raises(RuntimeError, match="start_token"):
        C.logits_constrain(x, hist, pos, 32, 2, 0, EOS)
    with pytest.raises(RuntimeError, match="n must"):
        C.logits_constrain(x, hist, pos, START, -1, 0, EOS)
    with pytest.raises(RuntimeError, match="ban_lse"):
        C.logits_constrain(x, hist, pos, START, 2, 0, EOS, ban_lse=torch.zeros(3, device=cuda))
    tok, off = C.word_tables(((2, 3), (4,)), cuda)
    with pytest.raises(RuntimeError, match="word_off"):
        C.logits_constrain(x, hist, pos, START, 2, 0, EOS, (tok, off.long()))
    with pytest.raises(RuntimeError, match="come together"):
        C.logits_constrain(x, hist, pos, START, 2, 0, EOS, (tok, None))
    with pytest.raises(RuntimeError, match="tokens in all"):
        C.logits_constrain(x, hist, pos, START, 2, 0, EOS,
                           (torch.zeros(C.MAX_WORD_TOKENS + 1, dtype=torch.int32, device=cuda), off))
    with pytest.raises(RuntimeError, match="words are supported"):
        C.logits_constrain(x, hist, pos, START, 2, 0, EOS,
                           (tok, torch.zeros(C.MAX_WORDS + 2, dtype=torch.int32, device=cuda)))
    from cloudtik_amd import ops
    assert ops.require_native().constrain_caps() == (C.MAX_STEPS, C.MAX_WORDS, C.MAX_WORD_TOKENS)
    # a broken offset table on the device bans nothing and reads nothing out of bounds
    bad_off = torch.tensor([0, 5000, -3], dtype=torch.int32, device=cuda)
    before = x.clone()
    C.logits_constrain(x, hist, pos, START, 0, 0, EOS, (tok, bad_off))
    assert torch.equal(x, before)


# ------------------------------------------------------------------- consumers on masked rows
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_beam_topk_on_rows_with_banned_entries(cuda, dtype):
    """V = 24 is below the kernel's 256 threads: most threads see nothing, some only -inf."""
    g = torch.Generator().manual_seed(3)
    x = torch.randn(6, 24, generator=g).to(dtype)
    for r in range(6):
        x[r, torch.randperm(24, generator=g)[:10]] = NEG_INF
    x[5, :10] = NEG_INF                                        # a whole leading run
    lse, val, tok = beam_ops.beam_topk(x.to(cuda), 4)
    torch.testing.assert_close(lse.cpu(), torch.logsumexp(x.float(), 1), rtol=1e-5, atol=1e-6)
    w_val, w_tok = torch.sort(x.float(), dim=1, descending=True, stable=True)
    assert bool(torch.isfinite(w_val[:, :8]).all())
    assert torch.equal(tok.cpu().long(), w_tok[:, :8]) and torch.equal(val.cpu(), w_val[:, :8])


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("V", [24, 32128])
def test_sample_step_skips_a_banned_arg_max(cuda, V, dtype):
    R, T, t = 4, 6, 2
    g = torch.Generator().manual_seed(V)
    logits = torch.randn(R, V, generator=g).to(dtype)
    logits[:, 7] = 9.0                                         # the arg-max, a one-token bad word
    logits[:, 11] = 8.0                                        # the runner-up
    out = torch.randint(2, 6, (R, T), generator=g).to(cuda)
    d = logits.to(cuda)
    pos = torch.tensor([t], device=cuda)
    C.logits_constrain(d, out, pos, START, 0, 0, EOS, C.word_tables(((7,),), cuda))
    done = torch.zeros(R, dtype=torch.bool, device=cuda)
    cur = torch.zeros(R, 1, dtype=torch.long, device=cuda)
    sample_ops.sample_step(d, out, done, cur, pos, torch.tensor([5], device=cuda), START, EOS, PAD, top_k=1)
    assert cur[:, 0].tolist() == [11] * R and out[:, t].tolist() == [11] * R and int(pos) == t + 1


# --------------------------------------------------------------------------------- end to end
STEPS = 10
BANS = dict(no_repeat_ngram_size=2, min_length=6, bad_words_ids=[[5], [17, 42]])


@pytest.fixture(scope="module")
def reference_model():
    """The fp32 copy on the CPU.  The weights are drawn here and rounded to bf16, so that the GPU
    model holds the same numbers and the inputs below can be judged on this model alone."""
    torch.manual_seed(0)
    ref = T5ForConditionalGeneration(T5Config.small(dropout_rate=0.0), dtype=torch.float32).eval()
    with torch.no_grad():
        for p in ref.parameters():
            p.copy_(p.bfloat16().float())
    return ref


@pytest.fixture(scope="module")
def small(cuda, reference_model):
    m = T5ForConditionalGeneration(T5Config.small(dropout_rate=0.0), device=cuda).eval()
    m.load_state_dict({k: v.bfloat16() for k, v in reference_model.state_dict().items()})
    return m


def _batch(seed, cuda):
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(2, 32128, (3, 24), generator=g).to(cuda)
    mask = torch.ones(3, 24, dtype=torch.long, device=cuda)
    mask[1, 17:] = 0
    return x, mask


# sources, one generator seed each, for which the fp32 reference's 2K candidates stay furthest apart
# over all steps (the largest margins among seeds 0 .. 191, found on the reference alone: 4.4e-3,
# 4.2e-3, 3.7e-3).  The test re-checks the margin.
BEAM_ITEMS = (156, 85, 104)


def _beam_batch(cuda):
    x = torch.cat([torch.randint(2, 32128, (1, 24), generator=torch.Generator().manual_seed(s)) for s in BEAM_ITEMS])
    return x.to(cuda), torch.ones(3, 24, dtype=torch.long, device=cuda)


def _assert_nothing_banned(seq, V):
    """Re-derives the ban set of every step on the CPU from the output itself."""
    seq = seq.cpu()
    rule = C.check_constrain_args(vocab=V, eos=EOS, **BANS)
    live = torch.ones(seq.shape[0], dtype=torch.bool)
    for t in range(seq.shape[1]):
        ban = C.ban_mask_reference(seq, t, V, START, rule[0], rule[1], EOS, rule[2])
        assert not bool((ban.gather(1, seq[:, t:t + 1])[:, 0] & live).any()), t
        live &= seq[:, t] != EOS


def test_generate_greedy_graph_matches_eager(cuda, small):
    x, mask = _batch(1, cuda)
    plain = small.generate(x, mask, max_new_tokens=STEPS)
    n0 = len(small._graphs)
    got = small.generate(x, mask, max_new_tokens=STEPS, **BANS)
    assert got.shape == (3, STEPS) and got.dtype == torch.long and not torch.equal(got, plain)
    assert torch.equal(got, small.generate(x, mask, max_new_tokens=STEPS, use_graph=False, **BANS))
    n1 = len(small._graphs)
    assert n1 == n0 + 1
    assert torch.equal(small.generate(x, mask, max_new_tokens=STEPS, **BANS), got) and len(small._graphs) == n1
    assert torch.equal(small.generate(x, mask, max_new_tokens=STEPS), plain) and len(small._graphs) == n1
    _assert_nothing_banned(got, small.cfg.vocab_size)


def test_generate_sampling_graph_matches_eager(cuda, small):
    x, mask = _batch(2, cuda)
    rule = dict(do_sample=True, seed=7, top_k=40, temperature=0.9, repetition_penalty=1.1, num_return_sequences=2)
    got = small.generate(x, mask, max_new_tokens=STEPS, **rule, **BANS)
    assert got.shape == (6, STEPS)
    n1 = len(small._graphs)
    cons = C.check_constrain_args(vocab=small.cfg.vocab_size, eos=EOS, **BANS)
    static = small._generate_sample_static(x, mask, STEPS, 2, 7, temperature=0.9, top_k=40, repetition_penalty=1.1,
                                           graph=False, cons=cons)
    assert torch.equal(got, static)                            # the same step, eager
    assert torch.equal(got, small.generate(x, mask, max_new_tokens=STEPS, use_graph=False, **rule, **BANS))
    n2 = len(small._graphs)
    assert torch.equal(small.generate(x, mask, max_new_tokens=STEPS, **rule, **BANS), got) and len(small._graphs) == n2
    keys = [k for k in small._graphs if k[0] == "sample" and k[1] == 6 and k[-1]]
    assert len(keys) == 1 and keys[0][-2] == cons and n2 == n1 + 1      # n2: the eager static step's entry
    _assert_nothing_banned(got, small.cfg.vocab_size)


@pytest.mark.parametrize("early", [True, False])
def test_generate_beam_graph_matches_eager_and_cpu(cuda, small, reference_model, early):
    K, V = 4, small.cfg.vocab_size
    cons = C.check_constrain_args(vocab=V, eos=EOS, num_beams=K, max_new_tokens=STEPS, **BANS)
    x, mask = _beam_batch(cuda)
    got, score = small.generate(x, mask, max_new_tokens=STEPS, num_beams=K, early_stopping=early, return_scores=True,
                                **BANS)
    assert got.shape == (3, STEPS) and score.shape == (3,)
    n1 = len(small._graphs)
    again = small.generate(x, mask, max_new_tokens=STEPS, num_beams=K, early_stopping=early, **BANS)
    assert torch.equal(again, got) and len(small._graphs) == n1
    keys = [k for k in small._graphs if k[0] == "beam" and k[6] == K and k[8] == early and k[9] and k[10]
            and k[-1] == cons]
    assert len(keys) == 1
    _assert_nothing_banned(got, V)
    # the same static step with the PyTorch bookkeeping, eager; and the growing-cache loop
    w_seq, w_score = small._generate_beam_static(x, mask, STEPS, K, 1.0, early, fused=False, graph=False, trace=[],
                                                 cons=cons)
    assert torch.equal(got, w_seq)
    torch.testing.assert_close(score, w_score, rtol=1e-4, atol=0)
    assert torch.equal(got, small.generate(x, mask, max_new_tokens=STEPS, num_beams=K, early_stopping=early,
                                           use_graph=False, **BANS))
    # the reference loop of an fp32 copy on the CPU, item by item where its candidates stay apart
    trace = []
    c_seq, _ = reference_model._generate_beam_eager(x.cpu(), mask.cpu(), STEPS, K, 1.0, early, trace, cons=cons)
    cand = torch.stack(trace)                                  # [steps, B, 2K]
    margin = (cand[:, :, :-1] - cand[:, :, 1:]).amin((0, 2))
    use = margin > MARGIN
    print("fp32 CPU reference: margins", margin.tolist(), "compared", int(use.sum()), "of 3; rows equal",
          (got.cpu() == c_seq).all(1).tolist())
    assert int((~use).sum()) <= 0.1 * 3
    assert torch.equal(got.cpu()[use], c_seq[use])
