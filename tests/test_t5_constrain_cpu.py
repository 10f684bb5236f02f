"""Token bans on the CPU: the rule (ops/constrain.py) against the logits processors of the installed
``transformers`` and hand-built rows, ``generate`` with ``no_repeat_ngram_size``, ``min_length`` /
``min_new_tokens`` and ``bad_words_ids`` against the library's ``generate`` on tiny random models
(greedy and beam search), the sampling properties, the argument checks and ``generate_kwargs_for_task``."""
import json

import pytest
import torch

from cloudtik_amd.models.t5 import T5ForConditionalGeneration, generate_kwargs_for_task
from cloudtik_amd.ops import beam as beam_ops
from cloudtik_amd.ops import constrain as C

from test_t5_beam_cpu import _cut, _inputs, _library_model, _tiny

NEG_INF = float("-inf")
START, EOS, PAD = 0, 1, 0
T = 10


# ------------------------------------------------------------------ the rule against the library
def _histories(R, Tn, seed):
    """4 symbols, so n-grams recur; row 1 has interior start tokens."""
    g = torch.Generator().manual_seed(seed)
    hist = torch.randint(2, 6, (R, Tn), generator=g)
    hist[1, 2] = hist[1, 5] = hist[1, 6] = START
    return hist, g


def _ids(hist, t):
    return torch.cat([torch.full((hist.shape[0], 1), START), hist[:, :t]], 1)


@pytest.mark.parametrize("V", [24, 1003])
@pytest.mark.parametrize("n", [1, 2, 3, 5])
def test_ngram_rule_matches_library(V, n):
    pytest.importorskip("transformers")
    from transformers.generation import logits_process as lp
    Tn = 12
    hist, g = _histories(6, Tn, V + n)
    banned_any = False
    for dtype in (torch.float32, torch.bfloat16):
        logits = (torch.randn(6, V, generator=g) * 3).to(dtype)
        for t in range(Tn):
            want = lp.NoRepeatNGramLogitsProcessor(n)(_ids(hist, t), logits.clone())
            x, lse = C.constrain_reference(logits, hist, t, START, n)
            assert x.dtype == dtype and torch.equal(x, want), (t, dtype)       # -inf == -inf: bit-equal rows
            ban = torch.isneginf(want.float())
            assert torch.equal(torch.isneginf(lse), ~ban.any(1))
            exact = torch.logsumexp(logits.double().masked_fill(~ban, NEG_INF), 1)
            torch.testing.assert_close(lse.double()[ban.any(1)], exact[ban.any(1)], rtol=1e-5, atol=1e-6)
            banned_any |= bool(ban.any())
            assert torch.equal(ban, C.ban_mask_reference(hist, t, V, START, n))
    assert banned_any


@pytest.mark.parametrize("V", [24, 1003])
def test_words_and_minimum_length_match_library(V):
    pytest.importorskip("transformers")
    from transformers.generation import logits_process as lp
    Tn = 12
    hist, g = _histories(6, Tn, V)
    hist[0, :4] = torch.tensor([2, 3, 2, 3])                   # at t = 3 the row ends in 2, which 3 has followed
    words = [[7], [2, 3], [3, 2, 4], [4, 5]]                   # 1, 2 and 3 tokens; [2, 3] ends in a token n-grams ban too
    logits = torch.randn(6, V, generator=g) * 3
    both = 0
    for t in range(Tn):
        ids = _ids(hist, t)
        want = lp.NoBadWordsLogitsProcessor(words, eos_token_id=EOS)(ids, logits.clone())
        x, _ = C.constrain_reference(logits, hist, t, START, bad_words=words)
        assert torch.equal(x, want), t
        for min_length in (0, 1, 5, 12):
            want = lp.MinLengthLogitsProcessor(min_length, EOS)(ids, logits.clone()) if min_length else logits
            x, _ = C.constrain_reference(logits, hist, t, START, min_new=max(min_length - 1, 0), eos=EOS)
            assert torch.equal(x, want), (t, min_length)
        for min_new in (1, 4):
            want = lp.MinNewTokensLengthLogitsProcessor(1, min_new, EOS)(ids, logits.clone())
            x, _ = C.constrain_reference(logits, hist, t, START, min_new=min_new, eos=EOS)
            assert torch.equal(x, want), (t, min_new)
        # all of them, in the library's order
        want = lp.NoRepeatNGramLogitsProcessor(2)(ids, logits.clone())
        ngram = torch.isneginf(want)
        want = lp.NoBadWordsLogitsProcessor(words, eos_token_id=EOS)(ids, want)
        want = lp.MinLengthLogitsProcessor(6, EOS)(ids, want)
        x, lse = C.constrain_reference(logits, hist, t, START, 2, 5, EOS, words)
        assert torch.equal(x, want), t
        ban = torch.isneginf(want)
        torch.testing.assert_close(lse.double(), torch.logsumexp(logits.double().masked_fill(~ban, NEG_INF), 1),
                                   rtol=1e-5, atol=1e-6)
        word_only = C.ban_mask_reference(hist, t, V, START, bad_words=words)
        both += int((ngram & word_only)[:, 3].sum())
    assert both > 0                                            # token 3 banned by the n-gram rule and by [2, 3] at once


# ------------------------------------------------------------------------------ hand-built rows
def _banned(hist_row, t, n=0, min_new=0, words=(), V=12):
    hist = torch.tensor([hist_row + [9] * (8 - len(hist_row))])
    mask = C.ban_mask_reference(hist, t, V, START, n, min_new, EOS, words)
    return sorted(mask[0].nonzero()[:, 0].tolist())


def test_ngram_edges():
    # n = 3: h has t + 1 tokens; nothing can be banned before it holds n of them
    assert _banned([0, 0], 1, n=3) == []                       # t + 1 == n - 1
    assert _banned([0, 0], 2, n=3) == [0]                      # t + 1 == n: h = [0, 0, 0], the start token counts
    assert _banned([5, 6], 2, n=3) == []
    assert _banned([5, 0, 5], 3, n=3) == [0]                   # t + 1 == n + 1: h = [0, 5, 0, 5]; (0, 5) was followed by 0
    assert _banned([5, 6, 5], 3, n=3) == []
    assert _banned([5, 6, 7, 5, 6, 8, 5, 6], 7, n=3) == []     # slot 7 is not read at t = 7: h ends 8, 5
    assert _banned([5, 6, 7, 8, 5, 6, 5, 6], 6, n=3) == [7]    # h ends 5, 6, which 7 followed
    assert _banned([6, 7, 6, 7, 6], 5, n=2) == [7]             # 6 was followed by 7 twice: once in the set
    assert _banned([5, 6, 7, 5, 6, 8, 5, 6], 7, n=2) == [6]
    # n = 2 and 1
    assert _banned([4, 5, 4], 3, n=2) == [5]
    assert _banned([4, 5, 4], 3, n=1) == [0, 4, 5]
    assert _banned([], 0, n=1) == [0]
    assert _banned([], 0, n=2) == []
    # later slots are never looked at, and a step outside the table bans nothing
    assert _banned([4, 5, 4, 5, 5, 5], 3, n=2) == [5]
    assert _banned([4, 5, 4], 8, n=1) == [] and _banned([4, 5, 4], -1, n=1, min_new=3) == []
    # a token outside the vocabulary equals nothing and bans nothing
    assert _banned([4, 12, 4, 12, 4], 5, n=1) == [0, 4]
    assert _banned([12, 4, 12], 3, n=2) == []
    assert _banned([-1, 4, -1], 3, n=3) == []


def test_word_edges():
    assert _banned([], 0, words=[[7]]) == [7]
    assert _banned([], 0, words=[[3, 7]]) == []
    assert _banned([3], 1, words=[[3, 7]]) == [7]
    assert _banned([3, 4], 2, words=[[3, 7]]) == []
    assert _banned([3, 4], 2, words=[[3, 4, 7], [4, 8], [5, 9]]) == [7, 8]
    assert _banned([3], 1, words=[[3, 4, 7]]) == []
    # m - 1 == t + 1: the start token is part of the prefix (the one case the library leaves out)
    assert _banned([], 0, words=[[0, 7]]) == [7]
    assert _banned([3], 1, words=[[0, 3, 7]]) == [7]
    assert _banned([3], 1, words=[[5, 0, 3, 7]]) == []
    assert _banned([], 0, min_new=1) == [EOS] and _banned([], 0, min_new=0) == []
    assert _banned([4, 4], 2, min_new=3) == [EOS] and _banned([4, 4, 4], 3, min_new=3) == []


def test_ban_lse_counts_a_token_once_and_empty_is_minus_inf():
    V = 12
    logits = torch.randn(2, V, generator=torch.Generator().manual_seed(0))
    logits[:, EOS] = 6.0                                       # most of the mass: a double count shifts ban_lse by ~log 2
    hist = torch.tensor([[7, EOS, 7, 9], [7, EOS, 7, 9]])
    words = [[7, EOS], [8]]
    # EOS by the n-gram rule (7 was followed by EOS), by the word [7, EOS] and by the minimum length
    for part in (dict(no_repeat_ngram_size=2), dict(bad_words=[[7, EOS]]), dict(min_new=9, eos=EOS)):
        assert C.ban_mask_reference(hist, 3, V, START, **part)[0].nonzero()[:, 0].tolist() == [EOS]
    x, lse = C.constrain_reference(logits, hist, 3, START, 2, 9, EOS, words)
    assert torch.isneginf(x[:, [EOS, 8]]).all() and int(torch.isneginf(x).sum()) == 4
    exact = torch.logsumexp(logits[:, [EOS, 8]].double(), 1)
    torch.testing.assert_close(lse.double(), exact, rtol=1e-6, atol=1e-6)
    assert float((lse.double() - exact).abs().max()) < 0.01 < 0.69
    keep = torch.ones(V, dtype=torch.bool)
    keep[[EOS, 8]] = False
    assert torch.equal(x[:, keep], logits[:, keep]) and lse.dtype == torch.float32
    x, lse = C.constrain_reference(logits, hist, 0, START, 2)
    assert torch.equal(x, logits) and lse.tolist() == [NEG_INF, NEG_INF]


def test_beam_step_reference_masks_after_the_log_softmax():
    V, K = 12, 2
    g = torch.Generator().manual_seed(1)
    logits = torch.randn(2 * K, V, generator=g)
    state = beam_ops.new_state(2, K, 4, PAD)
    state["run_score"] = -torch.rand(2, K, generator=g)
    len_pen = beam_ops.length_penalty_table(4, 1.0)
    ban = torch.zeros(2 * K, V, dtype=torch.bool)
    ban[torch.arange(2 * K), logits.argmax(-1)] = True         # every row loses its best token
    _, _, _, cand, idx = beam_ops.beam_step_reference(logits, state, 1, len_pen, EOS, ban=ban)
    flat = (torch.log_softmax(logits, -1).masked_fill(ban, NEG_INF).view(2, K, V) + state["run_score"][:, :, None])
    want, w_idx = torch.sort(flat.view(2, -1), dim=1, descending=True, stable=True)
    assert torch.equal(cand, want[:, :2 * K]) and torch.equal(idx, w_idx[:, :2 * K])
    plain = beam_ops.beam_step_reference(logits, state, 1, len_pen, EOS)
    none = beam_ops.beam_step_reference(logits, state, 1, len_pen, EOS, ban=torch.zeros_like(ban))
    assert torch.equal(plain[3], none[3]) and not torch.equal(plain[4], idx)


# ------------------------------------------------------------------- generate against the library
SEEDS = range(10)
MODES = [(1, False)] + [(K, early) for K in (2, 4) for early in (True, False)]
SETTINGS = {
    "ngram2": dict(no_repeat_ngram_size=2),
    "ngram3": dict(no_repeat_ngram_size=3),
    "min_new5": dict(min_new_tokens=5),
    "min_length6": dict(min_length=6),
    "words": dict(),                                           # built per case from the library's plain output
    "all": dict(no_repeat_ngram_size=2, min_length=6),         # and the built words
}
# (min_new_tokens and min_length are never given together here: the library then drops min_length,
# where this project takes the larger of the two.)


def _lib_generate(hf, x, mask, K, early, **kw):
    with torch.no_grad():
        y = hf.generate(input_ids=x, attention_mask=mask, max_new_tokens=T, num_beams=K, early_stopping=early,
                        do_sample=False, output_scores=True, return_dict_in_generate=True, **kw)
    seq = torch.nn.functional.pad(y.sequences[:, 1:], (0, T - (y.sequences.shape[1] - 1)))
    return _cut(seq), (y.sequences_scores if K > 1 else None)


def _built_words(plain):
    """From item 0 of the library's unconstrained output: its first token as a one-token word and its
    tokens 2-3 as a two-token word, wherever those are real tokens (not EOS or the pad after it)."""
    row = plain[0].tolist()
    words = []
    if row[0] not in (EOS, PAD):
        words.append([row[0]])
        if row[1] not in (EOS, PAD) and row[2] != PAD:
            words.append([row[1], row[2]])
    return words


@pytest.fixture(scope="module")
def library():
    """Per seed the library model, ours loaded from it and the inputs; per (seed, mode) the library's
    unconstrained output."""
    pytest.importorskip("transformers")
    models, plain = {}, {}
    for seed in SEEDS:
        hf = _library_model(seed)
        ours = T5ForConditionalGeneration.from_hf_config(hf.config, dtype=torch.float32).eval()
        ours.load_hf_state_dict(hf.state_dict())
        models[seed] = (hf, ours, *_inputs(seed))
        for K, early in MODES:
            plain[seed, K, early] = _lib_generate(hf, *_inputs(seed), K, early)[0]
    return models, plain


@pytest.mark.parametrize("name", list(SETTINGS))
def test_generate_matches_library(library, name):
    models, plain = library
    cases = changed = skipped = built = 0
    for seed in SEEDS:
        hf, ours, x, mask = models[seed]
        for K, early in MODES:
            kw = dict(SETTINGS[name])
            if name in ("words", "all"):
                words = _built_words(plain[seed, K, early])
                if not words:
                    continue                                   # the plain output starts with EOS: nothing to build
                kw["bad_words_ids"] = words
                built += 1
            cases += 1
            want, w_score = _lib_generate(hf, x, mask, K, early, **kw)
            differs = not torch.equal(want, plain[seed, K, early])
            changed += differs
            if name == "words":
                assert differs, (seed, K, early)               # the built words bite by construction
            trace = [] if K > 1 else None
            got = ours.generate(x, mask, max_new_tokens=T, num_beams=K, early_stopping=early, trace=trace,
                                return_scores=K > 1, **kw)
            if K > 1:
                got, score = got
                cand = torch.stack(trace)                      # [T, B, 2K]: the candidates the library ranks too
                gap = (cand[:, :, :-1] - cand[:, :, 1:])[torch.isfinite(cand[:, :, 1:])]
                if float(gap.min()) < 1e-6:                    # a tie: either order is right
                    skipped += 1
                    continue
            assert torch.equal(got, _cut(got))
            assert torch.equal(got, want), (name, seed, K, early)
            if K > 1:
                torch.testing.assert_close(score, w_score, rtol=1e-5, atol=1e-5)
    print(f"{name}: {cases} cases, {changed} changed by the setting, {skipped} skipped for a tie")
    assert skipped <= 0.1 * cases
    if name.startswith("ngram") or name == "all":
        assert changed >= 0.5 * cases, changed
    if name.startswith("min_"):
        assert changed >= 5, changed
    if name in ("words", "all"):
        assert built >= 0.8 * len(SEEDS) * len(MODES), built


# ------------------------------------------------------------------------------------ sampling
BANS = dict(no_repeat_ngram_size=2, min_new_tokens=4, bad_words_ids=[[5], [3, 4], [17, 9, 2]])


def _assert_nothing_banned(seq, V, n, min_new, words):
    live = torch.ones(seq.shape[0], dtype=torch.bool)
    for t in range(seq.shape[1]):
        ban = C.ban_mask_reference(seq, t, V, START, n, min_new, EOS, words)
        assert not bool((ban.gather(1, seq[:, t:t + 1])[:, 0] & live).any()), t
        live &= seq[:, t] != EOS


def test_sampling_with_constraints():
    m = _tiny(0)
    x, mask = _inputs(3)
    V = m.cfg.vocab_size
    for seed, extra in ((0, {}), (5, dict(top_k=8, temperature=1.5)), (9, dict(top_p=0.8, repetition_penalty=1.3))):
        kw = dict(max_new_tokens=T, do_sample=True, seed=seed, num_return_sequences=4, **extra)
        a = m.generate(x, mask, **kw, **BANS)
        assert a.shape == (12, T) and torch.equal(_cut(a), a)
        assert torch.equal(m.generate(x, mask, **kw, **BANS), a)                   # reproducible
        _assert_nothing_banned(a, V, 2, 4, BANS["bad_words_ids"])
        assert not bool((a[:, :4] == EOS).any())
        plain = m.generate(x, mask, **kw)
        assert not torch.equal(plain, a)
    # n = 1: no token twice, and never the start token, which is in every history
    a = m.generate(x, mask, max_new_tokens=T, do_sample=True, seed=2, no_repeat_ngram_size=1)
    for row in _cut(a).tolist():
        real = row[:row.index(EOS) + 1] if EOS in row else row
        assert len(set(real)) == len(real) and START not in real
    # top_k = 1 with the bans is greedy with the bans
    assert torch.equal(m.generate(x, mask, max_new_tokens=T, do_sample=True, seed=3, top_k=1, **BANS),
                       m.generate(x, mask, max_new_tokens=T, **BANS))
    # the first two steps by hand: the bans, then the sampling rule, on the model's own logits
    from cloudtik_amd.ops import sampling as S
    a = m.generate(x, mask, max_new_tokens=T, do_sample=True, seed=11, min_new_tokens=4, bad_words_ids=[[5], [3, 4]])
    enc, _ = m.encoder(x, mask)
    ids = torch.zeros(3, 1, dtype=torch.long)
    for t in range(2):
        dec, _ = m.decoder(ids, enc=enc, enc_mask=mask)
        l, _ = C.constrain_reference(m.logits(dec[:, -1]), a, t, START, 0, 4, EOS, [[5], [3, 4]])
        xx, keep = S.process_logits_reference(l, None)
        u = torch.tensor([S.philox_uniform_reference(11, r, t) for r in range(3)], dtype=torch.float32)
        assert torch.equal(a[:, t], S.draw_reference(xx, keep, u))
        ids = torch.cat([ids, a[:, t:t + 1]], 1)


# ---------------------------------------------------------------------------- arguments, defaults
def test_argument_validation():
    m = _tiny(0)                                               # V = 64
    x, mask = _inputs(0)
    for name in ("no_repeat_ngram_size", "min_new_tokens", "min_length"):
        for bad in (-1, 1.5, "2", True, None):
            with pytest.raises(ValueError, match=name):
                m.generate(x, mask, **{name: bad})
            with pytest.raises(ValueError, match=name):
                m.generate(x, mask, do_sample=True, num_beams=1, **{name: bad})
    for bad in ([[]], [3], "ab", [[2, 1.5]], [[2, True]], [[64]], [[-1]], [[2, 3], []], 7):
        with pytest.raises(ValueError, match="bad_words_ids"):
            m.generate(x, mask, bad_words_ids=bad)
    with pytest.raises(ValueError, match="use min_new_tokens"):
        m.generate(x, mask, bad_words_ids=[[2, 3], [EOS]])
    m.generate(x, mask, max_new_tokens=3, bad_words_ids=[[2, EOS]])               # EOS inside a longer word is fine
    with pytest.raises(ValueError, match=f"at most {C.MAX_WORDS}"):
        m.generate(x, mask, bad_words_ids=[[2, 3]] * (C.MAX_WORDS + 1))
    with pytest.raises(ValueError, match=f"at most {C.MAX_WORD_TOKENS}"):
        m.generate(x, mask, bad_words_ids=[[2] * 1025, [3] * 1024])
    with pytest.raises(ValueError, match=f"max_new_tokens <= {C.MAX_STEPS}"):
        m.generate(x, mask, max_new_tokens=C.MAX_STEPS + 1, no_repeat_ngram_size=2)
    # beam search keeps 2K finite candidates a row: V >= 2K + max_new_tokens + 1 + words
    with pytest.raises(ValueError, match="vocabulary"):
        m.generate(x, mask, num_beams=4, max_new_tokens=56, no_repeat_ngram_size=2)       # needs 8 + 56 + 1 = 65, has 64
    assert m.generate(x, mask, num_beams=4, max_new_tokens=56).shape == (3, 56)                   # no constraint, no demand
    with pytest.raises(ValueError, match="vocabulary"):
        m.generate(x, mask, num_beams=4, max_new_tokens=54, min_length=3, bad_words_ids=[[2], [3]])
    assert C.check_constrain_args(2, vocab=64, num_beams=4, max_new_tokens=55) is not None        # 8 + 55 + 1 = 64
    with pytest.raises(ValueError, match="vocabulary"):
        C.check_constrain_args(2, vocab=63, num_beams=4, max_new_tokens=55)
    assert C.check_constrain_args(2, vocab=8, num_beams=1, max_new_tokens=55) is not None         # greedy: no demand
    # the frozen rule: hashable, min_length counts the start token, nothing on is None
    assert C.check_constrain_args() is None and C.check_constrain_args(0, 0, 1, []) is None
    assert C.check_constrain_args(3, 2, 6, [[4, 5], (6,)]) == (3, 5, ((4, 5), (6,)))
    assert C.check_constrain_args(0, 7, 6) == (0, 7, ()) and hash(C.check_constrain_args(1, 0, 0, [[2]])) is not None
    # errors that were there before stay
    with pytest.raises(ValueError, match="beam sampling"):
        m.generate(x, mask, do_sample=True, num_beams=2, no_repeat_ngram_size=2)
    with pytest.raises(ValueError, match="never"):
        m.generate(x, mask, num_beams=2, early_stopping="never", min_length=4)
    with pytest.raises(RuntimeError, match="GPU kernel"):
        C.logits_constrain(torch.zeros(1, 8), torch.zeros(1, 2, dtype=torch.long), torch.zeros(1, dtype=torch.long), 0, 2)


def test_vocabulary_demand_message():
    m = _tiny(0)
    x, mask = _inputs(0)
    with pytest.raises(ValueError, match="= 65 tokens, got 64"):
        m.generate(x, mask, num_beams=4, max_new_tokens=56, no_repeat_ngram_size=2)


def test_defaults_are_the_parent_paths():
    m = _tiny(1)
    x, mask = _inputs(1)
    off = dict(no_repeat_ngram_size=0, min_new_tokens=0, min_length=0, bad_words_ids=None)
    greedy = m.generate(x, mask, max_new_tokens=T)
    assert torch.equal(m.generate(x, mask, max_new_tokens=T, **off), greedy)
    assert torch.equal(m.generate(x, mask, max_new_tokens=T, min_length=1, bad_words_ids=[]), greedy)
    beam, score = m.generate(x, mask, max_new_tokens=T, num_beams=3, length_penalty=0.6, return_scores=True)
    b2, s2 = m.generate(x, mask, max_new_tokens=T, num_beams=3, length_penalty=0.6, return_scores=True, **off)
    b3, s3 = m._generate_beam_eager(x, mask, T, 3, 0.6, False)
    assert torch.equal(b2, beam) and torch.equal(s2, score) and torch.equal(b3, beam) and torch.equal(s3, score)
    sample = m.generate(x, mask, max_new_tokens=T, do_sample=True, seed=4, top_k=9)
    assert torch.equal(m.generate(x, mask, max_new_tokens=T, do_sample=True, seed=4, top_k=9, **off), sample)
    assert torch.equal(m._generate_sample_eager(x, mask, T, 1, 4, top_k=9), sample)
    # a constraint that cannot bite leaves the tokens alone: a word longer than the output
    assert torch.equal(m.generate(x, mask, max_new_tokens=T, bad_words_ids=[[2] * (T + 2)]), greedy)


# ------------------------------------------------------------------------- task settings
STOCK = {  # the block the stock t5-small / t5-base / t5-large config.json carries
    "vocab_size": 32128, "d_model": 512,
    "task_specific_params": {
        "summarization": {"early_stopping": True, "length_penalty": 2.0, "max_length": 200, "min_length": 30,
                          "no_repeat_ngram_size": 3, "num_beams": 4, "prefix": "summarize: "},
        "translation_en_to_de": {"early_stopping": True, "max_length": 300, "num_beams": 4,
                                 "prefix": "translate English to German: "},
    },
}


def test_generate_kwargs_for_task(tmp_path):
    kw, prefix = generate_kwargs_for_task(STOCK, "summarization")
    assert prefix == "summarize: "
    assert kw == dict(early_stopping=True, length_penalty=2.0, max_new_tokens=199, min_length=30,
                      no_repeat_ngram_size=3, num_beams=4)
    kw, prefix = generate_kwargs_for_task(STOCK, "translation_en_to_de")
    assert kw == dict(early_stopping=True, max_new_tokens=299, num_beams=4) and prefix.startswith("translate")
    path = tmp_path / "config.json"
    path.write_text(json.dumps(STOCK))
    assert generate_kwargs_for_task(str(path), "summarization") == generate_kwargs_for_task(STOCK, "summarization")
    assert generate_kwargs_for_task(path, "summarization")[0]["min_length"] == 30

    class Config:
        def to_dict(self):
            return STOCK

    assert generate_kwargs_for_task(Config(), "summarization")[1] == "summarize: "
    with pytest.raises(KeyError, match="question_answering"):
        generate_kwargs_for_task(STOCK, "question_answering")
    with pytest.raises(KeyError, match="summarization"):
        generate_kwargs_for_task({"vocab_size": 8}, "summarization")
    odd = {"task_specific_params": {"summarization": {"num_beams": 4, "diversity_penalty": 0.5}}}
    with pytest.raises(ValueError, match="diversity_penalty"):
        generate_kwargs_for_task(odd, "summarization")
    # the settings run: a tiny model takes them as they are (fewer steps, to keep this quick)
    m = _tiny(2)
    x, mask = _inputs(2)
    kw, _ = generate_kwargs_for_task(STOCK, "summarization")
    kw.update(max_new_tokens=40, min_length=12)
    out = m.generate(x, mask, **kw)
    assert out.shape == (3, 40) and not bool((out[:, :11] == EOS).any())
    _assert_nothing_banned(out, m.cfg.vocab_size, 3, 11, ())
