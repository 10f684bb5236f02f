"""T5 sampling on the CPU: the Philox stream, the rule (ops/sampling.py) against the logits
processors of the installed ``transformers`` and hand-built rows, the draw and its distribution,
and ``generate(do_sample=True)`` / ``num_return_sequences`` on tiny random models."""
import pytest
import torch

from cloudtik_amd.ops import sampling as S

from test_t5_beam_cpu import T, _cut, _inputs, _library_model, _tiny
from cloudtik_amd.models.t5 import T5ForConditionalGeneration

NEG_INF = float("-inf")


# -------------------------------------------------------------------------------------- Philox
def test_philox_known_answers():
    f = 0xFFFFFFFF
    assert S.philox4x32((0, 0, 0, 0), (0, 0)) == (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)
    assert S.philox4x32((f, f, f, f), (f, f)) == (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)
    assert S.philox4x32((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0)) == \
        (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)


def test_uniform_range_and_tensor_form():
    assert S.uniform_of_word(0) == 0.0 and S.uniform_of_word(0xFF) == 0.0
    assert S.uniform_of_word(0xFFFFFFFF) == 1 - 2.0 ** -24
    assert torch.tensor(S.uniform_of_word(0xFFFFFFFF), dtype=torch.float32).item() == 1 - 2.0 ** -24   # exact in fp32
    assert S.philox_uniform_reference(0, 0, 0) == (0x6627E8D5 >> 8) * 2.0 ** -24
    for seed in (0, 1, 2 ** 32 + 5, 2 ** 63 - 1):
        for step in (0, 5):
            got = S.philox_uniform(torch.tensor([seed]), 130, torch.tensor([step]))
            assert got.dtype == torch.float32 and bool((got >= 0).all() and (got < 1).all())
            want = [S.philox_uniform_reference(seed, r, step) for r in range(130)]
            assert got.tolist() == want


# ---------------------------------------------------------------- steps 1-4 against the library
PARAMS = [  # (repetition_penalty, temperature, top_k, top_p)
    (1.0, 0.7, 50, 1.0), (1.0, 1.0, 0, 0.9), (1.2, 0.7, 50, 0.95), (1.3, 1.5, 0, 0.5), (1.0, 1.0, 1, 1.0),
    (1.1, 0.9, 400, 0.3)]


@pytest.mark.parametrize("V,R", [(32128, 6), (1003, 48)])
@pytest.mark.parametrize("rp,temp,k,p", PARAMS)
def test_processed_logits_match_library(V, R, rp, temp, k, p):
    pytest.importorskip("transformers")
    from transformers.generation import logits_process as lp
    g = torch.Generator().manual_seed(V + int(100 * temp) + k)
    logits = torch.randn(R, V, generator=g) * 3
    ids = torch.randint(0, V, (R, 7), generator=g)
    ids[:, 3] = ids[:, 1]                                        # a token seen twice
    seen = torch.zeros(R, V, dtype=torch.bool).scatter_(1, ids, True)
    assert bool((logits.gather(1, ids) < 0).any() and (logits.gather(1, ids) > 0).any())

    want = logits.clone()
    if rp != 1.0:
        want = lp.RepetitionPenaltyLogitsProcessor(rp)(ids, want)
    if temp != 1.0:
        want = lp.TemperatureLogitsWarper(temp)(ids, want)
    processed = want.clone()
    if k:
        want = lp.TopKLogitsWarper(k)(ids, want)
    if p < 1.0:
        want = lp.TopPLogitsWarper(p)(ids, want)

    x, keep = S.process_logits_reference(logits, seen, temp, k, p, rp)
    assert torch.equal(x, processed)                             # bit-equal processed values
    assert torch.equal(keep, want != NEG_INF)
    assert torch.equal(x[keep], want[keep])
    assert bool(keep.any(1).all())


def test_tie_groups_stay_whole():
    """The documented tie rule, not the library's: a tie group that straddles top_p or top_k stays."""
    x = torch.tensor([[0.4, 0.2, 0.2, 0.1, 0.1]]).log()
    _, keep = S.process_logits_reference(x, None, top_p=0.5)
    assert keep.tolist() == [[True, True, True, False, False]]       # A(0.2) = 0.4 < 0.5 for both 0.2s
    _, keep = S.process_logits_reference(x, None, top_p=0.3)
    assert keep.tolist() == [[True, False, False, False, False]]
    _, keep = S.process_logits_reference(torch.tensor([[3.0, 2.0, 1.0, 2.0]]), None, top_k=2)
    assert keep.tolist() == [[True, True, False, True]]
    x = torch.tensor([[1.0, float("nan"), NEG_INF, 0.5]])
    got, keep = S.process_logits_reference(x, None, top_k=3)
    assert got[0, 1] == NEG_INF and keep.tolist() == [[True, True, True, True]]   # NaN ranks as -inf, tied with it


# ------------------------------------------------------------------------------------ the draw
W8 = [1.0, 2.0, 3.0, 4.0, 0.0, 2.0, 1.0, 3.0]                  # weights / 16; token 4 can never be drawn


def test_draw_boundaries():
    x = torch.tensor([W8]).log()
    keep = torch.ones(1, 8, dtype=torch.bool)
    edges = [0.0, 1 / 16, 3 / 16, 6 / 16, 10 / 16, 10 / 16, 12 / 16, 13 / 16, 1.0]

    def draw(u, keep=keep):
        return int(S.draw_reference(x, keep, torch.tensor([u], dtype=torch.float32))[0])

    assert draw(0.0) == 0
    assert draw(1 - 2.0 ** -24) == 7
    for v in range(8):
        if W8[v] > 0:
            assert draw((edges[v] + edges[v + 1]) / 2) == v
    # over a kept subset {1, 3, 5}: weights 2, 4, 2
    sub = torch.tensor([[False, True, False, True, False, True, False, False]])
    assert [draw(u, sub) for u in (0.0, 0.2, 0.3, 0.7, 0.8, 1 - 2.0 ** -24)] == [1, 1, 3, 3, 5, 5]
    # no finite logit: token 0
    none = torch.full((1, 8), NEG_INF)
    assert int(S.draw_reference(none, keep, torch.tensor([0.5]))[0]) == 0


CHI_SEED = 2024            # picked once; the stream is deterministic, so the statistic below is too


def test_draw_distribution_chi_square():
    n, w = 65536, [1.0, 2.0, 3.0, 4.0, 1.0, 2.0, 1.0, 2.0]     # / 16: exact probabilities
    u = S.philox_uniform(torch.tensor([CHI_SEED]), n, torch.tensor([0]))
    x = torch.tensor([w]).log().expand(n, 8)
    tok = S.draw_reference(x, torch.ones(n, 8, dtype=torch.bool), u)
    obs = torch.bincount(tok, minlength=8).double()
    exp = torch.tensor(w, dtype=torch.float64) / 16 * n
    stat = float(((obs - exp) ** 2 / exp).sum())
    print("chi-square", stat)
    assert stat < 29.9                             # the 1 - 1e-4 quantile at 7 degrees of freedom


# ---------------------------------------------------------------------------- step bookkeeping
def test_step_bookkeeping():
    V, Tn, eos, pad = 8, 4, 1, 0
    logits = torch.tensor([W8, W8, [0, 1e-9, 0, 0, 0, 0, 0, 0], W8]).clamp(min=1e-30).log()
    logits[3] = NEG_INF
    out = torch.full((4, Tn), pad, dtype=torch.long)
    out[:, 0] = 5
    done = torch.tensor([False, True, False, False])
    cur = torch.full((4, 1), 5)
    pos, seed = torch.tensor([1]), torch.tensor([7])
    u = torch.tensor([0.5, 0.5, 0.5, 0.5])
    o, d, c, p, uu, thr, nk = S.sample_step_reference(logits, out, done, cur, pos, seed, 0, eos, pad, u=u)
    assert o[:, 1].tolist() == [3, pad, eos, 0] and torch.equal(o[:, 0], out[:, 0]) and bool((o[:, 2:] == pad).all())
    assert d.tolist() == [False, True, True, False] and c[:, 0].tolist() == [3, pad, eos, 0] and int(p) == 2
    assert int(pos) == 1 and bool((out[:, 1] == pad).all())      # the arguments are left alone
    assert nk.tolist() == [8, 8, 8, 8] and torch.equal(uu, u)
    # Philox when no u is given: the same seed twice is the same, the uniforms are the stream's
    a = S.sample_step_reference(logits, out, done, cur, pos, seed, 0, eos, pad)
    b = S.sample_step_reference(logits, out, done, cur, pos, seed, 0, eos, pad)
    assert torch.equal(a[0], b[0]) and a[4].tolist() == [S.philox_uniform_reference(7, r, 1) for r in range(4)]


def test_repetition_penalty_counts_start_and_duplicates_once():
    logits = torch.tensor([[2.0, -1.0, 3.0, 0.5, -4.0]])
    out = torch.tensor([[2, 2, 4, 0]])
    seen = S.seen_mask(out, torch.tensor([3]), 0, 5)
    assert seen.tolist() == [[True, False, True, False, True]]   # start token 0; 2 twice; 4; slot 3 not yet written
    x, _ = S.process_logits_reference(logits, seen, repetition_penalty=2.0)
    assert x.tolist() == [[1.0, -1.0, 1.5, 0.5, -8.0]]


# ------------------------------------------------------------------------------------ generate
def test_generate_sampling_properties():
    m = _tiny(0)
    x, mask = _inputs(3)
    greedy = m.generate(x, mask, max_new_tokens=T)
    for seed in (0, 5, 2 ** 40 + 1):
        assert torch.equal(m.generate(x, mask, max_new_tokens=T, do_sample=True, top_k=1, seed=seed), greedy)
    a = m.generate(x, mask, max_new_tokens=T, do_sample=True, seed=11)
    assert a.shape == (3, T) and a.dtype == torch.long and torch.equal(_cut(a), a)
    assert torch.equal(m.generate(x, mask, max_new_tokens=T, do_sample=True, seed=11), a)
    assert not torch.equal(m.generate(x, mask, max_new_tokens=T, do_sample=True, seed=12), a)
    # seed=None takes it from torch's generator
    torch.manual_seed(99)
    b = m.generate(x, mask, max_new_tokens=T, do_sample=True, temperature=1.3, top_p=0.9, repetition_penalty=1.2)
    torch.manual_seed(99)
    assert torch.equal(m.generate(x, mask, max_new_tokens=T, do_sample=True, temperature=1.3, top_p=0.9,
                                  repetition_penalty=1.2), b)
    # several samples per item: item-major rows, drawn independently (row r of the batch B * N)
    c = m.generate(x, mask, max_new_tokens=T, do_sample=True, num_return_sequences=3, seed=11, temperature=1.5)
    assert c.shape == (9, T) and torch.equal(_cut(c), c)
    for b_ in range(3):
        rows = c[3 * b_:3 * b_ + 3]
        assert not (torch.equal(rows[0], rows[1]) and torch.equal(rows[1], rows[2]))
    # the first token of row r is the rule's draw from item r // 3's first-step logits with u(seed, r, 0)
    enc, _ = m.encoder(x, mask)
    dec, _ = m.decoder(torch.zeros(3, 1, dtype=torch.long), enc=enc, enc_mask=mask)
    l0 = m.logits(dec[:, -1]).repeat_interleave(3, 0)
    xx, keep = S.process_logits_reference(l0, None, temperature=1.5)
    u = torch.tensor([S.philox_uniform_reference(11, r, 0) for r in range(9)], dtype=torch.float32)
    assert torch.equal(c[:, 0], S.draw_reference(xx, keep, u))


def test_generate_defaults_unchanged():
    m = _tiny(1)
    x, mask = _inputs(1)
    greedy = m.generate(x, mask, max_new_tokens=T)
    beam, score = m.generate(x, mask, max_new_tokens=T, num_beams=3, return_scores=True)
    m.generate(x, mask, max_new_tokens=T, do_sample=True, seed=1, top_k=5)
    assert torch.equal(m.generate(x, mask, max_new_tokens=T, do_sample=False, num_return_sequences=1), greedy)
    b2, s2 = m.generate(x, mask, max_new_tokens=T, num_beams=3, return_scores=True, num_return_sequences=1)
    assert torch.equal(b2, beam) and torch.equal(s2, score)
    # N <= K hypotheses: the first is today's result, scores descend
    seqs, scores = m.generate(x, mask, max_new_tokens=T, num_beams=3, return_scores=True, num_return_sequences=3)
    assert seqs.shape == (9, T) and scores.shape == (9,)
    assert torch.equal(seqs.view(3, 3, T)[:, 0], beam) and torch.equal(scores.view(3, 3)[:, 0], score)
    assert bool((scores.view(3, 3)[:, :-1] >= scores.view(3, 3)[:, 1:]).all())
    assert m.generate(x, mask, max_new_tokens=T, num_beams=3, num_return_sequences=2).shape == (6, T)


RETURN_CASES = [(seed, K, lp, early, N) for seed in range(4) for K, N in ((2, 2), (4, 2), (4, 4))
                for lp in (1.0, 0.6) for early in (True, False)]


@pytest.fixture(scope="module")
def library_models():
    pytest.importorskip("transformers")
    models = {}
    for seed in range(4):
        hf = _library_model(seed)
        ours = T5ForConditionalGeneration.from_hf_config(hf.config, dtype=torch.float32).eval()
        ours.load_hf_state_dict(hf.state_dict())
        models[seed] = (hf, ours, *_inputs(seed))
    return models


@pytest.mark.parametrize("seed,K,lp,early,N", RETURN_CASES)
def test_beam_return_sequences_match_library(library_models, seed, K, lp, early, N):
    hf, ours, x, mask = library_models[seed]
    with torch.no_grad():
        y = hf.generate(input_ids=x, attention_mask=mask, max_new_tokens=T, num_beams=K, length_penalty=lp,
                        early_stopping=early, do_sample=False, num_return_sequences=N, output_scores=True,
                        return_dict_in_generate=True)
    want = torch.nn.functional.pad(y.sequences[:, 1:], (0, T - (y.sequences.shape[1] - 1)))
    got, score = ours.generate(x, mask, max_new_tokens=T, num_beams=K, length_penalty=lp, early_stopping=early,
                               num_return_sequences=N, return_scores=True)
    assert got.shape == (3 * N, T) and score.shape == (3 * N,)
    assert torch.equal(got, _cut(want))
    torch.testing.assert_close(score, y.sequences_scores, rtol=1e-4, atol=1e-5)


def test_argument_validation():
    m = _tiny(0)
    x, mask = _inputs(0)
    for bad in (dict(temperature=0.0), dict(temperature=float("inf")), dict(temperature=float("nan")),
                dict(temperature=-1.0), dict(repetition_penalty=0.0), dict(repetition_penalty=float("nan")),
                dict(top_p=0.0), dict(top_p=1.5), dict(top_k=-1), dict(top_k=2.5), dict(num_return_sequences=0),
                dict(num_return_sequences=1.5), dict(seed=-1), dict(seed=2 ** 63), dict(seed=1.5)):
        with pytest.raises(ValueError, match=next(iter(bad))):
            m.generate(x, mask, do_sample=True, **bad)
    for ignored in (dict(temperature=0.7), dict(top_k=5), dict(top_p=0.9), dict(repetition_penalty=1.2), dict(seed=3)):
        with pytest.raises(ValueError, match="do_sample"):
            m.generate(x, mask, **ignored)
        with pytest.raises(ValueError, match="do_sample"):
            m.generate(x, mask, num_beams=2, **ignored)
    with pytest.raises(ValueError, match="beam sampling"):
        m.generate(x, mask, do_sample=True, num_beams=2)
    with pytest.raises(ValueError, match="num_return_sequences"):
        m.generate(x, mask, num_beams=2, num_return_sequences=3)
    with pytest.raises(ValueError, match="num_return_sequences"):
        m.generate(x, mask, num_return_sequences=2)
    with pytest.raises(ValueError, match="return_scores"):
        m.generate(x, mask, do_sample=True, return_scores=True)
    with pytest.raises(ValueError, match="return_scores"):
        m.generate(x, mask, do_sample=True, trace=[])
    with pytest.raises(ValueError, match="never"):
        m.generate(x, mask, num_beams=2, early_stopping="never")
    with pytest.raises(RuntimeError, match="GPU kernel"):
        S.sample_step(torch.zeros(1, 8), torch.zeros(1, 2, dtype=torch.long), torch.zeros(1, dtype=torch.bool),
                      torch.zeros(1, 1, dtype=torch.long), torch.zeros(1, dtype=torch.long),
                      torch.zeros(1, dtype=torch.long), 0, 1, 0)
