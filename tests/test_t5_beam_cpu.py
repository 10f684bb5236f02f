"""T5 beam search on the CPU: the reference rules (ops/beam.py) and ``generate(num_beams=K)``
against the beam search of the installed ``transformers`` on tiny random models, the weight
loader, and properties that need no oracle (greedy unchanged, never below greedy, exhaustive
search, argument checks)."""
import itertools

import pytest
import torch

from cloudtik_amd.models.t5 import T5Config, T5ForConditionalGeneration
from cloudtik_amd.ops import beam as beam_ops

T = 8
SEEDS = range(10)
BEAMS = (2, 4)
PENALTIES = (1.0, 0.6, 2.0)
EARLY = (True, False)
CASES = list(itertools.product(SEEDS, BEAMS, PENALTIES, EARLY))

HF_CONFIG = dict(vocab_size=24, d_model=32, d_kv=8, d_ff=64, num_layers=2, num_decoder_layers=2, num_heads=4,
                 relative_attention_num_buckets=8, relative_attention_max_distance=16, dropout_rate=0.0,
                 feed_forward_proj="relu", tie_word_embeddings=True, pad_token_id=0, eos_token_id=1,
                 decoder_start_token_id=0)


def _cut(seq, eos=1, pad=0):
    """Pad after the first EOS."""
    seq = seq.clone()
    after = ((seq == eos).long().cumsum(1) - (seq == eos).long()) > 0
    seq[after] = pad
    return seq


def _inputs(seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(2, 24, (3, 7), generator=g)
    mask = torch.ones(3, 7, dtype=torch.long)
    mask[2, 5:] = 0
    return x, mask


def _library_model(seed):
    transformers = pytest.importorskip("transformers")
    torch.manual_seed(seed)
    hf = transformers.T5ForConditionalGeneration(transformers.T5Config(**HF_CONFIG)).eval()
    with torch.no_grad():
        for p in hf.parameters():
            if p.dim() > 1:
                p.normal_(0.0, 0.5)
    return hf


@pytest.fixture(scope="module")
def library():
    """Per seed the library model, ours loaded from it, the inputs; per case the library's K
    best hypotheses [3, K, T], best first (start token dropped, padded to T)."""
    pytest.importorskip("transformers")
    models, outs = {}, {}
    for seed in SEEDS:
        hf = _library_model(seed)
        ours = T5ForConditionalGeneration.from_hf_config(hf.config, dtype=torch.float32).eval()
        ours.load_hf_state_dict(hf.state_dict())
        models[seed] = (hf, ours, *_inputs(seed))
    for seed, K, lp, early in CASES:
        hf, _, x, mask = models[seed]
        with torch.no_grad():
            y = hf.generate(input_ids=x, attention_mask=mask, max_new_tokens=T, num_beams=K, length_penalty=lp,
                            early_stopping=early, do_sample=False, num_return_sequences=K)[:, 1:]
        outs[seed, K, lp, early] = torch.nn.functional.pad(y, (0, T - y.shape[1])).view(3, K, T)
    return models, outs


@pytest.mark.parametrize("seed", SEEDS)
def test_loaded_model_logits_match_library(library, seed):
    hf, ours, x, mask = library[0][seed]
    g = torch.Generator().manual_seed(100 + seed)
    dec_ids = torch.randint(0, 24, (3, T), generator=g)
    with torch.no_grad():
        want = hf(input_ids=x, attention_mask=mask, decoder_input_ids=dec_ids).logits
        enc, _ = ours.encoder(x, mask)
        dec, _ = ours.decoder(dec_ids, enc=enc, enc_mask=mask)
        got = ours.logits(dec)
    torch.testing.assert_close(got, want, rtol=1e-5, atol=1e-5)
    greedy = hf.generate(input_ids=x, attention_mask=mask, max_new_tokens=T, num_beams=1, do_sample=False)[:, 1:]
    ref = torch.zeros(3, T, dtype=torch.long)
    ref[:, :greedy.shape[1]] = greedy
    assert torch.equal(_cut(ours.generate(x, mask, max_new_tokens=T)), _cut(ref))


@pytest.mark.parametrize("seed,K,lp,early", CASES)
def test_beam_search_matches_library(library, seed, K, lp, early):
    models, outs = library
    _, ours, x, mask = models[seed]
    got = ours.generate(x, mask, max_new_tokens=T, num_beams=K, length_penalty=lp, early_stopping=early)
    assert got.shape == (3, T) and got.dtype == torch.long
    assert torch.equal(_cut(got), got)                                   # already pad after EOS
    assert torch.equal(got, _cut(outs[seed, K, lp, early][:, 0]))


def test_oracle_cases_cover_eos_and_full_finished_sets(library):
    """On the library's output alone: enough cases end early for the comparison to exercise the
    finished-set and stopping rules."""
    _, outs = library
    with_eos = sum(bool((o[:, 0, :-1] == 1).any()) for o in outs.values())
    assert with_eos >= 0.2 * len(CASES), with_eos
    # an item finished K hypotheses before T: all K it returns end before the last position
    full = sum(bool((o[:, :, :-1] == 1).any(2).all(1).any()) for o in outs.values())
    assert full >= 5, full


# ------------------------------------------------------------------------------ no oracle
def _tiny(seed, **kw):
    torch.manual_seed(seed)
    m = T5ForConditionalGeneration(T5Config.tiny(**kw), dtype=torch.float32).eval()
    with torch.no_grad():
        for p in m.parameters():
            if p.dim() > 1:
                p.normal_(0.0, 0.5)
    return m


def _sequence_logprob(model, x, mask, seq):
    """Sum of log-probabilities of ``seq`` [B, T] up to and including its first EOS (or T)."""
    with torch.no_grad():
        enc, _ = model.encoder(x, mask)
        dec, _ = model.decoder(model._shift_right(seq), enc=enc, enc_mask=mask)
        lp = torch.log_softmax(model.logits(dec).float(), -1).gather(2, seq[:, :, None])[:, :, 0]
    eos = seq == model.cfg.eos_token_id
    live = (eos.long().cumsum(1) - eos.long()) == 0
    return (lp * live).sum(1)


def test_one_beam_is_todays_greedy():
    m = _tiny(0)
    x, mask = _inputs(3)
    want = m.generate(x, mask, max_new_tokens=T)
    assert torch.equal(m.generate(x, mask, max_new_tokens=T, num_beams=1, length_penalty=2.0, early_stopping=True), want)
    # the same tokens as the plain loop: arg-max, pad once EOS came
    enc, _ = m.encoder(x, mask)
    cur = torch.zeros(3, 1, dtype=torch.long)
    done = torch.zeros(3, dtype=torch.bool)
    for t in range(T):
        dec, _ = m.decoder(cur, enc=enc, enc_mask=mask)
        nxt = m.logits(dec[:, -1]).argmax(-1).masked_fill(done, 0)
        assert torch.equal(want[:, t], nxt)
        done |= nxt == 1
        cur = torch.cat([cur, nxt[:, None]], 1)


@pytest.mark.parametrize("K", [2, 3, 8])
def test_beam_never_scores_below_greedy(K):
    """length_penalty 0: the score is the summed log-probability, and greedy's path is what beam
    0 follows until a better one displaces it."""
    for seed in range(4):
        m = _tiny(seed)
        x, mask = _inputs(seed)
        greedy = m.generate(x, mask, max_new_tokens=T)
        seq, score = m.generate(x, mask, max_new_tokens=T, num_beams=K, length_penalty=0.0, return_scores=True)
        torch.testing.assert_close(score, _sequence_logprob(m, x, mask, seq), rtol=1e-5, atol=1e-5)
        assert (score >= _sequence_logprob(m, x, mask, greedy) - 1e-5).all()


def test_exhaustive_search_finds_the_best_sequence():
    """V = 6, T = 3 and K = V**2 = 36 beams: no live continuation is ever pruned, so the best
    finished hypothesis is the arg-max over all sequences under the same score.  K is beyond
    ``generate``'s limit, so the reference step is driven directly, with random logits after
    every prefix.  (V < 2K: dead beams' -1e9 candidates fill the spare ranks, and never win.)"""
    V, Tn, K, eos, pad = 6, 3, 36, 1, 0
    g = torch.Generator().manual_seed(5)

    def code(prefix):                                                 # prefix tokens -> row of tables[len]
        c = 0
        for tok in prefix:
            c = c * V + int(tok)
        return c

    for lp in (0.0, 1.0, 2.0):
        tables = [torch.randn(2, V ** t, V, generator=g) * 2 for t in range(Tn)]
        state = beam_ops.new_state(2, K, Tn, pad)
        len_pen = beam_ops.length_penalty_table(Tn, lp)
        for t in range(Tn):
            logits = torch.stack([tables[t][b, code(state["run_seq"][b, k, :t])] for b in range(2) for k in range(K)])
            state, _, _, _, _ = beam_ops.beam_step_reference(logits, state, t, len_pen, eos, False)
        for b in range(2):
            scored = {}
            for seq in itertools.product(range(V), repeat=Tn):
                total, out = 0.0, []
                for t, tok in enumerate(seq):
                    total += float(torch.log_softmax(tables[t][b, code(out)], -1)[tok])
                    out.append(tok)
                    if tok == eos:
                        break
                scored[tuple(out + [pad] * (Tn - len(out)))] = total / float(len(out)) ** lp
            best = max(scored, key=scored.get)
            assert state["fin_seq"][b, 0].tolist() == list(best)
            assert abs(float(state["fin_score"][b, 0]) - scored[best]) < 1e-5


def test_argument_validation():
    m = _tiny(0)
    x, mask = _inputs(0)
    with pytest.raises(ValueError, match="num_beams"):
        m.generate(x, mask, num_beams=9)
    with pytest.raises(ValueError, match="num_beams"):
        m.generate(x, mask, num_beams=0)
    with pytest.raises(ValueError, match="never"):
        m.generate(x, mask, num_beams=2, early_stopping="never")
    small = _tiny(0, vocab_size=7)
    with pytest.raises(ValueError, match="vocabulary"):
        small.generate(x % 7, mask, num_beams=4)
    assert small.generate(x % 7, mask, max_new_tokens=4, num_beams=3).shape == (3, 4)
    with pytest.raises(ValueError, match="return_scores"):
        m.generate(x, mask, return_scores=True)


def test_loader_rejects_missing_extra_and_untied_keys():
    pytest.importorskip("transformers")
    hf = _library_model(0)
    ours = T5ForConditionalGeneration.from_hf_config(hf.config.to_dict(), dtype=torch.float32)
    sd = dict(hf.state_dict())
    ours.load_hf_state_dict(sd)
    missing = {k: v for k, v in sd.items() if k != "decoder.block.1.layer.1.EncDecAttention.k.weight"}
    with pytest.raises(KeyError, match="missing keys.*EncDecAttention.k"):
        ours.load_hf_state_dict(missing)
    with pytest.raises(KeyError, match="unknown keys.*adapter"):
        ours.load_hf_state_dict({**sd, "decoder.adapter.weight": torch.zeros(1)})
    with pytest.raises(ValueError, match="untied"):
        ours.load_hf_state_dict({**sd, "lm_head.weight": sd["shared.weight"] + 1})
    with pytest.raises(ValueError, match="shape"):
        ours.load_hf_state_dict({**sd, "encoder.final_layer_norm.weight": torch.ones(5)})
    with pytest.raises(ValueError, match="untied"):
        T5ForConditionalGeneration.from_hf_config({**hf.config.to_dict(), "tie_word_embeddings": False})
