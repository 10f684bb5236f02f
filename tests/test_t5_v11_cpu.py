"""T5 v1.1 / Flan-T5 on the CPU: ``from_pretrained`` of a directory the installed ``transformers``
saved from a tiny gated-GELU model with an untied head, in the form the library writes and in the
published form of the config, single file and sharded; logits, loss, greedy and beam tokens against
the library; the loader's refusals; the presets; the int8 model of an untied model."""
import json
import os

import pytest
import torch

from cloudtik_amd.models.t5 import T5Config, T5ForConditionalGeneration
from cloudtik_amd.models.t5_quant import QuantT5ForConditionalGeneration

T = 8
SEEDS = (0, 1, 2)
V = 24

HF_CONFIG = dict(vocab_size=V, d_model=32, d_kv=8, d_ff=64, num_layers=2, num_decoder_layers=2, num_heads=4,
                 relative_attention_num_buckets=8, relative_attention_max_distance=16, dropout_rate=0.0,
                 feed_forward_proj="gated-gelu", tie_word_embeddings=False, pad_token_id=0, eos_token_id=1,
                 decoder_start_token_id=0)


def _cut(seq, eos=1, pad=0):
    """Pad after the first EOS."""
    seq = seq.clone()
    after = ((seq == eos).long().cumsum(1) - (seq == eos).long()) > 0
    seq[after] = pad
    return seq


def _inputs(seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(2, V, (3, 7), generator=g)
    mask = torch.ones(3, 7, dtype=torch.long)
    mask[2, 5:] = 0
    return x, mask


def _library_model(seed):
    """A tiny v1.1 model of the library with a head of its own.  The library builds it with the head
    sharing the embedding, whatever the config says; assigning a new parameter unties it."""
    transformers = pytest.importorskip("transformers")
    torch.manual_seed(seed)
    hf = transformers.T5ForConditionalGeneration(transformers.T5Config(**HF_CONFIG)).eval()
    with torch.no_grad():
        for p in hf.parameters():
            if p.dim() > 1:
                p.normal_(0.0, 0.5)
    hf.lm_head.weight = torch.nn.Parameter(torch.randn(V, HF_CONFIG["d_model"]) * 0.5)
    assert hf.lm_head.weight.data_ptr() != hf.shared.weight.data_ptr()
    return hf


@pytest.fixture(scope="module")
def saved(tmp_path_factory):
    """Per seed: the library model, the directory it was saved to, ours loaded from it, the inputs."""
    pytest.importorskip("transformers")
    out = {}
    for seed in SEEDS:
        hf = _library_model(seed)
        d = tmp_path_factory.mktemp(f"v11_{seed}")
        hf.save_pretrained(d)
        ours = T5ForConditionalGeneration.from_pretrained(d, dtype=torch.float32).eval()
        out[seed] = (hf, str(d), ours, *_inputs(seed))
    return out


def _logits(model, x, mask, dec_ids):
    with torch.no_grad():
        enc, _ = model.encoder(x, mask)
        dec, _ = model.decoder(dec_ids, enc=enc, enc_mask=mask)
        return model.logits(dec)


def _assert_matches_library(ours, hf, x, mask, seed):
    """Teacher-forced logits to 1e-4 absolute (3.5e-6 measured at this size at a logit scale of about
    10; the margin covers other seeds), the training loss with ignored labels, greedy tokens, and
    3-beam tokens and scores."""
    g = torch.Generator().manual_seed(100 + seed)
    dec_ids = torch.randint(0, V, (3, T), generator=g)
    labels = torch.randint(2, V, (3, T), generator=g)
    labels[1, 5:] = -100
    with torch.no_grad():
        want = hf(input_ids=x, attention_mask=mask, decoder_input_ids=dec_ids).logits
        want_loss = hf(input_ids=x, attention_mask=mask, labels=labels).loss
        got_loss = ours(x, labels, mask)
    got = _logits(ours, x, mask, dec_ids)
    err = (got - want).abs().max().item()
    print(f"seed {seed}: max |logit error| {err:.2e} at scale {want.abs().max().item():.1f}")
    assert err <= 1e-4
    torch.testing.assert_close(got_loss, want_loss, rtol=1e-5, atol=1e-5)
    with torch.no_grad():
        greedy = hf.generate(input_ids=x, attention_mask=mask, max_new_tokens=T, num_beams=1, do_sample=False)[:, 1:]
        y = hf.generate(input_ids=x, attention_mask=mask, max_new_tokens=T, num_beams=3, do_sample=False,
                        output_scores=True, return_dict_in_generate=True)
    ref = torch.nn.functional.pad(greedy, (0, T - greedy.shape[1]))
    assert torch.equal(_cut(ours.generate(x, mask, max_new_tokens=T)), _cut(ref))
    beam = torch.nn.functional.pad(y.sequences[:, 1:], (0, T - (y.sequences.shape[1] - 1)))
    seq, score = ours.generate(x, mask, max_new_tokens=T, num_beams=3, return_scores=True)
    assert torch.equal(seq, _cut(beam))
    torch.testing.assert_close(score, y.sequences_scores, rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("seed", SEEDS)
def test_from_pretrained_matches_library(saved, seed):
    hf, d, ours, x, mask = saved[seed]
    cfg = ours.cfg
    assert cfg.gated_gelu and not cfg.tie_word_embeddings and not cfg.scales_outputs
    assert ours.dtype == torch.float32 and ours.lm_head.weight.dtype == torch.float32
    assert torch.equal(ours.lm_head.weight, hf.lm_head.weight)
    assert not torch.equal(ours.lm_head.weight, ours.shared.weight)
    _assert_matches_library(ours, hf, x, mask, seed)


def test_head_is_the_untied_one(saved):
    """The logits are the unscaled product with ``lm_head``: not the embedding, not scaled."""
    _, _, ours, x, mask = saved[0]
    dec_ids = torch.zeros(3, 2, dtype=torch.long)
    with torch.no_grad():
        enc, _ = ours.encoder(x, mask)
        dec, _ = ours.decoder(dec_ids, enc=enc, enc_mask=mask)
    assert torch.equal(ours.logits(dec), torch.nn.functional.linear(dec, ours.lm_head.weight))


@pytest.mark.parametrize("seed", SEEDS)
def test_published_config_shape(saved, tmp_path, seed):
    """A published Flan-T5 ``config.json``: ``tie_word_embeddings: false`` and no ``scale_decoder_outputs``."""
    hf, d, first, x, mask = saved[seed]
    with open(os.path.join(d, "config.json")) as f:
        config = json.load(f)
    config.pop("scale_decoder_outputs", None)
    config["tie_word_embeddings"] = False
    with open(tmp_path / "config.json", "w") as f:
        json.dump(config, f)
    os.symlink(os.path.join(d, "model.safetensors"), tmp_path / "model.safetensors")
    ours = T5ForConditionalGeneration.from_pretrained(tmp_path, dtype=torch.float32).eval()
    assert not ours.cfg.tie_word_embeddings and not ours.cfg.scales_outputs
    for (n, a), (_, b) in zip(ours.state_dict().items(), first.state_dict().items()):
        assert torch.equal(a, b), n
    _assert_matches_library(ours, hf, x, mask, seed)


@pytest.mark.parametrize("fmt", ["safetensors", "bin"])
def test_sharded_checkpoint(saved, tmp_path, fmt):
    """The checkpoint split by hand into two files and an index loads equal to the unsharded one."""
    from safetensors.torch import load_file, save_file
    _, d, first, _, _ = saved[1]
    sd = load_file(os.path.join(d, "model.safetensors"))
    names = sorted(sd)
    halves = (names[:len(names) // 2], names[len(names) // 2:])
    stem, ext = ("model", "safetensors") if fmt == "safetensors" else ("pytorch_model", "bin")
    weight_map = {}
    for i, half in enumerate(halves):
        shard = f"{stem}-{i + 1:05d}-of-00002.{ext}"
        part = {k: sd[k].contiguous() for k in half}
        if fmt == "safetensors":
            save_file(part, str(tmp_path / shard))
        else:
            torch.save(part, tmp_path / shard)
        weight_map.update({k: shard for k in half})
    with open(tmp_path / f"{stem}.{ext}.index.json", "w") as f:
        json.dump({"metadata": {}, "weight_map": weight_map}, f)
    with open(os.path.join(d, "config.json")) as f, open(tmp_path / "config.json", "w") as out:
        out.write(f.read())
    ours = T5ForConditionalGeneration.from_pretrained(tmp_path, dtype=torch.float32)
    assert [n for n, _ in ours.state_dict().items()] == [n for n, _ in first.state_dict().items()]
    for (n, a), (_, b) in zip(ours.state_dict().items(), first.state_dict().items()):
        assert torch.equal(a, b), n
    os.remove(tmp_path / weight_map[names[0]])
    with pytest.raises(FileNotFoundError):
        T5ForConditionalGeneration.from_pretrained(tmp_path, dtype=torch.float32)


def test_from_pretrained_is_local_only(tmp_path):
    with pytest.raises(FileNotFoundError, match="local checkpoint directory"):
        T5ForConditionalGeneration.from_pretrained("google/flan-t5-small")
    with open(tmp_path / "config.json", "w") as f:
        json.dump(HF_CONFIG, f)
    with pytest.raises(FileNotFoundError, match="no model.safetensors"):
        T5ForConditionalGeneration.from_pretrained(tmp_path)


def test_tied_checkpoint_stays_tied(tmp_path):
    """A v1.0 directory (ReLU, tied) through ``from_pretrained``: no ``lm_head``, the scaled head."""
    transformers = pytest.importorskip("transformers")
    torch.manual_seed(3)
    hf = transformers.T5ForConditionalGeneration(transformers.T5Config(
        **{**HF_CONFIG, "feed_forward_proj": "relu", "tie_word_embeddings": True})).eval()
    hf.save_pretrained(tmp_path)
    ours = T5ForConditionalGeneration.from_pretrained(tmp_path, dtype=torch.float32).eval()
    assert ours.cfg.tie_word_embeddings and ours.cfg.scales_outputs and not hasattr(ours, "lm_head")
    x, mask = _inputs(3)
    dec_ids = torch.zeros(3, 3, dtype=torch.long)
    with torch.no_grad():
        want = hf(input_ids=x, attention_mask=mask, decoder_input_ids=dec_ids).logits
    assert (_logits(ours, x, mask, dec_ids) - want).abs().max().item() <= 1e-4


def test_from_hf_config_untied_head():
    config = {k: v for k, v in HF_CONFIG.items()}
    with pytest.raises(ValueError, match="untied.*from_pretrained.*untied_head"):
        T5ForConditionalGeneration.from_hf_config(config)
    m = T5ForConditionalGeneration.from_hf_config(config, dtype=torch.float32, untied_head=True)
    assert not m.cfg.tie_word_embeddings and not m.cfg.scales_outputs
    assert m.lm_head.weight.shape == (V, 32) and "lm_head.weight" in dict(m.named_parameters())
    # the keys the library writes for the same model
    m = T5ForConditionalGeneration.from_hf_config({**config, "tie_word_embeddings": True, "scale_decoder_outputs": False},
                                                  dtype=torch.float32, untied_head=True)
    assert not m.cfg.tie_word_embeddings and not m.cfg.scales_outputs
    m = T5ForConditionalGeneration.from_hf_config({**config, "tie_word_embeddings": True, "scale_decoder_outputs": False},
                                                  dtype=torch.float32)
    assert m.cfg.tie_word_embeddings and not m.cfg.scales_outputs and not hasattr(m, "lm_head")
    m = T5ForConditionalGeneration.from_hf_config({**config, "scale_decoder_outputs": True}, dtype=torch.float32,
                                                  untied_head=True)
    assert m.cfg.scales_outputs


def test_load_hf_state_dict_on_an_untied_model(saved):
    hf, _, _, _, _ = saved[2]
    sd = hf.state_dict()
    ours = T5ForConditionalGeneration.from_hf_config(HF_CONFIG, dtype=torch.float32, untied_head=True)
    ours.load_hf_state_dict(sd)
    assert torch.equal(ours.lm_head.weight, sd["lm_head.weight"])
    with pytest.raises(KeyError, match="missing keys.*lm_head.weight"):
        ours.load_hf_state_dict({k: v for k, v in sd.items() if k != "lm_head.weight"})
    with pytest.raises(ValueError, match="shape"):
        ours.load_hf_state_dict({**sd, "lm_head.weight": torch.zeros(V + 1, 32)})
    with pytest.raises(ValueError, match="embed_tokens.weight differs"):
        ours.load_hf_state_dict({**sd, "encoder.embed_tokens.weight": sd["shared.weight"] + 1})
    tied = T5ForConditionalGeneration.from_hf_config({**HF_CONFIG, "tie_word_embeddings": True}, dtype=torch.float32)
    with pytest.raises(ValueError, match="untied"):
        tied.load_hf_state_dict(sd)


def test_presets():
    table = {"small": (512, 1024, 8, 6), "base": (768, 2048, 12, 12), "large": (1024, 2816, 24, 16),
             "xl": (2048, 5120, 24, 32), "xxl": (4096, 10240, 24, 64)}
    for size, (d_model, d_ff, layers, heads) in table.items():
        c = T5Config.v1_1(size)
        assert (c.d_model, c.d_ff, c.num_layers, c.num_decoder_layers, c.num_heads) == (d_model, d_ff, layers, layers, heads)
        assert c.d_kv == 64 and c.gated_gelu and not c.tie_word_embeddings and not c.scales_outputs
        assert c.vocab_size == 32128
    assert T5Config.v1_1("base", dropout_rate=0.0).dropout_rate == 0.0
    with pytest.raises(ValueError, match="unknown"):
        T5Config.v1_1("huge")
    # the defaults are the tied, scaled head of v1.0
    assert T5Config().tie_word_embeddings and T5Config().scales_outputs and T5Config.base().scale_decoder_outputs is None


def test_untied_model_trains_its_head():
    torch.manual_seed(0)
    m = T5ForConditionalGeneration(T5Config.tiny(gated_gelu=True, tie_word_embeddings=False), dtype=torch.float32).train()
    x = torch.randint(2, 64, (2, 5))
    labels = torch.randint(2, 64, (2, 4))
    m(x, labels).backward()
    assert m.lm_head.weight.grad is not None and m.lm_head.weight.grad.abs().sum() > 0
    # rows of the embedding no input or decoder token selects get nothing from the head
    used = set(x.view(-1).tolist()) | set(m._shift_right(labels).view(-1).tolist())
    unused = [t for t in range(64) if t not in used]
    assert unused and not m.shared.weight.grad[unused].any()


@pytest.mark.parametrize("seed", SEEDS)
def test_int8_of_an_untied_model(seed):
    """Relative L2 error of the teacher-forced logits below 0.02, the bound of test_t5_quant_cpu.py at the
    same topology (measured here with the random untied head: 0.0121 - 0.0133 over seeds 0 - 5, against
    0.0087 - 0.0115 tied); the same greedy tokens; the state dict holds the int8 head and no float ``lm_head``.

    THE TOKENS.  Equal greedy tokens need a float model that has decided: a top-2 margin above the int8
    error of a logit, which the 0.02 bound lets reach 0.05 - 0.06 of a row's RMS (measured, seeds 0 - 5).
    The tied random model of test_t5_quant_cpu.py has decided, margin >= 4.5 RMS at every step, because
    a token's own embedding row dominates its logit.  A random head of its own prefers no token: its
    smallest margin over 12 steps is 0.001 - 0.27 RMS, and the int8 tokens leave the float ones at such a
    step in 3 of 6 seeds (1, 3, 5), which says nothing about the head.  So the tokens are compared on a
    head that is untied AND decided (the embedding's direction plus noise of its own, scaled so that the
    unscaled logits have the tied model's size), and the random head is held to the error bound."""
    torch.manual_seed(seed)
    cfg = T5Config(vocab_size=192, d_model=128, d_kv=64, num_heads=2, d_ff=256, num_layers=2, num_decoder_layers=2,
                   relative_attention_num_buckets=8, dropout_rate=0.0, gated_gelu=True, tie_word_embeddings=False)
    m = T5ForConditionalGeneration(cfg, dtype=torch.float32).eval()
    g = torch.Generator().manual_seed(100 + seed)
    ids = torch.randint(2, 192, (3, 9), generator=g)
    dec_ids = torch.randint(2, 192, (3, 7), generator=g)

    def error(model):
        q = model.quantize_dynamic()
        assert isinstance(q, QuantT5ForConditionalGeneration)
        a, b = _logits(q, ids, None, dec_ids).float(), _logits(model, ids, None, dec_ids)
        return q, ((a - b).norm() / b.norm()).item()

    q, rel = error(m)
    assert 0 < rel < 0.02
    with torch.no_grad():
        m.lm_head.weight.copy_(m.shared.weight * cfg.d_model ** -0.5 + 0.02 * torch.randn(192, 128, generator=g))
    assert not torch.equal(m.lm_head.weight, m.shared.weight)
    q, rel_decided = error(m)
    print(f"untied seed={seed}: rel {rel:.5f} (random head) {rel_decided:.5f} (decided head)")
    assert 0 < rel_decided < 0.02
    assert torch.equal(q.generate(ids, max_new_tokens=12), m.generate(ids, max_new_tokens=12))
    keys = set(q.state_dict())
    assert "head.w_q" in keys and "head.w_scale" in keys and "lm_head.weight" not in keys
    tied_keys = set(T5ForConditionalGeneration(T5Config.tiny(gated_gelu=True), dtype=torch.float32)
                    .quantize_dynamic().state_dict())
    assert {k for k in keys if "blocks" not in k} == {k for k in tied_keys if "blocks" not in k}
    # the head is lm_head's rows, unscaled
    w = m.lm_head.weight
    deq = q.head.w_q.float() * q.head.w_scale[:, None]
    assert ((deq - w).abs().max() <= w.abs().amax(1).max() / 127).item()
    # a skeleton takes the state dict
    skel = QuantT5ForConditionalGeneration(cfg, dtype=torch.float32)
    skel.load_state_dict(q.state_dict())
    assert torch.equal(_logits(skel, ids, None, dec_ids), _logits(q, ids, None, dec_ids))
