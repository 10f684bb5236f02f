"""T5 at d_kv = 128 (the head dim of t5-3b / t5-11b) on the GPU, on a tiny topology: the kernel
path against the SDPA path, graph-replayed against eager generation in every mode, the int8 model,
and the kernels a decode step runs.  Nothing here instantiates the 3B / 11B weights."""
import pytest
import torch

from cloudtik_amd.models.t5 import T5Config, T5ForConditionalGeneration

pytestmark = pytest.mark.gpu

STEPS = 10


def _cfg():
    return T5Config(vocab_size=512, d_model=256, d_kv=128, d_ff=512, num_layers=2, num_decoder_layers=2, num_heads=2,
                    relative_attention_num_buckets=8, relative_attention_max_distance=16, dropout_rate=0.0)


@pytest.fixture(scope="module")
def model(cuda):
    torch.manual_seed(0)
    return T5ForConditionalGeneration(_cfg(), device=cuda).eval()


@pytest.fixture(scope="module")
def sources(cuda):
    """Batch 3, one padded source."""
    g = torch.Generator().manual_seed(3)
    x = torch.randint(2, 512, (3, 24), generator=g).to(cuda)
    mask = torch.ones_like(x)
    mask[2, 18:] = 0
    return x, mask


def _kernel_names(fn):
    from torch.profiler import ProfilerActivity, profile
    fn()                                                                  # warm
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]


def test_encoder_kernel_path_matches_sdpa_path(cuda, sources):
    """The encoder through attn_fwd_d128_kernel == the materialised-bias SDPA path of the same
    weights (training mode with grad), at the tolerance test_t5_kernel_path_matches_sdpa_path uses."""
    torch.manual_seed(0)
    m = T5ForConditionalGeneration(_cfg(), device=cuda).eval()
    x, mask = sources
    with torch.no_grad():
        names = _kernel_names(lambda: m.encoder(x, mask))
        enc_k, _ = m.encoder(x, mask)
    assert sum("attn_fwd_d128_kernel<false, true>" in n for n in names) == 2, names
    m.train()
    enc_s, _ = m.encoder(x, mask)
    torch.testing.assert_close(enc_k.float(), enc_s.detach().float(), atol=5e-2, rtol=5e-2)


def test_graph_greedy_matches_eager(model, sources):
    x, mask = sources
    eager = model.generate(x, mask, max_new_tokens=STEPS, use_graph=False)
    graph = model._generate_graph(x, mask, STEPS)
    assert graph.shape == (3, STEPS) and torch.equal(eager, graph)


def test_graph_beam_matches_eager(model, sources):
    x, mask = sources
    got, score = model.generate(x, mask, max_new_tokens=STEPS, num_beams=4, num_return_sequences=2, return_scores=True)
    assert got.shape == (6, STEPS) and score.shape == (6,)
    eager, e_score = model._generate_beam_static(x, mask, STEPS, 4, 1.0, False, graph=False, num_return=2)
    assert torch.equal(got, eager)
    torch.testing.assert_close(score, e_score, rtol=1e-5, atol=0)


def test_graph_sampling_matches_eager(model, sources):
    x, mask = sources
    got = model.generate(x, mask, max_new_tokens=STEPS, do_sample=True, top_k=50, top_p=0.95, seed=7)
    assert got.shape == (3, STEPS)
    assert torch.equal(got, model._generate_sample_static(x, mask, STEPS, 1, 7, top_k=50, top_p=0.95, graph=False))


def test_graph_bans_match_eager(model, sources):
    x, mask = sources
    rule = dict(no_repeat_ngram_size=2, min_length=5)
    got = model.generate(x, mask, max_new_tokens=STEPS, **rule)
    assert torch.equal(got, model.generate(x, mask, max_new_tokens=STEPS, use_graph=False, **rule))
    assert (got[:, :4] != model.cfg.eos_token_id).all()                   # min_length counts the start token


def _greedy_state(m, B):
    keys = [k for k in m._graphs if k[0] == B]
    assert len(keys) == 1, keys
    return m._graphs[keys[0]]


def _attention_kernels_of_step(names):
    """The d128 kernels of one decode step of the 2-layer decoder: self-attention <false, true>
    (relative bias) and cross-attention <false, false>, two each, and nothing of the fallback
    (an fp32 softmax over materialised scores between two batched matrix products)."""
    assert sum("attn_fwd_d128_kernel<false, true>" in n for n in names) == 2, names
    assert sum("attn_fwd_d128_kernel<false, false>" in n for n in names) == 2, names
    assert not [n for n in names if "softmax" in n.lower() or "bmm" in n.lower()], names
    assert not [n for n in names if "attn_fwd_d64" in n], names


def test_int8_model_graph_greedy_and_kernels(model, sources):
    """quantize_dynamic() of the model: models/t5_quant.py calls the same two wrappers, so its
    decode step runs the d128 kernel; graph-replayed == the same step run eagerly."""
    x, mask = sources
    qm = model.quantize_dynamic()
    got = qm.generate(x, mask, max_new_tokens=STEPS)
    st = _greedy_state(qm, 3)
    st["reset"]()
    for _ in range(STEPS):
        st["step"]()
    assert got.shape == (3, STEPS) and torch.equal(got, st["out"].clone())
    st["reset"]()
    _attention_kernels_of_step(_kernel_names(st["step"]))


def test_decode_step_runs_d128_kernel(sources, cuda):
    """One replay of the captured greedy step, by kernel name from the profiler."""
    torch.manual_seed(0)
    m = T5ForConditionalGeneration(_cfg(), device=cuda).eval()
    x, mask = sources
    m.generate(x, mask, max_new_tokens=STEPS)
    st = _greedy_state(m, 3)
    st["reset"]()
    names = _kernel_names(st["graph"].replay)
    print("decode step kernels (replay): %d" % len(names))
    _attention_kernels_of_step(names)
