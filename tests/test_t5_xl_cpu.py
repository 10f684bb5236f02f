"""T5-3B / T5-11B topologies (d_kv = 128): parameter counts, ``from_hf_config``, and cached
generation at d_kv = 128 on the CPU."""
import torch

from cloudtik_amd.models.t5 import T5Config, T5ForConditionalGeneration


def _count(cfg):
    m = T5ForConditionalGeneration(cfg, device="meta", dtype=torch.float32)
    return sum(p.numel() for p in m.parameters())          # tied output head: counted once


def test_t5_xl_xxl_param_counts():
    assert _count(T5Config.xl()) == 2851598336              # HF t5-3b
    assert _count(T5Config.xxl()) == 11307321344            # HF t5-11b
    for cfg, heads in ((T5Config.xl(), 32), (T5Config.xxl(), 128)):
        assert (cfg.d_model, cfg.d_kv, cfg.num_heads, cfg.num_layers, cfg.num_decoder_layers) == (1024, 128, heads, 24, 24)


def test_from_hf_config_keeps_d_kv():
    """t5-3b's own numbers: d_model // num_heads = 32, d_kv = 128."""
    hf = dict(vocab_size=512, d_model=1024, d_kv=128, d_ff=64, num_layers=1, num_decoder_layers=1, num_heads=32,
              relative_attention_num_buckets=8, feed_forward_proj="relu")
    m = T5ForConditionalGeneration.from_hf_config(hf, device="meta", dtype=torch.float32)
    assert m.cfg.d_kv == 128 and m.cfg.d_model // m.cfg.num_heads == 32
    sa = m.encoder.blocks[0].sa
    assert sa.q.weight.shape == (32 * 128, 1024) and sa.o.weight.shape == (1024, 32 * 128)


def test_d_kv_128_cached_generation_equals_uncached_cpu():
    torch.manual_seed(0)
    cfg = T5Config.tiny(vocab_size=64, d_model=32, d_kv=128, num_heads=2)
    m = T5ForConditionalGeneration(cfg, dtype=torch.float32).eval()
    x = torch.randint(2, 64, (3, 10))
    g = m.generate(x, max_new_tokens=6)
    with torch.no_grad():
        enc, _ = m.encoder(x)
        ids = torch.cat([torch.zeros(3, 1, dtype=torch.long), g[:, :5]], 1)
        dec, _ = m.decoder(ids, enc=enc)
    # rows that ended keep emitting pad; compare up to and including each row's first EOS
    full = m.logits(dec).argmax(-1)
    done = torch.zeros(3, dtype=torch.bool)
    for t in range(6):
        assert torch.equal(full[~done, t], g[~done, t])
        done |= g[:, t] == cfg.eos_token_id
