"""T5 training at d_kv 128 (the head dim of t5-3b / t5-11b) on the MFMA attention kernels:
tests/test_t5_train_gpu.py at d_kv = 128 (read its docstring for the criterion and the topology's
gated-GELU feed-forward).  Gradients of every parameter against the same weights in fp32, for the
kernel route and for ``CLOUDTIK_AMD_T5_TRAIN_ATTN=0`` (SDPA with the materialised bias); dropout
determinism; the kernels a step runs under either setting.

TOPOLOGY.  vocab 128, d_model 128, d_kv 128, d_ff 256, 2 + 2 layers, 2 heads, 8 buckets.  The
yardstick passes on its own with margin there: bf16 against fp32 on a CPU gave worst cosine
0.99965 and worst relative error 0.0265 (both on encoder.blocks.1.ln_sa.weight).  At d_model 256 /
d_ff 512 the same check gives 0.99915 / 0.041, too close to the criterion to measure a route.
"""
import pytest
import torch

from cloudtik_amd import ops
from cloudtik_amd.models.t5 import T5Config, T5ForConditionalGeneration
from test_t5_train_gpu import SWITCH, _agreement, _attn_kernel_names, _batch, _step

NEW = ("attn_fwd_d128_drop", "attn_bwd_d128", "attn_drel_reduce_kernel")


def _sdpa_names(names):
    """test_t5_train_gpu.py's: kernels of F.scaled_dot_product_attention (PyTorch's fused attention
    kernels, or the softmax of its math path), with the d128 dropout forward among this project's."""
    mine = ("attn_fwd_d64_kernel", "attn_fwd_d128_kernel", "attn_fwd_d128_drop_kernel", "attn_fwd_pipe_kernel")
    out = []
    for n in names:
        low = n.lower()
        if "softmax" in low or "fmha" in low or "flash" in low or "bwd_kernel_dk_dv" in low or "bwd_kernel_dq" in low:
            out.append(n)
        elif "attn_fwd" in low and not any(m in n for m in mine):
            out.append(n)
    return out


def _cfg(dropout=0.0):
    return T5Config(vocab_size=128, d_model=128, d_kv=128, d_ff=256, num_layers=2, num_decoder_layers=2, num_heads=2,
                    relative_attention_num_buckets=8, relative_attention_max_distance=16, dropout_rate=dropout,
                    gated_gelu=True)


def _model(device, dtype, dropout=0.0, like=None):
    torch.manual_seed(0)
    m = T5ForConditionalGeneration(_cfg(dropout), device=device, dtype=dtype)
    if like is not None:
        m.load_state_dict({k: v.to(device=device, dtype=dtype) for k, v in like.state_dict().items()})
    return m.train()


@pytest.mark.gpu
def test_gradients_against_fp32(cuda, monkeypatch):
    """Loss and every parameter gradient of the kernel route, and of the SDPA route, against the
    same weights in fp32 (CPU)."""
    model = _model(cuda, torch.bfloat16)
    ref32 = _model("cpu", torch.float32, like=model)
    loss32, want = _step(ref32, _batch("cpu"))
    assert all(torch.isfinite(g).all() and g.norm() > 0 for g in want.values())
    rel_names = [n for n in want if n.endswith("sa.rel.weight")]
    assert len(rel_names) == 2, rel_names
    results = {}
    for route, switch in (("kernels", "1"), ("sdpa", "0")):
        monkeypatch.setenv(SWITCH, switch)
        loss, grads = _step(model, _batch(cuda))
        agree = _agreement(grads, want)
        results[route] = (loss, agree)
        worst_cos = min(agree.items(), key=lambda kv: kv[1][0])
        worst_rel = max(agree.items(), key=lambda kv: kv[1][1])
        print("t5-xl-train %s: loss %.6f (fp32 %.6f) worst cosine %s %.6f, worst rel %s %.4f; rel-embedding %s" % (
            route, loss, loss32, worst_cos[0], worst_cos[1][0], worst_rel[0], worst_rel[1][1],
            {n: "%.6f / %.4f" % agree[n] for n in rel_names}))
    for route, (loss, agree) in results.items():
        assert abs(loss - loss32) <= 2e-2 * abs(loss32), (route, loss, loss32)
        for n, (cos, rel) in agree.items():
            assert cos > 0.999 and rel <= 0.05, (route, n, cos, rel)


@pytest.mark.gpu
def test_dropout_is_seeded(cuda, monkeypatch):
    """Dropout 0.1 (attention dropout inside the kernels, the rest in PyTorch): the same seeds give
    the same loss bit for bit, another ops seed a different one, and every gradient is finite."""
    monkeypatch.delenv(SWITCH, raising=False)
    model = _model(cuda, torch.bfloat16, dropout=0.1)
    batch = _batch(cuda)

    def run(seed):
        torch.manual_seed(3)
        ops.manual_seed(seed)
        return _step(model, batch)

    a, ga = run(21)
    b, _ = run(21)
    c, _ = run(22)
    assert torch.equal(a, b), (a, b)
    assert not torch.equal(a, c), (a, c)
    for n, g in ga.items():
        assert torch.isfinite(g).all(), n


@pytest.mark.gpu
def test_training_step_runs_the_d128_kernels(cuda, monkeypatch):
    """One training step in the default routing runs the d128 forward (with dropout) and backward
    kernels for all three attentions and the d_rel reduce kernel, and no SDPA kernel; with the switch
    off it runs SDPA and none of them."""
    monkeypatch.delenv(SWITCH, raising=False)
    model = _model(cuda, torch.bfloat16, dropout=0.1)
    batch = _batch(cuda)
    names = _attn_kernel_names(model, batch)
    for want in ("attn_fwd_d128_drop_kernel<false, true>",             # encoder self-attention
                 "attn_fwd_d128_drop_kernel<true, true>",              # decoder self-attention
                 "attn_fwd_d128_drop_kernel<false, false>",            # cross-attention
                 "attn_bwd_d128_kernel<true, false, false, true>", "attn_bwd_d128_kernel<true, true, false, true>",
                 "attn_bwd_d128_kernel<true, false, false, false>",
                 "attn_drel_reduce_kernel"):
        assert any(want in n for n in names), (want, sorted(set(n for n in names if "attn" in n)))
    assert not _sdpa_names(names), _sdpa_names(names)
    monkeypatch.setenv(SWITCH, "0")
    names = _attn_kernel_names(model, batch)
    assert _sdpa_names(names)
    assert not any(new in n for n in names for new in NEW), sorted(set(n for n in names if "attn_" in n))
