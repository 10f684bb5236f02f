"""The parts of head-dim-128 attention training that need no GPU: ``attention_relbias`` without a
bias vector, its reference route at D = 128, and the rounding model behind the bounds of
tests/test_attention_d128_bwd_gpu.py."""
import torch

from cloudtik_amd import ops
from cloudtik_amd.ops import reference as ref
from cloudtik_amd.ops.attention import _relbias_reference
import test_attention_d128_bwd_gpu as d128

SEED = 5


def _qkv(B=2, Sq=9, Sk=12, H=3, D=128, dtype=torch.float32):
    g = torch.Generator().manual_seed(Sq * 100 + Sk)
    q, k, v = (torch.randn(B, S, H, D, generator=g).mul(0.5).to(dtype) for S in (Sq, Sk, Sk))
    kb = torch.randn(B, Sk, generator=g) * 0.5
    kb[1, Sk - 3:] = -10000.0
    return q, k, v, kb


def test_no_bias_vector_is_reference_attention():
    """rel_bias=None: ops.reference.attention on the transposed layout, at p = 0 and at p > 0 from
    the stream the front end draws, for both head dims; and it backpropagates."""
    for D in (64, 128):
        q, k, v, kb = _qkv(D=D)
        for p, causal in ((0.0, False), (0.0, True), (0.25, False)):
            leaves = [t.clone().requires_grad_() for t in (q, k, v)]
            ops.manual_seed(SEED)
            got = ops.attention_relbias(*leaves, None, key_bias=kb, scale=0.2, causal=causal, p=p)
            ops.manual_seed(SEED)
            seed, off = ops._rng.next(2 * 3 * 9 * 12) if p > 0 else (0, 0)
            want = ref.attention(q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2), kb, p, seed, off, 0.2,
                                 causal).transpose(1, 2)
            assert got.shape == q.shape and torch.equal(got, want), (D, p, causal)
            got.sum().backward()
            assert all(t.grad is not None and torch.isfinite(t.grad).all() and t.grad.abs().sum() > 0 for t in leaves)
        if D == 128:
            ops.manual_seed(SEED)
            a = ops.attention_relbias(q, k, v, None, key_bias=kb, scale=0.2, p=0.25)
            ops.manual_seed(SEED + 1)
            b = ops.attention_relbias(q, k, v, None, key_bias=kb, scale=0.2, p=0.25)
            assert not torch.equal(a, b)


def test_bias_vector_at_d128_is_the_reference_on_cpu():
    """With rel_bias given, on the CPU, D = 128 still computes _relbias_reference, gradient of the
    bias vector included."""
    q, k, v, kb = _qkv()
    rel = torch.randn(3, 9 + 12 - 1, generator=torch.Generator().manual_seed(1)) * 0.5
    for p in (0.0, 0.25):
        leaves = [t.clone().requires_grad_() for t in (q, k, v, rel)]
        ops.manual_seed(SEED)
        got = ops.attention_relbias(*leaves, 8, kb, scale=0.2, causal=True, p=p)
        ops.manual_seed(SEED)
        seed, off = ops._rng.next(2 * 3 * 9 * 12) if p > 0 else (0, 0)
        leaves2 = [t.clone().requires_grad_() for t in (q, k, v, rel)]
        want = _relbias_reference(*leaves2, 8, kb, 0.2, True, p, seed, off)
        assert torch.equal(got, want)
        got.sum().backward()
        want.sum().backward()
        for a, b in zip(leaves, leaves2):
            assert torch.equal(a.grad, b.grad)


def test_rounding_model_within_recorded_table():
    """The rounding model's worst figures, recomputed on the two smallest shapes of the matrix, do
    not exceed the recorded table (so they pass the bounds by the factor of 4), and every class of
    the table occurs in them."""
    worst = d128.model_table([(1, 40), (64, 72)])
    print("model worst:", " ".join("%s=%.3e" % kv for kv in sorted(worst.items())))
    assert set(worst) == set(d128.MODEL_WORST)
    for n, e in worst.items():      # 2 %: another CPU's summation order
        assert 0 < e <= d128.MODEL_WORST[n] * 1.02, (n, e, d128.MODEL_WORST[n])
