"""Streamed persistent GEMM (csrc/gemm_nt.hip gemm_nt_stream_kernel) with the fused FFN epilogues
(6: bias + GELU storing gelu'; 7: multiply by the stored gelu') and its counted waits across
output-tile boundaries: against fp32 references, and bit for bit against the one-tile kernel,
which shares the K order, the MFMA order and the epilogue code.  Every case is launched ten
times into NaN-filled outputs: a wait that is too short reads LDS before a DMA has landed and
shows up now and then, not always.  Then the FFN block with its two fused GEMMs routed to the
streamed kernel against the one-tile routing, bit for bit."""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

# M, N, K, workgroups (0 = one per CU)
CASES = [
    (256, 256, 64, 0),        # one tile, one K-tile
    (512, 256, 128, 1),       # one workgroup, two tiles, the boundary next to the drain
    (1024, 768, 192, 5),      # 12 tiles over 5 workgroups, uneven tails, 3 K-tiles
    (1536, 512, 320, 3),      # 5 K-tiles
    (512, 512, 1024, 2),      # the production K depth, two tiles per workgroup
]
REPEATS = 10
bf = torch.bfloat16


def _C():
    from cloudtik_amd import ops
    return ops.require_native()


def _gelu(x):
    return 0.5 * x * (1 + torch.erf(x / math.sqrt(2)))


def _gelu_grad(x):
    return 0.5 * (1 + torch.erf(x / math.sqrt(2))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2 * math.pi)


def _rand(*shape, scale=1.0, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.randn(*shape, device="cuda", generator=g) * scale).to(bf)


def _close(out, ref, tol=2e-2):
    err = (out.float() - ref).abs().max().item()
    assert err <= tol * max(1.0, ref.abs().max().item()), err


def _nan(M, N):
    return torch.full((M, N), float("nan"), device="cuda", dtype=bf)


@functools.lru_cache(maxsize=None)
def _operands(M, N, K, b_kn):
    """Operands, the fp32 product and the one-tile kernel's outputs of one case: computed once,
    shared by the tests, never written again."""
    C = _C()
    A = _rand(M, K, seed=11)
    B = _rand(K, N, scale=K ** -0.5, seed=12) if b_kn else _rand(N, K, scale=K ** -0.5, seed=12)
    bias = _rand(N, scale=0.5, seed=13)
    aux_in = _rand(M, N, seed=14)            # EPI 7's stored derivative stand-in
    base = _rand(M, N, seed=15)              # accumulate: the old D
    ref = A.float() @ (B.float() if b_kn else B.float().t())
    one = C.gemm_nn if b_kn else C.gemm_nt
    tile = {}
    for name, epi, acc, b, aux in (("plain", 0, False, None, None), ("bias", 5, False, bias, None),
                                   ("acc", 0, True, None, None)):
        D = base.clone() if acc else _nan(M, N)
        assert one(A, B, D, epi, acc, b, aux, None)
        tile[name] = D
    if b_kn:
        D = _nan(M, N)
        assert C.gemm_nn(A, B, D, 7, False, None, aux_in, None)
        tile["epi7"] = D
    else:
        h, d = _nan(M, N), _nan(M, N)
        assert C.gemm_nt(A, B, h, 6, False, bias, d, None)
        tile["epi6"] = (h, d)
    torch.cuda.synchronize()
    return A, B, bias, aux_in, base, ref, tile


@pytest.mark.parametrize("M,N,K,wgs", CASES)
def test_stream_epi6_matches_reference_and_one_tile(M, N, K, wgs):
    C = _C()
    A, B, bias, _, _, ref, tile = _operands(M, N, K, False)
    z = ref + bias.float()
    h_ref, d_ref = _gelu(z), _gelu_grad(z)
    h1, d1 = tile["epi6"]
    for _ in range(REPEATS):
        h, d = _nan(M, N), _nan(M, N)
        assert C.gemm_nt_stream(A, B, h, bias, False, wgs, False, epi=6, aux=d)
        _close(h, h_ref)
        _close(d, d_ref)
        assert torch.equal(h, h1)
        assert torch.equal(d, d1)


@pytest.mark.parametrize("M,N,K,wgs", CASES)
def test_stream_epi7_matches_reference_and_one_tile(M, N, K, wgs):
    C = _C()
    A, B, _, aux_in, _, ref, tile = _operands(M, N, K, True)
    want = ref * aux_in.float()
    keep = aux_in.clone()
    for _ in range(REPEATS):
        D = _nan(M, N)
        assert C.gemm_nt_stream(A, B, D, None, True, wgs, False, epi=7, aux=aux_in)
        _close(D, want)
        assert torch.equal(D, tile["epi7"])
    assert torch.equal(aux_in, keep)         # EPI 7 only reads its aux operand


@pytest.mark.parametrize("b_kn", [False, True])
@pytest.mark.parametrize("M,N,K,wgs", CASES)
def test_stream_plain_bias_accumulate_bitwise(M, N, K, wgs, b_kn):
    """The wait plan on the instantiations that existed before it."""
    C = _C()
    A, B, bias, _, base, ref, tile = _operands(M, N, K, b_kn)
    _close(tile["plain"], ref)
    for _ in range(REPEATS):
        D = _nan(M, N)
        assert C.gemm_nt_stream(A, B, D, None, b_kn, wgs)
        assert torch.equal(D, tile["plain"])
        D = _nan(M, N)
        assert C.gemm_nt_stream(A, B, D, bias, b_kn, wgs)
        assert torch.equal(D, tile["bias"])
        D = base.clone()
        assert C.gemm_nt_stream(A, B, D, None, b_kn, wgs, True)
        assert torch.equal(D, tile["acc"])


def test_stream_refuses_what_it_does_not_have():
    C = _C()
    M, N, K = 512, 256, 128
    A, Bnt, Bkn = _rand(M, K, seed=1), _rand(N, K, seed=2), _rand(K, N, seed=3)
    bias, aux = _rand(N, seed=4), _rand(M, N, seed=5)
    aux0 = aux.clone()

    def untouched(D):
        torch.cuda.synchronize()
        return bool(torch.isnan(D).all()) and torch.equal(aux, aux0)

    D = _nan(M, N)
    assert not C.gemm_nt_stream(A, Bkn, D, bias, True, 0, False, epi=6, aux=aux)     # epi 6 is NT only
    assert untouched(D)
    assert not C.gemm_nt_stream(A, Bkn, D, None, True, 0, False, epi=7)              # epi 7 without aux
    assert untouched(D)
    assert not C.gemm_nt_stream(A, Bnt, D, bias, False, 0, True, epi=6, aux=aux)     # accumulate + epi 6
    assert untouched(D)
    assert not C.gemm_nt_stream(A, Bkn, D, None, True, 0, True, epi=7, aux=aux)      # accumulate + epi 7
    assert untouched(D)
    M2 = 384                                                                          # not whole tiles
    A2, D2, aux2 = _rand(M2, K, seed=6), _nan(M2, N), _rand(M2, N, seed=7)
    assert not C.gemm_nt_stream(A2, Bnt, D2, bias, False, 0, False, epi=6, aux=aux2)
    assert not C.gemm_nt_stream(A2, Bkn, D2, None, True, 0, False, epi=7, aux=aux2)
    torch.cuda.synchronize()
    assert bool(torch.isnan(D2).all())


class _Counting:
    """The native module with its gemm_nt_stream calls counted per epilogue."""

    def __init__(self, C):
        self._C, self.epis = C, []

    def __getattr__(self, name):
        return getattr(self._C, name)

    def gemm_nt_stream(self, *args, **kw):
        self.epis.append(kw.get("epi", -1))
        return self._C.gemm_nt_stream(*args, **kw)


def _ffn_run(switch, p_drop, monkeypatch, min_tiles=0):
    from cloudtik_amd import ops
    from cloudtik_amd.ops import transformer as tr
    from cloudtik_amd.train.optim import FlatParamSpace
    Bsz, S, H, F = 8, 128, 256, 1024
    shapes = dict(W1=(F, H), b1f=(F,), W2=(H, F), b2f=(H,), g2=(H,), b2=(H,))
    params = {}
    for i, (n, shp) in enumerate(shapes.items()):
        v = torch.ones(shp, device="cuda", dtype=bf) if n == "g2" else _rand(*shp, scale=0.05, seed=40 + i)
        params[n] = torch.nn.Parameter(v)
    space = FlatParamSpace(list(params.values()), names=list(params))
    x = _rand(Bsz, S, H, seed=50).requires_grad_(True)
    dy = _rand(Bsz, S, H, seed=51)
    counting = _Counting(_C())
    monkeypatch.setattr(tr, "_C", lambda: counting)
    monkeypatch.setattr(tr, "_STREAM_FFN", switch)
    # 16 output tiles here: fewer than CUs, so the default floor would keep the one-tile kernel
    monkeypatch.setattr(tr, "_STREAM_FFN_MIN_TILES", min_tiles)
    ops.manual_seed(7)
    y = tr.ffn_block(x, params["W1"], params["b1f"], params["W2"], params["b2f"], params["g2"], params["b2"],
                     p_drop, 1e-12, training=True)
    y.backward(dy)
    torch.cuda.synchronize()
    return y.detach(), x.grad, space.grad.clone(), counting.epis


@pytest.mark.parametrize("p_drop", [0.0, 0.1])
def test_ffn_block_streamed_equals_one_tile(p_drop, monkeypatch):
    y0, dx0, g0, epis0 = _ffn_run("0", p_drop, monkeypatch)
    y1, dx1, g1, epis1 = _ffn_run("1", p_drop, monkeypatch)
    assert 6 not in epis0 and 7 not in epis0
    assert epis1.count(6) == 1 and epis1.count(7) == 1          # both fused sites took the streamed kernel
    assert torch.isfinite(y0.float()).all() and g0.float().abs().max() > 0
    assert torch.equal(y0, y1)
    assert torch.equal(dx0, dx1)
    assert torch.equal(g0, g1)                                   # every parameter gradient (flat buffer)


def test_ffn_block_keeps_one_tile_kernel_below_the_tile_floor(monkeypatch):
    """Switch on, default floor (the CU count): 16 tiles give no workgroup a second tile, so the
    one-tile kernels run, and with a floor of 15 the streamed ones do."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert cus >= 16
    *_, epis = _ffn_run("1", 0.0, monkeypatch, min_tiles=None)
    assert 6 not in epis and 7 not in epis
    *_, epis = _ffn_run("1", 0.0, monkeypatch, min_tiles=15)
    assert epis.count(6) == 1 and epis.count(7) == 1
