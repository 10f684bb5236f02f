"""The sampling kernel (csrc/sampling.hip) against the rule (ops/sampling.py) evaluated in fp64 on
the CPU, its Philox stream, its reproducibility and refusals, and graph-replayed
``generate(do_sample=True)`` against the eager static step.

A dense row's kept count cannot be compared exactly (fp32 and fp64 sums differ), so the filter and
the draw are accepted when they are the rule's for some ``top_p'`` / ``u'`` within ``eps`` of the
given ones.  ``eps`` is 4 x the largest deviation an fp32 CPU rounding model of the rule (sums in
descending-sorted order, in token order, and the kernel's fixed-point weights summed as integers)
shows against fp64 on the same rows; it is never taken from the kernel's output and never above
V * 2**-24.  Values of ``eps`` reached on these inputs (every test prints its own), largest over
rows, dtypes and parameter sets: 5.7e-7 at V = 32128, 5.8e-7 at V = 1003, 5.1e-7 at V = 17 (the
cap there is 1.0e-6), 5.6e-7 at V = 40000 and 0 at V = 1.  The kernel met every case at these.

``top_k = 1`` and ``top_p = 1e-6`` keep the maximum's tie group whole, as the rule says, so the
draw among n tied maxima is the floor(u * n)-th of them: the arg-max with the lowest id when the
maximum is single, which is what the exact assertions check (and ``u = 0`` gives the lowest id)."""
import functools

import pytest
import torch

from cloudtik_amd.models.t5 import T5Config, T5ForConditionalGeneration
from cloudtik_amd.ops import sampling as S

pytestmark = pytest.mark.gpu

EOS, PAD, START, T, POS = 1, 0, 0, 8, 3
NEG_INF = float("-inf")
BIG_V = 40000                       # beyond the 32768 floats the kernel stages in LDS
PARAMS = {                          # (repetition_penalty, temperature, top_k, top_p)
    "off": (1.0, 1.0, 0, 1.0), "t0.7_k50": (1.0, 0.7, 50, 1.0), "p0.9": (1.0, 1.0, 0, 0.9),
    "rp1.2_t0.7_k50_p0.95": (1.2, 0.7, 50, 0.95), "rp1.3_t1.5_p0.5": (1.3, 1.5, 0, 0.5), "k1": (1.0, 1.0, 1, 1.0),
    "k_ge_V": (1.0, 1.0, 1 << 20, 1.0), "p1e-6": (1.0, 1.0, 0, 1e-6)}
SHAPES = [(V, R, dt) for V in (32128, 1003, 17, 1) for R in (1, 3, 130) for dt in ("bf16", "fp32")] + \
         [(BIG_V, R, "fp32") for R in (1, 3, 130)]
EPS_SEEN = {}


@functools.lru_cache(maxsize=None)
def make_rows(V, R, dt):
    """(logits [R, V], out [R, T], done [R], u [R]) on the CPU, built once per shape and left as
    they are.  Slots < POS of ``out`` hold the tokens seen so far, one of them twice."""
    g = torch.Generator().manual_seed(V * 1000 + R)
    logits = torch.randn(R, V, generator=g) * 2.5
    out = torch.full((R, T), PAD, dtype=torch.long)
    out[:, :POS] = torch.randint(0, V, (R, POS), generator=g)
    out[:, 1] = out[:, 0]                                          # a duplicate in the seen set
    rows = torch.arange(R)
    if V >= 17:
        logits[rows, out[:, 0]] = 3.0 + torch.rand(R, generator=g)           # penalised, positive
        logits[rows, out[:, 2]] = -1.0 - torch.rand(R, generator=g)          # penalised, negative
        logits[:, START] = 2.0                                     # the start token is penalised too
        logits[:, 5] = NEG_INF
        logits[:, 11] = float("nan")
        logits[0, EOS] = 30.0                                      # row 0 draws EOS
    done = (rows % 5) == 4
    if R >= 3:
        logits[R - 1] = NEG_INF                                    # no finite logit
        if V >= 17:
            logits[R - 1, 11] = float("nan")
        done[R - 1] = False
        done[1] = True
    u = torch.rand(R, generator=g)
    u[0] = 0.5
    logits = logits.to(torch.bfloat16) if dt == "bf16" else logits
    return logits, out, done, u


def rounding_model_eps(x, keepk, V):
    """4 x the largest deviation of normalised partial sums of the weights, fp32 and fixed-point
    against fp64, in descending-sorted order (the filter's sums) and token order (the draw's)."""
    m = x.max(1, keepdim=True)[0]
    ok = torch.isfinite(m[:, 0])
    x, keepk, m = x[ok], keepk[ok], m[ok]
    if x.shape[0] == 0:
        return 0.0
    w32 = torch.where(keepk, torch.exp(x - m), torch.zeros(()))
    w64 = torch.where(keepk, torch.exp((x - m).double()), torch.zeros((), dtype=torch.float64))
    q = torch.floor(w32.double() * 2.0 ** S.weight_bits(V)).to(torch.int64)
    order = torch.sort(x, dim=1, descending=True, stable=True)[1]
    dev = 0.0
    for idx in (order, None):
        a32, a64, aq = (w if idx is None else w.gather(1, idx) for w in (w32, w64, q))
        c64 = a64.cumsum(1)
        c64 = c64 / c64[:, -1:]
        c32 = a32.cumsum(1)
        cq = aq.cumsum(1)
        dev = max(dev, float(((c32 / c32[:, -1:]).double() - c64).abs().max()),
                  float((cq.double() / cq[:, -1:].double() - c64).abs().max()))
    return 4 * dev


def run_kernel(cuda, logits, out, done, u, rp, temp, k, p, pos=POS, seed=0):
    dev = dict(out=out.clone().to(cuda), done=done.clone().to(cuda), cur=torch.full((out.shape[0], 1), -1, device=cuda),
               pos=torch.tensor([pos], device=cuda), seed=torch.tensor([seed], device=cuda))
    diag = S.sample_step(logits.to(cuda), dev["out"], dev["done"], dev["cur"], dev["pos"], dev["seed"], START, EOS, PAD,
                         temp, k, p, rp, u=None if u is None else u.to(cuda))
    return {k_: v.cpu() for k_, v in dev.items()}, [d.cpu() for d in diag]


@pytest.mark.parametrize("name", list(PARAMS))
@pytest.mark.parametrize("V,R,dt", SHAPES)
def test_kernel_follows_the_rule(cuda, V, R, dt, name):
    rp, temp, k, p = PARAMS[name]
    logits, out, done, u = make_rows(V, R, dt)
    st, (g_u, g_thr, g_keep) = run_kernel(cuda, logits, out, done, u, rp, temp, k, p)
    tok = st["out"][:, POS]

    # the reference's processed logits and top-k set (exact), weights in fp64
    seen = S.seen_mask(out, torch.tensor(POS), START, V)
    x, _ = S.process_logits_reference(logits, seen, temp, 0, 1.0, rp)
    k_on, p_on = 0 < k < V, p < 1.0
    kth = torch.topk(x, k, dim=1)[0][:, -1:] if k_on else x.min(1, keepdim=True)[0]
    keepk = x >= kth
    m = x.max(1, keepdim=True)[0]
    finite = torch.isfinite(m[:, 0])
    w = torch.where(keepk, torch.exp((x - m).double()), torch.zeros((), dtype=torch.float64))
    w = torch.where(finite[:, None], w, torch.zeros_like(w))
    Z = w.sum(1)
    eps = rounding_model_eps(x, keepk, V)
    EPS_SEEN[V, R, dt, name] = eps
    print(f"eps V={V} R={R} {dt} {name}: {eps:.3e}")
    assert eps <= V * 2.0 ** -24

    assert torch.equal(g_u, u)
    # (a) thr is one of the row's processed logits and n_keep counts the logits >= thr
    thr = g_thr[:, None]
    assert bool(((x == thr).any(1)).all())
    assert torch.equal(g_keep.long(), (x >= thr).sum(1))
    assert bool((g_thr <= m[:, 0]).all() and (thr >= kth).all())
    kept = x >= thr
    f = finite
    if not p_on:
        assert torch.equal(g_thr[f], kth[f, 0])                     # top-k alone (or nothing): exact
    else:
        # (b) the kept set is the rule's for some p' within eps of top_p
        A_thr = (w * (x > thr)).sum(1) / Z
        below = keepk & (x < thr)
        nxt = torch.where(below, x, torch.full_like(x, NEG_INF)).max(1, keepdim=True)[0]
        A_nxt = (w * (x > nxt)).sum(1) / Z
        assert bool((A_thr[f] < p + eps).all()), (A_thr[f].max(), p, eps)
        has = below.any(1) & f
        assert bool((A_nxt[has] >= p - eps).all()), (A_nxt[has].min(), p, eps)
    # (c) the token is kept and is the rule's draw over the kernel's kept set for some u' within eps of u
    live = f & ~done
    wk = w * kept
    C = wk.cumsum(1)
    Zk = C[:, -1]
    hi = C.gather(1, tok[:, None].clamp(0, V - 1))[:, 0] / Zk
    lo = hi - wk.gather(1, tok[:, None].clamp(0, V - 1))[:, 0] / Zk
    assert bool((tok[live] >= 0).all() and (tok[live] < V).all())
    assert bool(kept.gather(1, tok[:, None].clamp(0, V - 1))[:, 0][live].all())
    ud = u.double()
    assert bool((lo[live] <= ud[live] + eps).all() and (hi[live] > ud[live] - eps).all())
    # exact cases
    assert bool((tok[done] == PAD).all())
    assert bool((tok[~f & ~done] == 0).all())
    if V >= 17 and not done[0]:
        assert int(tok[0]) == EOS
    if name in ("k1", "p1e-6"):
        # the maximum's tie group alone: with n tied tokens the draw is the floor(u * n)-th of them,
        # the arg-max with the lowest id when the maximum is single
        top = x == m
        n_top = top.sum(1)
        assert torch.equal(g_keep.long()[f], n_top[f]) and torch.equal(g_thr[f], m[f, 0])
        j = torch.floor(ud * n_top.double()).long().clamp(max=V - 1)
        want = (top.long().cumsum(1) == (j + 1)[:, None]).long().argmax(1)
        assert torch.equal(tok[live], want[live])
        single = live & (n_top == 1)
        assert torch.equal(tok[single], x.argmax(1)[single])
    # bookkeeping
    want_out = out.clone()
    want_out[:, POS] = tok
    assert torch.equal(st["out"], want_out) and torch.equal(st["cur"][:, 0], tok)
    assert torch.equal(st["done"], done | (tok == EOS)) and int(st["pos"]) == POS + 1


def test_hand_built_row_exact(cuda):
    w8 = [1.0, 2.0, 3.0, 4.0, 0.0, 2.0, 1.0, 3.0]
    edges = [0.0, 1 / 16, 3 / 16, 6 / 16, 10 / 16, 10 / 16, 12 / 16, 13 / 16, 1.0]
    us = [0.0, 1 - 2.0 ** -24] + [(edges[v] + edges[v + 1]) / 2 for v in range(8) if w8[v] > 0]
    want = [0, 7] + [v for v in range(8) if w8[v] > 0]
    for dt in (torch.float32, torch.bfloat16):
        logits = torch.tensor([w8]).log().to(dt).expand(len(us), 8).contiguous()
        out = torch.full((len(us), T), PAD, dtype=torch.long)
        done = torch.zeros(len(us), dtype=torch.bool)
        st, (g_u, g_thr, g_keep) = run_kernel(cuda, logits, out, done, torch.tensor(us, dtype=torch.float32),
                                              1.0, 1.0, 0, 1.0, pos=0)
        assert st["out"][:, 0].tolist() == want
        assert g_keep.tolist() == [8] * len(us) and bool((g_thr == NEG_INF).all())
        # past the last step nothing changes
        st2, _ = run_kernel(cuda, logits, out, done, torch.tensor(us, dtype=torch.float32), 1.0, 1.0, 0, 1.0, pos=T)
        assert torch.equal(st2["out"], out) and int(st2["pos"]) == T and bool((st2["cur"] == -1).all())


def test_philox_stream(cuda):
    logits, out, done, _ = make_rows(1003, 130, "fp32")
    for seed in (0, 1, 2 ** 32 + 5, 2 ** 63 - 1):
        for step in (0, T - 1):
            st, (g_u, _, _) = run_kernel(cuda, logits, out, done, None, 1.0, 1.0, 0, 1.0, pos=step, seed=seed)
            assert g_u.tolist() == [S.philox_uniform_reference(seed, r, step) for r in range(130)]
            ref = S.sample_step_reference(logits, out, done, None, torch.tensor([step]), torch.tensor([seed]), START,
                                          EOS, PAD)
            assert torch.equal(ref[4], g_u)


@pytest.mark.parametrize("V,dt", [(32128, "bf16"), (BIG_V, "fp32")])
def test_same_call_twice_is_bit_equal(cuda, V, dt):
    logits, out, done, u = make_rows(V, 130, dt)
    for name in ("rp1.2_t0.7_k50_p0.95", "p0.9"):
        rp, temp, k, p = PARAMS[name]
        a, da = run_kernel(cuda, logits, out, done, None, rp, temp, k, p, seed=12345)
        b, db = run_kernel(cuda, logits, out, done, None, rp, temp, k, p, seed=12345)
        assert all(torch.equal(a[n], b[n]) for n in a)
        assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(da, db))


def test_binding_refusals(cuda):
    R, V = 4, 32
    a = dict(logits=torch.zeros(R, V, device=cuda), out=torch.zeros(R, T, dtype=torch.long, device=cuda),
             done=torch.zeros(R, dtype=torch.bool, device=cuda), cur=torch.zeros(R, 1, dtype=torch.long, device=cuda),
             pos=torch.zeros(1, dtype=torch.long, device=cuda), seed=torch.zeros(1, dtype=torch.long, device=cuda))

    def call(u=None, **kw):
        b = {**a, **kw}
        return S.sample_step(b["logits"], b["out"], b["done"], b["cur"], b["pos"], b["seed"], START, EOS, PAD, u=u)

    call()
    for match, kw in (("bf16 or fp32", dict(logits=a["logits"].half())), ("contiguous", dict(logits=a["logits"].t().contiguous().t())),
                      ("2-D", dict(logits=a["logits"][0])), ("out", dict(out=a["out"].int())),
                      ("out", dict(out=a["out"][:3])), ("done", dict(done=a["done"].long())),
                      ("cur", dict(cur=a["cur"][:, 0])), ("pos", dict(pos=a["pos"].int())),
                      ("seed", dict(seed=a["seed"].int())), ("seed", dict(seed=torch.zeros(2, dtype=torch.long, device=cuda))),
                      ("pos must be a contiguous GPU", dict(pos=a["pos"].cpu())), ("GPU", dict(logits=a["logits"].cpu())),
                      ("out must be a contiguous GPU", dict(out=a["out"].cpu()))):
        with pytest.raises(RuntimeError, match=match):
            call(**kw)
    with pytest.raises(RuntimeError, match="u must"):
        call(u=torch.zeros(R + 1, device=cuda))
    with pytest.raises(RuntimeError, match="u must"):
        call(u=torch.zeros(R, dtype=torch.float64, device=cuda))
    with pytest.raises(RuntimeError, match="start_token"):
        S.sample_step(a["logits"], a["out"], a["done"], a["cur"], a["pos"], a["seed"], V, EOS, PAD)
    with pytest.raises(ValueError, match="top_p"):
        S.sample_step(a["logits"], a["out"], a["done"], a["cur"], a["pos"], a["seed"], START, EOS, PAD, top_p=0.0)


# --------------------------------------------------------------------------------- end to end
STEPS = 6


def _model(cuda):
    torch.manual_seed(0)
    cfg = T5Config(d_model=512, d_ff=2048, num_layers=2, num_decoder_layers=2, num_heads=8, dropout_rate=0.0)
    m = T5ForConditionalGeneration(cfg, device=cuda).eval()
    with torch.no_grad():
        m.shared.weight.mul_(0.05)      # tied N(0, 1) embeddings put nearly all mass on one token: flatten it
    return m


@pytest.fixture(scope="module")
def model(cuda):
    return _model(cuda)


def _batch(cuda):
    g = torch.Generator().manual_seed(4)
    x = torch.randint(2, 32128, (2, 24), generator=g).to(cuda)
    mask = torch.ones(2, 24, dtype=torch.long, device=cuda)
    mask[1, 17:] = 0
    return x, mask


RULE = dict(temperature=0.8, top_k=40, top_p=0.9, repetition_penalty=1.2)


@pytest.mark.parametrize("N", [1, 3])
def test_graph_generate_matches_eager_static_step(cuda, model, N):
    x, mask = _batch(cuda)
    got = model.generate(x, mask, max_new_tokens=STEPS, do_sample=True, num_return_sequences=N, seed=7, **RULE)
    assert got.shape == (2 * N, STEPS) and got.dtype == torch.long
    eager = model._generate_sample_static(x, mask, STEPS, N, 7, **RULE, graph=False)
    assert torch.equal(got, eager)
    assert torch.equal(model.generate(x, mask, max_new_tokens=STEPS, do_sample=True, num_return_sequences=N, seed=7,
                                      **RULE), got)
    keys = [k for k in model._graphs if k[0] == "sample" and k[1] == 2 * N and k[-1]]
    assert len(keys) == 1                          # the second call replayed the first call's capture
    # another seed on the cached graph is what a fresh model gives for it: the seed is not baked in
    other = model.generate(x, mask, max_new_tokens=STEPS, do_sample=True, num_return_sequences=N, seed=8, **RULE)
    fresh = _model(cuda)
    assert torch.equal(other, fresh.generate(x, mask, max_new_tokens=STEPS, do_sample=True, num_return_sequences=N,
                                             seed=8, **RULE))
    assert not torch.equal(other, got)
    # another top_p is another capture
    rule2 = {**RULE, "top_p": 0.5}
    assert torch.equal(model.generate(x, mask, max_new_tokens=STEPS, do_sample=True, num_return_sequences=N, seed=7, **rule2),
                       fresh.generate(x, mask, max_new_tokens=STEPS, do_sample=True, num_return_sequences=N, seed=7, **rule2))


def test_eager_loop_on_the_gpu(cuda, model):
    """``use_graph=False``: the growing-cache decoder and the same kernel."""
    x, mask = _batch(cuda)
    a = model.generate(x, mask, max_new_tokens=STEPS, do_sample=True, num_return_sequences=3, seed=7, use_graph=False, **RULE)
    assert a.shape == (6, STEPS) and a.dtype == torch.long
    assert torch.equal(model.generate(x, mask, max_new_tokens=STEPS, do_sample=True, num_return_sequences=3, seed=7,
                                      use_graph=False, **RULE), a)
    assert torch.equal(model.generate(x, mask, max_new_tokens=STEPS, do_sample=True, top_k=1, seed=2, use_graph=False),
                       model.generate(x, mask, max_new_tokens=STEPS, use_graph=False))


def test_top_k_one_is_greedy_and_other_paths_unchanged(cuda, model):
    x, mask = _batch(cuda)
    greedy = model.generate(x, mask, max_new_tokens=STEPS)
    beam, score = model.generate(x, mask, max_new_tokens=STEPS, num_beams=2, return_scores=True)
    for seed in (0, 3):
        assert torch.equal(model.generate(x, mask, max_new_tokens=STEPS, do_sample=True, top_k=1, seed=seed), greedy)
    model.generate(x, mask, max_new_tokens=STEPS, do_sample=True, seed=5, **RULE)
    assert torch.equal(model.generate(x, mask, max_new_tokens=STEPS), greedy)
    b2, s2 = model.generate(x, mask, max_new_tokens=STEPS, num_beams=2, return_scores=True)
    assert torch.equal(b2, beam) and torch.equal(s2, score)
    both = model.generate(x, mask, max_new_tokens=STEPS, num_beams=2, num_return_sequences=2)
    assert both.shape == (4, STEPS) and torch.equal(both.view(2, 2, STEPS)[:, 0], beam)
