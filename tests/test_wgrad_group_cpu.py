"""Grouped weight-gradient routing (ops/linear.py) without a GPU: the slice chooser's values
and the fallback to the per-problem path when a problem does not qualify."""
import importlib

import torch

from cloudtik_amd.ops.linear import issue_wgrads, tn2_group_splits, tn2_splits, wgrad_accumulate_group

linear = importlib.import_module("cloudtik_amd.ops.linear")      # (ops.linear the attribute is the function)


def test_group_chooser_bert_large():
    T = 32768
    assert tn2_group_splits(T, [(1024, 1024), (3072, 1024)]) == 4      # Wo + Wqkv: 64 tiles
    assert tn2_group_splits(T, [(1024, 4096), (4096, 1024)]) == 2      # W2 + W1: 128 tiles
    # the single-problem chooser is what it was
    assert [tn2_splits(T, *s) for s in ((3072, 1024), (1024, 1024), (4096, 1024), (1024, 4096))] == [5, 16, 4, 4]


def test_group_chooser_is_the_single_formula_on_one_problem():
    for T, N, K in ((32768, 3072, 1024), (8192, 1024, 1024), (4096, 256, 512), (2048, 4096, 1024)):
        assert tn2_group_splits(T, [(N, K)]) == tn2_splits(T, N, K)


def test_group_chooser_refuses_shapes_outside_the_tiling():
    assert tn2_group_splits(32768, [(1024, 1024), (1000, 1024)]) == 1
    assert tn2_group_splits(32768 + 32, [(1024, 1024), (3072, 1024)]) == 1
    assert tn2_group_splits(32768, []) == 1
    assert tn2_group_splits(64, [(256, 256), (256, 256)]) == 1           # one K-tile: nothing to slice


# (T, (N, K)) -> (tn2_splits(T, N, K), tn2_group_splits(T, [(N, K)])) and (T, (shape, shape)) ->
# tn2_group_splits(T, shapes), recorded from the two separate cost-model bodies these wrappers
# had before they shared one.  The lone chooser counts whole tiles without checking the widths
# (its caller does), so the two differ at N or K = 1000.
_LONE = {
    (32768, (3072, 1024)): (5, 5),
    (32768, (1024, 1024)): (16, 16),
    (32768, (4096, 1024)): (4, 4),
    (32768, (1000, 1024)): (21, 1),
    (32768, (1024, 1000)): (21, 1),
    (32768, (768, 768)): (28, 28),
    (32768, (128, 1024)): (1, 1),
    (32800, (1024, 1024)): (1, 1),
    (8192, (1024, 1024)): (11, 11),
    (4096, (256, 512)): (8, 8),
    (2048, (4096, 1024)): (3, 3),
    (1024, (256, 256)): (2, 2),
    (1024, (768, 256)): (2, 2),
    (512, (256, 256)): (1, 1),
    (65536, (8192, 8192)): (1, 1),
    (64, (256, 256)): (1, 1),
}
_PAIRS = {
    (32768, ((1024, 1024), (3072, 1024))): 4,
    (32768, ((1024, 4096), (4096, 1024))): 2,
    (32768, ((1024, 1024), (1000, 1024))): 1,
    (32768, ((768, 768), (1024, 1024))): 10,
    (32800, ((1024, 1024), (3072, 1024))): 1,
    (1024, ((256, 256), (768, 256))): 2,
    (1024, ((256, 1024), (1024, 256))): 2,
    (768, ((256, 256), (768, 256))): 1,
    (2048, ((256, 256), (512, 256))): 4,
    (8192, ((1024, 1024), (3072, 1024))): 4,
    (65536, ((1024, 1024), (3072, 1024))): 4,
    (4096, ((128, 256), (256, 256))): 1,
}


def test_choosers_return_the_recorded_values():
    assert {k: (tn2_splits(k[0], *k[1]), tn2_group_splits(k[0], [k[1]])) for k in _LONE} == _LONE
    assert {k: tn2_group_splits(k[0], list(k[1])) for k in _PAIRS} == _PAIRS


class _Param:
    """A flat parameter as ``issue_wgrads`` sees one: ``.grad`` and the bucketer's callback."""

    def __init__(self, grad, log):
        self.grad = grad
        self._ct_grad_ready = log.append


def test_issue_wgrads_falls_through_per_item_and_reports_in_order(monkeypatch):
    """CPU tensors: no side stream and no grouped launch, so every item reaches
    ``wgrad_accumulate`` in order with its own gradient tensors, and each weight, then its bias,
    is reported ready once, in item order -- for one item and for a block's two."""
    calls, ready = [], []
    real = linear.wgrad_accumulate

    def spy(g, dy2, x2, dbias=None):
        calls.append((g, dbias))
        real(g, dy2, x2, dbias)

    monkeypatch.setattr(linear, "wgrad_accumulate", spy)
    gen = torch.Generator().manual_seed(1)
    T = 64
    dy_a, x_a = torch.randn(T, 256, generator=gen), torch.randn(T, 256, generator=gen)
    dy_b, x_b = torch.randn(T, 512, generator=gen), torch.randn(T, 256, generator=gen)
    wa, wb, bb = (_Param(t, ready) for t in (torch.ones(256, 256), torch.zeros(512, 256), torch.zeros(512)))
    issue_wgrads([(wa, dy_a, x_a, None), (wb, dy_b, x_b, bb)])
    assert len(calls) == 2 and calls[0][0] is wa.grad and calls[1][0] is wb.grad
    assert calls[0][1] is None and calls[1][1] is bb.grad
    assert ready == [wa, wb, bb]
    torch.testing.assert_close(wa.grad, 1 + dy_a.t() @ x_a)
    torch.testing.assert_close(wb.grad, dy_b.t() @ x_b)
    torch.testing.assert_close(bb.grad, dy_b.sum(0))
    del calls[:], ready[:]
    issue_wgrads([(wb, dy_b, x_b, bb)])
    assert len(calls) == 1 and calls[0][0] is wb.grad and calls[0][1] is bb.grad
    assert ready == [wb, bb]
    torch.testing.assert_close(wb.grad, 2 * (dy_b.t() @ x_b))


def test_group_falls_back_to_separate_calls(monkeypatch):
    """CPU tensors do not qualify: every problem goes through ``wgrad_accumulate`` in order,
    with its own arguments, and the sums are those of the plain products."""
    calls = []
    real = linear.wgrad_accumulate

    def spy(g, dy2, x2, dbias=None):
        calls.append((g, dy2, x2, dbias))
        real(g, dy2, x2, dbias)

    monkeypatch.setattr(linear, "wgrad_accumulate", spy)
    gen = torch.Generator().manual_seed(0)
    T = 64
    dy_a, x_a = torch.randn(T, 256, generator=gen), torch.randn(T, 256, generator=gen)
    dy_b, x_b = torch.randn(T, 512, generator=gen), torch.randn(T, 256, generator=gen)
    g_a, g_b, db = torch.ones(256, 256), torch.zeros(512, 256), torch.zeros(512)
    wgrad_accumulate_group([(g_a, dy_a, x_a, None), (g_b, dy_b, x_b, db)])
    assert [c[0] is g for c, g in zip(calls, (g_a, g_b))] == [True, True]
    assert calls[0][3] is None and calls[1][3] is db
    torch.testing.assert_close(g_a, 1 + dy_a.t() @ x_a)
    torch.testing.assert_close(g_b, dy_b.t() @ x_b)
    torch.testing.assert_close(db, dy_b.sum(0))


def test_group_qualification_rules():
    """A token count or a width outside the tiling, a single problem or more than four, and
    mismatched token counts all take the per-problem path."""
    bf = torch.bfloat16
    ok = (torch.zeros(256, 256, dtype=bf), torch.zeros(128, 256, dtype=bf), torch.zeros(128, 256, dtype=bf), None)
    assert not linear._group_qualifies([ok, ok])                          # not on a GPU
    assert not linear._group_qualifies([ok])
    assert not linear._group_qualifies([ok] * 5)
    other_t = (ok[0], torch.zeros(192, 256, dtype=bf), torch.zeros(192, 256, dtype=bf), None)
    assert not linear._group_qualifies([ok, other_t])
