"""Preconditions of tests/loss_cases.py, on the CPU: what makes the tight limits of test_gpu_loss_dma_forms.py meaningful.

For every (width, seed, margin) the GPU matrices use (loss_cases.WIDTHS and the generic-only GENERIC_WIDTHS):
  (a) queries and table lie on their grids and are bf16 numbers;
  (b) fp32 logits in two summation orders equal the fp64 logits exactly;
  (c) the guard band dropped at most 5 % of the query rows (and three 128-query blocks are left);
  (d) the false-negative mask removes between 3 % and 50 % of the in-batch pairs;
  (e) the hinge term and the cosine margin are each active on >= 3 % of the counted pairs and inactive on >= 3 %;
  (f) the lean oracle forms the references are built from equal the materialised oracle.losses on a small case.
(c)-(e) are conditions on the inputs, not measurements: a seed that misses one is replaced in loss_cases.SEEDS."""

import pytest
import torch

import loss_cases as LC
from oracle import lean
from oracle import losses as OL


@pytest.mark.parametrize("H", LC.WIDTHS + LC.GENERIC_WIDTHS)
def test_inputs_lie_on_their_grids_and_are_bf16_numbers(H):
    c = LC.inputs(H)
    for t, grid, bound in ((c.tok, LC.Q_GRID, 2.0), (c.table, LC.E_GRID, 0.25)):
        k = t.double() / grid
        assert torch.equal(k, k.round()) and float(t.abs().max()) <= bound
        assert torch.equal(t.to(torch.bfloat16).float(), t)
    assert bool((c.table[0] == 0).all()) and float(c.table[1:].abs().sum(dim=1).min()) > 0
    # every partial sum of products, in any order, is an integer below 2^24 in units of Q_GRID * E_GRID
    worst = (c.tok.double().abs() @ c.table.double().abs().T).max() / (LC.Q_GRID * LC.E_GRID)
    assert float(worst) < 2 ** 24


@pytest.mark.parametrize("H", LC.WIDTHS + LC.GENERIC_WIDTHS)
def test_fp32_logits_equal_fp64_in_two_summation_orders(H):
    c = LC.inputs(H)
    want = c.tok.double() @ c.table.double().T
    blocked = c.tok @ c.table.T  # the BLAS order
    backwards = torch.zeros_like(blocked)  # one term at a time, last column first
    for h in reversed(range(H)):
        backwards += c.tok[:, h, None] * c.table[None, :, h]
    assert blocked.dtype == backwards.dtype == torch.float32
    assert torch.equal(blocked.double(), want) and torch.equal(backwards.double(), want)


@pytest.mark.parametrize("H", LC.WIDTHS + LC.GENERIC_WIDTHS)
def test_shape_reaches_the_blocks_tiles_and_edges_it_is_meant_to(H):
    c = LC.inputs(H)
    nq, negs = int(c.qsel.sum()), c.neg[c.mask]
    assert 256 < nq <= 384  # three 128-query blocks, the last partial
    distinct = int(torch.unique(negs).numel())
    assert 128 < distinct < 192 and distinct % 64 and (LC.V + 1) % 64  # three / four column tiles, the last partial
    assert int(torch.bincount(negs).max()) > 1  # multiplicities above 1
    assert 0 < int((~c.mask).sum()) and int((c.mask & (c.pos == 0)).sum()) >= 3  # ragged; valid rows without a positive
    assert bool(((negs[None, :] == c.pos[c.qsel][:, None]).any(dim=1)).any())  # an exact false negative by item id
    assert bool((c.pos[~c.mask] == 0).all()) and bool((c.neg[~c.mask] == 0).all())
    assert not bool((LC.near_discontinuity(c.table, c.tok, c.pos) & c.qsel).any())  # the band is empty after the drop


@pytest.mark.parametrize("margin", LC.MARGINS)
@pytest.mark.parametrize("H", LC.WIDTHS + LC.GENERIC_WIDTHS)
def test_guard_band_is_narrow_and_masks_and_margins_are_active(H, margin):
    a = LC.activity(H, margin)
    assert a["dropped"] <= 0.05, a
    assert 0.03 <= a["masked_out"] <= 0.50 and 0.03 <= a["masked_out_cos"] <= 0.50, a
    for k, v in a.items():
        if k.startswith(("hinge/", "cosine/")):
            assert 0.03 <= v <= 0.97, (k, v)


@pytest.mark.parametrize("masked", [True, False])
def test_lean_oracle_forms_equal_the_materialised_oracle_on_a_small_case(masked):
    """The in-batch references come from oracle.lean (item-weighted sums, reference-form rows); here against
    oracle.losses on the materialised (Np, 1 + N, H) candidates of a slice of the H = 64 case, non-default scale and
    margin, ties by item id."""
    c = LC.inputs(64)
    table = c.table.double()
    q, pos = c.tok.double()[c.qsel][:48], c.pos[c.qsel][:48]
    neg = c.neg[c.mask][:90]
    assert bool((neg[None, :] == pos[:, None]).any())
    cand = torch.cat([table[pos][:, None, :], table[neg][None].expand(q.shape[0], -1, -1)], dim=1)
    ties = torch.cat([torch.zeros(q.shape[0], 1, dtype=torch.bool), neg[None, :] == pos[:, None]], dim=1)
    cfg = dict(mask_false_negatives=masked, scale=2.0, margin=0.3)
    got = lean.heads_by_item(q, pos, neg, table, **cfg)
    for kind in OL.LOSS_KINDS:
        qo = q.clone().requires_grad_(True)
        want = OL.embed_loss(kind, qo, cand, ties=ties, **cfg)
        (g_want,) = torch.autograd.grad(want, qo)
        assert got[f"loss/{kind}"] == pytest.approx(want.item(), rel=1e-10, abs=1e-10), kind
        loss, g = lean.rows_reference_form(kind, q, pos, neg, table, **cfg)
        assert loss.item() == pytest.approx(want.item(), rel=1e-10, abs=1e-10), kind
        assert float((g - g_want).norm()) <= 1e-10 * max(1.0, float(g_want.norm())), kind
    for k, v in OL.logits_statistics(q, cand, ties=ties, **cfg).items():  # (its density is a float32 tensor: 2^-23)
        assert got[k] == pytest.approx(v, rel=1e-6 if k.endswith("density") else 1e-9, abs=1e-10), k


def test_references_are_shared_and_count_what_the_kernel_counts():
    r = LC.reference(64, "batch", True)
    assert r is LC.reference(64, "batch", True)
    c = LC.inputs(64)
    assert r.counts["n_query"] == int(c.qsel.sum()) and r.counts["n_valid"] == int(c.mask.sum())
    for kind in OL.LOSS_KINDS:
        assert r.d_tok[kind].shape == (LC.T, 64) and float(r.d_tok[kind][~c.qsel].abs().max()) == 0.0
        assert float(r.d_tok[kind][c.qsel].abs().max()) > 0.0
    rc = LC.reference(64, "catalog", False)
    assert rc.counts["n_valid"] == LC.V + 1 and rc.stats["logits/neg/count"] == r.counts["n_query"] * LC.V
