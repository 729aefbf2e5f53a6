"""Preconditions of tests/loss_hard_cases.py, on the CPU: what makes the limits of test_gpu_loss_hard_negatives.py meaningful.

  (a) the by-item reference with the tie rule equals oracle.losses with torch.topk on a slice small enough to
      materialise: loss values on EVERY row (1e-10), gradients on every row that has no tie between different items at the
      threshold; both candidate kinds, masked and unmasked; with the restriction off it equals loss_cases.reference;
  (b) per (case, candidates, masked, k) of the GPU matrix at most 5 % of the query rows are flagged (a cosine of another
      item within COS_BAND of the row's cosine threshold);
  (c) the matrix is active: in the in-batch groups the threshold item is split by its multiplicity (rho < 1, one item) on
      at least a quarter of the rows; every width has an exact dot tie between DIFFERENT items at the threshold for some k;
      the large masked k has both restricted rows and rows with fewer than k counted negatives.
(b) and (c) are conditions on the inputs, not measurements: a (case, k) that misses one gets another k, not a wider cap."""

import pytest
import torch

import loss_cases as LC
import loss_hard_cases as HC
from oracle import losses as OL

ALL_WIDTHS = LC.WIDTHS + LC.GENERIC_WIDTHS
GROUPS = (("batch", True), ("batch", False), ("catalog", True), ("catalog", False))


@pytest.mark.parametrize("cand,masked", GROUPS)
def test_tie_rule_reference_equals_the_topk_oracle_on_a_small_slice(cand, masked):
    c = LC.inputs(64)
    table = c.table.double()
    q, pos = c.tok.double()[c.qsel][:48], c.pos[c.qsel][:48]
    cfg = dict(mask_false_negatives=masked, scale=2.0, margin=0.3)
    if cand == "batch":
        neg = c.neg[c.mask][:90]
        assert bool((neg[None, :] == pos[:, None]).any())
        full = torch.cat([table[pos][:, None, :], table[neg][None].expand(q.shape[0], -1, -1)], dim=1)
        ocfg = dict(ties=torch.cat([torch.zeros(q.shape[0], 1, dtype=torch.bool), neg[None, :] == pos[:, None]], dim=1), **cfg)
        target, mult, ks = None, torch.bincount(neg, minlength=LC.V + 1), (1, 3, 8, 40, 90, 91)
    else:
        full, target, mult, ks = table[None].expand(q.shape[0], -1, -1), pos, None, (1, 3, 40, 150, LC.V, LC.V + 1)
        ocfg = dict(target_position=None, **cfg)
    n_cols = full.shape[1]
    compared = dict(dot=0, cos=0)
    for k in ks:
        qo = q.clone().requires_grad_(True)
        rows, stats, sel = HC.heads(qo, pos, table, mult, n_cols, masked=masked, k=k, scale=2.0, margin=0.3)
        tied = dict(dot=HC.tie_between_items(sel.l, sel.w0_dot, sel.dot),
                    cos=HC.tie_between_items(sel.c, sel.w0_cos, sel.cos, 1e-12))
        for kind in OL.LOSS_KINDS:
            (g,) = torch.autograd.grad(rows[kind].sum(), qo, retain_graph=True)
            qw = q.clone().requires_grad_(True)
            want = OL.embed_loss(kind, qw, full, target, num_hard_negatives=k, **ocfg)
            (g_want,) = torch.autograd.grad(want, qw)
            for i in range(q.shape[0]):  # the loss values, row by row
                o1 = {kk: (v[i:i + 1] if kk == "ties" else v) for kk, v in ocfg.items()}
                w = OL.embed_loss(kind, q[i:i + 1], full[i:i + 1], None if target is None else target[i:i + 1],
                                  num_hard_negatives=k, **o1).item()
                assert rows[kind][i].item() == pytest.approx(w, rel=1e-10, abs=1e-10), (kind, k, i)
            which = "cos" if kind in OL.COSINE_KINDS else "dot"
            keep = ~tied[which] if kind != "AlignmentLoss" else torch.ones_like(tied[which])
            compared[which] += int(keep.sum())
            err = (g - g_want)[keep].norm(dim=1) / g_want[keep].norm(dim=1).clamp(min=1.0)
            assert float(err.max()) <= 1e-10, (kind, k, float(err.max()))
        for name, v in OL.logits_statistics(q, full, target, num_hard_negatives=k, **ocfg).items():  # (density: float32)
            assert stats[name] == pytest.approx(v, rel=1e-6 if name.endswith("density") else 1e-9, abs=1e-10), (name, k)
    assert min(compared.values()) >= 40 * len(ks)  # ties between different items are the exception


@pytest.mark.parametrize("cand,masked", GROUPS)
@pytest.mark.parametrize("H", ALL_WIDTHS)
def test_reference_with_the_restriction_off_is_the_plain_reference(H, cand, masked):
    base = LC.reference(H, cand, masked)
    for k in (0, HC.K_OFF if cand == "batch" else LC.V + 1):
        r = HC.reference(H, cand, masked, k)
        assert r is HC.reference(H, cand, masked, k)
        assert not bool(r.sel.dot[3].any()) and not bool(r.sel.cos[3].any()) and not bool(r.flagged.any())
        for kind in OL.LOSS_KINDS:
            assert r.sums[kind] == pytest.approx(base.sums[kind], rel=1e-10, abs=1e-10), kind
            assert float((r.d_tok[kind] - base.d_tok[kind]).norm()) <= 1e-10 * max(1.0, float(base.d_tok[kind].norm())), kind
        for name, v in base.stats.items():  # (the materialised oracle's density is a float32 tensor)
            assert r.stats[name] == pytest.approx(v, rel=1e-6 if name.endswith("density") else 1e-9, abs=1e-10), name


@pytest.mark.parametrize("cand,masked", GROUPS)
@pytest.mark.parametrize("H", ALL_WIDTHS)
def test_at_most_five_percent_of_the_rows_are_flagged_for_a_cosine_near_tie(H, cand, masked):
    for k in HC.ks_of(cand, H):
        r = HC.reference(H, cand, masked, k)
        n = r.flagged.numel()
        assert n == r.counts["n_query"]
        print(f"HARD_FLAGGED {H} {cand} masked={masked} k={k}: {int(r.flagged.sum())} of {n}")
        assert int(r.flagged.sum()) <= 0.05 * n, (H, cand, masked, k, int(r.flagged.sum()), n)
        # the dot selection needs no guard: a counted dot logit is either at the threshold exactly or a grid step away
        d = (r.sel.l - r.sel.dot[1][:, None]).abs()
        assert not bool(((r.sel.w0_dot > 0) & (d > 0) & (d < LC.Q_GRID * LC.E_GRID)).any())


@pytest.mark.parametrize("H", ALL_WIDTHS)
def test_matrix_reaches_split_multiplicities_ties_between_items_and_mixed_rows(H):
    ks = HC.ks_of("batch", H)
    ties = 0
    for cand, masked in GROUPS:
        for k in HC.ks_of(cand, H):
            s = HC.reference(H, cand, masked, k).sel
            ties += int(HC.tie_between_items(s.l, s.w0_dot, s.dot).sum())
            if cand == "batch" and bool(s.dot[3].any()):
                split = HC.split_by_multiplicity(s.l, s.w0_dot, s.dot)
                assert float(split.sum()) >= 0.25 * split.numel(), (H, masked, k, int(split.sum()))
    assert ties >= 1, H
    k_large = max(k for k in ks if k < HC.K_OFF)
    for sel in (HC.reference(H, "batch", True, k_large).sel.dot, HC.reference(H, "batch", True, k_large).sel.cos):
        assert 0 < int(sel[3].sum()) < sel[3].numel(), (H, k_large)
    # unmasked, every row has all ~300 columns: the large k restricts each of them
    assert bool(HC.reference(H, "batch", False, k_large).sel.dot[3].all())
    # the catalogue's k = V keeps every row whole (at most V counted negatives) and still is "restricted" for the density
    s = HC.reference(H, "catalog", False, LC.V).sel
    assert not bool(s.dot[3].any()) and float(s.dot[0].sum(dim=1).min()) == LC.V
