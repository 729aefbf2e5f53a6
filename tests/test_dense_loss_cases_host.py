"""Preconditions of tests/dense_loss_cases.py, on the CPU: what makes the limits of test_gpu_dense_loss_forms.py meaningful.

  (a) the by-column reference with the tie rule equals oracle.losses (embed_loss / logits_statistics in fp64 with
      torch.topk): loss values on EVERY row (1e-10), both gradients on every row without a tie at the threshold that the
      two resolve differently; with the restriction off (k = 0, k = C) it is the plain reference;
  (b) the cases are active (conditions on the inputs, asserted from the reference alone -- a case that misses one gets
      other inputs, not a wider cap): the plants are there in their stated shares; per matrix case the mask removes at least
      4 % of the (row, other column) pairs and keeps at least half, the hinge is active on at least 5 % and the cosine margin
      on at least 3 % of the counted pairs under every option set; some k gives rho < 1 between DIFFERENT candidates, some
      k rho < 1 between copies, some k restricted rows next to rows with fewer than k counted negatives; at most 5 % of a
      case's rows are flagged for a cosine near-tie;
  (c) the fp32 model of the kernel's algorithm (dense_loss_cases.model) stays within two thirds of every limit of the GPU
      test on every launch of every case -- fp32 arithmetic alone can meet the limits --, and every fault of
      dense_loss_cases.FAULTS, a plausible wrong kernel, misses a limit on a matrix or an edge case (one, found while this
      test was written and not on the list it was written from, on the single-row case)."""

import pytest
import torch

import dense_loss_cases as DC
import loss_cases as LC
import loss_hard_cases as HC
from oracle import losses as OL

ORACLE_STATS = {"neg_density": "logits/neg/density", "pos_mean": "logits/pos/mean", "pos_std": "logits/pos/std",
                "pos_min": "logits/pos/min", "pos_max": "logits/pos/max", "neg_mean": "logits/neg/mean",
                "neg_std": "logits/neg/std", "neg_min": "logits/neg/min", "neg_max": "logits/neg/max"}


# ------------------------------------------------------------------------------------------------ (a)
@pytest.mark.filterwarnings("ignore:std")  # (the oracle's std of a single logit: NaN, as the reference has it)
@pytest.mark.parametrize("name", ["w68", "w68-diagonal", "c17", "c2", "c1", "n1"])
def test_by_column_reference_equals_the_topk_oracle(name):
    inp = DC.inputs(name)
    N, C = inp.case.N, inp.case.C
    q, cand, tgt = inp.q.double(), inp.cand.double(), inp.target
    # No `ties` for the oracle: in fp64 these dot products are exact in any order, and its cosine reduces every column by
    # itself, so a copy of the target's vector gets the target's bits -- if it did not, the masked values below would show it.
    compared = 0
    for opt in DC.opts_of(name):
        ref = DC.reference(name, opt)
        cfg = dict(target_position=None, mask_false_negatives=opt.masked, num_hard_negatives=opt.k, scale=opt.scale,
                   margin=opt.margin)
        tied = dict(dot=HC.tie_between_items(ref.sel.l, ref.sel.w0_dot, ref.sel.dot),
                    cos=HC.tie_between_items(ref.sel.c, ref.sel.w0_cos, ref.sel.cos, 1e-12))
        for kind in OL.LOSS_KINDS:
            qw, cw = q.clone().requires_grad_(True), cand.clone().requires_grad_(True)
            gq, gc = torch.autograd.grad(OL.embed_loss(kind, qw, cw, tgt, **cfg), (qw, cw))
            for i in range(N):  # the loss values, row by row
                w = OL.embed_loss(kind, q[i:i + 1], cand[i:i + 1], tgt[i:i + 1], **cfg).item()
                assert ref.rows[kind][i].item() == pytest.approx(w, rel=1e-10, abs=1e-10), (kind, opt, i)
            keep = ~tied["cos" if kind in OL.COSINE_KINDS else "dot"] if kind != "AlignmentLoss" else torch.ones(N, dtype=bool)
            compared += int(keep.sum())
            for got, want in ((ref.d_query[kind], gq), (ref.d_cand[kind].reshape(N, -1), gc.reshape(N, -1))):
                err = (got - want)[keep].norm(dim=1) / want[keep].norm(dim=1).clamp(min=1.0)
                assert err.numel() == 0 or float(err.max()) <= 1e-10, (kind, opt, float(err.max()))
        want = OL.logits_statistics(q, cand, tgt, **cfg)
        for mine, theirs in ORACLE_STATS.items():  # (the oracle's density is a float32 tensor; no value: nan or absent)
            w = want.get(theirs, float("nan"))
            if mine in ref.stats:
                assert ref.stats[mine] == pytest.approx(w, rel=1e-6 if mine == "neg_density" else 1e-9, abs=1e-10), (mine, opt)
            else:
                assert w != w, (mine, opt, w)
    assert compared >= 0.6 * 7 * N * len(DC.opts_of(name))  # ties that the two resolve differently are the exception


@pytest.mark.parametrize("name", ["w68", "c17", "n33-diagonal"])
def test_reference_with_the_restriction_off_is_the_plain_reference(name):
    C = DC.CASES[name].C
    for masked in (True, False):
        plain, off = DC.reference(name, DC.Opt(masked, 0, 20.0, 0.3)), DC.reference(name, DC.Opt(masked, C, 20.0, 0.3))
        for r in (plain, off):
            assert not bool(r.sel.dot[3].any()) and not bool(r.sel.cos[3].any()) and not bool(r.flagged.any())
            assert not r.fractional
        for kind in OL.LOSS_KINDS:
            assert torch.equal(plain.rows[kind], off.rows[kind]), kind
            assert torch.equal(plain.d_query[kind], off.d_query[kind]) and torch.equal(plain.d_cand[kind], off.d_cand[kind])
        assert plain.stats == off.stats


# ------------------------------------------------------------------------------------------------ (b)
@pytest.mark.parametrize("name", list(DC.CASES))
def test_cases_hold_their_plants_targets_and_shapes(name):
    inp = DC.inputs(name)
    c = inp.case
    N, C, H = c.N, c.C, c.H
    assert inp.q.shape == (N, H) and inp.cand.shape == (N, C, H) and inp.cand.is_contiguous()
    assert float(inp.q.abs().max()) <= 2.0 and bool((inp.q / LC.Q_GRID == (inp.q / LC.Q_GRID).round()).all())
    grid = inp.cand / LC.E_GRID
    off_grid = grid != grid.round()
    assert float(inp.cand.abs().max()) <= 0.25 and int(off_grid.sum()) == (2 if c.group == "clamped" else 0)
    assert bool(((inp.target >= 0) & (inp.target < C)).all())
    if c.mode == "first":
        assert bool((inp.target == 0).all())
    elif c.mode == "diagonal":
        assert torch.equal(inp.target, torch.arange(N))
    else:
        assert int(inp.target[0]) == C - 1 and (N == 1 or int(inp.target[1]) == 0)
    rows = torch.arange(N)
    for what, (every, from_c) in DC.PLANT_SHARE.items():
        want = (rows % every == 0) & (C >= from_c)
        assert torch.equal(getattr(inp, what), want), what
    tcol = torch.arange(C)[None, :] == inp.target[:, None]
    n_copy = ((inp.items == inp.pos_item[:, None]) & ~tcol & (inp.items >= 0)).sum(dim=1)
    assert bool((n_copy[inp.dup_target] >= 1).all())  # a copy of the target's item at another column
    for r in range(N):
        vecs = {tuple(v.tolist()) for v in inp.cand[r]}
        plain_row = not (inp.dup_target[r] or inp.dup_other[r] or r in inp.zero_q)
        assert len(vecs) == C or not plain_row, (name, r)  # columns are distinct items, except where planted
        if inp.dup_other[r]:
            counts = torch.bincount(inp.items[r][inp.items[r] > 0])
            assert int(counts.max()) >= 3
        if inp.zero_cand[r]:
            assert bool((inp.cand[r].abs().sum(dim=1) == 0).any())
    if N >= 3:  # the all-zero query row; its positive is the zero vector
        z = N - 1
        assert z in inp.zero_q and float(inp.q[z].abs().max()) == 0.0 and float(inp.cand[z, inp.target[z]].abs().max()) == 0.0
    if c.group == "matrix":
        assert 20 <= int(inp.dup_target.sum()) and 14 <= int(inp.dup_other.sum()) and 10 <= int(inp.zero_cand.sum())
    if c.group == "clamped":  # the clamped branches WITH a gradient: a tiny target, a zero query with an ordinary target
        t0 = inp.cand[0, inp.target[0]]
        assert 0 < float(t0.norm()) < 1e-8 and float(inp.q[1].abs().max()) == 0.0
        assert float(inp.cand[1, inp.target[1]].norm()) > 0.1
        assert int(((inp.cand[2].norm(dim=1) > 0) & (inp.cand[2].norm(dim=1) < 1e-8)).sum()) == 1
        ref = DC.reference(name, DC.opts_of(name)[0])
        assert float(ref.d_cand["AlignmentLoss"][0, inp.target[0]].norm()) > 1e7  # 1 / 1e-8 at work
        assert float(ref.d_query["AlignmentLoss"][1].norm()) > 1e7


@pytest.mark.parametrize("name", DC.MATRIX)
def test_matrix_cases_are_active(name):
    inp = DC.inputs(name)
    N, C = inp.case.N, inp.case.C
    other = torch.arange(C)[None, :] != inp.target[:, None]
    live = torch.ones(N, dtype=torch.bool)
    live[list(inp.zero_q)] = False
    for opt in DC.opts_of(name):
        s = DC.reference(name, opt).sel
        for which, lg, pos, w0 in (("dot", s.l, s.p, s.w0_dot), ("cos", s.c, s.cp, s.w0_cos)):
            removed = float(((w0 == 0) & other)[live].sum() / other[live].sum())
            assert (0.04 <= removed <= 0.5) if opt.masked else removed == 0.0, (name, opt, which, removed)
        hinge = float(((s.w0_dot > 0) & (s.l - (1 - opt.margin) * s.p > 0)).sum() / (s.w0_dot > 0).sum())
        cosine = float(((s.w0_cos > 0) & (s.c - 1 + opt.margin > 0)).sum() / (s.w0_cos > 0).sum())
        print(f"DENSE_ACTIVITY {name} masked={opt.masked} k={opt.k} margin={opt.margin}: hinge {hinge:.3f} cosine {cosine:.3f}")
        assert hinge >= 0.05 and cosine >= 0.03, (name, opt, hinge, cosine)


def _vectors_at_threshold(inp, sel_l, w0, sel):
    """Per row: (#columns, #distinct vectors) at the threshold of a restricted row with rho < 1, else (0, 0)."""
    _w, tau, rho, restricted = sel
    at = (w0 > 0) & (sel_l == tau[:, None])
    out = []
    for r in range(inp.case.N):
        if bool(restricted[r]) and float(rho[r]) < 1:
            out.append((int(at[r].sum()), len({tuple(v.tolist()) for v in inp.cand[r][at[r]]})))
        else:
            out.append((0, 0))
    return out


@pytest.mark.parametrize("name", DC.MATRIX)
def test_matrix_cases_reach_both_kinds_of_tie_and_mixed_rows(name):
    inp = DC.inputs(name)
    C = inp.case.C
    diff = copies = mixed = 0
    for opt in DC.opts_of(name):
        s = DC.reference(name, opt).sel
        at = _vectors_at_threshold(inp, s.l, s.w0_dot, s.dot)
        diff += sum(1 for n_col, n_vec in at if n_vec > 1)
        copies += sum(1 for n_col, n_vec in at if n_vec == 1 and n_col > 1)
        if 0 < opt.k < C:
            few = ~s.dot[3] & (s.w0_dot.sum(dim=1) < opt.k)
            mixed += int(min(int(few.sum()), int(s.dot[3].sum())) >= 10)
    print(f"DENSE_TIES {name}: rho < 1 between different candidates {diff} rows, between copies {copies} rows, "
          f"option sets with >= 10 restricted and >= 10 short rows {mixed}")
    assert diff >= 1 and copies >= 1 and mixed >= 1, (name, diff, copies, mixed)


@pytest.mark.parametrize("name", list(DC.CASES))
def test_at_most_five_percent_of_a_case_s_rows_are_flagged(name):
    N = DC.CASES[name].N
    for opt in DC.opts_of(name):
        r = DC.reference(name, opt)
        print(f"DENSE_FLAGGED {name} masked={opt.masked} k={opt.k}: {int(r.flagged.sum())} of {N}")
        assert int(r.flagged.sum()) <= 0.05 * N, (name, opt, int(r.flagged.sum()))
        d = (r.sel.l - r.sel.dot[1][:, None]).abs()  # the dot selection needs no guard: at the threshold, or a grid step away
        assert not bool(((r.sel.w0_dot > 0) & (d > 0) & (d < LC.Q_GRID * LC.E_GRID * 2.0 ** -30)).any())


# ------------------------------------------------------------------------------------------------ (c)
_SHARE: dict = {}  # case -> what -> the model's worst share of the limit


@pytest.fixture(scope="module", autouse=True)
def _report():
    """Prints the fp32 model's share of each limit (pytest -s): profiles/dense_loss.md is made from these lines."""
    yield
    for name, worst in _SHARE.items():
        print(f"DENSE_MODEL {name} " + " ".join(f"{k.replace(' ', '_')} {v:.3f}" for k, v in sorted(worst.items())))


def _group(what: str) -> str:
    return what if what.startswith("d_") else what.split(" ")[0]


@pytest.mark.parametrize("name", list(DC.CASES))
def test_fp32_model_stays_within_two_thirds_of_every_limit(name):
    inp = DC.inputs(name)
    worst = _SHARE.setdefault(name, {})
    for opt, head, all_heads in DC.launches(name):
        ms = DC.measure(DC.model(inp, opt, head, all_heads), DC.reference(name, opt), inp, opt, head, all_heads)
        assert not DC.failures(ms, 2 / 3), (name, opt, head, all_heads, DC.failures(ms, 2 / 3))
        for m in ms:
            if m.limit > 0:
                worst[_group(m.what)] = max(worst.get(_group(m.what), 0.0), m.err / m.limit)


# where each fault is looked for first (any matrix or edge case would do; these are the cheap ones that can show it)
_WHERE = {"dq_cols_256": ("w260",), "dq_cols_768": ("w1024",), "diag_as_first": ("w68-diagonal",),
          "dcand_no_clamp_branch": ("clamped",), "skip_last_group": ("c17", "w68"), "reduce_first_256": ("c257", "w68"),
          "stat_sums_fp32": ("n1",)}  # (the one fault that only a single-row case shows: every selected logit equal)


@pytest.mark.parametrize("fault", DC.FAULTS)
def test_every_wrong_kernel_misses_a_limit(fault):
    caught = []
    for name in _WHERE.get(fault, ("c2", "c16", "c17", "c257", "w68")):
        assert name in DC.MATRIX + DC.EDGES or fault == "stat_sums_fp32"
        inp = DC.inputs(name)
        for opt, head, all_heads in DC.launches(name):
            bad = DC.failures(DC.measure(DC.model(inp, opt, head, all_heads, fault), DC.reference(name, opt), inp, opt, head,
                                         all_heads))
            if bad:
                caught.append((name, opt, head, all_heads, bad[0]))
        if caught:
            break
    print(f"DENSE_FAULT {fault}: {len(caught)} launches of {name} miss a limit, first {caught[:1]}")
    assert caught, fault
