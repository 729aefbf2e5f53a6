"""The top-k hard-negative path of the fused loss (LossConfig.num_hard_negatives: logits dump by loss_main_kernel,
hard_select_kernel, loss pass loss_epilogue_t<..., HARD = true>; csrc/loss.hip, csrc/loss_common.h) and the generic kernel's
widest instantiations against fp64 references, on inputs whose dot logits are EXACT in the kernels (tests/loss_cases.py,
tests/loss_hard_cases.py; preconditions proven on the CPU by test_loss_cases_host.py and test_loss_hard_cases_host.py).

The loss pass decides a negative's weight (1 above the row's threshold, rho at it, 0 below) with `sv > tau` and
`sv == tau`: that works only if the dump pass, the select kernel and the loss pass produce the same bits per (query,
column) in every template width, tile policy, column split and all_heads variant. If they disagree the threshold element
of a row silently gets weight 0 or 1 instead of rho -- one negative per row, far below a "random inputs, flips allowance"
limit. With exact logits a top-k over dot logits is the same selection in bf16, fp32 and fp64, so nothing here gets a flips
allowance or a hinge exemption: loss sums at the fp32 value limit, counts exact (neg_count included), the other statistics
at the limit of test_gpu_loss_dma_forms.py, dL/dtok -- whole and per 128-query block -- at the plain bf16 limit in bf16 and
the fp32 limit in fp32. A top-k over COSINES can differ between fp32 and fp64 where another item's cosine lies within
COS_BAND of the threshold: those rows (at most 5 % per case, counted on the CPU) stay in every loss sum and leave the
gradient comparison of the two contrastive heads only.

The hard path always takes the generic kernel (loss_plan): families generic_bf16 and fp32, plans nsplit = 1 / 3 (nsplit_grad
has no meaning there). Widths 64 ... 384 walk the register-prefetch forms, 512 / 1024 (loss_cases.GENERIC_WIDTHS, with the
control matrix without top-k) direct staging and the dQ column parts."""

import pytest
import torch

import loss_cases as LC
import loss_hard_cases as HC
from helpers import TOL, rel_l2
from oracle.losses import LOSS_KINDS

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PLANS = ((1, 1), (3, 3))
STAT_NAMES = ("neg_density", "pos_mean", "pos_std", "pos_min", "pos_max", "neg_mean", "neg_std", "neg_min", "neg_max")
CANDS = {"batch_masked": ("batch", True), "batch_unmasked": ("batch", False),
         "catalog_unmasked": ("catalog", False), "catalog_masked": ("catalog", True)}
CONTRASTIVE = ("AlignmentContrastiveLoss", "ContrastiveLoss")  # the heads whose negatives are selected by cosine
# (family, H, candidate group, k, loss) that misses the fp32 value limit for a reason that is rounding -> the reason
# (it then takes the bf16 value limit; profiles/loss_hard_negatives.md lists it):
BF16_VALUE_LIMIT: dict = {}
WIDE = [("generic_bf16", 512), ("generic_bf16", 1024), ("fp32", 512)]  # 1024 has no fp32 instantiation

_WORST: dict = {}  # (family, H, group, k, head) -> [worst value error, worst gradient rel-L2]


def _matrix_cases(widths_of_family):
    return [pytest.param(f, H, g, k, id=f"{f}-{H}-{g}-k{k}") for f, H in widths_of_family for g in CANDS
            for k in HC.ks_of(CANDS[g][0], H)]


@pytest.fixture(scope="module")
def ops():
    from xfmr_rec_amd import ops as _ops

    return _ops


@pytest.fixture(scope="module", autouse=True)
def _report():
    """Prints the measured table (pytest -s): profiles/loss_hard_negatives.md is made from these lines."""
    yield
    for (family, H, group, k, head), (ev, eg) in sorted(_WORST.items()):
        print(f"LOSS_HARD {family} {H} {group} k={k} {head} value {ev:.2e} grad {eg:.2e}")


_DEVICE_INPUTS: dict = {}


def _device_inputs(ops, H):
    if H not in _DEVICE_INPUTS:
        c = LC.inputs(H)
        table = c.table.to(DEV)
        rn, tb = ops.table_prepare(table)
        _DEVICE_INPUTS[H] = dict(c=c, table=table, rn=rn, tb=tb, tok=c.tok.to(DEV), mask=c.mask.to(torch.uint8).to(DEV),
                                 pos=c.pos.to(DEV), neg=c.neg.to(DEV), qidx=c.qsel.nonzero().flatten(),
                                 notq=(~c.qsel).to(DEV))
    return _DEVICE_INPUTS[H]


def _kw(d, family, group, head, all_heads, plan, k, *, scale=1.0, margin=0.5):
    from xfmr_rec_amd import _native as N

    cand, masked = CANDS[group]
    return dict(train_head=head, all_heads=all_heads, mask_false_negatives=masked,
                mode=N.NEG_CATALOG if cand == "catalog" else N.NEG_SHARED, scale=scale, margin=margin,
                precision="fp32" if family == "fp32" else "bf16", num_hard_negatives=k,
                table_bf16=d["tb"] if family == "table_bf16" else None, nsplit=plan[0], nsplit_grad=plan[1])


def _run(ops, d, family, group, head, all_heads, plan, k, *, need_grad=True, **cfg):
    return ops.sampled_loss(d["tok"], d["mask"], d["pos"], d["neg"], d["table"], d["rn"], need_grad=need_grad,
                            **_kw(d, family, group, head, all_heads, plan, k, **cfg))


def _reference(H, group, k):
    cand, masked = CANDS[group]
    return HC.reference(H, cand, masked, k) if k else LC.reference(H, cand, masked)


def _note(key, ev, eg):
    w = _WORST.setdefault(key, [0.0, 0.0])
    w[0], w[1] = max(w[0], ev), max(w[1], eg)


def _check_values(tag, key, losses, stats, ref, kinds, *, with_stats):
    from xfmr_rec_amd import _native as N

    worst = 0.0
    got = losses.tolist()
    for kind in kinds:
        w, g = ref.sums[kind], got[LOSS_KINDS.index(kind)]
        lim = TOL["fp32"]["loss_rel"] * max(1.0, abs(w))
        if key + (kind,) in BF16_VALUE_LIMIT:
            lim = TOL["bf16"]["loss_rel"] * max(1.0, abs(w))
        err = abs(g - w) / max(1.0, abs(w))
        print(f"  {tag} {kind}: {g!r} want {w!r} err {err:.2e}")
        assert abs(g - w) <= lim, (tag, kind, g, w)
        worst = max(worst, err)
    st = stats.tolist()
    for name in ("n_valid", "n_query", "neg_distinct"):
        assert st[N.STAT[name]] == ref.counts[name], (tag, name, st[N.STAT[name]], ref.counts[name])
    if with_stats:
        print(f"  {tag} neg_count: {st[N.STAT['neg_count']]!r} want {ref.stats['logits/neg/count']!r}")
        assert st[N.STAT["neg_count"]] == ref.stats["logits/neg/count"], (tag, st[N.STAT["neg_count"]])
        for name in STAT_NAMES:
            w = ref.stats["logits/" + name.replace("_", "/", 1)]
            assert abs(st[N.STAT[name]] - w) <= TOL["bf16"]["val"] * max(1.0, abs(w)), (tag, name, st[N.STAT[name]], w)
    return worst


def _check_grad(tag, d, d_tok, want, limit, leave_out=None):
    """Whole tensor and each 128-query block at `limit` (no flips factor, no hinge exemption); `leave_out`: (n_query,)
    bool, query rows excluded from the comparison (cosine near-ties at the threshold, contrastive heads only)."""
    qidx = d["qidx"] if leave_out is None else d["qidx"][~leave_out]
    blocks = [b[~leave_out[i * 128:(i + 1) * 128]] if leave_out is not None else b
              for i, b in enumerate(d["qidx"].split(128))]
    got = d_tok.double().cpu()
    errs = [rel_l2(got[qidx], want[qidx])] + [rel_l2(got[b], want[b]) for b in blocks]
    print(f"  {tag} d_tok rel-L2 whole / per 128-query block: " + " ".join(f"{e:.2e}" for e in errs))
    assert len(errs) == 4 and max(errs) <= limit, (tag, errs)
    assert float(d_tok[d["notq"]].abs().max()) == 0.0, tag  # rows that are not queries
    return max(errs)


def _same(a, b, tag, what="two runs"):
    assert torch.equal(a[0], b[0]), (tag, "losses of " + what)
    assert torch.equal(torch.isnan(a[1]), torch.isnan(b[1])) and torch.equal(
        torch.nan_to_num(a[1], nan=-7.0), torch.nan_to_num(b[1], nan=-7.0)), (tag, "statistics of " + what)
    assert (a[2] is None and b[2] is None) or torch.equal(a[2], b[2]), (tag, "d_tok of " + what)


def _grad_limit(family):
    return TOL["fp32" if family == "fp32" else "bf16"]["grad_l2"]


def _check_matrix(ops, family, H, group, k, *, heads=LOSS_KINDS, grad_limit=None):
    """Every (train head, all_heads, plan) of one width, candidate group and k against the shared fp64 reference, then plan
    against plan (1e-6) and run against run (bit for bit); with the restriction off, against the call without top-k (bits)."""
    d = _device_inputs(ops, H)
    ref = _reference(H, group, k)
    # k >= 1 + N columns (in-batch: one per valid position + the positive; catalogue: the table's rows): restriction off
    off = k >= ref.counts["n_valid"] + (CANDS[group][0] == "batch")
    limit = _grad_limit(family) if grad_limit is None else grad_limit
    key = (family, H, group, k)
    for head in heads:
        for all_heads in (True, False):
            first = None
            for plan in PLANS:
                tag = f"{family} H={H} {group} k={k} {head} all_heads={all_heads} plan={plan}"
                out = _run(ops, d, family, group, head, all_heads, plan, k)
                again = _run(ops, d, family, group, head, all_heads, plan, k)
                torch.cuda.synchronize()
                ev = _check_values(tag, key, out[0], out[1], ref, LOSS_KINDS if all_heads else (head,),
                                   with_stats=bool(all_heads))
                eg = _check_grad(tag, d, out[2], ref.d_tok[head], limit,
                                 ref.flagged if (k and head in CONTRASTIVE) else None)
                _note(key + (head,), ev, eg)
                _same(out, again, tag)
                if off:
                    _same(out, _run(ops, d, family, group, head, all_heads, plan, 0), tag, "the call without top-k")
                if first is None:
                    first = out
                    continue
                for kind in (LOSS_KINDS if all_heads else (head,)):  # plan against plan
                    i = LOSS_KINDS.index(kind)
                    assert float(out[0][i]) == pytest.approx(float(first[0][i]), rel=1e-6, abs=1e-6), (tag, kind)
                e = rel_l2(out[2], first[2])
                print(f"  {tag} d_tok against plan {PLANS[0]}: {e:.2e}")
                assert e <= 1e-6, (tag, e)
                if all_heads:
                    assert torch.allclose(out[1], first[1], rtol=1e-6, atol=1e-6, equal_nan=True), tag


@pytest.mark.parametrize("family,H,group,k", _matrix_cases([(f, H) for f in ("generic_bf16", "fp32") for H in LC.WIDTHS]))
def test_hard_negatives_all_heads_and_lean_in_two_plans_vs_fp64(ops, family, H, group, k):
    """Seven train heads x {all heads, lean} x nsplit {1, 3}; k small / middle / large / off (loss_hard_cases.K_BATCH,
    K_CATALOG: the catalogue's k = V restricts no row but sets the density's num_neg, k = V + 1 is off)."""
    _check_matrix(ops, family, H, group, k)


@pytest.mark.parametrize("family,H,group,k", _matrix_cases(WIDE))
def test_hard_negatives_at_the_widest_generic_widths_vs_fp64(ops, family, H, group, k):
    """Template widths 512 (fp32: the widest, direct staging) and 1024 (bf16 only), two k per candidate kind."""
    _check_matrix(ops, family, H, group, k)


@pytest.mark.parametrize("group", list(CANDS))
@pytest.mark.parametrize("family,H", WIDE)
def test_widest_generic_widths_without_top_k_vs_fp64(ops, family, H, group):
    """The control matrix of test_gpu_loss_dma_forms.py::test_generic_kernels_meet_the_same_limits_on_the_same_inputs,
    with its limits (fp32 value limit, bf16 gradient limit in both families), at widths 512 and 1024."""
    _check_matrix(ops, family, H, group, 0, grad_limit=TOL["bf16"]["grad_l2"])


@pytest.mark.parametrize("H", LC.WIDTHS + LC.GENERIC_WIDTHS)
def test_table_copy_does_not_leave_the_generic_path(ops, H):
    """With num_hard_negatives the plan keeps the generic kernel also when the bf16 table copy is passed (the LDS-DMA
    kernels know no thresholds): same bits as the call without it."""
    d = _device_inputs(ops, H)
    for group, k in (("batch_masked", 40 if H in LC.WIDTHS else 3), ("catalog_unmasked", 40)):
        for head in ("InfoNCELoss", "ContrastiveLoss"):
            for plan in PLANS:
                tag = f"table_bf16 H={H} {group} k={k} {head} plan={plan}"
                _same(_run(ops, d, "table_bf16", group, head, True, plan, k),
                      _run(ops, d, "generic_bf16", group, head, True, plan, k), tag, "the calls with and without the copy")


@pytest.mark.parametrize("group", list(CANDS))
@pytest.mark.parametrize("H", LC.WIDTHS)
def test_hard_negatives_values_only_skips_the_train_head(ops, H, group):
    """all_heads = 2 without a gradient (the step's deferred logging call) under the restriction: the train head's own sum
    left out (0), the other six and the statistics as in the matrix."""
    d = _device_inputs(ops, H)
    k = 40
    ref = _reference(H, group, k)
    for family in ("generic_bf16", "fp32"):
        for head in ("InfoNCELoss", "PairwiseLogisticLoss"):
            first = None
            for plan in PLANS:
                tag = f"{family} H={H} {group} k={k} {head} all_heads=2 plan={plan}"
                out = _run(ops, d, family, group, head, 2, plan, k, need_grad=False)
                again = _run(ops, d, family, group, head, 2, plan, k, need_grad=False)
                torch.cuda.synchronize()
                assert out[2] is None and float(out[0][LOSS_KINDS.index(head)]) == 0.0, tag
                ev = _check_values(tag, (family, H, group, k), out[0], out[1], ref, [x for x in LOSS_KINDS if x != head],
                                   with_stats=True)
                _note((family, H, group, k, "logging-only"), ev, 0.0)
                _same(out, again, tag)
                if first is not None:
                    assert torch.allclose(out[0], first[0], rtol=1e-6, atol=1e-6), tag
                    assert torch.allclose(out[1], first[1], rtol=1e-6, atol=1e-6, equal_nan=True), tag
                first = out


@pytest.mark.parametrize("H", LC.WIDTHS)
def test_hard_negatives_through_the_lists_entry_vs_fp64(ops, H):
    """ops.sampled_loss_lists (compacted queries + a negative list) shares run_loss: both in-batch groups, a small and the
    large k, three heads, both plans, both families."""
    d = _device_inputs(ops, H)
    c = d["c"]
    q, pos_q, negs = d["tok"][c.qsel.to(DEV)].contiguous(), c.pos[c.qsel].to(DEV), c.neg[c.mask].to(DEV)
    for family in ("generic_bf16", "fp32"):
        for group in ("batch_masked", "batch_unmasked"):
            for k in (HC.K_BATCH[0], HC.K_BATCH[2]):
                ref = _reference(H, group, k)
                for head in ("InfoNCELoss", "AlignmentContrastiveLoss", "PairwiseHingeLoss"):
                    for all_heads in (True, False):
                        for plan in PLANS:
                            tag = f"lists {family} H={H} {group} k={k} {head} all_heads={all_heads} plan={plan}"
                            kw = _kw(d, family, group, head, all_heads, plan, k)
                            losses, stats, d_q = ops.sampled_loss_lists(q, pos_q, negs, d["table"], d["rn"], **kw)
                            again = ops.sampled_loss_lists(q, pos_q, negs, d["table"], d["rn"], **kw)
                            torch.cuda.synchronize()
                            ev = _check_values(tag, (family, H, group, k), losses, stats, ref,
                                               LOSS_KINDS if all_heads else (head,), with_stats=bool(all_heads))
                            keep = ~ref.flagged if head in CONTRASTIVE else torch.ones_like(ref.flagged)
                            want, got = ref.d_tok[head][c.qsel][keep], d_q.double().cpu()[keep]
                            cut = keep.cumsum(0)[127::128].tolist()  # the 128-query blocks after the flagged rows left
                            errs = [rel_l2(got, want)] + [rel_l2(got[a:b], want[a:b])
                                                          for a, b in zip([0] + cut, cut + [len(want)])]
                            print(f"  {tag} d_query rel-L2: " + " ".join(f"{e:.2e}" for e in errs))
                            assert max(errs) <= _grad_limit(family), (tag, errs)
                            _note(("lists-" + family, H, group, k, head), ev, max(errs))
                            _same((losses, stats, d_q), again, tag)


@pytest.mark.parametrize("H", LC.WIDTHS)
def test_prepare_then_prepared_gives_the_bits_of_the_one_call_form(ops, H):
    """xfmr_sampled_loss_prepare + xfmr_sampled_loss_prepared on a caller's workspace (the step's split) against
    xfmr_sampled_loss, under the restriction."""
    d = _device_inputs(ops, H)
    n_rows = d["table"].shape[0]
    for family in ("generic_bf16", "fp32"):
        for group, k in (("batch_masked", HC.K_BATCH[2]), ("batch_unmasked", HC.K_BATCH[0]), ("catalog_unmasked", 40)):
            for head, all_heads in (("InfoNCELoss", True), ("ContrastiveLoss", False)):
                for plan in PLANS:
                    tag = f"prepared {family} H={H} {group} k={k} {head} plan={plan}"
                    kw = _kw(d, family, group, head, all_heads, plan, k)
                    one = _run(ops, d, family, group, head, all_heads, plan, k)
                    ws = ops.sampled_loss_workspace(d["tok"], LC.T, H, n_rows, **kw)
                    ops.sampled_loss_prepare(ws, d["mask"], d["pos"], d["neg"], d["rn"], n_rows, H, **kw)
                    two = ops.sampled_loss(d["tok"], d["mask"], d["pos"], d["neg"], d["table"], d["rn"], workspace=ws,
                                           prepared=True, **kw)
                    torch.cuda.synchronize()
                    _same(one, two, tag, "the one-call and the prepared form")


@pytest.mark.parametrize("entry", ["one_call", "prepare", "prepared"])
def test_workspace_sized_without_the_dump_is_refused_before_any_launch(ops, entry):
    """xfmr_sampled_loss_workspace knows no cfg and carves no logits dump: with num_hard_negatives every entry answers
    XFMR_EWORKSPACE (-3), and neither the workspace nor the gradient buffer is touched."""
    from xfmr_rec_amd import _native as N

    H = 64
    d = _device_inputs(ops, H)
    n_rows = d["table"].shape[0]
    kw = _kw(d, "generic_bf16", "batch_masked", "InfoNCELoss", True, (0, 0), 40)
    small = N.load().xfmr_sampled_loss_workspace(LC.T, H, n_rows)
    assert 0 < small < ops.sampled_loss_workspace(d["tok"], LC.T, H, n_rows, **kw).numel()
    ws = torch.full((small,), 0xAB, dtype=torch.uint8, device=DEV)
    d_tok = torch.full_like(d["tok"], 7.0)
    with pytest.raises(RuntimeError, match=r"code -3"):
        if entry == "prepare":
            ops.sampled_loss_prepare(ws, d["mask"], d["pos"], d["neg"], d["rn"], n_rows, H, **kw)
        else:
            ops.sampled_loss(d["tok"], d["mask"], d["pos"], d["neg"], d["table"], d["rn"], workspace=ws,
                             prepared=entry == "prepared", d_tok_zeroed=d_tok, **kw)
    torch.cuda.synchronize()
    assert bool((ws == 0xAB).all()) and bool((d_tok == 7.0).all())
