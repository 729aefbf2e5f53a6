"""Every form of the LDS-DMA bf16 loss kernels (csrc/loss_dma.inc with its launcher xfl_launch_form<H>, loss_plan, run_loss
and loss_combine_kernel of csrc/loss.hip) against fp64 references, on inputs whose dot logits are EXACT in the kernels
(tests/loss_cases.py; preconditions proven on the CPU by test_loss_cases_host.py).

With exact logits no mask and no hinge indicator can flip, so nothing here gets a "flips" allowance or a hinge
exemption: loss sums are held to the project's fp32 value limit (only fp32 epilogue arithmetic is left; a case that
misses it for a reason that is rounding would be listed in BF16_VALUE_LIMIT and in profiles/loss_dma_forms.md -- none
is), counts are exact, the other statistics at the bf16 value limit, and dL/dtok -- whole tensor and each 128-query block --
at the plain bf16 gradient limit (the one bf16 step left is the rounding of the gradient weights). Plans agree to 1e-6
(the online-maximum InfoNCE too: test_online_maximum_infonce_gradient_agrees_across_plans), a second run is
bit-identical, and the generic kernels (bf16 without the table copy, fp32) meet the same limits on the same inputs,
which shows that the inputs, not the kernel family, earn them.

How a call reaches a kernel form (loss_plan -> run_loss -> xfl_launch_form<H> -> loss_main_dma_kernel<H, HEAD_CODE, QIMG>;
tests/test_loss_plan_host.py asks the plan for the codes named here):
  * all_heads = True: gradient pass of the train head + logging pass (code -2 when the train head is InfoNCE, whose value
    then comes from the gradient records; -1 otherwise); all_heads = False: gradient pass only; AlignmentLoss has no
    gradient pass: logging pass -1, its gradient in loss_combine_kernel; all_heads = 2 without a gradient: logging only.
  * plan (1, 1): one split, rows finished INSIDE the gradient kernel (fp32 query rows, QIMG = false);
    (3, 3): split records + partial dQ, loss_combine_kernel finishes, query rows from the bf16 image (QIMG = true);
    (3, 1): logging pass in three splits on the image, gradient pass in one with the in-kernel finish.
The comment on each candidate group below names the head codes."""

import pytest
import torch

import loss_cases as LC
from helpers import TOL, loss_tol, rel_l2
from oracle.losses import LOSS_KINDS

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PLANS = ((1, 1), (3, 3), (3, 1))
STAT_NAMES = ("neg_density", "pos_mean", "pos_std", "pos_min", "pos_max", "neg_mean", "neg_std", "neg_min", "neg_max")
# Candidate groups: name -> (reference candidates, mask_false_negatives). Head codes per train head, gradient pass:
#   batch_masked     CCL -> HEAD_CCL_MASKED, Contrastive -> HEAD_CONTR_MASKED, InfoNCE -> HEAD_INFONCE_MASKED,
#                    PairwiseLogistic -> HEAD_BPR_MASKED (the lean epilogues); NCE, PairwiseHinge -> their general codes.
#                    Logging: H <= 256 HEAD_LOG_MASKED_LSE (-1) / HEAD_LOG_MASKED (-2), H = 384 the general -1 / -2.
#   batch_unmasked   every head its general code XFMR_LOSS_*; InfoNCE: H <= 128 online maximum in one part; H > 128
#                    all_heads = 1 -> HEAD_INFONCE_PINNED after a -2 logging pass, all_heads = False -> online maximum in
#                    2 (H = 256) / 3 (H = 384) dQ column parts, which keep the split form whatever the plan.
#                    Logging: general -1 / -2.
#   catalog_unmasked as batch_unmasked over every table row (mode NEG_CATALOG); logging -2 (InfoNCE trained, all heads):
#                    H <= 256 HEAD_LOG_UNMASKED_CATALOG, H = 384 general -2; otherwise general -1.
#   catalog_masked   admitted by check_loss_args: InfoNCE -> HEAD_INFONCE_MASKED, every other head and the logging
#                    passes general (the lean cosine / BPR epilogues and HEAD_LOG_MASKED* want in-batch negatives).
CANDS = {"batch_masked": ("batch", True), "batch_unmasked": ("batch", False),
         "catalog_unmasked": ("catalog", False), "catalog_masked": ("catalog", True)}
# (H, candidate group, loss) that takes loss_tol("bf16", w, flips=False) instead of the fp32 limit, with the reason:
BF16_VALUE_LIMIT: dict = {}

_WORST: dict = {}  # (family, H, group, head) -> [worst value error, worst gradient rel-L2]


@pytest.fixture(scope="module")
def ops():
    from xfmr_rec_amd import ops as _ops

    return _ops


@pytest.fixture(scope="module", autouse=True)
def _report():
    """Prints the measured table (pytest -s): profiles/loss_dma_forms.md is made from these lines."""
    yield
    for (family, H, group, head), (ev, eg) in sorted(_WORST.items()):
        print(f"LOSS_FORMS {family} {H} {group} {head} value {ev:.2e} grad {eg:.2e}")


_DEVICE_INPUTS: dict = {}


def _device_inputs(ops, H):
    if H not in _DEVICE_INPUTS:
        c = LC.inputs(H)
        table = c.table.to(DEV)
        rn, tb = ops.table_prepare(table)
        _DEVICE_INPUTS[H] = dict(c=c, table=table, rn=rn, tb=tb, tok=c.tok.to(DEV), mask=c.mask.to(torch.uint8).to(DEV),
                                 pos=c.pos.to(DEV), neg=c.neg.to(DEV),
                                 blocks=[b.to(DEV) for b in c.qsel.nonzero().flatten().split(128)],
                                 notq=(~c.qsel).to(DEV))
    return _DEVICE_INPUTS[H]


def _run(ops, d, family, group, head, all_heads, plan, *, scale=1.0, margin=0.5, need_grad=True):
    from xfmr_rec_amd import _native as N

    cand, masked = CANDS[group]
    return ops.sampled_loss(d["tok"], d["mask"], d["pos"], d["neg"], d["table"], d["rn"], train_head=head,
                            all_heads=all_heads, mask_false_negatives=masked,
                            mode=N.NEG_CATALOG if cand == "catalog" else N.NEG_SHARED, scale=scale, margin=margin,
                            precision="fp32" if family == "fp32" else "bf16", need_grad=need_grad,
                            table_bf16=d["tb"] if family == "dma" else None, nsplit=plan[0], nsplit_grad=plan[1])


def _note(key, ev, eg):
    w = _WORST.setdefault(key, [0.0, 0.0])
    w[0], w[1] = max(w[0], ev), max(w[1], eg)


def _check_values(tag, H, group, losses, stats, ref, kinds, *, with_stats):
    from xfmr_rec_amd import _native as N

    worst = 0.0
    got = losses.tolist()
    for kind in kinds:
        w, g = ref.sums[kind], got[LOSS_KINDS.index(kind)]
        lim = TOL["fp32"]["loss_rel"] * max(1.0, abs(w))
        if (H, group, kind) in BF16_VALUE_LIMIT:
            lim = loss_tol("bf16", w, flips=False)
        assert lim <= loss_tol("bf16", w, flips=False)
        err = abs(g - w) / max(1.0, abs(w))
        print(f"  {tag} {kind}: {g!r} want {w!r} err {err:.2e}")
        assert abs(g - w) <= lim, (tag, kind, g, w)
        worst = max(worst, err)
    st = stats.tolist()
    for name in ("n_valid", "n_query", "neg_distinct"):
        assert st[N.STAT[name]] == ref.counts[name], (tag, name, st[N.STAT[name]], ref.counts[name])
    if with_stats:
        assert st[N.STAT["neg_count"]] == ref.stats["logits/neg/count"], (tag, st[N.STAT["neg_count"]])
        for name in STAT_NAMES:
            w = ref.stats["logits/" + name.replace("_", "/", 1)]
            assert abs(st[N.STAT[name]] - w) <= TOL["bf16"]["val"] * max(1.0, abs(w)), (tag, name, st[N.STAT[name]], w)
    return worst


def _check_grad(tag, d, d_tok, want):
    want = want.to(DEV)
    errs = [rel_l2(d_tok, want)] + [rel_l2(d_tok[b], want[b]) for b in d["blocks"]]
    print(f"  {tag} d_tok rel-L2 whole / per 128-query block: " + " ".join(f"{e:.2e}" for e in errs))
    assert len(errs) == 4 and max(errs) <= TOL["bf16"]["grad_l2"], (tag, errs)  # no flips factor, no hinge exemption
    assert float(d_tok[d["notq"]].abs().max()) == 0.0, tag  # rows that are not queries
    return max(errs)


def _same(a, b, tag):
    assert torch.equal(a[0], b[0]), (tag, "losses of two runs")
    assert torch.equal(torch.isnan(a[1]), torch.isnan(b[1])) and torch.equal(
        torch.nan_to_num(a[1], nan=-7.0), torch.nan_to_num(b[1], nan=-7.0)), (tag, "statistics of two runs")
    assert (a[2] is None and b[2] is None) or torch.equal(a[2], b[2]), (tag, "d_tok of two runs")


def _check_matrix(ops, family, H, group, heads, all_heads_modes, plans, *, scale=1.0, margin=0.5):
    """Every (train head, all_heads, plan) of one width and candidate group against the shared fp64 reference, then
    plan against plan (1e-6) and run against run (bit for bit)."""
    d = _device_inputs(ops, H)
    cand, masked = CANDS[group]
    ref = LC.reference(H, cand, masked, scale, margin)
    for head in heads:
        for all_heads in all_heads_modes:
            first = None
            for plan in plans:
                tag = f"{family} H={H} {group} {head} all_heads={all_heads} plan={plan} scale={scale} margin={margin}"
                out = _run(ops, d, family, group, head, all_heads, plan, scale=scale, margin=margin)
                again = _run(ops, d, family, group, head, all_heads, plan, scale=scale, margin=margin)
                torch.cuda.synchronize()
                ev = _check_values(tag, H, group, out[0], out[1], ref, LOSS_KINDS if all_heads else (head,),
                                   with_stats=bool(all_heads))
                eg = _check_grad(tag, d, out[2], ref.d_tok[head])
                _note((family, H, group, head), ev, eg)
                _same(out, again, tag)
                if first is None:
                    first = out
                    continue
                for kind in (LOSS_KINDS if all_heads else (head,)):  # plan against plan
                    i = LOSS_KINDS.index(kind)
                    assert float(out[0][i]) == pytest.approx(float(first[0][i]), rel=1e-6, abs=1e-6), (tag, kind)
                e = rel_l2(out[2], first[2])
                print(f"  {tag} d_tok against plan {plans[0]}: {e:.2e}")
                assert e <= 1e-6, (tag, e)
                if all_heads:
                    assert torch.allclose(out[1], first[1], rtol=1e-6, atol=1e-6, equal_nan=True), tag


@pytest.mark.parametrize("group", list(CANDS))
@pytest.mark.parametrize("H", LC.WIDTHS)
def test_dma_forms_all_heads_and_lean_in_three_plans_vs_fp64(ops, H, group):
    """Default configuration (scale 1, margin 0.5): seven train heads x {all heads, lean} x three plans."""
    _check_matrix(ops, "dma", H, group, LOSS_KINDS, (True, False), PLANS)


@pytest.mark.parametrize("group", ["batch_masked", "batch_unmasked", "catalog_unmasked"])
@pytest.mark.parametrize("H", LC.WIDTHS)
def test_dma_forms_with_scale_2_and_margin_03_vs_fp64(ops, H, group):
    """scale = 2 (InfoNCE: the shared-exponential logging epilogue at H <= 128 needs scale 1 and is left) and margin = 0.3
    (cosine margin, pairwise kink), for the heads that read them; the other heads' sums ride along under all_heads."""
    heads = ("InfoNCELoss", "PairwiseHingeLoss", "PairwiseLogisticLoss", "AlignmentContrastiveLoss", "ContrastiveLoss")
    _check_matrix(ops, "dma", H, group, heads, (True, False), ((1, 1), (3, 3)), scale=2.0, margin=0.3)


@pytest.mark.parametrize("H", LC.WIDTHS)
def test_online_maximum_infonce_gradient_agrees_across_plans(ops, H):
    """Unmasked InfoNCE with the online maximum (lean LDS-DMA form, in 1 / 2 / 3 dQ column parts; generic bf16 kernel):
    dL/dtok of plans (1, 1), (3, 3) and (3, 1) to 1e-6, the limit every other form meets.

    This test found the one defect of the matrix: the gradient weight 2^(scale log2e l - m) was taken against the RUNNING
    maximum m of the columns a split had walked so far and rounded to bf16 for the dQ product, so two plans rounded the
    same weight at different scales and differed by 3.6e-4 ... 5.5e-4 rel-L2 (each within 7e-4 of fp64). Since then
    loss_epilogue_t (csrc/loss_common.h) keeps m an integer and takes the weight as 2^frac(x) scaled by the exact power
    of two 2^(floor(x) - m), and the pinned form pins an integer too: measured <= 3.0e-7 between plans."""
    d = _device_inputs(ops, H)
    worst = {}
    for family in ("dma", "generic_bf16"):
        for group in ("batch_unmasked", "catalog_unmasked"):
            for scale in (1.0, 2.0):
                outs = [_run(ops, d, family, group, "InfoNCELoss", False, plan, scale=scale)[2] for plan in PLANS]
                for plan, o in zip(PLANS[1:], outs[1:]):
                    e = rel_l2(o, outs[0])
                    print(f"  {family} H={H} {group} scale={scale} online-maximum InfoNCE d_tok, plan {plan} against (1, 1): {e:.2e}")
                    worst[(family, group, scale, plan)] = e
    assert max(worst.values()) <= 1e-6, {k: f"{v:.2e}" for k, v in worst.items() if v > 1e-6}


@pytest.mark.parametrize("group", list(CANDS))
@pytest.mark.parametrize("H", LC.WIDTHS)
def test_dma_values_only_logging_pass_skips_the_train_head(ops, H, group):
    """all_heads = 2 without a gradient (the step's deferred logging call): the logging pass alone -- code -2 when the train
    head is InfoNCE (no log-sum-exp), -1 otherwise --, the train head's own sum left out (0)."""
    d = _device_inputs(ops, H)
    cand, masked = CANDS[group]
    ref = LC.reference(H, cand, masked)
    for head in ("InfoNCELoss", "PairwiseLogisticLoss"):
        first = None
        for ns in (1, 3):
            tag = f"dma H={H} {group} {head} all_heads=2 nsplit={ns}"
            out = _run(ops, d, "dma", group, head, 2, (ns, ns), need_grad=False)
            again = _run(ops, d, "dma", group, head, 2, (ns, ns), need_grad=False)
            torch.cuda.synchronize()
            assert out[2] is None and float(out[0][LOSS_KINDS.index(head)]) == 0.0, tag
            ev = _check_values(tag, H, group, out[0], out[1], ref, [k for k in LOSS_KINDS if k != head], with_stats=True)
            _note(("dma", H, group, "logging-only"), ev, 0.0)
            _same(out, again, tag)
            if first is not None:
                assert torch.allclose(out[0], first[0], rtol=1e-6, atol=1e-6), tag
                assert torch.allclose(out[1], first[1], rtol=1e-6, atol=1e-6, equal_nan=True), tag
            first = out


@pytest.mark.parametrize("H", LC.WIDTHS)
def test_dma_forms_through_the_lists_entry_vs_fp64(ops, H):
    """ops.sampled_loss_lists (compacted queries + a negative list) shares run_loss: masked and unmasked in-batch forms
    of three heads, both plans."""
    d = _device_inputs(ops, H)
    c = d["c"]
    q, pos_q, negs = d["tok"][d["c"].qsel.to(DEV)].contiguous(), c.pos[c.qsel].to(DEV), c.neg[c.mask].to(DEV)
    for group in ("batch_masked", "batch_unmasked"):
        cand, masked = CANDS[group]
        ref = LC.reference(H, cand, masked)
        for head in ("InfoNCELoss", "AlignmentContrastiveLoss", "PairwiseHingeLoss"):
            for all_heads in (True, False):
                for plan in ((1, 1), (3, 3)):
                    tag = f"lists H={H} {group} {head} all_heads={all_heads} plan={plan}"
                    kw = dict(train_head=head, all_heads=all_heads, mask_false_negatives=masked, precision="bf16",
                              table_bf16=d["tb"], nsplit=plan[0], nsplit_grad=plan[1])
                    losses, stats, d_q = ops.sampled_loss_lists(q, pos_q, negs, d["table"], d["rn"], **kw)
                    again = ops.sampled_loss_lists(q, pos_q, negs, d["table"], d["rn"], **kw)
                    torch.cuda.synchronize()
                    ev = _check_values(tag, H, group, losses, stats, ref, LOSS_KINDS if all_heads else (head,),
                                       with_stats=bool(all_heads))
                    want = ref.d_tok[head][c.qsel].to(DEV)
                    errs = [rel_l2(d_q, want)] + [rel_l2(a, b) for a, b in zip(d_q.split(128), want.split(128))]
                    print(f"  {tag} d_query rel-L2: " + " ".join(f"{e:.2e}" for e in errs))
                    assert max(errs) <= TOL["bf16"]["grad_l2"], (tag, errs)
                    _note(("lists", H, group, head), ev, max(errs))
                    _same((losses, stats, d_q), again, tag)


@pytest.mark.parametrize("group", list(CANDS))
@pytest.mark.parametrize("H", LC.WIDTHS)
@pytest.mark.parametrize("family", ["generic_bf16", "fp32"])
def test_generic_kernels_meet_the_same_limits_on_the_same_inputs(ops, family, H, group):
    """Control: loss_main_kernel in the bf16 policy (no table copy passed) and in the fp32 policy, same cases, same
    references, same limits: the exact-logit inputs earn the limits, not the LDS-DMA family."""
    _check_matrix(ops, family, H, group, LOSS_KINDS, (True, False), ((1, 1), (3, 3)))
