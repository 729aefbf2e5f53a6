"""The LDS-DMA loss kernels' tile loop at the shapes where its address forms can go wrong (csrc/loss_dma.inc: the unrolled
tile pairs with their odd tail, the resident gather constants, the unsigned piece arithmetic) and the InfoNCE gradient
pass without its count (LossArgs::no_count; loss_plan's grad_no_count, XFMR_LOSS_STATS_ELSEWHERE).

Inputs follow tests/loss_cases.py -- query entries multiples of 2^-6, table entries multiples of 2^-7, so every dot logit
is exact in the kernels and no mask or hinge decision can flip; rows inside its guard band (near_discontinuity) are not
made queries -- and the limits are test_gpu_loss_dma_forms.py's (its _check_values: loss sums at the fp32 value limit,
exact counts, statistics at the bf16 value limit; dL/dtok at the plain bf16 gradient limit), against the same fp64
oracles (oracle.lean for in-batch negatives, oracle.losses over the expanded table for the catalogue).

Shapes: H in {64, 128, 256}; queries in {1, 33, 130, 257} (partial query blocks); distinct columns in {1, 63, 64, 65, 129,
1024, 1025, 1090}: a partial last tile, an odd tile count, a second side-data chunk (16 tiles each) of one tile and of
two; the gradient pass in 1, 2 and 3 column splits (XFMR_LOSS_NSPLIT_GRAD) under a three-split plan. Every (queries,
columns) pair runs at H = 128, and each of the two values with every width at H = 64 / 256 (a rotation). The catalogue
groups need a table of `columns` rows of which row 0 is the padding row, so they run from 63 columns on, and where the
fp64 reference's expanded (queries, columns, H) tensor stays under 64 MB.

Per case: every train head x {all heads, train head alone} x the three gradient plans, which walks every gradient code and
every logging code the launcher builds for the width (group -> code: test_gpu_loss_dma_forms.py's table)."""

import functools
import types

import pytest
import torch

import loss_cases as LC
import test_gpu_loss_dma_forms as F
from helpers import TOL, rel_l2
from oracle import lean
from oracle import losses as OL
from oracle.losses import LOSS_KINDS

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
QUERIES = (1, 33, 130, 257)
COLUMNS = (1, 63, 64, 65, 129, 1024, 1025, 1090)
GRAD_SPLITS = (1, 2, 3)
NSPLIT = 3
SHAPES = list(dict.fromkeys(
    [(128, q, n) for q in QUERIES for n in COLUMNS] +
    [(H, QUERIES[(i + j) % 4], n) for j, H in enumerate((64, 256)) for i, n in enumerate(COLUMNS)] +
    [(H, q, COLUMNS[(2 * i + j + 1) % 8]) for j, H in enumerate((64, 256)) for i, q in enumerate(QUERIES)]))
CATALOG_REF_BYTES = 64 << 20


@pytest.fixture(scope="module")
def ops():
    from xfmr_rec_amd import ops as _ops

    return _ops


def _grid_rows(g, centres, cl, level, amp, grid, lim):
    x = centres[cl] + level * amp * torch.randn(cl.numel(), centres.shape[1], generator=g).double()
    return ((x / grid).round() * grid).clamp(-lim, lim)


@functools.lru_cache(maxsize=None)
def case(H: int, nq: int, nd: int, catalog: bool):
    """(B*L)-entry inputs with exactly `nq` queries and `nd` columns. In-batch: a table of max(nd, 2) items + the padding
    row, T = max(nq, nd) + 5 + nq // 3 valid positions (+ 3 masked ones) whose negatives are the items 1..nd, each at least once
    and the surplus positions repeating them (multiplicities > 1); the first positions that pass the guard band carry a
    positive. Catalogue: the table has nd rows (row 0 the padding row), positives among rows 1..nd-1."""
    g = torch.Generator().manual_seed(1000 * H + 10 * nd + nq + (5 if catalog else 0))
    V = nd - 1 if catalog else max(nd, 2)
    amp = 0.125 * (64.0 / H) ** 0.5
    centres = (torch.randint(0, 2, (LC.CLUSTERS, H), generator=g).double() * 2 - 1) * amp
    cl = torch.randint(0, LC.CLUSTERS, (V + 1,), generator=g)
    table = _grid_rows(g, centres, cl, 0.2 + 0.8 * torch.rand(V + 1, 1, generator=g).double(), amp, LC.E_GRID, 0.25)
    table[0] = 0.0
    if nd == 1 and not catalog:
        table[1] = -table[2]  # the one column lies opposite item 2: counted under the mask for the queries of item 2
    T = max(nq, 1 if catalog else nd) + 8 + nq // 3  # (headroom for the guard band)
    mask = torch.arange(T) < T - 3
    nvalid = int(mask.sum())
    pos = torch.randint(1, V + 1, (T,), generator=g)
    if nd == 1 and not catalog:
        pos = torch.where(torch.arange(T) % 4 == 3, torch.ones_like(pos), torch.full_like(pos, 2))  # item 1: the exact tie
    if catalog:
        neg = torch.randint(1, V + 1, (T,), generator=g)  # (not read in catalogue mode)
    else:
        neg = torch.cat([torch.randperm(nd, generator=g) + 1, torch.randint(1, nd + 1, (T - nd,), generator=g)])
        neg = neg[torch.randperm(nvalid, generator=g).tolist() + list(range(nvalid, T))]
    length = 1.0 + 7.0 * torch.rand(T, 1, generator=g).double()
    tok = length * _grid_rows(g, centres, cl[pos], 0.2 + 0.7 * torch.rand(T, 1, generator=g).double(), amp, 1e-30, 1e30)
    tok = ((tok / LC.Q_GRID).round() * LC.Q_GRID).clamp(-2.0, 2.0)
    ok = mask & ~LC.near_discontinuity(table, tok, pos)
    keep = ok.nonzero().flatten()[:nq]
    assert keep.numel() == nq, (H, nq, nd, int(ok.sum()))
    qsel = torch.zeros(T, dtype=torch.bool)
    qsel[keep] = True
    pos = torch.where(qsel, pos, torch.zeros_like(pos))
    neg = torch.where(mask, neg, torch.zeros_like(neg))
    if not catalog:
        assert torch.unique(neg[mask]).numel() == nd
    return types.SimpleNamespace(H=H, table=table.float(), tok=tok.float(), mask=mask, pos=pos, neg=neg, qsel=qsel, T=T)


@functools.lru_cache(maxsize=None)
def reference(H: int, nq: int, nd: int, catalog: bool, masked: bool):
    """LC.reference for `case`: sums, statistics, counts and dL/dtok per head, fp64. Read only."""
    c = case(H, nq, nd, catalog)
    table, q, pos_q = c.table.double(), c.tok.double()[c.qsel], c.pos[c.qsel]
    cfg = dict(mask_false_negatives=masked, scale=1.0, margin=0.5)
    sums, grads = {}, {}

    def scatter(g_rows):
        d = torch.zeros(c.T, H, dtype=torch.float64)
        d[c.qsel] = g_rows
        return d

    if not catalog:
        negs = c.neg[c.mask]
        out = lean.heads_by_item(q, pos_q, negs, table, **cfg)
        for kind in LOSS_KINDS:
            _, g = lean.rows_reference_form(kind, q, pos_q, negs, table, **cfg)
            sums[kind], grads[kind] = out[f"loss/{kind}"], scatter(g)
        stats = {k: v for k, v in out.items() if k.startswith("logits/")}
        counts = dict(n_valid=int(c.mask.sum()), neg_distinct=nd)
    else:
        full = table[None].expand(q.shape[0], -1, -1)
        ocfg = dict(target_position=None, **cfg)
        for kind in LOSS_KINDS:
            qo = q.clone().requires_grad_(True)
            loss = OL.embed_loss(kind, qo, full, pos_q, **ocfg)
            (g,) = torch.autograd.grad(loss, qo)
            sums[kind], grads[kind] = loss.item(), scatter(g)
        stats = OL.logits_statistics(q, full, pos_q, **ocfg)
        l, p, _c, _cp, other = LC.pair_terms(table, q, pos_q)
        stats["logits/neg/count"] = float(((l < p) if masked else other).sum())
        counts = dict(n_valid=nd, neg_distinct=nd)
    counts["n_query"] = nq
    return types.SimpleNamespace(sums=sums, stats=stats, counts=counts, d_tok=grads)


_DEVICE: dict = {}


def device_case(ops, H, nq, nd, catalog):
    key = (H, nq, nd, catalog)
    if key not in _DEVICE:
        _DEVICE.clear()  # one case resident at a time
        c = case(*key)
        table = c.table.to(DEV)
        rn, tb = ops.table_prepare(table)
        _DEVICE[key] = dict(c=c, table=table, rn=rn, tb=tb, tok=c.tok.to(DEV), mask=c.mask.to(torch.uint8).to(DEV),
                            pos=c.pos.to(DEV), neg=c.neg.to(DEV), notq=(~c.qsel).to(DEV))
    return _DEVICE[key]


def run(ops, d, catalog, masked, head, all_heads, ns_grad, **kw):
    from xfmr_rec_amd import _native as N

    return ops.sampled_loss(d["tok"], d["mask"], d["pos"], d["neg"], d["table"], d["rn"], train_head=head,
                            all_heads=all_heads, mask_false_negatives=masked, mode=N.NEG_CATALOG if catalog else N.NEG_SHARED,
                            precision="bf16", table_bf16=d["tb"], nsplit=NSPLIT, nsplit_grad=ns_grad, **kw)


def groups_of(H, nq, nd):
    out = [("batch_masked", False, True), ("batch_unmasked", False, False)]
    if nd >= 63 and nq * nd * H * 8 <= CATALOG_REF_BYTES:
        out += [("catalog_unmasked", True, False), ("catalog_masked", True, True)]
    return out


def check_values(tag, H, group, losses, stats, ref, kinds, *, with_stats):
    """F._check_values' sums and counts; its statistics loop with the same limits, but NaN-aware: with one query the
    reference's (and the kernels') logits/pos/std is NaN."""
    from xfmr_rec_amd import _native as N

    F._check_values(tag, H, group, losses, stats, ref, kinds, with_stats=False)
    if not with_stats:
        return
    st = stats.tolist()
    assert st[N.STAT["neg_count"]] == ref.stats["logits/neg/count"], (tag, st[N.STAT["neg_count"]])
    for name in F.STAT_NAMES:
        w, g = ref.stats["logits/" + name.replace("_", "/", 1)], st[N.STAT[name]]
        if w != w:
            assert g != g, (tag, name, g, w)
        else:
            assert abs(g - w) <= TOL["bf16"]["val"] * max(1.0, abs(w)), (tag, name, g, w)


def check_grad(tag, d, d_tok, want):
    want = want.to(DEV)
    e = rel_l2(d_tok, want)
    print(f"  {tag} d_tok rel-L2 {e:.2e}")
    assert e <= TOL["bf16"]["grad_l2"], (tag, e)
    assert not bool(d_tok[d["notq"]].any()), tag  # rows that are not queries


@pytest.mark.parametrize("H,nq,nd", SHAPES)
def test_every_code_at_the_tile_loop_edge_shapes_vs_fp64(ops, H, nq, nd):
    for group, catalog, masked in groups_of(H, nq, nd):
        d = device_case(ops, H, nq, nd, catalog)
        ref = reference(H, nq, nd, catalog, masked)
        for head in LOSS_KINDS:
            for all_heads in (True, False):
                first = None
                for ns_grad in GRAD_SPLITS:
                    tag = f"H={H} q={nq} cols={nd} {group} {head} all_heads={all_heads} grad splits={ns_grad}"
                    out = run(ops, d, catalog, masked, head, all_heads, ns_grad)
                    torch.cuda.synchronize()
                    check_values(tag, H, group, out[0], out[1], ref, LOSS_KINDS if all_heads else (head,),
                                 with_stats=bool(all_heads))
                    check_grad(tag, d, out[2], ref.d_tok[head])
                    if first is None:
                        first = out
                        continue
                    # (plan against plan is test_gpu_loss_dma_forms.py's subject, at its shapes; here every plan is held to
                    #  fp64 and the figure is printed: with one query row the fp32 summation order of 1090 columns shows)
                    print(f"  {tag} d_tok against one split: {rel_l2(out[2], first[2]):.2e}")


def _stats_equal(a, b):
    return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a, nan=-7.0), torch.nan_to_num(b, nan=-7.0))


@pytest.mark.parametrize("H,nq,nd", SHAPES)
def test_infonce_gradient_without_its_count_keeps_every_other_bit(ops, H, nq, nd):
    """HEAD_INFONCE_MASKED (masked groups): the train head alone with XFMR_LOSS_STATS_ELSEWHERE against without -- d_tok
    and the train head's sum bit for bit, the count-derived statistics exactly 0 --, and all_heads = 1 against the
    overlapped step's two calls (flagged gradient call + all_heads = 2 logging call). HEAD_INFONCE_PINNED (unmasked
    catalogue, all_heads = 1: the only call that pins) runs beside its logging pass, so it never counts: with the flag and
    without it every output is the same, statistics included (they are the logging records')."""
    from xfmr_rec_amd import _native as N

    i = LOSS_KINDS.index("InfoNCELoss")
    for group, catalog, masked in groups_of(H, nq, nd):
        d = device_case(ops, H, nq, nd, catalog)
        for ns_grad in GRAD_SPLITS:
            tag = f"H={H} q={nq} cols={nd} {group} grad splits={ns_grad}"
            if masked:
                plain = run(ops, d, catalog, True, "InfoNCELoss", False, ns_grad)
                flagged = run(ops, d, catalog, True, "InfoNCELoss", False, ns_grad, stats_elsewhere=True)
                both = run(ops, d, catalog, True, "InfoNCELoss", True, ns_grad)
                logging = run(ops, d, catalog, True, "InfoNCELoss", 2, ns_grad, need_grad=False)
                torch.cuda.synchronize()
                assert torch.equal(flagged[2], plain[2]) and torch.equal(flagged[0][i], plain[0][i]), tag
                assert torch.equal(flagged[0][N.NUM_LOSSES + i], plain[0][N.NUM_LOSSES + i]), tag
                assert float(plain[1][N.STAT["neg_count"]]) > 0 or nd == 1, tag  # (the counting form counts)
                assert float(flagged[1][N.STAT["neg_count"]]) == 0.0 and float(flagged[1][N.STAT["neg_density"]]) == 0.0, tag
                for name in ("n_valid", "n_query", "neg_distinct"):
                    assert torch.equal(flagged[1][N.STAT[name]], plain[1][N.STAT[name]]), (tag, name)
                assert torch.equal(both[2], flagged[2]) and torch.equal(both[0][i], flagged[0][i]), tag
                assert float(logging[0][i]) == 0.0, tag
                others = [k for k in range(2 * N.NUM_LOSSES) if k % N.NUM_LOSSES != i]
                assert torch.equal(logging[0][others], both[0][others]), tag
                assert _stats_equal(logging[1], both[1]), tag
            elif catalog:
                plain = run(ops, d, True, False, "InfoNCELoss", True, ns_grad)
                flagged = run(ops, d, True, False, "InfoNCELoss", True, ns_grad, stats_elsewhere=True)
                torch.cuda.synchronize()
                assert torch.equal(flagged[0], plain[0]) and torch.equal(flagged[2], plain[2]), tag
                assert _stats_equal(flagged[1], plain[1]) and float(plain[1][N.STAT["neg_count"]]) > 0, tag


def test_records_are_written_not_inherited_from_a_nan_filled_workspace(ops):
    """One case over a workspace pre-filled with NaN patterns (0xFF bytes: split records, partial dQ, block sums): the
    flagged and the all-heads calls return what they return on a fresh workspace -- R_CNTD in particular is written (0)."""
    H, nq, nd = 128, 130, 1025
    d = device_case(ops, H, nq, nd, False)
    for all_heads, kw in ((False, dict(stats_elsewhere=True)), (True, {})):
        for ns_grad in GRAD_SPLITS:
            want = run(ops, d, False, True, "InfoNCELoss", all_heads, ns_grad, **kw)
            ws = ops.sampled_loss_workspace(d["tok"], d["tok"].shape[0], H, d["table"].shape[0], train_head="InfoNCELoss",
                                            all_heads=all_heads, nsplit=NSPLIT, nsplit_grad=ns_grad)
            ws.fill_(0xFF)
            got = run(ops, d, False, True, "InfoNCELoss", all_heads, ns_grad, workspace=ws, **kw)
            torch.cuda.synchronize()
            assert torch.equal(got[0], want[0]) and _stats_equal(got[1], want[1]) and torch.equal(got[2], want[2]), (all_heads, ns_grad)
            assert bool(torch.isfinite(got[2]).all()) and bool(torch.isfinite(got[0]).all())
