"""Cases of the dense-candidate loss form (csrc/dense_loss.hip: xfmr_dense_loss / xfmr_dense_loss_grads) on inputs whose
dot logits are EXACT, their fp64 references BY COLUMN, an fp32 model of the kernel's algorithm with switchable faults, and
the comparison that the CPU test (test_dense_loss_cases_host.py, on the model) and the GPU test
(test_gpu_dense_loss_forms.py, on the kernel) share. Plain module, no GPU.

Grid and construction are loss_cases.py's: query entries are multiples of 2^-6 in [-2, 2], candidate entries multiples of
2^-7 in [-0.25, 0.25], so a dot product of H <= 1024 terms is exact in fp32 in any order -- the kernel's dot logits, its
mask `l < pos` and its top-k over dot logits are the fp64 decisions. Items are a cluster centre plus noise, queries their
positive's centre plus noise at a per-row length, so that masks and margins are active. (Below H = 64 the centre entries
stay at 2^-3 instead of growing with 1 / sqrt(H): they would leave the candidate grid's range.)

A case is an index matrix `items` (N, C) into an item pool of C + 40 rows (row 0 is the zero vector): cand = pool[items].
Query rows are taken only from rows that pass loss_cases.near_discontinuity against EVERY item of the pool with their own
positive item (hinge kink, cosine mask band and cosine margin band for loss_cases.MARGINS); a row that fails is not chosen.
A row's columns are distinct items other than its positive and the zero vector, except for the plants:
    row % 2 == 0 (C >= 3): a copy of the target's item at another column -- an exact tie with the positive that is NOT the
                           positive column (masked: not a negative; unmasked: a negative like any other);
    row % 3 == 0 (C >= 8): three columns hold one non-target item, the row's best-scoring one (odd rows: the best one below
                           the positive, which stays counted under the mask) -- an exact tie between identical
                           vectors, which k = 1 splits;
    row % 4 == 0 (C >= 8): a column holds the pool's zero vector -- |e| = 0, the candidate norm is clamped;
    row N - 1 (N >= 3):    the query is all zeros and its positive is the zero vector: every logit is 0 (unmasked, every
                           column ties with every other at any threshold), |q| is clamped, and all its gradients through
                           the cosines vanish -- a 1 / 1e-8 there would set the scale of the whole tensor.
Target column: `first` 0, `diagonal` the row, `explicit` random with row 0 at C - 1 and row 1 at 0.

The case "clamped" is where the clamped-norm branches carry a gradient (of size 1e8, which is why it is a case of its own:
the per-row floor of `measure` is useless there, each such row is held relative to itself): row 0's target is a vector of
norm 2^-30 < 1e-8, row 1's query is all zeros with an ordinary target, row 2 holds such a tiny vector as a negative.

Tie rule, heads, `_wmean`: loss_hard_cases.py's (topk_weights with unit multiplicities). Cosines: F.normalize(., eps=1e-8)
on both sides (include/xfmr_hip.h). A top-k over cosines can differ between fp32 and fp64 where another counted column's
cosine lies within loss_cases.COS_BAND of the row's threshold: `reference(...).flagged` rows stay in every loss sum and
leave only the gradient comparison of the two contrastive heads."""

from __future__ import annotations

import functools
import math
import types
from typing import NamedTuple

import torch
import torch.nn.functional as F

import loss_cases as LC
import loss_hard_cases as HC
from helpers import TOL
from oracle.losses import COSINE_KINDS, LOSS_KINDS

CONTRASTIVE = ("AlignmentContrastiveLoss", "ContrastiveLoss")  # the heads whose negatives are selected by cosine
SM = ((1.0, 0.5), (20.0, 0.3))  # (scale, margin); scale 20 on these logits overflows exp in fp32 without the max shift
TINY = 2.0 ** -30  # the one non-zero entry of the "clamped" case's tiny vectors
POOL_EXTRA = 40
K_MIXED = 250
# A gradient norm below this is no fp32 quantity: the kernel's softmax weights exp2(z - max) flush to 0 below 2^-126 (at
# scale 20 a masked row's whole InfoNCE gradient can lie there), so a reference norm is never taken smaller than this.
FP32_FLOOR = 2.0 ** -100
STAT = dict(n_valid=0, n_query=1, neg_density=2, pos_mean=3, pos_std=4, pos_min=5, pos_max=6, neg_mean=7, neg_std=8,
            neg_min=9, neg_max=10, neg_count=11, neg_distinct=12)  # include/xfmr_hip.h: XFMR_STAT_*
PLANT_SHARE = dict(dup_target=(2, 3), dup_other=(3, 8), zero_cand=(4, 8))  # plant -> (every n-th row, from C =)


class Case(NamedTuple):
    name: str
    group: str  # "matrix" | "edge" | "limit" | "rows" | "clamped"
    N: int
    C: int
    H: int
    mode: str   # "first" | "diagonal" | "explicit"
    seed: int


class Opt(NamedTuple):
    masked: bool
    k: int
    scale: float
    margin: float


def _cases():
    out = []
    # N = 40, C = 273 = 256 + 17 = 17 * 16 + 1: partial in both strides (seeds chosen on the CPU: test_dense_loss_cases_host.py)
    for H, seed in ((8, 100), (68, 101), (260, 102), (384, 103), (1024, 150)):
        out.append(Case(f"w{H}", "matrix", 40, 273, H, "explicit", seed))
    out.append(Case("w68-first", "matrix", 40, 273, 68, "first", 110))
    out.append(Case("w68-diagonal", "matrix", 40, 273, 68, "diagonal", 111))
    for i, C in enumerate((1, 2, 15, 16, 17, 255, 256, 257)):
        out.append(Case(f"c{C}", "edge", 3, C, 68, "explicit", 120 + i))
    out.append(Case("limit-c", "limit", 2, 8192, 64, "explicit", 130))
    out.append(Case("limit-ch", "limit", 1, 8192, 1024, "explicit", 131))  # 135 200 bytes of LDS, a 32 MB tensor
    out.append(Case("n1", "rows", 1, 17, 68, "explicit", 140))
    out.append(Case("n33-diagonal", "rows", 33, 33, 68, "diagonal", 141))
    out.append(Case("n300", "rows", 300, 17, 8, "explicit", 142))  # the shared reduce / final kernels over > 256 records
    out.append(Case("clamped", "clamped", 5, 17, 68, "explicit", 143))
    return {c.name: c for c in out}


CASES = _cases()
MATRIX = tuple(n for n, c in CASES.items() if c.group == "matrix")
EDGES = tuple(n for n, c in CASES.items() if c.group in ("edge", "clamped"))


def ks_of(C: int):
    """num_hard_negatives: 0 (off), 1, 3, 40, C - 2 (restricts only rows with every negative counted), C - 1 (never
    restricts, sets the density's num_neg), C (off); at the matrix's C = 273 also 250, about the number of negatives the
    mask leaves a row: restricted rows and rows with fewer than k counted negatives in one launch."""
    return tuple(sorted({k for k in (0, 1, 3, 40, C - 2, C - 1, C) if k >= 0} | ({K_MIXED} if C == 273 else set())))


@functools.lru_cache(maxsize=None)
def opts_of(name: str):
    """The options a case runs with. The full list (both masks x every k, (scale, margin) alternating so that every k meets
    both) on the cheap cases; five or two on the wide ones, whose references cost seconds."""
    c = CASES[name]
    if name == "w68" or c.group in ("edge", "clamped") or name == "n1":
        return tuple(Opt(m, k, *SM[(i + j) % 2]) for i, m in enumerate((True, False)) for j, k in enumerate(ks_of(c.C)))
    k_mid = 40 if c.C > 40 else 3
    if name == "limit-ch":
        return (Opt(True, k_mid, *SM[1]), Opt(False, c.C - 2, *SM[0]))
    few = (Opt(True, k_mid, *SM[0]), Opt(False, 1, *SM[1]), Opt(True, c.C - 2, *SM[1]), Opt(False, 0, *SM[0]))
    return few + ((Opt(True, K_MIXED, *SM[0]),) if c.C == 273 else ())


def _pool_and_rows(H: int, P: int, n_try: int, seed: int):
    """loss_cases._raw_inputs' construction for a pool of P items and n_try candidate query rows."""
    g = torch.Generator().manual_seed(seed)
    amp = 0.125 * min(1.0, (64.0 / H) ** 0.5)
    centres = (torch.randint(0, 2, (LC.CLUSTERS, H), generator=g).double() * 2 - 1) * amp
    cl = torch.randint(0, LC.CLUSTERS, (P,), generator=g)
    level = 0.2 + 0.8 * torch.rand(P, 1, generator=g).double()
    pool = centres[cl] + level * amp * torch.randn(P, H, generator=g).double()
    pool = ((pool / LC.E_GRID).round() * LC.E_GRID).clamp(-0.25, 0.25)
    pool[0] = 0.0
    pos = torch.randint(1, P, (n_try,), generator=g)
    length = 1.0 + 7.0 * torch.rand(n_try, 1, generator=g).double()
    qlevel = 0.2 + 0.7 * torch.rand(n_try, 1, generator=g).double()
    tok = length * (centres[cl[pos]] + qlevel * amp * torch.randn(n_try, H, generator=g).double())
    tok = ((tok / LC.Q_GRID).round() * LC.Q_GRID).clamp(-2.0, 2.0)
    return g, pool, tok, pos


def _planted(row: int, C: int, what: str) -> bool:
    every, from_c = PLANT_SHARE[what]
    return row % every == 0 and C >= from_c


@functools.lru_cache(maxsize=None)
def inputs(name: str):
    """The case: fp32 `q` (N, H) and `cand` (N, C, H), int64 `target` (N) (the column; passed to the kernel in explicit
    mode), `items` (N, C) (-1: a tiny vector of the "clamped" case), `pos_item` (N), bool `dup_target` / `dup_other` /
    `zero_cand` (N: the row carries the plant), `zero_q` (rows with an all-zero query), `n_failed` / `n_tried` of the guard."""
    c = CASES[name]
    N, C, H = c.N, c.C, c.H
    assert c.mode != "diagonal" or N <= C
    P, n_try = C + POOL_EXTRA, 4 * N + 16
    g, pool, tok, pos = _pool_and_rows(H, P, n_try, c.seed)
    failed = LC.near_discontinuity(pool, tok, pos)
    good = (~failed).nonzero().flatten()
    assert good.numel() >= N, (name, int(good.numel()))
    q, pos_item = tok[good[:N]].clone(), pos[good[:N]].clone()
    zero_q = [N - 1] if N >= 3 else []
    for r in zero_q:
        q[r], pos_item[r] = 0.0, 0
    if c.mode == "first":
        target = torch.zeros(N, dtype=torch.int64)
    elif c.mode == "diagonal":
        target = torch.arange(N, dtype=torch.int64)
    else:
        target = torch.randint(0, C, (N,), generator=g)
        target[0] = C - 1
        if N > 1:
            target[1] = 0
    items = torch.zeros(N, C, dtype=torch.int64)
    plants = {w: torch.zeros(N, dtype=torch.bool) for w in PLANT_SHARE}
    for r in range(N):
        others = torch.randperm(P - 1, generator=g) + 1  # every item but the zero vector ...
        others = others[others != pos_item[r]][:C]       # ... and the positive: distinct columns
        items[r] = others
        t = int(target[r])
        items[r, t] = pos_item[r]
        free = torch.tensor([x for x in range(C) if x != t], dtype=torch.int64)
        free = free[torch.randperm(free.numel(), generator=g)]
        if _planted(r, C, "dup_target"):
            items[r, free[0]] = pos_item[r]
            plants["dup_target"][r] = True
        if _planted(r, C, "zero_cand"):
            items[r, free[1]] = 0
            plants["zero_cand"][r] = True
        if _planted(r, C, "dup_other"):  # the row's best-scoring other item, three times: k = 1 splits it (rho = 1 / 3)
            lr = pool[items[r]] @ q[r]
            if r % 2 and bool((lr < lr[t]).any()):  # every other time the best one BELOW the positive: masked, it counts
                lr[lr >= lr[t]] = -math.inf
            lr[free[:4]], lr[t] = -math.inf, -math.inf
            items[r, free[2]] = items[r, free[3]] = items[r, lr.argmax()]
            plants["dup_other"][r] = True
    cand = pool[items]
    if c.group == "clamped":
        cand[0, target[0]] = 0.0
        cand[0, target[0], 5] = TINY
        items[0, target[0]] = -1
        q[1] = 0.0
        zero_q = [1] + zero_q
        col = (int(target[2]) + 3) % C
        cand[2, col] = 0.0
        cand[2, col, 0] = -TINY
        items[2, col] = -1
    return types.SimpleNamespace(case=c, q=q.float(), cand=cand.float().contiguous(), target=target, items=items,
                                 pos_item=pos_item, zero_q=tuple(zero_q), n_failed=int(failed.sum()), n_tried=n_try,
                                 **plants)


# ------------------------------------------------------------------------------------------------ fp64 reference
def _logits(q, cand, tgt):
    """Differentiable (l, pos_l, cos, cos_pos), (N, C) / (N, 1). Every column is reduced by the same sum over its own H
    entries, so columns that hold the same vector get the same bits (a bmm gives no such promise)."""
    l = (q[:, None, :] * cand).sum(-1)
    c = (F.normalize(q, dim=-1, eps=1e-8)[:, None, :] * F.normalize(cand, dim=-1, eps=1e-8)).sum(-1)
    return l, l.gather(1, tgt[:, None]), c, c.gather(1, tgt[:, None])


def heads(q, cand, tgt, *, masked: bool, k: int, scale: float, margin: float):
    """Per-row values of the seven heads (dict kind -> (N,), differentiable in q and cand), LogitsStatistics (dict; keys
    without a value are absent) and the selection (`sel.dot` / `sel.cos`: weights, tau, rho, restricted), by column."""
    N, C = cand.shape[0], cand.shape[1]
    other = torch.arange(C)[None, :] != tgt[:, None]
    with torch.no_grad():
        l0, p0, c0, cp0 = _logits(q, cand, tgt)
        w0d = (other & (l0 < p0) if masked else other).double()
        w0c = (other & (c0 < cp0) if masked else other).double()
        sd = HC.topk_weights(l0, w0d, k, C)
        sc = HC.topk_weights(c0, w0c, k, C)
    wd, wc = sd[0], sc[0]
    l, p, c, cp = _logits(q, cand, tgt)
    rows = {}
    align = 1 - cp[:, 0]
    contr = HC._wmean((c - 1 + margin).relu(), wc)
    rows["AlignmentLoss"] = align
    rows["AlignmentContrastiveLoss"] = align + contr
    rows["ContrastiveLoss"] = contr
    # log(1 + sum_neg w exp(s l - s pos)): the value of loss_hard_cases.heads' shifted log-sum-exp, in the form whose
    # autograd keeps the negatives' softmax mass to RELATIVE precision. Through log(e_pos + sum) a mass below 2^-53 is lost
    # in the target's gradient even in fp64 -- at scale 20 a masked row's whole gradient is of that size.
    ratio = (wd * torch.exp((scale * (l - p)).masked_fill(wd == 0, -float("inf")))).sum(dim=1)
    assert bool(torch.isfinite(ratio).all())
    rows["InfoNCELoss"] = torch.log1p(ratio)
    rows["NCELoss"] = F.softplus(-p[:, 0]) + HC._wmean(F.softplus(l), wd)
    s = l - p * (1 - margin)
    rows["PairwiseHingeLoss"] = HC._wmean(s.relu(), wd)
    rows["PairwiseLogisticLoss"] = HC._wmean(F.softplus(s), wd)
    with torch.no_grad():  # LogitsStatistics (losses.py:375-405): the selected dot logits
        num_neg = C - 1
        if k > 0:
            num_neg = min(num_neg, k)
        cnt = wd.sum(dim=1)
        nc = float(round(float(cnt.sum())))  # (every row's weights sum to k or to its count: an integer)
        assert abs(nc - float(cnt.sum())) < 1e-6
        st = {"neg_density": float((cnt / (num_neg + 1e-9)).sum()) / N, "neg_count": nc, "pos_mean": float(p0.mean()),
              "pos_min": float(p0.min()), "pos_max": float(p0.max())}
        if N > 1:
            st["pos_std"] = float(p0.std())
        if nc > 0:
            ns, nss = float((wd * l0).sum()), float((wd * l0 * l0).sum())
            st["neg_mean"] = ns / nc
            if nc > 1:
                st["neg_std"] = max(0.0, (nss - ns * ns / nc) / (nc - 1)) ** 0.5
            st["neg_min"], st["neg_max"] = float(l0[wd > 0].min()), float(l0[wd > 0].max())
    return rows, st, types.SimpleNamespace(dot=sd, cos=sc, l=l0, p=p0, c=c0, cp=cp0, w0_dot=w0d, w0_cos=w0c)


@functools.lru_cache(maxsize=3)  # (a wide case's d_cand is 90 MB a head; a test asks for one reference at a time)
def reference(name: str, opt: Opt):
    """fp64 reference of one (case, options), per row: `rows[kind]` (N,), `sums[kind]`, `stats` (name -> float, absent where
    the reference has no value), `d_query[kind]` (N, H) and `d_cand[kind]` (N, C, H) by autograd with the selection weights
    detached, `sel` (see `heads`), `flagged` (N,) (near_tie of the cosines) and `fractional` (a weight strictly between 0
    and 1 exists: neg_count is then a sum of fractions in the kernel). Read only: the tests share it."""
    inp = inputs(name)
    qo, co = inp.q.double().requires_grad_(True), inp.cand.double().requires_grad_(True)
    rows, stats, sel = heads(qo, co, inp.target, masked=opt.masked, k=opt.k, scale=opt.scale, margin=opt.margin)
    d_query, d_cand = {}, {}
    for kind in LOSS_KINDS:
        gq, gc = torch.autograd.grad(rows[kind].sum(), (qo, co), retain_graph=True, allow_unused=True)
        d_query[kind] = torch.zeros_like(qo) if gq is None else gq
        d_cand[kind] = torch.zeros_like(co) if gc is None else gc
    rows = {kind: v.detach() for kind, v in rows.items()}
    wd = sel.dot[0]
    return types.SimpleNamespace(rows=rows, sums={kind: float(v.sum()) for kind, v in rows.items()}, stats=stats,
                                 d_query=d_query, d_cand=d_cand, sel=sel,
                                 flagged=HC.near_tie(sel.c, sel.w0_cos, sel.cos, LC.COS_BAND),
                                 fractional=bool(((wd > 0) & (wd < 1)).any()))


# ------------------------------------------------------------------------------------------------ fp32 model
FAULTS = (
    "rho_one",                   # the threshold element gets weight 1 instead of rho
    "rho_zero",                  # ... weight 0 instead of rho
    "mask_le",                   # the mask is `l <= pos`
    "value_identity",            # a copy of the target's vector is treated as the positive
    "density_c1",                # the density divides by C - 1 whatever k is
    "dq_cols_256",               # d_query columns >= 256 are dropped
    "dq_cols_768",               # d_query columns >= 768 are dropped
    "skip_last_group",           # the last partial group of 16 candidates is skipped (its LDS slots read as 0)
    "reduce_first_256",          # candidates from 256 on are left out of the row reductions
    "diag_as_first",             # `diagonal` is read as `first`
    "shift_no_pos",              # the log-sum-exp shift ignores the positive
    "no_shift",                  # no shift at all: exp(20 l) overflows fp32 from l = 4.5 on
    "dcand_no_clamp_branch",     # the clamped-candidate branch of d_candidates is missing
    "dcand_pairwise_no_margin",  # the target's d_candidates coefficient of the pairwise heads omits (1 - margin)
    "softmax_one_minus",         # InfoNCE's weight of the target as 1 - e_pos / sum instead of sum_neg / sum (cancellation)
    "stat_sums_fp32",            # the row's sums of l and l^2 behind logits/neg/std in fp32 (seen at N = 1 only: case n1)
)
_LOG2E, _LN2 = 1.4426950408889634, 0.6931471805599453


def _sort_key(v):
    """dense_loss.hip: sort_key -- monotone unsigned key of an fp32 value, here as int64."""
    b = v.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    return torch.where((b >> 31) == 1, b ^ 0xFFFFFFFF, b ^ 0x80000000)


def _model_topk(vals, counted, k: int, fault):
    """select_topk + TopK::weight: the k-th largest key among the counted, rho = (k - gt) / eq in fp32."""
    w = counted.float()
    C = vals.shape[1]
    if k <= 0 or k >= C:
        return w
    on = counted.sum(dim=1) > k
    key = torch.where(counted, _sort_key(vals), torch.full(vals.shape, -1, dtype=torch.int64))
    T = key.sort(dim=1, descending=True).values[:, k - 1:k]
    gt, eq = (key > T).sum(dim=1).float(), (key == T).sum(dim=1).float()
    rho = (float(k) - gt) / eq
    if fault == "rho_one":
        rho = torch.ones_like(rho)
    if fault == "rho_zero":
        rho = torch.zeros_like(rho)
    share = torch.where(key > T, torch.ones_like(w), torch.where(key == T, rho[:, None].expand_as(w), torch.zeros_like(w)))
    return torch.where(on[:, None], share * w, w)


def model(inp, opt: Opt, head: str, all_heads: bool, fault: str | None = None):
    """Vectorised fp32 restatement of dense_loss_kernel + the shared reduce / final kernels: the sort-key threshold,
    rho = (k - gt) / eq, fp32 sums within a row, fp64 across rows, the gradient formulas with their clamped branches.
    Returns what the kernel writes: `losses` (14,), `stats` (16,), `d_query` (N, H), `d_cand` (N, C, H), fp32. `fault`: one
    of FAULTS, a plausible wrong kernel."""
    assert fault is None or fault in FAULTS
    c = inp.case
    N, C, H = c.N, c.C, c.H
    f32 = torch.float32
    q, cand = inp.q, inp.cand
    hid = LOSS_KINDS.index(head)
    scale, margin = torch.tensor(opt.scale, dtype=f32), torch.tensor(opt.margin, dtype=f32)
    qq = (q * q).sum(-1)
    rq = 1.0 / qq.sqrt().clamp_min(1e-8)
    dot = (q[:, None, :] * cand).sum(-1) + 0.0  # (+ 0.0: the kernel's fma chains start from +0 and never give -0)
    rc = 1.0 / (cand * cand).sum(-1).sqrt().clamp_min(1e-8)
    cos = dot * rq[:, None] * rc
    if fault == "skip_last_group" and C % 16:
        dot[:, C - C % 16:], cos[:, C - C % 16:], rc[:, C - C % 16:] = 0.0, 0.0, 1.0
    tgt = inp.target.clone()
    if fault == "diag_as_first" and c.mode == "diagonal":
        tgt = torch.zeros_like(tgt)
    rows_i = torch.arange(N)
    pos, cpos, rcpos = dot[rows_i, tgt], cos[rows_i, tgt], rc[rows_i, tgt]
    is_t = torch.arange(C)[None, :] == tgt[:, None]
    not_pos = ~is_t
    if fault == "value_identity":
        not_pos = ~(cand == cand[rows_i, tgt][:, None, :]).all(-1)
    below = (lambda a, b: a <= b) if fault == "mask_le" else (lambda a, b: a < b)
    counted_d = not_pos & below(dot, pos[:, None]) if opt.masked else not_pos
    counted_c = not_pos & below(cos, cpos[:, None]) if opt.masked else not_pos
    need_dot = all_heads or head not in COSINE_KINDS
    need_cos = all_heads or head in COSINE_KINDS
    md = _model_topk(dot, counted_d, opt.k, fault) if need_dot else torch.zeros_like(dot)
    mc = _model_topk(cos, counted_c, opt.k, fault) if need_cos else torch.zeros_like(dot)
    if fault == "reduce_first_256":
        md[:, 256:], mc[:, 256:] = 0.0, 0.0
    sc2 = scale * torch.tensor(_LOG2E, dtype=f32)
    chinge = pos * (1.0 - margin)
    zs = dot * sc2
    neg_max = torch.where(md > 0, zs, torch.full_like(zs, -math.inf)).max(dim=1).values
    M = torch.maximum(pos * sc2, neg_max)
    if fault == "shift_no_pos":
        M = neg_max  # (-inf in a row without counted negatives)
    if fault == "no_shift":
        M = torch.zeros_like(neg_max)
    e = torch.where(md > 0, torch.exp2(zs - M[:, None]) * md, torch.zeros_like(md))
    d = dot - chinge[:, None]
    dc = cos - 1.0 + margin
    cnt_d, cnt_c = md.sum(1), mc.sum(1)
    l, nce, hinge, logi = e.sum(1), (F.softplus(dot) * md).sum(1), (d.relu() * md).sum(1), (F.softplus(d) * md).sum(1)
    contr = (dc.relu() * mc).sum(1)
    ssum, ssq = (dot.double() * md.double()).sum(1), (dot.double() * dot.double() * md.double()).sum(1)  # (fp64 in the kernel)
    if fault == "stat_sums_fp32":
        ssum, ssq = (dot * md).sum(1).double(), (dot * dot * md).sum(1).double()
    smin = torch.where(md > 0, dot, torch.full_like(dot, math.inf)).min(dim=1).values
    smax = torch.where(md > 0, dot, torch.full_like(dot, -math.inf)).max(dim=1).values
    epos = torch.exp2(pos * sc2 - M)
    ltot = l + epos
    inv_d, inv_c = 1.0 / (cnt_d + 1e-9), 1.0 / (cnt_c + 1e-9)
    pneg = 1.0 - epos / ltot if fault == "softmax_one_minus" else l / ltot  # the softmax mass of the negatives
    per_row = torch.stack([1.0 - cpos, (1.0 - cpos) + contr * inv_c, contr * inv_c,
                           (M + torch.log2(ltot)) * _LN2 - scale * pos, F.softplus(-pos) + nce * inv_d, hinge * inv_d,
                           logi * inv_d]).double()  # (7, N): fp32 values, summed across rows in fp64
    if not all_heads:
        per_row[torch.arange(7) != hid] = 0.0
    tot = per_row.sum(1)
    losses = torch.cat([tot, tot / (N + 1e-9)]).float()
    num_neg = C - 1
    if 0 < opt.k < num_neg and fault != "density_c1":
        num_neg = opt.k
    nan = float("nan")
    stats = torch.zeros(16, dtype=torch.float64)
    pd, nn = pos.double(), float(cnt_d.double().sum())
    s1, s2 = float(ssum.sum()), float(ssq.sum())
    stats[STAT["n_valid"]], stats[STAT["n_query"]], stats[STAT["neg_distinct"]] = C, N, C
    stats[STAT["neg_density"]] = float((cnt_d.double() / (num_neg + 1e-9)).sum()) / N
    stats[STAT["pos_mean"]] = float(pd.mean())
    stats[STAT["pos_std"]] = max(0.0, (float((pd * pd).sum()) - float(pd.sum()) ** 2 / N) / (N - 1)) ** 0.5 if N > 1 else nan
    stats[STAT["pos_min"]], stats[STAT["pos_max"]] = float(pd.min()), float(pd.max())
    stats[STAT["neg_count"]] = nn
    stats[STAT["neg_mean"]] = s1 / nn if nn > 0 else nan
    stats[STAT["neg_std"]] = max(0.0, (s2 - s1 * s1 / nn) / (nn - 1.0)) ** 0.5 if nn > 1 else nan
    stats[STAT["neg_min"]] = float(smin.min()) if nn > 0 else nan
    stats[STAT["neg_max"]] = float(smax.max()) if nn > 0 else nan
    stats[13] = N / (C + 1e-9)  # (positive / attention density of the (B*L) form: not part of the dense contract)
    # ---- gradients of the train head
    sig = torch.sigmoid
    w = {"InfoNCELoss": e, "NCELoss": md * sig(dot), "PairwiseHingeLoss": torch.where(d > 0, md, torch.zeros_like(md)),
         "PairwiseLogisticLoss": md * sig(d), "AlignmentLoss": torch.zeros_like(md)}.get(head)
    if w is None:  # the two contrastive heads: the weight carries the candidate's 1 / |e|
        w = torch.where(dc > 0, mc * rc, torch.zeros_like(mc))
    sw = w.sum(1)
    pw_t = -sw * inv_d if fault == "dcand_pairwise_no_margin" else -(1.0 - margin) * sw * inv_d
    unw = w * inv_c[:, None] * (1.0 / rc).clamp_min(1e-8)
    coef_t, coef_n = {
        "InfoNCELoss": (-scale * pneg, scale * w / ltot[:, None]),
        "NCELoss": (-sig(-pos), w * inv_d[:, None]),
        "PairwiseHingeLoss": (pw_t, w * inv_d[:, None]),
        "PairwiseLogisticLoss": (pw_t, w * inv_d[:, None]),
        "AlignmentLoss": (-torch.ones_like(pos), torch.zeros_like(w)),
        "ContrastiveLoss": (torch.zeros_like(pos), unw),
        "AlignmentContrastiveLoss": (-torch.ones_like(pos), unw),
    }[head]
    coef = torch.where(is_t, coef_t[:, None].expand_as(coef_n), coef_n)
    qh = q * rq[:, None]
    if head not in COSINE_KINDS:
        d_cand = coef[:, :, None] * q[:, None, :]
    else:
        normal = (coef * rc)[:, :, None] * (qh[:, None, :] - (cand * rc[:, :, None]) * cos[:, :, None])
        clamped = (coef * rc)[:, :, None] * qh[:, None, :]
        d_cand = normal if fault == "dcand_no_clamp_branch" else torch.where((rc >= 1e8)[:, :, None], clamped, normal)
    O = torch.einsum("nc,nch->nh", w, cand)
    et = cand[rows_i, tgt]
    g = {"InfoNCELoss": scale * (O / ltot[:, None] - pneg[:, None] * et),
         "NCELoss": -sig(-pos)[:, None] * et + O * inv_d[:, None],
         "PairwiseHingeLoss": (O - ((1.0 - margin) * sw)[:, None] * et) * inv_d[:, None],
         "PairwiseLogisticLoss": (O - ((1.0 - margin) * sw)[:, None] * et) * inv_d[:, None],
         "AlignmentLoss": -rcpos[:, None] * et, "ContrastiveLoss": O * inv_c[:, None],
         "AlignmentContrastiveLoss": -rcpos[:, None] * et + O * inv_c[:, None]}[head]
    if head in COSINE_KINDS:  # g is dL/dq_hat: the Jacobian of q / max(|q|, eps)
        dotp = (g * qh).sum(1)
        g = torch.where((qq.sqrt() < 1e-8)[:, None], g * rq[:, None], rq[:, None] * (g - qh * dotp[:, None]))
    if fault == "dq_cols_256":
        g[:, 256:] = 0.0
    if fault == "dq_cols_768":
        g[:, 768:] = 0.0
    return types.SimpleNamespace(losses=losses, stats=stats.float(), d_query=g.contiguous(), d_cand=d_cand.contiguous())


# ------------------------------------------------------------------------------------------------ the comparison
class Measure(NamedTuple):
    what: str
    err: float    # inf: an exact check (a count, fp32 bits, a NaN where none belongs) failed
    limit: float  # 0: an exact check


def _finite(x: float) -> float:
    return x if math.isfinite(x) else math.inf


def _f32(x: float) -> float:
    return float(torch.tensor(x, dtype=torch.float32))


def _rows_err(got, want, keep):
    """(whole rel-L2, worst per-row error) of (R, H) tensors over the rows `keep`: a row's error norm relative to the larger
    of its reference norm and the tensor's mean reference row norm (an absolute limit for rows with a zero or tiny
    reference gradient; no wrong row hides among forty)."""
    got, want = got.double(), want.double()
    rn = want.norm(dim=1)
    den = rn.clamp_min(max(float(rn.mean()), FP32_FLOOR))
    per = (got - want).norm(dim=1) / den
    per = torch.where(torch.isfinite(per), per, torch.full_like(per, math.inf))[keep]
    whole = float((got - want)[keep].norm()) / max(float(want[keep].norm()), FP32_FLOOR)
    return _finite(whole), (float(per.max()) if per.numel() else 0.0)


def measure(out, ref, inp, opt: Opt, head: str, all_heads: bool, *, grads=("d_query", "d_cand")):
    """Every comparison of section "the kernel against the references" for one launch, as Measure records; `out`: what the
    kernel (or `model`) wrote, CPU tensors. The limits are helpers.TOL["fp32"]: loss sums and their Mean half at loss_rel,
    statistics at val, gradients whole and per row at grad_l2; counts and selected logits exact."""
    c = inp.case
    N, C = c.N, c.C
    tol = TOL["fp32"]
    res = []
    got = out.losses.double().tolist()
    for i, kind in enumerate(LOSS_KINDS):
        if all_heads or kind == head:
            w = ref.sums[kind]
            res.append(Measure(f"loss {kind}", _finite(abs(got[i] - w) / max(1.0, abs(w))), tol["loss_rel"]))
            wm = w / N
            res.append(Measure(f"loss {kind} Mean", _finite(abs(got[7 + i] - wm) / max(1.0, abs(wm))), tol["loss_rel"]))
        else:
            res.append(Measure(f"loss {kind} is 0", 0.0 if got[i] == 0.0 and got[7 + i] == 0.0 else math.inf, 0.0))
    st = out.stats.double().tolist()
    exact = [("n_valid", float(C)), ("n_query", float(N)), ("neg_distinct", float(C)),
             ("pos_min", _f32(ref.stats["pos_min"])), ("pos_max", _f32(ref.stats["pos_max"]))]
    near = [("pos_mean", ref.stats["pos_mean"]), ("pos_std", ref.stats.get("pos_std"))]
    need_dot = all_heads or head not in COSINE_KINDS
    if need_dot:  # (a lean cosine launch walks no dot logits: its negative statistics describe nothing)
        for name in ("neg_min", "neg_max"):
            w = ref.stats.get(name)
            exact.append((name, None if w is None else _f32(w)))
        if ref.fractional:
            w, g = ref.stats["neg_count"], st[STAT["neg_count"]]
            ok = math.isfinite(g) and round(g) == w
            res.append(Measure("neg_count", _finite(abs(g - w) / max(1.0, w)) if ok else math.inf, tol["val"]))
        else:
            exact.append(("neg_count", ref.stats["neg_count"]))
        near += [(name, ref.stats.get(name)) for name in ("neg_density", "neg_mean", "neg_std")]
    for name, w in exact:
        g = st[STAT[name]]
        same = math.isnan(g) if w is None else g == w
        res.append(Measure(f"stat {name}", 0.0 if same else math.inf, 0.0))
    for name, w in near:
        g = st[STAT[name]]
        if w is None:
            res.append(Measure(f"stat {name} is NaN", 0.0 if math.isnan(g) else math.inf, 0.0))
        else:
            res.append(Measure(f"stat {name}", _finite(abs(g - w) / max(1.0, abs(w))), tol["val"]))
    keep = ~ref.flagged if head in CONTRASTIVE else torch.ones(N, dtype=torch.bool)
    if "d_query" in grads:
        whole, per = _rows_err(out.d_query, ref.d_query[head], keep)
        res += [Measure("d_query whole", whole, tol["grad_l2"]), Measure("d_query per row", per, tol["grad_l2"])]
    if "d_cand" in grads:
        H = c.H
        whole, per = _rows_err(out.d_cand.reshape(N * C, H), ref.d_cand[head].reshape(N * C, H),
                               keep[:, None].expand(N, C).reshape(-1))
        res += [Measure("d_cand whole", whole, tol["grad_l2"]), Measure("d_cand per row", per, tol["grad_l2"])]
    return res


def failures(measures, share: float = 1.0):
    """The records that miss `share` of their limit."""
    return [m for m in measures if not m.err <= share * m.limit]


def launches(name: str):
    """(opt, head, all_heads) of every launch of a case: per option set the seven lean launches and one with every head,
    whose train head walks the seven."""
    for i, opt in enumerate(opts_of(name)):
        for head in LOSS_KINDS:
            yield opt, head, False
        yield opt, LOSS_KINDS[i % 7], True
