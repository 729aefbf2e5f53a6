"""A host model of the refined item search (xfmr_search_refined: coarse bf16 pass, exact f32 refine, certificate) in
torch on the CPU, the named cases the host and the GPU tests share, and the plausible wrong implementations that the
cases must tell from the right one.

The model is a model of the RULES, not of the hardware's summation order: a score is ``rk_score`` on an f32 matmul,
the coarse one on operands rounded by ``.to(torch.bfloat16)``. What it pins down:
  eligible     1 <= j < n_rows and j not in the query's exclusion list;
  order        higher score first, then lower index (tt_better); non-finite scores never enter a list;
  shortlist    the k_short = max(top_k, min(top_k * refine_factor, 128)) best eligible coarse pairs;
  tau          the shortlist's last coarse score when it is full, -inf when every eligible item was kept;
  refine       exact scores of the kept items, non-finite ones dropped, best top_k, padded with -1 / -inf;
  certified    no non-finite coarse score in the row AND (shortlist not full OR k-th refined score > tau + bound).
``bound`` is DESIGN.md "Refined search" in f32, the operations in csrc/search.hip's order (sr_bound).
"""

import math

import torch

COSINE, DOT, L2 = 0, 1, 2
METRIC_NAMES = {COSINE: "cosine", DOT: "dot", L2: "l2"}
K_SHORT_MAX = 128
BETA = 2.0 ** -7 + 2.0 ** -12
INFL = 1.0 + 2.0 ** -9
DELTA = 2.0 ** -60
ULPS = 2.0 ** -20
NORM_MAX = 2.0 ** 40
U = 2.0 ** -7  # the spacing of bf16 at 1.0: the unit of the rounding adversary

# the plausible wrong implementations (`wrong=` of model_search); each must fail on at least one case
WRONG = ("bound_zero", "dot_bound_without_item_norm", "l2_bound_not_doubled", "tau_at_top_k", "greater_or_equal",
         "ties_by_higher_index", "excluded_kept_until_refine", "padding_row_eligible")


def k_short_of(top_k, refine_factor):
    return max(top_k, min(top_k * refine_factor, K_SHORT_MAX))


def f32(x):
    return torch.tensor(x, dtype=torch.float32)


def table_terms(table):
    """(rnorm, sqnorm) as the library makes them up to summation order: 1 / max(|e|, 1e-8) and |e|^2, in f32."""
    sq = (table * table).sum(-1)
    return 1.0 / sq.sqrt().clamp(min=1e-8), sq


def norm_bounds(table):
    """(largest row norm, largest inverse row norm) over rows 1.., rounded up by 2^-12: ExactItemIndex.norm_bounds."""
    if table.shape[0] < 2:
        return 0.0, 0.0
    rn, sq = table_terms(table)
    return float(sq[1:].max().sqrt().double() * (1 + 2.0 ** -12)), float(rn[1:].max().double() * (1 + 2.0 ** -12))


def scores(q, table, metric, coarse=False):
    """(B, V) f32 scores = 1 - distance; coarse: the dot products on bf16-rounded operands, everything else as exact."""
    rn, ee = table_terms(table)
    qq = (q * q).sum(-1, keepdim=True)
    rq = 1.0 / qq.sqrt().clamp(min=1e-8)
    if coarse:
        dot = q.to(torch.bfloat16).float() @ table.to(torch.bfloat16).float().T
    else:
        dot = q @ table.T
    if metric == COSINE:
        return dot * rq * rn
    if metric == DOT:
        return dot
    return 1.0 - (qq - 2.0 * dot + ee)


def bound(metric, qq, max_norm, max_rnorm, wrong=None):
    """sr_bound of csrc/search.hip, f32 operation by operation; qq: () f32 tensor."""
    if wrong == "bound_zero":
        return f32(0.0)
    nq = qq.sqrt()
    M, R = f32(max_norm), f32(max_rnorm)
    ok = bool(qq > 0) and bool(nq <= NORM_MAX) and bool(M >= 0) and bool(M <= NORM_MAX) and bool(R >= 0) and bool(R < math.inf)
    if not ok:
        return f32(math.inf)
    c = f32(BETA) * f32(INFL)
    d = c * nq * (f32(1.0) if wrong == "dot_bound_without_item_norm" else M) + f32(DELTA)
    if metric == DOT:
        return d
    if metric == L2:
        two = f32(1.0) if wrong == "l2_bound_not_doubled" else f32(2.0)
        return two * d + f32(ULPS) * ((nq + M) * (nq + M) + f32(1.0))
    return c + f32(ULPS) + f32(DELTA) * (f32(1.0) / nq.clamp(min=1e-8)) * R * f32(INFL)


def ranked(score_row, candidates, higher_index=False):
    """The candidates (an ascending int64 tensor of item indices) with a finite score, best first: score descending,
    then index ascending (a stable sort of the ascending candidates). Returns a list."""
    c = candidates.flip(0) if higher_index else candidates
    s = score_row[c]
    fin = torch.isfinite(s)
    c, s = c[fin], s[fin]
    return c[torch.sort(s, descending=True, stable=True).indices].tolist()


def eligible(V, ex, first=1):
    """Ascending tensor of the items first .. V - 1 that are not in the set ex."""
    mask = torch.ones(V, dtype=torch.bool)
    mask[:first] = False
    inside = [j for j in ex if 0 <= j < V]
    if inside:
        mask[torch.tensor(inside, dtype=torch.int64)] = False
    return mask.nonzero().flatten()


def exact_search(q, table, excl, top_k, metric):
    """The exact search of the model: (idx (B, top_k) int64 -1 padded, score (B, top_k) -inf padded)."""
    B, V = q.shape[0], table.shape[0]
    s = scores(q, table, metric)
    idx = torch.full((B, top_k), -1, dtype=torch.int64)
    sc = torch.full((B, top_k), -math.inf, dtype=torch.float32)
    for b in range(B):
        ex = set(excl[b]) if excl is not None else set()
        top = ranked(s[b], eligible(V, ex))[:top_k]
        idx[b, :len(top)] = torch.tensor(top, dtype=torch.int64)
        sc[b, :len(top)] = s[b, top]
    return idx, sc


def model_search(q, table, excl, top_k, refine_factor, metric, max_norm=None, max_rnorm=None, wrong=None):
    """The three stages. Returns a dict: idx, score (as exact_search), certified (B,) bool, shortlist (list of lists, best
    coarse first), tau, bound, margin (k-th refined score - tau; what the certificate compares with the bound)."""
    B, V = q.shape[0], table.shape[0]
    ks = k_short_of(top_k, refine_factor)
    mn, mr = norm_bounds(table)
    max_norm = mn if max_norm is None else max_norm
    max_rnorm = mr if max_rnorm is None else max_rnorm
    sx, sc = scores(q, table, metric), scores(q, table, metric, coarse=True)
    qq = (q * q).sum(-1)
    hi = wrong == "ties_by_higher_index"
    out = dict(idx=torch.full((B, top_k), -1, dtype=torch.int64), score=torch.full((B, top_k), -math.inf),
               certified=torch.zeros(B, dtype=torch.bool), shortlist=[], tau=[], bound=[], margin=[])
    for b in range(B):
        ex = set(excl[b]) if excl is not None else set()
        first = 0 if wrong == "padding_row_eligible" else 1
        elig = eligible(V, set() if wrong == "excluded_kept_until_refine" else ex, first)
        bad = not bool(torch.isfinite(sc[b, first:]).all())
        short = ranked(sc[b], elig, hi)[:ks]
        full = len(short) == ks
        at = top_k if wrong == "tau_at_top_k" else ks
        tau = float(sc[b, short[at - 1]]) if full else -math.inf
        kept = [j for j in short if j not in ex]
        top = ranked(sx[b], torch.tensor(sorted(kept), dtype=torch.int64), hi)[:top_k]
        out["idx"][b, :len(top)] = torch.tensor(top, dtype=torch.int64)
        out["score"][b, :len(top)] = sx[b, top]
        sk = sx[b, top[top_k - 1]] if len(top) == top_k else f32(-math.inf)
        bd = bound(metric, qq[b], max_norm, max_rnorm, wrong)
        rhs = f32(tau) + bd
        proven = (not full) or bool(sk >= rhs if wrong == "greater_or_equal" else sk > rhs)
        out["certified"][b] = (not bad) and proven
        out["shortlist"].append(short)
        out["tau"].append(tau)
        out["bound"].append(float(bd))
        out["margin"].append(float(sk) - tau)
    return out


def contract_problems(case, got, want=None):
    """What is wrong with a result `got` (dict with idx, score, certified) for `case`, as text; empty when it keeps the
    contract: a certified row is the exact search's row bit for bit; every row is a valid list (no padding row, no
    excluded item, no duplicate, every score the exact score of its item, sorted by tt_better, padding only at the end);
    and the case's own expectation of the certificate holds."""
    q, table, excl, top_k, metric = case["q"], case["table"], case["excl"], case["top_k"], case["metric"]
    want = exact_search(q, table, excl, top_k, metric) if want is None else want
    sx = scores(q, table, metric)
    bad = []
    for b in range(q.shape[0]):
        idx, sc = got["idx"][b], got["score"][b]
        if bool(got["certified"][b]) and not (torch.equal(idx, want[0][b]) and torch.equal(sc, want[1][b])):
            bad.append(f"row {b}: certified but not the exact row")
        ex = set(excl[b]) if excl is not None else set()
        items = [int(j) for j in idx if j >= 0]
        n = len(items)
        if any(int(j) >= 0 for j in idx[n:]) or not bool((sc[n:] == -math.inf).all()):
            bad.append(f"row {b}: padding inside the list")
        if any(j < 1 or j >= table.shape[0] or j in ex for j in items) or len(set(items)) != n:
            bad.append(f"row {b}: an item that is not eligible, or a repeat")
        elif not torch.equal(sc[:n], sx[b, items]):
            bad.append(f"row {b}: a score that is not the exact score of its item")
        elif any(not (float(sc[i]) > float(sc[i + 1]) or (float(sc[i]) == float(sc[i + 1]) and items[i] < items[i + 1]))
                 for i in range(n - 1)):
            bad.append(f"row {b}: not sorted by tt_better")
    if case["expect"] == "all" and not bool(got["certified"].all()):
        bad.append("a row that must be certified is not")
    if case["expect"] == "none" and bool(got["certified"].any()):
        bad.append("a row that must stay uncertified is certified")
    return bad


# ---------------------------------------------------------------------------------------------- the cases
def case(name, q, table, top_k, refine_factor, metric, excl=None, expect=None, **extra):
    """expect: "all" (every row must be certified), "none" (no row may be) or None (soundness only)."""
    return dict(name=name, q=q.float().contiguous(), table=table.float().contiguous(), top_k=top_k,
                refine_factor=refine_factor, metric=metric, excl=excl, expect=expect, **extra)


def unit_gaussian(V, H, B, seed):
    g = torch.Generator().manual_seed(seed)
    table = torch.randn(V + 1, H, generator=g)
    table = table / table.norm(dim=-1, keepdim=True)
    table[0] = 0
    q = torch.randn(B, H, generator=g)
    return q / q.norm(dim=-1, keepdim=True), table


def adversary(metric, scale=1.0, q_off_grid=False):
    """The rounding adversary: H = 32, q = c * ones (c = 1; 2 under l2, where a query of ones makes the score second order
    in the items' deviations), eight decoys whose bf16 rounding GAINS coarse score (half the components 1 + 0.51 u
    round up, half 1 + 0.495 u round down) and one true best whose rounding LOSES it (a quarter 1 + 1.499 u, the rest 1 +
    0.499 u, all rounded down); k_short = 4, top_k = 1. The shortlist is four decoys; the true best is not in it.
    `scale` multiplies the items (a power of two: the roundings scale with it). q_off_grid: the query's components are c *
    (1 + 0.499 u), rounded down too."""
    H = 32
    c = 2.0 if metric == L2 else 1.0
    q = torch.full((1, H), c * (1 + 0.499 * U if q_off_grid else 1.0), dtype=torch.float64)
    decoy = torch.tensor([1 + 0.51 * U] * 16 + [1 + 0.495 * U] * 16, dtype=torch.float64)
    best = torch.tensor([1 + 1.499 * U] * 8 + [1 + 0.499 * U] * 24, dtype=torch.float64)
    table = torch.stack([torch.zeros(H, dtype=torch.float64)] + [decoy] * 8 + [best]) * scale
    if metric == COSINE:
        # A cosine against ones is second order in the deviations too. Eight more dimensions hold a ballast of 4 in every
        # item (on the bf16 grid: no rounding) and 0 in the query: the items' norms hardly differ, the cosine follows
        # the dot product.
        q = torch.cat([q, torch.zeros(1, 8, dtype=torch.float64)], dim=1)
        table = torch.cat([table, torch.full((10, 8), 4.0 * scale, dtype=torch.float64)], dim=1)
        table[0] = 0
    return case(f"adversary_{METRIC_NAMES[metric]}_x{scale:g}{'_q' if q_off_grid else ''}", q, table, 1, 4, metric,
                expect="none", true_best=9)


def l2_half_bound_adversary():
    """Under l2 the score moves by TWICE the dot product's error. Query 2 (1 + 0.499 u) * ones and items whose components
    are 1 + (m + 0.499) u all round down: the dot product loses almost the whole of its bound. The true best x loses it on
    every component; the champion c of the shortlist only on half of them (the others sit on the bf16 grid), and starts
    just far enough ahead in coarse score to be kept while x is not. Between c's exact score and x's lies more than the
    dot product's bound: a rule that forgets the factor two certifies c."""
    H = 32
    q = torch.full((1, H), 2 * (1 + 0.499 * U), dtype=torch.float64)
    x = torch.tensor([1 + 0.499 * U] * H, dtype=torch.float64)
    c = torch.tensor([1 + 1.0 * U] * 2 + [1.0] * 14 + [1 + 0.499 * U] * 16, dtype=torch.float64)
    filler = torch.tensor([1 + 1.0 * U] * 1 + [1.0] * 31, dtype=torch.float64)
    table = torch.stack([torch.zeros(H, dtype=torch.float64), c, filler, filler, filler, x])
    return case("adversary_l2_half_bound", q, table, 1, 4, L2, expect="none", true_best=5)


def equality_case():
    """k-th refined score == tau + bound exactly (dot, q = e0, the table's norm bound given as 1): the rule says strictly
    greater, so the row is not certified. Item 1 scores fl(0.5 + bound) exactly and 0.5078125 coarsely; item 2 is tau."""
    H = 8
    q = torch.zeros(1, H)
    q[0, 0] = 1.0
    b = bound(DOT, f32(1.0), 1.0, 1.0)
    table = torch.zeros(6, H)
    table[1, 0] = f32(0.5) + b
    table[2, 0] = 0.5
    table[3, 0], table[4, 0], table[5, 0] = 0.25, 0.125, 0.0625
    return case("equality", q, table, 1, 2, DOT, expect="none", max_norm=1.0, max_rnorm=1.0)


def dyadic(V, H, B, seed):
    """Small dyadic values (multiples of 1/4 in [-2, 2]): every bf16 product and every partial sum is exact in f32 in any
    order, so the coarse scores under the dot metric are the same bits on every machine."""
    g = torch.Generator().manual_seed(seed)
    table = torch.randint(-8, 9, (V + 1, H), generator=g).float() / 4
    table[0] = 0
    return torch.randint(-8, 9, (B, H), generator=g).float() / 4, table


def host_cases():
    """Every named case; the GPU test runs them all too (they are small)."""
    out = []
    q, table = unit_gaussian(4000, 64, 256, 0)
    out.append(case("gaussian", q, table, 10, 4, COSINE, expect="all"))
    s = scores(q[:32], table, COSINE)
    s[:, 0] = -math.inf
    top20 = [sorted(int(j) for j in row.topk(20).indices) for row in s]
    out.append(case("gaussian_top_excluded", q[:32], table, 5, 8, COSINE, excl=top20, expect="all"))
    for metric in (COSINE, DOT, L2):
        out.append(adversary(metric))
    out.append(adversary(DOT, scale=128.0))
    out.append(l2_half_bound_adversary())
    out.append(equality_case())
    # ties: duplicate rows straddling place k_short (items 1 .. 12 are one vector, k_short = 8)
    q, table = unit_gaussian(40, 16, 3, 1)
    table[1:13] = table[1]
    q[0] = table[1]
    for metric in (COSINE, DOT, L2):
        out.append(case(f"duplicates_{METRIC_NAMES[metric]}", q[:1], table, 4, 2, metric, expect="none"))
    # ... and with every eligible item kept: the order among equals is the only thing left to get wrong
    out.append(case("duplicates_all_kept", q[:1], table[:14], 4, 8, COSINE, expect="all"))
    q, table = unit_gaussian(300, 16, 3, 2)
    out.append(case("zero_query", torch.zeros(1, 16), table, 5, 4, COSINE, expect="none"))
    bad_q = q.clone()
    bad_q[0, 3], bad_q[1, 5] = math.inf, math.nan
    out.append(case("nonfinite_query", bad_q[:2], table, 5, 4, COSINE, expect="none"))
    # the padding row holds the query itself: it must not be returned
    pad = table.clone()
    pad[0] = q[2]
    out.append(case("padding_row_best", q[2:3], pad, 5, 4, COSINE))
    # exclusions that leave fewer than top_k items, and fewer eligible items than k_short
    q, table = unit_gaussian(30, 24, 2, 3)
    out.append(case("few_left", q, table, 5, 4, DOT, excl=[list(range(1, 28)), list(range(4, 31))], expect="all"))
    out.append(case("fewer_than_k_short", q, table, 10, 4, L2, expect="all"))
    return out
