"""Host reference and cases for xfmr_candidate_ranks (TEST INFRASTRUCTURE): a target's rank among a GIVEN candidate list.

``rank_among_ref`` restates the entry's definition on one query's score vector: the items of the query are S =
distinct(candidates U targets) restricted to the eligible items (``1 <= j < n_rows``, not excluded, finite score), and
``rank(t) = 1 + |{c in S, c != t, c beats t}|`` (higher score first, then the lower index). It compares the scores it is
given and does no arithmetic on them, so it is exact for any scores: numpy's for the dot and l2 metrics on the cases
below (entries are small integers: every fp32 dot product is exact in any summation order and ties are real), the
device's own for cosine.

``cases()`` sits at the edges where a kernel can go wrong: list lengths around the 64-lane wave and the 256-place batch, a
20 000-candidate list (split over the grid), 130 targets (two target chunks) with repeats, a target inside its own
candidate list, duplicate candidates, ids 0 / negative / >= n_rows, excluded candidates and an excluded target, a table
row holding inf, and score ties between a target and candidates of lower and higher index."""

from __future__ import annotations

import dataclasses
import functools

import numpy as np

import rank_refs as R

RANK_NONE = R.RANK_NONE
LIST_SIZES = (63, 0, 1, 64, 65, 100, 1000)
TARGET_COUNTS = (1, 3, 0, 130)
LONG_LIST = 20_000
TIE_LOW, TIE_TARGET, TIE_HIGH = 10, 30, 50  # three equal table rows (cases with n_rows >= 65)


def eligible_mask(s, exclude):
    """The eligible table rows given one query's score vector."""
    s = np.asarray(s, dtype=np.float64)
    ok = np.isfinite(s)
    ok[0] = False
    for x in exclude or ():
        if 0 <= int(x) < s.size:
            ok[int(x)] = False
    return ok


def rank_among_ref(s, candidates, exclude, targets):
    """One query. ``s``: its score per table row; ``candidates`` / ``exclude`` / ``targets``: any ints, repeats allowed.
    Returns ``(ranks, target_scores, candidate_scores)`` parallel to ``targets``, ``targets`` and ``candidates``:
    RANK_NONE / -inf for an item that is not eligible."""
    s = np.asarray(s, dtype=np.float64)
    n = s.size
    ok = eligible_mask(s, exclude)

    def elig(j):
        return 0 <= int(j) < n and bool(ok[int(j)])

    items = np.asarray(sorted({int(c) for c in candidates if elig(c)} | {int(t) for t in targets if elig(t)}), dtype=np.int64)
    si = s[items] if items.size else np.zeros(0)
    ranks = []
    for t in targets:
        if not elig(t):
            ranks.append(RANK_NONE)
            continue
        st = s[int(t)]
        ranks.append(1 + int(np.count_nonzero((si > st) | ((si == st) & (items < int(t))))))
    tscore = [float(s[int(t)]) if elig(t) else -np.inf for t in targets]
    cscore = [float(s[int(c)]) if elig(c) else -np.inf for c in candidates]
    return ranks, tscore, cscore


@dataclasses.dataclass
class Case:
    name: str
    table: np.ndarray   # (n_rows, H) float32, integer-valued (one row may hold an inf)
    query: np.ndarray   # (n_query, H) float32, integer-valued
    cand: list          # per query: the candidate list, SORTED ascending (repeats and bad ids included)
    excl: list          # per query: the exclusion list, sorted ascending
    tgts: list          # per query: the target entries, in any order
    inf_row: int | None

    @property
    def shape(self):
        return self.query.shape[0], self.table.shape[0], self.table.shape[1]


def _case(name, n_query, n_rows, H, seed, long_query=None):
    rng = np.random.default_rng(seed)
    table = rng.integers(-3, 4, (n_rows, H)).astype(np.float32)
    for _ in range(n_rows // 6):  # equal rows: tied scores
        table[int(rng.integers(1, n_rows))] = table[int(rng.integers(1, n_rows))]
    inf_row = None
    if n_rows >= 65:
        table[TIE_LOW] = table[TIE_HIGH] = table[TIE_TARGET]
        inf_row = 40
        table[inf_row, int(rng.integers(0, H))] = np.inf
    query = rng.integers(-3, 4, (n_query, H)).astype(np.float32)
    cand, excl, tgts = [], [], []
    for b in range(n_query):
        size = LONG_LIST if b == long_query else LIST_SIZES[b % len(LIST_SIZES)]
        c = rng.integers(1, n_rows, size)  # (more entries than rows: repeats)
        n_t = TARGET_COUNTS[b % len(TARGET_COUNTS)]
        t = rng.integers(1, n_rows, n_t).tolist()
        if n_t >= 3:
            t[2] = t[0]  # a repeated target
        if n_t >= 130:
            t[100:110] = t[:10]
            t[7] = 0  # the padding row as a target
            t[8] = n_rows + 2  # past the table
        if n_t and c.size and b % 2 == 0:
            c[0] = t[0]  # a target inside its own candidate list
        extra = []
        if b % 3 == 0:
            extra += [0, -1, -5, n_rows, n_rows + 7]  # ids that are no item
        if c.size >= 2 and b % 3 == 1:
            extra += [int(c[0]), int(c[0]), int(c[1])]  # duplicate candidates
        if inf_row is not None and b % 5 == 0:
            extra.append(inf_row)
            if n_t:
                t.append(inf_row)  # a target with a non-finite score
        if b == 0 and n_rows >= 65:
            t[0] = TIE_TARGET  # ties with a candidate of lower and of higher index
            extra += [TIE_LOW, TIE_HIGH]
        c = np.sort(np.concatenate([c, np.asarray(extra, dtype=np.int64)]))
        ex = rng.integers(1, n_rows + 2, int(rng.integers(0, 8))).tolist()
        if c.size >= 3 and b % 2 == 1:
            ex += [int(c[c.size // 2]), int(c[-1])]  # excluded candidates
        if n_t >= 2 and b % 4 == 1:
            ex.append(int(t[1]))  # an excluded target
        cand.append(c.astype(np.int64).tolist())
        excl.append(sorted(ex))
        tgts.append([int(x) for x in t])
    return Case(name, table, query, cand, excl, tgts, inf_row)


@functools.lru_cache(maxsize=None)
def cases():
    """The cases, built once: (n_query, n_rows, H) over H in {4, 8, 36, 384, 1024}, n_rows in {2, 65, 4 097} and n_query in
    {1, 33, 257}; the largest holds the 20 000-candidate list, on a query with 130 targets."""
    return (
        _case("one-item", 1, 2, 4, 1),
        _case("one-query", 1, 65, 8, 2),
        _case("wave-edges", 33, 65, 36, 3),
        _case("widest-rows", 33, 65, 1024, 4),
        _case("many-queries", 257, 4097, 384, 5, long_query=3),
    )


def score_vector(case: Case, b: int, metric: str) -> np.ndarray:
    """Query b's exact scores over the table (dot and l2: every value is an integer below 2^24, or not finite)."""
    return R.scores(case.query[b], case.table, metric)


@functools.lru_cache(maxsize=None)
def expected(name: str, metric: str):
    """``rank_among_ref`` over a case's queries, flat in CSR order: ``(ranks int64, target scores, candidate scores)``.
    Computed once per (case, metric) and shared; for the dot and l2 metrics only (cosine scores are not exact)."""
    assert metric in ("dot", "l2")
    case = {c.name: c for c in cases()}[name]
    ranks, ts, cs = [], [], []
    for b in range(case.query.shape[0]):
        r, t, c = rank_among_ref(score_vector(case, b, metric), case.cand[b], case.excl[b], case.tgts[b])
        ranks += r
        ts += t
        cs += c
    return np.asarray(ranks, dtype=np.int64), np.asarray(ts, dtype=np.float64), np.asarray(cs, dtype=np.float64)


def csr(lists, lead: int = 0, fill: int = -99):
    """Lists -> ``(flat int64, offsets int64)`` with ``lead`` unrelated entries in front (the first offset is ``lead``, not
    0) and one behind, so that the CSR is a view into a longer array."""
    off = np.full(len(lists) + 1, lead, dtype=np.int64)
    off[1:] += np.cumsum([len(x) for x in lists])
    flat = np.concatenate([np.full(lead, fill, dtype=np.int64)] + [np.asarray(x, dtype=np.int64).reshape(-1) for x in lists]
                          + [np.full(1, fill, dtype=np.int64)])
    return flat, off
