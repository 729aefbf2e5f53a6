"""The host model of the two sequence samplers (tests/sampler_model.py) held to what it has to be before a GPU test may lean
on it. CPU only.

1. Every case of tests/sampler_cases.py, and the row sets of tests/test_sampler.py and tests/test_gpu_epoch_loader.py, pass the
   reference's per-row guarantees (``oracle.sampler.check_example``) when the model samples them.
2. The model's two statements of "rank -> item" (set difference, closed form) agree.
3. The model is uniform where the reference is: chi-square tables at fixed seeds over 2e5 draws each -- positions, positives,
   negatives in the three regimes of `rows` and in `xfmr_seq_sample`, and ORDERED PAIRS (neg[0], neg[1]) for the rounds and the
   exact path. Limit: the chi-square 1 - 1e-6 quantile. The same tables reject a deliberately biased variant (a negative rank
   drawn from [0, A - 1)). The statistics are integers in, so they are the same on every machine: profiles/sampler_exact.md
   lists them and the test checks that the listing is current (``pytest -s`` prints the lines anew).
4. Fixture validity: every case is what its name says ("fixture stale" otherwise), the 64-bit halves of seed and epoch reach
   the output, and the pinned tie seeds are what the search finds."""

from __future__ import annotations

import pathlib

import numpy as np
import pytest

import sampler_cases as SC
import sampler_model as SM
from oracle import sampler as OS

ROOT = pathlib.Path(__file__).resolve().parents[1]
PROFILE = ROOT / "profiles" / "sampler_exact.md"
R = 200_000
TABLE_SEED = 20_261_020


# ------------------------------------------------------------------------------------------------ 1. the reference's guarantees
def _check(c_hs, c_ls, rows, out, *, L, width, lookahead, n_items, monkeypatch=None):
    if n_items > 10**6 and monkeypatch is not None:  # check_example builds set(range(1, n_items + 1)): 4 GB at 5e7 items
        from test_gpu_epoch_loader import _lazy_set

        monkeypatch.setattr(OS, "set", _lazy_set, raising=False)
    for b, r in enumerate(rows):
        if out[4][b] is None:
            continue
        OS.check_example(c_hs[r], c_ls[r], out[0][b], out[1][b], out[2][b], max_seq_length=min(L, width),
                         pos_lookahead=lookahead, n_items=n_items)
        assert out[3][b] == min(len(c_hs[r]) - 1, L, width)


@pytest.mark.parametrize("name,kernel", SC.RUNS)
def test_model_keeps_the_reference_guarantees_on_every_case(name, kernel, monkeypatch):
    c = SC.BY_NAME[name]
    out = SC.model(c, kernel)
    rows = [int(c.order[c.first + b]) if c.first + b < len(c.order) else -1 for b in range(c.batch)]
    _check(c.hs, c.ls, rows, out, L=c.L, width=c.width, lookahead=c.lookahead, n_items=c.n_items, monkeypatch=monkeypatch)


@pytest.mark.parametrize("lookahead", [0, 3])
@pytest.mark.parametrize("which", ["test_sampler", "test_gpu_epoch_loader"])
def test_model_keeps_the_reference_guarantees_on_the_existing_row_sets(which, lookahead):
    hs, ls = __import__(which)._rows()
    rows = np.arange(len(hs))
    kw = dict(max_seq_length=32, width=32, lookahead=lookahead, n_items=SC.V)
    for seed in range(3):
        h, p, n, tr = SM.seq_sample(hs, ls, rows, seed, **kw)
        _check(hs, ls, rows, (h, p, n, [t["cnt"] for t in tr], tr), L=32, width=32, lookahead=lookahead, n_items=SC.V)
        _check(hs, ls, rows, SM.rows_sample(hs, ls, rows, len(rows), seed=seed, epoch=seed, **kw), L=32, width=32,
               lookahead=lookahead, n_items=SC.V)


# ------------------------------------------------------------------------------------------------ 2. rank -> item
@pytest.mark.parametrize("n_items,hist", [
    (57, []), (57, [1]), (57, [57]), (57, [1, 2, 3, 55, 56, 57]), (57, list(range(2, 57))), (57, list(range(1, 57))),
    (57, list(range(2, 58))), (57, [0, -3, 58, 7, 7, 9, 1000]), (1000, list(range(1, 1000, 2))), (1000, [500] * 7),
    (12, [12, 1, 6, 6, 5, 7]),
])
def test_the_two_statements_of_rank_to_item_agree(n_items, hist):
    items = SM.history_items(np.asarray(hist, dtype=np.int64), n_items)
    assert items.tolist() == sorted({x for x in hist if 1 <= x <= n_items})
    A = n_items - len(items)
    ranks = np.arange(A)
    a, b = SM.rank_to_item_setdiff(items, n_items, ranks), SM.rank_to_item_closed(items, n_items, ranks)
    assert np.array_equal(a, b) and len(a) == A
    assert a.tolist() == [x for x in range(1, n_items + 1) if x not in set(items.tolist())]


# ------------------------------------------------------------------------------------------------ 3. frequencies
Z6 = 4.753424308822899  # the standard normal 1 - 1e-6 quantile


def chi2_limit(df):
    try:
        from scipy.stats import chi2

        return float(chi2.ppf(1 - 1e-6, df))
    except ImportError:  # Wilson-Hilferty
        return df * (1 - 2 / (9 * df) + Z6 * (2 / (9 * df)) ** 0.5) ** 3


def _chi2(obs, expected):
    obs = np.asarray(obs, dtype=np.float64)
    return float(((obs - expected) ** 2 / expected).sum())


def _stream(kind):
    return SM.SeqStream(TABLE_SEED, np.arange(R)) if kind == "seq" else SM.RowsStream(TABLE_SEED, 3, np.arange(R))


def _sample(kind, h, lab=None, *, L, lookahead=0, n_items, rank_fn=None):
    lab = np.ones(len(h), dtype=bool) if lab is None else lab
    return SM.sample_row(_stream(kind), kind, h, lab, max_seq_length=L, width=L, lookahead=lookahead, n_items=n_items,
                         rank_fn=rank_fn)


def table_positions(kind):
    """13 events, 5 of the 12 positions. A row takes L of m without replacement, so the counts O_i (sum R L) have covariance
    R p (1 - p) m / (m - 1) (I - J / m) with p = L / m: sum (O_i - R p)^2 / (R p) * (m - 1) / (m (1 - p)) is chi-square with
    m - 1 degrees of freedom."""
    m, L = 12, 5
    tr = _sample(kind, np.arange(1, m + 2), L=L, n_items=40)[4]
    pos = tr["positions"]
    assert pos.shape == (R, L) and (np.diff(pos, axis=1) > 0).all()
    p = L / m
    return [(f"positions {kind}", _chi2(np.bincount(pos.ravel(), minlength=m), R * p) * (m - 1) / (m * (1 - p)), m - 1)]


def table_positives(kind):
    """13 events, every position taken, lookahead 4: slot k draws uniformly among its window's c_k candidates, independently of
    the other slots (its own counter): the sum of the slots' statistics is chi-square with sum (c_k - 1) degrees of freedom."""
    n, look = 13, 4
    h = np.array([7, 3, 11, 1, 13, 5, 2, 9, 4, 12, 6, 10, 8])
    lab = np.array([1, 0, 1, 1, 1, 0, 1, 1, 0, 1, 1, 0, 1], dtype=bool)
    pos = _sample(kind, h, lab, L=n - 1, lookahead=look, n_items=40)[1]
    stat = df = 0
    for k in range(n - 1):
        cand = h[[i for i in range(k + 1, min(k + look, n - 1) + 1) if lab[i]]]  # (the window, from its definition)
        counts = np.bincount(pos[:, k], minlength=41)
        assert counts[cand].sum() == R if len(cand) else counts[0] == R
        if len(cand) > 1:
            stat += _chi2(counts[cand], R / len(cand))
            df += len(cand) - 1
    assert df >= 12
    return [(f"positives {kind}", stat, df)]


NEG = {  # regime: history, n_items, L (= cnt), admissible items
    "replace": (np.array([2, 5, 9, 5, 14, 2, 9, 5, 2]), 9, 8),   # items 2 5 9 of 1..9 (14 is no item): A = 6 < cnt = 8
    "rounds": (np.array([2, 5, 9, 5]), 15, 3),                   # A = 12 = 4 cnt
    "exact": (np.array([2, 5, 9, 14, 5]), 14, 4),                # A = 10: cnt <= A < 4 cnt
    "seq": (np.array([2, 5, 9, 12]), 12, 3),                     # xfmr_seq_sample: 8 admissible items, 3 draws
}


def table_negatives(regime, rank_fn=None):
    """Per slot: uniform over the A admissible items (A - 1 degrees of freedom; the with-replacement regime draws its slots
    independently, so they are pooled into one table). Rounds and exact path: (neg[0], neg[1]) uniform over the A (A - 1)
    ordered pairs without repetition."""
    h, n_items, L = NEG[regime]
    kind = "seq" if regime == "seq" else "rows"
    _, _, neg, cnt, tr = _sample(kind, h, L=L, n_items=n_items, rank_fn=rank_fn)
    allowed = np.setdiff1d(np.arange(1, n_items + 1), h)
    A = len(allowed)
    assert cnt == L
    if kind == "rows":
        assert tr["A"] == A and (tr["regime"] == regime).all()
    out = []
    if regime == "replace":
        counts = np.bincount(neg.ravel(), minlength=n_items + 1)
        assert counts.sum() == counts[allowed].sum() == R * cnt
        return [(f"negatives rows {regime}, slots pooled", _chi2(counts[allowed], R * cnt / A), A - 1)]
    assert (np.sort(neg, axis=1)[:, 1:] != np.sort(neg, axis=1)[:, :-1]).all()  # without replacement
    for k in range(cnt):
        counts = np.bincount(neg[:, k], minlength=n_items + 1)
        assert counts.sum() == counts[allowed].sum() == R
        out.append((f"negatives {kind} {regime if kind == 'rows' else ''} slot {k}".replace("  ", " "),
                    _chi2(counts[allowed], R / A), A - 1))
    if kind == "rows":
        rank = np.searchsorted(allowed, neg[:, :2])
        pairs = np.bincount(rank[:, 0] * A + rank[:, 1], minlength=A * A).reshape(A, A)
        assert np.trace(pairs) == 0
        off = pairs[~np.eye(A, dtype=bool)]
        out.append((f"negatives rows {regime} ordered pairs (neg[0], neg[1])", _chi2(off, R / (A * (A - 1))), A * (A - 1) - 1))
    return out


def all_tables():
    rows = []
    for kind in ("seq", "rows"):
        rows += table_positions(kind) + table_positives(kind)
    for regime in NEG:
        rows += table_negatives(regime)
    return rows


def _line(name, stat, df):
    return f"| {name} | {df} | {stat:.2f} | {chi2_limit(df):.2f} |"


@pytest.fixture(scope="module")
def tables():
    return all_tables()


def test_model_is_uniform_where_the_reference_is(tables):
    assert len(tables) == 17
    for name, stat, df in tables:
        print(_line(name, stat, df))
    for name, stat, df in tables:
        assert stat < chi2_limit(df), f"{name}: chi-square {stat:.2f} over the 1 - 1e-6 limit {chi2_limit(df):.2f} ({df} d.f.)"


def test_profile_lists_the_current_statistics(tables):
    text = PROFILE.read_text()
    for name, stat, df in tables:
        want = f"| {name} | {df} | {stat:.2f} | "  # (the limit's digits depend on who computes the quantile)
        assert want in text, f"profiles/sampler_exact.md is stale: no line {_line(name, stat, df)!r}"


def _short_rank(r, A):
    """The biased variant: a rank from [0, A - 1), so the largest admissible item is never drawn."""
    return SM.below(r, A - 1)


@pytest.mark.parametrize("regime", ["replace", "rounds"])
def test_the_tables_reject_a_biased_rank(regime):
    got = table_negatives(regime, rank_fn=_short_rank)
    for name, stat, df in got:
        print("biased:", _line(name, stat, df))
        assert stat > chi2_limit(df), f"{name}: the biased variant passes ({stat:.2f} <= {chi2_limit(df):.2f})"


def test_wilson_hilferty_stands_in_for_scipy():
    """Within 6 % of the exact quantile at the tables' degrees of freedom, and never below it (never the stricter limit)."""
    stats = pytest.importorskip("scipy.stats")
    for df in (4, 11, 89, 131):
        wh = df * (1 - 2 / (9 * df) + Z6 * (2 / (9 * df)) ** 0.5) ** 3
        assert 1 <= wh / stats.chi2.ppf(1 - 1e-6, df) < 1.06


# ------------------------------------------------------------------------------------------------ 4. fixture validity
@pytest.mark.parametrize("name,kernel", SC.RUNS)
def test_case_is_what_it_claims(name, kernel):
    c = SC.BY_NAME[name]
    out = SC.model(c, kernel)
    assert out[0].shape == out[1].shape == out[2].shape == (c.batch, c.width) and out[3].shape == (c.batch,)
    if kernel == "seq":  # (the entry is given no row count and does not check the row index)
        assert all(0 <= r < len(c.hs) for r in c.order)
    if c.valid is not None:
        c.valid(c, kernel, out)


def test_the_table_covers_what_it_has_to():
    names = set(SC.BY_NAME)
    lens = {len(h) for c in SC.CASES if c.name.startswith("lengths-") for h in c.hs}
    assert lens == {1, 2, 33, 34, 64, 65, 255, 256, 257, 300, 513}
    assert {c.lookahead for c in SC.CASES if c.name.startswith("lengths-")} == {0, 1, 3, 10_000}
    assert {f"seed-{s}" for s in (0, 1, 2**32, 2**63 + 5)} | {f"epoch-{e}" for e in (0, 1, 2**32 + 1)} <= names
    big = SC.BY_NAME["longest-row-big-catalogue"]
    assert len(big.hs[0]) == 8192 and big.n_items == 100_003 and big.kernels == SC.BOTH
    for c in SC.CASES:
        if c.name not in ("longest-row-big-catalogue", "huge-catalogue", "tie-exact-path") and not c.name.startswith(
                ("tie-positions", "regime-limits", "rounds-both")):
            assert c.n_items == SC.V, c.name


@pytest.mark.parametrize("kernel", SC.BOTH)
def test_the_high_halves_of_seed_and_epoch_reach_the_output(kernel):
    a, b = (SC.model(SC.BY_NAME[f"seed-{s}"], kernel) for s in (0, 2**32))
    assert any((x != y).any() for x, y in zip(a[:3], b[:3])), "fixture stale: seeds 0 and 2^32 sample the same"
    if kernel == "rows":
        a, b = (SC.model(SC.BY_NAME[f"epoch-{e}"], "rows") for e in (1, 2**32 + 1))
        assert any((x != y).any() for x, y in zip(a[:3], b[:3])), "fixture stale: epochs 1 and 2^32 + 1 sample the same"


def test_identity_cases_hold_one_row_in_two_slots_and_at_two_offsets():
    two, off = SC.BY_NAME["identity-two-slots"], SC.BY_NAME["identity-other-first"]
    assert (two.order[[0, 2, 4]] == 9).all() and off.rows[1] == 9 and off.first > 0
    a, b = SC.model(two, "rows"), SC.model(off, "rows")
    for x, y in zip(a[:4], b[:4]):
        assert (x[0] == x[2]).all() and (x[0] == x[4]).all() and (x[0] == y[1]).all()
    assert a[3][0] == 32 and (a[2][0] != 0).all()


def test_pinned_tie_seeds_are_what_the_search_finds():
    """The search, re-run from a little below each pinned seed (the whole search from seed 0 takes ten seconds)."""
    for kind in SC.BOTH:
        seed, i, j = SC.POS_TIE[kind]
        got = SC.find_key_tie(kind, SM.P_POSITIONS, range(seed - 3, seed + 1), 700, lambda i, j, k: k + 1 < j + 1)
        assert got == (seed, i, j)
    seed, i, j = SC.EXACT_TIE
    got = SC.find_key_tie("rows", SM.P_EXACT, range(seed - 3, seed + 1), 700, lambda i, j, k: k + 1 <= j + 1 < 4 * (k + 1))
    assert got == (seed, i, j)

