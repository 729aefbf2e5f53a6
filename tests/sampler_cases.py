"""The case table of tests/test_gpu_sampler_exact.py, and the host model's answer to each case.

A case is ONE launch of ``xfmr_seq_sample`` ("seq") and / or ``xfmr_seq_sample_rows`` ("rows") over a few dataset rows.
tests/test_sampler_model_host.py proves on the CPU, from the model's trace and the inputs, that every case is what its name
says (``Case.valid``; a failure reads "fixture stale": the hash or the model moved and the case no longer reaches its
branch); the GPU test compares the launch with the model, array for array. Seeds that were searched for (threshold ties, the
rounds case, the walk-forward) are pinned here as constants; ``find_key_tie`` is the search that found them."""

from __future__ import annotations

import dataclasses
import functools

import numpy as np

import sampler_model as SM
from test_gpu_epoch_loader import _crowded, _labels

V = 57
LENS = (1, 2, 33, 34, 64, 65, 255, 256, 257, 300, 513)
SEEDS = (0, 1, 2**32, 2**63 + 5)
EPOCHS = (0, 1, 2**32 + 1)
BOTH = ("seq", "rows")

# (seed, i, j): positions i < j of dataset row 0 carry the same purpose-1 key, found by find_key_tie over seeds 0..;
# the row has j + 2 events and max_seq_length = width = #{keys below the tied key among 0..j} + 1: one of the pair is taken
POS_TIE = {"seq": (4859, 252, 670), "rows": (47734, 331, 672)}
# (seed, i, j): ranks i < j of dataset row 0 carry the same purpose-4 key; A = j + 1, cnt = #{keys below} + 1, cnt <= A < 4 cnt
EXACT_TIE = (16220, 294, 396)
ROUNDS_SEED = 0      # cnt = 32, A = 128: at least two rounds, rejections by a filled slot AND by a lower open slot
WALK_SEED = 0        # one admissible item left of 57: some slot of xfmr_seq_sample is rejected 65 times and walks forward


@dataclasses.dataclass
class Case:
    name: str
    kernels: tuple
    hs: list
    ls: list
    n_items: int
    L: int
    lookahead: int
    order: np.ndarray
    batch: int
    width: int
    first: int = 0
    seed: int = 0
    epoch: int = 0
    max_history: int | None = None   # None = the dataset's longest row
    valid: object = None             # valid(case, kernel, model output): asserts that the case is what it claims

    def __post_init__(self):
        self.order = np.asarray(self.order, dtype=np.int64)

    @property
    def rows(self):
        """The dataset rows of the batch (seq: the whole order, all of them inside the dataset)."""
        return self.order[self.first : self.first + self.batch]


def model(case: Case, kernel: str):
    """hist, pos, neg, len, traces of the case on ``kernel`` (len: the model's cnt per row for seq too)."""
    return _model(case.name, kernel)


@functools.lru_cache(maxsize=None)
def _model(name, kernel):
    c = BY_NAME[name]
    kw = dict(max_seq_length=c.L, width=c.width, lookahead=c.lookahead, n_items=c.n_items)
    if kernel == "rows":
        out = SM.rows_sample(c.hs, c.ls, c.order, c.batch, first=c.first, seed=c.seed, epoch=c.epoch,
                             max_history=c.max_history, **kw)
    else:
        assert c.first == 0 and c.batch == len(c.order)
        assert all(0 <= r < len(c.hs) for r in c.order)
        h, p, n, tr = SM.seq_sample(c.hs, c.ls, c.order, c.seed, max_history=c.max_history, **kw)
        out = (h, p, n, np.array([0 if t is None else t["cnt"] for t in tr], dtype=np.int32), tr)
    for a in out[:4]:
        a.setflags(write=False)
    return out


# ----------------------------------------------------------------------------------------------------- searches (CPU)
def find_key_tie(kind, purpose, seeds, max_m, accept=lambda i, j, below_k: True):
    """The first seed of ``seeds`` for which two counters i < j < max_m of dataset row 0's stream (epoch 0) carry the same
    ``purpose`` key and ``accept(i, j, #{keys below it among 0..j})`` holds: (seed, i, j)."""
    for seed in seeds:
        s = SM.SeqStream(seed, 0) if kind == "seq" else SM.RowsStream(seed, 0, 0)
        k = s.draw(purpose, np.arange(max_m))[0]
        o = np.argsort(k, kind="stable")
        for t in np.flatnonzero(k[o][1:] == k[o][:-1]):
            i, j = int(o[t]), int(o[t + 1])
            if accept(i, j, int((k[: j + 1] < k[i]).sum())):
                return seed, i, j
    return None


def tie_width(kind, purpose, seed, i, j):
    s = SM.SeqStream(seed, 0) if kind == "seq" else SM.RowsStream(seed, 0, 0)
    k = s.draw(purpose, np.arange(j + 1))[0]
    assert k[i] == k[j] and (k == k[i]).sum() == 2, "fixture stale: the pinned pair no longer ties"
    return int((k < k[i]).sum()) + 1


# ----------------------------------------------------------------------------------------------------- validity checks
def _windows(c, kernel, out):
    """Some slot has its window cut by the row's end, some slot has no candidate and returns 0, some slot has a positive
    right behind its window (at p + lookahead + 1) that it must not take."""
    cut = empty = behind = 0
    for b, r in enumerate(c.rows):
        tr, lab, n = out[4][b], np.asarray(c.ls[r]).astype(bool), len(c.hs[r])
        for k, p in enumerate(tr["positions"]):
            cut += p + c.lookahead > n - 1
            none = len(SM.candidates(lab, int(p), c.lookahead)) == 0
            empty += none
            assert not none or out[1][b, k] == 0
            behind += p + c.lookahead + 1 <= n - 1 and bool(lab[p + c.lookahead + 1])
    assert cut and empty and behind, f"fixture stale: {c.name} windows cut {cut}, empty {empty}, positive behind {behind}"


def _regimes(want):
    def valid(c, kernel, out):
        if kernel != "rows":  # (xfmr_seq_sample has no regimes of this kind; its trace says whether a slot walked)
            return
        got = [(t["A"], t["regime"], t["cnt"]) for t in out[4]]
        assert got == want, f"fixture stale: {c.name}: (A, regime, cnt) per row {got}, built for {want}"
    return valid


def _pos_tie(kernel_of_case):
    def valid(c, kernel, out):
        _, i, j = POS_TIE[kernel_of_case]
        t = out[4][0]
        assert kernel == kernel_of_case
        assert (t["pos_tie_took"], t["pos_tie_left"]) == (i, j), f"fixture stale: {c.name}: no tie at the threshold"
        assert i in t["positions"] and j not in t["positions"]
    return valid


def _exact_tie(c, kernel, out):
    _, i, j = EXACT_TIE
    t = out[4][0]
    assert t["regime"] == SM.EXACT and t["A"] == j + 1 and t["cnt"] <= t["A"] < 4 * t["cnt"], f"fixture stale: {c.name}"
    assert (t["neg_tie_took"], t["neg_tie_left"]) == (i, j), f"fixture stale: {c.name}: no tie at the threshold"
    items = SM.history_items(c.hs[0], c.n_items)
    assert SM.rank_to_item(items, c.n_items, i) == out[2][0, t["cnt"] - 1]  # the lower rank, as the last of the key order
    assert SM.rank_to_item(items, c.n_items, j) not in out[2][0]


def _rounds_both(c, kernel, out):
    if kernel == "rows":
        t = out[4][0]
        assert t["regime"] == SM.ROUNDS and t["cnt"] == 32 and t["A"] == 128
        assert t["rounds"] >= 2 and t["rejected_by_filled"] > 0 and t["rejected_by_lower"] > 0, \
            f"fixture stale: {c.name}: rounds {t['rounds']}, by filled {t['rejected_by_filled']}, by lower {t['rejected_by_lower']}"
        # round 0 from its definition (nothing is filled yet): of the slots that draw one rank, the lowest keeps it
        r = int(c.rows[0])
        d = SM.below(SM.RowsStream(c.seed, c.epoch, r).draw(SM.P_ROUND0, np.arange(32))[0], 128)
        ranks = np.searchsorted(np.setdiff1d(np.arange(1, c.n_items + 1), c.hs[r]), out[2][0])
        groups = [np.flatnonzero(d == v) for v in np.unique(d)]
        assert max(len(g) for g in groups) > 1
        for g in groups:
            assert ranks[g[0]] == d[g[0]] and (ranks[g[1:]] != d[g[0]]).all(), f"{c.name}: the lower slot keeps the rank"


def _walk(c, kernel, out):
    assert V - len(SM.history_items(c.hs[0], V)) == 1
    if kernel == "seq":
        assert out[4][0]["walked"] > 0, f"fixture stale: {c.name}: the walk-forward did not run"


def _zero_rows(zero):
    def valid(c, kernel, out):
        got = [t is None for t in out[4]]
        assert got == zero, f"fixture stale: {c.name}"
        for b, z in enumerate(zero):
            if z:
                assert all((a[b] == 0).all() for a in out[:4])
            else:
                assert out[3][b] > 0
    return valid


def _width_below(c, kernel, out):
    assert c.width < c.L and any(len(c.hs[r]) - 1 > c.width for r in c.rows) and out[3].max() == c.width


def _width_above(c, kernel, out):
    assert c.width > c.L and out[3].max() < c.width and (out[0][:, c.L :] == 0).all()


def _closed_form(c, kernel, out):
    assert c.n_items > SM.SETDIFF_LIMIT and out[2].max() > 2**24, f"fixture stale: {c.name}"


# ----------------------------------------------------------------------------------------------------- the table
def _distinct_row(rng, n_distinct, n_items, n, extra=()):
    """n events over exactly n_distinct items of 1..n_items (and ``extra`` values mixed in)."""
    items = rng.permutation(np.arange(1, n_items + 1))[:n_distinct]
    ev = np.concatenate([items, rng.choice(items, n - n_distinct - len(extra)), np.asarray(extra, dtype=np.int64)])
    return ev[rng.permutation(len(ev))]


def _build():
    rng = np.random.default_rng(2026)
    cases = []
    add = lambda *a, **k: cases.append(Case(*a, **k))  # noqa: E731

    # ---- row lengths x lookahead (labels from _labels), widths, seeds, epochs, row identity
    hs = [rng.integers(1, V + 1, n) for n in LENS]
    ls = [_labels(rng, n) for n in LENS]
    R = len(hs)
    every = np.arange(R)
    for look in (0, 1, 3, 10_000):
        add(f"lengths-lookahead{look}", BOTH, hs, ls, V, 32, look, every, R, 32, seed=3,
            valid=_windows if look == 3 else None)
    add("width-below-max_seq_length", BOTH, hs, ls, V, 32, 3, every, R, 8, seed=4, valid=_width_below)
    add("width-above-every-cnt", BOTH, hs, ls, V, 32, 3, every, R, 40, seed=4, valid=_width_above)
    some = np.array([3, 5, 9, 0, 10])  # 34, 65, 300, 1 and 513 events
    for s in SEEDS:
        add(f"seed-{s}", BOTH, hs, ls, V, 32, 3, some, len(some), 32, seed=s)
    for e in EPOCHS:
        add(f"epoch-{e}", ("rows",), hs, ls, V, 32, 3, some, len(some), 32, seed=1, epoch=e)
    add("identity-two-slots", ("rows",), hs, ls, V, 32, 3, [9, 0, 9, 7, 9], 5, 32, seed=11, epoch=4)
    add("identity-other-first", ("rows",), hs, ls, V, 32, 3, [4, 4, 2, 1, 6, 9, 3], 3, 32, first=4, seed=11, epoch=4)

    # ---- labels: the only positive is the last item; every item is positive
    hl = [rng.integers(1, V + 1, 50), rng.integers(1, V + 1, 50)]
    ll = [np.arange(50) == 49, np.ones(50, dtype=bool)]
    for look in (0, 3):
        add(f"labels-last-only-and-all-lookahead{look}", BOTH, hl, ll, V, 32, look, [0, 1], 2, 32, seed=5)

    # ---- threshold ties: positions (one per kernel: the streams differ), the exact path
    Vt = 1000
    for kind in BOTH:
        seed, i, j = POS_TIE[kind]
        w = tie_width(kind, SM.P_POSITIONS, seed, i, j)
        ht = [rng.permutation(np.arange(1, Vt + 1))[: j + 2]]
        add(f"tie-positions-{kind}", (kind,), ht, [_labels(rng, j + 2)], 4 * Vt, w, 3, [0], 1, w, seed=seed,
            valid=_pos_tie(kind))
    seed, i, j = EXACT_TIE
    cnt = tie_width("rows", SM.P_EXACT, seed, i, j)
    he = [rng.permutation(np.arange(1, cnt + 2))]  # cnt + 1 distinct events: every position taken, D = cnt + 1
    add("tie-exact-path", ("rows",), he, [_labels(rng, cnt + 1)], j + 1 + cnt + 1, cnt, 0, [0], 1, cnt, seed=seed,
        valid=_exact_tie)

    # ---- negatives: the regime limits at cnt = 32 (A admissible items of 160), history values outside the catalogue
    VA, cnt = 160, 32
    want = [(31, SM.REPLACE), (32, SM.EXACT), (33, SM.EXACT), (127, SM.EXACT), (128, SM.ROUNDS), (128, SM.ROUNDS)]
    hr = [_distinct_row(rng, VA - a, VA, max(VA - a + 8, 40)) for a, _ in want[:-1]]
    hr.append(_distinct_row(rng, VA - 128, VA, 48, extra=(0, -3, VA + 1, 0, -3, VA + 1, VA + 2)))
    lr = [_labels(rng, len(h)) for h in hr]
    for s in (0, 7):
        add(f"regime-limits-seed{s}", BOTH, hr, lr, VA, cnt, 2, np.arange(len(hr)), len(hr), cnt, seed=s,
            valid=_regimes([(a, g, cnt) for a, g in want]))
    add("rounds-both-rejections", BOTH, [hr[4]], [lr[4]], VA, cnt, 2, [0], 1, cnt, seed=ROUNDS_SEED, valid=_rounds_both)

    # ---- catalogue covered (cnt <= 57 and cnt > 57), one admissible item left, fewer admissible items than draws
    hc = [np.concatenate([np.arange(1, V + 1), rng.integers(1, V + 1, 20)])[rng.permutation(V + 20)]]
    lc = [_labels(rng, V + 20)]
    add("catalogue-covered-cnt32", BOTH, hc, lc, V, 32, 0, [0], 1, 32, seed=6, valid=_regimes([(V, SM.EXACT, 32)]))
    add("catalogue-covered-cnt64", BOTH, hc, lc, V, 64, 0, [0], 1, 64, seed=6, valid=_regimes([(V, SM.REPLACE, 64)]))
    h1 = [_crowded(rng, V - 1, n=70)]
    add("one-admissible-item", BOTH, h1, [_labels(rng, 70)], V, 32, 0, [0], 1, 32, seed=WALK_SEED, valid=_walk)
    hf = [_crowded(rng, V - 10, n=60), _crowded(rng, V - 31, n=60)]
    add("fewer-admissible-than-draws", BOTH, hf, [_labels(rng, 60) for _ in hf], V, 32, 0, [0, 1], 2, 32, seed=8,
        valid=_regimes([(10, SM.REPLACE, 32), (31, SM.REPLACE, 32)]))

    # ---- rows written as zeros
    add("zero-rows-past-the-order", ("rows",), hs, ls, V, 32, 3, [3, 5], 4, 32, seed=9,
        valid=_zero_rows([False, False, True, True]))
    add("zero-rows-outside-the-dataset", ("rows",), hs, ls, V, 32, 3, [3, -1, R, 5], 4, 32, seed=9,
        valid=_zero_rows([False, True, True, False]))
    add("zero-rows-over-max_history", BOTH, hs, ls, V, 32, 3, [4, 5, 9, 3], 4, 32, seed=9, max_history=64,
        valid=_zero_rows([False, True, True, False]))

    # ---- catalogue size: the longest supported row against 100 003 items; 5e7 items (the closed form of rank -> item)
    Vb = 100_003
    hb = [rng.integers(1, Vb + 1, 8192), rng.integers(1, Vb + 1, 50)]
    add("longest-row-big-catalogue", BOTH, hb, [_labels(rng, len(h)) for h in hb], Vb, 32, 3, [0, 1], 2, 32, seed=3)
    Vh = 50_000_000
    hh = [rng.integers(1, Vh + 1, n) for n in (2, 33, 64, 300)]
    hh[2][::2] = hh[2][1]  # repeated items
    add("huge-catalogue", ("rows",), hh, [_labels(rng, len(h)) for h in hh], Vh, 32, 0, np.arange(4), 4, 32, seed=1,
        valid=_closed_form)
    return cases


CASES = _build()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
RUNS = [(c.name, k) for c in CASES for k in c.kernels]
