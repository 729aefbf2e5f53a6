"""Host side of the sampled-candidate protocol (numpy only, no device): ``eval_rows.sample_eval_negatives`` draws what it
says it draws, is a function of ``(seed, row)`` alone, and explicit candidate lists are mapped like every other id list."""

import numpy as np
import pytest

from xfmr_rec_amd import eval_rows as E

N_ITEMS = 60


def _rows(n=25, seed=0):
    rng = np.random.default_rng(seed)
    hists = [rng.integers(1, N_ITEMS, int(rng.integers(0, 30))).tolist() for _ in range(n)]
    tgts = [rng.integers(1, N_ITEMS, int(rng.integers(0, 4))).tolist() for _ in range(n)]
    hists[3] = list(range(1, N_ITEMS - 4))  # only a handful of items left to draw from
    tgts[3] = [N_ITEMS - 4]
    hists[4] = list(range(1, N_ITEMS))  # nothing left
    return hists, tgts


def _lists(csr):
    flat, off = csr
    assert flat.dtype == np.int64 and off.dtype == np.int64 and off[0] == 0
    return [flat[off[i] : off[i + 1]].tolist() for i in range(off.size - 1)]


def test_lists_are_sorted_distinct_disjoint_and_of_the_asked_size():
    hists, tgts = _rows()
    for k in (0, 1, 10, 100):
        got = _lists(E.sample_eval_negatives(hists, tgts, N_ITEMS, k, seed=7))
        assert len(got) == len(hists)
        for h, t, neg in zip(hists, tgts, got):
            free = set(range(1, N_ITEMS)) - set(h) - set(t)
            assert neg == sorted(set(neg)) and set(neg) <= free
            assert len(neg) == min(k, len(free))  # all the eligible items where fewer exist than asked
        assert got[4] == [] and (k < 3 or got[3] == [N_ITEMS - 3, N_ITEMS - 2, N_ITEMS - 1])
    flat, off = E.sample_eval_negatives([], [], N_ITEMS, 5, seed=0)
    assert off.tolist() == [0] and flat.size == 1  # (flat_csr's placeholder element)


def test_same_seed_same_lists_and_another_seed_differs():
    hists, tgts = _rows()
    a = _lists(E.sample_eval_negatives(hists, tgts, N_ITEMS, 10, seed=3))
    assert a == _lists(E.sample_eval_negatives(hists, tgts, N_ITEMS, 10, seed=3))
    b = _lists(E.sample_eval_negatives(hists, tgts, N_ITEMS, 10, seed=4))
    assert a != b and sum(x != y for x, y in zip(a, b)) > len(a) // 2


def test_a_rows_list_does_not_depend_on_the_other_rows():
    hists, tgts = _rows()
    whole = _lists(E.sample_eval_negatives(hists, tgts, N_ITEMS, 10, seed=3))
    # the rows behind row 11 removed; every other row emptied: row i keeps its list as long as it keeps its place i
    head = _lists(E.sample_eval_negatives(hists[:12], tgts[:12], N_ITEMS, 10, seed=3))
    assert head == whole[:12]
    alone = _lists(E.sample_eval_negatives([h if i == 11 else [] for i, h in enumerate(hists)],
                                           [t if i == 11 else [] for i, t in enumerate(tgts)], N_ITEMS, 10, seed=3))
    assert alone[11] == whole[11]


def test_weighted_draws_never_pick_a_zero_weight_item():
    hists, tgts = _rows()
    w = np.zeros(N_ITEMS)
    w[5:40:2] = np.arange(1, 19)
    got = _lists(E.sample_eval_negatives(hists, tgts, N_ITEMS, 6, seed=1, weights=w))
    for h, t, neg in zip(hists, tgts, got):
        free = {i for i in range(1, N_ITEMS) if w[i] > 0} - set(h) - set(t)
        assert set(neg) <= free and neg == sorted(set(neg)) and len(neg) == min(6, len(free))
    assert got == _lists(E.sample_eval_negatives(hists, tgts, N_ITEMS, 6, seed=1, weights=w))
    # in proportion to the weights: over many rows the heavy item is drawn far more often than the light one
    many = _lists(E.sample_eval_negatives([[]] * 400, [[]] * 400, N_ITEMS, 3, seed=2, weights=w))
    count = np.bincount(np.concatenate(many), minlength=N_ITEMS)
    assert count[w == 0].sum() == 0 and count[39] > 3 * count[5]
    for bad in (np.ones(N_ITEMS - 1), -np.ones(N_ITEMS), np.full(N_ITEMS, np.nan)):
        with pytest.raises(ValueError, match="weights"):
            E.sample_eval_negatives(hists, tgts, N_ITEMS, 6, seed=1, weights=bad)
    with pytest.raises(ValueError):
        E.sample_eval_negatives(hists, tgts[:-1], N_ITEMS, 6, seed=1)


def test_explicit_candidates_are_mapped_and_unknown_ids_dropped():
    id2idx = {f"i{i}": i for i in range(1, N_ITEMS)}
    given = [["i7", "nope", "i3", "i7"], [], ["ghost"], ["i59", "i1"]]
    rows = E.map_candidates(given, lambda ids: E.lookup_rows(id2idx, ids))
    assert rows == [[7, 3, 7], [], [], [59, 1]]
    flat, off = E.candidates_csr(rows)
    assert _lists((flat, off)) == [[3, 7], [], [], [1, 59]]  # each row sorted ascending, repeats dropped
