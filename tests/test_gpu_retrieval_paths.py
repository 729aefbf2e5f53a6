"""The three retrieval paths held to each other and to numpy on inputs where summation order cannot matter: the scan
(``search``), the tiled search (``search_batch``) and the rank path (``rank_targets`` + ``rank_metrics_sum``).

Integer entries in [-3, 3], all finite: every dot product and every l2 score is an exact small integer in fp32 in any
order, so the lists must be EQUAL (indices and score bits), a target's rank must be its place in the list, and the rank
metrics must be the list metrics bit for bit. The numpy order is computed once per case and shared."""

import functools

import numpy as np
import pytest
import torch

import rank_refs as R

DEV = "cuda"
# (33, 389, 12): a second query tile with one real row, several slices with a partial last item tile, H % 8 != 0
SHAPES = [(33, 389, 12), (1, 2, 4)]
METRICS = ["dot", "l2"]
KS = [5, 100, 128]  # 100: a sort that is not a power of two in the scan kernel; 128: the tiled search's limit


@functools.lru_cache(maxsize=None)
def _case(n_query, n_rows, H, metric):
    rng = np.random.default_rng(7 * n_query + n_rows + H)
    table = rng.integers(-3, 4, (n_rows, H)).astype(np.float32)
    for _ in range(n_rows // 6):  # duplicated rows: exact ties
        table[int(rng.integers(1, n_rows))] = table[int(rng.integers(1, n_rows))]
    query = rng.integers(-3, 4, (n_query, H)).astype(np.float32)
    excl, tgts = [], []
    for b in range(n_query):
        if b % 4 == 2:  # a long history: fewer than 128 items stay eligible
            ex = rng.permutation(np.arange(1, n_rows + 3))[: (3 * n_rows) // 4]
        else:
            ex = rng.integers(1, n_rows + 3, int(rng.integers(0, 12)))  # ids >= n_rows among them
        ex = np.concatenate([ex, ex[: ex.size // 3]])  # repeats
        t = rng.integers(1, n_rows, int(rng.integers(1, 7))).tolist()
        if ex.size and b % 3 == 0:
            t[0] = int(ex[0])  # an excluded target (or one past the table)
        if b % 5 == 0:
            ex = np.concatenate([ex, [-1]])
        excl.append(np.sort(ex).astype(np.int64).tolist())  # sorted ascending, as the rank path needs
        if b % 4 == 1:
            t.append(t[0])  # a repeated target
        if b % 5 == 2:
            t.append(0)  # the padding row
        if b % 7 == 3:
            t.append(n_rows + int(rng.integers(0, 5)))  # past the table
        tgts.append(t)
    if n_query > 1:
        tgts[1] = []
    order, ranks = [], []
    for b in range(n_query):
        s = R.scores(query[b], table, metric)
        ok = np.isfinite(s)
        ok[0] = False
        ok[np.asarray([x for x in excl[b] if 0 <= x < n_rows], dtype=np.int64)] = False
        idx = np.flatnonzero(ok)
        idx = idx[np.lexsort((idx, -s[idx]))]  # score descending, ties by the lower index
        order.append((idx, s[idx].astype(np.float32)))
        ranks.append(R.ranks_from_scores(s, excl[b], tgts[b]))
    return table, query, excl, tgts, order, ranks


def _assert_inputs_bite(n_query, n_rows, H, metric):
    """From the numpy reference alone: the case has what the comparisons below are about."""
    _, _, _, tgts, order, ranks = _case(n_query, n_rows, H, metric)
    sizes = [idx.size for idx, _ in order]
    assert min(sizes) < 128  # a list that is padded
    if n_rows > 128:
        assert max(sizes) > 128 and min(sizes) > 5
        assert any(s.size > 5 and s[4] == s[5] for _, s in order)  # an exact tie straddling the 5th place
        flat = [r for row in ranks for r in row]
        assert any(r == R.RANK_NONE for r in flat) and any(5 < r <= 100 for r in flat) and any(128 < r < R.RANK_NONE for r in flat)


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("n_query,n_rows,H", SHAPES)
def test_inputs_have_ties_short_rows_and_long_rows(n_query, n_rows, H, metric):
    _assert_inputs_bite(n_query, n_rows, H, metric)


def _csr(lists):
    off = np.zeros(len(lists) + 1, dtype=np.int64)
    np.cumsum([len(x) for x in lists], out=off[1:])
    flat = np.concatenate([np.asarray(x, dtype=np.int64).reshape(-1) for x in lists] + [np.zeros(1, dtype=np.int64)])
    return torch.from_numpy(flat).to(DEV), torch.from_numpy(off).to(DEV)


@functools.lru_cache(maxsize=None)
def _index(n_query, n_rows, H, metric):
    from xfmr_rec_amd.retrieval import ExactItemIndex

    table, query = _case(n_query, n_rows, H, metric)[:2]
    return ExactItemIndex(torch.from_numpy(table).to(DEV), index_metric=metric), torch.from_numpy(query).to(DEV)


@functools.lru_cache(maxsize=None)
def _tiled_list(n_query, n_rows, H, metric, k):
    index, q = _index(n_query, n_rows, H, metric)
    return index.search_batch(q, _case(n_query, n_rows, H, metric)[2], top_k=k)


def _want_list(order, k):
    idx = np.full((len(order), k), -1, dtype=np.int64)
    score = np.full((len(order), k), -np.inf, dtype=np.float32)
    for b, (i, s) in enumerate(order):
        n = min(k, i.size)
        idx[b, :n], score[b, :n] = i[:n], s[:n]
    return idx, score


@pytest.mark.gpu
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("n_query,n_rows,H", SHAPES)
def test_scan_and_tiled_lists_are_the_numpy_list(n_query, n_rows, H, metric, k):
    _assert_inputs_bite(n_query, n_rows, H, metric)
    excl, order = _case(n_query, n_rows, H, metric)[2], _case(n_query, n_rows, H, metric)[4]
    index, q = _index(n_query, n_rows, H, metric)
    want_idx, want_score = _want_list(order, k)
    scan = index.search(q, excl, top_k=k)
    tiled = _tiled_list(n_query, n_rows, H, metric, k)
    for name, (idx, score) in (("scan", scan), ("tiled", tiled)):
        idx, score = idx.cpu().numpy(), score.cpu().numpy()
        for b in range(n_query):
            assert idx[b].tolist() == want_idx[b].tolist(), (name, b, idx[b][:8], want_idx[b][:8])
            assert score[b].view(np.uint32).tolist() == want_score[b].view(np.uint32).tolist(), (name, b)
    assert torch.equal(scan[0], tiled[0]) and torch.equal(scan[1].view(torch.int32), tiled[1].view(torch.int32))


@pytest.mark.gpu
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("n_query,n_rows,H", SHAPES)
def test_a_rank_is_the_place_in_the_list(n_query, n_rows, H, metric):
    """Every target against the k = 128 list, by its numpy rank w: w <= 128 -> in the list at place w - 1, with the list's
    score bits; no rank -> absent, RANK_NONE and -inf; w > 128 (only in a row whose list is full) -> absent, rank w and the
    numpy score's bits."""
    _assert_inputs_bite(n_query, n_rows, H, metric)
    _, _, excl, tgts, order, want = _case(n_query, n_rows, H, metric)
    index, q = _index(n_query, n_rows, H, metric)
    idx, score = (x.cpu().numpy() for x in _tiled_list(n_query, n_rows, H, metric, 128))
    csr = _csr(tgts)
    ranks, tscore = index.rank_targets(q, csr, _csr(excl), return_scores=True)
    ranks, tscore, off = ranks.cpu().numpy(), tscore.cpu().numpy(), csr[1].cpu().numpy()
    n_in = n_none = 0
    for b in range(n_query):
        place = {int(i): p for p, i in enumerate(idx[b]) if i >= 0}
        full = len(place) == 128
        assert full == (order[b][0].size >= 128)
        for e, t, w in zip(range(off[b], off[b + 1]), tgts[b], want[b]):
            assert ranks[e] == w, (b, t, ranks[e], w)
            if w <= 128:
                assert place.get(t) == w - 1, (b, t, w, place.get(t))
                assert tscore[e].view(np.uint32) == score[b, w - 1].view(np.uint32), (b, t, tscore[e], score[b, w - 1])
                n_in += 1
            elif w == R.RANK_NONE:
                assert t not in place and tscore[e] == -np.inf, (b, t, tscore[e])
                n_none += 1
            else:
                assert full and t not in place and tscore[e].view(np.uint32) == order[b][1][w - 1].view(np.uint32), (b, t, w)
    assert n_none > 0 and (n_in > 0 or n_rows == 2)


@pytest.mark.gpu
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("n_query,n_rows,H", SHAPES)
def test_rank_metrics_are_the_metrics_of_the_lists(n_query, n_rows, H, metric):
    from xfmr_rec_amd.retrieval import rank_metrics_sum, retrieval_metrics_sum

    _assert_inputs_bite(n_query, n_rows, H, metric)
    _, _, excl, tgts, _, _ = _case(n_query, n_rows, H, metric)
    index, q = _index(n_query, n_rows, H, metric)
    csr = _csr(tgts)
    ranks = index.rank_targets(q, csr, _csr(excl))
    use = np.random.default_rng(n_query).random(n_query) < 0.7
    use[0] = True
    for mask in (None, torch.from_numpy(use).to(DEV)):
        sums, vals, valid = rank_metrics_sum(ranks, csr, (5, 100), mask, per_row=True)
        assert valid.cpu().tolist() == [len(t) > 0 for t in tgts]
        for ci, k in enumerate((5, 100)):
            idx = _tiled_list(n_query, n_rows, H, metric, k)[0]
            wsums, wvals, wvalid = retrieval_metrics_sum(idx, csr, mask, top_k=k, per_row=True)
            assert torch.equal(valid, wvalid)
            assert torch.equal(vals[:, ci].view(torch.int32), wvals.view(torch.int32)), (k, (vals[:, ci] != wvals).nonzero()[:5].tolist())
            assert torch.equal(sums[ci].view(torch.int64), wsums.view(torch.int64)), (k, sums[ci].tolist(), wsums.tolist())
        assert float(sums[0, 7]) == float((np.asarray([len(t) > 0 for t in tgts]) & (use if mask is not None else True)).sum())
