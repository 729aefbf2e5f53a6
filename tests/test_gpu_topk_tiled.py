"""xfmr_topk_tiled (ExactItemIndex.search_batch): MFMA score tiles + a streaming top-k, checked against the exact
numpy search (oracle/metrics.py:topk) and against the scan kernel xfmr_topk (ExactItemIndex.search): all three metrics,
H from 32 to 1024, k in {1, 20, 128}, catalogues smaller than one item tile up to 2^20 rows, query counts around the
32-query tile, exclusion lists of every shape, exact ties, and run-to-run bit identity."""

import numpy as np
import pytest
import torch

from oracle import metrics as OMx

pytestmark = pytest.mark.gpu


def _data(V, H, B, seed):
    g = torch.Generator().manual_seed(seed)
    table = torch.randn(V + 1, H, generator=g)
    table[0] = 0
    q = torch.randn(B, H, generator=g)
    return table, q


def _oracle_excl(ex, V):
    return [int(x) for x in ex if 1 <= int(x) <= V] if ex is not None else None


def _check_rows(idx, score, q, table, excl, k, metric, rows):
    V = table.shape[0] - 1
    tnp, qnp = table.numpy(), q.numpy()
    for b in rows:
        ex = _oracle_excl(excl[b], V) if excl is not None else None
        want_idx, want_s = OMx.topk(qnp[b], tnp, ex, k, metric)
        n = len(want_s)
        np.testing.assert_allclose(score[b, :n], want_s, rtol=2e-5, atol=2e-5)
        assert (idx[b, n:] == -1).all() and np.isneginf(score[b, n:]).all(), b
        assert not (set(idx[b, :n].tolist()) & set(ex or ())) and 0 not in idx[b, :n]
        diff = set(idx[b, :n].tolist()) ^ set(want_idx[:n])  # same set up to numerically tied scores at the boundary
        assert len(diff) <= 2, (b, diff)
        assert (np.diff(score[b, :n]) <= 1e-7).all()


def _check_against_scan(got, want):
    (gi, gs), (wi, ws) = got, want
    gi, gs, wi, ws = gi.cpu().numpy(), gs.cpu().numpy(), wi.cpu().numpy(), ws.cpu().numpy()
    assert ((gi == -1) == (wi == -1)).all()
    fin = wi != -1
    np.testing.assert_allclose(gs[fin], ws[fin], rtol=2e-5, atol=2e-5)
    for b in range(gi.shape[0]):
        assert len(set(gi[b][gi[b] >= 0].tolist()) ^ set(wi[b][wi[b] >= 0].tolist())) <= 2, b


@pytest.mark.parametrize("metric,H,k,V,B", [
    ("cosine", 32, 20, 100, 1),       # catalogue smaller than one 128-item tile
    ("dot", 64, 1, 1000, 63),         # not a multiple of the tile
    ("l2", 100, 128, 777, 64),
    ("cosine", 384, 20, 3900, 65),
    ("dot", 1024, 20, 500, 9),
    ("l2", 384, 1, 300, 65),
    ("cosine", 64, 128, 100_003, 8),  # >= 100 k rows
    ("l2", 32, 20, 2000, 130),
])
def test_tiled_topk_matches_oracle_and_scan(metric, H, k, V, B):
    from xfmr_rec_amd.retrieval import ExactItemIndex

    table, q = _data(V, H, B, seed=V + H + B)
    rng = np.random.default_rng(k)
    excl = [rng.integers(1, V + 1, int(rng.integers(0, min(V, 60)))).tolist() for _ in range(B)]
    index = ExactItemIndex(table.cuda(), index_metric=metric)
    got = index.search_batch(q.cuda(), excl, top_k=k)
    idx, score = got[0].cpu().numpy(), got[1].cpu().numpy()
    _check_rows(idx, score, q, table, excl, k, metric, range(min(B, 12)))
    _check_against_scan(got, index.search(q.cuda(), excl, top_k=k))


def test_tiled_topk_all_users_deterministic():
    """ML-1M shape: 6 040 users x 3 900 items, H 384. A sample against the oracle, all against the scan, twice."""
    from xfmr_rec_amd.retrieval import ExactItemIndex

    V, H, B, k = 3900, 384, 6040, 20
    table, q = _data(V, H, B, seed=7)
    rng = np.random.default_rng(0)
    excl = [rng.integers(1, V + 1, int(n)).tolist() for n in rng.integers(1, 200, B)]
    index = ExactItemIndex(table.cuda())
    a = index.search_batch(q.cuda(), excl, top_k=k)
    b = index.search_batch(q.cuda(), excl, top_k=k)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
    rows = rng.choice(B, 16, replace=False)
    _check_rows(a[0].cpu().numpy(), a[1].cpu().numpy(), q, table, excl, k, "cosine", rows)
    _check_against_scan(a, index.search(q.cuda(), excl, top_k=k))


def test_tiled_topk_exclusion_shapes():
    from xfmr_rec_amd.retrieval import ExactItemIndex

    V, H, k = 300, 64, 20
    table, q = _data(V, H, 6, seed=3)
    excl = [
        [],                                           # nothing excluded
        [250, 3, 17, 3, 250, 99, 17, 1],             # unsorted, duplicates
        [-5, 0, V + 1, V + 100, 12],                 # out of range (ignored) + padding row
        list(range(V, 5, -1)),                       # all but 5 items: -1 padding after them
        list(range(1, V + 1))[::-1] + [1, 2],        # everything
        [7],
    ]
    for metric in ("cosine", "dot", "l2"):
        index = ExactItemIndex(table.cuda(), index_metric=metric)
        idx, score = index.search_batch(q.cuda(), excl, top_k=k)
        idx, score = idx.cpu().numpy(), score.cpu().numpy()
        _check_rows(idx, score, q, table, excl, k, metric, range(6))
        assert sorted(idx[3, :5].tolist()) == [1, 2, 3, 4, 5] and (idx[3, 5:] == -1).all()
        assert (idx[4] == -1).all() and np.isneginf(score[4]).all()
        none_idx, none_score = index.search_batch(q.cuda(), None, top_k=k)
        _check_rows(none_idx.cpu().numpy(), none_score.cpu().numpy(), q, table, None, k, metric, range(6))


@pytest.mark.parametrize("metric", ["cosine", "dot", "l2"])
def test_tiled_topk_exact_ties_lower_index_first(metric):
    """Seven distinct rows repeated over a 5 000-row catalogue: every score is tied with hundreds of others, across
    item tiles and catalogue slices. The list must be the oracle's exactly: the lowest indices of the best rows."""
    from xfmr_rec_amd.retrieval import ExactItemIndex

    g = torch.Generator().manual_seed(11)
    V, H, k, B = 5000, 96, 128, 40
    base = torch.randn(7, H, generator=g)
    table = base[torch.arange(V + 1) % 7].contiguous()
    table[0] = 0
    q = torch.randn(B, H, generator=g)
    idx, score = ExactItemIndex(table.cuda(), index_metric=metric).search_batch(q.cuda(), None, top_k=k)
    idx, score = idx.cpu().numpy(), score.cpu().numpy()
    for b in range(B):
        want_idx, want_s = OMx.topk(q[b].numpy(), table.numpy(), None, k, metric)
        assert idx[b].tolist() == want_idx, b
        np.testing.assert_allclose(score[b], want_s, rtol=2e-5, atol=2e-5)


def test_tiled_topk_million_row_catalogue():
    """2^20 rows at H 64 for 8 192 users: the scan's (B, n_rows) workspace would be 32 GB; the tiled search needs
    O(B k) scratch. A sample of users against an exact float64 search."""
    from xfmr_rec_amd import _native as N
    from xfmr_rec_amd.retrieval import ExactItemIndex

    V, H, B, k = (1 << 20) - 1, 64, 8192, 20
    assert N.load().xfmr_topk_workspace(B, V + 1) == B * (V + 1) * 4 == 32 << 30
    assert N.load().xfmr_topk_tiled_workspace(B, V + 1, k) < 64 << 20
    g = torch.Generator(device="cuda").manual_seed(5)
    table = torch.randn(V + 1, H, generator=g, device="cuda")
    table[0] = 0
    q = torch.randn(B, H, generator=g, device="cuda")
    idx, score = ExactItemIndex(table, index_metric="dot").search_batch(q, None, top_k=k)
    idx, score = idx.cpu().numpy(), score.cpu().numpy()
    t64 = table.cpu().double()
    rows = [0, 1, 4095, 8191]
    s = (t64 @ q.cpu().double()[rows].T).numpy()  # (V + 1, 4)
    s[0] = -np.inf
    for c, b in enumerate(rows):
        order = np.lexsort((np.arange(V + 1), -s[:, c]))[:k]
        np.testing.assert_allclose(score[b], s[order, c], rtol=2e-5, atol=2e-5)
        assert len(set(idx[b].tolist()) ^ set(order.tolist())) <= 2, b


def test_tiled_topk_rejects_k_over_128():
    from xfmr_rec_amd.retrieval import ExactItemIndex

    table, q = _data(200, 64, 3, seed=1)
    with pytest.raises(RuntimeError, match=r"code -2"):
        ExactItemIndex(table.cuda()).search_batch(q.cuda(), None, top_k=129)
