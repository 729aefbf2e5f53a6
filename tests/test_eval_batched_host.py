"""CPU-side checks of the batched evaluation path: argument validation of xfmr_topk_tiled and xfmr_pool_rows (an error
code before any launch), the tiled search's O(B k) workspace, per-history truncation and the sorted exclusion lists."""

import numpy as np
import pytest

EINVAL, EUNSUPPORTED, EWORKSPACE, EALIGN = -1, -2, -3, -5
P = 1 << 20  # a 16-byte-aligned address: never dereferenced, every call below fails validation first


@pytest.fixture(scope="module")
def lib():
    from xfmr_rec_amd import _native as N

    return N.load()


def _tiled(lib, **kw):
    a = dict(query=P, table=P, rnorm=P, sqnorm=P, n_rows=1000, n_query=64, H=64, ex=None, exo=None, k=20, metric=0,
             out_idx=P, out_score=P, ws=P, ws_bytes=0)
    a.update(kw)
    return lib.xfmr_topk_tiled(a["query"], a["table"], a["rnorm"], a["sqnorm"], a["n_rows"], a["n_query"], a["H"], a["ex"],
                               a["exo"], a["k"], a["metric"], a["out_idx"], a["out_score"], a["ws"], a["ws_bytes"], None)


def test_topk_tiled_validates_before_launch(lib):
    assert _tiled(lib, query=None) == EINVAL
    assert _tiled(lib, out_idx=None) == EINVAL
    assert _tiled(lib, ws=None) == EINVAL
    assert _tiled(lib, n_rows=0) == EINVAL
    assert _tiled(lib, n_query=-1) == EINVAL
    assert _tiled(lib, k=0) == EINVAL
    assert _tiled(lib, ex=P) == EINVAL  # exclusion list without offsets
    assert _tiled(lib, metric=3) == EINVAL
    assert _tiled(lib, metric=0, rnorm=None) == EINVAL  # cosine needs the inverse norms
    assert _tiled(lib, metric=2, sqnorm=None) == EINVAL  # l2 needs the squared norms
    assert _tiled(lib, k=129) == EUNSUPPORTED
    assert _tiled(lib, H=66) == EUNSUPPORTED
    assert _tiled(lib, H=1028) == EUNSUPPORTED
    assert _tiled(lib, n_rows=1 << 31) == EUNSUPPORTED
    assert _tiled(lib, query=P + 4) == EALIGN
    assert _tiled(lib, table=P + 8) == EALIGN
    assert _tiled(lib, ws_bytes=0) == EWORKSPACE
    # dot needs neither norm array: only the workspace size stops this one
    assert _tiled(lib, metric=1, rnorm=None, sqnorm=None, ws_bytes=16) == EWORKSPACE


def test_topk_tiled_workspace_is_o_of_queries_times_k(lib):
    assert lib.xfmr_topk_tiled_workspace(0, 100, 20) == 0
    assert lib.xfmr_topk_tiled_workspace(10, 0, 20) == 0
    assert lib.xfmr_topk_tiled_workspace(10, 100, 0) == 0
    for B, V, k in [(1, 100, 1), (6040, 3953, 20), (8192, 1 << 20, 20), (138_000, 27_000, 128)]:
        n = lib.xfmr_topk_tiled_workspace(B, V, k)
        assert 0 < n <= B * k * 8 * 16  # at most 16 catalogue slices of (score, index) pairs
        assert n < lib.xfmr_topk_workspace(B, V)


def test_pool_rows_validates_before_launch(lib):
    assert lib.xfmr_pool_rows(None, P, P, 4, 64, 0, 0, 1e-12, None) == EINVAL
    assert lib.xfmr_pool_rows(P, None, P, 4, 64, 0, 0, 1e-12, None) == EINVAL
    assert lib.xfmr_pool_rows(P, P, None, 4, 64, 0, 0, 1e-12, None) == EINVAL
    assert lib.xfmr_pool_rows(P, P, P, 0, 64, 0, 0, 1e-12, None) == EINVAL
    assert lib.xfmr_pool_rows(P, P, P, 4, 0, 0, 0, 1e-12, None) == EINVAL
    assert lib.xfmr_pool_rows(P, P, P, 4, 64, 4, 0, 1e-12, None) == EINVAL
    assert lib.xfmr_pool_rows(P, P, P, 4, 64, -1, 0, 1e-12, None) == EINVAL
    assert lib.xfmr_pool_rows(P, P, P, 4, 64, 0, 1, 0.0, None) == EINVAL
    assert lib.xfmr_table_sqnorm(None, P, 10, 64, None) == EINVAL
    assert lib.xfmr_table_sqnorm(P, P, 0, 64, None) == EINVAL


def test_truncation_is_per_history():
    from xfmr_rec_amd.models import truncate_histories

    h = [list(range(1, 41)), [5, 6], [], list(range(100, 133))]
    got = truncate_histories(h, 32)
    assert got[0] == list(range(9, 41))  # the last 32 rows of THIS history
    assert got[1] == [5, 6] and got[2] == []
    assert got[3] == list(range(101, 133))
    assert truncate_histories([np.array([3, 4, 5])], 2) == [[4, 5]]


def test_sorted_exclusion_csr():
    from xfmr_rec_amd.retrieval import sorted_exclusion_csr

    flat, off = sorted_exclusion_csr([[9, 3, 3, 7], [], [5], [2, 2, 2], [-1, 100, 4]])
    assert off.tolist() == [0, 3, 3, 4, 5, 8]
    assert flat.tolist() == [3, 7, 9, 5, 2, -1, 4, 100]
    assert flat.dtype == np.int64 and off.dtype == np.int64
    flat, off = sorted_exclusion_csr([[], []])
    assert off.tolist() == [0, 0, 0] and flat.size == 1  # (one placeholder element: never read)
