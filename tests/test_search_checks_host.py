"""CPU-side checks of the three search entries' refusals (xfmr_topk, xfmr_topk_tiled, xfmr_target_ranks): every code of
xfmr_topk, which no other test pins, and for all three the code that wins when two faults coincide -- EINVAL before
EUNSUPPORTED before EALIGN before EWORKSPACE. No call below reaches a launch."""

import pytest

EINVAL, EUNSUPPORTED, EWORKSPACE, EALIGN = -1, -2, -3, -5
P = 1 << 20  # a 16-byte-aligned address: never dereferenced, every call below fails validation first
BIG = 1 << 40


@pytest.fixture(scope="module")
def lib():
    from xfmr_rec_amd import _native as N

    return N.load()


def _scan(lib, **kw):
    a = dict(query=P, table=P, rnorm=P, n_rows=1000, n_query=4, H=64, ex=None, exo=None, k=20, metric=0, out_idx=P,
             out_score=P, ws=P, ws_bytes=BIG)
    a.update(kw)
    return lib.xfmr_topk(a["query"], a["table"], a["rnorm"], a["n_rows"], a["n_query"], a["H"], a["ex"], a["exo"], a["k"],
                         a["metric"], a["out_idx"], a["out_score"], a["ws"], a["ws_bytes"], None)


def _tiled(lib, **kw):
    a = dict(query=P, table=P, rnorm=P, sqnorm=P, n_rows=1000, n_query=64, H=64, ex=None, exo=None, k=20, metric=0,
             out_idx=P, out_score=P, ws=P, ws_bytes=BIG)
    a.update(kw)
    return lib.xfmr_topk_tiled(a["query"], a["table"], a["rnorm"], a["sqnorm"], a["n_rows"], a["n_query"], a["H"], a["ex"],
                               a["exo"], a["k"], a["metric"], a["out_idx"], a["out_score"], a["ws"], a["ws_bytes"], None)


def _ranks(lib, **kw):
    a = dict(query=P, table=P, rnorm=P, sqnorm=P, n_rows=1000, n_query=64, H=64, ex=None, exo=None, tgt=P, tgo=P,
             n_targets=500, metric=0, out=P, score=None, ws=P, ws_bytes=BIG)
    a.update(kw)
    return lib.xfmr_target_ranks(a["query"], a["table"], a["rnorm"], a["sqnorm"], a["n_rows"], a["n_query"], a["H"],
                                 a["ex"], a["exo"], a["tgt"], a["tgo"], a["n_targets"], a["metric"], a["out"], a["score"],
                                 a["ws"], a["ws_bytes"], None)


def test_topk_validates_before_launch(lib):
    for kw in (dict(query=None), dict(table=None), dict(rnorm=None), dict(out_idx=None), dict(out_score=None),
               dict(ws=None), dict(metric=1, rnorm=None), dict(metric=2, rnorm=None),  # the scan always takes the norms
               dict(n_rows=0), dict(n_rows=-1), dict(n_query=0), dict(n_query=-1), dict(H=0), dict(H=-4), dict(k=0),
               dict(k=-1), dict(ex=P), dict(exo=P), dict(metric=3), dict(metric=-1)):
        assert _scan(lib, **kw) == EINVAL, kw
    for kw in (dict(H=6), dict(H=66), dict(H=1028), dict(k=1025), dict(n_rows=1 << 31)):
        assert _scan(lib, **kw) == EUNSUPPORTED, kw
    for kw in (dict(table=P + 8), dict(ws=P + 4)):
        assert _scan(lib, **kw) == EALIGN, kw
    need = lib.xfmr_topk_workspace(4, 1000)
    assert need == 4 * 1000 * 4
    assert _scan(lib, ws_bytes=need - 1) == EWORKSPACE
    assert _scan(lib, ws_bytes=0) == EWORKSPACE
    # what the scan does NOT refuse: a query that is not 16-byte aligned, k and H at their limits, 2^31 queries --
    # only the workspace size stops these
    assert _scan(lib, query=P + 4, ws_bytes=0) == EWORKSPACE
    assert _scan(lib, k=1024, H=1024, ws_bytes=0) == EWORKSPACE
    assert _scan(lib, n_query=1 << 31, ws_bytes=BIG) == EWORKSPACE
    assert lib.xfmr_topk_workspace(0, 10) == 0 and lib.xfmr_topk_workspace(10, 0) == 0


def test_search_entries_refuse_in_one_precedence(lib):
    for name, call, too_many in (("topk", _scan, dict(k=1025)), ("tiled", _tiled, dict(k=129)),
                                 ("ranks", _ranks, dict(n_targets=1 << 31))):
        # EINVAL wins over everything
        assert call(lib, metric=3, table=P + 8) == EINVAL, name
        assert call(lib, metric=3, H=66, ws=P + 4, ws_bytes=0) == EINVAL, name
        assert call(lib, table=None, H=66) == EINVAL, name
        assert call(lib, ex=P, H=1028) == EINVAL, name
        assert call(lib, n_rows=0, **too_many) == EINVAL, name
        assert call(lib, rnorm=None, **too_many) == EINVAL, name  # (metric 0: every entry needs the inverse norms)
        # EUNSUPPORTED over EALIGN and EWORKSPACE
        assert call(lib, H=66, table=P + 8) == EUNSUPPORTED, name
        assert call(lib, n_rows=1 << 31, ws=P + 4, ws_bytes=0) == EUNSUPPORTED, name
        assert call(lib, ws_bytes=0, **too_many) == EUNSUPPORTED, name
        assert call(lib, table=P + 4, **too_many) == EUNSUPPORTED, name
        # EALIGN over EWORKSPACE
        assert call(lib, ws=P + 8, ws_bytes=0) == EALIGN, name
        assert call(lib, table=P + 4, ws_bytes=16) == EALIGN, name
    for name, call in (("tiled", _tiled), ("ranks", _ranks)):
        assert call(lib, metric=2, sqnorm=None, query=P + 4) == EINVAL, name
        assert call(lib, metric=0, rnorm=None, H=66) == EINVAL, name
        assert call(lib, n_query=1 << 31, query=P + 4) == EUNSUPPORTED, name
        assert call(lib, query=P + 4, ws_bytes=0) == EALIGN, name
    assert _ranks(lib, tgt=None, n_targets=1 << 31) == EINVAL
    assert _ranks(lib, n_targets=-1, H=66) == EINVAL
