"""CPU-side checks of xfmr_candidate_ranks: the symbol is exported and bound, and every refusal that the arguments alone
decide comes back as its error code, in the order EINVAL < EUNSUPPORTED < EALIGN, before anything is launched or read
(every pointer below is a bare address that is never dereferenced). The refusal of 2^31 or more candidates or targets
needs the offsets, which live on the device: tests/test_gpu_candidate_ranks.py holds it."""

import pathlib

import pytest

EINVAL, EUNSUPPORTED, EALIGN = -1, -2, -5
P = 1 << 20  # a 16-byte-aligned address: never dereferenced, every call below fails validation first
ROOT = pathlib.Path(__file__).resolve().parents[1]


@pytest.fixture(scope="module")
def lib():
    from xfmr_rec_amd import _native as N

    return N.load()


def _call(lib, **kw):
    a = dict(query=P, table=P, rnorm=P, sqnorm=P, n_rows=1000, n_query=64, H=64, cand=P, cando=P, ex=None, exo=None, tgt=P,
             tgo=P, metric=0, out=P, tscore=None, cscore=None)
    a.update(kw)
    return lib.xfmr_candidate_ranks(a["query"], a["table"], a["rnorm"], a["sqnorm"], a["n_rows"], a["n_query"], a["H"],
                                    a["cand"], a["cando"], a["ex"], a["exo"], a["tgt"], a["tgo"], a["metric"], a["out"],
                                    a["tscore"], a["cscore"], None)


def test_symbol_is_exported_declared_and_bound(lib):
    from xfmr_rec_amd import _native as N

    assert "xfmr_candidate_ranks" in N.EXPORTED_SYMBOLS
    assert hasattr(lib, "xfmr_candidate_ranks")
    header = (ROOT / "include" / "xfmr_hip.h").read_text()
    assert "int xfmr_candidate_ranks(" in header
    assert len(N._SIGNATURES["xfmr_candidate_ranks"][1]) == 18  # the header's argument list
    assert lib.xfmr_abi_version() == N.ABI_VERSION  # an added entry: the existing ones did not change


INVALID = (dict(query=None), dict(table=None), dict(cand=None), dict(cando=None), dict(tgo=None), dict(out=None),
           dict(n_rows=0), dict(n_query=0), dict(n_query=-3), dict(H=0), dict(ex=P), dict(exo=P), dict(metric=3),
           dict(metric=-1), dict(metric=0, rnorm=None), dict(metric=2, sqnorm=None),
           # the score-only form (no targets): no target output of any kind, and the candidates' scores are required
           dict(tgt=None, tgo=None, out=None, tscore=None, cscore=None), dict(tgt=None, tgo=P, out=None, cscore=P),
           dict(tgt=None, tgo=None, out=P, cscore=P), dict(tgt=None, tgo=None, out=None, tscore=P, cscore=P))
UNSUPPORTED = (dict(H=6), dict(H=66), dict(H=1028), dict(n_rows=1 << 31), dict(n_query=1 << 31))
MISALIGNED = (dict(query=P + 4), dict(table=P + 8))


def test_refusals_before_any_launch(lib):
    for kw in INVALID:
        assert _call(lib, **kw) == EINVAL, kw
    for kw in UNSUPPORTED:
        assert _call(lib, **kw) == EUNSUPPORTED, kw
    for kw in MISALIGNED:
        assert _call(lib, **kw) == EALIGN, kw
    for kw in (dict(tgt=None, tgo=None, out=None, cscore=P), dict(cscore=P, tscore=P)):  # both forms are refused alike
        assert _call(lib, H=6, **kw) == EUNSUPPORTED, kw
        assert _call(lib, query=P + 4, **kw) == EALIGN, kw


def test_refusals_keep_their_order(lib):
    """EINVAL before EUNSUPPORTED before EALIGN: an argument set with faults of two kinds reports the earlier kind."""
    for bad in INVALID:
        for worse in UNSUPPORTED + MISALIGNED:
            if set(bad) & set(worse):
                continue
            assert _call(lib, **bad, **worse) == EINVAL, (bad, worse)
    for bad in UNSUPPORTED:
        for worse in MISALIGNED:
            assert _call(lib, **bad, **worse) == EUNSUPPORTED, (bad, worse)
    # the metric decides which norm array is read: dot needs neither (the call then fails on the next fault)
    assert _call(lib, metric=1, rnorm=None, sqnorm=None, H=6) == EUNSUPPORTED
    assert _call(lib, metric=0, sqnorm=None, H=6) == EUNSUPPORTED
    assert _call(lib, metric=2, rnorm=None, query=P + 4) == EALIGN
