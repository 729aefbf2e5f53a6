"""CPU-side checks of the rank path: the metrics written from ranks against the oracle's list-based metrics, argument
validation of xfmr_target_ranks / xfmr_rank_metrics_sum (an error code before any launch), their workspace queries, and
the ``<metric>@<K>`` monitor names of ``Trainer.fit``."""

import ctypes as C

import numpy as np
import pytest

import rank_refs as R

EINVAL, EUNSUPPORTED, EWORKSPACE, EALIGN = -1, -2, -3, -5
P = 1 << 20  # a 16-byte-aligned address: never dereferenced, every call below fails validation first


@pytest.fixture(scope="module")
def lib():
    from xfmr_rec_amd import _native as N

    return N.load()


# ------------------------------------------------------------------------------------ the metrics written from ranks
def _case(rng):
    n_rows, H = int(rng.integers(2, 40)), 4
    table = rng.integers(-2, 3, (n_rows, H)).astype(np.float64)
    for _ in range(int(rng.integers(0, 4))):  # duplicated rows: tied scores
        table[int(rng.integers(1, n_rows))] = table[int(rng.integers(1, n_rows))]
    query = rng.integers(-2, 3, H).astype(np.float64)
    excl = rng.integers(1, n_rows, int(rng.integers(0, 6))).tolist()
    n_t = int(rng.integers(0, 7))
    tgts = rng.integers(1, n_rows, n_t).tolist()
    if n_t and rng.random() < 0.4 and excl:
        tgts[0] = excl[0]  # an excluded target
    if n_t > 1 and rng.random() < 0.4:
        tgts[1] = tgts[0]  # a repeated target
    if n_t > 2 and rng.random() < 0.3:
        tgts[2] = 0  # the padding row as a target
    return table, query, excl, tgts


def test_metrics_from_ranks_equal_the_oracle_metrics_on_lists():
    from oracle.metrics import compute_retrieval_metrics, topk

    rng = np.random.default_rng(0)
    worst, n_valid, seen = 0.0, 0, set()
    for case in range(300):
        table, query, excl, tgts = _case(rng)
        metric = ("dot", "l2", "cosine")[case % 3]
        if metric == "cosine":
            table[1:][np.abs(table[1:]).sum(1) == 0] = 1.0  # (the oracle divides by the row norm)
        ranks = R.ranks_from_scores(R.scores(query, table, metric), excl, tgts)
        for K in (1, 2, 5, 20, 64, 200):
            rec, _ = topk(query, table, excl, K, metric)
            want = compute_retrieval_metrics(rec, tgts, K)
            got = R.metrics_from_ranks(ranks, tgts, K)
            assert set(got) == set(want)
            for name in want:
                worst = max(worst, abs(got[name] - want[name]))
                assert abs(got[name] - want[name]) <= 1e-12, (case, K, name, got[name], want[name])
            n_valid += bool(want)
        seen |= {("excluded", bool(set(tgts) & set(excl))), ("repeat", len(set(tgts)) < len(tgts)), ("zero", 0 in tgts),
                 ("none", not tgts)}
    print(f"largest difference {worst:.3e} over {n_valid} valid (case, K) pairs")
    assert n_valid > 1000
    assert {("excluded", True), ("repeat", True), ("zero", True), ("none", True)} <= seen


def test_ranks_from_scores_eligibility_and_ties():
    s = np.array([9.0, 3.0, 5.0, 5.0, np.inf, 1.0, np.nan, 5.0])
    # eligible: 1, 2, 3, 5, 7 minus the excluded 3 -> order 2, 7, 1, 5
    got = R.ranks_from_scores(s, [3, 3, 100, -1], [2, 7, 1, 5, 3, 0, 4, 6, 8, -1, 2])
    assert got == [1, 2, 3, 4, R.RANK_NONE, R.RANK_NONE, R.RANK_NONE, R.RANK_NONE, R.RANK_NONE, R.RANK_NONE, 1]
    m = R.metrics_from_ranks(got, [2, 7, 1, 5, 3, 0, 4, 6, 8, -1, 2], 2)
    assert m["retrieval_recall"] == 2 / 10 and m["retrieval_precision"] == 1.0 and m["retrieval_auroc"] == 0.0
    assert R.metrics_from_ranks([], [], 5) == {}


# ------------------------------------------------------------------------------------ the C entry points refuse first
def _ranks(lib, **kw):
    a = dict(query=P, table=P, rnorm=P, sqnorm=P, n_rows=1000, n_query=64, H=64, ex=None, exo=None, tgt=P, tgo=P,
             n_targets=500, metric=0, out=P, score=None, ws=P, ws_bytes=1 << 40)
    a.update(kw)
    return lib.xfmr_target_ranks(a["query"], a["table"], a["rnorm"], a["sqnorm"], a["n_rows"], a["n_query"], a["H"],
                                 a["ex"], a["exo"], a["tgt"], a["tgo"], a["n_targets"], a["metric"], a["out"], a["score"],
                                 a["ws"], a["ws_bytes"], None)


def test_target_ranks_validates_before_launch(lib):
    for kw in (dict(query=None), dict(table=None), dict(tgt=None), dict(tgo=None), dict(out=None), dict(ws=None),
               dict(n_rows=0), dict(n_query=0), dict(n_query=-3), dict(H=0), dict(n_targets=-1), dict(ex=P), dict(exo=P),
               dict(metric=3), dict(metric=-1), dict(metric=0, rnorm=None), dict(metric=2, sqnorm=None)):
        assert _ranks(lib, **kw) == EINVAL, kw
    for kw in (dict(H=6), dict(H=66), dict(H=1028), dict(n_rows=1 << 31), dict(n_query=1 << 31), dict(n_targets=1 << 31)):
        assert _ranks(lib, **kw) == EUNSUPPORTED, kw
    for kw in (dict(query=P + 4), dict(table=P + 8), dict(ws=P + 4)):
        assert _ranks(lib, **kw) == EALIGN, kw
    need = lib.xfmr_target_ranks_workspace(64, 1000, 500)
    assert _ranks(lib, ws_bytes=need - 1) == EWORKSPACE
    assert _ranks(lib, ws_bytes=0) == EWORKSPACE
    assert _ranks(lib, metric=1, rnorm=None, sqnorm=None, ws_bytes=16) == EWORKSPACE  # dot needs neither norm array


def _metrics(lib, cutoffs=(5, 20), **kw):
    cut = (C.c_int32 * max(len(cutoffs), 1))(*cutoffs)
    a = dict(ranks=P, tgt=P, tgo=P, use=None, n_query=300, cut=cut, n_cut=len(cutoffs), sums=P, out=None, valid=None,
             ws=P, ws_bytes=1 << 40)
    a.update(kw)
    return lib.xfmr_rank_metrics_sum(a["ranks"], a["tgt"], a["tgo"], a["use"], a["n_query"], a["cut"], a["n_cut"],
                                     a["sums"], a["out"], a["valid"], a["ws"], a["ws_bytes"], None)


def test_rank_metrics_sum_validates_before_launch(lib):
    for kw in (dict(ranks=None), dict(tgt=None), dict(tgo=None), dict(sums=None), dict(ws=None), dict(cut=None),
               dict(n_query=0), dict(n_query=-1), dict(n_cut=0), dict(n_cut=9), dict(n_cut=-1)):
        assert _metrics(lib, **kw) == EINVAL, kw
    assert _metrics(lib, cutoffs=(1, 2, 3, 4, 5, 6, 7, 8, 9)) == EINVAL
    assert _metrics(lib, cutoffs=(5, 0)) == EINVAL
    assert _metrics(lib, cutoffs=(-20,)) == EINVAL
    assert _metrics(lib, n_query=1 << 31) == EUNSUPPORTED
    need = lib.xfmr_rank_metrics_sum_workspace(300, 2)
    assert _metrics(lib, ws_bytes=need - 1) == EWORKSPACE
    assert _metrics(lib, ws_bytes=0) == EWORKSPACE
    assert _metrics(lib, cutoffs=(1, 2, 3, 4, 5, 6, 7, 8), ws_bytes=need) == EWORKSPACE  # 8 cutoffs need 4 x as much


def test_workspace_queries_are_positive_and_monotone(lib):
    from xfmr_rec_amd import _native as N

    assert lib.xfmr_abi_version() == 3 == N.ABI_VERSION
    assert N.RANK_NONE == 2**31 - 1 == R.RANK_NONE and N.MAX_RANK_CUTOFFS == 8
    f = lib.xfmr_target_ranks_workspace
    assert f(0, 100, 10) == 0 and f(10, 0, 10) == 0 and f(10, 100, -1) == 0
    assert f(1, 2, 0) > 0  # no target at all is a valid input
    for B, V in [(1, 2), (257, 5000), (6040, 3900), (4096, 262_144)]:
        sizes = [f(B, V, t) for t in (0, 1, 100, 10_000, 1_000_000)]
        assert sizes[0] > 0 and all(b > a for a, b in zip(sizes, sizes[1:])), (B, V, sizes)
        # the per-entry arrays and one histogram bin per entry per catalogue slice (at least one slice)
        assert sizes[-1] >= 7 * 1_000_000 * 4
        assert sizes[-1] <= (6 + 16) * 1_000_000 * 4 + 4 * B
    g =lib.xfmr_rank_metrics_sum_workspace
    assert g(0, 1) == 0 and g(10, 0) == 0
    rows = [g(n, 3) for n in range(1, 70001, 257)]
    assert rows[0] >= 3 * 64 and all(b >= a for a, b in zip(rows, rows[1:])) and rows[-1] > rows[0]
    cuts = [g(1000, c) for c in range(1, 9)]
    assert all(b > a for a, b in zip(cuts, cuts[1:]))
    for n, c in ((1, 1), (256, 8), (257, 5), (65537, 8)):
        assert g(n, c) >= ((n + 255) // 256) * c * 64


# ------------------------------------------------------------------------------------ cutoffs and monitor names
def test_normalize_cutoffs():
    from xfmr_rec_amd.retrieval import normalize_cutoffs

    assert normalize_cutoffs((5, 10, 5, np.int64(20))) == (5, 10, 20)
    assert normalize_cutoffs(7) == (7,)
    assert normalize_cutoffs([500, 3]) == (500, 3)  # the order given is kept
    for bad in ((), (0,), (-1, 5), (2.5,), (True,), ("10",), (2**31,)):
        with pytest.raises(ValueError):
            normalize_cutoffs(bad)


def _trainer(**kw):
    import xfmr_rec_amd as X

    try:
        conf = X.LightningConfig(hidden_size=64, num_attention_heads=2, intermediate_size=128, num_hidden_layers=1,
                                 max_seq_length=8)
        return X.Trainer(X.RecommenderLightningModule(conf), **kw)
    except Exception as e:  # noqa: BLE001 - no device to build the model on
        pytest.skip(f"constructing a Trainer needs a device here: {e}")


def test_fit_monitor_names_with_a_cutoff():
    val = object()  # (never touched: no batch, so no pass)
    t = _trainer()
    name = "val/retrieval_normalized_dcg"
    assert t.fit([], val=val, val_check_interval=2, val_cutoffs=(10,), monitor={"name": name + "@10", "mode": "max"}) == []
    assert t.fit([], val=val, val_check_interval=2, val_cutoffs=(5, 10), monitor={"name": name, "mode": "max"}) == []
    assert t.val_history == [] and t.best_score is None
    for cutoffs, bad in (((10,), name + "@7"), (None, name + "@10"), ((10,), "val/nothing@10"), ((10,), "val/nothing"),
                         ((10,), name + "@"), ((10,), name + "@010"), ((10,), name + "@10@10"), ((10,), name + "@-10")):
        with pytest.raises(ValueError, match="monitor"):
            t.fit([], val=val, val_check_interval=2, val_cutoffs=cutoffs, monitor={"name": bad, "mode": "max"})
    with pytest.raises(ValueError, match="cutoffs"):
        t.fit([], val=val, val_cutoffs=(0,))
