"""Host side of validation inside ``Trainer.fit`` (no GPU): ``plan_eval_rows`` against a brute-force restatement, the
``EarlyStopping`` rule, ``xfmr_retrieval_metrics_sum``'s argument checks and workspace size, the header / binding of the
new entry points, and ``Trainer.fit``'s argument errors."""

import ctypes as C
import pathlib
import re

import numpy as np
import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]


# ---------------------------------------------------------------------------------------------------- plan_eval_rows
L = 8


def _rows():
    """Histories of lengths 0, 1, L-1, L, L+1 and 3L (twice each, one of each pair with an empty target list or not),
    items drawn from a small range so that every longer history holds duplicates."""
    rng = np.random.default_rng(0)
    hists, tgts = [], []
    for rep in range(3):
        for n in (0, 1, L - 1, L, L + 1, 3 * L):
            hists.append(rng.integers(1, 12, n).tolist())
            tgts.append(rng.integers(1, 12, int(rng.integers(1, 4))).tolist())
    tgts[3] = []             # a row with a history and no positive target
    tgts[10] = []
    hists[4] = [5, 5, 7, 5, 2, 2, 9, 1, 1]  # L + 1 entries with repeats: the truncation drops the first 5
    tgts[5] = [3, 3, 4]      # duplicate targets stay as given
    return hists, tgts


def _brute(hists, tgts, L, bs):
    kept = [i for i in range(len(hists)) if len(hists[i]) > 0 and len(tgts[i]) > 0]
    kept = sorted(kept, key=lambda i: -min(len(hists[i]), L))  # (sorted is stable)
    rows = [hists[i][-L:] for i in kept]
    chunks = [list(range(r0, min(r0 + bs, len(kept)))) for r0 in range(0, len(kept), bs)]
    return kept, rows, chunks


@pytest.mark.parametrize("bs", [1, 3, 64])
def test_plan_eval_rows_matches_brute_force(bs):
    from xfmr_rec_amd.evalset import plan_eval_rows

    hists, tgts = _rows()
    p = plan_eval_rows(hists, tgts, L, bs)
    kept, rows, chunks = _brute(hists, tgts, L, bs)
    assert 0 < len(kept) < len(hists)
    assert p.kept.dtype == np.int64 and p.kept.tolist() == kept  # the kept set, longest first, stable
    assert p.lengths.tolist() == [len(r) for r in rows]
    assert (np.diff(p.lengths) <= 0).all() and p.lengths.max() == L
    assert p.tok_offsets.tolist() == np.concatenate([[0], np.cumsum([len(r) for r in rows])]).tolist()
    assert p.hist.dtype == np.int64 and p.hist.tolist() == [x for r in rows for x in r]
    assert p.row_pos.dtype == np.int32 and p.row_pos.tolist() == [t for r in rows for t in range(len(r))]
    # exclusions: the sorted set of the FULL history; targets: as given
    assert p.excl_offsets.dtype == np.int64 and p.target_offsets.dtype == np.int64
    assert p.excl_offsets[0] == 0 and p.excl_offsets[-1] == p.excl.size
    assert p.target_offsets[0] == 0 and p.target_offsets[-1] == p.targets.size
    for i, src in enumerate(kept):
        assert p.excl[p.excl_offsets[i] : p.excl_offsets[i + 1]].tolist() == sorted(set(hists[src])), i
        assert p.targets[p.target_offsets[i] : p.target_offsets[i + 1]].tolist() == tgts[src], i
    assert any(len(set(hists[s])) < len(hists[s]) for s in kept)          # (duplicates were there to remove)
    assert any(set(hists[s]) != set(hists[s][-L:]) for s in kept)          # (and the full history differs from the kept part)
    # the chunks partition the rows, batch_size consecutive rows each
    assert [list(range(c.row0, c.row1)) for c in p.chunks] == chunks
    tok = 0
    for c in p.chunks:
        lens = [len(rows[i]) for i in range(c.row0, c.row1)]
        assert c.seq_offsets.dtype == np.int32 and c.seq_offsets[0] == 0
        assert c.seq_offsets.tolist() == np.concatenate([[0], np.cumsum(lens)]).tolist()
        assert (c.tok0, c.tok1) == (tok, tok + sum(lens)) and c.packed_rows == sum(lens) and c.max_len == max(lens)
        assert p.hist[c.tok0 : c.tok1].tolist() == [x for i in range(c.row0, c.row1) for x in rows[i]]
        tok += sum(lens)
    assert tok == p.hist.size


def test_plan_eval_rows_edge_cases():
    from xfmr_rec_amd.evalset import plan_eval_rows

    p = plan_eval_rows([[], [1]], [[2], []], L, 4)  # nothing counts
    assert p.kept.size == 0 and p.chunks == [] and p.hist.size == 0 and p.excl_offsets.tolist() == [0]
    p = plan_eval_rows([np.array([4, 4, 3])], [np.array([1])], 2, 1)  # array inputs
    assert p.kept.tolist() == [0] and p.hist.tolist() == [4, 3] and p.excl.tolist() == [3, 4]
    with pytest.raises(ValueError):
        plan_eval_rows([[1]], [[1], [2]], L, 4)
    with pytest.raises(ValueError):
        plan_eval_rows([[1]], [[1]], L, 0)


# ---------------------------------------------------------------------------------------------------- EarlyStopping
def test_early_stopping_rule():
    from xfmr_rec_amd.trainer import EarlyStopping

    es = EarlyStopping("max", patience=2, min_delta=0.0)
    assert [es.update(v) for v in (0.1, 0.1, 0.05)] == [False, False, True]  # an equal value is no improvement
    assert es.best == 0.1 and es.wait == 2
    es = EarlyStopping("max", patience=2, min_delta=0.0)
    assert [es.update(v) for v in (0.1, 0.1, 0.2, 0.2, 0.2)] == [False, False, False, False, True]  # 0.2 resets wait
    assert es.best == 0.2
    # min_delta: an improvement has to clear it
    es = EarlyStopping("max", patience=2, min_delta=0.05)
    assert [es.update(v) for v in (0.1, 0.14, 0.149)] == [False, False, True] and es.best == 0.1
    es = EarlyStopping("max", patience=2, min_delta=0.05)
    assert [es.update(v) for v in (0.1, 0.14, 0.16)] == [False, False, False] and es.best == 0.16 and es.improved
    # mode "min" is the mirror
    es = EarlyStopping("min", patience=2, min_delta=0.0)
    assert [es.update(v) for v in (0.5, 0.5, 0.6)] == [False, False, True] and es.best == 0.5
    es = EarlyStopping("min", patience=2, min_delta=0.05)
    assert [es.update(v) for v in (0.5, 0.46, 0.44)] == [False, False, False] and es.best == 0.44
    # patience 1: the first pass always improves; the loop stops at the second pass when that one does not improve (wait
    # reaches patience), not at the first
    es = EarlyStopping("max", patience=1)
    assert es.update(0.3) is False and es.improved
    assert es.update(0.3) is True and not es.improved
    es = EarlyStopping("max", patience=1)
    assert [es.update(v) for v in (0.3, 0.4, 0.5, 0.5)] == [False, False, False, True]
    # patience None only tracks the best; a NaN never improves
    es = EarlyStopping("max", patience=None)
    assert [es.update(v) for v in (0.3, float("nan"), 0.2)] == [False, False, False] and es.best == 0.3
    for bad in (dict(mode="up"), dict(patience=0), dict(min_delta=-1.0)):
        with pytest.raises(ValueError):
            EarlyStopping(**bad)


# ---------------------------------------------------------------------------------------------------- the C entry points
@pytest.fixture(scope="module")
def native():
    from xfmr_rec_amd import _native as N

    if not N.LIB_PATH.exists():
        pytest.fail(f"{N.LIB_PATH} missing: run build() first")
    return N


def test_metrics_sum_is_declared_and_bound(native):
    header = (ROOT / "include" / "xfmr_hip.h").read_text()
    for name in ("xfmr_retrieval_metrics_sum", "xfmr_retrieval_metrics_sum_workspace"):
        assert re.search(rf"\b{name}\s*\(", header), name
        assert name in native.EXPORTED_SYMBOLS
        fn = getattr(native.load(), name)
        assert fn.argtypes is not None and len(fn.argtypes) == {"xfmr_retrieval_metrics_sum": 13,
                                                                 "xfmr_retrieval_metrics_sum_workspace": 1}[name]
    assert native.load().xfmr_retrieval_metrics_sum_workspace.restype is C.c_size_t
    assert native.load().xfmr_abi_version() == 3


def test_metrics_sum_argument_checks_need_no_device(native):
    lib = native.load()
    buf = (C.c_double * 64)()  # host memory: every call below returns before any launch
    p = C.addressof(buf)
    n = 1000
    ws = lib.xfmr_retrieval_metrics_sum_workspace(n)
    assert ws > 0

    def call(rec=p, tgt=p, off=p, use=None, n_query=n, k=20, top_k=20, sums=p, out=None, valid=None, work=p, nbytes=None):
        return lib.xfmr_retrieval_metrics_sum(rec, tgt, off, use, n_query, k, top_k, sums, out, valid, work,
                                              ws if nbytes is None else nbytes, None)

    EINVAL, EUNSUPPORTED, EWORKSPACE = -1, -2, -3
    for kw in (dict(rec=None), dict(tgt=None), dict(off=None), dict(sums=None), dict(work=None), dict(n_query=0),
               dict(n_query=-5), dict(k=0), dict(top_k=0)):
        assert call(**kw) == EINVAL, kw
    assert call(nbytes=ws - 1) == EWORKSPACE
    assert call(nbytes=0) == EWORKSPACE
    assert call(n_query=1 << 31, nbytes=1 << 40) == EUNSUPPORTED


def test_metrics_sum_workspace_is_monotone(native):
    lib = native.load()
    assert lib.xfmr_retrieval_metrics_sum_workspace(0) == 0 and lib.xfmr_retrieval_metrics_sum_workspace(-1) == 0
    sizes = [lib.xfmr_retrieval_metrics_sum_workspace(n) for n in range(1, 70001, 257)]
    assert sizes[0] >= 64 and all(b >= a for a, b in zip(sizes, sizes[1:]))
    assert sizes[-1] > sizes[0]
    # one 8-double record per 256 rows at least (what the two kernels index)
    for n in (1, 256, 257, 65537):
        assert lib.xfmr_retrieval_metrics_sum_workspace(n) >= ((n + 255) // 256) * 64


# ---------------------------------------------------------------------------------------------------- Trainer.fit arguments
def _trainer(**kw):
    import xfmr_rec_amd as X

    try:
        conf = X.LightningConfig(hidden_size=64, num_attention_heads=2, intermediate_size=128, num_hidden_layers=1,
                                 max_seq_length=8)
        return X.Trainer(X.RecommenderLightningModule(conf), **kw)
    except Exception as e:  # noqa: BLE001 - no device to build the model on
        pytest.skip(f"constructing a Trainer needs a device here: {e}")


def test_fit_rejects_bad_validation_arguments_before_any_device_work():
    val = object()  # (never touched: the arguments are refused first)
    t = _trainer(accumulate_grad_batches=2)
    with pytest.raises(ValueError, match="multiple of accumulate_grad_batches"):
        t.fit([], val=val, val_check_interval=3)
    with pytest.raises(ValueError, match="val_check_interval"):
        t.fit([], val=val, val_check_interval=0)
    with pytest.raises(ValueError, match="early_stopping"):
        t.fit([], val=val, val_check_interval=2, early_stopping={"patience": 2, "tolerance": 0.1})
    with pytest.raises(ValueError, match="monitor"):
        t.fit([], val=val, val_check_interval=2, monitor={"name": "val/nothing", "mode": "max"})
    t2 = _trainer(world_size=2)
    with pytest.raises(ValueError, match="world_size"):
        t2.fit([], val=val)
    with pytest.raises(ValueError, match="world_size"):
        t2.validate(val)
