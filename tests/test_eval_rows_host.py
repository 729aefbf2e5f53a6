"""``xfmr_rec_amd.eval_rows`` (no GPU): the one row reader, CSR builder, padded array, cutoff rule, result table, refusal and
eval-mode guard, each against the rules it replaced -- restated here as they stood in ``trainer.py``, ``evalset.py``,
``retrieval.py`` and ``models.py`` before the module existed."""

import math
import pathlib
import subprocess
import sys

import numpy as np
import pytest
import torch

from test_evalset_host import L as PLAN_L
from test_evalset_host import _rows as plan_rows

ROOT = pathlib.Path(__file__).resolve().parents[1]


# ---------------------------------------------------------------------------------------------------- the old rules
def old_retrieval_flat_csr(rows):  # retrieval._flat_csr: one placeholder element only when the CSR is empty
    off = np.zeros(len(rows) + 1, dtype=np.int64)
    np.cumsum([len(r) for r in rows], out=off[1:])
    flat = np.concatenate(rows) if off[-1] else np.zeros(1, dtype=np.int64)
    return flat, off


def old_sorted_exclusion_csr(lists):  # retrieval.sorted_exclusion_csr: np.unique per list
    return old_retrieval_flat_csr([np.unique(np.asarray(x, dtype=np.int64).reshape(-1)) for x in lists])


def old_evalset_flat(lists, rows):  # evalset._flat: no placeholder
    lens = np.asarray([len(lists[r]) for r in rows], dtype=np.int64)
    off = np.zeros(len(rows) + 1, dtype=np.int64)
    np.cumsum(lens, out=off[1:])
    parts = [np.asarray(lists[r], dtype=np.int64).reshape(-1) for r in rows]
    flat = np.concatenate(parts) if off[-1] else np.zeros(0, dtype=np.int64)
    return flat, off


def old_trainer_targets_csr(tgts):  # trainer._evaluate_ranks, inline: always one trailing element
    tg = np.concatenate([np.asarray(t, dtype=np.int64).reshape(-1) for t in tgts] + [np.zeros(1, dtype=np.int64)])
    tgo = np.zeros(len(tgts) + 1, dtype=np.int64)
    np.cumsum([len(t) for t in tgts], out=tgo[1:])
    return tg, tgo


def old_plan_exclusions(full, full_off):  # evalset.plan_eval_rows: one lexsort over (row, item) pairs
    n = full_off.size - 1
    row_of_full = np.repeat(np.arange(n, dtype=np.int64), np.diff(full_off))
    o = np.lexsort((full, row_of_full))
    fs, rs = full[o], row_of_full[o]
    first = np.ones(fs.size, dtype=bool)
    first[1:] = (fs[1:] != fs[:-1]) | (rs[1:] != rs[:-1])
    excl_off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(rs[first], minlength=n), out=excl_off[1:])
    return fs[first], excl_off


CSR_INPUTS = {
    "duplicates and empty lists": [[9, 3, 3, 7], [], [5], [2, 2, 2], [-1, 100, 4], []],
    "all empty": [[], [], []],
    "no list": [],
    "negative and large": [[-5, 2**40, -5, 2**62, 0], [2**31, 2**31 - 1, -(2**40)]],
    "a numpy array as a list": [np.array([4, 4, 3]), [1], np.zeros(0, dtype=np.int64), np.array([8, 6, 6, 8], dtype=np.int32)],
    "leading and trailing empty": [[], [3, 1], []],
}


@pytest.mark.parametrize("name", list(CSR_INPUTS))
def test_flat_csr_against_the_three_old_builders(name):
    from xfmr_rec_amd.eval_rows import flat_csr

    lists = CSR_INPUTS[name]
    flat, off = flat_csr(lists)
    n = int(off[-1])
    assert flat.dtype == np.int64 and off.dtype == np.int64 and off.shape == (len(lists) + 1,)
    # the settled trailing-element rule: exactly the entries, one placeholder element only when there is none
    assert flat.size == max(n, 1)
    arrays = [np.asarray(x, dtype=np.int64).reshape(-1) for x in lists]
    for (want, want_off), exact in ((old_retrieval_flat_csr(arrays), True),
                                    (old_evalset_flat(lists, range(len(lists))), False),
                                    (old_trainer_targets_csr(lists), False)):
        assert off.tolist() == want_off.tolist()
        assert flat[:n].tolist() == want[:n].tolist()  # every element a kernel can read
        if exact:
            assert flat.tolist() == want.tolist()
    # sort_unique: np.unique per list, and the plan's lexsort
    sflat, soff = flat_csr(lists, sort_unique=True)
    want, want_off = old_sorted_exclusion_csr(lists)
    assert sflat.dtype == np.int64 and soff.dtype == np.int64
    assert soff.tolist() == want_off.tolist() and sflat.tolist() == want.tolist()
    for i, x in enumerate(arrays):
        assert sflat[soff[i] : soff[i + 1]].tolist() == np.unique(x).tolist()
    lex, lex_off = old_plan_exclusions(*old_evalset_flat(lists, range(len(lists))))
    assert soff.tolist() == lex_off.tolist() and sflat[: soff[-1]].tolist() == lex.tolist()


def test_flat_csr_on_the_plan_rows_and_through_its_callers():
    from xfmr_rec_amd.eval_rows import flat_csr
    from xfmr_rec_amd.evalset import plan_eval_rows
    from xfmr_rec_amd.retrieval import sorted_exclusion_csr

    hists, tgts = plan_rows()
    kept = [i for i in range(len(hists)) if hists[i] and tgts[i]]
    full, full_off = old_evalset_flat(hists, kept)
    want, want_off = old_plan_exclusions(full, full_off)
    got, got_off = flat_csr([hists[i] for i in kept], sort_unique=True)
    assert got.tolist() == want.tolist() and got_off.tolist() == want_off.tolist()
    pub, pub_off = sorted_exclusion_csr([hists[i] for i in kept])
    assert pub.tolist() == want.tolist() and pub_off.tolist() == want_off.tolist()
    plan = plan_eval_rows(hists, tgts, PLAN_L, 4)
    order = plan.kept.tolist()
    for arr, off, (w, w_off) in ((plan.excl, plan.excl_offsets, old_plan_exclusions(*old_evalset_flat(hists, order))),
                                 (plan.targets, plan.target_offsets, old_evalset_flat(tgts, order))):
        assert arr.dtype == w.dtype and arr.tolist() == w.tolist() and off.tolist() == w_off.tolist()
    empty = plan_eval_rows([[], [1]], [[2], []], PLAN_L, 4)  # a plan holds its entries and nothing else
    assert empty.excl.size == empty.targets.size == empty.hist.size == 0 and empty.target_pos.size == 0


# ---------------------------------------------------------------------------------------------------- ids and rows
class CountingDict(dict):
    """A dict ``id2idx`` that counts what is asked of it, per id."""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.contains, self.getitem = {}, {}

    def __contains__(self, key):
        self.contains[key] = self.contains.get(key, 0) + 1
        return super().__contains__(key)

    def __getitem__(self, key):
        self.getitem[key] = self.getitem.get(key, 0) + 1
        return super().__getitem__(key)


class ModuleStandIn:
    """``RecommenderLightningModule``'s id conversion without a device: the same two methods over ``model.id2idx``."""

    def __init__(self, id2idx):
        from xfmr_rec_amd.trainer import RecommenderLightningModule as M

        self.model = type("Model", (), {"id2idx": id2idx})()
        self._to_idx = M._to_idx.__get__(self)
        self._to_idx_or_empty = M._to_idx_or_empty.__get__(self)


def old_to_idx(id2idx, item_ids):  # trainer._to_idx
    if len(item_ids) and not isinstance(item_ids[0], (str, bytes)):
        return [int(i) for i in item_ids]
    if hasattr(id2idx, "index"):
        return [int(id2idx[i]) for i in item_ids if i in id2idx.index]
    return [int(id2idx[i]) for i in item_ids if i in id2idx]


def old_to_idx_or_empty(id2idx, item_ids):
    return old_to_idx(id2idx, item_ids) if len(item_ids) else []


def _reader_rows():
    """Distinct ids per row (so that per-id counts are per use): labels all false, targets with unknown ids, an empty
    history, a history of unknown ids only, integer ids."""
    def row(h, t, lab):
        return {"history": {"item_id": h}, "target": {"item_id": t, "label": lab}}

    return [
        row(["i1", "i2", "i3"], ["i4", "i5"], [True, False]),
        row(["i6", "i7"], ["i8", "i9"], [False, False]),                   # labels all false
        row(["i10", "nope-a", "i11"], ["nope-b", "i12"], [True, True]),    # unknown ids on both sides
        row([], ["i13"], [True]),                                          # an empty history
        row(["nope-c", "nope-d"], ["i14"], [True]),                        # a history of unknown ids only
        row([21, 22, 23], [24, 25], [True, True]),                         # integer ids are rows already
        row(np.array(["i15", "i16"]), np.array(["i17"]), np.array([True])),  # array columns, as a dataframe gives them
    ]


def _check_reader(make_id2idx, count):
    from xfmr_rec_amd.eval_rows import positive_target_ids, read_rows

    rows = _reader_rows()
    plain = make_id2idx()
    mod = ModuleStandIn(make_id2idx())
    hists, tgts = read_rows(rows, mod._to_idx_or_empty)
    # the four parent expressions: evaluate, _evaluate_ranks, from_rows (the same two comprehensions) and compute_metrics
    want_h = [old_to_idx_or_empty(plain, list(r["history"]["item_id"])) for r in rows]
    want_t = [old_to_idx_or_empty(plain, [i for i, l in zip(r["target"]["item_id"], r["target"]["label"]) if l]) for r in rows]
    assert hists == want_h and tgts == want_t
    assert hists[3] == [] and hists[4] == [] and tgts[1] == [] and hists[5] == [21, 22, 23] and tgts[2] == [12]
    assert all(type(x) is int for lst in hists + tgts for x in lst)
    for r in rows:
        ids = positive_target_ids(r)
        assert list(ids) == [i for i, l in zip(r["target"]["item_id"], r["target"]["label"]) if l]
        assert mod._to_idx(ids) == old_to_idx(plain, ids)
    if count:
        # every id of the rows went through the lookup once: one membership test each, one read per known id
        mod = ModuleStandIn(make_id2idx())
        read_rows(rows, mod._to_idx_or_empty)
        d = mod.model.id2idx
        asked = [str(i) for r in rows for i in list(r["history"]["item_id"]) + positive_target_ids(r) if isinstance(i, str)]
        assert len(asked) == len(set(asked)) and "nope-a" in asked and "i5" not in asked
        assert d.contains == {i: 1 for i in asked}
        assert d.getitem == {i: 1 for i in asked if not i.startswith("nope")}


def test_read_rows_with_a_dict():
    _check_reader(lambda: CountingDict({f"i{i}": i for i in range(1, 30)}), count=True)


def test_read_rows_with_a_series():
    pd = pytest.importorskip("pandas", reason="the pandas Series half of the id lookup needs pandas")
    _check_reader(lambda: pd.Series(range(1, 30), index=[f"i{i}" for i in range(1, 30)]), count=False)


def test_lookup_rows_is_what_model_encode_did():
    from xfmr_rec_amd.eval_rows import lookup_rows

    d = {f"i{i}": i for i in range(1, 30)}
    ids = ["i3", "nope", "i3", "i29"]
    known = [i for i in ids if i in d]  # models.RecommenderModel.encode
    assert lookup_rows(d, ids) == [d[i] for i in known] == [3, 3, 29]
    assert lookup_rows(d, []) == []


# ---------------------------------------------------------------------------------------------------- the result table
NAMES = ("retrieval_normalized_dcg", "retrieval_average_precision", "retrieval_auroc", "retrieval_precision",
         "retrieval_recall", "retrieval_hit_rate", "retrieval_reciprocal_rank")


def test_metric_names_are_one_tuple():
    from xfmr_rec_amd import eval_rows, retrieval

    assert eval_rows.METRIC_NAMES == NAMES and retrieval.METRIC_NAMES is eval_rows.METRIC_NAMES


def _same(got, want):
    assert list(got) == list(want)  # the keys, in insertion order
    for k, w in want.items():
        g = got[k]
        assert type(g) is type(w), (k, type(g))
        assert (math.isnan(g) and math.isnan(w)) or g == w, (k, g, w)


def test_metrics_dict_one_row_of_sums():
    from xfmr_rec_amd.eval_rows import metrics_dict

    s = [1.5, 2.25, 3.0, 0.1, 0.7, 3.0, 1.0 / 3.0, 3.0]
    want = {"val/retrieval_normalized_dcg": 1.5 / 3, "val/retrieval_average_precision": 2.25 / 3, "val/retrieval_auroc": 3.0 / 3,
            "val/retrieval_precision": 0.1 / 3, "val/retrieval_recall": 0.7 / 3, "val/retrieval_hit_rate": 3.0 / 3,
            "val/retrieval_reciprocal_rank": (1.0 / 3.0) / 3, "val/num_rows": 3}
    _same(metrics_dict("val", s, top_k=20), want)
    _same(metrics_dict("val", np.asarray(s), top_k=20), want)   # module.evaluate hands numpy sums, the set a list
    _same(metrics_dict("val", s), want)
    nan = float("nan")
    _same(metrics_dict("test", [0.0] * 8, top_k=20), {**{f"test/{n}": nan for n in NAMES}, "test/num_rows": 0})


@pytest.mark.parametrize("cutoffs,top_k", [((20, 5, 500), 20), ((5, 20, 500), 20), ((5, 500, 20), 20), ((20,), 20)])
def test_metrics_dict_with_cutoffs(cutoffs, top_k):
    """``top_k`` the first, a middle and the last cutoff: the plain keys and num_rows stand right behind its ``@K`` keys."""
    from xfmr_rec_amd.eval_rows import metrics_dict

    rng = np.random.default_rng(len(cutoffs) + cutoffs[0])
    sums = rng.random((len(cutoffs), 8))
    sums[:, 7] = [4 + i for i in range(len(cutoffs))]
    if len(cutoffs) > 1:
        sums[1] = 0.0  # a cutoff at which no row counts
    want = {}
    for K, s in zip(cutoffs, sums):  # the parent's loop (trainer._evaluate_ranks / DeviceEvalSet.evaluate)
        n = int(s[7])
        for i, name in enumerate(NAMES):
            want[f"val/{name}@{K}"] = float(s[i] / n) if n else float("nan")
        if K == top_k:
            for i, name in enumerate(NAMES):
                want[f"val/{name}"] = want[f"val/{name}@{K}"]
            want["val/num_rows"] = n
    assert list(want)[: 7] == [f"val/{n}@{cutoffs[0]}" for n in NAMES]
    _same(metrics_dict("val", sums, cutoffs, top_k), want)
    _same(metrics_dict("val", sums.tolist(), cutoffs, top_k), want)
    at = list(want).index(f"val/retrieval_reciprocal_rank@{top_k}")
    assert list(want)[at + 1 : at + 9] == [f"val/{n}" for n in NAMES] + ["val/num_rows"]


def test_metrics_dict_with_cutoffs_against_literal_dicts():
    from xfmr_rec_amd.eval_rows import metrics_dict

    nan = float("nan")
    two = [[2.0, 1.0, 4.0, 0.5, 3.0, 4.0, 0.25, 4.0], [0.0] * 8]  # the second cutoff: no row counts

    def at(K, v):
        return {f"val/{n}@{K}": x for n, x in zip(NAMES, v)}

    def plain(v, n):
        return {**{f"val/{m}": x for m, x in zip(NAMES, v)}, "val/num_rows": n}

    first = [0.5, 0.25, 1.0, 0.125, 0.75, 1.0, 0.0625]
    # top_k the first cutoff: the plain keys and num_rows stand between the two cutoffs' keys
    _same(metrics_dict("val", two, (20, 5), 20), {**at(20, first), **plain(first, 4), **at(5, [nan] * 7)})
    # top_k the last cutoff, and no row counting at it: NaN plain keys, num_rows 0
    _same(metrics_dict("val", two, (5, 20), 20), {**at(5, first), **at(20, [nan] * 7), **plain([nan] * 7, 0)})
    # top_k NOT among the cutoffs (callers append it with eval_cutoffs; the table itself adds nothing): no plain keys
    got = metrics_dict("val", two, (5, 500), 20)
    _same(got, {**at(5, first), **at(500, [nan] * 7)})
    assert "val/num_rows" not in got and len(got) == 14
    # ... and what the callers hand over in that case
    three = two + [[1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 2.0]]
    _same(metrics_dict("test", three, eval_cutoffs_of((5, 500), 20), 20),
          {**{k.replace("val/", "test/"): v for k, v in {**at(5, first), **at(500, [nan] * 7), **at(20, [0.5] * 7)}.items()},
           **{k.replace("val/", "test/"): v for k, v in plain([0.5] * 7, 2).items()}})


def eval_cutoffs_of(cutoffs, top_k):
    from xfmr_rec_amd.eval_rows import eval_cutoffs

    return eval_cutoffs(cutoffs, top_k)


def test_eval_cutoffs_rule():
    from xfmr_rec_amd.eval_rows import eval_cutoffs, normalize_cutoffs

    assert eval_cutoffs((5, 20, 500), 20) == (5, 20, 500)       # top_k among them: as given
    assert eval_cutoffs((5, 500), 20) == (5, 500, 20)           # missing: appended
    assert eval_cutoffs((20, 5, 5), 20) == (20, 5) and eval_cutoffs(7, 20) == (7, 20)
    assert eval_cutoffs(np.int64(20), np.int64(20)) == (20,) and type(eval_cutoffs((5,), np.int64(9))[1]) is int
    for bad in ((), (0,), (True,), (2.0,), (2**31,)):
        with pytest.raises(ValueError):
            eval_cutoffs(bad, 20)
        with pytest.raises(ValueError):
            normalize_cutoffs(bad)


def test_tiled_top_k_refusal():
    from xfmr_rec_amd.eval_rows import check_tiled_top_k

    check_tiled_top_k(1)
    check_tiled_top_k(128)
    with pytest.raises(ValueError, match=r"top_k = 129: the tiled top-k \(xfmr_topk_tiled\) returns at most 128 items per row$"):
        check_tiled_top_k(129)
    with pytest.raises(ValueError, match="top_k = 500: .* per row; evaluate it with cutoffs"):
        check_tiled_top_k(500, "; evaluate it with cutoffs")


# ---------------------------------------------------------------------------------------------------- the padded array
@pytest.mark.parametrize("lengths", [[5, 1, 5, 3, 5], [1], [4, 4], [1, 1, 2]])
def test_pad_histories_against_the_two_old_expressions(lengths):
    from xfmr_rec_amd.eval_rows import pad_histories

    rng = np.random.default_rng(sum(lengths))
    rows = [rng.integers(1, 50, n).tolist() for n in lengths]
    Lmax = max(lengths)
    # models.encode_batch
    lens_np = np.asarray(lengths, dtype=np.int64)
    hist_np = np.zeros((len(rows), Lmax), dtype=np.int64)
    hist_np[np.arange(Lmax)[None, :] < lens_np[:, None]] = np.concatenate([np.asarray(r, dtype=np.int64) for r in rows])
    # evalset.DeviceEvalSet.__init__ (a chunk of the plan: lengths non-increasing, the first the longest)
    order = np.argsort(-lens_np, kind="stable")
    flat_sorted = np.concatenate([np.asarray(rows[i], dtype=np.int64) for i in order])
    pad = np.zeros((len(rows), int(lens_np[order][0])), dtype=np.int64)
    pad[np.arange(pad.shape[1])[None, :] < lens_np[order][:, None]] = flat_sorted
    got = pad_histories(lengths, np.concatenate([np.asarray(r, dtype=np.int64) for r in rows]))
    assert got.dtype == np.int64 and got.shape == (len(rows), Lmax) and np.array_equal(got, hist_np)
    assert np.array_equal(pad_histories(lens_np[order], flat_sorted), pad)
    for b, r in enumerate(rows):
        assert got[b].tolist() == r + [0] * (Lmax - len(r))


# ---------------------------------------------------------------------------------------------------- the eval-mode guard
@pytest.mark.parametrize("was_training", [True, False])
def test_eval_mode_guard_restores_the_flag(was_training):
    from xfmr_rec_amd.eval_rows import eval_mode
    from xfmr_rec_amd.models import RecommenderModel

    m = torch.nn.Linear(2, 2)
    m.train(was_training)
    with eval_mode(m) as inside:
        assert inside is m and not m.training
    assert m.training is was_training
    with pytest.raises(KeyError):
        with eval_mode(m):
            assert not m.training
            raise KeyError("a pass that fails")
    assert m.training is was_training
    with RecommenderModel.eval_mode(m):  # the method on the model is the same guard
        assert not m.training
    assert m.training is was_training


# ---------------------------------------------------------------------------------------------------- imports
def test_eval_rows_needs_neither_the_native_library_nor_torch():
    """The package's ``__init__`` imports every module (``_native`` among them), so the module is loaded alone, from its
    file and under its own name: it must import without the package around it, and bring in neither ``_native`` nor torch."""
    path = ROOT / "transformer-recommenders_amd" / "xfmr_rec_amd" / "eval_rows.py"
    code = (
        "import importlib.util, sys\n"
        f"spec = importlib.util.spec_from_file_location('xfmr_rec_amd.eval_rows', {str(path)!r})\n"
        "mod = importlib.util.module_from_spec(spec)\n"
        "sys.modules[spec.name] = mod\n"
        "spec.loader.exec_module(mod)\n"
        "assert mod.flat_csr([[2, 1, 2]], sort_unique=True)[0].tolist() == [1, 2]\n"
        "bad = sorted(m for m in sys.modules if m == 'torch' or m.startswith('xfmr_rec_amd.') and m != spec.name)\n"
        "assert not bad, bad\n"
        "print('ok')\n"
    )
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr
