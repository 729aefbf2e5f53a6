"""The sampled-candidate protocol end to end on a small module: ``SampledEvalSet`` against the host reference
(``candidate_cases.rank_among_ref`` ranks, ``rank_refs.metrics_from_ranks`` metrics), against the full-catalogue set when
the negatives cover the catalogue, ``evaluate_sampled``, validation inside ``Trainer.fit``, and ``score_candidates``."""

import functools

import numpy as np
import pytest
import torch

import candidate_cases as CC
import rank_refs as R
from helpers import unit_table

pytestmark = pytest.mark.gpu
DEV = "cuda"
H_, A_, L_, V_, USERS = 64, 2, 24, 300, 40
CUT = (1, 10, 500)


def _module(top_k=20):
    import xfmr_rec_amd as X

    conf = X.LightningConfig(hidden_size=H_, num_attention_heads=A_, intermediate_size=2 * H_, num_hidden_layers=2,
                             max_seq_length=L_, top_k=top_k)
    mod = X.RecommenderLightningModule(conf)
    mod.configure_model()
    mod.model.set_table(unit_table(V_, H_, seed=3).to(DEV))
    mod.model.id2idx = {f"i{i}": i for i in range(1, V_ + 1)}
    return mod


def _val_rows(n=USERS, seed=4):
    rng = np.random.default_rng(seed)
    rows = []
    for u in range(n):
        h = [f"i{x}" for x in rng.integers(1, V_ + 1, int(rng.integers(1, 41)))]  # ragged, some longer than L_
        t = [f"i{x}" for x in rng.integers(1, V_ + 1, int(rng.integers(1, 4)))]
        lab = [True] * len(t)
        if u == 5:
            lab = [False] * len(t)  # a row without a target
        if u == 9:
            h = []  # an empty history
        if u == 13:
            t.append(h[0])  # a target inside the history: no rank
        if u == 17:
            t.append(t[0])  # a repeated target
        rows.append({"history": {"item_id": h}, "target": {"item_id": t, "label": lab}})
    return rows


@functools.lru_cache(maxsize=None)
def _sampled():
    import xfmr_rec_amd as X

    mod = _module()
    rows = _val_rows()
    return mod, rows, X.SampledEvalSet.from_rows(mod, rows, num_negatives=25, seed=11, batch_size=16)


def _row_lists(flat, off):
    flat, off = flat.cpu().numpy(), off.cpu().numpy()
    return [flat[off[i] : off[i + 1]].tolist() for i in range(off.size - 1)]


def test_sampled_set_equals_the_host_reference():
    """The device ranks equal ``rank_among_ref`` on the set's own score bits exactly. The metrics: the comparison of
    tests/test_gpu_target_ranks.py (``rank_metrics_sum`` against ``rank_refs``): per row float32 against the host
    reference's Python floats at rtol 1e-6, the fp64 sums against the per-row values summed in fp64 at 1e-12; the dict is
    those sums over the number of rows."""
    from xfmr_rec_amd.retrieval import METRIC_NAMES, rank_metrics_sum

    mod, rows, es = _sampled()
    assert (es.protocol, es.num_negatives, es.seed) == ("sampled", 25, 11)
    assert len(es) == USERS - 2 and len(es.plan.chunks) == 3
    cand, excl, tgts = (_row_lists(*x) for x in ((es.candidates, es.candidate_offsets), (es.excl, es.excl_offsets),
                                                 (es.targets, es.target_offsets)))
    for c, x, t in zip(cand, excl, tgts):  # 25 distinct negatives outside the history and the targets
        assert len(c) == 25 and c == sorted(set(c)) and not set(c) & (set(x) | set(t)) and 1 <= c[0] and c[-1] <= V_
    emb = es.encode()
    n = len(es)
    items = torch.arange(1, V_ + 1, dtype=torch.int64, device=DEV).repeat(n)
    off = torch.arange(0, n + 1, dtype=torch.int64, device=DEV) * V_
    _, score = mod.items_index.rank_targets(emb, (items, off), None, return_scores=True)
    s_all = np.concatenate([np.full((n, 1), np.nan), score.view(n, V_).cpu().numpy().astype(np.float64)], axis=1)
    want = [CC.rank_among_ref(s_all[b], cand[b], excl[b], tgts[b])[0] for b in range(n)]
    ranks = es.target_ranks()
    assert ranks.dtype == torch.int32 and ranks.cpu().numpy().tolist() == [r for w in want for r in w]
    assert sum(r == R.RANK_NONE for w in want for r in w) >= 1  # the target inside its row's history
    assert max(r for w in want for r in w if r != R.RANK_NONE) <= 25 + 4  # ranked among the negatives, not the catalogue

    ev = es.evaluate(cutoffs=CUT)
    cut = CUT + (20,)  # config.top_k joins the cutoffs and gives the plain keys
    assert set(ev) == ({f"val/{m}" for m in METRIC_NAMES} | {"val/num_rows"} | {f"val/{m}@{K}" for m in METRIC_NAMES for K in cut})
    sums, vals, valid = rank_metrics_sum(ranks, (es.targets, es.target_offsets), cut, per_row=True)
    vals_np, sums_np = vals.cpu().numpy(), sums.cpu().numpy()
    assert bool(valid.all()) and ev["val/num_rows"] == n
    worst = 0.0
    for ci, K in enumerate(cut):
        ref = np.asarray([[R.metrics_from_ranks(want[b], tgts[b], K)[m] for m in R.NAMES] for b in range(n)])
        err = np.abs(vals_np[:, ci] - ref) / np.maximum(np.abs(ref), 1e-300)
        worst = max(worst, float(err[ref != 0].max()))
        np.testing.assert_allclose(vals_np[:, ci], ref, rtol=1e-6, atol=0, err_msg=f"K={K}")
        np.testing.assert_allclose(sums_np[ci, :7], vals_np[:, ci].astype(np.float64).sum(axis=0), rtol=1e-12, atol=0)
        assert sums_np[ci, 7] == n
        for i, m in enumerate(METRIC_NAMES):
            assert ev[f"val/{m}@{K}"] == sums_np[ci, i] / n, (m, K)
            np.testing.assert_allclose(ev[f"val/{m}@{K}"], ref[:, i].mean(), rtol=1e-6, atol=0, err_msg=f"{m}@{K}")
            if K == 20:
                assert ev[f"val/{m}"] == ev[f"val/{m}@20"]
    print(f"worst per-row relative difference {worst:.3e} (limit 1e-6)")
    assert ev["val/retrieval_hit_rate@1"] < ev["val/retrieval_hit_rate@10"] <= ev["val/retrieval_hit_rate@500"]
    # the default cutoffs are (config.top_k,); a stage name is honoured; the full-catalogue list path is not this set's
    plain = es.evaluate("test")
    assert set(plain) == {f"test/{m}" for m in METRIC_NAMES} | {"test/num_rows"} | {f"test/{m}@20" for m in METRIC_NAMES}
    assert plain["test/retrieval_normalized_dcg"] == ev["val/retrieval_normalized_dcg@20"]
    with pytest.raises(ValueError):
        es.recommend()


def test_negatives_that_cover_the_catalogue_give_the_full_catalogue_set():
    import xfmr_rec_amd as X

    mod, rows, _ = _sampled()
    every = X.SampledEvalSet.from_rows(mod, rows, num_negatives=V_ + 50, seed=2, batch_size=16)
    full = X.DeviceEvalSet.from_rows(mod, rows, batch_size=16)
    got, want = every.evaluate(cutoffs=CUT), full.evaluate(cutoffs=CUT)
    assert set(got) == set(want)
    for k in want:
        assert got[k] == want[k], (k, got[k], want[k])  # value for value
    assert torch.equal(every.target_ranks(), full.target_ranks())
    # fewer negatives: easier, and a different set of numbers
    few = _sampled()[2].evaluate(cutoffs=CUT)
    assert few["val/retrieval_hit_rate@10"] > want["val/retrieval_hit_rate@10"]


def test_evaluate_sampled_is_the_sets_result_and_explicit_candidates():
    import xfmr_rec_amd as X

    mod, rows, es = _sampled()
    assert mod.evaluate_sampled(rows, num_negatives=25, seed=11, cutoffs=CUT, batch_size=16) == es.evaluate(cutoffs=CUT)
    assert mod.evaluate_sampled(rows, num_negatives=25, seed=11, stage="test", batch_size=16) == es.evaluate("test")
    other = mod.evaluate_sampled(rows, num_negatives=25, seed=12, cutoffs=CUT, batch_size=16)
    assert other != es.evaluate(cutoffs=CUT) and other["val/num_rows"] == len(es)
    # weights: an item of weight 0 is never a negative
    w = np.zeros(V_ + 1)
    w[1::2] = 1.0
    odd = X.SampledEvalSet.from_rows(mod, rows, num_negatives=25, seed=11, weights=w, batch_size=16)
    assert bool((odd.candidates % 2 == 1).all()) and odd.candidates.numel() == 25 * len(odd)
    # explicit candidates, as ids: the set's own negatives handed back give the set's result; unknown ids are dropped
    lists = _row_lists(es.candidates, es.candidate_offsets)
    given = [["nope"] for _ in rows]
    for i, r in enumerate(es.kept):
        given[r] = [f"i{x}" for x in reversed(lists[i])] + ["ghost", f"i{lists[i][0]}"]
    ex = X.SampledEvalSet.from_rows(mod, rows, candidates=given, batch_size=16)
    assert ex.protocol == "candidates" and ex.num_negatives is None
    assert torch.equal(ex.candidates, es.candidates) and torch.equal(ex.candidate_offsets, es.candidate_offsets)
    assert ex.evaluate(cutoffs=CUT) == es.evaluate(cutoffs=CUT)
    with pytest.raises(ValueError):
        X.SampledEvalSet.from_rows(mod, rows, candidates=given[:-1])


def test_world_size_above_one_is_refused():
    import xfmr_rec_amd as X

    mod, rows, _ = _sampled()
    with pytest.raises(ValueError, match="world_size"):
        X.SampledEvalSet.from_rows(mod, rows, world_size=2)
    with pytest.raises(ValueError, match="world_size"):
        X.SampledEvalSet.from_rows(mod, rows, rank=1, world_size=2)


def test_fit_validates_on_a_sampled_set():
    import xfmr_rec_amd as X

    g = torch.Generator().manual_seed(0)
    batches = []
    for i in range(6):
        b = {k: torch.randint(1, V_ + 1, (8, L_), generator=g) for k in ("history_item_idx", "pos_item_idx", "neg_item_idx")}
        for k in b:
            b[k][1, 5 + 2 * i:] = 0  # one ragged row
        batches.append({k: v.to(DEV) for k, v in b.items()})
    mod = _module()
    es = X.SampledEvalSet.from_rows(mod, _val_rows(), num_negatives=25, seed=11, batch_size=16)
    tr = X.Trainer(mod)
    name = "val/retrieval_normalized_dcg@10"
    tr.fit(batches, val=es, val_check_interval=2, val_cutoffs=(10,), monitor={"name": name, "mode": "max"},
           early_stopping=True)
    torch.cuda.synchronize()
    steps = [h["step"] for h in tr.val_history]
    assert steps and steps == list(range(2, 2 * len(steps) + 1, 2)) and steps[-1] <= 6
    for h in tr.val_history:
        assert {name, "val/retrieval_hit_rate@10", "val/retrieval_normalized_dcg", "val/num_rows"} <= set(h)
        assert h["val/num_rows"] == len(es) and 0.0 <= h[name] <= 1.0
    assert tr.best_score == max(h[name] for h in tr.val_history)
    assert mod.logged[name] == tr.val_history[-1][name]
    assert tr.val_history[-1] | {"step": 0} == es.evaluate(cutoffs=(10,)) | {"step": 0}  # the pass fit ran is the set's


def test_score_candidates_orders_by_score_with_the_tiled_bits():
    mod, rows, _ = _sampled()
    hists = [r["history"]["item_id"] for r in rows[:12]]
    emb = mod.model.encode_batch([mod._to_idx_or_empty(list(h)) for h in hists])
    idx, score = mod.items_index.search_batch(emb, None, top_k=128)  # xfmr_topk_tiled: the 128 best items of each user
    idx, score = idx.cpu().numpy(), score.cpu().numpy()
    rng = np.random.default_rng(0)
    given = []
    for b in range(len(hists)):
        c = [f"i{x}" for x in rng.permutation(idx[b][idx[b] > 0])[:60]] + [f"i{x}" for x in rng.integers(1, V_ + 1, 30)]
        given.append(c[:7] + ["unknown-id"] + c[7:] + c[:3])  # an id that is no item; three given twice
    got = mod.score_candidates(hists, given)
    assert len(got) == len(hists)
    n_bits = 0
    for b, (ids, s) in enumerate(got):
        if not hists[b]:
            assert ids == [] and len(s) == 0
            continue
        assert s.dtype == np.float32 and len(ids) == len(s) == len(set(given[b]) - {"unknown-id"})
        rows_of = [int(i[1:]) for i in ids]
        assert set(ids) == set(given[b]) - {"unknown-id"}
        order = np.lexsort((np.asarray(rows_of), -s.astype(np.float64)))  # score descending, then table row
        assert order.tolist() == list(range(len(ids))), b
        place = {int(i): p for p, i in enumerate(idx[b])}
        listed = [(place[r], x) for x, r in enumerate(rows_of) if r in place]
        assert [x for _, x in sorted(listed)] == sorted(x for _, x in listed)  # the tiled list's order
        for p, x in listed:
            assert s[x].view(np.uint32) == score[b, p].view(np.uint32), (b, ids[x], s[x], score[b, p])
            n_bits += 1
    assert n_bits > 500
