"""The rank path of validation: xfmr_target_ranks against numpy ranks on exact inputs, its scores against the tiled
search's, xfmr_rank_metrics_sum against the list path (bits, K <= 128) and against the host reference (any K), and the
Python surface end to end (``DeviceEvalSet.evaluate(cutoffs=)``, ``Trainer.fit(val_cutoffs=)``, ``top_k`` above 128)."""

import functools

import numpy as np
import pytest
import torch

import rank_refs as R
from helpers import unit_table

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = [(1, 2, 4), (33, 389, 12), (257, 5000, 64)]  # partial query tiles, a partial last item tile, several slices, H % 8 != 0
METRICS = ["dot", "l2"]


def _csr(lists, dev=DEV):
    off = np.zeros(len(lists) + 1, dtype=np.int64)
    np.cumsum([len(x) for x in lists], out=off[1:])
    flat = np.concatenate([np.asarray(x, dtype=np.int64).reshape(-1) for x in lists] + [np.zeros(1, dtype=np.int64)])
    return torch.from_numpy(flat).to(dev), torch.from_numpy(off).to(dev)


@functools.lru_cache(maxsize=None)
def _exact_case(n_query, n_rows, H, metric):
    """Integer entries in [-3, 3]: every dot product is exact in fp32 in any order. Duplicated rows (ties), one row with an
    inf, exclusion lists with repeats and ids >= n_rows, targets that are excluded / repeated / 0 / >= n_rows, a row with
    300 targets and one with none. The numpy ranks are computed once and shared."""
    rng = np.random.default_rng(1000 * n_query + n_rows + H)
    table = rng.integers(-3, 4, (n_rows, H)).astype(np.float32)
    for _ in range(n_rows // 6):
        table[int(rng.integers(1, n_rows))] = table[int(rng.integers(1, n_rows))]
    inf_row = None
    if n_rows > 10:
        inf_row = int(rng.integers(1, n_rows))
        table[inf_row, int(rng.integers(0, H))] = np.inf
    query = rng.integers(-3, 4, (n_query, H)).astype(np.float32)
    excl, tgts = [], []
    for b in range(n_query):
        ex = rng.integers(1, n_rows + 3, int(rng.integers(0, 12)))
        ex = np.sort(np.concatenate([ex, ex[: ex.size // 3]]))  # repeats; sorted ascending, as the kernel needs
        t = rng.integers(1, n_rows, int(rng.integers(1, 7))).tolist()
        if ex.size and b % 3 == 0:
            t[0] = int(ex[0])  # an excluded target (or one past the table)
        if b % 4 == 1:
            t.append(t[0])  # a repeated target
        if b % 5 == 2:
            t.append(0)  # the padding row
        if b % 7 == 3:
            t.append(n_rows + int(rng.integers(0, 5)))  # past the table
        if inf_row is not None and b % 6 == 4:
            t.append(inf_row)
        excl.append(ex.tolist())
        tgts.append(t)
    tgts[0] = rng.integers(0, n_rows + 2, 300).tolist()  # more than one histogram chunk, ids 0 and >= n_rows among them
    if n_query > 1:
        tgts[1] = []
    want = [R.ranks_from_scores(R.scores(query[b], table, metric), excl[b], tgts[b]) for b in range(n_query)]
    return table, query, excl, tgts, want, inf_row


def _index(table, metric):
    from xfmr_rec_amd.retrieval import ExactItemIndex

    return ExactItemIndex(torch.from_numpy(table).to(DEV), index_metric=metric)


@functools.lru_cache(maxsize=None)
def _device_ranks(n_query, n_rows, H, metric):
    table, query, excl, tgts, want, _ = _exact_case(n_query, n_rows, H, metric)
    index = _index(table, metric)
    q = torch.from_numpy(query).to(DEV)
    csr = _csr(tgts)
    ranks = index.rank_targets(q, csr, _csr(excl))
    return index, q, csr, ranks


# ------------------------------------------------------------------------------------ 1. exact inputs: the numpy ranks
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("n_query,n_rows,H", SHAPES)
def test_ranks_equal_numpy_ranks_on_exact_inputs(n_query, n_rows, H, metric):
    table, query, excl, tgts, want, inf_row = _exact_case(n_query, n_rows, H, metric)
    index, q, csr, ranks = _device_ranks(n_query, n_rows, H, metric)
    assert ranks.dtype == torch.int32 and ranks.numel() == csr[0].numel()
    got = ranks.cpu().numpy()
    off = csr[1].cpu().numpy()
    assert got[off[-1]:].tolist() == [R.RANK_NONE]  # (the placeholder entry past the CSR is not written)
    n_none = n_live = 0
    for b in range(n_query):
        g = got[off[b] : off[b + 1]].tolist()
        assert g == want[b], (b, tgts[b][:8], g[:8], want[b][:8])
        n_none += sum(r == R.RANK_NONE for r in g)
        n_live += sum(r != R.RANK_NONE for r in g)
        if inf_row is not None and inf_row in tgts[b]:
            assert g[tgts[b].index(inf_row)] == R.RANK_NONE
    assert n_none > 0 and (n_live > 0 or n_rows == 2)
    if n_rows > 300:
        assert sum(r != R.RANK_NONE for r in want[0]) > 128  # the 300-target row takes more than one pass
    again = index.rank_targets(q, csr, _csr(excl))
    assert torch.equal(again, ranks)  # integer counts only: the same bits
    # without exclusions: the same ranks as an empty list per query
    free = index.rank_targets(q, csr, None)
    want_free = [R.ranks_from_scores(R.scores(query[b], table, metric), [], tgts[b]) for b in range(min(n_query, 40))]
    free_np = free.cpu().numpy()
    for b, w in enumerate(want_free):
        assert free_np[off[b] : off[b + 1]].tolist() == w, b


def test_rank_targets_on_a_chunk_of_a_longer_csr():
    """Offsets that are a view into a longer array with absolute values: entries outside the view are left alone."""
    table, query, excl, tgts, want, _ = _exact_case(33, 389, 12, "dot")
    index, q, csr, ranks = _device_ranks(33, 389, 12, "dot")
    ex = _csr(excl)
    off = csr[1].cpu().numpy()
    out = torch.full_like(ranks, -7)
    index.rank_targets(q[8:20], (csr[0], csr[1][8:21]), (ex[0], ex[1][8:21]), n_targets=int(off[20] - off[8]), out=out)
    assert torch.equal(out[off[8] : off[20]], ranks[off[8] : off[20]])
    assert (out[: off[8]] == -7).all() and (out[off[20] :] == -7).all()


# ------------------------------------------------------------------------------------ 2. the tiled search's scores
@pytest.mark.parametrize("H,metric", [(36, "cosine"), (384, "cosine"), (36, "l2"), (384, "dot")])
def test_ranks_and_scores_agree_with_the_tiled_search(H, metric):
    """Random floats: with 120 items search_batch(top_k=128) returns every eligible item, so a target's rank is
    its place in that list plus one, and the score the pre-pass computed for it (an fmaf chain) is the list's score (an
    MFMA tile) bit for bit."""
    from xfmr_rec_amd.retrieval import ExactItemIndex, sorted_exclusion_csr

    n_query, n_rows = 40, 120
    g = torch.Generator().manual_seed(H)
    table = torch.randn(n_rows, H, generator=g).to(DEV)
    q = torch.randn(n_query, H, generator=g).to(DEV)
    rng = np.random.default_rng(H)
    excl = [rng.integers(1, n_rows, int(rng.integers(0, 30))).tolist() for _ in range(n_query)]
    tgts = [rng.integers(0, n_rows + 1, int(rng.integers(1, 20))).tolist() for _ in range(n_query)]
    index = ExactItemIndex(table, index_metric=metric)
    idx, score = index.search_batch(q, excl, top_k=128)
    flat, off = sorted_exclusion_csr(excl)
    csr = _csr(tgts)
    ranks, tscore = index.rank_targets(q, csr, (torch.from_numpy(flat).to(DEV), torch.from_numpy(off).to(DEV)),
                                       return_scores=True)
    idx, score, ranks, tscore = idx.cpu().numpy(), score.cpu().numpy(), ranks.cpu().numpy(), tscore.cpu().numpy()
    toff = csr[1].cpu().numpy()
    n_checked = 0
    for b in range(n_query):
        place = {int(i): p for p, i in enumerate(idx[b]) if i >= 0}
        assert len(place) == n_rows - 1 - len(set(excl[b]))  # every eligible item is in the list
        for e, t in zip(range(toff[b], toff[b + 1]), tgts[b]):
            if t in place:
                assert ranks[e] == place[t] + 1, (b, t, ranks[e], place[t])
                assert tscore[e].view(np.uint32) == score[b, place[t]].view(np.uint32), (b, t, tscore[e], score[b, place[t]])
                n_checked += 1
            else:
                assert ranks[e] == R.RANK_NONE and tscore[e] == -np.inf, (b, t)
    assert n_checked > 100


# ------------------------------------------------------------------------------------ 3. the metrics from ranks
def _use_mask(n_query):
    use = np.random.default_rng(n_query).random(n_query) < 0.7
    use[0] = True
    return use


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("n_query,n_rows,H", SHAPES)
def test_rank_metrics_are_the_list_metrics_bit_for_bit(n_query, n_rows, H, metric):
    from xfmr_rec_amd.retrieval import rank_metrics_sum, retrieval_metrics_sum

    table, query, excl, tgts, want, _ = _exact_case(n_query, n_rows, H, metric)
    index, q, csr, ranks = _device_ranks(n_query, n_rows, H, metric)
    use_np = _use_mask(n_query)
    use = torch.from_numpy(use_np).to(DEV)
    cut = (1, 5, 20, 128)
    sums, vals, valid = rank_metrics_sum(ranks, csr, cut, use, per_row=True)
    assert sums.shape == (4, 8) and sums.dtype == torch.float64 and vals.shape == (n_query, 4, 7)
    free = rank_metrics_sum(ranks, csr, cut)  # no mask, no per-row outputs
    for ci, K in enumerate(cut):
        idx, _ = index.search_batch(q, excl, top_k=K)
        wsums, wvals, wvalid = retrieval_metrics_sum(idx, csr, use, top_k=K, per_row=True)
        assert torch.equal(valid, wvalid)
        assert torch.equal(vals[:, ci], wvals), (K, (vals[:, ci] != wvals).nonzero()[:5].tolist())
        assert torch.equal(sums[ci], wsums), (K, sums[ci].tolist(), wsums.tolist())
        assert torch.equal(free[ci], retrieval_metrics_sum(idx, csr, None, top_k=K))
    assert float(sums[0, 7]) == float((valid.cpu().numpy() & use_np).sum())
    none = rank_metrics_sum(ranks, csr, cut, torch.zeros(n_query, dtype=torch.uint8, device=DEV))
    assert torch.equal(none, torch.zeros((4, 8), dtype=torch.float64, device=DEV))


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("n_query,n_rows,H", SHAPES)
def test_rank_metrics_beyond_the_list_path(n_query, n_rows, H, metric):
    """K = 200, 500, 10 000: per row float32 against the host reference's Python floats, rtol 1e-6; the fp64 sums against
    the per-row values summed in fp64, 1e-12. The per-row figure is dominated by the 300-target row, whose nDCG and AP are
    float32 sums of up to 300 terms (as ``metrics_row`` would sum them): measured worst relative differences 1.6e-7 /
    3.6e-7 (33 x 389, dot / l2) and 9.9e-7 / 6.4e-7 (257 x 5 000); the inputs are seeded, the kernel is deterministic."""
    from xfmr_rec_amd.retrieval import METRIC_NAMES, rank_metrics_sum

    table, query, excl, tgts, want, _ = _exact_case(n_query, n_rows, H, metric)
    index, q, csr, ranks = _device_ranks(n_query, n_rows, H, metric)
    use_np = _use_mask(n_query)
    use = torch.from_numpy(use_np).to(DEV)
    cut = (200, 500, 10_000)
    sums, vals, valid = rank_metrics_sum(ranks, csr, cut, use, per_row=True)
    vals_np, valid_np, sums_np = vals.cpu().numpy(), valid.cpu().numpy(), sums.cpu().numpy()
    assert METRIC_NAMES == R.NAMES
    worst = 0.0
    for b in range(n_query):
        assert bool(valid_np[b]) == (len(tgts[b]) > 0)
        for ci, K in enumerate(cut):
            ref = R.metrics_from_ranks(want[b], tgts[b], K)
            w = np.asarray([ref[n] for n in R.NAMES]) if ref else np.zeros(7)
            err = np.abs(vals_np[b, ci] - w) / np.maximum(np.abs(w), 1e-300)
            worst = max(worst, float(err[w != 0].max()) if (w != 0).any() else 0.0)
            np.testing.assert_allclose(vals_np[b, ci], w, rtol=1e-6, atol=0, err_msg=f"row {b} ({len(tgts[b])} targets) K={K}")
    print(f"{n_query} x {n_rows}, {metric}: worst per-row relative difference {worst:.3e} (limit 1e-6)")
    counted = valid_np & use_np
    for ci in range(len(cut)):
        assert sums_np[ci, 7] == float(counted.sum())
        want_sum = vals_np[counted, ci].astype(np.float64).sum(axis=0)
        np.testing.assert_allclose(sums_np[ci, :7], want_sum, rtol=1e-12, atol=0)
    # more than 8 cutoffs: one call per 8, the same bits per cutoff, in the order given
    many = (200, 1, 5, 500, 20, 128, 2, 3, 10_000, 7)
    msums, mvals, _ = rank_metrics_sum(ranks, csr, many, use, per_row=True)
    for ci, K in enumerate(cut):
        assert torch.equal(msums[many.index(K)], sums[ci]) and torch.equal(mvals[:, many.index(K)], vals[:, ci])


def test_wrappers_refuse_mismatched_arguments():
    from xfmr_rec_amd.retrieval import rank_metrics_sum

    index, q, csr, ranks = _device_ranks(33, 389, 12, "dot")
    with pytest.raises(ValueError):
        index.rank_targets(q, (csr[0], csr[1][:-1]))
    with pytest.raises(ValueError):
        index.rank_targets(q, (csr[0].int(), csr[1]))
    with pytest.raises(ValueError):
        index.rank_targets(q, csr, (csr[0], csr[1][:-1]))
    with pytest.raises(ValueError):
        index.rank_targets(q, csr, out=torch.empty(3, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError):
        rank_metrics_sum(ranks[:-1], csr, (5,))
    with pytest.raises(ValueError):
        rank_metrics_sum(ranks, csr, (5, 0))
    with pytest.raises(ValueError):
        rank_metrics_sum(ranks, csr, ())
    with pytest.raises(ValueError):
        rank_metrics_sum(ranks, csr, (5,), torch.ones(3, dtype=torch.uint8, device=DEV))


# ------------------------------------------------------------------------------------ 4. end to end
H_, A_, L_, V_ = 64, 2, 24, 100


def _module(top_k=20, **kw):
    import xfmr_rec_amd as X

    conf = X.LightningConfig(hidden_size=H_, num_attention_heads=A_, intermediate_size=2 * H_, num_hidden_layers=2,
                             max_seq_length=L_, top_k=top_k, **kw)
    mod = X.RecommenderLightningModule(conf)
    mod.configure_model()
    mod.model.set_table(unit_table(V_, H_, seed=3).to(DEV))
    mod.model.id2idx = {f"i{i}": i for i in range(1, V_ + 1)}
    return mod


def _val_rows(n=37, seed=4):
    rng = np.random.default_rng(seed)
    rows = []
    for u in range(n):
        h = [f"i{x}" for x in rng.integers(1, V_ + 1, int(rng.integers(1, 31)))]
        t = [f"i{x}" for x in rng.integers(1, V_ + 1, int(rng.integers(1, 6)))]
        lab = [True] * len(t)
        if u == 5:
            lab = [False] * len(t)  # a row without a target
        if u == 9:
            h = []  # an empty history
        if u == 13:
            t.append(h[0])  # a target inside the history: no rank
        rows.append({"history": {"item_id": h}, "target": {"item_id": t, "label": lab}})
    return rows


def test_evalset_cutoffs_end_to_end():
    import xfmr_rec_amd as X
    from xfmr_rec_amd.retrieval import METRIC_NAMES

    mod = _module(top_k=20)
    rows = _val_rows()
    es = X.DeviceEvalSet.from_rows(mod, rows, batch_size=16)
    assert len(es) == 35 and len(es.plan.chunks) == 3
    plain = es.evaluate()
    ev = es.evaluate(cutoffs=(5, 20, 50))
    keys = {f"val/{n}" for n in METRIC_NAMES} | {"val/num_rows"}
    assert set(ev) == keys | {f"val/{n}@{K}" for n in METRIC_NAMES for K in (5, 20, 50)}
    assert set(plain) == keys
    for k in keys:
        assert ev[k] == plain[k], (k, ev[k], plain[k])  # the same per-row bits through the same reduction
    for n in METRIC_NAMES:
        assert ev[f"val/{n}@20"] == plain[f"val/{n}"]
        assert 0.0 <= ev[f"val/{n}@5"] <= 1.0
    assert ev["val/num_rows"] == 35
    assert ev["val/retrieval_recall@5"] <= ev["val/retrieval_recall@20"] <= ev["val/retrieval_recall@50"]
    # top_k joins the cutoffs when it is missing; a stage name is honoured
    ev2 = es.evaluate("test", cutoffs=[50])
    assert set(ev2) == {k.replace("val/", "test/") for k in keys} | {f"test/{n}@{K}" for n in METRIC_NAMES for K in (50, 20)}
    assert ev2["test/retrieval_normalized_dcg"] == plain["val/retrieval_normalized_dcg"]
    assert ev2["test/retrieval_recall@50"] == ev["val/retrieval_recall@50"]
    ranks = es.target_ranks()
    assert ranks.dtype == torch.int32 and ranks.numel() == es.targets.numel() and int(ranks.min()) >= 1
    assert int((ranks == R.RANK_NONE).sum()) >= 1  # the target inside its row's history
    tr = X.Trainer(mod)
    assert tr.validate(es, cutoffs=(5,)) == es.evaluate(cutoffs=(5,))
    # the module's own row-list evaluate takes the same path per pass
    old = mod.evaluate(rows, batch_size=16, cutoffs=(5, 20, 50))
    assert set(old) == set(ev) and old["val/num_rows"] == 35


def test_top_k_above_128_builds_a_cutoffs_only_set():
    import xfmr_rec_amd as X
    from xfmr_rec_amd.retrieval import METRIC_NAMES

    mod = _module(top_k=300)
    rows = _val_rows()
    with pytest.raises(ValueError, match="top_k"):
        X.DeviceEvalSet.from_rows(mod, rows)
    es = X.DeviceEvalSet.from_rows(mod, rows, batch_size=16, cutoffs_only=True)
    ev = es.evaluate(cutoffs=(10,))
    assert set(ev) == ({f"val/{n}" for n in METRIC_NAMES} | {"val/num_rows"}
                       | {f"val/{n}@{K}" for n in METRIC_NAMES for K in (10, 300)})
    assert ev["val/num_rows"] == 35 and ev["val/retrieval_recall"] == ev["val/retrieval_recall@300"]
    # 100 items: cutoff 300 reaches every eligible target
    assert 0.0 < ev["val/retrieval_recall@10"] < ev["val/retrieval_recall@300"] <= 1.0
    with pytest.raises(ValueError, match="top_k"):
        es.evaluate()


def test_fit_with_val_cutoffs_monitors_a_cutoff_and_leaves_training_alone():
    import xfmr_rec_amd as X

    g = torch.Generator().manual_seed(0)
    B = 8
    batches = []
    for i in range(6):
        b = {k: torch.randint(1, V_ + 1, (B, L_), generator=g) for k in ("history_item_idx", "pos_item_idx", "neg_item_idx")}
        for k in b:
            b[k][1, 5 + 2 * i:] = 0  # one ragged row
        batches.append({k: v.to(DEV) for k, v in b.items()})
    rows = _val_rows()
    plain = _module()
    watched = _module()
    with torch.no_grad():
        watched.model.flat.copy_(plain.model.flat)
    tr_p = X.Trainer(plain)
    want = tr_p.fit(batches)
    es = X.DeviceEvalSet.from_rows(watched, rows, batch_size=16)
    tr_w = X.Trainer(watched)
    name = "val/retrieval_normalized_dcg@5"
    got = tr_w.fit(batches, val=es, val_check_interval=2, val_cutoffs=(5, 50), monitor={"name": name, "mode": "max"})
    torch.cuda.synchronize()
    assert got == want and torch.equal(plain.model.flat, watched.model.flat)  # dropout is on: the step count did not move
    st_p, st_w = tr_p.optimizer.state[plain.model.flat], tr_w.optimizer.state[watched.model.flat]
    assert torch.equal(st_p["exp_avg"], st_w["exp_avg"]) and torch.equal(st_p["exp_avg_sq"], st_w["exp_avg_sq"])
    assert [h["step"] for h in tr_w.val_history] == [2, 4, 6]
    for h in tr_w.val_history:
        assert {name, "val/retrieval_normalized_dcg", "val/retrieval_normalized_dcg@50", "val/retrieval_recall@20",
                "val/num_rows"} <= set(h)
    assert tr_w.best_score == max(h[name] for h in tr_w.val_history)
    assert tr_w.val_history[[h[name] for h in tr_w.val_history].index(tr_w.best_score)]["step"] == tr_w.best_step
    assert watched.logged[name] == tr_w.val_history[-1][name]
