"""Validation inside ``Trainer.fit``: xfmr_retrieval_metrics_sum against the per-row kernel, the chain that pins a resident
validation pass (``DeviceEvalSet.encode`` / ``recommend`` / ``evaluate``), training left undisturbed by validation passes
(eager and between hipGraph replays), and early stopping + the best checkpoint."""

import numpy as np
import pytest
import torch

from helpers import TOL, max_scaled_err, unit_table

pytestmark = pytest.mark.gpu
DEV = "cuda"


# ------------------------------------------------------------------------------------ 1. sums kernel vs per-row kernel
def _metric_inputs(n, k, seed):
    """rec (n, k) with -1 padding here and there, 0-8 targets per row (some rows none, row 0 or 1 a duplicated target),
    a random use mask. Items from a range small enough for hits."""
    rng = np.random.default_rng(seed)
    rec = rng.integers(1, 60, (n, k))
    rec[rng.random((n, k)) < 0.02] = -1
    tgts = [rng.integers(1, 60, int(c)).tolist() for c in rng.integers(0, 9, n)]
    dup = min(1, n - 1)
    tgts[dup] = [int(rec[dup, 0]), 7, int(rec[dup, 0])]  # a duplicate-target row (a hit at rank 1)
    if n > 2:
        tgts[2] = []
    use = rng.random(n) < 0.7
    use[dup] = True
    return rec, tgts, use


def _csr_dev(lists):
    off = np.zeros(len(lists) + 1, dtype=np.int64)
    np.cumsum([len(x) for x in lists], out=off[1:])
    flat = np.concatenate([np.asarray(x, dtype=np.int64) for x in lists]) if off[-1] else np.zeros(1, dtype=np.int64)
    return torch.from_numpy(flat).to(DEV), torch.from_numpy(off).to(DEV)


def _check_sums(n, k, top_k, with_use, seed):
    from xfmr_rec_amd.retrieval import retrieval_metrics, retrieval_metrics_sum

    rec_np, tgts, use_np = _metric_inputs(n, k, seed)
    rec = torch.from_numpy(rec_np).to(DEV)
    csr = _csr_dev(tgts)
    use = torch.from_numpy(use_np).to(DEV) if with_use else None
    want_vals, want_valid = retrieval_metrics(rec, tgts, top_k)
    sums, vals, valid = retrieval_metrics_sum(rec, csr, use, top_k=top_k, per_row=True)
    assert torch.equal(vals, want_vals) and torch.equal(valid, want_valid)  # one device function: the same bits
    counted = want_valid.cpu().numpy() & (use_np if with_use else True)
    s = sums.cpu().numpy()
    assert s.dtype == np.float64 and s.shape == (8,)
    assert s[7] == float(counted.sum()) and 0 < counted.sum()
    v64 = want_vals.cpu().numpy().astype(np.float64)[counted]
    for i in range(7):
        S = float(np.cumsum(v64[:, i])[-1])  # fp64, index order
        # both sides are fp64 sums of the same <= 1-valued terms: they differ by reassociation only
        lim = 2 * n * 2.0 ** -53 * max(1.0, S)
        print(f"n={n} k={k} top_k={top_k} metric {i}: |{s[i]!r} - {S!r}| = {abs(s[i] - S):.3e} (limit {lim:.3e})")
        assert abs(s[i] - S) <= lim, (i, s[i], S)
    again = retrieval_metrics_sum(rec, csr, use, top_k=top_k)  # (no per-row outputs this time: NULL pointers)
    assert torch.equal(again, sums)
    none = retrieval_metrics_sum(rec, csr, torch.zeros(n, dtype=torch.uint8, device=DEV), top_k=top_k)
    assert torch.equal(none, torch.zeros(8, dtype=torch.float64, device=DEV))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1000, 65537])
def test_metrics_sum_matches_the_per_row_kernel(n):
    _check_sums(n, 20, 20, True, seed=n)


def test_metrics_sum_without_a_mask_and_with_a_short_list():
    _check_sums(257, 20, 20, False, seed=1)
    _check_sums(257, 10, 20, True, seed=2)   # k < top_k: the slots past the list are misses


def test_metrics_sum_wrapper_refuses_mismatched_arguments():
    from xfmr_rec_amd.retrieval import retrieval_metrics_sum

    rec = torch.ones((4, 5), dtype=torch.int64, device=DEV)
    csr = _csr_dev([[1], [2], [3], [4]])
    with pytest.raises(ValueError):
        retrieval_metrics_sum(rec, (csr[0], csr[1][:-1]), top_k=5)
    with pytest.raises(ValueError):
        retrieval_metrics_sum(rec, csr, torch.ones(3, dtype=torch.uint8, device=DEV), top_k=5)


# ------------------------------------------------------------------------------------ 2. the chain that pins a pass
def _module(H, A, L, precision, V, seed=0, **kw):
    import xfmr_rec_amd as X

    conf = X.LightningConfig(hidden_size=H, num_attention_heads=A, intermediate_size=2 * H, num_hidden_layers=2,
                             max_seq_length=L, precision=precision, top_k=20, **kw)
    mod = X.RecommenderLightningModule(conf)
    mod.configure_model()
    mod.model.set_table(unit_table(V, H, seed=seed).to(DEV))
    mod.model.id2idx = {f"i{i}": i for i in range(1, V + 1)}
    return mod


def _val_rows(V, n, seed, max_hist=40):
    rng = np.random.default_rng(seed)
    rows = []
    for u in range(n):
        h = rng.integers(1, V + 1, int(rng.integers(1, max_hist + 1))).tolist()
        t = rng.integers(1, V + 1, int(rng.integers(1, 5))).tolist()
        lab = (rng.random(len(t)) < 0.7).tolist()
        if u % 7 == 3:
            lab = [False] * len(t)     # no positive target
        hs, ts = [f"i{x}" for x in h], [f"i{x}" for x in t]
        if u % 5 == 1:
            hs.insert(len(hs) // 2, "unknown-a")  # unknown ids are dropped
            ts.append("unknown-b")
            lab.append(True)
        if u == 11:
            hs = []                    # an empty history
        if u == 12:
            hs = ["unknown-c"]         # empty once the unknown id is dropped
        rows.append({"history": {"item_id": hs}, "target": {"item_id": ts, "label": lab}})
    return rows


@pytest.mark.parametrize("H,A,precision,packed", [(64, 2, "bf16", True), (128, 2, "fp32", False)])
def test_resident_pass_chain(H, A, precision, packed):
    import xfmr_rec_amd as X
    from oracle.metrics import compute_retrieval_metrics
    from xfmr_rec_amd.retrieval import METRIC_NAMES

    L, V, k = 16, 300, 20
    mod = _module(H, A, L, precision, V)
    mod.train()  # the pass runs in eval mode whatever the flag says, and puts the flag back
    rows = _val_rows(V, 200, seed=5)
    es = X.DeviceEvalSet.from_rows(mod, rows, batch_size=64)
    assert es.packed == packed == mod.model.supports_packed_rows(L)
    assert len(es.plan.chunks) >= 3 and es.plan.chunks[-1].row1 - es.plan.chunks[-1].row0 < 64  # a ragged last chunk
    hists = [mod._to_idx_or_empty(list(r["history"]["item_id"])) for r in rows]
    tgts = [mod._to_idx_or_empty([i for i, l in zip(r["target"]["item_id"], r["target"]["label"]) if l]) for r in rows]
    want_kept = [i for i in range(len(rows)) if hists[i] and tgts[i]]
    assert sorted(es.kept.tolist()) == want_kept and 11 not in want_kept and 12 not in want_kept
    assert es.kept.dtype == np.int64 and len(es) == len(want_kept) < len(rows)
    kept_hists = [hists[i] for i in es.kept]
    step_before = mod.model._step
    # (a) encode() against encode_batch of the same histories
    emb = es.encode()
    assert mod.model.training and mod.model._step == step_before
    ref = mod.model.encode_batch(kept_hists)
    assert emb.shape == ref.shape == (len(es), H)
    worst = 0.0
    for b in range(len(es)):
        err = max_scaled_err(emb[b], ref[b])
        worst = max(worst, err)
        assert err <= TOL[precision]["val"], (b, len(kept_hists[b]), err)
    print(f"[{precision}] encode() vs encode_batch: worst max_scaled_err {worst:.3e} (limit {TOL[precision]['val']:.1e})")
    # (b) recommend() against search_batch on encode()'s own output with the same exclusions
    idx, score = es.recommend()
    widx, wscore = mod.items_index.search_batch(emb, kept_hists, top_k=k)
    assert torch.equal(idx, widx) and torch.equal(score, wscore)
    idx_np = idx.cpu().numpy()
    assert (idx_np > 0).all()  # never the padding row, and (300 items, <= 40 excluded) never short
    for b, h in enumerate(kept_hists):
        assert not set(idx_np[b].tolist()) & set(h), b
    # (c) evaluate() against the oracle's metrics over recommend()'s lists
    ev = es.evaluate()
    per_row = [compute_retrieval_metrics(idx_np[b].tolist(), tgts[i], k) for b, i in enumerate(es.kept)]
    assert set(ev) == {f"val/{n}" for n in METRIC_NAMES} | {"val/num_rows"}
    for name in METRIC_NAMES:
        want = float(np.mean([p[name] for p in per_row]))
        assert ev[f"val/{name}"] == pytest.approx(want, rel=1e-5, abs=1e-6), name
    old = mod.evaluate(rows, batch_size=64)
    assert ev["val/num_rows"] == len(es.kept) == old["val/num_rows"]
    assert set(old) == set(ev)
    assert es.evaluate(stage="test")["test/num_rows"] == len(es.kept)
    dev_sums = es.evaluate_device()
    assert dev_sums.is_cuda and dev_sums.dtype == torch.float64 and dev_sums.shape == (8,)
    assert mod.model.training and mod.model._step == step_before


def test_from_rows_refusals():
    import xfmr_rec_amd as X

    mod = _module(64, 2, 16, "bf16", 300)
    with pytest.raises(ValueError, match="no validation row"):
        X.DeviceEvalSet.from_rows(mod, [{"history": {"item_id": []}, "target": {"item_id": ["i1"], "label": [True]}},
                                        {"history": {"item_id": ["i3"]}, "target": {"item_id": ["i1"], "label": [False]}}])
    mod.config.top_k = 129
    with pytest.raises(ValueError, match="top_k"):
        X.DeviceEvalSet.from_rows(mod, _val_rows(300, 10, seed=0))


# ------------------------------------------------------------------------------------ 3. training is not disturbed
def _train_setup(n_batches=8, dense=False, B=8, L=24, H=64, V=200, **conf_kw):
    import xfmr_rec_amd as X

    g = torch.Generator().manual_seed(0)
    conf = X.LightningConfig(hidden_size=H, num_attention_heads=H // 32, intermediate_size=2 * H, num_hidden_layers=2,
                             max_seq_length=L, **conf_kw)
    table = unit_table(V, H, seed=7).to(DEV)
    batches = []
    for i in range(n_batches):
        b = {k: torch.randint(1, V + 1, (B, L), generator=g) for k in ("history_item_idx", "pos_item_idx", "neg_item_idx")}
        if not dense:
            for k in b:
                b[k][1, 5 + 2 * i:] = 0  # one ragged row
        batches.append({k: v.to(DEV) for k, v in b.items()})
    rows = _val_rows(V, 40, seed=9, max_hist=30)

    def module(flat_from=None):
        mod = X.RecommenderLightningModule(conf)
        mod.configure_model()
        mod.model.set_table(table)
        mod.model.id2idx = {f"i{i}": i for i in range(1, V + 1)}
        if flat_from is not None:
            with torch.no_grad():
                mod.model.flat.copy_(flat_from.model.flat)
        return mod

    return X, module, batches, rows


def _moments(trainer):
    st = trainer.optimizer.state[trainer.module.model.flat]
    return st["exp_avg"], st["exp_avg_sq"]


@pytest.mark.parametrize("graph", ["off", "on"])
def test_validation_passes_leave_training_bit_identical(graph):
    X, module, batches, rows = _train_setup(dense=graph == "on")
    plain = module()
    init = module(plain)  # (keeps the initial parameters for the twin below)
    tr_p = X.Trainer(plain)
    want = tr_p.fit(batches, graph=graph)
    watched = module(init)
    es = X.DeviceEvalSet.from_rows(watched, rows, batch_size=16)
    tr_w = X.Trainer(watched)
    got = tr_w.fit(batches, graph=graph, val=es, val_check_interval=2)
    torch.cuda.synchronize()
    assert len(got) == len(batches) and got == want  # dropout is on: the passes did not move the step count
    assert torch.equal(plain.model.flat, watched.model.flat)
    for a, b in zip(_moments(tr_p), _moments(tr_w)):
        assert torch.equal(a, b)
    if graph == "on":
        assert tr_p.graph_choice == tr_w.graph_choice == "graph"
    assert [h["step"] for h in tr_w.val_history] == [2, 4, 6, 8]
    assert not tr_w.stopped_early and tr_w.val_elapsed > 0.0 and tr_w.best_model_path is None
    name = "val/retrieval_normalized_dcg"
    assert tr_w.best_score == max(h[name] for h in tr_w.val_history)
    assert tr_w.val_history[[h[name] for h in tr_w.val_history].index(tr_w.best_score)]["step"] == tr_w.best_step
    assert watched.logged[name] == tr_w.val_history[-1][name]  # the passes went through log_dict
    # the first entry is what Trainer.validate gives on a twin stopped after two steps
    twin = module(init)
    tr_t = X.Trainer(twin)
    assert tr_t.fit(batches[:2], graph="off" if graph == "off" else "on") == want[:2]
    first = tr_t.validate(X.DeviceEvalSet.from_rows(twin, rows, batch_size=16))
    assert {"step": 2, **first} == tr_w.val_history[0]
    # without an interval: one pass after the last batch
    if graph == "off":
        tr_t.fit(batches[2:4], val=X.DeviceEvalSet.from_rows(twin, rows, batch_size=16))
        assert [h["step"] for h in tr_t.val_history] == [2]
        assert {**tr_t.val_history[0], "step": 4} == tr_w.val_history[1]


# ------------------------------------------------------------------------------------ 4. early stop and best checkpoint
def test_early_stopping_stops_a_run_whose_metric_cannot_move():
    X, module, batches, rows = _train_setup(n_batches=10, learning_rate=0.0, weight_decay=0.0)
    mod = module()
    es = X.DeviceEvalSet.from_rows(mod, rows, batch_size=16)
    tr = X.Trainer(mod)
    out = tr.fit(batches, val=es, val_check_interval=2, early_stopping={"patience": 1, "min_delta": 0.0})
    assert len(out) == 4 and tr.stopped_early and tr.best_step == 2
    assert [h["step"] for h in tr.val_history] == [2, 4]
    assert tr.val_history[0]["val/retrieval_normalized_dcg"] == tr.val_history[1]["val/retrieval_normalized_dcg"] == tr.best_score


def test_best_checkpoint_reloads_to_the_best_score(tmp_path):
    X, module, batches, rows = _train_setup(n_batches=10, learning_rate=0.01)
    mod = module()
    es = X.DeviceEvalSet.from_rows(mod, rows, batch_size=16)
    tr = X.Trainer(mod)
    out = tr.fit(batches, val=es, val_check_interval=2, checkpoint_dir=tmp_path)
    name = "val/retrieval_normalized_dcg"
    assert len(out) == 10 and not tr.stopped_early and len(tr.val_history) == 5
    assert tr.best_score == max(h[name] for h in tr.val_history)
    assert tr.best_model_path == str(tmp_path / "best") and (tmp_path / "best" / "model.safetensors").exists()
    fresh = X.RecommenderLightningModule(mod.config)
    fresh.model = X.RecommenderModel.load(tr.best_model_path, device=DEV, precision=mod.config.precision)
    fresh.configure_model()
    fresh.model.set_table(mod.model.embeddings)
    fresh.model.id2idx = mod.model.id2idx
    again = X.DeviceEvalSet.from_rows(fresh, rows, batch_size=16).evaluate()
    print(f"best {tr.best_score!r} at step {tr.best_step}; reloaded {again[name]!r}; history "
          f"{[round(h[name], 6) for h in tr.val_history]}")
    assert abs(again[name] - tr.best_score) <= 1e-9  # same kernels, same parameters, deterministic
