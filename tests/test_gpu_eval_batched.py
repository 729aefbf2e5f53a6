"""Batched evaluation: xfmr_pool_rows against the padded xfmr_pool (+ xfmr_l2_normalize_fwd) bit for bit,
RecommenderModel.encode_batch against the per-row forward (packed and padded routes), and
RecommenderLightningModule.predict_batch / evaluate against the per-row predict_step / validation_step loop."""

import numpy as np
import pytest
import torch

from helpers import TOL, max_scaled_err

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("mode", ["mean", "max", "cls", "lasttoken"])
@pytest.mark.parametrize("normalize", [False, True])
def test_pool_rows_bit_identical_to_padded_pool(mode, normalize):
    from xfmr_rec_amd import ops

    L, H = 24, 100
    lens = [1, L, 5, 17, L, 3, 9, 1]
    g = torch.Generator().manual_seed(0)
    tok = torch.randn(sum(lens), H, generator=g).cuda()
    off = torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int32).cuda()
    padded = torch.zeros(len(lens), L, H, device="cuda")
    mask = torch.zeros(len(lens), L, dtype=torch.uint8, device="cuda")
    for b, n in enumerate(lens):
        padded[b, :n] = tok[int(off[b]) : int(off[b]) + n]
        mask[b, :n] = 1
    want = ops.pool(padded, mask, mode)
    if normalize:
        want = ops.l2_normalize(want)
    got = ops.pool_rows(tok, off, mode, normalize=normalize)
    assert torch.equal(got, want)
    # an empty sequence in the middle: a zero row, the others unchanged
    off2 = torch.tensor(np.concatenate([[0], np.cumsum(lens[:3] + [0] + lens[3:])]), dtype=torch.int32).cuda()
    got2 = ops.pool_rows(tok, off2, mode, normalize=normalize)
    assert torch.equal(got2[3], torch.zeros(H, device="cuda"))
    assert torch.equal(torch.cat([got2[:3], got2[4:]]), want)


def _module(H, A, L, precision, V=300, seed=0, **kw):
    import xfmr_rec_amd as X
    from helpers import unit_table

    conf = X.LightningConfig(hidden_size=H, num_attention_heads=A, intermediate_size=2 * H, num_hidden_layers=2,
                             max_seq_length=L, precision=precision, top_k=20, **kw)
    mod = X.RecommenderLightningModule(conf)
    mod.configure_model()
    mod.model.set_table(unit_table(V, H, seed=seed).cuda())
    mod.eval()
    return mod


@pytest.mark.parametrize("H,A,precision,pooling,normalized,packed", [
    (64, 2, "bf16", "mean", False, True),        # head size 32, bf16: the packed layout
    (64, 2, "bf16", "lasttoken", True, True),
    (128, 2, "fp32", "mean", False, False),      # fp32 policy, head size 64: the right-padded forward
    (128, 2, "fp32", "max", True, False),
])
def test_encode_batch_matches_per_row_forward(H, A, precision, pooling, normalized, packed):
    L, V = 16, 300
    mod = _module(H, A, L, precision, V=V, pooling_mode=pooling, is_normalized=normalized)
    m = mod.model
    assert m.supports_packed_rows(L) == packed
    rng = np.random.default_rng(1)
    hists = [rng.integers(1, V + 1, n).tolist() for n in (1, 5, L, 30, 3, 40, L - 1, 2)]
    got = m.encode_batch(hists)
    assert got.shape == (len(hists), H)
    for b, h in enumerate(hists):
        want = m(torch.as_tensor(h, device="cuda")[None])["sentence_embedding"][0]  # keeps the last L rows itself
        err = max_scaled_err(got[b], want)
        assert err <= TOL[precision]["val"], (b, len(h), err)
    # an empty history: a zero row, the others as before
    got2 = m.encode_batch(hists[:2] + [[]] + hists[2:])
    assert torch.equal(got2[2], torch.zeros(H, device="cuda"))


def _rows(V, n, rng, ids=True):
    rows = []
    for u in range(n):
        h = rng.integers(1, V + 1, int(rng.integers(3, 40))).tolist()
        t = rng.integers(1, V + 1, int(rng.integers(1, 5))).tolist()
        lab = (rng.random(len(t)) < 0.7).tolist()
        if u % 7 == 3:
            lab = [False] * len(t)  # no positive target: left out of the means
        hs, ts = [f"i{x}" for x in h], [f"i{x}" for x in t]
        if u % 5 == 1:
            hs.insert(1, "unknown-a")  # unknown ids are dropped
            ts.append("unknown-b")
            lab.append(True)
        rows.append({"history": {"item_id": hs}, "target": {"item_id": ts, "label": lab}})
    return rows


def test_predict_batch_and_evaluate_match_the_per_row_loop():
    from xfmr_rec_amd.retrieval import METRIC_NAMES

    V, k = 500, 20
    mod = _module(128, 2, 32, "fp32", V=V, seed=3)
    mod.model.id2idx = {f"i{i}": i for i in range(1, V + 1)}
    rng = np.random.default_rng(2)
    rows = _rows(V, 60, rng)
    got = mod.predict_batch(rows)
    gi, gs = got["item_idx"].cpu().numpy(), got["score"].cpu().numpy()
    per_row = []
    for b, r in enumerate(rows):
        want = mod.predict_step(r)
        wi = want["item_idx"].cpu().numpy()
        hist = mod._to_idx(list(r["history"]["item_id"]))
        emb = mod.model(torch.as_tensor(hist, device="cuda")[None])["sentence_embedding"]
        _, ref = mod.items_index.search(emb, [hist], top_k=k + 1)  # the k-th place's gap
        ref = ref[0].cpu().numpy()
        np.testing.assert_allclose(gs[b], want["score"].cpu().numpy(), rtol=1e-5, atol=1e-5)
        if ref[k - 1] - ref[k] > 1e-4:
            assert set(gi[b].tolist()) == set(wi.tolist()), b
            if (np.diff(ref[:k]) < -1e-4).all():
                assert gi[b].tolist() == wi.tolist(), b
        m = mod.validation_step(r)
        if m:
            per_row.append({n: float(v) for n, v in m.items()})
    ev = mod.evaluate(rows, stage="val", batch_size=23)  # several passes, the last one short
    assert ev["val/num_rows"] == len(per_row) and 0 < len(per_row) < len(rows)
    for name in METRIC_NAMES:
        want = float(np.mean([p[f"val/{name}"] for p in per_row]))
        assert abs(ev[f"val/{name}"] - want) <= 1e-5, (name, ev[f"val/{name}"], want)
    # empty histories (also after unknown ids are dropped): all -1, left out of the means and of num_rows
    empties = [{"history": {"item_id": []}, "target": {"item_id": ["i1"], "label": [True]}},
               {"history": {"item_id": ["unknown-c", "unknown-d"]}, "target": {"item_id": ["i2"], "label": [True]}}]
    rec = mod.predict_batch(empties + rows[:3])
    assert (rec["item_idx"][:2] == -1).all() and torch.isinf(rec["score"][:2]).all()
    assert torch.equal(rec["item_idx"][2:], got["item_idx"][:3])
    ev2 = mod.evaluate(empties + rows, stage="test", batch_size=1000)
    assert ev2["test/num_rows"] == ev["val/num_rows"]
    for name in METRIC_NAMES:
        assert abs(ev2[f"test/{name}"] - ev[f"val/{name}"]) <= 1e-6


def test_evaluate_after_training_matches_the_per_row_mean():
    """In the style of test_gpu_e2e: train briefly on the planted catalogue, then the batched validation nDCG equals the
    mean of the per-row validation_step values."""
    import xfmr_rec_amd as X
    from test_gpu_e2e import _histories, _planted_catalogue
    from xfmr_rec_amd.data import DeviceSeqDataset, SeqDataConfig

    V, H, L, B, steps = 400, 64, 32, 128, 300
    rng = np.random.default_rng(0)
    table = _planted_catalogue(V, H, seed=1)
    train = _histories(V, 3000, rng)
    val = [h[-(L + 1):] for h in _histories(V, 120, rng, noise=0.0)]
    conf = X.LightningConfig(hidden_size=H, num_attention_heads=2, intermediate_size=128, num_hidden_layers=2,
                             max_seq_length=L, precision="fp32", top_k=20, pooling_mode="lasttoken")
    mod = X.RecommenderLightningModule(conf)
    mod.configure_model()
    mod.model.set_table(table.cuda())
    ds = DeviceSeqDataset(SeqDataConfig(max_seq_length=L, pos_lookahead=0), train, [np.ones(len(h), bool) for h in train],
                          n_items=V, device="cuda")
    trainer = X.Trainer(mod)
    for step in range(steps):
        trainer.fit_step(ds.sample_batch(rng.integers(0, len(ds), size=B), seed=step))
    mod.eval()
    rows = [{"history": {"item_id": h[:-1]}, "target": {"item_id": h[-1:], "label": np.array([True])}} for h in val]
    per_row = [float(mod.validation_step(r)["val/retrieval_normalized_dcg"]) for r in rows]
    ev = mod.evaluate(rows)
    assert ev["val/num_rows"] == len(rows)
    assert abs(ev["val/retrieval_normalized_dcg"] - float(np.mean(per_row))) <= 1e-5
    assert ev["val/retrieval_normalized_dcg"] > 0.1  # it learned (chance <= 0.05)
