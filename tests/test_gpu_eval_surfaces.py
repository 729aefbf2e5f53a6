"""The evaluation surfaces over their shared host path (``eval_rows``, ``ExactItemIndex._tiled_search``,
``RecommenderModel.sentence_embeddings`` / ``eval_mode``): the resident set's search reaches the bits of ``search_batch``,
both evaluators name their results alike, and a pass that raises leaves the model's mode and step count alone. Once in
bf16 (the packed layout) and once in fp32 (the padded one)."""

import numpy as np
import pytest
import torch

from helpers import unit_table

pytestmark = pytest.mark.gpu
DEV = "cuda"
H, A, L, V, N_ROWS, K = 64, 2, 24, 300, 40, 20
CUTOFFS = (5, 20, 500)


def _rows():
    """40 rows with histories of 0 .. 3 L ids; some without a positive target, some with unknown string ids, one history
    empty and one of unknown ids only."""
    rng = np.random.default_rng(21)
    rows = []
    for u in range(N_ROWS):
        n = (0, 1, L - 1, L, L + 1, 3 * L)[u] if u < 6 else int(rng.integers(1, 3 * L + 1))
        h = [f"i{x}" for x in rng.integers(1, V + 1, n)]
        t = [f"i{x}" for x in rng.integers(1, V + 1, int(rng.integers(1, 5)))]
        lab = (rng.random(len(t)) < 0.7).tolist()
        if u % 7 == 3:
            lab = [False] * len(t)              # no positive target
        elif u < 6:
            lab[0] = True
        if u % 5 == 1:
            h.insert(len(h) // 2, "unknown-a")  # unknown ids are dropped
            t.append("unknown-b")
            lab.append(True)
        if u == 12:
            h = ["unknown-c"]                   # empty once the unknown id is dropped
        rows.append({"history": {"item_id": h}, "target": {"item_id": t, "label": lab}})
    return rows


@pytest.fixture(scope="module", params=[("bf16", True), ("fp32", False)], ids=["bf16-packed", "fp32-padded"])
def setup(request):
    import xfmr_rec_amd as X

    precision, packed = request.param
    conf = X.LightningConfig(hidden_size=H, num_attention_heads=A, intermediate_size=2 * H, num_hidden_layers=2,
                             max_seq_length=L, precision=precision, top_k=K)
    mod = X.RecommenderLightningModule(conf)
    mod.configure_model()
    mod.model.set_table(unit_table(V, H, seed=3).to(DEV))
    mod.model.id2idx = {f"i{i}": i for i in range(1, V + 1)}
    assert mod.model.supports_packed_rows(L) == packed
    mod.train()  # every pass runs in eval mode whatever the flag says, and puts the flag back
    mod.model._step = 5
    return X, mod, _rows(), packed


def test_resident_search_reaches_the_bits_of_search_batch(setup):
    X, mod, rows, packed = setup
    es = X.DeviceEvalSet.from_rows(mod, rows, batch_size=16)
    sizes = [c.row1 - c.row0 for c in es.plan.chunks]
    assert es.packed == packed and len(sizes) >= 2 and sizes[-1] < 16 == sizes[0]  # a short last chunk
    hists = [mod._to_idx_or_empty(list(r["history"]["item_id"])) for r in rows]
    kept_hists = [hists[i] for i in es.kept]
    assert 0 < len(kept_hists) < len(rows) and max(map(len, kept_hists)) > L and all(kept_hists)
    emb = es.encode()
    idx, score = es.recommend()
    widx, wscore = mod.items_index.search_batch(emb, kept_hists, K)
    assert idx.shape == (len(es), K) and idx.dtype == torch.int64 and score.dtype == torch.float32
    assert torch.equal(idx, widx) and torch.equal(score, wscore)
    idx2, score2 = es.recommend(emb)  # (the embedding handed in: the same search)
    assert torch.equal(idx2, idx) and torch.equal(score2, score)
    assert mod.model.training and mod.model._step == 5


def test_both_evaluators_name_their_results_alike(setup):
    X, mod, rows, _ = setup
    from xfmr_rec_amd.retrieval import METRIC_NAMES

    old = mod.evaluate(rows, batch_size=16, cutoffs=CUTOFFS)
    new = X.DeviceEvalSet.from_rows(mod, rows, batch_size=16, cutoffs_only=True).evaluate(cutoffs=CUTOFFS)
    # (the values are not compared: module.evaluate sums per chunk and adds on the host, the set sums once on the device)
    want = []
    for cut in CUTOFFS:
        want += [f"val/{n}@{cut}" for n in METRIC_NAMES]
        if cut == K:
            want += [f"val/{n}" for n in METRIC_NAMES] + ["val/num_rows"]
    assert list(old) == list(new) == want
    assert mod._evaluate_ranks(rows, "val", 16, CUTOFFS) == old  # (the rank path under its earlier name)
    assert old["val/num_rows"] == new["val/num_rows"] and type(old["val/num_rows"]) is type(new["val/num_rows"]) is int
    assert 0 < old["val/num_rows"] < len(rows)
    assert all(type(v) is float for d in (old, new) for k, v in d.items() if k != "val/num_rows")
    plain_old, plain_new = mod.evaluate(rows, batch_size=16), X.DeviceEvalSet.from_rows(mod, rows, batch_size=16).evaluate()
    assert list(plain_old) == list(plain_new) == [f"val/{n}" for n in METRIC_NAMES] + ["val/num_rows"]
    assert plain_old["val/num_rows"] == plain_new["val/num_rows"] == old["val/num_rows"]
    assert mod.model.training and mod.model._step == 5


def test_a_failing_pass_leaves_mode_and_step_count_alone(setup, monkeypatch):
    X, mod, rows, _ = setup
    monkeypatch.setattr(mod.config, "top_k", 200)
    es = X.DeviceEvalSet.from_rows(mod, rows, batch_size=16, cutoffs_only=True)  # (refused without cutoffs_only)
    with pytest.raises(ValueError, match="top_k = 200"):
        es.recommend()
    with pytest.raises(ValueError, match="top_k = 200"):
        es.evaluate()
    with pytest.raises(ValueError, match="top_k = 200"):
        X.DeviceEvalSet.from_rows(mod, rows, batch_size=16)
    assert mod.model.training and mod.model._step == 5
    monkeypatch.undo()

    def fails(chunk):  # a pass that raises inside the eval-mode guard, behind the first launch-free steps
        assert not mod.model.training
        raise KeyError("a failing pass")

    monkeypatch.setattr(mod.model, "sentence_embeddings", fails)
    es = X.DeviceEvalSet.from_rows(mod, rows, batch_size=16)
    for call in (es.encode, es.evaluate, lambda: es.evaluate(cutoffs=CUTOFFS), lambda: mod.evaluate(rows, batch_size=16),
                 lambda: mod.evaluate(rows, cutoffs=CUTOFFS), lambda: mod.predict_batch(rows)):
        with pytest.raises(KeyError, match="a failing pass"):
            call()
        assert mod.model.training and mod.model._step == 5
    monkeypatch.undo()
    mod.eval()
    with pytest.raises(ValueError, match="exclude_item_idx has 1 lists"):
        mod.items_index.search_batch(mod.model.encode_batch([[1, 2], [3]]), [[1]], K)
    assert not mod.model.training and mod.model._step == 5
    mod.train()
