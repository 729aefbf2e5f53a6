"""The evaluation surfaces take the forward-only encoder pass (ops.encoder_infer) and lose nothing by it: with ``XFMR_INFER=0``
(the training forward again) and by default, ``ops.encoder_infer`` / ``model.encode_batch`` / ``model.encode`` /
``DeviceEvalSet.encode`` / ``DeviceEvalSet.evaluate`` / ``module.recommend_batch`` give the same bits, in one process. Counting
wrappers show which of the two entries each surface calls; a training run with an ``encode_batch`` call between its steps
is bit-identical to one without. A small model (V = 50, H = 64, 2 heads, L = 16, 2 layers) and 12 users, once in bf16 --
where the surfaces run the packed layout -- and once in fp32 (padded)."""

import ctypes as C

import numpy as np
import pytest
import torch

from helpers import unit_table

pytestmark = pytest.mark.gpu
DEV = "cuda"
V, H, A, L, LAYERS, USERS = 50, 64, 2, 16, 2, 12


def _module(precision, seed=0):
    import xfmr_rec_amd as X

    conf = X.LightningConfig(hidden_size=H, num_attention_heads=A, intermediate_size=2 * H, num_hidden_layers=LAYERS,
                             max_seq_length=L, precision=precision, top_k=10)
    mod = X.RecommenderLightningModule(conf)
    mod.configure_model()
    mod.model.set_table(unit_table(V, H, seed=seed).to(DEV))
    mod.model.id2idx = {f"i{i}": i for i in range(1, V + 1)}
    return mod


def _rows(seed=5):
    """12 users: histories of 1 ... 20 items (some longer than L: truncated), 1-3 targets, at least one positive."""
    rng = np.random.default_rng(seed)
    rows = []
    for u in range(USERS):
        n = (1, L, 20)[u] if u < 3 else int(rng.integers(2, 21))
        h = rng.integers(1, V + 1, n).tolist()
        t = rng.integers(1, V + 1, int(rng.integers(1, 4))).tolist()
        rows.append({"history": {"item_id": [f"i{x}" for x in h]},
                     "target": {"item_id": [f"i{x}" for x in t], "label": [True] + [False] * (len(t) - 1)}})
    return rows


class Counters:
    """ops.encoder / ops.encoder_infer wrapped in counting functions (the surfaces look both up on the module per call)."""

    def __init__(self, monkeypatch):
        from xfmr_rec_amd import ops

        self.n = {"encoder": 0, "encoder_infer": 0}
        for name in self.n:
            monkeypatch.setattr(ops, name, self._wrap(name, getattr(ops, name)))

    def _wrap(self, name, fn):
        def counted(*a, **k):
            self.n[name] += 1
            return fn(*a, **k)

        return counted

    def take(self):
        got = (self.n["encoder"], self.n["encoder_infer"])
        self.n = {"encoder": 0, "encoder_infer": 0}
        return got


def _surfaces(mod, es, rows):
    """Every evaluation surface's result, as tensors / plain values."""
    hists = [mod._to_idx_or_empty(list(r["history"]["item_id"])) for r in rows]
    rec = mod.recommend_batch([r["history"]["item_id"] for r in rows], top_k=10)
    return {
        "encode_batch": mod.model.encode_batch(hists),
        "encode": mod.model.encode(rows[4]["history"]["item_id"]),
        "evalset.encode": es.encode(),
        "evalset.evaluate": es.evaluate(),
        "recommend_batch.item_idx": rec["item_idx"], "recommend_batch.score": rec["score"],
        "recommend": mod.recommend(rows[5]["history"]["item_id"], top_k=10)["item_idx"],
    }


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_surfaces_take_the_forward_only_entry_and_keep_their_bits(precision, monkeypatch):
    import xfmr_rec_amd as X
    from xfmr_rec_amd import _native as N
    from xfmr_rec_amd import ops

    mod = _module(precision)
    mod.eval()
    rows = _rows()
    es = X.DeviceEvalSet.from_rows(mod, rows, batch_size=8)
    assert es.packed == (precision == "bf16") == mod.model.supports_packed_rows(L) and len(es) == USERS
    step_before = mod.model._step

    # ops.encoder_infer against ops.encoder in eval mode, and the workspace it ran in
    m = mod.model
    idx = torch.zeros(USERS, L, dtype=torch.int64)
    for b, r in enumerate(rows):
        h = mod._to_idx_or_empty(list(r["history"]["item_id"]))[-L:]
        idx[b, :len(h)] = torch.as_tensor(h)
    idx = idx.to(DEV)
    kw = m._cfg_kwargs(USERS, L)
    with torch.no_grad():
        want_tok, want_km = ops.encoder(m.flat, idx, m.embeddings, kw)
        tok, km = ops.encoder_infer(m.flat, idx, m.embeddings, kw)
    assert torch.equal(tok, want_tok) and torch.equal(km, want_km)
    assert not tok.requires_grad and tok.grad_fn is None
    need = N.load().xfmr_encoder_infer_workspace_bytes(C.byref(ops.make_encoder_cfg(**kw)))
    assert ops.last_infer_workspace_nbytes == need > 0
    assert need < N.load().xfmr_encoder_workspace_bytes(C.byref(ops.make_encoder_cfg(**kw)))
    assert m.flat.requires_grad
    with pytest.raises(RuntimeError, match="forward-only"):  # grad mode on and a parameter that expects a gradient
        ops.encoder_infer(m.flat, idx, m.embeddings, kw)
    with torch.inference_mode():
        tok_i, _ = ops.encoder_infer(m.flat, idx, m.embeddings, kw)
    assert torch.equal(tok_i, want_tok)
    with pytest.raises(RuntimeError, match="eval"):  # forward(inference=True) is for eval mode
        m.train()
        try:
            with torch.no_grad():
                m(idx, inference=True)
        finally:
            m.eval()

    count = Counters(monkeypatch)
    monkeypatch.delenv("XFMR_INFER", raising=False)
    got = _surfaces(mod, es, rows)
    n_train, n_infer = count.take()
    assert n_train == 0 and n_infer >= 7, (n_train, n_infer)  # by default: only the forward-only entry
    monkeypatch.setenv("XFMR_INFER", "0")
    want = _surfaces(mod, es, rows)
    n_train, n_infer2 = count.take()
    assert n_infer2 == 0 and n_train == n_infer, (n_train, n_infer2)  # XFMR_INFER=0: only the training forward, as often
    monkeypatch.delenv("XFMR_INFER")
    assert set(got) == set(want)
    for k in got:
        if isinstance(got[k], dict):
            assert got[k] == want[k], k  # the metric means: the same floats
            assert got[k]["val/num_rows"] == USERS
        else:
            assert torch.equal(got[k], want[k]), k
            assert not got[k].requires_grad
    assert float(got["encode_batch"].abs().max()) > 0 and bool(torch.isfinite(got["evalset.encode"]).all())

    # forward(): the default keeps returning token embeddings that can be back-propagated -- through the training forward
    out = m(idx)
    assert count.take() == (1, 0) and out["token_embeddings"].requires_grad
    with torch.no_grad():
        inf = m(idx, inference=True)
    assert count.take() == (0, 1)
    for k in ("token_embeddings", "sentence_embedding", "attention_mask"):
        assert torch.equal(inf[k], out[k].detach()), k
    m.train()
    m(idx)["token_embeddings"].sum().backward()
    assert count.take() == (1, 0) and m.flat.grad is not None  # training mode: only the training forward
    m.eval()
    # nothing a following training step reads has moved: the step count is what forward() in training mode made it
    assert m._step == step_before + 1


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_training_is_not_disturbed_by_encode_batch_between_steps(precision):
    g = torch.Generator().manual_seed(0)
    batches = []
    for i in range(3):
        b = {k: torch.randint(1, V + 1, (4, L), generator=g) for k in ("history_item_idx", "pos_item_idx", "neg_item_idx")}
        for k in b:
            b[k][1, 3 + 2 * i:] = 0  # one ragged row
        batches.append({k: v.to(DEV) for k, v in b.items()})
    hists = [[1, 2, 3], [4], list(range(5, 25))]
    runs = []
    for with_eval in (False, True):
        mod = _module(precision)
        mod.train()
        opt = mod.configure_optimizers()
        losses = []
        for i, batch in enumerate(batches):
            opt.zero_grad(set_to_none=True)
            loss = mod.training_step(batch)
            loss.backward()
            mod.on_train_batch_end(loss, batch, i)
            opt.step()
            losses.append(loss.detach().clone())
            if with_eval:
                step, ctx = mod.model._step, getattr(mod.model, "_context", None)
                emb = mod.model.encode_batch(hists)
                assert emb.shape == (3, H) and mod.model.training
                assert mod.model._step == step and getattr(mod.model, "_context", None) is ctx
        torch.cuda.synchronize()
        runs.append((losses, mod.model.flat.detach().clone()))
    (l0, p0), (l1, p1) = runs
    for a, b in zip(l0, l1):
        assert torch.equal(a, b)
    assert torch.equal(p0, p1)


def test_opcheck_and_a_traced_eval_encode():
    from xfmr_rec_amd import ops

    mod = _module("bf16")
    mod.eval()
    m = mod.model
    g = torch.Generator().manual_seed(2)
    idx = torch.randint(1, V + 1, (4, L), generator=g)
    idx[1, 5:] = 0
    idx[3, 1:] = 0
    idx = idx.to(DEV)
    args = (m.flat.detach(), idx, m.embeddings, *ops.encoder_op_args(**m._cfg_kwargs(4, L)))
    torch.library.opcheck(torch.ops.xfmr.encoder_infer, args,
                          test_utils=("test_schema", "test_faketensor", "test_autograd_registration", "test_aot_dispatch_static"))
    with torch.no_grad():
        want = m(idx, inference=True)
        ref = m(idx)
    assert torch.equal(want["sentence_embedding"], ref["sentence_embedding"])

    def encode(i):  # what encode_batch does with a padded batch, as a traceable function
        return m(i, inference=True)["sentence_embedding"]

    torch._dynamo.reset()
    traced = torch.compile(encode, backend="aot_eager", fullgraph=True)
    with torch.no_grad():
        got = traced(idx)
    assert torch.equal(got, want["sentence_embedding"])
