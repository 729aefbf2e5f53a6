"""Epoch training from a resident dataset: the loop's sampler (``xfmr_seq_sample_rows``), ``DeviceSeqLoader`` and
``Trainer.fit(loader, max_epochs=...)``.

The sampler is held to the reference's per-row guarantees (``oracle.sampler.check_example``, a restatement of
``xfmr_rec/data.py:669-805``) and to its frequencies (the tolerances of ``tests/test_sampler.py``); the loader to a direct
call of the entry point on its own epoch order; ``fit`` to a hand-written loop of the same steps, bit for bit."""

import numpy as np
import pytest
import torch

from oracle import sampler as OS

pytestmark = pytest.mark.gpu
DEV = "cuda"
V = 57
KEYS = ("history_item_idx", "pos_item_idx", "neg_item_idx")


def _sample(ds, order, batch, *, width, first=0, seed=0, epoch=0, n_items=None, workspace_bytes=None):
    """One direct call of xfmr_seq_sample_rows; numpy outputs ``hist, pos, neg, len``."""
    from xfmr_rec_amd import _native as N

    lib = N.load()
    order_t = torch.as_tensor(np.asarray(order, dtype=np.int64)).to(DEV)
    out = [torch.full((batch, width), -7, dtype=torch.int64, device=DEV) for _ in range(3)]
    ln = torch.full((batch,), -7, dtype=torch.int32, device=DEV)
    nbytes = lib.xfmr_seq_sample_rows_workspace(batch, width)
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=DEV)
    N.check(lib.xfmr_seq_sample_rows(
        N.ptr(ds.items), N.ptr(ds.labels), N.ptr(ds.offsets), len(ds), N.ptr(order_t), len(order_t), first, batch, width,
        ds.config.max_seq_length, ds.config.pos_lookahead, ds.n_items if n_items is None else n_items,
        int(ds.lengths.max()), seed, epoch, N.ptr(out[0]), N.ptr(out[1]), N.ptr(out[2]), N.ptr(ln), N.ptr(ws),
        nbytes, N.stream()), "xfmr_seq_sample_rows")
    return [t.cpu().numpy() for t in out] + [ln.cpu().numpy()]


def _dataset(hs, ls, n_items, L=32, lookahead=0):
    from xfmr_rec_amd.data import DeviceSeqDataset, SeqDataConfig

    return DeviceSeqDataset(SeqDataConfig(max_seq_length=L, pos_lookahead=lookahead), hs, ls, n_items)


def _labels(rng, n):
    l = rng.random(n) < 0.6
    l[-1] = True  # process_events trims everything after the last positive
    return l


def _crowded(rng, n_distinct, n=40):
    """A row of n events over exactly n_distinct items of 1..V: V - n_distinct items stay admissible."""
    items = rng.permutation(np.arange(1, V + 1))[:n_distinct]
    return np.concatenate([items, rng.choice(items, n - n_distinct)])[rng.permutation(n)]


def _rows(seed=0):
    rng = np.random.default_rng(seed)
    hs = [rng.integers(1, V + 1, n) for n in (1, 2, 3, 9, 33, 255, 256, 257, 300)]
    hs.append(np.concatenate([np.arange(1, V + 1), rng.integers(1, V + 1, 20)]))  # covers the whole catalogue
    # 40 events -> cnt = 32 sampled positions; admissible items: exactly cnt, cnt + 1, cnt - 1
    hs += [_crowded(rng, V - 32), _crowded(rng, V - 33), _crowded(rng, V - 31)]
    return hs, [_labels(rng, len(h)) for h in hs]


def _check_rows(ds, hs, ls, rows, got, width, n_items, check=OS.check_example):
    hist, pos, neg, ln = got
    L, look = ds.config.max_seq_length, ds.config.pos_lookahead
    for b, r in enumerate(rows):
        pad = lambda a: np.concatenate([a[b], np.zeros(max(0, L - width), dtype=np.int64)])  # noqa: E731 - collate's zeros
        check(hs[r], ls[r], pad(hist), pad(pos), pad(neg), max_seq_length=L, pos_lookahead=look, n_items=n_items)
    cnt = np.minimum(ds.lengths[rows] - 1, min(L, width))
    assert (ln[: len(rows)] == cnt).all()
    assert (ln[: len(rows)] == (hist[: len(rows)] != 0).sum(1)).all()
    assert ((hist[: len(rows)] != 0) == (np.arange(width)[None, :] < cnt[:, None])).all()  # right-padded


# ------------------------------------------------------------------------------------------------ 1. invariants
@pytest.mark.parametrize("lookahead", [0, 3])
def test_rows_sampler_invariants_reproducibility_and_rows_past_the_order(lookahead):
    hs, ls = _rows()
    ds = _dataset(hs, ls, V, lookahead=lookahead)
    R = len(hs)
    crowded = [(R - 3, 32), (R - 2, 33), (R - 1, 31)]
    for r, want in crowded:  # (the set-up is what it claims to be)
        assert V - len(set(hs[r].tolist())) == want and min(len(hs[r]) - 1, 32) == 32
    order = np.random.default_rng(1).permutation(R)
    first = None
    for seed in range(6):
        got = _sample(ds, order, R + 2, width=32, seed=seed)  # two batch rows past n_order
        _check_rows(ds, hs, ls, order, got, 32, V)
        for a in got:
            assert (a[R:] == 0).all()  # all zero, length 0
        if seed == 0:
            first = got
            again = _sample(ds, order, R + 2, width=32, seed=0)
            assert all((x == y).all() for x, y in zip(got, again))
            other = _sample(ds, order, R + 2, width=32, seed=0, epoch=1)
            assert any((x != y).any() for x, y in zip(got, other))
            _check_rows(ds, hs, ls, order, other, 32, V)
        elif seed == 1:
            assert any((x != y).any() for x, y in zip(first, got))
    # width = the batch's longest row (pad_sequence), not max_seq_length
    short = np.array([3, 1, 0, 2])  # 9, 2, 1 and 3 events
    got = _sample(ds, short, 4, width=8, seed=2)
    assert got[0].shape == (4, 8)
    _check_rows(ds, hs, ls, short, got, 8, V)
    # a history of the longest supported length, against a catalogue that does not fit any bitmap in LDS
    Vb = 100_003
    rng = np.random.default_rng(4)
    hb = [rng.integers(1, Vb + 1, 8192), rng.integers(1, Vb + 1, 50)]
    lb = [_labels(rng, len(h)) for h in hb]
    big = _dataset(hb, lb, Vb, lookahead=lookahead)
    _check_rows(big, hb, lb, np.array([0, 1]), _sample(big, [0, 1], 2, width=32, seed=3), 32, Vb)


# ------------------------------------------------------------------------------------------------ 2. batch composition
def test_a_row_samples_the_same_values_in_any_batch_and_slot():
    hs, ls = _rows()
    ds = _dataset(hs, ls, V, lookahead=3)
    for r in (5, 8, len(hs) - 2):  # 255 and 300 events (positions are drawn), a crowded row (exact path)
        small = np.array([r, 0, 3])
        large = np.array([1, 2, 3, 4, 6, 7, 9, r, 0, 10, 11])
        a = _sample(ds, small, 3, width=32, seed=11, epoch=4)
        b = _sample(ds, large, 11, width=32, seed=11, epoch=4)
        for x, y in zip(a, b):
            assert (x[0] == y[7]).all()
        # ... and at another offset into a longer order
        c = _sample(ds, np.concatenate([np.arange(5), large]), 11, width=32, first=5, seed=11, epoch=4)
        assert all((y == z).all() for y, z in zip(b, c))


# ------------------------------------------------------------------------------------------------ 3. frequencies
def _tv(a, b):
    a, b = a / a.sum(), b / b.sum()
    return 0.5 * np.abs(a - b).sum()


@pytest.mark.parametrize("items,L,left", [(57, 16, 0), (40, 16, 17), (8, 12, 49)])
def test_negative_frequencies_match_the_oracle(items, L, left):
    """The set-up and tolerances of tests/test_sampler.py::test_device_sampler_frequencies_match_the_oracle -- whose row
    covers the whole catalogue (items = 57: negatives from all of it) -- and the same row folded onto fewer items, so that
    an admissible set exists: 17 items for 16 draws (the exact path) and 49 for 12 (the rejection rounds)."""
    rng = np.random.default_rng(7)
    n, look = 90, 5
    h = rng.permutation(np.arange(1, n + 1)) % items + 1
    l = rng.random(n) < 0.5
    l[-1] = True
    allowed = np.setdiff1d(np.arange(1, V + 1), h)
    assert len(allowed) == left
    ds64 = _dataset([h] * 64, [l] * 64, V, L=L, lookahead=look)  # 64 copies: every dataset row has its own stream
    dev_neg = np.zeros(V + 1)
    got = 0
    for seed in range(4000 // 64 + 1):
        hist, pos, neg, _ = _sample(ds64, np.arange(64), 64, width=L, seed=seed)
        for r in range(64):
            OS.check_example(h, l, hist[r], pos[r], neg[r], max_seq_length=L, pos_lookahead=look, n_items=V)
            np.add.at(dev_neg, neg[r], 1)
        got += 64
    assert got >= 4000
    orng = np.random.default_rng(11)
    ora_neg = np.zeros(V + 1)
    for _ in range(got):
        np.add.at(ora_neg, OS.get_item(orng, h, l, max_seq_length=L, pos_lookahead=look, n_items=V)["neg_item_idx"], 1)
    tv = _tv(dev_neg[1:] + 1e-9, ora_neg[1:] + 1e-9)
    print(f"items {items}: total variation against the oracle {tv:.4f} (limit 0.03)")
    assert tv < 0.03
    if left:
        assert dev_neg[allowed].sum() == dev_neg.sum()  # inside the admissible set only
        f = dev_neg[allowed] / dev_neg[allowed].sum()
        assert np.abs(f - 1 / len(allowed)).max() < 0.25 / len(allowed) + 0.01


def test_position_and_positive_frequencies():
    """tests/test_sampler.py::test_device_sampler_position_and_positive_frequencies on the new entry point: unique items
    make the positions recoverable; each is chosen with probability L / (n - 1), its positive uniformly in its window."""
    Vb, n, L, look = 400, 60, 12, 4
    rng = np.random.default_rng(3)
    h = rng.permutation(np.arange(1, Vb + 1))[:n]
    l = rng.random(n) < 0.5
    l[-1] = True
    ds = _dataset([h] * 128, [l] * 128, Vb, L=L, lookahead=look)
    where = {int(v): i for i, v in enumerate(h)}
    cnt_pos = np.zeros(n - 1)
    pair = {}
    total = 0
    for seed in range(40):
        hist, pos, _, _ = _sample(ds, np.arange(128), 128, width=L, seed=seed)
        for r in range(128):
            ps = [where[int(v)] for v in hist[r]]
            assert ps == sorted(ps) and len(set(ps)) == L
            cnt_pos[ps] += 1
            for p, pv in zip(ps, pos[r]):
                pair.setdefault(p, {}).setdefault(int(pv), 0)
                pair[p][int(pv)] += 1
            total += 1
    assert total >= 4000
    f = cnt_pos / total
    assert np.abs(f - L / (n - 1)).max() < 0.03, (f.min(), f.max(), L / (n - 1))
    for p, d in pair.items():
        cand = h[p + 1:p + 1 + look][l[p + 1:p + 1 + look]]
        if len(cand) == 0:
            assert set(d) == {0}
        else:
            assert set(d) <= set(int(c) for c in cand)
            tot = sum(d.values())
            if tot > 300:
                assert max(abs(d.get(int(c), 0) / tot - 1 / len(cand)) for c in cand) < 0.08


@pytest.mark.parametrize("extra", [3, 0])
def test_crowded_row_includes_every_admissible_item_at_the_right_rate(extra):
    """cnt + extra admissible items, 4 096 draws of cnt negatives without replacement: every admissible item is included
    with probability cnt / (cnt + extra). extra = 3: the binomial standard deviation of a frequency over 4 096 draws is
    sqrt(p (1 - p) / 4096) <= 0.008, and the bound is five of them; extra = 0: every item, every time."""
    rng = np.random.default_rng(5)
    cnt = 32
    h = _crowded(rng, V - cnt - extra)
    l = _labels(rng, len(h))
    ds = _dataset([h] * 64, [l] * 64, V)
    allowed = np.setdiff1d(np.arange(1, V + 1), h)
    assert len(allowed) == cnt + extra and min(len(h) - 1, 32) == cnt
    seen = np.zeros(V + 1)
    draws = 0
    for seed in range(64):
        _, _, neg, ln = _sample(ds, np.arange(64), 64, width=32, seed=seed)
        assert (ln == cnt).all()
        for r in range(64):
            assert len(set(neg[r].tolist())) == cnt and set(neg[r].tolist()) <= set(allowed.tolist())
            seen[neg[r]] += 1
        draws += 64
    assert draws == 4096 and seen.sum() == seen[allowed].sum()
    f = seen[allowed] / draws
    if extra == 0:
        assert (seen[allowed] == draws).all()
    else:
        assert np.abs(f - cnt / (cnt + extra)).max() < 0.04, (f.min(), f.max(), cnt / (cnt + extra))


# ------------------------------------------------------------------------------------------------ 4. catalogue size
class _RangeAsSet:
    """``set(range(lo, hi))`` without its elements: ``check_example`` intersects the history with the whole catalogue, which
    at 5e7 items is 4 GB and six seconds per row as a real set. Same intersection, same assertions."""

    def __init__(self, r):
        self.r = r

    def __rand__(self, other):
        return {x for x in other if x in self.r}


def _lazy_set(x=()):
    return _RangeAsSet(x) if isinstance(x, range) and x.step == 1 else set(x)


def test_nothing_grows_with_the_catalogue(monkeypatch):
    from xfmr_rec_amd import _native as N

    lib = N.load()
    assert lib.xfmr_seq_sample_rows_workspace.argtypes == [N.C.c_int32, N.C.c_int32]  # no catalogue size to depend on
    hs, ls = _rows()
    small = _dataset(hs, ls, V)
    Vbig = 50_000_000
    rng = np.random.default_rng(8)
    lens = [1, 2, 9, 33, 64, 257, 300, 1000]
    hb = [rng.integers(1, Vbig + 1, n) for n in lens]
    hb[4][::2] = hb[4][1]  # repeated items
    lb = [_labels(rng, n) for n in lens]
    big = _dataset(hb, lb, Vbig)
    ws = {v: lib.xfmr_seq_sample_rows_workspace(8, 32) for v in (V, Vbig)}
    assert ws[V] == ws[Vbig] <= 8 * 32 * 8  # at most the size of one output, whatever the catalogue
    _check_rows(small, hs, ls, np.arange(8), _sample(small, np.arange(8), 8, width=32, seed=1), 32, V)
    assert (_lazy_set(range(1, V + 1)).__rand__(set(hs[5].tolist()) | {0, V + 1})) == set(hs[5].tolist())
    monkeypatch.setattr(OS, "set", _lazy_set, raising=False)
    got = _sample(big, np.arange(8), 8, width=32, seed=1)
    _check_rows(big, hb, lb, np.arange(8), got, 32, Vbig)
    assert got[2].max() > 2**24  # the draws do reach across the catalogue


# ------------------------------------------------------------------------------------------------ 5. loader
def _loader_dataset():
    rng = np.random.default_rng(2)
    R, span, L = 37, 20, 12
    lens = [2, 3, L, L + 1, L + 2, 40] + [int(x) for x in rng.integers(2, 30, R - 6)]
    hs = [1 + span * r + rng.integers(0, span, n) for r, n in enumerate(lens)]  # disjoint item ranges: items name the row
    ls = [_labels(rng, n) for n in lens]
    return _dataset(hs, ls, span * R, L=L), hs, ls, np.asarray(lens), span


def test_loader_epochs_prefetch_and_direct_calls_agree():
    from xfmr_rec_amd.data import DeviceSeqLoader

    ds, hs, ls, lens, span = _loader_dataset()
    R, B, L = len(hs), 8, 12
    loaders = {p: DeviceSeqLoader(ds, B, seed=5, prefetch=p) for p in (True, False)}
    orders = []
    for e in range(2):
        epoch = {}
        for p, ld in loaders.items():
            ld.set_epoch(e)
            assert len(ld) == 5
            epoch[p] = [{k: v.cpu().numpy().copy() for k, v in b.items()} for b in ld]  # (a slot is rewritten later on)
            assert len(epoch[p]) == 5 and ld.state_dict() == {"epoch": e, "next_batch": 0}
        order = loaders[True].epoch_order(e)
        orders.append(order)
        seen = []
        for i, (a, b) in enumerate(zip(epoch[True], epoch[False])):
            rows = order[B * i : B * i + B]
            assert set(a) == set(KEYS) | {"lengths"}
            assert all((a[k] == b[k]).all() for k in a)
            want_len = np.minimum(lens[rows] - 1, L)
            width = int(want_len.max())
            assert a["history_item_idx"].shape == (len(rows), width) and len(rows) == (5 if i == 4 else 8)
            assert (a["lengths"] == want_len).all() and a["lengths"].dtype == np.int64
            assert (a["lengths"] == (a["history_item_idx"] != 0).sum(1)).all()
            assert ((a["history_item_idx"][:, 0] - 1) // span == rows).all()  # the rows the order names
            direct = _sample(ds, order, len(rows), width=width, first=B * i, seed=5, epoch=e)
            assert all((a[k] == d).all() for k, d in zip(KEYS, direct))
            assert (direct[3] == want_len).all()
            _check_rows(ds, hs, ls, rows, direct, width, ds.n_items)
            seen += rows.tolist()
        assert sorted(seen) == list(range(R))  # every row exactly once per epoch
    assert (orders[0] != orders[1]).any()
    # a loader restored mid-epoch yields what the original would have yielded next; fixed_width pads to max_seq_length
    src = DeviceSeqLoader(ds, B, seed=5, fixed_width=True)
    src.set_epoch(1)
    it = iter(src)
    for _ in range(3):
        next(it)
    new = DeviceSeqLoader(ds, B, seed=5, fixed_width=True, prefetch=False)
    new.load_state_dict(src.state_dict())
    rest_src = [{k: v.cpu().numpy().copy() for k, v in b.items()} for b in it]
    rest_new = [{k: v.cpu().numpy().copy() for k, v in b.items()} for b in new]
    assert len(rest_src) == len(rest_new) == 2 and rest_src[0]["history_item_idx"].shape == (8, L)
    assert all((a[k] == b[k]).all() for a, b in zip(rest_src, rest_new) for k in a)
    for ld in (*loaders.values(), src, new):
        ld.close()
        ld.close()  # (idempotent)


# ------------------------------------------------------------------------------------------------ 6. fit
def _fit_setup():
    import xfmr_rec_amd as X
    from helpers import unit_table

    H, L, Vf, R = 64, 16, 200, 40
    rng = np.random.default_rng(6)
    lens = [int(x) for x in rng.integers(2, 30, R)]
    hs = [rng.integers(1, Vf + 1, n) for n in lens]
    ls = [_labels(rng, n) for n in lens]
    ds = _dataset(hs, ls, Vf, L=L)
    conf = X.LightningConfig(hidden_size=H, num_attention_heads=2, intermediate_size=2 * H, num_hidden_layers=1,
                             max_seq_length=L)
    table = unit_table(Vf, H, seed=7).to(DEV)
    rows = []
    for u in range(12):
        h = [f"i{x}" for x in rng.integers(1, Vf + 1, int(rng.integers(1, 20)))]
        t = [f"i{x}" for x in rng.integers(1, Vf + 1, 3)]
        rows.append({"history": {"item_id": h}, "target": {"item_id": t, "label": [True, False, True]}})

    def module(flat_from=None):
        mod = X.RecommenderLightningModule(conf)
        mod.configure_model()
        mod.model.set_table(table)
        mod.model.id2idx = {f"i{i}": i for i in range(1, Vf + 1)}
        if flat_from is not None:
            with torch.no_grad():
                mod.model.flat.copy_(flat_from.model.flat)
        return mod

    return X, ds, module, rows


def test_fit_runs_epochs_and_equals_the_hand_written_loop():
    from xfmr_rec_amd.data import DeviceSeqLoader
    from xfmr_rec_amd.params import HIDDEN_DROPOUT_PROB

    X, ds, module, rows = _fit_setup()
    first = module()
    assert HIDDEN_DROPOUT_PROB > 0  # dropout is on (fit_step trains): the step count is one sequence across epochs
    init = module(first)
    tr = X.Trainer(first)
    ld = DeviceSeqLoader(ds, 8, seed=3)
    es = X.DeviceEvalSet.from_rows(first, rows, batch_size=8)
    got = tr.fit(ld, max_epochs=2, val=es)
    assert len(got) == 10 and all(np.isfinite(got))
    assert [(h["step"], h["epoch"]) for h in tr.val_history] == [(5, 0), (10, 1)]
    assert ld.fixed_width is False and ld.state_dict() == {"epoch": 1, "next_batch": 0}
    twin = module(init)
    tr_t = X.Trainer(twin)
    ld_t = DeviceSeqLoader(ds, 8, seed=3, prefetch=False)
    want = []
    for e in range(2):
        ld_t.set_epoch(e)
        for b in ld_t:
            want.append(tr_t.fit_step(b))
    want = [float(v) for v in want]
    torch.cuda.synchronize()
    assert got == want and torch.equal(first.model.flat, twin.model.flat)
    # every n-th epoch only; an interval in batches goes on counting across epochs
    tr.fit(ld, max_epochs=2, val=es, check_val_every_n_epoch=2)
    assert [(h["step"], h["epoch"]) for h in tr.val_history] == [(10, 1)]
    tr.fit(ld, max_epochs=2, val=es, val_check_interval=4)
    assert [(h["step"], h["epoch"]) for h in tr.val_history] == [(4, 0), (8, 1)]
    # limits
    assert len(tr.fit(ld, max_epochs=2, limit_train_batches=3)) == 6
    assert len(tr.fit(ld, max_epochs=2, max_steps=7)) == 7 and ld.state_dict() == {"epoch": 1, "next_batch": 2}
    assert len(tr.fit(ld, max_epochs=2)) == 3  # ... and goes on from there: the three batches epoch 1 has left
    batches = [dict(b) for b in ld_t]
    with pytest.raises(ValueError, match="DeviceSeqLoader"):
        tr.fit(batches, max_epochs=2)
    with pytest.raises(ValueError, match="max_epochs"):
        tr.fit(ld, limit_train_batches=3)
    with pytest.raises(ValueError, match="world_size"):
        tr.fit(DeviceSeqLoader(ds, 8, rank=1, world_size=2), max_epochs=1)
    assert len(tr.fit(ld)) == 5  # a loader without max_epochs: one pass over its current epoch, as any iterable
    ld.close()
    ld_t.close()


def test_fit_with_a_captured_step_replays_the_loader_batches():
    from xfmr_rec_amd.data import SEQ_BATCH_KEYS, DeviceSeqLoader

    X, ds, module, _ = _fit_setup()
    graphed = module()
    eager = module(graphed)
    tr_g = X.Trainer(graphed)
    ld = DeviceSeqLoader(ds, 8, seed=3, drop_last=True, fixed_width=True)
    got = tr_g.fit(ld, max_epochs=2, graph="on")
    assert len(got) == 10 and tr_g.graph_choice == "graph" and ld.fixed_width is True
    eager.model.use_device_step(True)
    tr_e = X.Trainer(eager)
    tr_e.optimizer.step_device = eager.model.step_device
    ld_e = DeviceSeqLoader(ds, 8, seed=3, drop_last=True, fixed_width=True)
    want = []
    for e in range(2):
        ld_e.set_epoch(e)
        for b in ld_e:
            assert b["history_item_idx"].shape == (8, 16)
            want.append(tr_e.fit_step({k: b[k] for k in SEQ_BATCH_KEYS}))  # no lengths: the padded layout, as the replays
    want = [float(v) for v in want]
    torch.cuda.synchronize()
    assert got == want and torch.equal(graphed.model.flat, eager.model.flat)
    # a loader of ragged widths is switched to one width for the call, and back; its short last batch steps eagerly
    ragged = DeviceSeqLoader(ds, 16, seed=3)  # batches of 16, 16 and 8 rows: the capture (step 4) meets a full one
    tr_r = X.Trainer(module(graphed))
    out = tr_r.fit(ragged, max_epochs=3, graph="on")
    assert len(out) == 9 and tr_r.graph_choice == "graph" and ragged.fixed_width is False
    for l_ in (ld, ld_e, ragged):
        l_.close()
