"""Both sequence samplers (csrc/sampler.hip: ``xfmr_seq_sample``, ``xfmr_seq_sample_rows``) against the exact host model of
their output (tests/sampler_model.py), value for value: no tolerance, no frequencies.

Every case of tests/sampler_cases.py is ONE launch into buffers filled with -7; ``hist``, ``pos``, ``neg`` (and ``len`` for
`rows`) must equal the model's arrays. tests/test_sampler_model_host.py proves on the CPU that each case reaches the branch it
is named for -- threshold ties of the positions' and the exact path's selections, the regime limits A = cnt - 1, cnt, cnt + 1,
4 cnt - 1, 4 cnt, rounds with both rejection reasons, the walk-forward, window ends, 64-bit seeds and epochs, zero rows -- and
that the model itself keeps the reference's guarantees and its uniformity. The loader is held to the model on its own epoch
order, batch by batch.

Not reachable, hence recorded (profiles/sampler_exact.md) and not tested: 32 rejection rounds that leave a slot open
(probability below 4^-32 per slot), and dataset row indices at or beyond 2^32 (the high word of the row in ``row_key``)."""

import numpy as np
import pytest
import torch

import sampler_cases as SC
import sampler_model as SM
from test_gpu_epoch_loader import _dataset, _sample

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAMES = ("hist", "pos", "neg", "len")


def _sample_seq(ds, rows, *, width, seed, n_items=None, max_history=None):
    """One direct call of xfmr_seq_sample (the twin of test_gpu_epoch_loader._sample); numpy outputs ``hist, pos, neg``.
    ``max_history``: None = the dataset's longest row."""
    from xfmr_rec_amd import _native as N

    lib = N.load()
    rows_t = torch.as_tensor(np.asarray(rows, dtype=np.int64)).to(DEV)
    max_history = int(ds.lengths.max()) if max_history is None else max_history
    n_items = ds.n_items if n_items is None else n_items
    out = [torch.full((len(rows), width), -7, dtype=torch.int64, device=DEV) for _ in range(3)]
    nbytes = lib.xfmr_seq_sample_workspace(len(rows), n_items)
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=DEV)
    N.check(lib.xfmr_seq_sample(
        N.ptr(ds.items), N.ptr(ds.labels), N.ptr(ds.offsets), N.ptr(rows_t), len(rows), width, ds.config.max_seq_length,
        ds.config.pos_lookahead, n_items, max_history, seed, N.ptr(out[0]), N.ptr(out[1]), N.ptr(out[2]), N.ptr(ws),
        nbytes, N.stream()), "xfmr_seq_sample")
    return [t.cpu().numpy() for t in out]


def _sample_rows_max_history(ds, order, batch, *, width, max_history, first=0, seed=0, epoch=0):
    """test_gpu_epoch_loader._sample with a ``max_history`` below the dataset's longest row (which that helper always passes)."""
    from xfmr_rec_amd import _native as N

    lib = N.load()
    order_t = torch.as_tensor(np.asarray(order, dtype=np.int64)).to(DEV)
    out = [torch.full((batch, width), -7, dtype=torch.int64, device=DEV) for _ in range(3)]
    ln = torch.full((batch,), -7, dtype=torch.int32, device=DEV)
    N.check(lib.xfmr_seq_sample_rows(
        N.ptr(ds.items), N.ptr(ds.labels), N.ptr(ds.offsets), len(ds), N.ptr(order_t), len(order_t), first, batch, width,
        ds.config.max_seq_length, ds.config.pos_lookahead, ds.n_items, max_history, seed, epoch, N.ptr(out[0]), N.ptr(out[1]),
        N.ptr(out[2]), N.ptr(ln), None, 0, N.stream()), "xfmr_seq_sample_rows")
    return [t.cpu().numpy() for t in out] + [ln.cpu().numpy()]


def _explain(label, want, got, traces):
    """The first row and slot at which a launch leaves the model, with the model's trace of that row."""
    for name, w, g in zip(NAMES, want, got):
        if not np.array_equal(w, g):
            bad = np.argwhere(np.asarray(w) != np.asarray(g))[0] if np.shape(w) == np.shape(g) else None
            b = int(bad[0]) if bad is not None else 0
            tr = {k: v for k, v in (traces[b] or {}).items() if k != "positions"}
            return (f"{label}: `{name}` leaves the model at row {b}, slot {bad[1:].tolist() if bad is not None else '?'}:\n"
                    f"  model  {np.asarray(w)[b].tolist()}\n  kernel {np.asarray(g)[b].tolist()}\n  trace  {tr}\n"
                    f"  positions {None if traces[b] is None else traces[b]['positions'].tolist()}")
    return None


_datasets = {}


def _ds(c):
    key = (id(c.hs), c.n_items, c.L, c.lookahead)
    if key not in _datasets:
        _datasets[key] = _dataset(c.hs, c.ls, c.n_items, L=c.L, lookahead=c.lookahead)
    return _datasets[key]


@pytest.mark.parametrize("name,kernel", SC.RUNS)
def test_launch_equals_the_model(name, kernel):
    c = SC.BY_NAME[name]
    want = SC.model(c, kernel)
    ds = _ds(c)
    if kernel == "seq":
        got = _sample_seq(ds, c.order, width=c.width, seed=c.seed, max_history=c.max_history)
        want_arrays = want[:3]
    elif c.max_history is not None:
        got = _sample_rows_max_history(ds, c.order, c.batch, width=c.width, max_history=c.max_history, first=c.first,
                                       seed=c.seed, epoch=c.epoch)
        want_arrays = want[:4]
    else:
        got = _sample(ds, c.order, c.batch, width=c.width, first=c.first, seed=c.seed, epoch=c.epoch)
        want_arrays = want[:4]
    msg = _explain(f"{name} [{kernel}]", want_arrays, got, want[4])
    if msg:
        print(msg)
    for w, g in zip(want_arrays, got):
        assert g.shape == w.shape and g.dtype == w.dtype
        assert np.array_equal(w, g), msg


def test_sample_batch_equals_the_model():
    """``DeviceSeqDataset.sample_batch``: the width is the batch's longest row, the seed goes through its 64-bit mask."""
    c = SC.BY_NAME["lengths-lookahead3"]
    ds = _ds(c)
    for rows, seed in ((np.array([1, 0]), 2**63 + 5), (np.arange(len(c.hs)), -1)):
        got = {k: v.cpu().numpy() for k, v in ds.sample_batch(rows, seed).items()}
        width = int(max(1, min(c.L, max(len(c.hs[r]) for r in rows) - 1)))
        h, p, n, tr = SM.seq_sample(c.hs, c.ls, rows, seed, max_seq_length=c.L, width=width, lookahead=c.lookahead,
                                    n_items=c.n_items)
        want = (h, p, n, np.array([t["cnt"] for t in tr]))
        keys = ("history_item_idx", "pos_item_idx", "neg_item_idx", "lengths")
        msg = _explain(f"sample_batch seed {seed}", want, [got[k] for k in keys], tr)
        assert msg is None, msg


@pytest.mark.parametrize("world", [(0, 1), (1, 2)])
def test_loader_batches_equal_the_model(world):
    """11 rows, batches of 4 (a short last one), shuffled, two epochs; alone and as rank 1 of 2."""
    from xfmr_rec_amd.data import DeviceSeqLoader

    c = SC.BY_NAME["lengths-lookahead3"]
    ds = _ds(c)
    assert len(c.hs) == 11
    rank, world_size = world
    ld = DeviceSeqLoader(ds, 4, shuffle=True, seed=2**32 + 9, rank=rank, world_size=world_size)
    seen = 0
    try:
        for epoch in (0, 1):
            ld.set_epoch(epoch)
            nb = len(ld)
            assert nb == (3 if world_size == 1 else 2)
            for i, batch in enumerate(ld):
                rows = ld.batch_rows(i)
                width = ld.batch_width(i)
                want = SM.rows_sample(c.hs, c.ls, rows, len(rows), seed=ld.seed, epoch=epoch, max_seq_length=c.L, width=width,
                                      lookahead=c.lookahead, n_items=c.n_items)
                got = [batch[k].cpu().numpy() for k in ("history_item_idx", "pos_item_idx", "neg_item_idx")]
                got.append(batch["lengths"].numpy())
                assert got[0].shape == (len(rows), width) and len(rows) == (4 if i < nb - 1 else ld.rows_per_epoch - 4 * i)
                msg = _explain(f"loader {world} epoch {epoch} batch {i}", want[:4], got, want[4])
                assert msg is None, msg
                seen += len(rows)
        assert seen == 2 * ld.rows_per_epoch
    finally:
        ld.close()
