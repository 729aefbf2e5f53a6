"""Host side of the epoch loop (no GPU, nothing launches): ``DeviceSeqLoader``'s epoch orders, sharding, batch geometry
and state over a dataset built with ``device="cpu"``, and ``reference_fit_options`` on the reference's ``config.yaml``
values."""

import numpy as np
import pytest

from xfmr_rec_amd.data import DeviceSeqDataset, DeviceSeqLoader, SeqDataConfig
from xfmr_rec_amd.trainer import reference_fit_options, reference_trainer_options

R, V, L = 37, 500, 12


def _dataset():
    rng = np.random.default_rng(0)
    lens = [1, 2, 3, L, L + 1, L + 2, 40] + [int(x) for x in rng.integers(1, 30, R - 7)]
    hs = [rng.integers(1, V + 1, n) for n in lens]
    ls = [np.ones(n, dtype=bool) for n in lens]
    return DeviceSeqDataset(SeqDataConfig(max_seq_length=L, pos_lookahead=0), hs, ls, V, device="cpu"), np.asarray(lens)


def test_epoch_order_is_a_seeded_permutation():
    ds, _ = _dataset()
    ld = DeviceSeqLoader(ds, 8, seed=3)
    o0, o1 = ld.epoch_order(0), ld.epoch_order(1)
    assert o0.dtype == np.int64 and sorted(o0.tolist()) == list(range(R)) == sorted(o1.tolist())
    assert (ld.epoch_order(0) == o0).all() and (DeviceSeqLoader(ds, 5, seed=3).epoch_order(0) == o0).all()
    assert (o0 != o1).any()
    assert (DeviceSeqLoader(ds, 8, seed=4).epoch_order(0) != o0).any()
    assert (DeviceSeqLoader(ds, 8, shuffle=False).epoch_order(5) == np.arange(R)).all()


def test_epoch_order_shards_like_distributed_sampler():
    ds, _ = _dataset()
    W = 4
    full = DeviceSeqLoader(ds, 8, seed=3).epoch_order(2)
    parts = [DeviceSeqLoader(ds, 8, seed=3, rank=r, world_size=W).epoch_order(2) for r in range(W)]
    assert [len(p) for p in parts] == [10] * W
    assert set(np.concatenate(parts).tolist()) == set(range(R))
    inter = np.stack(parts, axis=1).reshape(-1)  # rank r holds every W-th row from r on
    assert (inter[:R] == full).all() and (inter[R:] == full[:3]).all()  # the 3 extra rows: the wrapped head
    assert len(DeviceSeqLoader(ds, 8, rank=1, world_size=W)) == 2
    assert len(DeviceSeqLoader(ds, 8, rank=1, world_size=W, drop_last=True)) == 1
    with pytest.raises(ValueError, match="rank"):
        DeviceSeqLoader(ds, 8, rank=4, world_size=4)


def test_len_widths_and_lengths():
    ds, lens = _dataset()
    ld = DeviceSeqLoader(ds, 8, seed=1)
    assert len(ld) == 5 and len(DeviceSeqLoader(ds, 8, drop_last=True)) == 4
    ld.set_epoch(1)
    order = ld.epoch_order(1)
    seen = []
    for i in range(len(ld)):
        rows = ld.batch_rows(i)
        assert (rows == order[8 * i : 8 * i + 8]).all() and len(rows) == (8 if i < 4 else 5)
        want = np.minimum(lens[rows] - 1, L)
        assert (ld.batch_lengths(i) == want).all()
        assert ld.batch_width(i) == max(1, want.max())
        seen += rows.tolist()
    assert sorted(seen) == list(range(R))
    fixed = DeviceSeqLoader(ds, 8, seed=1, fixed_width=True)
    assert [fixed.batch_width(i) for i in range(len(fixed))] == [L] * 5
    # a batch of rows with one event each still has a column
    one = DeviceSeqDataset(SeqDataConfig(max_seq_length=L), [[3], [4]], [[True], [True]], V, device="cpu")
    assert DeviceSeqLoader(one, 2).batch_width(0) == 1
    with pytest.raises(IndexError):
        ld.batch_rows(5)


def test_state_dict_round_trip_mid_epoch():
    ds, _ = _dataset()
    ld = DeviceSeqLoader(ds, 8, seed=9)
    ld.set_epoch(1)
    ld.next_batch = 3  # what an iteration leaves behind once it has yielded batches 0, 1 and 2
    state = ld.state_dict()
    assert state == {"epoch": 1, "next_batch": 3}
    new = DeviceSeqLoader(ds, 8, seed=9)
    new.load_state_dict(state)
    assert new.state_dict() == state
    rest = [new.batch_rows(i).tolist() for i in range(new.next_batch, len(new))]
    assert rest == [ld.batch_rows(i).tolist() for i in (3, 4)]
    assert rest == [ld.epoch_order(1)[24:32].tolist(), ld.epoch_order(1)[32:].tolist()]
    new.set_epoch(2)
    assert new.state_dict() == {"epoch": 2, "next_batch": 0}


def test_iteration_without_a_device_is_an_error_not_a_fallback():
    ds, _ = _dataset()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        next(iter(DeviceSeqLoader(ds, 8)))


def _reference_cfg(**trainer):
    block = {"accelerator": "cpu", "max_epochs": 1, "min_epochs": None, "max_steps": -1, "limit_train_batches": 1,
             "limit_val_batches": 1, "val_check_interval": None, "check_val_every_n_epoch": 1, "accumulate_grad_batches": 1,
             "gradient_clip_val": None, "gradient_clip_algorithm": None, "use_distributed_sampler": True}
    block.update(trainer)
    return {"seed_everything": 0, "trainer": block,
            "data": {"config": {"max_seq_length": 32, "pos_lookahead": 0, "data_dir": "data", "batch_size": 32,
                                "num_workers": 0}},
            "optimizer": None, "lr_scheduler": None, "ckpt_path": None}


def test_reference_fit_options_on_the_reference_values():
    got = reference_fit_options(_reference_cfg())
    assert got == {"max_epochs": 1, "check_val_every_n_epoch": 1, "limit_train_batches": 1, "max_steps": None,
                   "val_check_interval": None, "batch_size": 32, "max_seq_length": 32, "pos_lookahead": 0}
    assert reference_fit_options(_reference_cfg(max_steps=40, limit_train_batches=None, val_check_interval=10)) == {
        **got, "max_steps": 40, "limit_train_batches": None, "val_check_interval": 10}
    with pytest.raises(ValueError, match="limit_train_batches"):
        reference_fit_options(_reference_cfg(limit_train_batches=0.5))
    with pytest.raises(ValueError, match="val_check_interval"):
        reference_fit_options(_reference_cfg(val_check_interval=0.25))
    with pytest.raises(ValueError, match="max_epochs"):
        reference_fit_options(_reference_cfg(max_epochs=-1))
    # the optimisation's keys are read by reference_trainer_options, as before
    assert reference_trainer_options(_reference_cfg()) == dict(gradient_clip_val=None, gradient_clip_algorithm=None,
                                                               accumulate_grad_batches=1, lr_scheduler=None)
