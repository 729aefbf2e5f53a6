"""Host side of the full-state checkpoints (no GPU, nothing launches): the file format and its atomic write, ``max_time``
parsing, the reference's ``config.yaml`` values, ``EarlyStopping``'s state, and the compatibility refusals of
``Trainer.load_state_dict`` over a trainer and a loader that live on the CPU."""

import datetime
import os

import numpy as np
import pytest
import torch

import xfmr_rec_amd as X
from xfmr_rec_amd import checkpoint as CK
from xfmr_rec_amd.data import DeviceSeqDataset, DeviceSeqLoader, SeqDataConfig
from xfmr_rec_amd.trainer import reference_fit_options

CONF = dict(hidden_size=64, num_attention_heads=2, intermediate_size=128, num_hidden_layers=1, max_seq_length=8)


def _trainer(conf=CONF, **kw):
    return X.Trainer(X.RecommenderLightningModule(X.LightningConfig(**conf)), **kw)


def _loader(rows=40, batch=8, **kw):
    rng = np.random.default_rng(0)
    lens = [int(x) for x in rng.integers(2, 30, rows)]
    hs = [rng.integers(1, 201, n) for n in lens]
    ds = DeviceSeqDataset(SeqDataConfig(max_seq_length=8, pos_lookahead=0), hs, [np.ones(n, dtype=bool) for n in lens], 200,
                          device="cpu")
    return DeviceSeqLoader(ds, batch, **kw)


def _state(**kw):
    """A trainer's state with optimizer moments in it (filled by hand: no step runs without a device)."""
    tr = _trainer(**kw)
    flat = tr.module.model.flat
    g = torch.Generator().manual_seed(1)
    tr.optimizer.state[flat] = {"step": 7, "exp_avg": torch.randn(flat.shape, generator=g),
                                "exp_avg_sq": torch.rand(flat.shape, generator=g)}
    tr.module.model._step = 7
    tr._loop = {**tr._empty_loop(), "batches_done": 7, "epoch": 1, "next_batch": 2, "best_score": np.float64(0.25),
                "val_history": [{"step": 4, "epoch": 0, "val/retrieval_normalized_dcg": np.float64(0.25), "val/num_rows": 12}],
                "tracker": {"best": 0.25, "wait": 0, "improved": True}}
    return tr


# ------------------------------------------------------------------------------------------------ the file
def test_round_trip_survives_weights_only_and_checks_format_and_version(tmp_path):
    tr = _state(gradient_clip_val=0.5, lr_scheduler={"name": "warmup_cosine", "warmup_steps": 2, "total_steps": 9})
    ld = _loader(seed=3)
    path = tmp_path / "sub" / "last.ckpt"
    size = tr.save_checkpoint(path, loader=ld)
    assert size == os.path.getsize(path) and os.listdir(path.parent) == ["last.ckpt"]
    raw = torch.load(str(path), weights_only=True, map_location="cpu")  # nothing pickled beyond tensors and plain values
    assert set(raw) == set(CK.KEYS) and raw["format"] == "xfmr-trainer-checkpoint" and raw["version"] == 1
    state = CK.read_checkpoint(path)
    flat = tr.module.model.flat.detach()
    pre = "model.model.0.auto_model."
    assert set(state["state_dict"]) == set(tr.module.state_dict()) and all(k.startswith(pre) for k in state["state_dict"])
    live = {k: v.cpu() for k, v in tr.module.state_dict().items()}  # (the module sits on the device where there is one)
    assert all(torch.equal(v, live[k]) for k, v in state["state_dict"].items())
    assert CK.state_flat_numel(state) == flat.numel()
    assert size < 3 * 4 * flat.numel() + 65536  # parameters and two moments, each ONCE (the keyed tensors share a storage)
    assert state["hyper_parameters"] == {"config": CK.plain(tr.module.config.model_dump())}
    assert (state["epoch"], state["global_step"]) == (1, 7)
    st = state["optimizer"]["state"][0]
    assert st["step"] == 7 and torch.equal(st["exp_avg"], tr.optimizer.state[tr.module.model.flat]["exp_avg"])
    assert torch.equal(st["exp_avg_sq"], tr.optimizer.state[tr.module.model.flat]["exp_avg_sq"])
    assert state["model"] == {"dropout_step": 7, "seed": 0, "device_step": False}
    assert state["trainer"] == {"accumulate_grad_batches": 1, "gradient_clip_algorithm": "norm", "gradient_clip_val": 0.5,
                                "lr_scheduler": {"name": "warmup_cosine", "warmup_steps": 2, "total_steps": 9}, "world_size": 1}
    assert state["loader"] == {"seed": 3, "batch_size": 8, "shuffle": True, "drop_last": False, "rank": 0, "world_size": 1,
                               "dataset_length": 40, "fixed_width": False}
    loop = state["loop"]
    assert (loop["batches_done"], loop["epoch"], loop["next_batch"]) == (7, 1, 2)
    assert type(loop["best_score"]) is float and loop["best_score"] == 0.25
    assert loop["val_history"] == [{"step": 4, "epoch": 0, "val/retrieval_normalized_dcg": 0.25, "val/num_rows": 12}]
    # ... and into a trainer built from other weights: everything comes back, the loader stands at the loop's position
    new = _trainer(gradient_clip_val=0.5, lr_scheduler={"name": "warmup_cosine", "warmup_steps": 2, "total_steps": 9})
    with torch.no_grad():
        new.module.model.flat.mul_(0.5)
    ld2 = _loader(seed=3)
    got = new.load_checkpoint(path, loader=ld2)
    assert got == loop and ld2.state_dict() == {"epoch": 1, "next_batch": 2}
    assert torch.equal(new.module.model.flat, flat)
    st2 = new.optimizer.state[new.module.model.flat]
    assert st2["step"] == 7 and torch.equal(st2["exp_avg"].cpu(), st["exp_avg"].cpu())
    assert torch.equal(st2["exp_avg_sq"].cpu(), st["exp_avg_sq"].cpu())
    assert new.module.model._step == 7 and getattr(new.module.model, "step_device", None) is None
    assert new.val_history == loop["val_history"] and new.best_score == 0.25
    assert new.optimizer.param_groups[0]["betas"] == (0.9, 0.999)
    # other formats and versions are refused by name
    for key, value, word in (("version", 2, "version 2"), ("format", "something-else", "format")):
        torch.save({**raw, key: value}, str(tmp_path / "other.ckpt"))
        with pytest.raises(ValueError, match=word):
            CK.read_checkpoint(tmp_path / "other.ckpt")
    with pytest.raises(ValueError, match="version"):
        CK.write_checkpoint({**raw, "version": 3}, tmp_path / "never.ckpt")
    with pytest.raises(TypeError, match="loop"):
        CK.plain({"loop": {"x": np.zeros(3)}}["loop"], "loop")  # no numpy arrays, no objects
    assert not (tmp_path / "never.ckpt").exists()


def test_a_failed_write_leaves_the_previous_file_and_no_temporary(tmp_path, monkeypatch):
    tr = _state()
    path = tmp_path / "last.ckpt"
    tr.save_checkpoint(path)
    before = path.read_bytes()
    real_save = torch.save

    def half_a_file(obj, f, *a, **k):
        f.write(b"PK\x03\x04 half a file")
        f.flush()
        raise OSError("disk full")

    monkeypatch.setattr(CK.torch, "save", half_a_file)
    tr._loop = {**tr._loop, "batches_done": 9}
    with pytest.raises(OSError, match="disk full"):
        tr.save_checkpoint(path)
    monkeypatch.setattr(CK.torch, "save", real_save)
    assert os.listdir(tmp_path) == ["last.ckpt"] and path.read_bytes() == before
    assert CK.read_checkpoint(path)["loop"]["batches_done"] == 7
    # a failing rename cleans up as well
    monkeypatch.setattr(CK.os, "replace", lambda *a: (_ for _ in ()).throw(OSError("no rename")))
    with pytest.raises(OSError, match="no rename"):
        tr.save_checkpoint(path)
    monkeypatch.undo()
    assert os.listdir(tmp_path) == ["last.ckpt"] and path.read_bytes() == before
    tr.save_checkpoint(path)
    assert CK.read_checkpoint(path)["loop"]["batches_done"] == 9


# ------------------------------------------------------------------------------------------------ max_time, the reference's values
def test_parse_max_time():
    assert CK.parse_max_time("00:04:00:00") == 14400.0 and X.parse_max_time("01:02:03:04") == 93784.0
    assert CK.parse_max_time({"days": 1, "hours": 2, "minutes": 3, "seconds": 4.5}) == 93784.5
    assert CK.parse_max_time({"minutes": 90}) == 5400.0
    assert CK.parse_max_time(datetime.timedelta(hours=4)) == 14400.0
    assert CK.parse_max_time(None) is None
    assert CK.parse_max_time(30) == 30.0 and type(CK.parse_max_time(30)) is float and CK.parse_max_time(1e-9) == 1e-9
    for bad in ("4h", "04:00:00", "00:04:00:xx", "", {"weeks": 1}, {}, {"hours": "4"}, [4], True, float("nan"), object()):
        with pytest.raises(ValueError, match="max_time"):
            CK.parse_max_time(bad)


def _reference_cfg(**trainer):
    block = {"accelerator": "cpu", "max_epochs": 1, "min_epochs": None, "max_steps": -1, "max_time": "00:04:00:00",
             "limit_train_batches": 1, "limit_val_batches": 1, "val_check_interval": None, "check_val_every_n_epoch": 1,
             "accumulate_grad_batches": 1, "gradient_clip_val": None, "gradient_clip_algorithm": None,
             "use_distributed_sampler": True}
    block.update(trainer)
    return {"seed_everything": 0, "trainer": block,
            "data": {"config": {"max_seq_length": 32, "pos_lookahead": 0, "data_dir": "data", "batch_size": 32,
                                "num_workers": 0}},
            "optimizer": None, "lr_scheduler": None, "ckpt_path": None, "weights_only": None}


def test_reference_checkpoint_options_on_the_reference_values():
    assert CK.reference_checkpoint_options(_reference_cfg()) == {"max_time": 14400.0, "ckpt_path": None}
    assert X.reference_checkpoint_options({**_reference_cfg(max_time=None), "ckpt_path": "runs/last.ckpt"}) == {
        "max_time": None, "ckpt_path": "runs/last.ckpt"}
    assert CK.reference_checkpoint_options({**_reference_cfg(), "ckpt_path": ""})["ckpt_path"] is None  # the entry points' ""
    assert CK.reference_checkpoint_options({}) == {"max_time": None, "ckpt_path": None}
    with pytest.raises(ValueError, match=r"trainer\.max_time"):
        CK.reference_checkpoint_options(_reference_cfg(max_time="four hours"))
    with pytest.raises(ValueError, match="ckpt_path"):
        CK.reference_checkpoint_options({**_reference_cfg(), "ckpt_path": 3})


def test_reference_fit_options_still_returns_its_pinned_dict():
    assert reference_fit_options(_reference_cfg()) == {
        "max_epochs": 1, "check_val_every_n_epoch": 1, "limit_train_batches": 1, "max_steps": None,
        "val_check_interval": None, "batch_size": 32, "max_seq_length": 32, "pos_lookahead": 0}


# ------------------------------------------------------------------------------------------------ EarlyStopping
def test_early_stopping_state_round_trip_carries_wait_and_best():
    a = X.EarlyStopping("max", patience=3)
    assert [a.update(v) for v in (0.5, 0.4)] == [False, False]
    state = CK.plain(a.state_dict())
    assert state == {"best": 0.5, "wait": 1, "improved": False}
    b = X.EarlyStopping("max", patience=3)
    b.load_state_dict(state)
    assert (b.best, b.wait, b.improved) == (0.5, 1, False)
    assert [b.update(v) for v in (0.3, 0.2)] == [False, True] == [a.update(v) for v in (0.3, 0.2)]
    fresh = X.EarlyStopping("max", patience=3)
    assert [fresh.update(v) for v in (0.3, 0.2)] == [False, False]  # a rule that started from zero would go on
    empty = X.EarlyStopping("min", patience=None)
    empty.load_state_dict(X.EarlyStopping("min").state_dict())
    assert empty.best is None and empty.wait == 0


# ------------------------------------------------------------------------------------------------ refusals
def test_incompatible_checkpoints_are_refused_by_field_before_anything_is_touched():
    sched = {"name": "warmup_cosine", "warmup_steps": 2, "total_steps": 9}
    state = _state(accumulate_grad_batches=2, lr_scheduler=sched).state_dict(_loader(seed=3))
    same = dict(accumulate_grad_batches=2, lr_scheduler=sched)
    cases = [
        ("loader seed", same, dict(seed=4), CONF),
        ("loader batch_size", same, dict(seed=3, batch=4), CONF),
        ("loader world_size", same, dict(seed=3, world_size=2), CONF),
        ("loader drop_last", same, dict(seed=3, drop_last=True), CONF),
        ("loader fixed_width", same, dict(seed=3, fixed_width=True), CONF),
        ("loader shuffle", same, dict(seed=3, shuffle=False), CONF),
        ("loader dataset_length", same, dict(seed=3, rows=41), CONF),
        ("flat parameter count", same, dict(seed=3), {**CONF, "intermediate_size": 64}),
        ("accumulate_grad_batches", dict(lr_scheduler=sched), dict(seed=3), CONF),
        ("lr_scheduler", dict(accumulate_grad_batches=2, lr_scheduler={**sched, "total_steps": 10}), dict(seed=3), CONF),
        ("lr_scheduler", dict(accumulate_grad_batches=2), dict(seed=3), CONF),
        ("gradient_clip_algorithm", dict(**same, gradient_clip_val=0.5), dict(seed=3), CONF),  # (clipping on against off)
        ("world_size", dict(**same, world_size=2), dict(seed=3), CONF),
    ]
    for field, tkw, lkw, conf in cases:
        tr = _trainer(conf, **tkw)
        before = tr.module.model.flat.detach().clone()
        ld = _loader(**lkw)
        with pytest.raises(ValueError, match=field):
            tr.load_state_dict(state, loader=ld)
        assert torch.equal(tr.module.model.flat, before) and not tr.optimizer.state and tr.module.model._step == 0
        assert ld.state_dict() == {"epoch": 0, "next_batch": 0}
    with pytest.raises(ValueError, match="loader"):
        _trainer(**same).load_state_dict(state)  # taken over a loader, resumed over a plain iterable
    clipped = _state(gradient_clip_val=0.5).state_dict()
    with pytest.raises(ValueError, match="gradient_clip_val"):
        _trainer(gradient_clip_val=0.25).load_state_dict(clipped)
    with pytest.raises(ValueError, match="gradient_clip_algorithm"):
        _trainer(gradient_clip_val=0.5, gradient_clip_algorithm="value").load_state_dict(clipped)
    # what only bounds a run is not part of a checkpoint, and the same options load
    tr = _trainer(**same)
    assert tr.load_state_dict(state, loader=_loader(seed=3))["batches_done"] == 7
    assert not any(k in state["trainer"] or k in state["loop"]
                   for k in ("max_epochs", "max_steps", "val_check_interval", "limit_train_batches"))


def test_checkpoint_between_micro_batches_and_bad_fit_arguments_are_refused(tmp_path):
    tr = _trainer(accumulate_grad_batches=2)
    tr._micro = 1  # what one micro-batch of two leaves behind
    with pytest.raises(ValueError, match="micro-batches"):
        tr.save_checkpoint(tmp_path / "x.ckpt")
    assert os.listdir(tmp_path) == []
    tr._micro = 0
    with pytest.raises(ValueError, match="multiple of accumulate_grad_batches"):
        tr.fit([], checkpoint_every_n_steps=3, checkpoint_dir=tmp_path)
    with pytest.raises(ValueError, match="checkpoint_dir"):
        tr.fit([], checkpoint_every_n_steps=2)
    with pytest.raises(ValueError, match="checkpoint_dir"):
        tr.fit([], save_last=True)
    with pytest.raises(ValueError, match="checkpoint_every_n_steps"):
        tr.fit([], checkpoint_every_n_steps=0, checkpoint_dir=tmp_path)
    with pytest.raises(ValueError, match="max_time"):
        tr.fit([], max_time="soon")
    two = _trainer(world_size=2)
    for kw in (dict(ckpt_path=tmp_path / "x.ckpt"), dict(save_last=True, checkpoint_dir=tmp_path),
               dict(checkpoint_every_n_steps=2, checkpoint_dir=tmp_path), dict(max_time=60)):
        with pytest.raises(ValueError, match="world_size"):
            two.fit([], **kw)
    two.save_checkpoint(tmp_path / "rank.ckpt")  # the file itself works on any rank
    assert _trainer(world_size=2).load_checkpoint(tmp_path / "rank.ckpt")["batches_done"] == 0
