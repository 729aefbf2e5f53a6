"""Full-state checkpoints on the device: a run that stops, is written to a file and goes on in a NEW module (built from
other weights), a new ``Trainer`` and a new loader equals the run that never stopped -- losses, parameters, both AdamW
moments, the step count and the validation history, all compared exactly (float ``==`` / ``torch.equal``). Eagerly,
between the replays of a captured step, mid-epoch, at an epoch's last batch, under clipping + schedule + accumulation,
with early stopping, and when ``max_time`` ends the run.

Shapes: those of ``tests/test_gpu_epoch_loader.py::_fit_setup`` (H 64, 2 heads, I 128, 1 layer, L 16, V 200; 40 rows in
batches of 8: 5 batches per epoch; 12 validation rows). Dropout is on."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
H, L, V, R, B = 64, 16, 200, 40, 8


class _Setup:
    def __init__(self):
        import xfmr_rec_amd as X
        from helpers import unit_table
        from xfmr_rec_amd.data import DeviceSeqDataset, SeqDataConfig

        self.X = X
        rng = np.random.default_rng(6)
        lens = [int(x) for x in rng.integers(2, 30, R)]
        hs = [rng.integers(1, V + 1, n) for n in lens]
        ls = [np.concatenate([rng.random(n - 1) < 0.6, [True]]) for n in lens]
        self.ds = DeviceSeqDataset(SeqDataConfig(max_seq_length=L, pos_lookahead=0), hs, ls, V)
        self.conf = X.LightningConfig(hidden_size=H, num_attention_heads=2, intermediate_size=2 * H, num_hidden_layers=1,
                                      max_seq_length=L)
        self.table = unit_table(V, H, seed=7).to(DEV)
        self.rows = []
        for _ in range(12):
            h = [f"i{x}" for x in rng.integers(1, V + 1, int(rng.integers(1, 20)))]
            t = [f"i{x}" for x in rng.integers(1, V + 1, 3)]
            self.rows.append({"history": {"item_id": h}, "target": {"item_id": t, "label": [True, False, True]}})

    def module(self, other_weights=False):
        """The run's initial module; ``other_weights``: one that shares nothing with it (what a resumed run starts from)."""
        mod = self.X.RecommenderLightningModule(self.conf)
        mod.configure_model()
        mod.model.set_table(self.table)
        mod.model.id2idx = {f"i{i}": i for i in range(1, V + 1)}
        if other_weights:
            with torch.no_grad():
                mod.model.flat.mul_(-0.5).add_(0.01)
        return mod

    def loader(self, **kw):
        from xfmr_rec_amd.data import DeviceSeqLoader

        return DeviceSeqLoader(self.ds, B, **{"seed": 3, **kw})

    def evalset(self, mod):
        return self.X.DeviceEvalSet.from_rows(mod, self.rows, batch_size=8)


@pytest.fixture(scope="module")
def S():
    from xfmr_rec_amd.params import HIDDEN_DROPOUT_PROB

    assert HIDDEN_DROPOUT_PROB > 0  # the dropout stream's position is part of what a checkpoint has to carry
    return _Setup()


def _final(tr):
    torch.cuda.synchronize()
    flat = tr.module.model.flat
    st = tr.optimizer.state[flat]
    return {"flat": flat.detach().clone(), "exp_avg": st["exp_avg"].clone(), "exp_avg_sq": st["exp_avg_sq"].clone(),
            "step": int(tr.optimizer.state_dict()["state"][0]["step"]), "val_history": [dict(h) for h in tr.val_history],
            "best_score": tr.best_score, "best_step": tr.best_step}


def _same(got, want):
    for k in ("flat", "exp_avg", "exp_avg_sq"):
        assert torch.equal(got[k], want[k]), k
    assert got["step"] == want["step"]
    assert got["val_history"] == want["val_history"]  # steps, epochs and every metric value
    assert (got["best_score"], got["best_step"]) == (want["best_score"], want["best_step"])


def _straight(S, fit_kw, loader_kw=None, trainer_kw=None, with_val=True):
    mod = S.module()
    tr = S.X.Trainer(mod, **(trainer_kw or {}))
    ld = S.loader(**(loader_kw or {}))
    losses = tr.fit(ld, **fit_kw, **({"val": S.evalset(mod)} if with_val else {}))
    ld.close()
    return losses, _final(tr)


def _interrupted(S, stop_kw, fit_kw, d, loader_kw=None, trainer_kw=None, with_val=True):
    """``fit(**fit_kw, **stop_kw, save_last=True)``, then ``fit(**fit_kw, ckpt_path=last.ckpt)`` in a new module (other
    weights), a new trainer and a new loader: nothing survives except the file."""
    mod = S.module()
    tr = S.X.Trainer(mod, **(trainer_kw or {}))
    ld = S.loader(**(loader_kw or {}))
    val = {"val": S.evalset(mod)} if with_val else {}
    first = tr.fit(ld, **{**fit_kw, **stop_kw}, **val, save_last=True, checkpoint_dir=d)
    ld.close()
    mod2 = S.module(other_weights=True)
    assert not torch.equal(mod2.model.flat, mod.model.flat)
    tr2 = S.X.Trainer(mod2, **(trainer_kw or {}))
    ld2 = S.loader(**(loader_kw or {}))
    val2 = {"val": S.evalset(mod2)} if with_val else {}
    second = tr2.fit(ld2, **fit_kw, **val2, ckpt_path=d / "last.ckpt")
    ld2.close()
    return first, second, tr, tr2


# ------------------------------------------------------------------------------------------------ 1, 2: eager
@pytest.fixture(scope="module")
def straight_eager(S):
    return _straight(S, dict(max_epochs=3, val_check_interval=4))


def test_eager_resume_mid_epoch_equals_the_uninterrupted_run(S, straight_eager, tmp_path):
    want_losses, want = straight_eager
    assert len(want_losses) == 15 and [(h["step"], h["epoch"]) for h in want["val_history"]] == [(4, 0), (8, 1), (12, 2)]
    first, second, tr, tr2 = _interrupted(S, dict(max_steps=7), dict(max_epochs=3, val_check_interval=4), tmp_path)
    assert len(first) == 7 and len(second) == 8  # the returned list: this call's losses only
    assert first + second == want_losses
    _same(_final(tr2), want)
    state = S.X.read_checkpoint(tmp_path / "last.ckpt")
    assert (state["epoch"], state["global_step"]) == (1, 7) and state["model"]["device_step"] is False
    assert (state["loop"]["batches_done"], state["loop"]["epoch"], state["loop"]["next_batch"]) == (7, 1, 2)
    assert state["model"]["dropout_step"] == 7 and [h["step"] for h in state["loop"]["val_history"]] == [4]
    assert tr2.ckpt_elapsed == 0.0 and tr.ckpt_elapsed > 0.0 and not tr2.stopped_on_time


def test_resume_at_an_epoch_boundary_runs_the_next_epoch_only(S, straight_eager, tmp_path):
    want_losses, want = straight_eager
    first, second, _, tr2 = _interrupted(S, dict(max_steps=10), dict(max_epochs=3, val_check_interval=4), tmp_path)
    state = S.X.read_checkpoint(tmp_path / "last.ckpt")
    assert (state["loop"]["epoch"], state["loop"]["next_batch"]) == (2, 0)  # after the last batch of epoch 1: epoch 2
    assert len(first) == 10 and len(second) == 5
    assert first + second == want_losses
    _same(_final(tr2), want)
    assert [(h["step"], h["epoch"]) for h in tr2.val_history] == [(4, 0), (8, 1), (12, 2)]


# ------------------------------------------------------------------------------------------------ 3: trainer options
def test_resume_under_clipping_schedule_and_accumulation(S, tmp_path):
    opts = dict(gradient_clip_val=0.5, lr_scheduler={"name": "warmup_cosine", "warmup_steps": 2, "total_steps": 8},
                accumulate_grad_batches=2)
    fit_kw = dict(max_epochs=3, val_check_interval=4)
    want_losses, want = _straight(S, fit_kw, trainer_kw=opts)
    assert want["step"] == 7  # 15 micro-batches: 7 optimizer steps (and one micro-batch left over)
    first, second, tr, tr2 = _interrupted(S, dict(max_steps=6), fit_kw, tmp_path, trainer_kw=opts)
    assert S.X.read_checkpoint(tmp_path / "last.ckpt")["global_step"] == 3
    assert first + second == want_losses
    _same(_final(tr2), want)
    # between the micro-batches of one optimizer step there is no checkpoint
    assert tr2._micro == 1
    with pytest.raises(ValueError, match="micro-batches"):
        tr2.save_checkpoint(tmp_path / "odd.ckpt")
    assert not (tmp_path / "odd.ckpt").exists()


# ------------------------------------------------------------------------------------------------ 4: captured step
@pytest.fixture(scope="module")
def straight_graph(S):
    return _straight(S, dict(max_epochs=3, val_check_interval=4, graph="on"), loader_kw=dict(drop_last=True, fixed_width=True))


def test_resume_between_replays_of_a_captured_step(S, straight_graph, tmp_path):
    want_losses, want = straight_graph
    fit_kw = dict(max_epochs=3, val_check_interval=4, graph="on")
    first, second, tr, tr2 = _interrupted(S, dict(max_steps=7), fit_kw, tmp_path, loader_kw=dict(drop_last=True, fixed_width=True))
    assert tr.graph_choice == "graph" and tr2.graph_choice == "graph"  # the resumed call warmed up and captured again
    state = S.X.read_checkpoint(tmp_path / "last.ckpt")
    assert state["model"]["device_step"] is True and state["global_step"] == 7
    assert state["optimizer"]["state"][0]["step"] == 7  # the device-side counter, written back
    assert len(first) == 7 and len(second) == 8 and first + second == want_losses
    _same(_final(tr2), want)
    assert int(tr2.module.model.step_device.item()) == 15 == want["step"]
    # a restored trainer has its counter before any step: filled with the optimizer's step, wired to the optimizer
    mod3 = S.module(other_weights=True)
    tr3 = S.X.Trainer(mod3)
    ld3 = S.loader(drop_last=True, fixed_width=True)
    loop = tr3.load_checkpoint(tmp_path / "last.ckpt", loader=ld3)
    assert loop["batches_done"] == 7 and ld3.state_dict() == {"epoch": 1, "next_batch": 2}
    assert int(mod3.model.step_device.item()) == 7 and tr3.optimizer.step_device is mod3.model.step_device
    ld3.close()


# ------------------------------------------------------------------------------------------------ 5: no perturbation
@pytest.mark.parametrize("graph", ["off", "on"])
def test_periodic_checkpoints_do_not_perturb_training(S, straight_eager, straight_graph, graph, tmp_path):
    want_losses, want = straight_eager if graph == "off" else straight_graph
    lkw = {} if graph == "off" else dict(drop_last=True, fixed_width=True)
    mod = S.module()
    tr = S.X.Trainer(mod)
    ld = S.loader(**lkw)
    got = tr.fit(ld, max_epochs=3, val=S.evalset(mod), val_check_interval=4, graph=graph, checkpoint_every_n_steps=2,
                 checkpoint_dir=tmp_path)
    ld.close()
    assert got == want_losses
    _same(_final(tr), want)
    state = S.X.read_checkpoint(tmp_path / "last.ckpt")
    assert state["loop"]["batches_done"] == 14 and state["global_step"] == 14
    assert [h["step"] for h in state["loop"]["val_history"]] == [4, 8, 12]  # written BEHIND the pass that fell on batch 12
    names = [p.name for p in tmp_path.iterdir()]
    assert tr.ckpt_elapsed > 0.0 and "last.ckpt" in names and not any(n.endswith(".tmp") for n in names)


# ------------------------------------------------------------------------------------------------ 6: early stopping
class _ScriptedVal:
    """A validation set whose passes return scripted values of the monitor."""

    def __init__(self, values):
        self.values, self.calls = list(values), 0

    def evaluate(self, stage, cutoffs=None):
        v = self.values[self.calls]
        self.calls += 1
        return {f"{stage}/retrieval_normalized_dcg": v, f"{stage}/num_rows": 12}


def test_early_stopping_counts_across_a_resume(S, tmp_path):
    fit_kw = dict(max_epochs=3, val_check_interval=2, early_stopping={"patience": 3})
    mod = S.module()
    tr = S.X.Trainer(mod)
    ld = S.loader()
    want = tr.fit(ld, val=_ScriptedVal([0.5, 0.4, 0.3, 0.2, 0.1, 0.0, 0.0]), **fit_kw)
    ld.close()
    assert tr.stopped_early and len(want) == 8 and [h["step"] for h in tr.val_history] == [2, 4, 6, 8]
    want_final = _final(tr)
    mod1 = S.module()
    tr1 = S.X.Trainer(mod1)
    ld1 = S.loader()
    first = tr1.fit(ld1, val=_ScriptedVal([0.5, 0.4]), max_steps=4, save_last=True, checkpoint_dir=tmp_path, **fit_kw)
    ld1.close()
    assert len(first) == 4 and not tr1.stopped_early
    state = S.X.read_checkpoint(tmp_path / "last.ckpt")
    assert state["loop"]["stopper"] == {"best": 0.5, "wait": 1, "improved": False}
    mod2 = S.module(other_weights=True)
    tr2 = S.X.Trainer(mod2)
    ld2 = S.loader()
    val2 = _ScriptedVal([0.3, 0.2, 0.1, 0.0, 0.0])
    second = tr2.fit(ld2, val=val2, ckpt_path=tmp_path / "last.ckpt", **fit_kw)
    ld2.close()
    # its second pass is the fourth overall: wait 1 + 2 = patience. A rule that started from zero would have gone on.
    assert tr2.stopped_early and val2.calls == 2 and len(second) == 4
    assert first + second == want
    _same(_final(tr2), want_final)
    assert (tr2.best_score, tr2.best_step) == (0.5, 2)


# ------------------------------------------------------------------------------------------------ 7: max_time
def test_max_time_ends_the_run_after_a_batch_and_the_resume_finishes_it(S, straight_eager, tmp_path):
    want_losses, want = straight_eager
    first, second, tr, tr2 = _interrupted(S, dict(max_time=1e-9), dict(max_epochs=3, val_check_interval=4), tmp_path)
    assert len(first) == 1 and tr.stopped_on_time and not tr.stopped_early and (tmp_path / "last.ckpt").exists()
    assert len(second) == 14 and not tr2.stopped_on_time  # the resumed call has no limit (and would have its own budget)
    assert first + second == want_losses
    _same(_final(tr2), want)


# ------------------------------------------------------------------------------------------------ 8: refusals
def test_refusals(S, tmp_path):
    from xfmr_rec_amd.data import DeviceSeqLoader

    mod = S.module()
    tr = S.X.Trainer(mod)
    ld = S.loader()
    tr.fit(ld, max_epochs=1, max_steps=2, save_last=True, checkpoint_dir=tmp_path)
    ld.close()
    ck = tmp_path / "last.ckpt"
    before = mod.model.flat.detach().clone()
    for field, kw in (("loader seed", dict(seed=4)), ("loader batch_size", None)):
        other = S.loader(**kw) if kw is not None else DeviceSeqLoader(S.ds, 4, seed=3)
        fresh = S.X.Trainer(S.module(other_weights=True))
        kept = fresh.module.model.flat.detach().clone()
        with pytest.raises(ValueError, match=field):
            fresh.fit(other, max_epochs=1, ckpt_path=ck)
        assert torch.equal(fresh.module.model.flat, kept) and other.state_dict() == {"epoch": 0, "next_batch": 0}
        other.close()
    two = S.X.Trainer(S.module(), world_size=2)
    for kw in (dict(ckpt_path=ck), dict(save_last=True, checkpoint_dir=tmp_path),
               dict(checkpoint_every_n_steps=2, checkpoint_dir=tmp_path), dict(max_time="00:00:01:00")):
        with pytest.raises(ValueError, match="world_size"):
            two.fit([], **kw)
    with pytest.raises(ValueError, match="checkpoint_dir"):
        tr.fit(S.loader(), max_epochs=1, checkpoint_every_n_steps=2)
    acc = S.X.Trainer(S.module(), accumulate_grad_batches=2)
    with pytest.raises(ValueError, match="multiple of accumulate_grad_batches"):
        acc.fit(S.loader(), max_epochs=1, checkpoint_every_n_steps=3, checkpoint_dir=tmp_path)
    torch.cuda.synchronize()
    assert torch.equal(mod.model.flat, before)
