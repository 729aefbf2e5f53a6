"""``Trainer.fit``'s plan, batch source and schedule (``xfmr_rec_amd/fit_loop.py``) without a device: nothing launches.

The plan refuses what ``fit`` refuses, with its messages, before anything is restored. The schedule -- which batch is
stepped on, where validation passes, ``last.ckpt`` writes and stops fall, what position a resume starts from -- is driven
through a stand-in loader and recording events and compared with a straight-line model of the run over a grid of the
arguments; a run started from any checkpointed loop state gives the uninterrupted run's remaining events; and a batch is
fetched when the rule says: a loader only behind the previous step and only to be stepped on, a plain iterable one ahead."""

import dataclasses
import itertools
import re

import pytest

import xfmr_rec_amd as X
from xfmr_rec_amd import fit_loop as FL

NAME = "val/retrieval_normalized_dcg"


# ------------------------------------------------------------------------------------------------ stand-ins
class Loader:
    """``DeviceSeqLoader``'s protocol over batch ids ``(epoch, index)``; what it is asked for goes into ``log``."""

    world_size = 1

    def __init__(self, n, epoch=0, next_batch=0, log=None):
        self.n, self.epoch, self.next_batch = n, epoch, next_batch
        self.log = [] if log is None else log

    def __len__(self):
        return self.n

    def set_epoch(self, epoch):
        self.log.append(("set_epoch", epoch))
        self.epoch, self.next_batch = int(epoch), 0

    def __iter__(self):  # as the loader's: its state is a batch ahead of the consumer, and (e, 0) behind the last batch
        for i in range(self.next_batch, self.n):
            self.next_batch = i + 1
            self.log.append(("fetch", self.epoch, i))
            yield (self.epoch, i)
        self.next_batch = 0

    def load_state_dict(self, state):
        self.epoch, self.next_batch = state["epoch"], state["next_batch"]


class Untouchable(Loader):
    def _no(self, *a, **k):
        raise AssertionError("building a plan touches no loader")

    load_state_dict = set_epoch = __iter__ = __len__ = _no


class Events:
    """The run's events, recorded. ``early_at``: the number of the pass that asks to stop; ``time_at``: the batch number
    at which the clock has run out."""

    def __init__(self, log, base, last_pass=None, early_at=None, time_at=None):
        self.log, self.done, self.last_pass, self.early_at, self.time_at = log, base, last_pass, early_at, time_at
        self.pos, self.passes, self.states = None, 0, {}

    def step(self, batch, ahead, i):
        self.done += 1
        self.log.append(("step", self.done, *(batch if isinstance(batch, tuple) else (batch,))))

    def validate(self, done, epoch):
        self.log.append(("val", done))
        self.passes, self.last_pass = self.passes + 1, done
        return self.passes == self.early_at

    def checkpoint(self, done):
        self.log.append(("ckpt", done))
        self.states[done] = (self.pos, self.last_pass)  # what ``loop_state`` carries of the schedule's state

    def out_of_time(self):
        return self.time_at is not None and self.done >= self.time_at


def drive(plan, loader, log, base=0, start=None, last_pass=None, **stops):
    """The real source and the real loop over the stand-ins; returns the events object (``pos``: the final position)."""
    ev = Events(log, base, last_pass, **stops)
    ev.pos = FL.start_position(loader, plan) if start is None else start
    done, stop = FL.run_schedule(plan, FL.batch_source(loader, plan, ev.pos, base, is_loader=True), base, ev)
    assert done == ev.done
    if stop is not None:
        log.append(("stop", stop))
    return ev


# ------------------------------------------------------------------------------------------------ the model
def model(n, start, base, last_pass, *, max_epochs, max_steps, val_check_interval, check_val_every_n_epoch,
          limit_train_batches, checkpoint_every_n_steps, early_at=None, time_at=None):
    """The run written out: first every (epoch, index, ends the epoch) it could reach from ``start``, then one walk."""
    e0, j0 = start
    if max_epochs is None:
        reach = [(e0, j, j + 1 == n) for j in range(j0, n)]
    else:
        n_b = n if limit_train_batches is None else min(n, limit_train_batches)
        reach = [(e, j, j + 1 == n_b) for e in range(e0, max_epochs) for j in range(j0 if e == e0 else 0, n_b)]
    events, pos, done, passes, stop = [], start, base, 0, None
    for e, j, last in reach:
        if stop is not None or (max_steps is not None and done >= max_steps):
            break
        done += 1
        events.append(("step", done, e, j))
        pos = (e + 1, 0) if last else (e, j + 1)
        if val_check_interval is not None:
            passes_here = done % val_check_interval == 0
        else:
            passes_here = max_epochs is not None and last and (e + 1) % check_val_every_n_epoch == 0
        if passes_here:
            events.append(("val", done))
            passes, last_pass = passes + 1, done
        if checkpoint_every_n_steps is not None and done % checkpoint_every_n_steps == 0:
            events.append(("ckpt", done))
        if passes_here and passes == early_at:
            stop = "early"
        elif time_at is not None and done >= time_at:
            stop = "time"
    if val_check_interval is None and max_epochs is None and done > 0 and last_pass != done:
        events.append(("val", done))
    if stop is not None:
        events.append(("stop", stop))
    return events, pos


def fresh_start(loader, max_epochs):
    """Where a call that restores nothing begins: mid-epoch it goes on; at an epoch's start the epoch loop begins at 0."""
    return (loader.epoch if loader.next_batch > 0 or max_epochs is None else 0, loader.next_batch)


GRID = dict(n=(1, 3, 5), max_epochs=(None, 0, 1, 3), max_steps=(None, 0, 4, 7), val_check_interval=(None, 2, 4),
            check_val_every_n_epoch=(1, 2), limit_train_batches=(None, 0, 2), checkpoint_every_n_steps=(None, 2, 3),
            mid_epoch=(False, True))


def _grid():
    for values in itertools.product(*GRID.values()):
        yield dict(zip(GRID, values))


def _plan(kw, tmp_path, **more):
    kw = {k: v for k, v in kw.items() if k not in ("n", "mid_epoch")}
    return FL.FitPlan.build(None, Loader(1), world_size=1, accumulate_grad_batches=1, val=object(), checkpoint_dir=tmp_path,
                            **kw, **more)


def _loader_at(kw, log=None):
    # "mid-epoch": batch n // 2 of epoch 1 -- with one batch per epoch that is (1, 0), a loader that has FINISHED an epoch
    return Loader(kw["n"], 1, kw["n"] // 2, log) if kw["mid_epoch"] else Loader(kw["n"], log=log)


def _only_schedule(kw):
    return {k: v for k, v in kw.items() if k not in ("n", "mid_epoch")}


def test_schedule_equals_the_model_and_a_resume_gives_the_remaining_events(tmp_path):
    """One place is outside the resume property, by what the arguments mean: without ``max_epochs`` a call runs "what is
    left of the loader's current epoch", and nothing in the loop state says that a pass is over -- behind its last batch
    the position is (e + 1, 0), the same as behind epoch e of an epoch loop that goes on. A call resumed from a file
    written THERE is therefore a new pass over epoch e + 1 (as before this module existed; telling the two apart would
    take a new key in the file). It is held to the model run from that state instead; everywhere else, to the
    uninterrupted run's remaining events as well."""
    ran = resumed = total = new_pass = 0
    for kw in _grid():
        total += 1
        try:
            plan = _plan(kw, tmp_path)
        except ValueError:
            continue  # (limit_train_batches / check_val_every_n_epoch without max_epochs)
        ran += 1
        log = []
        loader = _loader_at(kw, log)
        start = fresh_start(loader, kw["max_epochs"])
        want, want_pos = model(kw["n"], start, 0, None, **_only_schedule(kw))
        ev = drive(plan, loader, log)
        got = [x for x in log if x[0] not in ("fetch", "set_epoch")]
        assert got == want and ev.pos == want_pos, (kw, got, want, ev.pos, want_pos)
        # fetch timing: every fetch stands behind the step on the batch before it, and every fetched batch is stepped on
        order = [x[0] for x in log if x[0] in ("fetch", "step")]
        assert order == ["fetch", "step"] * (len(order) // 2), (kw, log)
        assert [x[1:] for x in log if x[0] == "fetch"] == [x[2:] for x in log if x[0] == "step"], (kw, log)
        # resume: from the loop state of every checkpoint, in a new loader put there as Trainer.load_state_dict puts it
        for done, (pos, last_pass) in ev.states.items():
            resumed += 1
            again = Loader(kw["n"])
            again.load_state_dict({"epoch": pos[0], "next_batch": pos[1]})
            log2 = []
            ev2 = drive(plan, again, log2, base=done, start=pos, last_pass=last_pass)
            assert (log2, ev2.pos) == model(kw["n"], pos, done, last_pass, **_only_schedule(kw))
            if kw["max_epochs"] is None and pos == (start[0] + 1, 0):
                new_pass += 1
                continue
            rest = want[want.index(("ckpt", done)) + 1:]
            assert log2 == rest and ev2.pos == want_pos, (kw, done, pos, log2, rest)
    assert 2 * ran >= total and resumed >= 500 and 20 * new_pass < resumed, (ran, resumed, new_pass, total)


@pytest.mark.parametrize("stops", [dict(early_at=1), dict(early_at=2), dict(time_at=1), dict(time_at=3),
                                   dict(early_at=2, time_at=4), dict(early_at=2, time_at=3)])
def test_stops_fall_where_the_model_puts_them(tmp_path, stops):
    for kw in _grid():
        if kw["max_epochs"] in (None, 0) or kw["max_steps"] == 0 or kw["limit_train_batches"] == 0:
            continue
        plan = _plan(kw, tmp_path, early_stopping=True, max_time=3600)
        loader = _loader_at(kw)
        want, want_pos = model(kw["n"], fresh_start(loader, kw["max_epochs"]), 0, None, **_only_schedule(kw), **stops)
        log = []
        ev = drive(plan, loader, log, **stops)
        assert log == want and ev.pos == want_pos, (kw, log, want)
    # a checkpoint that falls on the batch of the pass that stops the run is still written, behind the pass
    plan = FL.FitPlan.build(None, Loader(1), world_size=1, accumulate_grad_batches=1, val=object(), checkpoint_dir=tmp_path,
                            max_epochs=2, val_check_interval=2, checkpoint_every_n_steps=2)
    log = []
    drive(plan, Loader(5), log, early_at=1)
    assert log == [("step", 1, 0, 0), ("step", 2, 0, 1), ("val", 2), ("ckpt", 2), ("stop", "early")]


def test_an_epoch_cut_short_is_over_and_a_finished_loader_starts_at_epoch_zero(tmp_path):
    plan = _plan(dict(max_epochs=2, limit_train_batches=2), tmp_path)
    loader = Loader(5)
    ev = drive(plan, loader, loader.log)
    assert [x for x in loader.log if x[0] == "set_epoch"] == [("set_epoch", e) for e in (0, 0, 1, 1)]
    assert [x[2:] for x in loader.log if x[0] == "step"] == [(0, 0), (0, 1), (1, 0), (1, 1)] and ev.pos == (2, 0)
    assert (loader.epoch, loader.next_batch) == (1, 0)  # (not half-way through epoch 1)
    # a loader that has run epoch 1 to its end reads (1, 0): the epoch loop takes that for "start at epoch 0" ...
    loader = Loader(3, 1, 0)
    ev = drive(_plan(dict(max_epochs=1), tmp_path), loader, loader.log)
    assert [x[2:] for x in loader.log if x[0] == "step"] == [(0, 0), (0, 1), (0, 2)] and ev.pos == (1, 0)
    # ... a restored LOOP names its epoch itself: (1, 0) is where epoch 1 begins; a loader left mid-epoch goes on there
    loader = Loader(3, 1, 0)
    drive(_plan(dict(max_epochs=2), tmp_path), loader, loader.log, base=3, start=(1, 0))
    assert [x[1:] for x in loader.log if x[0] == "step"] == [(4, 1, 0), (5, 1, 1), (6, 1, 2)]
    loader = Loader(3, 1, 2)
    drive(_plan(dict(max_epochs=3), tmp_path), loader, loader.log)
    assert [x[2:] for x in loader.log if x[0] == "step"] == [(1, 2), (2, 0), (2, 1), (2, 2)]
    # without max_epochs: what is left of the loader's current epoch, positions in that epoch
    loader = Loader(5, 4, 3)
    ev = drive(_plan({}, tmp_path), loader, loader.log)
    assert [x for x in loader.log if x[0] != "fetch"] == [("step", 1, 4, 3), ("step", 2, 4, 4), ("val", 2)] and ev.pos == (5, 0)


class Reads:
    """A plain iterable of ``n`` batch ids that counts how far it has been read (and may fail behind the last one)."""

    def __init__(self, n, fail=False):
        self.n, self.read, self.fail = n, 0, fail

    def __iter__(self):
        for i in range(self.n):
            self.read = i + 1
            yield i
        if self.fail:
            raise RuntimeError("no more batches")


@pytest.mark.parametrize("max_steps", [None, 0, 2, 4, 9])
def test_a_plain_iterable_is_read_exactly_one_ahead(tmp_path, max_steps):
    plan = FL.FitPlan.build([], None, world_size=1, accumulate_grad_batches=1, max_steps=max_steps)
    batches = Reads(4)
    seen = []

    class Ev(Events):
        def step(self, batch, ahead, i):
            super().step(batch, ahead, i)
            seen.append((batch, ahead, batches.read))

    ev = Ev([], 0)
    FL.run_schedule(plan, FL.batch_source(batches, plan, (0, 0), 0, is_loader=False), 0, ev)
    steps = 4 if max_steps is None else min(4, max_steps)
    # at step i batch i + 1 has been read (it is handed on, for the ring to stage) and batch i + 2 has not
    assert seen == [(i, i + 1 if i + 1 < 4 else None, min(4, i + 2)) for i in range(steps)]
    assert batches.read == (min(4, steps + 1) if steps else 0) and ev.pos == ((0, steps) if steps else None)
    # a resumed call over a plain iterable counts on from the restored number: the caller supplies the batches from there
    log = []
    ev = Events(log, 7)
    FL.run_schedule(plan, FL.batch_source([70, 80], plan, (0, 7), 7, is_loader=False), 7, ev)
    assert [x[:2] for x in log] == ([("step", 8), ("step", 9)] if max_steps in (None, 9) else [])


def test_a_failed_read_ahead_is_raised_when_its_batch_is_due(tmp_path):
    plan = FL.FitPlan.build([], None, world_size=1, accumulate_grad_batches=1)
    log = []
    with pytest.raises(RuntimeError, match="no more batches"):
        FL.run_schedule(plan, FL.batch_source(Reads(2, fail=True), plan, (0, 0), 0, is_loader=False), 0, Events(log, 0))
    assert log == [("step", 1, 0), ("step", 2, 1)]  # the batch in hand is stepped on first


# ------------------------------------------------------------------------------------------------ building the plan
def _build(batches=None, loader=None, world_size=1, accumulate_grad_batches=1, **kw):
    return FL.FitPlan.build([] if batches is None else batches, loader, world_size=world_size,
                            accumulate_grad_batches=accumulate_grad_batches, **kw)


VAL = object()  # (never touched)
REFUSALS = [  # one per ValueError of the loop's argument checks, in their order, with the message
    (dict(max_time="soon"), "max_time"),
    (dict(world_size=2, max_time=60), "ckpt_path / save_last / checkpoint_every_n_steps / max_time inside a data-parallel run "
     "(world_size > 1) are not supported"),
    (dict(checkpoint_every_n_steps=0, checkpoint_dir="d"), "checkpoint_every_n_steps must be an integer >= 1 or None; got 0"),
    (dict(checkpoint_every_n_steps=True, checkpoint_dir="d"), "checkpoint_every_n_steps must be an integer >= 1 or None; got True"),
    (dict(accumulate_grad_batches=2, checkpoint_every_n_steps=3, checkpoint_dir="d"),
     "checkpoint_every_n_steps = 3 is not a multiple of accumulate_grad_batches = 2: a checkpoint would fall between the "
     "micro-batches of one step"),
    (dict(save_last=True), "checkpoint_every_n_steps / save_last write checkpoint_dir / 'last.ckpt': pass checkpoint_dir"),
    (dict(checkpoint_every_n_steps=2), "checkpoint_every_n_steps / save_last write checkpoint_dir / 'last.ckpt'"),
    (dict(limit_train_batches=2), "limit_train_batches / check_val_every_n_epoch belong to the epoch loop: pass max_epochs"),
    (dict(check_val_every_n_epoch=2), "limit_train_batches / check_val_every_n_epoch belong to the epoch loop: pass max_epochs"),
    (dict(max_epochs=1), "max_epochs needs a DeviceSeqLoader to run epochs over; got list"),
    (dict(loader=Loader(3), max_epochs=-1), "max_epochs must be an integer >= 0; got -1"),
    (dict(loader=Loader(3), max_epochs=1, check_val_every_n_epoch=0), "check_val_every_n_epoch must be an integer >= 1; got 0"),
    (dict(loader=Loader(3), max_epochs=1, limit_train_batches=0.5), "limit_train_batches must be an integer >= 0; got 0.5"),
    (dict(loader=Loader(3), world_size=2), "the loader shards its epochs over world_size = 1, this trainer runs world_size = 2"),
    (dict(val=VAL, val_check_interval=0), "val_check_interval must be an integer >= 1 or None; got 0"),
    (dict(val=VAL, accumulate_grad_batches=2, val_check_interval=3),
     "val_check_interval = 3 is not a multiple of accumulate_grad_batches = 2: a pass would fall between the micro-batches "
     "of one step"),
    (dict(monitor={"name": NAME}), "monitor must be {'name', 'mode'}; got {'name': 'val/retrieval_normalized_dcg'}"),
    (dict(monitor={"name": NAME, "mode": "most"}), "mode must be 'max' or 'min'; got 'most'"),
    (dict(early_stopping={"patience": 2, "tolerance": 0.1}), "early_stopping: unknown keys ['tolerance']"),
    (dict(early_stopping=3), "early_stopping must be None, True or a dict; got 3"),
    (dict(val_cutoffs=(0,)), "cutoffs must be positive integers below 2^31; got 0"),
    (dict(val=VAL, monitor={"name": "val/nothing", "mode": "max"}),
     "monitor name 'val/nothing': expected '<stage>/<metric>' with a metric of"),
    (dict(val=VAL, val_cutoffs=(10,), monitor={"name": NAME + "@7", "mode": "max"}),
     f"monitor name '{NAME}@7': '@<K>' needs K among val_cutoffs = (10,)"),
    (dict(graph="maybe"), "graph must be 'off', 'on' or 'auto', got 'maybe'"),
    (dict(accumulate_grad_batches=2, graph="on"), "a captured step cannot accumulate micro-batches (accumulate_grad_batches > 1)"),
]


@pytest.mark.parametrize("kw,message", REFUSALS, ids=[f"{i}-{next(iter(kw))}" for i, (kw, _) in enumerate(REFUSALS)])
def test_the_plan_refuses_what_fit_refuses_with_its_message(kw, message):
    with pytest.raises(ValueError, match=re.escape(message)):
        _build(**kw)
    if "loader" not in kw and "world_size" not in kw and "accumulate_grad_batches" not in kw and kw.get("val") is None:
        with pytest.raises(ValueError, match=re.escape(message)):  # ... and so does fit, with nothing else touched
            X.Trainer(X.RecommenderLightningModule(X.LightningConfig(
                hidden_size=64, num_attention_heads=2, intermediate_size=128, num_hidden_layers=1, max_seq_length=8))).fit([], **kw)


def test_which_refusal_wins_is_the_order_of_the_checks():
    both = dict(checkpoint_every_n_steps=0, val=VAL, val_check_interval=0, checkpoint_dir="d")
    with pytest.raises(ValueError, match="checkpoint_every_n_steps must be"):
        _build(**both)
    with pytest.raises(ValueError, match="max_time"):
        _build(max_time="soon", graph="maybe", monitor={})
    with pytest.raises(ValueError, match="monitor must be"):
        _build(graph="maybe", monitor={})
    with pytest.raises(ValueError, match="val_check_interval must be"):  # every other check stands in front of graph's
        _build(graph="maybe", val=VAL, val_check_interval=0)


def test_building_a_plan_touches_no_loader_and_every_check_precedes_the_restore(tmp_path):
    loader = Untouchable(3)
    plan = _build(loader, loader, max_epochs=2, ckpt_path=tmp_path / "missing.ckpt", save_last=True, checkpoint_dir=tmp_path)
    assert plan.epoch_loop and not list(tmp_path.iterdir())
    tr = X.Trainer(X.RecommenderLightningModule(X.LightningConfig(hidden_size=64, num_attention_heads=2, intermediate_size=128,
                                                                  num_hidden_layers=1, max_seq_length=8)))
    with pytest.raises(ValueError, match="graph must be"):  # not a file error: the file is never opened
        tr.fit([], graph="maybe", ckpt_path=tmp_path / "missing.ckpt")
    acc = X.Trainer(X.RecommenderLightningModule(X.LightningConfig(hidden_size=64, num_attention_heads=2, intermediate_size=128,
                                                                   num_hidden_layers=1, max_seq_length=8)),
                    accumulate_grad_batches=2)
    with pytest.raises(ValueError, match="cannot accumulate micro-batches"):
        acc.fit([], graph="on", ckpt_path=tmp_path / "missing.ckpt")
    with pytest.raises(FileNotFoundError):  # with nothing to refuse, the restore is next
        tr.fit([], ckpt_path=tmp_path / "missing.ckpt")


def test_the_plan_holds_the_normalised_values_and_cannot_be_changed(tmp_path):
    plan = _build(val=VAL, val_cutoffs=[10, 5, 10], monitor={"name": NAME + "@5", "mode": "min"}, max_time="00:01:00:30",
                  checkpoint_dir=str(tmp_path), early_stopping=True, graph="auto", max_steps=9)
    assert (plan.stage, plan.monitor, plan.mode, plan.val_cutoffs) == ("val", NAME + "@5", "min", (10, 5))
    assert plan.time_limit == 3630.0 and plan.early_stopping == (3, 0.0) and plan.validates and not plan.epoch_loop
    assert (plan.last_path, plan.best_path) == (tmp_path / "last.ckpt", tmp_path / "best")
    assert plan.graph == "auto" and _build(world_size=2, graph="auto").graph == "off"  # (a data-parallel step is not captured)
    assert _build().last_path is None and _build().early_stopping is None and _build().time_limit is None
    assert _build(early_stopping={"patience": 5, "min_delta": 0.25}).early_stopping == (5, 0.25)
    with pytest.raises(dataclasses.FrozenInstanceError):
        plan.max_steps = 10
    # the schedule's four questions, on one plan
    plan = _build(Loader(5), Loader(5), val=VAL, max_epochs=3, check_val_every_n_epoch=2, checkpoint_every_n_steps=4,
                  checkpoint_dir=tmp_path, max_steps=12)
    assert [plan.validates_after(10, e, last) for e, last in ((0, True), (1, True), (1, False), (3, True))] == [False, True, False, True]
    assert not plan.validates_at_end(12, None) and [plan.checkpoints_after(d) for d in (3, 4, 8)] == [False, True, True]
    assert plan.more_after(11) and not plan.more_after(12)
    one = _build(val=VAL)
    assert one.validates_at_end(5, None) and one.validates_at_end(5, 3) and not one.validates_at_end(5, 5)
    assert not one.validates_at_end(0, None) and not _build().validates_at_end(5, None)
