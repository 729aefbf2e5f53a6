"""``Trainer.fit``'s loop in its parts (DESIGN.md sections 10 and 11).

Without a device, a module or a file (tests/test_fit_plan_host.py): :class:`FitPlan` -- every argument checked and
normalised once, and the schedule as pure functions of the counters; :func:`batch_source` -- the batches with their
positions and the one rule of when each is fetched; :func:`run_schedule` -- the loop, over any object with the run's
events. Behind those events on the device: :class:`DeviceFeed` (a batch becomes the step's argument),
:class:`StepChooser` (eager step, capture, probe, replay) and :class:`FitRun` (validation passes, ``last.ckpt``, and the
setup and teardown that also runs when the loop raises)."""

from __future__ import annotations

import contextlib
import dataclasses
import pathlib
import time

import torch

from . import checkpoint as CK
from .data import SEQ_BATCH_KEYS, PinnedBatchRing
from .params import METRIC
from .trainer import (_NO_ACCUMULATED_CAPTURE, EarlyStopping, GraphedStep, _early_stopping_from,
                      _refuse_capture_after_default_stream_steps)


def _not_a_count(v, least: int) -> bool:
    return isinstance(v, bool) or not isinstance(v, int) or v < least


def _check_interval(name: str, n, accumulate: int, what: str) -> None:
    if n is None:
        return
    if _not_a_count(n, 1):
        raise ValueError(f"{name} must be an integer >= 1 or None; got {n!r}")
    if n % accumulate:
        raise ValueError(f"{name} = {n} is not a multiple of accumulate_grad_batches = {accumulate}: {what} would fall "
                         "between the micro-batches of one step")


@dataclasses.dataclass(frozen=True)
class FitPlan:
    """One ``fit`` call's arguments, checked and normalised (:meth:`build`), and its schedule: on which batch a validation
    pass, a ``last.ckpt`` or the end of the loop falls, as functions of the loop's counters alone."""

    max_steps: int | None
    ring_slots: int
    graph: str                      # "off" under world_size > 1 (the all-reduce of a data-parallel step is not captured)
    graph_probe_steps: int
    validates: bool                 # a validation set was given
    val_check_interval: int | None
    monitor: str                    # the monitored key of a pass's metrics: '<stage>/<metric>[@<K>]'
    mode: str
    stage: str
    early_stopping: tuple | None    # (patience, min_delta)
    val_cutoffs: tuple | None
    max_epochs: int | None
    check_val_every_n_epoch: int
    limit_train_batches: int | None
    checkpoint_every_n_steps: int | None
    save_last: bool
    time_limit: float | None        # seconds of this call (checkpoint.parse_max_time)
    last_path: pathlib.Path | None  # checkpoint_dir / "last.ckpt"
    best_path: pathlib.Path | None  # checkpoint_dir / "best"

    @classmethod
    def build(cls, batches, loader, *, world_size: int, accumulate_grad_batches: int, max_steps=None, ring_slots=6,
              graph="off", graph_probe_steps=20, val=None, val_check_interval=None, monitor=METRIC, early_stopping=None,
              checkpoint_dir=None, val_cutoffs=None, max_epochs=None, check_val_every_n_epoch=1, limit_train_batches=None,
              ckpt_path=None, save_last=False, checkpoint_every_n_steps=None, max_time=None) -> "FitPlan":
        """``fit``'s arguments (same names, same defaults) and the trainer's ``world_size`` and ``accumulate_grad_batches``;
        ``loader`` is ``batches`` where that is a loader, else None (only its ``world_size`` is read). Every refusal is a
        ``ValueError``, and all of them come before anything is restored from ``ckpt_path``."""
        from .retrieval import METRIC_NAMES, normalize_cutoffs

        time_limit = CK.parse_max_time(max_time)
        if world_size > 1 and (ckpt_path is not None or save_last or checkpoint_every_n_steps is not None
                               or max_time is not None):
            raise ValueError("ckpt_path / save_last / checkpoint_every_n_steps / max_time inside a data-parallel run "
                             "(world_size > 1) are not supported: ranks that read their own clocks would leave the all-reduce "
                             "at different steps, and a multi-rank run has never executed (save_checkpoint / load_checkpoint "
                             "work on any rank)")
        _check_interval("checkpoint_every_n_steps", checkpoint_every_n_steps, accumulate_grad_batches, "a checkpoint")
        if (checkpoint_every_n_steps is not None or save_last) and checkpoint_dir is None:
            raise ValueError("checkpoint_every_n_steps / save_last write checkpoint_dir / 'last.ckpt': pass checkpoint_dir")
        if max_epochs is None:
            if limit_train_batches is not None or check_val_every_n_epoch != 1:
                raise ValueError("limit_train_batches / check_val_every_n_epoch belong to the epoch loop: pass max_epochs")
        else:
            if loader is None:
                raise ValueError(f"max_epochs needs a DeviceSeqLoader to run epochs over; got {type(batches).__name__}")
            for name, v, least in (("max_epochs", max_epochs, 0), ("check_val_every_n_epoch", check_val_every_n_epoch, 1),
                                   ("limit_train_batches", limit_train_batches, 0)):
                if v is not None and _not_a_count(v, least):
                    raise ValueError(f"{name} must be an integer >= {least}; got {v!r}")
        if loader is not None and loader.world_size != world_size:
            raise ValueError(f"the loader shards its epochs over world_size = {loader.world_size}, this trainer runs "
                             f"world_size = {world_size}")
        _check_interval("val_check_interval", val_check_interval, accumulate_grad_batches, "a pass")
        if not isinstance(monitor, dict) or set(monitor) != {"name", "mode"}:
            raise ValueError(f"monitor must be {{'name', 'mode'}}; got {monitor!r}")
        stage, _, metric_name = str(monitor["name"]).rpartition("/")
        EarlyStopping(monitor["mode"], patience=None)  # (refuses a mode that is neither 'max' nor 'min')
        stopper = _early_stopping_from(early_stopping, monitor["mode"])
        if val_cutoffs is not None:
            val_cutoffs = normalize_cutoffs(val_cutoffs)
        if val is not None:
            metric_name, at, at_k = metric_name.partition("@")
            if not stage or metric_name not in METRIC_NAMES:
                raise ValueError(f"monitor name {monitor['name']!r}: expected '<stage>/<metric>' with a metric of {METRIC_NAMES}")
            if at and (val_cutoffs is None or not at_k.isdecimal() or str(int(at_k)) != at_k or int(at_k) not in val_cutoffs):
                raise ValueError(f"monitor name {monitor['name']!r}: '@<K>' needs K among val_cutoffs = {val_cutoffs!r}")
        if graph not in ("off", "on", "auto"):
            raise ValueError(f"graph must be 'off', 'on' or 'auto', got {graph!r}")
        if graph != "off" and accumulate_grad_batches > 1:
            raise ValueError(_NO_ACCUMULATED_CAPTURE)
        ckpt_dir = pathlib.Path(checkpoint_dir) if checkpoint_dir is not None else None
        return cls(max_steps=max_steps, ring_slots=ring_slots, graph=graph if world_size == 1 else "off",
                   graph_probe_steps=graph_probe_steps, validates=val is not None, val_check_interval=val_check_interval,
                   monitor=monitor["name"], mode=monitor["mode"], stage=stage,
                   early_stopping=(stopper.patience, stopper.min_delta) if stopper is not None else None,
                   val_cutoffs=val_cutoffs, max_epochs=max_epochs, check_val_every_n_epoch=check_val_every_n_epoch,
                   limit_train_batches=limit_train_batches, checkpoint_every_n_steps=checkpoint_every_n_steps,
                   save_last=save_last, time_limit=time_limit, last_path=ckpt_dir / "last.ckpt" if ckpt_dir else None,
                   best_path=ckpt_dir / "best" if ckpt_dir else None)

    @property
    def epoch_loop(self) -> bool:
        return self.max_epochs is not None

    # ------------------------------------------------------------------ the schedule: `done` counts batches over all calls
    def validates_after(self, done: int, epoch: int, ends_epoch: bool) -> bool:
        """Whether a pass follows batch number ``done``, a batch of ``epoch`` (and its last one: ``ends_epoch``)."""
        if not self.validates:
            return False
        if self.val_check_interval is not None:
            return done % self.val_check_interval == 0
        return self.epoch_loop and ends_epoch and (epoch + 1) % self.check_val_every_n_epoch == 0

    def validates_at_end(self, done: int, last_pass: int | None) -> bool:
        """Whether one pass follows the loop, which ended behind batch number ``done`` (Lightning's end-of-epoch pass over
        one iteration; the epoch loop has placed its passes itself). ``last_pass``: the batch number the last pass stands
        behind, None without one -- a run resumed from a ``last.ckpt`` written behind its last batch still owes the
        pass, one resumed from the file of the loop's end does not repeat it."""
        return (self.validates and self.val_check_interval is None and not self.epoch_loop and done > 0
                and last_pass != done)

    def checkpoints_after(self, done: int) -> bool:
        return self.checkpoint_every_n_steps is not None and done % self.checkpoint_every_n_steps == 0

    def more_after(self, done: int) -> bool:
        """Whether another batch is to be asked for once ``done`` are stepped on."""
        return self.max_steps is None or done < self.max_steps


def start_position(loader, plan: FitPlan) -> tuple[int, int]:
    """(epoch, batch) of a call's first step when nothing was restored: a loader left mid-epoch goes on there; one that
    stands at an epoch's start -- after a finished epoch e it reads (e, 0) -- starts the epoch loop at epoch 0."""
    if loader is None:
        return (0, 0)
    return (loader.epoch if (loader.next_batch > 0 or not plan.epoch_loop) else 0, loader.next_batch)


def _positions(batches, plan: FitPlan, start, base: int, is_loader: bool):
    """``(batch, epoch, index in the epoch, whether it ends the epoch)``. A plain iterable is one endless epoch 0 whose
    index is the global batch number; a loader without ``max_epochs`` gives what is left of its current epoch."""
    if not is_loader:
        for j, b in enumerate(batches, base):
            yield b, 0, j, False
    elif not plan.epoch_loop:
        n_b = len(batches)
        for j, b in enumerate(batches, batches.next_batch):
            yield b, batches.epoch, j, j + 1 == n_b
    else:
        # a loader restored mid-epoch goes on from there; a restored LOOP names its epoch itself (load_state_dict has put
        # the loader there: after the last batch of epoch e that is (e + 1, 0))
        for e in range(start[0], plan.max_epochs):
            if e > start[0] or batches.next_batch == 0:
                batches.set_epoch(e)
            n_b = len(batches) if plan.limit_train_batches is None else min(len(batches), plan.limit_train_batches)
            it = iter(batches)
            for j in range(batches.next_batch, n_b):
                yield next(it), e, j, j + 1 == n_b
            it.close()
            batches.set_epoch(e)  # (an epoch cut short by limit_train_batches is over, not half done)


def batch_source(batches, plan: FitPlan, start, base: int, *, is_loader: bool):
    """The call's batches in order, as ``(batch, epoch, j, ends_epoch, ahead)``: each with its position, from which
    :func:`run_schedule` derives the one the next step reads. ``base`` batches were done before this call; ``start`` is
    the (epoch, batch) it begins at.

    When a batch is fetched is this one rule. A plain iterable is read ONE AHEAD, before the step (``ahead`` is that
    next batch, for the ring to stage underneath the step). A loader (``is_loader``: ``epoch``, ``next_batch``,
    ``__len__``, ``set_epoch``, ``__iter__`` with a ``close``) rewrites its slots underneath the steps and its state is
    what a resumed run starts from: it is asked only when the consumer comes back -- after the step is enqueued -- and
    the consumer comes back only for a batch it will step on. An exception out of the read-ahead is raised when its
    batch is due, behind the step on the batch in hand."""
    if not plan.more_after(base):
        return
    it = _positions(batches, plan, start, base, is_loader)
    cur, failed = next(it, None), None
    while cur is not None:
        ahead = None
        if not is_loader:
            try:
                ahead = next(it, None)
            except Exception as exc:  # noqa: BLE001
                failed = exc
        yield (*cur, ahead[0] if ahead is not None else None)
        if failed is not None:
            raise failed
        cur = next(it, None) if is_loader else ahead


def run_schedule(plan: FitPlan, source, base: int, run) -> tuple[int, str | None]:
    """The loop. ``run`` has the events: ``step(batch, ahead, i)`` (``i`` counts this call's batches: the capture's
    warm-up and the probe are this call's), ``validate(done, epoch) -> stop``, ``checkpoint(done)``, ``out_of_time()``,
    ``pos``, kept at the position the next step reads, and ``last_pass``, the batch number of the last validation pass
    (None without one). Returns the batches done over all calls and what stopped the loop: "early", "time" or None."""
    i, stop = 0, None
    for batch, epoch, j, ends_epoch, ahead in source:
        run.step(batch, ahead, i)
        i += 1
        done = base + i
        # from the loop's own counters (a loader's state is a batch ahead): behind the last batch of epoch e stands (e + 1, 0)
        run.pos = (epoch + 1, 0) if ends_epoch else (epoch, j + 1)
        early = plan.validates_after(done, epoch, ends_epoch) and run.validate(done, epoch)
        if plan.checkpoints_after(done):
            run.checkpoint(done)  # behind the pass that fell on this batch: the file carries it
        if early:
            stop = "early"
        elif run.out_of_time():  # (a host clock: no device sync)
            stop = "time"
        if stop is not None or not plan.more_after(done):
            break
    if plan.validates_at_end(base + i, run.last_pass):
        run.validate(base + i, None)
    return base + i, stop


class DeviceFeed:
    """A yielded batch becomes the step's argument. Batches in HOST memory go through a ``PinnedBatchRing`` (made for the
    first one, made again for a larger one): the batch in hand is taken, the next one staged underneath the step when
    it fits. ``drop_lengths`` (``graph != "off"``): a captured step has fixed launch sizes, so it runs the padded layout
    and so do the eager steps around it -- host and loader batches are passed on without their rows' lengths."""

    def __init__(self, model, ring_slots: int, drop_lengths: bool, from_loader: bool):
        self.model, self.ring_slots, self.drop_lengths, self.from_loader = model, ring_slots, drop_lengths, from_loader
        self.ring = None

    def _fits_ring(self, b) -> bool:
        h = b[SEQ_BATCH_KEYS[0]]
        return not h.is_cuda and self.ring is not None and h.shape[0] <= self.ring.shape[1] and h.shape[1] <= self.ring.shape[2]

    def __call__(self, batch, ahead):
        on_host = not batch[SEQ_BATCH_KEYS[0]].is_cuda
        if on_host:
            if not self._fits_ring(batch):
                if self.ring is not None:
                    self.ring.close()
                bs, width = batch[SEQ_BATCH_KEYS[0]].shape
                self.ring = PinnedBatchRing(self.model.device, bs, max(width, self.model.max_seq_length), slots=self.ring_slots)
            if self.ring.pending == 0:
                self.ring.stage(batch)
            batch = self.ring.take()
        if ahead is not None and self._fits_ring(ahead):
            self.ring.stage(ahead)  # in flight while this step computes
        if self.drop_lengths and (on_host or self.from_loader):
            batch = {k: batch[k] for k in SEQ_BATCH_KEYS}
        return batch

    def close(self) -> None:
        if self.ring is not None:
            self.ring.release()
            self.ring.close()


class StepChooser:
    """Which form of the step runs. ``mode`` "off": the eager step, always. "on": after ``N_WARM`` eager steps (they
    create every lazily made object) the step is captured once and replayed for every batch of the captured shape.
    "auto": ``probe_steps`` eager steps are timed, then as many replays, and the faster form runs the rest. Every probe
    step is a real training step on its own batch."""

    N_WARM = 3

    def __init__(self, trainer, mode: str, probe_steps: int):
        self.trainer, self.mode, self.probe_steps = trainer, mode, probe_steps
        self.gstep, self.use_graph = None, False
        self.probe: dict = {}  # eager_t0 / eager_i0 / eager_ms, then graph_t0 / graph_i0 / graph_ms ("auto")

    def _sync_time(self) -> float:
        torch.cuda.synchronize(self.trainer.module.model.device)
        return time.perf_counter()

    def _choose(self, batch, i: int) -> None:
        probe, auto = self.probe, self.mode == "auto"
        if auto and "eager_t0" not in probe:
            probe["eager_t0"], probe["eager_i0"] = self._sync_time(), i
        if self.gstep is None and (not auto or i - probe["eager_i0"] >= self.probe_steps):
            if auto:
                probe["eager_ms"] = (self._sync_time() - probe["eager_t0"]) / (i - probe["eager_i0"]) * 1e3
            self.gstep = GraphedStep(self.trainer, batch, warmup=0)
            self.use_graph = True
            if auto:
                probe["graph_t0"], probe["graph_i0"] = self._sync_time(), i
        elif auto and self.gstep is not None and "graph_ms" not in probe and i - probe["graph_i0"] >= self.probe_steps:
            probe["graph_ms"] = (self._sync_time() - probe["graph_t0"]) / (i - probe["graph_i0"]) * 1e3
            self.use_graph = probe["graph_ms"] < probe["eager_ms"]

    def __call__(self, batch, i: int) -> torch.Tensor:
        """This call's ``i``-th step, on ``batch``; its loss."""
        if self.mode != "off" and i >= self.N_WARM:
            self._choose(batch, i)
        if self.use_graph and self.gstep.matches(batch):
            return self.gstep(batch).clone()  # (the captured loss tensor is overwritten by the next replay)
        return self.trainer.fit_step(batch)

    def take_out(self, spent: float) -> None:
        """The probe compares STEPS: ``spent`` seconds of a validation pass or a checkpoint leave the open window."""
        for k0, k1 in (("eager_t0", "eager_ms"), ("graph_t0", "graph_ms")):
            if k0 in self.probe and k1 not in self.probe:
                self.probe[k0] += spent


class FitRun:
    """One ``fit`` call on the device: the events of :func:`run_schedule`, their state, and the call's setup and teardown.
    Results go where ``fit`` documents them, on the trainer."""

    def __init__(self, trainer, plan: FitPlan, batches, loader, val, loop: dict | None, t_fit: float):
        """``loader``: ``batches`` where that is a loader, else None. ``loop``: the state ``load_checkpoint`` restored
        (the counters, the best tracker and the early-stopping rule go on from it) or None. ``t_fit``: the call's start on
        the monotonic clock."""
        self.trainer, self.plan, self.batches, self.loader, self.val, self.t_fit = trainer, plan, batches, loader, val, t_fit
        self.tracker = EarlyStopping(plan.mode, patience=None)  # the best value: strict improvements (ModelCheckpoint)
        self.stopper = EarlyStopping(plan.mode, *plan.early_stopping) if plan.early_stopping is not None else None
        # the loop's position is its OWN: batches done over all calls (`base` + this call's) and the (epoch, batch) the
        # next step reads
        self.base, self.seconds_before, self.pos = 0, 0.0, start_position(loader, plan)
        if loop is not None:
            self.base, self.seconds_before = int(loop["batches_done"]), float(loop["train_seconds"])
            self.pos = (int(loop["epoch"]), int(loop["next_batch"]))
            if loop["tracker"] is not None:
                self.tracker.load_state_dict(loop["tracker"])
            if self.stopper is not None and loop["stopper"] is not None:
                self.stopper.load_state_dict(loop["stopper"])
        self.losses: list[torch.Tensor] = []
        self.chooser = StepChooser(trainer, plan.graph, plan.graph_probe_steps)
        self.feed = DeviceFeed(trainer.module.model, plan.ring_slots, plan.graph != "off", loader is not None)

    # ------------------------------------------------------------------ the events
    def step(self, batch, ahead, i: int) -> None:
        self.losses.append(self.chooser(self.feed(batch, ahead), i))

    @property
    def last_pass(self) -> int | None:
        history = self.trainer.val_history
        return history[-1]["step"] if history else None

    def out_of_time(self) -> bool:
        return self.plan.time_limit is not None and time.monotonic() - self.t_fit >= self.plan.time_limit

    def validate(self, done: int, epoch: int | None) -> bool:
        """One pass between two steps; True when the loop should stop."""
        tr, plan, val = self.trainer, self.plan, self.val
        torch.cuda.current_stream(tr.module.model.device).synchronize()  # the steps enqueued so far are not validation time
        tv = time.perf_counter()
        metrics = val.evaluate(plan.stage) if plan.val_cutoffs is None else val.evaluate(plan.stage, cutoffs=plan.val_cutoffs)
        tr.val_elapsed += time.perf_counter() - tv
        tr.module.log_dict(metrics)
        tr.val_history.append({"step": done, **({"epoch": epoch} if plan.epoch_loop else {}), **metrics})
        value = metrics[plan.monitor]
        self.tracker.update(value)
        if self.tracker.improved:
            tr.best_score, tr.best_step = self.tracker.best, done
            if plan.best_path is not None:
                # replicas hold the same weights: rank 0 writes, nobody goes on before the directory is whole
                if tr.world_size == 1 or val.rank == 0:
                    tr.module.save(plan.best_path)
                if tr.world_size > 1:
                    torch.distributed.barrier(tr.process_group)
                tr.best_model_path = str(plan.best_path)
        stop = self.stopper.update(value) if self.stopper is not None else False
        self.chooser.take_out(time.perf_counter() - tv)
        return stop

    def loop_state(self, done: int) -> dict:
        tr = self.trainer
        return {"batches_done": done, "epoch": self.pos[0], "next_batch": self.pos[1], "tracker": self.tracker.state_dict(),
                "stopper": self.stopper.state_dict() if self.stopper is not None else None,
                "val_history": [dict(h) for h in tr.val_history], "best_score": tr.best_score, "best_step": tr.best_step,
                "best_model_path": tr.best_model_path,
                "train_seconds": self.seconds_before + (time.monotonic() - self.t_fit)}  # (for information only)

    def checkpoint(self, done: int) -> None:
        """``last.ckpt`` between two steps, on the loop's stream: one stream sync, the device-to-host copies, the write."""
        tr = self.trainer
        assert not torch.cuda.is_current_stream_capturing()
        torch.cuda.current_stream(tr.module.model.device).synchronize()  # the steps enqueued so far are not its time
        tc = time.perf_counter()
        tr._loop = self.loop_state(done)
        tr.save_checkpoint(self.plan.last_path)
        spent = time.perf_counter() - tc
        tr.ckpt_elapsed += spent
        self.chooser.take_out(spent)

    # ------------------------------------------------------------------ setup, loop, teardown
    @contextlib.contextmanager
    def _on_device(self):
        """What a call changes for its duration, and puts back however the loop ends. Under ``graph != "off"``: the step
        counter moves to the device, ``defer_logging`` "auto" becomes False (one stream: what the capture records), a
        loader runs ``fixed_width`` (one shape for the captured step, one layout for the steps around it), and the whole
        loop runs on a side stream -- torch's capture protocol: autograd's AccumulateGrad nodes are bound to the stream of
        their first backward, and captured from the default stream the capture faults."""
        tr, loader, graphed = self.trainer, self.loader, self.plan.graph != "off"
        module, dev = tr.module, tr.module.model.device
        defer_before = module.defer_logging
        fixed_before = loader.fixed_width if loader is not None else None
        cur = side = None
        if graphed:
            _refuse_capture_after_default_stream_steps(tr)
        try:
            if graphed:
                tr._seed_device_step()
                if defer_before == "auto":
                    module.defer_logging = False
                cur, side = torch.cuda.current_stream(dev), torch.cuda.Stream(device=dev)
                side.wait_stream(cur)
                if loader is not None:
                    loader.fixed_width = True
            with (torch.cuda.stream(side) if side is not None else contextlib.nullcontext()):
                yield
        finally:
            if loader is not None:
                loader.fixed_width = fixed_before
            if side is not None:
                cur.wait_stream(side)
            if graphed:
                module.defer_logging = defer_before
                tr.optimizer.sync_step_from_device()  # replays advanced the counter on the device only
            tr.graph_choice = "graph" if self.chooser.use_graph else "eager"
            tr.graph_probe = {k: round(v, 4) for k, v in self.chooser.probe.items() if k.endswith("_ms")}
            self.feed.close()

    def run(self) -> list[float]:
        tr, plan = self.trainer, self.plan
        t0 = time.time()
        with self._on_device():
            source = batch_source(self.batches, plan, self.pos, self.base, is_loader=self.loader is not None)
            done, stop = run_schedule(plan, source, self.base, self)
            tr.stopped_early, tr.stopped_on_time = stop == "early", stop == "time"
            tr._loop = self.loop_state(done)
            if plan.save_last:
                self.checkpoint(done)
        tr.elapsed = time.time() - t0
        return [float(v) for v in self.losses]  # (one host sync at the end, not one per step)
