"""Full-state trainer checkpoints: the file format, ``max_time`` parsing and the compatibility checks.

Nothing here needs a GPU or the native library: :class:`~xfmr_rec_amd.trainer.Trainer` gathers the state and puts it back
(``state_dict`` / ``load_state_dict``), this module says what a file holds, writes it so that a failure leaves the file
that was there, and decides whether a state may be loaded into a given trainer and loader.

A checkpoint is ONE ``torch.save`` of a plain dict -- tensors, Python scalars, strings, lists and dicts, nothing pickled
beyond them -- read back with ``torch.load(..., weights_only=True, map_location="cpu")``:

    format, version      "xfmr-trainer-checkpoint", 1
    state_dict           ``module.state_dict()``: HF-keyed encoder tensors under ``model.model.0.auto_model.``, no table
    hyper_parameters     {"config": config.model_dump()}
    epoch, global_step   Lightning's names; global_step counts OPTIMIZER steps
    optimizer            ``FusedAdamW.state_dict()``
    model                {"dropout_step", "seed", "device_step"}
    trainer              accumulate_grad_batches, gradient_clip_algorithm, gradient_clip_val, lr_scheduler, world_size
    loop                 ``Trainer.fit``'s counters, best tracker, stopper and validation history
    loader               the loader's identity (LOADER_FIELDS), or None for a plain iterable

``state_dict``, ``hyper_parameters``, ``epoch`` and ``global_step`` carry the names Lightning gives them; Lightning itself
has never read one of these files.
"""

from __future__ import annotations

import datetime
import os
import pathlib
import tempfile

import torch

FORMAT = "xfmr-trainer-checkpoint"
VERSION = 1
KEYS = ("format", "version", "state_dict", "hyper_parameters", "epoch", "global_step", "optimizer", "model", "trainer",
        "loop", "loader")
TRAINER_FIELDS = ("accumulate_grad_batches", "gradient_clip_algorithm", "gradient_clip_val", "lr_scheduler", "world_size")
LOADER_FIELDS = ("seed", "batch_size", "shuffle", "drop_last", "rank", "world_size", "dataset_length", "fixed_width")
ENC_PREFIX = "model.model.0.auto_model."


def plain(obj, where: str = "checkpoint"):
    """``obj`` as the file holds it: tuples become lists, everything else must be a tensor, a Python scalar, a string,
    None, a list or a dict with string or integer keys. Anything else raises a ``TypeError`` that names where it sits."""
    if obj is None or isinstance(obj, str):
        return obj
    for t in (bool, int, float):  # (exactly these: a subclass such as numpy.float64 would be pickled as an object)
        if isinstance(obj, t):
            return t(obj)
    if torch.is_tensor(obj):
        return obj.detach().cpu()
    if getattr(obj, "ndim", None) == 0 and hasattr(obj, "item"):  # a numpy scalar (a metric's value): its Python value
        return plain(obj.item(), where)
    if isinstance(obj, (list, tuple)):
        return [plain(v, f"{where}[{i}]") for i, v in enumerate(obj)]
    if isinstance(obj, dict):
        for k in obj:
            if isinstance(k, bool) or not isinstance(k, (str, int)):
                raise TypeError(f"{where}: key {k!r} is neither a string nor an integer")
        return {k: plain(v, f"{where}[{k!r}]") for k, v in obj.items()}
    raise TypeError(f"{where}: {type(obj).__name__} cannot be part of a checkpoint (tensors, scalars, strings, lists, dicts)")


def write_checkpoint(state: dict, path) -> int:
    """``state`` -> ``path``, atomically: written under a temporary name in the same directory, flushed and fsynced, then
    moved over ``path`` (``os.replace``). A failure at any point leaves the file that was at ``path`` as it was and no
    temporary file behind. Returns the file's size in bytes."""
    path = pathlib.Path(path)
    state = plain(state)
    if state.get("format") != FORMAT or state.get("version") != VERSION:
        raise ValueError(f"not a version {VERSION} {FORMAT!r} state: format = {state.get('format')!r}, "
                         f"version = {state.get('version')!r}")
    path.parent.mkdir(parents=True, exist_ok=True)
    fd, tmp = tempfile.mkstemp(dir=str(path.parent), prefix=path.name + ".", suffix=".tmp")
    try:
        with os.fdopen(fd, "wb") as f:
            torch.save(state, f)
            f.flush()
            os.fsync(f.fileno())
        size = os.path.getsize(tmp)
        os.replace(tmp, path)
    except BaseException:
        _unlink_quietly(tmp)
        raise
    return size


def _unlink_quietly(name) -> None:
    try:
        os.unlink(name)
    except FileNotFoundError:
        pass


def read_checkpoint(path) -> dict:
    """The dict of :func:`write_checkpoint`, tensors on the host. A file of another format or version raises a
    ``ValueError`` that says which."""
    state = torch.load(str(path), weights_only=True, map_location="cpu")
    if not isinstance(state, dict) or state.get("format") != FORMAT:
        got = state.get("format") if isinstance(state, dict) else type(state).__name__
        raise ValueError(f"{path}: format {got!r} is not {FORMAT!r}")
    if state.get("version") != VERSION:
        raise ValueError(f"{path}: checkpoint version {state.get('version')!r} is not supported (this build reads version "
                         f"{VERSION})")
    missing = [k for k in KEYS if k not in state]
    if missing:
        raise ValueError(f"{path}: checkpoint keys {missing} are missing")
    return state


def parse_max_time(v) -> float | None:
    """Lightning's ``Trainer(max_time=...)`` forms as seconds: None, a number of seconds, a ``datetime.timedelta``, a
    ``"DD:HH:MM:SS"`` string or a dict of ``days`` / ``hours`` / ``minutes`` / ``seconds``."""
    if v is None:
        return None
    if isinstance(v, datetime.timedelta):
        return v.total_seconds()
    if isinstance(v, (int, float)) and not isinstance(v, bool):
        if v != v:
            raise ValueError(f"max_time: {v!r} is not a duration")
        return float(v)
    if isinstance(v, str):
        parts = v.strip().split(":")
        if len(parts) == 4 and all(p.isdecimal() for p in parts):
            d, h, m, s = (int(p) for p in parts)
            return float(((d * 24 + h) * 60 + m) * 60 + s)
        raise ValueError(f"max_time: {v!r} is not of the form 'DD:HH:MM:SS'")
    if isinstance(v, dict):
        units = {"days": 86400.0, "hours": 3600.0, "minutes": 60.0, "seconds": 1.0}
        extra = sorted(set(v) - set(units))
        if extra or not v:
            raise ValueError(f"max_time: a dict takes the keys {sorted(units)}; got {sorted(v)}")
        for k, x in v.items():
            if isinstance(x, bool) or not isinstance(x, (int, float)) or x != x:
                raise ValueError(f"max_time: {k} = {x!r} is not a number")
        return float(sum(units[k] * x for k, x in v.items()))
    raise ValueError(f"max_time: {v!r} is not a number of seconds, a timedelta, a 'DD:HH:MM:SS' string or a dict")


def reference_checkpoint_options(cfg: dict) -> dict:
    """``{"max_time": seconds | None, "ckpt_path": str | None}`` of a parsed reference ``config.yaml``: its
    ``trainer.max_time`` (``xfmr_rec/trainer.py:453``: "00:04:00:00") and the top-level ``ckpt_path`` -- ``Trainer.fit``'s
    arguments of the same names. An empty ``ckpt_path`` means none, as in the reference's entry points."""
    block = cfg.get("trainer") or {}
    if not isinstance(block, dict):
        raise ValueError(f"trainer: expected a mapping, got {type(block).__name__}")
    try:
        max_time = parse_max_time(block.get("max_time"))
    except ValueError as e:
        raise ValueError(f"trainer.{e}") from None
    ckpt = cfg.get("ckpt_path")
    if ckpt is not None and not isinstance(ckpt, (str, os.PathLike)):
        raise ValueError(f"ckpt_path: {ckpt!r} is not a path")
    return {"max_time": max_time, "ckpt_path": (os.fspath(ckpt) or None) if ckpt is not None else None}


def loader_fields(loader) -> dict | None:
    """What identifies a :class:`~xfmr_rec_amd.data.DeviceSeqLoader`'s sequence of batches (LOADER_FIELDS); None for
    anything else (a plain iterable of batches)."""
    if loader is None or not all(hasattr(loader, k) for k in ("epoch_order", "batch_size", "fixed_width", "dataset")):
        return None
    return {"seed": int(loader.seed), "batch_size": int(loader.batch_size), "shuffle": bool(loader.shuffle),
            "drop_last": bool(loader.drop_last), "rank": int(loader.rank), "world_size": int(loader.world_size),
            "dataset_length": int(len(loader.dataset)), "fixed_width": bool(loader.fixed_width)}


def state_flat_numel(state: dict) -> int:
    """Parameters in a checkpoint's ``state_dict``: the elements of its tensors under the encoder prefix."""
    return int(sum(v.numel() for k, v in state["state_dict"].items() if k.startswith(ENC_PREFIX) and torch.is_tensor(v)))


def check_compatible(state: dict, *, flat_numel: int, trainer: dict, loader: dict | None) -> None:
    """Whether ``state`` continues in a trainer of ``flat_numel`` parameters with the options ``trainer``
    (TRAINER_FIELDS) over ``loader`` (:func:`loader_fields`). The first difference raises a ``ValueError`` that names the
    field. What only bounds a run -- ``max_epochs``, ``max_steps``, ``val_check_interval``, ``limit_train_batches`` -- is
    not part of a checkpoint: extending a run is the common case."""
    got = state_flat_numel(state)
    if got != int(flat_numel):
        raise ValueError(f"checkpoint mismatch: flat parameter count {got} in the checkpoint, {int(flat_numel)} in this model")
    saved = state["trainer"]
    for k in TRAINER_FIELDS:
        if plain(saved.get(k)) != plain(trainer.get(k)):
            raise ValueError(f"checkpoint mismatch: trainer {k} = {saved.get(k)!r} in the checkpoint, {trainer.get(k)!r} in "
                             "this trainer")
    saved_ld = state["loader"]
    if (saved_ld is None) != (loader is None):
        raise ValueError("checkpoint mismatch: loader: the checkpoint was taken over "
                         f"{'a plain iterable' if saved_ld is None else 'a DeviceSeqLoader'}, this run is over "
                         f"{'a plain iterable' if loader is None else 'a DeviceSeqLoader'}")
    if loader is not None:
        for k in LOADER_FIELDS:
            if saved_ld.get(k) != loader.get(k):
                raise ValueError(f"checkpoint mismatch: loader {k} = {saved_ld.get(k)!r} in the checkpoint, {loader.get(k)!r} "
                                 "in this loader")
