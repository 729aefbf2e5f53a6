"""The training step's host side in its parts ("The step's parts").

Without a device or a module (tests/test_step_plan_host.py): :class:`StepPlan` -- what one ``compute_losses`` call
decides before it launches anything (the refusals, the layout, the form, the logged heads, the loss options);
:data:`KEY_TABLE` -- every key the reference logs and where its value lives; :func:`head_vector` -- which vector
carries a head in which form; :func:`step_result` -- the dict ``compute_losses`` returns, in its three forms; and the
two views of that dict, :func:`host_values` (floats) and :func:`device_values` (0-dim device tensors)."""

from __future__ import annotations

import functools
from typing import NamedTuple

import torch

from . import _native as N
from .ops import LossOpts

HEADS = tuple(N.LOSS_IDS)  # head i of the kernels' loss vector is LOSS_CLASSES[i] (tests/test_step_plan_host.py)

# the side-stream logging pass pays once it is long enough to be worth hiding: B x L >= 51 200 tokens
# (round 4, bench.py --overlap on / off, one box: batch 256 x 200 1.918-1.947 against 1.958-1.962 ms, batch 128
#  1.193 against 1.178; round 1 had measured -1.4 % at 256 and set 102 400)
AUTO_DEFER_TOKENS = 51200
# PACKED rows only below this fill of the padded batch (a nearly full batch gains nothing: the pack launch and the
# length-ordered offsets cost what the few padding rows would)
PACKED_MAX_FILL = 0.97


_ALL_HEADS = tuple(enumerate(HEADS))


def logged_heads(train_loss: str, log_all_losses: bool) -> tuple:
    """The ``(index, name)`` pairs of the heads a step logs: all seven, or the train head alone."""
    return _ALL_HEADS if log_all_losses else ((N.LOSS_IDS[train_loss], train_loss),)


class StepPlan(NamedTuple):
    """What one ``compute_losses`` call does, decided from plain values by :meth:`build` before anything launches.
    (A ``NamedTuple``: it is built inside ``torch.compile(fullgraph=True)`` traces of the step, too.)"""

    catalogue: bool         # negatives="catalogue": every table row is a column, pos_item_idx the target
    batch: int
    L: int                  # what the encoder keeps of the history: min(width, max_seq_length)
    packed: bool            # the encoder and the loss run on each sequence's own rows only
    rows: int               # token rows they run on: the lengths' sum when packed, else batch * L
    padded_positions: int   # batch * L when packed (the densities' denominator stays the padded shape), else 0
    defer: bool             # the caller's defer_logging, "auto" resolved
    overlap: bool           # the logging heads run on the side stream underneath the backward
    train_loss: str
    log_all_losses: bool
    heads: tuple            # logged_heads(train_loss, log_all_losses)
    opts: LossOpts          # the loss calls' options (what belongs to one call -- table_bf16, a workspace -- is its argument)

    @classmethod
    def build(cls, cfg, *, batch: int, width: int, max_seq_length: int, has_lengths: bool = False, rows: int = 0,
              supports_packed: bool = False, tracing: bool = False, capturing: bool = False, defer_logging=False,
              grad: bool = False, has_table_bf16: bool = False) -> "StepPlan":
        """``cfg``: anything with the fields ``negatives``, ``target_position``, ``train_loss``, ``log_all_losses``,
        ``mask_false_negatives``, ``scale``, ``margin``, ``precision`` and ``num_hard_negatives`` (a ``LightningConfig``).
        ``batch`` x ``width``: the history's shape. ``has_lengths``: the batch carries its rows' lengths on the HOST, and
        ``rows`` is their sum. ``supports_packed``: the model's answer for L. ``tracing`` / ``capturing``: under
        ``torch.compile`` / inside a stream capture. ``defer_logging``: True, False or "auto". ``grad``: the parameters
        require a gradient and autograd is on. Every refusal is a ``ValueError``."""
        c = cfg
        if c.negatives not in ("in_batch", "catalogue"):
            raise ValueError(f"invalid {c.negatives = }")
        catalogue = c.negatives == "catalogue"
        if not catalogue and c.target_position != "first":
            raise ValueError("the training path scores [positive | shared negatives]: target_position='first'")
        if catalogue and c.target_position is not None:
            raise ValueError("negatives='catalogue' names the positive by `target` (= pos_item_idx): "
                             "target_position=None (losses.py:233-238)")
        L = min(width, max_seq_length)  # what _encode_tokens keeps of the history
        # PACKED rows (xfmr_encoder_cfg.seq_offsets): when the batch carries its rows' lengths on the HOST -- the collate that
        # right-padded them knows them (data.py:799-805); PinnedBatchRing hands them over -- the encoder and the loss run on
        # each sequence's own rows only. The reference's padded layout computes the padding rows too and then drops them
        # (models.py:392); on MovieLens-like lengths that is half of the encoder's work. The launch sizes need the row
        # count on the host (device-side lengths would cost a sync per step), a traced or captured step has one fixed size,
        # and a history wider than L is cut by the padded path.
        packed = (has_lengths and width == L and supports_packed and not tracing and not capturing
                  and 0 < rows <= PACKED_MAX_FILL * batch * L)
        if defer_logging == "auto":
            defer_logging = batch * L >= AUTO_DEFER_TOKENS
        overlap = (bool(defer_logging) and c.log_all_losses and grad and has_table_bf16 and c.precision == "bf16"
                   and c.num_hard_negatives == 0
                   # unmasked InfoNCE: ONE call runs the logging pass first and pins the gradient pass's running
                   # maximum from its records (lean epilogue) -- worth more than the overlap
                   and not (c.train_loss == "InfoNCELoss" and not c.mask_false_negatives)
                   # a traced step is one stream (the overlapped form hands a raw event handle to the forward)
                   and not tracing)
        padded_positions = batch * L if packed else 0
        opts = LossOpts(train_head=c.train_loss, all_heads=c.log_all_losses, mask_false_negatives=c.mask_false_negatives,
                        mode=N.NEG_CATALOG if catalogue else N.NEG_SHARED, scale=c.scale, margin=c.margin,
                        precision=c.precision, num_hard_negatives=c.num_hard_negatives, padded_positions=padded_positions)
        return cls(catalogue=catalogue, batch=batch, L=L, packed=packed, rows=rows if packed else batch * L,
                   padded_positions=padded_positions, defer=bool(defer_logging), overlap=overlap, train_loss=c.train_loss,
                   log_all_losses=c.log_all_losses, heads=logged_heads(c.train_loss, c.log_all_losses), opts=opts)


def _key_table() -> tuple:
    S = N.STAT
    rows = []
    for i, name in enumerate(HEADS):
        rows += [(f"loss/{name}", "sum", i, None), (f"loss/{name}Mean", "mean", i, None)]
    rows += [(f"batch/{k}", "const", k, None) for k in ("size", "seq_len", "numel")]  # trainer.py:241-244
    rows += [("batch/attention_non_zero", "stat", S["n_valid"], None), ("batch/attention_density", "stat", S["attn_density"], None),
             ("batch/positive_non_zero", "stat", S["n_query"], None), ("batch/positive_density", "stat", S["pos_density"], None),
             ("logits/neg/density", "stat", S["neg_density"], None)]
    for side, gate in (("pos", "n_query"), ("neg", "neg_count")):  # losses.py:392-404
        rows += [(f"logits/{side}/{k}", "stat", S[f"{side}_{k}"], S[gate]) for k in ("mean", "std", "min", "max")]
    return tuple(rows)


KEY_TABLE = _key_table()
"""Every key the reference logs per step (``trainer.py:241-263``, ``losses.py:392-404``) as ``(key, kind, index, gate)``:
kind "sum" / "mean" -- entry ``index`` / ``NUM_LOSSES + index`` of the loss vector that :func:`head_vector` names; "const"
-- a host constant of the PADDED batch shape, known without a sync; "stat" -- entry ``index`` of the statistics vector.
A step logs the rows :func:`logged_keys` selects.

:func:`device_values` is the table read literally. :func:`host_values` differs from it in three ways, all of them kept
as they have always been:

- It divides in double where the kernel divides in fp32: ``loss/<Class>Mean`` is the head's sum over
  ``n_query + 1e-9``, ``batch/positive_density`` is ``n_query / (n_valid + 1e-9)`` and ``batch/attention_density`` is
  ``n_valid / (batch/numel + 1e-9)``; the two counts are ints. (The synchronous form of ``compute_losses`` keeps its loss
  entries as the kernels' tensors -- the train head carries the gradient -- so its means are the kernel's.)
- It omits a gated row whose ``gate`` entry of the statistics vector is not > 0 -- ``logits/pos/*`` of a step without
  a query row, ``logits/neg/{mean,std,min,max}`` without a negative -- as the reference does; the device view has the
  kernel's NaN there.
- ``batch/attention_density`` comes from the host constant ``batch/numel``, not from the statistics vector's entry.
"""

_N_VALID, _N_QUERY = N.STAT["n_valid"], N.STAT["n_query"]


@functools.lru_cache(maxsize=None)
def logged_keys(train_loss: str, log_all_losses: bool) -> tuple:
    """The rows of :data:`KEY_TABLE` a step logs: the logged heads' and ``batch/*``; with all heads, ``logits/*`` too."""
    if log_all_losses:
        return KEY_TABLE
    return tuple(r for r in KEY_TABLE if (HEADS[r[2]] == train_loss if r[1] in ("sum", "mean") else r[0].startswith("batch/")))


def head_vector(name: str, train_loss: str, losses, losses_train=None):
    """The ONE rule of which loss vector carries a head's sum and mean. The plain forms: the vector the single loss call
    returned. The overlapped form: the side-stream pass's vector (``losses``), except that the train head's entries come
    from the gradient call's (``losses_train``): each pass leaves the other's heads at 0."""
    return losses_train if (losses_train is not None and name == train_loss) else losses


def step_result(plan: StepPlan, train_loss, losses, losses_train, stats, *, sync: bool) -> dict:
    """The dict ``compute_losses`` returns, in one of three forms. ``loss/<Class>`` of the logged heads (the train head's
    is ``train_loss``, the tensor that carries the gradient) and the three host constants are in all of them. Plain
    (``losses_train`` None): ``loss/<Class>Mean`` too, and then either ``stats/device`` or, with ``sync``, the host view of
    the statistics (one device->host sync; the reference does 11 ``.item()`` calls). Overlapped: the raw vectors
    ``stats/device``, ``losses/device`` (the side-stream pass: train head entries = 0) and ``losses_train/device`` (the
    gradient call: train head only) -- nothing of the side stream's may be read before ``sync_logging()``."""
    out: dict = {}
    for i, name in plan.heads:
        out[f"loss/{name}"] = train_loss if name == plan.train_loss else losses[i]
        if losses_train is None:
            out[f"loss/{name}Mean"] = losses[N.NUM_LOSSES + i]  # computed by the final kernel
    if losses_train is not None:
        out["losses/device"] = losses
        out["losses_train/device"] = losses_train
    # trainer.py:241-244: known without a device sync, logged in every form (the padded shape, also when the rows were packed)
    out |= {"batch/size": plan.batch, "batch/seq_len": plan.L, "batch/numel": plan.batch * plan.L}
    if sync and losses_train is None:
        return out | host_values(out | {"stats/device": stats}, plan, losses=False)
    out["stats/device"] = stats
    return out


def host_values(out: dict, cfg, *, losses: bool = True) -> dict:
    """The logged keys of a :func:`step_result` as host numbers: one ``.tolist()`` per vector the dict carries (head sums
    that are tensors of their own -- the train head's, and all of them in the plain device form -- are read one by one).
    ``cfg``: the plan or the config (``train_loss``, ``log_all_losses``). ``losses=False``: without the ``loss/*`` rows.
    The differences from :func:`device_values` are :data:`KEY_TABLE`'s three."""
    if "stats/device" not in out:  # the synchronous form: already complete
        return {k: float(v) for k, v in out.items() if not k.endswith("/device")}
    s = out["stats/device"].tolist()
    n_valid, n_query = int(s[_N_VALID]), int(s[_N_QUERY])
    in_double = {"batch/attention_non_zero": n_valid, "batch/attention_density": n_valid / (out["batch/numel"] + 1e-9),
                 "batch/positive_non_zero": n_query, "batch/positive_density": n_query / (n_valid + 1e-9)}
    side = out.get("losses/device")
    vals = side.tolist() if (side is not None and losses) else None
    res: dict = {}
    for key, kind, i, gate in logged_keys(cfg.train_loss, cfg.log_all_losses):
        if kind == "sum" and losses:
            res[key] = float(out[key]) if (vals is None or HEADS[i] == cfg.train_loss) else vals[i]
        elif kind == "mean" and losses:
            res[key] = res[f"loss/{HEADS[i]}"] / (n_query + 1e-9)
        elif kind == "const":
            res[key] = out[key]
        elif key in in_double:
            res[key] = in_double[key]
        elif kind == "stat" and (gate is None or s[gate] > 0):
            res[key] = s[i]
    return res


def device_values(out: dict, cfg) -> dict:
    """The logged keys of a :func:`step_result` as 0-dim tensors -- views of the kernels' output vectors: no host sync, no
    torch arithmetic. ``cfg``: the plan or the config. Read after ``sync_logging()``."""
    stats = out.get("stats/device")
    if stats is None:  # the synchronous form: already complete
        return {k: torch.as_tensor(v) for k, v in out.items() if not k.endswith("/device")}
    side, own = out.get("losses/device"), out.get("losses_train/device")
    res: dict = {}
    for key, kind, i, _ in logged_keys(cfg.train_loss, cfg.log_all_losses):
        if kind == "sum":
            res[key] = out[key].detach()
        elif kind == "mean":
            res[key] = out[key] if side is None else head_vector(HEADS[i], cfg.train_loss, side, own)[N.NUM_LOSSES + i]
        elif kind == "const":
            res[key] = torch.as_tensor(out[key])
        else:
            res[key] = stats[i]
    return res
