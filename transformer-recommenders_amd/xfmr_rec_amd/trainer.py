"""Training-step driver: host-side mirror of ``xfmr_rec/trainer.py`` (the LightningModule surface).

``RecommenderLightningModule`` keeps the reference's method names and semantics for the training path --
``configure_model``, ``forward``, ``compute_losses`` (all seven heads + batch / logits statistics every
step, ``trainer.py:213-264``), ``training_step`` (returns ``loss/{train_loss}``, ``trainer.py:288-291``),
``configure_optimizers`` (AdamW lr 1e-3 / wd 0.01 over all parameters, ``trainer.py:327-332``) and
``state_dict`` without the frozen table (``trainer.py:352-362``). When ``lightning`` is importable it
subclasses ``lightning.pytorch.LightningModule`` so ``LightningCLI(lightning_module_cls=...)``
(``trainer.py:377-395``) accepts it; otherwise it is a plain ``nn.Module`` driven by :class:`Trainer`.

One step on the device is: gather+mask+BertEmbeddings -> N x BertLayer -> fused loss (7 heads + stats +
dL/dtok in one pass) -> encoder backward -> [flat-gradient all-reduce under DDP] -> fused AdamW. All of it is
HIP kernels from ``libxfmr_hip.so``; torch supplies memory, streams, autograd bookkeeping and RCCL.
"""

from __future__ import annotations

import ctypes
import math
import os
import time

import numpy as np
import torch

from . import _native as N
from . import eval_rows as E
from . import ops
from .losses import LOSS_CLASSES, LossConfig, LossType
from .models import ModelConfig, RecommenderModel
from .params import METRIC, TOP_K
from .step_plan import StepPlan, device_values, host_values, step_result

try:  # pragma: no cover - lightning is not installed in the build image
    import lightning.pytorch as _lp

    _Base = _lp.LightningModule
except Exception:  # noqa: BLE001
    _lp = None
    _Base = torch.nn.Module


class LightningConfig(LossConfig, ModelConfig):
    """``trainer.py:98-115`` minus the LanceDB index configs (retrieval is out of the hot path)."""

    train_loss: LossType = "InfoNCELoss"
    learning_rate: float = 0.001
    weight_decay: float = 0.01
    top_k: int = TOP_K
    # trainer.py:103-115: the LanceDB index configs. Accepted so that the reference's config files load unchanged; the
    # exact top-k search of this build (retrieval.py) has no index to configure.
    items_config: dict = {}
    users_config: dict = {}
    # build-specific knobs (not in the reference)
    precision: str = "bf16"  # MFMA arithmetic: "bf16" (reference default bf16-mixed) or "fp32"
    log_all_losses: bool = True  # evaluate all 7 heads + statistics every step like trainer.py:250-264
    # "in_batch": [positive | the batch's sampled negatives] (models.py:366-419, the reference's only mode);
    # "catalogue": every row of the item table is a column and pos_item_idx is the target -- the reference API's
    # EmbedLoss.forward(q, table[None].expand(N,-1,-1), target=pos_idx) with target_position=None (SURVEY F9;
    # BASELINE config 4 "full-catalogue softmax"). The (Np x V) logits are never materialised.
    negatives: str = "in_batch"


class FusedAdamW(torch.optim.Optimizer):
    """``torch.optim.AdamW`` semantics (decoupled decay, bias correction, eps outside sqrt) as one HIP launch
    over the flat parameter buffer. Parameters without a gradient are skipped, as torch does.

    ``step_device``: an int32 device tensor holding the number of completed steps. The launch then reads the step count
    from it (``xfmr_adamw_dev``) and advances it afterwards (``xfmr_step_advance``) -- no host-computed argument changes
    from step to step, so the step can be captured into a hipGraph and replayed."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, grad_scale=1.0, step_device=None,
                 clip_mode=None, clip_val=None, schedule=None):
        """``clip_mode``: None, "norm" (``clip_grad_norm_``) or "value" (``clip_grad_value_``) with ``clip_val``;
        ``schedule``: ``{"name": "constant" | "warmup_constant" | "warmup_linear" | "warmup_cosine", "warmup_steps",
        "total_steps"}`` -- a ``LambdaLR`` stepped once per optimizer step. With either set the step is
        ``xfmr_opt_prepare`` + ``xfmr_adamw_ctl``: norm, clip coefficient and learning rate are produced and consumed on
        the device (``self.ctl``), so the step stays capturable. The clip is folded into the update: ``p.grad`` itself is
        left unclipped. Neither is part of ``state_dict()``: the schedule is a function of the step
        count that is."""
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, grad_scale=grad_scale))
        self.step_device = step_device
        ops.make_opt_cfg(lr=lr, clip_mode=clip_mode, clip_val=clip_val, schedule=schedule)  # (validates, loudly, now)
        self.clip_mode, self.clip_val = clip_mode, clip_val
        self.schedule = dict(schedule) if schedule is not None else None
        self._opt_bufs: dict = {}  # parameter -> (ctl, workspace), created at the first step

    @property
    def has_options(self) -> bool:
        return self.clip_mode is not None or (self.schedule is not None and self.schedule.get("name", "constant") != "constant")

    @property
    def ctl(self) -> torch.Tensor | None:
        """The xfmr_opt_ctl record of the last step as 8 fp32 device words (``_native.CTL`` names them); None before the
        first step with an option set."""
        return next(iter(self._opt_bufs.values()))[0] if self._opt_bufs else None

    def ctl_log_dict(self) -> dict[str, torch.Tensor]:
        """``grad/norm``, ``grad/clip_coef`` and ``lr`` of the last step: 0-dim device views of ``ctl``, no host sync."""
        ctl = self.ctl
        if ctl is None:
            return {}
        return {"grad/norm": ctl[N.CTL["grad_norm"]], "grad/clip_coef": ctl[N.CTL["clip_coef"]], "lr": ctl[N.CTL["lr"]]}

    @torch.no_grad()
    def step(self, closure=None):
        loss = closure() if closure is not None else None
        options = self.has_options
        if options and self.clip_mode == "norm" and sum(p.grad is not None for g in self.param_groups for p in g["params"]) > 1:
            raise ValueError("clip_mode='norm' clips by the norm of ONE flat gradient buffer; this optimizer holds several")
        for group in self.param_groups:
            b1, b2 = group["betas"]
            for p in group["params"]:
                if p.grad is None:
                    continue
                st = self.state[p]
                if not st:
                    st["step"] = 0
                    st["exp_avg"] = torch.zeros_like(p)
                    st["exp_avg_sq"] = torch.zeros_like(p)
                st["step"] += 1
                if not options:
                    ops.adamw_(p.data, p.grad.contiguous(), st["exp_avg"], st["exp_avg_sq"], lr=group["lr"], beta1=b1,
                               beta2=b2, eps=group["eps"], weight_decay=group["weight_decay"], step=st["step"],
                               grad_scale=group["grad_scale"], step_device=self.step_device)
                    continue
                grad = p.grad.contiguous()
                if p not in self._opt_bufs:
                    self._opt_bufs[p] = ops.opt_buffers(grad)
                ctl, ws = self._opt_bufs[p]
                cfg = ops.make_opt_cfg(lr=group["lr"], beta1=b1, beta2=b2, eps=group["eps"], weight_decay=group["weight_decay"],
                                       grad_scale=group["grad_scale"], clip_mode=self.clip_mode, clip_val=self.clip_val,
                                       schedule=self.schedule, step=st["step"], step_device=self.step_device)
                ops.opt_prepare_(cfg, grad, ws, ctl)
                ops.adamw_ctl_(cfg, p.data, grad, st["exp_avg"], st["exp_avg_sq"], ctl)
        if self.step_device is not None:
            ops.step_advance_(self.step_device)
        return loss

    def sync_step_from_device(self) -> None:
        """Write the device-side step counter back into ``state[p]["step"]``. Replays of a captured step advance the counter
        on the device only: without this a ``state_dict()`` taken after ``fit(graph="on")`` would carry a stale step, and a
        resume (or a later ``fit`` seeding its counter from it) the wrong bias corrections. One host sync."""
        if self.step_device is None:
            return
        n = int(self.step_device.item())
        for st in self.state.values():
            if "step" in st:
                st["step"] = n

    def state_dict(self):
        self.sync_step_from_device()
        return super().state_dict()


class RecommenderLightningModule(_Base):
    def __init__(self, config: LightningConfig) -> None:
        super().__init__()
        self.config = LightningConfig.model_validate(config)
        if _lp is not None:  # pragma: no cover
            self.save_hyperparameters(self.config.model_dump())
            self.strict_loading = False
        self.model: RecommenderModel | None = None
        self.items_dataset = None
        self.loss_fns: torch.nn.ModuleList | None = None
        self.logged: dict = {}
        # ---- the training step's state (compute_losses / training_step / on_train_batch_end)
        self.defer_logging: bool | str = "auto"  # training_step's form: True / False, or "auto" (StepPlan: by the batch's size)
        self.profile_events = None   # bench.py: (gradient pass, logging pass) hipEvent pairs handed to the loss calls
        self.last_plan: StepPlan | None = None  # what the last compute_losses call decided
        self.last_out: dict | None = None       # the last finished step's raw device outputs (detached)
        self._pending_out: dict | None = None   # training_step's outputs until on_train_batch_end logs them
        self._side = None                # the logging stream (lowest priority), made by the first overlapped step
        self._logging_pending = False    # a logging pass is in flight on it: sync_logging() joins
        self._ev_embed = self._ev_prep = None  # overlapped step: "the key mask is written" / "both loss calls are prepared"

    # lightning supplies .device; the plain-module build derives it from the parameters
    def _device(self):
        if self.model is not None:
            return self.model.device
        return torch.device("cuda" if torch.cuda.is_available() else "cpu")

    def configure_model(self) -> None:
        """``trainer.py:139-161``."""
        if self.model is None:
            self.model = RecommenderModel(self.config, device=self._device(), precision=self.config.precision)
        if self.items_dataset is None and _lp is not None:  # pragma: no cover
            try:
                self.items_dataset = self.trainer.datamodule.items_dataset
            except RuntimeError:
                pass
        if self.items_dataset is not None:
            self.model.configure_embeddings(self.items_dataset)
        if self.loss_fns is None:
            self.loss_fns = self.get_loss_fns()

    def get_loss_fns(self) -> torch.nn.ModuleList:
        """``trainer.py:163-170``."""
        return torch.nn.ModuleList([cls(self.config, precision=self.config.precision) for cls in LOSS_CLASSES])

    def forward(self, item_idx: torch.Tensor) -> dict[str, torch.Tensor]:
        assert self.model is not None
        return self.model(item_idx.to(self.model.device))

    def _side_stream(self):
        if self._side is None:
            # lowest priority: the logging pass fills what the training chain leaves idle instead of competing with it
            # (XFMR_LOG_STREAM_PRIORITY overrides; torch: lower number = higher priority, 0 = the default stream's)
            # (torch offers only "normal" and "high": the stream comes from the library. XFMR_LOG_STREAM_PRIORITY=0:
            # a normal-priority torch stream.)
            if os.environ.get("XFMR_LOG_STREAM_PRIORITY", "low") == "0":
                self._side = torch.cuda.Stream(device=self.model.device)
            else:
                handle = ctypes.c_void_p()
                with torch.cuda.device(self.model.device):
                    N.check(N.load().xfmr_low_priority_stream_create(ctypes.byref(handle)), "xfmr_low_priority_stream_create")
                self._side = torch.cuda.ExternalStream(handle.value, device=self.model.device)
        return self._side

    def sync_logging(self) -> None:
        """Join the side stream of a deferred logging pass (see compute_losses(defer_logging=True))."""
        if self._logging_pending:
            torch.cuda.current_stream().wait_stream(self._side)
            self._logging_pending = False

    def compute_losses(self, batch, *, sync_metrics: bool = True, defer_logging: bool | str = False, profile_grad=None,
                       profile_log=None) -> dict:
        """``trainer.py:213-264``: every head's summed loss and ``...Mean``, batch and logits statistics.

        One encoder forward + ONE fused loss launch sequence produce all of it (the reference recomputes the
        logits eight times). ``loss/{train_loss}`` carries the gradient; the other heads are logging values.
        ``sync_metrics=False`` keeps the statistics on the device (no host sync in the step).
        ``defer_logging=True`` (implies device-side metrics; "auto": by the batch's size) runs the logging heads on a side
        stream; the non-train entries of the returned dict must then only be read after ``sync_logging()``.
        ``profile_grad`` / ``profile_log``: (start, stop) hipEvent_t handles recorded around the gradient-pass /
        logging-pass kernel of the loss (``bench.py``'s roofline figures).
        What the call decides is a :class:`~xfmr_rec_amd.step_plan.StepPlan` (kept as ``last_plan``); what it returns is
        ``step_plan.step_result``'s dict.
        """
        assert self.model is not None
        m, c = self.model, self.config
        dev = m.device
        hist = batch["history_item_idx"]
        lens = batch.get("lengths")
        tracing = torch.compiler.is_compiling()
        # what only a packed plan needs is asked only where one is possible: the lengths are on the HOST (the launch sizes
        # need the row count there: device-side lengths would cost a sync per step) and the step is not being traced (the
        # model's answer reads the environment)
        ask = lens is not None and not (torch.is_tensor(lens) and lens.is_cuda) and not tracing
        plan = self.last_plan = StepPlan.build(
            c, batch=hist.shape[0], width=hist.shape[1], max_seq_length=m.max_seq_length, has_lengths=ask,
            rows=(int(batch["packed_rows"]) if "packed_rows" in batch else int(lens.sum())) if ask else 0,
            supports_packed=ask and m.supports_packed_rows(min(hist.shape[1], m.max_seq_length)), tracing=tracing,
            capturing=ask and torch.cuda.is_current_stream_capturing(), defer_logging=defer_logging,
            grad=m.flat.requires_grad and torch.is_grad_enabled(), has_table_bf16=m.table_bf16 is not None)
        pos = batch["pos_item_idx"][:, -plan.L:].to(dev, torch.int64).contiguous()
        neg = None if plan.catalogue else batch["neg_item_idx"][:, -plan.L:].to(dev, torch.int64).contiguous()
        packed = None
        if plan.packed:
            packed = self._pack_rows(batch, plan, pos, neg)
            pos, neg = packed["pos"], packed["neg"]
        ws = self._overlap_workspaces(plan) if plan.overlap else None
        # (the forward records the event right after the launch that writes the key mask: xfmr_encoder_cfg.embed_event)
        tok, key_mask = m._encode_tokens(None if packed else hist, embed_event=self._ev_embed.cuda_event if plan.overlap else None,
                                         packed=packed)
        if m.config.is_normalized:  # models.py:393-394: the queries are the L2-normalised token embeddings
            tok = ops.l2_normalize(tok)
        assert packed is not None or tok.shape[1] == plan.L
        if plan.overlap:
            train_loss, losses, losses_train, stats = self._losses_overlapped(plan.opts, ws, tok, key_mask, pos, neg,
                                                                              profile_grad, profile_log)
        else:
            train_loss, losses, stats = ops.sampled_loss_train(
                tok, key_mask, pos, neg, m.embeddings, m.table_rnorm, plan.opts, table_bf16=m.table_bf16,
                profile_grad=profile_grad, profile_log=profile_log
            )
            losses_train = None
        return step_result(plan, train_loss, losses, losses_train, stats, sync=sync_metrics)

    def _pack_rows(self, batch, plan: StepPlan, pos, neg) -> dict:
        """The batch in the packed layout (``ops.pack_rows``'s dict, with the padded shape it came from)."""
        dev = self.model.device
        # the sequences go into the packed layout by length, LONGEST first (ops.length_order: nothing depends on the order
        # of a batch's rows -- every loss is a sum over them -- and the attention kernels start their longest workgroups
        # first); PinnedBatchRing ships the order and the offsets in that order with the batch
        offs64, order = batch.get("offsets"), batch.get("order")
        if offs64 is None:
            order, offs64 = ops.length_order(batch["lengths"])
            order, offs64 = order.to(dev), offs64.to(dev)
        packed = ops.pack_rows(batch["history_item_idx"].to(dev, torch.int64).contiguous(), pos, neg, offs64, plan.rows, order=order)
        return packed | {"batch": plan.batch, "seq_len": plan.L}

    def _overlap_workspaces(self, plan: StepPlan) -> tuple:
        """In front of the forward of an overlapped step: the two events (made once) and the two loss calls' workspaces,
        the logging pass's first."""
        m = self.model
        if self._ev_embed is None:
            self._ev_embed, self._ev_prep = torch.cuda.Event(), torch.cuda.Event()
            self._ev_embed.record()  # (creates the handle)
        H, n_rows = m.config.hidden_size, m.embeddings.shape[0]
        return (ops.sampled_loss_workspace(m.flat, plan.rows, H, n_rows, plan.opts),
                ops.sampled_loss_workspace(m.flat, plan.rows, H, n_rows, plan.opts))

    def _losses_overlapped(self, opts: ops.LossOpts, ws: tuple, tok, key_mask, pos, neg, profile_grad, profile_log) -> tuple:
        """The overlapped form: ``(train_loss, losses, losses_train, stats)`` of the logging pass on the side stream and
        the gradient pass on the main one."""
        m = self.model
        # The index-only half of both loss calls (query compaction, multiplicities, distinct negatives: 7 small launches
        # each) needs the key mask, not the token embeddings: it runs on the side stream underneath the forward, behind an
        # event the encoder forward records right after the launch that writes the mask -- instead of 40 us of small
        # launches between the forward's last kernel and the loss kernels.
        # The six logging heads + statistics do not feed the gradient: evaluate them on a side stream so the
        # (VALU-bound) logging pass runs underneath the (latency-bound) encoder backward. The caller joins
        # with sync_logging() before reading them (Trainer.fit_step / bench.py do, after optimizer.step()).
        main = torch.cuda.current_stream()
        side = self._side_stream()
        (ws_log, ws_grad), H, n_rows = ws, m.config.hidden_size, m.embeddings.shape[0]
        side.wait_event(self._ev_embed)  # the key mask exists (the forward is still running)
        with torch.cuda.stream(side):
            for w, heads in ((ws_log, 2), (ws_grad, False)):
                ops.sampled_loss_prepare(w, key_mask, pos, neg, m.table_rnorm, n_rows, H, opts.replace(all_heads=heads))
            d_tok0 = torch.zeros_like(tok)  # the gradient buffer, zeroed here instead of in front of the gradient pass
            self._ev_prep.record(side)
        # enqueued BEFORE the gradient pass: it needs the forward's output only, and at its lowest priority it takes
        # what the gradient pass (800 workgroups on 512 slots: 1.56 rounds) leaves idle, then the encoder backward's gaps
        side.wait_stream(main)
        with torch.cuda.stream(side):
            # all_heads=2: every head except the train head (its value comes from the launch below)
            losses, stats, _ = ops.sampled_loss(
                tok.detach(), key_mask, pos, neg, m.embeddings, m.table_rnorm, opts.replace(all_heads=2), need_grad=False,
                table_bf16=m.table_bf16, workspace=ws_log, prepared=True, profile_log=profile_log
            )
        main.wait_event(self._ev_prep)  # (recorded long ago)
        # stats_elsewhere: this call's statistics are dropped right here -- they are the logging call's above
        train_loss, losses_train, _ = ops.sampled_loss_train(
            tok, key_mask, pos, neg, m.embeddings, m.table_rnorm, opts.replace(all_heads=False), table_bf16=m.table_bf16,
            workspace=ws_grad, prepared=True, d_tok_zeroed=d_tok0, stats_elsewhere=True, profile_grad=profile_grad
        )
        for tns in (ws_log, ws_grad):
            tns.record_stream(side)
        d_tok0.record_stream(main)  # allocated on the side stream, used on the main one
        for tns in (tok, key_mask, pos, neg):
            if tns is not None:
                tns.record_stream(side)
        self._logging_pending = True
        return train_loss, losses, losses_train, stats

    def logged_values(self, out: dict) -> dict[str, float]:
        """Host-side view of a ``compute_losses`` result (``step_plan.host_values``): joins the side stream and returns
        every ``loss/<Class>``, ``loss/<Class>Mean``, ``batch/*`` and ``logits/*`` entry as floats (one device->host sync
        per vector), exactly the keys the reference logs (``trainer.py:241-263``)."""
        self.sync_logging()
        return host_values(out, self.config)

    # ------------------------------------------------------------------ validation path (trainer.py:186-325)
    @property
    def items_index(self):
        """Exact item index over the model's frozen table (the reference builds a LanceDB ANN index at
        ``on_validation_start``, ``trainer.py:316-325``; the table here never changes, so the index is a view)."""
        from .retrieval import ExactItemIndex

        assert self.model is not None and self.model.embeddings is not None
        idx = getattr(self, "_items_index", None)
        if idx is None or idx.table.data_ptr() != self.model.embeddings.data_ptr():
            idx = ExactItemIndex(self.model.embeddings, self.model.table_rnorm, table_bf16=self.model.table_bf16)
            self._items_index = idx
        return idx

    def _to_idx(self, item_ids) -> list[int]:
        """Item ids -> table rows; unknown ids are dropped (``models.py:347-364``). Integer inputs are rows already."""
        if len(item_ids) and not isinstance(item_ids[0], (str, bytes)):
            return [int(i) for i in item_ids]
        assert self.model.id2idx is not None, "configure_embeddings(items_dataset) provides the id -> row mapping"
        return E.lookup_rows(self.model.id2idx, item_ids)

    def _to_idx_or_empty(self, item_ids) -> list[int]:
        return self._to_idx(item_ids) if len(item_ids) else []

    @torch.no_grad()
    def recommend(self, item_ids, *, top_k: int = 0, exclude_item_ids=None):
        """``trainer.py:186-211``: nearest items to the pooled embedding of ``item_ids``, ``exclude_item_ids`` left
        out. Returns ``{"item_idx": (k,) int64 rows of the table (-1 = fewer than k left), "score": (k,)}``."""
        hist = self._to_idx(item_ids)
        emb = self.model(torch.as_tensor(hist, dtype=torch.int64, device=self.model.device)[None, :],
                         inference=not self.model.training)["sentence_embedding"]
        excl = None if exclude_item_ids is None else [self._to_idx(exclude_item_ids)]
        idx, score = self.items_index.search(emb, excl, top_k=top_k or self.config.top_k)
        return {"item_idx": idx[0], "score": score[0]}

    def predict_step(self, row):
        """``trainer.py:305-314``: recommendations for the row's history, the history itself excluded."""
        hist = list(row["history"]["item_id"])
        return self.recommend(hist, top_k=self.config.top_k, exclude_item_ids=hist)

    @torch.no_grad()
    def recommend_batch(self, item_ids_lists, *, top_k: int = 0, exclude_item_ids=None, search: str = "exact"):
        """:meth:`recommend` for many users in one pass: one batched encoder forward (``encode_batch``) and one
        xfmr_topk_tiled search. Returns ``{"item_idx": (B, k), "score": (B, k)}``; a history that is empty (also after
        unknown ids are dropped) gets all -1 / -inf. ``search="refined"`` takes the bf16 shortlist + exact re-rank
        (``ExactItemIndex.search_refined`` with ``exact=True``): the same bits."""
        hists = [self._to_idx_or_empty(list(x)) for x in item_ids_lists]
        excl = None if exclude_item_ids is None else [self._to_idx_or_empty(list(x)) for x in exclude_item_ids]
        return self._recommend_rows(hists, excl, top_k or self.config.top_k, search)

    def _recommend_rows(self, hists, excl, top_k: int, search: str = "exact"):
        """:meth:`recommend_batch` behind the id conversion: histories and exclusions are lists of table rows."""
        emb = self.model.encode_batch(hists)
        idx, score = self.items_index.search_rows(emb, excl, top_k=top_k, search=search)
        empty = [b for b, h in enumerate(hists) if not h]
        if empty:
            e = torch.as_tensor(empty, dtype=torch.int64, device=idx.device)
            idx.index_fill_(0, e, -1)
            score.index_fill_(0, e, float("-inf"))
        return {"item_idx": idx, "score": score}

    def predict_batch(self, rows):
        """:meth:`predict_step` for a list of rows: each row's history excluded from its recommendations."""
        hists = [list(r["history"]["item_id"]) for r in rows]
        return self.recommend_batch(hists, top_k=self.config.top_k, exclude_item_ids=hists)

    def open_sessions(self, n_slots: int, **encoder_kw):
        """A :class:`~xfmr_rec_amd.session.SessionRecommender` over this module's model and item index: sessions whose
        histories grow by one event at a time are served from cached K / V instead of being re-encoded at every call."""
        from .session import SessionRecommender

        return SessionRecommender(self, n_slots, **encoder_kw)

    @torch.no_grad()
    def evaluate(self, rows, stage: str = "val", batch_size: int = 1024, cutoffs=None) -> dict[str, float]:
        """The epoch means of the seven retrieval metrics over ``rows`` (the reference's format: ``{"history":
        {"item_id"}, "target": {"item_id", "label"}}``), batch_size rows per pass. Each mean is over the rows with at
        least one positive target and a non-empty history -- what Lightning logs from ``validation_step(...,
        batch_size=1)``, where a row without a target logs nothing (metrics.py:58-59) -- and
        ``{stage}/num_rows`` is their number.

        ``cutoffs`` (e.g. ``(5, 10, 20, 500)``): the rank path -- per pass ``encode_batch``, every target's exact rank
        over the whole catalogue (``ExactItemIndex.rank_targets``) and the metrics at every cutoff from the ranks. Adds
        ``{stage}/<metric>@<K>`` per cutoff; the plain keys are those of cutoff ``config.top_k`` (added when missing), which
        may then exceed 128.

        Every id is converted once (``eval_rows.read_rows``); the list pass then runs what :meth:`predict_batch` runs
        behind its id conversion (``_recommend_rows``), not :meth:`predict_batch` itself."""
        rows, bs = list(rows), max(1, int(batch_size))
        cut = None if cutoffs is None else E.eval_cutoffs(cutoffs, self.config.top_k)
        total = np.zeros(8 if cut is None else (len(cut), 8), dtype=np.float64)
        for b0 in range(0, len(rows), bs):
            hists, tgts = E.read_rows(rows[b0 : b0 + bs], self._to_idx_or_empty)
            total += self._list_pass(hists, tgts) if cut is None else self._rank_pass(hists, tgts, cut)
        return E.metrics_dict(stage, total, cut, int(self.config.top_k))

    def evaluate_sampled(self, rows, num_negatives: int = 100, seed: int = 0, cutoffs=None, stage: str = "val",
                         weights=None, batch_size: int = 1024) -> dict[str, float]:
        """:meth:`evaluate` under the sampled-candidate protocol: every row's targets are ranked among ``num_negatives``
        negatives drawn for the row (``eval_rows.sample_eval_negatives``: outside its history and targets, keyed by
        ``(seed, row)``, uniform or in proportion to ``weights``) instead of the catalogue. One
        :class:`~xfmr_rec_amd.evalset.SampledEvalSet` built from ``rows`` and evaluated once: its dict (``cutoffs``
        defaults to ``(config.top_k,)``)."""
        from .evalset import SampledEvalSet

        return SampledEvalSet.from_rows(self, rows, num_negatives=num_negatives, seed=seed, weights=weights,
                                        batch_size=batch_size).evaluate(stage, cutoffs=cutoffs)

    @torch.no_grad()
    def score_candidates(self, histories, candidate_item_ids) -> list:
        """Re-ranking: per history (a list of item ids), the given candidates best first -- ``(item_ids, scores)`` with
        the ids as given, ordered by score descending and then by table row, and their float32 scores (the bits
        :meth:`recommend_batch` reports for the item). One ``encode_batch`` and one ``ExactItemIndex.score_candidates``
        call. Unknown ids are dropped, as :meth:`recommend_batch` drops them, and a candidate given twice is scored once;
        an empty history gets ``([], no scores)``."""
        from .retrieval import _csr

        hists = [self._to_idx_or_empty(list(x)) for x in histories]
        given = [list(x) for x in candidate_item_ids]
        if len(given) != len(hists):
            raise ValueError(f"{len(given)} candidate lists for {len(hists)} histories")
        if not hists:
            return []
        # (table row, id as given) per known candidate: one lookup per id, so that a row's id can be handed back
        pairs = [[(r, i) for i in c for r in self._to_idx_or_empty([i])] if h else [] for h, c in zip(hists, given)]
        flat, off = E.candidates_csr([[r for r, _ in p] for p in pairs])
        dev = self.model.device
        emb = self.model.encode_batch(hists)
        score = self.items_index.score_candidates(emb, (torch.from_numpy(flat).to(dev), torch.from_numpy(off).to(dev)))
        score = score.cpu().numpy()
        out = []
        for b, p in enumerate(pairs):
            name = {}
            for row, item in p:
                name.setdefault(row, item)
            f, s = flat[off[b] : off[b + 1]], score[off[b] : off[b + 1]]
            order = np.lexsort((f, -s.astype(np.float64)))
            out.append(([name[int(x)] for x in f[order]], s[order]))
        return out

    def _evaluate_ranks(self, rows, stage: str, batch_size: int, cutoffs) -> dict[str, float]:
        """:meth:`evaluate` with ``cutoffs`` (kept under its earlier name)."""
        return self.evaluate(rows, stage, batch_size, cutoffs)

    def _list_pass(self, hists, tgts) -> np.ndarray:
        """One chunk through the ranked lists: the per-row values are read back and added here, in float64 and in row
        order, over the rows with a target and a history -> the 7 sums and the number of rows."""
        from .retrieval import retrieval_metrics

        recs = self._recommend_rows(hists, hists, self.config.top_k)["item_idx"]
        vals, valid = retrieval_metrics(recs, tgts, self.config.top_k)
        vals, valid = vals.cpu().numpy().astype(np.float64), valid.cpu().numpy()
        use = valid & np.asarray([bool(h) for h in hists])
        return np.append(vals[use].sum(axis=0), float(use.sum()))

    def _rank_pass(self, hists, tgts, cut) -> np.ndarray:
        """One chunk through the target ranks: ``(len(cut), 8)`` sums, formed on the device and read back."""
        from .retrieval import _csr, rank_metrics_sum

        dev = self.model.device
        emb = self.model.encode_batch(hists)
        excl = _csr(hists, dev, sort_unique=True)
        csr = _csr(tgts, dev)
        ranks = self.items_index.rank_targets(emb, csr, excl, n_targets=sum(len(t) for t in tgts))
        use = torch.from_numpy(np.asarray([bool(h) for h in hists], dtype=np.uint8)).to(dev)
        return rank_metrics_sum(ranks, csr, cut, use).cpu().numpy()

    def compute_metrics(self, row, stage: str = "val") -> dict[str, torch.Tensor]:
        """``trainer.py:266-286``: the seven retrieval metrics of one validation row under ``{stage}/<name>``."""
        from .retrieval import compute_retrieval_metrics

        recs = self.predict_step(row)
        tgt = self._to_idx(E.positive_target_ids(row))
        metrics = compute_retrieval_metrics(recs["item_idx"], tgt, top_k=self.config.top_k)
        return {f"{stage}/{k}": v for k, v in metrics.items()}

    def validation_step(self, row, batch_idx: int = 0):
        metrics = self.compute_metrics(row, stage="val")
        self.log_dict(metrics, batch_size=1)
        return metrics

    def test_step(self, row, batch_idx: int = 0):
        metrics = self.compute_metrics(row, stage="test")
        self.log_dict(metrics, batch_size=1)
        return metrics

    def training_step(self, batch, batch_idx: int = 0) -> torch.Tensor:
        """``trainer.py:288-291``. Runs the step the benchmark measures: metrics stay on the device (no host sync), the
        six logging heads + statistics go to the lowest-priority side stream underneath the backward. The train loss is
        logged here; everything else is logged by :meth:`on_train_batch_end` -- after the side stream has been joined --
        as 0-dim DEVICE tensors (Lightning's ``log_dict`` takes them and converts at its own logging interval)."""
        prof = self.profile_events or (None, None)  # bench.py: hipEvent pairs around the two loss passes
        # ("auto": the plan's rule, by the batch's size)
        out = self.compute_losses(batch, sync_metrics=False, defer_logging=self.defer_logging,
                                  profile_grad=prof[0], profile_log=prof[1])
        key = f"loss/{self.config.train_loss}"
        # only DETACHED tensors outlive the step: a retained train loss would keep the step's autograd graph -- the saved
        # activations and `flat`'s AccumulateGrad node with the stream it was created on -- alive into the next step (and
        # into a later hipGraph capture on another stream: ADVICE r3)
        self._pending_out = {k: (v.detach() if (torch.is_tensor(v) and v.requires_grad) else v) for k, v in out.items()}
        self.logged = {}
        self.log_dict({key: out[key].detach()})
        return out[key]

    def backward(self, loss: torch.Tensor, *args, **kwargs) -> None:
        """Lightning's ``LightningModule.backward`` hook (called by its automatic optimisation; ``Trainer.fit_step`` and
        ``bench.py`` call it too): ``loss.backward()`` with the persistent unit gradient -- no ones-fill launch, and the fused
        loss skips its multiply by 1 (ops.unit_grad)."""
        if loss.dim() == 0 and loss.is_cuda and not args and not kwargs:
            loss.backward(gradient=ops.unit_grad(loss))
        else:
            loss.backward(*args, **kwargs)

    def on_train_batch_end(self, outputs=None, batch=None, batch_idx: int = 0) -> None:
        """Lightning hook (after ``optimizer.step``): join the logging stream and log the step's remaining values."""
        out = self._pending_out
        if out is None:
            return
        self._pending_out = None
        self.last_out = out  # the step's raw device outputs (bench.py reads the statistics vector from it)
        self.sync_logging()
        self.log_dict(self.device_log_dict(out))

    def device_log_dict(self, out: dict) -> dict[str, torch.Tensor]:
        """Every key the reference logs (``trainer.py:241-263``, ``losses.py:392-404``) as 0-dim device tensors -- views
        of the kernels' output vectors, no host sync, no torch arithmetic (``step_plan.device_values``). Call after
        :meth:`sync_logging`. (``logits/{pos,neg}/*`` of an empty selection are NaN here where the reference omits the key.)"""
        return device_values(out, self.config)

    def log_dict(self, d, *a, **k):  # noqa: D401 - lightning API
        if _lp is not None and getattr(self, "_trainer", None) is not None:  # pragma: no cover
            return super().log_dict(d, *a, **k)
        # plain-module build: the step's values accumulate in `logged` (training_step starts a fresh dict)
        self.logged.update(d)
        return None

    def configure_optimizers(self) -> torch.optim.Optimizer:
        """``trainer.py:327-332`` with the fused kernel."""
        return FusedAdamW(self.parameters(), lr=self.config.learning_rate, weight_decay=self.config.weight_decay)

    @property
    def example_input_array(self):
        return (torch.as_tensor([[0], [1]], device=self._device()),)

    def state_dict(self, *args, **kwargs):
        """HF-keyed encoder tensors under the reference's prefix; the frozen table is omitted
        (``trainer.py:352-362``)."""
        sd = super().state_dict(*args, **kwargs)
        sd.pop("model.embeddings.weight", None)
        if self.model is not None:
            sd.pop("model.flat", None)
            for k, v in self.model.encoder_state_dict().items():
                sd[f"model.model.0.auto_model.{k}"] = v
        return sd

    _ENC_PREFIX = "model.model.0.auto_model."
    # tensors a reference checkpoint carries that this build has no use for (never trained on this path: SURVEY F12)
    _IGNORED_ENC_KEYS = ("embeddings.word_embeddings.weight", "embeddings.position_ids", "embeddings.token_type_ids",
                         "pooler.dense.weight", "pooler.dense.bias")

    def load_state_dict(self, state_dict, strict: bool = True, assign: bool = False):
        """Inverse of :meth:`state_dict`: HF-keyed encoder tensors under ``model.model.0.auto_model.`` -- this build's
        checkpoints and the reference's (``trainer.py:352-362`` only pops the table) -- go back into the flat buffer.
        Returns torch's ``(missing_keys, unexpected_keys)``; ``strict=True`` raises on either, as ``nn.Module`` does.
        Lightning resumes with ``strict_loading=False`` (``trainer.py:129``), i.e. ``strict=False``."""
        from torch.nn.modules.module import _IncompatibleKeys

        if self.model is None:
            self.configure_model()
        pre = self._ENC_PREFIX
        enc = {k[len(pre):]: v for k, v in state_dict.items() if k.startswith(pre)}
        views = self.model.encoder_state_dict()
        if "model.flat" in state_dict and not enc:  # a raw dump of the flat buffer
            flat = torch.as_tensor(state_dict["model.flat"])
            if flat.shape != self.model.flat.shape:
                raise RuntimeError(f"model.flat: shape {tuple(flat.shape)} != {tuple(self.model.flat.shape)}")
            with torch.no_grad():
                self.model.flat.copy_(flat.to(self.model.flat.device, torch.float32))
            enc = {k: None for k in views}
        missing = [pre + k for k in views if k not in enc]
        unexpected = [pre + k for k in enc if k not in views and k not in self._IGNORED_ENC_KEYS]
        unexpected += [k for k in state_dict if not k.startswith(pre) and k not in ("model.flat", "model.embeddings.weight")]
        bad_shape = [pre + k for k, v in enc.items() if k in views and v is not None
                     and tuple(torch.as_tensor(v).shape) != tuple(views[k].shape)]
        if bad_shape:
            raise RuntimeError(f"size mismatch for {bad_shape[:4]}")
        if strict and (missing or unexpected):
            raise RuntimeError(f"Error(s) in loading state_dict: missing keys {missing[:4]}{'...' if len(missing) > 4 else ''}, "
                               f"unexpected keys {unexpected[:4]}{'...' if len(unexpected) > 4 else ''}")
        self.model.load_encoder_state_dict({k: v for k, v in enc.items() if v is not None and k in views}, strict=False)
        if "model.embeddings.weight" in state_dict:  # a checkpoint that kept the table (not the reference's): install it
            self.model.set_table(torch.as_tensor(state_dict["model.embeddings.weight"]).to(self.model.device, torch.float32))
        return _IncompatibleKeys(missing, unexpected)

    def save(self, path) -> None:
        assert self.model is not None
        self.model.save(str(path))


# lr_scheduler class paths of a reference config (LightningCLI: {"class_path", "init_args"}) -> FusedAdamW schedule names
_REFERENCE_SCHEDULERS = {
    "get_constant_schedule": "constant",
    "get_constant_schedule_with_warmup": "warmup_constant",
    "get_linear_schedule_with_warmup": "warmup_linear",
    "get_cosine_schedule_with_warmup": "warmup_cosine",
}


def reference_trainer_options(cfg: dict) -> dict:
    """The :class:`Trainer` arguments a parsed reference ``config.yaml`` asks for (``Trainer.from_reference_config``)."""
    block = cfg.get("trainer") or {}
    if not isinstance(block, dict):
        raise ValueError(f"trainer: expected a mapping, got {type(block).__name__}")
    algo = block.get("gradient_clip_algorithm")
    if algo not in (None, "norm", "value"):
        raise ValueError(f"trainer.gradient_clip_algorithm: {algo!r} is not supported ('norm', 'value' or null)")
    clip = block.get("gradient_clip_val")
    if clip is not None and (isinstance(clip, bool) or not isinstance(clip, (int, float)) or not clip >= 0):
        raise ValueError(f"trainer.gradient_clip_val: {clip!r} is not a number >= 0")
    acc = block.get("accumulate_grad_batches")
    acc = 1 if acc is None else acc
    if isinstance(acc, bool) or not isinstance(acc, int) or acc < 1:
        raise ValueError(f"trainer.accumulate_grad_batches: {acc!r} is not an integer >= 1")
    if cfg.get("optimizer") is not None:  # (the module's configure_optimizers is AdamW, as the reference's)
        raise ValueError(f"optimizer: {cfg['optimizer']!r} cannot be honoured (the step is the module's fused AdamW)")
    sched = cfg.get("lr_scheduler")
    schedule = None
    if sched is not None:
        if not isinstance(sched, dict):
            raise ValueError(f"lr_scheduler: expected a mapping, got {sched!r}")
        if "class_path" in sched:
            name = _REFERENCE_SCHEDULERS.get(str(sched["class_path"]).rsplit(".", 1)[-1])
            if name is None:
                raise ValueError(f"lr_scheduler: class_path {sched['class_path']!r} is not supported (one of "
                                 f"transformers.optimization.{{{', '.join(_REFERENCE_SCHEDULERS)}}})")
            args = dict(sched.get("init_args") or {})
            schedule = {"name": name}
            if name != "constant":
                schedule["warmup_steps"] = args.pop("num_warmup_steps", 0)
            if name in ("warmup_linear", "warmup_cosine"):
                if "num_training_steps" not in args:
                    raise ValueError(f"lr_scheduler: {sched['class_path']} needs init_args.num_training_steps")
                schedule["total_steps"] = args.pop("num_training_steps")
            left = {k: v for k, v in args.items() if not (k == "last_epoch" and v == -1) and not (k == "num_cycles" and v == 0.5)}
            if left:
                raise ValueError(f"lr_scheduler: init_args {sorted(left)} cannot be honoured")
        else:
            schedule = dict(sched)
        try:
            ops._schedule_ids(schedule)
        except ValueError as e:
            raise ValueError(f"lr_scheduler: {e}") from None
    return dict(gradient_clip_val=clip, gradient_clip_algorithm=algo, accumulate_grad_batches=acc, lr_scheduler=schedule)


def reference_fit_options(cfg: dict) -> dict:
    """What a parsed reference ``config.yaml`` asks of the epoch loop: the ``trainer:`` block's ``max_epochs``,
    ``check_val_every_n_epoch``, ``limit_train_batches``, ``max_steps`` (-1 -> None) and ``val_check_interval`` --
    :meth:`Trainer.fit`'s arguments of the same names -- and ``batch_size``, ``max_seq_length`` and ``pos_lookahead`` of
    ``data.config`` (``DeviceSeqLoader`` / ``SeqDataConfig``). Lightning also takes fractions of an epoch for the two
    batch limits; the loop counts batches, so a float raises a ``ValueError`` that names the key."""
    block = cfg.get("trainer") or {}
    if not isinstance(block, dict):
        raise ValueError(f"trainer: expected a mapping, got {type(block).__name__}")

    def _count(key, default, least):
        v = block.get(key, default)
        v = default if v is None else v
        if v is not None and (isinstance(v, bool) or not isinstance(v, int) or v < least):
            raise ValueError(f"trainer.{key}: {v!r} is not an integer >= {least} (fractions of an epoch are not supported)")
        return v

    max_steps = block.get("max_steps", -1)
    max_steps = -1 if max_steps is None else max_steps
    if isinstance(max_steps, bool) or not isinstance(max_steps, int) or max_steps < -1:
        raise ValueError(f"trainer.max_steps: {max_steps!r} is not an integer >= -1")
    max_epochs = block.get("max_epochs")
    if max_epochs == -1 or (max_epochs is None and max_steps == -1):
        raise ValueError(f"trainer.max_epochs: {max_epochs!r} with max_steps = -1 asks for an endless loop")
    data = (cfg.get("data") or {}).get("config") or {}
    out = dict(max_epochs=_count("max_epochs", None, 0), check_val_every_n_epoch=_count("check_val_every_n_epoch", 1, 1),
               limit_train_batches=_count("limit_train_batches", None, 0), max_steps=None if max_steps == -1 else max_steps,
               val_check_interval=_count("val_check_interval", None, 1))
    for key, default in (("batch_size", 32), ("max_seq_length", 32), ("pos_lookahead", 0)):  # data.py:543-566
        v = data.get(key, default)
        if isinstance(v, bool) or not isinstance(v, int) or v < (0 if key == "pos_lookahead" else 1):
            raise ValueError(f"data.config.{key}: {v!r} is not a valid count")
        out[key] = v
    return out


class EarlyStopping:
    """Lightning's ``EarlyStopping`` rule on one monitored value: ``update(value)`` returns True when the loop should stop.

    A value improves when ``value - min_delta > best`` (mode "max"; ``value + min_delta < best`` for "min"); the first value
    always does. A value that does not improve (a NaN never does) adds one to ``wait``; the loop stops once
    ``wait >= patience``. ``patience=None`` never stops: the object then only tracks the best value. ``improved`` says
    whether the last value did."""

    def __init__(self, mode: str = "max", patience: int | None = 3, min_delta: float = 0.0):
        if mode not in ("max", "min"):
            raise ValueError(f"mode must be 'max' or 'min'; got {mode!r}")
        if patience is not None and (isinstance(patience, bool) or not isinstance(patience, int) or patience < 1):
            raise ValueError(f"patience must be an integer >= 1 (or None); got {patience!r}")
        if not float(min_delta) >= 0.0:
            raise ValueError(f"min_delta must be >= 0; got {min_delta!r}")
        self.mode, self.patience, self.min_delta = mode, patience, float(min_delta)
        self.best: float | None = None
        self.wait = 0
        self.improved = False

    def update(self, value: float) -> bool:
        v = float(value)
        if self.best is None:
            better = not math.isnan(v)
        elif self.mode == "max":
            better = v - self.min_delta > self.best
        else:
            better = v + self.min_delta < self.best
        self.improved = better
        if better:
            self.best, self.wait = v, 0
        else:
            self.wait += 1
        return self.patience is not None and self.wait >= self.patience

    def state_dict(self) -> dict:
        """What the rule has seen so far: ``best``, ``wait`` and ``improved``. The rule itself (mode, patience, min_delta) is
        the constructor's: a resumed run may change its patience."""
        return {"best": self.best, "wait": self.wait, "improved": self.improved}

    def load_state_dict(self, state: dict) -> None:
        self.best = None if state["best"] is None else float(state["best"])
        self.wait, self.improved = int(state["wait"]), bool(state["improved"])


def _early_stopping_from(arg, mode: str) -> EarlyStopping | None:
    """``Trainer.fit``'s ``early_stopping`` argument: None / False (off), True (Lightning's defaults: patience 3, min_delta 0)
    or ``{"patience", "min_delta"}``."""
    if arg is None or arg is False:
        return None
    if arg is True:
        return EarlyStopping(mode)
    if isinstance(arg, dict):
        extra = set(arg) - {"patience", "min_delta"}
        if extra:
            raise ValueError(f"early_stopping: unknown keys {sorted(extra)} ('patience', 'min_delta')")
        return EarlyStopping(mode, patience=arg.get("patience", 3), min_delta=arg.get("min_delta", 0.0))
    raise ValueError(f"early_stopping must be None, True or a dict; got {arg!r}")


class Trainer:
    """Minimal stand-in for Lightning's automatic optimisation (``zero_grad -> training_step -> backward ->
    [all-reduce] -> optimizer.step``), single process or one process per GPU (``torch.distributed``)."""

    def __init__(self, module: RecommenderLightningModule, *, world_size: int = 1, process_group=None,
                 gradient_clip_val: float | None = None, gradient_clip_algorithm: str | None = None,
                 accumulate_grad_batches: int = 1, lr_scheduler: dict | None = None):
        """``gradient_clip_val`` / ``gradient_clip_algorithm`` / ``accumulate_grad_batches``: Lightning's ``Trainer``
        arguments of the same names (algorithm None = "norm"; 0 or None = no clipping). ``lr_scheduler``: ``{"name",
        "warmup_steps", "total_steps"}`` (:class:`FusedAdamW`), stepped once per optimizer step. All of them act inside
        the optimizer's launches; with none set the step is what it is without them."""
        self.module = module
        module.configure_model()
        self.optimizer = module.configure_optimizers()
        self.world_size = world_size
        self.process_group = process_group
        self.exchange = None
        self.default_stream_steps = 0  # eager steps this trainer ran on the device's DEFAULT stream
        if gradient_clip_algorithm not in (None, "norm", "value"):
            raise ValueError(f"gradient_clip_algorithm must be 'norm', 'value' or None (= 'norm'); got {gradient_clip_algorithm!r}")
        if isinstance(accumulate_grad_batches, bool) or not isinstance(accumulate_grad_batches, int) or accumulate_grad_batches < 1:
            raise ValueError(f"accumulate_grad_batches must be an integer >= 1; got {accumulate_grad_batches!r}")
        if gradient_clip_val is not None and not float(gradient_clip_val) >= 0.0:
            raise ValueError(f"gradient_clip_val must be >= 0 or None; got {gradient_clip_val!r}")
        self.accumulate_grad_batches = accumulate_grad_batches
        self._micro = 0          # micro-batches accumulated since the last optimizer step
        self._grad_acc = None    # their gradient sum (accumulate_grad_batches > 1), persistent
        self._loop = None        # fit's loop state as of its last checkpoint or its end (state_dict)
        self._loader_fields = None  # identity of the DeviceSeqLoader the last fit / load_state_dict saw (None: an iterable)
        clip = float(gradient_clip_val) if gradient_clip_val else None  # (Lightning: 0 and None both mean "off")
        if clip is not None or lr_scheduler is not None:
            if not isinstance(self.optimizer, FusedAdamW):
                raise ValueError("gradient_clip_val / lr_scheduler act inside FusedAdamW's launches; configure_optimizers() "
                                 f"returned {type(self.optimizer).__name__}")
            ops.make_opt_cfg(lr=1.0, clip_mode=(gradient_clip_algorithm or "norm") if clip is not None else None,
                             clip_val=clip, schedule=lr_scheduler)  # (validates)
            if clip is not None:
                self.optimizer.clip_mode, self.optimizer.clip_val = gradient_clip_algorithm or "norm", clip
            self.optimizer.schedule = dict(lr_scheduler) if lr_scheduler is not None else None
        if accumulate_grad_batches > 1:
            for g in self.optimizer.param_groups:
                g["grad_scale"] = 1.0 / accumulate_grad_batches  # the optimizer sees the MEAN of the micro-batch gradients
        if world_size > 1:
            import os

            for g in self.optimizer.param_groups:
                # DDP averages gradients: SUM all-reduce then / W (times 1 / k for k accumulated micro-batches)
                g["grad_scale"] = 1.0 / (world_size * accumulate_grad_batches)
            # One message behind the backward by default. XFMR_ALLREDUCE_HALVES=1: two halves, the upper layers' underneath
            # the lower layers' backward (distributed.HalvedAllReduce) -- its event ordering is tested on one GPU
            # (tests/test_gpu_ddp.py), but RCCL's transport has never run under it (no multi-GPU box was available to the
            # build: DESIGN.md section 6), so it stays opt-in until a scaling record exists.
            if os.environ.get("XFMR_ALLREDUCE_HALVES", "0") == "1" and os.environ.get("XFMR_ALLREDUCE_SINGLE", "0") != "1":
                from .distributed import HalvedAllReduce

                if accumulate_grad_batches > 1:
                    raise ValueError("XFMR_ALLREDUCE_HALVES=1 exchanges halves of the backward's own buffer underneath the "
                                     "backward; accumulate_grad_batches > 1 exchanges the accumulated sum once instead")
                self.exchange = HalvedAllReduce(module.model, process_group)
            elif os.environ.get("XFMR_ALLREDUCE", "") == "abi" and module.model.flat.is_cuda:
                # the exchange through the C ABI (xfmr_allreduce_flat: RCCL underneath, no torch collective in the step)
                from .distributed import AbiAllReduce

                self.exchange = AbiAllReduce(module.model.device, process_group)

    def allreduce_(self, flat_grad: torch.Tensor) -> None:
        """The step's one exchange: SUM of the flat gradient over the ranks (1 / W is folded into AdamW); with
        XFMR_ALLREDUCE_HALVES=1 in two halves, the upper layers' underneath the rest of the backward."""
        if self.world_size <= 1:
            return
        if self.exchange is not None:
            self.exchange.reduce_(flat_grad)
        else:
            from .distributed import allreduce_flat_grad_

            allreduce_flat_grad_(flat_grad, self.process_group)

    def fit_step(self, batch) -> torch.Tensor:
        """One step through the module's Lightning seam, in Lightning's order (``zero_grad -> training_step -> backward
        -> [all-reduce] -> optimizer.step -> on_train_batch_end``): what ``bench.py`` times."""
        m = self.module
        m.train()
        dev = m.model.device
        if dev.type == "cuda" and not torch.cuda.is_current_stream_capturing() \
                and torch.cuda.current_stream(dev) == torch.cuda.default_stream(dev):
            self.default_stream_steps += 1  # (a later hipGraph capture refuses: GraphedStep)
        self.optimizer.zero_grad(set_to_none=True)
        loss = m.training_step(batch, 0)
        m.backward(loss)
        k = self.accumulate_grad_batches
        if k > 1:
            # one call = one micro-batch: its gradient joins the persistent sum; the k-th call exchanges the sum once and
            # steps on it (grad_scale = 1 / (W k)). Calls 1 .. k-1 leave parameters, moments and step count alone.
            flat = m.model.flat
            if self._grad_acc is None:
                self._grad_acc = torch.empty_like(flat.grad)
            ops.grad_accumulate_(self._grad_acc, flat.grad.contiguous(), first=self._micro == 0)
            self._micro += 1
            if self._micro < k:
                m.on_train_batch_end(loss, batch, 0)
                return loss.detach()
            self._micro = 0
            flat.grad = self._grad_acc  # (what the optimizer reads; the next zero_grad drops the reference, not the buffer)
        self.allreduce_(m.model.flat.grad)
        self.optimizer.step()
        if getattr(self.optimizer, "has_options", False):
            m.log_dict(self.optimizer.ctl_log_dict())  # grad/norm, grad/clip_coef, lr: device views, no host sync
        m.on_train_batch_end(loss, batch, 0)  # joins the logging stream (leaving the pass to finish underneath the next
        return loss.detach()                  # step's forward measured no gain: 3.411 vs 3.414 ms)

    @classmethod
    def from_reference_config(cls, module: RecommenderLightningModule, cfg: dict, **kwargs) -> "Trainer":
        """A trainer from a parsed reference ``config.yaml``: its ``trainer:`` block's ``gradient_clip_val``,
        ``gradient_clip_algorithm`` and ``accumulate_grad_batches`` and the top-level ``lr_scheduler``. The block's other
        keys are orchestration (devices, logging, checkpointing: the caller's; the epoch loop's keys are read by
        :func:`reference_fit_options` for :meth:`fit`) and are not read here. A non-null
        value that changes the optimisation and cannot be honoured raises a ``ValueError`` that names its key."""
        return cls(module, **reference_trainer_options(cfg), **kwargs)

    def _check_val(self, val) -> None:
        """The validation set's world is the trainer's: its ``world_size`` (1 for anything that does not say) equals this
        trainer's, and under ``world_size > 1`` its ``rank`` is this process's rank in ``process_group``."""
        if val is None:
            return
        import torch.distributed as dist

        val_world = getattr(val, "world_size", 1)
        if val_world != self.world_size:
            raise ValueError(f"the validation set is sharded over world_size = {val_world!r}, this trainer runs world_size = "
                             f"{self.world_size}: build it with DeviceEvalSet.from_rows(..., rank=, world_size=, "
                             "process_group=) of this run")
        if self.world_size > 1:
            rank = dist.get_rank(self.process_group) if dist.is_available() and dist.is_initialized() else 0
            if getattr(val, "rank", None) != rank:
                raise ValueError(f"the validation set holds the shard of rank {getattr(val, 'rank', None)!r}, this process is "
                                 f"rank {rank} of world_size = {self.world_size}")

    def validate(self, val, stage: str = "val", cutoffs=None) -> dict:
        """One validation pass over ``val`` (a :class:`~xfmr_rec_amd.evalset.DeviceEvalSet`) outside ``fit``: the dict of
        ``DeviceEvalSet.evaluate``, also handed to ``module.log_dict``. ``cutoffs``: the rank path, with the
        ``<metric>@<K>`` keys (``DeviceEvalSet.evaluate(stage, cutoffs=...)``). Under ``world_size > 1`` ``val`` is this
        rank's sharded set, the call is collective (every rank makes it) and every rank gets the same dict."""
        self._check_val(val)
        metrics = val.evaluate(stage) if cutoffs is None else val.evaluate(stage, cutoffs=cutoffs)
        self.module.log_dict(metrics)
        return metrics

    # ------------------------------------------------------------------ full-state checkpoints
    def _trainer_fields(self) -> dict:
        opt = self.optimizer
        return {"accumulate_grad_batches": self.accumulate_grad_batches,
                "gradient_clip_algorithm": getattr(opt, "clip_mode", None), "gradient_clip_val": getattr(opt, "clip_val", None),
                "lr_scheduler": getattr(opt, "schedule", None), "world_size": self.world_size}

    def _optimizer_steps(self) -> int:
        return int(max((st.get("step", 0) for st in self.optimizer.state.values()), default=0))

    def _seed_device_step(self) -> None:
        """The step counter the captured kernels read (dropout stream, AdamW's bias corrections) lives in HBM from here
        on: a new one continues the optimizer's completed steps, so that the eager steps in front of a capture and the
        replays after it are one sequence."""
        mdl = self.module.model
        if getattr(mdl, "step_device", None) is None:
            mdl.use_device_step(True)
            mdl.step_device.fill_(self._optimizer_steps())
        self.optimizer.step_device = mdl.step_device

    @staticmethod
    def _empty_loop() -> dict:
        return {"batches_done": 0, "epoch": 0, "next_batch": 0, "tracker": None, "stopper": None, "val_history": [],
                "best_score": None, "best_step": None, "best_model_path": None, "train_seconds": 0.0}

    def state_dict(self, loader=None) -> dict:
        """Everything a run needs to go on as if it had not stopped (``checkpoint.py`` lists the keys): the module's weights
        under the reference's keys, the optimizer's moments and step count, the dropout stream's position and whether it
        is keyed on the device, the options that shape the optimisation, ``fit``'s loop state as of its last checkpoint
        or its end, and the identity of ``loader`` (the :class:`~xfmr_rec_amd.data.DeviceSeqLoader` the run reads; by
        default the one the last ``fit`` or ``load_state_dict`` saw, None for a plain iterable). Tensors are host copies: one stream sync, then the device-to-host copies. Refused between the
        micro-batches of one optimizer step (``accumulate_grad_batches > 1``): the gradient sum is not part of it."""
        from . import checkpoint as CK

        if self._micro != 0:
            raise ValueError(f"a checkpoint between the micro-batches of one optimizer step ({self._micro} of "
                             f"accumulate_grad_batches = {self.accumulate_grad_batches} done) is refused: the gradient sum is "
                             "not part of a checkpoint")
        m, mdl = self.module, self.module.model
        if mdl.flat.is_cuda:
            torch.cuda.current_stream(mdl.device).synchronize()
        optimizer = CK.plain(self.optimizer.state_dict(), "optimizer")  # (FusedAdamW reads its device-side step count first)
        host = mdl.flat.detach().cpu()  # ONE copy: the HF-keyed tensors of the file are views of it (one storage in the file)
        sd = {}
        offsets = {CK.ENC_PREFIX + name: (off, shape) for name, shape, off in zip(mdl._names, mdl._shapes, mdl._offsets)}
        for k, v in m.state_dict().items():
            if k in offsets:
                off, shape = offsets[k]
                sd[k] = host[off : off + v.numel()].view(shape)
            else:
                sd[k] = v.detach().cpu()
        loop = dict(self._loop) if self._loop is not None else self._empty_loop()
        return {
            "format": CK.FORMAT, "version": CK.VERSION, "state_dict": sd,
            "hyper_parameters": {"config": CK.plain(m.config.model_dump(), "config")},
            "epoch": loop["epoch"], "global_step": self._optimizer_steps(), "optimizer": optimizer,
            "model": {"dropout_step": int(mdl._step), "seed": int(mdl._seed),
                      "device_step": getattr(mdl, "step_device", None) is not None},
            "trainer": CK.plain(self._trainer_fields(), "trainer"), "loop": CK.plain(loop, "loop"),
            "loader": CK.loader_fields(loader) if loader is not None else self._loader_fields,
        }

    def load_state_dict(self, state: dict, loader=None) -> dict:
        """Inverse of :meth:`state_dict`. Compatibility is checked before anything is touched
        (``checkpoint.check_compatible``: a ``ValueError`` that names the field); then, in this order: module weights,
        optimizer state, the dropout stream's position and seed, and the device-step mode -- a checkpoint taken with the
        step counter on the device gets one again, filled with the restored step count and wired to the optimizer; one
        taken without leaves it off. ``loader`` is positioned at the batch the run goes on with. Returns the ``loop``
        state, which a later :meth:`fit` continues only when it is given the file (``ckpt_path``)."""
        from . import checkpoint as CK

        m, mdl = self.module, self.module.model
        CK.check_compatible(state, flat_numel=mdl.flat.numel(), trainer=self._trainer_fields(), loader=CK.loader_fields(loader))
        keys = m.load_state_dict(state["state_dict"], strict=False)
        if keys.missing_keys:
            raise ValueError(f"checkpoint state_dict: missing keys {keys.missing_keys[:4]}")
        opt_state = {"state": state["optimizer"]["state"],
                     "param_groups": [{k: (tuple(v) if k == "betas" else v) for k, v in g.items()}
                                      for g in state["optimizer"]["param_groups"]]}
        self.optimizer.load_state_dict(opt_state)
        mdl._step, mdl._seed = int(state["model"]["dropout_step"]), int(state["model"]["seed"])
        if state["model"]["device_step"] and getattr(mdl, "step_device", None) is None:
            mdl.use_device_step(True)
        if getattr(mdl, "step_device", None) is not None:
            mdl.step_device.fill_(self._optimizer_steps())
            self.optimizer.step_device = mdl.step_device
        self._micro = 0
        loop = {**self._empty_loop(), **state["loop"]}
        self._loop, self._loader_fields = dict(loop), CK.loader_fields(loader)
        self.val_history = [dict(h) for h in loop["val_history"]]
        self.best_score, self.best_step, self.best_model_path = loop["best_score"], loop["best_step"], loop["best_model_path"]
        if loader is not None and CK.loader_fields(loader) is not None:
            loader.load_state_dict({"epoch": loop["epoch"], "next_batch": loop["next_batch"]})
        return loop

    def save_checkpoint(self, path, loader=None) -> int:
        """:meth:`state_dict` written to ``path`` (``checkpoint.write_checkpoint``: a temporary name, fsync, then
        ``os.replace``). Synchronous, on the calling thread. Returns the file's size in bytes."""
        from . import checkpoint as CK

        return CK.write_checkpoint(self.state_dict(loader), path)

    def load_checkpoint(self, path, loader=None) -> dict:
        """``checkpoint.read_checkpoint(path)`` into :meth:`load_state_dict`; returns the restored ``loop`` state."""
        from . import checkpoint as CK

        return self.load_state_dict(CK.read_checkpoint(path), loader=loader)

    def fit(self, batches, max_steps: int | None = None, *, ring_slots: int = 6, graph: str = "off",
            graph_probe_steps: int = 20, val=None, val_check_interval: int | None = None, monitor: dict = METRIC,
            early_stopping=None, checkpoint_dir=None, val_cutoffs=None, max_epochs: int | None = None,
            check_val_every_n_epoch: int = 1, limit_train_batches: int | None = None, ckpt_path=None,
            save_last: bool = False, checkpoint_every_n_steps: int | None = None, max_time=None) -> list[float]:
        """Steps over an iterable of collated batches. Batches that arrive in HOST memory (the reference's DataLoader
        output, ``data.py:915-927``) are handed over through a :class:`~xfmr_rec_amd.data.PinnedBatchRing`: the copy of
        batch i + 1 runs underneath step i; device-resident batches (``DeviceSeqDataset.sample_batch``) are used as they are.

        ``graph``: "off" -- every step is enqueued launch by launch; "on" -- after three eager steps (they create every
        lazily made object) the step is captured once as a hipGraph (:class:`GraphedStep`) and replayed for every batch
        of the captured shape; "auto" -- ``graph_probe_steps`` eager steps are timed, then as many replays, and the faster
        form runs the rest (replay wins where the host's launch rate bounds the step -- BASELINE config 1's shape: 0.31
        against 0.48 ms -- and changes nothing where the GPU does: DESIGN.md section 5). Every probe step is a real
        training step on its own batch. Batches of another shape (a short last batch) take the eager step. Single
        process only; ``self.graph_choice`` records what ran. What the call changes for its duration (the current stream,
        ``module.defer_logging``, a loader's ``fixed_width``) is put back, and the optimizer's host-side step count brought
        up to the device's, when it raises, too.

        ``val`` (a :class:`~xfmr_rec_amd.evalset.DeviceEvalSet`): validate inside the loop, as Lightning does with the
        reference's ``ModelCheckpoint`` + ``EarlyStopping`` on ``val/retrieval_normalized_dcg`` (``trainer.py:334-341``).
        ``val_check_interval=n``: a pass after every n-th batch (a multiple of ``accumulate_grad_batches``); None: one pass
        after the last batch. A pass runs between steps on the loop's stream, never inside a capture (under ``graph`` it is
        enqueued eagerly between replays) and its time is taken out of the "auto" probe's windows. ``monitor``: ``{"name",
        "mode"}``. ``early_stopping``: None, True (patience 3, min_delta 0) or ``{"patience", "min_delta"}``
        (:class:`EarlyStopping`). ``checkpoint_dir``: every strict improvement of the monitor overwrites
        ``checkpoint_dir / "best"`` with ``module.save`` (``ModelCheckpoint(save_top_k=1)``; ``RecommenderModel.load`` reads
        it). Afterwards: ``val_history`` (``{"step": batches done, **metrics}`` per pass), ``best_score``, ``best_step``,
        ``best_model_path``, ``stopped_early`` and ``val_elapsed`` (seconds in validation passes: a host clock from a
        stream sync in front of the pass to its read-back).

        Under ``world_size > 1`` ``val`` is this rank's SHARDED set (``DeviceEvalSet.from_rows(..., rank=, world_size=,
        process_group=)`` of this run; anything else is a ``ValueError``). Every rank runs the pass on its own rows and
        its one exchange; the metrics are over all global rows and the same bits on every rank, so the best tracker,
        the early-stopping rule, ``val_history``, ``best_score``, ``best_step`` and ``stopped_early`` are the same
        everywhere and all ranks leave the loop after the same batch -- no decision is broadcast, and no rank is left
        waiting in a gradient all-reduce. ``checkpoint_dir / "best"`` is written by rank 0 only, a barrier follows, and
        ``best_model_path`` is set on every rank.

        ``val_cutoffs`` (e.g. ``(5, 10, 20, 500)``): every pass takes the rank path (``DeviceEvalSet.evaluate(stage,
        cutoffs=val_cutoffs)``): the metrics at every cutoff under ``<stage>/<metric>@<K>`` next to the plain keys (those
        of ``config.top_k``), all of them in ``val_history``. ``monitor["name"]`` may then be ``'<stage>/<metric>@<K>'`` for
        a K among ``val_cutoffs``.

        ``max_epochs`` (``batches`` must then be a :class:`~xfmr_rec_amd.data.DeviceSeqLoader`, built with this trainer's
        ``world_size``): the epoch loop of the reference's ``trainer:`` block (:func:`reference_fit_options`). Epoch e is
        ``loader.set_epoch(e)`` and one iteration of the loader, at most ``limit_train_batches`` batches of it; ``max_steps``
        still caps the total, and the returned list holds every step's loss across the epochs. With ``val`` and no
        ``val_check_interval`` a pass follows every ``check_val_every_n_epoch``-th epoch (Lightning's default; nothing
        extra after the last batch); ``val_check_interval`` counts batches across epochs as before. ``val_history``
        entries carry the ``"epoch"`` they ran in. Under ``graph != "off"`` the loader runs ``fixed_width`` for the call
        and its batches are taken without their lengths: eager warm-up, probe and replays are one layout; the sample
        launch itself stays outside the captured graph. A loader that was restored mid-epoch (``load_state_dict``)
        continues there.

        ``ckpt_path``: a file of :meth:`save_checkpoint`, loaded before the loop (:meth:`load_checkpoint` with this call's
        loader: an incompatible trainer or loader is a ``ValueError``). The loop's counters continue: ``val_check_interval``
        and ``check_val_every_n_epoch`` fall on the global batch numbers of the uninterrupted run, ``max_steps`` and
        ``max_epochs`` cap the totals including the restored part (Lightning's meaning), ``val_history``, the best tracker
        and the early-stopping rule start from their restored state. The returned list holds this call's losses only. The
        resumed steps are the uninterrupted run's, bit for bit (tests/test_gpu_resume.py). A loader is put at the restored
        position (the loop's own, not the loader's, which is a batch ahead); with a plain iterable the caller supplies the
        batches from ``loop["batches_done"]`` on. ``checkpoint_every_n_steps=n`` (a multiple of
        ``accumulate_grad_batches``; needs ``checkpoint_dir``): after every n-th global batch -- behind a validation pass
        that falls on it, so that the file carries the pass -- ``checkpoint_dir / "last.ckpt"`` is rewritten.
        ``save_last=True``: the same file is written when the loop ends, whatever ended it (not when it raises). A write is
        synchronous, between two steps on the loop's stream, never inside a capture and on no other thread; its time
        goes into ``ckpt_elapsed`` and out of the "auto" probe's windows.

        ``max_time`` (``checkpoint.parse_max_time``: seconds, a ``timedelta``, ``"DD:HH:MM:SS"`` or a dict): the budget of
        THIS call on the host's monotonic clock, from its start. It is looked at after each batch, without a device
        sync; once it is spent the loop ends, ``stopped_on_time`` is True and ``save_last`` applies. A limit <= 0 still
        runs one batch. This deviates from Lightning, whose ``Timer`` carries the elapsed time across a resume: there, a
        run stopped on time and resumed with the same limit stops after one batch; here the resumed call has the whole
        budget again. None of the four is supported under ``world_size > 1`` (validation, early stopping and the best
        model are: above; full-state checkpoints and a host-clock limit inside a data-parallel loop are not)."""
        from . import checkpoint as CK
        from . import fit_loop
        from .data import DeviceSeqLoader

        t_fit = time.monotonic()
        self._check_val(val)
        loader = batches if isinstance(batches, DeviceSeqLoader) else None
        plan = fit_loop.FitPlan.build(
            batches, loader, world_size=self.world_size, accumulate_grad_batches=self.accumulate_grad_batches,
            max_steps=max_steps, ring_slots=ring_slots, graph=graph, graph_probe_steps=graph_probe_steps, val=val,
            val_check_interval=val_check_interval, monitor=monitor, early_stopping=early_stopping,
            checkpoint_dir=checkpoint_dir, val_cutoffs=val_cutoffs, max_epochs=max_epochs,
            check_val_every_n_epoch=check_val_every_n_epoch, limit_train_batches=limit_train_batches, ckpt_path=ckpt_path,
            save_last=save_last, checkpoint_every_n_steps=checkpoint_every_n_steps, max_time=max_time)
        self.val_history: list[dict] = []
        self.best_score = self.best_step = self.best_model_path = None
        self.stopped_early = self.stopped_on_time = False
        self.val_elapsed = self.ckpt_elapsed = 0.0
        self._loader_fields = CK.loader_fields(loader)
        # (load_checkpoint checks compatibility first; it sets val_history and the best_* fields)
        loop = self.load_checkpoint(ckpt_path, loader=loader) if ckpt_path is not None else None
        return fit_loop.FitRun(self, plan, batches, loader, val, loop, t_fit).run()


_NO_ACCUMULATED_CAPTURE = ("a captured step cannot accumulate micro-batches (accumulate_grad_batches > 1): the device-side step "
                           "counter advances once per OPTIMIZER step, so the micro-batches of one step would share their "
                           "dropout masks; run accumulated steps eagerly (graph='off')")


def _refuse_capture_after_default_stream_steps(trainer: "Trainer") -> None:
    """torch's capture protocol: autograd's AccumulateGrad node of a parameter is bound to the stream of the first backward
    that used it and synchronises with that stream from then on; eager steps on the device's DEFAULT (legacy) stream
    followed by a capture on a side stream made the capture fault (scripts/probe/fit_graph_probe.py, round 3). A clear
    Python error instead of that fault."""
    if getattr(trainer, "default_stream_steps", 0) > 0:
        raise RuntimeError(
            f"this Trainer has run {trainer.default_stream_steps} eager step(s) on the device's default stream; a hipGraph "
            "capture after that is refused (torch's capture protocol: warm-up steps must run on a side stream -- "
            "`with torch.cuda.stream(torch.cuda.Stream()): trainer.fit_step(...)`, or let Trainer.fit(graph=...) / "
            "GraphedStep(warmup=...) run them). Build a new Trainer for the captured run.")


class GraphedStep:
    """One training step of ``trainer`` (``Trainer.fit_step``: zero_grad -> training_step -> backward -> AdamW ->
    on_train_batch_end) captured ONCE as a hipGraph for a fixed batch shape and replayed per step: the ~80 kernel
    launches of a step become one graph launch. For small batches the eager step is bound by the host's launch rate,
    not by the GPU (batch 32 at config 2: 0.84 ms per step against 0.8-0.95 ms of enqueueing).

    What changes from step to step is read from DEVICE memory inside the captured kernels -- the dropout stream
    (``xfmr_encoder_cfg.step_device``) and AdamW's step count (``xfmr_adamw_dev``), both the model's ``step_device``
    counter, advanced by the step's last launch (``xfmr_step_advance``) -- so every replay draws new masks and applies the
    right bias corrections: replay == the eager step with the same counter, bit for bit (tests/test_gpu_graph.py).

        step = GraphedStep(trainer, example_batch)     # device tensors of the shape every batch will have
        loss = step(batch)                             # copies the indices into the captured buffers, replays

    Single process only (the all-reduce of a data-parallel step is not captured here). The eager steps in front of the
    capture must NOT have run on the default stream (torch's capture protocol; the capture faults otherwise:
    scripts/probe/fit_graph_probe.py) -- the warm-up here and ``Trainer.fit(graph=...)`` both use a side stream."""

    def __init__(self, trainer: Trainer, example_batch: dict, warmup: int = 3, overlap: bool = False):
        """``overlap=True`` captures the step with its two forks at ANY size -- the weight-gradient GEMMs on the context's
        side stream (``XFMR_ENC_DW_SIDE_ANY``) and the logging heads on the logging stream (``defer_logging``) -- as
        branches of the graph. Same bits (tests/test_gpu_graph.py), but on this runtime (ROCm 7.2 / torch 2.10) a graph
        with cross-stream branches replays 2-3x SLOWER than the single-stream capture (config 2 at batch 32: 2.07 ms
        against 0.85; H 64 / L 50 / batch 64: 1.39 against 0.31), so the default is the single-stream step."""
        from .data import SEQ_BATCH_KEYS

        m = trainer.module
        if trainer.world_size != 1:
            raise ValueError("GraphedStep captures a single-process step")
        if getattr(trainer, "accumulate_grad_batches", 1) > 1:
            raise ValueError(_NO_ACCUMULATED_CAPTURE)
        _refuse_capture_after_default_stream_steps(trainer)
        self.trainer, self.keys = trainer, SEQ_BATCH_KEYS
        dev = m.model.device
        if overlap:
            m.model.enc_flags = getattr(m.model, "enc_flags", 0) | N.ENC_DW_SIDE_ANY
            m.defer_logging = True
        elif m.defer_logging == "auto":
            m.defer_logging = False  # one stream inside the capture
        trainer._seed_device_step()
        m.train()
        m._pending_out = None  # nothing of an earlier step (its tensors, their autograd graph) reaches into the capture
        m.last_out = None
        self.static = {k: example_batch[k].to(dev, torch.int64).clone() for k in self.keys}
        # eager warm-up on a side stream (torch's capture protocol): creates every lazily made object -- optimizer state,
        # the model's xfmr_context, allocator pools -- so that the capture itself creates nothing. ``warmup=0``: the caller
        # has already run eager steps of this shape (Trainer.fit does, on real batches).
        if warmup > 0:
            side = torch.cuda.Stream(device=dev)
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(warmup):
                    trainer.fit_step(self.static)
            torch.cuda.current_stream().wait_stream(side)
        trainer.optimizer.zero_grad(set_to_none=True)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.loss = trainer.fit_step(self.static)
        self.logged = dict(m.logged)  # 0-dim device tensors inside the graph's pool: refreshed by every replay

    def matches(self, batch: dict) -> bool:
        """Whether ``batch`` has the captured shape (a replay needs it)."""
        return all(tuple(batch[k].shape) == tuple(self.static[k].shape) for k in self.keys)

    def __call__(self, batch: dict) -> torch.Tensor:
        for k in self.keys:
            self.static[k].copy_(batch[k], non_blocking=True)
        self.graph.replay()
        return self.loss
