"""A validation set prepared ONCE and kept in HBM (a peer of ``data.DeviceSeqDataset`` for the validation path).

``RecommenderLightningModule.evaluate(rows)`` redoes, on every call, host work that depends on the rows only and never on
the model: id -> row conversion, truncation, padding, the length order, the packed layout behind an upload, one
``np.unique`` per user for the exclusions, the targets CSR, and a read-back + host sum per pass (profiles/eval_batched.md:
0.18-0.29 s for 6 040 users, host-bound). Here all of that is :func:`plan_eval_rows` (numpy, once) + one upload;
a pass is then the packed forward, one pooling launch and one tiled top-k per chunk, ONE ``xfmr_retrieval_metrics_sum``
over all rows, and a 64-byte read-back. ``Trainer.fit(val=...)`` runs it between steps.
"""

from __future__ import annotations

import dataclasses

import numpy as np
import torch

from . import _native as N
from . import ops
from .retrieval import METRIC_NAMES, METRICS, normalize_cutoffs, rank_metrics_sum, retrieval_metrics_sum


@dataclasses.dataclass
class EvalChunk:
    """``batch_size`` consecutive rows of the plan: rows [row0, row1), their tokens [tok0, tok1) of the flat encoder input,
    the chunk's own ``seq_offsets`` (int32, starting at 0), ``packed_rows`` = tok1 - tok0 and its longest length."""

    row0: int
    row1: int
    tok0: int
    tok1: int
    seq_offsets: np.ndarray
    packed_rows: int
    max_len: int


@dataclasses.dataclass
class EvalPlan:
    """What :func:`plan_eval_rows` returns; every array is numpy, rows are in PLAN order (longest history first)."""

    kept: np.ndarray         # (n,) int64: plan row i is input row kept[i]
    lengths: np.ndarray      # (n,) int64: truncated history lengths, non-increasing
    hist: np.ndarray         # (tokens,) int64: each history's last max_seq_length rows, back to back
    row_pos: np.ndarray      # (tokens,) int32: 0 .. len - 1 within each sequence
    tok_offsets: np.ndarray  # (n + 1,) int64: cumulative lengths
    chunks: list             # [EvalChunk]
    excl: np.ndarray         # exclusions CSR: each row's WHOLE history, sorted ascending, unique
    excl_offsets: np.ndarray  # (n + 1,) int64, absolute: a chunk is excl_offsets[row0 : row1 + 1] over the one flat array
    targets: np.ndarray      # targets CSR: the positive target indices as given
    target_offsets: np.ndarray  # (n + 1,) int64, absolute
    max_seq_length: int
    batch_size: int


def _flat(lists, rows) -> tuple[np.ndarray, np.ndarray]:
    lens = np.asarray([len(lists[r]) for r in rows], dtype=np.int64)
    off = np.zeros(len(rows) + 1, dtype=np.int64)
    np.cumsum(lens, out=off[1:])
    parts = [np.asarray(lists[r], dtype=np.int64).reshape(-1) for r in rows]
    flat = np.concatenate(parts) if off[-1] else np.zeros(0, dtype=np.int64)
    return flat, off


def plan_eval_rows(hist_idx_lists, target_idx_lists, max_seq_length: int, batch_size: int) -> EvalPlan:
    """The model-independent half of a validation pass, in numpy (no device).

    ``hist_idx_lists`` / ``target_idx_lists``: per input row, the history and the POSITIVE targets as table rows (unknown
    ids already dropped). A row counts when its history is non-empty and it has at least one positive target -- the rows
    ``RecommenderLightningModule.evaluate`` averages over. The rows that count are ordered by truncated history length,
    longest first, stable (``ops.length_order``'s rule), and cut into chunks of ``batch_size`` consecutive rows."""
    L, bs = int(max_seq_length), int(batch_size)
    if L < 1 or bs < 1:
        raise ValueError(f"max_seq_length and batch_size must be >= 1; got {max_seq_length}, {batch_size}")
    if len(hist_idx_lists) != len(target_idx_lists):
        raise ValueError(f"{len(hist_idx_lists)} histories for {len(target_idx_lists)} target lists")
    hl = np.asarray([len(h) for h in hist_idx_lists], dtype=np.int64)
    tl = np.asarray([len(t) for t in target_idx_lists], dtype=np.int64)
    keep = np.flatnonzero((hl > 0) & (tl > 0))
    trunc = np.minimum(hl[keep], L)
    order = np.argsort(-trunc, kind="stable")
    kept, lengths = keep[order].astype(np.int64), trunc[order]
    n = kept.size
    full, full_off = _flat(hist_idx_lists, kept)
    tok_off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lengths, out=tok_off[1:])
    # the last `lengths[i]` entries of each full history: token t of row i is full[full_off[i + 1] - lengths[i] + t]
    row_of_tok = np.repeat(np.arange(n, dtype=np.int64), lengths)
    pos = np.arange(tok_off[-1], dtype=np.int64) - tok_off[:-1][row_of_tok]
    hist = full[(full_off[1:] - lengths)[row_of_tok] + pos] if n else np.zeros(0, dtype=np.int64)
    # exclusions: sort (row, item) pairs, drop repeats within a row
    row_of_full = np.repeat(np.arange(n, dtype=np.int64), np.diff(full_off))
    o = np.lexsort((full, row_of_full))
    fs, rs = full[o], row_of_full[o]
    first = np.ones(fs.size, dtype=bool)
    first[1:] = (fs[1:] != fs[:-1]) | (rs[1:] != rs[:-1])
    excl = fs[first]
    excl_off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(rs[first], minlength=n), out=excl_off[1:])
    targets, target_off = _flat(target_idx_lists, kept)
    chunks = []
    for r0 in range(0, n, bs):
        r1 = min(r0 + bs, n)
        t0, t1 = int(tok_off[r0]), int(tok_off[r1])
        chunks.append(EvalChunk(r0, r1, t0, t1, (tok_off[r0 : r1 + 1] - t0).astype(np.int32), t1 - t0, int(lengths[r0])))
    return EvalPlan(kept=kept, lengths=lengths, hist=hist, row_pos=pos.astype(np.int32), tok_offsets=tok_off, chunks=chunks,
                    excl=excl, excl_offsets=excl_off, targets=targets, target_offsets=target_off, max_seq_length=L,
                    batch_size=bs)


class DeviceEvalSet:
    """The validation rows of ``module``, planned once (:func:`plan_eval_rows`) and resident on the module's device.

        evalset = DeviceEvalSet.from_rows(module, rows)      # once: id conversion, plan, one upload
        evalset.evaluate()                                   # per validation: launches + one 64-byte read-back
        trainer.fit(batches, val=evalset, val_check_interval=12, early_stopping=True, checkpoint_dir="ckpt")

    A pass makes no host -> device copy and loops over chunks, not rows. It runs in eval mode (the model's training flag is
    restored), so neither the dropout step count nor the optimizer is touched."""

    def __init__(self, module, plan: EvalPlan, cutoffs_only: bool = False):
        model = module.model
        assert model is not None and model.embeddings is not None, "configure_model() and an item table come first"
        top_k = int(module.config.top_k)
        if top_k > 128 and not cutoffs_only:
            raise ValueError(f"top_k = {top_k}: the tiled top-k (xfmr_topk_tiled) returns at most 128 items per row")
        self.cutoffs_only = bool(cutoffs_only)
        if plan.kept.size == 0:
            raise ValueError("no validation row has both a non-empty history and a positive target")
        self.module, self.plan, self.top_k = module, plan, top_k
        self.kept = plan.kept
        dev = self.device = model.device

        def up(a):
            return torch.from_numpy(np.ascontiguousarray(a)).to(dev)

        self.hist, self.row_pos = up(plan.hist), up(plan.row_pos)
        self.excl, self.excl_offsets = up(plan.excl), up(plan.excl_offsets)
        self.targets, self.target_offsets = up(plan.targets), up(plan.target_offsets)
        self.packed = bool(model.supports_packed_rows(plan.chunks[0].max_len))
        self._chunks = []
        for c in plan.chunks:
            d = {"rows": (c.row0, c.row1), "excl_offsets": self.excl_offsets[c.row0 : c.row1 + 1]}
            if self.packed:
                d["packed"] = {"hist": self.hist[c.tok0 : c.tok1], "row_pos": self.row_pos[c.tok0 : c.tok1],
                               "seq_offsets": up(c.seq_offsets), "batch": c.row1 - c.row0, "seq_len": c.max_len}
            else:
                # right-padded (b, L_chunk) with the padding row 0, as encode_batch builds it
                lens = plan.lengths[c.row0 : c.row1]
                pad = np.zeros((c.row1 - c.row0, c.max_len), dtype=np.int64)
                pad[np.arange(c.max_len)[None, :] < lens[:, None]] = plan.hist[c.tok0 : c.tok1]
                d["padded"] = up(pad)
            self._chunks.append(d)
        torch.cuda.synchronize(dev)  # (the uploads came from pageable numpy memory)

    @classmethod
    def from_rows(cls, module, rows, batch_size: int = 1024, cutoffs_only: bool = False) -> "DeviceEvalSet":
        """``rows`` in the reference's format: ``{"history": {"item_id"}, "target": {"item_id", "label"}}``. Ids go through
        the module's own ``_to_idx`` (unknown ids are dropped), exactly as ``module.evaluate(rows)`` maps them.
        ``cutoffs_only=True``: a set that is only ever evaluated with ``cutoffs`` (the rank path, which has no top_k
        limit); ``recommend`` and ``evaluate()`` without cutoffs then refuse a ``top_k`` above 128."""
        if module.model is None:
            module.configure_model()
        if int(module.config.top_k) > 128 and not cutoffs_only:
            raise ValueError(f"top_k = {module.config.top_k}: the tiled top-k (xfmr_topk_tiled) returns at most 128 items per row")
        hists, tgts = [], []
        for r in rows:
            hists.append(module._to_idx_or_empty(list(r["history"]["item_id"])))
            tgts.append(module._to_idx_or_empty([i for i, l in zip(r["target"]["item_id"], r["target"]["label"]) if l]))
        return cls(module, plan_eval_rows(hists, tgts, module.model.max_seq_length, batch_size), cutoffs_only=cutoffs_only)

    def __len__(self) -> int:
        return int(self.kept.size)

    @torch.no_grad()
    def encode(self) -> torch.Tensor:
        """Sentence embeddings (n_kept, H) in plan order, in eval mode."""
        model = self.module.model
        cfg = model.config
        out = torch.empty((len(self), cfg.hidden_size), dtype=torch.float32, device=self.device)
        was_training = model.training
        model.eval()
        try:
            for c in self._chunks:
                r0, r1 = c["rows"]
                if self.packed:
                    tok, _ = model._encode_tokens(packed=c["packed"])
                    out[r0:r1] = ops.pool_rows(tok, c["packed"]["seq_offsets"], cfg.pooling_mode,
                                               normalize=bool(cfg.is_normalized))
                else:
                    out[r0:r1] = model(c["padded"])["sentence_embedding"]
        finally:
            model.train(was_training)
        return out

    @torch.no_grad()
    def recommend(self, embedding: torch.Tensor | None = None):
        """``(item_idx (n_kept, k) int64, -1 padded; score (n_kept, k))``: xfmr_topk_tiled per chunk over the module's
        ``items_index`` (its metric, table and norms), each row's whole history excluded."""
        if self.top_k > 128:
            raise ValueError(f"top_k = {self.top_k}: the tiled top-k (xfmr_topk_tiled) returns at most 128 items per row; "
                             "this set was built with cutoffs_only=True: evaluate it with cutoffs")
        emb = self.encode() if embedding is None else embedding
        index = self.module.items_index
        k, n_rows, H = self.top_k, index.table.shape[0], emb.shape[1]
        idx = torch.empty((len(self), k), dtype=torch.int64, device=self.device)
        score = torch.empty((len(self), k), dtype=torch.float32, device=self.device)
        rnorm = index.rnorm if index.metric == METRICS["cosine"] else None
        sqnorm = index.sqnorm if index.metric == METRICS["l2"] else None
        lib = N.load()
        for c in self._chunks:
            r0, r1 = c["rows"]
            nbytes = lib.xfmr_topk_tiled_workspace(r1 - r0, n_rows, k)
            ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=self.device)
            N.check(
                lib.xfmr_topk_tiled(N.ptr(emb[r0:r1]), N.ptr(index.table), N.ptr(rnorm), N.ptr(sqnorm), n_rows, r1 - r0, H,
                                    N.ptr(self.excl), N.ptr(c["excl_offsets"]), k, index.metric, N.ptr(idx[r0:r1]),
                                    N.ptr(score[r0:r1]), N.ptr(ws), nbytes, N.stream()),
                "xfmr_topk_tiled",
            )
        return idx, score

    @torch.no_grad()
    def evaluate_device(self) -> torch.Tensor:
        """One pass: 8 doubles on the device (the sums of the seven metrics over the kept rows, and their number); no
        host sync."""
        idx, _ = self.recommend()
        return retrieval_metrics_sum(idx, (self.targets, self.target_offsets), None, top_k=self.top_k)

    @torch.no_grad()
    def target_ranks(self, embedding: torch.Tensor | None = None) -> torch.Tensor:
        """The exact rank of every target of every kept row among the row's eligible items (int32, parallel to
        ``self.targets``; ``_native.RANK_NONE`` where a target is in the row's history): one encode, then
        ``ExactItemIndex.rank_targets`` per chunk into one resident tensor. No limit on ``top_k``."""
        emb = self.encode() if embedding is None else embedding
        index = self.module.items_index
        ranks = torch.empty((self.targets.numel(),), dtype=torch.int32, device=self.device)
        toff = self.plan.target_offsets
        for c in self._chunks:
            r0, r1 = c["rows"]
            index.rank_targets(emb[r0:r1], (self.targets, self.target_offsets[r0 : r1 + 1]),
                               (self.excl, c["excl_offsets"]), n_targets=int(toff[r1] - toff[r0]), out=ranks)
        return ranks

    def _cutoffs(self, cutoffs) -> tuple[int, ...]:
        cut = normalize_cutoffs(cutoffs)
        return cut if self.top_k in cut else cut + (self.top_k,)

    @torch.no_grad()
    def evaluate_ranks_device(self, cutoffs) -> torch.Tensor:
        """One rank pass and one ``rank_metrics_sum``: ``(len(cutoffs), 8)`` doubles on the device, no host sync. The
        cutoffs are taken as given (``config.top_k`` is not added here)."""
        return rank_metrics_sum(self.target_ranks(), (self.targets, self.target_offsets), normalize_cutoffs(cutoffs))

    def evaluate(self, stage: str = "val", cutoffs=None) -> dict[str, float]:
        """The keys of ``RecommenderLightningModule.evaluate``: ``{stage}/<metric>`` means and ``{stage}/num_rows``. One
        read-back of 64 bytes.

        ``cutoffs`` (e.g. ``(5, 10, 20, 500)``): the rank path instead of the ranked list -- one pass over the catalogue
        gives every target's exact rank, one launch pair the metrics at every cutoff, one read-back of 64 bytes per
        cutoff. Adds ``{stage}/<metric>@<K>`` for every cutoff; the plain keys are those of cutoff ``config.top_k``
        (added to the cutoffs when missing), equal to what the call without cutoffs returns."""
        if cutoffs is not None:
            cut = self._cutoffs(cutoffs)
            sums = self.evaluate_ranks_device(cut).tolist()
            out = {}
            for K, s in zip(cut, sums):
                n = int(s[7])
                for i, name in enumerate(METRIC_NAMES):
                    out[f"{stage}/{name}@{K}"] = s[i] / n if n else float("nan")
                if K == self.top_k:
                    for i, name in enumerate(METRIC_NAMES):
                        out[f"{stage}/{name}"] = out[f"{stage}/{name}@{K}"]
                    out[f"{stage}/num_rows"] = n
            return out
        s = self.evaluate_device().tolist()
        n = int(s[7])
        out = {f"{stage}/{name}": (s[i] / n if n else float("nan")) for i, name in enumerate(METRIC_NAMES)}
        out[f"{stage}/num_rows"] = n
        return out
