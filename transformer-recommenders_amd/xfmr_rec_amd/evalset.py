"""A validation set prepared ONCE and kept in HBM (a peer of ``data.DeviceSeqDataset`` for the validation path).

``RecommenderLightningModule.evaluate(rows)`` redoes, on every call, host work that depends on the rows only and never on
the model: id -> row conversion, truncation, padding, the length order, the packed layout behind an upload, the sorted
exclusions, the targets CSR, and a read-back + host sum per pass (profiles/eval_batched.md:
0.18-0.29 s for 6 040 users, host-bound). Here all of that is :func:`plan_eval_rows` (numpy, once) + one upload;
a pass is then the packed forward, one pooling launch and one tiled top-k per chunk, ONE ``xfmr_retrieval_metrics_sum``
over all rows, and a 64-byte read-back. ``Trainer.fit(val=...)`` runs it between steps.

Data-parallel runs shard the plan (:func:`shard_eval_plan`: global plan row i belongs to rank ``i % world_size``). A rank's
pass is the same pass over its own rows; ONE exchange per pass (:func:`gather_rows`) then puts every rank's lists -- or
target ranks -- into global plan order on every rank, and the one metrics launch runs over the global rows everywhere:
the same kernels over the same bytes, so every rank holds the same doubles, bit for bit, without a floating-point
reduction across ranks.
"""

from __future__ import annotations

import dataclasses

import numpy as np
import torch

from . import eval_rows as E
from .retrieval import normalize_cutoffs, rank_metrics_sum, retrieval_metrics_sum


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
    targets: np.ndarray      # targets CSR: the positive target indices as given (of a shard: the GLOBAL plan's)
    target_offsets: np.ndarray  # (n + 1,) int64, absolute (of a shard: the GLOBAL plan's, n_global + 1 entries)
    max_seq_length: int
    batch_size: int
    # a plan's place among the shards of a data-parallel run (shard_eval_plan); an unsharded plan is the one shard of a
    # world of one: n_global = n, global_rows = 0 .. n - 1, target_pos = 0 .. targets.size - 1 (filled in when left out)
    n_global: int = 0                      # rows of the global plan
    global_rows: np.ndarray | None = None  # (n,) int64: plan row i is row global_rows[i] of the global plan
    target_pos: np.ndarray | None = None   # int64: where this plan's rows' targets lie in the flat `targets`, row by row
    rank: int = 0
    world_size: int = 1

    def __post_init__(self):
        if self.global_rows is None:  # an unsharded plan
            self.n_global = int(self.kept.size)
            self.global_rows = np.arange(self.n_global, dtype=np.int64)
            self.target_pos = np.arange(self.targets.size, dtype=np.int64)

    def local_targets(self) -> tuple[np.ndarray, np.ndarray]:
        """The targets CSR of THIS plan's rows (``targets[target_pos]`` and its own offsets, n + 1 entries)."""
        lens = np.diff(self.target_offsets)[self.global_rows]
        off = np.zeros(lens.size + 1, dtype=np.int64)
        np.cumsum(lens, out=off[1:])
        return self.targets[self.target_pos], off


def _exact_csr(lists) -> tuple[np.ndarray, np.ndarray]:
    """``eval_rows.flat_csr`` without the placeholder element of an empty CSR: a plan's arrays hold their entries and
    nothing else (the shards index them by position)."""
    flat, off = E.flat_csr(lists)
    return flat[: off[-1]], off


@dataclasses.dataclass
class DeviceChunk:
    """An :class:`EvalChunk` on the device: its rows, its view of the resident exclusion offsets and its encoder input --
    what ``RecommenderModel.sentence_embeddings`` takes: the host-planned packed dict, or the right-padded tensor."""

    row0: int
    row1: int
    excl_offsets: torch.Tensor
    tokens: dict | torch.Tensor


def _take_csr(off: np.ndarray, rows: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """For the CSR rows ``rows`` of offsets ``off``: the flat positions of their entries, row by row, and the offsets of
    the CSR those entries form on their own."""
    rows = np.asarray(rows, dtype=np.int64)
    lens = off[rows + 1] - off[rows]
    new_off = np.zeros(rows.size + 1, dtype=np.int64)
    np.cumsum(lens, out=new_off[1:])
    row_of = np.repeat(np.arange(rows.size, dtype=np.int64), lens)
    pos = off[rows][row_of] + (np.arange(new_off[-1], dtype=np.int64) - new_off[:-1][row_of])
    return pos, new_off


def _chunks(tok_off: np.ndarray, lengths: np.ndarray, bs: int) -> list:
    n = lengths.size
    chunks = []
    for r0 in range(0, n, bs):
        r1 = min(r0 + bs, n)
        t0, t1 = int(tok_off[r0]), int(tok_off[r1])
        chunks.append(EvalChunk(r0, r1, t0, t1, (tok_off[r0 : r1 + 1] - t0).astype(np.int32), t1 - t0, int(lengths[r0])))
    return chunks


def shard_rows_of(n_global: int, rank: int, world_size: int) -> np.ndarray:
    """The global plan rows of ``rank``: ``rank, rank + world_size, ...`` (int64). Round-robin over the length-sorted
    order gives every rank its share of the long histories; contiguous blocks would give rank 0 all of them."""
    return np.arange(int(rank), int(n_global), int(world_size), dtype=np.int64)


def shard_eval_plan(plan: EvalPlan, rank: int, world_size: int) -> EvalPlan:
    """``rank``'s shard of a global plan: the global rows ``i`` with ``i % world_size == rank`` in global order, chunked by
    the plan's ``batch_size`` with their own ``seq_offsets``, ``tok_offsets`` and ``excl`` / ``excl_offsets`` -- exactly
    the plan :func:`plan_eval_rows` builds of those rows alone (they are in length order already, and the order is
    stable). The shard keeps the GLOBAL ``targets`` / ``target_offsets`` (small; the final sum on every rank reads
    them), ``n_global``, its rows' places in the global plan (``global_rows``) and its targets' places in the global flat
    array (``target_pos``; :meth:`EvalPlan.local_targets` is the shard's own CSR). A shard is empty when ``rank >=
    n_global``. ``world_size=1`` returns ``plan`` itself."""
    W, r = int(world_size), int(rank)
    if W < 1 or not 0 <= r < W:
        raise ValueError(f"rank must lie in [0, world_size) and world_size be >= 1; got rank {rank}, world_size {world_size}")
    if plan.world_size != 1:
        raise ValueError(f"the plan is shard {plan.rank} of {plan.world_size} already: shard the global plan")
    if W == 1:
        return plan
    rows = shard_rows_of(plan.kept.size, r, W)
    lengths = plan.lengths[rows]
    tok_pos, tok_off = _take_csr(plan.tok_offsets, rows)
    excl_pos, excl_off = _take_csr(plan.excl_offsets, rows)
    target_pos, _ = _take_csr(plan.target_offsets, rows)
    return EvalPlan(kept=plan.kept[rows], lengths=lengths, hist=plan.hist[tok_pos], row_pos=plan.row_pos[tok_pos],
                    tok_offsets=tok_off, chunks=_chunks(tok_off, lengths, plan.batch_size), excl=plan.excl[excl_pos],
                    excl_offsets=excl_off, targets=plan.targets, target_offsets=plan.target_offsets,
                    max_seq_length=plan.max_seq_length, batch_size=plan.batch_size, n_global=int(plan.kept.size),
                    global_rows=rows, target_pos=target_pos, rank=r, world_size=W)


def gather_index(owned) -> tuple[list[int], np.ndarray]:
    """The host half of :func:`gather_rows`. ``owned[r]``: the global positions that rank r's local entries belong at, in
    the rank's local order; together they partition ``0 .. n - 1``. Returns every rank's count and the int64 index with
    ``global = concat_r(pad(local_r, max(counts)))[index]``."""
    owned = [np.asarray(o, dtype=np.int64).reshape(-1) for o in owned]
    counts = [int(o.size) for o in owned]
    pad, n = max(counts, default=0), sum(counts)
    index = np.full(n, -1, dtype=np.int64)
    for r, o in enumerate(owned):
        if o.size and (o.min() < 0 or o.max() >= n):
            raise ValueError(f"rank {r} owns positions outside 0 .. {n - 1}")
        index[o] = r * pad + np.arange(o.size, dtype=np.int64)
    if (index < 0).any():
        raise ValueError("the ranks' positions do not partition 0 .. n - 1")
    return counts, index


def gather_rows(local: torch.Tensor, counts, index: torch.Tensor, group=None, fill=-1) -> torch.Tensor:
    """A pass's ONE exchange: every rank's ``local`` ``(counts[rank], ...)`` rows, on every rank, in global order.

    ``local`` is padded to ``max(counts)`` rows with ``fill``, ``torch.distributed.all_gather`` collects the equal-sized
    blocks in rank order, and one ``index_select`` with ``index`` (:func:`gather_index`, on ``local``'s device) puts the
    rows in place; the padding is never selected. Collective: every rank of ``group`` calls it, an empty shard included.
    Works on any device the group's backend moves (CPU tensors over gloo, HBM tensors over RCCL or gloo)."""
    import torch.distributed as dist

    counts = [int(c) for c in counts]
    if len(counts) != dist.get_world_size(group):
        raise ValueError(f"{len(counts)} counts for a group of {dist.get_world_size(group)} ranks")
    mine = counts[dist.get_rank(group)]
    if local.shape[0] != mine:
        raise ValueError(f"rank {dist.get_rank(group)} holds {local.shape[0]} rows where the plan gives it {mine}")
    buf = local.new_full((max(counts),) + tuple(local.shape[1:]), fill)
    buf[:mine] = local
    parts = [torch.empty_like(buf) for _ in counts]
    dist.all_gather(parts, buf, group=group)
    return torch.cat(parts).index_select(0, index)


def plan_eval_rows(hist_idx_lists, target_idx_lists, max_seq_length: int, batch_size: int, *, rank: int = 0,
                   world_size: int = 1) -> EvalPlan:
    """The model-independent half of a validation pass, in numpy (no device).

    ``hist_idx_lists`` / ``target_idx_lists``: per input row, the history and the POSITIVE targets as table rows (unknown
    ids already dropped). A row counts when its history is non-empty and it has at least one positive target -- the rows
    ``RecommenderLightningModule.evaluate`` averages over. The rows that count are ordered by truncated history length,
    longest first, stable (``ops.length_order``'s rule), and cut into chunks of ``batch_size`` consecutive rows.

    ``rank`` / ``world_size``: that global plan's shard for the rank (:func:`shard_eval_plan`)."""
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
    full, full_off = _exact_csr([hist_idx_lists[r] for r in kept])
    tok_off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lengths, out=tok_off[1:])
    # the last `lengths[i]` entries of each full history: token t of row i is full[full_off[i + 1] - lengths[i] + t]
    row_of_tok = np.repeat(np.arange(n, dtype=np.int64), lengths)
    pos = np.arange(tok_off[-1], dtype=np.int64) - tok_off[:-1][row_of_tok]
    hist = full[(full_off[1:] - lengths)[row_of_tok] + pos] if n else np.zeros(0, dtype=np.int64)
    excl, excl_off = E.sort_unique_rows(full, full_off)  # exclusions: each row's WHOLE history, sorted, repeats dropped
    targets, target_off = _exact_csr([target_idx_lists[r] for r in kept])
    plan = EvalPlan(kept=kept, lengths=lengths, hist=hist, row_pos=pos.astype(np.int32), tok_offsets=tok_off,
                    chunks=_chunks(tok_off, lengths, bs), excl=excl, excl_offsets=excl_off, targets=targets,
                    target_offsets=target_off, max_seq_length=L, batch_size=bs)
    return shard_eval_plan(plan, rank, world_size)


class DeviceEvalSet:
    """The validation rows of ``module``, planned once (:func:`plan_eval_rows`) and resident on the module's device.

        evalset = DeviceEvalSet.from_rows(module, rows)      # once: id conversion, plan, one upload
        evalset.evaluate()                                   # per validation: launches + one 64-byte read-back
        trainer.fit(batches, val=evalset, val_check_interval=12, early_stopping=True, checkpoint_dir="ckpt")

    A pass makes no host -> device copy and loops over chunks, not rows. It runs in eval mode (the model's training flag is
    restored), so neither the dropout step count nor the optimizer is touched.

    Data-parallel runs (``rank`` / ``world_size`` / ``process_group``; the defaults are the single-process set): the set
    holds the rank's shard of the plan (:func:`shard_eval_plan`) -- its histories and exclusions -- and the global targets
    CSR. ``len(set)`` is the GLOBAL number of kept rows, ``n_local`` the shard's; ``kept`` and ``global_rows`` name the
    local rows. :meth:`encode`, :meth:`recommend` and :meth:`target_ranks` work on the LOCAL rows (shapes ``(n_local,
    ...)``; an empty shard launches nothing and returns empty tensors). :meth:`evaluate_device`,
    :meth:`evaluate_ranks_device` and :meth:`evaluate` are COLLECTIVE: every rank calls them, and each makes exactly one
    exchange per pass (:func:`gather_rows` through ``torch.distributed`` on ``process_group``), behind its chunk loop --
    however many chunks a rank has. The exchanged lists (or target ranks) are put in global plan order and the one
    metrics launch runs over all global rows on every rank, so every rank holds the same doubles bit for bit: those of
    the unsharded set whenever the local passes gave the unsharded pass's lists. Two ranks on one device over gloo is
    what has run; RCCL's transport has not."""

    def __init__(self, module, plan: EvalPlan, cutoffs_only: bool = False, *, rank: int = 0, world_size: int = 1,
                 process_group=None):
        model = module.model
        assert model is not None and model.embeddings is not None, "configure_model() and an item table come first"
        top_k = int(module.config.top_k)
        if not cutoffs_only:
            E.check_tiled_top_k(top_k)
        self.cutoffs_only = bool(cutoffs_only)
        if plan.world_size == 1 and int(world_size) > 1:
            plan = shard_eval_plan(plan, rank, world_size)
        elif (plan.rank, plan.world_size) != (int(rank), int(world_size)):
            raise ValueError(f"the plan is shard {plan.rank} of world_size {plan.world_size}; the set was asked for rank "
                             f"{rank} of world_size {world_size}")
        if plan.n_global == 0:
            raise ValueError("no validation row has both a non-empty history and a positive target")
        self.module, self.plan, self.top_k = module, plan, top_k
        self.kept, self.global_rows = plan.kept, plan.global_rows
        self.rank, self.world_size, self.process_group = plan.rank, plan.world_size, process_group
        self.n_global, self.n_local = int(plan.n_global), int(plan.kept.size)
        dev = self.device = model.device

        def up(a):
            return torch.from_numpy(np.ascontiguousarray(a)).to(dev)

        self.hist, self.row_pos = up(plan.hist), up(plan.row_pos)
        self.excl, self.excl_offsets = up(plan.excl), up(plan.excl_offsets)
        self.targets, self.target_offsets = up(plan.targets), up(plan.target_offsets)
        if self.world_size == 1:
            self.local_targets, self.local_target_offsets = self.targets, self.target_offsets
            self._local_toff = plan.target_offsets
        else:
            # the shard's own targets CSR (what its rank pass reads) and, for the one exchange of a pass, every rank's
            # count and the index that puts the gathered blocks in global order: rows for the lists, targets for the ranks
            tg, self._local_toff = plan.local_targets()
            self.local_targets, self.local_target_offsets = up(tg), up(self._local_toff)
            W = self.world_size
            owned = [shard_rows_of(self.n_global, r, W) for r in range(W)]
            self._row_counts, index = gather_index(owned)
            self._row_index = up(index)
            self._tgt_counts, index = gather_index([_take_csr(plan.target_offsets, o)[0] for o in owned])
            self._tgt_index = up(index)
        self.packed = bool(model.supports_packed_rows(plan.chunks[0].max_len if plan.chunks else plan.max_seq_length))
        self._chunks = []
        for c in plan.chunks:
            if self.packed:
                tokens = {"hist": self.hist[c.tok0 : c.tok1], "row_pos": self.row_pos[c.tok0 : c.tok1],
                          "seq_offsets": up(c.seq_offsets), "batch": c.row1 - c.row0, "seq_len": c.max_len}
            else:  # right-padded (b, L_chunk) with the padding row 0, as encode_batch builds it
                tokens = up(E.pad_histories(plan.lengths[c.row0 : c.row1], plan.hist[c.tok0 : c.tok1]))
            self._chunks.append(DeviceChunk(c.row0, c.row1, self.excl_offsets[c.row0 : c.row1 + 1], tokens))
        torch.cuda.synchronize(dev)  # (the uploads came from pageable numpy memory)

    @classmethod
    def from_rows(cls, module, rows, batch_size: int = 1024, cutoffs_only: bool = False, *, rank: int = 0,
                  world_size: int = 1, process_group=None) -> "DeviceEvalSet":
        """``rows`` in the reference's format: ``{"history": {"item_id"}, "target": {"item_id", "label"}}``. Ids go through
        the module's own ``_to_idx`` (unknown ids are dropped), exactly as ``module.evaluate(rows)`` maps them.
        ``cutoffs_only=True``: a set that is only ever evaluated with ``cutoffs`` (the rank path, which has no top_k
        limit); ``recommend`` and ``evaluate()`` without cutoffs then refuse a ``top_k`` above 128.
        ``rank`` / ``world_size`` / ``process_group``: every rank passes the SAME ``rows`` and its own rank; the set
        uploads that rank's shard only (see the class)."""
        if module.model is None:
            module.configure_model()
        if not cutoffs_only:
            E.check_tiled_top_k(module.config.top_k)
        hists, tgts = E.read_rows(rows, module._to_idx_or_empty)
        return cls(module, plan_eval_rows(hists, tgts, module.model.max_seq_length, batch_size), cutoffs_only=cutoffs_only,
                   rank=rank, world_size=world_size, process_group=process_group)

    def __len__(self) -> int:
        return self.n_global

    @torch.no_grad()
    def encode(self) -> torch.Tensor:
        """Sentence embeddings (n_local, H) in plan order, in eval mode."""
        model = self.module.model
        out = torch.empty((self.n_local, model.config.hidden_size), dtype=torch.float32, device=self.device)
        with model.eval_mode():
            for c in self._chunks:
                out[c.row0 : c.row1] = model.sentence_embeddings(c.tokens)
        return out

    @torch.no_grad()
    def recommend(self, embedding: torch.Tensor | None = None):
        """``(item_idx (n_local, k) int64, -1 padded; score (n_local, k))``: xfmr_topk_tiled per chunk over the module's
        ``items_index`` (its metric, table and norms), each row's whole history excluded."""
        E.check_tiled_top_k(self.top_k, "; this set was built with cutoffs_only=True: evaluate it with cutoffs")
        emb = self.encode() if embedding is None else embedding
        if emb.dtype != torch.float32 or emb.dim() != 2 or emb.shape[0] != self.n_local or not emb.is_contiguous():
            raise ValueError(f"embedding must be a contiguous float32 ({self.n_local}, H) tensor; got {emb.dtype}, "
                             f"{tuple(emb.shape)}")
        search = self.module.items_index._tiled_search(self.top_k)
        idx = torch.empty((self.n_local, self.top_k), dtype=torch.int64, device=self.device)
        score = torch.empty((self.n_local, self.top_k), dtype=torch.float32, device=self.device)
        for c in self._chunks:
            r0, r1 = c.row0, c.row1
            search(emb[r0:r1], self.excl, c.excl_offsets, idx[r0:r1], score[r0:r1])
        return idx, score

    @torch.no_grad()
    def evaluate_device(self) -> torch.Tensor:
        """One pass: 8 doubles on the device (the sums of the seven metrics over the kept rows, and their number); no
        host sync. Sharded: collective; the local lists are exchanged once and the sums are those over ALL global rows,
        the same bits on every rank (the exchange synchronises as its backend does)."""
        idx, _ = self.recommend()
        if self.world_size > 1:
            idx = gather_rows(idx, self._row_counts, self._row_index, self.process_group)
        return retrieval_metrics_sum(idx, (self.targets, self.target_offsets), None, top_k=self.top_k)

    @torch.no_grad()
    def target_ranks(self, embedding: torch.Tensor | None = None) -> torch.Tensor:
        """The exact rank of every target of every LOCAL row among the row's eligible items (int32, parallel to
        ``self.local_targets`` -- ``self.targets`` itself in a single-process set; ``_native.RANK_NONE`` where a target is
        in the row's history): one encode, then ``ExactItemIndex.rank_targets`` per chunk into one resident tensor. No
        limit on ``top_k``."""
        emb = self.encode() if embedding is None else embedding
        index = self.module.items_index
        ranks = torch.empty((self.local_targets.numel(),), dtype=torch.int32, device=self.device)
        toff = self._local_toff
        for c in self._chunks:
            r0, r1 = c.row0, c.row1
            index.rank_targets(emb[r0:r1], (self.local_targets, self.local_target_offsets[r0 : r1 + 1]),
                               (self.excl, c.excl_offsets), n_targets=int(toff[r1] - toff[r0]), out=ranks)
        return ranks

    @torch.no_grad()
    def evaluate_ranks_device(self, cutoffs) -> torch.Tensor:
        """One rank pass and one ``rank_metrics_sum``: ``(len(cutoffs), 8)`` doubles on the device, no host sync. The
        cutoffs are taken as given (``config.top_k`` is not added here). Sharded: collective; the local ranks are
        exchanged once into the order of the global targets, and the sums are those over ALL global rows, the same bits
        on every rank."""
        ranks = self.target_ranks()
        if self.world_size > 1:
            ranks = gather_rows(ranks, self._tgt_counts, self._tgt_index, self.process_group)
        return rank_metrics_sum(ranks, (self.targets, self.target_offsets), normalize_cutoffs(cutoffs))

    def evaluate(self, stage: str = "val", cutoffs=None) -> dict[str, float]:
        """The keys of ``RecommenderLightningModule.evaluate``: ``{stage}/<metric>`` means and ``{stage}/num_rows``. One
        read-back of 64 bytes. Sharded: collective, and the dict -- over all global rows, ``num_rows`` included -- is the
        same on every rank.

        ``cutoffs`` (e.g. ``(5, 10, 20, 500)``): the rank path instead of the ranked list -- one pass over the catalogue
        gives every target's exact rank, one launch pair the metrics at every cutoff, one read-back of 64 bytes per
        cutoff. Adds ``{stage}/<metric>@<K>`` for every cutoff; the plain keys are those of cutoff ``config.top_k``
        (added to the cutoffs when missing), equal to what the call without cutoffs returns."""
        if cutoffs is None:
            return E.metrics_dict(stage, self.evaluate_device().tolist(), top_k=self.top_k)
        cut = E.eval_cutoffs(cutoffs, self.top_k)
        return E.metrics_dict(stage, self.evaluate_ranks_device(cut).tolist(), cut, self.top_k)


class SampledEvalSet(DeviceEvalSet):
    """A :class:`DeviceEvalSet` under the SAMPLED-CANDIDATE protocol (SASRec, BERT4Rec: HR@10 / NDCG@10 of the held-out
    item against 100 sampled negatives): a row's targets are ranked among the row's own candidate list, not the catalogue.

        val = SampledEvalSet.from_rows(module, rows, num_negatives=100, seed=0)   # negatives drawn once, resident
        val.evaluate(cutoffs=(10,))                                               # val/retrieval_hit_rate@10, ...
        trainer.fit(batches, val=val, val_cutoffs=(10,), monitor={"name": "val/retrieval_normalized_dcg@10", "mode": "max"})

    The plan, the encoder input, the exclusions (each row's whole history: a history item is neither drawn as a negative
    nor eligible) and the targets are the full-catalogue set's, so the two sets differ only in the items a target is
    ranked among. ``candidates`` is the resident sorted CSR of those items per plan row: the drawn negatives
    (``eval_rows.sample_eval_negatives``, keyed by ``(seed, input row)``: a row's negatives do not depend on the other
    rows or on ``batch_size``), or the explicit lists given. Every pass takes the rank path
    (``ExactItemIndex.rank_among`` per chunk, ``rank_metrics_sum`` once): there is no ranked list, so no limit on
    ``top_k`` or a cutoff. Attributes: ``protocol`` ("sampled" or "candidates"), ``num_negatives`` (None for explicit
    candidates), ``seed``. Single process only: a sharded sampled set is not built (``world_size > 1`` raises)."""

    def __init__(self, module, plan: EvalPlan, candidates, *, protocol: str = "candidates", num_negatives=None,
                 seed: int = 0, world_size: int = 1):
        """``candidates``: ``(flat, offsets)`` numpy int64 CSR over the PLAN's rows, each row sorted ascending."""
        if int(world_size) != 1 or plan.world_size != 1:
            raise ValueError(f"SampledEvalSet runs in a single process: world_size = {max(int(world_size), plan.world_size)} "
                             "(a sharded sampled set) is not supported; evaluate it on one rank")
        super().__init__(module, plan, cutoffs_only=True)
        flat, off = (np.asarray(x, dtype=np.int64) for x in candidates)
        if off.size != self.n_local + 1:
            raise ValueError(f"candidates offsets have {off.size} entries for {self.n_local} rows")
        self.protocol, self.num_negatives, self.seed = str(protocol), num_negatives, int(seed)
        self.candidates = torch.from_numpy(np.ascontiguousarray(flat if flat.size else np.zeros(1, np.int64))).to(self.device)
        self.candidate_offsets = torch.from_numpy(np.ascontiguousarray(off)).to(self.device)
        torch.cuda.synchronize(self.device)

    @classmethod
    def from_rows(cls, module, rows, num_negatives: int = 100, seed: int = 0, weights=None, candidates=None,
                  batch_size: int = 1024, *, rank: int = 0, world_size: int = 1) -> "SampledEvalSet":
        """``rows`` as :meth:`DeviceEvalSet.from_rows`. Without ``candidates``: every row draws ``num_negatives`` distinct
        negatives outside its history and targets, uniformly or in proportion to ``weights`` (one non-negative number per
        table row). ``candidates``: per input row, the item ids to rank the row's targets among instead (mapped through the
        module's id lookup; unknown ids are dropped)."""
        if int(world_size) != 1:
            raise ValueError(f"SampledEvalSet runs in a single process: world_size = {world_size} (a sharded sampled set) is "
                             "not supported; evaluate it on one rank")
        if module.model is None:
            module.configure_model()
        rows = list(rows)
        hists, tgts = E.read_rows(rows, module._to_idx_or_empty)
        plan = plan_eval_rows(hists, tgts, module.model.max_seq_length, batch_size)
        if candidates is None:
            n_items = int(module.model.embeddings.shape[0])
            lists = _rows_of_csr(E.sample_eval_negatives(hists, tgts, n_items, num_negatives, seed, weights), plan.kept)
            return cls(module, plan, E.candidates_csr(lists), protocol="sampled", num_negatives=int(num_negatives), seed=seed)
        candidates = list(candidates)
        if len(candidates) != len(rows):
            raise ValueError(f"{len(candidates)} candidate lists for {len(rows)} rows")
        lists = E.map_candidates(candidates, module._to_idx_or_empty)
        return cls(module, plan, E.candidates_csr([lists[r] for r in plan.kept]), protocol="candidates", seed=seed)

    @torch.no_grad()
    def target_ranks(self, embedding: torch.Tensor | None = None) -> torch.Tensor:
        """The rank of every target among its row's candidates and targets (int32, parallel to ``self.targets``;
        ``_native.RANK_NONE`` where a target is in the row's history): one encode, then ``ExactItemIndex.rank_among``
        per chunk into one resident tensor."""
        emb = self.encode() if embedding is None else embedding
        index = self.module.items_index
        ranks = torch.empty((self.targets.numel(),), dtype=torch.int32, device=self.device)
        for c in self._chunks:
            r0, r1 = c.row0, c.row1
            index.rank_among(emb[r0:r1], (self.candidates, self.candidate_offsets[r0 : r1 + 1]),
                             (self.targets, self.target_offsets[r0 : r1 + 1]), (self.excl, c.excl_offsets), out=ranks)
        return ranks

    def recommend(self, embedding=None):
        raise ValueError("a SampledEvalSet has no ranked list over the catalogue: use evaluate(cutoffs=) or target_ranks()")

    def evaluate(self, stage: str = "val", cutoffs=None) -> dict[str, float]:
        """The keys of ``DeviceEvalSet.evaluate(stage, cutoffs=...)`` under the sampled protocol: always the rank path.
        ``cutoffs`` defaults to ``(config.top_k,)``; ``config.top_k`` is added when missing and gives the plain keys."""
        cut = E.eval_cutoffs((self.top_k,) if cutoffs is None else cutoffs, self.top_k)
        return E.metrics_dict(stage, self.evaluate_ranks_device(cut).tolist(), cut, self.top_k)


def _rows_of_csr(csr, rows) -> list:
    """The CSR's rows ``rows`` as a list of arrays."""
    flat, off = csr
    return [flat[off[r] : off[r + 1]] for r in rows]
