"""Exact GPU retrieval + ranking metrics for the validation path.

Mirrors what ``RecommenderLightningModule.recommend / predict_step / compute_metrics`` do through LanceDB and
torchmetrics (``xfmr_rec/trainer.py:186-211, 266-314``, ``index.py:214-255``, ``metrics.py:17-79``), for a batch of
users at once: ``ExactItemIndex.search`` = exact top-k over the item table with each user's history excluded;
``compute_retrieval_metrics`` = the seven metrics under the reference's names. ``ExactItemIndex.search_batch`` is the
same search for a whole user set (xfmr_topk_tiled: no per-(user, item) workspace).
"""

from __future__ import annotations

import ctypes as C
import os

import torch

from . import _native as N
from .eval_rows import METRIC_NAMES, flat_csr, normalize_cutoffs  # noqa: F401 - (names of this module too)

METRICS = {"cosine": 0, "dot": 1, "l2": 2}
SEARCH_MODES = ("exact", "refined")  # the ``search=`` option of recommend_batch / SessionRecommender.recommend


def refined_search_enabled() -> bool:
    """``XFMR_SEARCH=exact``, read per call, routes every refined search through the exact one again (A/B runs and a
    way back without a code change, as ``XFMR_INFER=0`` is for the encoder)."""
    return os.environ.get("XFMR_SEARCH", "") != "exact"


def _csr(lists, device, sort_unique: bool = False):
    return tuple(torch.from_numpy(x).to(device) for x in flat_csr(lists, sort_unique))


def sorted_exclusion_csr(lists):
    """Host side of xfmr_topk_tiled's exclusions: each query's list sorted ascending with duplicates removed, as one
    flat int64 array + (B + 1) int64 offsets (numpy; ``eval_rows.flat_csr``). The kernel binary-searches each list."""
    return flat_csr(lists, sort_unique=True)


def _queries(embedding):
    """(B,H) or (H,) -> (contiguous float32 (B,H), B, H, device)."""
    q = embedding.reshape(-1, embedding.shape[-1]).contiguous().to(torch.float32)
    return q, q.shape[0], q.shape[1], q.device


def _check_csr(name, csr, B, rows="queries", int64=True):
    flat, off = csr
    if off.numel() != B + 1:
        raise ValueError(f"{name} offsets have {off.numel()} entries for {B} {rows}")
    if int64 and (flat.dtype != torch.int64 or off.dtype != torch.int64):
        raise ValueError(f"{name} must be int64 tensors")
    return flat, off


def _use_mask(use, B):
    if use is None:
        return None
    if use.numel() != B:
        raise ValueError(f"use has {use.numel()} entries for {B} rows")
    use = use.view(torch.uint8) if use.dtype == torch.bool else use
    if use.dtype != torch.uint8:
        raise ValueError(f"use must be uint8 or bool, got {use.dtype}")
    return use


class ExactItemIndex:
    """``LanceIndex.search`` (``index.py:214-255``) as an exact scan of the item table (row 0 = padding)."""

    def __init__(self, table: torch.Tensor, table_rnorm: torch.Tensor | None = None, index_metric: str = "cosine",
                 table_bf16: torch.Tensor | None = None):
        from . import ops

        self.table = table.contiguous()
        self.rnorm = table_rnorm if table_rnorm is not None else ops.table_rnorm(self.table)
        self.metric = METRICS[index_metric]
        self._sqnorm = None
        self._table_bf16 = table_bf16  # the model's bf16 copy of the table when it has one (ops.table_prepare)
        self._norm_bounds = None

    @property
    def sqnorm(self) -> torch.Tensor:
        """Squared item norms (the l2 metric's item term of :meth:`search_batch`), computed once."""
        if self._sqnorm is None:
            from . import ops

            self._sqnorm = ops.table_sqnorm(self.table)
        return self._sqnorm

    def _norms(self):
        """(rnorm, sqnorm) as the tile kernels take them: only the array the metric reads."""
        return (self.rnorm if self.metric == METRICS["cosine"] else None,
                self.sqnorm if self.metric == METRICS["l2"] else None)

    def search(self, embedding: torch.Tensor, exclude_item_idx=None, top_k: int = 20):
        """embedding (B,H) or (H,); exclude_item_idx: per-query lists of item indices (the users' histories).
        Returns (item_idx (B,top_k) int64, -1 padded; score (B,top_k) = 1 - distance), best first."""
        q, B, H, dev = _queries(embedding)
        idx = torch.empty((B, top_k), dtype=torch.int64, device=dev)
        score = torch.empty((B, top_k), dtype=torch.float32, device=dev)
        ex, exo = (None, None) if exclude_item_idx is None else _csr(exclude_item_idx, dev)
        lib = N.load()
        nbytes = lib.xfmr_topk_workspace(B, self.table.shape[0])
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        N.check(
            lib.xfmr_topk(N.ptr(q), N.ptr(self.table), N.ptr(self.rnorm), self.table.shape[0], B, H, N.ptr(ex),
                          N.ptr(exo), top_k, self.metric, N.ptr(idx), N.ptr(score), N.ptr(ws), nbytes, N.stream()),
            "xfmr_topk",
        )
        return idx, score

    def search_batch(self, embedding: torch.Tensor, exclude_item_idx=None, top_k: int = 20):
        """:meth:`search` for a batch of users through xfmr_topk_tiled: score tiles on the matrix cores and a streaming
        top-k, no (B, n_items) workspace. Same results as :meth:`search` up to the summation order of the scores (so up
        to near-tied scores at the k-th place). top_k <= 128."""
        q, B, _, dev = _queries(embedding)
        idx = torch.empty((B, top_k), dtype=torch.int64, device=dev)
        score = torch.empty((B, top_k), dtype=torch.float32, device=dev)
        if B == 0:
            return idx, score
        ex = exo = None
        if exclude_item_idx is not None:
            if len(exclude_item_idx) != B:
                raise ValueError(f"exclude_item_idx has {len(exclude_item_idx)} lists for {B} queries")
            ex, exo = _csr(exclude_item_idx, dev, sort_unique=True)
        self._tiled_search(top_k)(q, ex, exo, idx, score)
        return idx, score

    def _tiled_search(self, top_k: int):
        """The one xfmr_topk_tiled call, as the function of a pass: what stays the same from chunk to chunk (library, table,
        norms, metric, ``top_k``) is bound here once. ``run(q, ex, exo, idx, score)`` then searches the non-empty contiguous
        float32 queries ``q`` (B, H) (:func:`_queries`; a row range of such a tensor is one) into ``idx`` (B, top_k) int64
        and ``score`` (B, top_k) float32; ``ex`` / ``exo``: the exclusions as int64 device CSR, each row sorted ascending
        (:func:`sorted_exclusion_csr`; B + 1 offsets, a view into a longer array with absolute values is fine), or None.
        Private: the callers allocate and shape every tensor themselves, nothing is checked here beyond ``N.ptr``."""
        lib, metric = N.load(), self.metric
        table, n_rows = N.ptr(self.table), self.table.shape[0]
        rnorm, sqnorm = (N.ptr(x) for x in self._norms())

        def run(q, ex, exo, idx, score):
            B, H = q.shape
            nbytes = lib.xfmr_topk_tiled_workspace(B, n_rows, top_k)
            ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=q.device)
            N.check(
                lib.xfmr_topk_tiled(N.ptr(q), table, rnorm, sqnorm, n_rows, B, H, N.ptr(ex), N.ptr(exo), top_k, metric,
                                    N.ptr(idx), N.ptr(score), N.ptr(ws), nbytes, N.stream()),
                "xfmr_topk_tiled",
            )

        return run

    @property
    def table_bf16(self) -> torch.Tensor:
        """The bf16 copy of the table that :meth:`search_refined`'s first pass reads (``xfmr_table_prepare``: round to
        nearest even, bit for bit ``table.to(torch.bfloat16)``), made once when the index was not given the model's."""
        if self._table_bf16 is None:
            from . import ops

            self._table_bf16 = ops.table_prepare(self.table)[1]
        return self._table_bf16

    @property
    def norm_bounds(self) -> tuple[float, float]:
        """(largest row norm, largest inverse row norm) over the items 1 .. n - 1, as host floats: the two table
        constants of :meth:`search_refined`'s error bound. Computed once (one read-back), from the f32 squared norms and
        rounded up by 2^-12 (the f32 sums are good to 2^-14 at H <= 1024); a non-finite table gives a non-finite bound,
        which certifies nothing."""
        if self._norm_bounds is None:
            if self.table.shape[0] < 2:
                self._norm_bounds = (0.0, 0.0)
            else:
                both = torch.stack([self.sqnorm[1:].max().sqrt(), self.rnorm[1:].max()]).double() * (1.0 + 2.0 ** -12)
                self._norm_bounds = tuple(float(x) for x in both.tolist())
        return self._norm_bounds

    def search_refined(self, embedding: torch.Tensor, exclude_item_idx=None, top_k: int = 20, refine_factor: int = 4,
                       exact: bool = True):
        """The search in the reference's two-stage form (``LanceIndex.search(...).refine_factor(4)``,
        ``index.py:214-255``) through xfmr_search_refined: a full scan on the bf16 matrix cores keeps the
        ``k_short = max(top_k, min(top_k * refine_factor, 128))`` best items per query, the exact search's f32 arithmetic
        re-ranks them, and ``certified[q]`` says that row q is provably :meth:`search_batch`'s row (DESIGN.md "Refined
        search": may be pessimistic, never wrong). Returns ``(idx (B, top_k) int64, score (B, top_k), certified (B,)
        bool)``; every score is the bits :meth:`search_batch` reports for the item.

        ``exact=True``: the rows that are not certified are searched again by :meth:`search_batch` with their own
        exclusions and patched in (one read-back of ``certified.all()``): idx and score are then :meth:`search_batch`'s
        for every row, bit for bit; ``certified`` still reports which rows the first call proved. ``exact=False``: the
        refined lists as they are, in the meaning of the reference's ``refine_factor``. ``XFMR_SEARCH=exact`` (read per
        call) takes :meth:`search_batch` for everything. top_k <= 128, H a multiple of 8."""
        if refine_factor < 1:
            raise ValueError(f"refine_factor must be at least 1; got {refine_factor}")
        q, B, H, dev = _queries(embedding)
        if exclude_item_idx is not None and len(exclude_item_idx) != B:
            raise ValueError(f"exclude_item_idx has {len(exclude_item_idx)} lists for {B} queries")
        if not refined_search_enabled():
            idx, score = self.search_batch(q, exclude_item_idx, top_k=top_k)
            return idx, score, torch.ones((B,), dtype=torch.bool, device=dev)
        idx = torch.empty((B, top_k), dtype=torch.int64, device=dev)
        score = torch.empty((B, top_k), dtype=torch.float32, device=dev)
        cert = torch.empty((B,), dtype=torch.uint8, device=dev)
        if B == 0:
            return idx, score, cert.bool()
        ex, exo = (None, None) if exclude_item_idx is None else _csr(exclude_item_idx, dev, sort_unique=True)
        k_short = max(top_k, min(top_k * refine_factor, 128))
        n_rows = self.table.shape[0]
        rnorm, sqnorm = self._norms()
        max_norm, max_rnorm = self.norm_bounds
        lib = N.load()
        nbytes = lib.xfmr_search_refined_workspace(B, n_rows, k_short)
        ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
        N.check(
            lib.xfmr_search_refined(N.ptr(q), N.ptr(self.table), N.ptr(self.table_bf16), N.ptr(rnorm), N.ptr(sqnorm),
                                    max_norm, max_rnorm, n_rows, B, H, N.ptr(ex), N.ptr(exo), top_k, k_short,
                                    self.metric, N.ptr(idx), N.ptr(score), N.ptr(cert), N.ptr(ws), nbytes, N.stream()),
            "xfmr_search_refined",
        )
        cert = cert.bool()
        if exact and not bool(cert.all()):
            rows = (~cert).nonzero().flatten()
            excl = None if exclude_item_idx is None else [exclude_item_idx[i] for i in rows.tolist()]
            sub_idx, sub_score = self.search_batch(q[rows], excl, top_k=top_k)
            idx[rows] = sub_idx
            score[rows] = sub_score
        return idx, score, cert

    def search_rows(self, embedding: torch.Tensor, exclude_item_idx=None, top_k: int = 20, search: str = "exact"):
        """``(idx, score)`` of :meth:`search_batch` (``search="exact"``) or of :meth:`search_refined` with
        ``exact=True`` (``search="refined"``): the same bits either way. What ``recommend_batch`` and the session
        recommender call with their ``search=`` option."""
        if search not in SEARCH_MODES:
            raise ValueError(f"search must be one of {SEARCH_MODES}; got {search!r}")
        if search == "refined":
            return self.search_refined(embedding, exclude_item_idx, top_k=top_k)[:2]
        return self.search_batch(embedding, exclude_item_idx, top_k=top_k)

    def rank_targets(self, embedding: torch.Tensor, targets_csr, exclude_csr=None, *, n_targets: int | None = None,
                     out: torch.Tensor | None = None, return_scores: bool = False):
        """The exact rank of every target among all eligible items (xfmr_target_ranks): no ranked list, no cutoff limit.

        ``targets_csr``: ``(flat, offsets)`` int64 DEVICE tensors, offsets with B + 1 entries (a view into a longer
        offsets array with absolute values is fine); ``exclude_csr``: the same form, each row SORTED ascending
        (:func:`sorted_exclusion_csr`), or None. Returns int32 ranks parallel to ``flat``: 1 = best; ``_native.RANK_NONE``
        for a target that is excluded, out of [1, n_items) or has a non-finite score. ``n_targets``: an upper bound on the
        entries the offsets cover (default: all of ``flat``; sizes the workspace); ``out``: an int32 tensor parallel to
        ``flat`` to write into (entries outside the offsets are left alone). ``return_scores=True`` also returns the
        targets' scores (float32, -inf where there is no rank): the bits :meth:`search_batch` reports for the item."""
        q, B, H, dev = _queries(embedding)
        tg, tgo = _check_csr("targets_csr", targets_csr, B)
        ex, exo = (None, None) if exclude_csr is None else _check_csr("exclude_csr", exclude_csr, B)
        if out is None:
            out = torch.full((tg.numel(),), N.RANK_NONE, dtype=torch.int32, device=dev)
        elif out.dtype != torch.int32 or out.numel() != tg.numel():
            raise ValueError(f"out must be int32 with {tg.numel()} entries")
        score = torch.full((tg.numel(),), float("-inf"), dtype=torch.float32, device=dev) if return_scores else None
        if B == 0:
            return (out, score) if return_scores else out
        nt = int(tg.numel() if n_targets is None else n_targets)
        n_rows = self.table.shape[0]
        rnorm, sqnorm = self._norms()
        lib = N.load()
        nbytes = lib.xfmr_target_ranks_workspace(B, n_rows, nt)
        ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
        N.check(
            lib.xfmr_target_ranks(N.ptr(q), N.ptr(self.table), N.ptr(rnorm), N.ptr(sqnorm), n_rows, B, H, N.ptr(ex),
                                  N.ptr(exo), N.ptr(tg), N.ptr(tgo), nt, self.metric, N.ptr(out), N.ptr(score), N.ptr(ws),
                                  nbytes, N.stream()),
            "xfmr_target_ranks",
        )
        return (out, score) if return_scores else out

    def _candidate_ranks(self, q, cand, ex, tg, out, tscore, cscore):
        """The one xfmr_candidate_ranks call: ``q`` from :func:`_queries`, the CSR pairs as checked by the callers
        (``ex`` and ``tg`` may be ``(None, None)``), the outputs allocated by them."""
        B, H = q.shape
        rnorm, sqnorm = self._norms()
        N.check(
            N.load().xfmr_candidate_ranks(N.ptr(q), N.ptr(self.table), N.ptr(rnorm), N.ptr(sqnorm), self.table.shape[0], B,
                                          H, N.ptr(cand[0]), N.ptr(cand[1]), N.ptr(ex[0]), N.ptr(ex[1]), N.ptr(tg[0]),
                                          N.ptr(tg[1]), self.metric, N.ptr(out), N.ptr(tscore), N.ptr(cscore), N.stream()),
            "xfmr_candidate_ranks",
        )

    def rank_among(self, embedding: torch.Tensor, candidates_csr, targets_csr, exclude_csr=None, *,
                   out: torch.Tensor | None = None, candidate_scores: bool = False):
        """The rank of every target among the query's GIVEN candidates (xfmr_candidate_ranks): the sampled-candidate
        protocol. ``candidates_csr``, ``targets_csr``, ``exclude_csr``: ``(flat, offsets)`` int64 DEVICE tensors as
        :meth:`rank_targets` takes them; each row of the candidates (``eval_rows.candidates_csr``) and of the exclusions
        SORTED ascending. A query's items are its distinct candidates and targets that are eligible (in [1, n_items),
        not excluded, finite score); a target's rank is 1 + those that beat it, so with every item as a candidate the
        result is :meth:`rank_targets`'. Returns int32 ranks parallel to the flat targets (``out``: a tensor to write
        into; entries outside the offsets are left alone), ``_native.RANK_NONE`` for a target that is not eligible.
        ``candidate_scores=True`` also returns the candidates' scores, parallel to the flat candidates (-inf: not
        eligible; float32, the bits :meth:`search_batch` reports for the item)."""
        q, B, _, dev = _queries(embedding)
        cand = _check_csr("candidates_csr", candidates_csr, B)
        tg = _check_csr("targets_csr", targets_csr, B)
        ex = (None, None) if exclude_csr is None else _check_csr("exclude_csr", exclude_csr, B)
        if out is None:
            out = torch.full((tg[0].numel(),), N.RANK_NONE, dtype=torch.int32, device=dev)
        elif out.dtype != torch.int32 or out.numel() != tg[0].numel():
            raise ValueError(f"out must be int32 with {tg[0].numel()} entries")
        cscore = torch.full((cand[0].numel(),), float("-inf"), dtype=torch.float32, device=dev) if candidate_scores else None
        if B > 0:
            self._candidate_ranks(q, cand, ex, tg, out, None, cscore)
        return (out, cscore) if candidate_scores else out

    def score_candidates(self, embedding: torch.Tensor, candidates_csr, exclude_csr=None) -> torch.Tensor:
        """The scores of each query's given candidates (the score-only form of xfmr_candidate_ranks; re-ranking):
        float32 parallel to the flat candidates, -inf for a candidate that is not eligible. CSR arguments as
        :meth:`rank_among`."""
        q, B, _, dev = _queries(embedding)
        cand = _check_csr("candidates_csr", candidates_csr, B)
        ex = (None, None) if exclude_csr is None else _check_csr("exclude_csr", exclude_csr, B)
        cscore = torch.full((cand[0].numel(),), float("-inf"), dtype=torch.float32, device=dev)
        if B > 0:
            self._candidate_ranks(q, cand, ex, (None, None), None, None, cscore)
        return cscore


def rank_metrics_sum(ranks: torch.Tensor, targets_csr, cutoffs, use: torch.Tensor | None = None, per_row: bool = False):
    """The seven metrics at every cutoff from the ranks of :meth:`ExactItemIndex.rank_targets`
    (xfmr_rank_metrics_sum), nothing read back: a device tensor ``(len(cutoffs), 8)`` of doubles -- per cutoff the sums of
    the METRIC_NAMES values over the rows that have a target and are used, and their number. ``ranks`` parallels the
    flat targets; ``targets_csr`` and ``use`` as :func:`retrieval_metrics_sum`; ``cutoffs``: positive ints in any order
    (also above the catalogue size); more than 8 take one call per 8. ``per_row=True`` returns ``(sums, values (B,
    len(cutoffs), 7), valid (B,) bool)``; for a cutoff K <= 128 the values are the bits of :func:`retrieval_metrics_sum`
    on :meth:`ExactItemIndex.search_batch`'s list of K."""
    cut = [int(k) for k in cutoffs]
    if not cut or any(k <= 0 or k >= 2**31 for k in cut):
        raise ValueError(f"cutoffs must be positive integers below 2^31; got {cutoffs!r}")
    tg, tgo = targets_csr
    B = tgo.numel() - 1
    dev = ranks.device
    if ranks.dtype != torch.int32 or ranks.numel() != tg.numel():
        raise ValueError(f"ranks must be int32 with one entry per target ({tg.numel()}); got {ranks.dtype}, {ranks.numel()}")
    if B < 1:
        raise ValueError("targets_csr has no row")
    use = _use_mask(use, B)
    nc = len(cut)
    sums = torch.empty((nc, 8), dtype=torch.float64, device=dev)
    vals = torch.empty((B, nc, len(METRIC_NAMES)), dtype=torch.float32, device=dev) if per_row else None
    valid = torch.empty((B,), dtype=torch.uint8, device=dev) if per_row else None
    lib = N.load()
    for c0 in range(0, nc, N.MAX_RANK_CUTOFFS):
        part = cut[c0 : c0 + N.MAX_RANK_CUTOFFS]
        whole = len(part) == nc
        part_vals = vals if whole or not per_row else torch.empty((B, len(part), len(METRIC_NAMES)), dtype=torch.float32,
                                                                  device=dev)
        nbytes = lib.xfmr_rank_metrics_sum_workspace(B, len(part))
        ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
        N.check(
            lib.xfmr_rank_metrics_sum(N.ptr(ranks.contiguous()), N.ptr(tg), N.ptr(tgo), N.ptr(use), B,
                                      (C.c_int32 * len(part))(*part), len(part), N.ptr(sums[c0 : c0 + len(part)]),
                                      N.ptr(part_vals), N.ptr(valid), N.ptr(ws), nbytes, N.stream()),
            "xfmr_rank_metrics_sum",
        )
        if per_row and not whole:
            vals[:, c0 : c0 + len(part)] = part_vals
    return (sums, vals, valid.bool()) if per_row else sums


def retrieval_metrics(rec_idx: torch.Tensor, target_idx, top_k: int):
    """(values (B,7) on the device in the order of METRIC_NAMES, valid (B,) bool)."""
    B, k = rec_idx.shape
    dev = rec_idx.device
    tg, tgo = _csr(target_idx, dev)
    out = torch.empty((B, len(METRIC_NAMES)), dtype=torch.float32, device=dev)
    valid = torch.empty((B,), dtype=torch.uint8, device=dev)
    N.check(
        N.load().xfmr_retrieval_metrics(N.ptr(rec_idx.contiguous()), N.ptr(tg), N.ptr(tgo), B, k, top_k, N.ptr(out),
                                        N.ptr(valid), N.stream()),
        "xfmr_retrieval_metrics",
    )
    return out, valid.bool()


def retrieval_metrics_sum(rec_idx: torch.Tensor, targets_csr, use: torch.Tensor | None = None, *, top_k: int,
                          per_row: bool = False):
    """:func:`retrieval_metrics` and its sums in one call (xfmr_retrieval_metrics_sum), nothing read back: returns the
    device tensor of 8 doubles -- ``[0..6]`` the sums of the METRIC_NAMES values over the rows that have a target and are
    used, ``[7]`` their number. ``targets_csr``: ``(flat, offsets)`` int64 DEVICE tensors (offsets: B + 1 entries; a view
    into a longer offsets array with absolute values is fine); ``use`` (B,) uint8 / bool on the device or None = every
    row. ``per_row=True`` returns ``(sums, values (B,7), valid (B,) bool)``: the bits of :func:`retrieval_metrics`."""
    B, k = rec_idx.shape
    dev = rec_idx.device
    tg, tgo = _check_csr("targets_csr", targets_csr, B, rows="rows", int64=False)
    use = _use_mask(use, B)
    sums = torch.empty((8,), dtype=torch.float64, device=dev)
    out = torch.empty((B, len(METRIC_NAMES)), dtype=torch.float32, device=dev) if per_row else None
    valid = torch.empty((B,), dtype=torch.uint8, device=dev) if per_row else None
    lib = N.load()
    nbytes = lib.xfmr_retrieval_metrics_sum_workspace(B)
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
    N.check(
        lib.xfmr_retrieval_metrics_sum(N.ptr(rec_idx.contiguous()), N.ptr(tg), N.ptr(tgo), N.ptr(use), B, k, top_k,
                                       N.ptr(sums), N.ptr(out), N.ptr(valid), N.ptr(ws), nbytes, N.stream()),
        "xfmr_retrieval_metrics_sum",
    )
    return (sums, out, valid.bool()) if per_row else sums


def compute_retrieval_metrics(rec_idx, target_idx, top_k: int) -> dict[str, torch.Tensor]:
    """``metrics.py:17-79`` for ONE ranked list (item indices instead of id strings): {} when there is no target."""
    rec = torch.as_tensor(rec_idx, dtype=torch.int64, device="cuda").reshape(1, -1)
    vals, valid = retrieval_metrics(rec, [list(target_idx)], top_k)
    if not bool(valid[0]):
        return {}
    return {name: vals[0, i] for i, name in enumerate(METRIC_NAMES)}
