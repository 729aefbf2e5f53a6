"""The host half of evaluation that depends on the rows and the config only (plain Python and numpy: no native library,
no device). ``trainer.py`` (``recommend`` .. ``evaluate``), ``evalset.py`` (the resident set), ``retrieval.py`` (the
searches) and ``models.py`` (``encode`` / ``encode_batch``) all read rows, build CSR arrays, pad histories and name their
results through the functions here, so the row format, the exclusion rule and the key names each stand in one place.
"""

from __future__ import annotations

import contextlib

import numpy as np

METRIC_NAMES = (  # metrics.py:7-15, in the order of XFMR_RM_*
    "retrieval_normalized_dcg", "retrieval_average_precision", "retrieval_auroc", "retrieval_precision",
    "retrieval_recall", "retrieval_hit_rate", "retrieval_reciprocal_rank",
)
MAX_TILED_TOP_K = 128  # xfmr_topk_tiled's longest list


# ------------------------------------------------------------------------------------------------ ids and rows
def lookup_rows(id2idx, item_ids) -> list[int]:
    """Item ids -> table rows through ``id2idx`` (a dict, or a pandas ``Series`` indexed by id); unknown ids are dropped
    (``models.py:347-364``). One membership test per id; a dict is read once per known id, a ``Series`` once for all of
    them (with a repeated index label it gives every matching row, as the reference's vectorised read does)."""
    if hasattr(id2idx, "index"):
        known = [i for i in item_ids if i in id2idx.index]
        return [int(v) for v in id2idx[known].to_numpy()] if known else []
    return [int(id2idx[i]) for i in item_ids if i in id2idx]


def positive_target_ids(row) -> list:
    """The target ids of one row (the reference's format) whose ``label`` is true."""
    return [i for i, l in zip(row["target"]["item_id"], row["target"]["label"]) if l]


def read_rows(rows, to_idx) -> tuple[list, list]:
    """``rows`` in the reference's format (``{"history": {"item_id"}, "target": {"item_id", "label"}}``) -> ``(histories,
    positive targets)``, each a list of lists of table rows. ``to_idx``: ids -> rows (the module's ``_to_idx_or_empty``);
    it sees every id once."""
    rows = list(rows)
    return ([to_idx(list(r["history"]["item_id"])) for r in rows], [to_idx(positive_target_ids(r)) for r in rows])


# ------------------------------------------------------------------------------------------------ arrays
def flat_csr(lists, sort_unique: bool = False) -> tuple[np.ndarray, np.ndarray]:
    """Lists of table rows -> ``(flat int64, offsets int64 with len(lists) + 1 entries)``. ``sort_unique``: each list
    sorted ascending with repeats dropped (what the retrieval kernels binary-search as exclusions), by one sort of
    (list, item) pairs.

    The trailing-element rule: ``flat`` holds exactly ``offsets[-1]`` entries, except that a CSR without any entry gets ONE
    placeholder element (0, never read: every offset is 0), so that the array always has an address to hand to a kernel."""
    parts = [np.asarray(x, dtype=np.int64).reshape(-1) for x in lists]
    off = np.zeros(len(parts) + 1, dtype=np.int64)
    np.cumsum([p.size for p in parts], out=off[1:])
    flat = np.concatenate(parts) if off[-1] else np.zeros(0, dtype=np.int64)
    if sort_unique:
        flat, off = sort_unique_rows(flat, off)
    return (flat if flat.size else np.zeros(1, dtype=np.int64)), off


def sort_unique_rows(flat: np.ndarray, off: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """The CSR ``(flat, off)`` with every row sorted ascending and its repeats dropped (``flat`` holds ``off[-1]`` entries
    on both sides: no placeholder)."""
    n = off.size - 1
    row = np.repeat(np.arange(n, dtype=np.int64), np.diff(off))
    o = np.lexsort((flat[: off[-1]], row))
    flat, row = flat[o], row[o]
    first = np.ones(flat.size, dtype=bool)
    first[1:] = (flat[1:] != flat[:-1]) | (row[1:] != row[:-1])
    new_off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(row[first], minlength=n), out=new_off[1:])
    return flat[first], new_off


def pad_histories(lengths, flat) -> np.ndarray:
    """The right-padded ``(len(lengths), max(lengths))`` int64 array (padding row 0) of the histories that lie back to back
    in ``flat``."""
    lengths = np.asarray(lengths, dtype=np.int64)
    width = int(lengths.max())
    out = np.zeros((lengths.size, width), dtype=np.int64)
    out[np.arange(width)[None, :] < lengths[:, None]] = flat
    return out


# ------------------------------------------------------------------------------------------------ sampled candidates
def candidates_csr(lists) -> tuple[np.ndarray, np.ndarray]:
    """Explicit per-row candidate lists (table rows) as xfmr_candidate_ranks takes them: each row sorted ascending,
    repeats dropped (:func:`flat_csr`)."""
    return flat_csr(lists, sort_unique=True)


def map_candidates(candidates, to_idx) -> list:
    """Per-row lists of candidate item IDS -> lists of table rows through ``to_idx`` (the module's ``_to_idx_or_empty``, or
    ``lambda ids: lookup_rows(id2idx, ids)``): unknown ids are dropped, as the histories' are."""
    return [to_idx(list(c)) for c in candidates]


def sample_eval_negatives(hist_lists, target_lists, n_items: int, num_negatives: int, seed: int,
                          weights=None) -> tuple[np.ndarray, np.ndarray]:
    """The negatives of the sampled-candidate protocol (one held-out item against ``num_negatives`` sampled ones), as a
    sorted-unique CSR ``(flat int64, offsets int64)`` over the rows of ``hist_lists`` / ``target_lists`` (table rows).

    Row i draws ``num_negatives`` DISTINCT items from ``1 .. n_items - 1`` minus (its history U its targets): uniformly,
    or with ``weights`` (``n_items`` non-negative numbers by table row, e.g. popularity counts) in proportion to the
    weights without replacement -- an item of weight 0 is never drawn. A row with fewer items to draw from than asked
    takes all of them. The generator of row i is keyed by ``(seed, i)`` alone: a row's negatives do not depend on which
    other rows there are, on their order or on how the rows are batched."""
    n_items, k = int(n_items), int(num_negatives)
    if n_items < 1 or k < 0 or int(seed) < 0:
        raise ValueError(f"n_items must be >= 1, num_negatives and seed >= 0; got {n_items}, {num_negatives}, {seed}")
    if len(hist_lists) != len(target_lists):
        raise ValueError(f"{len(hist_lists)} histories for {len(target_lists)} target lists")
    w = None
    if weights is not None:
        w = np.asarray(weights, dtype=np.float64).reshape(-1)
        if w.size != n_items or not np.isfinite(w).all() or (w < 0).any():
            raise ValueError(f"weights must be {n_items} finite non-negative numbers")
    free = np.empty(n_items, dtype=bool)
    parts = []
    for i, (h, t) in enumerate(zip(hist_lists, target_lists)):
        free[:] = True if w is None else w > 0
        free[0] = False
        for own in (h, t):
            own = np.asarray(own, dtype=np.int64).reshape(-1)
            free[own[(own >= 0) & (own < n_items)]] = False
        pool = np.flatnonzero(free)
        if pool.size > k:
            rng = np.random.default_rng((int(seed), i))
            p = None if w is None else w[pool] / w[pool].sum()
            pool = np.sort(rng.choice(pool, size=k, replace=False, p=p))
        parts.append(pool.astype(np.int64))
    return flat_csr(parts)


# ------------------------------------------------------------------------------------------------ config rules
def check_tiled_top_k(top_k: int, hint: str = "") -> None:
    """The one refusal of a list longer than xfmr_topk_tiled returns."""
    if int(top_k) > MAX_TILED_TOP_K:
        raise ValueError(f"top_k = {top_k}: the tiled top-k (xfmr_topk_tiled) returns at most {MAX_TILED_TOP_K} items per "
                         f"row{hint}")


def normalize_cutoffs(cutoffs) -> tuple[int, ...]:
    """The cutoffs as given, repeats dropped, each a positive int below 2^31 (ValueError otherwise)."""
    if isinstance(cutoffs, (int, np.integer)) and not isinstance(cutoffs, bool):
        cutoffs = (cutoffs,)
    out = []
    for k in cutoffs:
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 0 < int(k) < 2**31:
            raise ValueError(f"cutoffs must be positive integers below 2^31; got {k!r}")
        if int(k) not in out:
            out.append(int(k))
    if not out:
        raise ValueError("cutoffs is empty")
    return tuple(out)


def eval_cutoffs(cutoffs, top_k: int) -> tuple[int, ...]:
    """:func:`normalize_cutoffs` with ``top_k`` (the cutoff of the plain keys) appended when it is missing."""
    cut = normalize_cutoffs(cutoffs)
    return cut if int(top_k) in cut else cut + (int(top_k),)


def metrics_dict(stage: str, sums, cutoffs=None, top_k: int | None = None) -> dict:
    """What every evaluator returns, from its sums (per record: the seven METRIC_NAMES sums and the number of rows).

    Without ``cutoffs``: ``sums`` is 8 numbers -> ``{stage}/<metric>`` means and ``{stage}/num_rows``. With ``cutoffs``:
    ``sums`` is ``(len(cutoffs), 8)`` -> ``{stage}/<metric>@<K>`` per cutoff in cutoff order, and right behind the keys of
    cutoff ``top_k`` the plain keys (the same values) and ``{stage}/num_rows``. Means are Python floats, NaN when no row
    counts; ``num_rows`` is an int."""
    sums = np.asarray(sums, dtype=np.float64)
    out = {}
    for K, s in zip((top_k,) if cutoffs is None else cutoffs, sums.reshape(-1, 8)):
        n = int(s[7])
        means = [float(s[i] / n) if n else float("nan") for i in range(len(METRIC_NAMES))]
        if cutoffs is not None:
            out.update((f"{stage}/{name}@{K}", v) for name, v in zip(METRIC_NAMES, means))
        if cutoffs is None or K == top_k:
            out.update((f"{stage}/{name}", v) for name, v in zip(METRIC_NAMES, means))
            out[f"{stage}/num_rows"] = n
    return out


# ------------------------------------------------------------------------------------------------ the eval-mode guard
@contextlib.contextmanager
def eval_mode(module):
    """``module.eval()`` for the block; the ``training`` flag it had is put back afterwards, also when the block raises."""
    was_training = module.training
    module.eval()
    try:
        yield module
    finally:
        module.train(was_training)
