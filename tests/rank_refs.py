"""Host references for the rank path (TEST INFRASTRUCTURE): every target's rank among the eligible items, and the seven
retrieval metrics written from ranks.

An item j is eligible for a query when ``1 <= j < n_rows``, j is not excluded and its score is finite; ``rank(t) = 1 +``
the eligible items that beat t (higher score first, then the lower index). ``metrics_from_ranks`` restates
``oracle.metrics.compute_retrieval_metrics`` as a function of the ranks of the row's distinct targets and their number
(tests/test_ranks_host.py holds the two to each other)."""

from __future__ import annotations

import math

import numpy as np

RANK_NONE = 0x7FFFFFFF
NAMES = ("retrieval_normalized_dcg", "retrieval_average_precision", "retrieval_auroc", "retrieval_precision",
         "retrieval_recall", "retrieval_hit_rate", "retrieval_reciprocal_rank")


def scores(query, table, metric):
    """float64 scores of one query against every table row (exact for small-integer inputs)."""
    q = np.asarray(query, dtype=np.float64)
    t = np.asarray(table, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        dot = t @ q
        if metric == "cosine":
            return dot / (max(np.linalg.norm(q), 1e-8) * np.maximum(np.linalg.norm(t, axis=1), 1e-8))
        if metric == "dot":
            return dot
        return 1.0 - ((t - q[None]) ** 2).sum(1)


def ranks_from_scores(s, exclude, targets):
    """Ranks of ``targets`` (any ints, repeats allowed) given one query's score vector ``s`` over the table rows."""
    s = np.asarray(s, dtype=np.float64)
    n = s.size
    ok = np.isfinite(s)
    ok[0] = False
    for x in exclude or ():
        if 0 <= int(x) < n:
            ok[int(x)] = False
    idx = np.flatnonzero(ok)
    order = idx[np.lexsort((idx, -s[idx]))]  # score descending, then index ascending, over the eligible set
    place = np.full(n, RANK_NONE, dtype=np.int64)
    place[order] = np.arange(1, order.size + 1)
    return [int(place[t]) if 0 <= int(t) < n else RANK_NONE for t in targets]


def metrics_from_ranks(ranks, targets, K):
    """The seven metrics at cutoff K from the ranks of a row's target entries (parallel to ``targets``, RANK_NONE = not
    eligible); {} for a row without a target."""
    if len(targets) == 0:
        return {}
    by_target = {}
    for t, r in zip(targets, ranks):
        by_target[int(t)] = int(r)
    n_pos = len(by_target)
    pos = sorted(r for r in by_target.values() if r != RANK_NONE and r <= K)
    hits = len(pos)
    dcg = sum(1.0 / math.log2(r + 1) for r in pos)
    idcg = sum(1.0 / math.log2(i + 2) for i in range(min(n_pos, K)))
    auroc = 0.0
    if hits > 0 and K - hits > 0:
        auroc = sum((K - p) - (hits - 1 - j) for j, p in enumerate(pos)) / (hits * (K - hits))
    return {
        "retrieval_normalized_dcg": dcg / idcg if idcg > 0 else 0.0,
        "retrieval_average_precision": float(np.mean([(j + 1) / p for j, p in enumerate(pos)])) if pos else 0.0,
        "retrieval_auroc": auroc,
        "retrieval_precision": hits / K,
        "retrieval_recall": hits / n_pos,
        "retrieval_hit_rate": 1.0 if hits > 0 else 0.0,
        "retrieval_reciprocal_rank": 1.0 / pos[0] if pos else 0.0,
    }
