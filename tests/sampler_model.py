"""Host statement of what the two sequence samplers (csrc/sampler.hip: ``xfmr_seq_sample``, ``xfmr_seq_sample_rows``) put out,
value for value, in numpy uint32 arithmetic. Both are integer-only and counter-based, so a test can say what a launch must
write without asking any kernel for it (the precedent: tests/dropout_model.py for the dropout masks).

Taken from the library, as its contract (sampler.hip's header comments, csrc/common.h):

    h(x)         = xf_hash32:  x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16     (mod 2^32)
    below(r, n)  = (r * n) >> 32                                                     a uniform integer in [0, n)
    xfmr_seq_sample       stream(purpose, ctr) = SeqStream{seed, row}.draw(purpose, ctr):
                          x = h(lo32(seed) ^ hi32(seed) * 0x9e3779b9 ^ lo32(row) * 0x85ebca6b)
                          x = h(x ^ purpose * 0xc2b2ae35 ^ ctr);  h(x + 0x27d4eb2f * ctr)
    xfmr_seq_sample_rows  stream(purpose, ctr) = RowsStream{row_key(seed, epoch, row)}.draw(purpose, ctr):
                          a = h(lo32(seed) ^ h(hi32(seed) + 0x9e3779b9));  a = h(a ^ lo32(epoch) * 0x85ebca6b)
                          a = h(a + hi32(epoch) * 0xc2b2ae35);  b = h(a ^ 0x27d4eb2f)
                          k0 = h(a ^ lo32(row));  k1 = h(b + hi32(row) * 0x165667b1 + lo32(row) * 0x9e3779b9)
                          x = h(k0 ^ purpose * 0xc2b2ae35 ^ ctr);  h((x ^ k1) + 0x27d4eb2f * ctr)
    purposes     1 positions, 2 positives, 3 negatives (and the with-replacement regime of `rows`), 16 + round the rejection
                 rounds of `rows`, 4 its exact path
    regimes      `rows`: A < cnt with replacement; A >= 4 cnt rounds (32 of them); otherwise exact.  `xfmr_seq_sample`: 64
                 rejected attempts per slot are drawn again, the 65th walks forward

Everything else says WHAT is selected, never how a kernel finds it (no bit-by-bit threshold search, no ballots, no sorting
network, no per-thread loops):

    positions    m = n - 1, L = min(max_seq_length, width). m <= L: all of 0..m-1. Otherwise the L positions with the smallest
                 (stream(1, i), i), in ascending position. cnt = min(max(m, 0), L).
    positives    slot k at position p: candidates = positive-labelled positions in (p, min(p + lookahead, n - 1)] (lookahead
                 0: (p, n - 1]); none -> 0, else h[candidates[below(stream(2, k), c)]].
    negatives    xfmr_seq_sample   one counter per row from 0 across the slots; a draw is 1 + below(stream(3, ctr++), n_items),
                                   rejected if in the history (unless nothing else exists: any_item) or already chosen (unless
                                   replace); after the 65th rejected draw of a slot, the first admissible item walking forward
                                   cyclically from that draw.
                 rows              D distinct in-range history items, A = n_items - D (0 -> D := 0, A = n_items); "rank j" is
                                   the j-th smallest of {1..n_items} minus the history.
                                   A < cnt:        slot k takes rank below(stream(3, k), A)
                                   A >= 4 cnt:     rounds r = 0..31: every open slot draws below(stream(16 + r, k), A) and
                                                   closes unless a filled slot, or an open slot of lower index, holds that
                                                   rank; a slot still open after 32 rounds -> the exact path for the row
                                   otherwise:      the cnt ranks with the smallest (stream(4, rank), rank), in that order
    zero rows    both: lengths outside 1..max_history. `rows` also: batch rows past n_order, row indices outside the dataset
                 (`xfmr_seq_sample` is given no row count and does not check the index). Zeros, length 0.

The core functions work on ONE history and a batch of R streams ("lanes": the same row under R different (seed, row id)
keys), so that a frequency table over 2e5 draws is a handful of array operations; ``seq_sample`` / ``rows_sample`` wrap them
into what one launch over a batch of dataset rows writes. Every call also returns a trace (which regime ran, rounds used,
rejections by reason, whether the walk-forward ran, whether a key tie sat exactly on a selection threshold and which index
won) with which a test proves that a case reaches the branch it is named for."""

from __future__ import annotations

import numpy as np

M32 = 0xFFFFFFFF
M64 = 0xFFFFFFFFFFFFFFFF
P_POSITIONS, P_POSITIVES, P_NEGATIVES, P_EXACT, P_ROUND0 = 1, 2, 3, 4, 16
REJECT_ROUNDS = 32      # rounds of `rows` before the exact path takes over
REJECT_ATTEMPTS = 64    # rejected draws of a slot of xfmr_seq_sample that are drawn again; the next one walks forward
SETDIFF_LIMIT = 10**6   # catalogues up to here: rank -> item by np.setdiff1d; beyond: the closed form
REPLACE, ROUNDS, EXACT, ROUNDS_THEN_EXACT = "replace", "rounds", "exact", "rounds+exact"


def h32(x):
    """xf_hash32 on uint32 arrays (wrap-around arithmetic)."""
    x = np.array(x, dtype=np.uint32, copy=True, ndmin=1)
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x7FEB352D)
    x ^= x >> np.uint32(15)
    x *= np.uint32(0x846CA68B)
    x ^= x >> np.uint32(16)
    return x


def below(r, n):
    """(r * n) >> 32: uint32 draws -> integers in [0, n). ``n`` may be an array (0 where the result is not used)."""
    return ((np.asarray(r, dtype=np.uint64) * np.asarray(n, dtype=np.uint64)) >> np.uint64(32)).astype(np.int64)


def _lanes(seed, row):
    seed = np.atleast_1d(np.asarray([int(s) & M64 for s in np.atleast_1d(seed).tolist()], dtype=np.uint64))
    row = np.atleast_1d(np.asarray(row, dtype=np.int64)).astype(np.uint64)
    seed, row = np.broadcast_arrays(seed, row)
    lo = lambda v: (v & np.uint64(M32)).astype(np.uint32)  # noqa: E731
    hi = lambda v: (v >> np.uint64(32)).astype(np.uint32)  # noqa: E731
    return lo(seed), hi(seed), lo(row), hi(row)


class _Stream:
    """R lanes of a counter-based stream. ``draw(purpose, ctr)``: ctr [C] -> [R, C]; ``draw_each``: ctr [R] -> [R]."""

    lanes: int

    def _at(self, purpose, ctr, sel):
        raise NotImplementedError

    def draw(self, purpose, ctr):
        ctr = np.asarray(ctr, dtype=np.int64).astype(np.uint32)
        return self._at(purpose, ctr[None, :], (slice(None), None))

    def draw_each(self, purpose, ctr, lanes=None):
        ctr = np.asarray(ctr, dtype=np.int64).astype(np.uint32)
        return self._at(purpose, ctr, slice(None) if lanes is None else lanes)


class SeqStream(_Stream):
    """SeqStream{seed, row}.draw(purpose, ctr) of xfmr_seq_sample for broadcast arrays of seeds and dataset rows."""

    def __init__(self, seed, row):
        slo, shi, rlo, _ = _lanes(seed, row)
        self.x = h32(slo ^ (shi * np.uint32(0x9E3779B9)) ^ (rlo * np.uint32(0x85EBCA6B)))
        self.lanes = self.x.size

    def _at(self, purpose, ctr, sel):
        x = h32(self.x[sel] ^ np.uint32((purpose * 0xC2B2AE35) & M32) ^ ctr)
        return h32(x + np.uint32(0x27D4EB2F) * ctr)


class RowsStream(_Stream):
    """RowsStream{row_key(seed, epoch, row)}.draw(purpose, ctr) of xfmr_seq_sample_rows; ``epoch`` is one 64-bit number."""

    def __init__(self, seed, epoch, row):
        slo, shi, rlo, rhi = _lanes(seed, row)
        epoch = int(epoch) & M64
        a = h32(slo ^ h32(shi + np.uint32(0x9E3779B9)))
        a = h32(a ^ np.uint32(((epoch & M32) * 0x85EBCA6B) & M32))
        a = h32(a + np.uint32(((epoch >> 32) * 0xC2B2AE35) & M32))
        b = h32(a ^ np.uint32(0x27D4EB2F))
        self.k0 = h32(a ^ rlo)
        self.k1 = h32(b + rhi * np.uint32(0x165667B1) + rlo * np.uint32(0x9E3779B9))
        self.lanes = self.k0.size

    def _at(self, purpose, ctr, sel):
        x = h32(self.k0[sel] ^ np.uint32((purpose * 0xC2B2AE35) & M32) ^ ctr)
        return h32((x ^ self.k1[sel]) + np.uint32(0x27D4EB2F) * ctr)


# --------------------------------------------------------------------------------------------------- selection by key
def smallest_keys(keys, want):
    """keys [R, m] -> the indices of the ``want`` smallest (key, index) pairs of every lane, in (key, index) order [R, want],
    and the tie at the selection threshold: (index taken, lowest index left out with the same key), -1 / -1 without one."""
    R, m = keys.shape
    order = np.argsort(keys, axis=1, kind="stable")
    took, left = np.full(R, -1, dtype=np.int64), np.full(R, -1, dtype=np.int64)
    if 0 < want < m:
        last, nxt = order[:, want - 1], order[:, want]
        tied = keys[np.arange(R), last] == keys[np.arange(R), nxt]
        took[tied], left[tied] = last[tied], nxt[tied]
    return order[:, :want], took, left


def positions(stream, n, L):
    """[R, cnt] sampled positions, ascending, and the threshold tie (taken, left)."""
    m = n - 1
    cnt = min(max(m, 0), L)
    if m <= L:
        none = np.full(stream.lanes, -1, dtype=np.int64)
        return np.tile(np.arange(cnt, dtype=np.int64), (stream.lanes, 1)), none, none
    sel, took, left = smallest_keys(stream.draw(P_POSITIONS, np.arange(m)), L)
    return np.sort(sel, axis=1), took, left


def candidates(lab, p, lookahead):
    """The positive-labelled positions a slot at position ``p`` may take its positive from."""
    n = len(lab)
    last = min(p + lookahead, n - 1) if lookahead > 0 else n - 1
    return np.array([i for i in range(p + 1, last + 1) if lab[i]], dtype=np.int64)


def positives(stream, h, lab, pos, lookahead):
    """[R, cnt] positives of the slots at positions ``pos`` [R, cnt]."""
    R, cnt = pos.shape
    out = np.zeros((R, cnt), dtype=np.int64)
    if cnt == 0:
        return out
    uniq = np.unique(pos)
    cands = [candidates(lab, int(p), lookahead) for p in uniq]
    table = np.zeros((len(uniq), max(1, max(len(c) for c in cands))), dtype=np.int64)
    for i, c in enumerate(cands):
        table[i, : len(c)] = c
    at = np.searchsorted(uniq, pos)
    c = np.array([len(x) for x in cands], dtype=np.int64)[at]
    pick = below(stream.draw(P_POSITIVES, np.arange(cnt)), c)
    return np.where(c > 0, np.asarray(h, dtype=np.int64)[table[at, pick]], 0)


# --------------------------------------------------------------------------------------------------- admissible items
def history_items(h, n_items):
    """The distinct history items that are catalogue items (1..n_items), ascending."""
    h = np.asarray(h, dtype=np.int64)
    return np.unique(h[(h >= 1) & (h <= n_items)])


def rank_to_item_setdiff(items, n_items, ranks):
    return np.setdiff1d(np.arange(1, n_items + 1, dtype=np.int64), items)[ranks]


def rank_to_item_closed(items, n_items, ranks):
    """Item ``items[i]`` has ``items[i] - 1 - i`` admissible items below it: rank j sits behind every history item with at
    most j of them."""
    ranks = np.asarray(ranks, dtype=np.int64)
    return ranks + 1 + np.searchsorted(items - 1 - np.arange(len(items)), ranks, side="right")


def rank_to_item(items, n_items, ranks):
    f = rank_to_item_setdiff if n_items <= SETDIFF_LIMIT else rank_to_item_closed
    return f(np.asarray(items, dtype=np.int64), int(n_items), ranks)


# --------------------------------------------------------------------------------------------------- negatives
def negatives_seq(stream, h, cnt, n_items):
    """xfmr_seq_sample: [R, cnt] negatives and ``walked`` [R]: slots of the lane that went through the walk-forward."""
    R = stream.lanes
    in_hist = np.zeros(n_items + 1, dtype=bool)
    in_hist[history_items(h, n_items)] = True
    n_cand = n_items - int(in_hist.sum())
    any_item = n_cand == 0
    replace = n_items < cnt if any_item else n_cand < cnt
    forbidden = np.zeros(n_items + 1, dtype=bool) if any_item else in_hist
    chosen = np.zeros((R, n_items + 1), dtype=bool)
    ctr = np.zeros(R, dtype=np.int64)
    neg = np.zeros((R, cnt), dtype=np.int64)
    walked = np.zeros(R, dtype=np.int64)
    for k in range(cnt):
        x = np.zeros(R, dtype=np.int64)
        open_ = np.arange(R)
        for _ in range(REJECT_ATTEMPTS + 1):
            if open_.size == 0:
                break
            d = 1 + below(stream.draw_each(P_NEGATIVES, ctr[open_], open_), n_items)
            ctr[open_] += 1
            x[open_] = d
            bad = forbidden[d] | (chosen[open_, d] & (not replace))
            open_ = open_[bad]
        for lane in open_:  # the 65th draw was rejected too
            for s in range(n_items):
                y = 1 + (x[lane] - 1 + s) % n_items
                if not (forbidden[y] or (chosen[lane, y] and not replace)):
                    x[lane] = y
                    break
            walked[lane] += 1
        chosen[np.arange(R), x] = True
        neg[:, k] = x
    return neg, walked


def negatives_rows(stream, h, cnt, n_items, rank_fn=None):
    """xfmr_seq_sample_rows: [R, cnt] negatives and the trace arrays. ``rank_fn(draws, A)``: how a draw becomes a rank (the
    frequency tests put a biased one in to prove that they would notice)."""
    rank_fn = below if rank_fn is None else rank_fn
    R = stream.lanes
    items = history_items(h, n_items)
    A = n_items - len(items)
    if A == 0:
        items, A = items[:0], n_items
    slots = np.arange(cnt)
    tr = {"regime": np.full(R, EXACT, dtype=object), "rounds": np.zeros(R, dtype=np.int64),
          "rejected_by_filled": np.zeros(R, dtype=np.int64), "rejected_by_lower": np.zeros(R, dtype=np.int64),
          "neg_tie_took": np.full(R, -1, dtype=np.int64), "neg_tie_left": np.full(R, -1, dtype=np.int64), "A": A}
    ranks = np.zeros((R, cnt), dtype=np.int64)
    exact = np.arange(R)
    if cnt == 0:
        return ranks, tr
    if A < cnt:
        tr["regime"][:] = REPLACE
        ranks = rank_fn(stream.draw(P_NEGATIVES, slots), A)
        exact = exact[:0]
    elif A >= 4 * cnt:
        tr["regime"][:] = ROUNDS
        filled = np.zeros((R, cnt), dtype=bool)
        lower = slots[None, :] < slots[:, None]  # [k, q]: q < k
        for r in range(REJECT_ROUNDS):
            live = np.flatnonzero(~filled.all(axis=1))
            if live.size == 0:
                break
            tr["rounds"][live] += 1
            d = rank_fn(stream.draw(P_ROUND0 + r, slots), A)
            ranks = np.where(filled, ranks, d)
            for c0 in range(0, live.size, 4096):
                ln = live[c0 : c0 + 4096]
                v, f = ranks[ln], filled[ln]
                same = v[:, :, None] == v[:, None, :]  # [lane, k, q]
                by_filled = (same & f[:, None, :]).any(axis=2) & ~f
                by_lower = (same & ~f[:, None, :] & lower[None]).any(axis=2) & ~f
                tr["rejected_by_filled"][ln] += by_filled.sum(axis=1)
                tr["rejected_by_lower"][ln] += by_lower.sum(axis=1)
                filled[ln] = f | ~(by_filled | by_lower)
        exact = np.flatnonzero(~filled.all(axis=1))
        tr["regime"][exact] = ROUNDS_THEN_EXACT
    if exact.size:
        sub = stream if exact.size == R else _Sub(stream, exact)
        sel, took, left = smallest_keys(sub.draw(P_EXACT, np.arange(A)), cnt)
        ranks[exact] = sel
        tr["neg_tie_took"][exact], tr["neg_tie_left"][exact] = took, left
    return rank_to_item(items, n_items, ranks), tr


class _Sub(_Stream):
    def __init__(self, stream, lanes):
        self.s, self.idx, self.lanes = stream, lanes, len(lanes)

    def _at(self, purpose, ctr, sel):
        if isinstance(sel, tuple):
            return self.s._at(purpose, ctr, (self.idx, None))
        return self.s._at(purpose, ctr, self.idx[sel])


# --------------------------------------------------------------------------------------------------- one row, R lanes
def sample_row(stream, kind, h, lab, *, max_seq_length, width, lookahead, n_items, rank_fn=None):
    """What R lanes of ``stream`` sample from the row (h, lab): hist, pos, neg [R, width] right-padded with 0, cnt, trace."""
    h, lab = np.asarray(h, dtype=np.int64), np.asarray(lab).astype(bool)
    n, R = len(h), stream.lanes
    L = min(max_seq_length, width)
    p, took, left = positions(stream, n, L)
    cnt = p.shape[1]
    out = np.zeros((3, R, width), dtype=np.int64)
    out[0, :, :cnt] = h[p]
    out[1, :, :cnt] = positives(stream, h, lab, p, lookahead)
    if kind == "seq":
        out[2, :, :cnt], walked = negatives_seq(stream, h, cnt, n_items)
        tr = {"walked": walked}
    else:
        out[2, :, :cnt], tr = negatives_rows(stream, h, cnt, n_items, rank_fn)
    tr.update(positions=p, pos_tie_took=took, pos_tie_left=left, cnt=cnt)
    return out[0], out[1], out[2], cnt, tr


def _lane0(tr):
    return {k: (v[0] if isinstance(v, np.ndarray) and v.ndim >= 1 else v) for k, v in tr.items()}


# --------------------------------------------------------------------------------------------------- one launch
def seq_sample(hs, ls, rows, seed, *, max_seq_length, width, lookahead, n_items, max_history=None):
    """xfmr_seq_sample over dataset rows ``rows`` (all inside the dataset: the entry does not check them): hist, pos, neg
    [B, width] and one trace per batch row (None for a row written as zeros)."""
    max_history = max(len(h) for h in hs) if max_history is None else max_history
    out = np.zeros((3, len(rows), width), dtype=np.int64)
    traces = [None] * len(rows)
    for b, r in enumerate(rows):
        if not 1 <= len(hs[r]) <= max_history:
            continue
        a = sample_row(SeqStream(seed, int(r)), "seq", hs[r], ls[r], max_seq_length=max_seq_length, width=width,
                       lookahead=lookahead, n_items=n_items)
        out[0, b], out[1, b], out[2, b] = a[0][0], a[1][0], a[2][0]
        traces[b] = _lane0(a[4])
    return out[0], out[1], out[2], traces


def rows_sample(hs, ls, order, batch, *, first=0, seed=0, epoch=0, max_seq_length, width, lookahead, n_items,
                max_history=None):
    """xfmr_seq_sample_rows over ``order[first : first + batch]``: hist, pos, neg [batch, width], len [batch] and one trace
    per batch row (None for a row written as zeros)."""
    max_history = max(len(h) for h in hs) if max_history is None else max_history
    out = np.zeros((3, batch, width), dtype=np.int64)
    ln = np.zeros(batch, dtype=np.int32)
    traces = [None] * batch
    for b in range(batch):
        if first + b >= len(order):
            continue
        r = int(order[first + b])
        if not 0 <= r < len(hs) or not 1 <= len(hs[r]) <= max_history:
            continue
        a = sample_row(RowsStream(seed, epoch, r), "rows", hs[r], ls[r], max_seq_length=max_seq_length, width=width,
                       lookahead=lookahead, n_items=n_items)
        out[0, b], out[1, b], out[2, b], ln[b] = a[0][0], a[1][0], a[2][0], a[3]
        traces[b] = _lane0(a[4])
    return out[0], out[1], out[2], ln, traces
