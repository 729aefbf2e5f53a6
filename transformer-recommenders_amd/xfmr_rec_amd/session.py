"""Serving sessions: append events to cached histories instead of re-encoding them.

The reference serves ``recommend_with_query`` by encoding the user's whole history at every call (``service.py`` ->
``Model.embed``). Its encoder is causal with absolute positions, so row t of ``token_embeddings`` depends on rows 0 .. t only
and no earlier row changes when an event is appended. :class:`SessionEncoder` keeps every layer's K and V per session on
the device (``include/xfmr_session.h``) and runs only the new rows; :class:`SessionRecommender` puts keys, slots, pooling
and the item search around it. :func:`session_plan` and :func:`check_rows` are the host logic, in plain Python (no torch, no
device), so the window rule can be tested anywhere.
"""

from __future__ import annotations


def session_plan(lengths, new_items, max_len: int) -> dict:
    """What to run for a batch of appended events. ``lengths``: {slot: rows the slot holds}; ``new_items``: {slot: [table
    rows]} or a list of (slot, rows) pairs -- several pairs of one slot are taken in order; ``max_len``: the window
    (``max_seq_length``). Returns, per slot with at least one new item, one of

    * ``("append", p, items)``: write ``items`` at positions p, p + 1, ... (p = the slot's length); nothing stored changes;
    * ``("rebuild", keep, items)``: the slot becomes its last ``keep`` stored items followed by ``items``, ``max_len`` rows
      in all, written from position 0. The reference encodes the last ``max_seq_length`` events with positions counted from
      the window's start: once a slot is full an append shifts every position, and every cached row is stale.

    A rebuild happens exactly when the stored and the new items together exceed the window. Unknown slots, lengths
    outside [0, max_len] and a non-positive window raise ``ValueError``."""
    max_len = int(max_len)
    if max_len <= 0:
        raise ValueError(f"max_len must be positive; got {max_len}")
    pairs = new_items.items() if isinstance(new_items, dict) else new_items
    merged: dict = {}
    for slot, items in pairs:
        if slot not in lengths:
            raise ValueError(f"slot {slot!r} is not open")
        merged.setdefault(slot, []).extend(int(i) for i in items)
    plan = {}
    for slot, items in merged.items():
        n = int(lengths[slot])
        if not 0 <= n <= max_len:
            raise ValueError(f"slot {slot!r} holds {n} rows, outside [0, {max_len}]")
        if not items:
            continue
        if n + len(items) <= max_len:
            plan[slot] = ("append", n, items)
        else:
            tail = items[-max_len:]
            plan[slot] = ("rebuild", max_len - len(tail), tail)
    return plan


def check_rows(row_slot, row_pos, n_slots: int, max_len: int) -> None:
    """The caller's contract of one ``xfmr_session_append`` call, checked on the host: every slot in [0, n_slots), every
    position in [0, max_len), no (slot, position) pair twice. ``ValueError`` otherwise. (The device clamps instead of
    faulting, but a clamped row is a lost event.)"""
    if len(row_slot) != len(row_pos):
        raise ValueError(f"{len(row_slot)} slots for {len(row_pos)} positions")
    seen = set()
    for s, p in zip(row_slot, row_pos):
        s, p = int(s), int(p)
        if not 0 <= s < n_slots:
            raise ValueError(f"slot {s} outside [0, {n_slots})")
        if not 0 <= p < max_len:
            raise ValueError(f"position {p} of slot {s} outside [0, {max_len})")
        if (s, p) in seen:
            raise ValueError(f"(slot {s}, position {p}) occurs twice in one call")
        seen.add((s, p))


class SessionEncoder:
    """Per-session K / V caches of ``model``'s encoder for ``n_slots`` sessions: owns the state buffer and the workspace.

    ``prefill(slots, histories)`` stores whole histories, ``append(slots, item_idx)`` adds events, ``embeddings(slots)``
    returns the sentence embeddings under the model's ``pooling_mode`` / ``is_normalized`` -- what
    ``model.encode_batch(histories)`` returns for the same histories, within the kernels' rounding (the cached path runs
    the same Linear / LayerNorm kernels on fewer rows and its own attention kernel). ``reset(slots)`` empties slots;
    ``refresh()`` must follow a weight change (it re-converts the parameters and rebuilds every slot from its items).

    Window rule. The reference encodes the last ``max_seq_length`` events, positions counted from the window's start. An
    append to a FULL slot therefore shifts every position and invalidates the slot's cache: the slot is re-prefilled from
    its last ``max_seq_length`` items through the same device call. The result is still ``encode(history)``, at the cost
    of a full encode (:func:`session_plan`).

    Each slot's items are kept on the host; slot and position ranges and duplicates are checked there. A call runs at most
    ``max_rows_per_call`` rows on the device (longer work is split in order, which keeps every row behind the rows it
    attends to). A bidirectional model (``is_decoder=False``) raises ``ValueError``.

    Where it pays (profiles/session.md: one MI355X, config 2's model, bf16; append + pooling against ``encode_batch`` of
    the full histories, HIP-event times): 1 024 sessions of 200 events 0.33 against 9.76 ms (1.59 ms for the device part of
    ``encode_batch`` alone); 64 x 200: 0.19 against 1.05 (0.36); one session of 50 events: 0.13 against 0.34 (0.19) -- there
    both paths are chains of ~36 launches and the gain is the smaller kernels and the host work saved, nothing more. No
    measured shape has the incremental path losing; the crossover is the window: a session AT ``max_seq_length`` pays a full
    re-prefill per event, i.e. ``encode``'s price plus the bookkeeping, and is better served by ``encode_batch``."""

    def __init__(self, model, n_slots: int, max_rows_per_call: int = 4096):
        import torch

        from . import ops

        if not bool(model.config.is_decoder):
            raise ValueError("SessionEncoder needs a causal encoder (is_decoder=True): with a bidirectional one an appended "
                             "event changes every earlier row, so nothing can be cached")
        if int(n_slots) <= 0 or int(max_rows_per_call) <= 0:
            raise ValueError("n_slots and max_rows_per_call must be positive")
        assert model.embeddings is not None, "call configure_embeddings() / set_table() first"
        self.model, self.n_slots, self.max_rows = model, int(n_slots), int(max_rows_per_call)
        self.max_len = model.max_seq_length
        with model.eval_mode():
            kw = model._cfg_kwargs(self.n_slots, self.max_len)
        self.cfg = ops.make_encoder_cfg(**kw)
        self.plan = ops.session_plan(self.cfg)
        nbytes, wbytes = ops.session_state_bytes(self.cfg, self.n_slots), ops.session_workspace_bytes(self.cfg, self.max_rows)
        if not nbytes or not wbytes:
            raise RuntimeError("xfmr_session_state_bytes: the encoder configuration is refused")
        dev = model.device
        self.state = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        self.workspace = torch.empty(wbytes, dtype=torch.uint8, device=dev)
        self.items: list[list[int]] = [[] for _ in range(self.n_slots)]
        ops.session_init(self.cfg, model.flat.detach(), self.state, self.n_slots)

    @property
    def state_bytes_per_slot(self) -> int:
        return self.state.numel() // self.n_slots

    def lengths(self, slots) -> list[int]:
        return [len(self.items[self._slot(s)]) for s in slots]

    def _slot(self, s) -> int:
        s = int(s)
        if not 0 <= s < self.n_slots:
            raise ValueError(f"slot {s} outside [0, {self.n_slots})")
        return s

    def reset(self, slots) -> None:
        """Empty the slots. Host only: keys beyond a slot's length are never read, so stale rows need no clearing."""
        for s in slots:
            self.items[self._slot(s)] = []

    def refresh(self) -> None:
        """After a weight change: convert the parameters again and rebuild every non-empty slot from its items."""
        from . import ops

        ops.session_init(self.cfg, self.model.flat.detach(), self.state, self.n_slots)
        held = [(s, it) for s, it in enumerate(self.items) if it]
        self.items = [[] for _ in range(self.n_slots)]
        if held:
            self.prefill([s for s, _ in held], [it for _, it in held])

    def prefill(self, slots, histories, *, return_tokens: bool = False):
        """Replace the slots' contents by ``histories`` (lists of table rows; each truncated to its last
        ``max_seq_length`` rows, as ``encode_batch`` truncates)."""
        slots = [self._slot(s) for s in slots]
        if len(set(slots)) != len(slots) or len(slots) != len(histories):
            raise ValueError("prefill takes distinct slots and one history per slot")
        self.reset(slots)
        return self._extend([(s, [int(i) for i in h][-self.max_len:]) for s, h in zip(slots, histories)], return_tokens)

    def append(self, slots, item_idx, *, return_tokens: bool = False):
        """Append events: ``item_idx[i]`` (one table row, or a list of them) to ``slots[i]``; a slot may occur more than
        once, its items are taken in order. ``return_tokens``: the new rows' token embeddings (rows, H), slots in the
        order of first occurrence and positions ascending -- for a slot that had to be rebuilt, all of its rows."""
        if len(slots) != len(item_idx):
            raise ValueError(f"{len(slots)} slots for {len(item_idx)} items")
        pairs = [(self._slot(s), list(i) if isinstance(i, (list, tuple)) else [int(i)]) for s, i in zip(slots, item_idx)]
        return self._extend(pairs, return_tokens)

    def _extend(self, pairs, return_tokens: bool):
        import torch

        from . import ops

        plan = session_plan({s: len(self.items[s]) for s, _ in pairs}, pairs, self.max_len)
        row_slot, row_pos, row_item = [], [], []
        for s, (kind, p, items) in plan.items():
            if kind == "rebuild":  # the window moved: every position shifts, the slot is written again from position 0
                items = self.items[s][len(self.items[s]) - p:] + items
                self.items[s], p = [], 0
            row_slot += [s] * len(items)
            row_pos += range(p, p + len(items))
            row_item += items
            self.items[s] = self.items[s] + items
        check_rows(row_slot, row_pos, self.n_slots, self.max_len)
        dev, out = self.model.device, []
        for a in range(0, len(row_item), self.max_rows):  # (in order: a row's earlier positions are in this call or before)
            b = a + self.max_rows
            tok = ops.session_append(
                self.cfg, self.model.flat.detach(), self.state, self.n_slots,
                torch.tensor(row_item[a:b], dtype=torch.int64, device=dev),
                torch.tensor(row_slot[a:b], dtype=torch.int32, device=dev),
                torch.tensor(row_pos[a:b], dtype=torch.int32, device=dev),
                self.model.embeddings, self.workspace, want_tok=return_tokens)
            out.append(tok)
        if not return_tokens:
            return None
        H = self.cfg.hidden
        return torch.cat(out) if out else torch.empty((0, H), dtype=torch.float32, device=dev)

    def embeddings(self, slots):
        """Sentence embeddings (n, H) of the slots' sessions; an empty slot gives a zero row."""
        import torch

        from . import ops

        slots = [self._slot(s) for s in slots]
        dev, c = self.model.device, self.model.config
        if not slots:
            return torch.empty((0, self.cfg.hidden), dtype=torch.float32, device=dev)
        return ops.session_pool(self.cfg, self.state, self.n_slots,
                                torch.tensor(slots, dtype=torch.int32, device=dev),
                                torch.tensor(self.lengths(slots), dtype=torch.int32, device=dev),
                                c.pooling_mode, normalize=bool(c.is_normalized))


class SessionRecommender:
    """Keyed sessions over a :class:`SessionEncoder` (``RecommenderLightningModule.open_sessions(n_slots)``):
    ``start(key, item_ids)``, ``append(key, item_id)``, ``close(key)`` and ``recommend(keys, top_k=0, exclude_seen=True)``.

    Item ids are converted as ``recommend_batch`` converts them (unknown ids are dropped; integers are table rows already).
    Slots are handed out by ``start`` and returned by ``close``, explicitly: a full store raises ``RuntimeError`` and
    nothing is evicted silently. The whole session (not only the encoder's window) is what ``exclude_seen`` excludes."""

    def __init__(self, module, n_slots: int, *, encoder=None, **encoder_kw):
        self.module = module
        self.encoder = encoder if encoder is not None else SessionEncoder(module.model, n_slots, **encoder_kw)
        self.n_slots = int(n_slots)
        self.free = list(range(self.n_slots - 1, -1, -1))  # (pop() hands out the lowest slot first)
        self.slot_of: dict = {}
        self.seen: dict = {}

    def __len__(self) -> int:
        return len(self.slot_of)

    def start(self, key, item_ids=()) -> int:
        """Open a session for ``key`` with the history ``item_ids``; returns its slot."""
        if key in self.slot_of:
            raise KeyError(f"session {key!r} is already open")
        if not self.free:
            raise RuntimeError(f"all {self.n_slots} session slots are in use: close a session first")
        rows = self.module._to_idx_or_empty(list(item_ids))
        slot = self.free.pop()
        self.slot_of[key], self.seen[key] = slot, list(rows)
        self.encoder.prefill([slot], [rows])
        return slot

    def append(self, key, item_id) -> None:
        """One more event of session ``key`` (an unknown id is dropped)."""
        slot = self.slot_of[key]
        rows = self.module._to_idx_or_empty([item_id])
        if rows:
            self.seen[key] += rows
            self.encoder.append([slot] * len(rows), rows)

    def close(self, key) -> None:
        slot = self.slot_of.pop(key)
        del self.seen[key]
        self.encoder.reset([slot])
        self.free.append(slot)

    def recommend(self, keys, top_k: int = 0, exclude_seen: bool = True, search: str = "exact") -> dict:
        """``{"item_idx": (n, k), "score": (n, k)}`` for the sessions ``keys``: the pooled session embedding against the
        item index, the session's own items left out; an empty session gets -1 / -inf (as ``recommend_batch``).
        ``search="refined"``: the bf16 shortlist + exact re-rank, the same bits (``ExactItemIndex.search_rows``)."""
        import torch

        keys = list(keys)
        emb = self.encoder.embeddings([self.slot_of[k] for k in keys])
        excl = [self.seen[k] for k in keys] if exclude_seen else None
        idx, score = self.module.items_index.search_rows(emb, excl, top_k=top_k or self.module.config.top_k, search=search)
        empty = [i for i, k in enumerate(keys) if not self.seen[k]]
        if empty:
            e = torch.as_tensor(empty, dtype=torch.int64, device=idx.device)
            idx.index_fill_(0, e, -1)
            score.index_fill_(0, e, float("-inf"))
        return {"item_idx": idx, "score": score}
