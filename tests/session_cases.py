"""The session encoder's cases (xfmr_session_append), shared by the CPU and the GPU tests. Plain module: numpy + the oracle, no
GPU and no library.

* `MODELS`, `params`, `table`: the two small encoders (head size 32 and 64) with biases and LayerNorm weights off 0 / 1.
* `SCENARIOS`: name -> list of CALLS; a call is a list of rows (slot, position, item) exactly as xfmr_session_append takes
  them. A write at position 0 starts a new session in its slot (what `reset` + `prefill` do on the host).
* `expected(key, calls)`: per call the fp64 rows of `oracle.encoder.encoder_forward` over the WHOLE session each row belongs
  to, and per row whether its query sees any key. The oracle keeps HF's finite mask bias, which turns a row without a
  visible key into a uniform average over all keys, later ones included; the kernels' convention for such a row is ctx = 0
  (attention; tests/attn_mask_cases.py). Rows that see a key -- every valid row among them -- are held to the
  oracle; the others are held to `Incremental`, the fp64 model below, whose rows with a key are shown equal to the oracle's.
* `Incremental(key, ..., mutant=)`: numpy fp64 model of the incremental pass the way the library walks it: per (slot, layer)
  one flat panel memory with the kernels' index arithmetic, mask bytes, the APPEND launch of all rows before the ATTEND
  launch. `MUTANTS` are switches of it, each a plausible kernel error.
"""

from __future__ import annotations

import functools
import math

import numpy as np
import torch

from helpers import unit_table

MODELS = {"h32": (64, 2, 128, 2), "h64": (128, 2, 256, 2)}  # key -> (H, heads, I, layers)
V, N_SLOTS, MAX_LEN = 200, 4, 40
CHUNK = 32          # xfmr_session_plan's key chunk; the GPU test reads it from the library and asserts this value
EDGE_MAX_LEN = 72   # the chunk-edge scenario: 2 CHUNK + 1 rows and some room
MUTANTS = ("keys_to_pos_plus_1", "keys_to_stale_length", "mask_ignored", "position_row_0", "kv_swapped",
           "head_stride_of_other_size", "chunk_sees_earlier_calls_only")


@functools.lru_cache(maxsize=None)
def params(key: str, max_len: int = MAX_LEN, layers: int | None = None) -> dict:
    """HF-keyed fp32 tensors of the model; biases and LayerNorm weights moved off 0 / 1 (tests/test_gpu_encoder_infer.py)."""
    from oracle import encoder as OE

    H, _, I, nl = MODELS[key]
    p = OE.init_params(H, layers or nl, I, max_len, seed=7)
    g = torch.Generator().manual_seed(11)
    for v in p.values():
        if v.dim() == 1:
            v += 0.05 * torch.randn(v.shape, generator=g)
    return p


@functools.lru_cache(maxsize=None)
def table(key: str) -> torch.Tensor:
    return unit_table(V, MODELS[key][0])


def _items(n: int, seed: int) -> list[int]:
    return torch.randint(1, V + 1, (n,), generator=torch.Generator().manual_seed(seed)).tolist()


HIST = {0: _items(1, 100), 1: _items(17, 101), 2: _items(MAX_LEN, 102)}  # lengths 1, 17 and max_len


def _one_token_at_a_time():
    """Slots 0, 1, 2 grow by one token per call; which slots take part changes from call to call."""
    calls, done, k = [], {s: 0 for s in HIST}, 0
    while any(done[s] < len(HIST[s]) for s in HIST):
        rows = [(s, done[s], HIST[s][done[s]]) for s in HIST if done[s] < len(HIST[s]) and (k % (s + 2)) != 0]
        for s, _, _ in rows:
            done[s] += 1
        if rows:
            calls.append(rows)
        k += 1
    return calls


def _chunked_prefill():
    """Slot 3: prefill 13, append 1, a chunk of 5, append 1 -- the first 20 items of the one-token scenario's slot 2."""
    h, calls, at = HIST[2], [], 0
    for n in (13, 1, 5, 1):
        calls.append([(3, at + j, h[at + j]) for j in range(n)])
        at += n
    return calls


def chunk_edges(chunk: int = CHUNK):
    """One slot each of lengths C - 1, C, C + 1 and 2 C + 1: prefill to length - 1 (one call), then one token."""
    lens = [chunk - 1, chunk, chunk + 1, 2 * chunk + 1]
    hist = [_items(n, 200 + s) for s, n in enumerate(lens)]
    return [[(s, t, h[t]) for s, h in enumerate(hist) for t in range(len(h) - 1)],
            [(s, len(h) - 1, h[-1]) for s, h in enumerate(hist)]]


def _masks():
    """Item 0 in front of, inside and at the end of a session, and a session of item 0 only: a prefill call, then tokens."""
    a = _items(12, 300)
    hist = {0: [0, 0] + a[:7], 1: a[:3] + [0, 0] + a[3:6] + [0] + a[6:8], 2: a[:6] + [0, 0], 3: [0] * 6}
    calls = [[(s, t, h[t]) for s, h in hist.items() for t in range(len(h) - 3)]]
    for j in (3, 2, 1):
        calls.append([(s, len(h) - j, h[len(h) - j]) for s, h in hist.items()])
    return calls


def _stale():
    """Slot 0 holds 40 items, is reset (host only) and prefilled with 9 others in two calls: the old rows 9 .. 39, their mask
    bytes included, are still in the state."""
    old, new = _items(MAX_LEN, 400), _items(9, 401)
    return [[(0, t, old[t]) for t in range(MAX_LEN)], [(0, t, new[t]) for t in range(5)], [(0, t, new[t]) for t in range(5, 9)]]


SCENARIOS = {"one_token": _one_token_at_a_time(), "chunked": _chunked_prefill(), "masks": _masks(), "stale": _stale()}


def sessions_of(calls):
    """Per row of every call: (session id, position). A session = the items a slot received since its last write at position 0."""
    ids, items, tags, n = {}, {}, [], 0
    for rows in calls:
        tag = []
        for s, pos, item in rows:
            if pos == 0:
                ids[s], n = n, n + 1
                items[ids[s]] = []
            assert len(items[ids[s]]) == pos, "a scenario appends positions in order"
            items[ids[s]].append(item)
            tag.append((ids[s], pos))
        tags.append(tag)
    return tags, items


def expected(key: str, calls, *, max_len: int = MAX_LEN, layers: int | None = None):
    """([per call (n, H) fp64 oracle rows], [per call (n,) bool: the row's query sees a key])."""
    from oracle import encoder as OE

    p64 = {k: v.double() for k, v in params(key, max_len, layers).items()}
    tags, items = sessions_of(calls)
    fwd, sees = {}, {}
    for sid, h in items.items():
        idx = torch.tensor(h, dtype=torch.int64)
        fwd[sid] = OE.encoder_forward(p64, table(key).double()[idx][None], (idx != 0)[None], MODELS[key][1])[0]
        sees[sid] = torch.cumsum((idx != 0).long(), 0) > 0
    rows = [torch.stack([fwd[sid][pos] for sid, pos in tag]) for tag in tags]
    vis = [torch.tensor([bool(sees[sid][pos]) for sid, pos in tag]) for tag in tags]
    return rows, vis


def _ln(x, g, b):
    mu = x.mean(-1, keepdims=True)
    var = ((x - mu) ** 2).mean(-1, keepdims=True)
    return (x - mu) / np.sqrt(var + 1e-12) * g + b


_erf = np.vectorize(math.erf)


class Incremental:
    """fp64 model of xfmr_session_init / xfmr_session_append. Panel memory per (slot, layer): a flat array addressed as the
    kernels address it -- head base = head * 2 * max_len * hs, K row = base + pos * hs, V row = base + (max_len + pos) * hs --
    with slack behind it, so a wrong stride reads other data instead of raising. `fill`: what unwritten memory holds."""

    def __init__(self, key, *, n_slots=N_SLOTS, max_len=MAX_LEN, layers=None, mutant=None, fill=0.0):
        assert mutant is None or mutant in MUTANTS
        self.H, self.A, self.I, nl = MODELS[key]
        self.layers, self.max_len, self.n_slots, self.mutant = layers or nl, max_len, n_slots, mutant
        self.hs = self.H // self.A
        self.p = {k: v.double().numpy() for k, v in params(key, max_len, layers).items()}
        self.table = table(key).double().numpy()
        self.mem = np.full((n_slots, self.layers, 4 * 2 * max_len * self.H), fill, dtype=np.float64)
        self.mask = np.zeros((n_slots, max_len), dtype=np.uint8)  # xfmr_session_init zeroes the mask bytes
        self.tok = np.full((n_slots, max_len, self.H), fill, dtype=np.float64)
        self.length = [0] * n_slots  # what a kernel that trusts a stored length would read (mutant keys_to_stale_length)

    def _row(self, head, which, pos, hs_base=None):
        hs = self.hs
        return head * 2 * self.max_len * (hs_base or hs) + (which * self.max_len + pos) * hs

    def append(self, rows):
        """One call: rows = [(slot, pos, item)]. Returns (n, H) last-layer rows; rows out of range come back as zeros."""
        p, H, hs, A = self.p, self.H, self.hs, self.A
        ok = [0 <= s < self.n_slots and 0 <= t < self.max_len for s, t, _ in rows]
        item = np.array([i if 0 <= i <= V else 0 for _, _, i in rows])
        pos_row = np.array([t if o and self.mutant != "position_row_0" else 0 for (_, t, _), o in zip(rows, ok)])
        emb = self.table[item]
        km = (emb != 0).any(-1).astype(np.uint8)
        x = _ln(emb + p["embeddings.token_type_embeddings.weight"][0] + p["embeddings.position_embeddings.weight"][pos_row],
                p["embeddings.LayerNorm.weight"], p["embeddings.LayerNorm.bias"])
        before = (self.mem.copy(), self.mask.copy()) if self.mutant == "chunk_sees_earlier_calls_only" else None
        prev_len = list(self.length)
        for i in range(self.layers):
            pre = f"encoder.layer.{i}."
            lin = lambda v, name: v @ p[pre + name + ".weight"].T + p[pre + name + ".bias"]  # noqa: E731
            q, k, v = (lin(x, "attention.self." + n) for n in ("query", "key", "value"))
            for r, (s, t, _) in enumerate(rows):  # the APPEND launch: every row's K, V and mask byte first
                if not ok[r]:
                    continue
                for h in range(A):
                    self.mem[s, i, self._row(h, 0, t):self._row(h, 0, t) + hs] = k[r, h * hs:(h + 1) * hs]
                    self.mem[s, i, self._row(h, 1, t):self._row(h, 1, t) + hs] = v[r, h * hs:(h + 1) * hs]
                self.mask[s, t] = km[r]
            mem, mask = before if before is not None else (self.mem, self.mask)
            ctx = np.zeros_like(x)
            other = 96 - hs if self.mutant == "head_stride_of_other_size" else None
            kw, vw = (1, 0) if self.mutant == "kv_swapped" else (0, 1)
            for r, (s, t, _) in enumerate(rows):  # the ATTEND launch
                if not ok[r]:
                    continue
                last = t
                if self.mutant == "keys_to_pos_plus_1":
                    last = min(t + 1, self.max_len - 1)
                if self.mutant == "keys_to_stale_length":
                    last = max(t, prev_len[s] - 1)
                keys = [j for j in range(last + 1) if self.mutant == "mask_ignored" or mask[s, j]]
                if not keys:
                    continue  # no visible key: ctx = 0
                for h in range(A):
                    K = np.stack([mem[s, i, self._row(h, kw, j, other):self._row(h, kw, j, other) + hs] for j in keys])
                    Vv = np.stack([mem[s, i, self._row(h, vw, j, other):self._row(h, vw, j, other) + hs] for j in keys])
                    sc = K @ q[r, h * hs:(h + 1) * hs] / math.sqrt(hs)
                    w = np.exp(sc - sc.max())
                    ctx[r, h * hs:(h + 1) * hs] = (w / w.sum()) @ Vv
            x1 = _ln(lin(ctx, "attention.output.dense") + x, p[pre + "attention.output.LayerNorm.weight"],
                     p[pre + "attention.output.LayerNorm.bias"])
            f = lin(x1, "intermediate.dense")
            f = 0.5 * f * (1.0 + _erf(f / math.sqrt(2.0)))
            x = _ln(lin(f, "output.dense") + x1, p[pre + "output.LayerNorm.weight"], p[pre + "output.LayerNorm.bias"])
        out = np.zeros_like(x)
        for r, (s, t, _) in enumerate(rows):
            if ok[r]:
                self.tok[s, t] = out[r] = x[r]
                self.length[s] = max(self.length[s], t + 1)
        return out

    def run(self, calls):
        return [self.append(rows) for rows in calls]


def scaled_err(got, want) -> float:
    """helpers.max_scaled_err on numpy / torch rows: max |d| / max(1, |want|)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float((np.abs(got - want) / np.maximum(np.abs(want), 1.0)).max()) if got.size else 0.0
