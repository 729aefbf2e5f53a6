"""The session encoder on the device: xfmr_session_init / _append / _pool (csrc/session.hip) and the Python around them
(xfmr_rec_amd/session.py).

The reference is always the fp64 `oracle.encoder.encoder_forward` of the WHOLE session, row by row (session_cases.expected),
at tests/helpers.py's `val` limits through `assert_close` -- the limits xfmr_encoder_infer is held to at these sizes. The
cases are session_cases.SCENARIOS (tests/test_session_cases_host.py shows on the CPU that the incremental pass reproduces the
full forward on them to 1e-10 and that each plausible kernel error exceeds the fp32 limit on one of them). One deviation from
"every row against the oracle": a row whose query sees NO key (item 0 in front of a session, a session of item 0 only) is
HF's uniform average over all keys in the oracle and ctx = 0 in this library's convention (attention); those rows
are held to the fp64 incremental model instead, which takes the convention and equals the oracle on every other row.

Models: (H, heads, I, layers) = (64, 2, 128, 2) and (128, 2, 256, 2), table unit_table(200, H), 4 slots, max_len 40, both
precision policies. Every test runs well under a second of GPU work."""

import numpy as np
import pytest
import torch

import session_cases as SC
from helpers import TOL, assert_close

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 4096
KEYS, PRECS = ("h32", "h64"), ("fp32", "bf16")


def flat_of(p):
    from xfmr_rec_amd.models import encoder_param_names

    return torch.cat([p[k].reshape(-1) for k in encoder_param_names(1 + max(int(k.split(".")[2]) for k in p if "layer." in k))])


class Device:
    """The entries at the ops level: state and workspace of exactly the library's sizes, optionally between guard bands and
    filled with 0xFF before xfmr_session_init."""

    def __init__(self, key, prec, *, max_len=SC.MAX_LEN, layers=None, n_slots=SC.N_SLOTS, max_rows=64, guard=False, flags=0,
                 **cfg_kw):
        from xfmr_rec_amd import ops

        H, A, I, nl = SC.MODELS[key]
        self.ops, self.n_slots, self.key = ops, n_slots, key
        self.flat = flat_of(SC.params(key, max_len, layers)).to(DEV)
        self.table = SC.table(key).to(DEV)
        self.cfg = ops.make_encoder_cfg(batch=n_slots, seq_len=max_len, hidden=H, heads=A, inter=I, layers=layers or nl,
                                        max_pos=max_len, precision=prec, flags=flags, **cfg_kw)
        self.sizes = (ops.session_state_bytes(self.cfg, n_slots), ops.session_workspace_bytes(self.cfg, max_rows))
        self.bufs = []
        for n in self.sizes:
            buf = torch.empty(GUARD + max(n, 16) + GUARD, dtype=torch.uint8, device=DEV)
            buf[:GUARD], buf[GUARD + n:] = 0xA5, 0x5A
            buf[GUARD:GUARD + n] = 0xFF if guard else 0
            self.bufs.append(buf)
        self.state, self.work = (b[GUARD:GUARD + n] for b, n in zip(self.bufs, self.sizes))

    def init(self):
        self.ops.session_init(self.cfg, self.flat, self.state, self.n_slots)
        return self

    def append(self, rows):
        s, t, i = (torch.tensor(c, dtype=d, device=DEV) for c, d in zip(zip(*rows), (torch.int32, torch.int32, torch.int64)))
        return self.ops.session_append(self.cfg, self.flat, self.state, self.n_slots, i, s, t, self.table, self.work)

    def run(self, calls):
        return [self.append(rows).cpu() for rows in calls]

    def guards_intact(self):
        torch.cuda.synchronize()
        return all(bool((b[:GUARD] == 0xA5).all()) and bool((b[GUARD + n:] == 0x5A).all()) for b, n in zip(self.bufs, self.sizes))


def check_rows(name, prec, got, want, sees, model=None):
    """Every call's rows: finite; rows that see a key against the oracle; the others (`model` given) against the fp64 model."""
    worst = 0.0
    for k, (g, w, v) in enumerate(zip(got, want, sees)):
        assert bool(torch.isfinite(g).all()), f"{name} call {k}: non-finite rows"
        if bool(v.any()):
            worst = max(worst, assert_close(f"{name} call {k}", g[v], w[v], prec))
        if model is not None and not bool(v.all()):
            worst = max(worst, assert_close(f"{name} call {k} (no visible key)", g[~v], torch.from_numpy(model[k])[~v], prec))
    print(f"{name} [{prec}]: worst scaled error {worst:.3e} (limit {TOL[prec]['val']:.1e})")


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("key", KEYS)
def test_one_token_at_a_time(key, prec):
    """Histories of lengths 1, 17 and max_len, interleaved across slots with a changing set of active slots per call; every
    step's tok_out row is checked."""
    calls = SC.SCENARIOS["one_token"]
    got = Device(key, prec).init().run(calls)
    check_rows("one_token", prec, got, *SC.expected(key, calls))


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("key", KEYS)
def test_chunked_prefill(key, prec):
    """Prefill 13, append 1, a chunk of 5, append 1: the rows of the one-token scenario's reference (its slot 2, rows 0 .. 19)."""
    tags, _ = SC.sessions_of(SC.SCENARIOS["one_token"])
    want1, _ = SC.expected(key, SC.SCENARIOS["one_token"])
    ref = {pos: want1[k][r] for k, (rows, tag) in enumerate(zip(SC.SCENARIOS["one_token"], tags))
           for r, ((slot, pos, _), _) in enumerate(zip(rows, tag)) if slot == 2}
    calls = SC.SCENARIOS["chunked"]
    got = Device(key, prec).init().run(calls)
    want = [torch.stack([ref[pos] for _, pos, _ in rows]) for rows in calls]
    check_rows("chunked", prec, got, want, [torch.ones(len(r), dtype=torch.bool) for r in calls])


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("key", KEYS)
def test_lengths_around_the_key_chunk(key, prec):
    """One layer; slots of lengths C - 1, C, C + 1 and 2 C + 1 with C read from the library's plan: prefill to length - 1, then
    one token. Every row of both calls is checked -- the last row and rows inside each chunk among them."""
    d = Device(key, prec, max_len=SC.EDGE_MAX_LEN, layers=1, max_rows=200)
    C = d.ops.session_plan(d.cfg)["chunk"]
    assert C == SC.CHUNK and 2 * C + 1 <= SC.EDGE_MAX_LEN
    calls = SC.chunk_edges(C)
    assert len(calls[0]) <= 200
    got = d.init().run(calls)
    check_rows("chunk_edges", prec, got, *SC.expected(key, calls, max_len=SC.EDGE_MAX_LEN, layers=1))


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("key", KEYS)
def test_masked_keys(key, prec):
    """Item 0 in front of, inside and at the end of a session, and a session of item 0 only: every value finite; rows that
    see a key against the oracle with that key mask, the rows that see none against the fp64 model (ctx = 0)."""
    calls = SC.SCENARIOS["masks"]
    got = Device(key, prec, guard=True).init().run(calls)  # (0xFF = NaN in unwritten rows: a masked row must not reach a sum)
    want, sees = SC.expected(key, calls)
    assert sum(int((~v).sum()) for v in sees) >= 8  # two rows in front of slot 0's first item, all six of slot 3
    check_rows("masks", prec, got, want, sees, model=SC.Incremental(key).run(calls))


def make_model(key, prec, *, max_len=SC.MAX_LEN, pooling="mean", normalized=False, is_decoder=True):
    import xfmr_rec_amd as X

    H, A, I, nl = SC.MODELS[key]
    conf = X.ModelConfig(hidden_size=H, num_attention_heads=A, intermediate_size=I, num_hidden_layers=nl,
                         max_seq_length=max_len, pooling_mode=pooling, is_normalized=normalized, is_decoder=is_decoder)
    m = X.RecommenderModel(conf, device=DEV, precision=prec, model=SC.params(key, max_len))
    m.set_table(SC.table(key).to(DEV))
    return m.eval()


@pytest.mark.parametrize("prec", PRECS)
def test_stale_state_does_not_matter(prec):
    """Prefill a slot with 40 items, reset, prefill 9 others: bit for bit what a freshly initialised state gives."""
    from xfmr_rec_amd.session import SessionEncoder

    _, items = SC.sessions_of(SC.SCENARIOS["stale"])
    old, new = list(items.values())
    m = make_model("h32", prec)
    used, fresh = SessionEncoder(m, SC.N_SLOTS), SessionEncoder(m, SC.N_SLOTS)
    used.prefill([0], [old])
    used.reset([0])
    assert used.lengths([0]) == [0]
    a = used.prefill([0], [new], return_tokens=True)
    b = fresh.prefill([0], [new], return_tokens=True)
    assert a.shape == (9, 64) and torch.equal(a, b)
    assert torch.equal(used.embeddings([0, 1]), fresh.embeddings([0, 1]))
    want, sees = SC.expected("h32", [SC.SCENARIOS["stale"][1] + SC.SCENARIOS["stale"][2]])
    check_rows("stale", prec, [a.cpu()], want, sees)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("key", KEYS)
def test_guard_bands_repeatability_and_rows_out_of_range(key, prec):
    """State and workspace at exactly the library's sizes between two 4 KiB guard bands, 0xFF-filled before xfmr_session_init:
    the bands come back untouched, all outputs are finite, the same calls repeated give the same bits; rows with a slot or a
    position out of range leave every byte of the state as it was and come back as zero rows."""
    calls = SC.SCENARIOS["chunked"] + SC.SCENARIOS["one_token"][:12]
    d = Device(key, prec, guard=True, max_rows=max(len(r) for r in calls))
    first = d.init().run(calls)
    pooled = d.ops.session_pool(d.cfg, d.state, d.n_slots, torch.tensor([3, 2, 0, 1], dtype=torch.int32, device=DEV),
                                torch.tensor([20, 5, 0, 3], dtype=torch.int32, device=DEV), "mean", normalize=True)
    assert d.guards_intact()
    assert all(bool(torch.isfinite(t).all()) for t in first) and bool(torch.isfinite(pooled).all())
    assert not bool(pooled[2].any())  # a length of 0: a zero row
    again = d.init().run(calls)
    assert all(torch.equal(a, b) for a, b in zip(first, again))
    before = d.state.clone()
    bad = [(d.n_slots, 0, 5), (-1, 3, 5), (1, SC.MAX_LEN, 5), (1, -1, 5), (2 ** 31 - 1, 2 ** 31 - 1, 5)]
    out = d.append(bad)
    assert d.guards_intact() and torch.equal(d.state, before), "a row out of range wrote to the state"
    assert out.shape == (len(bad), SC.MODELS[key][0]) and not bool(out.any())
    # ... also beside good rows, which are not disturbed by them
    slot2 = [r for rows in SC.SCENARIOS["one_token"][:12] for r in rows if r[0] == 2]
    nxt = (2, len(slot2), SC.HIST[2][len(slot2)])
    mixed = d.append([bad[0], nxt, bad[2]])
    alone = Device(key, prec, max_rows=max(len(r) for r in calls)).init()
    alone.run(calls)
    assert torch.equal(mixed[1], alone.append([nxt])[0]) and not bool(mixed[0].any()) and not bool(mixed[2].any())


@pytest.mark.parametrize("prec", PRECS)
def test_pooled_embeddings_against_fp64(prec):
    """SessionEncoder.embeddings for the four pooling modes, with and without normalisation, against oracle.encoder.pool on the
    fp64 rows; slots of lengths 40, 17 (grown by appends), 11 (item 0 inside, grown by appends) and 0."""
    from oracle import encoder as OE
    from xfmr_rec_amd.session import SessionEncoder

    key = "h32"
    m = make_model(key, prec)
    enc = SessionEncoder(m, SC.N_SLOTS)
    _, mask_items = SC.sessions_of(SC.SCENARIOS["masks"])
    hists = {0: SC.HIST[2], 1: SC.HIST[1], 2: list(mask_items.values())[1]}
    enc.prefill([0, 1, 2], [hists[0], hists[1][:9], hists[2][:4]])
    enc.append([1, 2] * 2, [hists[1][9:12], hists[2][4:6], hists[1][12:], hists[2][6:]])
    assert enc.lengths([0, 1, 2, 3]) == [40, 17, 11, 0] and 0 in hists[2][1:-1]
    p64 = {k: v.double() for k, v in SC.params(key).items()}
    for mode in ("mean", "max", "cls", "lasttoken"):
        for normalized in (False, True):
            m.config.pooling_mode, m.config.is_normalized = mode, normalized
            got = enc.embeddings([3, 0, 1, 2]).cpu()
            assert not bool(got[0].any())  # the empty slot
            for row, s in enumerate((0, 1, 2), start=1):
                idx = torch.tensor(hists[s], dtype=torch.int64)
                tok = OE.encoder_forward(p64, SC.table(key).double()[idx][None], (idx != 0)[None], SC.MODELS[key][1])
                want = OE.pool(tok, (idx != 0)[None], mode)[0]
                if normalized:
                    want = want / want.norm().clamp(min=1e-12)
                assert_close(f"pool {mode} normalized={normalized} slot {s}", got[row], want, prec)


# ---------------------------------------------------------------------------------------------- surfaces
SURF_L, SURF_V, SURF_K = 16, 60, 3


def planted_catalogue(state, heads, histories):
    """(table (V + planted, H) fp32, fp64 best-first item rows per history, smallest fp64 score gap among each history's first
    SURF_K + 1 places). Rows 1 .. SURF_V are unit_table's and the only ones a history holds; behind them SURF_K planted rows
    per history, at cosines 0.98, 0.86, 0.74 to that history's fp64 sentence embedding (mean pooling), along directions
    orthogonal to every history's embedding."""
    from oracle import encoder as OE

    H = state["embeddings.LayerNorm.weight"].numel()
    base = SC.unit_table(SURF_V, H).double()
    p64 = {k: v.double().cpu() for k, v in state.items()}
    embs = []
    for h in histories:
        idx = torch.tensor(h[-SURF_L:], dtype=torch.int64)
        tok = OE.encoder_forward(p64, base[idx][None], (idx != 0)[None], heads)
        e = OE.pool(tok, (idx != 0)[None], "mean")[0]
        embs.append(e / e.norm())
    g = torch.Generator().manual_seed(77)
    E = torch.stack(embs)
    rows = []
    for e in embs:
        for c in (0.98, 0.86, 0.74)[:SURF_K]:
            w = torch.randn(H, generator=g, dtype=torch.float64)
            w = w - torch.linalg.lstsq(E.T, w[:, None]).solution[:, 0] @ E  # orthogonal to every embedding
            rows.append(c * e + (1 - c * c) ** 0.5 * w / w.norm())
    table = torch.cat([base, torch.stack(rows)])
    best, gap = [], float("inf")
    for e, h in zip(embs, histories):
        score = table @ e / table.norm(dim=-1).clamp(min=1e-8)
        score[0] = -float("inf")
        score[torch.tensor(sorted(set(h)))] = -float("inf")  # the history itself is excluded
        top = torch.argsort(score, descending=True)[:SURF_K + 1]
        best.append(top[:SURF_K].tolist())
        gap = min(gap, float((score[top][:-1] - score[top][1:]).min()))
    return table.float(), best, gap


def surface_histories():
    """Histories below, at and past max_seq_length, of rows 1 .. SURF_V."""
    return [[(i - 1) % SURF_V + 1 for i in SC._items(n, seed)] for n, seed in ((5, 500), (SURF_L, 501), (SURF_L + 6, 502))]


def surface_state():
    return SC.params("h32", SURF_L)


@pytest.mark.parametrize("prec", PRECS)
def test_session_recommender_agrees_with_recommend_batch(prec):
    """start + appends, one session run past max_seq_length (the rebuild path): the item rows of recommend_batch on the full
    histories with the histories excluded, on a planted catalogue whose first places are separated by more than the `val`
    limit in fp64 (checked here), so the order cannot flip."""
    import xfmr_rec_amd as X

    hists = surface_histories()
    conf = X.LightningConfig(hidden_size=64, num_attention_heads=2, intermediate_size=128, num_hidden_layers=2,
                             max_seq_length=SURF_L, precision=prec, top_k=SURF_K)
    mod = X.RecommenderLightningModule(conf)
    mod.configure_model()
    mod.model.load_encoder_state_dict(surface_state())
    table, best, gap = planted_catalogue(surface_state(), 2, hists)
    assert gap > 2 * TOL[prec]["val"], f"planted scores are only {gap:.3e} apart"
    mod.model.set_table(table.to(DEV))
    mod.eval()
    rec = mod.open_sessions(4)
    assert type(rec).__name__ == "SessionRecommender" and rec.encoder.max_len == SURF_L
    rec.start("a", hists[0][:2])
    rec.start("b", hists[1][:9])
    rec.start("c", hists[2][:SURF_L - 1])
    rec.start("empty", [])
    for k, h, n0 in (("a", hists[0], 2), ("b", hists[1], 9), ("c", hists[2], SURF_L - 1)):
        for item in h[n0:]:
            rec.append(k, item)
    assert rec.encoder.lengths([0, 1, 2, 3]) == [5, SURF_L, SURF_L, 0]
    assert rec.encoder.items[2] == hists[2][-SURF_L:] and rec.seen["c"] == hists[2]
    got = rec.recommend(["a", "b", "c", "empty"])
    want = mod.recommend_batch(hists + [[]], top_k=SURF_K, exclude_item_ids=hists + [[]])
    assert got["item_idx"].shape == (4, SURF_K) and got["score"].shape == (4, SURF_K)
    assert torch.equal(got["item_idx"], want["item_idx"]), (got["item_idx"].tolist(), want["item_idx"].tolist())
    assert got["item_idx"][:3].tolist() == best  # ... and both are the fp64 order
    assert got["item_idx"][3].tolist() == [-1] * SURF_K and bool(torch.isinf(got["score"][3]).all())
    assert float((got["score"][:3] - want["score"][:3]).abs().max()) <= TOL[prec]["val"]
    # the embeddings themselves: what encode_batch returns for the histories
    emb = rec.encoder.embeddings([0, 1, 2]).cpu()
    assert_close("embeddings vs encode_batch", emb, mod.model.encode_batch(hists).cpu().double(), prec)
    rec.close("b")
    assert rec.start("d", hists[1]) == 1  # the freed slot, prefilled at once
    assert torch.equal(rec.recommend(["d"])["item_idx"][0], want["item_idx"][1])
    with pytest.raises(RuntimeError, match="in use"):
        rec.start("e", [1])


def test_refusals():
    from xfmr_rec_amd import _native as N
    from xfmr_rec_amd.session import SessionEncoder

    with pytest.raises(ValueError, match="causal"):
        SessionEncoder(make_model("h32", "bf16", is_decoder=False), 2)
    with pytest.raises(RuntimeError, match="not supported"):
        Device("h32", "bf16", flags=N.ENC_BIDIRECTIONAL).init()
    with pytest.raises(RuntimeError, match="invalid argument"):
        Device("h32", "bf16", hidden_dropout=0.1).init()
    d = Device("h32", "bf16")
    short = d.state[:d.state.numel() - 16]
    with pytest.raises(RuntimeError, match="workspace too small"):
        d.ops.session_init(d.cfg, d.flat, short, d.n_slots)
    d.init()
    with pytest.raises(RuntimeError, match="workspace too small"):
        d.ops.session_append(d.cfg, d.flat, short, d.n_slots, torch.ones(1, dtype=torch.int64, device=DEV),
                             torch.zeros(1, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV),
                             d.table, d.work)
    enc = SessionEncoder(make_model("h32", "bf16"), 2)
    with pytest.raises(ValueError, match="slot 2"):
        enc.append([2], [5])
    assert np.isfinite(enc.state_bytes_per_slot) and enc.state_bytes_per_slot > 0
