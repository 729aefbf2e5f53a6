"""xfmr_candidate_ranks on the device: ranks and scores against ``candidate_cases.rank_among_ref`` exactly (dot and l2 on
numpy's exact scores, cosine on the device's own score bits), the scores against xfmr_target_ranks' and xfmr_topk_tiled's
bits, the reduction to xfmr_target_ranks when every item is a candidate, guards around every output, run-to-run bits,
the score-only form, CSR views, and the refusal that needs the offsets."""

import functools

import numpy as np
import pytest
import torch

import candidate_cases as CC

pytestmark = pytest.mark.gpu
DEV = "cuda"
METRICS = ["dot", "cosine", "l2"]
CASES = [c.name for c in CC.cases()]
LEAD_C, LEAD_X, LEAD_T = 3, 2, 5  # unrelated entries in front of each CSR: no first offset is 0
GUARD_RANK, GUARD_SCORE = -7, 123.0


def _dev(csr):
    return tuple(torch.from_numpy(x).to(DEV) for x in csr)


def _case(name):
    return {c.name: c for c in CC.cases()}[name]


@functools.lru_cache(maxsize=None)
def _setup(name, metric):
    """The case on the device: index, queries and the three CSRs (each a view into a longer array)."""
    from xfmr_rec_amd.retrieval import ExactItemIndex

    case = _case(name)
    index = ExactItemIndex(torch.from_numpy(case.table).to(DEV), index_metric=metric)
    q = torch.from_numpy(case.query).to(DEV)
    return index, q, _dev(CC.csr(case.cand, LEAD_C)), _dev(CC.csr(case.excl, LEAD_X)), _dev(CC.csr(case.tgts, LEAD_T))


def _run(index, q, cand, ex, tg, rank_fill=GUARD_RANK):
    """One call with all three outputs, each pre-filled: what the call does not own must come back as it was."""
    out = torch.full((tg[0].numel(),), rank_fill, dtype=torch.int32, device=DEV)
    ts = torch.full((tg[0].numel(),), GUARD_SCORE, dtype=torch.float32, device=DEV)
    cs = torch.full((cand[0].numel(),), GUARD_SCORE, dtype=torch.float32, device=DEV)
    index._candidate_ranks(q, cand, ex, tg, out, ts, cs)
    torch.cuda.synchronize()
    return out, ts, cs


@functools.lru_cache(maxsize=None)
def _device_result(name, metric):
    index, q, cand, ex, tg = _setup(name, metric)
    return _run(index, q, cand, ex, tg)


@functools.lru_cache(maxsize=None)
def _all_item_scores(name, metric):
    """Every query's score of every item 1 .. n_rows - 1 as xfmr_target_ranks reports a target's own score (the fmaf chain
    that equals the MFMA tile): (n_query, n_rows) float32, column 0 and non-finite scores -inf."""
    index, q, *_ = _setup(name, metric)
    n_query, n_rows, _ = _case(name).shape
    items = torch.arange(1, n_rows, dtype=torch.int64, device=DEV).repeat(n_query)
    off = torch.arange(0, n_query + 1, dtype=torch.int64, device=DEV) * (n_rows - 1)
    _, score = index.rank_targets(q, (items, off), None, return_scores=True)
    s = torch.full((n_query, n_rows), float("-inf"), dtype=torch.float32, device=DEV)
    s[:, 1:] = score.view(n_query, n_rows - 1)
    return s.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _inside(n, lead):
    """The flat entries that belong to the CSR: everything but the ``lead`` entries in front and the one behind."""
    return slice(lead, n - 1)


# ------------------------------------------------------------------------------------ 1. the reference, exactly
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("name", CASES)
def test_ranks_and_scores_equal_the_reference(name, metric):
    case = _case(name)
    out, ts, cs = (x.cpu().numpy() for x in _device_result(name, metric))
    ti, ci = _inside(out.size, LEAD_T), _inside(cs.size, LEAD_C)
    if metric == "cosine":
        # not exact in fp32: the reference ranks the scores the device reports for the items (checked in test 2)
        s_all = _all_item_scores(name, metric).astype(np.float64)
        s_all[~np.isfinite(s_all)] = np.nan  # (as a score that is not finite, not as an excluded one)
        want_r, want_t, want_c = [], [], []
        for b in range(case.query.shape[0]):
            r, t, c = CC.rank_among_ref(s_all[b], case.cand[b], case.excl[b], case.tgts[b])
            want_r += r
            want_t += t
            want_c += c
        want_r, want_t, want_c = np.asarray(want_r), np.asarray(want_t), np.asarray(want_c)
    else:
        want_r, want_t, want_c = CC.expected(name, metric)
    bad = np.flatnonzero(out[ti] != want_r)
    assert bad.size == 0, (name, metric, bad[:5].tolist(), out[ti][bad[:5]].tolist(), want_r[bad[:5]].tolist())
    assert np.array_equal(ts[ti].astype(np.float64), want_t), np.flatnonzero(ts[ti] != want_t)[:5]
    assert np.array_equal(cs[ci].astype(np.float64), want_c), np.flatnonzero(cs[ci] != want_c)[:5]
    assert (want_r == CC.RANK_NONE).any() and ((want_r != CC.RANK_NONE).any() or case.table.shape[0] == 2)
    # the guards: nothing outside the CSR's own entries is written
    assert (out[:LEAD_T] == GUARD_RANK).all() and out[-1] == GUARD_RANK
    assert (ts[:LEAD_T] == GUARD_SCORE).all() and ts[-1] == GUARD_SCORE
    assert (cs[:LEAD_C] == GUARD_SCORE).all() and cs[-1] == GUARD_SCORE


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("name", ["wave-edges", "many-queries"])
def test_two_calls_give_the_same_bits_whatever_out_rank_held(name, metric):
    index, q, cand, ex, tg = _setup(name, metric)
    first = _device_result(name, metric)
    again = _run(index, q, cand, ex, tg, rank_fill=0x5A5A5A5A)
    ti = _inside(first[0].numel(), LEAD_T)
    assert torch.equal(again[0][ti], first[0][ti])  # out_rank need not be zeroed
    assert torch.equal(again[1].view(torch.int32), first[1].view(torch.int32))
    assert torch.equal(again[2].view(torch.int32), first[2].view(torch.int32))
    assert (again[0][:LEAD_T] == 0x5A5A5A5A).all() and int(again[0][-1]) == 0x5A5A5A5A


# ------------------------------------------------------------------------------------ 2. the other entries' score bits
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("name", CASES)
def test_scores_are_the_rank_entrys_bits(name, metric):
    """A candidate's or target's score is bit for bit the score xfmr_target_ranks reports for that item."""
    case = _case(name)
    _, ts, cs = (x.cpu().numpy() for x in _device_result(name, metric))
    s_all = _all_item_scores(name, metric)
    n_rows = case.table.shape[0]
    n = 0
    for lists, got, lead in ((case.cand, cs, LEAD_C), (case.tgts, ts, LEAD_T)):
        at = lead
        for b, items in enumerate(lists):
            ids = np.asarray(items, dtype=np.int64)
            g = got[at : at + ids.size]
            at += ids.size
            real = (ids >= 1) & (ids < n_rows)
            assert (g[~real] == -np.inf).all()
            live = real & (g != -np.inf)
            assert np.array_equal(_bits(g[live]), _bits(s_all[b, ids[live]])), (name, metric, b)
            excluded = np.isin(ids, case.excl[b])
            assert (g[excluded] == -np.inf).all()
            assert (live | excluded | ~real | (s_all[b, np.clip(ids, 0, n_rows - 1)] == -np.inf)).all()
            n += int(live.sum())
    assert n > 0 or n_rows == 2


@pytest.mark.parametrize("metric", METRICS)
def test_scores_are_the_tiled_searchs_bits(metric):
    """64 items: ``search_batch(top_k=64)`` (xfmr_topk_tiled) returns every eligible item, so each live candidate has a place
    in that list, with the same score bits; and a live target's rank among ALL items is its place + 1."""
    name = "wave-edges"
    case = _case(name)
    index, q, cand, ex, tg = _setup(name, metric)
    _, _, cs = (x.cpu().numpy() for x in _device_result(name, metric))
    idx, score = index.search_batch(q, case.excl, top_k=64)
    idx, score = idx.cpu().numpy(), score.cpu().numpy()
    at, n = LEAD_C, 0
    for b, items in enumerate(case.cand):
        place = {int(i): p for p, i in enumerate(idx[b]) if i >= 0}
        for x, c in enumerate(items):
            g = cs[at + x]
            if c in place:
                assert _bits(g) == _bits(score[b, place[c]]), (b, c, g, score[b, place[c]])
                n += 1
            else:
                assert g == -np.inf, (b, c, g)
        at += len(items)
    assert n > 500


# ------------------------------------------------------------------------------------ 3. every item as a candidate
@pytest.mark.parametrize("metric", METRICS)
def test_with_every_item_as_a_candidate_the_ranks_are_xfmr_target_ranks(metric):
    name = "many-queries"  # 257 queries, 4 097 rows, H = 384, with its exclusion CSR
    n_query, n_rows, H = _case(name).shape
    assert (n_query, n_rows, H) == (257, 4097, 384)
    index, q, _, ex, tg = _setup(name, metric)
    items = torch.arange(1, n_rows, dtype=torch.int64, device=DEV).repeat(n_query)
    off = torch.arange(0, n_query + 1, dtype=torch.int64, device=DEV) * (n_rows - 1)
    got = index.rank_among(q, (items, off), tg, ex)
    want = index.rank_targets(q, tg, ex)
    ti = _inside(got.numel(), LEAD_T)
    assert torch.equal(got[ti], want[ti])
    assert int((got[ti] != CC.RANK_NONE).sum()) > 1000 and int(got[ti][got[ti] != CC.RANK_NONE].max()) > 2000
    assert (got[:LEAD_T] == CC.RANK_NONE).all() and int(got[-1]) == CC.RANK_NONE  # (the wrapper's fill, left alone)


# ------------------------------------------------------------------------------------ 4. the wrappers
@pytest.mark.parametrize("metric", METRICS)
def test_score_only_form_and_wrappers(metric):
    name = "wave-edges"
    index, q, cand, ex, tg = _setup(name, metric)
    out, ts, cs = _device_result(name, metric)
    ci, ti = _inside(cs.numel(), LEAD_C), _inside(out.numel(), LEAD_T)
    only = index.score_candidates(q, cand, ex)  # targets NULL
    assert only.dtype == torch.float32 and torch.equal(only[ci].view(torch.int32), cs[ci].view(torch.int32))
    assert (only[:LEAD_C] == float("-inf")).all() and only[-1] == float("-inf")
    ranks, scores = index.rank_among(q, cand, tg, ex, candidate_scores=True)
    assert torch.equal(ranks[ti], out[ti]) and torch.equal(scores[ci].view(torch.int32), cs[ci].view(torch.int32))
    assert torch.equal(index.rank_among(q, cand, tg, ex)[ti], out[ti])
    # without exclusions: the reference with an empty list per query
    case = _case(name)
    if metric != "cosine":
        free = index.rank_among(q, cand, tg)[ti].cpu().numpy()
        want = []
        for b in range(case.query.shape[0]):
            want += CC.rank_among_ref(CC.score_vector(case, b, metric), case.cand[b], [], case.tgts[b])[0]
        assert free.tolist() == want
    # a chunk of a longer CSR: offsets are views with absolute values, entries outside the view are left alone
    toff = tg[1].cpu().numpy()
    part = torch.full_like(out, -3)
    index.rank_among(q[8:20], (cand[0], cand[1][8:21]), (tg[0], tg[1][8:21]), (ex[0], ex[1][8:21]), out=part)
    assert torch.equal(part[toff[8] : toff[20]], out[toff[8] : toff[20]])
    assert (part[: toff[8]] == -3).all() and (part[toff[20] :] == -3).all()
    for bad in (lambda: index.rank_among(q, (cand[0], cand[1][:-1]), tg), lambda: index.rank_among(q, cand, (tg[0].int(), tg[1])),
                lambda: index.rank_among(q, cand, tg, (ex[0], ex[1][:-1])),
                lambda: index.rank_among(q, cand, tg, out=torch.empty(3, dtype=torch.int32, device=DEV)),
                lambda: index.score_candidates(q, (cand[0], cand[1][:-1]))):
        with pytest.raises(ValueError):
            bad()


def test_list_sizes_are_checked_on_the_device_offsets_before_any_launch():
    """2^31 candidates (or targets) are refused with XFMR_EUNSUPPORTED, offsets that run backwards with XFMR_EINVAL: the
    offsets say so, the arrays themselves are one element long and nothing is launched over them."""
    from xfmr_rec_amd import _native as N

    index, q, cand, ex, tg = _setup("one-query", "dot")
    lib = N.load()
    one = torch.ones(1, dtype=torch.int64, device=DEV)
    out = torch.full((4,), GUARD_RANK, dtype=torch.int32, device=DEV)
    cs = torch.full((4,), GUARD_SCORE, dtype=torch.float32, device=DEV)

    def call(cando, tgo):
        cando, tgo = (torch.tensor(x, dtype=torch.int64, device=DEV) for x in (cando, tgo))
        rc = lib.xfmr_candidate_ranks(N.ptr(q), N.ptr(index.table), None, None, index.table.shape[0], 1, q.shape[1], N.ptr(one),
                                      N.ptr(cando), None, None, N.ptr(one), N.ptr(tgo), 1, N.ptr(out), None, N.ptr(cs),
                                      N.stream())
        torch.cuda.synchronize()
        return rc

    assert call([0, 1 << 31], [0, 1]) == -2 and call([5, 5 + (1 << 31)], [0, 1]) == -2
    assert call([0, 1], [0, 1 << 31]) == -2
    assert call([1, 0], [0, 1]) == -1 and call([0, 1], [3, 2]) == -1
    assert (out == GUARD_RANK).all() and (cs == GUARD_SCORE).all()
    assert call([0, 1], [0, 1]) == 0  # the same call with honest sizes: item 1 among {1}
    assert out.tolist() == [1, GUARD_RANK, GUARD_RANK, GUARD_RANK] and bool(torch.isfinite(cs[0]))
