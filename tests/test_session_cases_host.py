"""CPU-side test (no GPU, no library) of tests/session_cases.py: the premise of tests/test_gpu_session.py, checked where it can
be, and the evidence that its cases tell a right kernel from a plausibly wrong one.

1. Row t of the full causal forward (oracle/encoder.py: encoder_forward over the whole session) is the row the incremental
   fp64 model produces when token t is appended, to 1e-10, in every scenario and for both head sizes -- on every row whose
   query sees a key. (A row without one is HF's uniform average in the oracle and ctx = 0 in the kernels' convention:
   session_cases.expected marks those rows, and the test shows they exist only where the mask says so.)
2. Unwritten state is never read: the same rows come out of a model whose memory starts as NaN.
3. Every mutant of the model -- one kernel error each -- exceeds the fp32 limit on at least one scenario.
"""

import numpy as np
import pytest

import session_cases as SC
from helpers import TOL

KEYS = ("h32", "h64")


def all_scenarios():
    out = [(name, calls, {}) for name, calls in SC.SCENARIOS.items()]
    out.append(("chunk_edges", SC.chunk_edges(), dict(max_len=SC.EDGE_MAX_LEN, layers=1)))
    return out


@pytest.mark.parametrize("key", KEYS)
def test_incremental_rows_are_the_full_forward_rows(key):
    for name, calls, kw in all_scenarios():
        want, sees = SC.expected(key, calls, **kw)
        got = SC.Incremental(key, fill=np.nan, **kw).run(calls)
        n_blind = 0
        for g, w, v in zip(got, want, sees):
            v = v.numpy()
            assert np.isfinite(g).all(), (key, name)
            assert SC.scaled_err(g[v], w.numpy()[v]) <= 1e-10, (key, name)
            n_blind += int((~v).sum())
        # rows without a visible key: only in front of a session's first non-zero item
        assert (n_blind > 0) == (name == "masks"), (key, name, n_blind)


def test_the_scenarios_cover_what_the_issue_lists():
    one = SC.SCENARIOS["one_token"]
    sizes = {len(rows) for rows in one}
    assert sizes == {1, 2, 3} and all(len({s for s, _, _ in rows}) == len(rows) for rows in one)  # a changing set of slots
    tags, items = SC.sessions_of(one)
    assert sorted(len(h) for h in items.values()) == [1, 17, SC.MAX_LEN]
    assert [len(rows) for rows in SC.SCENARIOS["chunked"]] == [13, 1, 5, 1]
    assert SC.SCENARIOS["chunked"][2][0][:2] == (3, 14)
    pre, last = SC.chunk_edges(SC.CHUNK)
    assert sorted(t + 1 for _, t, _ in last) == [SC.CHUNK - 1, SC.CHUNK, SC.CHUNK + 1, 2 * SC.CHUNK + 1]
    assert max(t for _, t, _ in last) < SC.EDGE_MAX_LEN
    _, items = SC.sessions_of(SC.SCENARIOS["masks"])
    h = list(items.values())
    assert h[0][:2] == [0, 0] and 0 in h[1][1:-1] and h[1][0] and h[1][-1] and h[2][-1] == 0 and set(h[3]) == {0}
    _, items = SC.sessions_of(SC.SCENARIOS["stale"])
    assert [len(v) for v in items.values()] == [SC.MAX_LEN, 9]


def test_rows_out_of_range_store_nothing_and_come_back_zero():
    m = SC.Incremental("h32")
    m.append([(0, 0, 5), (0, 1, 6)])
    mem, mask, tok = m.mem.copy(), m.mask.copy(), m.tok.copy()
    out = m.append([(SC.N_SLOTS, 2, 7), (-1, 0, 7), (1, SC.MAX_LEN, 7), (1, -1, 7)])
    assert not out.any() and (m.mem == mem).all() and (m.mask == mask).all() and (m.tok == tok).all()


@pytest.mark.parametrize("mutant", SC.MUTANTS)
def test_every_mutant_exceeds_the_fp32_limit_somewhere(mutant):
    worst = {}
    for key in KEYS:
        for name, calls, kw in all_scenarios():
            want, sees = SC.expected(key, calls, **kw)
            got = SC.Incremental(key, mutant=mutant, **kw).run(calls)
            errs = [SC.scaled_err(g[v.numpy()], w.numpy()[v.numpy()]) for g, w, v in zip(got, want, sees)]
            worst[key, name] = max(e if np.isfinite(e) else np.inf for e in errs)
    assert max(worst.values()) > TOL["fp32"]["val"], (mutant, worst)
    # ... and where it is said to show: the scenario built for it
    built_for = {"keys_to_pos_plus_1": "chunked", "keys_to_stale_length": "stale", "mask_ignored": "masks",
                 "position_row_0": "one_token", "kv_swapped": "one_token", "head_stride_of_other_size": "one_token",
                 "chunk_sees_earlier_calls_only": "chunked"}[mutant]
    assert min(worst[key, built_for] for key in KEYS) > TOL["fp32"]["val"], (mutant, built_for, worst)
