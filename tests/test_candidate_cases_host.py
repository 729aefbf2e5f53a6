"""CPU-side checks of the cases behind the xfmr_candidate_ranks tests: the cases cover what they claim, the reference
reduces to the full-catalogue ranks when every item is a candidate, and plausible WRONG kernels -- each the reference
with one rule broken -- give different ranks on them, so a kernel that passes the cases has none of these faults."""

import numpy as np
import pytest

import candidate_cases as CC
import rank_refs as R


def _flawed_ranks(flaw, s, candidates, exclude, targets):
    """``CC.rank_among_ref``'s ranks with one rule broken (``flaw`` None: the rule book itself, written as the loop a
    kernel runs rather than as sets)."""
    s = np.asarray(s, dtype=np.float64)
    n = s.size
    ok = CC.eligible_mask(s, () if flaw == "ignores_exclusions" else exclude)
    if flaw == "counts_ineligible":
        ok = np.ones(n, dtype=bool)
        for x in exclude:
            if 0 <= x < n:
                ok[x] = False

    def elig(j):
        return 0 <= j < n and bool(ok[j])

    def beats(c, t):
        if flaw == "greater_equal":
            return s[c] >= s[t]
        if flaw == "tie_reversed":
            return s[c] > s[t] or (s[c] == s[t] and c > t)
        return s[c] > s[t] or (s[c] == s[t] and c < t)

    cand = list(candidates)
    if flaw == "drops_last_partial_64":
        cand = cand[: len(cand) // 64 * 64]
    places = []  # the items that are counted, in the order a kernel walks them
    for x, c in enumerate(cand):
        if elig(c) and (flaw == "duplicates_twice" or not (x > 0 and cand[x - 1] == c)):
            places.append(c)
    if flaw != "ignores_other_targets":
        for f, t in enumerate(targets):
            if elig(t) and t not in cand and t not in targets[:f]:
                places.append(t)
    ranks = []
    ranked = CC.eligible_mask(s, exclude) if flaw == "counts_ineligible" else ok  # (that flaw is in the counting only)
    for t in targets:
        if not (0 <= t < n and ranked[t]):
            ranks.append(CC.RANK_NONE)
            continue
        ranks.append(1 + sum(1 for c in places if (c == t and flaw == "counts_itself") or (c != t and beats(c, t))))
    return ranks


FLAWS = ("duplicates_twice", "counts_itself", "ignores_other_targets", "ignores_exclusions", "greater_equal",
         "tie_reversed", "counts_ineligible", "drops_last_partial_64")


def _small_queries():
    """(case, query) pairs that a Python loop walks quickly: everything but the 20 000-candidate list's bulk."""
    for case in CC.cases():
        for b in range(min(case.query.shape[0], 40)):
            if len(case.cand[b]) <= 2000:
                yield case, b


def test_the_loop_model_without_a_flaw_is_the_reference():
    n = 0
    for case, b in _small_queries():
        for metric in ("dot", "l2"):
            s = CC.score_vector(case, b, metric)
            want = CC.rank_among_ref(s, case.cand[b], case.excl[b], case.tgts[b])[0]
            assert _flawed_ranks(None, s, case.cand[b], case.excl[b], case.tgts[b]) == want, (case.name, b, metric)
            n += len(want)
    assert n > 500


@pytest.mark.parametrize("flaw", FLAWS)
def test_a_wrong_kernel_fails_on_the_cases(flaw):
    caught = []
    for case, b in _small_queries():
        s = CC.score_vector(case, b, "dot")
        want = CC.rank_among_ref(s, case.cand[b], case.excl[b], case.tgts[b])[0]
        if _flawed_ranks(flaw, s, case.cand[b], case.excl[b], case.tgts[b]) != want:
            caught.append((case.name, b))
    print(f"{flaw}: wrong ranks on {len(caught)} queries, e.g. {caught[:3]}")
    assert caught, f"no case tells a kernel that {flaw} from a right one"


def test_reference_with_every_item_as_a_candidate_is_the_full_catalogue_rank():
    """S_q = every eligible item: ``rank_among_ref`` is ``rank_refs.ranks_from_scores`` (the property the device tests
    lean on: xfmr_candidate_ranks against xfmr_target_ranks)."""
    n = 0
    for case in CC.cases():
        n_rows = case.table.shape[0]
        everything = list(range(1, n_rows))
        for b in range(min(case.query.shape[0], 40)):
            for metric in ("dot", "l2"):
                s = CC.score_vector(case, b, metric)
                got = CC.rank_among_ref(s, everything, case.excl[b], case.tgts[b])[0]
                assert got == R.ranks_from_scores(s, case.excl[b], case.tgts[b]), (case.name, b, metric)
                # ... and the candidates given in any other form that covers the items: repeats, ids that are no item
                noisy = sorted(everything + everything[::3] + [0, -4, n_rows, n_rows + 9])
                assert CC.rank_among_ref(s, noisy, case.excl[b], case.tgts[b])[0] == got
                n += len(got)
    assert n > 1000


def test_the_cases_cover_their_edges():
    cs = CC.cases()
    assert {c.shape[2] for c in cs} == {4, 8, 36, 384, 1024}
    assert {c.shape[1] for c in cs} == {2, 65, 4097}
    assert {c.shape[0] for c in cs} == {1, 33, 257}
    sizes, counts, seen = set(), set(), set()
    for case in cs:
        n_rows = case.table.shape[0]
        for b, (c, ex, t) in enumerate(zip(case.cand, case.excl, case.tgts)):
            assert c == sorted(c) and ex == sorted(ex)
            sizes.add(len(c))
            counts.add(len(t))
            s = CC.score_vector(case, b, "dot")
            ok = CC.eligible_mask(s, ex)
            live = [x for x in t if 0 <= x < n_rows and ok[x]]
            seen |= {("target in list", bool(set(t) & set(c))), ("duplicate candidates", len(set(c)) < len(c)),
                     ("repeated target", len(set(t)) < len(t)), ("id 0", 0 in c), ("negative id", bool(c) and c[0] < 0),
                     ("id past the table", bool(c) and c[-1] >= n_rows), ("excluded candidate", bool(set(c) & set(ex))),
                     ("excluded target", bool(set(t) & set(ex))), ("inf candidate", case.inf_row in c),
                     ("inf target", case.inf_row in t), ("more than one chunk of targets", len(t) > 128),
                     ("long list with targets", len(c) >= CC.LONG_LIST and len(t) > 128)}
            for x in live:  # a tie with a candidate of lower and one of higher index
                tied = [y for y in set(c) if y != x and 0 <= y < n_rows and ok[y] and s[y] == s[x]]
                seen |= {("tie below", any(y < x for y in tied)), ("tie above", any(y > x for y in tied))}
    # (the lists carry a few ids that are no item on top of their drawn size)
    assert all(any(k <= n <= k + 12 for n in sizes) for k in (0, 1, 63, 64, 65, 100, 1000, CC.LONG_LIST)), sorted(sizes)
    assert {0, 1, 3} <= counts and any(n >= 130 for n in counts)
    for what in ("target in list", "duplicate candidates", "repeated target", "id 0", "negative id", "id past the table",
                 "excluded candidate", "excluded target", "inf candidate", "inf target", "more than one chunk of targets",
                 "long list with targets", "tie below", "tie above"):
        assert (what, True) in seen, what
    # first offset != 0
    flat, off = CC.csr([[1, 2], [], [3]], lead=4)
    assert off.tolist() == [4, 6, 6, 7] and flat.tolist() == [-99] * 4 + [1, 2, 3] + [-99]
