"""CPU-side test (no GPU, nothing compiled) of tests/search_cases.py: the host model of the refined search keeps its own
contract on every named case, certifies what it should with room to spare, refuses what it must, and every plausible
wrong implementation is told from it by at least one case."""

import math

import pytest
import search_cases as S
import torch


@pytest.fixture(scope="module")
def cases():
    out = {}
    for c in S.host_cases():
        kw = {k: c[k] for k in ("max_norm", "max_rnorm") if k in c}
        want = S.exact_search(c["q"], c["table"], c["excl"], c["top_k"], c["metric"])
        got = S.model_search(c["q"], c["table"], c["excl"], c["top_k"], c["refine_factor"], c["metric"], **kw)
        out[c["name"]] = (c, kw, want, got)
    return out


def test_the_model_keeps_the_contract_on_every_case(cases):
    assert len(cases) == 17
    for name, (c, _, want, got) in cases.items():
        assert S.contract_problems(c, got, want) == [], name


def test_k_short_clamps_at_128_and_is_never_below_top_k():
    assert [S.k_short_of(k, r) for k, r in ((1, 1), (1, 4), (20, 4), (32, 4), (33, 4), (128, 1), (128, 4), (100, 4))] == [
        1, 4, 80, 128, 128, 128, 128, 128]


def test_unit_gaussians_are_certified_with_room_to_spare(cases):
    """V = 4 000, H = 64, top_k = 10, refine 4, 256 queries: every row certified, the smallest margin (k-th refined score
    - tau) at least twice the bound. Measured here: margin 0.0309, bound 0.00807."""
    _, _, _, got = cases["gaussian"]
    assert bool(got["certified"].all()) and len(got["margin"]) == 256
    assert max(got["bound"]) < 0.0081 and min(got["margin"]) >= 2 * max(got["bound"])
    _, _, _, got = cases["gaussian_top_excluded"]  # the 20 best of every row excluded: the shortlist starts behind them
    assert bool(got["certified"].all()) and min(got["margin"]) >= 2 * max(got["bound"])


@pytest.mark.parametrize("name,coarse_decoy,coarse_best,exact_decoy,exact_best", [
    ("adversary_dot_x1", 32.125, 32.0625, 32.1256, 32.1872),
    ("adversary_dot_x128", 128 * 32.125, 128 * 32.0625, 128 * 32.1256, 128 * 32.1872),
])
def test_the_rounding_adversary_is_what_it_says(cases, name, coarse_decoy, coarse_best, exact_decoy, exact_best):
    c, kw, want, got = cases[name]
    sc, sx = S.scores(c["q"], c["table"], c["metric"], coarse=True)[0], S.scores(c["q"], c["table"], c["metric"])[0]
    assert float(sc[1]) == coarse_decoy and float(sc[9]) == coarse_best  # exact in f32: sums of few bf16 values
    assert float(sx[1]) == pytest.approx(exact_decoy, rel=2e-6) and float(sx[9]) == pytest.approx(exact_best, rel=2e-6)
    assert got["shortlist"][0] == [1, 2, 3, 4] and int(want[0][0, 0]) == 9 and int(got["idx"][0, 0]) == 1
    assert not bool(got["certified"][0])
    zero = S.model_search(c["q"], c["table"], None, 1, 4, c["metric"], wrong="bound_zero", **kw)
    assert bool(zero["certified"][0])  # a zero bound would certify the wrong answer


@pytest.mark.parametrize("name", ["adversary_cosine_x1", "adversary_l2_x1", "adversary_l2_half_bound"])
def test_the_adversary_under_the_other_metrics(cases, name):
    c, _, want, got = cases[name]
    assert c["true_best"] not in got["shortlist"][0] and int(want[0][0, 0]) == c["true_best"]
    assert not bool(got["certified"][0]) and got["margin"][0] > 0  # (a zero bound would certify)


def test_the_equality_case_sits_exactly_on_the_bound(cases):
    c, kw, _, got = cases["equality"]
    assert S.f32(got["tau"][0]) + S.f32(got["bound"][0]) == got["score"][0, 0] and got["tau"][0] == 0.5
    assert not bool(got["certified"][0])


def test_ties_zero_and_non_finite_queries_stay_uncertified(cases):
    for name in ("duplicates_cosine", "duplicates_dot", "duplicates_l2", "zero_query", "nonfinite_query"):
        c, _, want, got = cases[name]
        assert not bool(got["certified"].any()), name
    _, _, want, got = cases["duplicates_cosine"]
    assert got["idx"][0].tolist() == [1, 2, 3, 4] == want[0][0].tolist()  # equal rows leave by ascending index
    _, _, want, got = cases["nonfinite_query"]
    assert bool((got["idx"] == -1).all()) and bool((want[0] == -1).all()) and all(math.isinf(b) for b in got["bound"])
    _, _, _, got = cases["zero_query"]
    assert math.isinf(got["bound"][0]) and got["idx"][0].tolist() == [1, 2, 3, 4, 5]


def test_rows_with_every_eligible_item_kept_are_certified(cases):
    for name in ("duplicates_all_kept", "few_left", "fewer_than_k_short"):
        _, _, want, got = cases[name]
        assert bool(got["certified"].all()) and torch.equal(got["idx"], want[0]) and all(t == -math.inf for t in got["tau"])
    _, _, _, got = cases["few_left"]
    assert sorted(got["idx"][0, :3].tolist()) == [28, 29, 30] and sorted(got["idx"][1, :3].tolist()) == [1, 2, 3]
    assert bool((got["idx"][:, 3:] == -1).all()) and bool((got["score"][:, 3:] == -math.inf).all())


def test_the_bound_refuses_where_an_assumption_fails():
    one = S.f32(1.0)
    for metric in (S.COSINE, S.DOT, S.L2):
        assert math.isfinite(float(S.bound(metric, one, 1.0, 1.0)))
        for qq, M, R in ((0.0, 1.0, 1.0), (math.inf, 1.0, 1.0), (math.nan, 1.0, 1.0), (2.0 ** 82, 1.0, 1.0),
                         (1.0, math.inf, 1.0), (1.0, math.nan, 1.0), (1.0, 2.0 ** 41, 1.0), (1.0, -1.0, 1.0),
                         (1.0, 1.0, math.inf), (1.0, 1.0, math.nan)):
            assert math.isinf(float(S.bound(metric, S.f32(qq), M, R))), (metric, qq, M, R)
    # cosine: beta; dot: beta |q| M; l2: twice that (and a few ulps of the squared lengths)
    assert float(S.bound(S.COSINE, one, 1.0, 1.0)) == pytest.approx(2.0 ** -7 + 2.0 ** -12, rel=3e-3)
    assert float(S.bound(S.DOT, S.f32(9.0), 5.0, 1.0)) == pytest.approx(15 * (2.0 ** -7 + 2.0 ** -12), rel=3e-3)
    assert float(S.bound(S.L2, S.f32(9.0), 5.0, 1.0)) == pytest.approx(30 * (2.0 ** -7 + 2.0 ** -12), rel=1e-2)


@pytest.mark.parametrize("wrong", S.WRONG)
def test_every_wrong_implementation_fails_on_some_case(cases, wrong):
    caught = []
    for name, (c, kw, want, _) in cases.items():
        if name == "gaussian" and wrong != "tau_at_top_k":
            continue  # (256 rows: only the variant that needs them)
        got = S.model_search(c["q"], c["table"], c["excl"], c["top_k"], c["refine_factor"], c["metric"], wrong=wrong, **kw)
        if S.contract_problems(c, got, want):
            caught.append(name)
    expected = {"bound_zero": "adversary_dot_x1", "dot_bound_without_item_norm": "adversary_dot_x128",
                "l2_bound_not_doubled": "adversary_l2_half_bound", "tau_at_top_k": "gaussian",
                "greater_or_equal": "equality", "ties_by_higher_index": "duplicates_all_kept",
                "excluded_kept_until_refine": "few_left", "padding_row_eligible": "padding_row_best"}
    assert expected[wrong] in caught, (wrong, caught)
