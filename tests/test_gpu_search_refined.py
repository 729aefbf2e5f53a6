"""xfmr_search_refined (ExactItemIndex.search_refined): the bf16 MFMA shortlist, the exact f32 refine and the
certificate, held to ExactItemIndex.search_batch bit for bit.

The contract: with exact=True every row is search_batch's row (torch.equal on idx and score); with exact=False every
CERTIFIED row is, and every other row is still a valid list (no padding row, excluded item or repeat; every score the
exact search's bits for its item; sorted by tt_better). The certificate must hold where it should (unit Gaussians:
every row) and must refuse where it must (the rounding adversary, ties, zero and non-finite queries). The shortlist
itself is compared with the host model only on inputs whose bf16 products and partial sums are exact in f32 in any
order; elsewhere the MFMA's summation order is the hardware's."""

import math

import pytest
import search_cases as S
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
METRICS = ("cosine", "dot", "l2")


def make_index(table, metric):
    from xfmr_rec_amd.retrieval import ExactItemIndex

    return ExactItemIndex(table.to(DEV), index_metric=metric)


def exact_bits_of(index, q, idx, excl):
    """The exact search's score bits for the items of idx (B, k), -inf where idx is -1: score_candidates on each row's
    items in ascending order, put back in the row's order."""
    B, k = idx.shape
    order = torch.argsort(idx, dim=1)
    srt = torch.gather(idx, 1, order)
    real = srt >= 0
    flat = srt[real]
    if flat.numel() == 0:  # (nothing to score: an empty candidate array has no address)
        return torch.full((B, k), -math.inf, device=idx.device)
    off =torch.zeros(B + 1, dtype=torch.int64, device=idx.device)
    off[1:] = real.sum(1).cumsum(0)
    ex = None
    if excl is not None:
        from xfmr_rec_amd.retrieval import sorted_exclusion_csr

        ex = tuple(torch.from_numpy(x).to(idx.device) for x in sorted_exclusion_csr(excl))
    sc = index.score_candidates(q, (flat.contiguous(), off), ex)
    out_sorted = torch.full((B, k), -math.inf, device=idx.device)
    out_sorted[real] = sc
    out = torch.empty_like(out_sorted)
    out.scatter_(1, order, out_sorted)
    return out


def check_contract(index, q, excl, top_k, refine, expect=None):
    """Runs the three forms and checks the contract; returns (certified, refined idx, exact idx) on the CPU."""
    want_idx, want_score = index.search_batch(q, excl, top_k=top_k)
    idx, score, cert = index.search_refined(q, excl, top_k=top_k, refine_factor=refine, exact=True)
    assert torch.equal(idx, want_idx) and torch.equal(score, want_score), "exact=True is not search_batch"
    ridx, rscore, rcert = index.search_refined(q, excl, top_k=top_k, refine_factor=refine, exact=False)
    assert torch.equal(rcert, cert) and rcert.dtype == torch.bool
    assert torch.equal(ridx[rcert], want_idx[rcert]) and torch.equal(rscore[rcert], want_score[rcert]), "a certified row differs"
    again = index.search_refined(q, excl, top_k=top_k, refine_factor=refine, exact=False)
    assert all(torch.equal(a, b) for a, b in zip(again, (ridx, rscore, rcert))), "two calls differ"
    # every row, certified or not, is a valid list
    n_rows = index.table.shape[0]
    real = ridx >= 0
    assert bool(((ridx >= 1) & (ridx < n_rows) | ~real).all()), "the padding row or an index out of range"
    assert bool((rscore[~real] == -math.inf).all()) and bool(torch.isfinite(rscore[real]).all())
    assert bool((real[:, :-1] | ~real[:, 1:]).all()), "padding inside a list"
    assert torch.equal(rscore, exact_bits_of(index, q, ridx, excl)), "a score is not the exact search's (or an excluded item)"
    a_s, b_s, a_i, b_i = rscore[:, :-1], rscore[:, 1:], ridx[:, :-1], ridx[:, 1:]
    better = (a_s > b_s) | ((a_s == b_s) & (a_i < b_i))
    assert bool((better | ~real[:, 1:]).all()), "not sorted by tt_better, or a repeat"
    if excl is not None:
        for b, ex in enumerate(excl):
            assert not set(ridx[b].tolist()) & set(int(x) for x in ex), b
    if expect == "all":
        assert bool(cert.all()), f"{int((~cert).sum())} of {cert.numel()} rows are not certified"
    if expect == "none":
        assert not bool(cert.any()), "a row that must stay uncertified is certified"
    return cert.cpu(), ridx.cpu(), want_idx.cpu()


def test_table_bf16_is_the_rounded_table_bit_for_bit():
    """The bound rests on it: xfmr_table_prepare rounds to nearest even as torch does (values around every tie)."""
    g = torch.Generator().manual_seed(5)
    table = torch.randn(257, 24, generator=g)
    table[1, :8] = torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -1 - 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -20, 65280.0, 1e-30, -0.0, 3.0])
    table[0] = 0
    index = make_index(table, "cosine")
    assert index.table_bf16.dtype == torch.bfloat16 and index.table_bf16.shape == table.shape
    assert torch.equal(index.table_bf16.view(torch.int16).cpu(), table.to(torch.bfloat16).view(torch.int16))
    big, small = index.norm_bounds
    norms = table[1:].double().norm(dim=1)
    assert norms.max() <= big <= norms.max() * 1.001 and (1 / norms.min()) <= small <= (1 / norms.min()) * 1.001


def exclusions(kind, index, q, n_rows, top_k, g):
    if kind == "none":
        return None
    B = q.shape[0]
    if kind == "few":  # leave three items (fewer than top_k wherever top_k > 3), unsorted and with repeats
        return [[j for j in range(n_rows - 1, 0, -1) if j not in (2, 5, n_rows - 1)] + [1, 1] for _ in range(B)]
    top = index.search_batch(q, None, top_k=min(5, top_k))[0].cpu()
    rnd = torch.randint(1, n_rows, (B, 7), generator=g)
    return [[int(x) for x in top[b] if x >= 0] + rnd[b].tolist() + [n_rows + 3, 0] for b in range(B)]


@pytest.mark.parametrize("H,n_rows,B,top_k,refine,excl_kind", [
    (8, 2, 1, 1, 4, "none"),          # one item
    (24, 128, 31, 20, 4, "top"),      # one tile exactly; H not a multiple of 16
    (64, 129, 32, 32, 4, "none"),     # k_short = 128 = every eligible item
    (384, 130, 33, 128, 4, "few"),    # the refine factor clamps to 1; exclusions leave fewer than top_k
    (1024, 4001, 65, 32, 4, "top"),   # the streaming form at its largest H and k_short = 128, several slices
    (384, 4001, 65, 20, 1, "none"),   # the prefetching form at its largest H, a partial last slice
    (64, 4001, 33, 1, 1, "top"),      # k_short = 1
    (1024, 130, 1, 20, 4, "few"),
    (24, 60, 31, 20, 4, "none"),      # fewer eligible items than k_short = 80
    (8, 4001, 32, 128, 1, "top"),
    (392, 300, 5, 20, 4, "none"),     # the first H of the streaming form: its last chunk holds half a k-step
])
def test_the_contract(H, n_rows, B, top_k, refine, excl_kind):
    g = torch.Generator().manual_seed(H * 7 + n_rows)
    table = torch.randn(n_rows, H, generator=g) * 0.5
    table[0] = 0
    q = (torch.randn(B, H, generator=g)).to(DEV)
    for metric in METRICS:
        index = make_index(table, metric)
        excl = exclusions(excl_kind, index, q, n_rows, top_k, g)
        cert, ridx, want = check_contract(index, q, excl, top_k, refine)
        if n_rows - 1 <= S.k_short_of(top_k, refine) and excl_kind != "top":
            assert bool(cert.all()), metric  # every eligible item kept: certified whatever the scores


def test_unit_gaussians_are_certified_row_by_row():
    """V = 4 000, H = 64, top_k = 10, refine 4, 256 queries: the host model certifies every row with the smallest margin at
    least twice the bound (tests/test_search_cases_host.py); the kernel must certify every row too, so the bit test above
    is not vacuous."""
    c = next(c for c in S.host_cases() if c["name"] == "gaussian")
    index = make_index(c["table"], "cosine")
    cert, _, _ = check_contract(index, c["q"].to(DEV), None, c["top_k"], c["refine_factor"], expect="all")
    assert cert.numel() == 256


@pytest.mark.parametrize("name", [c["name"] for c in S.host_cases() if c["name"] not in ("gaussian", "equality")])
def test_the_named_cases(name):
    """The host model's cases on the device: the contract, and certified / uncertified where the case says so. (The
    equality case is the model's alone: it sits on one particular f32 value of the bound.)"""
    c = next(c for c in S.host_cases() if c["name"] == name)
    index = make_index(c["table"], S.METRIC_NAMES[c["metric"]])
    cert, ridx, want = check_contract(index, c["q"].to(DEV), c["excl"], c["top_k"], c["refine_factor"], expect=c["expect"])
    if "true_best" in c:  # the shortlist misses the true best: the refined answer is a decoy, the exact one is not
        assert int(want[0, 0]) == c["true_best"] and int(ridx[0, 0]) != c["true_best"] and not bool(cert[0])
    if name == "adversary_dot_x1":
        assert int(ridx[0, 0]) == 1  # coarse scores exact in f32 in any order: the four kept decoys are items 1 .. 4


def test_the_shortlist_is_the_models_on_exactly_summable_inputs():
    """Values with magnitude in [1, 2) on a 2^-10 grid (and zeros): bf16 rounds them to a 2^-7 grid, products of two are
    multiples of 2^-14 below 4, and 64 of them sum exactly in f32 in any order. With refine_factor = 1 the returned items
    ARE the shortlist (re-ordered by exact score): the same set as the host model's, ties at its end cut by the lower
    index. Rows of equal items make such ties."""
    g = torch.Generator().manual_seed(11)
    V, H, B, k = 700, 64, 40, 16

    def grid(*shape):
        mag = 1 + torch.randint(0, 1024, shape, generator=g).float() / 1024
        sign = torch.randint(0, 3, shape, generator=g).float() - 1  # -1, 0, 1
        return mag * sign

    table, q = grid(V + 1, H), grid(B, H)
    table[0] = 0
    table[100:140] = table[100]  # forty equal items
    q[0] = table[100]            # ... that one query ranks first
    excl = [[int(x) for x in torch.randint(1, V + 1, (9,), generator=g)] for _ in range(B)]
    index = make_index(table, "dot")
    for ex in (None, excl):
        model = S.model_search(q, table, ex, k, 1, S.DOT)
        idx, score, cert = index.search_refined(q.to(DEV), ex, top_k=k, refine_factor=1, exact=False)
        for b in range(B):
            assert sorted(idx[b].tolist()) == sorted(model["shortlist"][b]), b
        assert sorted(idx[0].tolist()) == list(range(100, 116)) or ex is not None


def small_module(top_k=7):
    import xfmr_rec_amd as X

    conf = X.LightningConfig(hidden_size=64, num_attention_heads=2, intermediate_size=128, num_hidden_layers=2,
                             max_seq_length=16, precision="fp32", top_k=top_k)
    mod = X.RecommenderLightningModule(conf)
    mod.configure_model()
    g = torch.Generator().manual_seed(3)
    table = torch.randn(301, 64, generator=g)
    table[0] = 0
    mod.model.set_table(table.to(DEV))
    mod.eval()
    return mod, g


def test_recommend_batch_and_sessions_take_the_search_option(monkeypatch):
    monkeypatch.delenv("XFMR_SEARCH", raising=False)
    mod, g = small_module()
    hists = [[int(x) for x in torch.randint(1, 301, (n,), generator=g)] for n in (3, 16, 1, 9)] + [[]]
    want = mod.recommend_batch(hists, exclude_item_ids=hists)
    got = mod.recommend_batch(hists, exclude_item_ids=hists, search="refined")
    assert torch.equal(got["item_idx"], want["item_idx"]) and torch.equal(got["score"], want["score"])
    assert got["item_idx"][4].tolist() == [-1] * 7 and mod.items_index.table_bf16 is mod.model.table_bf16
    assert torch.equal(mod.recommend_batch(hists, top_k=3, search="refined")["item_idx"], mod.recommend_batch(hists, top_k=3)["item_idx"])
    with pytest.raises(ValueError, match="search must be one of"):
        mod.recommend_batch(hists, search="ann")
    rec = mod.open_sessions(4)
    for key, h in zip("abcd", hists):
        rec.start(key, h)
    want, got = rec.recommend("abcd"), rec.recommend("abcd", search="refined")
    assert torch.equal(got["item_idx"], want["item_idx"]) and torch.equal(got["score"], want["score"])
    got = rec.recommend("abcd", exclude_seen=False, search="refined")
    assert torch.equal(got["item_idx"], rec.recommend("abcd", exclude_seen=False)["item_idx"])


def test_the_environment_switch_routes_back_to_the_exact_search(monkeypatch):
    """On the rounding adversary the refined call proves nothing and (exact=False) returns a decoy; under XFMR_SEARCH=exact
    the same call is search_batch: the true best, every row reported as certified."""
    c = next(c for c in S.host_cases() if c["name"] == "adversary_dot_x1")
    index, q = make_index(c["table"], "dot"), c["q"].to(DEV)
    monkeypatch.delenv("XFMR_SEARCH", raising=False)
    idx, _, cert = index.search_refined(q, None, top_k=1, refine_factor=4, exact=False)
    assert int(idx[0, 0]) == 1 and not bool(cert[0])
    monkeypatch.setenv("XFMR_SEARCH", "exact")
    idx, score, cert = index.search_refined(q, None, top_k=1, refine_factor=4, exact=False)
    want = index.search_batch(q, None, top_k=1)
    assert int(idx[0, 0]) == 9 and bool(cert[0]) and torch.equal(idx, want[0]) and torch.equal(score, want[1])
    assert torch.equal(index.search_rows(q, None, top_k=1, search="refined")[0], want[0])


def test_arguments_are_checked():
    g = torch.Generator().manual_seed(1)
    table = torch.randn(50, 12, generator=g)
    index = make_index(table, "dot")
    q = torch.randn(3, 12, generator=g).to(DEV)
    with pytest.raises(RuntimeError, match="xfmr_search_refined failed"):
        index.search_refined(q, None, top_k=5)  # H = 12 is not a multiple of 8
    index = make_index(torch.randn(50, 16, generator=g), "dot")
    q = torch.randn(3, 16, generator=g).to(DEV)
    with pytest.raises(ValueError, match="refine_factor"):
        index.search_refined(q, None, top_k=5, refine_factor=0)
    with pytest.raises(ValueError, match="2 lists for 3 queries"):
        index.search_refined(q, [[1], [2]], top_k=5)
    with pytest.raises(RuntimeError, match="xfmr_search_refined failed"):
        index.search_refined(q, None, top_k=129)
    idx, score, cert = index.search_refined(q[:0], None, top_k=5)
    assert idx.shape == (0, 5) and score.shape == (0, 5) and cert.shape == (0,) and cert.dtype == torch.bool
