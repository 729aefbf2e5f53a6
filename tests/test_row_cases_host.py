"""What makes the cases of tests/row_cases.py worth their GPU time, shown on the CPU: through the SAME check_* helpers
test_gpu_row_kernels.py uses,
  (a) the fp32 model of every family passes every case of its table, and on the LayerNorm offset case with a margin:
      its error stays <= 1/4 of the tolerance (a width that breaks this gets a smaller offset, never a wider tolerance);
  (b) every mutant of row_cases.MUTANTS fails on a case this file names;
  (c) the row counts reach the plans, record counts and loop trips they are chosen for (by row_cases' plan rules, which
      test_row_plan_host.py holds the library to)."""

import pytest
import torch

import row_cases as RC
from helpers import TOL, max_scaled_err


def _worst(into, figs):
    for k, v in figs.items():
        into[k] = max(into.get(k, 0.0), v)


def _fig(tag, figs):
    """The model's worst error per output: the CPU column of profiles/row_kernels.md (pytest -s)."""
    print(f"FIG row-model {tag}: " + "  ".join(f"{k} {v:.2e}" for k, v in figs.items()))


def fails(fn):
    """True when the check raises its AssertionError (the mutant is caught)."""
    try:
        fn()
    except AssertionError:
        return True
    return False


# ---------------------------------------------------------------------------------------------------- (c) plans
def test_every_mutant_has_a_test_here():
    names = {n[len("test_mutant_"):] for n in globals() if n.startswith("test_mutant_")}
    assert names == set(RC.MUTANTS)


def test_widths_reach_every_instantiation_and_the_refusal():
    forms = {RC.ln_form(H) for H in RC.LN_WIDTHS}
    assert forms == {"npl1", "npl2", "npl4", "npl8", "npl16", "v4-16", "v4-32", "v4-64"}
    assert {H: RC.ln_form(H) for H in (63, 65, 129, 255, 320, 512, 768, 1024)} == {
        63: "npl1", 65: "npl2", 129: "npl4", 255: "npl4", 320: "npl8", 512: "npl8", 768: "npl16", 1024: "npl16"}
    assert all(RC.ln_form(H) is None for H in RC.LN_REFUSED)
    assert [RC.ln_form(H, aligned=False) for H in (64, 128, 256)] == ["npl1", "npl2", "npl4"]  # the unaligned fallback
    assert any(H % 4 for H in RC.LN_WIDTHS) and any(H % 64 and H > 64 for H in RC.LN_WIDTHS) and 384 in RC.LN_WIDTHS
    assert {RC.ln_form(H) for H in RC.EMBED_WIDTHS} == {"npl1", "npl2", "npl8", "npl16", "v4-16", "v4-32", "v4-64"}


def test_row_counts_reach_every_backward_plan():
    assert RC.ln_bwd_plan(77, 320) == (20, 4) and RC.ln_bwd_plan(77, 64) == (5, 16)  # what the older test reached
    for H, it in ((64, 16), (96, 4)):
        assert RC.ln_bwd_plan(4095, H) == (-(-4095 // it), it)  # one iteration per block (H = 96: 1 024 blocks, at the cap)
        assert RC.ln_bwd_plan(4096, H) == (256, 16)
        assert RC.ln_bwd_plan(16383, H) == (1024, 16)
        assert RC.ln_bwd_plan(16384, H) == (512, 32)
        blocks, rpb = RC.ln_bwd_plan(33001, H)
        assert -(-33001 // 32) > 1024 and rpb == (48 if H == 64 else 36) and 33001 % rpb == 25 and blocks == -(-33001 // rpb)
    for H, rows, records in RC.LN_RECORD_CASES:
        assert RC.ln_bwd_plan(rows, H)[0] == records
    assert sorted(r for _, _, r in RC.LN_RECORD_CASES) == [49, 50, 64, 65, 113]
    for H, edge in RC.LN_V4_EDGE_ROWS.items():  # forward: 256 / H rows per wave x 4 waves
        assert edge == (4 * 256 // H - 1, 4 * 256 // H, 4 * 256 // H + 1)


def test_row_counts_reach_the_row_sum_loop_and_the_column_sum_cap():
    assert [B for B, _ in RC.PARAM_SHAPES] == [1, 3, 17, 33, 130] and [L for _, L in RC.PARAM_SHAPES] == [1, 10, 13, 29, 5]
    assert sum(B >= 13 for B, _ in RC.PARAM_SHAPES) >= 3 and sum(L >= 13 for _, L in RC.PARAM_SHAPES) >= 2  # r + 12 < rows
    assert RC.colsum_plan(1000) == (4, 252) and RC.colsum_plan(256) == (1, 256) and RC.colsum_plan(257) == (2, 132)
    assert RC.colsum_plan(33000) == (127, 260) and -(-33000 // 256) > 128 and 33000 % 260  # capped, last block partial
    assert max(RC.PACKED_B) > 128 and 128 in RC.PACKED_B and 129 in RC.PACKED_B  # pos_grad_packed_kernel's second trip
    for B in RC.PACKED_B:
        ln = RC.packed_lengths(B)
        assert RC.PACKED_L in ln and (B == 1 or (0 in ln and 1 in ln)) and max(ln) <= RC.PACKED_L
    m = RC.pool_masks(9)
    assert m[0].all() and not m[1].any() and int(m[2].sum()) == 1 and m[3, 1] and not m[3, 2] and m[3, 3]


# ---------------------------------------------------------------------------------------------------- (a) models pass
@pytest.mark.parametrize("H", RC.LN_WIDTHS)
def test_layernorm_model_passes_every_width(H):
    worst = {}
    for rows in RC.LN_ROWS + RC.LN_V4_EDGE_ROWS.get(H, ()):
        case = RC.ln_case(H, rows)
        _worst(worst, RC.check_ln(case, RC.model_ln(case)))
        if H in (64, 128, 256):
            _worst(worst, RC.check_ln(case, RC.model_ln(case, form=RC.ln_form(H, aligned=False))))
    _fig(f"ln {RC.ln_form(H)} H={H}", worst)


@pytest.mark.parametrize("H", RC.LN_OFFSET_WIDTHS)
def test_layernorm_offset_case_separates_two_pass_from_one_pass(H):
    """The condition on the offset case: the two-pass fp32 model errs by <= tolerance / 4 (on every output), the one-pass
    E[x^2] - mean^2 model by >= 4 x the tolerance on y."""
    case = RC.ln_case(H, 77, "offset")
    figs = RC.check_ln(case, RC.model_ln(case))
    _fig(f"ln-offset {RC.ln_form(H)} H={H}", figs)
    assert max(figs[k] for k in ("y", "mean", "rstd")) <= TOL["fp32"]["val"] / 4, figs
    assert max(figs[k] for k in ("dx", "d_gamma", "d_beta", "d_bias")) <= TOL["fp32"]["grad_l2"] / 4, figs
    bad =RC.model_ln(case, mutant="one_pass_variance")
    assert max_scaled_err(bad["y"], case.ref["y"]) >= 4 * TOL["fp32"]["val"]


@pytest.mark.parametrize("H", RC.LN_PLAN_WIDTHS)
def test_layernorm_model_passes_every_row_plan(H):
    worst = {}
    for rows in RC.LN_PLAN_ROWS:
        case = RC.ln_case(H, rows)
        _worst(worst, RC.check_ln(case, RC.model_ln(case)))
    _fig(f"ln-plan {RC.ln_form(H)} H={H}", worst)


def test_layernorm_model_passes_every_record_count_and_dropout():
    worst = {}
    for H, rows, _ in RC.LN_RECORD_CASES:
        case = RC.ln_case(H, rows)
        _worst(worst, RC.check_ln(case, RC.model_ln(case)))
    _fig("ln-records", worst)
    for H in (64, 96):
        case = RC.ln_case(H, 77)
        ks = RC.keep_scale(7, 3, 77, H, 0.25)
        assert 0.6 < float((ks > 0).double().mean()) < 0.9 and float(ks.max()) == pytest.approx(4 / 3, rel=1e-6)
        m = RC.model_ln(case)
        dx, _, _, dbias, d_lin = RC.model_ln_bwd(case.dy, case.x, m["mean"], m["rstd"], case.gamma, form=RC.ln_form(H),
                                                 keep_scale=ks.float())
        want = case.ref["dx"] * ks
        _fig(f"ln-dropout H={H}", dict(d_lin=RC.assert_close("d_lin", d_lin, want, "fp32", "grad"),
                                       d_bias=RC.assert_close("d_bias", dbias, want.sum(0), "fp32", "grad")))


@pytest.mark.parametrize("H", RC.EMBED_WIDTHS)
def test_embed_model_passes(H):
    seen, worst = set(), {}
    for B, L in RC.EMBED_SHAPES:
        case = RC.embed_case(H, B, L)
        _worst(worst, RC.check_embed(case, RC.model_embed(case)))
        seen |= set(case.idx.flatten().tolist())
        assert case.pos.shape[0] > L
    n = RC.EMBED_V + 1
    assert {0, RC.EMBED_ZERO_ROW, n - 1, n, n + 5, -1, -(2 ** 40)} <= seen
    case = RC.embed_case(H, 3, 10)
    assert not case.ref["mask"].view(-1)[[0, 1, 2, 4, 5, 6]].any() and case.ref["mask"].view(-1)[3]
    _fig(f"embed {RC.ln_form(H)} H={H}", worst)


def test_param_grad_models_pass():
    worst, worst_packed = {}, {}
    for B, L in RC.PARAM_SHAPES:
        for H in RC.PARAM_WIDTHS:
            for extra in (0, 3):
                case = RC.param_case(B, L, H, extra)
                d_pos, d_type = RC.model_param_grads(case.d_pre, case.max_pos)
                _worst(worst, RC.check_param_grads(case, dict(d_pos=d_pos, d_type=d_type)))
    for B in RC.PACKED_B:
        for H in RC.PACKED_WIDTHS:
            case = RC.packed_case(B, H)
            d_pos, d_type = RC.ref_param_grads_packed(case.d_pre, case.lengths, case.L, case.max_pos, dtype=torch.float32)
            _worst(worst_packed, RC.check_param_grads(case, dict(d_pos=d_pos, d_type=d_type)))
    _fig("param_grads", worst)
    _fig("param_grads_packed", worst_packed)


@pytest.mark.parametrize("H", RC.ROW_WIDTHS)
def test_pool_and_normalise_models_pass(H):
    from oracle import encoder as enc

    worst = {}
    for B in RC.ROW_BATCHES:
        case = RC.pool_case(H, B)
        for mode in RC.POOL_MODES:
            want = RC.ref_pool(case.tok, case.mask, mode)
            e = RC.check_pool(f"pool H={H} B={B}", mode, RC.ref_pool(case.tok, case.mask, mode, dtype=torch.float32), want)
            _worst(worst, dict(pool_mean=e))
            # the oracle's restatement on fp64 inputs agrees with the reference written here
            assert torch.allclose(enc.pool(case.tok.double(), case.mask.long(), mode), want, rtol=1e-12, atol=1e-12), mode
            for normalize in (False, True):
                e = RC.check_pool(f"pool_rows H={H} B={B}", "mean" if normalize else mode,
                                  RC.ref_pool_rows(case.packed, case.lengths, mode, torch.float32, normalize),
                                  RC.ref_pool_rows(case.packed, case.lengths, mode, normalize=normalize))
                _worst(worst, {"pool_rows_normalized" if normalize else "pool_rows_mean": e})
        lc = RC.l2_case(H, B)
        y, dx = RC.model_l2(lc.x, lc.dy)
        _worst(worst, RC.check_l2(lc, y, dx))
        sq = RC._lane_sum(lc.x * lc.x)
        _worst(worst, dict(sq=RC.assert_close("sqnorm", sq, lc.ref["sq"], "fp32"),
                           rnorm=RC.assert_close("rnorm", 1.0 / sq.sqrt().clamp(min=1e-8), lc.ref["rnorm"], "fp32")))
        assert float(lc.ref["rnorm"][B]) == 1e8 and float(lc.ref["inv"][B]) == 1e12 and float(lc.ref["inv"][B + 2]) == 1e12
        assert float(lc.ref["inv"][B + 1]) == pytest.approx(1e10, rel=1e-6)
    _fig(f"pool+l2 H={H}", worst)


def test_scale_and_colsum_models_pass():
    for n in RC.SCALE_SIZES:
        x = RC.scale_case(n)
        for f in RC.SCALE_FACTORS:
            RC.check_scale(x, f, RC.model_scale(x, f))
    worst = {}
    for M, N in RC.colsum_shapes():
        case = RC.colsum_case(M, N)
        _worst(worst, {f"M={M}": RC.check_colsum(case, RC.model_colsum(case.a))})
    _fig("colsum", worst)
    assert (33000, 96) in RC.colsum_shapes() and (33000, 64) not in RC.colsum_shapes()


# ---------------------------------------------------------------------------------------------------- (b) mutants fail
def test_mutant_one_pass_variance():
    for H in RC.LN_OFFSET_WIDTHS:  # caught by the offset case at every width it is run at ...
        case = RC.ln_case(H, 77, "offset")
        assert fails(lambda: RC.check_ln(case, RC.model_ln(case, mutant="one_pass_variance"), only=("y",))), H
        plain = RC.ln_case(H, 77)  # ... and by it alone: on zero-mean rows the one-pass model passes
        RC.check_ln(plain, RC.model_ln(plain, mutant="one_pass_variance"))


def test_mutant_stat_skips_tail_columns():
    for H in (48, 63, 65, 100, 129, 255, 1000):  # every width that is no multiple of 64, at every row count
        for rows in RC.LN_ROWS:
            case = RC.ln_case(H, rows)
            assert fails(lambda: RC.check_ln(case, RC.model_ln(case, mutant="stat_skips_tail_columns"), only=("y", "mean"))), (H, rows)
    case = RC.embed_case(100, 3, 10)
    assert fails(lambda: RC.check_embed(case, RC.model_embed(case, mutant="stat_skips_tail_columns")))
    full = RC.ln_case(320, 77)  # a multiple of 64 has no such tail
    RC.check_ln(full, RC.model_ln(full, mutant="stat_skips_tail_columns"))


def test_mutant_reduce_stops_at_48():
    for H, rows, records in RC.LN_RECORD_CASES:
        case = RC.ln_case(H, rows)
        for k in ("d_gamma", "d_beta", "d_bias"):
            assert fails(lambda: RC.check_ln(case, RC.model_ln(case, mutant="reduce_stops_at_48"), only=(k,))), (records, k)
    for H in RC.LN_PLAN_WIDTHS:
        case = RC.ln_case(H, 4096)
        assert fails(lambda: RC.check_ln(case, RC.model_ln(case, mutant="reduce_stops_at_48"), only=("d_gamma",)))
    small = RC.ln_case(320, 77)  # 20 records: the older test's shape cannot see it
    RC.check_ln(small, RC.model_ln(small, mutant="reduce_stops_at_48"))


def test_mutant_rowsum_drops_partial_stride():
    m = "rowsum_drops_partial_stride"
    for B, L in ((17, 13), (33, 29), (130, 5)):
        case = RC.param_case(B, L, 64, 3)
        d_pos, d_type = RC.model_param_grads(case.d_pre, case.max_pos, mutant=m)
        assert fails(lambda: RC.check_param_grads(case, dict(d_pos=d_pos, d_type=d_type))), (B, L)
    for M in (255, 257, 1000, 33000):  # (256 rows are sixteen whole strides)
        case = RC.colsum_case(M, 96)
        assert fails(lambda: RC.check_colsum(case, RC.model_colsum(case.a, mutant=m))), M
    # the slow and the fast statement of the row-sum order agree on what the mutant drops
    a = RC.colsum_case(257, 64).a
    assert torch.allclose(RC.model_rowsum(a, 132), RC._fast_rowsum(a, 132), rtol=1e-5, atol=1e-5)


def test_mutant_gather_without_clamp():
    for H in (64, 100):
        for B, L in ((1, 1), (1, 5), (3, 10), (1, 67)):  # every B * L carries an out-of-range index that is not = 0 mod n_rows
            case = RC.embed_case(H, B, L)
            assert fails(lambda: RC.check_embed(case, RC.model_embed(case, mutant="gather_without_clamp"))), (H, B, L)


def test_mutant_mean_divides_by_L():
    for H in RC.ROW_WIDTHS:
        case = RC.pool_case(H, 3)  # a single-token sequence
        bad = RC.ref_pool(case.tok, case.mask, "mean", torch.float32, mutant="mean_divides_by_L")
        assert fails(lambda: RC.check_pool("pool", "mean", bad, RC.ref_pool(case.tok, case.mask, "mean"))), H
    full = RC.pool_case(64, 1)  # full length alone cannot see it
    RC.check_pool("pool", "mean", RC.ref_pool(full.tok, full.mask, "mean", torch.float32, mutant="mean_divides_by_L"),
                  RC.ref_pool(full.tok, full.mask, "mean"))


def test_mutant_lasttoken_takes_last_row():
    for H in RC.ROW_WIDTHS:
        case = RC.pool_case(H, 3)
        bad = RC.ref_pool(case.tok, case.mask, "lasttoken", torch.float32, mutant="lasttoken_takes_last_row")
        assert fails(lambda: RC.check_pool("pool", "lasttoken", bad, RC.ref_pool(case.tok, case.mask, "lasttoken"))), H


def test_mutant_scale_skips_tail():
    for n in (1, 3, 5, 1023, 262147):
        x = RC.scale_case(n)
        for f in (0.0, -2.5):
            assert fails(lambda: RC.check_scale(x, f, RC.model_scale(x, f, mutant="scale_skips_tail"))), (n, f)
    x = RC.scale_case(4)  # no tail
    RC.check_scale(x, -2.5, RC.model_scale(x, -2.5, mutant="scale_skips_tail"))
