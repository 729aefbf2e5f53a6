"""The row kernels against fp64, every instantiation at the smallest shapes where it can go wrong: LayerNorm forward and
backward, gather + LayerNorm, the embedding-parameter gradients (padded and packed), pooling, L2 normalisation, the table
norms, the device-scalar scale (csrc/norm.hip, table_sqnorm_kernel of csrc/retrieval.hip) and the column sums
(rowsum_kernel / xfmr_colsum of csrc/gemm.hip). Cases, references and assertions are tests/row_cases.py's;
tests/test_row_cases_host.py shows on the CPU that they tell a right kernel from eight plausible wrong ones.

Every case runs twice and must be bit-equal: once through the C entry with every output pre-filled with NaN and
over-allocated by GUARD rows (which must still be NaN afterwards), once through the xfmr_rec_amd.ops wrapper where there
is one. Values are held to helpers.TOL["fp32"] (1e-4 scaled / rel-L2 1e-4), exact arithmetic to torch.equal.

The instantiation a case runs, its partial records and its rows per block are read from the library (xf_row_plan: the plan
the launchers themselves read) -- the test ids are built from them -- and every case asserts that they are what the rules of
row_cases.ln_form / ln_bwd_plan / colsum_plan say, the rules tests/test_row_plan_host.py holds the whole plan to. The record
tests tie the plan to the run: a NaN-filled workspace of the size query's bytes plus a guard holds exactly `records` finite
records afterwards.

Where the row counts come from:
* LayerNorm forward: one wave per row, four per workgroup -> rows 1, 3, 77; the float4 kernels hold 256 / H rows per wave ->
  one row below, at and above a workgroup's 16 / 8 / 4 rows at H = 64 / 128 / 256. Widths: two or three per instantiation,
  its first and last width among them; 1025 and 2048 are refused.
* LayerNorm backward row map: 4 095 | 4 096 rows (one iteration -> 16 rows per block), 16 383 | 16 384 (16 -> 32), 33 001 (1 032 blocks
  asked, capped at 1 024, rows per block rounded to whole iterations, the last block partial).
* ln_bwd_reduce_kernel: its unrolled loop needs 49 records (b + 48 < blocks): 49, 50, 64, 65 and 113 records from 196, 200,
  256, 260 and 452 rows at four rows per record.
* rowsum_kernel: its unrolled loop needs 13 rows (r + 12 < rows): B = 17, 33, 130 for d_pos, L = 13, 29 for d_type.
* column sums: 256 rows per block (255 | 256 | 257), at most 128 blocks (33 000 rows -> 127 blocks of 260, the last partial).
* pos_grad_packed_kernel: 16 waves x 8 sequences per trip -> B = 16 | 17 and 128 | 129, 300 for a third trip; H = 1024 asks
  for exactly 64 KiB of dynamic LDS."""

import math

import pytest
import torch

import row_cases as RC
from helpers import assert_close

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 2
NAN = float("nan")
f32 = torch.float32


@pytest.fixture(scope="module")
def ops():
    from xfmr_rec_amd import ops as _ops

    return _ops


@pytest.fixture(scope="module")
def N():
    from xfmr_rec_amd import _native

    _native.load()
    return _native


LN_FWD, GATHER_LN_FWD, LN_BWD, COLSUM = range(4)  # internal.h RowOp


def _plan(op, rows, H, keep=1, aligned=1):
    """xf_row_plan's answer for a key: (form name as row_cases.ln_form writes it, grid, rows_per_block, records, room)."""
    import ctypes

    from xfmr_rec_amd import _native

    out = (ctypes.c_int32 * 12)()
    rc = _native.load().xf_row_plan(op, rows, H, keep, int(aligned), out)
    form = None if rc else f"v4-{out[1]}" if out[0] == 2 else f"npl{out[1]}"
    return form, out[2], out[5], out[6], out[7]


def _form(H, aligned=True, op=LN_FWD):
    """The instantiation the library takes at width H (the test ids), held to the rule."""
    form = _plan(op, 77, H, 1, aligned)[0]
    assert form == RC.ln_form(H, aligned) == _plan(LN_BWD, 77, H, 1, aligned)[0], (H, aligned, form)
    return form


def _nan_ws(nbytes):
    """A float workspace of nbytes plus GUARD * 256 floats, all NaN."""
    assert nbytes % 4 == 0
    return torch.full((nbytes // 4 + GUARD * 256,), NAN, device=DEV)


def _finite_prefix(ws, n, what):
    """Exactly the first n floats of a NaN-filled workspace were written."""
    torch.cuda.synchronize()
    assert bool(ws[:n].isfinite().all()), f"{what}: fewer than {n} floats written"
    assert bool(ws[n:].isnan().all()), f"{what}: wrote past its {n} floats"


def _put(t, off=0):
    """Device copy of t whose storage starts `off` elements into its allocation (off = 1: no 16-byte alignment)."""
    base = torch.empty(t.numel() + off, dtype=t.dtype, device=DEV)
    v = base[off:].view(t.shape)
    v.copy_(t)
    return v


def _out(rows, cols=None, off=0, dtype=f32, fill=NAN):
    """(rows + GUARD[, cols]) filled with NaN, `off` elements into its allocation."""
    shape = (rows + GUARD,) if cols is None else (rows + GUARD, cols)
    base = torch.full((math.prod(shape) + off,), fill, dtype=dtype, device=DEV)
    return base[off:].view(shape)


def _used(t, rows, what):
    """The first `rows` rows of an over-allocated output, after checking that the guard rows are untouched."""
    g = t[rows:]
    assert bool(g.isnan().all() if t.is_floating_point() else (g == 0xFF).all()), f"{what}: wrote past its {rows} rows"
    return t[:rows]


def _same(a, b, what):
    for k in a:
        if a[k] is not None:
            assert torch.equal(a[k].cpu(), b[k].cpu()), f"{what}: {k} differs between two runs"


def _fig(tag, figs):
    print(f"FIG rows {tag}: " + "  ".join(f"{k} {v:.2e}" for k, v in figs.items()))


def _worst(into, figs):
    for k, v in figs.items():
        into[k] = max(into.get(k, 0.0), v)


# ---------------------------------------------------------------------------------------------------- LayerNorm
def _ln_direct(N, case, off=0, p=0.0, seed=0, site=0, ws=None):
    lib, st, rows, H = N.load(), N.stream(), case.rows, case.H
    x, gamma, beta, dy = (_put(t, off) for t in (case.x, case.gamma, case.beta, case.dy))
    y, mean, rstd = _out(rows, H, off), _out(rows), _out(rows)
    N.check(lib.xfmr_layernorm_fwd(N.ptr(x), N.ptr(gamma), N.ptr(beta), N.ptr(y), N.ptr(mean), N.ptr(rstd), rows, H,
                                   RC.LN_EPS, st), "xfmr_layernorm_fwd")
    dx, d_lin = _out(rows, H, off), (_out(rows, H, off) if p > 0 else None)
    dg, db, dbias = _out(1, H), _out(1, H), _out(1, H)
    if ws is None:
        ws = torch.empty(max(lib.xfmr_layernorm_bwd_workspace(rows, H), 16), dtype=torch.uint8, device=DEV)
    N.check(lib.xfmr_layernorm_bwd(N.ptr(dy), N.ptr(x), N.ptr(mean), N.ptr(rstd), N.ptr(gamma), N.ptr(dx), N.ptr(d_lin),
                                   N.ptr(dg), N.ptr(db), N.ptr(dbias), rows, H, p, seed, site, N.ptr(ws), st),
            "xfmr_layernorm_bwd")
    tag = f"ln H={H} rows={rows}"
    return dict(y=_used(y, rows, tag), mean=_used(mean, rows, tag), rstd=_used(rstd, rows, tag), dx=_used(dx, rows, tag),
                d_gamma=_used(dg, 1, tag)[0], d_beta=_used(db, 1, tag)[0], d_bias=_used(dbias, 1, tag)[0],
                d_lin=None if d_lin is None else _used(d_lin, rows, tag))


def _ln_ops(ops, case, p=0.0, seed=0, site=0):
    x, gamma, beta, dy = (t.to(DEV) for t in (case.x, case.gamma, case.beta, case.dy))
    y, mean, rstd = ops.layernorm_fwd(x, gamma, beta)
    dx, d_lin, dg, db, dbias = ops.layernorm_bwd(dy, x, mean, rstd, gamma, dropout_p=p, seed=seed, site=site)
    return dict(y=y, mean=mean, rstd=rstd, dx=dx, d_gamma=dg, d_beta=db, d_bias=dbias, d_lin=d_lin)


def _ln_twice(N, ops, case, off=0):
    got = _ln_direct(N, case, off)
    _same(got, _ln_ops(ops, case) if off == 0 else _ln_direct(N, case, off), f"ln H={case.H} rows={case.rows} off={off}")
    return RC.check_ln(case, got)


@pytest.mark.parametrize("H", RC.LN_WIDTHS, ids=[f"{_form(H)}-H{H}" for H in RC.LN_WIDTHS])
def test_layernorm_every_instantiation(N, ops, H):
    worst = {}
    for rows in RC.LN_ROWS + RC.LN_V4_EDGE_ROWS.get(H, ()):
        _worst(worst, _ln_twice(N, ops, RC.ln_case(H, rows)))
    _fig(f"ln {_form(H)} H={H}", worst)


@pytest.mark.parametrize("H", RC.LN_OFFSET_WIDTHS, ids=[f"{_form(H)}-H{H}" for H in RC.LN_OFFSET_WIDTHS])
def test_layernorm_offset_rows_need_a_two_pass_variance(N, ops, H):
    """x = 30 + 0.3 N(0,1): E[x^2] - mean^2 in fp32 errs by >= 9.7e-4 here, a two-pass variance by <= 1.9e-5."""
    _fig(f"ln-offset {_form(H)} H={H}", _ln_twice(N, ops, RC.ln_case(H, 77, "offset")))


@pytest.mark.parametrize("H", [64, 128, 256], ids=lambda H: f"{_form(H, aligned=False)}-H{H}-unaligned")
def test_layernorm_unaligned_pointers_take_the_generic_kernel(N, ops, H):
    """Every fp32 tensor one float into its allocation: the float4 kernels would fault or read shifted rows; the launchers
    take ln_fwd_kernel / ln_bwd_kernel <1 | 2 | 4> instead (same row plan)."""
    worst = {}
    for rows in RC.LN_ROWS + RC.LN_V4_EDGE_ROWS[H]:
        _worst(worst, _ln_twice(N, ops, RC.ln_case(H, rows), off=1))
    _fig(f"ln-unaligned {_form(H, aligned=False)} H={H}", worst)


@pytest.mark.parametrize("rows", RC.LN_PLAN_ROWS)
@pytest.mark.parametrize("H", RC.LN_PLAN_WIDTHS, ids=lambda H: f"{_form(H)}-H{H}")
def test_layernorm_backward_row_plans(N, ops, H, rows):
    _, grid, rpb, blocks, room = _plan(LN_BWD, rows, H)
    assert (blocks, rpb) == RC.ln_bwd_plan(rows, H) and grid == blocks <= room
    _fig(f"ln-plan {_form(H)} H={H} rows={rows} blocks={blocks} rows_per_block={rpb}", _ln_twice(N, ops, RC.ln_case(H, rows)))


LN_THRESHOLD_RECORD_CASES = tuple((H, rows, _plan(LN_BWD, rows, H)[3]) for H in RC.LN_PLAN_WIDTHS for rows in (4095, 4096))


@pytest.mark.parametrize("H,rows,records", RC.LN_RECORD_CASES + LN_THRESHOLD_RECORD_CASES,
                         ids=[f"records{r}-H{H}" for H, _, r in RC.LN_RECORD_CASES]
                         + [f"records{r}-H{H}-rows{rows}" for H, rows, r in LN_THRESHOLD_RECORD_CASES])
def test_layernorm_backward_partial_record_counts(N, ops, H, rows, records):
    """The plan tied to the run: the partials workspace, sized by xfmr_layernorm_bwd_workspace plus a guard and filled with NaN,
    holds exactly the plan's `records` records of 3 x H finite floats after the backward."""
    assert RC.ln_bwd_plan(rows, H)[0] == records
    _, _, rpb, plan_records, room = _plan(LN_BWD, rows, H)
    assert (plan_records, rpb) == RC.ln_bwd_plan(rows, H) and plan_records == records <= room
    nbytes = N.load().xfmr_layernorm_bwd_workspace(rows, H)
    assert nbytes == room * 3 * H * 4
    ws = _nan_ws(nbytes)
    got = _ln_direct(N, RC.ln_case(H, rows), ws=ws)
    _finite_prefix(ws, records * 3 * H, f"ln partials H={H} rows={rows}")
    _same(got, _ln_ops(ops, RC.ln_case(H, rows)), f"ln H={H} rows={rows}")
    _fig(f"ln-records {records} H={H} rows={rows}", RC.check_ln(RC.ln_case(H, rows), got))


@pytest.mark.parametrize("H", [64, 96], ids=lambda H: f"{_form(H)}-H{H}")
def test_layernorm_backward_linear_output_dropout(N, ops, H):
    """d_lin = dx * keep / (1 - p) with the host model's mask of (seed, site); d_bias = the column sums of d_lin."""
    case, p, seed, site = RC.ln_case(H, 77), 0.25, 7, 3
    got = _ln_direct(N, case, p=p, seed=seed, site=site)
    _same(got, _ln_ops(ops, case, p=p, seed=seed, site=site), f"ln dropout H={H}")
    ks = RC.keep_scale(seed, site, 77, H, p)
    figs = RC.check_ln(case, got, only=("y", "mean", "rstd", "dx", "d_gamma", "d_beta"))
    dx64 = got["dx"].double().cpu()
    assert torch.equal(got["d_lin"].cpu() == 0, (ks == 0) | (dx64 == 0)), "d_lin: not the host model's mask"
    figs["d_lin"] = assert_close("ln.d_lin", got["d_lin"], case.ref["dx"] * ks, "fp32", "grad")
    figs["d_bias"] = assert_close("ln.d_bias", got["d_bias"], (case.ref["dx"] * ks).sum(0), "fp32", "grad")
    _fig(f"ln-dropout {_form(H)} H={H}", figs)


@pytest.mark.parametrize("H", RC.LN_REFUSED)
def test_layernorm_refuses_widths_above_1024_and_writes_nothing(N, H):
    lib, st, rows = N.load(), N.stream(), 3
    x, v = torch.ones(rows, H, device=DEV), torch.ones(H, device=DEV)
    y, mean, rstd = _out(rows, H), _out(rows), _out(rows)
    with pytest.raises(RuntimeError, match="not supported"):
        N.check(lib.xfmr_layernorm_fwd(N.ptr(x), N.ptr(v), N.ptr(v), N.ptr(y), N.ptr(mean), N.ptr(rstd), rows, H, 1e-12, st), "fwd")
    dx, dg, db, dbias = _out(rows, H), _out(1, H), _out(1, H), _out(1, H)
    stat = torch.ones(rows, device=DEV)
    ws = torch.empty(max(lib.xfmr_layernorm_bwd_workspace(rows, H), 16), dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match="not supported"):
        N.check(lib.xfmr_layernorm_bwd(N.ptr(x), N.ptr(x), N.ptr(stat), N.ptr(stat), N.ptr(v), N.ptr(dx), None, N.ptr(dg),
                                       N.ptr(db), N.ptr(dbias), rows, H, 0.0, 0, 0, N.ptr(ws), st), "bwd")
    torch.cuda.synchronize()
    for t in (y, mean, rstd, dx, dg, db, dbias):
        assert bool(t.isnan().all())


@pytest.mark.parametrize("H", [64, 100], ids=lambda H: f"{_form(H)}-H{H}")
def test_layernorm_forward_only_and_bf16_copy_forms(N, H):
    """xf_layernorm_fwd_ex (extern "C", not in include/xfmr_hip.h; exported by the built library): with mean = rstd = NULL
    the forward-only instantiation, y bit-equal to the training form's; with y16 the bf16 copy = y.to(bfloat16) bit for bit."""
    lib, st = N.load(), N.stream()
    assert hasattr(lib, "xf_layernorm_fwd_ex")
    case = RC.ln_case(H, 77)
    rows = case.rows
    x, gamma, beta = (_put(t) for t in (case.x, case.gamma, case.beta))
    outs = {}
    for form, keep, with16 in (("train", True, False), ("infer", False, False), ("train16", True, True), ("infer16", False, True)):
        y, mean, rstd = _out(rows, H), _out(rows), _out(rows)
        y16 = _out(rows, H, dtype=torch.bfloat16) if with16 else None
        rc = lib.xf_layernorm_fwd_ex(N.ptr(x), N.ptr(gamma), N.ptr(beta), N.ptr(y), N.ptr(y16), N.ptr(mean) if keep else None,
                                     N.ptr(rstd) if keep else None, rows, H, RC.LN_EPS, st)
        N.check(rc, form)
        outs[form] = _used(y, rows, form)
        if keep:
            RC.check_ln(case, dict(y=outs[form], mean=_used(mean, rows, form), rstd=_used(rstd, rows, form)))
        else:
            assert bool(mean.isnan().all()) and bool(rstd.isnan().all())
        if with16:
            got16 = _used(y16, rows, form)
            assert torch.equal(got16.view(torch.int16), outs[form].to(torch.bfloat16).view(torch.int16)), form
    for form in ("infer", "train16", "infer16"):
        assert torch.equal(outs[form], outs["train"]), form


# ---------------------------------------------------------------------------------------------------- gather + LayerNorm
def _embed_direct(N, case, p=0.0, seed=0, site=0):
    lib, st, B, L, H = N.load(), N.stream(), case.B, case.L, case.H
    T = B * L
    idx, table, pos, typ, gamma, beta = (_put(t) for t in (case.idx, case.table, case.pos, case.typ, case.gamma, case.beta))
    out, pre, mean, rstd = _out(T, H), _out(T, H), _out(T), _out(T)
    mask = _out(T, dtype=torch.uint8, fill=0xFF)
    N.check(lib.xfmr_embed_ln_fwd(N.ptr(idx), N.ptr(table), case.n_rows, N.ptr(pos), N.ptr(typ), N.ptr(gamma), N.ptr(beta),
                                  N.ptr(out), N.ptr(pre), N.ptr(mean), N.ptr(rstd), N.ptr(mask), B, L, H, RC.LN_EPS, p, seed,
                                  site, st), "xfmr_embed_ln_fwd")
    tag = f"embed H={H} B={B} L={L}"
    return dict(out=_used(out, T, tag).view(B, L, H), pre=_used(pre, T, tag).view(B, L, H), mean=_used(mean, T, tag).view(B, L),
                rstd=_used(rstd, T, tag).view(B, L), mask=_used(mask, T, tag).view(B, L))


def _embed_ops(ops, case, **kw):
    out, pre, mean, rstd, mask = ops.embed_ln_fwd(*(t.to(DEV) for t in (case.idx, case.table, case.pos, case.typ, case.gamma,
                                                                         case.beta)), **kw)
    return dict(out=out, pre=pre, mean=mean, rstd=rstd, mask=mask)


@pytest.mark.parametrize("H", RC.EMBED_WIDTHS, ids=[f"{_form(H, op=GATHER_LN_FWD)}-H{H}" for H in RC.EMBED_WIDTHS])
def test_embedding_gather_layernorm(N, ops, H):
    """pre and the key mask exact; an index outside [0, n_rows) -- n_rows, n_rows + 5, -1, -2^40 -- reads row 0 and is masked;
    a non-padding all-zero row is masked; L < max_pos. With dropout: the undropped fp64 output times the host model's mask."""
    worst = {}
    for B, L in RC.EMBED_SHAPES:
        case = RC.embed_case(H, B, L)
        got = _embed_direct(N, case)
        _same(got, _embed_ops(ops, case), f"embed H={H} B={B} L={L}")
        _worst(worst, RC.check_embed(case, got))
    for B, L in ((3, 10), (1, 67)):
        case, p, seed = RC.embed_case(H, B, L), 0.1, 5
        got = _embed_direct(N, case, p=p, seed=seed, site=0)
        _same(got, _embed_ops(ops, case, dropout_p=p, seed=seed, site=0), f"embed dropout H={H}")
        ks = RC.keep_scale(seed, 0, B * L, H, p).view(B, L, H)
        assert torch.equal(got["out"].cpu() == 0, ks == 0), "embed dropout: not the host model's mask"
        worst["out_dropout"] = max(worst.get("out_dropout", 0.0), RC.check_embed(case, got, keep_scale=ks)["out"])
    _fig(f"embed {_form(H, op=GATHER_LN_FWD)} H={H}", worst)


# ---------------------------------------------------------------------------------------------------- d_pos / d_type
@pytest.mark.parametrize("H", RC.PARAM_WIDTHS)
@pytest.mark.parametrize("B,L", RC.PARAM_SHAPES, ids=lambda v: str(v))
def test_embed_param_grads(N, ops, B, L, H):
    lib, st, worst = N.load(), N.stream(), {}
    for extra in (0, 3):
        case = RC.param_case(B, L, H, extra)
        d_pre, d_pos, d_type = _put(case.d_pre), _out(case.max_pos, H), _out(2, H)
        N.check(lib.xfmr_embed_param_grads(N.ptr(d_pre), N.ptr(d_pos), N.ptr(d_type), B, L, H, case.max_pos, st), "param_grads")
        got = dict(d_pos=_used(d_pos, case.max_pos, "d_pos"), d_type=_used(d_type, 2, "d_type"))
        again = ops.embed_param_grads(d_pre, case.max_pos)
        _same(got, dict(d_pos=again[0], d_type=again[1]), f"param_grads B={B} L={L} H={H}")
        _worst(worst, RC.check_param_grads(case, got))
    _fig(f"param_grads B={B} L={L} H={H}", worst)


def _packed_direct(N, case, H=None):
    lib, st = N.load(), N.stream()
    H = case.H if H is None else H
    offs = torch.tensor([0] + list(torch.tensor(case.lengths).cumsum(0)), dtype=torch.int32, device=DEV)
    d_pre = _put(case.d_pre) if H == case.H else torch.zeros(case.d_pre.shape[0], H, device=DEV)
    d_pos, d_type = _out(case.max_pos, H), _out(2, H)
    rc = lib.xf_embed_param_grads_packed(N.ptr(d_pre), N.ptr(d_pos), N.ptr(d_type), N.ptr(offs), case.B, case.L, H, case.max_pos, st)
    return rc, d_pos, d_type


@pytest.mark.parametrize("H", RC.PACKED_WIDTHS)
@pytest.mark.parametrize("B", RC.PACKED_B, ids=lambda B: f"B{B}")
def test_embed_param_grads_packed(N, B, H):
    """xf_embed_param_grads_packed (extern "C", not in include/xfmr_hip.h): d_pos per position against fp64 -- a few wrong
    rows cannot hide in the norm of a whole flat gradient --, lengths 0, 1 and L, bit-equal between two runs."""
    assert hasattr(N.load(), "xf_embed_param_grads_packed")
    case = RC.packed_case(B, H)
    runs = []
    for _ in range(2):
        rc, d_pos, d_type = _packed_direct(N, case)
        N.check(rc, "xf_embed_param_grads_packed")
        runs.append(dict(d_pos=_used(d_pos, case.max_pos, "d_pos"), d_type=_used(d_type, 2, "d_type")))
    _same(runs[0], runs[1], f"packed B={B} H={H}")
    _fig(f"param_grads_packed B={B} H={H}", RC.check_param_grads(case, runs[0]))


def test_embed_param_grads_packed_refuses_width_1025(N):
    rc, d_pos, d_type = _packed_direct(N, RC.packed_case(3, 48), H=1025)
    with pytest.raises(RuntimeError, match="not supported"):
        N.check(rc, "xf_embed_param_grads_packed")
    torch.cuda.synchronize()
    assert bool(d_pos.isnan().all()) and bool(d_type.isnan().all())


# ---------------------------------------------------------------------------------------------------- pooling / norms
@pytest.mark.parametrize("H", RC.ROW_WIDTHS, ids=lambda H: f"H{H}")
def test_pooling_padded_and_packed(N, ops, H):
    """xfmr_pool and xfmr_pool_rows each against fp64 (not against each other): an empty sequence, a single token, an
    interior hole (padded form), full length; pool_rows with the fused normalisation against fp64 pool-then-normalise."""
    lib, st, worst = N.load(), N.stream(), {}
    for B in RC.ROW_BATCHES:
        case = RC.pool_case(H, B)
        tok, mask, packed = _put(case.tok), _put(case.mask.to(torch.uint8)), _put(case.packed)
        offs = torch.tensor([0] + list(torch.tensor(case.lengths).cumsum(0)), dtype=torch.int32, device=DEV)
        for mode in RC.POOL_MODES:
            out = _out(B, H)
            N.check(lib.xfmr_pool(N.ptr(tok), N.ptr(mask), N.ptr(out), B, case.L, H, N.POOL_MODES[mode], st), "xfmr_pool")
            got = _used(out, B, f"pool {mode}")
            assert torch.equal(got, ops.pool(tok, mask, mode)), f"pool {mode}: two runs differ"
            e = RC.check_pool(f"pool H={H} B={B}", mode, got, RC.ref_pool(case.tok, case.mask, mode))
            worst["pool_mean"] = max(worst.get("pool_mean", 0.0), e)
            for normalize in (False, True):
                out = _out(B, H)
                N.check(lib.xfmr_pool_rows(N.ptr(packed), N.ptr(offs), N.ptr(out), B, H, N.POOL_MODES[mode], int(normalize),
                                           RC.L2_EPS, st), "xfmr_pool_rows")
                got = _used(out, B, f"pool_rows {mode}")
                assert torch.equal(got, ops.pool_rows(packed, offs, mode, normalize=normalize)), f"pool_rows {mode}: two runs differ"
                want = RC.ref_pool_rows(case.packed, case.lengths, mode, normalize=normalize)
                e = RC.check_pool(f"pool_rows H={H} B={B}", "mean" if normalize else mode, got, want)
                k = "pool_rows_normalized" if normalize else "pool_rows_mean"
                worst[k] = max(worst.get(k, 0.0), e)
    _fig(f"pool H={H}", worst)


@pytest.mark.parametrize("H", RC.ROW_WIDTHS, ids=lambda H: f"H{H}")
def test_l2_normalize_and_table_norms(N, ops, H):
    """Rows: N(0,1), a zero row, a row of norm 1e-10, a row of norm 1e-13 (below eps = 1e-12: the clamped, linear branch)."""
    lib, st, worst = N.load(), N.stream(), {}
    for B in RC.ROW_BATCHES:
        case = RC.l2_case(H, B)
        rows = B + 3
        x, dy = _put(case.x), _put(case.dy)
        y, inv, dx = _out(rows, H), _out(rows), _out(rows, H)
        N.check(lib.xfmr_l2_normalize_fwd(N.ptr(x), N.ptr(y), N.ptr(inv), rows, H, RC.L2_EPS, st), "l2 fwd")
        N.check(lib.xfmr_l2_normalize_bwd(N.ptr(dy), N.ptr(y), N.ptr(inv), N.ptr(dx), rows, H, RC.L2_EPS, st), "l2 bwd")
        y, inv, dx = _used(y, rows, "l2 y"), _used(inv, rows, "l2 inv"), _used(dx, rows, "l2 dx")
        xa = x.clone().requires_grad_(True)
        ya = ops.l2_normalize(xa)
        ya.backward(dy)
        assert torch.equal(ya.detach(), y) and torch.equal(xa.grad, dx), "l2: two runs differ"
        figs = RC.check_l2(case, y, dx)
        figs["inv"] = assert_close("l2 inv", inv, case.ref["inv"], "fp32")
        for name, fn, entry in (("rnorm", ops.table_rnorm, lib.xfmr_table_rnorm), ("sq", ops.table_sqnorm, lib.xfmr_table_sqnorm)):
            o = _out(rows)
            N.check(entry(N.ptr(x), N.ptr(o), rows, H, st), name)
            o = _used(o, rows, name)
            assert torch.equal(o, fn(x)), f"{name}: two runs differ"
            figs[name] = assert_close(f"table {name} H={H}", o, case.ref[name], "fp32")
        _worst(worst, figs)
    _fig(f"l2 H={H}", worst)


# ---------------------------------------------------------------------------------------------------- scale / colsum
@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "unaligned"])
@pytest.mark.parametrize("n", RC.SCALE_SIZES, ids=lambda n: f"n{n}")
def test_scale_by_device_scalar(N, n, off):
    """One IEEE multiply per element: the CPU's fp32 product bit for bit. Scalar 1: untouched, a planted NaN included;
    scalar 0: the NaN stays NaN. off = 1: the view starts one float into its allocation (no float4 body)."""
    lib, st = N.load(), N.stream()
    x = RC.scale_case(n)
    for f in RC.SCALE_FACTORS:
        s = torch.tensor([f], device=DEV)
        runs = []
        for _ in range(2):
            base = torch.full((n + off + GUARD,), NAN, device=DEV)
            d = base[off:off + n]
            d.copy_(x)
            N.check(lib.xfmr_scale_by_device_scalar(N.ptr(d), n, N.ptr(s), st), "xfmr_scale_by_device_scalar")
            assert bool(base[off + n:].isnan().all()) and bool(base[:off].isnan().all())
            runs.append(d.cpu())
        assert torch.equal(runs[0].view(torch.int32), runs[1].view(torch.int32))
        RC.check_scale(x, f, runs[0])


@pytest.mark.parametrize("M,Nc", RC.colsum_shapes(), ids=lambda v: str(v))
def test_colsum(N, ops, M, Nc):
    lib, st = N.load(), N.stream()
    case = RC.colsum_case(M, Nc)
    """Against fp64, and the plan tied to the run: the workspace, sized by xfmr_colsum_workspace plus a guard and filled with
    NaN, holds exactly the plan's `blocks` records of N finite floats afterwards."""
    a, out = _put(case.a), _out(1, Nc)
    _, grid, rows_per, blocks, room = _plan(COLSUM, M, Nc)
    assert (blocks, rows_per) == RC.colsum_plan(M) and blocks <= room and grid == blocks * -(-Nc // 64)
    nbytes = lib.xfmr_colsum_workspace(M, Nc)
    assert nbytes == room * Nc * 4
    ws = _nan_ws(nbytes)
    N.check(lib.xfmr_colsum(N.ptr(a), N.ptr(out), M, Nc, N.ptr(ws), st), "xfmr_colsum")
    _finite_prefix(ws, blocks * Nc, f"colsum partials M={M} N={Nc}")
    got = _used(out, 1, "colsum")[0]
    assert torch.equal(got, ops.colsum(a)), "colsum: two runs differ"
    _fig(f"colsum M={M} N={Nc} blocks={blocks}", dict(sum=RC.check_colsum(case, got)))
