"""Cases, fp64 references and fp32 models of the row kernels (csrc/norm.hip, rowsum_kernel / xfmr_colsum of csrc/gemm.hip,
table_sqnorm_kernel of csrc/retrieval.hip). Plain module, no GPU and no library: shared by test_row_cases_host.py (which
shows on the CPU that the cases tell a right kernel from a subtly wrong one) and test_gpu_row_kernels.py (which holds the
kernels to the same references through the same `check_*` helpers).

* `ref_*`: the operation in fp64 on the fp32 INPUT VALUES, written from the definitions (BertEmbeddings / LayerNorm,
  sentence-transformers Pooling and Normalize, torch.nn.functional.normalize).
* `model_*`: the operation in fp32 the way the kernels compute it (lane-strided row sums and wave butterflies, partial
  records per workgroup and their fixed-order reduction, rows added one at a time). Not bit-exact restatements: they
  bound what a correct fp32 kernel errs by.
* `MUTANTS`: switches of those models, each a plausible kernel error. A case table is worth its GPU time when every
  mutant of its family fails on a case the test names.
* `check_*`: the assertions, with the project's tolerances (helpers.TOL["fp32"]: values 1e-4 scaled, gradients rel-L2
  1e-4) or torch.equal where the arithmetic is exact. They return the figures they measured.

`ln_form`, `ln_bwd_plan` and `colsum_plan` are the RULES of the row kernels' launch plan (csrc/row_plan.inc), written down
from the launchers that plan replaced: test_row_plan_host.py holds the library's plan to them key by key, the GPU tests read
the plan from the library and assert it equals them, the case tables derive their row counts from them, and
test_row_cases_host.py asserts what each count reaches."""

from __future__ import annotations

import functools
import types

import torch

import dropout_model as DM
from helpers import assert_close

F32, F64 = torch.float32, torch.float64
LN_EPS = 1e-12
MUTANTS = ("one_pass_variance", "stat_skips_tail_columns", "reduce_stops_at_48", "rowsum_drops_partial_stride",
           "gather_without_clamp", "mean_divides_by_L", "lasttoken_takes_last_row", "scale_skips_tail")


def _randn(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------ launch plans
def ln_form(H: int, aligned: bool = True) -> str:
    """The instantiation row_plan takes for LayerNorm forward and backward: 'v4-16' / 'v4-32' / 'v4-64' at H = 64 / 128 / 256 with
    16-byte aligned pointers, else 'npl<N>' with N = the power of two >= ceil(H / 64); None above H = 1024 (refused)."""
    if aligned and H in (64, 128, 256):
        return f"v4-{H // 4}"
    npl = _cdiv(H, 64)
    for n in (1, 2, 4, 8, 16):
        if npl <= n:
            return f"npl{n}"
    return None


def ln_bwd_plan(rows: int, H: int):
    """(records, rows_per_block) of row_plan for the LayerNorm backward: one workgroup iteration (16 / 8 / 4 rows at H = 64 / 128 / other) per
    block below 4 096 rows, 16 rows below 16 384, 32 from there; at most 1 024 blocks; whole iterations per block."""
    it = 16 if H == 64 else 8 if H == 128 else 4
    per = 32 if rows >= 16384 else 16 if rows >= 4096 else it
    blocks = min(max(_cdiv(rows, per), 1), 1024)
    rpb = _cdiv(_cdiv(rows, blocks), it) * it
    return _cdiv(rows, rpb), rpb


def colsum_plan(M: int):
    """(records, rows_per_block) of row_plan for the column sums: 256 rows per block, at most 128 blocks, rows_per a multiple of 4."""
    blocks = min(max(_cdiv(M, 256), 1), 128)
    rp = _cdiv(_cdiv(M, blocks), 4) * 4
    return _cdiv(M, rp), rp


# ------------------------------------------------------------------------------------------------ fp32 building blocks
def _butterfly(s):
    """xf_wave_sum / row_sum<LPR>: v += shfl_xor(v, o) for o = W/2 .. 1 over the last axis (a power of two)."""
    W = s.shape[-1]
    idx = torch.arange(W)
    o = W // 2
    while o:
        s = s + s[..., idx ^ o]
        o //= 2
    return s[..., 0]


def _lane_sum(v, form="npl"):
    """Row sums of fp32 (rows, H) in the kernels' order. 'npl': lane l adds columns l, l + 64, ... then the 64 lanes are
    combined; 'v4': lane l adds (c0 + c1) + (c2 + c3) of its four columns, then the H / 4 lanes are combined."""
    rows, H = v.shape
    if form == "v4":
        q = v.view(rows, H // 4, 4)
        return _butterfly((q[..., 0] + q[..., 1]) + (q[..., 2] + q[..., 3]))
    pad = (-H) % 64
    q = torch.nn.functional.pad(v, (0, pad)).view(rows, -1, 64)
    s = torch.zeros(rows, 64, dtype=v.dtype)
    for i in range(q.shape[1]):
        s = s + q[:, i]
    return _butterfly(s)


def model_rowsum(src, rows_per=None, mutant=None):
    """rowsum_kernel: (rows, cols) fp32 -> (ceil(rows / rows_per), cols). Per block, row group g of 4 adds rows g, g + 4,
    ... in four accumulators (rows 16 apart share one) while 16 rows are left, the rest into the first; then
    (s0 + s1) + (s2 + s3) and the four groups pairwise. mutant 'rowsum_drops_partial_stride': the rest is never added."""
    rows, cols = src.shape
    rows_per = rows if rows_per is None else rows_per
    out = []
    for r0 in range(0, rows, rows_per):
        blk = src[r0:min(r0 + rows_per, rows)]
        n = blk.shape[0]
        groups = []
        for g in range(4):
            s = [torch.zeros(cols, dtype=F32) for _ in range(4)]
            r = g
            while r + 12 < n:
                for u in range(4):
                    s[u] = s[u] + blk[r + 4 * u]
                r += 16
            if mutant != "rowsum_drops_partial_stride":
                while r < n:
                    s[0] = s[0] + blk[r]
                    r += 4
            groups.append((s[0] + s[1]) + (s[2] + s[3]))
        out.append((groups[0] + groups[1]) + (groups[2] + groups[3]))
    return torch.stack(out)


def _fast_rowsum(src, rows_per, mutant=None):
    """model_rowsum for many rows: the same grouping (block, row group, accumulator) with torch sums inside an accumulator."""
    rows, cols = src.shape
    nb = _cdiv(rows, rows_per)
    pad = nb * rows_per - rows
    assert rows_per % 4 == 0
    keep = torch.ones(nb * rows_per, dtype=torch.bool)
    if mutant == "rowsum_drops_partial_stride":  # per block, rows from the last whole 16-row stride on
        for b in range(nb):
            n = min(rows_per, rows - b * rows_per)
            keep[b * rows_per + 16 * (n // 16):(b + 1) * rows_per] = False
    x = torch.nn.functional.pad(src, (0, 0, 0, pad)) * keep[:, None]
    x = x.view(nb, rows_per // 4, 4, cols).sum(1)  # row groups
    return (x[:, 0] + x[:, 1]) + (x[:, 2] + x[:, 3])


# ------------------------------------------------------------------------------------------------ LayerNorm
def ref_ln_fwd(x, gamma, beta, eps=LN_EPS):
    x, gamma, beta = x.double(), gamma.double(), beta.double()
    mean = x.mean(-1)
    d = x - mean[:, None]
    rstd = ((d * d).mean(-1) + eps).rsqrt()
    return d * rstd[:, None] * gamma + beta, mean, rstd


def ref_ln_bwd(dy, x, gamma, eps=LN_EPS):
    """dx, d_gamma, d_beta and the bias gradient sum_rows(dx) of the Linear that feeds the LayerNorm."""
    dy, gamma = dy.double(), gamma.double()
    _, mean, rstd = ref_ln_fwd(x, gamma, gamma, eps)
    xh = (x.double() - mean[:, None]) * rstd[:, None]
    g = dy * gamma
    dx = rstd[:, None] * (g - g.mean(-1, keepdim=True) - xh * (g * xh).mean(-1, keepdim=True))
    return dx, (dy * xh).sum(0), dy.sum(0), dx.sum(0)


def model_ln_fwd(x, gamma, beta, eps=LN_EPS, form="npl", mutant=None):
    rows, H = x.shape
    form = "v4" if form.startswith("v4") else "npl"
    stat = (lambda v: _lane_sum(v, form))
    if mutant == "stat_skips_tail_columns":  # the statistic stops at the last whole 64-column group
        stat = (lambda v: _lane_sum(v[:, :64 * (H // 64)], "npl") if H >= 64 else torch.zeros(rows))
    Hf = torch.tensor(float(H), dtype=F32)
    mean = stat(x) / Hf
    d = x - mean[:, None]
    if mutant == "one_pass_variance":
        var = (stat(x * x) / Hf - mean * mean).clamp(min=0)
    else:
        var = stat(d * d) / Hf
    rstd = (var + torch.tensor(eps, dtype=F32)).rsqrt()
    return d * rstd[:, None] * gamma + beta, mean, rstd


def model_ln_reduce(records, mutant=None):
    """ln_bwd_reduce_kernel: records (blocks, 3, H); record group g of 16 adds records g, g + 16, ..., then the groups."""
    if mutant == "reduce_stops_at_48":
        records = records[:48]
    nb = records.shape[0]
    pad = (-nb) % 16
    r = torch.nn.functional.pad(records, (0, 0, 0, 0, 0, pad)).view(-1, 16, *records.shape[1:])
    s = torch.zeros(16, *records.shape[1:], dtype=F32)
    for i in range(r.shape[0]):
        s = s + r[i]
    out = torch.zeros(records.shape[1:], dtype=F32)
    for g in range(16):
        out = out + s[g]
    return out


def model_ln_bwd(dy, x, mean, rstd, gamma, form="npl", mutant=None, keep_scale=None):
    """fp32: dx per row with lane-strided row means; (d_gamma, d_beta, d_bias) as per-block partial records of
    ln_bwd_plan reduced by model_ln_reduce. keep_scale: the Linear-output dropout's keep / (1 - p); d_lin = dx * keep_scale
    and d_bias sums d_lin."""
    rows, H = x.shape
    form = "v4" if form.startswith("v4") else "npl"
    Hf = torch.tensor(float(H), dtype=F32)
    xh = (x - mean[:, None]) * rstd[:, None]
    g = dy * gamma
    mg, mgx = _lane_sum(g, form) / Hf, _lane_sum(g * xh, form) / Hf
    dx = rstd[:, None] * (g - mg[:, None] - xh * mgx[:, None])
    d_lin = dx if keep_scale is None else dx * keep_scale
    blocks, rpb = ln_bwd_plan(rows, H)
    three = torch.stack([dy * xh, dy, d_lin], 1).reshape(rows, 3 * H)
    rec = _fast_rowsum(three, rpb).view(blocks, 3, H)
    red = model_ln_reduce(rec, mutant)
    return dx, red[0], red[1], red[2], (None if keep_scale is None else d_lin)


# widths by instantiation (row_plan); 1025 and 2048 are refused
LN_WIDTHS = (1, 48, 63, 65, 100, 129, 192, 255, 320, 384, 512, 768, 1000, 1024, 64, 128, 256)
LN_REFUSED = (1025, 2048)
LN_ROWS = (1, 3, 77)  # one wave of a workgroup, three of four, twenty workgroups with the last one partial
LN_V4_EDGE_ROWS = {64: (15, 16, 17), 128: (7, 8, 9), 256: (3, 4, 5)}  # one below / at / above one workgroup's rows
LN_OFFSET_WIDTHS = (64, 100, 384, 1024)
# backward row plans (ln_bwd_plan), H = 64 and 96: the last count with one iteration per block and the first with 16 rows;
# the last with 16 and the first with 32; 33 001 rows ask for 1 032 blocks of 32 -> capped at 1 024 -> 33 rows per block,
# rounded to whole iterations (48 at H = 64, 36 at H = 96): 33 001 = 687 * 48 + 25 = 916 * 36 + 25, a partial last block
LN_PLAN_WIDTHS = (64, 96)
LN_PLAN_ROWS = (4095, 4096, 16383, 16384, 33001)
# partial-record counts of the reduction (4 rows per record below 4 096 rows at these widths): 49 is the first count at
# which ln_bwd_reduce_kernel's unrolled loop runs (b + 48 < blocks), 50 the issue's example, 64 / 65 the first second-trip
# boundary of record group 0, 113 the first count with two unrolled trips and a tail
LN_RECORD_CASES = ((96, 196, 49), (320, 200, 50), (96, 256, 64), (96, 260, 65), (96, 452, 113))


@functools.lru_cache(maxsize=64)
def ln_case(H: int, rows: int, kind: str = "normal"):
    """fp32 inputs and fp64 references of one LayerNorm case (read only: shared). kind 'offset': x = 30 + 0.3 N(0,1), the
    case that tells a two-pass variance from E[x^2] - mean^2; gamma, beta, dy as everywhere."""
    x = _randn(rows, H, seed=1)
    if kind == "offset":
        x = 30 + 0.3 * x
    gamma, beta, dy = 1 + 0.1 * _randn(H, seed=2), 0.1 * _randn(H, seed=3), _randn(rows, H, seed=4)
    y, mean, rstd = ref_ln_fwd(x, gamma, beta)
    dx, dg, db, dbias = ref_ln_bwd(dy, x, gamma)
    return types.SimpleNamespace(H=H, rows=rows, kind=kind, x=x, gamma=gamma, beta=beta, dy=dy,
                                 ref=dict(y=y, mean=mean, rstd=rstd, dx=dx, d_gamma=dg, d_beta=db, d_bias=dbias))


def model_ln(case, form=None, mutant=None):
    form = form or ln_form(case.H)
    y, mean, rstd = model_ln_fwd(case.x, case.gamma, case.beta, form=form, mutant=mutant)
    dx, dg, db, dbias, _ = model_ln_bwd(case.dy, case.x, mean, rstd, case.gamma, form=form, mutant=mutant)
    return dict(y=y, mean=mean, rstd=rstd, dx=dx, d_gamma=dg, d_beta=db, d_bias=dbias)


def check_ln(case, got, only=None):
    """got: y, mean, rstd (values) and dx, d_gamma, d_beta, d_bias (gradients) of the case; returns {name: error}."""
    figs = {}
    for k in ("y", "mean", "rstd"):
        if k in got and (only is None or k in only):
            figs[k] = assert_close(f"ln.{k} H={case.H} rows={case.rows} {case.kind}", got[k], case.ref[k], "fp32")
    for k in ("dx", "d_gamma", "d_beta", "d_bias"):
        if k in got and (only is None or k in only):
            figs[k] = assert_close(f"ln.{k} H={case.H} rows={case.rows} {case.kind}", got[k], case.ref[k], "fp32", "grad")
    return figs


# ------------------------------------------------------------------------------------------------ gather + LayerNorm
EMBED_WIDTHS = (64, 128, 256, 48, 100, 384, 1024)
EMBED_SHAPES = ((1, 1), (1, 5), (3, 10), (1, 67))  # B * L = 1, 5, 30, 67: one lane group, a partial wave, partial workgroups
EMBED_V, EMBED_ZERO_ROW = 20, 7


@functools.lru_cache(maxsize=64)
def embed_case(H: int, B: int, L: int):
    """Table of EMBED_V + 1 rows (row 0 and the non-padding row 7 all zero), max_pos = L + 3, and indices that include 0,
    the zero row, n_rows - 1 and the out-of-range n_rows, n_rows + 5, -1, -2^40 (all of them from B * L = 30 on)."""
    n_rows = EMBED_V + 1
    table = _randn(n_rows, H, seed=11)
    table[0] = 0
    table[EMBED_ZERO_ROW] = 0
    pos, typ = 0.02 * _randn(L + 3, H, seed=13), 0.02 * _randn(2, H, seed=14)
    gamma, beta = 1 + 0.1 * _randn(H, seed=15), 0.1 * _randn(H, seed=16)
    idx = torch.randint(1, n_rows, (B * L,), generator=torch.Generator().manual_seed(12))
    special = [n_rows + 5, -1, EMBED_ZERO_ROW, n_rows - 1, -(2 ** 40), n_rows, 0]
    if B * L > 1:
        k = min(len(special), B * L)
        idx[:k] = torch.tensor(special[:k])
    else:
        idx[0] = n_rows + 5
    idx = idx.view(B, L)
    pre, mask = ref_embed_pre(idx, table, pos, typ)
    y, mean, rstd = ref_ln_fwd(pre.view(B * L, H), gamma, beta)
    return types.SimpleNamespace(H=H, B=B, L=L, n_rows=n_rows, idx=idx, table=table, pos=pos, typ=typ, gamma=gamma, beta=beta,
                                 ref=dict(pre=pre, mask=mask, out=y.view(B, L, H), mean=mean.view(B, L), rstd=rstd.view(B, L)))


def ref_embed_pre(idx, table, pos, typ, mutant=None):
    """BertEmbeddings' sum before its LayerNorm, in fp32 with the kernel's association (e + type_0) + pos_l -- three fp32
    numbers added in a fixed order: exact to compare -- and the key mask 'any non-zero in the gathered row'. An index
    outside [0, n_rows) reads row 0 (and so is masked). mutant 'gather_without_clamp': it reads row idx mod n_rows."""
    B, L = idx.shape
    n_rows = table.shape[0]
    if mutant == "gather_without_clamp":
        item = idx % n_rows
    else:
        item = torch.where((idx < 0) | (idx >= n_rows), torch.zeros_like(idx), idx)
    e = table[item]
    return (e + typ[0]) + pos[:L][None], (e != 0).any(-1)


def model_embed(case, mutant=None):
    pre, mask = ref_embed_pre(case.idx, case.table, case.pos, case.typ, mutant)
    y, mean, rstd = model_ln_fwd(pre.view(-1, case.H), case.gamma, case.beta, form=ln_form(case.H), mutant=mutant)
    return dict(pre=pre, mask=mask, out=y.view_as(pre), mean=mean.view(case.B, case.L), rstd=rstd.view(case.B, case.L))


def check_embed(case, got, keep_scale=None):
    """pre and mask exact; out / mean / rstd against fp64. keep_scale (B, L, H): out is held to ref * keep_scale."""
    tag = f"embed H={case.H} B={case.B} L={case.L}"
    assert torch.equal(got["pre"].cpu(), case.ref["pre"]), f"{tag}: pre differs"
    assert torch.equal(got["mask"].cpu().bool(), case.ref["mask"]), f"{tag}: key mask differs"
    want = case.ref["out"] if keep_scale is None else case.ref["out"] * keep_scale
    figs = dict(out=assert_close(f"{tag} out", got["out"], want, "fp32"))
    for k in ("mean", "rstd"):
        figs[k] = assert_close(f"{tag} {k}", got[k], case.ref[k], "fp32")
    return figs


def keep_scale(seed, site, rows, cols, p):
    """keep / (1 - p) of a hidden-state dropout site as an fp64 (rows, cols) tensor (tests/dropout_model.py)."""
    return torch.from_numpy(DM.hidden_keep(seed, site, rows, cols, p).astype("float64")) * DM.scale(p)


# ------------------------------------------------------------------------------------------------ d_pos / d_type
PARAM_SHAPES = ((1, 1), (3, 10), (17, 13), (33, 29), (130, 5))  # (B, L): rowsum rows = B for d_pos, L for d_type
PARAM_WIDTHS = (48, 64, 384)
PACKED_B = (1, 16, 17, 128, 129, 300)  # 16 waves of sequences; 128 = one trip of pos_grad_packed_kernel's outer loop
PACKED_WIDTHS = (48, 64, 384, 1024)
PACKED_L = 6


def ref_param_grads(d_pre, max_pos):
    B, L, H = d_pre.shape
    d_pos = torch.zeros(max_pos, H, dtype=F64)
    d_pos[:L] = d_pre.double().sum(0)
    d_type = torch.zeros(2, H, dtype=F64)
    d_type[0] = d_pos.sum(0)
    return d_pos, d_type


def model_param_grads(d_pre, max_pos, mutant=None):
    B, L, H = d_pre.shape
    d_pos = torch.zeros(max_pos, H, dtype=F32)
    d_pos[:L] = model_rowsum(d_pre.view(B, L * H), mutant=mutant).view(L, H)
    d_type = torch.zeros(2, H, dtype=F32)
    d_type[0] = model_rowsum(d_pos[:L], mutant=mutant)[0]
    return d_pos, d_type


def packed_lengths(B: int, L: int = PACKED_L):
    """Lengths that include 0, 1 and L (B = 1: L alone), the rest cycling through 0 .. L."""
    base = [L, 0, 1]
    return [(base[b] if b < 3 else (b * 5) % (L + 1)) for b in range(B)]


def ref_param_grads_packed(d_pre, lengths, L, max_pos, dtype=F64):
    """d_pos[p] = sum over the sequences longer than p of their row p, in ascending sequence order."""
    H = d_pre.shape[1]
    d_pos = torch.zeros(max_pos, H, dtype=dtype)
    o = 0
    for n in lengths:
        d_pos[:n] += d_pre[o:o + n].to(dtype)
        o += n
    d_type = torch.zeros(2, H, dtype=dtype)
    d_type[0] = d_pos[:L].sum(0)
    return d_pos, d_type


@functools.lru_cache(maxsize=32)
def param_case(B: int, L: int, H: int, extra: int):
    d_pre = _randn(B, L, H, seed=21)
    d_pos, d_type = ref_param_grads(d_pre, L + extra)
    return types.SimpleNamespace(B=B, L=L, H=H, max_pos=L + extra, d_pre=d_pre, ref=dict(d_pos=d_pos, d_type=d_type))


@functools.lru_cache(maxsize=32)
def packed_case(B: int, H: int):
    L, lengths = PACKED_L, packed_lengths(B)
    d_pre = _randn(max(sum(lengths), 1), H, seed=22)
    d_pos, d_type = ref_param_grads_packed(d_pre, lengths, L, L + 2)
    return types.SimpleNamespace(B=B, L=L, H=H, max_pos=L + 2, lengths=lengths, d_pre=d_pre,
                                 ref=dict(d_pos=d_pos, d_type=d_type))


def check_param_grads(case, got):
    """d_pos per position and d_type[0] against fp64 (a position no sequence reaches is an exact zero row); rows L ..
    max_pos - 1 of d_pos and d_type[1] are exact zeros."""
    tag = f"param_grads B={case.B} L={case.L} H={case.H}"
    d_pos, d_type = got["d_pos"].cpu(), got["d_type"].cpu()
    worst = 0.0
    for p in range(case.L):  # per position: a wrong row cannot hide in the norm of the others
        worst = max(worst, assert_close(f"{tag} d_pos[{p}]", d_pos[p], case.ref["d_pos"][p], "fp32", "grad"))
    assert torch.equal(d_pos[case.L:], torch.zeros(case.max_pos - case.L, case.H)), f"{tag}: d_pos tail not zero"
    assert torch.equal(d_type[1], torch.zeros(case.H)), f"{tag}: d_type[1] not zero"
    return dict(d_pos=worst, d_type=assert_close(f"{tag} d_type[0]", d_type[0], case.ref["d_type"][0], "fp32", "grad"))


# ------------------------------------------------------------------------------------------------ pooling / normalise
POOL_MODES = ("mean", "max", "cls", "lasttoken")
ROW_WIDTHS = (1, 48, 64, 100, 384, 1024)
ROW_BATCHES = (1, 3, 4, 5, 9)  # one wave; three of a workgroup's four; a full workgroup; one more; three workgroups
POOL_L = 7
L2_EPS = 1e-12


def pool_masks(B: int, L: int = POOL_L):
    """(B, L) bool: full length, an empty sequence, a single token, an interior hole, then lengths cycling 2 .. L."""
    m = torch.zeros(B, L, dtype=torch.bool)
    for b in range(B):
        if b == 0:
            m[b] = True
        elif b == 2:
            m[b, 0] = True
        elif b == 3:
            m[b, :5] = True
            m[b, 2] = False
        elif b > 3:
            m[b, :2 + (b * 3) % (L - 1)] = True
    return m


def ref_pool(tok, mask, mode, dtype=F64, mutant=None):
    """sentence-transformers Pooling over (B, L, H) with a (B, L) bool mask: mean = masked sum / clamp(count, 1e-9);
    max with masked positions at -1e9; cls = token 0; lasttoken = the last position with mask 1 (zero row when none)."""
    t = tok.to(dtype)
    B, L, H = t.shape
    if mode == "mean":
        s = torch.zeros(B, H, dtype=dtype)
        for l in range(L):  # one position at a time: the fp32 model adds in the kernel's order
            s = s + t[:, l] * mask[:, l, None].to(dtype)
        n = torch.full((B, 1), float(L), dtype=dtype) if mutant == "mean_divides_by_L" else mask.sum(1, keepdim=True).to(dtype)
        return s / n.clamp(min=1e-9)
    if mode == "max":
        return t.masked_fill(~mask[..., None], -1e9).max(1).values
    if mode == "cls":
        return t[:, 0].clone()
    out = torch.zeros(B, H, dtype=dtype)
    for b in range(B):
        nz = mask[b].nonzero()
        if mutant == "lasttoken_takes_last_row":
            out[b] = t[b, L - 1]
        elif nz.numel():
            out[b] = t[b, int(nz[-1])]
    return out


def ref_pool_rows(tok, lengths, mode, dtype=F64, normalize=False, eps=L2_EPS):
    """The packed form: sequence b = the next lengths[b] rows of tok (rows, H); an empty sequence gives a zero row."""
    H = tok.shape[1]
    out = torch.zeros(len(lengths), H, dtype=dtype)
    o = 0
    for b, n in enumerate(lengths):
        if n:
            seq = tok[o:o + n][None]
            out[b] = ref_pool(seq, torch.ones(1, n, dtype=torch.bool), mode, dtype)[0]
        o += n
    return ref_l2_fwd(out, eps, dtype)[0] if normalize else out


def ref_l2_fwd(x, eps=L2_EPS, dtype=F64):
    x = x.to(dtype)
    inv = 1.0 / x.norm(dim=-1).clamp(min=eps)
    return x * inv[:, None], inv


def ref_l2_bwd(dy, x, eps=L2_EPS, dtype=F64):
    """d/dx of x / max(|x|, eps): inv (dy - y (y . dy)); with the norm clamped the map is linear, dx = dy / eps."""
    y, inv = ref_l2_fwd(x, eps, dtype)
    dy = dy.to(dtype)
    clamped = x.to(dtype).norm(dim=-1) < eps
    dot = torch.where(clamped, torch.zeros_like(inv), (y * dy).sum(-1))
    return inv[:, None] * (dy - y * dot[:, None])


def model_l2(x, dy, eps=L2_EPS):
    s = _lane_sum(x * x)
    inv = 1.0 / s.sqrt().clamp(min=eps)
    y = x * inv[:, None]
    dot = torch.where(inv * eps >= 1, torch.zeros_like(inv), _lane_sum(y * dy))
    return y, inv[:, None] * (dy - y * dot[:, None])


@functools.lru_cache(maxsize=64)
def pool_case(H: int, B: int):
    tok = _randn(B, POOL_L, H, seed=31)
    mask = pool_masks(B)
    lengths = [int(n) for n in mask.sum(1)]
    packed = torch.cat([tok[b, :n] for b, n in enumerate(lengths)])  # the packed form holds prefixes: lengths, no holes
    return types.SimpleNamespace(H=H, B=B, L=POOL_L, tok=tok, mask=mask, lengths=lengths, packed=packed)


@functools.lru_cache(maxsize=64)
def l2_case(H: int, B: int):
    """B + 3 rows: N(0,1) rows, then a zero row, a row of norm 1e-10 and a row of norm 1e-13 (below eps = 1e-12)."""
    x = _randn(B + 3, H, seed=32)
    x[B] = 0
    x[B + 1] = (x[B + 1].double() / x[B + 1].double().norm() * 1e-10).float()
    x[B + 2] = (x[B + 2].double() / x[B + 2].double().norm() * 1e-13).float()
    dy = _randn(B + 3, H, seed=33)
    y, inv = ref_l2_fwd(x)
    return types.SimpleNamespace(H=H, B=B, x=x, dy=dy, ref=dict(y=y, inv=inv, dx=ref_l2_bwd(dy, x), sq=(x.double() ** 2).sum(-1),
                                                                rnorm=1.0 / x.double().norm(dim=-1).clamp(min=1e-8)))


def check_pool(tag, mode, got, want):
    """max / cls / lasttoken select an input value: exact. mean: against fp64."""
    if mode == "mean":
        return assert_close(f"{tag} {mode}", got, want, "fp32")
    assert torch.equal(got.cpu(), want.float()), f"{tag} {mode}: not the selected input values"
    return 0.0


def check_l2(case, y, dx):
    """y by value. dx with every row weighted by max(|x|, eps) (its Jacobian is 1 / that: unweighted, the clamped rows'
    1e12 dy would be the whole norm and every other row would vanish in it), as one rel-L2 over all rows."""
    tag = f"l2 H={case.H} B={case.B}"
    w = (1.0 / case.ref["inv"])[:, None]
    return dict(y=assert_close(f"{tag} y", y, case.ref["y"], "fp32"),
                dx=assert_close(f"{tag} dx", dx.detach().double().cpu() * w, case.ref["dx"] * w, "fp32", "grad"))


# ------------------------------------------------------------------------------------------------ scale / column sums
SCALE_SIZES = (1, 3, 4, 5, 1023, 262147)  # tail only; tail only; body only; body + 1; 255 float4 + 3; 1 025 blocks + 3
SCALE_FACTORS = (1.0, 0.0, -2.5)


def scale_case(n: int):
    """N(0,1) with a NaN planted in the middle (from n = 3 on: a single element stays a number, to show it is scaled)."""
    x = _randn(n, seed=41)
    if n >= 3:
        x[n // 2] = float("nan")
    return x


def model_scale(x, f, mutant=None):
    """x * f in fp32 (one IEEE multiply per element: exact to compare). mutant 'scale_skips_tail': elements past the last
    whole group of four keep their value."""
    y = x * torch.tensor(f, dtype=F32)
    if mutant == "scale_skips_tail":
        n4 = 4 * (x.numel() // 4)
        y[n4:] = x[n4:]
    return y


def check_scale(x, f, got):
    """Against the CPU's fp32 product, bit for bit where it is a number and NaN where it is NaN; f = 1: untouched bits."""
    if f == 1.0:
        assert torch.equal(got.cpu().view(torch.int32), x.view(torch.int32)), f"scale n={x.numel()} f=1: buffer touched"
        return
    want = x * torch.tensor(f, dtype=F32)
    got = got.cpu()
    assert torch.equal(got.isnan(), want.isnan()), f"scale n={x.numel()} f={f}: NaN pattern differs"
    ok = ~want.isnan()
    assert torch.equal(got[ok].view(torch.int32), want[ok].view(torch.int32)), f"scale n={x.numel()} f={f}: product differs"


COLSUM_M = (1, 3, 255, 256, 257, 1000, 33000)  # 33 000 > 128 * 256: the column sums' block cap, 260 rows per block, last partial
COLSUM_N = (1, 64, 96, 100)
COLSUM_BIG_N = 96


def colsum_shapes():
    return [(M, N) for M in COLSUM_M for N in COLSUM_N if M < 33000 or N == COLSUM_BIG_N]


@functools.lru_cache(maxsize=32)
def colsum_case(M: int, N: int):
    a = _randn(M, N, seed=51)
    return types.SimpleNamespace(M=M, N=N, a=a, ref=a.double().sum(0))


def model_colsum(a, mutant=None):
    blocks, rp = colsum_plan(a.shape[0])
    part = _fast_rowsum(a, rp, mutant)
    assert part.shape[0] == blocks
    return model_rowsum(part, mutant=mutant)[0]


def check_colsum(case, got):
    return assert_close(f"colsum M={case.M} N={case.N}", got, case.ref, "fp32")
