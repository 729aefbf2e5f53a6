"""CPU-side test (no GPU) of the GEMM family's plan (csrc/gemm_plan.inc: GemmPlan / gemm_plan / gemm_switches, read through the
internal entry points xf_gemm_plan and xf_gemm_switches): which kernel a call of the linear forward / dX / dW entries, of the
LayerNorm-fused GEMMs and of the fused FFN kernels launches, with which tile, slice depth, slabs, tile counts, grid and LDS, is
ONE function of the call's key and of eleven environment switches. The rules are written here a second time, in Python, from
the launchers of the commit before the plan existed (d94dca2: launch_gemm, launch_gemm_bk, dispatch_gemm, xf_plan_row_tiles,
dw_split_plan, dw_split_bound, dw_ring.hip's xf_dw_ring_takes / dw_ring_plan, xf_linear_bwd_dw_group's groupable test and the
entry points' own checks), and a decision table is walked through the library on both sides of every boundary, in a fresh
process per environment. The slab room (xfmr_linear_bwd_dw_workspace) is pinned to that commit's values.
tests/test_gpu_gemm_forms.py ties each family and tile of this table to a run on the device."""

import itertools
import json
import os
import pathlib
import re

import pytest

from abi_worker import run_worker

ROOT = pathlib.Path(__file__).resolve().parents[1]
F32, BF16 = 0, 1
OK, EINVAL, EUNSUPPORTED = 0, -1, -2
A, B, C_, P, AUX = 1, 2, 4, 8, 0x100  # XF_S16_* storage bits, XF_AUX_GELU_GRAD
AB, ABC, ABCP = A | B, A | B | C_, A | B | C_ | P
# enum GemmOp / GemmFamily (csrc/internal.h), in the enums' order
(FWD_BIAS, FWD_GELU, FWD_DROP_RES, LN_FWD, LN_FWD_RE, LN_FWD_RE_DROP, DX, DX_GELU, DX_LNBWD, DW, DW_DEFERRED, DW_GROUP, FFN_FWD,
 FFN_FWD_RE, FFN_BWD) = range(15)
NONE, TILE, GROUP, RING, FFN_FWD_KERNEL, FFN_BWD_KERNEL = range(6)
# the epilogue ids of gemm.hip
(EPI_STORE, EPI_GELU, EPI_DROP_RES, EPI_GELU_GRAD, EPI_SPLITK, EPI_DROP_RES_LN, EPI_DX_LNBWD, EPI_DROP_RES_LN_RE,
 EPI_DROP_RES_LN_RED) = range(9)
FIELDS = ("family", "epi", "precision", "s16", "bm", "bn", "bk", "splits", "k_chunk", "nt_n", "nt_m", "nt_z", "nt_full",
          "short_rows", "grid", "block", "lds", "ffn_chunk", "ffn_ring", "records")
SWITCHES = ("tile_bm", "tile_bn", "tile_bk", "tile_set", "dw_bm", "dw_bn", "dw_tile_set", "pad_lds", "dw_maxsplit",
            "row_tiles_short", "skip_dw", "dw_ring", "dwr_tokens", "dwr_minwg", "ffn_chunk", "ffn_reg_stage")
ENV_NAMES = ("XFMR_GEMM_TILE", "XFMR_DW_TILE", "XFMR_GEMM_PAD_LDS", "XFMR_DW_MAXSPLIT", "XFMR_ROW_TILES_SHORT", "XFMR_FFN_CHUNK",
             "XFMR_FFN_REG_STAGE", "XFMR_EXP_SKIP_DW", "XFMR_DW_RING", "XFMR_DWR_TOKENS", "XFMR_DWR_MINWG")
REFUSED = dict.fromkeys(FIELDS, 0)
GRID_MAX = 0x7FFFFFFF
RING_TILE, RING_STAGE_TOKENS, RING_LDS = 128, 64, 2 * 4 * 64 * 128 * 2
# the storage masks each (transposes, epilogue) combination is instantiated for besides 0 (dispatch_gemm's S16 lists)
MASKS = {FWD_BIAS: (C_, C_ | B, ABC), FWD_GELU: (C_, C_ | B, ABC), FWD_DROP_RES: (A, AB), LN_FWD: (A, AB), DX: (A, A | C_, AB, ABC),
         DX_GELU: (A | C_ | P, ABCP), DX_LNBWD: (A, AB), DW: (A, AB), DW_DEFERRED: (A, AB), DW_GROUP: (A, AB)}
# the five weight shapes (N, K) of the BASELINE encoder (H = 128, I = 512: QKV, out-projection, FFN1, FFN2; H = 256: QKV)
WEIGHTS = ((384, 128), (128, 128), (512, 128), (128, 512), (768, 256))
BENCH_TOKENS = 512 * 200


# ---------------------------------------------------------------------------------------------- the switches
def atoi(s):
    m = re.match(r"\s*([+-]?\d+)", s)
    return int(m.group(1)) if m else 0


def scan_ints(s, n):
    """sscanf(s, "%d,%d,..."): the leading integers that parse, the rest 0."""
    out = [0] * n
    for i in range(n):
        m = re.match(r"\s*([+-]?\d+)", s)
        if not m:
            break
        out[i] = int(m.group(1))
        s = s[m.end():]
        if not s.startswith(","):
            break
        s = s[1:]
    return out


def switches(env):
    def on(name):  # set, not empty, not starting with '0'
        return int(bool(env.get(name)) and env[name][0] != "0")

    s = dict.fromkeys(SWITCHES, 0)
    if "XFMR_GEMM_TILE" in env:
        s["tile_set"] = 1
        s["tile_bm"], s["tile_bn"], s["tile_bk"] = scan_ints(env["XFMR_GEMM_TILE"], 3)
    if "XFMR_DW_TILE" in env:
        s["dw_tile_set"] = 1
        s["dw_bm"], s["dw_bn"] = scan_ints(env["XFMR_DW_TILE"], 2)
    s["pad_lds"] = atoi(env.get("XFMR_GEMM_PAD_LDS", "0"))
    s["dw_maxsplit"] = min(max(atoi(env.get("XFMR_DW_MAXSPLIT", "128")), 1), 256)
    s["row_tiles_short"] = on("XFMR_ROW_TILES_SHORT")
    s["skip_dw"] = int(env.get("XFMR_EXP_SKIP_DW", "")[:1] == "1")
    s["dw_ring"] = int(env.get("XFMR_DW_RING", "")[:1] != "0")
    s["dwr_tokens"] = max(atoi(env.get("XFMR_DWR_TOKENS", "3072")), 128)
    s["dwr_minwg"] = max(atoi(env.get("XFMR_DWR_MINWG", "64")), 1)
    s["ffn_chunk"] = 64 if atoi(env.get("XFMR_FFN_CHUNK", "64")) == 64 else 128
    s["ffn_reg_stage"] = on("XFMR_FFN_REG_STAGE")
    return s


# ---------------------------------------------------------------------------------------------- the rules
def case(op, M, N, K, prec=BF16, s16=0, items=1, cus=256):
    return dict(op=op, M=M, N=N, K=K, prec=prec, s16=s16, items=items, cus=cus)


def row_tiles(M, cus, short_on, BM=64):
    """xf_plan_row_tiles: (nt_m, nt_full, short_rows)."""
    plain = ((M + BM - 1) // BM, 0, 0)
    if not short_on or cus < 1:
        return plain
    per_cu = M // (BM * cus)
    rem = M - per_cu * BM * cus
    if per_cu < 1 or rem <= 0 or rem > 32 * cus:
        return plain
    each = ((rem + cus - 1) // cus + 15) // 16 * 16
    return per_cu * cus + (rem + each - 1) // each, per_cu * cus, each


def dw_split_plan(M, N, K, max_split):
    tiles = ((N + 63) // 64) * ((K + 63) // 64)
    want = max(min((1024 + tiles - 1) // tiles, max_split), 1)
    chunk = (M + want - 1) // want
    chunk = (chunk + 127) // 128 * 128
    if M >= 4096 and chunk < 256:
        chunk = 256
    chunk = max(chunk, 64)
    return (M + chunk - 1) // chunk, chunk


def dw_split_bound(M, N, K, max_split):
    """The slab room: the cap is 256 whatever XFMR_DW_MAXSPLIT says; the plan inside reads the switch."""
    tiles = ((N + 63) // 64) * ((K + 63) // 64)
    want = min((1024 + tiles - 1) // tiles, 256)
    return max(min((M + 127) // 128, want), dw_split_plan(M, N, K, max_split)[0])


def ring_takes(c, sw, items):
    return bool(sw["dw_ring"] and 1 <= items <= 4 and c["prec"] == BF16 and (c["s16"] & AB) == AB and c["M"] > 0 and c["N"] > 0
                and c["K"] > 0 and c["N"] % 128 == 0 and c["K"] % 128 == 0 and c["M"] * max(c["N"], c["K"]) * 2 < 1 << 32)


def dw_ring_plan(M, N, K, sw):
    launch_tiles = (N // 128) * (K // 128)
    generic, generic_chunk = dw_split_plan(M, N, K, sw["dw_maxsplit"])
    want = (M + sw["dwr_tokens"] - 1) // sw["dwr_tokens"]
    want = max(want, (sw["dwr_minwg"] + launch_tiles - 1) // launch_tiles)
    want = max(min(want, generic), 1)
    chunk = ((M + want - 1) // want + 127) // 128 * 128
    chunk = max(chunk, generic_chunk)
    return (M + chunk - 1) // chunk, chunk


def _plan(**kw):
    return OK, REFUSED | kw


def whole_row(c, sw, **kw):
    nt_m, nt_full, short_rows = row_tiles(c["M"], c["cus"], sw["row_tiles_short"])
    groups = (nt_m + 7) // 8
    if groups * 8 > GRID_MAX:
        return EUNSUPPORTED, REFUSED
    return _plan(nt_n=1, nt_m=nt_m, nt_z=1, nt_full=nt_full, short_rows=short_rows, grid=groups * 8, block=256, **kw)


def rules(c, sw):
    """(return code, plan fields) of the call c under the switches sw: the parent commit's entry points and launchers."""
    op, M, N, K, prec, s16 = c["op"], c["M"], c["N"], c["K"], c["prec"], c["s16"]
    if op in (FFN_FWD, FFN_FWD_RE, FFN_BWD):  # ffn_fwd_fused, xf_ffn_bwd_dx_fused_ex (N = H, K = I)
        fwd = op != FFN_BWD
        if M <= 0:
            return EINVAL, REFUSED
        if N != 128 or K <= 0 or K % (128 if fwd else 64) or (fwd and K > 1024):
            return EUNSUPPORTED, REFUSED
        if fwd:
            rc, p = whole_row(c, sw, family=FFN_FWD_KERNEL, epi=EPI_DROP_RES_LN_RE if op == FFN_FWD_RE else EPI_DROP_RES_LN,
                              precision=BF16, bm=64, bn=128, ffn_chunk=sw["ffn_chunk"])
        else:
            rc, p = whole_row(c, sw, family=FFN_BWD_KERNEL, epi=EPI_DX_LNBWD, precision=BF16, bm=64, bn=128,
                              ffn_ring=int(not sw["ffn_reg_stage"]))
            if rc == OK:
                p["records"] = p["nt_m"]
        return rc, p

    # ---- the entry's checks; the GEMM in the kernel's terms: gm x gn outputs, contraction in spans of kspan
    gm, gn, kspan, splits, k_chunk = M, N, K, 1, 0
    if op in (LN_FWD, LN_FWD_RE, LN_FWD_RE_DROP):  # linear_ln_fwd
        if M <= 0 or K <= 0:
            return EINVAL, REFUSED
        if N != 128 or K & 7 or prec != BF16:
            return EUNSUPPORTED, REFUSED
        epi, mask = {LN_FWD: EPI_DROP_RES_LN, LN_FWD_RE: EPI_DROP_RES_LN_RE, LN_FWD_RE_DROP: EPI_DROP_RES_LN_RED}[op], s16 & AB
        if op != LN_FWD and mask != AB:
            return EUNSUPPORTED, REFUSED
    elif op == DX_LNBWD:  # xf_linear_bwd_dx_lnbwd_ex
        if M <= 0 or N <= 0:
            return EINVAL, REFUSED
        if K != 128 or N & 7 or prec != BF16:
            return EUNSUPPORTED, REFUSED
        epi, mask, gn, kspan = EPI_DX_LNBWD, s16 & AB, K, N
    elif 0 <= op < FFN_FWD:  # xf_linear_fwd_ex, xf_linear_bwd_dx_ex, xf_linear_bwd_dw_ex / _deferred / _group
        if op == DW_GROUP and not 1 <= c["items"] <= 4:
            return EINVAL, REFUSED
        if M <= 0 or N <= 0 or K <= 0:
            return EINVAL, REFUSED
        if K & 3 or N & 3:
            return EUNSUPPORTED, REFUSED
        if s16 & ~AUX and prec != BF16:
            return EINVAL, REFUSED
        if s16 & ABCP and (K & 7 or N & 7):
            return EUNSUPPORTED, REFUSED
        if op in (DW, DW_DEFERRED, DW_GROUP):
            epi, mask, gm, gn = EPI_SPLITK, s16 & AB, N, K
        elif op in (DX, DX_GELU):
            epi, mask, gn, kspan = (EPI_STORE if op == DX else EPI_GELU_GRAD), s16 & ABCP, K, N
        else:
            epi, mask = {FWD_BIAS: EPI_STORE, FWD_GELU: EPI_GELU, FWD_DROP_RES: EPI_DROP_RES}[op], s16 & ABC
    else:
        return EINVAL, REFUSED

    dw = epi == EPI_SPLITK
    if dw:
        # xf_linear_bwd_dw_deferred asks the ring unless XFMR_EXP_SKIP_DW; xf_linear_bwd_dw_group asks it for all its items
        asks_ring = (op == DW_DEFERRED and not sw["skip_dw"]) or op == DW_GROUP
        if asks_ring and ring_takes(c, sw, c["items"] if op == DW_GROUP else 1):
            splits, k_chunk = dw_ring_plan(M, N, K, sw)  # xf_dw_ring_launch
            grid = (splits + 7) // 8 * 8 * (N // 128) * (K // 128)
            if grid > GRID_MAX:
                return EUNSUPPORTED, REFUSED
            return _plan(family=RING, epi=EPI_SPLITK, precision=BF16, s16=AB, bm=RING_TILE, bn=RING_TILE, bk=RING_STAGE_TOKENS,
                         splits=splits, k_chunk=k_chunk, nt_n=K // 128, nt_m=N // 128, nt_z=splits, grid=grid, block=512,
                         lds=RING_LDS)
        splits, k_chunk = dw_split_plan(M, N, K, sw["dw_maxsplit"])
        kspan = k_chunk
        if op == DW_DEFERRED and sw["skip_dw"]:  # XFMR_EXP_SKIP_DW: the slab count is written, nothing is dispatched
            return _plan(family=NONE, epi=epi, precision=prec, s16=mask, splits=splits, k_chunk=k_chunk)

    # ---- launch_gemm_bk's tile, launch_gemm's slice depth, dispatch_gemm's instantiation list
    rows = epi in (EPI_DROP_RES_LN, EPI_DROP_RES_LN_RE, EPI_DROP_RES_LN_RED, EPI_DX_LNBWD)
    bm, bn = 64, (128 if gn >= 256 and epi != EPI_GELU_GRAD else 64)
    if rows:
        bn = 128
    if dw and gm > 64 and gn > 64:
        bm, bn = 128, 64
        if sw["dw_bm"]:
            bm, bn = sw["dw_bm"], sw["dw_bn"]
    if sw["tile_bm"] and not rows:
        bm, bn = sw["tile_bm"], sw["tile_bn"]
    assert bm >= 1 and bn >= 1  # (the parent divided by zero on a malformed override: no such case in the tables)
    bk = 32
    if prec == BF16 and sw["tile_bk"] != 32:
        if dw and kspan % 128 == 0:
            bk = 128
        elif not dw and kspan % 64 == 0:
            bk = 64
    if prec == F32:
        if mask:
            return EINVAL, REFUSED
    elif prec != BF16:
        return EINVAL, REFUSED
    elif op not in (LN_FWD_RE, LN_FWD_RE_DROP) and mask and mask not in MASKS[op]:
        return EINVAL, REFUSED

    # xf_linear_bwd_dw_group's grouped launch: gemm_group_kernel<PrecBF16, 128, 64, 128, ...>
    group = (op == DW_GROUP and c["items"] > 1 and prec == BF16 and mask == AB and not sw["tile_set"] and not sw["dw_tile_set"]
             and N > 64 and K > 64 and not (N | K) & 7)
    common = dict(epi=epi, precision=prec, s16=mask, bm=bm, bn=bn, bk=bk, splits=splits if dw else 0, k_chunk=k_chunk)
    if group:
        assert (bm, bn, bk) == (128, 64, 128)
    common |= dict(family=GROUP if group else TILE, lds=0 if group else sw["pad_lds"])
    if rows:
        rc, p = whole_row(c, sw, **common)
        if rc == OK and epi == EPI_DX_LNBWD:
            p["records"] = p["nt_m"]
        return rc, p
    nt_n, nt_m = (gn + bn - 1) // bn, (gm + bm - 1) // bm
    groups = (splits + 7) // 8 if splits > 1 else (nt_m + 7) // 8
    per = nt_n * nt_m if splits > 1 else nt_n
    if groups * per * 8 > GRID_MAX:
        return EUNSUPPORTED, REFUSED
    return _plan(nt_n=nt_n, nt_m=nt_m, nt_z=splits, grid=groups * per * 8, block=256, **common)


# ---------------------------------------------------------------------------------------------- the library
WORKER = r"""
I32 = C.c_int32
sw = (I32 * 16)()
lib.xf_gemm_switches(sw)
res = []
for c in json.load(sys.stdin):
    out = (I32 * 24)()
    rc = lib.xf_gemm_plan(c["op"], c["M"], c["N"], c["K"], c["prec"], c["s16"], c["items"], c["cus"], sw, out)
    res.append([rc, list(out)])
report(list(sw), res)
"""


@pytest.fixture(scope="module")
def native():
    from xfmr_rec_amd import _native as N

    if not N.LIB_PATH.exists():
        pytest.fail(f"{N.LIB_PATH} missing: run build() first")
    return N


def run_script(native, script, env, stdin=""):
    clean = {k: v for k, v in os.environ.items() if k not in ENV_NAMES}
    torch_imported, values = run_worker(script, native.LIB_PATH, clean | env, stdin)
    assert torch_imported is False
    return values


def run_table(native, table, env):
    """(switches as the library read them, [(rc, plan fields, the rest of out)]) from a fresh process whose environment has
    exactly the switches of env."""
    sw, res = run_script(native, WORKER, env, json.dumps(table))
    return dict(zip(SWITCHES, sw)), [(rc, dict(zip(FIELDS, out)), out[len(FIELDS):]) for rc, out in res]


def check_table(native, table, env):
    sw, got = run_table(native, table, env)
    assert sw == switches(env), (env, sw)
    assert len(got) == len(table)
    plans = []
    for c, (rc, plan, rest) in zip(table, got):
        want_rc, want = rules(c, sw)
        assert rc == want_rc, (c, env, rc, want_rc)
        assert plan == want, (c, env, {k: (plan[k], want[k]) for k in FIELDS if plan[k] != want[k]})
        assert rest == [0] * (24 - len(FIELDS))
        plans.append((rc, plan))
    return plans


# ---------------------------------------------------------------------------------------------- the tables
def tile_table():
    t = []
    # N 252 / 256 (bn 64 -> 128; gelu' stays at 64), K % 64 and % 128 for the slice depth, fp32 (always 32-deep), partial tiles
    for op, (M, N, K), prec in itertools.product((FWD_BIAS, FWD_GELU, FWD_DROP_RES, DX, DX_GELU),
                                                 ((70, 72, 64), (70, 252, 96), (70, 256, 128), (129, 264, 36), (64, 128, 512),
                                                  (1, 4, 4), (102400, 512, 128), (102400, 128, 512), (300, 256, 252)),
                                                 (BF16, F32)):
        t.append(case(op, M, N, K, prec))
    # every storage mask, instantiated or not, with features that are and are not multiples of 8; the gelu' flag rides along
    for op, mask, (N, K), prec in itertools.product((FWD_BIAS, FWD_GELU, FWD_DROP_RES, DX, DX_GELU, DW, DW_DEFERRED),
                                                    list(range(16)) + [AUX, AUX | ABC, AUX | ABCP],
                                                    ((72, 64), (68, 36)), (BF16, F32)):
        t.append(case(op, 70, N, K, prec, mask))
    # the whole-row epilogues: N != 128 / K != 128, K & 7, fp32, masks; several M for the row map
    for op, (N, K), prec, mask in itertools.product((LN_FWD, LN_FWD_RE, LN_FWD_RE_DROP), ((128, 128), (128, 512), (128, 96), (128, 36),
                                                                                         (64, 128), (256, 128), (128, 0)),
                                                    (BF16, F32), (0, A, B, AB, ABC)):
        t.append(case(op, 70, N, K, prec, mask))
    for (N, K), prec, mask in itertools.product(((384, 128), (128, 128), (96, 128), (36, 128), (384, 64), (384, 256), (0, 128)),
                                                (BF16, F32), (0, A, B, AB, ABC)):
        t.append(case(DX_LNBWD, 70, N, K, prec, mask))
    # split-K: M > 64 && N > 64 in the GEMM's terms (N and K of the Linear) on both sides: 128 x 64 against the forward rule
    for op, (N, K), M in itertools.product((DW, DW_DEFERRED), ((64, 64), (64, 68), (68, 64), (68, 68), (192, 136), (64, 256), (256, 64),
                                                               (384, 128), (128, 512)), (63, 200, 300, 6400)):
        t.append(case(op, M, N, K, BF16, AB))
        t.append(case(op, M, N, K, F32))
    # nothing positive, not a multiple of 4, an unknown operation or precision, the grid's 31 bits
    for op in (FWD_BIAS, DX, DW, DW_DEFERRED, DW_GROUP):
        t += [case(op, 0, 64, 64), case(op, 70, 0, 64), case(op, 70, 64, -4), case(op, 70, 66, 64), case(op, 70, 64, 66),
              case(op, 70, 64, 64, prec=2), case(op, 70, 64, 64, prec=2, s16=A)]
    t += [case(15, 70, 64, 64), case(-1, 70, 64, 64)]
    # (two N-tiles: 2^27 groups of eight M-tiles are one workgroup too many. The whole-row kernels' one N-tile leaves their
    # check to row counts whose tile count does not fit an int either)
    t += [case(FWD_BIAS, 64 * (2**30 - 8), 128, 64), case(FWD_BIAS, 64 * (2**30 - 8) + 1, 128, 64),
          case(LN_FWD, 64 * (2**31 - 8), 128, 128, s16=AB)]
    return t


def slab_table():
    t = []
    tokens = (63, 64, 2750, 4095, 4096, 6400, 102400)
    for (N, K), M, op in itertools.product(WEIGHTS, tokens, (DW, DW_DEFERRED)):
        t.append(case(op, M, N, K, BF16, AB))
    for (N, K), M, n in itertools.product(WEIGHTS + ((192, 136), (64, 64), (64, 128), (128, 64), (136, 128)), tokens, (1, 2, 4)):
        t.append(case(DW_GROUP, M, N, K, BF16, AB, items=n))
    # the ring takes: N or K not a multiple of 128; M x widest x 2 on both sides of 2^32; fp32; a missing storage bit; items
    for N, K in ((128, 128), (384, 128), (128, 192), (192, 128), (1024, 128)):
        for M in (64, 3072, 3073, 2**32 // (2 * max(N, K)) - 1, 2**32 // (2 * max(N, K))):
            t += [case(DW_DEFERRED, M, N, K, BF16, AB), case(DW_GROUP, M, N, K, BF16, AB, items=4)]
        t += [case(DW_DEFERRED, 300, N, K, F32), case(DW_DEFERRED, 300, N, K, BF16, A), case(DW_DEFERRED, 300, N, K, BF16, 0),
              case(DW_GROUP, 300, N, K, BF16, AB, items=0), case(DW_GROUP, 300, N, K, BF16, AB, items=5),
              case(DW_GROUP, 300, N, K, F32, 0, items=2), case(DW_GROUP, 300, N, K, BF16, A, items=2)]
    return t


def row_table():
    t = []
    for M, cus in itertools.product((102400, 25600, 300, 70, 64 * 256 * 3, 64 * 256 * 2 + 1, 64 * 256 + 32 * 256, 64 * 256 + 32 * 256 + 1),
                                    (256, 304, 0)):
        t += [case(LN_FWD, M, 128, 128, s16=AB, cus=cus), case(LN_FWD_RE, M, 128, 512, s16=AB, cus=cus),
              case(DX_LNBWD, M, 384, 128, s16=AB, cus=cus), case(FFN_FWD, M, 128, 512, cus=cus), case(FFN_BWD, M, 128, 512, cus=cus)]
    return t


def ffn_table():
    t = []
    for op, I, M, H in itertools.product((FFN_FWD, FFN_FWD_RE, FFN_BWD), (0, 64, 128, 192, 256, 320, 1024, 1088, 1152), (0, 70, 102400),
                                         (128, 64, 256)):
        t.append(case(op, M, H, I))
    for op in (FFN_FWD, FFN_BWD):
        t.append(case(op, 64 * (2**31 - 8), 128, 128))
    return t


ENVS = [{}, {"XFMR_GEMM_TILE": "128,128,128"}, {"XFMR_GEMM_TILE": "64,128,32"}, {"XFMR_GEMM_TILE": "128,64"}, {"XFMR_GEMM_TILE": ""},
        {"XFMR_DW_TILE": "64,64"}, {"XFMR_DW_TILE": "128,128", "XFMR_GEMM_PAD_LDS": "65536"}, {"XFMR_GEMM_PAD_LDS": "32768"},
        {"XFMR_EXP_SKIP_DW": "1"}, {"XFMR_DW_RING": "0"}]


@pytest.mark.parametrize("env", ENVS, ids=lambda e: "-".join(f"{k}={v}" for k, v in e.items()) or "default")
def test_tile_kernel_plan_follows_the_rules(native, env):
    plans = check_table(native, tile_table() + slab_table(), env)
    ok = [p for rc, p in plans if rc == OK]
    if not env:
        assert {(p["bm"], p["bn"], p["bk"]) for p in ok if p["family"] == TILE} >= {(64, 64, 64), (64, 128, 64), (64, 64, 32),
                                                                                   (64, 128, 32), (128, 64, 128)}
        assert {p["family"] for p in ok} == {TILE, GROUP, RING}
        assert {rc for rc, _ in plans} == {OK, EINVAL, EUNSUPPORTED}
    if env.get("XFMR_GEMM_TILE", "").startswith("128,128"):
        assert {(p["bm"], p["bn"]) for p in ok if p["family"] == TILE and p["epi"] < EPI_DROP_RES_LN} == {(128, 128)}
        assert GROUP not in {p["family"] for p in ok}
    if env.get("XFMR_GEMM_TILE") == "64,128,32":
        assert {p["bk"] for p in ok if p["family"] == TILE} == {32}
    if env.get("XFMR_GEMM_TILE") == "":  # set, nothing parsed: the tiles stay, the grouped launch goes
        assert GROUP not in {p["family"] for p in ok} and (128, 64, 128) in {(p["bm"], p["bn"], p["bk"]) for p in ok}
    if "XFMR_DW_TILE" in env:
        want = tuple(int(v) for v in env["XFMR_DW_TILE"].split(","))
        assert want in {(p["bm"], p["bn"]) for p in ok if p["epi"] == EPI_SPLITK and p["family"] == TILE}
        assert GROUP not in {p["family"] for p in ok}
    if "XFMR_GEMM_PAD_LDS" in env:
        assert {p["lds"] for p in ok if p["family"] == TILE} == {int(env["XFMR_GEMM_PAD_LDS"])}
    if "XFMR_EXP_SKIP_DW" in env:
        assert {p["family"] for p in ok} == {NONE, TILE, GROUP, RING}
    if env.get("XFMR_DW_RING") == "0":
        assert RING not in {p["family"] for p in ok}


@pytest.mark.parametrize("env", [{}, {"XFMR_DW_MAXSPLIT": "1"}, {"XFMR_DW_MAXSPLIT": "64"}, {"XFMR_DW_MAXSPLIT": "300"},
                                 {"XFMR_DWR_TOKENS": "1024"}, {"XFMR_DWR_TOKENS": "100"}, {"XFMR_DWR_MINWG": "1"},
                                 {"XFMR_DWR_MINWG": "256", "XFMR_DWR_TOKENS": "4096"}, {"XFMR_DW_RING": "0", "XFMR_DW_MAXSPLIT": "64"}],
                         ids=lambda e: "-".join(f"{k}={v}" for k, v in e.items()) or "default")
def test_slab_plan_follows_the_rules(native, env):
    table = slab_table()
    plans = check_table(native, table, env)
    sw = switches(env)
    for c, (rc, p) in zip(table, plans):
        if rc == OK:
            generic = dw_split_plan(c["M"], c["N"], c["K"], sw["dw_maxsplit"])[0]
            assert 1 <= p["splits"] <= generic <= sw["dw_maxsplit"], (c, p)  # never more slabs than the generic plan
            assert (p["splits"] - 1) * p["k_chunk"] < c["M"] <= p["splits"] * p["k_chunk"]
    if not env:
        assert {p["family"] for rc, p in plans if rc == OK} == {TILE, GROUP, RING}


@pytest.mark.parametrize("env", [{}, {"XFMR_ROW_TILES_SHORT": "1"}, {"XFMR_ROW_TILES_SHORT": "0"}],
                         ids=lambda e: "-".join(f"{k}={v}" for k, v in e.items()) or "default")
def test_row_map_follows_the_rules(native, env):
    table = row_table()
    plans = check_table(native, table, env)
    short = {c["M"]: p for c, (rc, p) in zip(table, plans) if c["op"] == FFN_BWD and c["cus"] == 256}
    if env.get("XFMR_ROW_TILES_SHORT") == "1":  # the Ms of test_host_logic.py's row-tile test, and its values
        assert [short[m]["records"] for m in (102400, 25600, 300, 64 * 256 * 3, 64 * 256 * 2 + 1)] == [6 * 256 + 256, 400, 5, 768, 513]
        assert (short[102400]["nt_full"], short[102400]["short_rows"]) == (6 * 256, 16)
    else:
        assert [short[m]["records"] for m in (102400, 25600, 300, 64 * 256 * 3, 64 * 256 * 2 + 1)] == [1600, 400, 5, 768, 513]
        assert all(p["nt_full"] == 0 and p["short_rows"] == 0 for _, p in plans)


@pytest.mark.parametrize("env", [{}, {"XFMR_FFN_CHUNK": "128"}, {"XFMR_FFN_CHUNK": "64"}, {"XFMR_FFN_CHUNK": "96"},
                                 {"XFMR_FFN_REG_STAGE": "1"}, {"XFMR_FFN_REG_STAGE": "0"}, {"XFMR_ROW_TILES_SHORT": "1"}],
                         ids=lambda e: "-".join(f"{k}={v}" for k, v in e.items()) or "default")
def test_fused_ffn_plan_follows_the_rules(native, env):
    table = ffn_table()
    plans = check_table(native, table, env)
    ok = [p for rc, p in plans if rc == OK]
    assert {p["ffn_chunk"] for p in ok if p["family"] == FFN_FWD_KERNEL} == {64 if env.get("XFMR_FFN_CHUNK", "64") == "64" else 128}
    assert {p["ffn_ring"] for p in ok if p["family"] == FFN_BWD_KERNEL} == {0 if env.get("XFMR_FFN_REG_STAGE") == "1" else 1}
    assert len({p["grid"] for p in ok}) >= 3 and {rc for rc, _ in plans} == {OK, EINVAL, EUNSUPPORTED}


ROOM_WORKER = r"""
I32 = C.c_int32
req = json.load(sys.stdin)
sw, off = (I32 * 16)(), (I32 * 16)()
lib.xf_gemm_switches(sw)
lib.xf_gemm_switches(off)
off[11] = 0  # dw_ring: the generic plan of the same key
out, kc = (I32 * 24)(), C.c_int()
T = req["tokens"]
worst = []
for n, k in req["weights"]:
    room = lib.xfmr_linear_bwd_dw_workspace(T, n, k) // (4 * n * k)
    most = [0, 0, 0]
    for t in range(1, T + 1):
        for i, s in enumerate((sw, off)):
            assert lib.xf_gemm_plan(10, t, n, k, 1, 3, 1, 0, s, out) == 0  # kGemmDwDeferred, bf16, A | B
            assert out[0] == (3 if i == 0 else 1), (t, n, k, list(out))  # ring | tile
            most[i] = max(most[i], out[7])
        assert lib.xf_dw_split_plan(t, n, k, C.byref(kc)) == out[7] and kc.value == out[8]
    worst.append([room] + most[:2])
records = max(lib.xf_ln_row_tiles(t) for t in range(1, T + 1))
sizes = [lib.xfmr_linear_bwd_dw_workspace(*c) for c in req["pinned"]]
report(worst, records, lib.xf_ln_row_tiles(T), sizes)
"""

# xfmr_linear_bwd_dw_workspace(M, N, K) of the parent commit's library (d94dca2), default environment
WORKSPACE_BYTES = [((63, 128, 128), 65536), ((64, 384, 128), 196608), ((300, 192, 136), 313344), ((200, 64, 64), 32768),
                   ((2750, 512, 128), 5767168), ((4095, 128, 128), 2097152), ((4096, 128, 128), 2097152),
                   ((6400, 384, 128), 9830400), ((6400, 128, 512), 13107200), ((25600, 512, 128), 16777216),
                   ((102400, 128, 128), 16777216), ((102400, 384, 128), 16908288), ((102400, 512, 128), 16777216),
                   ((102400, 128, 512), 16777216), ((40000, 768, 256), 17301504), ((40000, 256, 1024), 16777216), ((1, 4, 4), 64)]


@pytest.mark.parametrize("env", [{}, {"XFMR_DW_MAXSPLIT": "64"}, {"XFMR_DW_MAXSPLIT": "256"}, {"XFMR_ROW_TILES_SHORT": "1"}],
                         ids=lambda e: "-".join(f"{k}={v}" for k, v in e.items()) or "default")
def test_room_holds_every_token_count(native, env):
    """The slab buffers and the LayerNorm records are carved for batch x seq_len tokens and then run with the real row count
    (packed rows): for EVERY token count up to the benchmark's, on the ring's plan and on the generic one, the slabs planned
    fit the room, and the records of the row map fit those carved. The room itself is the parent commit's, switch or not."""
    req = dict(tokens=BENCH_TOKENS, weights=WEIGHTS, pinned=[c for c, _ in WORKSPACE_BYTES])
    worst, records, carved, sizes = run_script(native, ROOM_WORKER, env, json.dumps(req))
    for (n, k), (room, ring, generic) in zip(WEIGHTS, worst):
        assert 1 <= ring <= generic <= room, (n, k, room, ring, generic)
        assert room == dw_split_bound(BENCH_TOKENS, n, k, switches(env)["dw_maxsplit"])
    assert records <= carved
    assert sizes == [want for _, want in WORKSPACE_BYTES]


SWITCH_WORKER = r"""
sw = (C.c_int32 * 16)()
lib.xf_gemm_switches(sw)
first = list(sw)
os.environ.update(json.load(sys.stdin))
lib.xf_gemm_switches(sw)
report(first, list(sw))
"""


def test_switches_are_read_once_but_for_the_two_per_call_ones(native):
    later = {"XFMR_GEMM_TILE": "128,128,32", "XFMR_DW_TILE": "64,64", "XFMR_GEMM_PAD_LDS": "4096", "XFMR_DW_MAXSPLIT": "7",
             "XFMR_ROW_TILES_SHORT": "1", "XFMR_EXP_SKIP_DW": "1", "XFMR_DW_RING": "0", "XFMR_DWR_TOKENS": "512",
             "XFMR_DWR_MINWG": "8", "XFMR_FFN_CHUNK": "128", "XFMR_FFN_REG_STAGE": "1"}
    first, second = run_script(native, SWITCH_WORKER, {}, json.dumps(later))
    assert dict(zip(SWITCHES, first)) == switches({})
    assert dict(zip(SWITCHES, second)) == switches({}) | dict(ffn_chunk=128, ffn_reg_stage=1)
    # every variable as the library reads it, clamps and odd spellings included
    for env in ({"XFMR_DW_MAXSPLIT": "0"}, {"XFMR_DW_MAXSPLIT": "300"}, {"XFMR_DW_MAXSPLIT": "x"}, {"XFMR_DWR_TOKENS": "64"},
                {"XFMR_DWR_MINWG": "0"}, {"XFMR_DW_RING": "off"}, {"XFMR_DW_RING": ""}, {"XFMR_EXP_SKIP_DW": "2"},
                {"XFMR_EXP_SKIP_DW": "1"}, {"XFMR_GEMM_TILE": "64"}, {"XFMR_GEMM_TILE": "64,128,32"}, {"XFMR_DW_TILE": "64,64"},
                {"XFMR_ROW_TILES_SHORT": ""}, {"XFMR_FFN_REG_STAGE": "0"}, {"XFMR_FFN_CHUNK": "abc"}, later):
        first, _ = run_script(native, SWITCH_WORKER, env, "{}")
        assert dict(zip(SWITCHES, first)) == switches(env), env


def test_plan_is_internal(native):
    header = (ROOT / "include" / "xfmr_hip.h").read_text()
    for name in ("xf_gemm_plan", "xf_gemm_switches"):
        assert name not in header and name not in native.EXPORTED_SYMBOLS
