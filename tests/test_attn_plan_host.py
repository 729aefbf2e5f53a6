"""CPU-side test (no GPU) of attention's plan (csrc/attention.hip: AttnPlan / attn_plan_fwd / attn_plan_bwd, read through
the internal entry point xf_attn_plan): which kernels a call launches, with which grid and how much LDS, is ONE function of
the call's key and of three environment switches. The rules are written here a second time, in Python, from the launchers of
the commit before the plan existed (ea660de: launch_fwd_bf16, launch_bwd_bf16, launch_fwd_generic, launch_bwd_generic,
dispatch_fwd, dispatch_bwd), with their LDS formulas, and a decision table is walked through the library on both sides of
every boundary. The GPU tests that compare one form with another rely on the launcher having picked the form they name;
tests/test_gpu_attn_forms.py ties each form id of this table to a run on the device."""

import ctypes as C
import itertools
import os
import pathlib
import re

import pytest

import test_encoder_plan_host as EP
from abi_worker import run_worker

ROOT = pathlib.Path(__file__).resolve().parents[1]
F32, BF16 = 0, 1
OK, EINVAL, EUNSUPPORTED = 0, -1, -2
FWD_SPLIT, BWD_SPLIT, BWD_ROLES = 1, 2, 4  # the bits of xf_attn_switches
# enum AttnForm, in the enum's order
FORMS = ("kAttnNone", "kAttnGenericPanel", "kAttnGenericStream", "kAttnBf16Seq", "kAttnBf16Fused", "kAttnBf16Roles4",
         "kAttnBf16Roles8", "kAttnBf16Panel", "kAttnBf16Stream")
(NONE, GENERIC_PANEL, GENERIC_STREAM, BF16_SEQ, BF16_FUSED, BF16_ROLES4, BF16_ROLES8, BF16_PANEL, BF16_STREAM) = range(9)
FIELDS = ("form", "kernels", "grid_x", "grid_y", "block", "lds0", "lds1")
LDS_LIMIT = 160 * 1024
FUSED_MAX_L, SEQ_MAX_L = 256, 512
SCRATCH = 4 * 32 * 33 * 4  # the fp32 output-transposition scratch of the 128-row-block kernels


# ---------------------------------------------------------------------------------------------- LDS formulas
def _lp(L):
    return (L + 31) // 32 * 32


def _align(x):
    return (x + 15) & ~15


def bf16_panel_bytes(L):
    return _align(max(2 * _lp(L) * 32 * 2, SCRATCH))


def bf16_smem_fwd(L):
    return bf16_panel_bytes(L) + (_lp(L) // 32 + 2) * 4


def bf16_smem_dkv(L):
    return bf16_panel_bytes(L) + 3 * _lp(L) * 4


def bf16_smem_fwd_seq(L):
    return 2 * _lp(L) * 32 * 2 + (_lp(L) // 32 + 2) * 4


def bf16_smem_roles(L):
    return 4 * _lp(L) * 32 * 2 + 3 * _lp(L) * 4 + (_lp(L) // 32 + 2) * 4


def bf16_smem_fused(L):
    return 2 * _lp(L) * 32 * 2 + _lp(L) * 32 * 4 + 3 * _lp(L) * 4 + 4 * 32 * 32 * 2


BF16_STREAM_CH = 256
BF16_STREAM_FWD = 2 * BF16_STREAM_CH * 32 * 2 + _align((BF16_STREAM_CH // 32 + 2) * 4)  # forward and dQ
BF16_STREAM_DKV = 2 * BF16_STREAM_CH * 32 * 2 + 3 * BF16_STREAM_CH * 4


class Generic:
    """AttnSmem<P, DHT> / AttnStream<P, DHT> of one generic family: es = bytes per LDS element, ldr = padded row length."""

    def __init__(self, prec, dh):
        self.es, self.dh = (2 if prec == BF16 else 4), dh
        self.ldr = dh + (8 if prec == BF16 else 4)
        self.ch = 128 if (self.es == 2 or dh == 32) else 64

    def row(self, rows):
        return _align(rows * self.ldr * self.es)

    def t(self, rows):
        return _align(self.dh * (rows + 4) * self.es)

    def fwd_smem(self, L):
        return self.row(_lp(L)) + self.t(_lp(L)) + SCRATCH + _lp(L)

    def dq_smem(self, L):
        return 2 * self.row(_lp(L)) + self.t(_lp(L)) + SCRATCH + _lp(L)

    def dkv_smem(self, L):
        return 2 * self.row(_lp(L)) + 2 * self.t(_lp(L)) + SCRATCH + 2 * _lp(L) * 4

    def stream(self):  # fwd, dQ, dK/dV
        k_row, k_t = self.ch * self.ldr * self.es, self.dh * (self.ch + 4) * self.es
        return (max(k_row + k_t, SCRATCH) + self.ch, max(2 * k_row + k_t, SCRATCH) + self.ch,
                max(2 * k_row + 2 * k_t, SCRATCH) + 2 * self.ch * 4)


# ---------------------------------------------------------------------------------------------- the rules
def case(prec, dh, B, L, *, A=2, s16=False, causal=True, packed=False, stream_keys=False, switches=0):
    return dict(prec=prec, s16=s16, B=B, L=L, A=A, H=A * dh, causal=causal, packed=packed, stream_keys=stream_keys,
                switches=switches)


def _plan(form, n, gx, gy, block, lds0, lds1=0):
    return OK, dict(zip(FIELDS, (form, n, gx, gy, block, lds0, lds1)))


REFUSED = dict.fromkeys(FIELDS, 0)


def rules(c, bwd):
    """(return code, plan fields) of the call c: check_shape, dispatch_* and the four launchers of the parent commit."""
    B, L, A, H = c["B"], c["L"], c["A"], c["H"]
    if B <= 0 or L <= 0 or A <= 0 or H <= 0:
        return EINVAL, REFUSED
    if H != A * 32 and H != A * 64:
        return EUNSUPPORTED, REFUSED
    dh = H // A
    if c["packed"] and not (c["prec"] == BF16 and dh == 32):
        return EUNSUPPORTED, REFUSED
    if c["prec"] == BF16 and dh == 32:
        return rules_bf16_bwd(c) if bwd else rules_bf16_fwd(c)
    if c["prec"] == BF16 or (c["prec"] == F32 and not c["s16"]):
        g = Generic(c["prec"], dh)
        grid = ((L + 127) // 128, B * A)
        s = g.stream()
        if not bwd:
            sm = g.fwd_smem(L)
            if c["stream_keys"] or sm > LDS_LIMIT:
                return _plan(GENERIC_STREAM, 1, *grid, 256, s[0])
            return _plan(GENERIC_PANEL, 1, *grid, 256, sm)
        s1, s2 = g.dq_smem(L), g.dkv_smem(L)
        if c["stream_keys"] or s1 > LDS_LIMIT or s2 > LDS_LIMIT:
            return _plan(GENERIC_STREAM, 2, *grid, 256, s[1], s[2])
        return _plan(GENERIC_PANEL, 2, *grid, 256, s1, s2)
    return EINVAL, REFUSED


def rules_bf16_fwd(c):
    B, L, A = c["B"], c["L"], c["A"]
    stream = L > SEQ_MAX_L if c["packed"] else c["stream_keys"]
    two_blocks = bool(c["switches"] & FWD_SPLIT)
    if c["packed"] and not c["causal"]:
        return EUNSUPPORTED, REFUSED
    b8 = (B + 7) // 8 * 8
    if not stream and (not two_blocks or c["packed"]) and c["causal"] and L <= SEQ_MAX_L:
        return _plan(BF16_SEQ, 1, A * b8, 1, 256, bf16_smem_fwd_seq(L))
    gx = (L + 127) // 128 * A * b8
    sm = bf16_smem_fwd(L)
    if stream or sm > LDS_LIMIT:
        return _plan(BF16_STREAM, 1, gx, 1, 256, BF16_STREAM_FWD)
    return _plan(BF16_PANEL, 1, gx, 1, 256, sm)


def rules_bf16_bwd(c):
    B, L, A = c["B"], c["L"], c["A"]
    stream = L > SEQ_MAX_L if c["packed"] else c["stream_keys"]
    two_kernels = bool(c["switches"] & BWD_SPLIT)
    roles = bool(c["switches"] & BWD_ROLES)
    if c["packed"] and not c["causal"]:
        return EUNSUPPORTED, REFUSED
    b8 = (B + 7) // 8 * 8
    if not stream and (not two_kernels or c["packed"]) and (roles or L > FUSED_MAX_L) and c["causal"] and L <= SEQ_MAX_L:
        if L > FUSED_MAX_L:
            return _plan(BF16_ROLES8, 1, A * b8, 1, 1024, bf16_smem_roles(L))
        return _plan(BF16_ROLES4, 1, A * b8, 1, 512, bf16_smem_roles(L))
    sf = bf16_smem_fused(L)
    if not stream and (not two_kernels or c["packed"]) and c["causal"] and L <= FUSED_MAX_L and sf <= LDS_LIMIT:
        return _plan(BF16_FUSED, 1, A * b8, 1, 256, sf)
    gx = (L + 127) // 128 * A * b8
    s1, s2 = bf16_smem_fwd(L), bf16_smem_dkv(L)
    if stream or s1 > LDS_LIMIT or s2 > LDS_LIMIT:
        return _plan(BF16_STREAM, 2, gx, 1, 256, BF16_STREAM_FWD, BF16_STREAM_DKV)
    return _plan(BF16_PANEL, 2, gx, 1, 256, s1, s2)


def last_fit(smem):
    """The last L at which the panel whose bytes smem(L) gives fits LDS (the sizes grow with L)."""
    L = 32
    while smem(L + 1) <= LDS_LIMIT:
        L += 1
    return L


GENERIC_FAMILIES = ((F32, 32), (F32, 64), (BF16, 64))


def generic_boundaries(prec, dh):
    g = Generic(prec, dh)
    return {name: last_fit(f) for name, f in (("fwd", g.fwd_smem), ("dq", g.dq_smem), ("dkv", g.dkv_smem))}


def decision_table():
    t = []
    flags = (False, True)
    # bf16 at head size 32: L on both sides of 32 (one tile), kFusedMaxL, kSeqMaxL and the two panel limits
    for L, B, causal, packed, stream_keys, sw, s16 in itertools.product(
            (32, 33, 256, 257, 512, 513, 1152, 1153, 1248, 1249), (1, 8, 9), flags, flags, flags, range(8), flags):
        t.append(case(BF16, 32, B, L, s16=s16, causal=causal, packed=packed, stream_keys=stream_keys, switches=sw))
    # the generic families: the last L at which each panel fits, the next one, and the ends of the 32-row step around it
    for prec, dh in GENERIC_FAMILIES:
        for last in sorted(set(generic_boundaries(prec, dh).values())):
            for L, B, causal, stream_keys, sw, s16 in itertools.product(
                    (last - 32, last - 31, last, last + 1, last + 32), (1, 8, 9), flags, flags, (0, 7), flags):
                t.append(case(prec, dh, B, L, s16=s16, causal=causal, stream_keys=stream_keys, switches=sw))
        t.append(case(prec, dh, 2, 200, packed=True))
    return t


TABLE = decision_table()


# ---------------------------------------------------------------------------------------------- the library
@pytest.fixture(scope="module")
def native():
    from xfmr_rec_amd import _native as N

    if not N.LIB_PATH.exists():
        pytest.fail(f"{N.LIB_PATH} missing: run build() first")
    return N


@pytest.fixture(scope="module")
def plan(native):
    lib = native.load()

    def ask(c, bwd):
        out = (C.c_int32 * 8)(*([-1] * 8))
        rc = lib.xf_attn_plan(int(bwd), c["prec"], int(c["s16"]), c["B"], c["L"], c["A"], c["H"], int(c["causal"]),
                              int(c["packed"]), int(c["stream_keys"]), c["switches"], out)
        assert out[7] == 0
        return rc, dict(zip(FIELDS, out))

    return ask


def test_plan_follows_the_rules_and_names_every_form(plan):
    assert len(TABLE) > 4000
    seen = {False: set(), True: set()}
    for c, bwd in itertools.product(TABLE, (False, True)):
        want = rules(c, bwd)
        assert plan(c, bwd) == want, (c, bwd, want)
        seen[bwd].add(want[1]["form"])
    assert seen[False] == {NONE, GENERIC_PANEL, GENERIC_STREAM, BF16_SEQ, BF16_PANEL, BF16_STREAM}
    assert seen[True] == {NONE, GENERIC_PANEL, GENERIC_STREAM, BF16_FUSED, BF16_ROLES4, BF16_ROLES8, BF16_PANEL, BF16_STREAM}
    # every form id the library's enum has: a form added there needs a name here and a row in the table
    src = (ROOT / "transformer-recommenders_amd" / "csrc" / "attention.hip").read_text()
    body = re.search(r"enum AttnForm[^{]*\{(.*?)\n\};", src, re.S).group(1)
    assert tuple(re.findall(r"^\s*(kAttn\w+)", body, re.M)) == FORMS
    assert seen[False] | seen[True] == set(range(len(FORMS)))


def test_decisions_the_issue_names(plan):
    """Spelled out, besides the table: the packed rule, the split switches ignored for packed rows, the backward streaming
    when EITHER panel is over the limit."""
    for bwd, one_wg in ((False, BF16_SEQ), (True, BF16_ROLES8)):
        # packed: the one-workgroup forms up to 512 whatever stream_keys and the split switches say, streaming beyond
        for sk, sw in itertools.product((False, True), (0, FWD_SPLIT | BWD_SPLIT)):
            assert plan(case(BF16, 32, 9, 512, packed=True, stream_keys=sk, switches=sw), bwd)[1]["form"] == one_wg
            assert plan(case(BF16, 32, 9, 513, packed=True, stream_keys=sk, switches=sw), bwd)[1]["form"] == BF16_STREAM
        # padded: the split switch of the pass gives the 128-row-block form, the other pass's does not
        own, other = (BWD_SPLIT, FWD_SPLIT) if bwd else (FWD_SPLIT, BWD_SPLIT)
        assert plan(case(BF16, 32, 9, 512, switches=own), bwd)[1]["form"] == BF16_PANEL
        assert plan(case(BF16, 32, 9, 512, switches=other), bwd)[1]["form"] == one_wg
        assert plan(case(BF16, 32, 9, 512, stream_keys=True), bwd)[1]["form"] == BF16_STREAM
    # 1152 < L <= 1248: the K/V panel fits, the Q/dO panel does not -- panel forward, streaming dQ AND dK/dV
    assert bf16_smem_fwd(1153) <= LDS_LIMIT < bf16_smem_dkv(1153)
    assert plan(case(BF16, 32, 2, 1153), False)[1]["form"] == BF16_PANEL
    assert plan(case(BF16, 32, 2, 1153), True)[1] == dict(zip(FIELDS, (BF16_STREAM, 2, 10 * 2 * 8, 1, 256, 32816, 35840)))
    # the lock-step backward never meets the LDS limit where it runs (the launcher's test on it could not fire)
    assert max(bf16_smem_fused(L) for L in range(1, FUSED_MAX_L + 1)) == 76800 <= LDS_LIMIT


def test_generic_boundaries_move_in_32_row_steps(plan):
    for prec, dh in GENERIC_FAMILIES:
        g, bounds = Generic(prec, dh), generic_boundaries(prec, dh)
        assert bounds["dkv"] <= bounds["dq"] <= bounds["fwd"]
        for name, smem in (("fwd", g.fwd_smem), ("dq", g.dq_smem), ("dkv", g.dkv_smem)):
            last = bounds[name]
            assert last % 32 == 0 and last >= 128
            assert smem(last - 31) == smem(last) <= LDS_LIMIT < smem(last + 1) == smem(last + 32)
        for bwd, last in ((False, bounds["fwd"]), (True, bounds["dkv"])):  # the backward: either panel over the limit
            for L, form in ((last - 31, GENERIC_PANEL), (last, GENERIC_PANEL), (last + 1, GENERIC_STREAM),
                            (last + 32, GENERIC_STREAM)):
                rc, p = plan(case(prec, dh, 2, L), bwd)
                assert (rc, p["form"]) == (OK, form), (prec, dh, bwd, L, p)
            a, b = plan(case(prec, dh, 2, last - 31), bwd)[1], plan(case(prec, dh, 2, last), bwd)[1]
            assert (a["lds0"], a["lds1"]) == (b["lds0"], b["lds1"])


def _blocks_of_grid(gx, B, L, A):
    """attn_block's mapping of the one-dimensional bf16 grid: the (128-row block, b * A + h) of every valid workgroup."""
    nblk = (L + 127) // 128
    per_b = nblk * A
    got = []
    for d in range(gx):
        xcd, slot = d & 7, d >> 3
        b, r = (slot // per_b) * 8 + xcd, slot % per_b
        if b < B:
            got.append((r % nblk, b * A + r // nblk))
    return got


def test_pins_against_the_parent_commits_record(plan):
    # streaming LDS (attention.hip's table; profiles/attn_stream.md)
    assert (BF16_STREAM_FWD, BF16_STREAM_DKV) == (32816, 35840)
    rc, p = plan(case(BF16, 32, 2, 257, stream_keys=True), True)
    assert (rc, p["form"], p["lds0"], p["lds1"]) == (OK, BF16_STREAM, 32816, 35840)
    assert plan(case(BF16, 32, 2, 257, stream_keys=True), False)[1]["lds0"] == 32816
    # the bf16 panel at L = 1024 (profiles/attn_stream.md)
    assert plan(case(BF16, 32, 2, 1024, causal=False), False)[1]["lds0"] == 131208
    rc, p = plan(case(BF16, 32, 2, 1024, causal=False), True)
    assert (p["form"], p["lds0"], p["lds1"]) == (BF16_PANEL, 131208, 143360)
    # where the bf16 head-size-32 panels stop fitting (commit 33b8f6a): 1248 forward, 1152 backward
    assert last_fit(bf16_smem_fwd) == 1248 and last_fit(bf16_smem_dkv) == 1152
    for bwd, last in ((False, 1248), (True, 1152)):
        assert plan(case(BF16, 32, 2, last), bwd)[1]["form"] == BF16_PANEL
        assert plan(case(BF16, 32, 2, last + 1), bwd)[1]["form"] == BF16_STREAM
    # the grid of 32 x 12 x 1024: eight 128-row blocks per (batch, head)
    B, A, L = 32, 12, 1024
    for bwd in (False, True):
        rc, p = plan(case(BF16, 32, B, L, A=A), bwd)
        assert (rc, p["form"], p["grid_x"], p["grid_y"], p["block"]) == (OK, BF16_PANEL, 3072, 1, 256)
        rc, p = plan(case(F32, 32, B, L, A=A), bwd)
        assert (rc, p["form"], p["grid_x"], p["grid_y"], p["block"]) == (OK, GENERIC_STREAM, 8, 384, 256)
    assert plan(case(BF16, 32, B, 512, A=A), False)[1]["grid_x"] == 384  # one workgroup per (batch, head)
    # the one-dimensional grids cover every (block, batch, head) exactly once, also with the batch padded to eight
    for B_, L_ in ((32, 1024), (9, 130), (1, 33)):
        gx = plan(case(BF16, 32, B_, L_, A=A, causal=False), False)[1]["grid_x"]
        want = sorted(itertools.product(range((L_ + 127) // 128), range(B_ * A)))
        assert sorted(_blocks_of_grid(gx, B_, L_, A)) == want


def test_return_codes_are_the_parents(plan):
    def rc(c, bwd):
        got = plan(c, bwd)
        assert got == rules(c, bwd) and (got[0] == OK or got[1] == REFUSED)
        return got[0]

    for bwd in (False, True):
        # packed rows: the bf16 head-size-32 causal kernels only
        assert rc(case(BF16, 32, 2, 40, packed=True), bwd) == OK
        assert rc(case(F32, 32, 2, 40, packed=True), bwd) == EUNSUPPORTED
        assert rc(case(F32, 32, 2, 40, packed=True, s16=True), bwd) == EUNSUPPORTED  # (refused before the storage is looked at)
        assert rc(case(BF16, 64, 2, 40, packed=True), bwd) == EUNSUPPORTED
        assert rc(case(BF16, 32, 2, 40, packed=True, causal=False), bwd) == EUNSUPPORTED
        assert rc(case(BF16, 32, 2, 600, packed=True, causal=False), bwd) == EUNSUPPORTED
        # the fp32 policy has no bf16 storage; an unknown policy
        assert rc(case(F32, 32, 2, 40, s16=True), bwd) == EINVAL
        assert rc(case(F32, 64, 2, 40, s16=True), bwd) == EINVAL
        assert rc(case(2, 32, 2, 40), bwd) == EINVAL
        # check_shape: head sizes other than 32 and 64; non-positive sizes
        assert rc(dict(case(BF16, 32, 2, 40), H=96), bwd) == EUNSUPPORTED  # 2 heads of 48
        assert rc(dict(case(F32, 32, 2, 40, s16=True), H=96), bwd) == EUNSUPPORTED
        for k in ("B", "L", "A", "H"):
            for v in (0, -1):
                assert rc(dict(case(BF16, 32, 2, 40), **{k: v}), bwd) == EINVAL


def test_every_configuration_the_encoder_accepts_has_a_plan(native, plan):
    """The encoder's check_cfg and attention's plan agree: a configuration with a workspace size gets XFMR_OK from both
    passes at its shape, storage (bf16 storage where the encoder mixes) and mask -- packed and padded."""
    cfgs = [EP.cfg(3, L, hidden=64, inter=128, precision=prec, flags=flags, packed_rows=(L + 7) * packed)
            for L, packed, (prec, flags) in itertools.product((513, 2048), (0, 1), ((BF16, 0), (F32, 0),
                                                                                    (BF16, EP.BIDIRECTIONAL)))]
    cfgs += [dict(EP.cfg(3, L, hidden=64, inter=128, packed_rows=(L + 7) * packed), heads=1)  # head size 64
             for L, packed in itertools.product((513, 2048), (0, 1))]
    cfgs += EP.TABLE[::5]
    got = EP.run_table(native, cfgs, {})
    accepted = packed_ok = 0
    for c, (rc, p, _, nbytes) in zip(cfgs, got):
        if not nbytes:
            assert c["packed_rows"]  # (the padded layout is accepted throughout these tables)
            continue
        accepted += 1
        packed_ok += bool(c["packed_rows"])
        key = dict(prec=c["precision"], s16=bool(p["mix"]), B=c["batch"], L=c["seq_len"], A=c["heads"], H=c["hidden"],
                   causal=bool(p["causal"]), packed=bool(c["packed_rows"]), stream_keys=False, switches=0)
        for bwd in (False, True):
            assert plan(key, bwd)[0] == OK, (c, bwd)
    assert accepted > 100 and packed_ok >= 4


SWITCH_WORKER = r"""
report(lib.xf_attn_switches(), lib.xf_attn_switches())
"""


@pytest.mark.parametrize("env,want", [
    ({}, 0),
    ({"XFMR_ATTN_FWD_SPLIT": "0", "XFMR_ATTN_BWD_SPLIT": "0", "XFMR_ATTN_BWD_FORM": "lockstep"}, 0),
    ({"XFMR_ATTN_FWD_SPLIT": "1"}, FWD_SPLIT),
    ({"XFMR_ATTN_BWD_SPLIT": "1"}, BWD_SPLIT),
    ({"XFMR_ATTN_BWD_FORM": "roles"}, BWD_ROLES),
    ({"XFMR_ATTN_FWD_SPLIT": "1", "XFMR_ATTN_BWD_SPLIT": "1", "XFMR_ATTN_BWD_FORM": "roles"}, 7),
    ({"XFMR_ATTN_FWD_SPLIT": "", "XFMR_ATTN_BWD_SPLIT": "on", "XFMR_ATTN_BWD_FORM": ""}, 0),  # atoi; a leading 'r'
    ({"XFMR_ATTN_FWD_SPLIT": "2", "XFMR_ATTN_BWD_SPLIT": "-1", "XFMR_ATTN_BWD_FORM": "r"}, 7),
], ids=lambda v: "-".join(f"{k[10:]}={x}" for k, x in v.items()) or "unset" if isinstance(v, dict) else str(v))
def test_switches_as_the_library_reads_them(native, env, want):
    """A fresh process each (the two split switches are read once per process); no GPU."""
    clean = {k: v for k, v in os.environ.items() if not k.startswith("XFMR_ATTN_")}
    torch_imported, got = run_worker(SWITCH_WORKER, native.LIB_PATH, clean | env)
    assert torch_imported is False and got == [want] * 2


def test_split_switches_are_read_once_and_the_backward_form_per_call(native):
    worker = SWITCH_WORKER.replace("report(", "first = lib.xf_attn_switches()\n"
                                   "os.environ.update(XFMR_ATTN_FWD_SPLIT='1', XFMR_ATTN_BWD_SPLIT='1', "
                                   "XFMR_ATTN_BWD_FORM='roles')\nreport(first, ")
    clean = {k: v for k, v in os.environ.items() if not k.startswith("XFMR_ATTN_")}
    torch_imported, got = run_worker(worker, native.LIB_PATH, clean)
    assert torch_imported is False and got == [0, BWD_ROLES, BWD_ROLES]


def test_plan_entry_is_internal(native):
    header = (ROOT / "include" / "xfmr_hip.h").read_text()
    for name in ("xf_attn_plan", "xf_attn_switches"):
        assert name not in header and name not in native.EXPORTED_SYMBOLS
    assert re.search(r"#define\s+XFMR_ABI_VERSION\s+3\b", header) and native.ABI_VERSION == 3
