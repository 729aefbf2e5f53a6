"""The row kernels' plan (csrc/row_plan.inc: row_plan, exported as xf_row_plan) held to the rules of tests/row_cases.py --
`ln_form`, `ln_bwd_plan`, `colsum_plan`, restated from the launchers the plan replaced -- without a GPU: the instantiation and
its LDS per width, alignment and op; the forward grids; the backward row map at every threshold; and, for every row count up
to 70 000, that the record room the two public size queries return covers the records of every smaller call.

The library is asked in a fresh process without torch (tests/abi_worker.py), one process per table or sweep."""

import json
import os

import pytest

import row_cases as RC
from abi_worker import run_worker

OK, EINVAL, EUNSUPPORTED = 0, -1, -2
LN_FWD, GATHER_LN_FWD, LN_BWD, COLSUM = range(4)  # internal.h RowOp
NONE, GENERIC, FLOAT4 = range(3)  # RowForm
FIELDS = ("form", "width", "grid", "block", "lds", "rows_per_block", "records", "room")  # xf_row_plan's out, then zeros
REFUSED = dict.fromkeys(FIELDS, 0)
WIDTHS = (1, 63, 64, 65, 96, 127, 128, 129, 255, 256, 257, 320, 384, 512, 513, 768, 1024, 1025, 2048)
SWEEP_ROWS = 70000
SWEEP_WIDTHS = (64, 96, 128, 256, 320)


def cdiv(a, b):
    return -(-a // b)


def ln_room(rows):
    return min(1024, max(1, cdiv(rows, 4)))


def colsum_room(M):
    return min(128, max(1, cdiv(M, 256)))


def rules(op, rows, H, keep, aligned):
    """(rc, plan) the library has to give for a key, from row_cases' rules."""
    if rows <= 0 or H <= 0:
        return EINVAL, REFUSED
    if op == COLSUM:
        blocks, rp = RC.colsum_plan(rows)
        return OK, dict(form=GENERIC, width=64, grid=cdiv(H, 64) * blocks, block=256, lds=0, rows_per_block=rp, records=blocks,
                        room=colsum_room(rows))
    name = RC.ln_form(H, bool(aligned))
    if name is None:
        return EUNSUPPORTED, REFUSED
    form, width = (FLOAT4, int(name[3:])) if name.startswith("v4-") else (GENERIC, int(name[3:]))
    if op == LN_BWD:
        blocks, rpb = RC.ln_bwd_plan(rows, H)
        return OK, dict(form=form, width=width, grid=blocks, block=256, lds=12 * H * 4 if form == GENERIC else 0,
                        rows_per_block=rpb, records=blocks, room=ln_room(rows))
    rpb = 4 * (64 // width) if form == FLOAT4 else 4  # four waves of 64 / LPR rows, or of one
    return OK, dict(form=form, width=width, grid=cdiv(rows, rpb), block=256, lds=0, rows_per_block=rpb, records=0, room=0)


# ---------------------------------------------------------------------------------------------- the library
TABLE_WORKER = r"""
res = []
for op, rows, H, keep, aligned in json.load(sys.stdin):
    out = (C.c_int32 * 12)()
    rc = lib.xf_row_plan(op, rows, H, keep, aligned, out)
    res.append([rc, list(out)])
report(res)
"""

# records, rows_per_block, room and the public size query's bytes for every row count 1 ... n of one (op, H)
SWEEP_WORKER = r"""
op, H, n = json.load(sys.stdin)
size = lib.xfmr_colsum_workspace if op == 3 else lib.xfmr_layernorm_bwd_workspace
out = (C.c_int32 * 12)()
cols = [[], [], [], []]
for rows in range(1, n + 1):
    assert lib.xf_row_plan(op, rows, H, 1, 1, out) == 0
    for col, v in zip(cols, (out[6], out[5], out[7], size(rows, H))):
        col.append(v)
report(*cols)
"""


@pytest.fixture(scope="module")
def native():
    from xfmr_rec_amd import _native as N

    if not N.LIB_PATH.exists():
        pytest.fail(f"{N.LIB_PATH} missing: run build() first")
    return N


def ask(native, script, payload):
    torch_imported, values = run_worker(script, native.LIB_PATH, dict(os.environ), json.dumps(payload))
    assert torch_imported is False
    return values


def check_table(native, table):
    (res,) = ask(native, TABLE_WORKER, table)
    assert len(res) == len(table)
    plans = []
    for key, (rc, out) in zip(table, res):
        want_rc, want = rules(*key)
        plan = dict(zip(FIELDS, out))
        assert rc == want_rc, (key, rc, want_rc)
        assert plan == want, (key, {k: (plan[k], want[k]) for k in FIELDS if plan[k] != want[k]})
        assert out[len(FIELDS):] == [0] * (12 - len(FIELDS)), key
        plans.append(plan)
    return plans


# ---------------------------------------------------------------------------------------------- the tables
def test_decision_table(native):
    table = [(op, 77, H, keep, aligned) for op in (LN_FWD, GATHER_LN_FWD, LN_BWD, COLSUM) for H in WIDTHS
             for aligned in (0, 1) for keep in (0, 1)]
    plans = dict(zip(table, check_table(native, table)))
    for op in (LN_FWD, GATHER_LN_FWD, LN_BWD):  # the rules' own corner stones, so that the rules cannot drift with the library
        for keep in (0, 1):
            assert [(plans[op, 77, H, keep, 0]["form"], plans[op, 77, H, keep, 0]["width"]) for H in (64, 128, 256)] == [
                (GENERIC, 1), (GENERIC, 2), (GENERIC, 4)]
            assert [(plans[op, 77, H, keep, 1]["form"], plans[op, 77, H, keep, 1]["width"]) for H in (64, 128, 256)] == [
                (FLOAT4, 16), (FLOAT4, 32), (FLOAT4, 64)]
            for H in (1025, 2048):
                assert plans[op, 77, H, keep, 1] == REFUSED
            assert plans[op, 77, 1024, keep, 1]["width"] == 16 and plans[op, 77, 513, keep, 1]["width"] == 16
    assert plans[LN_BWD, 77, 320, 1, 1]["lds"] == 12 * 320 * 4 and plans[LN_BWD, 77, 256, 1, 1]["lds"] == 0
    assert plans[COLSUM, 77, 2048, 0, 0]["grid"] == 32  # the column sums take any width


def test_bad_keys_are_refused_with_all_zeros(native):
    table = [(op, rows, H, 1, 1) for op in (LN_FWD, GATHER_LN_FWD, LN_BWD, COLSUM) for rows, H in ((0, 64), (-1, 64), (5, 0), (5, -3))]
    check_table(native, table)
    (res,) = ask(native, TABLE_WORKER, [(4, 5, 64, 1, 1), (-1, 5, 64, 1, 1)])  # no such op
    assert res == [[EINVAL, [0] * 12]] * 2


def test_forward_grids(native):
    table = [(op, rows, H, keep, 1) for op in (LN_FWD, GATHER_LN_FWD) for keep in (0, 1) for H in (48, 100, 384, 1024)
             for rows in (1, 3, 4, 5, 77)]
    for H, edge in RC.LN_V4_EDGE_ROWS.items():  # one below, at and above a workgroup's 16 / 8 / 4 rows
        for rows in edge + (1, 77):
            table += [(op, rows, H, keep, aligned) for op in (LN_FWD, GATHER_LN_FWD) for keep in (0, 1) for aligned in (0, 1)]
    plans = dict(zip(table, check_table(native, table)))
    assert [plans[LN_FWD, rows, 100, 1, 1]["grid"] for rows in (1, 3, 4, 5, 77)] == [1, 1, 1, 2, 20]
    for H, edge in RC.LN_V4_EDGE_ROWS.items():
        assert [plans[LN_FWD, rows, H, 1, 1]["grid"] for rows in edge] == [1, 1, 2]
        assert plans[LN_FWD, edge[1], H, 1, 1]["rows_per_block"] == edge[1]


def test_backward_row_map(native):
    table = []
    for H in (64, 96, 128, 256, 320, 1024):
        it = 16 if H == 64 else 8 if H == 128 else 4
        for rows in (1, it - 1, it, it + 1, 77, 4095, 4096, 16383, 16384, 32768, 33001, 102400, 2 ** 20):
            table += [(LN_BWD, rows, H, 1, aligned) for aligned in (0, 1)]
    table += [(LN_BWD, rows, H, 1, 1) for H, rows, _ in RC.LN_RECORD_CASES]
    plans = dict(zip(table, check_table(native, table)))

    def pair(rows, H, aligned=1):
        p = plans[LN_BWD, rows, H, 1, aligned]
        return p["records"], p["rows_per_block"]

    # the pairs tests/test_row_cases_host.py states for the rule, from the library
    assert pair(77, 320) == (20, 4) and pair(77, 64) == (5, 16)
    for H, it in ((64, 16), (96, 4)):
        assert pair(4095, H) == (cdiv(4095, it), it) and pair(4096, H) == (256, 16)
        assert pair(16383, H) == (1024, 16) and pair(16384, H) == (512, 32)
        assert pair(33001, H) == ((688, 48) if H == 64 else (917, 36))
    for H, rows, records in RC.LN_RECORD_CASES:
        assert pair(rows, H)[0] == records
    for H in (64, 128, 256):  # an unaligned call takes the generic kernel and keeps the row map
        for rows in (77, 4096, 33001):
            assert pair(rows, H, 0) == pair(rows, H, 1)
            assert plans[LN_BWD, rows, H, 1, 0]["form"] == GENERIC and plans[LN_BWD, rows, H, 1, 1]["form"] == FLOAT4


# ---------------------------------------------------------------------------------------------- the room
def _sweep(native, op, H, rule, room, record_bytes):
    records, rpb, rooms, nbytes = ask(native, SWEEP_WORKER, [op, H, SWEEP_ROWS])
    assert len(records) == SWEEP_ROWS
    most, below = 0, 0
    for i in range(SWEEP_ROWS):
        rows = i + 1
        assert (records[i], rpb[i]) == rule(rows), (op, H, rows)
        below += records[i] < most
        most = max(most, records[i])
        assert rooms[i] == room(rows) and most <= rooms[i], (op, H, rows, most, rooms[i])
        assert nbytes[i] == rooms[i] * record_bytes, (op, H, rows)
    return below


@pytest.mark.parametrize("H", SWEEP_WIDTHS)
def test_layernorm_record_room_covers_every_smaller_call(native, H):
    """records == the rule; the running maximum of records <= room == min(1024, ceil(rows / 4)); xfmr_layernorm_bwd_workspace ==
    room records of 3 x H floats -- for every row count 1 ... 70 000."""
    _sweep(native, LN_BWD, H, lambda rows: RC.ln_bwd_plan(rows, H), ln_room, 3 * H * 4)


def test_colsum_record_room_covers_every_smaller_call(native):
    """The same for the column sums: room == min(128, ceil(M / 256)), xfmr_colsum_workspace == room records of N floats. The
    plan is not monotone (32 768 rows: 128 records, 32 769: 127): such counts exist, and the room covers them."""
    N = 96
    below = _sweep(native, COLSUM, N, RC.colsum_plan, colsum_room, N * 4)
    assert below > 0
    assert RC.colsum_plan(32768)[0] == 128 and RC.colsum_plan(32769)[0] == 127 and colsum_room(32769) == 128
