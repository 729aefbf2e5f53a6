"""CPU-side test (no GPU) of the session path's host logic: xfmr_rec_amd/session.py's pure functions (the window rule, the
caller's contract), SessionRecommender's slot bookkeeping on a stub encoder, and -- on the built library -- the session
entries' size queries, their plan and every refusal, all of which return before anything is launched. The new header
(include/xfmr_session.h) is held to its ctypes table with the parser of tests/test_abi_tables_host.py."""

import ctypes as C

import pytest

from xfmr_rec_amd.session import SessionRecommender, check_rows, session_plan

HANDLE = 0x7F0000001000
EINVAL, EUNSUPPORTED, EWORKSPACE, EALIGN = -1, -2, -3, -5
F32, BF16 = 0, 1
BIDIRECTIONAL = 1


# ---------------------------------------------------------------------------------------------- session_plan / check_rows
def test_append_below_the_window():
    assert session_plan({0: 0, 1: 5}, {0: [7], 1: [8]}, 10) == {0: ("append", 0, [7]), 1: ("append", 5, [8])}
    assert session_plan({2: 9}, {2: [4]}, 10) == {2: ("append", 9, [4])}  # the last free row is still an append
    assert session_plan({2: 3}, {2: []}, 10) == {}                        # nothing new: nothing to run


def test_rebuild_exactly_when_the_slot_is_full():
    assert session_plan({0: 10}, {0: [4]}, 10) == {0: ("rebuild", 9, [4])}   # keep the last 9 stored, then the new one
    assert session_plan({0: 9}, {0: [4, 5]}, 10) == {0: ("rebuild", 8, [4, 5])}
    assert session_plan({0: 9}, {0: [4]}, 10) == {0: ("append", 9, [4])}
    # more new items than the window holds: the last max_len of them, nothing stored survives
    assert session_plan({0: 3}, {0: list(range(1, 15))}, 10) == {0: ("rebuild", 0, list(range(5, 15)))}
    kind, keep, items = session_plan({0: 10}, {0: [1, 2, 3]}, 10)[0]
    assert kind == "rebuild" and keep + len(items) == 10


def test_several_items_for_one_slot_in_one_call():
    plan = session_plan({0: 2, 1: 0}, [(0, [5]), (1, [6]), (0, [7, 8])], 10)
    assert plan == {0: ("append", 2, [5, 7, 8]), 1: ("append", 0, [6])}
    assert list(plan) == [0, 1]  # slots in the order of their first occurrence


def test_plan_refuses_unknown_slots_and_bad_lengths():
    with pytest.raises(ValueError, match="not open"):
        session_plan({0: 1}, {1: [3]}, 10)
    with pytest.raises(ValueError, match="outside"):
        session_plan({0: 11}, {0: [3]}, 10)
    with pytest.raises(ValueError, match="outside"):
        session_plan({0: -1}, {0: [3]}, 10)
    with pytest.raises(ValueError, match="positive"):
        session_plan({0: 0}, {0: [3]}, 0)


def test_check_rows_sees_duplicates_and_ranges():
    check_rows([0, 0, 1, 3], [0, 1, 0, 9], n_slots=4, max_len=10)
    with pytest.raises(ValueError, match="twice"):
        check_rows([0, 1, 0], [2, 2, 2], 4, 10)
    for slots, pos in (([4], [0]), ([-1], [0])):
        with pytest.raises(ValueError, match="slot"):
            check_rows(slots, pos, 4, 10)
    for slots, pos in (([0], [10]), ([0], [-1])):
        with pytest.raises(ValueError, match="position"):
            check_rows(slots, pos, 4, 10)
    with pytest.raises(ValueError, match="slots for"):
        check_rows([0, 1], [0], 4, 10)


# ---------------------------------------------------------------------------------------------- slot bookkeeping
class StubEncoder:
    """What SessionRecommender asks of an encoder, recorded."""

    def __init__(self):
        self.log = []

    def prefill(self, slots, histories):
        self.log.append(("prefill", list(slots), [list(h) for h in histories]))

    def append(self, slots, items):
        self.log.append(("append", list(slots), list(items)))

    def reset(self, slots):
        self.log.append(("reset", list(slots)))


class StubModule:
    known = {"a": 1, "b": 2, "c": 3}

    def _to_idx_or_empty(self, ids):
        return [self.known[i] if isinstance(i, str) else int(i) for i in ids if not isinstance(i, str) or i in self.known]


def test_slots_are_handed_out_returned_and_reused():
    enc = StubEncoder()
    rec = SessionRecommender(StubModule(), 2, encoder=enc)
    assert rec.start("u1", ["a", "zzz", "b"]) == 0 and rec.start("u2") == 1 and len(rec) == 2
    assert enc.log == [("prefill", [0], [[1, 2]]), ("prefill", [1], [[]])]  # the unknown id is dropped
    with pytest.raises(RuntimeError, match="all 2 session slots are in use"):
        rec.start("u3", ["a"])
    assert len(rec) == 2 and "u3" not in rec.slot_of  # nothing was evicted, nothing half-opened
    with pytest.raises(KeyError):
        rec.start("u1")
    rec.append("u1", "c")
    rec.append("u1", "unknown")  # dropped: no device call
    assert enc.log[-1] == ("append", [0], [3]) and rec.seen["u1"] == [1, 2, 3]
    rec.close("u1")
    assert enc.log[-1] == ("reset", [0]) and len(rec) == 1
    with pytest.raises(KeyError):
        rec.append("u1", "a")
    with pytest.raises(KeyError):
        rec.close("u1")
    assert rec.start("u3", [5]) == 0 and rec.seen["u3"] == [5]  # the freed slot is reused; integers are rows already
    assert sorted(rec.slot_of.values()) == [0, 1]


# ---------------------------------------------------------------------------------------------- the built library
@pytest.fixture(scope="module")
def native():
    from xfmr_rec_amd import _native as N

    if not N.LIB_PATH.exists():
        pytest.fail(f"{N.LIB_PATH} missing: run build() first")
    return N


def make(native, hidden=128, heads=4, inter=512, layers=2, max_pos=200, precision=BF16, flags=0, batch=4, seq_len=None, **kw):
    return native.EncoderCfg(batch=batch, seq_len=seq_len or max_pos, hidden=hidden, heads=heads, inter=inter, layers=layers,
                             max_pos=max_pos, precision=precision, ln_eps=1e-12, flags=flags, **kw)


def plan_of(native, cfg):
    out = (C.c_int32 * 8)()
    rc = native.load().xfmr_session_plan(C.byref(cfg), out)
    return rc, list(out)


def test_plan_names_the_split_for_both_head_sizes_and_element_types(native):
    # (chunk, lanes per key, keys per load, bytes per element, bf16 storage, max_len)
    assert plan_of(native, make(native))[1][:6] == [32, 4, 16, 2, 1, 200]                      # head size 32, bf16
    assert plan_of(native, make(native, precision=F32))[1][:6] == [32, 8, 8, 4, 0, 200]
    assert plan_of(native, make(native, heads=2))[1][:6] == [32, 8, 8, 2, 1, 200]              # head size 64
    assert plan_of(native, make(native, heads=2, precision=F32))[1][:6] == [32, 16, 4, 4, 0, 200]
    assert plan_of(native, make(native, max_pos=2048))[1][5] == 2048  # the length the bf16 family trains at
    for rc, out in (plan_of(native, make(native, heads=2, precision=p)) for p in (F32, BF16)):
        assert rc == 0 and out[0] % out[2] == 0 and out[1] * out[2] == 64 and out[1] * 16 == 64 * out[3]


def test_state_bytes_are_the_panels_the_masks_the_rows_and_the_copy(native):
    lib = native.load()
    for prec, es in ((F32, 4), (BF16, 2)):
        cfg = make(native, precision=prec)
        one, nine = (lib.xfmr_session_state_bytes(C.byref(cfg), n) for n in (1, 9))
        per_slot = 200 * (2 * 128 * 2 * es + 1 + 128 * 4)  # K and V of two layers, a mask byte and an fp32 row per position
        assert nine - one == pytest.approx(8 * per_slot, abs=3 * 256)  # (each part is rounded up to 256 bytes)
        copy = 2 * lib.xfmr_param_count(C.byref(cfg)) if prec == BF16 else 0
        assert one == pytest.approx(per_slot + copy, abs=4 * 256)
        ws1, ws64 = (lib.xfmr_session_workspace_bytes(C.byref(cfg), r) for r in (1, 64))
        # per row: x, x1, the pre-LayerNorm sum, qkv, ctx (8 H floats at most), the gelu output, a mask byte and a position
        assert 0 < ws1 < ws64 < 64 * (128 * 4 * 8 + 512 * 4 + 8) + 10 * 256
    assert lib.xfmr_session_state_bytes(None, 4) == 0 and lib.xfmr_session_state_bytes(C.byref(make(native)), 0) == 0
    assert lib.xfmr_session_workspace_bytes(C.byref(make(native)), 0) == 0


def test_refusals_come_before_any_launch(native):
    """Every call below returns from the entries' own checks: nothing is launched, no pointer is dereferenced."""
    lib = native.load()
    cfg = make(native, hidden=64, heads=2, inter=128)
    state_n, work_n = lib.xfmr_session_state_bytes(C.byref(cfg), 4), lib.xfmr_session_workspace_bytes(C.byref(cfg), 8)
    assert state_n > 0 and work_n > 0
    ptrs = dict(params=HANDLE, state=HANDLE, item_idx=HANDLE, row_slot=HANDLE, row_pos=HANDLE, table=HANDLE, tok_out=HANDLE,
                workspace=HANDLE)

    def append(cfg=cfg, state_bytes=state_n, work_bytes=work_n, n_rows=8, **over):
        p = ptrs | over
        return lib.xfmr_session_append(C.byref(cfg) if cfg is not None else None, p["params"], p["state"], state_bytes, 4,
                                       p["item_idx"], p["row_slot"], p["row_pos"], n_rows, p["table"], 201, p["tok_out"],
                                       p["workspace"], work_bytes, None)

    def init(cfg=cfg, state_bytes=state_n, params=HANDLE, state=HANDLE):
        return lib.xfmr_session_init(C.byref(cfg), params, state, state_bytes, 4, None)

    def pool(cfg=cfg, state_bytes=state_n, mode=0, slots=HANDLE, n=2):
        return lib.xfmr_session_pool(C.byref(cfg), HANDLE, state_bytes, 4, slots, HANDLE, n, mode, 0, 1e-12, HANDLE, None)

    refused = [
        (make(native, hidden=64, heads=2, inter=128, flags=BIDIRECTIONAL), EUNSUPPORTED),  # an append changes every row there
        (make(native, hidden=64, heads=2, inter=128, hidden_dropout=0.1), EINVAL),
        (make(native, hidden=64, heads=2, inter=128, attn_dropout=0.1), EINVAL),
        (make(native, hidden=64, heads=3, inter=128), EUNSUPPORTED),                        # head size
        (make(native, hidden=64, heads=2, inter=128, layers=65), EUNSUPPORTED),
        (make(native, hidden=64, heads=2, inter=128, seq_offsets=HANDLE, row_pos=HANDLE, packed_rows=8), EINVAL),
        (make(native, hidden=64, heads=2, inter=128, row_pos=HANDLE), EINVAL),               # this entry has its own row arrays
        (make(native, hidden=64, heads=2, inter=128, precision=7), EINVAL),
    ]
    for bad, code in refused:
        assert append(cfg=bad) == code and init(cfg=bad) == code and pool(cfg=bad) == code
        assert plan_of(native, bad)[0] == code
        assert lib.xfmr_session_state_bytes(C.byref(bad), 4) == 0 and lib.xfmr_session_workspace_bytes(C.byref(bad), 8) == 0
        assert append(cfg=bad, params=None, state_bytes=0) == code  # the cfg is judged first
    assert append(cfg=None) == EINVAL
    for name in ptrs:
        if name != "tok_out":  # (optional: NULL is a valid call, which would launch -- not here)
            assert append(**{name: None}) == EINVAL, name
    for name in ("params", "state", "table", "workspace", "tok_out"):
        assert append(**{name: HANDLE + 4}) == EALIGN, name
    assert append(params=None, table=HANDLE + 4) == EINVAL     # null before misaligned
    assert append(n_rows=0) == EINVAL
    assert append(state_bytes=state_n - 1) == EWORKSPACE and append(work_bytes=work_n - 1) == EWORKSPACE
    assert append(n_rows=9) == EWORKSPACE                      # more rows than the workspace was sized for
    assert append(table=HANDLE + 4, work_bytes=0) == EALIGN    # alignment before the sizes
    assert init(state_bytes=state_n - 1) == EWORKSPACE and init(params=None) == EINVAL and init(state=HANDLE + 8) == EALIGN
    assert pool(state_bytes=state_n - 1) == EWORKSPACE and pool(mode=4) == EINVAL and pool(slots=None) == EINVAL
    assert pool(n=0) == EINVAL


def test_the_session_header_is_its_table(native):
    """include/xfmr_session.h against _abi.SESSION_SIGNATURES, position by position, with test_abi_tables_host's parser; the
    ABI version stays 3 and xfmr_hip.h keeps its prototypes (that file's own test counts them)."""
    import re

    import test_abi_tables_host as T
    from xfmr_rec_amd import _abi

    text = T.clean((T.ROOT / "include" / "xfmr_session.h").read_text())
    protos = T.prototypes(T.without_structs(text), "xfmr_")
    assert len(protos) == 6 and tuple(protos) == tuple(_abi.SESSION_SIGNATURES) == native.SESSION_SYMBOLS
    assert T.table_problems(protos, _abi.SESSION_SIGNATURES) == []
    assert not set(_abi.SESSION_SIGNATURES) & (set(_abi.SIGNATURES) | set(_abi.INTERNAL_SIGNATURES))
    lib = native.load()
    for name, (res, args) in _abi.SESSION_SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.argtypes == args and fn.restype is res, name
    assert lib.xfmr_abi_version() == 3 and C.sizeof(native.EncoderCfg) == 136
    # a dropped argument is seen
    res, args = _abi.SESSION_SIGNATURES["xfmr_session_append"]
    got = T.table_problems(protos, _abi.SESSION_SIGNATURES | {"xfmr_session_append": (res, args[:-1])})
    assert got == ["xfmr_session_append: 15 parameters, the table has 14"]
    assert re.search(r"#define\s+XFMR_ABI_VERSION\s+3\b", (T.ROOT / "include" / "xfmr_hip.h").read_text())
