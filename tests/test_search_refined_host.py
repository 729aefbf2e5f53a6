"""CPU-side test (no GPU) of the refined search's C surface: include/xfmr_search.h against its ctypes table, every refusal
and their order with nothing launched, and the host-only plan query."""

import ctypes as C
import re

import pytest

HANDLE = 0x7F0000001000  # an aligned address that no call below may dereference
EINVAL, EUNSUPPORTED, EWORKSPACE, EALIGN = -1, -2, -3, -5
COSINE, DOT, L2 = 0, 1, 2


@pytest.fixture(scope="module")
def native():
    from xfmr_rec_amd import _native as N

    if not N.LIB_PATH.exists():
        pytest.fail(f"{N.LIB_PATH} missing: run build() first")
    return N


def plan_of(native, n_query=1024, n_rows=262144, H=384, k=20, refine=4):
    out = (C.c_int32 * 8)()
    rc = native.load().xfmr_search_refined_plan(n_query, n_rows, H, k, refine, out)
    return rc, list(out)


def test_the_search_header_is_its_table(native):
    import test_abi_tables_host as T
    from xfmr_rec_amd import _abi

    text = T.clean((T.ROOT / "include" / "xfmr_search.h").read_text())
    protos = T.prototypes(T.without_structs(text), "xfmr_")
    assert len(protos) == 3 and tuple(protos) == tuple(_abi.SEARCH_SIGNATURES) == native.SEARCH_SYMBOLS
    assert T.table_problems(protos, _abi.SEARCH_SIGNATURES) == []
    assert not set(_abi.SEARCH_SIGNATURES) & (set(_abi.SIGNATURES) | set(_abi.INTERNAL_SIGNATURES) | set(_abi.SESSION_SIGNATURES))
    lib = native.load()
    for name, (res, args) in _abi.SEARCH_SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.argtypes == args and fn.restype is res, name
    assert lib.xfmr_abi_version() == 3
    assert re.search(r"#define\s+XFMR_ABI_VERSION\s+3\b", (T.ROOT / "include" / "xfmr_hip.h").read_text())
    # a dropped argument and two exchanged ones are seen
    res, args = _abi.SEARCH_SIGNATURES["xfmr_search_refined"]
    got = T.table_problems(protos, _abi.SEARCH_SIGNATURES | {"xfmr_search_refined": (res, args[:-1])})
    assert got == ["xfmr_search_refined: 21 parameters, the table has 20"]
    swapped = args[:4] + [args[5], args[4]] + args[6:]  # table_sqnorm <-> table_max_norm
    got = T.table_problems(protos, _abi.SEARCH_SIGNATURES | {"xfmr_search_refined": (res, swapped)})
    assert got == ["xfmr_search_refined: parameter 4 is ptr, the table says f32",
                   "xfmr_search_refined: parameter 5 is f32, the table says ptr"]


def test_the_shared_device_pieces_are_written_once():
    """tt_better, the sort, the merge, the score formula and its scalar mirror live in csrc/retrieval_common.h; neither
    source file defines them again."""
    import test_abi_tables_host as T

    common = (T.CSRC / "retrieval_common.h").read_text()
    for name in ("tt_better", "tt_finite", "tt_sort", "tt_excluded", "tt_merge", "rk_score", "rk_chain_dot", "rk_inv_norm",
                 "rk_query_sqnorm", "rk_item_score", "tiled_plan", "search_check"):
        define = re.compile(r"^[\w\s<>]*\b" + name + r"\s*\([^;{}]*\)\s*\{", re.M)
        assert len(define.findall(common)) == 1, name
        for src in ("retrieval.hip", "search.hip"):
            text = (T.CSRC / src).read_text()
            assert not define.findall(text), (src, name)
            assert '#include "retrieval_common.h"' in text


def test_the_plan_names_tiles_slices_lds_and_k_short(native):
    rc, out = plan_of(native)
    assert rc == 0 and out[:2] == [32, 128]
    assert out[2] == 16 and out[3] == 16384 and out[2] * out[3] >= 262144  # 32 query tiles x 16 slices = 512 workgroups
    assert out[5] == 80 and out[6] == 128 and out[4] == 32 * 128 * 8 + 2 * 32 * 128 * 8 and out[4] <= 160 * 1024
    assert out[7] == 24                                                     # H <= 384: query fragments + two item images
    assert plan_of(native, H=392)[1][7] == 64 and plan_of(native, H=1024)[1][7] == 64 and plan_of(native, H=8)[1][7] == 24
    # k_short = max(k, min(k * refine, 128))
    got = [plan_of(native, k=k, refine=r)[1][5] for k, r in ((1, 1), (1, 4), (20, 4), (32, 4), (33, 4), (128, 1), (128, 4), (100, 4))]
    assert got == [1, 4, 80, 128, 128, 128, 128, 128]
    assert plan_of(native, k=20, refine=1)[1][5:7] == [20, 32] and plan_of(native, k=1, refine=1)[1][5:7] == [1, 1]
    assert plan_of(native, k=3, refine=10 ** 9)[1][5] == 128                # (no overflow on the way to the clamp)
    # the slices are the exact search's: one slice for a small catalogue, a partial last one at 4 001 rows
    assert plan_of(native, n_query=33, n_rows=4001)[1][2:4] == [16, 256] and plan_of(native, n_query=5, n_rows=100)[1][2:4] == [1, 128]
    # the workspace: per (query, slice) k_short pairs and a flag
    ws = native.load().xfmr_search_refined_workspace
    assert ws(1024, 262144, 80) == 1024 * 16 * (80 * 8 + 4) and ws(5, 100, 4) == 5 * (4 * 8 + 4)
    assert ws(0, 100, 4) == 0 and ws(5, 0, 4) == 0 and ws(5, 100, 0) == 0


def test_the_plan_refuses_what_the_search_refuses(native):
    for kw in (dict(n_query=0), dict(n_rows=0), dict(H=0), dict(k=0), dict(refine=0), dict(k=-1)):
        assert plan_of(native, **kw)[0] == EINVAL, kw
    for kw in (dict(H=12), dict(H=4), dict(H=1032), dict(k=129), dict(n_rows=2 ** 31), dict(n_query=2 ** 31)):
        assert plan_of(native, **kw)[0] == EUNSUPPORTED, kw
    assert plan_of(native, H=0, k=129)[0] == EINVAL  # EINVAL first
    assert native.load().xfmr_search_refined_plan(4, 100, 64, 5, 4, None) == EINVAL


def test_refusals_come_before_any_launch_and_in_order(native):
    """Every call below returns from the entry's own checks: nothing is launched, no pointer is dereferenced."""
    lib = native.load()
    need = lib.xfmr_search_refined_workspace(8, 100, 20)
    assert need > 0
    ptrs = dict(query=HANDLE, table=HANDLE, table_bf16=HANDLE, rnorm=HANDLE, sqnorm=HANDLE, excl=HANDLE, excl_off=HANDLE,
                out_idx=HANDLE, out_score=HANDLE, out_cert=HANDLE, workspace=HANDLE)

    def search(n_rows=100, n_query=8, H=64, k=5, k_short=20, metric=COSINE, ws_bytes=need, **over):
        p = ptrs | over
        return lib.xfmr_search_refined(p["query"], p["table"], p["table_bf16"], p["rnorm"], p["sqnorm"], 1.0, 1.0, n_rows,
                                       n_query, H, p["excl"], p["excl_off"], k, k_short, metric, p["out_idx"], p["out_score"],
                                       p["out_cert"], p["workspace"], ws_bytes, None)

    for name in ("query", "table", "table_bf16", "out_idx", "out_score", "out_cert", "workspace"):
        assert search(**{name: None}) == EINVAL, name
    assert search(excl=None) == EINVAL and search(excl_off=None) == EINVAL  # the pair, or neither
    assert search(rnorm=None) == EINVAL and search(rnorm=None, metric=DOT, ws_bytes=0) == EWORKSPACE  # only cosine needs it
    assert search(sqnorm=None, metric=L2) == EINVAL and search(sqnorm=None, ws_bytes=0) == EWORKSPACE
    for kw in (dict(n_rows=0), dict(n_query=0), dict(H=0), dict(k=0), dict(k=6, k_short=5), dict(metric=3), dict(metric=-1)):
        assert search(**kw) == EINVAL, kw
    for kw in (dict(H=12), dict(H=1032), dict(k_short=129), dict(k=129, k_short=129), dict(n_rows=2 ** 31), dict(n_query=2 ** 31)):
        assert search(**kw) == EUNSUPPORTED, kw
    for name in ("query", "table", "table_bf16", "workspace"):
        assert search(**{name: HANDLE + 8}) == EALIGN, name
    assert search(ws_bytes=need - 1) == EWORKSPACE and search(n_query=9) == EWORKSPACE
    # the order: EINVAL < EUNSUPPORTED < EALIGN < EWORKSPACE
    assert search(table=None, H=12, query=HANDLE + 8, ws_bytes=0) == EINVAL
    assert search(H=12, query=HANDLE + 8, ws_bytes=0) == EUNSUPPORTED
    assert search(k_short=129, table_bf16=HANDLE + 8, ws_bytes=0) == EUNSUPPORTED
    assert search(query=HANDLE + 8, ws_bytes=0) == EALIGN and search(table_bf16=HANDLE + 8, ws_bytes=0) == EALIGN


def test_search_option_names_and_the_environment_switch(monkeypatch):
    from xfmr_rec_amd import retrieval as R

    assert R.SEARCH_MODES == ("exact", "refined")
    monkeypatch.delenv("XFMR_SEARCH", raising=False)
    assert R.refined_search_enabled()
    monkeypatch.setenv("XFMR_SEARCH", "exact")
    assert not R.refined_search_enabled()  # read per call
    monkeypatch.setenv("XFMR_SEARCH", "refined")
    assert R.refined_search_enabled()
    with pytest.raises(ValueError, match="search must be one of"):
        R.ExactItemIndex.search_rows(object(), None, None, 5, search="ann")
