"""CPU-side test (no GPU) of the one plan field behind those tests/test_loss_plan_host.py reads: whether the gradient pass
keeps its count of counted logits (csrc/loss.hip: LossPlan::grad_no_count, read through the internal entry
xf_loss_plan_ext). The rule, restated here from the kernels' needs: only the two lean InfoNCE gradient codes can do
without the count (no InfoNCE result divides by it), and only when its readers -- the density / count statistics -- are
served elsewhere: by a logging pass of the same call (loss_buf), or because the caller says the call's stats[] are not
read (XFMR_LOSS_STATS_ELSEWHERE). xf_loss_plan itself shows the plan it showed before, flag or no flag."""

import ctypes as C
import itertools
import pathlib
import re

import pytest

from test_loss_plan_host import (BF16, CATALOG, DMA, F32, HEAD_INFONCE_MASKED, HEAD_INFONCE_PINNED, INFONCE, OK, QB, SHARED,
                                 FIELDS, case, flags)

ROOT = pathlib.Path(__file__).resolve().parents[1]
STATS_ELSEWHERE = 2
GRAD = 0


@pytest.fixture(scope="module")
def native():
    from xfmr_rec_amd import _native as N

    if not N.LIB_PATH.exists():
        pytest.fail(f"{N.LIB_PATH} missing: run build() first")
    return N


@pytest.fixture(scope="module")
def ask(native):
    lib = native.load()

    def both(c):
        out, ext = (C.c_int32 * 40)(*([-1] * 40)), (C.c_int32 * 8)(*([-1] * 8))
        args = (c["T"], c["H"], c["n_rows"], c["head"], c["all_heads"], c["masked"], c["mode"], c["prec"], c["hard"], c["flags"],
                int(c["d_tok"]), int(c["table_bf16"]), c["cus"], c["sw"])
        rc, rc2 = lib.xf_loss_plan(*args, out), lib.xf_loss_plan_ext(*args, ext)
        assert rc == rc2 and not any(ext[1:]) and not any(out[len(FIELDS):])
        return rc, dict(zip(FIELDS, out)), ext[0]

    return both


def grad_code(p):
    for i in range(p["npass"]):
        if p[f"p{i}_role"] == GRAD and p["family"] == DMA:
            return p[f"p{i}_code"]
    return None


def test_the_count_is_dropped_only_where_nobody_reads_it(ask):
    seen = set()
    table = itertools.product((64, 128, 256, 384), (3 * QB, 600 * QB), range(7), (0, 1, 2), (0, 1), (SHARED, CATALOG),
                              (BF16, F32), (0, 4), (False, True), (False, True), (0, STATS_ELSEWHERE),
                              (flags(), flags(3, 1), flags(3, 3)))
    for H, T, head, all_heads, masked, mode, prec, hard, d_tok, tbf, flag, plan_flags in table:
        if all_heads == 2 and d_tok:
            continue
        c = case(T, H, head=head, all_heads=all_heads, masked=masked, mode=mode, prec=prec, hard=hard, d_tok=d_tok,
                 table_bf16=tbf, flags=plan_flags | flag)
        rc, p, no_count = ask(c)
        rc0, p0, _ = ask(c | {"flags": plan_flags})
        assert (rc, p) == (rc0, p0), c  # the flag changes nothing xf_loss_plan shows
        if rc != OK:
            assert no_count == 0, c
            continue
        code = grad_code(p)
        lean_infonce = code in (HEAD_INFONCE_MASKED, HEAD_INFONCE_PINNED) and p["need_grad"] + p["p0_finish"] + p["p1_finish"] > 0
        want = int(lean_infonce and (p["loss_buf"] == 1 or flag != 0))
        assert no_count == want, (c, code, p)
        seen.add((code if lean_infonce else None, p["loss_buf"], flag, no_count))
    # every branch of the rule was walked: both codes drop it beside a logging pass without being told; the masked code
    # alone drops it on the flag and keeps it without; every other code keeps it, flag or not
    for code in (HEAD_INFONCE_MASKED, HEAD_INFONCE_PINNED):
        assert (code, 1, 0, 1) in seen and (code, 1, STATS_ELSEWHERE, 1) in seen
    assert (HEAD_INFONCE_MASKED, 0, STATS_ELSEWHERE, 1) in seen and (HEAD_INFONCE_MASKED, 0, 0, 0) in seen
    assert (None, 0, STATS_ELSEWHERE, 0) in seen and (None, 1, STATS_ELSEWHERE, 0) in seen and (None, 1, 0, 0) in seen
    assert not any(k[0] is None and k[3] for k in seen)


def test_the_benchmark_steps_calls(ask):
    """Config 2 at batch 512 (overlapped: gradient call all_heads = 0 with the flag, one split, rows finished in the kernel)
    and at batch 128 (in-line: all_heads = 1); --lean (all_heads = 0, no flag) keeps counting."""
    big = dict(head=INFONCE, masked=1, mode=SHARED, n_rows=3884)
    rc, p, no_count = ask(case(512 * 200, 128, all_heads=0, flags=1 | STATS_ELSEWHERE, **big))
    assert rc == OK and (grad_code(p), p["p0_gy"], p["p0_finish"], p["loss_buf"], no_count) == (HEAD_INFONCE_MASKED, 1, 1, 0, 1)
    rc, p, no_count = ask(case(128 * 200, 128, all_heads=1, **big))
    assert rc == OK and (grad_code(p), p["loss_buf"], no_count) == (HEAD_INFONCE_MASKED, 1, 1)
    rc, p, no_count = ask(case(512 * 200, 128, all_heads=0, flags=1, **big))
    assert rc == OK and (grad_code(p), no_count) == (HEAD_INFONCE_MASKED, 0)


def test_the_flag_is_public_and_the_entry_internal(native):
    header = (ROOT / "include" / "xfmr_hip.h").read_text()
    assert re.search(r"XFMR_LOSS_STATS_ELSEWHERE\s*=\s*2u", header) and native.LOSS_STATS_ELSEWHERE == STATS_ELSEWHERE
    assert native.LOSS_DTOK_ZEROED & native.LOSS_STATS_ELSEWHERE == 0 and STATS_ELSEWHERE < 1 << 8  # below the split fields
    assert "xf_loss_plan_ext" not in header and "xf_loss_plan_ext" not in native.EXPORTED_SYMBOLS
