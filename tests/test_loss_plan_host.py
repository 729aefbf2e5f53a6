"""CPU-side test (no GPU) of the fused sampled loss's plan (csrc/loss.hip: LossPlan / loss_plan, read through the internal
entry point xf_loss_plan): which main passes a call launches, in which kernel forms, with which grids and split counts, and
how the combine kernel is wired, is ONE function of the call's key, of the device's compute units and of four environment
switches. The rules are written here a second time, in Python, from the commit before the plan existed (d751a8e: run_loss
and launch_main_h of loss.hip, the four launchers xf_launch_loss_dma_<H> of loss_dma_h*.hip, xf_loss_dma_256_hparts and
loss_dma_hparts of loss_dma.inc), and a decision table is walked through the library on both sides of every boundary.
tests/test_gpu_loss_dma_forms.py names in comments the head code each of its cases reaches; the last tests here ask the
plan for them."""

import ctypes as C
import itertools
import os
import pathlib
import re

import pytest

from abi_worker import run_worker

ROOT = pathlib.Path(__file__).resolve().parents[1]
F32, BF16 = 0, 1
SHARED, CATALOG = 0, 1
OK, EINVAL, EUNSUPPORTED = 0, -1, -2
QB, BN = 128, 64  # queries per workgroup, negatives per tile (loss_common.h)
COMBINE_ROWS, VALUE_ROWS = 8, 256  # rows per workgroup of loss_combine_kernel and of its values-only form
GENERIC_BF16, GENERIC_F32, DMA = 0, 1, 2  # LossPlan::family
GRAD, LOG = 0, 1  # LossPass::role
# XFMR_LOSS_* heads and the kernel-template codes beyond them (loss_common.h)
ALIGNMENT, CCL, CONTRASTIVE, INFONCE, NCE, HINGE, BPR = range(7)
HEAD_INFONCE_MASKED, HEAD_INFONCE_PINNED, HEAD_BPR_MASKED, HEAD_CCL_MASKED, HEAD_CONTR_MASKED = range(7, 12)
HEAD_LOG_MASKED, HEAD_LOG_MASKED_LSE, HEAD_LOG_UNMASKED_CATALOG = -3, -4, -5
GENERAL_HEADS = {CCL, CONTRASTIVE, INFONCE, NCE, HINGE, BPR}
LEAN_CODES = {HEAD_INFONCE_MASKED, HEAD_INFONCE_PINNED, HEAD_BPR_MASKED, HEAD_CCL_MASKED, HEAD_CONTR_MASKED}
FAST_LOG_CODES = {HEAD_LOG_MASKED, HEAD_LOG_MASKED_LSE, HEAD_LOG_UNMASKED_CATALOG}
# the bits of xf_loss_switches
Q_FP32, LOGM256 = 1, 2


def switches(*, q_fp32=False, logm256=True, nsplit=0, nsplit_grad=0):
    return int(q_fp32) | int(logm256) << 1 | max(nsplit, 0) << 2 | max(nsplit_grad, 0) << 33


def flags(nsplit=0, nsplit_grad=0):  # XFMR_LOSS_NSPLIT(n) | XFMR_LOSS_NSPLIT_GRAD(n)
    return (nsplit & 0xff) << 8 | (nsplit_grad & 0xff) << 16


PASS_FIELDS = ("role", "code", "all", "gx", "gy", "gz", "nsplit", "buf", "image", "finish", "pinned")
FIELDS = (("family", "hard", "qprep", "npass") + tuple(f"p{i}_{f}" for i in (0, 1) for f in PASS_FIELDS) +
          ("need_grad", "c_nsplit", "c_nsplit_loss", "loss_buf", "lse_from_grad", "skip_train_head", "values_only", "blocks"))
REFUSED = dict.fromkeys(FIELDS, 0)


def case(T, H, *, n_rows=201, head=INFONCE, all_heads=1, masked=1, mode=SHARED, prec=BF16, hard=0, flags=0, d_tok=True,
         table_bf16=True, cus=256, sw=switches()):
    return dict(T=T, H=H, n_rows=n_rows, head=head, all_heads=all_heads, masked=masked, mode=mode, prec=prec, hard=hard,
                flags=flags, d_tok=d_tok, table_bf16=table_bf16, cus=cus, sw=sw)


# ---------------------------------------------------------------------------------------------- the parent's rules
def carve_nsplit(T, n_rows, ns_env, ns_flag):
    """make_plan's column-split count."""
    qblocks = (T + QB - 1) // QB
    tiles = (max(T, n_rows) + BN - 1) // BN
    ns = min((1024 + qblocks // 2) // qblocks, 16)
    if 32 <= qblocks < 64 and ns > 8:
        ns = 8
    ns = max(ns, 2)
    if ns < 4 and qblocks >= 512:
        ns = 4
    if ns_env > 0:
        ns = ns_env
    if ns_flag > 0:
        ns = ns_flag
    return max(min(ns, tiles), 1)


def generic_width(f32, H):
    """launch_main_h: the template width, or None (XFMR_EUNSUPPORTED)."""
    if H <= 0 or H & 31:
        return None
    for w in (64, 128, 256, 384, 512):
        if H <= w:
            return w
    if f32:
        return None
    return 768 if H <= 768 else 1024 if H <= 1024 else None


def generic_hparts(f32, W):
    """loss_main_hparts<P, W>."""
    return 1 if W <= 256 else W // 64 if f32 and W >= 512 else W // 128


def dma_256_hparts(head, masked, pin):
    """xf_loss_dma_256_hparts in the product build (XFL_H256_LEAN_HALVES = 0)."""
    return 2 if head == INFONCE and not masked and not pin else 1


def dma_launcher(H, head, masked, mode, pin, logm256):
    """xf_launch_loss_dma_<H>: (HEAD_* code, grid.z) for the head (or -1 / -2) run_loss passes."""
    gz = 1
    if H == 256 and head >= 0:
        gz = dma_256_hparts(head, masked, pin)
    if H == 384 and head == INFONCE and not masked and not pin:
        gz = 3
    fast_log = H in (64, 128) or (H == 256 and logm256)  # H = 384 has none of the three
    lean = masked and mode == SHARED
    if head == -1:
        return (HEAD_LOG_MASKED_LSE if fast_log and lean else -1), gz
    if head == -2:
        if fast_log and lean:
            return HEAD_LOG_MASKED, gz
        if fast_log and not masked and mode == CATALOG:
            return HEAD_LOG_UNMASKED_CATALOG, gz
        return -2, gz
    if head == CCL:
        return (HEAD_CCL_MASKED if lean else CCL), gz
    if head == CONTRASTIVE:
        return (HEAD_CONTR_MASKED if lean else CONTRASTIVE), gz
    if head == INFONCE:
        return (HEAD_INFONCE_MASKED if masked else HEAD_INFONCE_PINNED if pin else INFONCE), gz
    if head == BPR:
        return (HEAD_BPR_MASKED if lean else BPR), gz
    assert head in (NCE, HINGE)
    return head, gz


def _pass(role, code, all_, gx, gy, gz, buf, image, finish, pinned):
    return dict(zip(PASS_FIELDS, (role, code, int(all_), gx, gy, gz, gy, buf, int(image), int(finish), int(pinned))))


def rules(c):
    """(return code, plan fields) of the call c as d751a8e ran it."""
    T, H, n_rows, head, all_heads = c["T"], c["H"], c["n_rows"], c["head"], c["all_heads"]
    masked, mode, d_tok = bool(c["masked"]), c["mode"], c["d_tok"]
    sw = c["sw"]
    q_fp32, logm256 = bool(sw & Q_FP32), bool(sw & LOGM256)
    ns_env, ns_grad_env = sw >> 2 & 0x7fffffff, sw >> 33
    # check_loss_args
    if T <= 0 or n_rows <= 0 or T > 1 << 30 or n_rows > 1 << 30 or not 0 <= head < 7 or c["hard"] < 0:
        return EINVAL, REFUSED
    if c["prec"] not in (F32, BF16):
        return EINVAL, REFUSED
    f32 = c["prec"] == F32
    gx = (T + QB - 1) // QB
    ns = carve_nsplit(T, n_rows, ns_env, c["flags"] >> 8 & 0xff)
    ns_grad_flag = c["flags"] >> 16 & 0xff
    hard = c["hard"] > 0
    dma_width = H in (64, 128, 256, 384) and n_rows * H * 2 < 1 << 32
    passes = []
    p = dict(hard=int(hard), loss_buf=0, lse_from_grad=0)
    fused_finish = False
    if not hard and not f32 and c["table_bf16"] and dma_width:
        p["family"] = DMA
        grad_pass = d_tok and head != ALIGNMENT
        pinned = grad_pass and all_heads == 1 and head == INFONCE and not masked
        col_parts = (H > 128 and head == INFONCE and not masked and not pinned) or (
            H == 256 and grad_pass and not pinned and dma_256_hparts(head, masked, False) > 1)
        ns_grad = ns
        if gx >= 512 or (H <= 128 and gx > 256):
            ns_grad = 1
        if ns_grad_env > 0:
            ns_grad = ns_grad_env
        if ns_grad_flag > 0:
            ns_grad = ns_grad_flag
        ns_grad = min(max(ns_grad, 1), ns)
        if H > 128 and gx < 512 and ns_grad_env <= 0 and ns_grad_flag <= 0:
            best, best_cost = ns, 1e30
            for n in range(1, ns + 1):
                cost = ((gx * n + c["cus"] - 1) // c["cus"]) / n + 0.01 * n
                if cost < best_cost - 1e-9:
                    best, best_cost = n, cost
            ns_grad = best
        if not grad_pass or col_parts:
            ns_grad = ns
            if col_parts and ns_grad_env > 0:
                ns_grad = min(ns_grad_env, ns)
            if col_parts and ns_grad_flag > 0:
                ns_grad = min(ns_grad_flag, ns)
        ns_part = ns
        if grad_pass:
            ns_part = ns_grad
            fused_finish = ns_grad == 1 and not col_parts

        def image(n):
            return not q_fp32 and n > 1

        def grad(pin):
            code, gz = dma_launcher(H, head, masked, mode, pin, logm256)
            return _pass(GRAD, code, 0, gx, ns_grad, gz, 0, image(ns_grad), fused_finish, pin)

        def log(head_code, buf):
            code, gz = dma_launcher(H, head_code, masked, mode, False, logm256)
            return _pass(LOG, code, 0, gx, ns, gz, buf, image(ns), False, False)

        if pinned:
            passes = [log(-2, 1), grad(True)]
            p.update(loss_buf=1, lse_from_grad=1)
        else:
            if grad_pass:
                passes.append(grad(False))
            if all_heads != 0 or not grad_pass:
                lse_elsewhere = head == INFONCE and (grad_pass or all_heads == 2)
                passes.append(log(-2 if lse_elsewhere else -1, int(grad_pass)))
                p.update(loss_buf=int(grad_pass), lse_from_grad=int(lse_elsewhere and grad_pass))
        p["c_nsplit"], p["c_nsplit_loss"] = ns_part, ns if p["loss_buf"] else ns_part
    else:
        W = generic_width(f32, H)
        if W is None:
            return EUNSUPPORTED, REFUSED
        p["family"] = GENERIC_F32 if f32 else GENERIC_BF16
        gz = generic_hparts(f32, W) if d_tok else 1
        passes = [_pass(GRAD, W, all_heads != 0, gx, ns, gz, 0, False, False, False)]
        p["c_nsplit"] = p["c_nsplit_loss"] = ns
    p["npass"] = len(passes)
    p["qprep"] = int(any(q["image"] for q in passes))
    for i in (0, 1):
        q = passes[i] if i < len(passes) else dict.fromkeys(PASS_FIELDS, 0)
        p.update({f"p{i}_{f}": v for f, v in q.items()})
    p["need_grad"] = int(d_tok and not fused_finish)
    p["skip_train_head"] = int(all_heads == 2 and not d_tok)
    p["values_only"] = int(not p["need_grad"])
    rows = VALUE_ROWS if p["values_only"] else COMBINE_ROWS
    p["blocks"] = (T + rows - 1) // rows
    return OK, {f: p[f] for f in FIELDS}


# ---------------------------------------------------------------------------------------------- the decision table
QBLOCKS = (8, 31, 32, 63, 64, 100, 256, 257, 511, 512, 800)
WIDTHS_ALL = (32, 64, 96, 128, 256, 384, 512, 768, 1024, 1056)
DMA_WIDTHS = (64, 128, 256, 384)
# (train head, all_heads, d_tok, masked, mode): every combination
CALLS = list(itertools.product(range(7), (0, 1, 2), (True, False), (1, 0), (SHARED, CATALOG)))
SOME_CALLS = [k for k in CALLS if k[0] in (ALIGNMENT, CCL, INFONCE, BPR) and (k[1], k[2]) in ((0, True), (1, True), (2, False))]


def _call(T, H, k, **kw):
    return case(T, H, head=k[0], all_heads=k[1], d_tok=k[2], masked=k[3], mode=k[4], **kw)


def decision_table():
    t = []
    # every width x every call, below and above the 256-block threshold of the one-split gradient pass
    for H, qb, k in itertools.product(WIDTHS_ALL, (8, 257), CALLS):
        t.append(_call(qb * QB - 5, H, k))
    # the block thresholds; at H > 128 the CU-rounds cost search on three chips
    for H, qb, k in itertools.product(DMA_WIDTHS, QBLOCKS, SOME_CALLS):
        for cus in ((64, 256, 304) if H > 128 else (256,)):
            t.append(_call(qb * QB, H, k, cus=cus))
    # flag overrides (n_grad above n; the column-parts forms keep the split form) x the four switches
    plans = ((1, 1), (3, 3), (3, 1), (3, 5), (0, 2), (5, 0), (2, 0))
    sws = (switches(), switches(q_fp32=True), switches(logm256=False), switches(nsplit=6), switches(nsplit_grad=2),
           switches(q_fp32=True, logm256=False, nsplit=3, nsplit_grad=7))
    for H, qb, k, plan, sw in itertools.product(DMA_WIDTHS, (8, 800), SOME_CALLS[::3], plans, sws):
        t.append(_call(qb * QB - 1, H, k, flags=flags(*plan), sw=sw))
    # family: precision (one invalid), the table copy, hard negatives, n_rows H 2 on both sides of 2^32
    for H, prec, tb, hard, d_tok, all_heads in itertools.product(WIDTHS_ALL, (F32, BF16, 2), (True, False), (0, 4),
                                                                 (True, False), (0, 1)):
        edge = (1 << 32) // (2 * H)  # the first n_rows with n_rows H 2 >= 2^32 (its ceiling where H does not divide)
        for n_rows in (201, edge - 1, edge, edge + 1):
            t.append(case(1000, H, n_rows=n_rows, prec=prec, table_bf16=tb, hard=hard, d_tok=d_tok, all_heads=all_heads))
    # the key alone refused
    t += [case(0, 64), case(-3, 64), case((1 << 30) + 1, 64), case(320, 64, n_rows=0), case(320, 64, n_rows=(1 << 30) + 1),
          case(320, 64, head=7), case(320, 64, head=-1), case(320, 64, hard=-1), case(1 << 30, 64, n_rows=1 << 30)]
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
def lib(native):
    return native.load()


@pytest.fixture(scope="module")
def plan(lib):
    def ask(c):
        out = (C.c_int32 * 40)(*([-1] * 40))
        rc = lib.xf_loss_plan(c["T"], c["H"], c["n_rows"], c["head"], c["all_heads"], c["masked"], c["mode"], c["prec"],
                              c["hard"], c["flags"], int(c["d_tok"]), int(c["table_bf16"]), c["cus"], c["sw"], out)
        assert not any(out[len(FIELDS):])
        return rc, dict(zip(FIELDS, out))

    return ask


def test_plan_follows_the_parents_rules(plan):
    assert len(TABLE) > 8000
    seen = {}
    for c in TABLE:
        want = rules(c)
        assert plan(c) == want, (c, want)
        if want[0] == OK:
            seen.setdefault(want[1]["family"], set()).update(want[1][f"p{i}_code"] for i in range(want[1]["npass"]))
        else:
            seen.setdefault(want[0], set())
    assert set(seen) == {GENERIC_BF16, GENERIC_F32, DMA, EINVAL, EUNSUPPORTED}
    assert seen[GENERIC_BF16] == {64, 128, 256, 384, 512, 768, 1024} and seen[GENERIC_F32] == {64, 128, 256, 384, 512}
    assert seen[DMA] == {-1, -2} | GENERAL_HEADS | LEAN_CODES | FAST_LOG_CODES


def test_split_counts_the_parent_documents(plan):
    """The outcomes d751a8e's comments give for the CU-rounds cost search, the thresholds and the overrides."""
    def grad_splits(c):
        rc, p = plan(c)
        assert rc == OK and p["p0_role"] == GRAD and p["p0_finish"] == int(p["p0_gy"] == 1)
        return p["p0_gy"]

    lean = dict(head=CCL, all_heads=0)
    assert grad_splits(case(256 * QB, 256, **lean)) == 1           # config 5: one full round, rows finished in the kernel
    assert grad_splits(case(100 * QB, 256, **lean)) == 5           # config 4: two rounds of 250 instead of 10 splits
    assert grad_splits(case(100 * QB, 256, cus=304, **lean)) == 3  # (one round of 300)
    # 8 blocks at H = 384 (the reference's default model, 32 x 32 tokens): one round whatever n <= 16 on 256 CUs, so the
    # rule stops at the minimum of 1 / n + 0.01 n, n = 10 (0.2000; 0.2050 at the 8 its comment measured against 4 and 16).
    # 8 is what it gives where 8 n blocks stop fitting one round beyond n = 8 (64 CUs), or with XFMR_LOSS_NSPLIT(8).
    assert grad_splits(case(8 * QB, 384, **lean)) == 10
    assert grad_splits(case(8 * QB, 384, cus=64, **lean)) == 8
    assert grad_splits(case(8 * QB, 384, flags=flags(8), **lean)) == 8
    # H <= 128: one split from 257 blocks on; every width from 512 on
    assert [grad_splits(case(qb * QB, 128, **lean)) for qb in (256, 257, 511, 512)] == [4, 1, 1, 1]
    assert [grad_splits(case(qb * QB, 384, **lean)) for qb in (257, 512)] == [4, 1]  # (257: 5 rounds of a quarter walk)
    # the carve's count: 16 at most, 8 for 32 ... 63 blocks, 2 at least, 4 from 512 blocks on, never more than the tiles
    log_only = dict(all_heads=1, d_tok=False)
    got = [plan(case(qb * QB, 128, **log_only))[1]["p0_gy"] for qb in QBLOCKS]
    assert got == [16, 16, 8, 8, 16, 10, 4, 4, 2, 4, 4]
    assert plan(case(100, 128, n_rows=130, **log_only))[1]["p0_gy"] == 3
    # overrides: the flag beats the environment, the gradient count is clamped to the carve's
    rc, p = plan(case(320, 64, all_heads=0, flags=flags(3, 5), sw=switches(nsplit=7, nsplit_grad=2)))
    assert (p["p0_gy"], p["c_nsplit"], p["need_grad"], p["p0_image"]) == (3, 3, 1, 1)
    rc, p = plan(case(320, 64, all_heads=0, sw=switches(nsplit=3, nsplit_grad=2)))
    assert (p["p0_gy"], p["c_nsplit"]) == (2, 2)
    # the column-parts forms keep the split form whatever the plan says: partial dQ and the combine kernel's finish also
    # with one split; without a gradient override they take the carve's count, not the cost search's
    for H, parts in ((256, 2), (384, 3)):
        rc, p = plan(case(320, H, all_heads=0, masked=0, flags=flags(3, 1)))
        assert (p["p0_code"], p["p0_gz"], p["p0_gy"], p["p0_finish"], p["need_grad"]) == (INFONCE, parts, 1, 0, 1)
        rc, p = plan(case(320, H, all_heads=0, masked=0, flags=flags(3)))
        assert (p["p0_gz"], p["p0_gy"], p["p0_finish"], p["p0_image"], p["need_grad"]) == (parts, 3, 0, 1, 1)
        rc, p = plan(case(320, H, all_heads=0, masked=0, flags=flags(1, 1)))
        assert (p["p0_gz"], p["p0_gy"], p["p0_finish"], p["p0_image"], p["need_grad"]) == (parts, 1, 0, 0, 1)
    rc, p = plan(case(320, 128, all_heads=0, masked=0, flags=flags(3, 1)))
    assert (p["p0_code"], p["p0_gz"], p["p0_gy"], p["p0_finish"], p["need_grad"]) == (INFONCE, 1, 1, 1, 0)


def test_pass_sequences_and_combine_wiring(plan):
    """Spelled out, besides the table: logging -> pinned gradient, gradient -> logging, and what the combine kernel reads."""
    keys = ("npass", "qprep", "p0_role", "p0_code", "p0_buf", "p1_role", "p1_code", "p1_buf", "p1_pinned", "loss_buf",
            "lse_from_grad", "c_nsplit", "c_nsplit_loss", "need_grad", "values_only", "blocks")

    def ask(**kw):
        rc, p = plan(case(320, 256, flags=flags(3, 1), **kw))
        assert rc == OK and p["family"] == DMA
        return tuple(p[k] for k in keys)

    # unmasked InfoNCE, all heads: the logging pass (-2, part2, three splits on the image) first, its maxima pin the gradient
    assert ask(masked=0) == (2, 1, LOG, -2, 1, GRAD, HEAD_INFONCE_PINNED, 0, 1, 1, 1, 1, 3, 0, 1, 2)
    assert ask(masked=0, mode=CATALOG) == (2, 1, LOG, HEAD_LOG_UNMASKED_CATALOG, 1, GRAD, HEAD_INFONCE_PINNED, 0, 1, 1, 1,
                                           1, 3, 0, 1, 2)
    # masked: gradient (one split, finished in the kernel), then logging without the log-sum-exp into part2
    assert ask() == (2, 1, GRAD, HEAD_INFONCE_MASKED, 0, LOG, HEAD_LOG_MASKED, 1, 0, 1, 1, 1, 3, 0, 1, 2)
    assert ask(head=BPR) == (2, 1, GRAD, HEAD_BPR_MASKED, 0, LOG, HEAD_LOG_MASKED_LSE, 1, 0, 1, 0, 1, 3, 0, 1, 2)
    assert ask(sw=switches(logm256=False)) == (2, 1, GRAD, HEAD_INFONCE_MASKED, 0, LOG, -2, 1, 0, 1, 1, 1, 3, 0, 1, 2)
    assert ask(sw=switches(q_fp32=True))[:2] == (2, 0)
    # gradient only; AlignmentLoss: logging only, its gradient in the combine kernel; the deferred logging call
    assert ask(all_heads=0) == (1, 0, GRAD, HEAD_INFONCE_MASKED, 0, 0, 0, 0, 0, 0, 0, 1, 1, 0, 1, 2)
    assert ask(head=ALIGNMENT) == (1, 1, LOG, HEAD_LOG_MASKED_LSE, 0, 0, 0, 0, 0, 0, 0, 3, 3, 1, 0, 40)
    assert ask(all_heads=2, d_tok=False) == (1, 1, LOG, HEAD_LOG_MASKED, 0, 0, 0, 0, 0, 0, 0, 3, 3, 0, 1, 2)
    assert plan(case(320, 256, all_heads=2, d_tok=False))[1]["skip_train_head"] == 1
    assert plan(case(320, 256, all_heads=2))[1]["skip_train_head"] == 0
    # the generic family: one kernel in the gradient role (profile_grad goes around it), after the dump + select prologue
    # with hard negatives; dQ column parts only with a gradient
    for prec, fam, parts in ((BF16, GENERIC_BF16, 4), (F32, GENERIC_F32, 8)):
        rc, p = plan(case(320, 480, prec=prec, hard=4, all_heads=0))
        assert (rc, p["family"], p["hard"], p["npass"], p["p0_role"], p["p0_code"], p["p0_all"], p["p0_gz"]) == (
            OK, fam, 1, 1, GRAD, 512, 0, parts)
        rc, p = plan(case(320, 480, prec=prec, table_bf16=False, d_tok=False))
        assert (p["hard"], p["p0_all"], p["p0_gz"], p["values_only"]) == (0, 1, 1, 1)
    assert plan(case(320, 768, prec=F32))[0] == EUNSUPPORTED and plan(case(320, 1056))[0] == EUNSUPPORTED
    assert plan(case(320, 64, prec=2))[0] == EINVAL and plan(case(320, 100, prec=2))[0] == EINVAL


# ---------------------------------------------------------------------------------------------- environment reads
SWITCH_WORKER = r"""
report(lib.xf_loss_switches(), lib.xf_loss_switches())
"""


def _clean_env():
    return {k: v for k, v in os.environ.items() if not k.startswith("XFMR_LOSS_")}


@pytest.mark.parametrize("env,want", [
    ({}, switches()),
    ({"XFMR_LOSS_Q_FP32": ""}, switches()),
    ({"XFMR_LOSS_Q_FP32": "0"}, switches()),
    ({"XFMR_LOSS_Q_FP32": "1"}, switches(q_fp32=True)),
    ({"XFMR_LOSS_Q_FP32": "00"}, switches(q_fp32=True)),  # only the one-character "0" is off
    ({"XFMR_LOSS_LOGM256": "0"}, switches(logm256=False)),
    ({"XFMR_LOSS_LOGM256": "01"}, switches(logm256=False)),  # a leading '0'
    ({"XFMR_LOSS_LOGM256": ""}, switches()),
    ({"XFMR_LOSS_LOGM256": "1"}, switches()),
    ({"XFMR_LOSS_LOGM256": "off"}, switches()),
    ({"XFMR_LOSS_NSPLIT": "6", "XFMR_LOSS_NSPLIT_GRAD": "2"}, switches(nsplit=6, nsplit_grad=2)),
    ({"XFMR_LOSS_NSPLIT": "0", "XFMR_LOSS_NSPLIT_GRAD": "-3"}, switches()),  # atoi; <= 0: none
    ({"XFMR_LOSS_NSPLIT": "", "XFMR_LOSS_NSPLIT_GRAD": "x4"}, switches()),
    ({"XFMR_LOSS_NSPLIT": " 12abc", "XFMR_LOSS_NSPLIT_GRAD": "300"}, switches(nsplit=12, nsplit_grad=300)),
], ids=lambda v: "-".join(f"{k[10:]}={x}" for k, x in v.items()) or "unset" if isinstance(v, dict) else str(v))
def test_switches_as_the_library_reads_them(native, env, want):
    """A fresh process each (three of the four are read once per process); no GPU."""
    torch_imported, got = run_worker(SWITCH_WORKER, native.LIB_PATH, _clean_env() | env)
    assert torch_imported is False and got == [want] * 2


def test_three_switches_are_read_once_and_q_fp32_per_call(native):
    worker = SWITCH_WORKER.replace("report(", "first = lib.xf_loss_switches()\n"
                                   "os.environ.update(XFMR_LOSS_NSPLIT='5', XFMR_LOSS_NSPLIT_GRAD='2', "
                                   "XFMR_LOSS_LOGM256='0', XFMR_LOSS_Q_FP32='1')\nreport(first, ")
    torch_imported, got = run_worker(worker, native.LIB_PATH, _clean_env())
    assert torch_imported is False and got == [switches(), switches(q_fp32=True), switches(q_fp32=True)]


# ---------------------------------------------------------------------------------------------- the workspace carve
# (positions, H, n_rows, num_hard_negatives, XFMR_LOSS_NSPLIT flag) -> bytes, from d751a8e's library
WORKSPACES = (
    (102400, 128, 3884, 0, 0, 293700608),  # the benchmark's shape
    (1024, 384, 3884, 0, 0, 28119296),     # the reference's default model: 32 x 32 tokens at H = 384
    (320, 64, 201, 0, 0, 674048),
    (320, 64, 201, 0, 3, 428288),
    (320, 384, 201, 0, 1, 796928),
    (320, 64, 201, 4, 0, 1091328),
    (6400, 128, 3884, 0, 0, 34755840),
    (12800, 256, 1000001, 0, 0, 158680320),
    (32768, 256, 26745, 0, 0, 169584128),
    (7, 96, 50, 0, 0, 8448),
    (1024, 1024, 100, 0, 5, 23778816),
    (100, 32, 100000, 2, 7, 40608768),
    (50000, 384, 40, 0, 0, 290602752),
)


def test_workspace_totals_are_the_parents(native, lib):
    assert "XFMR_LOSS_NSPLIT" not in os.environ
    for T, H, n_rows, hard, ns, want in WORKSPACES:
        cfg = native.LossCfg()
        cfg.num_hard_negatives, cfg.flags = hard, flags(ns)
        assert lib.xfmr_sampled_loss_workspace_cfg(C.byref(cfg), T, H, n_rows) == want, (T, H, n_rows, hard, ns)
        for n_query, n_neg in ((T, T // 2), (T - T // 5, T)):  # the list form carves for the longer list
            assert lib.xfmr_sampled_loss_lists_workspace_cfg(C.byref(cfg), n_query, n_neg, H, n_rows) == want


# ---------------------------------------------------------------------------------------------- head codes reached
def gpu_forms_cases():
    """(test of tests/test_gpu_loss_dma_forms.py, key) of every LDS-DMA call that file makes."""
    import loss_cases as LC
    import test_gpu_loss_dma_forms as G
    from oracle.losses import LOSS_KINDS

    def key(T, H, group, head, all_heads, plan_, d_tok=True):
        cand, masked = G.CANDS[group]
        return case(T, H, n_rows=LC.V + 1, head=LOSS_KINDS.index(head), all_heads=int(all_heads), masked=int(masked),
                    mode=CATALOG if cand == "catalog" else SHARED, d_tok=d_tok, flags=flags(*plan_))

    for H in LC.WIDTHS:
        for group, head, all_heads, plan_ in itertools.product(G.CANDS, LOSS_KINDS, (True, False), G.PLANS):
            yield "all_heads_and_lean", key(LC.T, H, group, head, all_heads, plan_)
        heads = ("InfoNCELoss", "PairwiseHingeLoss", "PairwiseLogisticLoss", "AlignmentContrastiveLoss", "ContrastiveLoss")
        for group, head, all_heads, plan_ in itertools.product(("batch_masked", "batch_unmasked", "catalog_unmasked"), heads,
                                                               (True, False), ((1, 1), (3, 3))):
            yield "scale_and_margin", key(LC.T, H, group, head, all_heads, plan_)
        for group, plan_ in itertools.product(("batch_unmasked", "catalog_unmasked"), G.PLANS):
            yield "online_maximum", key(LC.T, H, group, "InfoNCELoss", False, plan_)
        for group, head, ns in itertools.product(G.CANDS, ("InfoNCELoss", "PairwiseLogisticLoss"), (1, 3)):
            yield "logging_only", key(LC.T, H, group, head, 2, (ns, ns), d_tok=False)
        c = LC.inputs(H)
        rows = max(int(c.qsel.sum()), int(c.mask.sum()))  # the list form: the longer of queries and negatives
        for group, head, all_heads, plan_ in itertools.product(
                ("batch_masked", "batch_unmasked"), ("InfoNCELoss", "AlignmentContrastiveLoss", "PairwiseHingeLoss"),
                (True, False), ((1, 1), (3, 3))):
            yield "lists", key(rows, H, group, head, all_heads, plan_)


def test_gpu_forms_file_reaches_the_codes_its_comments_name(plan):
    """Per width exactly the sets d751a8e's message lists: -1, -2, the six general heads and the five lean gradient codes
    at every width; the three fast logging codes at H <= 256 and none of them at H = 384."""
    reached, by_test = {}, {}
    for test, c in gpu_forms_cases():
        rc, p = plan(c)
        assert rc == OK and p["family"] == DMA, c
        codes = {p[f"p{i}_code"] for i in range(p["npass"])}
        reached.setdefault(c["H"], set()).update(codes)
        by_test.setdefault((test, c["H"]), set()).update(codes)
    everywhere = {-1, -2} | GENERAL_HEADS | LEAN_CODES
    assert reached == {64: everywhere | FAST_LOG_CODES, 128: everywhere | FAST_LOG_CODES,
                       256: everywhere | FAST_LOG_CODES, 384: everywhere}
    for H in DMA_WIDTHS:
        # the online maximum in 1 / 2 / 3 dQ column parts; the logging-only calls run logging codes alone
        assert by_test[("online_maximum", H)] == {INFONCE}
        assert by_test[("logging_only", H)] == ({-1, -2} | (FAST_LOG_CODES if H <= 256 else set()))


def test_gpu_forms_comments_per_candidate_group(plan):
    """The comment above CANDS in tests/test_gpu_loss_dma_forms.py, line by line, at its shape and plans."""
    import test_gpu_loss_dma_forms as G

    def codes(H, group, head, all_heads, plan_=(3, 3), d_tok=True):
        cand, masked = G.CANDS[group]
        rc, p = plan(case(320, H, head=head, all_heads=all_heads, masked=int(masked), d_tok=d_tok,
                          mode=CATALOG if cand == "catalog" else SHARED, flags=flags(*plan_)))
        assert rc == OK
        return [(p[f"p{i}_code"], p[f"p{i}_gz"]) for i in range(p["npass"])]

    for H in DMA_WIDTHS:
        fast = H <= 256
        # batch_masked: the lean epilogues; NCE and PairwiseHinge general; logging fast up to 256
        for head, code in ((CCL, HEAD_CCL_MASKED), (CONTRASTIVE, HEAD_CONTR_MASKED), (INFONCE, HEAD_INFONCE_MASKED),
                           (BPR, HEAD_BPR_MASKED), (NCE, NCE), (HINGE, HINGE)):
            log = (-2 if head == INFONCE else -1) if not fast else HEAD_LOG_MASKED if head == INFONCE else HEAD_LOG_MASKED_LSE
            assert codes(H, "batch_masked", head, 1) == [(code, 1), (log, 1)]
            assert codes(H, "batch_masked", head, 0) == [(code, 1)]
        assert codes(H, "batch_masked", ALIGNMENT, 1) == [(HEAD_LOG_MASKED_LSE if fast else -1, 1)]
        # batch_unmasked / catalog_unmasked: general codes; InfoNCE pinned after a -2 logging pass with all heads, the
        # online maximum in H / 128 parts without (one part up to 128); the catalogue's -2 is fast up to 256
        for group, log2 in (("batch_unmasked", -2), ("catalog_unmasked", HEAD_LOG_UNMASKED_CATALOG if fast else -2)):
            for head in (CCL, CONTRASTIVE, NCE, HINGE, BPR):
                assert codes(H, group, head, 1) == [(head, 1), (-1, 1)]
            parts = max(H // 128, 1)
            assert codes(H, group, INFONCE, 0) == [(INFONCE, parts)]
            if H > 128:
                assert codes(H, group, INFONCE, 1) == [(log2, 1), (HEAD_INFONCE_PINNED, 1)]
                assert codes(H, group, INFONCE, 0, (3, 1)) == [(INFONCE, parts)]
        # (up to 128 the condition is the same: all heads pins, lean walks the online maximum in one part)
        assert codes(H, "batch_unmasked", INFONCE, 1)[1][0] == HEAD_INFONCE_PINNED
        # catalog_masked: InfoNCE lean, every other head and the logging passes general
        assert codes(H, "catalog_masked", INFONCE, 1) == [(HEAD_INFONCE_MASKED, 1), (-2, 1)]
        for head in (CCL, CONTRASTIVE, BPR):
            assert codes(H, "catalog_masked", head, 1) == [(head, 1), (-1, 1)]
        # logging only (all_heads = 2, no gradient): -2 when the train head is InfoNCE, -1 otherwise
        assert codes(H, "batch_unmasked", INFONCE, 2, d_tok=False) == [(-2, 1)]
        assert codes(H, "batch_unmasked", BPR, 2, d_tok=False) == [(-1, 1)]


def test_plan_entry_is_internal(native):
    header = (ROOT / "include" / "xfmr_hip.h").read_text()
    for name in ("xf_loss_plan", "xf_loss_switches"):
        assert name not in header and name not in native.EXPORTED_SYMBOLS
    assert re.search(r"#define\s+XFMR_ABI_VERSION\s+3\b", header) and native.ABI_VERSION == 3
