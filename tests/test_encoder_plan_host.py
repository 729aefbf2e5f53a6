"""CPU-side test (no GPU) of the encoder's plan (csrc/encoder.hip: EncPlan / make_plan, read through the internal entry point
xf_encoder_plan): which form every part of a training step takes is ONE function of the configuration and of three
environment variables. The rules are written here a second time, in Python, and a decision table is walked through the library
on both sides of every boundary. The workspace size of a dozen configurations is pinned to the values of the commit before the
plan existed: the carve's total must not move unless a change means to resize the workspace (which then updates the literals)."""

import itertools
import json
import os
import pathlib
import re

import pytest

from abi_worker import run_worker

ROOT = pathlib.Path(__file__).resolve().parents[1]
F32, BF16 = 0, 1
BIDIRECTIONAL, LN_UNFUSED, FFN_UNFUSED, FFN_BWD_UNFUSED, DW_INLINE, DW_SIDE_ANY, DW_UNPAIRED, REDUCE_HALF_EARLY = (
    1 << b for b in range(8))
FIELDS = ("Tplan", "T", "mix", "causal", "fuse_ln", "fuse_ffn", "rederive", "fuse_ffn_bwd", "dw_buffers_per_layer", "dw_side",
          "group_dw", "lin_copy", "half_layer")
ENV_NAMES = ("XFMR_ACT_FP32", "XFMR_LN_STORE_X", "XFMR_LN_FUSED_MIN_TOKENS")
EUNSUPPORTED = -2
HANDLE = 0x1000  # a dummy non-null handle / device pointer: the plan only asks whether it is null


def rules(c, env):
    """The plan of configuration c under the environment env: the table of the encoder's forms, independent of the C++."""
    def on(name):  # the library's reading of a switch: set, not empty, not starting with '0'
        return bool(env.get(name)) and env[name][0] != "0"

    f = c["flags"]
    p = {}
    p["Tplan"] = c["batch"] * c["seq_len"]
    p["T"] = c["packed_rows"] if c["packed_rows"] else p["Tplan"]
    p["mix"] = c["precision"] == BF16 and not on("XFMR_ACT_FP32")
    p["causal"] = not f & BIDIRECTIONAL
    min_tokens = int(env.get("XFMR_LN_FUSED_MIN_TOKENS", 12288))
    p["fuse_ln"] = p["mix"] and c["hidden"] == 128 and p["Tplan"] >= min_tokens and not f & LN_UNFUSED
    p["fuse_ffn"] = (p["fuse_ln"] and p["Tplan"] >= 16384 and c["inter"] % 128 == 0 and c["inter"] <= 1024
                     and not f & FFN_UNFUSED)
    p["rederive"] = p["fuse_ln"] and not on("XFMR_LN_STORE_X")
    p["fuse_ffn_bwd"] = p["fuse_ffn"] and p["fuse_ln"] and not f & FFN_BWD_UNFUSED
    side_any = bool(f & DW_SIDE_ANY)
    p["dw_buffers_per_layer"] = (p["mix"] and c["layers"] <= 64 and (side_any or (c["hidden"] == 128 and p["Tplan"] >= 40960))
                                 and c["context"] and not f & DW_INLINE)
    p["dw_side"] = p["dw_buffers_per_layer"] and (side_any or p["T"] >= 40960 or not c["packed_rows"])
    p["group_dw"] = not f & DW_UNPAIRED and not p["dw_side"] and p["mix"]
    p["lin_copy"] = c["hidden_dropout"] > 0 or p["mix"]
    p["half_layer"] = c["layers"] // 2 if (c["grads_half_event"] or f & REDUCE_HALF_EARLY) and c["layers"] >= 2 else -1
    return {k: int(v) for k, v in p.items()}


def cfg(batch, seq_len, hidden=128, inter=512, layers=2, precision=BF16, flags=0, context=False, grads_half_event=False,
        packed_rows=0, hidden_dropout=0.0):
    return dict(batch=batch, seq_len=seq_len, hidden=hidden, heads=hidden // 32, inter=inter, layers=layers, max_pos=seq_len,
                precision=precision, flags=flags, context=context, grads_half_event=grads_half_event, packed_rows=packed_rows,
                hidden_dropout=hidden_dropout)


def decision_table():
    t = []
    # batch x seq_len on both sides of every token threshold (12 288, 16 384, 40 960) and of the XFMR_LN_FUSED_MIN_TOKENS the
    # environment case sets (20 000); hidden 128 against 64 and 256; inter a multiple of 128, not one, and above 1024
    shapes = [dict(batch=b, seq_len=s) for b, s in ((4, 24), (11, 1117), (64, 192), (129, 127), (128, 128), (99, 200),
                                                    (100, 200), (111, 369), (160, 256))]
    shapes += [dict(batch=160, seq_len=256, hidden=h) for h in (64, 256)]
    shapes += [dict(batch=128, seq_len=128, inter=i) for i in (192, 1152)]
    flagsets = [0] + [1 << b for b in range(8)] + [DW_SIDE_ANY | DW_INLINE, LN_UNFUSED | DW_UNPAIRED]
    for s, prec, f, ctx in itertools.product(shapes, (BF16, F32), flagsets, (False, True)):
        t.append(cfg(**s, precision=prec, flags=f, context=ctx))
    # the early upper-half reduction: by event or by flag, for every layer count around its rules and around the 64 layers
    # the per-layer gradient buffers stop at
    for layers, half, f, s in itertools.product((1, 2, 3, 64, 65), (False, True), (0, REDUCE_HALF_EARLY, DW_SIDE_ANY),
                                                ((4, 24), (160, 256))):
        t.append(cfg(*s, layers=layers, grads_half_event=half, flags=f, context=True))
    # packed rows: the buffers follow the padded size, the side stream the rows actually run
    for (b, s), rows, f, ctx in itertools.product(((256, 200), (100, 200)), (19999, 40959, 40960), (0, DW_SIDE_ANY, DW_INLINE),
                                                  (False, True)):
        if rows <= b * s:
            t.append(cfg(b, s, packed_rows=rows, flags=f, context=ctx))
    # d_lin is a copy of its own with dropout or bf16 storage
    for prec, drop in itertools.product((BF16, F32), (0.0, 0.1)):
        t.append(cfg(4, 24, precision=prec, hidden_dropout=drop))
    return t


TABLE = decision_table()

WORKER = r"""
res = []
for raw in json.load(sys.stdin):
    cfg, out = abi.EncoderCfg.from_buffer_copy(bytes.fromhex(raw)), (C.c_int32 * 16)()
    rc = lib.xf_encoder_plan(C.byref(cfg), out)
    res.append([rc, list(out), lib.xfmr_encoder_workspace_bytes(C.byref(cfg))])
report(res)
"""


@pytest.fixture(scope="module")
def native():
    from xfmr_rec_amd import _native as N

    if not N.LIB_PATH.exists():
        pytest.fail(f"{N.LIB_PATH} missing: run build() first")
    return N


def run_table(native, table, env):
    """[(rc, plan fields, workspace bytes)] of every configuration, from a fresh process whose environment has exactly the
    switches of env (two of the three are read once per process)."""
    raw = []
    for c in table:
        s = native.EncoderCfg(**{k: v for k, v in c.items() if k not in ("context", "grads_half_event", "packed_rows")},
                              ln_eps=1e-12, context=HANDLE if c["context"] else None,
                              grads_half_event=HANDLE if c["grads_half_event"] else None,
                              seq_offsets=HANDLE if c["packed_rows"] else None, row_pos=HANDLE if c["packed_rows"] else None,
                              packed_rows=c["packed_rows"])
        raw.append(bytes(s).hex())
    clean = {k: v for k, v in os.environ.items() if k not in ENV_NAMES}
    torch_imported, (res,) = run_worker(WORKER, native.LIB_PATH, clean | env, json.dumps(raw))
    assert torch_imported is False
    return [(rc, dict(zip(FIELDS, out)), out[len(FIELDS):], nbytes) for rc, out, nbytes in res]


@pytest.mark.parametrize("env", [{}, {"XFMR_ACT_FP32": "1"}, {"XFMR_ACT_FP32": "0"}, {"XFMR_LN_STORE_X": "1"},
                                 {"XFMR_LN_STORE_X": "0"}, {"XFMR_LN_FUSED_MIN_TOKENS": "20000"}],
                         ids=lambda e: "-".join(f"{k}={v}" for k, v in e.items()) or "default")
def test_plan_follows_the_rules(native, env):
    got = run_table(native, TABLE, env)
    assert len(got) == len(TABLE) > 500
    seen = {k: set() for k in FIELDS}
    for c, (rc, plan, rest, nbytes) in zip(TABLE, got):
        want = rules(c, env)
        if c["packed_rows"] and not want["mix"]:  # the packed layout needs bf16 storage (check_cfg)
            assert rc == EUNSUPPORTED and nbytes == 0, (c, rc)
            continue
        assert rc == 0 and nbytes > 0, (c, rc)
        assert plan == want, (c, env, {k: (plan[k], want[k]) for k in FIELDS if plan[k] != want[k]})
        assert rest == [0] * (16 - len(FIELDS))
        for k in FIELDS:
            seen[k].add(want[k])
    # the table reaches both values of every decision (under XFMR_ACT_FP32=1 nothing is fused, by the rules above)
    fp32_only = env.get("XFMR_ACT_FP32") == "1"
    for k in FIELDS[2:]:
        if fp32_only and k in ("mix", "fuse_ln", "fuse_ffn", "rederive", "fuse_ffn_bwd", "dw_buffers_per_layer", "dw_side",
                               "group_dw"):
            assert seen[k] == {0}, (k, seen[k])
        elif env.get("XFMR_LN_STORE_X") == "1" and k == "rederive":
            assert seen[k] == {0}
        else:
            assert len(seen[k]) >= 2, (k, seen[k])


def test_plan_checks_the_configuration_and_is_internal(native):
    bad = dict(cfg(4, 24), heads=3)  # head size 128 / 3: check_cfg refuses it before any plan is made
    (rc, _, _, nbytes), = run_table(native, [bad], {})
    assert rc == EUNSUPPORTED and nbytes == 0
    header = (ROOT / "include" / "xfmr_hip.h").read_text()
    assert "xf_encoder_plan" not in header and "xf_encoder_plan" not in native.EXPORTED_SYMBOLS
    assert re.search(r"#define\s+XFMR_ABI_VERSION\s+3\b", header) and native.ABI_VERSION == 3


# xfmr_encoder_workspace_bytes at commit 90601cd (the parent of the plan / carve-once change), default environment
WORKSPACE_BYTES = [
    (cfg(4, 24, hidden=64, inter=128), 1841920),
    (cfg(4, 24, hidden=64, inter=128, precision=F32), 1950208),
    (cfg(62, 200), 338798592),
    (cfg(82, 200, layers=1), 250503168),
    (cfg(82, 200, layers=3, context=True), 563037184),
    (cfg(205, 200, context=True), 920598016),                      # per-layer gradient buffers
    (cfg(205, 200, context=True, flags=DW_INLINE), 815638016),
    (cfg(205, 200, layers=1, context=True), 522209792),
    (cfg(205, 200, precision=F32, context=True), 1129672704),
    (cfg(256, 200, packed_rows=25000, context=True), 1109337600),  # packed: sized for batch x seq_len
    (cfg(4, 24, layers=64, context=True, flags=DW_SIDE_ANY), 188690432),
    (cfg(4, 24, layers=65, context=True, flags=DW_SIDE_ANY), 177449728),
    (cfg(160, 256, hidden=256, inter=1024, layers=4, context=True), 2561110016),
]


def test_workspace_bytes_are_the_parent_commits(native):
    got = run_table(native, [c for c, _ in WORKSPACE_BYTES], {})
    assert [nbytes for _, _, _, nbytes in got] == [want for _, want in WORKSPACE_BYTES]
