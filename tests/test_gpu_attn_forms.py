"""One case per form id of attention's plan (csrc/attention.hip: AttnForm; tests/test_attn_plan_host.py has the rules): the
library is asked which form a call takes (xf_attn_plan, with the switches as the library reads them), the expected form is
asserted, and the same call then runs and is compared with the fp64 reference at the existing attention tests' tolerances --
so "the plan names form X" and "form X ran and is right" are asserted together. Smallest shapes at which each form can go
wrong: two sequences (nine where the grid pads the batch to eight), two heads, a ragged key mask with holes, one sequence
shorter than a 32-row tile, L one past a tile / a chunk boundary."""

import ctypes as C

import pytest
import torch

from helpers import assert_close
from test_attn_plan_host import (BF16, BF16_FUSED, BF16_PANEL, BF16_ROLES4, BF16_ROLES8, BF16_SEQ, BF16_STREAM, F32, FIELDS,
                                 GENERIC_PANEL, GENERIC_STREAM, OK)
from test_gpu_attn_long_bf16 import _attention_reference, _inputs
from test_gpu_model import _encoder_shape_vs_oracle

pytestmark = pytest.mark.gpu
DEV = "cuda"
A = 2


@pytest.fixture(scope="module")
def ops():
    from xfmr_rec_amd import ops as _ops

    return _ops


@pytest.fixture(scope="module")
def X():
    import xfmr_rec_amd as x

    return x


@pytest.fixture(scope="module")
def forms():
    """(forward form, backward form) of a call, under the switches the library reads from the environment right now."""
    from xfmr_rec_amd import _native as N

    lib = N.load()

    def ask(prec, dh, B, L, *, causal=True, stream_keys=False, packed=False, s16=False):
        got = []
        for bwd in (0, 1):
            out = (C.c_int32 * 8)()
            rc = lib.xf_attn_plan(bwd, prec, int(s16), B, L, A, A * dh, int(causal), int(packed), int(stream_keys),
                                  lib.xf_attn_switches(), out)
            assert rc == OK
            got.append(dict(zip(FIELDS, out))["form"])
        return tuple(got)

    return ask


def _run_vs_fp64(ops, prec, dh, B, L, lengths, causal=True, stream_keys=False):
    name = "bf16" if prec == BF16 else "fp32"
    qkv, mask, w = _inputs(B, L, A, dh, lengths)
    ref_in = qkv.clone().double().requires_grad_(True)
    ref = _attention_reference(ref_in, mask, A, causal)
    (ref * w.double()).sum().backward()
    kw = dict(precision=name, causal=causal, stream_keys=stream_keys)
    ctx, lse = ops.attn_fwd(qkv.to(DEV), mask.to(DEV), A, **kw)
    valid = mask.bool()
    assert_close("attn.ctx", ctx.cpu()[valid], ref.detach()[valid], name)
    d_qkv = ops.attn_bwd(qkv.to(DEV), mask.to(DEV), ctx, lse, w.to(DEV), A, **kw)
    assert float(d_qkv.abs().sum()) > 0
    assert_close("attn.d_qkv", d_qkv, ref_in.grad, name, "grad")


def test_one_workgroup_forward_and_fused_backward(ops, forms, monkeypatch):
    monkeypatch.delenv("XFMR_ATTN_BWD_FORM", raising=False)
    assert forms(BF16, 32, 2, 33) == (BF16_SEQ, BF16_FUSED)
    _run_vs_fp64(ops, BF16, 32, 2, 33, [33, 20])


def test_roles_backward_four_waves(ops, forms, monkeypatch):
    monkeypatch.setenv("XFMR_ATTN_BWD_FORM", "roles")
    assert forms(BF16, 32, 2, 33) == (BF16_SEQ, BF16_ROLES4)
    _run_vs_fp64(ops, BF16, 32, 2, 33, [33, 20])


def test_roles_backward_eight_waves(ops, forms, monkeypatch):
    monkeypatch.delenv("XFMR_ATTN_BWD_FORM", raising=False)  # (above 256 rows whatever the switch says)
    assert forms(BF16, 32, 2, 257) == (BF16_SEQ, BF16_ROLES8)
    _run_vs_fp64(ops, BF16, 32, 2, 257, [257, 20])


def test_bf16_panel_pair(ops, forms):
    """Bidirectional: no one-workgroup form; nine sequences on a grid padded to sixteen."""
    assert forms(BF16, 32, 9, 33, causal=False) == (BF16_PANEL, BF16_PANEL)
    _run_vs_fp64(ops, BF16, 32, 9, 33, [33, 20, 1, 32, 31, 7, 33, 2, 25], causal=False)


def test_bf16_streaming_pair_padded(ops, forms):
    """XFMR_ATTN_STREAM_KEYS at L = 257: two chunks of 256 rows, the second of one row."""
    assert forms(BF16, 32, 2, 257, stream_keys=True) == (BF16_STREAM, BF16_STREAM)
    _run_vs_fp64(ops, BF16, 32, 2, 257, [257, 20], stream_keys=True)


def test_bf16_streaming_pair_packed(X, forms, monkeypatch):
    """Packed rows beyond 512 per sequence, through the encoder (bf16 storage) as tests/test_gpu_packed_long.py runs it,
    against the oracle under the host model's dropout masks (the helper's tolerances)."""
    assert forms(BF16, 32, 2, 513, packed=True, s16=True) == (BF16_STREAM, BF16_STREAM)
    _encoder_shape_vs_oracle(X, "bf16", B=2, L=513, H=32 * A, A=A, I=128, nL=1, V=300, lengths=[513, 20],
                             dropout=monkeypatch, packed=True)


@pytest.mark.parametrize("prec,dh", [(F32, 32), (BF16, 64)], ids=["fp32-h32", "bf16-h64"])
@pytest.mark.parametrize("stream_keys", [False, True], ids=["panel", "streaming"])
def test_generic_panel_and_streaming(ops, forms, prec, dh, stream_keys):
    """L = 129: two 128-row blocks, and two chunks of 128 rows when streaming."""
    form = GENERIC_STREAM if stream_keys else GENERIC_PANEL
    assert forms(prec, dh, 2, 129, stream_keys=stream_keys) == (form, form)
    _run_vs_fp64(ops, prec, dh, 2, 129, [129, 20], stream_keys=stream_keys)
