"""Every attention form of csrc/attention.hip under key masks that are not a prefix (tests/attn_mask_cases.py: left padding
of one key / a tile / a chunk, a masked interior tile, Bernoulli and alternating holes, one / two / no visible keys), against
the fp64 reference through attn_mask_cases.check -- per sequence, per gradient slice, finite on padding rows, ctx exactly 0
and lse +inf on rows without keys. As in test_gpu_attn_forms.py the library is asked which forms the call takes
(xf_attn_plan), they are asserted, and the same call then runs. One launch covers the table: B = 13 sequences (the grid
pads to sixteen), two heads. tests/test_attn_mask_cases_host.py shows on the CPU what the table catches and that the bf16
rounding model stays within a third of each limit on these very shapes."""

import pytest
import torch

import attn_mask_cases as MC
from test_attn_plan_host import (BF16, BF16_FUSED, BF16_PANEL, BF16_ROLES4, BF16_ROLES8, BF16_SEQ, BF16_STREAM, F32,
                                 GENERIC_PANEL, GENERIC_STREAM)
from test_gpu_attn_forms import forms  # noqa: F401  (the fixture that asks xf_attn_plan)

pytestmark = pytest.mark.gpu
DEV = "cuda"
A = 2
B = len(MC.NAMES)


@pytest.fixture(scope="module")
def ops():
    from xfmr_rec_amd import ops as _ops

    return _ops


def _run(ops, tag, prec, dh, L, chunk, causal, stream_keys=False):
    name = "bf16" if prec == BF16 else "fp32"
    c = MC.case(L, A, dh, chunk, causal)
    kw = dict(precision=name, causal=causal, stream_keys=stream_keys)
    qkv, mask, w = c.qkv.to(DEV), c.mask.to(DEV), c.w.to(DEV)
    ctx, lse = ops.attn_fwd(qkv, mask, A, **kw)
    d_qkv = ops.attn_bwd(qkv, mask, ctx, lse, w, A, **kw)
    figs = None
    try:
        figs = MC.check(tag, name, ctx, d_qkv, c, lse=lse)
    finally:
        if figs is None:  # the figures of a failing case: measured without the assertions' limits
            _report(tag, name, ctx, d_qkv, c)
    print(MC.fig_line(f"{tag} {name} dh={dh} L={L} causal={causal}", figs))
    assert float(d_qkv.abs().sum()) > 0


def _report(tag, name, ctx, d_qkv, c):
    ctx, d = ctx.double().cpu(), d_qkv.double().cpu()
    H = c.ref_ctx.shape[-1]
    for b, seq in enumerate(c.names):
        v = c.mask[b].bool()
        e = ((ctx[b][v] - c.ref_ctx[b][v]).abs() / c.ref_ctx[b][v].abs().clamp(min=1.0)).max().item() if v.any() else 0.0
        den = c.ref_grad[b].norm().item() or 1.0
        g = [((d[b, :, i * H:(i + 1) * H] - c.ref_grad[b, :, i * H:(i + 1) * H]).norm().item() / den) for i in range(3)]
        print(f"FIG attn-masks {tag} {name} {seq}: ctx {e:.2e} dq {g[0]:.2e} dk {g[1]:.2e} dv {g[2]:.2e} "
              f"nonfinite ctx rows {int((~torch.isfinite(ctx[b]).all(-1)).sum())} d_qkv rows {int((~torch.isfinite(d[b]).all(-1)).sum())}")


def test_one_workgroup_forward_and_fused_backward(ops, forms, monkeypatch):
    """L = 130: five tiles, the last of two rows."""
    monkeypatch.delenv("XFMR_ATTN_BWD_FORM", raising=False)
    assert forms(BF16, 32, B, 130) == (BF16_SEQ, BF16_FUSED)
    _run(ops, "seq+fused", BF16, 32, 130, 128, True)


def test_roles_backward_four_waves(ops, forms, monkeypatch):
    monkeypatch.setenv("XFMR_ATTN_BWD_FORM", "roles")
    assert forms(BF16, 32, B, 130) == (BF16_SEQ, BF16_ROLES4)
    _run(ops, "seq+roles4", BF16, 32, 130, 128, True)


def test_roles_backward_eight_waves(ops, forms, monkeypatch):
    """L = 290: ten tiles, the four-tiles-per-wave deal."""
    monkeypatch.delenv("XFMR_ATTN_BWD_FORM", raising=False)
    assert forms(BF16, 32, B, 290) == (BF16_SEQ, BF16_ROLES8)
    _run(ops, "seq+roles8", BF16, 32, 290, 256, True)


def test_bf16_panel_pair(ops, forms):
    assert forms(BF16, 32, B, 130, causal=False) == (BF16_PANEL, BF16_PANEL)
    _run(ops, "panel", BF16, 32, 130, 128, False)


@pytest.mark.parametrize("causal", [True, False], ids=["causal", "bidirectional"])
def test_bf16_streaming_pair(ops, forms, causal):
    """L = 290: chunks of 256 + 34 keys; `left_chunk` empties the first."""
    assert forms(BF16, 32, B, 290, causal=causal, stream_keys=True) == (BF16_STREAM, BF16_STREAM)
    _run(ops, "stream", BF16, 32, 290, 256, causal, stream_keys=True)


@pytest.mark.parametrize("causal", [True, False], ids=["causal", "bidirectional"])
@pytest.mark.parametrize("prec,dh", [(F32, 32), (BF16, 64)], ids=["fp32-h32", "bf16-h64"])
@pytest.mark.parametrize("stream_keys", [False, True], ids=["panel", "streaming"])
def test_generic_panel_and_streaming(ops, forms, prec, dh, stream_keys, causal):
    """L = 162: query blocks / key chunks of 128 + 34."""
    form = GENERIC_STREAM if stream_keys else GENERIC_PANEL
    assert forms(prec, dh, B, 162, causal=causal, stream_keys=stream_keys) == (form, form)
    _run(ops, "generic-stream" if stream_keys else "generic-panel", prec, dh, 162, 128, causal, stream_keys=stream_keys)


def test_dropout_on_rows_without_keys_stay_zero_and_runs_repeat(ops, forms, monkeypatch):
    """dropout_p = 0.2 through BF16_SEQ / BF16_FUSED at L = 130: the empty-row paths with the keep scale multiplied in.
    (Values under dropout are held to the host mask model in test_gpu_dropout_reference.py.)"""
    monkeypatch.delenv("XFMR_ATTN_BWD_FORM", raising=False)
    assert forms(BF16, 32, B, 130) == (BF16_SEQ, BF16_FUSED)
    c = MC.case(130, A, 32, 128, True)
    kw = dict(precision="bf16", causal=True, dropout_p=0.2, seed=6018027440424182934, site=3)
    qkv, mask, w = c.qkv.to(DEV), c.mask.to(DEV), c.w.to(DEV)
    runs = []
    for _ in range(2):
        ctx, lse = ops.attn_fwd(qkv, mask, A, **kw)
        runs.append((ctx, lse, ops.attn_bwd(qkv, mask, ctx, lse, w, A, **kw)))
    for name, a, b in zip(("ctx", "lse", "d_qkv"), *runs):
        assert torch.equal(a, b), name
    ctx, lse, d_qkv = (t.cpu() for t in runs[0])
    assert bool(torch.isfinite(ctx).all()) and bool(torch.isfinite(d_qkv).all())
    blind = ~c.sees
    assert bool((ctx[blind] == 0).all())
    assert bool((lse.transpose(1, 2)[blind] == float("inf")).all()) and bool(torch.isfinite(lse.transpose(1, 2)[c.sees]).all())
    none = MC.NAMES.index("none")
    assert bool((d_qkv[none] == 0).all()) and float(d_qkv.abs().sum()) > 0
    # dropout changed something: the run is not the dropout-free one
    ctx0, _ = ops.attn_fwd(qkv, mask, A, precision="bf16", causal=True)
    assert not torch.equal(ctx0.cpu(), ctx)
    print(f"FIG attn-masks dropout seq+fused L=130: bit-equal runs, {int(blind.sum())} rows without keys exactly 0")
