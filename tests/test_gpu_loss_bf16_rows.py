"""Query rows as bf16, converted once per call (csrc/loss_dma.inc: loss_qprep_kernel, LossArgs::qimg).

A loss launch with n > 1 column splits used to read and round every fp32 query row -- and gather and multiply its
positive's row -- once per split. It now stages the rows from a bf16 image that one small kernel writes per call into the
loss workspace, together with |q|^2 and the positive's dot product. The image holds the SAME rounding of the same fp32
pieces and the two per-query numbers are taken with the same arithmetic, so nothing may change: every loss, every
statistic and dL/dtok are compared with ``torch.equal`` against the old behaviour, which XFMR_LOSS_Q_FP32=1 (read per
call) keeps. No tolerance anywhere in this file.

Shapes: the headline loss shape (T = 102 400 queries = 800 query blocks, V = 3 883, H = 128) under the library's own plan
(logging pass: 4 splits on the image; gradient pass: one split, which reads the fp32 rows itself) and under a forced plan
that puts the gradient pass on the image too (3 splits); and one packed-rows case (MovieLens-like lengths, only the
valid rows, ``padded_positions`` = B x L as the training step passes it).
"""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

HEADS = ["AlignmentLoss", "AlignmentContrastiveLoss", "ContrastiveLoss", "InfoNCELoss", "NCELoss", "PairwiseHingeLoss",
         "PairwiseLogisticLoss"]
H, V, B, L = 128, 3883, 512, 200
SWITCH = "XFMR_LOSS_Q_FP32"


@pytest.fixture(scope="module")
def ops():
    from xfmr_rec_amd import ops as _ops

    return _ops


def _inputs(lengths: str, seed=61):
    g = torch.Generator().manual_seed(seed)
    table = torch.randn(V + 1, H, generator=g)
    table = table / table.norm(dim=-1, keepdim=True)
    table[0] = 0
    tok = torch.randn(B * L, H, generator=g)
    if lengths == "dense":
        lens = torch.full((B,), L)
    else:  # MovieLens-like: len = clip(round(exp(N(4.35, 1))), 16, L)
        lens = torch.exp(4.35 + torch.randn(B, generator=g)).round().clamp(16, L).long()
    mask = (torch.arange(L)[None, :] < lens[:, None]).reshape(-1)
    pos = torch.randint(1, V + 1, (B * L,), generator=g)
    neg = torch.randint(1, V + 1, (B * L,), generator=g)
    pos[torch.rand(B * L, generator=g) < 0.01] = 0  # valid positions whose positive is padding
    pos[~mask] = 0
    neg[~mask] = 0
    return table, tok, mask, pos, neg


class _fp32_rows:
    """The old behaviour for the calls inside the block (the library reads the switch on every call)."""

    def __enter__(self):
        self.old = os.environ.get(SWITCH)
        os.environ[SWITCH] = "1"

    def __exit__(self, *exc):
        if self.old is None:
            os.environ.pop(SWITCH, None)
        else:
            os.environ[SWITCH] = self.old


def _same(a, b, what):
    (l0, s0, d0), (l1, s1, d1) = a, b
    assert torch.equal(l0, l1), (what, "losses", l0.tolist(), l1.tolist())
    # (NaN == NaN here: a train-head-only statistic a lean epilogue does not count is NaN in both forms)
    assert torch.equal(torch.nan_to_num(s0, nan=-12345.0), torch.nan_to_num(s1, nan=-12345.0)), (what, "stats")
    assert torch.equal(torch.isnan(s0), torch.isnan(s1)), (what, "stats NaN pattern")
    assert d0 is not None and d1 is not None and torch.equal(d0, d1), (what, "dL/dtok", float((d0 - d1).abs().max()))


def _run_all_heads(ops, tok, mask, pos, neg, table, plan, padded=0):
    dev = "cuda:0"
    table, tok, mask, pos, neg = (t.to(dev) for t in (table, tok, mask, pos, neg))
    rn, tb = ops.table_prepare(table)
    assert os.environ.get(SWITCH, "") in ("", "0")
    for head in HEADS:
        kw = dict(train_head=head, all_heads=True, precision="bf16", table_bf16=tb, need_grad=True,
                  padded_positions=padded, **plan)
        new = ops.sampled_loss(tok, mask, pos, neg, table, rn, **kw)
        again = ops.sampled_loss(tok, mask, pos, neg, table, rn, **kw)
        with _fp32_rows():
            old = ops.sampled_loss(tok, mask, pos, neg, table, rn, **kw)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(new[0]).all()) and bool(torch.isfinite(new[2]).all()), head
        _same(new, again, (head, plan, "two runs of the image path"))
        _same(new, old, (head, plan, "image path against the fp32 rows"))


@pytest.mark.parametrize("plan", [dict(), dict(nsplit=5, nsplit_grad=3)], ids=["library_plan", "grad_3_splits"])
def test_headline_shape_image_path_equals_fp32_rows_bit_for_bit(ops, plan):
    table, tok, mask, pos, neg = _inputs("dense")
    _run_all_heads(ops, tok, mask, pos, neg, table, plan)


def test_packed_rows_image_path_equals_fp32_rows_bit_for_bit(ops):
    table, tok, mask, pos, neg = _inputs("ragged", seed=62)
    keep = mask.clone()
    tok, pos, neg = tok[keep].contiguous(), pos[keep].contiguous(), neg[keep].contiguous()
    assert 0 < tok.shape[0] < 0.97 * B * L
    mask = torch.ones(tok.shape[0], dtype=torch.bool)
    _run_all_heads(ops, tok, mask, pos, neg, table, dict(), padded=B * L)
    _run_all_heads(ops, tok, mask, pos, neg, table, dict(nsplit=4, nsplit_grad=2), padded=B * L)


def test_the_switch_selects_the_path_and_the_image_lives_in_the_workspace(ops):
    """The image and its per-query records are the LAST two regions of the caller's workspace (no allocation inside the
    call): written by a call on the image path, left untouched by one under the switch."""
    dev = "cuda:0"
    table, tok, mask, pos, neg = (t.to(dev) for t in _inputs("dense"))
    rn, tb = ops.table_prepare(table)
    T = tok.shape[0]
    kw = dict(train_head="InfoNCELoss", all_heads=2, precision="bf16", table_bf16=tb)
    up = lambda n: (n + 255) // 256 * 256
    tail = up(T * H * 2) + up(T * 8)
    for fp32 in (True, False):
        ws = ops.sampled_loss_workspace(tok, T, H, table.shape[0], **kw)
        assert ws.numel() > tail
        ws.zero_()
        if fp32:
            with _fp32_rows():
                ops.sampled_loss(tok, mask, pos, neg, table, rn, need_grad=False, workspace=ws, **kw)
        else:
            ops.sampled_loss(tok, mask, pos, neg, table, rn, need_grad=False, workspace=ws, **kw)
        torch.cuda.synchronize()
        region = ws.view(torch.uint8)[-tail:]
        assert bool(region.any()) == (not fp32), fp32
        if not fp32:  # row qi of the image is the bf16 rounding of the qi-th query's fp32 row (here: every row with pos != 0)
            img = region[: T * H * 2].view(torch.bfloat16).view(T, H)
            q = tok[(mask & (pos != 0))]
            assert torch.equal(img[: q.shape[0]], q.to(torch.bfloat16))
