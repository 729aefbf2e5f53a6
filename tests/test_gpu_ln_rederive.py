"""Under the LayerNorm-fused forms the encoder forward does not store the fp32 LayerNorm outputs x0 / x1 / x2 (of every layer
but the last): their one reader, the residual operand of the next kernel's epilogue, re-derives them from pre / mean / rstd /
gamma / beta (layer 0: and regenerates the embedding dropout). XFMR_LN_STORE_X=1 (read per call) restores the stores and the
loaded residual. Both modes must give the same bits: the encoder output and the whole flat gradient buffer.

Shapes: H 128, 4 heads, I 512, bf16. T = 82 x 200 = 16 400 is the fused FFN at its threshold (256 full 64-row tiles + a 16-row
tail); T = 62 x 200 = 12 400 the LayerNorm-fused GEMMs with the FFN as separate GEMMs (48-row tail). Two layers: x2 of layer 0
is layer 1's residual, and layer 0 takes the embedding dropout."""

import ctypes

import pytest
import torch

from helpers import unit_table

pytestmark = pytest.mark.gpu
DEV = "cuda"
H, A, I, L, V = 128, 4, 512, 200, 300


@pytest.fixture(scope="module")
def ops():
    from xfmr_rec_amd import ops as o

    return o


def _inputs(ops, B, nL, drop, lengths=None, seed=7):
    from xfmr_rec_amd import _native as N

    g = torch.Generator().manual_seed(seed)
    idx = torch.randint(1, V + 1, (B, L), generator=g)
    if lengths is not None:
        idx = idx * (torch.arange(L)[None, :] < torch.tensor(lengths)[:, None])
    idx = idx.to(DEV)
    kw = dict(batch=B, seq_len=L, hidden=H, heads=A, inter=I, layers=nL, max_pos=L, precision="bf16",
              hidden_dropout=drop, attn_dropout=drop, seed=1234)
    keep = None
    if lengths is not None:
        off = torch.zeros(B + 1, dtype=torch.int64)
        off[1:] = torch.cumsum(torch.tensor(lengths, dtype=torch.int64), 0)
        keep = ops.pack_rows(idx, idx, None, off.to(DEV), int(off[-1]))
        kw.update(seq_offsets=keep["seq_offsets"], row_pos=keep["row_pos"])
        idx = keep["hist"]
    cfg = ops.make_encoder_cfg(**kw)
    n_params = N.load().xfmr_param_count(ctypes.byref(cfg))
    flat = (0.05 * torch.randn(n_params, generator=g)).to(DEV)
    rows = cfg.packed_rows if lengths is not None else B * L
    d_out = torch.randn(rows, H, generator=g).to(DEV)
    return cfg, flat, idx, unit_table(V, H).to(DEV), d_out, keep


def _step(ops, cfg, flat, idx, table, d_out):
    tok, key_mask, acts = ops.encoder_fwd(cfg, flat, idx, table)
    grads = ops.encoder_bwd(cfg, flat, d_out.clone().view_as(tok), key_mask, acts)
    return tok, grads


def _both_modes(ops, monkeypatch, *args):
    monkeypatch.setenv("XFMR_LN_STORE_X", "1")
    tok_s, g_s = _step(ops, *args)
    monkeypatch.delenv("XFMR_LN_STORE_X")
    tok_r, g_r = _step(ops, *args)
    assert torch.isfinite(tok_r).all() and torch.isfinite(g_r).all()
    assert torch.equal(tok_r, tok_s)
    assert torch.equal(g_r, g_s)


@pytest.mark.parametrize("drop", [0.1, 0.0])
@pytest.mark.parametrize("B", [82, 62])  # fused FFN at its threshold / LayerNorm-fused GEMMs with the FFN unfused
def test_rederived_residual_equals_the_stored_one(ops, monkeypatch, B, drop):
    cfg, flat, idx, table, d_out, _ = _inputs(ops, B, 2, drop)
    _both_modes(ops, monkeypatch, cfg, flat, idx, table, d_out)


def test_rederived_residual_single_layer(ops, monkeypatch):
    cfg, flat, idx, table, d_out, _ = _inputs(ops, 82, 1, 0.1)
    _both_modes(ops, monkeypatch, cfg, flat, idx, table, d_out)


def test_rederived_residual_packed_rows(ops, monkeypatch):
    B = 82  # planned for 16 400 rows (fused FFN); the rows actually run are ragged and no multiple of 64
    g = torch.Generator().manual_seed(3)
    lengths = torch.randint(1, L + 1, (B,), generator=g).tolist()
    lengths[0], lengths[1], lengths[2] = L, 0, 1
    if sum(lengths) % 64 == 0:
        lengths[3] += 1 if lengths[3] < L else -1
    assert sum(lengths) % 64 != 0
    cfg, flat, idx, table, d_out, keep = _inputs(ops, B, 2, 0.1, lengths=lengths)
    _both_modes(ops, monkeypatch, cfg, flat, idx, table, d_out)
    del keep


def test_nothing_reads_the_unstored_outputs(ops, monkeypatch):
    """The workspace is all-ones bytes (NaN as fp32 and as bf16) before the forward: whatever the forward does not write stays
    NaN, so a kernel that still read x0 / x1 / x2 would show in the results. And the regions do go unwritten: 2 x layers fp32
    row tensors (x0, x1 per layer, x2 of every layer but the last) more than with the stores on."""
    from xfmr_rec_amd import _native as N

    B, nL = 82, 2
    cfg, flat, idx, table, d_out, _ = _inputs(ops, B, nL, 0.1)
    lib = N.load()
    nbytes = lib.xfmr_encoder_workspace_bytes(ctypes.byref(cfg))
    assert nbytes > 0 and nbytes % 4 == 0

    def run():
        acts = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=DEV)
        tok = torch.empty(B, L, H, device=DEV)
        key_mask = torch.empty(B, L, dtype=torch.uint8, device=DEV)
        N.check(lib.xfmr_encoder_fwd(ctypes.byref(cfg), N.ptr(flat), N.ptr(idx), N.ptr(table), table.shape[0], N.ptr(tok),
                                     N.ptr(key_mask), N.ptr(acts), nbytes, N.stream()), "xfmr_encoder_fwd")
        untouched = int((acts.view(torch.int32) == -1).sum())
        grads = ops.encoder_bwd(cfg, flat, d_out.clone().view_as(tok), key_mask, acts)
        return tok, grads, untouched

    monkeypatch.setenv("XFMR_LN_STORE_X", "1")
    tok_s, g_s, untouched_s = run()
    monkeypatch.delenv("XFMR_LN_STORE_X")
    tok_r, g_r, untouched_r = run()
    assert torch.isfinite(tok_r).all() and torch.isfinite(g_r).all()
    assert torch.equal(tok_r, tok_s) and torch.equal(g_r, g_s)
    assert untouched_r - untouched_s == 2 * nL * B * L * H, (untouched_r, untouched_s)
