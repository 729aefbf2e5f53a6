"""The fused FFN backward dX kernel (gemm.hip: ffn_bwd_dx_fused_kernel) stages its W2 / W1 chunks by LDS-DMA into swizzled
images, one chunk ahead of their use; XFMR_FFN_REG_STAGE=1 (read per call) keeps the register-staged form it replaces. Only
the way the weight operand reaches LDS differs: each tile runs the same MFMAs on the same operands in the same order, so the
two forms must agree BIT FOR BIT on every output -- dX, dI, the bf16 copy of the LayerNorm input gradient, and the
LayerNorm-backward partial records (raw and reduced).

Shapes are the smallest at which the staging can go wrong: H 128; I 128 / 512 / 1024 (one chunk pair, the benchmark's count,
the fused forward's maximum); 64 / 72 / 200 / 448 rows (one tile, a partial tile, a partial tile after full ones, seven
tiles); dropout on and off. One encoder-level case runs two layers at the fused FFN's threshold (82 x 200 = 16 400 tokens)."""

import ctypes as C

import pytest
import torch

from helpers import unit_table

pytestmark = pytest.mark.gpu
DEV = "cuda"
H = 128


@pytest.fixture(scope="module")
def lib():
    from xfmr_rec_amd import _native as N

    return N.load()


def _inputs(M, I):
    g = torch.Generator().manual_seed(1000 * I + M)
    t = dict(dy=torch.randn(M, H, generator=g).to(torch.bfloat16),
             w2=(torch.randn(H, I, generator=g) * 0.05).to(torch.bfloat16),
             u=torch.randn(M, I, generator=g).to(torch.bfloat16),
             w1=(torch.randn(I, H, generator=g) * 0.08).to(torch.bfloat16),
             rg=torch.randn(M, H, generator=g),
             lnx=torch.randn(M, H, generator=g),
             gamma=1 + 0.1 * torch.randn(H, generator=g))
    t = {k: v.to(DEV) for k, v in t.items()}
    t["mean"] = t["lnx"].mean(-1).contiguous()
    t["rstd"] = (t["lnx"].var(-1, unbiased=False) + 1e-12).rsqrt().contiguous()
    return t


def _run(lib, t, M, I, p_drop, fill=None):
    """One launch; `fill`: byte pattern the outputs hold beforehand (0xFF: NaN as fp32 and as bf16)."""
    from xfmr_rec_amd import _native as N

    n_tiles = lib.xf_ln_row_tiles(M)
    assert n_tiles >= (M + 63) // 64

    def out(shape, dtype):
        if fill is None:
            return torch.zeros(shape, device=DEV, dtype=dtype)
        nbytes = torch.empty(shape, dtype=dtype).numel() * torch.empty((), dtype=dtype).element_size()
        return torch.full((nbytes,), fill, dtype=torch.uint8, device=DEV).view(dtype).view(shape)

    o = dict(dx=out((M, H), torch.float32), di=out((M, I), torch.bfloat16), dlin=out((M, H), torch.bfloat16),
             parts=out((n_tiles, 3, H), torch.float32))
    blocks = C.c_int(0)
    rc = lib.xf_ffn_bwd_dx_fused_ex(N.ptr(t["dy"]), N.ptr(t["w2"]), N.ptr(t["u"]), N.ptr(t["w1"]), N.ptr(o["di"]), M, H, I,
                                    N.ptr(t["rg"]), N.ptr(t["lnx"]), N.ptr(t["mean"]), N.ptr(t["rstd"]), N.ptr(t["gamma"]),
                                    p_drop, 5, 9, N.ptr(o["dx"]), N.ptr(o["dlin"]), N.ptr(o["parts"]), C.byref(blocks),
                                    N.stream())
    assert rc == 0, rc
    assert (M + 63) // 64 <= blocks.value <= n_tiles
    o["parts"] = o["parts"][:blocks.value]
    o["reduced"] = o["parts"].sum(0)
    return o


def _both(lib, monkeypatch, t, M, I, p_drop, fill=None):
    monkeypatch.setenv("XFMR_FFN_REG_STAGE", "1")
    reg = _run(lib, t, M, I, p_drop, fill)
    monkeypatch.delenv("XFMR_FFN_REG_STAGE")
    ring = _run(lib, t, M, I, p_drop, fill)
    return ring, reg


@pytest.mark.parametrize("p_drop", [0.0, 0.1])
@pytest.mark.parametrize("M", [64, 72, 200, 64 * 7])
@pytest.mark.parametrize("I", [128, 512, 1024])
def test_ring_staged_backward_equals_the_register_staged_one(lib, monkeypatch, I, M, p_drop):
    t = _inputs(M, I)
    ring, reg = _both(lib, monkeypatch, t, M, I, p_drop)
    for k in ("dx", "di", "dlin", "parts", "reduced"):
        assert torch.isfinite(ring[k].float()).all(), k
        assert torch.equal(ring[k], reg[k]), k
    assert bool((ring["di"] != 0).any()) and bool((ring["dx"] != 0).any())


@pytest.mark.parametrize("M,I", [(200, 512), (64 * 7, 1024)])
def test_every_output_is_written_over_a_nan_pattern(lib, monkeypatch, M, I):
    """All-ones bytes (NaN as fp32 and as bf16) in every output beforehand: a ring that stalls one stage short would leave
    stale or unwritten rows. None survives, in either form, and the two forms still agree."""
    t = _inputs(M, I)
    ring, reg = _both(lib, monkeypatch, t, M, I, 0.1, fill=0xFF)
    for k in ("dx", "di", "dlin", "parts", "reduced"):
        assert torch.isfinite(ring[k].float()).all(), k
        assert torch.isfinite(reg[k].float()).all(), k
        assert torch.equal(ring[k], reg[k]), k


def test_encoder_step_at_the_fused_ffn_threshold(monkeypatch):
    """Two layers at T = 82 x 200 = 16 400 (the fused FFN pair's threshold: 256 full 64-row tiles + a 16-row tail): the encoder
    output and the whole flat gradient, bit for bit, between the two settings."""
    import ctypes

    from xfmr_rec_amd import _native as N
    from xfmr_rec_amd import ops

    B, L, A, I, V, nL = 82, 200, 4, 512, 300, 2
    g = torch.Generator().manual_seed(11)
    idx = torch.randint(1, V + 1, (B, L), generator=g).to(DEV)
    cfg = ops.make_encoder_cfg(batch=B, seq_len=L, hidden=H, heads=A, inter=I, layers=nL, max_pos=L, precision="bf16",
                               hidden_dropout=0.1, attn_dropout=0.1, seed=1234)
    n_params = N.load().xfmr_param_count(ctypes.byref(cfg))
    flat = (0.05 * torch.randn(n_params, generator=g)).to(DEV)
    d_out = torch.randn(B * L, H, generator=g).to(DEV)
    table = unit_table(V, H).to(DEV)

    def step():
        tok, key_mask, acts = ops.encoder_fwd(cfg, flat, idx, table)
        grads = ops.encoder_bwd(cfg, flat, d_out.clone().view_as(tok), key_mask, acts)
        return tok, grads

    monkeypatch.setenv("XFMR_FFN_REG_STAGE", "1")
    tok_s, g_s = step()
    monkeypatch.delenv("XFMR_FFN_REG_STAGE")
    tok_r, g_r = step()
    assert torch.isfinite(tok_r).all() and torch.isfinite(g_r).all()
    assert torch.equal(tok_r, tok_s)
    assert torch.equal(g_r, g_s)
