"""The two fused backward kernels of the encoder's dX chain against fp64 references (fused_refs.py, proven on the host by
test_fused_refs_host.py) instead of against each other:

  xf_ffn_bwd_dx_fused_ex (gemm.hip: ffn_bwd_dx_fused_kernel, both weight-staging forms)
  xf_linear_bwd_dx_lnbwd_ex (the dX GEMM with the LayerNorm backward in its epilogue) at small and ragged M, with the
  dropout of the LayerNorm OUTPUT (layer 0's call: the embedding LayerNorm)

Inputs are bf16-representable, so the references see exactly the operands the MFMAs see. Dropout masks come from the FORWARD
kernels that apply them (the Linear + dropout + residual epilogue; the embedding LayerNorm), never from the kernel under test,
and are held to the host model of the mask (dropout_model.py) where they are extracted.
Every output is pre-filled with 0xFF bytes (NaN as fp32 and as bf16) and has 64 guard rows behind it that must keep them.

Limits. dI is bf16(fp32 accumulation): against bf16(fp64) it may differ by one bf16 ulp where the fp32 error (and the 1.5e-7 of
the kernel's erf polynomial) crosses a rounding boundary -- a CPU model of exactly that gives a share of 3.8e-4 ... 3.9e-4 of
the elements, the cap is the forward twin's 2e-3 (test_ffn_forward_in_one_kernel_vs_the_two_gemm_form). The second stage is
judged from the kernel's OWN dI, where only fp32 accumulation remains: helpers.TOL["fp32"]."""

import ctypes as C
import functools

import numpy as np
import pytest
import torch

import dropout_model as dm
from fused_refs import dx_lnbwd_ref, ffn_bwd_dx_ref
from helpers import assert_close
from test_gpu_ffn_weight_ring import H, _inputs

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 64
SEED, SITE, SITE_OUT = 5, 9, 2
BF16, F32 = torch.bfloat16, torch.float32


@pytest.fixture(scope="module")
def lib():
    from xfmr_rec_amd import _native as N

    return N.load()


# ------------------------------------------------------------------------------------------------ guards, masks
def _guarded(rows, cols, dtype):
    """[rows + GUARD][cols] of all-ones bytes; the kernel gets its start and is told about `rows` only."""
    nbytes = (rows + GUARD) * cols * torch.empty((), dtype=dtype).element_size()
    return torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=DEV).view(dtype).view(rows + GUARD, cols)


def _guard_intact(t, rows):
    return bool((t[rows:].contiguous().view(torch.uint8) == 0xFF).all())


def _one_bf16_ulp(got, ref):
    """|d| <= 2^-7 |ref| + 1e-6, elementwise (fp64)."""
    got, ref = got.double().cpu(), ref.double().cpu()
    return bool(((got - ref).abs() <= 2.0 ** -7 * ref.abs() + 1e-6).all())


@functools.lru_cache(maxsize=None)
def _keep(M, p):
    """The 0/1 mask of hidden-state dropout (SEED, SITE) on an [M][128] tensor, from the forward epilogue that applies it:
    x = 0, w = 0, bias = 1, residual = 0 leaves keep / (1 - p) (test_hidden_dropout_keep_rate_and_structure)."""
    from xfmr_rec_amd import _native as N
    from xfmr_rec_amd import ops

    y = ops.linear_fwd(torch.zeros(M, 64, device=DEV), torch.zeros(H, 64, device=DEV), torch.ones(H, device=DEV),
                       epilogue=N.EPI_BIAS_DROP_RES, residual=torch.zeros(M, H, device=DEV), dropout_p=p, seed=SEED,
                       site=SITE, precision="bf16")
    assert bool(((y == 0) | ((y - 1 / (1 - p)).abs() < 1e-6)).all())
    keep = (y != 0).double().cpu()
    assert 0 < float(keep.mean()) < 1
    assert np.array_equal(keep.numpy(), dm.hidden_keep(SEED, SITE, M, H, p).astype(np.float64))  # = the host model's mask
    return keep


@functools.lru_cache(maxsize=None)
def _keep_out(M, p):
    """The mask of the dropout on the embedding LayerNorm's OUTPUT (SEED, SITE_OUT), from the kernel that makes it:
    gamma = 0, beta = 1 makes the LayerNorm output 1 everywhere (no exact zeros), so out != 0 is the mask."""
    from xfmr_rec_amd import ops

    g = torch.Generator().manual_seed(M)
    table = torch.randn(8, H, generator=g).to(DEV)
    idx = torch.randint(1, 8, (1, M), generator=g).to(DEV)
    out = ops.embed_ln_fwd(idx, table, torch.zeros(M, H, device=DEV), torch.zeros(2, H, device=DEV),
                           torch.zeros(H, device=DEV), torch.ones(H, device=DEV), dropout_p=p, seed=SEED, site=SITE_OUT)[0]
    out = out.view(M, H)
    assert bool(((out == 0) | ((out - 1 / (1 - p)).abs() < 1e-6)).all())
    keep = (out != 0).double().cpu()
    assert np.array_equal(keep.numpy(), dm.hidden_keep(SEED, SITE_OUT, M, H, p).astype(np.float64))  # = the host model's mask
    return keep


def _check_ln_stage(tag, o, ref, M, blocks, n_tiles, keep, p, with_dlin):
    """dx, the reduced partial records and the bf16 copy of one launch against `ref` (ln_chain_ref's dict)."""
    assert (M + 63) // 64 <= blocks <= n_tiles, (blocks, n_tiles)
    for k, rows in (("dx", M), ("parts", n_tiles)) + ((("dlin", M),) if with_dlin else ()):
        assert _guard_intact(o[k], rows), f"{tag}: rows behind {k} were written"
    dx = o["dx"][:M]
    parts = o["parts"][:blocks].view(blocks, 3, H)
    assert torch.isfinite(dx).all() and torch.isfinite(parts).all(), tag
    red = parts.sum(0)
    e = [assert_close(f"{tag} dx", dx, ref["dx"], "fp32")]
    for j, k in enumerate(("d_gamma", "d_beta", "d_bias")):
        e.append(assert_close(f"{tag} {k}", red[j], ref[k], "fp32", "grad"))
    print(f"FIG {tag}: dx {e[0]:.2e}  d_gamma {e[1]:.2e}  d_beta {e[2]:.2e}  d_bias {e[3]:.2e}  blocks {blocks}/{n_tiles}")
    if with_dlin:
        dlin = o["dlin"][:M]
        if keep is not None:
            assert bool((dlin.cpu()[keep == 0] == 0).all()), f"{tag}: d_lin16 not zero where the Linear's output was dropped"
        assert _one_bf16_ulp(dlin, ref["d_lin"]), f"{tag}: d_lin16"
        if p == 0:
            assert torch.equal(dlin, dx.to(BF16)), f"{tag}: d_lin16 != bf16(dx) without dropout"


# ------------------------------------------------------------------------------------------------ xf_ffn_bwd_dx_fused_ex
SHAPES = [(1, 64),        # one row, one chunk
          (65, 64),       # a second tile with a single valid row
          (72, 192),      # odd chunk count
          (136, 128),     # one chunk pair -- the smallest I the encoder sends -- and an 8-row third tile
          (200, 512),     # partial tile after full ones
          (448, 1024)]    # seven tiles, the fused forward's maximum I


@functools.lru_cache(maxsize=None)
def _ffn_case(M, I):
    t = _inputs(M, I)
    ref = ffn_bwd_dx_ref(t["dy"], t["w2"], t["u"], t["w1"], None, t["lnx"], t["gamma"], None, 0.0)
    return t, ref["di"]


def _run_ffn(lib, t, M, I, p_drop, with_rg, with_dlin):
    from xfmr_rec_amd import _native as N

    n_tiles = lib.xf_ln_row_tiles(M)
    o = dict(dx=_guarded(M, H, F32), di=_guarded(M, I, BF16), parts=_guarded(n_tiles, 3 * H, F32))
    if with_dlin:
        o["dlin"] = _guarded(M, H, BF16)
    blocks = C.c_int(0)
    rc = lib.xf_ffn_bwd_dx_fused_ex(N.ptr(t["dy"]), N.ptr(t["w2"]), N.ptr(t["u"]), N.ptr(t["w1"]), N.ptr(o["di"]), M, H, I,
                                    N.ptr(t["rg"]) if with_rg else None, N.ptr(t["lnx"]), N.ptr(t["mean"]), N.ptr(t["rstd"]),
                                    N.ptr(t["gamma"]), p_drop, SEED, SITE, N.ptr(o["dx"]),
                                    N.ptr(o["dlin"]) if with_dlin else None, N.ptr(o["parts"]), C.byref(blocks), N.stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return o, blocks.value, n_tiles


@pytest.mark.parametrize("with_dlin", [True, False], ids=["dlin", "nodlin"])
@pytest.mark.parametrize("with_rg", [True, False], ids=["rg", "norg"])
@pytest.mark.parametrize("p_drop", [0.0, 0.1])
@pytest.mark.parametrize("M,I", SHAPES)
def test_fused_ffn_backward_dx_against_fp64(lib, monkeypatch, M, I, p_drop, with_rg, with_dlin):
    """The table of shapes is the entry point's contract (any I that is a multiple of 64; the encoder only sends multiples
    of 128). Measured on an MI355X: dI unequal to bf16(fp64) in 0 of 64, 1 of 4160, 2 of 13 824, 21 of 102 400 and 88 of
    458 752 elements -- shares 0, 2.4e-4, 1.4e-4, 2.1e-4, 1.9e-4 against the cap of 2e-3, none further than one bf16 ulp;
    the second stage from the kernel's own dI: dx <= 1.7e-6 (limit 1e-4), reduced records <= 2.9e-7 rel-L2 (limit 1e-4)."""
    t, di64 = _ffn_case(M, I)
    keep = _keep(M, p_drop) if p_drop > 0 else None
    monkeypatch.setenv("XFMR_FFN_REG_STAGE", "1")
    reg, blocks_reg, _ = _run_ffn(lib, t, M, I, p_drop, with_rg, with_dlin)
    monkeypatch.delenv("XFMR_FFN_REG_STAGE")
    ring, blocks, n_tiles = _run_ffn(lib, t, M, I, p_drop, with_rg, with_dlin)
    tag = f"ffn_bwd M={M} I={I} p={p_drop}"
    # dI against bf16(dI64)
    assert _guard_intact(ring["di"], M), "rows behind dI were written"
    di = ring["di"][:M].cpu()
    assert torch.isfinite(di.float()).all()
    want = di64.to(BF16)
    n_off = int((di != want).sum())
    print(f"FIG {tag}: dI unequal {n_off} of {di.numel()} = {n_off / di.numel():.2e}")
    assert _one_bf16_ulp(di, want), "dI: more than one bf16 ulp from bf16(fp64)"
    assert n_off <= 2e-3 * di.numel(), (n_off, di.numel())
    # dx, records, d_lin16: the reference evaluated from the kernel's own dI
    ref = ffn_bwd_dx_ref(t["dy"], t["w2"], t["u"], t["w1"], t["rg"] if with_rg else None, t["lnx"], t["gamma"], keep, p_drop,
                         di=di)
    _check_ln_stage(tag, ring, ref, M, blocks, n_tiles, keep, p_drop, with_dlin)
    # the two staging forms: bit for bit, guard rows included
    assert blocks_reg == blocks
    for k in ring:
        assert torch.equal(ring[k].view(torch.uint8), reg[k].view(torch.uint8)), k


# ------------------------------------------------------------------------------------------------ xf_linear_bwd_dx_lnbwd_ex
@functools.lru_cache(maxsize=None)
def _lnbwd_inputs(M, Nn):
    g = torch.Generator().manual_seed(1000 * Nn + M)
    t = dict(dy=torch.randn(M, Nn, generator=g).to(BF16), w=(torch.randn(Nn, H, generator=g) * 0.05).to(BF16),
             rg=torch.randn(M, H, generator=g), lnx=torch.randn(M, H, generator=g),
             gamma=1 + 0.1 * torch.randn(H, generator=g))
    t = {k: v.to(DEV) for k, v in t.items()}
    t["mean"] = t["lnx"].mean(-1).contiguous()
    t["rstd"] = (t["lnx"].var(-1, unbiased=False) + 1e-12).rsqrt().contiguous()
    return t


@pytest.mark.parametrize("p_drop,p_out", [(0.0, 0.0), (0.1, 0.0), (0.0, 0.1)], ids=["nodrop", "drop", "outdrop"])
@pytest.mark.parametrize("M", [1, 72, 200])
@pytest.mark.parametrize("Nn", [384, 512, 96])  # QKV; FFN1 when the FFN is unfused; 32-deep K slices
def test_dx_gemm_with_layernorm_backward_epilogue_against_fp64(lib, Nn, M, p_drop, p_out):
    """Small and ragged M, and the dropout of the LayerNorm OUTPUT (`drop2`: layer 0's call, where no Linear is in front of
    the embedding LayerNorm and d_lin16 is null). bf16-representable operands: only the fp32 accumulation remains.
    Measured on an MI355X: dx <= 1.3e-6 (limit 1e-4), reduced records <= 2.1e-7 rel-L2 (limit 1e-4)."""
    from xfmr_rec_amd import _native as N

    t = _lnbwd_inputs(M, Nn)
    with_dlin = p_out == 0.0
    keep = _keep(M, p_drop) if p_drop > 0 else None
    keep2 = _keep_out(M, p_out) if p_out > 0 else None
    n_tiles = lib.xf_ln_row_tiles(M)
    o = dict(dx=_guarded(M, H, F32), parts=_guarded(n_tiles, 3 * H, F32))
    if with_dlin:
        o["dlin"] = _guarded(M, H, BF16)
    blocks = C.c_int(0)
    rc = lib.xf_linear_bwd_dx_lnbwd_ex(N.ptr(t["dy"]), N.ptr(t["w"]), M, Nn, H, N.ptr(t["rg"]), N.ptr(t["lnx"]),
                                       N.ptr(t["mean"]), N.ptr(t["rstd"]), N.ptr(t["gamma"]), p_drop, SEED, SITE,
                                       N.ptr(o["dx"]), N.ptr(o["dlin"]) if with_dlin else None, N.ptr(o["parts"]),
                                       C.byref(blocks), N.precision_id("bf16"), 3, N.stream(), p_out, SITE_OUT)
    assert rc == 0, rc
    torch.cuda.synchronize()
    ref = dx_lnbwd_ref(t["dy"], t["w"], t["rg"], t["lnx"], t["gamma"], keep, p_drop, keep2, p_out)
    _check_ln_stage(f"dx_lnbwd M={M} N={Nn} p={p_drop} p_out={p_out}", o, ref, M, blocks.value, n_tiles, keep, p_drop,
                    with_dlin)
