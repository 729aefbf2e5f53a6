"""The dropout-on path of the kernels against the HOST model of the mask (dropout_model.py, pinned by
test_dropout_model_host.py) and against fp64 references that apply that mask -- not against each other.

1. Every kernel family that applies or differentiates a dropout site draws exactly the host model's mask: the hidden-state
   sites through x = 0 / w = 0 / bias = 1 / residual = 0 (the output is keep / (1 - p) itself), attention through q = k = 0
   and one-hot value rows (ctx spells out the mask of the visible pairs, 32 or 64 key columns per forward).
2. attn_fwd / attn_bwd under dropout against fp64 attention with the mask on the normalised probabilities (HF's place), dq,
   dk and dv each on its own; and the bf16 kernels at the fp32 level against their rounding model.

A slip that forward and backward share -- the mask keyed by the wrong head, a lost 1 / (1 - p), dropout on the wrong side of
the bias -- passes every forward-against-backward and kernel-against-kernel check; it fails here."""

import functools

import numpy as np
import pytest
import torch

import dropout_model as dm
from helpers import assert_close
from test_gpu_ops import _attention_bf16_emulation, _attention_reference, _rand, fp32_level

pytestmark = pytest.mark.gpu
DEV = "cuda"
BIG_SEED = 6018027440424182934  # both halves of the 64-bit seed in use
BF16 = torch.bfloat16


@pytest.fixture(scope="module")
def ops():
    from xfmr_rec_amd import ops as _ops

    return _ops


@pytest.fixture(scope="module")
def lib():
    from xfmr_rec_amd import _native as N

    return N.load()


def _is_the_mask(tag, y, keep, p):
    """y is keep / (1 - p): non-zero exactly where the host model keeps, and every non-zero the fp32 scale exactly."""
    y = y.detach().float().cpu().numpy().reshape(keep.shape)
    wrong = int(((y != 0) != (keep != 0)).sum())
    assert wrong == 0, f"{tag}: {wrong} of {keep.size} elements differ from the host model's mask"
    assert bool((y[keep != 0] == np.float32(dm.scale(p))).all()), f"{tag}: a kept element is not 1 / (1 - p) in fp32"
    assert 0 < keep.mean() < 1 or keep.size < 8, tag


# ------------------------------------------------------------------------------------------------ hidden-state sites
@pytest.mark.parametrize("p", [0.1, 0.25])
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_linear_dropout_residual_epilogue_draws_the_host_mask(ops, prec, p):
    """EPI_BIAS_DROP_RES (xfmr_linear_fwd): one row, a tile less one, a tile plus one, partial tiles after full ones; N with
    32-wide, one and several column tiles."""
    from xfmr_rec_amd import _native as N

    for M in (1, 63, 65, 300):
        for Nn in (96, 128, 512):
            for seed, site in ((5, 3), (BIG_SEED, 9)):
                y = ops.linear_fwd(torch.zeros(M, 64, device=DEV), torch.zeros(Nn, 64, device=DEV), torch.ones(Nn, device=DEV),
                                   epilogue=N.EPI_BIAS_DROP_RES, residual=torch.zeros(M, Nn, device=DEV), dropout_p=p,
                                   seed=seed, site=site, precision=prec)
                _is_the_mask(f"linear M={M} N={Nn} {prec} p={p} seed={seed}", y, dm.hidden_keep(seed, site, M, Nn, p), p)


@pytest.mark.parametrize("p", [0.1, 0.25])
@pytest.mark.parametrize("M", [300, 4113])
def test_linear_layernorm_epilogue_draws_the_host_mask(lib, M, p):
    """EPI_DROP_RES_LN (xf_linear_ln_fwd_ex): its `pre` output, the LayerNorm's input."""
    from xfmr_rec_amd import _native as N

    Nn, K = 128, 128
    z = lambda *s, dt=torch.float32: torch.zeros(*s, device=DEV, dtype=dt)  # noqa: E731
    pre, y, y16, mean, rstd = z(M, Nn), z(M, Nn), z(M, Nn, dt=BF16), z(M), z(M)
    x, w, res, beta = z(M, K, dt=BF16), z(Nn, K, dt=BF16), z(M, Nn), z(Nn)  # (named: N.ptr keeps no tensor alive)
    bias, gamma = torch.ones(Nn, device=DEV), torch.ones(Nn, device=DEV)
    rc = lib.xf_linear_ln_fwd_ex(N.ptr(x), N.ptr(w), N.ptr(bias), N.ptr(pre), M, Nn, K, N.ptr(res), p, BIG_SEED, 6,
                                 N.ptr(gamma), N.ptr(beta), 1e-12, N.ptr(y), N.ptr(y16), N.ptr(mean), N.ptr(rstd),
                                 N.precision_id("bf16"), 3, N.stream())
    assert rc == 0, rc
    _is_the_mask(f"linear_ln M={M} p={p}", pre, dm.hidden_keep(BIG_SEED, 6, M, Nn, p), p)


@pytest.mark.parametrize("chunk", ["64", "128"])
@pytest.mark.parametrize("p", [0.1, 0.25])
@pytest.mark.parametrize("M", [300, 4113])
def test_fused_ffn_forward_draws_the_host_mask(lib, monkeypatch, M, p, chunk):
    """ffn_fwd_fused_kernel: w2 = 0, b2 = 1, residual 0 leave `pre` = keep / (1 - p) -- dropout AFTER the bias (a build that
    drops before it returns 1 everywhere)."""
    from xfmr_rec_amd import _native as N

    H, I = 128, 512
    monkeypatch.setenv("XFMR_FFN_CHUNK", chunk)
    z = lambda *s, dt=torch.float32: torch.zeros(*s, device=DEV, dtype=dt)  # noqa: E731
    g = torch.Generator().manual_seed(M)
    x16 = torch.randn(M, H, generator=g).to(DEV).to(BF16)
    w1 = (torch.randn(I, H, generator=g) * 0.08).to(DEV).to(BF16)
    o = dict(d=z(M, I, dt=BF16), g=z(M, I, dt=BF16), pre=z(M, H), y=z(M, H), y16=z(M, H, dt=BF16), mean=z(M), rstd=z(M))
    b1, w2, res, beta = z(I), z(H, I, dt=BF16), z(M, H), z(H)  # (named: N.ptr keeps no tensor alive)
    b2, gamma = torch.ones(H, device=DEV), torch.ones(H, device=DEV)
    rc = lib.xf_ffn_fwd_fused_ex(N.ptr(x16), N.ptr(w1), N.ptr(b1), N.ptr(w2), N.ptr(b2), N.ptr(o["d"]), N.ptr(o["g"]),
                                 N.ptr(o["pre"]), M, H, I, N.ptr(res), p, 5, 11, N.ptr(gamma), N.ptr(beta), 1e-12,
                                 N.ptr(o["y"]), N.ptr(o["y16"]), N.ptr(o["mean"]), N.ptr(o["rstd"]), N.stream())
    assert rc == 0, rc
    _is_the_mask(f"ffn_fwd M={M} p={p} chunk={chunk}", o["pre"], dm.hidden_keep(5, 11, M, H, p), p)


@pytest.mark.parametrize("p", [0.1, 0.25])
@pytest.mark.parametrize("H", [96, 128, 256])  # the generic LayerNorm kernel; 32 and 64 lanes per row
def test_embedding_layernorm_output_draws_the_host_mask(ops, H, p):
    """SITE_EMB: gamma = 0, beta = 1 make the LayerNorm output 1, so the stored output is the mask."""
    for M in (65, 300):
        g = torch.Generator().manual_seed(M)
        table = torch.randn(8, H, generator=g).to(DEV)
        idx = torch.randint(1, 8, (1, M), generator=g).to(DEV)
        out = ops.embed_ln_fwd(idx, table, torch.zeros(M, H, device=DEV), torch.zeros(2, H, device=DEV),
                               torch.zeros(H, device=DEV), torch.ones(H, device=DEV), dropout_p=p, seed=BIG_SEED,
                               site=dm.SITE_EMB)[0]
        _is_the_mask(f"embed_ln M={M} H={H} p={p}", out, dm.hidden_keep(BIG_SEED, dm.SITE_EMB, M, H, p), p)


@pytest.mark.parametrize("p", [0.1, 0.25])
@pytest.mark.parametrize("H", [96, 128])
def test_layernorm_backward_d_lin_is_zero_exactly_where_the_host_model_drops(ops, H, p):
    """xfmr_layernorm_bwd's d_lin (gradient of the Linear in front of the dropout): dx * keep / (1 - p)."""
    M = 300
    x, dy = _rand(M, H, seed=1).to(DEV), _rand(M, H, seed=2).to(DEV)
    gamma = (1 + 0.1 * _rand(H, seed=3)).to(DEV)
    _, mean, rstd = ops.layernorm_fwd(x, gamma, torch.zeros(H, device=DEV))
    dx, d_lin, *_ = ops.layernorm_bwd(dy, x, mean, rstd, gamma, dropout_p=p, seed=BIG_SEED, site=7)
    keep = torch.from_numpy(dm.hidden_keep(BIG_SEED, 7, M, H, p)).to(DEV)
    assert bool((dx != 0).all())
    assert torch.equal(d_lin != 0, keep != 0)
    torch.testing.assert_close(d_lin, dx * keep * dm.scale(p), rtol=1e-6, atol=0)


# ------------------------------------------------------------------------------------------------ attention: the mask
def _key_mask(B, L, lengths):
    mask = torch.zeros(B, L, dtype=torch.uint8)
    for b, n in enumerate(lengths):
        mask[b, :n] = 1
    if B > 1:
        mask[1, 2] = 0  # a hole in the middle: the kernels take an arbitrary key mask
    return mask


def _visible(mask, causal):
    B, L = mask.shape
    tri = torch.ones(L, L, dtype=torch.bool)
    return (tri.tril() if causal else tri)[None] & mask.bool()[:, None, :]  # (B, q, key)


ATTN_MASK_CASES = (
    [("bf16", 32, B, L, A, False) for B, L, A in ((2, 40, 2), (2, 200, 4), (1, 320, 2), (1, 512, 1))]
    + [("fp32", 32, B, L, A, False) for B, L, A in ((2, 40, 2), (2, 200, 4))]
    + [("bf16", 64, 2, 130, 2, False), ("fp32", 64, 2, 130, 2, False),
       ("fp32", 32, 1, 512, 1, True)])  # the key-streaming form (test_gpu_attn_long.py's switch)


@pytest.mark.parametrize("causal", [True, False], ids=["causal", "bidirectional"])
@pytest.mark.parametrize("prec,dh,B,L,A,stream", ATTN_MASK_CASES)
def test_attention_kernels_draw_the_host_mask(ops, prec, dh, B, L, A, stream, causal):
    """q = k = 0: every visible key has probability 1 / n_visible(q). v[key, d] = 1 iff key = d + dh j makes
    ctx[b, q, h, d] = keep(q, d + dh j) / (1 - p) / n_visible(q): ceil(L / dh) forwards spell out the (B, A, L, L) mask on the
    visible pairs. B = 2 and A >= 2 are what hold the row to (b A + h) L + q."""
    p, seed, site = 0.1, BIG_SEED, dm.site_attn(1)
    H = dh * A
    mask = _key_mask(B, L, [L, L - 3][:B])
    vis = _visible(mask, causal)[:, None].expand(B, A, L, L)
    nvis = vis.sum(-1).clamp(min=1).float()  # (B, A, q)
    want = torch.from_numpy(dm.attention_keep(seed, site, B, A, L, p)).bool()
    got = torch.zeros(B, A, L, L, dtype=torch.bool)
    mdev = mask.to(DEV)
    sc = float(np.float32(dm.scale(p)))
    for j in range((L + dh - 1) // dh):
        qkv = torch.zeros(B, L, 3 * H)
        v = qkv[..., 2 * H:].view(B, L, A, dh)
        n = min(dh, L - dh * j)
        v[:, dh * j + torch.arange(n), :, torch.arange(n)] = 1.0
        ctx, _ = ops.attn_fwd(qkv.to(DEV), mdev, A, dropout_p=p, seed=seed, site=site, precision=prec, causal=causal,
                              stream_keys=stream)
        c = ctx.cpu().view(B, L, A, dh).permute(0, 2, 1, 3)[..., :n]  # (B, A, q, key - dh j)
        got[..., dh * j:dh * j + n] = c != 0
        # a kept visible pair holds scale / n_visible (bf16: the probability operand is bf16(scale))
        ref = vis[..., dh * j:dh * j + n] & want[..., dh * j:dh * j + n]
        val = (sc if prec == "fp32" else float(torch.tensor(sc).to(BF16))) / nvis[..., None]
        torch.testing.assert_close(c, ref.float() * val, rtol=2e-6, atol=0)
    assert torch.equal(got & vis, want & vis)
    assert not bool((got & ~vis).any())
    assert 0.85 < float(got[vis].float().mean()) < 0.95


# ------------------------------------------------------------------------------------------------ attention: values
ATTN_SHAPES = [(3, 12, 1, [12, 7, 1]), (2, 130, 2, [130, 77]), (2, 200, 4, [200, 150]), (2, 320, 2, [320, 301]),
               (1, 512, 1, [512])]


def _covered(prec, dh, L):
    """test_attention_fwd_bwd's limits: the fp32 policy and head size 64 through the lengths their panel kernels hold."""
    return not (prec == "fp32" and L > (256 if dh == 32 else 128)) and not (dh == 64 and L > 256)


ATTN_VALUE_CASES = [(prec, dh, *shape) for prec in ("fp32", "bf16") for dh in (32, 64) for shape in ATTN_SHAPES
                    if _covered(prec, dh, shape[1])]


@functools.lru_cache(maxsize=None)
def _attn_inputs(B, L, A, dh, lengths):
    H = dh * A
    qkv = _rand(B, L, 3 * H, seed=3)
    mask = _key_mask(B, L, lengths)
    w = _rand(B, L, H, seed=4) * mask[..., None]  # the training path only back-propagates valid rows
    return qkv, mask, w


@pytest.mark.parametrize("causal", [True, False], ids=["causal", "bidirectional"])
@pytest.mark.parametrize("p", [0.1, 0.3])
@pytest.mark.parametrize("prec,dh,B,L,A,lengths", ATTN_VALUE_CASES)
def test_attention_under_dropout_vs_fp64(ops, prec, dh, B, L, A, lengths, p, causal):
    """ctx on the valid rows and dq, dk, dv each on its own against fp64 attention that multiplies the normalised
    probabilities by the host model's keep / (1 - p). L = 320 / 512 in bf16: the two-block forward and the dQ + dK/dV pair,
    which no other dropout check reaches. Measured on an MI355X at p = 0.1, bf16, causal -- L = 320: ctx 8.2e-3, dq 4.3e-3,
    dk 4.3e-3, dv 3.1e-3; L = 512: ctx 5.4e-3, dq 5.0e-3, dk 5.0e-3, dv 3.0e-3 (limits 3e-2); fp32 policy <= 6.9e-7 (1e-4)."""
    seed, site = BIG_SEED, dm.site_attn(2)
    H = dh * A
    qkv, mask, w = _attn_inputs(B, L, A, dh, tuple(lengths))
    keep = torch.from_numpy(dm.attention_keep(seed, site, B, A, L, p).astype("float64")) * dm.scale(p)
    ref_in = qkv.clone().double().requires_grad_(True)
    ref = _attention_reference(ref_in, mask, A, causal, keep=keep)
    (ref * w.double()).sum().backward()
    kw = dict(dropout_p=p, seed=seed, site=site, precision=prec, causal=causal)
    ctx, lse = ops.attn_fwd(qkv.to(DEV), mask.to(DEV), A, **kw)
    valid = mask.bool()
    e = [assert_close("attn.ctx", ctx.cpu()[valid], ref.detach()[valid], prec)]
    d_qkv = ops.attn_bwd(qkv.to(DEV), mask.to(DEV), ctx, lse, w.to(DEV), A, **kw)
    for name, sl in (("dq", slice(0, H)), ("dk", slice(H, 2 * H)), ("dv", slice(2 * H, 3 * H))):
        e.append(assert_close(f"attn.{name}", d_qkv[..., sl], ref_in.grad[..., sl], prec, "grad"))
    print(f"FIG attn dropout {prec} dh={dh} B={B} L={L} A={A} p={p} causal={causal}: ctx {e[0]:.2e}  dq {e[1]:.2e}  "
          f"dk {e[2]:.2e}  dv {e[3]:.2e}")


@pytest.mark.parametrize("causal", [True, False], ids=["causal", "bidirectional"])
@pytest.mark.parametrize("B,L,A,lengths", [(1, 512, 2, [512]), (2, 320, 2, [320, 301]), (2, 200, 4, [200, 150])])
def test_bf16_attention_under_dropout_at_fp32_level_against_the_rounding_model(ops, B, L, A, lengths, causal):
    """test_bf16_attention_kernels_at_fp32_level_against_their_rounding_model with p = 0.1, at its limits (rel-L2 1e-4, at most
    2e-3 of the elements outside 1e-4). The kernels multiply by keep / (1 - p) in fp32 BEFORE each bf16 rounding -- forward:
    bf16(p keep) into P V, the row sum from the unmasked p; backward: bf16(P keep) into dV, bf16(P (dP keep - delta)) into dQ
    and dK (attention.hip: attn_fwd_bf16_kernel, attn_bwd_dq_bf16_kernel, attn_bwd_dkv_bf16_kernel and the fused one-workgroup
    forms) -- and so does the model (_attention_bf16_emulation's `keep`).
    The backward is modelled from ITS inputs -- the forward kernel's stored ctx and lse, after both are held to the model's
    own -- and with the fp32 roundings of its exponent chain (_attention_bf16_emulation's `fwd`). The fp64-only model of the
    backward, whose probabilities sit up to ~1e-6 from the kernel's, measured dv rel-L2 1.007e-4 at (2, 200, 4) causal on an
    MI355X: 98.4 % of that squared error in ONE dV row (b = 1, key 13, head 1), exactly along dO of query 23 with a weight
    change of -2^-10 -- one probability P keep of a row with few visible keys on the other side of a bf16 rounding boundary,
    1.3e-5 without that row: the mis-modelled rounding points were the fp32 ones in front of the bf16 rounding.
    Measured with `fwd` over the six cases: lse within 1.4e-7 of the model's; rel-L2 ctx 4.8e-6 ... 3.2e-5, dq 2.2e-6 ...
    1.5e-5, dk 1.1e-7 ... 1.8e-5, dv 7.3e-8 ... 1.8e-7 (no probability of the dV operand rounds differently any more); share
    outside 1e-4 at most 4.6e-4 (ctx, L = 512, causal). (fp64-only backward model, the other cases: 9.9e-6 ... 3.8e-5.)"""
    p, seed, site = 0.1, BIG_SEED, dm.site_attn(0)
    H = 32 * A
    qkv = _rand(B, L, 3 * H, seed=13).to(BF16).float()
    mask = _key_mask(B, L, lengths)
    w = (_rand(B, L, H, seed=14) * mask[..., None]).to(BF16).float()
    keep = torch.from_numpy(dm.attention_keep(seed, site, B, A, L, p).astype("float64")) * dm.scale(p)
    kw = dict(dropout_p=p, seed=seed, site=site, precision="bf16", causal=causal)
    ctx, lse = ops.attn_fwd(qkv.to(DEV), mask.to(DEV), A, **kw)
    want_ctx, want_d, want_lse = _attention_bf16_emulation(qkv, mask, A, w, causal, keep=keep, fwd=(ctx, lse))
    valid = mask.bool()
    figs = [fp32_level("attn.ctx", ctx.cpu()[valid], want_ctx[valid])]
    rows = valid[:, None, :].expand(B, A, L)  # (causal: every valid query sees a key; bidirectional: every query does)
    e_lse = assert_close("attn.lse", lse.cpu()[rows], want_lse[rows], "fp32")  # the forward's other output, before it is used
    d_qkv = ops.attn_bwd(qkv.to(DEV), mask.to(DEV), ctx, lse, w.to(DEV), A, **kw)
    figs.append(fp32_level("attn.d_qkv", d_qkv, want_d))
    for name, sl in (("dq", slice(0, H)), ("dk", slice(H, 2 * H)), ("dv", slice(2 * H, 3 * H))):
        figs.append(fp32_level(f"attn.{name}", d_qkv[..., sl], want_d[..., sl]))
    print(f"FIG attn dropout fp32-level B={B} L={L} A={A} causal={causal}: lse {e_lse:.1e}; (rel-L2, share outside 1e-4) ctx / d_qkv / dq / dk / dv"
          " = " + "  ".join(f"({a:.2e}, {b:.1e})" for a, b in figs))
