"""GPU parity of the individual HIP kernels, called through the C ABI (ctypes), against plain fp32/fp64
PyTorch on the CPU. Sizes are small enough for the CPU side to take seconds; they cover ragged / partial
tiles (M, N, K not multiples of the tile), both MFMA precisions, and the encoder's real shapes."""

import pytest
import torch
import torch.nn.functional as F

from helpers import assert_close, rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def ops():
    from xfmr_rec_amd import ops as _ops

    return _ops


def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def test_mfma_lane_maps(ops):
    out = ops.selftest_mfma(DEV)
    assert out[:3] == [0, 0, 0], f"MFMA fragment/accumulator maps wrong: total/bf16/f32 mismatches = {out[:3]}"


@pytest.mark.parametrize("H", [32, 64, 128, 256, 320])
def test_layernorm_fwd_bwd(ops, H):
    rows = 77
    x, gamma, beta, dy = _rand(rows, H, seed=1), 1 + 0.1 * _rand(H, seed=2), 0.1 * _rand(H, seed=3), _rand(rows, H, seed=4)
    xr = x.clone().double().requires_grad_(True)
    gr, br = gamma.clone().double().requires_grad_(True), beta.clone().double().requires_grad_(True)
    yr = F.layer_norm(xr, (H,), gr, br, 1e-12)
    yr.backward(dy.double())
    y, mean, rstd = ops.layernorm_fwd(x.to(DEV), gamma.to(DEV), beta.to(DEV))
    assert_close("ln.y", y, yr, "fp32")
    assert_close("ln.mean", mean, xr.mean(-1), "fp32")
    dx, d_lin, dg, db, dbias = ops.layernorm_bwd(dy.to(DEV), x.to(DEV), mean, rstd, gamma.to(DEV))
    assert d_lin is None
    assert_close("ln.dx", dx, xr.grad, "fp32", "grad")
    assert_close("ln.dgamma", dg, gr.grad, "fp32", "grad")
    assert_close("ln.dbeta", db, br.grad, "fp32", "grad")
    assert_close("ln.dbias", dbias, xr.grad.sum(0), "fp32", "grad")


def test_layernorm_bwd_dropout_consistency(ops):
    """d_lin = dx * keep/(1-p) with the same mask the forward GEMM epilogue applied (same seed/site)."""
    from xfmr_rec_amd import _native as N

    M, H, p = 200, 128, 0.25
    x, w, b = _rand(M, H, seed=1).to(DEV), _rand(H, H, seed=2, scale=0.1).to(DEV), _rand(H, seed=3).to(DEV)
    res = torch.zeros(M, H, device=DEV)
    y0 = ops.linear_fwd(x, w, b, epilogue=N.EPI_BIAS_DROP_RES, residual=res, dropout_p=0.0, precision="fp32")
    y1 = ops.linear_fwd(x, w, b, epilogue=N.EPI_BIAS_DROP_RES, residual=res, dropout_p=p, seed=7, site=3, precision="fp32")
    keep = (y1 != 0)
    frac = keep.float().mean().item()
    assert abs(frac - (1 - p)) < 0.02, frac
    torch.testing.assert_close(y1[keep], (y0 / (1 - p))[keep], rtol=1e-5, atol=1e-6)
    y2 = ops.linear_fwd(x, w, b, epilogue=N.EPI_BIAS_DROP_RES, residual=res, dropout_p=p, seed=7, site=3, precision="fp32")
    assert torch.equal(y1, y2)  # same seed/site -> same mask
    y3 = ops.linear_fwd(x, w, b, epilogue=N.EPI_BIAS_DROP_RES, residual=res, dropout_p=p, seed=8, site=3, precision="fp32")
    assert not torch.equal(y1, y3)
    gamma = torch.ones(H, device=DEV)
    _, mean, rstd = ops.layernorm_fwd(y1, gamma, torch.zeros(H, device=DEV))
    dy = _rand(M, H, seed=5).to(DEV)
    dx, d_lin, *_ = ops.layernorm_bwd(dy, y1, mean, rstd, gamma, dropout_p=p, seed=7, site=3)
    torch.testing.assert_close(d_lin, dx * keep / (1 - p), rtol=1e-5, atol=1e-7)


SHAPES = [(100, 96, 32), (300, 128, 128), (513, 384, 128), (257, 128, 512), (64, 64, 64), (1000, 512, 128),
          # configs 4 / 5 (H = 256, I = 1024): QKV, FFN1, FFN2 / out-proj
          (300, 768, 256), (257, 1024, 256), (200, 256, 1024), (130, 256, 256),
          # the reference's default model (H = 384, I = 48): QKV, FFN1, FFN2 (K = 48: 32-deep slices + a 16-deep tail)
          (150, 1152, 384), (150, 48, 384), (150, 384, 48)]


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_linear_forward_epilogues(ops, prec, M, N, K):
    from xfmr_rec_amd import _native as Nn

    x, w, b, r = _rand(M, K, seed=1), _rand(N, K, seed=2, scale=K**-0.5), _rand(N, seed=3), _rand(M, N, seed=4)
    ref = x.double() @ w.double().T + b.double()
    y = ops.linear_fwd(x.to(DEV), w.to(DEV), b.to(DEV), precision=prec)
    assert_close("linear.bias", y, ref, prec)
    y, pre = ops.linear_fwd(x.to(DEV), w.to(DEV), b.to(DEV), epilogue=Nn.EPI_BIAS_GELU, precision=prec)
    assert_close("linear.gelu.pre", pre, ref, prec)
    assert_close("linear.gelu", y, F.gelu(ref), prec)
    y = ops.linear_fwd(x.to(DEV), w.to(DEV), b.to(DEV), epilogue=Nn.EPI_BIAS_DROP_RES, residual=r.to(DEV), precision=prec)
    assert_close("linear.residual", y, ref + r.double(), prec)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_linear_backward(ops, prec, M, N, K):
    dy, w, x = _rand(M, N, seed=1), _rand(N, K, seed=2, scale=N**-0.5), _rand(M, K, seed=3)
    rg, pre = _rand(M, K, seed=4), _rand(M, K, seed=5)
    ref_dx = dy.double() @ w.double()
    dx = ops.linear_bwd_dx(dy.to(DEV), w.to(DEV), precision=prec)
    assert_close("dx", dx, ref_dx, prec, "grad")
    dx = ops.linear_bwd_dx(dy.to(DEV), w.to(DEV), residual_grad=rg.to(DEV), precision=prec)
    assert_close("dx+res", dx, ref_dx + rg.double(), prec, "grad")
    pr = pre.clone().double().requires_grad_(True)
    F.gelu(pr).backward(ref_dx)
    dx = ops.linear_bwd_dx(dy.to(DEV), w.to(DEV), gelu_pre=pre.to(DEV), precision=prec)
    assert_close("dx*gelu'", dx, pr.grad, prec, "grad")
    dw = ops.linear_bwd_dw(dy.to(DEV), x.to(DEV), precision=prec)
    assert_close("dw", dw, dy.double().T @ x.double(), prec, "grad")
    assert_close("colsum", ops.colsum(dy.to(DEV)), dy.double().sum(0), "fp32", "grad")


def test_linear_bwd_dw_is_deterministic(ops):
    dy, x = _rand(5000, 128, seed=1).to(DEV), _rand(5000, 128, seed=2).to(DEV)
    a = ops.linear_bwd_dw(dy, x, precision="bf16")
    b = ops.linear_bwd_dw(dy, x, precision="bf16")
    assert torch.equal(a, b)  # split-K slabs are reduced in a fixed order (no float atomics)


def test_embed_gather_layernorm_and_param_grads(ops):
    B, L, H, V, Lmax = 3, 10, 64, 20, 12
    table = _rand(V + 1, H, seed=1)
    table[0] = 0
    table[7] = 0  # a non-padding id whose embedding is all zero: the mask follows the VALUES (models.py:343)
    idx = torch.randint(0, V + 1, (B, L), generator=torch.Generator().manual_seed(2))
    idx[0, 3] = 7
    pos, typ = _rand(Lmax, H, seed=3, scale=0.02), _rand(2, H, seed=4, scale=0.02)
    gamma, beta = 1 + 0.1 * _rand(H, seed=5), 0.1 * _rand(H, seed=6)
    out, pre, mean, rstd, mask = ops.embed_ln_fwd(idx.to(DEV), table.to(DEV), pos.to(DEV), typ.to(DEV), gamma.to(DEV), beta.to(DEV))
    e = F.embedding(idx, table)
    ref_pre = e + typ[0] + pos[:L]
    assert torch.equal(mask.cpu().bool(), (e != 0).any(-1))
    assert not mask[0, 3]
    torch.testing.assert_close(pre.cpu(), ref_pre, rtol=0, atol=0)
    assert_close("embed.ln", out, F.layer_norm(ref_pre.double(), (H,), gamma.double(), beta.double(), 1e-12), "fp32")
    d_pre = _rand(B, L, H, seed=7)
    d_pos, d_type = ops.embed_param_grads(d_pre.to(DEV), Lmax)
    ref_pos = torch.zeros(Lmax, H, dtype=torch.float64)
    ref_pos[:L] = d_pre.double().sum(0)
    assert_close("d_pos", d_pos, ref_pos, "fp32", "grad")
    assert_close("d_type0", d_type[0], d_pre.double().sum((0, 1)), "fp32", "grad")
    assert torch.count_nonzero(d_type[1]) == 0


def _attention_reference(qkv, key_mask, A, causal=True, keep=None):
    """fp64 restatement of eager attention (TF:modeling_bert.py:111-136) with the causal+padding mask (causal=False:
    the padding mask alone, BertConfig.is_decoder=False). `keep`: (B, A, L, L) tensor of keep * 1/(1-p) (0 or the scale;
    tests/dropout_model.py) -- attention-probability dropout where HF applies it, on the normalised probabilities."""
    B, L, H3 = qkv.shape
    H = H3 // 3
    dh = H // A
    q, k, v = (t.view(B, L, A, dh).transpose(1, 2) for t in qkv.split(H, dim=-1))
    scores = q @ k.transpose(2, 3) * dh**-0.5
    tri = torch.ones(L, L, dtype=torch.bool)
    allowed = (tri.tril() if causal else tri)[None] & key_mask.bool()[:, None, :]
    scores = scores.masked_fill(~allowed[:, None], float("-inf"))
    probs = torch.softmax(scores, dim=-1)
    probs = torch.nan_to_num(probs, nan=0.0)  # rows without any visible key -> zeros (documented)
    if keep is not None:
        probs = probs * keep.to(probs.dtype)
    return (probs @ v).transpose(1, 2).reshape(B, L, H)


@pytest.mark.parametrize("causal", [True, False], ids=["causal", "bidirectional"])
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("B,L,A,lengths", [(3, 12, 1, [12, 7, 1]), (2, 40, 2, [33, 40]), (2, 130, 2, [130, 77]),
                                           (2, 200, 4, [200, 150]), (1, 256, 1, [250]),
                                           # L > 256: the two-block forward and the two-kernel backward
                                           (2, 320, 2, [320, 301]), (1, 512, 1, [512])])
@pytest.mark.parametrize("dh", [32, 64])
def test_attention_fwd_bwd(ops, prec, B, L, A, lengths, causal, dh):
    """dh = 32: the production kernels (bf16) / the generic ones (fp32); dh = 64 (e.g. 384 / 6, 768 / 12): the generic
    kernels in both policies."""
    if prec == "fp32" and L > (256 if dh == 32 else 128):
        pytest.skip("fp32 parity policy: its kernels keep whole fp32 panels in LDS (L <= 256 at head size 32, <= 128 at "
                    "64); see DESIGN.md section 2")
    if dh == 64 and L > 256:
        pytest.skip("head size 64: the generic kernels keep whole panels in LDS (the dK/dV kernel's four: L <= 256 in bf16)")
    H = dh * A
    qkv = _rand(B, L, 3 * H, seed=3)
    mask = torch.zeros(B, L, dtype=torch.uint8)
    for b, n in enumerate(lengths):
        mask[b, :n] = 1
    if B > 1:
        mask[1, 2] = 0  # a hole in the middle: the kernels take an arbitrary key mask
    w = _rand(B, L, H, seed=4) * mask[..., None]  # the training path only back-propagates valid rows
    ref_in = qkv.clone().double().requires_grad_(True)
    ref = _attention_reference(ref_in, mask, A, causal)
    (ref * w.double()).sum().backward()
    ctx, lse = ops.attn_fwd(qkv.to(DEV), mask.to(DEV), A, precision=prec, causal=causal)
    valid = mask.bool()
    assert_close("attn.ctx", ctx.cpu()[valid], ref.detach()[valid], prec)
    d_qkv = ops.attn_bwd(qkv.to(DEV), mask.to(DEV), ctx, lse, w.to(DEV), A, precision=prec, causal=causal)
    assert_close("attn.d_qkv", d_qkv, ref_in.grad, prec, "grad")


def _bf16r(x):
    """fp64 -> (fp32 ->) bf16 -> fp64: the rounding the kernels apply to an fp32 value on its way into an MFMA operand."""
    return x.to(torch.float32).to(torch.bfloat16).to(torch.float64)


def _attention_bf16_emulation(qkv, key_mask, A, w, causal=True, keep=None, fwd=None):
    """fp64 arithmetic with the bf16 kernels' ROUNDING POINTS (attention.hip, head size 32): operands Q / K / V / dO are
    bf16 values (the caller passes bf16-representable inputs, so staging rounds nothing); forward = online softmax over
    32-key blocks, p = 2^(s c - m_running) rounded to bf16 as the P V operand while the row sum takes the unrounded p;
    backward: P = exp(s / sqrt(dh) - lse) from the forward's lse, bf16(P) into dV, dS = P (dP - delta) rounded to bf16
    into dQ and dK, delta = rowsum(dO * ctx) in full precision. What is left between this and the kernels is fp32
    accumulation order and the 1-ulp exp2 -- parity at the fp32 level (1e-4) for the kernels no fp32-policy run reaches
    (L > 256: the two-block forward and the dQ + dK/dV pair).
    `keep` ((B, A, L, L), keep * 1/(1-p)): dropout at the kernels' own points -- BEFORE each bf16 rounding, in fp32. Forward
    (attn_fwd_bf16_kernel): the P V operand is bf16(p * keep) with p the unnormalised 2^(s c - m_running), the row sum takes
    p without the mask. Backward (attn_bwd_dq_bf16_kernel, attn_bwd_dkv_bf16_kernel and the fused forms): the dV operand is
    bf16(P * keep), dS = bf16(P * (dP * keep - delta)) with dP = dO V^T unrounded; delta = rowsum(dO * ctx) of the dropped-out
    ctx.
    `fwd` = (ctx, lse) as the FORWARD KERNEL stored them ((B, L, H) and (B, A, L), fp32): the backward is then modelled from
    the backward kernels' own inputs and with the fp32 roundings of their exponent chain -- lse is an fp32 value in HBM,
    lse2 = fp32(lse * log2e), the argument is ONE fp32 fma(s, fp32(1/sqrt(32) * log2e), -lse2) of the fp32 score, P is an fp32
    value, P * keep an fp32 product before the bf16 rounding, and delta comes from the stored ctx. The fp64 form above places
    P up to ~1e-6 (relative) from the kernel's, this form ~1e-7 (the MFMA's accumulation order of s and the 1-ulp exp2 are
    left), so that many fewer probabilities fall on the other side of a bf16 rounding boundary than in the kernel. Only the
    chain up to P and the product P * keep are rounded to fp32: the kernels' other fp32 steps in front of the bf16 rounding of
    dS -- dP * keep, - delta, * P -- stay in fp64 here (the compiler may contract dP * keep - delta into one fma, so their
    rounding is not fixed by the source; at ~1e-7 of a sum of O(1) terms they sit well inside the 1e-4 of the comparison).
    Returns ctx, d_qkv and the model's own lse ((B, A, L), natural log), which a caller that passes `fwd` holds the kernel's to."""
    B, L, H3 = qkv.shape
    H = H3 // 3
    dh = H // A
    q, k, v = (t.double().view(B, L, A, dh).transpose(1, 2) for t in qkv.split(H, dim=-1))  # (B,A,L,dh)
    do = w.double().view(B, L, A, dh).transpose(1, 2)
    s = q @ k.transpose(2, 3)
    tri = torch.ones(L, L, dtype=torch.bool)
    vis = ((tri.tril() if causal else tri)[None] & key_mask.bool()[:, None, :])[:, None].expand(B, A, L, L)
    c = dh**-0.5 * 1.4426950408889634
    m = torch.full((B, A, L), -float("inf"), dtype=torch.float64)
    lsum = torch.zeros(B, A, L, dtype=torch.float64)
    o = torch.zeros(B, A, L, dh, dtype=torch.float64)
    for k0 in range(0, L, 32):
        sb = (s[..., k0:k0 + 32] * c).masked_fill(~vis[..., k0:k0 + 32], -float("inf"))
        mnew = torch.maximum(m, sb.max(dim=-1).values)
        msafe = torch.where(torch.isinf(mnew), torch.zeros_like(mnew), mnew)
        alpha = torch.exp2(m - msafe)
        p = torch.exp2(sb - msafe[..., None])
        lsum = lsum * alpha + p.sum(-1)
        pk = p if keep is None else p * keep[..., k0:k0 + 32].double()
        o = o * alpha[..., None] + _bf16r(pk) @ v[:, :, k0:k0 + 32]
        m = mnew
    ctx = o / lsum.clamp(min=1e-300)[..., None]
    ctx = torch.where((lsum > 0)[..., None], ctx, torch.zeros_like(ctx))
    lse = (m + torch.log2(lsum)) * 0.6931471805599453  # natural log, as the kernel stores it
    f32 = lambda t: t.to(torch.float32).double()  # noqa: E731  (one fp32 rounding of an fp64 value)
    if fwd is None:
        pr = torch.exp(s * dh**-0.5 - lse[..., None]).masked_fill(~vis, 0.0)
        pr = torch.nan_to_num(pr, nan=0.0)
        ctx_b = ctx
    else:
        assert dh == 32
        ctx_k, lse_k = (t.detach().cpu() for t in fwd)
        sc32 = float(torch.tensor(0.17677669529663687, dtype=torch.float32) * torch.tensor(1.4426950408889634, dtype=torch.float32))
        lse2 = (lse_k.to(torch.float32) * torch.tensor(1.4426950408889634, dtype=torch.float32)).double()  # fp32 product
        arg = f32(f32(s) * sc32 - lse2[..., None])  # fma: the product of two fp32 values is exact in fp64, one rounding
        pr = f32(torch.exp2(arg)).masked_fill(~vis, 0.0)
        pr = torch.nan_to_num(pr, nan=0.0)
        ctx_b = ctx_k.double().view(B, L, A, dh).transpose(1, 2)
    dp = do @ v.transpose(2, 3)
    delta = (do * ctx_b).sum(-1, keepdim=True)
    if keep is not None:
        dp = dp * keep.double()
    ds = _bf16r(pr * (dp - delta))
    pd = pr  # P.D, the dV operand
    if keep is not None:
        pd = pr * keep.double()
        if fwd is not None:
            pd = f32(pd)  # the kernel's fp32 product of the fp32 P and the fp32 scale
    dv = _bf16r(pd).transpose(2, 3) @ do
    dq = (ds @ k) * dh**-0.5
    dk = (ds.transpose(2, 3) @ q) * dh**-0.5
    back = lambda t: t.transpose(1, 2).reshape(B, L, H)  # noqa: E731
    return back(ctx), torch.cat([back(dq), back(dk), back(dv)], dim=-1), lse


def fp32_level(name, got, want):
    """rel-L2 <= 1e-4 over the tensor, and all but a handful of elements within 1e-4 * max(1, |x|). A probability that
    lies within fp32 rounding (~1e-6 relative: the exponent's argument) of a bf16 rounding boundary lands on the other
    side of it in the kernel than in the fp64 model -- a 2^-8 relative step of ONE probability, which a row with few
    visible keys passes on almost undiluted (measured: 1.5-2.1e-4 on one or two elements of 51 200). The count-based
    limit tolerates those; a slip in a tile's indexing moves whole 32 x 32 tiles and fails both."""
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    assert rel_l2(got, want) <= 1e-4, (name, rel_l2(got, want))
    off = ((got - want).abs() > 1e-4 * want.abs().clamp(min=1.0)).double().mean().item()
    assert off <= 2e-3, (name, off)
    assert_close(name, got, want, "bf16")  # and nothing beyond the bf16 limit anywhere
    return rel_l2(got, want), off


@pytest.mark.parametrize("causal", [True, False], ids=["causal", "bidirectional"])
@pytest.mark.parametrize("B,L,A,lengths", [(1, 512, 2, [512]), (2, 320, 2, [320, 301]), (2, 200, 4, [200, 150])])
def test_bf16_attention_kernels_at_fp32_level_against_their_rounding_model(ops, B, L, A, lengths, causal):
    """BASELINE config 5's L = 512 attention (and 320; 200 = the fused one-workgroup kernels, for comparison) in the bf16
    policy, at the FP32 level (rel-L2 1e-4; element-wise 1e-4 but for a handful of rounding-boundary cases), against the fp64 model of the kernels' own
    rounding points on bf16-representable inputs. test_attention_fwd_bwd holds these shapes to the exact fp64 attention
    at the bf16 tolerance (3e-2): an indexing slip worth 1 % would pass there, not here."""
    H = 32 * A
    qkv = _rand(B, L, 3 * H, seed=13).to(torch.bfloat16).float()
    mask = torch.zeros(B, L, dtype=torch.uint8)
    for b, n in enumerate(lengths):
        mask[b, :n] = 1
    if B > 1:
        mask[1, 2] = 0
    w = (_rand(B, L, H, seed=14) * mask[..., None]).to(torch.bfloat16).float()
    ctx, lse = ops.attn_fwd(qkv.to(DEV), mask.to(DEV), A, precision="bf16", causal=causal)
    want_ctx, want_d, _lse_m = _attention_bf16_emulation(qkv, mask, A, w, causal)
    valid = mask.bool()

    fp32_level("attn.ctx", ctx.cpu()[valid], want_ctx[valid])
    # the backward under test reads the FORWARD KERNEL's ctx / lse; the model used its own (equal to 1e-4 by the line above)
    d_qkv = ops.attn_bwd(qkv.to(DEV), mask.to(DEV), ctx, lse, w.to(DEV), A, precision="bf16", causal=causal)
    fp32_level("attn.d_qkv", d_qkv, want_d)
    for name, sl in (("dq", slice(0, H)), ("dk", slice(H, 2 * H)), ("dv", slice(2 * H, 3 * H))):
        fp32_level(f"attn.{name}", d_qkv[..., sl], want_d[..., sl])


@pytest.mark.parametrize("B,L,A,lengths", [(2, 200, 4, [200, 150]), (3, 130, 2, [130, 77, 1]), (1, 256, 1, [250]), (2, 40, 2, [33, 40])])
def test_attention_backward_roles_form_equals_the_lockstep_form(ops, monkeypatch, B, L, A, lengths):
    """XFMR_ATTN_BWD_FORM=roles (attention.hip: attn_bwd_roles_bf16_kernel -- one workgroup per (batch, head), eight waves:
    four own key tiles for dK / dV, four own query tiles for dQ, every probability evaluated by both; an experiment that
    measured no faster than the lock-step form and is not the default) against the default form: the same products, the
    tiles added in ascending order instead of the lock-step schedule's (fp32 summation order: 1e-6), dropout on. And
    against the fp64 rounding model like the other kernels."""
    H = 32 * A
    qkv = _rand(B, L, 3 * H, seed=21).to(torch.bfloat16).float()
    mask = torch.zeros(B, L, dtype=torch.uint8)
    for b, n in enumerate(lengths):
        mask[b, :n] = 1
    if B > 1:
        mask[1, 2] = 0
    w = (_rand(B, L, H, seed=22) * mask[..., None]).to(torch.bfloat16).float()
    kw = dict(dropout_p=0.2, seed=5, site=1, precision="bf16")
    ctx, lse = ops.attn_fwd(qkv.to(DEV), mask.to(DEV), A, **kw)
    monkeypatch.delenv("XFMR_ATTN_BWD_FORM", raising=False)
    d0 = ops.attn_bwd(qkv.to(DEV), mask.to(DEV), ctx, lse, w.to(DEV), A, **kw)
    monkeypatch.setenv("XFMR_ATTN_BWD_FORM", "roles")
    d1 = ops.attn_bwd(qkv.to(DEV), mask.to(DEV), ctx, lse, w.to(DEV), A, **kw)
    d1b = ops.attn_bwd(qkv.to(DEV), mask.to(DEV), ctx, lse, w.to(DEV), A, **kw)
    assert torch.equal(d1, d1b)  # bit-reproducible
    for name, sl in (("dq", slice(0, H)), ("dk", slice(H, 2 * H)), ("dv", slice(2 * H, 3 * H))):
        assert rel_l2(d1[..., sl], d0[..., sl]) <= 2e-5, name  # (fp32 order of up to 7 tile sums of bf16-rounded products)
    # without dropout: the rounding model of the bf16 kernels
    ctx0, lse0 = ops.attn_fwd(qkv.to(DEV), mask.to(DEV), A, precision="bf16")
    d2 = ops.attn_bwd(qkv.to(DEV), mask.to(DEV), ctx0, lse0, w.to(DEV), A, precision="bf16")
    _ctx_m, want_d, _lse_m = _attention_bf16_emulation(qkv, mask, A, w, True)
    assert rel_l2(d2, want_d) <= 1e-4


def test_attention_causality_and_padding_invariance(ops):
    """Changing a later key/value or a masked key never changes an earlier / any output."""
    B, L, A = 1, 96, 2
    H = 32 * A
    qkv = _rand(B, L, 3 * H, seed=1).to(DEV)
    mask = torch.ones(B, L, dtype=torch.uint8, device=DEV)
    mask[0, 50] = 0
    base, _ = ops.attn_fwd(qkv, mask, A, precision="fp32")
    q2 = qkv.clone()
    q2[0, 70:, H:] += 1.0  # keys and values of positions >= 70
    out2, _ = ops.attn_fwd(q2, mask, A, precision="fp32")
    assert torch.equal(base[0, :70], out2[0, :70])
    q3 = qkv.clone()
    q3[0, 50, H:] += 5.0  # the masked key
    out3, _ = ops.attn_fwd(q3, mask, A, precision="fp32")
    keep = torch.ones(L, dtype=torch.bool, device=DEV)
    assert torch.equal(base[0, keep], out3[0, keep])


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_bidirectional_attention_sees_later_keys_but_never_masked_ones(ops, prec):
    """XFMR_ATTN_BIDIRECTIONAL (BertConfig.is_decoder=False): a later key changes EVERY query's output (first and
    second 128-row block alike), a masked key changes none; the causal entry point and mode 0 are the same kernels."""
    B, L, A = 1, 160, 2
    H = 32 * A
    qkv = _rand(B, L, 3 * H, seed=1).to(DEV)
    mask = torch.ones(B, L, dtype=torch.uint8, device=DEV)
    mask[0, 50] = 0
    base, lse = ops.attn_fwd(qkv, mask, A, precision=prec, causal=False)
    q2 = qkv.clone()
    q2[0, 150, H:] += 1.0
    out2, _ = ops.attn_fwd(q2, mask, A, precision=prec, causal=False)
    changed = (base[0] != out2[0]).any(-1)
    assert bool(changed.all())
    q3 = qkv.clone()
    q3[0, 50, H:] += 5.0
    out3, _ = ops.attn_fwd(q3, mask, A, precision=prec, causal=False)
    assert torch.equal(base, out3)
    causal_out, _ = ops.attn_fwd(qkv, mask, A, precision=prec)
    # the last query sees the same key set either way
    assert_close("last row", base[0, -1].cpu(), causal_out[0, -1].cpu(), prec)
    assert not torch.allclose(base[0, :100], causal_out[0, :100])
    import ctypes as C

    from xfmr_rec_amd import _native as N

    ctx, lse2 = torch.empty_like(base), torch.empty_like(lse)
    rc = N.load().xfmr_attn_fwd_mode(N.ptr(qkv), N.ptr(mask), N.ptr(ctx), N.ptr(lse2), B, L, A, H, 0.0, 0, 0,
                                     N.precision_id(prec), N.ATTN_CAUSAL, N.stream())
    assert rc == 0 and torch.equal(ctx, causal_out)
    rc = N.load().xfmr_attn_fwd_mode(N.ptr(qkv), N.ptr(mask), N.ptr(ctx), N.ptr(lse2), B, L, A, H, 0.0, 0, 0,
                                     N.precision_id(prec), 7, N.stream())
    assert rc == -1  # XFMR_EINVAL: unknown attn_mode


@pytest.mark.parametrize("causal", [True, False], ids=["causal", "bidirectional"])
def test_attention_dropout_forward_backward_agree(ops, causal):
    """With dropout on, backward must differentiate the SAME masked forward: check by finite differences."""
    B, L, A = 1, 40, 1
    H = 32
    qkv = _rand(B, L, 3 * H, seed=1).to(DEV)
    mask = torch.ones(B, L, dtype=torch.uint8, device=DEV)
    w = _rand(B, L, H, seed=2).to(DEV)
    kw = dict(dropout_p=0.3, seed=11, site=5, precision="fp32", causal=causal)
    ctx, lse = ops.attn_fwd(qkv, mask, A, **kw)
    d = ops.attn_bwd(qkv, mask, ctx, lse, w, A, **kw)
    direction = _rand(B, L, 3 * H, seed=3).to(DEV)
    eps = 1e-2
    fp = (ops.attn_fwd(qkv + eps * direction, mask, A, **kw)[0] * w).sum().item()
    fm = (ops.attn_fwd(qkv - eps * direction, mask, A, **kw)[0] * w).sum().item()
    fd = (fp - fm) / (2 * eps)
    an = (d * direction).sum().item()
    assert abs(fd - an) <= 2e-2 * max(1.0, abs(an)), (fd, an)
    ctx0, _ = ops.attn_fwd(qkv, mask, A, precision="fp32", causal=causal)
    assert not torch.allclose(ctx, ctx0)  # dropout really changed the output


@pytest.mark.parametrize("causal", [True, False], ids=["causal", "bidirectional"])
@pytest.mark.parametrize("B,L,A", [(2, 200, 2), (1, 96, 1)])
def test_attention_dropout_mask_is_shared_by_all_kernels(ops, B, L, A, causal):
    """The dropout decision is a function of (seed, site, query row, key column) only: the bf16 kernels (forward,
    dQ, dK/dV -- interior and diagonal tiles, row keys staged in LDS) must apply the mask the fp32 kernels apply,
    whose forward / backward agreement the finite-difference test above checks."""
    H = 32 * A
    qkv = _rand(B, L, 3 * H, seed=5).to(DEV)
    mask = torch.ones(B, L, dtype=torch.uint8, device=DEV)
    mask[0, L - 9:] = 0
    w = (_rand(B, L, H, seed=6).to(DEV)) * mask[..., None]
    kw = dict(dropout_p=0.25, seed=3, site=2, causal=causal)
    ctx32, lse32 = ops.attn_fwd(qkv, mask, A, precision="fp32", **kw)
    d32 = ops.attn_bwd(qkv, mask, ctx32, lse32, w, A, precision="fp32", **kw)
    ctx16, lse16 = ops.attn_fwd(qkv, mask, A, precision="bf16", **kw)
    d16 = ops.attn_bwd(qkv, mask, ctx16, lse16, w, A, precision="bf16", **kw)
    valid = mask.bool()
    assert_close("attn.ctx (dropout)", ctx16[valid].cpu(), ctx32[valid].cpu(), "bf16")
    assert_close("attn.d_qkv (dropout)", d16.cpu(), d32.cpu(), "bf16", "grad")
    # another site (= layer) draws another mask
    ctx_other, _ = ops.attn_fwd(qkv, mask, A, precision="bf16", **(kw | {"site": 3}))
    assert not torch.allclose(ctx_other, ctx16)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_attention_dropout_keep_rate(ops, prec):
    """q = k = 0 makes the causal softmax uniform and v = 1 turns ctx[q] into (kept keys of row q) / ((q+1)(1-p)):
    the kept fraction over all (row, key) pairs must be 1 - p within sampling error, per head and overall."""
    B, L, A, p = 16, 200, 4, 0.1
    H = 32 * A
    qkv = torch.zeros(B, L, 3 * H, device=DEV)
    qkv[..., 2 * H:] = 1.0
    mask = torch.ones(B, L, dtype=torch.uint8, device=DEV)
    ctx, _ = ops.attn_fwd(qkv, mask, A, dropout_p=p, seed=1234, site=1, precision=prec)
    rows = torch.arange(1, L + 1, device=DEV, dtype=torch.float32)
    kept = ctx.view(B, L, A, 32)[..., 0] * rows[None, :, None] * (1 - p)  # (B, L, A) kept keys per row
    total = B * A * L * (L + 1) / 2
    rate = float(kept.sum()) / total
    sigma = (p * (1 - p) / total) ** 0.5
    assert abs(rate - (1 - p)) <= 5 * sigma + 2e-3 * (prec == "bf16"), (rate, sigma)
    per_head = kept.sum(dim=(0, 1)) / (total / A)
    assert float((per_head - (1 - p)).abs().max()) <= 5 * sigma * A**0.5 + 2e-3 * (prec == "bf16")
    # per-key-column and per-row keep rates show no structure (columns 0..L-1 are seen by L-col rows each)
    assert float(kept[:, -1, :].mean()) / L == pytest.approx(1 - p, abs=0.02)


def test_multi_segment_row_reduction(ops):
    """xf_multi_rowsum (one launch reduces every split-K slab, bias partial and LayerNorm partial record of the encoder
    backward): tall strided segments (the LayerNorm records: 1600 x 128 out of a [1600][3][128] buffer), wide short ones
    (weight slabs), a segment whose width is not a multiple of 4 (one-column form), fewer rows than row groups -- against
    fp64 sums, and bit-for-bit equal over repeated launches."""
    from xfmr_rec_amd import _native as N

    g = torch.Generator().manual_seed(0)
    rec = torch.randn(1600, 3, 128, generator=g).to(DEV)           # LayerNorm partial records
    slab = torch.randn(62, 4096, generator=g).to(DEV)               # split-K slabs
    odd = torch.randn(37, 6, generator=g).to(DEV)                   # cols % 4 != 0
    few = torch.randn(3, 256, generator=g).to(DEV)                  # rows < 16
    tall = torch.randn(1000, 64, generator=g).to(DEV)               # a partial last round (1000 = 3 * 256 + 232)
    cases = [(rec[:, 0], 1600, 128, 384), (rec[:, 1], 1600, 128, 384), (rec[:, 2], 1600, 128, 384),
             (slab, 62, 4096, 4096), (odd, 37, 6, 6), (few, 3, 256, 256), (tall, 1000, 64, 64)]
    outs = [torch.full((c,), float("nan"), device=DEV) for _, _, c, _ in cases]
    segs = (N.ReduceSeg * len(cases))()
    for i, ((src, rows, cols, ld), dst) in enumerate(zip(cases, outs)):
        segs[i] = N.ReduceSeg(src.data_ptr(), dst.data_ptr(), rows, cols, ld, 0)
    fn = N.load().xf_multi_rowsum
    assert fn(segs, len(cases), N.stream()) == 0
    torch.cuda.synchronize()
    first = [o.clone() for o in outs]
    for (src, rows, cols, ld), o in zip(cases, outs):
        torch.testing.assert_close(o.double(), src.double().sum(0), rtol=1e-5, atol=2e-4)
    assert fn(segs, len(cases), N.stream()) == 0
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(first, outs))


def test_hidden_dropout_keep_rate_and_structure(ops):
    """Hidden-state dropout (the Linear + dropout + residual epilogues, the LayerNorm kernels) decides from a hash of the
    ROW spent once per row and one xor-multiply per element (common.h: xf_drop4). x = 0, bias = 1, residual = 0 makes
    the output of the epilogue the mask itself times 1/(1-p): the keep rate must be 1 - p overall, per row and per column
    within sampling error, neighbouring elements / rows uncorrelated, and another site or seed another mask."""
    from xfmr_rec_amd import _native as N

    M, K, Nn, p = 8192, 64, 128, 0.1
    x = torch.zeros(M, K, device=DEV)
    w = torch.zeros(Nn, K, device=DEV)
    b = torch.ones(Nn, device=DEV)
    res = torch.zeros(M, Nn, device=DEV)

    def mask(seed, site):
        y = ops.linear_fwd(x, w, b, epilogue=N.EPI_BIAS_DROP_RES, residual=res, dropout_p=p, seed=seed, site=site,
                           precision="bf16")
        assert bool(((y == 0) | ((y - 1 / (1 - p)).abs() < 1e-6)).all())
        return (y != 0).float()

    m = mask(7, 3)
    n = m.numel()
    sigma = (p * (1 - p) / n) ** 0.5
    assert abs(float(m.mean()) - (1 - p)) <= 5 * sigma
    assert float((m.mean(1) - (1 - p)).abs().max()) <= 6 * (p * (1 - p) / Nn) ** 0.5   # per row (128 samples each)
    assert float((m.mean(0) - (1 - p)).abs().max()) <= 6 * (p * (1 - p) / M) ** 0.5    # per column
    c = m - m.mean()
    var = float((c * c).mean())
    for shifted in (torch.roll(c, 1, 1), torch.roll(c, 1, 0), torch.roll(c, 4, 1), torch.roll(torch.roll(c, 1, 0), 1, 1)):
        assert abs(float((c * shifted).mean()) / var) <= 6 / n ** 0.5  # lag-1 / lag-4 / diagonal correlations
    for other in (mask(7, 4), mask(8, 3)):
        agree = float((other == m).float().mean())
        assert abs(agree - ((1 - p) ** 2 + p * p)) <= 6 * 0.4 / n ** 0.5  # independent masks agree at (1-p)^2 + p^2
    assert torch.equal(mask(7, 3), m)


# K = 96: not a multiple of 64 -> 32-deep K slices, whose operand images are SMALLER than the epilogue's scratch strips
# plus exchange records (the LDS allocation must be sized by the epilogue there)
@pytest.mark.parametrize("K,M,p_drop", [(128, 300, 0.0), (512, 1000, 0.0), (128, 4096 + 17, 0.2), (96, 1000, 0.1)])
@pytest.mark.parametrize("bf16_storage", [False, True])
def test_linear_with_layernorm_in_the_epilogue(ops, K, M, p_drop, bf16_storage):
    """xf_linear_ln_fwd_ex (internal entry point of the encoder forward at T >= 16 384: out-proj / FFN2 Linear +
    bias + dropout + residual + LayerNorm in ONE kernel) against the two-kernel form it replaces: same pre-LayerNorm
    sum bit for bit (same GEMM arithmetic, same dropout mask), LayerNorm output / mean / rstd to fp32 rounding, and the
    bf16 copy = the rounded fp32 output. Partial last tile (M not a multiple of 64) included."""
    from xfmr_rec_amd import _native as N

    lib = N.load()
    Nn = 128
    g = torch.Generator().manual_seed(K + M)
    x = torch.randn(M, K, generator=g).to(DEV)
    w = (torch.randn(Nn, K, generator=g) * 0.05).to(DEV)
    b = torch.randn(Nn, generator=g).to(DEV)
    res = torch.randn(M, Nn, generator=g).to(DEV)
    gamma = (1 + 0.1 * torch.randn(Nn, generator=g)).to(DEV)
    beta = (0.1 * torch.randn(Nn, generator=g)).to(DEV)
    # reference: the public two-kernel path (bf16 MFMA policy)
    pre_ref = ops.linear_fwd(x, w, b, epilogue=N.EPI_BIAS_DROP_RES, residual=res, dropout_p=p_drop, seed=5, site=9,
                             precision="bf16")
    y_ref, mean_ref, rstd_ref = ops.layernorm_fwd(pre_ref, gamma, beta)
    xs, ws, s16 = x, w, 0
    if bf16_storage:  # the encoder's storage: bf16 A and B operands (identical products)
        xs, ws, s16 = x.to(torch.bfloat16), w.to(torch.bfloat16), 3
        pre_ref = ops.linear_fwd(xs.float(), ws.float(), b, epilogue=N.EPI_BIAS_DROP_RES, residual=res,
                                 dropout_p=p_drop, seed=5, site=9, precision="bf16")
        y_ref, mean_ref, rstd_ref = ops.layernorm_fwd(pre_ref, gamma, beta)
    pre = torch.empty(M, Nn, device=DEV)
    y = torch.empty(M, Nn, device=DEV)
    y16 = torch.empty(M, Nn, device=DEV, dtype=torch.bfloat16)
    mean = torch.empty(M, device=DEV)
    rstd = torch.empty(M, device=DEV)
    fn = lib.xf_linear_ln_fwd_ex
    rc = fn(N.ptr(xs), N.ptr(ws), N.ptr(b), N.ptr(pre), M, Nn, K, N.ptr(res), p_drop, 5, 9, N.ptr(gamma), N.ptr(beta),
            1e-12, N.ptr(y), N.ptr(y16), N.ptr(mean), N.ptr(rstd), N.precision_id("bf16"), s16, N.stream())
    assert rc == 0, rc
    assert torch.equal(pre, pre_ref)
    torch.testing.assert_close(mean, mean_ref, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(rstd, rstd_ref, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(y, y_ref, rtol=1e-5, atol=2e-6)
    assert torch.equal(y16, y.to(torch.bfloat16))
    # and against fp64 with the host model's mask (dropout_model.py), not only against the sibling kernels: bf16 operands (the
    # MFMA policy rounds fp32 storage on its way in), (acc + bias) * keep / (1 - p) + residual, then the LayerNorm. What is
    # left is fp32 accumulation over K <= 512 products of O(1) sums and the hardware rsqrt (1 ulp): the limits of
    # test_ffn_forward_in_one_kernel_vs_the_two_gemm_form's restatement.
    import dropout_model as dm

    ks = torch.from_numpy(dm.hidden_keep(5, 9, M, Nn, p_drop).astype("float64") * dm.scale(p_drop)).to(DEV)
    xr, wr = x.to(torch.bfloat16).double(), w.to(torch.bfloat16).double()
    pre64 = ks * (xr @ wr.T + b.double()) + res.double()
    torch.testing.assert_close(pre.double(), pre64, rtol=2e-5, atol=2e-5)
    if p_drop > 0:
        assert torch.equal(pre == res, ks == 0)  # dropped: the residual alone, bit for bit
    ln64 = torch.nn.functional.layer_norm(pre64, (Nn,), gamma.double(), beta.double(), 1e-12)
    torch.testing.assert_close(y.double(), ln64, rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(mean.double(), pre64.mean(-1), rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(rstd.double(), (pre64.var(-1, unbiased=False) + 1e-12).rsqrt(), rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("chunk", ["64", "128"])
@pytest.mark.parametrize("M,I,p_drop", [(300, 512, 0.0), (4096 + 17, 512, 0.2), (1000, 128, 0.1), (102400, 512, 0.1)])
def test_ffn_forward_in_one_kernel_vs_the_two_gemm_form(ops, M, I, p_drop, chunk, monkeypatch):
    """xf_ffn_fwd_fused_ex (FFN1 -> GELU -> FFN2 -> dropout + residual + LayerNorm, TF:modeling_bert.py:325-351, in one
    kernel; the encoder forward's path at T >= 16 384, H = 128) against the two launches it replaces
    (xf_linear_fwd_ex with the GELU epilogue, xf_linear_ln_fwd_ex). The only arithmetic difference: the fused kernel
    rounds the pre-activation u to bf16 before the GELU (as bf16 autocast holds it) and saves u where the two-kernel form
    saves gelu'(u) -- so g agrees to a bf16 ulp (+ gelu's slope times an ulp of u), gelu'(u) evaluated from the saved u
    agrees with the saved gelu', and everything downstream agrees to bf16 rounding noise; against an fp64 restatement of
    the fused kernel's own rounding points the pre-LayerNorm sum agrees to fp32 accumulation error. Partial last tile,
    dropout, the benchmark's row count, and both chunk widths (XFMR_FFN_CHUNK, read per call)."""
    from xfmr_rec_amd import _native as N

    lib = N.load()
    H = 128
    g = torch.Generator().manual_seed(M + I)
    x16 = torch.randn(M, H, generator=g).to(DEV).to(torch.bfloat16)
    w1 = (torch.randn(I, H, generator=g) * 0.08).to(DEV).to(torch.bfloat16)
    b1 = (0.1 * torch.randn(I, generator=g)).to(DEV)
    w2 = (torch.randn(H, I, generator=g) * 0.05).to(DEV).to(torch.bfloat16)
    b2 = (0.1 * torch.randn(H, generator=g)).to(DEV)
    res = torch.randn(M, H, generator=g).to(DEV)
    gamma = (1 + 0.1 * torch.randn(H, generator=g)).to(DEV)
    beta = (0.1 * torch.randn(H, generator=g)).to(DEV)

    def outs():
        return dict(g=torch.empty(M, I, device=DEV, dtype=torch.bfloat16), d=torch.empty(M, I, device=DEV, dtype=torch.bfloat16),  # d: gelu' (two-kernel form) / u (fused)
                    pre=torch.empty(M, H, device=DEV), y=torch.empty(M, H, device=DEV),
                    y16=torch.empty(M, H, device=DEV, dtype=torch.bfloat16), mean=torch.empty(M, device=DEV),
                    rstd=torch.empty(M, device=DEV))

    # the two-kernel form, with the encoder's storage masks (bf16 A, B, C; gelu' as the auxiliary output)
    ref = outs()
    f1 = lib.xf_linear_fwd_ex
    rc = f1(N.ptr(x16), N.ptr(w1), N.ptr(b1), N.ptr(ref["g"]), M, I, H, N.EPI_BIAS_GELU, None, N.ptr(ref["d"]), 0.0, 0, 0,
            N.precision_id("bf16"), 1 | 2 | 4 | 0x100, N.stream())
    assert rc == 0, rc
    f2 = lib.xf_linear_ln_fwd_ex
    rc = f2(N.ptr(ref["g"]), N.ptr(w2), N.ptr(b2), N.ptr(ref["pre"]), M, H, I, N.ptr(res), p_drop, 5, 9, N.ptr(gamma),
            N.ptr(beta), 1e-12, N.ptr(ref["y"]), N.ptr(ref["y16"]), N.ptr(ref["mean"]), N.ptr(ref["rstd"]),
            N.precision_id("bf16"), 3, N.stream())
    assert rc == 0, rc

    monkeypatch.setenv("XFMR_FFN_CHUNK", chunk)  # read per call
    fn = lib.xf_ffn_fwd_fused_ex

    def run():
        o = outs()
        rc = fn(N.ptr(x16), N.ptr(w1), N.ptr(b1), N.ptr(w2), N.ptr(b2), N.ptr(o["d"]), N.ptr(o["g"]), N.ptr(o["pre"]), M, H,
                I, N.ptr(res), p_drop, 5, 9, N.ptr(gamma), N.ptr(beta), 1e-12, N.ptr(o["y"]), N.ptr(o["y16"]),
                N.ptr(o["mean"]), N.ptr(o["rstd"]), N.stream())
        assert rc == 0, rc
        return o

    got = run()
    # g, and gelu' of the saved u against the saved gelu': a bf16 ulp of each other
    u = got["d"].double()
    gelu_grad = 0.5 * (1 + torch.erf(u / 2 ** 0.5)) + u * torch.exp(-u * u / 2) / (2 * torch.pi) ** 0.5
    for k, a, b in (("g", got["g"].float(), ref["g"].float()), ("gelu'", gelu_grad.float(), ref["d"].float())):
        # two roundings (u, then the value) against one: a bf16 ulp of the value plus gelu's slope times a bf16 ulp of u
        assert bool(((a - b).abs() <= 2.0 ** -6 * b.abs() + 4e-3).all()), k
        assert rel_l2(a, b) <= 5e-3, k
    assert rel_l2(got["pre"], ref["pre"]) <= 2e-3 and rel_l2(got["y"], ref["y"]) <= 2e-3
    assert torch.equal(got["y16"], got["y"].to(torch.bfloat16))
    # the fused kernel's own rounding points, restated in fp64, the dropout mask from the host model (dropout_model.py): the
    # kernel scales (acc + bias) in fp32, then adds the residual. (The benchmark's row count is left to the comparisons above:
    # M = 4113 has the partial tile, and 13 M fp64 products per chunk width are not worth their seconds.)
    if M <= 8192:
        import dropout_model as dm

        ks = torch.from_numpy(dm.hidden_keep(5, 9, M, H, p_drop).astype("float64") * dm.scale(p_drop)).to(DEV)
        u = (x16.double() @ w1.double().T + b1.double()).to(torch.bfloat16)
        assert int((u != got["d"]).sum()) <= 2e-3 * u.numel()
        gg = torch.nn.functional.gelu(u.double()).to(torch.bfloat16)
        n_off = int((gg != got["g"]).sum())  # fp32-vs-fp64 accumulation flips a bf16 rounding now and then
        assert n_off <= 2e-3 * gg.numel(), n_off
        pre = ks * (got["g"].double() @ w2.double().T + b2.double()) + res.double()
        torch.testing.assert_close(got["pre"].double(), pre, rtol=2e-5, atol=2e-5)
        ln = torch.nn.functional.layer_norm(pre, (H,), gamma.double(), beta.double(), 1e-12)
        torch.testing.assert_close(got["y"].double(), ln, rtol=1e-4, atol=1e-4)
        torch.testing.assert_close(got["mean"].double(), pre.mean(-1), rtol=1e-5, atol=1e-5)
    again = run()  # no atomics, fixed reduction orders: bit-reproducible
    assert all(torch.equal(got[k], again[k]) for k in got)
    # arguments the kernel is not built for fail loudly
    bad = fn(N.ptr(x16), N.ptr(w1), N.ptr(b1), N.ptr(w2), N.ptr(b2), None, None, N.ptr(got["pre"]), M, H, 96, N.ptr(res), 0.0,
             0, 0, N.ptr(gamma), N.ptr(beta), 1e-12, N.ptr(got["y"]), None, N.ptr(got["mean"]), N.ptr(got["rstd"]), N.stream())
    assert bad == -2  # XFMR_EUNSUPPORTED


@pytest.mark.parametrize("Nn,p_drop", [(512, 0.1), (384, 0.0)])  # FFN1 dX (+ LayerNorm 1) / QKV dX (+ LayerNorm 2)
def test_dx_gemm_with_layernorm_backward_epilogue_vs_separate_kernels_and_bit_reproducible(ops, Nn, p_drop):
    """xf_linear_bwd_dx_lnbwd_ex (the dX GEMM whose epilogue applies the LayerNorm backward of the row it produces)
    against the two-kernel form, at the benchmark's row count, and bit-for-bit equal over repeated launches. Builds of
    this epilogue that contained packed-fp32 `op_sel` broadcasts returned 1-5 wrong rows of 102 400 in most launches
    (scripts/probe/lnbwd_determinism.py is the long form of this test)."""
    import ctypes as C

    from xfmr_rec_amd import _native as N

    lib = N.load()
    M, K = 102400, 128
    g = torch.Generator().manual_seed(Nn)
    dy = torch.randn(M, Nn, generator=g).to(DEV).to(torch.bfloat16)
    w = (torch.randn(Nn, K, generator=g) * 0.05).to(DEV).to(torch.bfloat16)
    rg = torch.randn(M, K, generator=g).to(DEV)
    lnx = torch.randn(M, K, generator=g).to(DEV)
    mean = lnx.mean(-1).contiguous()
    rstd = (lnx.var(-1, unbiased=False) + 1e-12).rsqrt().contiguous()
    gamma = (1 + 0.1 * torch.randn(K, generator=g)).to(DEV)
    fn = lib.xf_linear_bwd_dx_lnbwd_ex

    # row tiles = LayerNorm partial records: (M + 63) / 64, or more when the last round is dealt as short tiles
    n_tiles = lib.xf_ln_row_tiles(M)
    assert n_tiles >= (M + 63) // 64

    def run():
        dx = torch.empty(M, K, device=DEV)
        d16 = torch.empty(M, K, device=DEV, dtype=torch.bfloat16)
        parts = torch.zeros(n_tiles, 3, K, device=DEV)
        blocks = C.c_int(0)
        rc = fn(N.ptr(dy), N.ptr(w), M, Nn, K, N.ptr(rg), N.ptr(lnx), N.ptr(mean), N.ptr(rstd), N.ptr(gamma), p_drop, 5,
                9, N.ptr(dx), N.ptr(d16), N.ptr(parts), C.byref(blocks), N.precision_id("bf16"), 3, N.stream(), 0.0, 0)
        assert rc == 0 and blocks.value == n_tiles
        return dx, d16, parts

    dx, d16, parts = run()
    # the separate kernels: dX GEMM (+ residual gradient), then the LayerNorm backward kernel with the same dropout
    dpre = ops.linear_bwd_dx(dy.float(), w.float(), residual_grad=rg, precision="bf16")
    dx_ref, dlin_ref, dg_ref, db_ref, dbias_ref = ops.layernorm_bwd(dpre, lnx, mean, rstd, gamma, dropout_p=p_drop, seed=5, site=9)
    assert rel_l2(dx, dx_ref) <= 1e-5
    if p_drop > 0:
        assert rel_l2(d16.float(), dlin_ref) <= 4e-3  # bf16 copy
    assert rel_l2(parts[:, 0].sum(0), dg_ref) <= 1e-4 and rel_l2(parts[:, 1].sum(0), db_ref) <= 1e-4
    assert rel_l2(parts[:, 2].sum(0), dbias_ref) <= 1e-4
    for _ in range(8):
        dx2, d162, parts2 = run()
        assert torch.equal(dx, dx2) and torch.equal(d16, d162) and torch.equal(parts, parts2)


def test_adamw_matches_torch(ops):
    n = 10007
    p, g = _rand(n, seed=1), _rand(n, seed=2)
    ref = torch.nn.Parameter(p.clone())
    opt = torch.optim.AdamW([ref], lr=1e-3, weight_decay=0.01)
    pd, m, v = p.to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    for step in range(1, 4):
        gs = g * step
        ref.grad = gs.clone()
        opt.step()
        ops.adamw_(pd, gs.to(DEV), m, v, lr=1e-3, weight_decay=0.01, step=step)
    torch.testing.assert_close(pd.cpu(), ref.detach(), rtol=1e-5, atol=1e-7)


@pytest.mark.parametrize("world", [2, 8])
def test_adamw_grad_scale_is_the_ddp_average(ops, world):
    """DDP averages gradients (config.yaml:5-6,35: torch DDP divides the SUM by the world size). Here the flat gradient
    is SUM-all-reduced and the 1/W rides in the AdamW launch (`grad_scale`): xfmr_adamw(g_sum, grad_scale=1/W) must be
    torch.optim.AdamW on g_sum / W."""
    n = 4099
    p, g = _rand(n, seed=1), _rand(n, seed=2)
    ref = torch.nn.Parameter(p.clone())
    opt = torch.optim.AdamW([ref], lr=1e-3, weight_decay=0.01)
    pd, m, v = p.to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    for step in range(1, 4):
        g_sum = g * step * world  # what the all-reduce leaves in the flat gradient
        ref.grad = g_sum / world
        opt.step()
        ops.adamw_(pd, g_sum.to(DEV), m, v, lr=1e-3, weight_decay=0.01, step=step, grad_scale=1.0 / world)
    torch.testing.assert_close(pd.cpu(), ref.detach(), rtol=1e-5, atol=1e-7)
    # and through the optimizer object the Trainer builds for world_size > 1
    from xfmr_rec_amd.trainer import FusedAdamW

    q = torch.nn.Parameter(p.clone().to(DEV))
    fo = FusedAdamW([q], lr=1e-3, weight_decay=0.01, grad_scale=1.0 / world)
    ref2 = torch.nn.Parameter(p.clone())
    opt2 = torch.optim.AdamW([ref2], lr=1e-3, weight_decay=0.01)
    q.grad = (g * world).to(DEV)
    ref2.grad = g.clone()
    fo.step()
    opt2.step()
    torch.testing.assert_close(q.detach().cpu(), ref2.detach(), rtol=1e-5, atol=1e-7)


def test_errors_are_loud(ops):
    with pytest.raises(RuntimeError, match="CPU tensor"):
        ops.layernorm_fwd(torch.zeros(4, 64), torch.ones(64), torch.zeros(64))
    qkv = torch.zeros(1, 8, 3 * 48, device=DEV)
    with pytest.raises(RuntimeError, match="not supported"):
        ops.attn_fwd(qkv, torch.ones(1, 8, dtype=torch.uint8, device=DEV), 1)  # head size 48


@pytest.mark.parametrize("mode", ["mean", "max", "cls", "lasttoken"])
def test_pooling_modes_vs_oracle(ops, mode):
    """ModelConfig.pooling_mode (models.py:47). Only 'mean' is pinned by a reference run (G3 sentence path); the
    other modes follow the oracle's restatement of sentence-transformers Pooling (parity unpinned, see oracle)."""
    from oracle import encoder as enc

    g = torch.Generator().manual_seed(3)
    B, L, H = 5, 17, 64
    tok = torch.randn(B, L, H, generator=g)
    lens = torch.tensor([17, 1, 9, 0, 12])
    mask = (torch.arange(L)[None, :] < lens[:, None])
    mask[2, 3] = False  # an interior padding position
    got = ops.pool(tok.to(DEV), mask.to(torch.uint8).to(DEV), mode).cpu()
    want = enc.pool(tok, mask.long(), mode)
    if mode == "max":  # rows with no visible token: -1e9 in both
        assert torch.equal(got[3], want[3])
    torch.testing.assert_close(got, want, rtol=1e-6, atol=1e-6)


def test_l2_normalize_fwd_bwd_vs_torch(ops):
    """torch.nn.functional.normalize (models.py:393-394), including a zero row (norm clamped at eps)."""
    g = torch.Generator().manual_seed(4)
    x = torch.randn(37, 128, generator=g)
    x[5] = 0
    dy = torch.randn(37, 128, generator=g)
    xr = x.clone().requires_grad_(True)
    yr = torch.nn.functional.normalize(xr, dim=-1)
    yr.backward(dy)
    xd = x.to(DEV).requires_grad_(True)
    yd = ops.l2_normalize(xd)
    yd.backward(dy.to(DEV))
    torch.testing.assert_close(yd.detach().cpu(), yr.detach(), rtol=1e-6, atol=1e-6)
    ok = torch.ones(37, dtype=torch.bool)
    ok[5] = False  # d/dx of x / eps is 1e12 * dy: compare on a relative scale
    torch.testing.assert_close(xd.grad.cpu()[ok], xr.grad[ok], rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(xd.grad.cpu()[5], xr.grad[5], rtol=1e-5, atol=0)
