"""The fp64 reference builders of fused_refs.py against whole blocks differentiated end to end by autograd (no GPU): the
kernels are judged by these builders, so the builders are proven first. The blocks are written the way the encoder is --
Linear output z, dropout, residual, LayerNorm, then what consumes the LayerNorm output -- and never go through fused_refs."""

import pytest
import torch
import torch.nn.functional as F

from fused_refs import LN_EPS, dx_lnbwd_ref, ffn_bwd_dx_ref, gelu_grad

H = 128
TOL = 1e-12


def _close(name, got, want):
    err = (got - want).abs().max().item() / max(1.0, want.abs().max().item())
    assert err <= TOL, f"{name}: {err:.3e}"


def _leaves(M, p, g):
    z = torch.randn(M, H, generator=g, dtype=torch.float64).requires_grad_(True)  # output of the Linear in front
    res = torch.randn(M, H, generator=g, dtype=torch.float64)
    keep = (torch.rand(M, H, generator=g) >= p).double() if p > 0 else torch.ones(M, H, dtype=torch.float64)
    gamma = (1 + 0.1 * torch.randn(H, generator=g, dtype=torch.float64)).requires_grad_(True)
    beta = (0.1 * torch.randn(H, generator=g, dtype=torch.float64)).requires_grad_(True)

    def make_pre():  # dropout of the Linear output + residual: the LayerNorm input
        pre = keep / (1 - p) * z + res
        pre.retain_grad()
        return pre

    return z, keep, gamma, beta, make_pre


def test_gelu_grad_is_the_derivative_of_torch_gelu():
    u = torch.linspace(-6, 6, 1001, dtype=torch.float64).requires_grad_(True)
    F.gelu(u).sum().backward()
    _close("gelu'", gelu_grad(u.detach()), u.grad)


@pytest.mark.parametrize("with_rg", [True, False])
@pytest.mark.parametrize("M,I,p", [(1, 64, 0.0), (70, 192, 0.1), (37, 128, 0.25)])
def test_ffn_bwd_dx_ref_returns_the_ffn_blocks_own_gradients(M, I, p, with_rg):
    g = torch.Generator().manual_seed(100 * M + I)
    z, keep, gamma, beta, make_pre = _leaves(M, p, g)
    pre = make_pre()
    w1 = 0.08 * torch.randn(I, H, generator=g, dtype=torch.float64)
    b1 = 0.1 * torch.randn(I, generator=g, dtype=torch.float64)
    w2 = 0.05 * torch.randn(H, I, generator=g, dtype=torch.float64)
    b2 = 0.1 * torch.randn(H, generator=g, dtype=torch.float64)
    dy = torch.randn(M, H, generator=g, dtype=torch.float64)
    rg = torch.randn(M, H, generator=g, dtype=torch.float64) if with_rg else None
    x1 = F.layer_norm(pre, (H,), gamma, beta, LN_EPS)
    u = x1 @ w1.T + b1
    u.retain_grad()
    y = F.gelu(u) @ w2.T + b2
    loss = (y * dy).sum()
    if with_rg:
        loss = loss + (x1 * rg).sum()  # the residual branch around the FFN
    loss.backward()
    ref = ffn_bwd_dx_ref(dy, w2, u, w1, rg, pre, gamma, keep if p > 0 else None, p)
    _close("di", ref["di"], u.grad)
    _close("dx", ref["dx"], pre.grad)
    _close("d_lin", ref["d_lin"], z.grad)
    _close("d_gamma", ref["d_gamma"], gamma.grad)
    _close("d_beta", ref["d_beta"], beta.grad)
    _close("d_bias", ref["d_bias"], z.grad.sum(0))
    # the second stage from a given dI: the same block with u's gradient replaced
    di = u.grad + 0.01 * torch.randn(M, I, generator=g, dtype=torch.float64)
    for t in (z, gamma, beta):
        t.grad = None
    pre = make_pre()
    x1 = F.layer_norm(pre, (H,), gamma, beta, LN_EPS)
    x1.backward(di @ w1 + (rg if with_rg else 0))
    ref = ffn_bwd_dx_ref(dy, w2, u, w1, rg, pre, gamma, keep if p > 0 else None, p, di=di)
    _close("dx(di)", ref["dx"], pre.grad)
    _close("d_gamma(di)", ref["d_gamma"], gamma.grad)
    _close("d_bias(di)", ref["d_bias"], z.grad.sum(0))


@pytest.mark.parametrize("with_rg", [True, False])
@pytest.mark.parametrize("M,N,p,p2", [(1, 96, 0.0, 0.0), (70, 384, 0.1, 0.0), (37, 96, 0.0, 0.1), (37, 512, 0.2, 0.3)])
def test_dx_lnbwd_ref_returns_the_blocks_own_gradients(M, N, p, p2, with_rg):
    g = torch.Generator().manual_seed(100 * M + N)
    z, keep, gamma, beta, make_pre = _leaves(M, p, g)
    pre = make_pre()
    keep2 = (torch.rand(M, H, generator=g) >= p2).double() if p2 > 0 else None
    w = 0.05 * torch.randn(N, H, generator=g, dtype=torch.float64)
    b = 0.1 * torch.randn(N, generator=g, dtype=torch.float64)
    dy = torch.randn(M, N, generator=g, dtype=torch.float64)
    rg = torch.randn(M, H, generator=g, dtype=torch.float64) if with_rg else None
    x0 = F.layer_norm(pre, (H,), gamma, beta, LN_EPS)
    if keep2 is not None:
        x0 = x0 * keep2 / (1 - p2)  # dropout of the LayerNorm output (the embedding site)
    v = x0 @ w.T + b
    loss = (v * dy).sum()
    if with_rg:
        loss = loss + (x0 * rg).sum()
    loss.backward()
    ref = dx_lnbwd_ref(dy, w, rg, pre, gamma, keep if p > 0 else None, p, keep2, p2)
    _close("dx", ref["dx"], pre.grad)
    _close("d_lin", ref["d_lin"], z.grad)
    _close("d_gamma", ref["d_gamma"], gamma.grad)
    _close("d_beta", ref["d_beta"], beta.grad)
    _close("d_bias", ref["d_bias"], z.grad.sum(0))
