"""fp64 references of the two fused backward kernels of the encoder's dX chain (plain module, shared by
test_fused_refs_host.py, test_gpu_ffn_bwd_reference.py and test_gpu_dx_lnbwd_reference.py):

  xf_ffn_bwd_dx_fused_ex     dI = (dy W2) * gelu'(u);  dI W1 + rg  ->  LayerNorm backward
  xf_linear_bwd_dx_lnbwd_ex  dy W + rg (w.r.t. the possibly dropped-out LayerNorm OUTPUT)  ->  LayerNorm backward

The LayerNorm backward is never restated by hand: the gradient at the LayerNorm output goes through F.layer_norm by
autograd. The Linear that fed the LayerNorm is a leaf z with  pre = keep / (1 - p) * z + r,  r chosen so that pre is the
LayerNorm input the kernel was given; then dx = pre.grad, d_lin = z.grad, d_bias = z.grad.sum(0).
test_fused_refs_host.py proves these builders against whole blocks differentiated end to end."""

from __future__ import annotations

import math

import torch
import torch.nn.functional as F

LN_EPS = 1e-12  # (LAYER_NORM_EPS of the product; what the tests' mean / rstd are computed with)


def gelu_grad(u: torch.Tensor) -> torch.Tensor:
    """gelu'(u) = Phi(u) + u phi(u) of the exact-erf GELU, in u's precision (fp64 here)."""
    return 0.5 * (1 + torch.erf(u / math.sqrt(2.0))) + u * torch.exp(-0.5 * u * u) / math.sqrt(2 * math.pi)


def _f64(t):
    return None if t is None else t.detach().double().cpu()


def ln_chain_ref(g_out, lnx, gamma, keep=None, p=0.0, keep2=None, p2=0.0, eps=LN_EPS):
    """g_out: gradient w.r.t. x0 = keep2 / (1 - p2) * LayerNorm(pre) (keep2 None: x0 is the LayerNorm output itself).
    Returns dx (w.r.t. pre), d_lin (w.r.t. the Linear output z), d_gamma, d_beta, d_bias -- all by autograd."""
    g_out, lnx, gamma = _f64(g_out), _f64(lnx), _f64(gamma)
    H = lnx.shape[-1]
    s = torch.ones_like(lnx) if keep is None else _f64(keep) / (1.0 - p)
    z = torch.zeros_like(lnx, requires_grad=True)
    r = lnx - s * z.detach()
    pre = s * z + r
    assert torch.equal(pre.detach(), lnx)
    pre.retain_grad()
    gam = gamma.clone().requires_grad_(True)
    bet = torch.zeros_like(gamma, requires_grad=True)
    x0 = F.layer_norm(pre, (H,), gam, bet, eps)
    if keep2 is not None:
        x0 = _f64(keep2) / (1.0 - p2) * x0
    x0.backward(g_out)
    return dict(dx=pre.grad, d_lin=z.grad, d_gamma=gam.grad, d_beta=bet.grad, d_bias=z.grad.sum(0))


def ffn_bwd_dx_ref(dy, w2, u, w1, rg, lnx, gamma, keep, p, di=None):
    """xf_ffn_bwd_dx_fused_ex. dy (M,H), w2 (H,I), u (M,I), w1 (I,H), rg (M,H) or None, lnx (M,H): the LayerNorm input,
    gamma (H,), keep (M,H) 0/1 or None, p: its dropout rate. `di`: evaluate the second stage from THIS dI (the kernel's own
    bf16 one: the stage is then judged at fp32 level) instead of the fp64 one. Returns di (always the fp64 one) and
    ln_chain_ref's dict."""
    dy, w2, u, w1 = _f64(dy), _f64(w2), _f64(u), _f64(w1)
    di64 = (dy @ w2) * gelu_grad(u)
    src = di64 if di is None else _f64(di)
    g_out = src @ w1
    if rg is not None:
        g_out = g_out + _f64(rg)
    out = ln_chain_ref(g_out, lnx, gamma, keep, p)
    out["di"] = di64
    return out


def dx_lnbwd_ref(dy, w, rg, lnx, gamma, keep, p, keep2=None, p2=0.0):
    """xf_linear_bwd_dx_lnbwd_ex. dy (M,N), w (N,128); the incoming gradient dy w + rg is w.r.t.
    x0 = keep2 / (1 - p2) * LayerNorm(pre) (the embedding LayerNorm's dropped-out output; keep2 None: no such dropout)."""
    g_out = _f64(dy) @ _f64(w)
    if rg is not None:
        g_out = g_out + _f64(rg)
    return ln_chain_ref(g_out, lnx, gamma, keep, p, keep2, p2)
