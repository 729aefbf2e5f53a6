"""Key masks that are NOT a prefix, for every attention form of csrc/attention.hip. Plain module, no GPU and no library:
shared by test_attn_mask_cases_host.py (which shows on the CPU that the table tells a right kernel from a subtly wrong one,
and that the bf16 rounding model stays well inside the limits on it) and test_gpu_attn_masks.py (which holds the kernels to
the fp64 reference through the same `check`).

* `masks(L, chunk)`: the named (L,) masks; one batch = one sequence per name, so one launch covers the table.
* `inputs` / `case`: seeded qkv and w (drawn as test_gpu_attn_long_bf16._inputs draws them, w zero on masked rows -- the
  entry point's contract: the training path only back-propagates valid rows) and the fp64 reference of ctx, lse and d_qkv
  (`_attention_reference`: a query without a visible key gives zeros), computed once per shape and left unchanged.
* `model(case, mutant=)`: fp64 forward + backward the way the kernels walk it -- 32-key tiles, a running max per query, the
  wave-wide `continue` over 32 queries, `msafe`, lse = +inf for a row without keys, the backward from that lse. `MUTANTS`
  are switches of it, each a plausible kernel error.
* `check`: the assertions, with the project's tolerances (helpers.TOL). It returns the figures it measured, per sequence.

What a row without a visible key yields (attention): ctx = 0, lse = +inf, zero gradients."""

from __future__ import annotations

import functools
import types

import torch

from helpers import TOL
from test_gpu_attn_long_bf16 import _attention_reference, _rand

F64 = torch.float64
LOG2E, LN2 = 1.4426950408889634, 0.6931471805599453
NAMES = ("left1", "left31", "left32", "left33", "left_chunk", "tile1", "tile1_pm1", "bern", "even", "first_only", "last_only",
         "two", "none")
SLICES = ("dq", "dk", "dv")
MUTANTS = ("alpha_without_msafe", "interior_ignores_mask", "chunk_bits_not_rebased", "halfwave_shift_dropped",
           "stops_at_first_empty_tile", "mask_as_length", "empty_row_lse_zero")
# mutants of a path only some forms have: the wave-wide `continue` leaves a row at -inf beside rows that are not only under
# the causal mask (bidirectional: every query of a sequence sees the same keys); only the streaming forms restage mask bits
CAUSAL_ONLY = ("alpha_without_msafe",)
STREAMING_ONLY = ("chunk_bits_not_rebased",)
BERN_SEED = 5


def masks(L: int, chunk: int) -> dict:
    """name -> (L,) uint8. `chunk`: the form's key chunk (256: bf16 streaming, 128: generic; panel forms pass 128, so the
    long left pad still crosses a 128-row query block)."""
    assert L > chunk + 1 and L > 65
    one = lambda: torch.ones(L, dtype=torch.uint8)  # noqa: E731
    zero = lambda: torch.zeros(L, dtype=torch.uint8)  # noqa: E731
    out = {}
    for name, p in (("left1", 1), ("left31", 31), ("left32", 32), ("left33", 33), ("left_chunk", chunk + 1)):
        out[name] = one()
        out[name][:p] = 0
    out["tile1"] = one()
    out["tile1"][32:64] = 0
    out["tile1_pm1"] = one()
    out["tile1_pm1"][31:65] = 0
    out["bern"] = (torch.rand(L, generator=torch.Generator().manual_seed(BERN_SEED)) < 0.5).to(torch.uint8)
    out["bern"][L - 1] = 1
    out["even"] = one()
    out["even"][1::2] = 0
    out["first_only"] = zero()
    out["first_only"][0] = 1
    out["last_only"] = zero()
    out["last_only"][L - 1] = 1
    out["two"] = zero()
    out["two"][40] = 1
    out["two"][L - 1] = 1
    out["none"] = zero()
    assert tuple(out) == NAMES
    return out


def inputs(L: int, A: int, dh: int, chunk: int, seed: int = 3):
    """qkv (B, L, 3 A dh), mask (B, L) uint8 and w (B, L, A dh) with B = len(NAMES); w is zero on masked rows."""
    B, H = len(NAMES), A * dh
    qkv = _rand(B, L, 3 * H, seed=seed)
    mask = torch.stack(list(masks(L, chunk).values()))
    w = _rand(B, L, H, seed=seed + 1) * mask[..., None]
    return qkv, mask, w


def _heads(t, A):
    B, L, H = t.shape
    return t.view(B, L, A, H // A).transpose(1, 2)  # (B, A, L, dh)


def _merge(t):
    B, A, L, dh = t.shape
    return t.transpose(1, 2).reshape(B, L, A * dh)


def _allowed(L, causal):
    tri = torch.ones(L, L, dtype=torch.bool)
    return tri.tril() if causal else tri


@functools.lru_cache(maxsize=32)
def case(L: int, A: int, dh: int, chunk: int, causal: bool, seed: int = 3):
    """Inputs and fp64 reference of one shape (read only: shared). `sees` (B, L): the query has a visible key."""
    qkv, mask, w = inputs(L, A, dh, chunk, seed)
    ref_in = qkv.clone().double().requires_grad_(True)
    ref = _attention_reference(ref_in, mask, A, causal)
    (ref * w.double()).sum().backward()
    vis = _allowed(L, causal)[None] & mask.bool()[:, None, :]
    q, k = (_heads(t, A) for t in qkv.double().split(A * dh, dim=-1)[:2])
    s = (q @ k.transpose(2, 3) * dh**-0.5).masked_fill(~vis[:, None], -float("inf"))
    lse = torch.logsumexp(s, dim=-1)  # (B, A, L); -inf on a row without keys: the kernels store +inf there
    sees = vis.any(-1)
    lse = torch.where(sees[:, None], lse, torch.full_like(lse, float("inf")))
    return types.SimpleNamespace(L=L, A=A, dh=dh, chunk=chunk, causal=causal, names=NAMES, qkv=qkv, mask=mask, w=w,
                                 sees=sees, ref_ctx=ref.detach(), ref_grad=ref_in.grad, ref_lse=lse)


# ------------------------------------------------------------------------------------------------ the model
def _visible(mask, L, causal, chunk, mutant):
    """(B, L, L) bool [b, query, key]: what the walk treats as visible."""
    B = mask.shape[0]
    km = mask.bool().clone()
    key = torch.arange(L)
    if mutant == "mask_as_length":  # the mask is a prefix of mask.sum() keys
        km = key[None] < mask.sum(1, keepdim=True)
    elif mutant == "stops_at_first_empty_tile":  # trailing padding assumed: nothing after the first 32-key tile without a key
        for b in range(B):
            for k0 in range(0, L, 32):
                if not km[b, k0:k0 + 32].any():
                    km[b, k0:] = False
                    break
    elif mutant == "halfwave_shift_dropped":  # lanes 32..63 (keys 4..7, 12..15, ... of a tile) test the bits of lanes 0..31
        km = km[:, key - 4 * ((key >> 2) & 1)]
    elif mutant == "chunk_bits_not_rebased":  # chunk c reads chunk 0's mask words
        km = km[:, key % chunk]
    vis = _allowed(L, causal)[None] & km[:, None, :]
    if mutant == "interior_ignores_mask":  # a whole tile at or before the wave's first query counts as fully visible
        for q0 in range(0, L, 32):
            for k0 in range(0, L - 31, 32):
                if k0 + 31 <= q0 or not causal:
                    vis[:, q0:q0 + 32, k0:k0 + 32] = True
    return vis


def model(c, mutant=None):
    """ctx (B, L, H), d_qkv (B, L, 3 H) and lse (B, A, L), fp64, of the case `c` as the kernels walk it."""
    assert mutant is None or mutant in MUTANTS
    L, A, dh = c.L, c.A, c.dh
    H = A * dh
    q, k, v = (_heads(t, A) for t in c.qkv.double().split(H, dim=-1))
    do = _heads(c.w.double(), A)
    B = q.shape[0]
    s = q @ k.transpose(2, 3)
    vis = _visible(c.mask, L, c.causal, c.chunk, mutant)[:, None].expand(B, A, L, L)
    sc = dh**-0.5 * LOG2E
    ninf = -float("inf")
    m = torch.full((B, A, L), ninf, dtype=F64)
    lsum = torch.zeros(B, A, L, dtype=F64)
    o = torch.zeros(B, A, L, dh, dtype=F64)
    for k0 in range(0, L, 32):
        sb = (s[..., k0:k0 + 32] * sc).masked_fill(~vis[..., k0:k0 + 32], ninf)
        mnew = torch.maximum(m, sb.max(dim=-1).values)
        skip = torch.zeros(B, A, L, dtype=torch.bool)
        for q0 in range(0, L, 32):  # `if (__all(mnew == -INFINITY)) continue;` over the wave's 32 queries
            skip[..., q0:q0 + 32] = (mnew[..., q0:q0 + 32] == ninf).all(-1, keepdim=True)
        msafe = mnew if mutant == "alpha_without_msafe" else torch.where(mnew == ninf, torch.zeros_like(mnew), mnew)
        alpha = torch.exp2(m - msafe)  # (-inf) - (-inf) = NaN without msafe
        p = torch.exp2(sb - msafe[..., None])
        lsum = torch.where(skip, lsum, lsum * alpha + p.sum(-1))
        o = torch.where(skip[..., None], o, o * alpha[..., None] + p @ v[:, :, k0:k0 + 32])
        m = torch.where(skip, m, mnew)
    some = lsum > 0
    inv = torch.where(some, 1.0 / lsum.clamp(min=1e-300), torch.zeros_like(lsum))
    ctx = o * inv[..., None]
    lse = torch.where(some, (m + torch.log2(lsum.clamp(min=1e-300))) * LN2, torch.full_like(m, float("inf")))
    # backward, from the stored lse: P = exp(s / sqrt(dh) - lse) on the visible pairs
    pr = torch.exp(s * dh**-0.5 - lse[..., None]).masked_fill(~vis, 0.0)
    if mutant == "empty_row_lse_zero":  # lse = 0 stored for a row without keys, and the backward relies on lse to zero P
        lse = torch.where(some, lse, torch.zeros_like(lse))
        allowed = _allowed(L, c.causal)[None, None].expand(B, A, L, L)
        pr = torch.where(some[..., None], pr, torch.exp(s * dh**-0.5).masked_fill(~allowed, 0.0))
    dp = do @ v.transpose(2, 3)
    delta = (do * ctx).sum(-1, keepdim=True)
    ds = pr * (dp - delta)
    dv = pr.transpose(2, 3) @ do
    dq = (ds @ k) * dh**-0.5
    dk = (ds.transpose(2, 3) @ q) * dh**-0.5
    return _merge(ctx), torch.cat([_merge(dq), _merge(dk), _merge(dv)], dim=-1), lse


# ------------------------------------------------------------------------------------------------ the check
def check(name, prec, ctx, d_qkv, c, lse=None):
    """Holds ctx (B, L, H) and d_qkv (B, L, 3 H) of the case `c` to its fp64 reference:
      * finite everywhere, masked rows included; ctx exactly 0 on every row that sees no key;
      * per sequence, ctx on the valid rows within TOL[prec]["val"] (max scaled error);
      * per sequence b and slice s of dq / dk / dv: |got[b, s] - want[b, s]|_2 <= TOL[prec]["grad_l2"] * |want[b]|_2 with
        want[b] the sequence's WHOLE reference gradient (with one visible key dq and dk are exactly 0 in the reference);
        where want[b] is 0, got[b] is exactly 0;
      * `lse` ((B, A, L), optional): +inf exactly on the rows that see no key -- the convention the backward kernels take
        back in, which neither ctx nor (with w = 0 on masked rows) d_qkv can show -- and within TOL[prec]["val"] elsewhere.
    Returns {sequence name: {ctx, dq, dk, dv[, lse]: error}}."""
    tol = TOL[prec]
    ctx, d_qkv = ctx.detach().double().cpu(), d_qkv.detach().double().cpu()
    B, L, H = c.ref_ctx.shape
    assert ctx.shape == (B, L, H) and d_qkv.shape == (B, L, 3 * H), (name, ctx.shape, d_qkv.shape)
    assert bool(torch.isfinite(ctx).all()), f"{name}: ctx is not finite on {_rows_of(~torch.isfinite(ctx).all(-1), c)}"
    assert bool(torch.isfinite(d_qkv).all()), f"{name}: d_qkv is not finite on {_rows_of(~torch.isfinite(d_qkv).all(-1), c)}"
    blind = ~c.sees
    assert bool((ctx[blind] == 0).all()), f"{name}: ctx is not 0 on rows without keys: {_rows_of((ctx != 0).any(-1) & blind, c)}"
    valid = c.mask.bool()
    figs = {}
    for b, seq in enumerate(c.names):
        f = dict(ctx=0.0)
        if valid[b].any():
            got, want = ctx[b][valid[b]], c.ref_ctx[b][valid[b]]
            f["ctx"] = ((got - want).abs() / want.abs().clamp(min=1.0)).max().item()
            assert f["ctx"] <= tol["val"], f"{name} [{prec}] {seq}: ctx error {f['ctx']:.3e} > {tol['val']:.1e}"
        want_b = c.ref_grad[b]
        den = want_b.norm().item()
        for i, sl in enumerate(SLICES):
            got, want = d_qkv[b, :, i * H:(i + 1) * H], want_b[:, i * H:(i + 1) * H]
            if den == 0:
                assert bool((got == 0).all()), f"{name} {seq}: {sl} is not exactly 0 where the reference gradient is"
                f[sl] = 0.0
            else:
                f[sl] = (got - want).norm().item() / den
                assert f[sl] <= tol["grad_l2"], f"{name} [{prec}] {seq}: {sl} error {f[sl]:.3e} > {tol['grad_l2']:.1e}"
        if lse is not None:
            got = lse.detach().double().cpu()[b]  # (A, L)
            assert got.shape == c.ref_lse[b].shape, (name, got.shape)
            bl = blind[b][None].expand_as(got)
            assert bool((got[bl] == float("inf")).all()), f"{name} {seq}: lse is not +inf on rows without keys"
            assert bool(torch.isfinite(got[~bl]).all()), f"{name} {seq}: lse is not finite on a row with keys"
            want = c.ref_lse[b][~bl]
            f["lse"] = ((got[~bl] - want).abs() / want.abs().clamp(min=1.0)).max().item() if want.numel() else 0.0
            assert f["lse"] <= tol["val"], f"{name} [{prec}] {seq}: lse error {f['lse']:.3e} > {tol['val']:.1e}"
        figs[seq] = f
    return figs


def _rows_of(bad, c):
    """'name: rows' of a (B, L) bool, for a message."""
    return "; ".join(f"{c.names[b]}: {bad[b].nonzero().flatten().tolist()[:8]}" for b in range(bad.shape[0]) if bad[b].any())


def worst(figs):
    """(worst ctx error, worst per-slice gradient error) over the sequences, each with the sequence's name."""
    cx = max(figs, key=lambda n: figs[n]["ctx"])
    gr = max(figs, key=lambda n: max(figs[n][s] for s in SLICES))
    return (figs[cx]["ctx"], cx), (max(figs[gr][s] for s in SLICES), gr)


def fig_line(tag, figs):
    (ec, nc), (eg, ng) = worst(figs)
    return f"FIG attn-masks {tag}: worst ctx {ec:.2e} ({nc})  worst gradient slice {eg:.2e} ({ng})"
