"""Inputs on which the loss kernels' dot logits are EXACT, and their fp64 references (plain module, shared by
test_loss_cases_host.py, test_gpu_loss_dma_forms.py, loss_hard_cases.py and test_gpu_loss_hard_negatives.py).

Every query entry is a multiple of 2^-6 in [-2, 2] and every table entry a multiple of 2^-7 in [-0.25, 0.25]: both are
bf16 numbers (staging rounds nothing), every product is a multiple of 2^-13 of size <= 2^-1, and a sum of H <= 1024 of
them is an integer of at most 2^22 in units of 2^-13 -- it fits the 24-bit significand of fp32 at every step, in any order.
The kernels' dot logits are therefore the fp64 values bit for bit, and every decision taken on a dot logit (the
false-negative mask `l < pos`, the hinge indicator up to the fp32 rounding of (1 - margin) pos) is the reference's. What
stays inexact is the cosine normalisation, the epilogue arithmetic and the bf16 rounding of the gradient weights.

Construction (clustered, so that masks and margins are ACTIVE, which they almost never are on random unit vectors):
items are one of `CLUSTERS` sign-pattern centres plus noise of a per-item level, queries their positive's centre plus
noise at a per-row length. Shape: `T` positions = three 128-query blocks (the last partial); `V` items, so the ~155
distinct in-batch negatives fill three 64-column tiles and the 201 catalogue columns four (the last one partial in both),
and the multiplicities exceed 1; ragged validity; valid positions whose positive is padding; one exact false negative by item id.

Guard band: a query row keeps its positive only if none of its pairs with a DIFFERENT item (every table row, which
covers in-batch and catalogue candidates) is near a discontinuity, for every margin in `MARGINS`:
    |l - (1 - margin) pos| < 2^-20 max(1, |pos|)     the hinge kink (and, margin-free, l == pos exactly)
    |cos - cos_pos| < 1e-5                           the false-negative mask of the cosine heads
    |cos - 1 + margin| < 1e-5                        the cosine margin
Otherwise its `pos` is set to 0: it stops being a query and stays a negative. The widths are stated, not measured: a
few dozen fp32 ulps of the quantity compared."""

from __future__ import annotations

import functools
import types

import torch

from oracle import lean
from oracle import losses as OL

WIDTHS = (64, 128, 256, 384)  # the widths of the LDS-DMA kernels (and of the generic kernel's narrow instantiations)
# The generic kernel's widest instantiations only: 512 = the widest fp32 width (direct staging), 1024 = bf16 only
GENERIC_WIDTHS = (512, 1024)
SEEDS = {64: 11, 128: 12, 256: 13, 384: 14, 512: 15, 1024: 16}  # one case per width (chosen on the CPU: test_loss_cases_host.py)
MARGINS = (0.5, 0.3)  # every margin the GPU matrix uses
T, V, CLUSTERS = 320, 200, 6  # T = 4 sequences of 80 slots
Q_GRID, E_GRID = 2.0 ** -6, 2.0 ** -7
HINGE_BAND, COS_BAND = 2.0 ** -20, 1e-5


def _raw_inputs(H: int, seed: int):
    g = torch.Generator().manual_seed(seed)
    amp = 0.125 * (64.0 / H) ** 0.5  # centre entries: |centre|^2 = 1 at every width
    centres = (torch.randint(0, 2, (CLUSTERS, H), generator=g).double() * 2 - 1) * amp
    cl = torch.randint(0, CLUSTERS, (V + 1,), generator=g)
    level = 0.2 + 0.8 * torch.rand(V + 1, 1, generator=g).double()  # noise norm / centre norm, per item
    table = centres[cl] + level * amp * torch.randn(V + 1, H, generator=g).double()
    table = ((table / E_GRID).round() * E_GRID).clamp(-0.25, 0.25)
    table[0] = 0.0
    lens = torch.randint(66, 80, (4,), generator=g)  # ragged validity: four right-padded sequences of 80 slots
    lens[0] = 80
    mask = (torch.arange(80)[None, :] < lens[:, None]).reshape(-1)
    pos = torch.randint(1, V + 1, (T,), generator=g)
    neg = torch.randint(1, V + 1, (T,), generator=g)
    length = 1.0 + 7.0 * torch.rand(T, 1, generator=g).double()  # "varied length": |q| between 1 and 8 centre norms ...
    qlevel = 0.2 + 0.7 * torch.rand(T, 1, generator=g).double()
    tok = length * (centres[cl[pos]] + qlevel * amp * torch.randn(T, H, generator=g).double())
    tok = ((tok / Q_GRID).round() * Q_GRID).clamp(-2.0, 2.0)
    pos[torch.rand(T, generator=g) < 0.02] = 0  # valid positions whose positive is padding
    pos[7] = 0
    first = int(mask.nonzero()[0])
    neg[first] = pos[first] if int(pos[first]) != 0 else neg[first]  # an exact false negative by item id
    pos[~mask] = 0
    neg[~mask] = 0
    return table, tok, mask, pos, neg


def pair_terms(table, tok, pos):
    """fp64 (l, pos_l, cos, cos_pos, other) of every (position, table row) pair; `other`: the row is a DIFFERENT item."""
    t64, q64 = table.double(), tok.double()
    l = q64 @ t64.T
    p = l.gather(1, pos[:, None])
    tn = torch.nn.functional.normalize(t64, dim=-1, eps=1e-8)
    qn = torch.nn.functional.normalize(q64, dim=-1, eps=1e-8)
    c = qn @ tn.T
    cp = c.gather(1, pos[:, None])
    other = torch.arange(table.shape[0])[None, :] != pos[:, None]
    return l, p, c, cp, other


def near_discontinuity(table, tok, pos):
    """(T,) bool: the row has a pair with a different item inside the guard band (module docstring)."""
    l, p, c, cp, other = pair_terms(table, tok, pos)
    bad = (l == p) | ((c - cp).abs() < COS_BAND)
    for m in MARGINS:
        bad |= (l - (1 - m) * p).abs() < HINGE_BAND * p.abs().clamp(min=1.0)
        bad |= (c - 1 + m).abs() < COS_BAND
    return (bad & other).any(dim=1)


@functools.lru_cache(maxsize=None)
def inputs(H: int, seed: int | None = None):
    """The case of width H: fp32 `table` (V+1, H) and `tok` (T, H), bool `mask` (T), int64 `pos` / `neg` (T), the query
    selector `qsel`, and `n_dropped` / `n_before` of the guard band."""
    seed = SEEDS[H] if seed is None else seed
    table, tok, mask, pos, neg = _raw_inputs(H, seed)
    before = mask & (pos != 0)
    drop = near_discontinuity(table, tok, pos) & before
    pos = pos.clone()
    pos[drop] = 0
    return types.SimpleNamespace(H=H, seed=seed, table=table.float(), tok=tok.float(), mask=mask, pos=pos, neg=neg,
                                 qsel=mask & (pos != 0), n_dropped=int(drop.sum()), n_before=int(before.sum()))


def _scatter_rows(case, g_rows):
    d = torch.zeros(T, case.H, dtype=torch.float64)
    d[case.qsel] = g_rows
    return d


@functools.lru_cache(maxsize=None)
def reference(H: int, cand: str, masked: bool, scale: float = 1.0, margin: float = 0.5, seed: int | None = None):
    """fp64 reference of one configuration. cand = "batch": the valid positions' negatives, shared by every query
    (oracle.lean); "catalog": every table row (oracle.losses on table[None].expand, target = pos). Returns
    `sums[kind]` (floats), `stats` ("logits/..." -> float, plus the exact counts) and `d_tok[kind]` ((T, H) fp64: dL/dq
    in the query rows, 0 elsewhere). Read only: the tests share it."""
    case = inputs(H, seed)
    table, q = case.table.double(), case.tok.double()[case.qsel]
    pos_q = case.pos[case.qsel]
    cfg = dict(mask_false_negatives=masked, scale=scale, margin=margin)
    sums, grads = {}, {}
    if cand == "batch":
        negs = case.neg[case.mask]
        out = lean.heads_by_item(q, pos_q, negs, table, **cfg)
        for kind in OL.LOSS_KINDS:
            loss, g = lean.rows_reference_form(kind, q, pos_q, negs, table, **cfg)
            sums[kind] = out[f"loss/{kind}"]
            assert abs(float(loss) - sums[kind]) <= 1e-9 * max(1.0, abs(sums[kind])), kind  # the two oracle forms agree
            grads[kind] = _scatter_rows(case, g)
        stats = {k: v for k, v in out.items() if k.startswith("logits/")}
        counts = dict(n_valid=int(case.mask.sum()), neg_distinct=int(torch.unique(negs).numel()))
    else:
        assert cand == "catalog"
        full = table[None].expand(q.shape[0], -1, -1)
        ocfg = dict(target_position=None, **cfg)
        for kind in OL.LOSS_KINDS:
            qo = q.clone().requires_grad_(True)
            loss = OL.embed_loss(kind, qo, full, pos_q, **ocfg)
            (g,) = torch.autograd.grad(loss, qo)
            sums[kind] = loss.item()
            grads[kind] = _scatter_rows(case, g)
        stats = OL.logits_statistics(q, full, pos_q, **ocfg)
        l, p, _c, _cp, other = pair_terms(table, q, pos_q)
        stats["logits/neg/count"] = float(((l < p) if masked else other).sum())
        counts = dict(n_valid=V + 1, neg_distinct=V + 1)
    counts["n_query"] = int(case.qsel.sum())
    return types.SimpleNamespace(sums=sums, stats=stats, counts=counts, d_tok=grads)


def activity(H: int, margin: float, seed: int | None = None):
    """How active the discontinuous terms are on the case (conditions (c)-(e) of test_loss_cases_host.py), as fractions:
    `dropped` query rows; `masked_out` in-batch (query, negative) pairs that the false-negative mask removes (dot and
    cosine form); `hinge` / `cosine`: counted pairs with the hinge term / the cosine margin active, for masked and
    unmasked in-batch candidates and the catalogue."""
    case = inputs(H, seed)
    l, p, c, cp, other = pair_terms(case.table, case.tok[case.qsel], case.pos[case.qsel])
    mult = torch.bincount(case.neg[case.mask], minlength=V + 1).double()[None, :]
    out = dict(dropped=case.n_dropped / case.n_before,
               masked_out=float((((l >= p) | ~other) * mult).sum() / (mult.sum() * l.shape[0])),
               masked_out_cos=float((((c >= cp) | ~other) * mult).sum() / (mult.sum() * l.shape[0])))
    one = torch.ones_like(mult)
    for name, w_dot, w_cos in (("batch_masked", (l < p) * other * mult, (c < cp) * other * mult),
                               ("batch_unmasked", mult.expand_as(l), mult.expand_as(l)),
                               ("catalog_unmasked", other * one, other * one),
                               ("catalog_masked", (l < p) * other * one, (c < cp) * other * one)):
        out[f"hinge/{name}"] = float((w_dot * (l - (1 - margin) * p > 0)).sum() / w_dot.sum())
        out[f"cosine/{name}"] = float((w_cos * (c - 1 + margin > 0)).sum() / w_cos.sum())
    return out
