"""fp64 reference of the top-k hard-negative restriction (LossConfig.num_hard_negatives, losses.py:295-330) on the
exact-logit cases of tests/loss_cases.py (plain module, shared by test_loss_hard_cases_host.py and
test_gpu_loss_hard_negatives.py).

Everything is computed BY ITEM from the fp64 (query, table row) logits -- no (Np, 1 + N, H) candidates: a column's term is
a function of its item, so an item that the N in-batch negatives hold `mult` times is one column of weight `mult`.

The TIE RULE (the library's contract, include/xfmr_hip.h: "ties at the threshold share the remaining weight"). Per query
row and per logit kind (dot logits for InfoNCE, NCE, the pairwise heads and LogitsStatistics; cosines for the contrastive
term), over the COUNTED negatives -- the false-negative mask is `l < pos`, an item equal to the positive takes the
positive's logit, the catalogue form leaves the positive's column out --:
    tau  = the k-th largest counted logit, every item counted `mult` times,
    rho  = (k - #greater) / #equal          (# = summed multiplicities above / at tau),
    weight = mult * (1 if l > tau, rho if l == tau, 0 if l < tau).
A row with at most k counted negatives keeps them all, and k >= 1 + N columns switches the restriction off. torch.topk
selects WHOLE columns instead; every head depends on the multiset of the selected logits only, so the loss values are the
same for any of topk's choices, and the gradients are the same unless the tie at tau is between DIFFERENT items
(test_loss_hard_cases_host.py compares both with oracle.losses on a slice).

On the exact-logit cases a top-k over dot logits is the same selection in bf16, fp32 and fp64. A top-k over cosines is
not: `reference(...).flagged` (`near_tie`) marks the rows whose threshold has another item's cosine within loss_cases.COS_BAND of
it. Such rows stay in every loss sum (a near-tie moves a value by at most the band) and leave the gradient comparison of the
contrastive heads."""

from __future__ import annotations

import functools
import types

import torch
import torch.nn.functional as F

import loss_cases as LC
from oracle import losses as OL

K_OFF = 400  # >= 1 + N for the ~300 in-batch negative columns: the restriction is off
# the k of the GPU matrix: small, middle, large (masked rows mix restricted and unrestricted ones), off
K_BATCH = (3, 40, 250, K_OFF)
K_CATALOG = (3, 40, LC.V, LC.V + 1)  # V + 1 = every column of the catalogue form: off
K_WIDE = {"batch": (3, 250), "catalog": (40, LC.V)}  # the two k of the wide generic widths


def ks_of(cand: str, H: int):
    if H in LC.GENERIC_WIDTHS:
        return K_WIDE[cand]
    return K_BATCH if cand == "batch" else K_CATALOG


def topk_weights(lg, w0, k: int, n_cols: int):
    """The tie rule of the module docstring. lg (Np, V + 1): logits by item; w0: counted weights (multiplicity, 0 = not
    counted); n_cols = 1 + N columns of the reference's logits. Returns (weights, tau, rho, restricted), tau = -inf and
    rho = 1 where nothing is cut."""
    lg, w0 = lg.detach(), w0.to(torch.float64)
    total = w0.sum(dim=1, keepdim=True)
    if k <= 0 or k >= n_cols:
        restricted = torch.zeros_like(total, dtype=torch.bool)
    else:
        restricted = total > k
    order = lg.argsort(dim=1, descending=True)
    cum = w0.gather(1, order).cumsum(dim=1)
    first = (cum >= k).to(torch.int8).argmax(dim=1, keepdim=True)  # the sorted column that holds the k-th element
    tau = lg.gather(1, order).gather(1, first)
    tau = torch.where(restricted, tau, torch.full_like(tau, -float("inf")))
    greater = (w0 * (lg > tau)).sum(dim=1, keepdim=True)
    equal = (w0 * (lg == tau)).sum(dim=1, keepdim=True)
    rho = torch.where(restricted, (k - greater) / equal.clamp(min=1.0), torch.ones_like(tau))
    assert bool(((rho > 0) & (rho <= 1)).all())
    share = torch.where(lg > tau, torch.ones_like(lg), torch.where(lg == tau, rho.expand_as(lg), torch.zeros_like(lg)))
    w = w0 * share
    kept = torch.where(restricted, torch.full_like(total, float(k)), total)  # every row keeps k, or all it has
    assert bool(((w.sum(dim=1, keepdim=True) - kept).abs() < 1e-9).all())
    return w, tau[:, 0], rho[:, 0], restricted[:, 0]


def _wmean(values, weights):
    """losses.py:90-111. The reference's weights are a bool mask: its `sum + 1e-9` is a float32 tensor whatever the
    logits' type, i.e. the count itself from 1 on (with k = 1 an fp64 epsilon would show at 1e-9)."""
    den = (weights.sum(dim=1, keepdim=True).float() + 1e-9).double()
    return (values * weights / den).sum(dim=1)


def _logits(q, table, pos):
    """Differentiable (l, pos_l, cos, cos_pos) by item; the positive's column IS the positive (ties by item id)."""
    l = q @ table.T
    c = F.normalize(q, dim=-1, eps=1e-8) @ F.normalize(table, dim=-1, eps=1e-8).T
    return l, l.gather(1, pos[:, None]), c, c.gather(1, pos[:, None])


def counted(q, pos, table, mult, masked: bool):
    """(w0_dot, w0_cos): counted weights by item. mult: (V + 1,) multiplicities of the in-batch negatives, or None for the
    catalogue form (every table row once, the positive's own column left out)."""
    l, p, c, cp = _logits(q, table, pos)
    other = torch.arange(table.shape[0])[None, :] != pos[:, None]
    base = other.double() if mult is None else mult.double()[None, :].expand_as(l)
    if not masked:
        return base.clone(), base.clone()
    return base * (l < p), base * (c < cp)


def heads(q, pos, table, mult, n_cols: int, *, masked: bool, k: int, scale=1.0, margin=0.5):
    """Per-row values of the seven heads (dict kind -> (Np,) tensor, differentiable in q), LogitsStatistics (dict) and the
    selection (`sel.dot` / `sel.cos`: weights, tau, rho, restricted) under the top-k restriction."""
    with torch.no_grad():
        w0d, w0c = counted(q, pos, table, mult, masked)
        l0, _p0, c0, _cp0 = _logits(q, table, pos)
        sd = topk_weights(l0, w0d, k, n_cols)
        sc = topk_weights(c0, w0c, k, n_cols)
    wd, wc = sd[0], sc[0]
    l, p, c, cp = _logits(q, table, pos)
    rows = {}
    align = 1 - cp[:, 0]
    contr = _wmean((c - 1 + margin).relu(), wc)
    rows["AlignmentLoss"] = align
    rows["AlignmentContrastiveLoss"] = align + contr
    rows["ContrastiveLoss"] = contr
    z = (scale * l).masked_fill(wd == 0, -float("inf"))
    zmax = torch.maximum(z.max(dim=1, keepdim=True).values, scale * p).detach()
    lse = zmax[:, 0] + torch.log(torch.exp(scale * p[:, 0] - zmax[:, 0]) + (wd * torch.exp(z - zmax)).sum(dim=1))
    rows["InfoNCELoss"] = lse - scale * p[:, 0]
    rows["NCELoss"] = F.softplus(-p[:, 0]) + _wmean(F.softplus(l), wd)
    s = l - p * (1 - margin)
    rows["PairwiseHingeLoss"] = _wmean(s.relu(), wd)
    rows["PairwiseLogisticLoss"] = _wmean(F.softplus(s), wd)
    with torch.no_grad():  # LogitsStatistics (losses.py:375-405): the selected dot logits
        n = float(q.shape[0])
        num_neg = n_cols - 1
        if k > 0:
            num_neg = min(num_neg, k)
        cnt = wd.sum(dim=1)
        nc = float(round(float(cnt.sum())))  # (every row's weights sum to k or to its count: an integer)
        assert abs(nc - float(cnt.sum())) < 1e-6
        st = {"logits/neg/density": float((cnt / (num_neg + 1e-9)).sum()) / n, "logits/neg/count": nc,
              "logits/pos/mean": float(p.mean()), "logits/pos/std": float(p.std()) if n > 1 else float("nan"),
              "logits/pos/min": float(p.min()), "logits/pos/max": float(p.max())}
        if nc > 0:
            ns, nss = float((wd * l).sum()), float((wd * l * l).sum())
            st["logits/neg/mean"] = ns / nc
            st["logits/neg/std"] = max(0.0, (nss - ns * ns / nc) / (nc - 1)) ** 0.5 if nc > 1 else float("nan")
            st["logits/neg/min"], st["logits/neg/max"] = float(l[wd > 0].min()), float(l[wd > 0].max())
    return rows, st, types.SimpleNamespace(dot=sd, cos=sc, l=l0, c=c0, w0_dot=w0d, w0_cos=w0c)


def _case_terms(H: int, cand: str):
    case = LC.inputs(H)
    table, q, pos = case.table.double(), case.tok.double()[case.qsel], case.pos[case.qsel]
    if cand == "batch":
        negs = case.neg[case.mask]
        return case, table, q, pos, torch.bincount(negs, minlength=LC.V + 1), 1 + int(negs.numel())
    assert cand == "catalog"
    return case, table, q, pos, None, LC.V + 1


@functools.lru_cache(maxsize=None)
def reference(H: int, cand: str, masked: bool, k: int, scale: float = 1.0, margin: float = 0.5):
    """fp64 reference of one configuration with num_hard_negatives = k, in the layout of loss_cases.reference: `sums`,
    `stats` (with "logits/neg/count"), `counts`, `d_tok[kind]` ((T, H), by autograd), plus `sel` (the selection, see
    `heads`) and `flagged` ((n_query,) bool: near_tie of the cosines). Read only: the tests share it."""
    case, table, q, pos, mult, n_cols = _case_terms(H, cand)
    qo = q.clone().requires_grad_(True)
    rows, stats, sel = heads(qo, pos, table, mult, n_cols, masked=masked, k=k, scale=scale, margin=margin)
    sums, grads = {}, {}
    for kind in OL.LOSS_KINDS:
        total = rows[kind].sum()
        (g,) = torch.autograd.grad(total, qo, retain_graph=True)
        sums[kind] = total.item()
        d = torch.zeros(LC.T, H, dtype=torch.float64)
        d[case.qsel] = g
        grads[kind] = d
    base = LC.reference(H, cand, masked, scale, margin)
    return types.SimpleNamespace(sums=sums, stats=stats, counts=base.counts, d_tok=grads, sel=sel,
                                 flagged=near_tie(sel.c, sel.w0_cos, sel.cos, LC.COS_BAND))


def near_tie(lg, w0, sel, band: float):
    """(Np,) bool: the row is restricted and a counted item OTHER than one at its threshold has a logit within `band` of
    tau (on either side: broader than "the neighbour across the boundary")."""
    _w, tau, _rho, restricted = sel
    d = (lg - tau[:, None]).abs()
    return restricted & ((w0 > 0) & (d > 0) & (d < band)).any(dim=1)


def split_by_multiplicity(lg, w0, sel):
    """(Np,) bool: rho < 1 with ONE item at the threshold -- the item's multiplicity is cut."""
    _w, tau, rho, restricted = sel
    n_at = ((w0 > 0) & (lg == tau[:, None])).sum(dim=1)
    return restricted & (rho < 1) & (n_at == 1)


def tie_between_items(lg, w0, sel, band: float = 0.0):
    """(Np,) bool: rho < 1 and MORE than one counted item at the threshold (|l - tau| <= band)."""
    _w, tau, rho, restricted = sel
    n_at = ((w0 > 0) & ((lg - tau[:, None]).abs() <= band)).sum(dim=1)
    return restricted & (rho < 1) & (n_at > 1)
