"""The PACKED layout (xfmr_encoder_cfg.seq_offsets) beyond 512 rows per sequence: attention runs its key-streaming bf16
head-size-32 kernels, which walk each sequence by its offsets -- its own start, its own length, workgroups past its end
leave at once. They run the same 32-row tiles in the same order as the padded layout's two-kernel forms, so valid rows
must come out as the padded layout computes them: the forward bit for bit, weight gradients to fp32 summation order. lse
and the dropout row keys stay indexed by slot * seq_len + q (tests/dropout_model.py), which the dropout case pins against
the host model's masks. Then the product API: the training step and encode_batch take the packed route at these lengths."""

import ctypes

import numpy as np
import pytest
import torch

from helpers import TOL, grad_tol, loss_tol, max_scaled_err, rel_l2, unit_table
from test_gpu_model import _encoder_shape_vs_oracle
from test_gpu_packed import _module, _offsets, _ragged

pytestmark = pytest.mark.gpu
DEV = "cuda"
H, A, I, V = 64, 2, 128, 300

CASES = [
    # B not a multiple of 8, an empty and a one-row sequence, exactly one 128-row block, one block + 1, chunk (256) + 1, L not a
    # multiple of 32; the padded side runs the panel two-kernel forms
    (9, 520, 2, [520, 513, 300, 129, 128, 33, 1, 0, 257]),
    # the shortest sequence first; both sides stream (the panels stop fitting at 1152 / 1248 rows)
    (4, 1300, 1, [5, 1300, 700, 1153]),
    # exact chunk multiples
    (2, 2048, 1, [2048, 1024]),
]


@pytest.fixture(scope="module")
def X():
    import xfmr_rec_amd as pkg

    return pkg


@pytest.fixture(scope="module")
def ops():
    from xfmr_rec_amd import ops as o

    return o


def _packed_vs_padded(ops, B, L, nL, lengths, ordered=False):
    """test_gpu_packed.py's construction at these lengths: the packed run in slot order against the padded run. Returns the
    packed run's (tok, gradient); `ordered`: additionally the run packed longest first, its tok back in slot order."""
    from xfmr_rec_amd import _native as N

    g = torch.Generator().manual_seed(11)
    table = unit_table(V, H).to(DEV)
    batch = _ragged(B, L, V, lengths, seed=5)
    idx = batch["history_item_idx"].to(DEV)
    off = _offsets(lengths)
    rows = int(off[-1])
    pk = ops.pack_rows(idx, batch["pos_item_idx"].to(DEV), None, off.to(DEV), rows)
    kw = dict(batch=B, seq_len=L, hidden=H, heads=A, inter=I, layers=nL, max_pos=L, precision="bf16")
    cfg_pad = ops.make_encoder_cfg(**kw)
    cfg_pk = ops.make_encoder_cfg(**kw, seq_offsets=pk["seq_offsets"], row_pos=pk["row_pos"])
    n_params = N.load().xfmr_param_count(ctypes.byref(cfg_pad))
    flat = (0.05 * torch.randn(n_params, generator=g)).to(DEV)
    valid = (torch.arange(L)[None, :] < torch.tensor(lengths)[:, None]).to(DEV)
    tok_p, km_p, acts_p = ops.encoder_fwd(cfg_pad, flat, idx, table)
    tok_k, km_k, acts_k = ops.encoder_fwd(cfg_pk, flat, pk["hist"], table)
    assert tok_k.shape == (rows, H) and km_k.shape == (rows,)
    assert torch.equal(tok_k, tok_p[valid]) and torch.equal(km_k, km_p[valid])
    d_out = torch.randn(B, L, H, generator=g).to(DEV) * valid[..., None]  # padding rows carry no gradient (models.py:392)
    g_p = ops.encoder_bwd(cfg_pad, flat, d_out.clone(), km_p, acts_p)
    g_k = ops.encoder_bwd(cfg_pk, flat, d_out[valid].contiguous(), km_k, acts_k)
    assert torch.isfinite(g_k).all() and float(g_k.abs().max()) > 0
    assert rel_l2(g_k, g_p) <= 2e-5, rel_l2(g_k, g_p)  # (weight gradients sum the rows in another order)
    g_k2 = ops.encoder_bwd(cfg_pk, flat, d_out[valid].contiguous(), km_k, acts_k)
    assert torch.equal(g_k, g_k2)  # bit-reproducible
    if not ordered:
        return
    # longest first, as the trainer packs (ops.length_order): slot b holds sequence order[b]
    order, off_o = ops.length_order(lengths)
    assert [lengths[i] for i in order.tolist()] == sorted(lengths, reverse=True) != list(lengths)
    pk_o = ops.pack_rows(idx, batch["pos_item_idx"].to(DEV), None, off_o.to(DEV), rows, order=order.to(DEV))
    cfg_o = ops.make_encoder_cfg(**kw, seq_offsets=pk_o["seq_offsets"], row_pos=pk_o["row_pos"])
    tok_o, km_o, acts_o = ops.encoder_fwd(cfg_o, flat, pk_o["hist"], table)
    for slot, b in enumerate(order.tolist()):  # undo the order: sequence b's rows of both runs
        assert torch.equal(tok_o[int(off_o[slot]):int(off_o[slot + 1])], tok_k[int(off[b]):int(off[b + 1])]), b
    order_d = order.to(DEV)
    g_o = ops.encoder_bwd(cfg_o, flat, d_out[order_d][valid[order_d]].contiguous(), km_o, acts_o)
    assert rel_l2(g_o, g_k) <= 2e-5, rel_l2(g_o, g_k)


@pytest.mark.parametrize("B,L,nL,lengths", CASES, ids=[f"L{c[1]}" for c in CASES])
def test_packed_encoder_equals_the_padded_layout_on_valid_rows(ops, B, L, nL, lengths):
    _packed_vs_padded(ops, B, L, nL, lengths)


def test_packed_longest_first_equals_the_slot_order_run(ops):
    B, L, nL, lengths = CASES[1]
    _packed_vs_padded(ops, B, L, nL, lengths, ordered=True)


def test_training_mode_packed_encoder_vs_oracle_beyond_512(X, monkeypatch):
    """Dropout on: tok and every gradient against the oracle under the host model's masks -- the attention masks are keyed
    by slot * seq_len + q and the key's position, whatever the sequence's offset is (the helper's tolerances)."""
    _encoder_shape_vs_oracle(X, "bf16", B=3, L=600, H=H, A=A, I=I, nL=2, V=V, lengths=[600, 257, 5], dropout=monkeypatch,
                             packed=True)


def test_packed_training_step_equals_the_padded_step_and_the_oracle_beyond_512(X, ops, monkeypatch):
    """compute_losses on a batch that carries its rows' lengths runs packed at max_seq_length 600 (one pack_rows call): every
    logged scalar equals the padded step's bit for bit, the gradient to summation order, both agree with the CPU oracle."""
    from oracle import model as OM

    B, L, V_, nL = 4, 600, 100, 1
    lengths = [600, 300, 0, 17]
    batch = _ragged(B, L, V_, lengths, seed=1, hole=(1, 3))
    calls = []
    real = ops.pack_rows
    monkeypatch.setattr(ops, "pack_rows", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    res = []
    for with_lengths in (False, True):
        mod = _module(X, H=H, A=A, I=I, nL=nL, L=L, V=V_)
        mod.eval()  # dropout off: its masks are keyed by the row index, which the layouts do not share
        b = {k: v.to(DEV) for k, v in batch.items()}
        if with_lengths:
            b["lengths"] = torch.tensor(lengths)
        calls.clear()
        out = mod.compute_losses(b)
        out["loss/InfoNCELoss"].backward()
        assert len(calls) == int(with_lengths)
        res.append((out, mod.model.flat.grad.clone(), mod))
    (o0, g0, mod0), (o1, g1, mod1) = res
    n = 0
    for k, v in o0.items():
        if torch.is_tensor(v) and v.dim() == 0 or isinstance(v, (int, float)):
            n += 1
            assert float(o1[k]) == float(v) or (float(v) != float(v) and float(o1[k]) != float(o1[k])), (k, float(v), float(o1[k]))
    assert n >= 3 and float(g0.abs().max()) > 0
    assert rel_l2(g1, g0) <= 2e-5, rel_l2(g1, g0)
    params = {k: v.detach().cpu().clone().requires_grad_(True) for k, v in mod1.model.encoder_state_dict().items()}
    want = OM.compute_losses(params, unit_table(V_, H), batch, num_heads=A, max_seq_length=L, loss_cfg={}, resolve_ties=True)
    want["loss/InfoNCELoss"].backward()
    for out, mod in ((o0, mod0), (o1, mod1)):
        for cls in X.LOSS_CLASSES:
            k = f"loss/{cls.__name__}"
            w = float(want[k].detach())
            assert abs(float(out[k]) - w) <= loss_tol("bf16", w, flips=True), (k, float(out[k]), w)
        got = mod.model.grad_state_dict()
        for k, p_ in params.items():
            if not k.endswith("key.bias"):
                assert rel_l2(got[k], p_.grad) <= grad_tol("bf16", flips=True), k


def test_encode_batch_takes_the_packed_route_beyond_512(X, ops, monkeypatch):
    """A module with max_seq_length 600: supports_packed_rows(600) holds (profiles/packed_long.md: the packed step was not
    slower than the padded one above 512), encode_batch packs once and agrees with the per-row forward; a 700-item history
    keeps its last 600."""
    L = 600
    mod = _module(X, H=H, A=A, I=I, nL=2, L=L, V=V)
    mod.eval()
    m = mod.model
    assert m.supports_packed_rows(L)
    calls = []
    real = ops.pack_rows
    monkeypatch.setattr(ops, "pack_rows", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    rng = np.random.default_rng(1)
    hists = [rng.integers(1, V + 1, n).tolist() for n in (1, 5, 300, 600, 700)]
    got = m.encode_batch(hists)
    assert len(calls) == 1 and got.shape == (len(hists), H)
    for b, h in enumerate(hists):
        want = m(torch.as_tensor(h, device=DEV)[None])["sentence_embedding"][0]  # keeps the last L rows itself
        err = max_scaled_err(got[b], want)
        assert err <= TOL["bf16"]["val"], (b, len(h), err)
    want_last = m(torch.as_tensor(hists[4][-L:], device=DEV)[None])["sentence_embedding"][0]
    assert max_scaled_err(got[4], want_last) <= TOL["bf16"]["val"]
