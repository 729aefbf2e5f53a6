"""bf16 attention at head size 32 beyond the whole-panel LDS limit (L > 1152 backward, > 1248 forward): the key-streaming
forms of the production two-kernel family against an fp64 reference, bit for bit against the panel two-kernel forms where
both run, against the host model of the dropout mask, and through the encoder (bf16 storage) and a whole training step at
L = 1300 against the CPU oracle."""

import numpy as np
import pytest
import torch

import dropout_model as dm
from helpers import assert_close, grad_tol, loss_tol, ragged_batch, rel_l2, unit_table

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16
DH = 32


@pytest.fixture(scope="module")
def ops():
    from xfmr_rec_amd import ops as _ops

    return _ops


@pytest.fixture(scope="module")
def X():
    import xfmr_rec_amd as x

    return x


def _rand(*shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g)


def _attention_reference(qkv, key_mask, A, causal=True):
    """fp64 eager attention (TF:modeling_bert.py:111-136) with the causal + padding mask (causal=False: the padding mask
    alone); a query with no visible key gets zeros."""
    B, L, H3 = qkv.shape
    H = H3 // 3
    dh = H // A
    q, k, v = (t.view(B, L, A, dh).transpose(1, 2) for t in qkv.split(H, dim=-1))
    scores = q @ k.transpose(2, 3) * dh**-0.5
    tri = torch.ones(L, L, dtype=torch.bool)
    allowed = (tri.tril() if causal else tri)[None] & key_mask.bool()[:, None, :]
    scores = scores.masked_fill(~allowed[:, None], float("-inf"))
    probs = torch.nan_to_num(torch.softmax(scores, dim=-1), nan=0.0)
    return (probs @ v).transpose(1, 2).reshape(B, L, H)


def _inputs(B, L, A, dh, lengths, seed=3):
    H = dh * A
    qkv = _rand(B, L, 3 * H, seed=seed)
    mask = torch.zeros(B, L, dtype=torch.uint8)
    for b, n in enumerate(lengths):
        mask[b, :n] = 1
    mask[-1, lengths[-1] // 2] = 0  # a hole in the middle of the last sequence
    mask[-1, 2] = 0
    w = _rand(B, L, H, seed=seed + 1) * mask[..., None]  # the training path only back-propagates valid rows
    return qkv, mask, w


# ------------------------------------------------------------------------------------------ kernels vs fp64
@pytest.mark.parametrize("causal", [True, False], ids=["causal", "bidirectional"])
@pytest.mark.parametrize("B,L,lengths", [(2, 1153, [1153, 1116]),  # panel forward into streaming dQ and dK/dV
                                         (2, 1300, [1300, 1263]),  # both passes streaming; no multiple of 32 or the chunk
                                         (1, 2048, [2048])])       # an exact multiple of the chunk
def test_long_bf16_attention_vs_fp64(ops, B, L, lengths, causal):
    """Lengths whose whole Q/dO (1153) or K/V (1300, 2048) panel does not fit LDS: the launchers take the key-streaming
    forms of the bf16 head-size-32 kernels."""
    A = 2
    qkv, mask, w = _inputs(B, L, A, DH, lengths)
    ref_in = qkv.clone().double().requires_grad_(True)
    ref = _attention_reference(ref_in, mask, A, causal)
    (ref * w.double()).sum().backward()
    ctx, lse = ops.attn_fwd(qkv.to(DEV), mask.to(DEV), A, precision="bf16", causal=causal)
    valid = mask.bool()
    assert_close("attn.ctx", ctx.cpu()[valid], ref.detach()[valid], "bf16")
    d_qkv = ops.attn_bwd(qkv.to(DEV), mask.to(DEV), ctx, lse, w.to(DEV), A, precision="bf16", causal=causal)
    assert_close("attn.d_qkv", d_qkv, ref_in.grad, "bf16", "grad")


# ------------------------------------------------------------------------------------------ streaming == panel
def _both_forms(ops, L, causal, dropout_p):
    B, A = 3, 2
    qkv, mask, w = _inputs(B, L, A, DH, [L, L - 9, 5], seed=11)
    qkv, mask, w = qkv.to(DEV), mask.to(DEV), w.to(DEV)
    kw = dict(precision="bf16", causal=causal, dropout_p=dropout_p, seed=1234, site=5)
    out = {}
    for stream in (False, True):
        ctx, lse = ops.attn_fwd(qkv, mask, A, stream_keys=stream, **kw)
        d_qkv = ops.attn_bwd(qkv, mask, ctx, lse, w, A, stream_keys=stream, **kw)
        out[stream] = (ctx, lse, d_qkv)
    return out, mask


@pytest.mark.parametrize("dropout_p", [0.0, 0.1])
@pytest.mark.parametrize("causal,L", [(False, 40), (False, 200), (True, 640), (True, 1024)],
                         ids=["bidirectional-40", "bidirectional-200", "causal-640", "causal-1024"])
def test_streaming_equals_panel_bf16(ops, causal, L, dropout_p):
    """XFMR_ATTN_STREAM_KEYS forces the key-streaming form where the two-kernel panel form is the default (bidirectional at
    any L; causal above the one-workgroup forms' 512): same blocks in the same order, same per-tile arithmetic and dropout
    keys -- ctx, lse and d_qkv bit-identical."""
    out, _ = _both_forms(ops, L, causal, dropout_p)
    for name, a, b in zip(("ctx", "lse", "d_qkv"), out[False], out[True]):
        assert torch.equal(a, b), (name, (a - b).abs().max().item())
    assert out[True][2].abs().sum().item() > 0


def test_streaming_vs_one_workgroup_forms_bf16(ops):
    """Causal L = 200: the default is the one-workgroup forward and the fused backward, which walk the tiles in another
    order -- the streaming form agrees with them within the bf16 tolerances, not bit for bit."""
    out, mask = _both_forms(ops, 200, True, 0.0)
    valid = mask.bool().cpu()
    assert_close("attn.ctx", out[True][0].cpu()[valid], out[False][0].cpu()[valid], "bf16")
    assert_close("attn.lse", out[True][1], out[False][1], "bf16")
    assert_close("attn.d_qkv", out[True][2], out[False][2], "bf16", "grad")
    assert out[True][2].abs().sum().item() > 0


# ------------------------------------------------------------------------------------------ the dropout mask
@pytest.mark.parametrize("causal", [True, False], ids=["causal", "bidirectional"])
def test_long_bf16_attention_draws_the_host_mask(ops, causal):
    """The construction of test_gpu_dropout_reference.py::test_attention_kernels_draw_the_host_mask at L = 1300, where
    keys and rows lie beyond any panel and in later chunks: q = k = 0 makes every visible key's probability
    1 / n_visible(q), and v[key, d] = 1 iff key = d + 32 j makes ctx[b, q, h, d] = keep(q, d + 32 j) / (1 - p) /
    n_visible(q), so ceil(L / 32) forwards spell out the (B, A, L, L) mask on the visible pairs."""
    B, A, L, p = 1, 2, 1300, 0.1
    seed, site = 6018027440424182934, dm.site_attn(1)  # both halves of the 64-bit seed in use
    H = DH * A
    mask = torch.ones(B, L, dtype=torch.uint8)
    tri = torch.ones(L, L, dtype=torch.bool)
    vis = ((tri.tril() if causal else tri)[None] & mask.bool()[:, None, :])[:, None].expand(B, A, L, L)
    nvis = vis.sum(-1).clamp(min=1).float()  # (B, A, q)
    want = torch.from_numpy(dm.attention_keep(seed, site, B, A, L, p)).bool()
    got = torch.zeros(B, A, L, L, dtype=torch.bool)
    mdev = mask.to(DEV)
    val = float(torch.tensor(float(np.float32(dm.scale(p)))).to(BF16)) / nvis[..., None]  # the probability operand is bf16
    for j in range((L + DH - 1) // DH):
        qkv = torch.zeros(B, L, 3 * H)
        v = qkv[..., 2 * H:].view(B, L, A, DH)
        n = min(DH, L - DH * j)
        v[:, DH * j + torch.arange(n), :, torch.arange(n)] = 1.0
        ctx, _ = ops.attn_fwd(qkv.to(DEV), mdev, A, dropout_p=p, seed=seed, site=site, precision="bf16", causal=causal)
        c = ctx.cpu().view(B, L, A, DH).permute(0, 2, 1, 3)[..., :n]  # (B, A, q, key - 32 j)
        got[..., DH * j:DH * j + n] = c != 0
        ref = vis[..., DH * j:DH * j + n] & want[..., DH * j:DH * j + n]
        torch.testing.assert_close(c, ref.float() * val, rtol=2e-6, atol=0)
    assert torch.equal(got & vis, want & vis)
    assert not bool((got & ~vis).any())
    assert 0.85 < float(got[vis].float().mean()) < 0.95


# ------------------------------------------------------------------------------------------ encoder at L = 1300
def test_encoder_bf16_at_1300_vs_oracle(X):
    """The bf16 policy keeps qkv / ctx in bf16 storage, so the encoder runs the S16 instantiations of the streaming kernels
    (ops.attn_* passes fp32 operands): H 64, 2 heads (head size 32), I 128, 2 layers at L = 1300."""
    from oracle import model as OM

    prec, B, L, H, A, I, nL, V = "bf16", 3, 1300, 64, 2, 128, 2, 300
    table = unit_table(V, H)
    batch, lengths = ragged_batch(B, L, V, lengths=[1300, 700, 5], seed=2)
    cfg = X.ModelConfig(hidden_size=H, num_attention_heads=A, intermediate_size=I, num_hidden_layers=nL, max_seq_length=L)
    m = X.RecommenderModel(cfg, device=DEV, precision=prec)
    m.set_table(table.to(DEV))
    m.eval()
    params = {k: v.detach().cpu().clone().requires_grad_(True) for k, v in m.encoder_state_dict().items()}
    ref = OM.forward(params, table, batch["history_item_idx"], num_heads=A, max_seq_length=L)
    out = m(batch["history_item_idx"].to(DEV))
    valid = ref["attention_mask"].bool()
    assert torch.equal(out["attention_mask"].cpu().bool(), valid)
    assert_close("tok", out["token_embeddings"].cpu()[valid], ref["token_embeddings"].detach()[valid], prec)
    assert_close("sentence_embedding", out["sentence_embedding"], ref["sentence_embedding"].detach(), prec)
    w = torch.linspace(-1, 1, H)
    (ref["token_embeddings"] * w * valid[..., None]).sum().backward()
    (out["token_embeddings"] * w.to(DEV) * valid.to(DEV)[..., None]).sum().backward()
    got = m.grad_state_dict()
    for k, p in params.items():
        if k.endswith("key.bias"):  # exactly zero in exact arithmetic
            continue
        assert_close(k, got[k], p.grad, prec, "grad")


# ------------------------------------------------------------------------------------------ training step at L = 1300
def test_training_step_bf16_at_1300_vs_oracle(X):
    """The whole bf16 step -- encoder, the fused loss of all seven heads, backward -- at L = 1300 against the oracle's."""
    from oracle import model as OM

    H, A, I, L, V, B = 64, 2, 128, 1300, 300, 3
    train_loss = "InfoNCELoss"
    table = unit_table(V, H)
    batch, lengths = ragged_batch(B, L, V, lengths=[1300, 300, 5], seed=5)
    conf = X.LightningConfig(hidden_size=H, num_attention_heads=A, intermediate_size=I, num_hidden_layers=1,
                             max_seq_length=L, precision="bf16", train_loss=train_loss)
    mod = X.RecommenderLightningModule(conf)
    mod.configure_model()
    mod.model.set_table(table.to(DEV))
    mod.eval()
    params = {k: v.detach().cpu().clone().requires_grad_(True) for k, v in mod.model.encoder_state_dict().items()}
    want = OM.compute_losses(params, table, batch, num_heads=A, max_seq_length=L, loss_cfg={}, resolve_ties=True)
    want[f"loss/{train_loss}"].backward()
    out = mod.compute_losses(batch)
    out[f"loss/{train_loss}"].backward()
    for cls in X.LOSS_CLASSES:
        k = f"loss/{cls.__name__}"
        w = float(want[k].detach())
        assert abs(float(out[k]) - w) <= loss_tol("bf16", w, flips=True), (k, float(out[k]), w)
    got = mod.model.grad_state_dict()
    for k, p_ in params.items():
        if k.endswith("key.bias"):
            continue
        e = rel_l2(got[k], p_.grad)
        assert e <= grad_tol("bf16", flips=True), (k, e)
