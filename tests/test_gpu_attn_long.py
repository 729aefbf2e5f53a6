"""Attention beyond the whole-panel LDS limit: the key-streaming forms of the generic kernels (fp32 policy at head size 32
and 64, bf16 policy at head size 64) against an fp64 reference up to L = 1024, bit for bit against the panel kernels where
both run, and through the encoder and a whole training step at L = 512 against the CPU oracle."""

import pytest
import torch

from helpers import assert_close, grad_tol, loss_tol, ragged_batch, rel_l2, unit_table

pytestmark = pytest.mark.gpu
DEV = "cuda"


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
@pytest.mark.parametrize("prec,dh,L", [("fp32", 32, 320), ("fp32", 32, 512), ("fp32", 32, 1024),
                                       ("fp32", 64, 200), ("fp32", 64, 512),
                                       ("bf16", 64, 320), ("bf16", 64, 512), ("bf16", 64, 1024)])
def test_long_attention_vs_fp64(ops, prec, dh, L, causal):
    """Lengths whose whole K/V (Q/dO) panel does not fit LDS: the launchers take the key-streaming forms."""
    B, A = 2, 2
    qkv, mask, w = _inputs(B, L, A, dh, [L, L - 37])
    ref_in = qkv.clone().double().requires_grad_(True)
    ref = _attention_reference(ref_in, mask, A, causal)
    (ref * w.double()).sum().backward()
    ctx, lse = ops.attn_fwd(qkv.to(DEV), mask.to(DEV), A, precision=prec, causal=causal)
    valid = mask.bool()
    assert_close("attn.ctx", ctx.cpu()[valid], ref.detach()[valid], prec)
    d_qkv = ops.attn_bwd(qkv.to(DEV), mask.to(DEV), ctx, lse, w.to(DEV), A, precision=prec, causal=causal)
    assert_close("attn.d_qkv", d_qkv, ref_in.grad, prec, "grad")


# ------------------------------------------------------------------------------------------ streaming == panel
@pytest.mark.parametrize("dropout_p", [0.0, 0.1])
@pytest.mark.parametrize("causal", [True, False], ids=["causal", "bidirectional"])
@pytest.mark.parametrize("prec,dh,L", [("fp32", 32, 40), ("fp32", 32, 130), ("fp32", 32, 256),
                                       ("fp32", 64, 40), ("fp32", 64, 128),
                                       ("bf16", 64, 200), ("bf16", 64, 256)])
def test_streaming_equals_panel(ops, prec, dh, L, causal, dropout_p):
    """XFMR_ATTN_STREAM_KEYS forces the key-streaming form where the panel kernels run: same blocks in the same order,
    same per-block arithmetic and dropout keys -- ctx, lse and d_qkv bit-identical."""
    B, A = 3, 2
    qkv, mask, w = _inputs(B, L, A, dh, [L, L - 9, 5], seed=11)
    qkv, mask, w = qkv.to(DEV), mask.to(DEV), w.to(DEV)
    kw = dict(precision=prec, causal=causal, dropout_p=dropout_p, seed=1234, site=5)
    out = {}
    for stream in (False, True):
        ctx, lse = ops.attn_fwd(qkv, mask, A, stream_keys=stream, **kw)
        d_qkv = ops.attn_bwd(qkv, mask, ctx, lse, w, A, stream_keys=stream, **kw)
        out[stream] = (ctx, lse, d_qkv)
    for name, a, b in zip(("ctx", "lse", "d_qkv"), out[False], out[True]):
        assert torch.equal(a, b), (name, (a - b).abs().max().item())
    assert out[True][2].abs().sum().item() > 0


def test_stream_keys_mode_bits(ops):
    """Modes 0-3 are accepted (causal / bidirectional, with or without the streaming bit); any other bit is EINVAL."""
    from xfmr_rec_amd import _native as N

    B, L, A, H = 1, 64, 2, 64
    qkv, mask, _ = _inputs(B, L, A, H // A, [L])
    qkv, mask = qkv.to(DEV), mask.to(DEV)
    ctx, lse = torch.empty(B, L, H, device=DEV), torch.empty(B, A, L, device=DEV)
    lib = N.load()

    def run(mode):
        rc = lib.xfmr_attn_fwd_mode(N.ptr(qkv), N.ptr(mask), N.ptr(ctx), N.ptr(lse), B, L, A, H, 0.0, 0, 0, N.PREC_F32,
                                    mode, N.stream())
        torch.cuda.synchronize()
        return rc

    for mode in (0, 1, 2, 3):
        assert run(mode) == 0, mode
    for mode in (4, 6, -1):
        assert run(mode) == -1, mode  # XFMR_EINVAL


# ------------------------------------------------------------------------------------------ encoder at L = 512
def _encoder_vs_oracle(X, prec, *, B, L, H, A, I, nL, V, lengths):
    from oracle import model as OM

    table = unit_table(V, H)
    batch, lengths = ragged_batch(B, L, V, lengths=lengths, seed=2)
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


def test_encoder_config5_fp32_at_512_vs_oracle(X):
    """BASELINE config 5's layer shape (H 256, 8 heads, I 1024; 2 layers) at L = 512 in the fp32 parity policy."""
    _encoder_vs_oracle(X, "fp32", B=3, L=512, H=256, A=8, I=1024, nL=2, V=300, lengths=[512, 300, 5])


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("H,A,I", [(768, 12, 192), (128, 2, 256)])
def test_encoder_head64_at_512_vs_oracle(X, prec, H, A, I):
    """Head size 64 at L = 512: all-mpnet's 768 / 12 and 128 / 2. The bf16 policy keeps qkv / ctx in bf16 storage, so
    its cases run the S16 streaming kernels."""
    _encoder_vs_oracle(X, prec, B=3, L=512, H=H, A=A, I=I, nL=2, V=300, lengths=[512, 300, 5])


# ------------------------------------------------------------------------------------------ training steps at L = 512
def test_all_mpnet_defaults_train(X):
    """sentence-transformers/all-mpnet-base-v2 resolves to 768 / 12 (head size 64), I 3072 and max_seq_length 512: one
    bf16 loss + backward on a ragged 4 x 512 batch."""
    from oracle import model as OM

    conf = X.LightningConfig(pretrained_model_name="sentence-transformers/all-mpnet-base-v2", hidden_size=None,
                             num_attention_heads=None, intermediate_size=None, max_seq_length=None, num_hidden_layers=1,
                             precision="bf16")
    mod = X.RecommenderLightningModule(conf)
    mod.configure_model()
    c = mod.model.config
    assert (c.hidden_size, c.num_attention_heads, c.intermediate_size, c.max_seq_length) == (768, 12, 3072, 512)
    H, A, L, V, B = 768, 12, 512, 200, 4
    table = unit_table(V, H)
    mod.model.set_table(table.to(DEV))
    mod.eval()
    batch, lengths = ragged_batch(B, L, V, lengths=[512, 301, 7, 512], seed=7)
    params = {k: v.detach().cpu().clone() for k, v in mod.model.encoder_state_dict().items()}
    ref = OM.forward(params, table, batch["history_item_idx"], num_heads=A, max_seq_length=L)
    with torch.no_grad():
        enc = mod.model(batch["history_item_idx"].to(DEV))
    valid = ref["attention_mask"].bool()
    assert_close("tok", enc["token_embeddings"].cpu()[valid], ref["token_embeddings"][valid], "bf16")
    out = mod.compute_losses(batch)
    loss = out["loss/InfoNCELoss"]
    assert torch.isfinite(loss).item()
    loss.backward()
    grads = mod.model.grad_state_dict()
    for k, g in grads.items():
        assert torch.isfinite(g).all().item(), k
    assert grads["encoder.layer.0.attention.self.query.weight"].abs().sum().item() > 0


def test_training_step_config5_fp32_at_512_vs_oracle(X):
    """The whole fp32 step -- encoder, the fused loss of all seven heads, backward -- at config 5's layer shape and
    L = 512, against the oracle's."""
    from oracle import model as OM

    H, A, I, L, V, B = 256, 8, 1024, 512, 300, 4
    train_loss = "InfoNCELoss"
    table = unit_table(V, H)
    batch, lengths = ragged_batch(B, L, V, lengths=[512, 300, 5, 512], seed=5)
    conf = X.LightningConfig(hidden_size=H, num_attention_heads=A, intermediate_size=I, num_hidden_layers=1,
                             max_seq_length=L, precision="fp32", train_loss=train_loss)
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
        assert abs(float(out[k]) - w) <= loss_tol("fp32", w, flips=True), (k, float(out[k]), w)
    got = mod.model.grad_state_dict()
    for k, p_ in params.items():
        if k.endswith("key.bias"):
            continue
        e = rel_l2(got[k], p_.grad)
        assert e <= grad_tol("fp32", flips=True), (k, e)
