"""The one-workgroup bf16 attention kernels (attn_fwd_seq_bf16_kernel, attn_bwd_fused_bf16_kernel). The fused backward runs
its score epilogue in a straight line -- dropout and the interior-tile test decided once per tile, one of four instances of
the same arithmetic -- and fetches the key-mask byte of both key tiles of a wave and the wave's row of the lock-step schedule
before its first barrier, so no step loads from global memory. The shapes where that can go wrong:

  L = 200   7 tiles: the benchmark's schedule row, three tile switches, a last tile of 8 valid rows
  L = 33    a second tile of one valid row, one tile switch
  L = 32    a single tile, no switch
  L = 256   the 9-step schedule, which has an idle slot

B = 3 (odd: the XCD-padded grid has invalid blocks), 2 heads of 32; key masks: all valid, a padded tail of 5 keys in one
sequence, a masked key inside one sequence's first tile (a non-interior tile below the diagonal); dropout 0 and 0.1.

Through the public entry points (fp32 storage) and through a 1-layer encoder in the bf16 policy (bf16 storage):
  (a) two runs are bit-equal;
  (b) forward and backward against fp64 at the existing attention / encoder tests' tolerances (fp32_level against the
      kernels' rounding model and helpers.TOL["bf16"] against exact fp64 attention; the encoder against the fp64 oracle under
      the host model's masks, helpers.TOL["bf16"]);
  (c) XFMR_ATTN_BWD_FORM=roles (read per call) agrees with the lock-step form to the form-comparison test's 2e-5."""

import functools

import pytest
import torch

import dropout_model as dm
import test_gpu_model as tgm
from helpers import assert_close, ragged_batch, rel_l2, unit_table
from test_gpu_ops import _attention_bf16_emulation, _attention_reference, _rand, fp32_level

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16
B, A, H = 3, 2, 64
LENGTHS = [200, 33, 32, 256]
MASKS = ["all", "tail", "hole"]
FORM_TOL = 2e-5  # test_attention_backward_roles_form_equals_the_lockstep_form
SEED = 6018027440424182934  # both halves of the 64-bit seed in use


@pytest.fixture(scope="module")
def ops():
    from xfmr_rec_amd import ops as _ops

    return _ops


@pytest.fixture(scope="module")
def X():
    import xfmr_rec_amd as x

    return x


def _key_mask(L, kind):
    mask = torch.ones(B, L, dtype=torch.uint8)
    if kind == "tail":
        mask[1, L - 5:] = 0
    elif kind == "hole":
        mask[1, 2] = 0
    return mask


@functools.lru_cache(maxsize=None)
def _inputs(L, kind):
    """bf16-representable inputs (staging rounds nothing: the rounding model applies), left unchanged."""
    qkv = _rand(B, L, 3 * H, seed=31).to(BF16).float()
    mask = _key_mask(L, kind)
    w = (_rand(B, L, H, seed=32) * mask[..., None]).to(BF16).float()  # the training path only back-propagates valid rows
    return qkv, mask, w


@functools.lru_cache(maxsize=None)
def _keep(L, p):
    if p == 0.0:
        return None
    return torch.from_numpy(dm.attention_keep(SEED, dm.site_attn(0), B, A, L, p).astype("float64")) * dm.scale(p)


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("kind", MASKS)
@pytest.mark.parametrize("L", LENGTHS)
def test_public_entry_points(ops, monkeypatch, L, kind, p):
    qkv, mask, w = _inputs(L, kind)
    keep = _keep(L, p)
    kw = dict(dropout_p=p, seed=SEED, site=dm.site_attn(0), precision="bf16")
    dev = [t.to(DEV) for t in (qkv, mask, w)]
    monkeypatch.delenv("XFMR_ATTN_BWD_FORM", raising=False)
    ctx, lse = ops.attn_fwd(dev[0], dev[1], A, **kw)
    ctx2, lse2 = ops.attn_fwd(dev[0], dev[1], A, **kw)
    d = ops.attn_bwd(dev[0], dev[1], ctx, lse, dev[2], A, **kw)
    d2 = ops.attn_bwd(dev[0], dev[1], ctx, lse, dev[2], A, **kw)
    monkeypatch.setenv("XFMR_ATTN_BWD_FORM", "roles")
    dr = ops.attn_bwd(dev[0], dev[1], ctx, lse, dev[2], A, **kw)
    monkeypatch.delenv("XFMR_ATTN_BWD_FORM", raising=False)
    valid = mask.bool()
    parts = (("dq", slice(0, H)), ("dk", slice(H, 2 * H)), ("dv", slice(2 * H, 3 * H)))
    # the figures first, then the assertions
    want_ctx, want_d, want_lse = _attention_bf16_emulation(qkv, mask, A, w, True, keep=keep, fwd=(ctx, lse))
    ref_in = qkv.clone().double().requires_grad_(True)
    ref = _attention_reference(ref_in, mask, A, True, keep=keep)
    (ref * w.double()).sum().backward()
    form = {n: rel_l2(dr[..., sl], d[..., sl]) for n, sl in parts}
    print(f"FIG straightline public L={L} mask={kind} p={p}: model rel-L2 ctx {rel_l2(ctx.cpu()[valid], want_ctx[valid]):.2e}"
          f"  d_qkv {rel_l2(d, want_d):.2e}; fp64 rel-L2 ctx {rel_l2(ctx.cpu()[valid], ref.detach()[valid]):.2e}"
          f"  d_qkv {rel_l2(d, ref_in.grad):.2e}; roles vs lock-step " + "  ".join(f"{n} {e:.2e}" for n, e in form.items()))
    # (a)
    assert torch.equal(ctx, ctx2) and torch.equal(lse, lse2)
    assert torch.equal(d, d2)
    # (b) the rounding model at the fp32 level, exact fp64 attention at the bf16 tolerances
    fp32_level("attn.ctx", ctx.cpu()[valid], want_ctx[valid])
    rows = valid[:, None, :].expand(B, A, L)
    assert_close("attn.lse", lse.cpu()[rows], want_lse[rows], "fp32")
    fp32_level("attn.d_qkv", d, want_d)
    for name, sl in parts:
        fp32_level(f"attn.{name}", d[..., sl], want_d[..., sl])
    assert_close("attn.ctx", ctx.cpu()[valid], ref.detach()[valid], "bf16")
    for name, sl in parts:
        assert_close(f"attn.{name}", d[..., sl], ref_in.grad[..., sl], "bf16", "grad")
    # (c)
    for name, e in form.items():
        assert e <= FORM_TOL, (name, e)


# ------------------------------------------------------------------------------------------ 1-layer encoder, bf16 storage
ENC = dict(H=H, A=A, I=128, nL=1, V=300)


def _lengths(L, kind):
    return [L, L - 5, L] if kind == "tail" else [L, L, L]


def _batch(L, kind):
    """helpers.ragged_batch, with a padding id at position 2 of sequence 1 for the `hole` mask (the key mask follows the
    embedding VALUES: a zero row is a masked key)."""
    batch, lengths = ragged_batch(B, L, ENC["V"], lengths=_lengths(L, kind), seed=2)
    if kind == "hole":
        batch["history_item_idx"][1, 2] = 0
    return batch, lengths


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("kind", MASKS)
@pytest.mark.parametrize("L", LENGTHS)
def test_encoder_vs_oracle(X, monkeypatch, L, kind, p):
    """(b) through the encoder: test_gpu_model's helper (token embeddings, sentence embedding and every parameter's gradient
    against the oracle at helpers.TOL["bf16"]; p = 0.1: the product's rates under the host model's masks)."""
    from xfmr_rec_amd import models

    assert models.ATTENTION_PROBS_DROPOUT_PROB == 0.1
    monkeypatch.delenv("XFMR_ATTN_BWD_FORM", raising=False)
    monkeypatch.setattr(tgm, "ragged_batch", lambda *a, **k: _batch(L, kind))
    tgm._encoder_shape_vs_oracle(X, "bf16", B=B, L=L, lengths=_lengths(L, kind), dropout=monkeypatch if p else None, **ENC)


def _encoder_step(m, idx, w, train):
    """One forward + backward of sum(tok * w) over the valid rows, at the same dropout step every time."""
    if train:
        m._seed, m._step = 0x5DEECE66D, 6
    m.flat.grad = None
    out = m(idx)
    tok = out["token_embeddings"]
    (tok * w * out["attention_mask"][..., None]).sum().backward()
    return tok.detach().clone(), {k: v.detach().clone() for k, v in m.grad_state_dict().items()}


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("kind", MASKS)
@pytest.mark.parametrize("L", LENGTHS)
def test_encoder_runs_are_bit_equal_and_forms_agree(X, monkeypatch, L, kind, p):
    """(a) and (c) through the encoder. The forms differ in the fp32 summation order of dQ alone, which reaches the
    parameters through the query projection and everything below it."""
    monkeypatch.delenv("XFMR_ATTN_BWD_FORM", raising=False)
    batch, _ = _batch(L, kind)
    m = tgm._model(X, Lmax=L, prec="bf16", table=unit_table(ENC["V"], H), **{k: ENC[k] for k in ("H", "A", "I", "nL")})
    m.load_encoder_state_dict(tgm._perturbed_state([(k, v.shape) for k, v in m.encoder_state_dict().items()]))
    if p:
        m.train()
    idx, w = batch["history_item_idx"].to(DEV), torch.linspace(-1, 1, H).to(DEV)
    tok, g = _encoder_step(m, idx, w, bool(p))
    tok2, g2 = _encoder_step(m, idx, w, bool(p))
    monkeypatch.setenv("XFMR_ATTN_BWD_FORM", "roles")
    _, gr = _encoder_step(m, idx, w, bool(p))
    monkeypatch.delenv("XFMR_ATTN_BWD_FORM", raising=False)
    errs = {k: rel_l2(gr[k], g[k]) for k in g if not k.endswith("key.bias")}  # (key.bias: zero in exact arithmetic)
    worst = max(errs, key=errs.get)
    print(f"FIG straightline encoder L={L} mask={kind} p={p}: roles vs lock-step worst gradient {errs[worst]:.2e} ({worst})")
    assert float(tok.abs().sum()) > 0 and all(float(v.abs().sum()) > 0 for k, v in g.items() if not k.endswith("key.bias"))
    assert torch.equal(tok, tok2)
    for k in g:
        assert torch.equal(g[k], g2[k]), k
    for k, e in errs.items():
        assert e <= FORM_TOL, (k, e)
