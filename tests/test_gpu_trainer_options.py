"""``Trainer``'s Lightning options -- ``gradient_clip_val`` / ``gradient_clip_algorithm``, ``accumulate_grad_batches``,
``lr_scheduler`` -- through ``fit_step`` and ``GraphedStep``: the step against torch's own clip + AdamW on the CPU, fed with
the step's (by design unclipped) ``flat.grad``; accumulated micro-batches against AdamW on their mean gradient; a captured
clipped + scheduled step against the eager one, bit for bit. The model is that of tests/test_gpu_graph.py (B 8, L 24, H 64,
2 layers, V 200, one ragged row) in fp32."""

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def X():
    import xfmr_rec_amd as X

    return X


@pytest.fixture()
def no_dropout(monkeypatch):
    from xfmr_rec_amd import models

    monkeypatch.setattr(models, "HIDDEN_DROPOUT_PROB", 0.0)
    monkeypatch.setattr(models, "ATTENTION_PROBS_DROPOUT_PROB", 0.0)


def _setup(X, B=8, L=24, H=64, V=200, seed=0):
    g = torch.Generator().manual_seed(seed)
    table = torch.randn(V + 1, H, generator=g)
    table = table / table.norm(dim=-1, keepdim=True)
    table[0] = 0
    conf = X.LightningConfig(hidden_size=H, num_attention_heads=H // 32, intermediate_size=2 * H, num_hidden_layers=2,
                             max_seq_length=L, precision="fp32")
    mod = X.RecommenderLightningModule(conf)
    mod.configure_model()
    mod.model.set_table(table.to(DEV))
    batches = []
    for i in range(5):
        b = {k: torch.randint(1, V + 1, (B, L), generator=g) for k in ("history_item_idx", "pos_item_idx", "neg_item_idx")}
        n = 5 + 3 * i
        for k in b:
            b[k][1, n:] = 0  # one ragged row
        batches.append({k: v.to(DEV) for k, v in b.items()})
    return mod, batches


def _cpu_adamw(p0, lr=1e-3, weight_decay=0.01):
    ref = torch.nn.Parameter(p0.detach().cpu().clone())
    return ref, torch.optim.AdamW([ref], lr=lr, weight_decay=weight_decay)


def test_clip_through_the_trainer_matches_torch_clip_and_adamw(X, no_dropout):
    twin, batches = _setup(X)
    tr_twin = X.Trainer(twin, gradient_clip_val=1e30)  # never active: its grad/norm is the unclipped first step's norm
    tr_twin.fit_step(batches[0])
    norm1 = float(twin.logged["grad/norm"])
    assert float(twin.logged["grad/clip_coef"]) == 1.0 and norm1 > 0
    mod, _ = _setup(X)
    clip = 0.5 * norm1
    tr = X.Trainer(mod, gradient_clip_val=clip)
    assert tr.optimizer.clip_mode == "norm"
    ref, opt = _cpu_adamw(mod.model.flat)
    for i in range(3):
        tr.fit_step(batches[i])
        grad = mod.model.flat.grad.detach().cpu()  # unclipped by design: the clip is folded into the AdamW launch
        ref.grad = grad.clone()
        total = torch.nn.utils.clip_grad_norm_([ref], clip)
        opt.step()
        got_norm, got_coef = float(mod.logged["grad/norm"]), float(mod.logged["grad/clip_coef"])
        want_norm = float(grad.double().norm())
        print(f"step {i + 1}: grad/norm {got_norm!r} |flat.grad| {want_norm!r} torch {float(total)!r} coef {got_coef!r}")
        assert abs(got_norm - want_norm) <= 1e-5 * want_norm
        assert got_coef < 1.0
        assert float(mod.logged["lr"]) == pytest.approx(1e-3, rel=1e-6)
    err = float((mod.model.flat.detach().cpu() - ref.detach()).abs().max())
    print(f"max |p - p_ref| after three clipped steps: {err:.3e}")
    assert err <= 3e-5


def test_value_clip_algorithm_reaches_the_optimizer(X, no_dropout):
    mod, batches = _setup(X)
    tr = X.Trainer(mod, gradient_clip_val=1e-4, gradient_clip_algorithm="value")
    ref, opt = _cpu_adamw(mod.model.flat)
    tr.fit_step(batches[0])
    ref.grad = mod.model.flat.grad.detach().cpu().clone()
    assert float((ref.grad.abs() > 1e-4).float().mean()) > 0.01  # the clamp is active
    torch.nn.utils.clip_grad_value_([ref], 1e-4)
    opt.step()
    torch.testing.assert_close(mod.model.flat.detach().cpu(), ref.detach(), rtol=1e-5, atol=1e-7)


def test_accumulate_two_micro_batches_is_adamw_on_their_mean_gradient(X, no_dropout):
    mod, batches = _setup(X)
    tr = X.Trainer(mod, accumulate_grad_batches=2)
    assert tr.optimizer.param_groups[0]["grad_scale"] == 0.5
    flat = mod.model.flat
    p0 = flat.detach().clone()
    # g1, g2 from a twin with the same initial weights that only runs backward
    twin, _ = _setup(X)
    twin.train()
    assert torch.equal(twin.model.flat, p0)
    grads = []
    for b in batches[:2]:
        twin.model.flat.grad = None
        twin.backward(twin.training_step(b, 0))
        twin.on_train_batch_end(None, b, 0)
        grads.append(twin.model.flat.grad.detach().cpu().clone())
    assert not torch.allclose(grads[0], grads[1])
    tr.fit_step(batches[0])
    torch.cuda.synchronize()
    assert torch.equal(flat, p0)  # micro-step 1: parameters untouched, no optimizer step taken
    assert all(st.get("step", 0) == 0 for st in tr.optimizer.state.values()) and "grad/norm" not in mod.logged
    tr.fit_step(batches[1])
    ref, opt = _cpu_adamw(p0)
    ref.grad = (grads[0] + grads[1]) / 2
    opt.step()
    torch.testing.assert_close(flat.detach().cpu(), ref.detach(), rtol=1e-5, atol=1e-7)
    assert [st["step"] for st in tr.optimizer.state.values()] == [1]
    # the next cycle's first micro-step leaves parameters AND moments alone
    st = tr.optimizer.state[flat]
    p1, m1, v1 = flat.detach().clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone()
    tr.fit_step(batches[2])
    torch.cuda.synchronize()
    assert torch.equal(flat, p1) and torch.equal(st["exp_avg"], m1) and torch.equal(st["exp_avg_sq"], v1) and st["step"] == 1


def test_micro_batches_draw_their_own_dropout_masks(X, monkeypatch):
    """The same batch twice inside one accumulated step (the parameters do not change in between): with dropout 0.1 the two
    losses differ -- each forward advances the dropout stream --, with dropout 0 they are equal."""
    mod, batches = _setup(X)
    tr = X.Trainer(mod, accumulate_grad_batches=2)
    a, b = float(tr.fit_step(batches[0])), float(tr.fit_step(batches[0]))
    assert a != b
    from xfmr_rec_amd import models

    monkeypatch.setattr(models, "HIDDEN_DROPOUT_PROB", 0.0)
    monkeypatch.setattr(models, "ATTENTION_PROBS_DROPOUT_PROB", 0.0)
    mod, _ = _setup(X)
    tr = X.Trainer(mod, accumulate_grad_batches=2)
    a, b = float(tr.fit_step(batches[0])), float(tr.fit_step(batches[0]))
    assert a == b


def test_graphed_clipped_scheduled_step_replays_the_eager_step_bit_for_bit(X):
    """GraphedStep(overlap=False) with clip on, the warmup-linear schedule and dropout on: norm, clip coefficient and
    learning rate are written and read on the device, so four replays == four eager steps with the same device counter,
    on the parameters and on the control record."""
    opts = dict(gradient_clip_val=1e-3, lr_scheduler={"name": "warmup_linear", "warmup_steps": 2, "total_steps": 10})
    eager, batches = _setup(X)
    eager.model.use_device_step(True)
    tr_e = X.Trainer(eager, **opts)
    tr_e.optimizer.step_device = eager.model.step_device
    graphed, _ = _setup(X)
    tr_g = X.Trainer(graphed, **opts)
    step = X.GraphedStep(tr_g, batches[0], warmup=3, overlap=False)
    for _ in range(3):
        tr_e.fit_step(batches[0])
    torch.cuda.synchronize()
    assert int(eager.model.step_device) == int(graphed.model.step_device) == 3
    assert torch.equal(eager.model.flat, graphed.model.flat)
    lrs = []
    for b in batches[1:5]:
        loss_e = tr_e.fit_step(b).clone()
        loss_g = step(b).clone()
        torch.cuda.synchronize()
        assert float(loss_e) == float(loss_g)
        assert torch.equal(eager.model.flat, graphed.model.flat)
        assert torch.equal(tr_e.optimizer.ctl.view(torch.int32), tr_g.optimizer.ctl.view(torch.int32))
        assert float(step.logged["grad/clip_coef"]) < 1.0 and float(step.logged["grad/norm"]) > 0
        assert float(step.logged["lr"]) == float(eager.logged["lr"])
        lrs.append(float(step.logged["lr"]))
    # steps 4 .. 7 of warmup 2 / total 10: s = 3 .. 6 completed steps, factor (10 - s) / 8
    assert lrs == pytest.approx([1e-3 * (10 - s) / 8 for s in (3, 4, 5, 6)], rel=1e-6)


def test_capture_of_an_accumulated_step_is_refused(X):
    mod, batches = _setup(X)
    tr = X.Trainer(mod, accumulate_grad_batches=2)
    with pytest.raises(ValueError, match="accumulate_grad_batches"):
        X.GraphedStep(tr, batches[0])
    with pytest.raises(ValueError, match="accumulate_grad_batches"):
        tr.fit(batches[:2], graph="on")
