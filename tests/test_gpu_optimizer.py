"""The optimizer step's options on the device (include/xfmr_hip.h K18b, csrc/optim.hip): xfmr_opt_prepare (gradient
norm, max |g|, non-finite count, clip coefficient, scheduled learning rate into the 32-byte control record),
xfmr_adamw_ctl (AdamW that consumes the record) and xfmr_grad_accumulate. The references are torch's own on the CPU:
``torch.optim.AdamW``, ``clip_grad_norm_``, ``clip_grad_value_``, ``LambdaLR`` with the transformers formulas."""

import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
COSINE = {"name": "warmup_cosine", "warmup_steps": 2, "total_steps": 5}


@pytest.fixture(scope="module")
def ops():
    from xfmr_rec_amd import ops

    return ops


@pytest.fixture(scope="module")
def N():
    from xfmr_rec_amd import _native as N

    return N


def _rand(n, seed):
    return torch.randn(n, generator=torch.Generator().manual_seed(seed))


def _cosine_lambda(s, W=2, T=5):
    """transformers.optimization.get_cosine_schedule_with_warmup's lr_lambda."""
    if s < W:
        return float(s) / float(max(1, W))
    progress = float(s - W) / float(max(1, T - W))
    return max(0.0, 0.5 * (1.0 + math.cos(math.pi * progress)))


def _ctl_host(ctl, N):
    f = ctl.cpu()
    out = {k: float(f[i]) for k, i in N.CTL.items() if k != "nonfinite"}
    out["nonfinite"] = int(f.view(torch.int32)[N.CTL["nonfinite"]])
    return out


# 1 .. 5: below / at / above one 16-byte group (tail only, groups only, both); 1 023: one workgroup with a tail; 262 151:
# 65 workgroups with a tail; 819 200: config 2's flat buffer, 200 workgroups; 2 100 003: more 16-byte groups than the
# 256 x 1024 threads of the fixed grid, so the grid-stride loop runs its paired and its single iteration
@pytest.mark.parametrize("n,offset", [(1, 0), (3, 0), (4, 0), (5, 0), (1023, 0), (262151, 0), (819200, 0), (2100003, 0),
                                      (1023, 4), (262151, 4)])
def test_prepare_norm_max_and_nonfinite_against_numpy_fp64(ops, N, n, offset):
    """grad_norm: fp64 accumulation leaves only the final rounding to fp32 (2^-24 relative), x4 margin = 2^-22;
    grad_max_abs is exact. 8 relaunches give the same bits (no atomics). offset: the buffer starts 16 bytes into its
    allocation."""
    g = _rand(n, seed=n)
    buf = torch.empty(n + offset, device=DEV)
    gd = buf[offset:]
    gd.copy_(g)
    ctl, ws = ops.opt_buffers(gd)
    cfg = ops.make_opt_cfg(lr=1e-3)
    ops.opt_prepare_(cfg, gd, ws, ctl)
    got = _ctl_host(ctl, N)
    g64 = g.numpy().astype(np.float64)
    want = math.sqrt(float(np.sum(g64 * g64)))
    print(f"n={n}: grad_norm {got['grad_norm']!r} want {want!r} rel {abs(got['grad_norm'] - want) / want:.3e}")
    assert abs(got["grad_norm"] - want) <= 2.0 ** -22 * want
    assert got["grad_max_abs"] == float(np.max(np.abs(g.numpy())))
    assert got["nonfinite"] == 0 and got["clip_coef"] == 1.0 and got["lr"] == float(np.float32(1e-3))
    first = ctl.view(torch.int32).clone()
    for _ in range(8):
        ctl.zero_()
        ops.opt_prepare_(cfg, gd, ws, ctl)
        assert torch.equal(ctl.view(torch.int32), first)
    # grad_scale enters the norm: what is clipped is the gradient the update sees
    ops.opt_prepare_(ops.make_opt_cfg(lr=1e-3, grad_scale=0.125), gd, ws, ctl)
    assert abs(_ctl_host(ctl, N)["grad_norm"] - want / 8) <= 2.0 ** -22 * want / 8
    if n >= 5:  # one planted inf and one NaN are counted, the norm propagates them, the maximum skips the NaN
        gd[n // 2] = float("inf")
        gd[n - 1] = float("nan")
        ops.opt_prepare_(ops.make_opt_cfg(lr=1e-3, clip_mode="norm", clip_val=1.0), gd, ws, ctl)
        bad = _ctl_host(ctl, N)
        assert bad["nonfinite"] == 2 and math.isnan(bad["grad_norm"]) and math.isnan(bad["clip_coef"])
        assert bad["grad_max_abs"] == float("inf")


def test_prepare_and_update_refuse_bad_arguments(ops):
    g = torch.zeros(64, device=DEV)
    ctl, ws = ops.opt_buffers(g)
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        ops.opt_prepare_(ops.make_opt_cfg(lr=1e-3), g[1:], ws, ctl)
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        ops.grad_accumulate_(g[1:33], g[32:], True)
    with pytest.raises(ValueError, match="clip_val"):
        ops.make_opt_cfg(lr=1e-3, clip_mode="norm")
    with pytest.raises(ValueError, match="clip_mode"):
        ops.make_opt_cfg(lr=1e-3, clip_mode="agc", clip_val=1.0)
    cfg = ops.make_opt_cfg(lr=1e-3, step=0)
    with pytest.raises(RuntimeError, match="invalid argument"):
        ops.opt_prepare_(cfg, g, ws, ctl)


@pytest.mark.parametrize("device_step", [True, False])
def test_adamw_ctl_without_options_is_adamw_bit_for_bit(ops, device_step):
    n = 10007
    p, g = _rand(n, seed=1), _rand(n, seed=2)
    pa, ma, va = p.to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    pb, mb, vb = p.to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    cnt_a = torch.zeros(1, dtype=torch.int32, device=DEV) if device_step else None
    cnt_b = torch.zeros(1, dtype=torch.int32, device=DEV) if device_step else None
    ctl, ws = ops.opt_buffers(pa)
    for step in range(1, 4):
        gs = (g * step).to(DEV)
        ops.adamw_(pa, gs, ma, va, lr=1e-3, weight_decay=0.01, step=step, grad_scale=0.5, step_device=cnt_a)
        cfg = ops.make_opt_cfg(lr=1e-3, weight_decay=0.01, grad_scale=0.5, step=step, step_device=cnt_b)
        ops.opt_prepare_(cfg, gs, ws, ctl)
        ops.adamw_ctl_(cfg, pb, gs, mb, vb, ctl)
        if device_step:
            ops.step_advance_(cnt_a)
            ops.step_advance_(cnt_b)
        assert torch.equal(pa, pb) and torch.equal(ma, mb) and torch.equal(va, vb), step
    assert not torch.equal(pa.cpu(), p)


def _clipped_steps(ops, N, world, device_step, clip_mode, clip_val, g, p):
    """Three steps of prepare + adamw_ctl on the SUM gradient g * step * world with grad_scale = 1 / world, against torch
    on the CPU: clip the averaged gradient -> AdamW -> LambdaLR.step. Returns the reference's clip record per step."""
    n = p.numel()
    ref = torch.nn.Parameter(p.clone())
    opt = torch.optim.AdamW([ref], lr=1e-3, weight_decay=0.01)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, _cosine_lambda)
    pd, m, v = p.to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    cnt = torch.zeros(1, dtype=torch.int32, device=DEV) if device_step else None
    ctl, ws = ops.opt_buffers(pd)
    record = []
    for step in range(1, 4):
        ref.grad = (g * step).clone()  # the average over the ranks
        if clip_mode == "norm":
            total = torch.nn.utils.clip_grad_norm_([ref], clip_val)
            record.append(float(clip_val / (total + 1e-6)))
        else:
            record.append(float((ref.grad.abs() > clip_val).float().mean()))
            torch.nn.utils.clip_grad_value_([ref], clip_val)
        lr_ref = opt.param_groups[0]["lr"]
        opt.step()
        sched.step()
        cfg = ops.make_opt_cfg(lr=1e-3, weight_decay=0.01, grad_scale=1.0 / world, clip_mode=clip_mode, clip_val=clip_val,
                               schedule=COSINE, step=step, step_device=cnt)
        gsum = (g * step * world).to(DEV)  # (x world and x 1 / world are exact: powers of two)
        ops.opt_prepare_(cfg, gsum, ws, ctl)
        ops.adamw_ctl_(cfg, pd, gsum, m, v, ctl)
        if device_step:
            ops.step_advance_(cnt)
        got = _ctl_host(ctl, N)
        print(f"step {step}: ctl {got} reference coef / clipped share {record[-1]!r} lr {lr_ref!r}")
        assert abs(got["lr"] - lr_ref) <= 1e-6 * abs(lr_ref)
        if clip_mode == "norm":
            want_coef = min(1.0, record[-1])
            assert abs(got["clip_coef"] - want_coef) <= 1e-6 * want_coef
            assert abs(got["grad_norm"] - float(total)) <= 1e-6 * float(total)
        else:
            assert got["clip_coef"] == 1.0
        assert torch.equal(gsum.cpu(), g * step * world)  # the gradient buffer itself is left unclipped
    torch.testing.assert_close(pd.cpu(), ref.detach(), rtol=1e-5, atol=1e-7)
    return record


@pytest.mark.parametrize("world,device_step", [(1, False), (8, True)])
def test_norm_clipping_with_cosine_schedule_matches_torch(ops, N, world, device_step):
    n = 4099
    p, g = _rand(n, seed=1), _rand(n, seed=2)
    coefs = _clipped_steps(ops, N, world, device_step, "norm", 1.5 * float(g.norm()), g, p)
    assert coefs[0] > 1.0 and coefs[1] < 1.0 and coefs[2] < 1.0  # inactive at step 1, active at steps 2 and 3


@pytest.mark.parametrize("world,device_step", [(1, False), (8, True)])
def test_value_clipping_with_cosine_schedule_matches_torch(ops, N, world, device_step):
    n = 4099
    p, g = _rand(n, seed=1), _rand(n, seed=2)
    share = _clipped_steps(ops, N, world, device_step, "value", 1.5, g, p)
    assert 0.0 < share[0] < share[1] < share[2] < 1.0  # the clamp is active on a growing part of the elements, never all


def test_resume_from_state_dict_continues_the_schedule_bit_for_bit():
    """Two steps, ``state_dict()``, a new optimizer from it, one step == three steps in one optimizer: the schedule (and
    the bias corrections) are functions of the step count the state dict already carries."""
    from xfmr_rec_amd.trainer import FusedAdamW

    n = 4099
    p0, g = _rand(n, seed=1), _rand(n, seed=2)
    kw = dict(lr=1e-3, weight_decay=0.01, clip_mode="norm", clip_val=1.5 * float(g.norm()), schedule=COSINE)
    grads = [(g * s).to(DEV) for s in (1, 2, 3)]

    def run(param, opt, steps):
        for s in steps:
            param.grad = grads[s].clone()
            opt.step()

    pa = torch.nn.Parameter(p0.to(DEV))
    oa = FusedAdamW([pa], **kw)
    run(pa, oa, (0, 1, 2))
    pb = torch.nn.Parameter(p0.to(DEV))
    ob = FusedAdamW([pb], **kw)
    run(pb, ob, (0, 1))
    sd = ob.state_dict()
    assert set(sd["param_groups"][0]) >= {"lr", "betas", "eps", "weight_decay"} and "schedule" not in sd["param_groups"][0]
    assert [st["step"] for st in sd["state"].values()] == [2]
    pc = torch.nn.Parameter(pb.detach().clone())
    oc = FusedAdamW([pc], **kw)
    oc.load_state_dict(sd)
    run(pc, oc, (2,))
    torch.cuda.synchronize()
    assert torch.equal(pc, pa)
    for k in ("exp_avg", "exp_avg_sq"):
        assert torch.equal(oc.state[pc][k], oa.state[pa][k])
    assert torch.equal(oc.ctl.view(torch.int32), oa.ctl.view(torch.int32))
    assert float(oc.ctl_log_dict()["lr"]) == pytest.approx(1e-3 * _cosine_lambda(2), rel=1e-6)  # step 3: s = 2, the peak
    assert not torch.equal(pa, pb)


@pytest.mark.parametrize("n", [5, 10007])
def test_grad_accumulate_overwrites_first_then_adds_exactly(ops, n):
    g1, g2 = _rand(n, seed=3).to(DEV), _rand(n, seed=4).to(DEV)
    acc = torch.full((n,), float("nan"), device=DEV)  # stale contents
    ops.grad_accumulate_(acc, g1, first=True)
    assert torch.equal(acc, g1)
    ops.grad_accumulate_(acc, g2, first=False)
    assert torch.equal(acc, g1 + g2)
    ops.grad_accumulate_(acc, g2, first=True)
    assert torch.equal(acc, g2)
