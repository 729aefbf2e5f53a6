"""Host side of the optimizer step's options (include/xfmr_hip.h K18b; no GPU): the exported learning-rate factor
``xfmr_lr_lambda`` -- the host form of what the control kernel evaluates -- against the formulas of
``transformers.optimization.get_*_schedule_with_warmup`` restated here (and against that library's own ``lr_lambda``s
where it is importable), and ``Trainer.from_reference_config`` on the values of the reference's ``config.yaml``."""

import math

import pytest
import torch

SCHEDULES = ("constant", "warmup_constant", "warmup_linear", "warmup_cosine")


def _lambda_ref(name, W, T, s):
    """``lr_lambda(current_step = s)`` of transformers.optimization (optimization.py: get_constant_schedule,
    get_constant_schedule_with_warmup, get_linear_schedule_with_warmup, get_cosine_schedule_with_warmup)."""
    if name == "constant":
        return 1.0
    if s < W:
        return float(s) / float(max(1, W))
    if name == "warmup_constant":
        return 1.0
    if name == "warmup_linear":
        return max(0.0, float(T - s) / float(max(1, T - W)))
    progress = float(s - W) / float(max(1, T - W))
    return max(0.0, 0.5 * (1.0 + math.cos(math.pi * progress)))


def _transformers_lambda(name, W, T):
    try:
        import transformers.optimization as O
    except Exception:  # noqa: BLE001 - not installed (or not importable) here: the restated formulas above stand alone
        return None
    opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=1.0)
    sched = {
        "constant": lambda: O.get_constant_schedule(opt),
        "warmup_constant": lambda: O.get_constant_schedule_with_warmup(opt, W),
        "warmup_linear": lambda: O.get_linear_schedule_with_warmup(opt, W, T),
        "warmup_cosine": lambda: O.get_cosine_schedule_with_warmup(opt, W, T),
    }[name]()
    return sched.lr_lambdas[0]


@pytest.mark.parametrize("W,T", [(0, 10), (3, 10), (10, 10)])
@pytest.mark.parametrize("name", SCHEDULES)
def test_exported_lr_lambda_equals_the_transformers_formulas(name, W, T):
    """fp64 arithmetic rounded once to fp32: 1e-7 absolute (the values are in [0, 1]; half an fp32 ulp is <= 3e-8)."""
    from xfmr_rec_amd import ops

    schedule = {"name": name, "warmup_steps": W, "total_steps": T}
    theirs = _transformers_lambda(name, W, T)
    for s in range(0, T + 3):
        got = ops.lr_lambda(schedule, s)
        assert abs(got - _lambda_ref(name, W, T, s)) <= 1e-7, (name, W, T, s, got)
        if theirs is not None:
            assert abs(got - float(theirs(s))) <= 1e-7, (name, W, T, s, got, float(theirs(s)))
    assert ops.lr_lambda(None, 5) == 1.0
    with pytest.raises(ValueError, match="schedule name"):
        ops.lr_lambda({"name": "polynomial"}, 0)
    with pytest.raises(ValueError, match="total_steps"):
        ops.lr_lambda({"name": "warmup_linear", "warmup_steps": 2}, 0)


# the `trainer:` block and the top-level keys of the reference's config.yaml that bear on the optimisation, with a few of
# its orchestration keys (their values as the file has them)
def _reference_cfg(**trainer):
    block = {"accelerator": "cpu", "strategy": "auto", "devices": "auto", "precision": "bf16-mixed", "max_epochs": 1,
             "max_steps": -1, "max_time": "00:04:00:00", "limit_train_batches": 1, "log_every_n_steps": None,
             "accumulate_grad_batches": 1, "gradient_clip_val": None, "gradient_clip_algorithm": None,
             "deterministic": None, "detect_anomaly": False, "use_distributed_sampler": True}
    block.update(trainer)
    return {"seed_everything": 0, "trainer": block, "optimizer": None, "lr_scheduler": None, "ckpt_path": None}


@pytest.fixture()
def module():
    import xfmr_rec_amd as X

    conf = X.LightningConfig(hidden_size=64, num_attention_heads=2, intermediate_size=128, num_hidden_layers=1,
                             max_seq_length=8)
    return X.RecommenderLightningModule(conf)


def test_from_reference_config_with_the_reference_values_sets_no_option(module):
    import xfmr_rec_amd as X

    tr = X.Trainer.from_reference_config(module, _reference_cfg())
    opt = tr.optimizer
    assert tr.accumulate_grad_batches == 1
    assert opt.clip_mode is None and opt.clip_val is None and opt.schedule is None and not opt.has_options
    assert opt.param_groups[0]["grad_scale"] == 1.0 and opt.ctl is None


def test_from_reference_config_reads_the_four_keys(module):
    import xfmr_rec_amd as X

    tr = X.Trainer.from_reference_config(module, _reference_cfg(gradient_clip_val=0.5))
    assert tr.optimizer.clip_mode == "norm" and tr.optimizer.clip_val == 0.5 and tr.optimizer.has_options
    cfg = _reference_cfg(gradient_clip_val=0.25, gradient_clip_algorithm="value", accumulate_grad_batches=4)
    cfg["lr_scheduler"] = {"class_path": "transformers.optimization.get_cosine_schedule_with_warmup",
                           "init_args": {"num_warmup_steps": 3, "num_training_steps": 10}}
    tr = X.Trainer.from_reference_config(module, cfg)
    assert tr.optimizer.clip_mode == "value" and tr.optimizer.clip_val == 0.25
    assert tr.optimizer.schedule == {"name": "warmup_cosine", "warmup_steps": 3, "total_steps": 10}
    assert tr.accumulate_grad_batches == 4 and tr.optimizer.param_groups[0]["grad_scale"] == 0.25
    # the same arguments straight to the constructor; a constant schedule alone is no option
    tr = X.Trainer(module, lr_scheduler={"name": "constant"})
    assert not tr.optimizer.has_options
    tr = X.Trainer(module, gradient_clip_val=0.0)  # Lightning: 0 is "off"
    assert not tr.optimizer.has_options


def test_from_reference_config_raises_on_what_it_cannot_honour_and_names_the_key(module):
    import xfmr_rec_amd as X

    with pytest.raises(ValueError, match="gradient_clip_algorithm"):
        X.Trainer.from_reference_config(module, _reference_cfg(gradient_clip_val=0.5, gradient_clip_algorithm="agc"))
    cfg = _reference_cfg()
    cfg["lr_scheduler"] = {"class_path": "torch.optim.lr_scheduler.OneCycleLR", "init_args": {"max_lr": 0.01}}
    with pytest.raises(ValueError, match="lr_scheduler"):
        X.Trainer.from_reference_config(module, cfg)
    cfg["lr_scheduler"] = {"class_path": "transformers.optimization.get_cosine_schedule_with_warmup",
                           "init_args": {"num_warmup_steps": 3, "num_training_steps": 10, "num_cycles": 2.0}}
    with pytest.raises(ValueError, match="lr_scheduler"):
        X.Trainer.from_reference_config(module, cfg)
    with pytest.raises(ValueError, match="accumulate_grad_batches"):
        X.Trainer.from_reference_config(module, _reference_cfg(accumulate_grad_batches=0))
    cfg = _reference_cfg()
    cfg["optimizer"] = {"class_path": "torch.optim.SGD", "init_args": {"lr": 0.1}}
    with pytest.raises(ValueError, match="optimizer"):
        X.Trainer.from_reference_config(module, cfg)
    with pytest.raises(ValueError, match="gradient_clip_algorithm"):
        X.Trainer(module, gradient_clip_val=1.0, gradient_clip_algorithm="agc")
