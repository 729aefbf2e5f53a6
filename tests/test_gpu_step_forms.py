"""The three forms of ``compute_losses`` -- synchronous host values, device vectors, logging heads overlapped on the side
stream -- on the padded and on the packed layout: the plan the module built, the two views of each result against each
other, and the forms against each other (``xfmr_rec_amd/step_plan.py``; the host side of it: tests/test_step_plan_host.py)."""

import pytest
import torch

from test_gpu_graph import _setup
from test_step_plan_host import ALL_KEYS, HEADS, IN_DOUBLE

pytestmark = pytest.mark.gpu
LENGTHS = [24, 5, 12, 3, 17, 9, 20, 6]  # 96 of the 8 x 24 = 192 padded positions


@pytest.fixture(scope="module")
def step():
    import xfmr_rec_amd as X

    mod, batches = _setup(X)
    mod.eval()  # dropout off: the three forms are three calls
    assert mod.model.flat.requires_grad
    padded = {k: v.clone() for k, v in batches[0].items()}
    for b, n in enumerate(LENGTHS):
        for v in padded.values():
            v[b, n:] = 0
    return mod, {"padded": padded, "packed": padded | {"lengths": torch.tensor(LENGTHS)}}


@pytest.mark.parametrize("layout", ["padded", "packed"])
def test_forms_plans_and_views(step, layout):
    mod, batches = step
    batch, packed = batches[layout], layout == "packed"
    outs, plans = {}, {}
    for form, kw in (("sync", dict(sync_metrics=True)), ("device", dict(sync_metrics=False)),
                     ("overlapped", dict(sync_metrics=False, defer_logging=True))):
        mod.model.flat.grad = None
        outs[form] = mod.compute_losses(batch, **kw)
        plans[form] = mod.last_plan
    outs["overlapped"]["loss/InfoNCELoss"].backward()
    mod.sync_logging()
    torch.cuda.synchronize()
    assert torch.isfinite(mod.model.flat.grad).all()
    # the plan
    for form, p in plans.items():
        assert p.packed is packed and p.overlap is (form == "overlapped"), (form, p)
        assert (p.batch, p.L, p.rows) == (8, 24, sum(LENGTHS) if packed else 192)
        assert p.padded_positions == (192 if packed else 0)
    # the forms' keys
    heads = {f"loss/{h}" for h in HEADS}
    consts = {"batch/size", "batch/seq_len", "batch/numel"}
    assert set(outs["sync"]) == ALL_KEYS
    assert set(outs["device"]) == heads | {h + "Mean" for h in heads} | consts | {"stats/device"}
    assert set(outs["overlapped"]) == heads | consts | {"stats/device", "losses/device", "losses_train/device"}
    # the views against each other
    host = {}
    for form, out in outs.items():
        host[form], dev = mod.logged_values(out), mod.device_log_dict(out)
        assert set(host[form]) == set(dev) == ALL_KEYS, form
        for k, v in host[form].items():
            print(layout, form, k, v, float(dev[k]))
            if k in IN_DOUBLE:
                assert float(dev[k]) == pytest.approx(v, rel=1e-6), (form, k)
            else:
                assert float(dev[k]) == v, (form, k)
    assert host["sync"]["batch/attention_non_zero"] == sum(LENGTHS) and host["sync"]["batch/numel"] == 192
    # the forms against each other: every head bit for bit, and the same statistics
    for h in HEADS:
        assert host["sync"][f"loss/{h}"] == host["device"][f"loss/{h}"] == host["overlapped"][f"loss/{h}"], h
    assert torch.equal(outs["device"]["stats/device"], outs["overlapped"]["stats/device"])
    assert {k: v for k, v in host["device"].items() if k not in heads} == \
           {k: v for k, v in host["overlapped"].items() if k not in heads}


def test_traced_plan_is_padded_and_not_overlapped(step):
    from xfmr_rec_amd.step_plan import StepPlan

    mod, batches = step
    mod.compute_losses(batches["packed"], sync_metrics=False, defer_logging=True)
    mod.sync_logging()
    assert mod.last_plan.packed and mod.last_plan.overlap
    kw = dict(batch=8, width=24, max_seq_length=mod.model.max_seq_length, has_lengths=True, rows=sum(LENGTHS),
              supports_packed=mod.model.supports_packed_rows(24), defer_logging=True, grad=True,
              has_table_bf16=mod.model.table_bf16 is not None)
    assert StepPlan.build(mod.config, **kw)[:-1] == mod.last_plan[:-1] and StepPlan.build(mod.config, **kw).opts == mod.last_plan.opts
    traced = StepPlan.build(mod.config, tracing=True, **kw)
    assert not traced.packed and not traced.overlap and traced.rows == 192 and traced.padded_positions == 0
