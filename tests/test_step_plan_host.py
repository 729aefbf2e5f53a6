"""The training step's plan, key table and views (``xfmr_rec_amd/step_plan.py``) without a device: nothing launches.

The plan: the layout rule with its fill boundary, the overlap rule condition by condition, the "auto" rule and the three
refusals with their messages. The views: over fabricated CPU vectors, in each of the three forms ``compute_losses``
returns, both give exactly the reference's key set; they read the vector the rule names; and they agree key by key --
exactly where both read the same fp32 entry, to rel 1e-6 where the host view divides in double and the kernel in fp32."""

import math
import types

import pytest
import torch

import xfmr_rec_amd as X
from xfmr_rec_amd import _native as N
from xfmr_rec_amd import step_plan as SP

HEADS = ("AlignmentLoss", "AlignmentContrastiveLoss", "ContrastiveLoss", "InfoNCELoss", "NCELoss", "PairwiseHingeLoss",
         "PairwiseLogisticLoss")
BATCH_KEYS = {"batch/size", "batch/seq_len", "batch/numel", "batch/attention_non_zero", "batch/attention_density",
              "batch/positive_non_zero", "batch/positive_density"}
LOGITS_KEYS = {"logits/neg/density", "logits/pos/mean", "logits/pos/std", "logits/pos/min", "logits/pos/max",
               "logits/neg/mean", "logits/neg/std", "logits/neg/min", "logits/neg/max"}
# the keys the reference logs per step (trainer.py:241-263, losses.py:392-404)
ALL_KEYS = {f"loss/{h}" for h in HEADS} | {f"loss/{h}Mean" for h in HEADS} | BATCH_KEYS | LOGITS_KEYS
# the host view's own arithmetic: exact against the device view everywhere else
IN_DOUBLE = {f"loss/{h}Mean" for h in HEADS} | {"batch/attention_density", "batch/positive_density"}


def cfg(**kw):
    base = dict(negatives="in_batch", target_position="first", train_loss="PairwiseHingeLoss", log_all_losses=True,
                mask_false_negatives=True, scale=20.0, margin=0.5, precision="bf16", num_hard_negatives=0)
    return types.SimpleNamespace(**(base | kw))


def build(c=None, **kw):
    base = dict(batch=8, width=25, max_seq_length=25)
    return SP.StepPlan.build(c or cfg(), **(base | kw))


def test_head_order_is_the_loss_classes():
    assert SP.HEADS == HEADS == tuple(cls.__name__ for cls in X.LOSS_CLASSES)
    assert len(HEADS) == N.NUM_LOSSES


# ------------------------------------------------------------------------------------------------ the plan
PACKABLE = dict(has_lengths=True, rows=100, supports_packed=True)


def test_layout_rule():
    p = build(**PACKABLE)
    assert p.packed and p.rows == 100 and p.padded_positions == 8 * 25 and (p.batch, p.L) == (8, 25)
    assert p.opts["padded_positions"] == 200
    # lengths absent, the model's refusal, a trace, a capture, a history wider than max_seq_length (the padded path cuts it)
    for flip in (dict(has_lengths=False), dict(supports_packed=False), dict(tracing=True), dict(capturing=True), dict(width=26)):
        q = build(**(PACKABLE | flip))
        assert not q.packed and q.padded_positions == 0 and q.opts["padded_positions"] == 0, flip
        assert q.L == 25 and q.rows == 8 * 25, flip
    q = build(**(PACKABLE | dict(width=24)))  # a narrower history is its own L
    assert q.packed and q.L == 24 and q.padded_positions == 8 * 24


@pytest.mark.parametrize("rows,packed", [(0, False), (1, True), (194, True), (195, False), (200, False)])
def test_fill_boundary(rows, packed):
    """B = 8, L = 25: 200 padded positions; packed up to floor(0.97 * 200) = 194 rows."""
    assert math.floor(0.97 * 200) == 194
    p = build(**(PACKABLE | dict(rows=rows)))
    assert p.packed is packed
    assert p.padded_positions == (200 if packed else 0)
    assert p.rows == (rows if packed else 200)


OVERLAPS = dict(defer_logging=True, grad=True, has_table_bf16=True)


def test_overlap_rule_each_condition_alone():
    assert build(**OVERLAPS).overlap
    flips = [
        (cfg(), dict(defer_logging=False)),
        (cfg(log_all_losses=False), {}),
        (cfg(), dict(grad=False)),
        (cfg(), dict(has_table_bf16=False)),
        (cfg(precision="fp32"), {}),
        (cfg(num_hard_negatives=4), {}),
        (cfg(train_loss="InfoNCELoss", mask_false_negatives=False), {}),  # the unmasked-InfoNCE exception
        (cfg(), dict(tracing=True)),
    ]
    assert len(flips) == 8
    for c, kw in flips:
        assert not build(c, **(OVERLAPS | kw)).overlap, (c, kw)
    # the exception is that one head in that one mode
    assert build(cfg(train_loss="InfoNCELoss", mask_false_negatives=True), **OVERLAPS).overlap
    for head in HEADS:
        if head != "InfoNCELoss":
            assert build(cfg(train_loss=head, mask_false_negatives=False), **OVERLAPS).overlap, head
    # a captured step overlaps (GraphedStep(overlap=True)); a packed one does
    assert build(**(OVERLAPS | dict(capturing=True))).overlap
    p = build(**(OVERLAPS | PACKABLE))
    assert p.overlap and p.packed


def test_auto_rule():
    auto = dict(OVERLAPS, defer_logging="auto")
    p = build(batch=256, width=200, max_seq_length=200, **auto)
    assert p.defer and p.overlap
    p = build(batch=255, width=200, max_seq_length=200, **auto)
    assert not p.defer and not p.overlap
    p = build(batch=512, width=300, max_seq_length=100, **auto)  # 512 x 100 = 51 200 tokens
    assert p.L == 100 and p.defer and p.overlap
    assert not build(batch=511, width=300, max_seq_length=100, **auto).defer
    assert build(defer_logging=True).defer and not build(defer_logging=False).defer  # (the caller's answer, at any size)


def test_refusals():
    with pytest.raises(ValueError, match=r"^invalid c\.negatives = 'sampled'$"):
        build(cfg(negatives="sampled"))
    with pytest.raises(ValueError, match=r"^the training path scores \[positive \| shared negatives\]: target_position='first'$"):
        build(cfg(target_position=None))
    with pytest.raises(ValueError, match=r"^negatives='catalogue' names the positive by `target` \(= pos_item_idx\): "
                                         r"target_position=None \(losses\.py:233-238\)$"):
        build(cfg(negatives="catalogue"))
    p = build(cfg(negatives="catalogue", target_position=None))
    assert p.catalogue and p.opts["mode"] == N.NEG_CATALOG
    assert not build().catalogue and build().opts["mode"] == N.NEG_SHARED


def test_heads_and_opts():
    p = build()
    assert p.heads == tuple(enumerate(HEADS))
    assert build(cfg(log_all_losses=False)).heads == ((5, "PairwiseHingeLoss"),)
    assert p.opts == dict(train_head="PairwiseHingeLoss", all_heads=True, mask_false_negatives=True, mode=N.NEG_SHARED,
                          scale=20.0, margin=0.5, precision="bf16", num_hard_negatives=0, padded_positions=0)
    real = X.LightningConfig(train_loss="NCELoss")  # the config the module hands over
    assert SP.StepPlan.build(real, batch=2, width=3, max_seq_length=4).opts["train_head"] == "NCELoss"


def test_plan_builds_inside_a_full_graph_trace():
    """compute_losses is traced with fullgraph=True: building the plan there must not break the graph."""
    c = cfg()

    def f(x):
        p = SP.StepPlan.build(c, batch=x.shape[0], width=x.shape[1], max_seq_length=25, tracing=torch.compiler.is_compiling(),
                              defer_logging=True, grad=torch.is_grad_enabled(), has_table_bf16=True, **PACKABLE)
        out = SP.step_result(p, x.sum(), x.flatten()[: 2 * N.NUM_LOSSES], None, x.flatten()[: N.NUM_STATS], sync=False)
        return out["loss/PairwiseHingeLoss"] + (1 if p.packed else 0) + (2 if p.overlap else 0), out["batch/numel"]

    x = torch.ones(8, 25)
    torch._dynamo.reset()
    got, numel = torch.compile(f, backend="eager", fullgraph=True)(x)
    assert float(got) == 200.0 and numel == 200  # padded and not overlapped
    assert float(f(x)[0]) == 203.0


# ------------------------------------------------------------------------------------------------ the views
def vectors(n_query=37.0, neg_count=500.0):
    """fp32 vectors as the kernels would write them: the means and densities are fp32 divisions."""
    f32 = lambda v: torch.tensor(v, dtype=torch.float32)  # noqa: E731
    stats = torch.zeros(N.NUM_STATS)
    S = N.STAT
    stats[S["n_valid"]], stats[S["n_query"]], stats[S["neg_count"]] = 123.0, n_query, neg_count
    stats[S["neg_density"]] = 0.7311
    for j, k in enumerate(("mean", "std", "min", "max")):
        stats[S[f"pos_{k}"]] = 0.1 + j if n_query else float("nan")
        stats[S[f"neg_{k}"]] = -0.3 - j if neg_count else float("nan")
    stats[S["attn_density"]] = f32(123.0) / (f32(200.0) + f32(1e-9))
    stats[S["pos_density"]] = f32(n_query) / (f32(123.0) + f32(1e-9))

    def losses(seed):
        v = torch.zeros(2 * N.NUM_LOSSES)
        v[: N.NUM_LOSSES] = torch.rand(N.NUM_LOSSES, generator=torch.Generator().manual_seed(seed)) * 300 + 1
        v[N.NUM_LOSSES:] = v[: N.NUM_LOSSES] / (f32(n_query) + f32(1e-9)) if n_query else float("nan")
        return v

    return stats, losses(1), losses(2)


def forms(c, **kw):
    """The three forms of one step's result, by the helper ``compute_losses`` uses."""
    stats, side, own = vectors(**kw)
    ti = HEADS.index(c.train_loss)
    plain = build(c)
    over = build(c, **OVERLAPS) if c.log_all_losses else None
    assert over is None or over.overlap
    out = {"sync": SP.step_result(plain, side[ti].clone(), side, None, stats, sync=True),
           "device": SP.step_result(plain, side[ti].clone(), side, None, stats, sync=False)}
    if over is not None:
        # the side-stream pass leaves the train head at 0, the gradient call everything else
        s2, o2 = side.clone(), torch.zeros_like(own)
        s2[ti] = s2[N.NUM_LOSSES + ti] = 0.0
        o2[ti], o2[N.NUM_LOSSES + ti] = own[ti], own[N.NUM_LOSSES + ti]
        out["overlapped"] = SP.step_result(over, o2[ti].clone(), s2, o2, stats, sync=False)
    return out, (stats, side, own)


@pytest.mark.parametrize("log_all", [True, False])
def test_result_forms_and_key_sets(log_all):
    c = cfg(log_all_losses=log_all)
    out, _ = forms(c)
    want = ALL_KEYS if log_all else {"loss/PairwiseHingeLoss", "loss/PairwiseHingeLossMean"} | BATCH_KEYS
    heads = {k for k in want if k.startswith("loss/")}
    consts = {"batch/size", "batch/seq_len", "batch/numel"}
    assert set(out["sync"]) == want
    assert set(out["device"]) == heads | consts | {"stats/device"}
    if log_all:
        assert set(out["overlapped"]) == ({k for k in heads if not k.endswith("Mean")} | consts
                                          | {"stats/device", "losses/device", "losses_train/device"})
    for name, o in out.items():
        assert set(SP.host_values(o, c)) == want, name
        assert set(SP.device_values(o, c)) == want, name
        assert (o["batch/size"], o["batch/seq_len"], o["batch/numel"]) == (8, 25, 200)
        assert all(torch.is_tensor(v) and v.dim() == 0 for v in SP.device_values(o, c).values()), name
    # the plan and the config are the same thing to the views
    assert SP.host_values(out["device"], build(c)) == SP.host_values(out["device"], c)


def test_overlapped_form_reads_the_train_head_from_the_gradient_calls_vector():
    c = cfg()
    out, (stats, side, own) = forms(c)
    ti = HEADS.index(c.train_loss)
    host, dev = SP.host_values(out["overlapped"], c), SP.device_values(out["overlapped"], c)
    for i, h in enumerate(HEADS):
        src = own if i == ti else side
        assert host[f"loss/{h}"] == float(src[i]) == float(dev[f"loss/{h}"]), h
        assert float(dev[f"loss/{h}Mean"]) == float(src[N.NUM_LOSSES + i]), h
        assert host[f"loss/{h}Mean"] == float(src[i]) / (37 + 1e-9), h
        assert SP.head_vector(h, c.train_loss, side, own) is src
        assert SP.head_vector(h, c.train_loss, side) is side
    # and no torch arithmetic: the device view's entries are views of the vectors
    o = out["overlapped"]
    assert dev["loss/NCELossMean"].data_ptr() == o["losses/device"][N.NUM_LOSSES + 4].data_ptr()
    assert dev[f"loss/{c.train_loss}Mean"].data_ptr() == o["losses_train/device"][N.NUM_LOSSES + ti].data_ptr()
    assert dev["logits/pos/std"].data_ptr() == o["stats/device"][N.STAT["pos_std"]].data_ptr()


def test_empty_selections():
    c = cfg()
    out, _ = forms(c, n_query=0.0)
    pos = {k for k in LOGITS_KEYS if k.startswith("logits/pos/")}
    for name, o in out.items():
        assert set(SP.host_values(o, c)) == ALL_KEYS - pos, name
        dev = SP.device_values(o, c)
        if name != "sync":  # (the synchronous form holds host values already: nothing to be NaN)
            assert set(dev) == ALL_KEYS and all(math.isnan(float(dev[k])) for k in pos), name
    out, _ = forms(c, neg_count=0.0)
    neg = {f"logits/neg/{k}" for k in ("mean", "std", "min", "max")}
    assert set(SP.host_values(out["device"], c)) == ALL_KEYS - neg  # (logits/neg/density stays)
    assert all(math.isnan(float(SP.device_values(out["device"], c)[k])) for k in neg)


@pytest.mark.parametrize("log_all", [True, False])
def test_views_agree_key_by_key(log_all):
    c = cfg(log_all_losses=log_all)
    out, _ = forms(c)
    for name, o in out.items():
        host, dev = SP.host_values(o, c), SP.device_values(o, c)
        assert set(host) == set(dev)
        for k, v in host.items():
            if k in IN_DOUBLE:  # (the synchronous form's densities are doubles that its device view rounds to fp32)
                assert float(dev[k]) == pytest.approx(v, rel=1e-6), (name, k)
            else:
                assert float(dev[k]) == v, (name, k)
        assert isinstance(host["batch/attention_non_zero"], int if name != "sync" else float)
    # the two plain forms hold the same step: the same host view, the means of the synchronous form being the kernel's
    a, s = SP.host_values(out["device"], c), SP.host_values(out["sync"], c)
    for k in a:
        assert s[k] == (pytest.approx(a[k], rel=1e-6) if k.endswith("Mean") else a[k]), k


def test_stats_to_dict_reads_the_same_table():
    stats, _, _ = vectors(n_query=0.0)
    got = X.losses.stats_to_dict(stats.tolist())
    assert set(got) == LOGITS_KEYS - {k for k in LOGITS_KEYS if k.startswith("logits/pos/")}
    assert got["logits/neg/density"] == float(stats[N.STAT["neg_density"]])
