"""The operator layer between the plans and the C ABI (``ops.py``'s loss and encoder half, ``custom_ops.py``) without a
device: nothing launches.

The encoder cfg: for a table of ``make_encoder_cfg`` keyword sets, the struct equals field by field a literal written out
here, and byte for byte the struct the registered route builds from ``encoder_op_args`` of the same keywords. The loss cfg:
for every public loss entry and a table of keyword sets, the ``xfmr_loss_cfg`` the library is handed -- captured by a
stand-in for the library handle that records and returns -- equals a literal; the per-entry defaults; and the eager and the
registered route of the three differentiable entries hand over the same struct. The loss node's backward on CPU tensors,
``xfmr_scale_by_device_scalar`` being an in-place multiply: what only the sampled (B*L) form does, and the dense form's two
gradient slots."""

import pytest
import torch

from xfmr_rec_amd import _native as N
from xfmr_rec_amd import ops

HEADS = ("AlignmentLoss", "AlignmentContrastiveLoss", "ContrastiveLoss", "InfoNCELoss", "NCELoss", "PairwiseHingeLoss",
         "PairwiseLogisticLoss")


def fields(s) -> dict:
    """A ctypes struct as {field: value}; a pointer pair as a list."""
    return {k: (list(v) if hasattr(v, "__len__") else v) for k, v in ((k, getattr(s, k)) for k, _ in s._fields_)}


# ------------------------------------------------------------------------------------------------ the encoder cfg
ENV = ("XFMR_LN_UNFUSED", "XFMR_FFN_UNFUSED", "XFMR_FFN_BWD_UNFUSED", "XFMR_DW_SIDE", "XFMR_DW_PAIR", "XFMR_REDUCE_HALF_EARLY")
SHAPE = dict(batch=4, seq_len=24, hidden=64)
BASE = dict(SHAPE, heads=2, inter=128, layers=2, max_pos=24, precision="bf16")
ENC_DEFAULT = dict(batch=4, seq_len=24, hidden=64, heads=2, inter=128, layers=2, max_pos=24, precision=N.PREC_BF16,
                   ln_eps=torch.tensor(1e-12).item(), hidden_dropout=0.0, attn_dropout=0.0, flags=0, seed=0, step_device=None,
                   embed_event=None, context=None, grads_half_event=None, profile_kernel=0, profile_layer=0,
                   profile_events=[None, None], seq_offsets=None, row_pos=None, packed_rows=0)
SWITCHES = [({"XFMR_LN_UNFUSED": "1"}, 2), ({"XFMR_FFN_UNFUSED": "1"}, 4), ({"XFMR_FFN_BWD_UNFUSED": "1"}, 8),
            ({"XFMR_DW_SIDE": "0"}, 16), ({"XFMR_DW_SIDE": "any"}, 32), ({"XFMR_DW_PAIR": "0"}, 64),
            ({"XFMR_REDUCE_HALF_EARLY": "1"}, 128)]
TOGETHER = {k: v for env, _ in SWITCHES for k, v in env.items()}  # (XFMR_DW_SIDE ends as "any": one variable, two values)
SEQ_OFFSETS = torch.tensor([0, 24, 41, 46, 70], dtype=torch.int32)
ROW_POS = torch.arange(70, dtype=torch.int32)

# (environment, make_encoder_cfg keywords beyond BASE, the fields that differ from ENC_DEFAULT)
ENCODER_CASES = [({}, {}, {})]
ENCODER_CASES += [(env, {}, {"flags": bit}) for env, bit in SWITCHES]
ENCODER_CASES += [
    (TOGETHER, {}, {"flags": 2 | 4 | 8 | 32 | 64 | 128}),
    (TOGETHER | {"XFMR_DW_SIDE": "0"}, {}, {"flags": 2 | 4 | 8 | 16 | 64 | 128}),
    (TOGETHER, {"flags": None, "causal": False, "extra_flags": 256}, {"flags": 2 | 4 | 8 | 32 | 64 | 128 | 1 | 256}),
    # explicit flags: the environment is not read
    (TOGETHER, {"flags": N.ENC_DW_INLINE, "extra_flags": N.ENC_FFN_UNFUSED}, {"flags": 16 | 4}),
    (TOGETHER, {"flags": 0}, {}),
    ({}, {"causal": False}, {"flags": N.ENC_BIDIRECTIONAL}),
    ({}, {"seed": (1 << 63) + 5}, {"seed": (1 << 63) + 5}),
    ({}, {"seed": (1 << 64) - 1, "ln_eps": 0.5, "hidden_dropout": 0.25, "attn_dropout": 0.125, "precision": "fp32"},
     {"seed": (1 << 64) - 1, "ln_eps": 0.5, "hidden_dropout": 0.25, "attn_dropout": 0.125, "precision": N.PREC_F32}),
    ({}, {"embed_event": 0x1000, "context": 0x2000, "grads_half_event": 0x3000, "profile": (N.PROF_ATTN_BWD, 1, 0x4000, 0x5000)},
     {"embed_event": 0x1000, "context": 0x2000, "grads_half_event": 0x3000, "profile_kernel": 4, "profile_layer": 1,
      "profile_events": [0x4000, 0x5000]}),
    ({}, {"profile": (N.PROF_FFN_FWD, 0, 0x4000, 0x5000)}, {"profile_kernel": 1, "profile_events": [0x4000, 0x5000]}),
    ({}, {"seq_offsets": SEQ_OFFSETS, "row_pos": ROW_POS},
     {"seq_offsets": SEQ_OFFSETS.data_ptr(), "row_pos": ROW_POS.data_ptr(), "packed_rows": 70}),
    ({}, {"step_device": None}, {}),
]


@pytest.fixture
def host_pointers(monkeypatch):
    """N.ptr refuses a CPU tensor; here its address stands for the device's."""
    monkeypatch.setattr(N, "ptr", lambda t: None if t is None else t.data_ptr())
    for name in ENV:
        monkeypatch.delenv(name, raising=False)


@pytest.mark.parametrize("env,kw,want", ENCODER_CASES)
def test_encoder_cfg_fields_and_the_registered_routes_bytes(env, kw, want, host_pointers, monkeypatch):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    eager = ops.make_encoder_cfg(**(BASE | kw))
    assert fields(eager) == ENC_DEFAULT | want
    args = ops.encoder_op_args(**(BASE | kw))
    assert len(args) == 15
    assert args[-1] == (24 if "seq_offsets" in kw else 0)  # packed_seq_len: the op cannot read L off a (rows,) index tensor
    assert -(1 << 63) <= args[9] < (1 << 63) and args[9] % (1 << 64) == kw.get("seed", 0)  # a schema int is signed
    registered = ops.encoder_cfg(SHAPE["batch"], SHAPE["seq_len"], SHAPE["hidden"], *args[:-1])
    assert bytes(registered) == bytes(eager)


def test_encoder_flags_are_read_when_the_cfg_is_made(host_pointers, monkeypatch):
    monkeypatch.setenv("XFMR_LN_UNFUSED", "0")  # "0" and "" are off
    monkeypatch.setenv("XFMR_FFN_UNFUSED", "")
    assert ops.make_encoder_cfg(**BASE).flags == 0 and ops.encoder_op_args(**BASE)[8] == 0
    monkeypatch.setenv("XFMR_LN_UNFUSED", "yes")
    assert ops.make_encoder_cfg(**BASE).flags == 2 and ops.encoder_op_args(**BASE)[8] == 2


# ------------------------------------------------------------------------------------------------ the loss cfg
class Library:
    """Stands in for the library handle: every entry records its name and the xfmr_loss_cfg it was handed, fills the fp32
    tensors it was handed that are not ``inputs`` with 2 (N.ptr hands tensors through here), and returns: a size for a
    workspace query, XFMR_OK for a launch. ``xfmr_scale_by_device_scalar`` is the in-place multiply."""

    def __init__(self):
        self.calls, self.inputs = [], []

    def names(self):
        return [name for name, _ in self.calls]

    def cfgs(self):
        return [cfg for _, cfg in self.calls if cfg is not None]

    def __getattr__(self, name):
        def entry(*args):
            cfg = [fields(a._obj) for a in args if hasattr(a, "_obj")]  # ctypes.byref(cfg)
            self.calls.append((name, cfg[0] if cfg else None))
            if name == "xfmr_scale_by_device_scalar":
                args[0].mul_(args[2])
                return 0
            for a in args:
                if torch.is_tensor(a) and a.dtype == torch.float32 and not any(a is t for t in self.inputs):
                    a.fill_(2.0)
            return 4096 if "workspace" in name else 0

        return entry


@pytest.fixture
def lib(monkeypatch):
    rec = Library()
    monkeypatch.setattr(N, "load", lambda: rec)
    monkeypatch.setattr(N, "ptr", lambda t: t)
    monkeypatch.setattr(N, "stream", lambda: 0)
    monkeypatch.delenv("XFMR_TORCH_OPS", raising=False)
    return rec


T, H, V = 6, 8, 11


def tensors(lib, *, grad=False):
    t = dict(tok=torch.ones(T, H, requires_grad=grad), key_mask=torch.ones(T, dtype=torch.uint8),
             pos=torch.ones(T, dtype=torch.int64), neg=torch.ones(T, dtype=torch.int64), table=torch.ones(V, H),
             rnorm=torch.ones(V), cand=torch.ones(T, 3, H))
    lib.inputs += list(t.values())
    return t


def call_workspace(t, **kw):
    return ops.sampled_loss_workspace(t["tok"], T, H, V, **kw)


def call_prepare(t, **kw):
    return ops.sampled_loss_prepare(torch.empty(4096, dtype=torch.uint8), t["key_mask"], t["pos"], t["neg"], t["rnorm"], V, H, **kw)


def call_sampled(t, **kw):
    return ops.sampled_loss(t["tok"], t["key_mask"], t["pos"], t["neg"], t["table"], t["rnorm"], **kw)


def call_lists(t, **kw):
    return ops.sampled_loss_lists(t["tok"], t["pos"], t["neg"], t["table"], t["rnorm"], **kw)


def call_dense(t, **kw):
    return ops.dense_loss(t["tok"], t["cand"], None, **kw)


# entry -> (the call, the library entries it reaches in order, the entry's own defaults beyond LOSS_DEFAULT)
ENTRIES = {
    "workspace": (call_workspace, ["xfmr_sampled_loss_workspace_cfg"], {}),
    "prepare": (call_prepare, ["xfmr_sampled_loss_prepare"], {}),
    "sampled": (call_sampled, ["xfmr_sampled_loss_workspace_cfg", "xfmr_sampled_loss"], {}),
    "lists": (call_lists, ["xfmr_sampled_loss_lists_workspace_cfg", "xfmr_sampled_loss_lists"], {"all_heads": 0}),
    "dense": (call_dense, ["xfmr_dense_loss_workspace", "xfmr_dense_loss_grads"], {"all_heads": 0, "precision": N.PREC_F32}),
}
SAMPLED = ("workspace", "prepare", "sampled", "lists")
LOSS_DEFAULT = dict(train_head=3, all_heads=1, mask_false_negatives=1, mode=N.NEG_SHARED, precision=N.PREC_BF16, scale=1.0,
                    margin=0.5, num_hard_negatives=0, flags=0, profile_grad=[None, None], profile_log=[None, None],
                    padded_positions=0)

# (entries, keywords beyond train_head="InfoNCELoss", the fields that differ from the entry's defaults)
LOSS_CASES = [(tuple(ENTRIES), {}, {})]
LOSS_CASES += [(tuple(ENTRIES), {"train_head": name}, {"train_head": i}) for i, name in enumerate(HEADS)]
LOSS_CASES += [(tuple(ENTRIES), {"train_head": i}, {"train_head": i}) for i in range(len(HEADS))]
LOSS_CASES += [(tuple(ENTRIES), {"all_heads": v}, {"all_heads": n}) for v, n in ((False, 0), (True, 1), (2, 2))]
LOSS_CASES += [
    (SAMPLED, {"mode": N.NEG_SHARED}, {"mode": 0}),
    (SAMPLED, {"mode": N.NEG_CATALOG}, {"mode": 1}),
    (SAMPLED, {"nsplit": 3}, {"flags": 3 << 8}),
    (SAMPLED, {"nsplit_grad": 5}, {"flags": 5 << 16}),
    (SAMPLED, {"nsplit": 255, "nsplit_grad": 1}, {"flags": (255 << 8) | (1 << 16)}),
    (SAMPLED, {"precision": "fp32"}, {"precision": N.PREC_F32}),
    (tuple(ENTRIES), {"mask_false_negatives": False, "scale": 20.0, "margin": 0.25, "num_hard_negatives": 4},
     {"mask_false_negatives": 0, "scale": 20.0, "margin": 0.25, "num_hard_negatives": 4}),
    # padded_positions is read by the final reduction of a loss call alone (csrc/loss.hip: run_loss); neither the workspace
    # size nor the prepare pass reads it, and both are handed the cfg the call runs with
    (("workspace", "prepare", "sampled"), {"padded_positions": 200}, {"padded_positions": 200}),
    (("workspace", "prepare", "sampled"), {"padded_positions": 200, "nsplit": 2, "all_heads": 2},
     {"padded_positions": 200, "flags": 2 << 8, "all_heads": 2}),
    (("sampled",), {"profile_grad": (0x10, 0x20), "profile_log": (0x30, 0x40)},
     {"profile_grad": [0x10, 0x20], "profile_log": [0x30, 0x40]}),
    (("sampled",), {"profile_log": (0x30, 0x40), "need_grad": False}, {"profile_log": [0x30, 0x40]}),
]


@pytest.mark.parametrize("entries,kw,want", LOSS_CASES)
def test_loss_cfg_handed_to_the_library(entries, kw, want, lib):
    t = tensors(lib)
    for entry in entries:
        call, names, own = ENTRIES[entry]
        lib.calls.clear()
        call(t, **({"train_head": "InfoNCELoss"} | kw))
        assert lib.names() == names, entry
        assert len(lib.cfgs()) >= 1 and all(c == LOSS_DEFAULT | own | want for c in lib.cfgs()), (entry, lib.cfgs())


def test_loss_cfg_of_the_per_call_extras(lib):
    t = tensors(lib)
    zeroed = torch.zeros(T, H)
    _, _, d_tok = call_sampled(t, train_head=3, d_tok_zeroed=zeroed)
    assert d_tok is zeroed and all(c == LOSS_DEFAULT | {"flags": N.LOSS_DTOK_ZEROED} for c in lib.cfgs())
    lib.calls.clear()
    _, _, d_tok = call_sampled(t, train_head=3, d_tok_zeroed=zeroed, nsplit=2, nsplit_grad=3)
    assert all(c == LOSS_DEFAULT | {"flags": 1 | (2 << 8) | (3 << 16)} for c in lib.cfgs())
    lib.calls.clear()
    _, _, d_tok = call_sampled(t, train_head=3, d_tok_zeroed=zeroed, need_grad=False)  # no gradient: nothing was zeroed for it
    assert d_tok is None and all(c == LOSS_DEFAULT for c in lib.cfgs())
    lib.calls.clear()
    ws = torch.empty(4096, dtype=torch.uint8)
    call_sampled(t, train_head=3, workspace=ws)  # the caller's workspace: no size query
    assert lib.names() == ["xfmr_sampled_loss"]
    lib.calls.clear()
    call_sampled(t, train_head=3, workspace=ws, prepared=True)
    assert lib.names() == ["xfmr_sampled_loss_prepared"] and lib.cfgs() == [LOSS_DEFAULT]


def test_an_unknown_option_is_refused_not_dropped(lib):
    t = tensors(lib)
    for entry in ("workspace", "prepare", "sampled", "lists", "dense"):
        with pytest.raises(TypeError):
            ENTRIES[entry][0](t, train_head=3, no_such_option=1)
    assert lib.calls == []


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_per_entry_defaults(entry, lib):
    """Every caller in the package passes ``all_heads``; a caller that does not gets the entry's own default: every head for
    the (B*L) entries, the train head alone for the list and the dense form."""
    call, _, own = ENTRIES[entry]
    call(tensors(lib), train_head="InfoNCELoss")
    assert lib.cfgs() and all(c == LOSS_DEFAULT | own for c in lib.cfgs())
    assert lib.cfgs()[0]["all_heads"] == {"workspace": 1, "prepare": 1, "sampled": 1, "lists": 0, "dense": 0}[entry]


def test_dense_target_modes(lib):
    t = tensors(lib)
    assert N.TARGET_MODES == {"first": 0, "diagonal": 1, None: 2}
    seen = []
    real = lib.__getattr__("xfmr_dense_loss_grads")
    lib.xfmr_dense_loss_grads = lambda *a: (seen.append(a[4]), real(*a))[1]
    for name in ("first", "diagonal", None):
        call_dense(t, train_head=3, target_position=name)
    assert seen == [N.TARGET_FIRST, N.TARGET_DIAGONAL, N.TARGET_EXPLICIT]
    with pytest.raises(KeyError):
        call_dense(t, train_head=3, target_position="last")


TRAIN_OPTS = dict(train_head="NCELoss", all_heads=2, mask_false_negatives=False, mode=N.NEG_CATALOG, scale=20.0, margin=0.25,
                  precision="fp32", num_hard_negatives=4)
TRAIN_WANT = LOSS_DEFAULT | dict(train_head=4, all_heads=2, mask_false_negatives=0, mode=1, scale=20.0, margin=0.25,
                                 precision=N.PREC_F32, num_hard_negatives=4)


def train_sampled(t, opts):
    return ops.sampled_loss_train(t["tok"], t["key_mask"], t["pos"], t["neg"], t["table"], t["rnorm"], opts)


def train_lists(t, opts):
    return ops.sampled_loss_lists_train(t["tok"], t["pos"], t["neg"], t["table"], t["rnorm"], opts)


def train_dense(t, opts):
    return ops.dense_loss_train(t["tok"], t["cand"], None, opts)


@pytest.mark.parametrize("train,want", [(train_sampled, TRAIN_WANT), (train_lists, TRAIN_WANT),
                                        (train_dense, TRAIN_WANT | {"mode": 0})])  # the dense form: fp32, its own candidates
def test_both_routes_hand_the_library_the_same_loss_cfg(train, want, lib, monkeypatch):
    seen = []
    for route in ("0", "1"):
        monkeypatch.setenv("XFMR_TORCH_OPS", route)
        lib.calls.clear()
        loss, losses, stats = train(tensors(lib, grad=True), TRAIN_OPTS)
        assert loss.shape == () and float(loss.detach()) == 2.0 and losses.shape == (14,) and stats.shape == (16,)
        seen.append(lib.calls[:])
    assert seen[0] == seen[1] and all(c == want for _, c in seen[0] if c is not None) and len(seen[0]) == 2


def test_a_call_with_eager_only_extras_takes_the_eager_node_on_either_route(lib, monkeypatch):
    """The overlapped step's calls carry a workspace (a byte tensor: its truth value is not to be asked for)."""
    ws = torch.empty(4096, dtype=torch.uint8)
    for route in ("0", "1"):
        monkeypatch.setenv("XFMR_TORCH_OPS", route)
        lib.calls.clear()
        loss, _, _ = train_sampled_with(tensors(lib, grad=True), OPTS, workspace=ws, prepared=True, d_tok_zeroed=torch.zeros(T, H))
        assert lib.names() == ["xfmr_sampled_loss_prepared"] and lib.cfgs()[0]["flags"] == N.LOSS_DTOK_ZEROED
        assert type(loss.grad_fn).__name__ == "LossFunctionBackward"
    lib.calls.clear()
    loss, _, _ = train_sampled_with(tensors(lib, grad=True), OPTS, workspace=None, prepared=False, profile_grad=None)
    assert type(loss.grad_fn).__name__ != "LossFunctionBackward"  # nothing eager-only is set: the registered op


def train_sampled_with(t, opts, **extras):
    return ops.sampled_loss_train(t["tok"], t["key_mask"], t["pos"], t["neg"], t["table"], t["rnorm"], opts, **extras)


# ------------------------------------------------------------------------------------------------ the loss node's backward
class Probe(torch.autograd.Function):
    """Identity in front of a loss: shows the tensor object its backward is handed."""

    seen: list = []

    @staticmethod
    def forward(ctx, x):
        return x.view_as(x)

    @staticmethod
    def backward(ctx, d):
        Probe.seen.append(d)
        return d


def probed(lib, name="tok"):
    Probe.seen.clear()
    t = tensors(lib)
    leaf = t[name].requires_grad_(True)
    t[name] = Probe.apply(leaf)
    lib.inputs.append(t[name])
    return t, leaf


def scales(lib):
    return lib.names().count("xfmr_scale_by_device_scalar")


OPTS = dict(train_head="NCELoss", all_heads=True)


def test_sampled_backward_unit_gradient_and_hand_over(lib):
    # the unit-gradient object: no multiply, one hit, and the buffer is handed over (grad mode is off in a plain backward)
    t, leaf = probed(lib)
    loss, _, _ = train_sampled(t, OPTS)
    hits = ops.unit_grad_hits
    loss.backward(gradient=ops.unit_grad(loss))
    assert scales(lib) == 0 and ops.unit_grad_hits == hits + 1
    assert torch.equal(leaf.grad, torch.full((T, H), 2.0))
    assert len(Probe.seen) == 1 and getattr(Probe.seen[0], "_xfmr_consumable", False) is True
    # any other gradient, a plain 1 included: one multiply, no hit
    t, leaf = probed(lib)
    loss, _, _ = train_sampled(t, OPTS)
    (3.0 * loss).backward()
    assert scales(lib) == 1 and ops.unit_grad_hits == hits + 1
    assert torch.equal(leaf.grad, torch.full((T, H), 6.0)) and Probe.seen[0]._xfmr_consumable is True
    # under create_graph grad mode is on: the buffer is not handed over
    t, leaf = probed(lib)
    loss, _, _ = train_sampled(t, OPTS)
    (g,) = torch.autograd.grad(3.0 * loss, leaf, create_graph=True)
    assert torch.equal(g.detach(), torch.full((T, H), 6.0)) and not hasattr(Probe.seen[0], "_xfmr_consumable")
    # no gradient for the train loss: None for every forward argument, nothing launched
    t, leaf = probed(lib)
    loss, _, _ = train_sampled(t, OPTS)
    before = len(lib.calls)
    out = loss.grad_fn.apply(None, None, None)
    assert out == (None,) * 10 and len(lib.calls) == before  # (run, head, slots, sampled) + the six tensors


def test_list_backward_has_neither_shortcut_nor_hand_over(lib):
    t, leaf = probed(lib)
    loss, _, _ = train_lists(t, OPTS)
    hits = ops.unit_grad_hits
    loss.backward(gradient=ops.unit_grad(loss))
    assert scales(lib) == 1 and ops.unit_grad_hits == hits
    assert torch.equal(leaf.grad, torch.full((T, H), 2.0)) and not hasattr(Probe.seen[0], "_xfmr_consumable")


@pytest.mark.parametrize("need_q,need_c", [(False, False), (True, False), (False, True), (True, True)])
def test_dense_backward_fills_the_right_slots(need_q, need_c, lib):
    t = tensors(lib)
    q, c = t["tok"].requires_grad_(need_q), t["cand"].requires_grad_(need_c)
    loss, _, _ = train_dense(t, OPTS)
    assert loss.requires_grad is (need_q or need_c)
    if not loss.requires_grad:
        return
    hits = ops.unit_grad_hits
    (3.0 * loss).backward()
    assert scales(lib) == int(need_q) + int(need_c) and ops.unit_grad_hits == hits
    assert torch.equal(q.grad, torch.full((T, H), 6.0)) if need_q else q.grad is None
    assert torch.equal(c.grad, torch.full((T, 3, H), 6.0)) if need_c else c.grad is None


@pytest.mark.parametrize("train,name", [(train_sampled, "tok"), (train_lists, "tok"), (train_dense, "tok"), (train_dense, "cand")])
def test_registered_backward_scales_a_copy_and_hands_over_the_sampled_forms(train, name, lib, monkeypatch):
    """The registered route (XFMR_TORCH_OPS=1): its backward multiplies into a NEW tensor (a traced graph may not rescale a
    forward output in place), so the unit gradient is no shortcut there; only the sampled form marks the result."""
    monkeypatch.setenv("XFMR_TORCH_OPS", "1")
    t, leaf = probed(lib, name)
    loss, _, _ = train(t, OPTS)
    hits = ops.unit_grad_hits
    (3.0 * loss).backward()
    assert scales(lib) == 1 and ops.unit_grad_hits == hits
    assert torch.equal(leaf.grad, torch.full(leaf.shape, 6.0))
    assert getattr(Probe.seen[0], "_xfmr_consumable", False) is (train is train_sampled)


# ------------------------------------------------------------------------------------------------ the in-place rule
def test_scratch_rule():
    """A backward may use the incoming gradient in place only if its producer marked it."""
    for same in (lambda a, b: a is b, lambda a, b: a.data_ptr() == b.data_ptr()):
        d = torch.ones(3, 4)
        assert ops.backward_scratch(d, same) is not d and torch.equal(ops.backward_scratch(d, same), d)
        d._xfmr_consumable = True
        assert ops.backward_scratch(d, same) is d
        strided = torch.ones(4, 3).t()  # contiguous() already made a copy: nothing of the producer's is touched
        out = ops.backward_scratch(strided, same)
        assert out.is_contiguous() and out.data_ptr() != strided.data_ptr()
