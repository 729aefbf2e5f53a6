"""The dense-candidate loss kernel (csrc/dense_loss.hip: xfmr_dense_loss / xfmr_dense_loss_grads) against fp64 references,
on inputs whose dot logits are EXACT in the kernel (tests/dense_loss_cases.py; its preconditions, an fp32 model of the
kernel within two thirds of every limit here, and a list of wrong kernels that miss one, are proven on the CPU by
test_dense_loss_cases_host.py).

The C ABI is called directly (xfmr_rec_amd._native, cfg from ops.LossOpts(...).cfg()) so that the test owns the buffers:
`losses`, `stats`, `d_query` and `d_cand` are pre-filled with the bytes 0xFF (a NaN pattern the kernels never produce), each
is followed by a guard region, and so is the workspace; after the call every output element has been written and every guard
byte is untouched. One launch per (case, options, head), compared by dense_loss_cases.measure with the project's fp32 limits
(helpers.TOL["fp32"]): loss sums and their Mean half per head (the heads a lean launch skips are 0), d_query and d_cand whole
and per row (a row's error relative to the larger of its reference norm and the tensor's mean reference row norm), counts and
selected logits exact, the other statistics at the value limit, NaN where the reference has no value. No flips allowance,
no hinge exemption: the inputs make them unnecessary. Rows flagged for a cosine near-tie at the threshold leave the gradient
comparison of the two contrastive heads only.

Shapes: H = 8 / 68 / 260 / 384 / 1024 at N = 40, C = 273 (every gradient slot, lanes idle or in a lone second sweep, partial in
both candidate strides), C = 1 ... 257 around the group of 16 and the stride of 256, the limits C = 8192 and (1, 8192, 1024) --
135 232 bytes of dynamic LDS --, N = 1, N = C diagonal, 300 rows through the shared reduce / final kernels."""

import ctypes as C
import types

import pytest
import torch

import dense_loss_cases as DC
from oracle.losses import LOSS_KINDS

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 1024  # elements (fp32 outputs) / bytes (workspace) after each buffer
EINVAL, EUNSUPPORTED, EWORKSPACE, EALIGN = -1, -2, -3, -5
MODE = {"first": 0, "diagonal": 1, "explicit": 2}
# (case, options, head, what) that misses the fp32 limit for a reason that is rounding -> the reason and the measured value
# against the fp64 reference (it then takes that named limit; profiles/dense_loss.md lists it)
ROUNDING: dict = {}

_WORST: dict = {}  # (case, head) -> [worst value error, worst gradient error]


@pytest.fixture(scope="module")
def native():
    from xfmr_rec_amd import _native

    _native.load()
    return _native


@pytest.fixture(scope="module", autouse=True)
def _report():
    """Prints the measured table (pytest -s): profiles/dense_loss.md is made from these lines."""
    yield
    for (name, head), (ev, eg) in sorted(_WORST.items()):
        print(f"DENSE_LOSS {name} {head} value {ev:.2e} grad {eg:.2e}")


_DEVICE: dict = {}


def _device_inputs(name):
    if name not in _DEVICE:
        inp = DC.inputs(name)
        _DEVICE[name] = (inp, inp.q.to(DEV), inp.cand.to(DEV), inp.target.to(DEV))
    return _DEVICE[name]


def _guarded(n: int):
    """A buffer of n fp32 elements + GUARD, every byte 0xFF."""
    return torch.full((n + GUARD,), -1, dtype=torch.int32, device=DEV)


def _cfg(opt, head, all_heads):
    from xfmr_rec_amd import ops

    return ops.LossOpts(train_head=head, all_heads=all_heads, mask_false_negatives=opt.masked, scale=opt.scale,
                        margin=opt.margin, num_hard_negatives=opt.k, precision="fp32").cfg()


class Run:
    """One direct call on guarded buffers. `rc`; the outputs as int32 views of what was written (`*_bits`, device) and as
    fp32 CPU tensors (`losses`, `stats`, `d_query`, `d_cand`; None where NULL was passed)."""

    def __init__(self, native, q, cand, target, mode, opt, head, all_heads, *, entry="grads", want_dq=True, want_dc=True,
                 ws_short=0, q_ptr=None, cand_ptr=None, shape=None):
        N, Cn, H = shape if shape is not None else (q.shape[0], cand.shape[1], q.shape[1])
        lib = native.load()
        self.n = dict(losses=14, stats=16, d_query=N * H if want_dq else 0, d_cand=N * Cn * H if want_dc else 0)
        self.shapes = dict(losses=(14,), stats=(16,), d_query=(N, H), d_cand=(N, Cn, H))
        self.buf = {k: _guarded(n) for k, n in self.n.items()}
        nbytes = lib.xfmr_dense_loss_workspace(N, Cn, H)
        self.ws_bytes = nbytes
        self.ws = torch.full((nbytes + GUARD,), 0xAB, dtype=torch.uint8, device=DEV)
        cfg = _cfg(opt, head, all_heads)
        p = lambda k: native.ptr(self.buf[k]) if self.n[k] else None  # noqa: E731
        args = [C.byref(cfg), native.ptr(q) if q_ptr is None else q_ptr, native.ptr(cand) if cand_ptr is None else cand_ptr,
                native.ptr(target), int(mode), N, Cn, H, p("losses"), p("stats"), p("d_query")]
        tail = [native.ptr(self.ws), nbytes - ws_short, native.stream()]
        if entry == "grads":
            self.rc = lib.xfmr_dense_loss_grads(*args, p("d_cand"), *tail)
        else:
            assert not want_dc
            self.rc = lib.xfmr_dense_loss(*args, *tail)
        torch.cuda.synchronize()

    def bits(self, k):
        return self.buf[k][:self.n[k]]

    def untouched(self):
        """Nothing was written at all (a refusal)."""
        return all(bool((b == -1).all()) for b in self.buf.values()) and bool((self.ws == 0xAB).all())

    def check_writes(self, tag):
        for k, b in self.buf.items():
            assert bool((b[self.n[k]:] == -1).all()), (tag, k, "guard region written")
            assert bool((b[:self.n[k]] != -1).all()), (tag, k, "output element not written")
        assert bool((self.ws[self.ws_bytes:] == 0xAB).all()), (tag, "workspace guard written")

    def out(self):
        t = {k: (self.bits(k).view(torch.float32).reshape(self.shapes[k]).cpu() if self.n[k] else None) for k in self.n}
        return types.SimpleNamespace(**t)


def _same_bits(a: Run, b: Run, tag, keys=("losses", "stats", "d_query", "d_cand")):
    for k in keys:
        if a.n[k] and b.n[k]:
            assert torch.equal(a.bits(k), b.bits(k)), (tag, k)


def _run_case(native, name, opt, head, all_heads, **kw):
    inp, q, cand, target = _device_inputs(name)
    mode = MODE[inp.case.mode]
    return Run(native, q, cand, target if mode == 2 else None, mode, opt, head, all_heads, **kw)


def _check_launch(native, name, opt, head, all_heads):
    inp = DC.inputs(name)
    tag = f"{name} masked={opt.masked} k={opt.k} scale={opt.scale} {head} all_heads={int(all_heads)}"
    run = _run_case(native, name, opt, head, all_heads)
    assert run.rc == 0, (tag, run.rc)
    run.check_writes(tag)
    ms = DC.measure(run.out(), DC.reference(name, opt), inp, opt, head, all_heads)
    bad = []
    for m in ms:
        limit = ROUNDING.get((name, opt, head, m.what), (None, m.limit))[1]
        if not m.err <= limit:
            bad.append(m)
    ev = max((m.err for m in ms if m.limit > 0 and not m.what.startswith("d_")), default=0.0)
    eg = max((m.err for m in ms if m.what.startswith("d_")), default=0.0)
    print(f"  {tag}: value {ev:.2e} grad {eg:.2e}")
    w = _WORST.setdefault((name, head if not all_heads else "all-heads"), [0.0, 0.0])
    w[0], w[1] = max(w[0], ev), max(w[1], eg)
    assert not bad, (tag, bad)
    return run


def _check_opt(native, name, i):
    opt = DC.opts_of(name)[i]
    for o, head, all_heads in DC.launches(name):
        if o == opt:
            _check_launch(native, name, opt, head, all_heads)


_MATRIX = [pytest.param(n, i, id=f"{n}-{i}") for n in DC.MATRIX for i in range(len(DC.opts_of(n)))]
_OTHERS = [n for n, c in DC.CASES.items() if c.group in ("edge", "rows", "clamped")]
_LIMITS = [pytest.param(n, i, id=f"{n}-{i}") for n, c in DC.CASES.items() if c.group == "limit"
           for i in range(len(DC.opts_of(n)))]


@pytest.mark.parametrize("name,i", _MATRIX)
def test_matrix_widths_and_target_modes_vs_fp64(native, name, i):
    """N = 40, C = 273 at H = 8 / 68 / 260 / 384 / 1024 (explicit targets) and the three target modes at H = 68: per option
    set the seven lean launches and one with every head."""
    _check_opt(native, name, i)


@pytest.mark.parametrize("name", _OTHERS)
def test_column_edges_row_counts_and_clamped_norms_vs_fp64(native, name):
    """C = 1 ... 257 at N = 3 (C = 1: no negatives -- Alignment, NCE's positive term and InfoNCE = 0 are defined, the
    negative statistics NaN, neg_count 0), N = 1, N = C = 33 diagonal, 300 rows, and the case whose clamped norms carry a
    gradient."""
    for i in range(len(DC.opts_of(name))):
        _check_opt(native, name, i)


@pytest.mark.parametrize("name,i", _LIMITS)
def test_the_limits_of_the_header_vs_fp64(native, name, i):
    """(2, 8192, 64) and (1, 8192, 1024): the widest row of logits, the largest dynamic-LDS request, a 32 MB tensor."""
    _check_opt(native, name, i)


def test_c_equal_one_is_defined(native):
    """What the C = 1 reference holds, spelled out: no negatives, the three defined heads, NaN statistics, neg_count 0."""
    opt = DC.Opt(True, 0, 20.0, 0.3)
    ref, out = DC.reference("c1", opt), _run_case(native, "c1", opt, "InfoNCELoss", True).out()
    assert ref.sums["InfoNCELoss"] == 0.0 and float(out.losses[3]) == pytest.approx(0.0, abs=1e-4)
    assert ref.stats["neg_count"] == 0.0 and float(out.stats[DC.STAT["neg_count"]]) == 0.0
    for name in ("neg_mean", "neg_std", "neg_min", "neg_max"):
        assert name not in ref.stats and bool(torch.isnan(out.stats[DC.STAT[name]])), name
    assert float(out.losses[0]) == pytest.approx(ref.sums["AlignmentLoss"], abs=1e-4)
    assert float(out.losses[4]) == pytest.approx(ref.sums["NCELoss"], abs=1e-4) and ref.sums["NCELoss"] > 0


@pytest.mark.parametrize("name", ["w68", "w1024", "c17", "limit-c"])
def test_launches_repeat_and_optional_outputs_change_no_bits(native, name):
    """Two launches give the same bits; k = C gives the bits of k = 0; d_query = NULL and d_cand = NULL each leave the other
    outputs' bits unchanged; xfmr_dense_loss gives the bits of xfmr_dense_loss_grads(..., d_cand = NULL)."""
    Cn = DC.CASES[name].C
    for masked, k, (scale, margin), head, all_heads in ((True, 3, DC.SM[1], "InfoNCELoss", True),
                                                        (False, 40, DC.SM[0], "AlignmentContrastiveLoss", False),
                                                        (True, 1, DC.SM[0], "PairwiseHingeLoss", False)):
        opt = DC.Opt(masked, k, scale, margin)
        tag = f"{name} {opt} {head}"
        one, two = _run_case(native, name, opt, head, all_heads), _run_case(native, name, opt, head, all_heads)
        assert one.rc == 0 and two.rc == 0
        _same_bits(one, two, tag + " two launches")
        no_dq = _run_case(native, name, opt, head, all_heads, want_dq=False)
        no_dc = _run_case(native, name, opt, head, all_heads, want_dc=False)
        short = _run_case(native, name, opt, head, all_heads, want_dc=False, entry="loss")
        for r, what in ((no_dq, "d_query = NULL"), (no_dc, "d_cand = NULL"), (short, "xfmr_dense_loss")):
            assert r.rc == 0, (tag, what)
            r.check_writes(tag + " " + what)
            _same_bits(one, r, tag + " " + what)
        off, plain = (_run_case(native, name, DC.Opt(masked, kk, scale, margin), head, all_heads) for kk in (Cn, 0))
        _same_bits(off, plain, tag + " k = C against k = 0")


def test_documented_refusals_write_nothing(native):
    opt = DC.Opt(True, 0, 1.0, 0.5)

    def call(N, Cn, H, mode=0, target=False, **kw):
        q = torch.zeros(N * H + 4, device=DEV)
        cand = torch.zeros(N * Cn * H + 4, device=DEV)
        t = torch.zeros(N, dtype=torch.int64, device=DEV) if target else None
        r = Run(native, q, cand, t, mode, opt, "InfoNCELoss", True, shape=(N, Cn, H), **kw)
        assert r.untouched(), (N, Cn, H, mode, kw)
        return r.rc

    for shape in ((2, 3, 6), (1, 2, 1028), (1, 8193, 4)):
        assert call(*shape) == EUNSUPPORTED, shape
    assert call(3, 2, 4, mode=1) == EINVAL                 # diagonal with N > C
    assert call(2, 3, 8, mode=2, target=False) == EINVAL   # explicit mode without `target`
    assert call(2, 3, 8, mode=0, target=True) == EINVAL    # `target` given in another mode
    assert call(2, 3, 8, mode=1, target=True) == EINVAL
    q, cand = torch.zeros(2 * 8 + 4, device=DEV), torch.zeros(2 * 3 * 8 + 4, device=DEV)
    assert call(2, 3, 8, q_ptr=native.ptr(q) + 4) == EALIGN
    assert call(2, 3, 8, cand_ptr=native.ptr(cand) + 4) == EALIGN
    assert call(2, 3, 8, ws_short=1) == EWORKSPACE


def test_a_valid_call_of_the_refusal_shapes_does_write(native):
    """The control of test_documented_refusals_write_nothing: the same helper sees a valid call write."""
    q, cand = torch.zeros(2 * 8, device=DEV), torch.zeros(2 * 3 * 8, device=DEV)
    r = Run(native, q, cand, None, 0, DC.Opt(True, 0, 1.0, 0.5), "InfoNCELoss", True, shape=(2, 3, 8))
    assert r.rc == 0 and not r.untouched()
    r.check_writes("valid call")


@pytest.mark.parametrize("head,all_heads", [("InfoNCELoss", True), ("AlignmentContrastiveLoss", False),
                                            ("PairwiseLogisticLoss", False)])
def test_out_of_range_explicit_targets_are_loud(native, head, all_heads):
    """target[row] outside [0, C) -- -1, C, an item id far above C, and 2^32 + 5, which a cast to int would bring back in
    range -- turns that row's loss values, its d_query row and its d_cand rows into NaN, so both halves of losses[14] read
    NaN; the in-range rows of the same launch keep their gradient bits."""
    inp, q, cand, target = _device_inputs("w68")
    Cn = inp.case.C
    opt = DC.Opt(True, 40, 20.0, 0.3)
    good = Run(native, q, cand, target, 2, opt, head, all_heads)
    bad_rows = {3: -1, 7: Cn, 11: 2 ** 32 + 5, 13: 10 ** 6}
    t2 = target.clone()
    for r, v in bad_rows.items():
        t2[r] = v
    bad = Run(native, q, cand, t2, 2, opt, head, all_heads)
    assert good.rc == 0 and bad.rc == 0
    bad.check_writes("out-of-range targets")
    g, b = good.out(), bad.out()
    assert bool(torch.isfinite(g.losses).all()) and bool(torch.isnan(b.losses).all())
    rows = torch.tensor(sorted(bad_rows))
    keep = torch.ones(inp.case.N, dtype=torch.bool)
    keep[rows] = False
    assert bool(torch.isnan(b.d_query[rows]).all()) and bool(torch.isnan(b.d_cand[rows]).all())
    assert torch.equal(b.d_query[keep].view(torch.int32), g.d_query[keep].view(torch.int32))
    assert torch.equal(b.d_cand[keep].view(torch.int32), g.d_cand[keep].view(torch.int32))
    for name in ("n_valid", "n_query", "neg_distinct"):
        assert float(b.stats[DC.STAT[name]]) == float(g.stats[DC.STAT[name]])


def _bits(t):
    return t.detach().contiguous().view(torch.int32).cpu()


@pytest.mark.parametrize("surface,name", [("ops", "w68-diagonal"), ("class", "w68"), ("torch_op", "w68-first")])
def test_python_surfaces_give_the_direct_call_s_bits(native, surface, name):
    """ops.dense_loss, the class API xfmr_rec_amd.losses.<Head> and torch.ops.xfmr.dense_loss on one matrix case each: the
    bits of the direct call, and autograd into q and cand with an upstream factor (2: exact in fp32) gives them times 2."""
    import xfmr_rec_amd.losses as L
    from xfmr_rec_amd import ops

    inp, q, cand, target = _device_inputs(name)
    mode = inp.case.mode
    tgt = target if mode == "explicit" else None
    position = None if mode == "explicit" else mode
    for head, opt in (("InfoNCELoss", DC.Opt(True, 40, 20.0, 0.3)), ("AlignmentContrastiveLoss", DC.Opt(False, 3, 1.0, 0.5)),
                      ("PairwiseHingeLoss", DC.Opt(True, 0, 1.0, 0.5))):
        tag = f"{surface} {name} {head} {opt}"
        hid = LOSS_KINDS.index(head)
        direct = _run_case(native, name, opt, head, False)
        assert direct.rc == 0
        d = direct.out()
        qd, cd = q.clone().requires_grad_(True), cand.clone().requires_grad_(True)
        if surface == "ops":
            losses, stats, d_q, d_c = ops.dense_loss(q, cand, tgt, target_position=position, need_cand_grad=True,
                                                     train_head=head, mask_false_negatives=opt.masked, scale=opt.scale,
                                                     margin=opt.margin, num_hard_negatives=opt.k)
            assert torch.equal(_bits(losses), _bits(d.losses)) and torch.equal(_bits(stats), _bits(d.stats)), tag
            assert torch.equal(_bits(d_q), _bits(d.d_query)) and torch.equal(_bits(d_c), _bits(d.d_cand)), tag
            continue
        if surface == "class":
            conf = L.LossConfig(target_position=position, mask_false_negatives=opt.masked, num_hard_negatives=opt.k,
                                scale=opt.scale, margin=opt.margin)
            loss = getattr(L, head)(conf)(qd, cd, tgt)
        else:
            loss, losses, stats, _dq, _dc = torch.ops.xfmr.dense_loss(qd, cd, tgt, MODE[mode], hid, 0, opt.masked,
                                                                       opt.scale, opt.margin, opt.k, True, True)
            assert torch.equal(_bits(losses), _bits(d.losses)) and torch.equal(_bits(stats), _bits(d.stats)), tag
        assert torch.equal(_bits(loss), _bits(d.losses[hid])), tag
        (2.0 * loss).backward()
        assert torch.equal(_bits(qd.grad), _bits(2.0 * d.d_query)), tag
        assert torch.equal(_bits(cd.grad), _bits(2.0 * d.d_cand)), tag

