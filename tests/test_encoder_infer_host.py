"""CPU-side test (no GPU) of the forward-only encoder entry (csrc/encoder.hip: xfmr_encoder_infer_workspace_bytes,
xfmr_encoder_infer): what its workspace holds -- nothing per layer but the bf16 parameter copy, sized by the rows actually run
--, where the configuration is refused, and what the call refuses before it launches anything. Host code only: the refusals
return before the first launch, so no device is touched."""

import ctypes as C
import itertools
import pathlib
import re

import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]
F32, BF16 = 0, 1
BIDIRECTIONAL, LN_UNFUSED, FFN_UNFUSED = 1, 2, 4
OK, EINVAL, EUNSUPPORTED, EWORKSPACE, EALIGN = 0, -1, -2, -3, -5
HANDLE = 0x1000  # a dummy non-null, 16-byte aligned device pointer: nothing here dereferences it

# BASELINE.json's five configurations as bench.py's presets shape them: (seq_len, hidden, inter, layers)
BASELINE_SHAPES = {
    "config1": (50, 64, 256, 2),
    "config2": (200, 128, 512, 4),
    "config3": (200, 128, 512, 4),
    "config4": (200, 256, 1024, 6),
    "config5": (512, 256, 1024, 4),
}


@pytest.fixture(scope="module")
def native():
    from xfmr_rec_amd import _native as N

    if not N.LIB_PATH.exists():
        pytest.fail(f"{N.LIB_PATH} missing: run build() first")
    return N


def make(native, batch, seq_len, hidden=128, inter=512, layers=2, precision=BF16, flags=0, packed_rows=0, heads=None,
         hidden_dropout=0.0, attn_dropout=0.0, max_pos=None):
    return native.EncoderCfg(batch=batch, seq_len=seq_len, hidden=hidden, heads=heads or hidden // 32, inter=inter,
                             layers=layers, max_pos=max_pos or seq_len, precision=precision, ln_eps=1e-12, flags=flags,
                             hidden_dropout=hidden_dropout, attn_dropout=attn_dropout,
                             seq_offsets=HANDLE if packed_rows else None, row_pos=HANDLE if packed_rows else None,
                             packed_rows=packed_rows)


def sizes(native, cfg):
    lib = native.load()
    return lib.xfmr_encoder_workspace_bytes(C.byref(cfg)), lib.xfmr_encoder_infer_workspace_bytes(C.byref(cfg))


def test_refused_exactly_where_the_training_workspace_is(native):
    refused = [
        dict(batch=0, seq_len=24), dict(batch=4, seq_len=0), dict(batch=4, seq_len=24, layers=0),
        dict(batch=4, seq_len=24, heads=3),                      # head size 128 / 3
        dict(batch=4, seq_len=24, inter=130),                    # inter not a multiple of 4
        dict(batch=4, seq_len=24, max_pos=23),                   # seq_len > max_pos
        dict(batch=4, seq_len=24, precision=7), dict(batch=4, seq_len=24, flags=1 << 20),
        dict(batch=4, seq_len=24, packed_rows=4 * 24 + 1),       # more packed rows than batch x seq_len
        dict(batch=4, seq_len=24, packed_rows=50, precision=F32),            # packed rows: fp32 policy,
        dict(batch=4, seq_len=24, packed_rows=50, heads=2),                  # head size 64,
        dict(batch=4, seq_len=24, packed_rows=50, flags=BIDIRECTIONAL),      # bidirectional
    ]
    for kw in refused:
        assert sizes(native, make(native, **kw)) == (0, 0), kw
    accepted = [
        dict(batch=4, seq_len=24), dict(batch=4, seq_len=24, heads=2), dict(batch=4, seq_len=24, precision=F32),
        dict(batch=4, seq_len=24, flags=BIDIRECTIONAL), dict(batch=4, seq_len=24, packed_rows=50),
        dict(batch=4, seq_len=24, packed_rows=4 * 24), dict(batch=3, seq_len=600, hidden=64, inter=128),
        dict(batch=4, seq_len=24, hidden_dropout=0.1),           # (the size query does not look at dropout: the call refuses it)
    ]
    for kw in accepted:
        train, infer = sizes(native, make(native, **kw))
        assert train > 0 and infer > 0, kw
    lib = native.load()
    assert lib.xfmr_encoder_workspace_bytes(None) == 0 and lib.xfmr_encoder_infer_workspace_bytes(None) == 0


@pytest.mark.parametrize("name", sorted(BASELINE_SHAPES))
def test_smaller_than_the_training_workspace_at_the_baseline_shapes(native, name):
    L, H, I, layers = BASELINE_SHAPES[name]
    for batch, prec in itertools.product((32, 512), (BF16, F32)):
        train, infer = sizes(native, make(native, batch, L, hidden=H, inter=I, layers=layers, precision=prec))
        assert 0 < infer < train, (name, batch, prec, infer, train)


def test_independent_of_the_layer_count_but_for_the_parameter_copy(native):
    lib = native.load()
    shapes = [(4, 24, 64, 128), (62, 200, 128, 512), (82, 200, 128, 512), (82, 200, 128, 320), (32, 512, 256, 1024)]
    for (b, L, H, I), flags in itertools.product(shapes, (0, LN_UNFUSED, FFN_UNFUSED)):
        c1, c8 = (make(native, b, L, hidden=H, inter=I, layers=n, flags=flags) for n in (1, 8))
        grow = sizes(native, c8)[1] - sizes(native, c1)[1]
        params = lib.xfmr_param_count(C.byref(c8)) - lib.xfmr_param_count(C.byref(c1))
        assert 0 <= grow <= 2 * params + 256, (b, L, H, I, flags, grow, params)  # bf16 copy + the carve's 256-byte rounding
        f1, f8 = (make(native, b, L, hidden=H, inter=I, layers=n, flags=flags, precision=F32) for n in (1, 8))
        assert sizes(native, f8)[1] == sizes(native, f1)[1]  # fp32 policy: no copy at all


def test_non_decreasing_in_batch_seq_len_and_packed_rows(native):
    def infer(**kw):
        n = sizes(native, make(native, **kw))[1]
        assert n > 0, kw
        return n

    for prec in (BF16, F32):
        by_batch = [infer(batch=b, seq_len=200, precision=prec) for b in (1, 2, 31, 61, 62, 63, 81, 82, 83, 128, 512)]
        assert by_batch == sorted(by_batch), by_batch
        # (seq_len 61 / 62 x batch 200 and 81 / 82 cross the 12 288- and 16 384-token form thresholds)
        by_len = [infer(batch=200, seq_len=s, precision=prec, max_pos=600) for s in (1, 7, 61, 62, 81, 82, 83, 200, 513, 600)]
        assert by_len == sorted(by_len), by_len
    # packed rows: by the rows actually run, on both sides of the thresholds (the forms follow batch x seq_len, the sizes the
    # rows), and never more than the padded configuration of the same batch
    for b, L in ((62, 200), (82, 200), (128, 200), (3, 40)):
        padded = infer(batch=b, seq_len=L)
        steps = sorted({1, 2, 63, 64, 65, 4095, 4096, 12287, 12288, 12289, 16383, 16384, 16385, b * L - 1, b * L})
        by_rows = [infer(batch=b, seq_len=L, packed_rows=r) for r in steps if 1 <= r <= b * L]
        assert by_rows == sorted(by_rows), (b, L, by_rows)
        assert by_rows[-1] <= padded and by_rows[0] < padded, (b, L, by_rows[-1], padded)


def test_refusals_come_before_any_launch(native):
    """Every call below returns from the entry's own checks: nothing is launched, no pointer is dereferenced."""
    lib = native.load()
    cfg = make(native, 4, 24, hidden=64, inter=128)
    need = lib.xfmr_encoder_infer_workspace_bytes(C.byref(cfg))
    ptrs = dict(params=HANDLE, item_idx=HANDLE, table=HANDLE, tok=HANDLE, key_mask=HANDLE, workspace=HANDLE)

    def call(cfg=cfg, nbytes=need, **over):
        p = ptrs | over
        return lib.xfmr_encoder_infer(C.byref(cfg) if cfg is not None else None, p["params"], p["item_idx"], p["table"], 101,
                                      p["tok"], p["key_mask"], p["workspace"], nbytes, None)

    assert call(cfg=None) == EINVAL
    for name in ptrs:
        assert call(**{name: None}) == EINVAL, name
    for name in ("params", "table", "tok", "workspace"):
        assert call(**{name: HANDLE + 4}) == EALIGN, name
    assert call(params=None, tok=HANDLE + 4) == EINVAL  # a null pointer is reported before a misaligned one
    assert call(nbytes=need - 1) == EWORKSPACE
    assert call(nbytes=0) == EWORKSPACE
    assert call(tok=HANDLE + 4, nbytes=need - 1) == EALIGN  # ... and alignment before the workspace size
    # this entry is eval: any dropout is refused, before the pointers are looked at
    for kw in (dict(hidden_dropout=0.1), dict(attn_dropout=0.1)):
        drop = make(native, 4, 24, hidden=64, inter=128, **kw)
        assert call(cfg=drop) == EINVAL and call(cfg=drop, nbytes=0) == EINVAL
    # the configuration's own rules, as the training forward applies them
    assert call(cfg=make(native, 4, 24, heads=3)) == EUNSUPPORTED
    assert call(cfg=make(native, 4, 24, packed_rows=50, precision=F32)) == EUNSUPPORTED
    assert call(cfg=make(native, 4, 24, packed_rows=4 * 24 + 1)) == EINVAL
    # the same calls on the training forward give the same codes (one precedence for both entries)
    train_need = lib.xfmr_encoder_workspace_bytes(C.byref(cfg))

    def train(nbytes=train_need, **over):
        p = ptrs | over
        return lib.xfmr_encoder_fwd(C.byref(cfg), p["params"], p["item_idx"], p["table"], 101, p["tok"], p["key_mask"],
                                    p["workspace"], nbytes, None)

    assert train(params=None, tok=HANDLE + 4) == EINVAL and train(tok=HANDLE + 4, nbytes=0) == EALIGN
    assert train(nbytes=train_need - 1) == EWORKSPACE


def test_abi_is_still_3_and_both_symbols_are_declared_exported_and_bound(native):
    header = (ROOT / "include" / "xfmr_hip.h").read_text()
    assert re.search(r"#define\s+XFMR_ABI_VERSION\s+3\b", header) and native.ABI_VERSION == 3
    assert native.load().xfmr_abi_version() == 3
    raw = C.CDLL(str(native.LIB_PATH))
    for name, nargs in (("xfmr_encoder_infer_workspace_bytes", 1), ("xfmr_encoder_infer", 10)):
        assert re.search(rf"\b{name}\s*\(", header), name
        assert hasattr(raw, name), name
        assert name in native.EXPORTED_SYMBOLS
        fn = getattr(native.load(), name)
        assert fn.argtypes is not None and len(fn.argtypes) == nargs
    assert native.load().xfmr_encoder_infer_workspace_bytes.restype is C.c_size_t
    # the cfg keeps its layout and no flag bit was added
    assert C.sizeof(native.EncoderCfg) == 136
    assert re.search(r"XFMR_ENC_FLAGS_ALL\s*=\s*255u\b", header)
