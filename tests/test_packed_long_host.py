"""Host-side surface of the packed layout (xfmr_encoder_cfg.seq_offsets) beyond 512 rows per sequence, where attention
runs its key-streaming forms: check_cfg accepts the bf16 policy at head size 32, causal, at any length -- the workspace
is the padded configuration's -- and still refuses every combination no kernel walks offsets for. The error text says so
(no GPU needed)."""

import ctypes as C

import pytest

F32, BF16 = 0, 1
BIDIRECTIONAL = 1
HANDLE = 0x1000  # a dummy non-null device pointer: the configuration check only asks whether it is null


@pytest.fixture(scope="module")
def native():
    from xfmr_rec_amd import _native as N

    if not N.LIB_PATH.exists():
        pytest.fail(f"{N.LIB_PATH} missing: run build() first")
    return N


def _workspace_bytes(native, seq_len, *, packed, hidden=64, heads=2, precision=BF16, flags=0, row_pos=True, batch=3):
    lib = native.load()
    kw = dict(batch=batch, seq_len=seq_len, hidden=hidden, heads=heads, inter=128, layers=2, max_pos=seq_len,
              precision=precision, ln_eps=1e-12, flags=flags)
    if packed:
        kw |= dict(seq_offsets=HANDLE, row_pos=HANDLE if row_pos else None, packed_rows=seq_len + 7)
    cfg = native.EncoderCfg(**kw)
    return int(lib.xfmr_encoder_workspace_bytes(C.byref(cfg)))


@pytest.mark.parametrize("seq_len", [513, 2048])
def test_packed_rows_are_accepted_beyond_512_and_sized_as_the_padded_layout(native, seq_len):
    padded = _workspace_bytes(native, seq_len, packed=False)
    assert padded > 0
    assert _workspace_bytes(native, seq_len, packed=True) == padded  # (sized for batch x seq_len, as at every length)


@pytest.mark.parametrize("seq_len", [513, 2048])
@pytest.mark.parametrize("bad", [dict(precision=F32), dict(flags=BIDIRECTIONAL), dict(heads=1), dict(row_pos=False)],
                         ids=["fp32", "bidirectional", "head-size-64", "no-row_pos"])
def test_packed_rows_stay_refused_where_no_kernel_walks_offsets(native, seq_len, bad):
    assert _workspace_bytes(native, seq_len, packed=False, **{k: v for k, v in bad.items() if k != "row_pos"}) > 0
    assert _workspace_bytes(native, seq_len, packed=True, **bad) == 0


def test_unsupported_text_names_both_packed_forms(native):
    lib = native.load()
    text = lib.xfmr_strerror(-2).decode()
    assert text.startswith("shape not supported")
    assert "L <= 512" in text  # where the one-workgroup forms stop and the key-streaming forms take over
    assert "L <= 512, causal)" not in text  # the old closing words: a length limit of the packed layout
    assert "key-streaming" in text and "any length" in text
