"""Host-side surface of the key-streaming attention kernels: the mode bit and the error text (no GPU needed)."""

import pytest


@pytest.fixture(scope="module")
def native():
    from xfmr_rec_amd import _native

    return _native


def test_stream_keys_mode_bit(native):
    assert native.ATTN_STREAM_KEYS == 2
    assert native.ATTN_STREAM_KEYS & (native.ATTN_CAUSAL | native.ATTN_BIDIRECTIONAL) == 0


def test_unsupported_text_drops_the_attention_length_limits(native):
    text = native.load().xfmr_strerror(-2).decode()
    assert text.startswith("shape not supported")
    assert "L <= 256 in the fp32 policy" not in text
    assert "L <= 128 in fp32" not in text
