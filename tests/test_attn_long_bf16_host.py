"""Host-side surface of the key-streaming bf16 head-size-32 attention kernels: no ABI change, the same mode bit, and the
header and error text no longer describe a length limit or an ignored bit (no GPU needed)."""

import pathlib
import re

import pytest

HEADER = pathlib.Path(__file__).resolve().parents[1] / "include" / "xfmr_hip.h"


@pytest.fixture(scope="module")
def native():
    from xfmr_rec_amd import _native

    return _native


def test_abi_version_is_unchanged():
    assert re.search(r"^#define\s+XFMR_ABI_VERSION\s+3\s*$", HEADER.read_text(), re.M)


def test_stream_keys_mode_bit_is_unchanged(native):
    assert native.ATTN_STREAM_KEYS == 2
    assert re.search(r"XFMR_ATTN_STREAM_KEYS\s*=\s*2\b", HEADER.read_text())


def test_header_says_what_the_bit_selects_in_bf16_at_head_size_32():
    text = HEADER.read_text()
    end = text.index("enum { XFMR_ATTN_STREAM_KEYS")
    comment = text[text.rindex("/*", 0, end):end]
    assert "ignores it" not in comment
    assert "bf16" in comment and "head size 32" in comment and "bit-identical" in comment


def test_unsupported_text_drops_the_bf16_attention_length_limit(native):
    text = native.load().xfmr_strerror(-2).decode()
    assert text.startswith("shape not supported")
    assert "L <= 1024 (packed" not in text
    assert "L <= 512" in text  # the packed layout is the remaining limit
