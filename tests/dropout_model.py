"""Host restatement of the kernels' dropout masks (csrc/common.h: xf_hash32, xf_make_dropout, xf_drop_resolve,
xf_drop_rowkey, xf_keep_scale_rc, kDropColMul), in numpy uint32 arithmetic. A mask is a pure function of
(seed, site, row, column, p) -- plus the device step counter where one is in use -- so a test can build the mask a kernel
applied without asking any kernel for it. test_dropout_model_host.py pins this module to known answers of a stand-alone host
build of those functions (scripts/probe/dropout_host_model.hip -> tests/golden/dropout_model.json).

    h(x)    = xf_hash32:  x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16      (mod 2^32)
    key     = h(lo32(seed) ^ h(hi32(seed) + 0x9E3779B9 * (site + 1)))
    key     = h(key ^ (step * 0x9E3779B9 + 0x7F4A7C15))                 only with a device step counter `step`
    thresh  = (uint32)((double)(float)p * 2^32)                         p is a FLOAT32: 0.1f -> 429 496 736
    keep   <=> ((h(row ^ key) ^ col * 0x9E3779B1) * 0x7feb352d mod 2^32) >= thresh
    scale   = 1.f / (1.f - p) in fp32                                   1.11111116 for 0.1f

Row and column of an element, read from the kernels:

* Hidden-state sites (embedding LayerNorm output; attention-output and FFN-output Linear): row = the row of the [rows][N]
  tensor as it is stored, column = the feature. Padded layout: row = b * L + l. PACKED layout (xfmr_encoder_cfg.seq_offsets):
  the token axis holds each sequence's own rows only, and the row is the PACKED row index (gemm.hip's `m`, norm.hip's `row`),
  not b * L + l -- padded and packed runs of the same batch draw different hidden masks by design.
* Attention probabilities: row = (b * A + h) * L + q, column = the key position (attention.hip: xf_drop_rowkey(a.drop,
  blockIdx.y * L + q) with blockIdx.y = b * A + h). In the packed layout b is the sequence's SLOT in seq_offsets, q and the
  key are positions inside the sequence, and L stays the cfg's seq_len ("lse and the dropout row keys stay indexed by L"):
  the attention mask of slot b equals the padded layout's mask of batch row b.

Sites (encoder.hip): SITE_EMB = 0, site_attn(i) = 1 + 4 i, site_out(i) = 2 + 4 i, site_ffn(i) = 3 + 4 i.
Seed (models.py::_cfg_kwargs): (_seed * 0x9E3779B97F4A7C15 + _step) mod 2^64, `_step` incremented BEFORE the forward; with
use_device_step the host part is _seed * 0x9E3779B97F4A7C15 alone and the counter is mixed into the key on the device."""

from __future__ import annotations

import numpy as np

M32 = 0xFFFFFFFF
K_COL_MUL = 0x9E3779B1
SITE_EMB = 0


def site_attn(i: int) -> int:
    return 1 + 4 * i


def site_out(i: int) -> int:
    return 2 + 4 * i


def site_ffn(i: int) -> int:
    return 3 + 4 * i


def model_seed(seed: int, step: int, device_step: bool = False) -> int:
    """The 64-bit seed the model hands the encoder for its forward number `step` (1 for the first training forward)."""
    return (int(seed) * 0x9E3779B97F4A7C15 + (0 if device_step else int(step))) & 0xFFFFFFFFFFFFFFFF


def _h(x):
    """xf_hash32 on a uint32 array (wrap-around arithmetic)."""
    x = np.asarray(x, dtype=np.uint32).copy()
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x7FEB352D)
    x ^= x >> np.uint32(15)
    x *= np.uint32(0x846CA68B)
    x ^= x >> np.uint32(16)
    return x


def _h1(x: int) -> int:
    with np.errstate(over="ignore"):
        return int(_h(np.array([x & M32], dtype=np.uint32))[0])


def drop_key(seed: int, site: int, step=None) -> int:
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    key = _h1((seed & M32) ^ _h1((seed >> 32) + 0x9E3779B9 * (int(site) + 1)))
    if step is not None:
        key = _h1(key ^ (((int(step) & M32) * 0x9E3779B9 + 0x7F4A7C15) & M32))
    return key


def thresh(p) -> int:
    p = np.float32(p)
    return 0xFFFFFFFF if p >= 1 else int(np.float64(p) * 4294967296.0)


def scale(p) -> float:
    """1.f / (1.f - p), the fp32 value (as a Python float)."""
    p = np.float32(p)
    return float(np.float32(1.0) / (np.float32(1.0) - p)) if p > 0 else 1.0


def keep_rc(key: int, rows, cols, p):
    """0/1 uint8 array [len(rows)][len(cols)] for explicit uint32 row and column indices."""
    rows = np.asarray(rows, dtype=np.int64).astype(np.uint32)
    cols = np.asarray(cols, dtype=np.int64).astype(np.uint32)
    if not np.float32(p) > 0:
        return np.ones((rows.size, cols.size), dtype=np.uint8)
    with np.errstate(over="ignore"):
        rk = _h(rows ^ np.uint32(key))
        x = (rk[:, None] ^ (cols * np.uint32(K_COL_MUL))[None, :]) * np.uint32(0x7FEB352D)
    return (x >= np.uint32(thresh(p))).astype(np.uint8)


def hidden_keep(seed, site, rows: int, cols: int, p, step=None, row_index=None):
    """[rows][cols] mask of a hidden-state site. `row_index`: the stored row of each of the `rows` rows when it is not
    0 .. rows - 1 (e.g. the padded position b * L + l of packed rows, to restate a padded run row by row)."""
    r = np.arange(rows) if row_index is None else np.asarray(row_index)
    assert r.shape == (rows,)
    return keep_rc(drop_key(seed, site, step), r, np.arange(cols), p)


def attention_keep(seed, site, B: int, A: int, L: int, p, step=None):
    """(B, A, L, L) mask of attention-probability dropout: [b, h, q, key]."""
    return keep_rc(drop_key(seed, site, step), np.arange(B * A * L), np.arange(L), p).reshape(B, A, L, L)
