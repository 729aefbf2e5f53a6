"""dropout_model.py (the numpy restatement of the kernels' dropout masks) against known answers of a host build of
common.h's own functions -- tests/golden/dropout_model.json, printed by scripts/probe/dropout_host_model.hip -- and against
what a dropout mask has to be. No GPU and nothing compiled: the GPU tests judge kernels by this model, so it is pinned first."""

import json
import struct

import numpy as np
import pytest

import dropout_model as dm


def _f32(bits):
    return struct.unpack("<f", struct.pack("<I", bits))[0]


@pytest.fixture(scope="module")
def golden(golden_dir):
    return json.loads((golden_dir / "dropout_model.json").read_text())


def test_known_answers_of_the_issue():
    """The numbers written down before any of this was built (p = 0.1f throughout)."""
    want = {(5, 0): 1509349684, (5, 3): 95825044, (5, 9): 3768759902, (6018027440424182934, 0): 912943853,
            (6018027440424182934, 3): 3849509318, (6018027440424182934, 9): 724413455}
    for (seed, site), key in want.items():
        assert dm.drop_key(seed, site) == key, (seed, site)
    assert dm.drop_key(5, 3, step=41) == 1211467697
    keep = dm.hidden_keep(5, 0, 300, 130, np.float32(0.1), row_index=np.arange(300) * 977)
    assert int(keep.sum()) == 35105


def test_host_build_fixture(golden):
    """18 (p, seed, site) cases of 300 x 130 elements: key, threshold, fp32 scale, kept count, an order-sensitive FNV-1a
    signature of the keep bits and the first row verbatim; and the step-counter keys."""
    assert len(golden["cases"]) == 18 and len(golden["steps"]) == 8
    rows = np.arange(golden["rows"]) * golden["row_mul"]
    for c in golden["cases"]:
        p = _f32(c["p_bits"])
        tag = (p, c["seed"], c["site"])
        assert dm.drop_key(c["seed"], c["site"]) == c["key"], tag
        assert dm.thresh(p) == c["thresh"], tag
        assert struct.pack("<f", dm.scale(p)) == struct.pack("<I", c["scale_bits"]), tag
        keep = dm.hidden_keep(c["seed"], c["site"], golden["rows"], golden["cols"], p, row_index=rows)
        assert keep.shape == (golden["rows"], golden["cols"])
        assert int(keep.sum()) == c["kept"], tag
        assert "".join("01"[k] for k in keep[0]) == c["row0"], tag
        sig = 2166136261
        for k in keep.ravel().tolist():
            sig = ((sig ^ k) * 16777619) & 0xFFFFFFFF
        assert sig == c["sig"], tag
    for s in golden["steps"]:
        assert dm.drop_key(s["seed"], s["site"], step=s["step"]) == s["key"], s
    # step 0 still mixes: a device counter at zero is not "no counter"
    assert dm.drop_key(5, 3, step=0) != dm.drop_key(5, 3)


def test_threshold_takes_p_as_float32_not_double():
    assert dm.thresh(0.1) == 429496736 == dm.thresh(np.float32(0.1))  # (double)(0.1f) * 2^32
    assert int(0.1 * 4294967296.0) == 429496729  # what a Python double would give: 7 hashes apart
    assert dm.scale(0.1) == float(np.float32(1.0) / np.float32(0.9)) != 1 / 0.9
    assert abs(dm.scale(0.1) - 1.11111116) < 1e-8
    assert dm.thresh(1.0) == 0xFFFFFFFF and dm.thresh(0.0) == 0 and dm.scale(0.0) == 1.0
    # an element whose hash falls between the two thresholds exists and is DROPPED by the float32 rule
    key = dm.drop_key(5, 0)
    with np.errstate(over="ignore"):
        rk = dm._h(np.arange(4096, dtype=np.uint32) ^ np.uint32(key))
        x = (rk[:, None] ^ (np.arange(4096, dtype=np.uint32) * np.uint32(dm.K_COL_MUL))[None, :]) * np.uint32(0x7FEB352D)
    assert np.array_equal(x >= np.uint32(429496736), dm.keep_rc(key, np.arange(4096), np.arange(4096), 0.1).astype(bool))


def test_p_zero_keeps_everything():
    assert dm.hidden_keep(5, 3, 77, 130, 0.0).all()
    assert dm.attention_keep(5, 1, 2, 2, 40, 0.0).all()


@pytest.mark.parametrize("p", [0.1, 0.25, 0.3])
def test_keep_rate_overall_and_per_row(p):
    """A smoke check of the RATE only, at 300 x 512 (the largest M and N of the op-level mask tests): it would notice a wrong
    threshold or a lost bit of the hash, and that is all it claims. It does NOT show that the rows are binomial, and they are
    not: the per-row tail of this hash is heavier, and this table's 4.9 / 4.8 / 4.3 sigma (p = 0.1 / 0.25 / 0.3; 300 binomial
    rows would reach about 3) already says so. Larger tables exceed 5 sigma: 2048 x 512 reaches 5.6 / 5.3 at p = 0.1 / 0.25,
    and at (seed 1234, site 7), 8192 x 128, p = 0.1 row 6483 keeps 84 of 128 elements, 9.2 sigma low -- a weakness of the
    xor-multiply element step for certain row keys, the same on the device (the kernels equal this model bit for bit). It is
    not repaired here, because another element step changes every mask the product draws; DESIGN.md section 7 lists it as
    open work of its own, and test_known_heavy_row_of_the_element_step below keeps the figure in sight."""
    rows, cols = 300, 512
    keep = dm.hidden_keep(1234, 7, rows, cols, p).astype(np.float64)
    p32 = float(np.float32(p))
    sigma = (p32 * (1 - p32)) ** 0.5
    assert abs(keep.mean() - (1 - p32)) <= 5 * sigma / (rows * cols) ** 0.5
    assert np.abs(keep.mean(1) - (1 - p32)).max() <= 5 * sigma / cols ** 0.5
    assert np.abs(keep.mean(0) - (1 - p32)).max() <= 5 * sigma / rows ** 0.5


def test_known_heavy_row_of_the_element_step():
    """The recorded outlier, as a known answer: (seed 1234, site 7), p = 0.1, 128 columns, row 6483 keeps 84 elements where
    115 are expected (9.2 sigma of a binomial), and the 8192 rows' z-scores otherwise have unit spread. Whoever replaces the
    element step meets this test and replaces it with a bound on the tail."""
    keep = dm.hidden_keep(1234, 7, 8192, 128, 0.1).astype(np.float64)
    p32 = float(np.float32(0.1))
    z = (keep.mean(1) - (1 - p32)) / (p32 * (1 - p32) / 128) ** 0.5
    assert int(keep[6483].sum()) == 84 and int(np.argmin(z)) == 6483
    assert 0.95 <= z.std() <= 1.05


def test_site_seed_and_step_change_the_mask():
    base = dm.hidden_keep(5, 3, 64, 128, 0.25)
    n = base.size
    for other in (dm.hidden_keep(5, 4, 64, 128, 0.25), dm.hidden_keep(6, 3, 64, 128, 0.25),
                  dm.hidden_keep(5 + (1 << 32), 3, 64, 128, 0.25), dm.hidden_keep(5, 3, 64, 128, 0.25, step=0),
                  dm.hidden_keep(5, 3, 64, 128, 0.25, step=1)):
        agree = float((other == base).mean())
        assert abs(agree - (0.75 ** 2 + 0.25 ** 2)) <= 6 * 0.5 / n ** 0.5  # independent masks agree at (1-p)^2 + p^2
    assert np.array_equal(dm.hidden_keep(5, 3, 64, 128, 0.25, step=1), dm.hidden_keep(5, 3, 64, 128, 0.25, step=1))
    assert not np.array_equal(dm.hidden_keep(5, 3, 64, 128, 0.25, step=1), dm.hidden_keep(5, 3, 64, 128, 0.25, step=2))


def test_attention_rows_are_batch_head_query():
    B, A, L, p = 2, 3, 40, 0.1
    m = dm.attention_keep(9, dm.site_attn(1), B, A, L, p)
    assert m.shape == (B, A, L, L)
    key = dm.drop_key(9, 5)
    for b, h, q in ((0, 0, 0), (1, 2, 39), (1, 0, 7)):
        assert np.array_equal(m[b, h, q], dm.keep_rc(key, [(b * A + h) * L + q], np.arange(L), p)[0])
    assert not np.array_equal(m[0, 0], m[0, 1]) and not np.array_equal(m[0, 0], m[1, 0])
    # the same flat rows as a hidden-state site of that key would draw: one rule for both kinds
    assert np.array_equal(m.reshape(B * A * L, L), dm.hidden_keep(9, 5, B * A * L, L, p))


def test_sites_and_model_seed():
    assert (dm.SITE_EMB, dm.site_attn(0), dm.site_out(0), dm.site_ffn(0)) == (0, 1, 2, 3)
    assert (dm.site_attn(2), dm.site_out(2), dm.site_ffn(2)) == (9, 10, 11)
    assert dm.model_seed(0, 1) == 1 and dm.model_seed(3, 2) == (3 * 0x9E3779B97F4A7C15 + 2) % 2 ** 64
    assert dm.model_seed(3, 2, device_step=True) == (3 * 0x9E3779B97F4A7C15) % 2 ** 64
