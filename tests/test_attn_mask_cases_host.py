"""What makes the mask table of tests/attn_mask_cases.py worth its GPU time, shown on the CPU through the SAME `check`
test_gpu_attn_masks.py uses:
  (a) the unmutated tile-walking model passes every sequence at the fp32 tolerance;
  (b) every mutant of attn_mask_cases.MUTANTS fails `check` (at the looser bf16 tolerance) on sequences this file names, at
      both causal settings where the mutant applies, with only that sequence's outputs replaced by the mutant's;
  (c) headroom: the bf16 rounding model (_attention_bf16_emulation on the inputs rounded to bf16) stays at or below one
      third of each bf16 limit against the fp64 reference of the UNROUNDED inputs, on every sequence of every shape the GPU
      file uses -- a sequence that breaks this gets another seed or pattern, never a wider limit;
  (d) the masks reach the paths they are in the table for, asserted from the masks themselves."""

import pytest
import torch

import attn_mask_cases as MC
from helpers import TOL
from test_gpu_ops import _attention_bf16_emulation

A = 2
# (L, dh of the bf16 form at that length, key chunk) of test_gpu_attn_masks.py; each at both causal settings
SHAPES = ((130, 32, 128), (290, 32, 256), (162, 64, 128))
STREAM_SHAPES = ((290, 32, 256), (162, 64, 128))

# mutant -> causal -> sequences that must catch it (through ctx / d_qkv alone unless LSE_ONLY names the pair)
CATCHES = {
    # query 0 (left1), 0..30 (left31), 32 (left33), `chunk` (left_chunk) sit at -inf beside rows of the same wave that have
    # seen a key; left32 does NOT catch it: its first tile is empty for the whole wave, which `continue` steps over
    "alpha_without_msafe": {True: ("left1", "left31", "left33", "left_chunk", "bern", "last_only", "two")},
    "interior_ignores_mask": {True: ("left32", "tile1", "tile1_pm1", "bern", "even", "none"),
                              False: ("left32", "tile1", "tile1_pm1", "bern", "even", "first_only", "none")},
    "chunk_bits_not_rebased": {True: ("left_chunk", "left1", "bern", "last_only", "two"),
                               False: ("left_chunk", "left1", "bern", "first_only", "last_only", "two")},
    # `even` does NOT catch it (key - 4 has the key's parity), nor do the word-aligned left32 / tile1
    "halfwave_shift_dropped": {True: ("left1", "left31", "left33", "tile1_pm1", "bern", "two"),
                               False: ("left1", "left31", "left33", "tile1_pm1", "bern", "first_only", "two")},
    "stops_at_first_empty_tile": {True: ("left32", "left33", "left_chunk", "tile1", "tile1_pm1", "last_only", "two"),
                                  False: ("left32", "left33", "left_chunk", "tile1", "tile1_pm1", "last_only", "two")},
    "mask_as_length": {True: ("left1", "left31", "left32", "left33", "left_chunk", "tile1", "tile1_pm1", "bern", "even",
                              "last_only", "two"),
                       False: ("left1", "left31", "left32", "left33", "left_chunk", "tile1", "tile1_pm1", "bern", "even",
                               "last_only", "two")},
    # w is zero on masked rows and a row without keys is a masked row (causal) or the whole of `none` (bidirectional), so
    # dO = 0 there and P = exp(s) is multiplied away: d_qkv cannot show this one. `check` therefore takes the stored lse
    # and requires +inf on those rows -- the case added for this mutant
    "empty_row_lse_zero": {True: ("left1", "left32", "left_chunk", "last_only", "two", "none"), False: ("none",)},
}
LSE_ONLY = ("empty_row_lse_zero",)


def fails(fn):
    """True when the check raises its AssertionError (the mutant is caught)."""
    try:
        fn()
    except AssertionError:
        return True
    return False


def _caught(c, mutant, with_lse):
    """The sequences on which `check` fails when that sequence alone carries the mutant's outputs (the others the reference)."""
    ctx, d, lse = MC.model(c, mutant)
    out = []
    for b, name in enumerate(MC.NAMES):
        cx, dd, ll = c.ref_ctx.clone(), c.ref_grad.clone(), c.ref_lse.clone()
        cx[b], dd[b], ll[b] = ctx[b], d[b], lse[b]
        if fails(lambda: MC.check(mutant, "bf16", cx, dd, c, lse=ll if with_lse else None)):
            out.append(name)
    return out


def _applies(mutant, shape, causal):
    return not ((mutant in MC.CAUSAL_ONLY and not causal) or (mutant in MC.STREAMING_ONLY and shape not in STREAM_SHAPES))


# ---------------------------------------------------------------------------------------------------- (a) the model passes
@pytest.mark.parametrize("causal", [True, False], ids=["causal", "bidirectional"])
@pytest.mark.parametrize("L,dh,chunk", SHAPES)
def test_unmutated_model_passes(L, dh, chunk, causal):
    c = MC.case(L, A, dh, chunk, causal)
    ctx, d, lse = MC.model(c)
    figs = MC.check("model", "fp32", ctx, d, c, lse=lse)
    print(MC.fig_line(f"model L={L} dh={dh} chunk={chunk} causal={causal}", figs))
    assert set(figs) == set(MC.NAMES) and len(MC.NAMES) == 13


# ---------------------------------------------------------------------------------------------------- (b) mutants fail
def test_every_mutant_is_named_here_and_every_family_catches_one():
    assert set(CATCHES) == set(MC.MUTANTS)
    for mutant, by_causal in CATCHES.items():
        assert set(by_causal) == ({True} if mutant in MC.CAUSAL_ONLY else {True, False})
    named = {n for by_causal in CATCHES.values() for names in by_causal.values() for n in names}
    assert named == set(MC.NAMES)  # a mask family that catches no mutant is dropped from the table


@pytest.mark.parametrize("mutant", MC.MUTANTS)
def test_mutant_is_caught_by_the_named_sequences(mutant):
    for shape in SHAPES:
        for causal, names in CATCHES[mutant].items():
            if not _applies(mutant, shape, causal):
                continue
            c = MC.case(shape[0], A, shape[1], shape[2], causal)
            got = _caught(c, mutant, with_lse=mutant in LSE_ONLY)
            print(f"FIG attn-masks mutant {mutant} L={shape[0]} causal={causal}: caught by {', '.join(got)}")
            assert set(names) <= set(got), (mutant, shape, causal, sorted(set(names) - set(got)))
            if mutant in LSE_ONLY:  # ... and by nothing else: that is why `check` takes lse
                assert _caught(c, mutant, with_lse=False) == []


def test_mutant_free_columns_are_what_the_comments_say():
    """The sequences the table above says do NOT catch a mutant really do not (the comments are part of the record)."""
    c = MC.case(130, A, 32, 128, True)
    assert "left32" not in _caught(c, "alpha_without_msafe", False)
    got = _caught(c, "halfwave_shift_dropped", False)
    assert not {"even", "left32", "tile1"} & set(got)


# ---------------------------------------------------------------------------------------------------- (c) headroom
@pytest.mark.parametrize("causal", [True, False], ids=["causal", "bidirectional"])
@pytest.mark.parametrize("L,dh,chunk", SHAPES + ((162, 32, 128),))
def test_bf16_rounding_model_keeps_two_thirds_of_every_limit(L, dh, chunk, causal):
    """(162, 32) is the fp32 form's shape: listed so that every (L, chunk, causal) of the GPU file is here at both head sizes."""
    c = MC.case(L, A, dh, chunk, causal)
    r = lambda t: t.to(torch.bfloat16).float()  # noqa: E731
    ctx, d, _lse = _attention_bf16_emulation(r(c.qkv), c.mask, A, r(c.w), causal)
    figs = MC.check("rounding model", "bf16", ctx, d, c)
    print(MC.fig_line(f"rounding-model L={L} dh={dh} chunk={chunk} causal={causal}", figs))
    for name, f in figs.items():
        assert f["ctx"] <= TOL["bf16"]["val"] / 3, (name, f)
        for s in MC.SLICES:
            assert f[s] <= TOL["bf16"]["grad_l2"] / 3, (name, s, f)


# ---------------------------------------------------------------------------------------------------- (d) what it reaches
def _words(m):
    """32-bit mask words of an (L,) mask, the last one zero-padded."""
    L = m.shape[0]
    pad = torch.nn.functional.pad(m, (0, (-L) % 32)).view(-1, 32).bool()
    return pad


@pytest.mark.parametrize("L,dh,chunk", SHAPES)
def test_masks_reach_the_paths_they_are_here_for(L, dh, chunk):
    m = MC.masks(L, chunk)
    assert tuple(m) == MC.NAMES and all(v.shape == (L,) and v.dtype == torch.uint8 for v in m.values())
    first = {n: int(v.nonzero()[0]) for n, v in m.items() if v.any()}
    assert [first[n] for n in ("left1", "left31", "left32", "left33", "left_chunk")] == [1, 31, 32, 33, chunk + 1]
    # a valid query whose first ceil(p / 32) key tiles are empty (left32 / left33: one and two tiles; left_chunk: a chunk's)
    for n, tiles in (("left32", 1), ("left33", 1), ("left_chunk", chunk // 32)):
        w = _words(m[n])
        assert not w[:tiles].any() and w[tiles].any() and bool(m[n][first[n]])
    assert not _words(m["left33"])[1, 0] and _words(m["left33"])[1, 1:].all()  # (the second tile has one hole in front)
    # a wave (32 consecutive queries) in which, under the causal mask, some rows have seen a key after a tile and others not
    for n in ("left1", "left31", "left33", "left_chunk"):
        q0 = 32 * (first[n] // 32)
        assert q0 < first[n] < min(q0 + 32, L)  # rows q0 .. first - 1 see nothing, row `first` sees itself
    assert first["left32"] % 32 == 0  # ... and the word-aligned one where the whole wave steps over the tile together
    # an all-zero 32-bit word between two non-zero words
    for n in ("tile1", "tile1_pm1"):
        w = _words(m[n])
        assert w[0].any() and not w[1].any() and w[2].any()
    assert _words(m["tile1"])[0].all() and _words(m["tile1"])[2].all()  # word-aligned: both neighbours are interior tiles
    assert not _words(m["tile1_pm1"])[0, 31] and not _words(m["tile1_pm1"])[2, 0]  # straddling both
    # a whole chunk of zeros in front of visible keys; a 128-query block with no visible key under the causal mask
    assert not m["left_chunk"][:chunk].any() and m["left_chunk"][chunk + 1:].all() and L > chunk + 1
    assert first["left_chunk"] > 128 and first["last_only"] == L - 1 >= 128 and first["two"] == 40
    # exactly one / two / no visible keys, not at the front
    assert [int(m[n].sum()) for n in ("first_only", "last_only", "two", "none")] == [1, 1, 2, 0]
    assert bool(m["two"][40]) and bool(m["two"][L - 1]) and bool(m["bern"][L - 1])
    # bern: the half-waves' bits differ (bit k of a word against bit k - 4), some word is neither 0 nor all ones
    b = m["bern"]
    key = torch.arange(L)
    assert bool((b != b[key - 4 * ((key >> 2) & 1)]).any()) and 0.3 < float(b.float().mean()) < 0.7
    assert all(0 < int(w.sum()) < 32 for w in _words(b)[:L // 32])
    assert not m["even"][1::2].any() and m["even"][0::2].all()


@pytest.mark.parametrize("causal", [True, False], ids=["causal", "bidirectional"])
def test_case_marks_the_rows_without_keys_and_zeroes_w_on_masked_rows(causal):
    c = MC.case(130, A, 32, 128, causal)
    i = MC.NAMES.index
    assert not c.sees[i("none")].any()
    assert bool((c.w[~c.mask.bool()] == 0).all()) and bool((c.w[c.mask.bool()] != 0).any())
    assert bool((c.ref_grad[i("none")] == 0).all()) and bool((c.ref_ctx[~c.sees] == 0).all())
    assert bool((c.ref_lse[:, 0][~c.sees] == float("inf")).all()) and bool(torch.isfinite(c.ref_lse[:, 0][c.sees]).all())
    if causal:
        assert c.sees[i("left_chunk")].nonzero()[0] == 129 and c.sees[i("last_only")].sum() == 1
        assert c.sees[i("first_only")].all()  # masked queries behind key 0 still see it: ctx there is finite, not checked by value
    else:
        assert all(c.sees[b].all() for b in range(len(MC.NAMES)) if b != i("none"))
    # with one visible key dq and dk are exactly 0 in the reference: the per-slice norm is taken against the whole gradient
    H = A * 32
    g = c.ref_grad[i("last_only")]
    assert float(g[:, :2 * H].abs().max()) < 1e-12 and float(g[:, 2 * H:].norm()) > 0
