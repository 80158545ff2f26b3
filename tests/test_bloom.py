"""The bloom chain of the output stage (csrc/pt_post.hpp k_bloom_downsample / k_bloom_upsample / bloomTap, the level plan of
csrc/pt_output_host.hpp postprocessImage, their twins in oracle/pt_oracle_post.c) against tests/bloom_ref.py.

Kernel and oracle are the same text twice, so device == oracle says nothing about a mistake made once and copied.  Three things do:

1. Known answers derived by hand from the tap tables in bloom_ref.py's docstring, stated here as integers (DOWN_WEIGHTS,
   UP_WEIGHTS, LEVELS): they pin the reference.  Where every step of a frame is an exact 2:1 and every extent a power of two, all
   of the arithmetic is exact in float32 as well (_exact_case), and the same hand model then pins the oracle and the device
   end to end, without going through the reference at all.
2. reference(float32) == oracle, bit for bit, at every shape of SHAPES: pins the oracle's arithmetic and its level plan.
3. device == oracle, bit for bit, at the same shapes; and device against reference(float64) under test_present.py's rule.

Tolerance against float64.  Both bounds are measured ON THE REFERENCE ALONE, per case, as its float32 instance against its float64
instance on the binary16 image: the maximum difference and the share of values that differ at all.  They are the constants
REF_F32_VS_F64 below, printed by

    python tests/test_bloom.py

and test_reference_float32_against_float64 recomputes them without a GPU.  The device may differ from float64 by 8 x that maximum,
with a floor of one binary16 step (2^-11 max(1, |value|)), on at most 4 x that share of the values."""
import os
import sys

import numpy as np
import pytest

import bloom_ref as B

SAMPLES = 8
THRESHOLD = 0.8
# (BloomIntensity, Exposure).  10 * 0.1f rounds to exactly 1.0f: level 0 of the chain reaches the output unscaled
PARAMS = [(10.0, 1.0), (0.35, 2.5)]
# (H, W), each for an edge
SHAPES = [
    (15, 15),                                         # the largest frame without a chain
    (16, 16), (16, 15), (8, 16), (17, 31),            # the first chain; odd extents halve by flooring
    (31, 33), (32, 9),                                # either side of the third level
    (1, 16), (16, 1),                                 # levels one texel high, both orientations
    (3, 64), (2, 127), (127, 2),                      # one axis sits at 1 (H >> l reaches 0) while the other still halves
    (33, 67), (45, 67),                               # the present tests' frame
    (100, 257),                                       # six levels
    (1, 32768), (32768, 1), (3, 40000), (1, 65536),   # the 12-level cap
]
CASES = [(h, w, bi, ex) for (h, w) in SHAPES for (bi, ex) in PARAMS]
# one shape per line above, for the SDR / sRGB8 run
SHAPE_CLASSES = [(15, 15), (17, 31), (32, 9), (16, 1), (2, 127), (45, 67), (100, 257), (3, 40000)]
# a constant 30000 on four levels: level 1 holds 90000, infinite in binary16.  40 x 72: no tap of the last up step has a weight of
# exactly 0, every value is +infinity; 3 x 64: level 1 is one texel high, its taps read the clamped row with weights 1 and 0, and
# infinity * 0 makes NaN
NON_FINITE = [(40, 72), (3, 64)]

# (H, W, BloomIntensity, Exposure) -> (max |ref(float32) - ref(float64)| on the binary16 image, share of values that differ)
REF_F32_VS_F64 = {
    (15, 15, 10.0, 1.0): (6.250e-02, 1.481e-03),
    (15, 15, 0.35, 2.5): (4.883e-04, 1.481e-03),
    (16, 16, 10.0, 1.0): (0.000e+00, 0.000e+00),
    (16, 16, 0.35, 2.5): (3.906e-03, 7.812e-03),
    (16, 15, 10.0, 1.0): (2.441e-04, 1.389e-03),
    (16, 15, 0.35, 2.5): (6.250e-02, 4.167e-03),
    (8, 16, 10.0, 1.0): (0.000e+00, 0.000e+00),
    (8, 16, 0.35, 2.5): (6.250e-02, 1.042e-02),
    (17, 31, 10.0, 1.0): (7.812e-03, 4.428e-03),
    (17, 31, 0.35, 2.5): (9.766e-04, 3.795e-03),
    (31, 33, 10.0, 1.0): (1.250e-01, 9.449e-03),
    (31, 33, 0.35, 2.5): (6.250e-02, 5.213e-03),
    (32, 9, 10.0, 1.0): (0.000e+00, 0.000e+00),
    (32, 9, 0.35, 2.5): (4.000e+00, 5.787e-03),
    (1, 16, 10.0, 1.0): (0.000e+00, 0.000e+00),
    (1, 16, 0.35, 2.5): (0.000e+00, 0.000e+00),
    (16, 1, 10.0, 1.0): (0.000e+00, 0.000e+00),
    (16, 1, 0.35, 2.5): (0.000e+00, 0.000e+00),
    (3, 64, 10.0, 1.0): (0.000e+00, 0.000e+00),
    (3, 64, 0.35, 2.5): (4.883e-04, 1.736e-03),
    (2, 127, 10.0, 1.0): (0.000e+00, 0.000e+00),
    (2, 127, 0.35, 2.5): (4.883e-04, 2.625e-03),
    (127, 2, 10.0, 1.0): (0.000e+00, 0.000e+00),
    (127, 2, 0.35, 2.5): (9.766e-04, 5.249e-03),
    (33, 67, 10.0, 1.0): (0.000e+00, 0.000e+00),
    (33, 67, 0.35, 2.5): (6.250e-02, 8.141e-03),
    (45, 67, 10.0, 1.0): (3.906e-03, 4.422e-04),
    (45, 67, 0.35, 2.5): (1.953e-03, 6.412e-03),
    (100, 257, 10.0, 1.0): (1.953e-03, 1.038e-04),
    (100, 257, 0.35, 2.5): (6.250e-02, 7.328e-03),
    (1, 32768, 10.0, 1.0): (0.000e+00, 0.000e+00),
    (1, 32768, 0.35, 2.5): (1.953e-03, 5.737e-03),
    (32768, 1, 10.0, 1.0): (0.000e+00, 0.000e+00),
    (32768, 1, 0.35, 2.5): (9.766e-04, 6.073e-03),
    (3, 40000, 10.0, 1.0): (1.250e-01, 4.419e-02),
    (3, 40000, 0.35, 2.5): (6.250e-02, 1.894e-02),
    (1, 65536, 10.0, 1.0): (4.883e-04, 5.086e-06),
    (1, 65536, 0.35, 2.5): (1.953e-03, 5.803e-03),
}

# ---- the hand-derived tables ----------------------------------------------------------------------------------------------------
# down, an exact 2:1 step: a destination centre lies on the corner shared by source texels 2X and 2X + 1, so every tap is the mean
# of a 2 x 2 block and a source texel's weight depends on |offset| of its centre from the destination centre, 0.5 / 1.5 / 2.5 per
# axis (index 0 / 1 / 2).  In 1/512: the block of e (0.125 / 4 = 16) and of the j k l m tap on its side (16) cover (0.5, 0.5): 32;
# (0.5, 1.5): one of j k l m (16) and one of b d f h (0.0625 / 4 = 8): 24; (1.5, 1.5): one of j k l m and one corner tap
# (0.03125 / 4 = 4): 20; (0.5, 2.5): one of b d f h: 8; (1.5, 2.5) and (2.5, 2.5): one corner tap: 4.
DOWN_WEIGHTS = np.array([[32, 24, 8], [24, 20, 4], [8, 4, 4]])  # / 512; over the 6 x 6 footprint they sum to 512
# up, an exact 1:2 step: destination texel 2s + r reads at source coordinate s - 1/4 (r = 0) or s + 1/4 (r = 1); the tent's three
# columns, weights 1 2 1 / 4, sit one source texel apart and each weighs two texels 3/4 : 1/4.  For r = 0 that is texels
# s - 2 .. s + 1 with (1/4, 3/4 + 2/4, 6/4 + 1/4, 3/4) / 4 = (1, 5, 7, 3) / 16; r = 1 is the mirror image.  Read the other way, a
# unit source texel s reaches destination texels 2s - 3 .. 2s + 4 with (1, 3, 5, 7, 7, 5, 3, 1) / 16 per axis.
UP_GATHER = {0: ((-2, 1), (-1, 5), (0, 7), (1, 3)), 1: ((-1, 3), (0, 7), (1, 5), (2, 1))}  # r -> (source texel - s, weight * 16)
UP_WEIGHTS = np.array([1, 3, 5, 7, 7, 5, 3, 1])  # / 16 per axis; the outer product sums to 4 * 256 / 256
# the larger extent -> number of levels that take part: 5 mips are the first with `mips - 3` >= 2; 15 - 3 = 12 reaches the cap unaided
LEVELS = {1: 1, 15: 1, 16: 2, 31: 2, 32: 3, 63: 3, 64: 4, 32767: 12, 32768: 12, 65536: 12}


# =====================================================================================================
# inputs and references: computed once, shared, left unchanged
# =====================================================================================================
def _frame(h, w, samples=SAMPLES):
    """test_output.py's running sum: a ramp with noise, a hot spot that blooms and, where the extent has room, a NaN and an Inf
    marker pixel."""
    rng = np.random.default_rng(h * 7 + w)
    img = np.zeros((h, w, 4), np.float32)
    yy, xx = np.mgrid[0:h, 0:w]
    img[..., 0] = 0.2 + 0.6 * xx / w
    img[..., 1] = 0.1 + 0.5 * yy / h
    img[..., 2] = 0.3
    img[h // 3:h // 3 + 6, w // 2:w // 2 + 6, :3] = 40.0
    img[..., :3] += rng.uniform(0, 0.02, (h, w, 3))
    if h > 4 and w > 5:
        img[2, 3, 0] = np.nan   # -> (5000, 0, 0) marker, postprocess.comp:24-25
        img[4, 5, 1] = np.inf   # -> (0, 5000, 0) marker, :26-27
    img[..., :3] *= samples
    img[..., 3] = 1.0
    return img


_cache = {}


def _once(key, make):
    if key not in _cache:
        v = make()
        for a in (v if isinstance(v, tuple) else (v,)):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _cache[key] = v
    return _cache[key]


def _acc(h, w):
    return _once(("acc", h, w), lambda: _frame(h, w))


def _ref(case, dtype):
    h, w, bi, ex = case
    return _once(("ref", case, np.dtype(dtype).name), lambda: B.composed(_acc(h, w), SAMPLES, ex, THRESHOLD, bi, dtype))


def _oracle(orc, case, tone=1):
    h, w, bi, ex = case
    return _once(("orc", case, tone), lambda: orc.postprocess(_acc(h, w), SAMPLES, exposure=ex, bloom_threshold=THRESHOLD, bloom_intensity=bi, tone_mapping=tone))


def _non_finite_acc(shape):
    def make():
        acc = np.full(shape + (4,), 30000.0 * SAMPLES, np.float32)
        acc[..., 3] = 1.0
        return acc
    return _once(("non finite", shape), make)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(a, b):
    """The same bits, or NaN on both sides."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return (_bits(a) == _bits(b)) | (np.isnan(a) & np.isnan(b))


def _differs(a, b):
    """Values that are not the same number (two NaNs count as the same)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return ~((a == b) | (np.isnan(a) & np.isnan(b)))


def _measure(case):
    a, b = _ref(case, np.float32), _ref(case, np.float64)
    with np.errstate(all="ignore"):
        d = np.abs(a.astype(np.float64) - b)
    return float(np.max(np.where(np.isfinite(d), d, 0.0))), float(_differs(a, b).mean())


# ---- the hand model: exact 2:1 steps, by the integer tables above ---------------------------------------------------------------
def _f16(x):
    return np.asarray(x, np.float64).astype(np.float16).astype(np.float64)


def _model_down(src):
    sh, sw = src.shape[:2]
    assert sh % 2 == 0 and sw % 2 == 0
    dst = np.zeros((sh // 2, sw // 2) + src.shape[2:])
    for Y in range(sh // 2):
        for X in range(sw // 2):
            for dy in range(-2, 4):      # source row 2Y + dy, its centre dy - 0.5 below the destination centre
                for dx in range(-2, 4):
                    wgt = DOWN_WEIGHTS[int(abs(dy - 0.5)), int(abs(dx - 0.5))] / 512.0
                    dst[Y, X] += wgt * src[min(max(2 * Y + dy, 0), sh - 1), min(max(2 * X + dx, 0), sw - 1)]  # clamp to edge
    return _f16(dst)


def _model_up(src, dst):
    sh, sw = src.shape[:2]
    assert dst.shape[0] == 2 * sh and dst.shape[1] == 2 * sw
    out = np.array(dst, np.float64)
    for y in range(2 * sh):
        for x in range(2 * sw):
            for oy, wy in UP_GATHER[y % 2]:
                for ox, wx in UP_GATHER[x % 2]:
                    out[y, x] += (wy * wx / 256.0) * src[min(max(y // 2 + oy, 0), sh - 1), min(max(x // 2 + ox, 0), sw - 1)]
    return _f16(out)


def _exact_case(h, w):
    """A frame on which the whole output stage is exact in float32, and its composed colour by the hand model.

    BloomThreshold 0, Exposure 1, TotalSamples 1, BloomIntensity 10.  Every pixel is zero or has a power of two >= 8 as its
    largest channel: the prefilter's factor is br * (1 / br) = 1 (zero pixels: anything times 0), so bloom colour = colour.  All
    values are multiples of 8 up to 256: level 1 holds multiples of 1/64 up to 256 (14 bits), an up tap multiples of 2^-10
    (18 bits), the tent's sum stays below 2^12 (22 bits) and level 0 + tent / 16 below 2^9 in multiples of 2^-14 (23 bits).
    Nothing rounds but the binary16 stores, which the model makes in the same places."""
    assert (h, w) in ((16, 16), (16, 8), (8, 16), (16, 4), (2, 16)) and len(B.levels_used(w, h)) == 2
    rng = np.random.default_rng(h * 100 + w)
    top = 2.0 ** rng.integers(3, 9, (h, w))
    colour = np.stack([top, 8.0 * rng.integers(0, 33, (h, w)), 8.0 * rng.integers(0, 33, (h, w))], axis=-1)
    colour = np.minimum(colour, top[..., None])
    colour = np.take_along_axis(colour, rng.permuted(np.tile(np.arange(3), (h, w, 1)), axis=-1), axis=-1)  # the largest channel moves about
    colour[rng.uniform(size=(h, w)) < 0.3] = 0.0
    colour[h // 2, w // 2] = (256.0, 0.0, 8.0)
    acc = np.ones((h, w, 4), np.float32)
    acc[..., :3] = colour
    level0 = _model_up(_model_down(colour), colour)
    want = _f16(level0 * 1.0 + colour)
    return acc, want.astype(np.float32)


EXACT_FRAMES = [(16, 16), (16, 8), (8, 16), (16, 4), (2, 16)]
EXACT_POST = dict(exposure=1.0, bloom_threshold=0.0, bloom_intensity=10.0)


def _exact(h, w):
    return _once(("exact", h, w), lambda: _exact_case(h, w))


def _constant_case(h, w):
    """A constant colour whose prefilter factor is 1 (largest channel 2, threshold 0): every filter weight sums to 1 and clamp to
    edge keeps a constant constant, so each up step adds one more copy and level 0 ends as n c; composed with BloomIntensity 10
    that is (n + 1) c, exact in binary16."""
    c = np.float32([0.5, 2.0, 1.25])
    acc = np.ones((h, w, 4), np.float32)
    acc[..., :3] = c * np.float32(SAMPLES)
    n = len(B.levels_used(w, h))
    return acc, np.broadcast_to(c * np.float32(n + 1), (h, w, 3)), n


CONSTANT_FRAMES = [(15, 15), (16, 15), (32, 9), (16, 1), (3, 64), (127, 2), (100, 257), (1, 32768), (3, 40000)]

# An extent of 3 halves to 1 (floor), not to 2, and the hand model above cannot say so: it needs even extents.  This can: light on
# line 0 only, of a frame three lines thick and two levels deep.  Level 1 is one texel thick, so whatever the up step reads from
# it is that one line, with weights that sum to 1: lines 1 and 2, black before, come out alike.  (Alike, not equal: a (1 - t) + a t
# is a to within an ulp of the dtype, and the binary16 store may round the two lines apart by one step.)  A level 1 two thick
# would leave line 2 with a fraction of line 1's light.
THIN_FRAMES = [(3, 16), (16, 3)]


def _thin_case(h, w):
    def make():
        acc = np.zeros((h, w, 4), np.float32)
        acc[..., 3] = 1.0
        line = 8.0 * np.random.default_rng(h).integers(1, 33, (16, 3))
        if h == 3:
            acc[0, :, :3] = line
        else:
            acc[:, 0, :3] = line
        return acc
    return _once(("thin", h, w), make)


def _check_thin(out, h, w):
    lines = np.asarray(out, np.float64)[..., :3]
    lines = lines if h == 3 else lines.transpose(1, 0, 2)
    assert lines.shape == (3, 16, 3) and (lines[1] >= 0.5).all() and (lines[0] > lines[1]).all()  # the bloom of line 0 is there
    step = 2.0 ** -10 * np.maximum(lines[1], lines[2])  # no less than the spacing of binary16 at the larger value
    assert (np.abs(lines[1] - lines[2]) <= step).all(), float(np.abs(lines[1] - lines[2]).max())


# =====================================================================================================
# without a GPU: known answers
# =====================================================================================================
def test_levels_used_table():
    for m, n in LEVELS.items():
        for other in (1, 3, m):
            if other > m:
                continue
            lv = B.levels_used(m, other)
            assert len(lv) == n and len(B.levels_used(other, m)) == n, (m, other)
            assert lv == [(max(1, other >> l), max(1, m >> l)) for l in range(n)]  # (h, w): floors, and 1 once the shift reaches 0
            assert B.levels_used(other, m) == [(hh, ww) for (ww, hh) in lv]
    assert B.levels_used(257, 100) == [(100, 257), (50, 128), (25, 64), (12, 32), (6, 16), (3, 8)]
    assert B.levels_used(64, 3) == [(3, 64), (1, 32), (1, 16), (1, 8)]
    assert B.levels_used(31, 17) == [(17, 31), (8, 15)]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_tap_is_the_linear_filter_with_clamp_to_edge(dtype):
    img = np.arange(12, dtype=dtype).reshape(3, 4, 1)  # value = 4 y + x
    t = lambda u, v: B.tap(img, dtype(u), dtype(v), dtype)[0, 0, 0]  # noqa: E731
    assert t(0.375, 0.5) == 5.0                  # u * 4 - 0.5 = 1, v * 3 - 0.5 = 1: texel (1, 1) alone
    assert t(0.5, 0.5) == 5.5                    # half way to texel x = 2
    assert t(0.4375, 0.5) == 5.25                # a quarter of the way: weights 3/4 and 1/4, the larger on the nearer texel
    assert t(0.375, 0.75) == 5.0 + 0.75 * 4.0    # y = 1.75: three quarters of the way down to row 2
    assert t(0.0, 0.0) == 0.0 and t(1.0, 1.0) == 11.0 and t(-3.0, 0.5) == 4.0 and t(0.375, 9.0) == 9.0  # the edge texel, not a wrap
    grid = B.tap(img, np.array([0.125, 0.375, 0.625, 0.875], dtype), np.array([1 / 6, 0.5, 5 / 6], dtype), dtype)
    assert grid.shape == (3, 4, 1) and np.abs(grid - img).max() <= (1e-5 if dtype == np.float32 else 1e-14)  # u along x, v along y


def test_down_step_gather_weights():
    """One 2:1 step, interior destination texel: the 6 x 6 weights over 512, one impulse of 512 per channel."""
    assert DOWN_WEIGHTS[[0, 1, 2, 2, 1, 0]][:, [0, 1, 2, 2, 1, 0]].sum() == 512 and (DOWN_WEIGHTS == DOWN_WEIGHTS.T).all()
    sh, sw, Y, X = 12, 20, 2, 5  # non-square, 1 / 12 and 1 / 20 are not exact: the binary16 store absorbs it
    src = np.zeros((sh, sw, 36))
    want = np.zeros((6, 6))
    for dy in range(-2, 4):
        for dx in range(-2, 4):
            src[2 * Y + dy, 2 * X + dx, (dy + 2) * 6 + dx + 2] = 512.0
            want[dy + 2, dx + 2] = DOWN_WEIGHTS[int(abs(dy - 0.5)), int(abs(dx - 0.5))]
    assert (want == want[::-1]).all() and (want == want[:, ::-1]).all() and want[2, 2] == 32 and want[2, 1] == 24 and want[0, 0] == 4
    for dtype in (np.float64, np.float32):
        got = B.down(src, (sh // 2, sw // 2), dtype)
        assert got.shape == (6, 10, 36)
        assert (got[Y, X].reshape(6, 6) == want).all(), dtype
        assert got[Y, X].sum() == 512
    # ... and the hand model used further down says the same, edges included, on a dense image
    rng = np.random.default_rng(3)
    img = 8.0 * rng.integers(0, 33, (8, 16, 3))
    assert (B.down(img, (4, 8), np.float64) == _model_down(img)).all()


def test_up_step_scatter_weights():
    """One 1:2 step, interior: a unit source texel reaches 8 x 8 destination texels with (1 3 5 7 7 5 3 1) (x) (1 3 5 7 7 5 3 1) / 256."""
    sh, sw, s, t = 6, 10, 3, 4
    src = np.zeros((sh, sw, 1))
    src[s, t] = 256.0
    want = np.zeros((2 * sh, 2 * sw, 1))
    want[2 * s - 3:2 * s + 5, 2 * t - 3:2 * t + 5, 0] = np.outer(UP_WEIGHTS, UP_WEIGHTS)
    assert want.sum() == 4 * 256
    for dtype in (np.float64, np.float32):
        assert (B.up(src, np.zeros_like(want), dtype) == want).all(), dtype
        assert (B.up(src, np.full_like(want, 3.0), dtype) == want + 3.0).all()  # added onto the existing level
    for r, taps in UP_GATHER.items():  # the gather form of the same table
        for off, wgt in taps:
            assert UP_WEIGHTS[r - 2 * off + 3] == wgt
    rng = np.random.default_rng(4)
    small, big = rng.integers(0, 257, (4, 8, 3)) / 64.0, 8.0 * rng.integers(0, 33, (8, 16, 3))
    assert (B.up(small, big, np.float64) == _model_up(small, big)).all()


@pytest.mark.parametrize("shape", CONSTANT_FRAMES, ids=lambda s: "%dx%d" % s)
def test_constant_colour_gains_one_copy_per_level(orc, shape):
    h, w = shape
    acc, want, n = _constant_case(h, w)
    c = want[0, 0] / np.float32(n + 1)
    for dtype in (np.float64, np.float32):
        post, bloom0 = B.prefilter(acc, SAMPLES, 1.0, 0.0, dtype)
        assert (post == c).all() and (bloom0 == c).all()
        assert (B.chain(bloom0, dtype) == c * dtype(n)).all(), (shape, dtype)
        assert (B.composed(acc, SAMPLES, 1.0, 0.0, 10.0, dtype) == want).all()
    got = orc.postprocess(acc, SAMPLES, exposure=1.0, bloom_threshold=0.0, bloom_intensity=10.0, tone_mapping=1)
    assert (got[..., :3] == want).all() and (got[..., 3] == 1).all()


@pytest.mark.parametrize("shape", EXACT_FRAMES, ids=lambda s: "%dx%d" % s)
def test_exact_frames_match_the_hand_model(orc, shape):
    """Where nothing rounds but the binary16 stores, reference (either dtype) and oracle must give the hand model's bits."""
    acc, want = _exact(*shape)
    assert len(np.unique(want)) > 20
    for dtype in (np.float64, np.float32):
        got = B.composed(acc, 1, EXACT_POST["exposure"], EXACT_POST["bloom_threshold"], EXACT_POST["bloom_intensity"], dtype)
        assert (got == want).all(), (shape, dtype, float(np.abs(got - want).max()))
    got = orc.postprocess(acc, 1, tone_mapping=1, **EXACT_POST)[..., :3]
    assert (_bits(got) == _bits(want)).all(), (shape, float(np.abs(got - want).max()))


@pytest.mark.parametrize("shape", THIN_FRAMES, ids=lambda s: "%dx%d" % s)
def test_an_extent_of_three_halves_to_one(orc, shape):
    h, w = shape
    acc = _thin_case(h, w)
    assert B.levels_used(w, h) == [(h, w), (max(1, h >> 1), max(1, w >> 1))] and 1 in B.levels_used(w, h)[1]
    for dtype in (np.float64, np.float32):
        _check_thin(B.composed(acc, 1, EXACT_POST["exposure"], EXACT_POST["bloom_threshold"], EXACT_POST["bloom_intensity"], dtype), h, w)
    _check_thin(orc.postprocess(acc, 1, tone_mapping=1, **EXACT_POST), h, w)


def test_reference_is_symmetric():
    """float64, 33 x 67: mirrored in x, mirrored in y and transposed frames give the mirrored and transposed image, to the bit on
    the binary16 image: what an x / y mix-up on a non-square level would break."""
    acc = _acc(33, 67)
    for bi, ex in PARAMS:
        base = _ref((33, 67, bi, ex), np.float64)
        assert np.isfinite(base).all() and len(B.levels_used(67, 33)) == 4
        for name, there, back in (("mirror x", lambda a: a[:, ::-1], lambda a: a[:, ::-1]), ("mirror y", lambda a: a[::-1], lambda a: a[::-1]),
                                  ("transpose", lambda a: a.transpose(1, 0, 2), lambda a: a.transpose(1, 0, 2))):
            got = back(B.composed(np.ascontiguousarray(there(acc)), SAMPLES, ex, THRESHOLD, bi, np.float64))
            assert got.shape == base.shape and float(np.abs(got - base).max()) == 0.0, (name, bi)


def test_prefilter_markers_and_knee():
    acc = np.zeros((1, 6, 4), np.float32)
    acc[0, :, :3] = [[np.nan, 1, 1], [1, np.inf, 1], [-np.inf, np.nan, 1], [0.25, 0.125, 0], [0.75, 0.25, 0.5], [4, 2, 1]]
    for dtype in (np.float64, np.float32):
        post, bloom = B.prefilter(acc, 1, 1.0, 1.0, dtype)
        assert (post[0, 0] == [5000, 0, 0]).all() and (post[0, 1] == [0, 5000, 0]).all()
        assert (post[0, 2] == [5000, 0, 0]).all()               # NaN is tested first and its marker is finite
        assert (bloom[0, 3] == 0).all()                         # below threshold - knee
        assert (bloom[0, 4] == _f16(np.float64([0.75, 0.25, 0.5]) / 24.0)).all()  # inside the knee: colour * 0.5 (br - 0.5)^2 / br = colour / 24
        assert (bloom[0, 5] == post[0, 5] * 0.75).all()         # above it: (br - threshold) / br
        assert np.abs(bloom[0, 0] - np.float64([4999, 0, 0])).max() <= 4.0  # one binary16 step at 5000


# =====================================================================================================
# without a GPU: the reference against the oracle, float32 against float64
# =====================================================================================================
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_reference_float32_is_the_oracle(orc, shape):
    h, w = shape
    for bi, ex in PARAMS:
        case = (h, w, bi, ex)
        ref, got = _ref(case, np.float32), _oracle(orc, case)
        assert ref.dtype == np.float32 and got.shape == (h, w, 4) and (got[..., 3] == 1).all()
        same = _same(ref, got[..., :3])
        assert same.all(), (case, int((~same).sum()))
        if h > 4 and w > 5:
            assert got[2, 3, 0] >= 4096 and got[4, 5, 1] >= 4096  # the marker pixels are in
        if bi == 10.0 and len(B.levels_used(w, h)) > 1:
            off = orc.postprocess(_acc(h, w), SAMPLES, exposure=ex, bloom_threshold=THRESHOLD, bloom_intensity=0.0, tone_mapping=1)
            assert (got[..., :3] > off[..., :3]).mean() > 0.5  # and so is the bloom


def test_reference_float32_against_float64():
    """The measured figures behind every tolerance, recomputed: within a factor of 1.5 of the constants."""
    assert set(REF_F32_VS_F64) == set(CASES)
    for case in CASES:
        got, want = _measure(case), REF_F32_VS_F64[case]
        print(case, "max %.3e share %.3e" % got)
        for g, w in zip(got, want):
            assert w / 1.5 <= g <= w * 1.5 if w else g == 0.0, (case, got, want)
        assert np.isfinite(_ref(case, np.float64)).all()


@pytest.mark.parametrize("shape", NON_FINITE, ids=lambda s: "%dx%d" % s)
def test_non_finite_leg_reference_and_oracle_agree(orc, shape):
    h, w = shape
    assert len(B.levels_used(w, h)) == 4
    acc = _non_finite_acc(shape)
    for bi, ex in PARAMS:
        ref = B.composed(acc, SAMPLES, ex, THRESHOLD, bi, np.float32)
        got = orc.postprocess(acc, SAMPLES, exposure=ex, bloom_threshold=THRESHOLD, bloom_intensity=bi, tone_mapping=1)[..., :3]
        assert (np.isnan(ref) == np.isnan(got)).all() and _same(ref, got).all()
        assert not np.isfinite(got).any() and np.isnan(got).any() == (h == 3)


# =====================================================================================================
# on the GPU
# =====================================================================================================
def _run(pkg, acc, samples, tone, fmt=None, r=None, **post):
    """resize + write_accumulation + postprocess + read_output on `r`, or on a fresh handle that is closed again."""
    import torch  # noqa: F401  (first, so the HIP library shares torch's HIP runtime)

    own = r is None
    if own:
        r = pkg.Renderer()
    r.resize(acc.shape[1], acc.shape[0])
    r.write_accumulation(acc)
    r.postprocess(samples, tone_mapping=tone, **post)
    out = r.read_output(pkg.OUTPUT_RGBA32F if fmt is None else fmt)
    if own:
        r.close()
    return out


def _post(case):
    return dict(exposure=case[3], bloom_threshold=THRESHOLD, bloom_intensity=case[2])


def _device(pkg, case):
    return _once(("device", case), lambda: _run(pkg, _acc(case[0], case[1]), SAMPLES, pkg.TONE_MAPPING_HDR, **_post(case)))


_case_id = lambda c: "%dx%d-%g-%g" % c  # noqa: E731


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_device_is_the_oracle(pkg, orc, case):
    got, ref = _device(pkg, case), _oracle(orc, case)
    same = _same(got, ref)
    assert got.shape == ref.shape and same.all(), (case, int((~same).sum()))


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_device_against_float64_reference(pkg, case):
    got = _device(pkg, case).astype(np.float64)
    ref = _ref(case, np.float64)
    worst, share = REF_F32_VS_F64[case]
    assert got.shape == ref.shape[:2] + (4,) and (got[..., 3] == 1).all()
    got = got[..., :3]
    with np.errstate(all="ignore"):
        d = np.abs(got - ref)
    tol = np.maximum(8.0 * worst, 2.0 ** -11 * np.maximum(1.0, np.abs(ref)))
    differing = float(_differs(got, ref).mean())
    print(case, "max |device - ref64| %.3e (measured on the reference %.3e), differing %.3e (%.3e)" % (float(np.nanmax(d)), worst, differing, share))
    assert np.isfinite(got).all() and (d <= tol).all(), (case, float(d.max()))
    assert differing <= 4.0 * share, (case, differing, share)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPE_CLASSES, ids=lambda s: "%dx%d" % s)
def test_device_sdr_and_srgb8_are_the_oracle_s(pkg, orc, shape):
    import torch  # noqa: F401

    case = shape + PARAMS[1]
    ref = _oracle(orc, case, tone=0)
    r = pkg.Renderer()
    lin = _run(pkg, _acc(*shape), SAMPLES, pkg.TONE_MAPPING_SDR, r=r, **_post(case))
    srgb = r.read_output(pkg.OUTPUT_RGBA8_SRGB)
    r.close()
    assert (_bits(lin) == _bits(ref)).all() and np.isfinite(ref).all()
    assert (srgb == orc.encode_output(ref, 0)).all()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", EXACT_FRAMES + CONSTANT_FRAMES + THIN_FRAMES, ids=lambda s: "%dx%d" % s)
def test_device_known_answers(pkg, shape):
    """The hand model, the constant colour and the thin frames, end to end on the device: no reference, no oracle."""
    if shape in THIN_FRAMES:
        return _check_thin(_run(pkg, _thin_case(*shape), 1, pkg.TONE_MAPPING_HDR, **EXACT_POST), *shape)
    if shape in EXACT_FRAMES:
        acc, want = _exact(*shape)
        got = _run(pkg, acc, 1, pkg.TONE_MAPPING_HDR, **EXACT_POST)
    else:
        acc, want, _ = _constant_case(*shape)
        got = _run(pkg, acc, SAMPLES, pkg.TONE_MAPPING_HDR, exposure=1.0, bloom_threshold=0.0, bloom_intensity=10.0)
    assert (_bits(got[..., :3]) == _bits(want)).all() and (got[..., 3] == 1).all(), shape


@pytest.mark.gpu
def test_one_handle_across_level_plans_leaves_nothing_stale(pkg, orc):
    """bloomRgb is reused across sizes and k_bloom_upsample is read-modify-write: a level left over from another plan would show."""
    import torch  # noqa: F401

    r = pkg.Renderer()
    for shape in ((100, 257), (16, 16), (15, 15), (3, 64), (100, 257)):
        for bi, ex in PARAMS:
            case = shape + (bi, ex)
            got = _run(pkg, _acc(*shape), SAMPLES, pkg.TONE_MAPPING_HDR, r=r, **_post(case))
            assert (_bits(got) == _bits(_device(pkg, case))).all(), case  # a fresh handle's
            assert (_bits(got) == _bits(_oracle(orc, case))).all(), case
    r.close()


@pytest.mark.gpu
def test_postprocess_twice_gives_the_same_bits(pkg):
    import torch  # noqa: F401

    r = pkg.Renderer()
    for shape in ((45, 67), (3, 64)):
        case = shape + PARAMS[1]
        first = _run(pkg, _acc(*shape), SAMPLES, pkg.TONE_MAPPING_HDR, r=r, **_post(case))
        r.postprocess(SAMPLES, tone_mapping=pkg.TONE_MAPPING_HDR, **_post(case))
        second = r.read_output(pkg.OUTPUT_RGBA32F)
        r.postprocess(SAMPLES, tone_mapping=pkg.TONE_MAPPING_HDR, **_post(case))
        third = r.read_output(pkg.OUTPUT_RGBA32F)
        assert (_bits(first) == _bits(second)).all() and (_bits(first) == _bits(third)).all() and (_bits(first) == _bits(_device(pkg, case))).all()
    r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", NON_FINITE, ids=lambda s: "%dx%d" % s)
def test_non_finite_leg_device_is_the_oracle(pkg, orc, shape):
    acc = _non_finite_acc(shape)
    for bi, ex in PARAMS:
        post = dict(exposure=ex, bloom_threshold=THRESHOLD, bloom_intensity=bi)
        got = _run(pkg, acc, SAMPLES, pkg.TONE_MAPPING_HDR, **post)
        ref = orc.postprocess(acc, SAMPLES, tone_mapping=1, **post)
        assert (np.isnan(got) == np.isnan(ref)).all() and _same(got, ref).all()
        assert not np.isfinite(got[..., :3]).any() and np.isnan(got).any() == (shape[0] == 3)


@pytest.mark.gpu
def test_denoised_entry_runs_the_same_chain(pkg, orc):
    """ptx_postprocess_denoised on a denoised image that was read back: the oracle's output stage of that image with TotalSamples
    1; ptx_present at the frame's size then re-reads level 0 of the chain and must give read_output's image."""
    import test_denoise as TD

    r, _, S = TD._filter_state(pkg, "67x45", "synthetic")
    r.denoise(TD.SAMPLES, 3, 1.5, TD.SIGMA_NORMAL, TD.SIGMA_POSITION)
    D = r.read_denoised()
    assert len(B.levels_used(TD.W, TD.H)) == 4
    for bi, ex in PARAMS:
        post = dict(exposure=ex, bloom_threshold=THRESHOLD, bloom_intensity=bi)
        r.postprocess_denoised(7, tone_mapping=pkg.TONE_MAPPING_HDR, **post)  # the uniform's TotalSamples is ignored: the image is a mean
        got = r.read_output(pkg.OUTPUT_RGBA32F)
        ref = orc.postprocess(D, 1, tone_mapping=1, **post)
        assert _same(got, ref).all(), (bi, ex)
        assert _same(got[..., :3], B.composed(D, 1, ex, THRESHOLD, bi, np.float32)).all()
        # the screen path composes again from level 0 and tone-maps itself: at the frame's size, SDR, it is the SDR output image
        r.postprocess_denoised(7, tone_mapping=pkg.TONE_MAPPING_SDR, **post)
        sdr = r.read_output(pkg.OUTPUT_RGBA32F)
        assert (_bits(sdr) == _bits(orc.postprocess(D, 1, tone_mapping=0, **post))).all(), (bi, ex)
        r.present(TD.W, TD.H, pkg.PRESENT_R16G16B16A16_SFLOAT, pkg.TONE_MAPPING_SDR)
        screen = r.read_present()
        assert screen.dtype == np.float16 and (np.ascontiguousarray(screen).view(np.uint16) == sdr.astype(np.float16).view(np.uint16)).all()
    assert (_bits(r.readback()) == _bits(S)).all()


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    print("REF_F32_VS_F64 = {")
    for case in CASES:
        print("    %r: (%.3e, %.3e)," % ((case,) + _measure(case)))
    print("}")
