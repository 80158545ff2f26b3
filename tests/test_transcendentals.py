"""The fixed transcendental kernels (sincos_, pow_ / log2_ / exp2_, atan2_ / asin_, exp_, f16Round) on the inputs the renderer
can pass them -- exhaustively where the production domain is small enough (rnd() returns only the 2^23 values k / 2^23; every
input of the tone-map and sRGB-encode kernels is a binary16 value), densely around every branch edge elsewhere.

Every group is two tests: a CPU test that holds the oracle (oracle/pt_oracle_math.h, the definition) against float64 numpy, and a
gpu test in which the device returns the oracle's bits on the same inputs.  Device == oracle bit for bit, so the accuracy
figures shown on the CPU hold for the device.  The measured figures are in profiles/transcendental_domains.txt; a constant that
the text calls "measured" is the maximum over the deterministic sets below, rounded up to two digits."""
import time

import numpy as np
import pytest

import util

CHUNK = 1 << 22  # rows per test_eval call
LATTICE = 1 << 23  # rnd() returns k / 2^23
PT_PI = np.float32(3.14159265359)  # common.glsl:3
F32_MIN_NORMAL = 2.0 ** -126
F32_ROUNDS_TO_INF = (2.0 - 2.0 ** -24) * 2.0 ** 127  # the midpoint above FLT_MAX
PINF = np.uint32(0x7f800000)

# measured on the oracle over the sets A, B and C of section 1 (the sets are deterministic and the oracle is the definition)
SIN_MAX_ABS_ERR = 7.0e-8
COS_MAX_ABS_ERR = 7.8e-8
UNIT_CIRCLE_EXCESS = 1.5e-7  # s^2 + c^2 - 1 in float64; measured 1.36e-7
# double-precision kernels rounded once to binary32: half a unit plus the kernels' own error in double
ONE_ROUNDING_ULP = 0.51
# the samplers on the RNG lattice: z = sqrt(1 - x^2 - y^2) is NaN on the disk's rim where sin^2 + cos^2 comes out above 1
HEMISPHERE_NANS = {"(0, lat)": 3585487, "(lat, 0)": 2035786, "(lat, lat)": 1}


def _f32(bits):
    return np.asarray(bits, np.uint32).view(np.float32)


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _floats_between(lo, hi):
    """Every binary32 value of [lo, hi], 0 < lo <= hi."""
    lo, hi = np.float32(lo), np.float32(hi)
    return np.arange(int(lo.view(np.uint32)), int(hi.view(np.uint32)) + 1, dtype=np.uint32).view(np.float32)


def _rows(*columns):
    n = max(np.size(c) for c in columns)
    return np.stack([np.broadcast_to(np.asarray(c, np.float32), (n,)) for c in columns], axis=1).view(np.uint32)


def _oracle(pkg, orc, name, rows):
    """The oracle on `rows` (uint32 words), CHUNK rows a call: the float32 view of its outputs."""
    fn = pkg.FN[name]
    nout = orc.OUT_STRIDE[fn]
    out = np.empty((len(rows), nout), np.uint32)
    for lo in range(0, len(rows), CHUNK):
        out[lo:lo + CHUNK] = orc.test_eval(fn, rows[lo:lo + CHUNK], nout)
    return out.view(np.float32)


def _device_differs(pkg, orc, gpu, name, rows):
    """How many output words of the device differ from the oracle's on `rows` (two NaNs count as equal)."""
    fn = pkg.FN[name]
    nout = orc.OUT_STRIDE[fn]
    bad = 0
    for lo in range(0, len(rows), CHUNK):
        got = gpu.test_eval(fn, rows[lo:lo + CHUNK])
        bad += int((~util.bits_equal_or_both_nan(got, orc.test_eval(fn, rows[lo:lo + CHUNK], nout))).sum())
    return bad


def _report(label, t0, rows, bad):
    print(f"{label}: {rows} rows, {time.perf_counter() - t0:.2f} s, {bad} differing")


# ---------------------------------------------------------------------------------------
# the definitions of oracle/pt_oracle_math.h restated in numpy, operation by operation: +, -, *, /, sqrt, floor and the
# conversions are IEEE operations in C and in numpy alike, so the restatement returns the oracle's bits or one of the two is wrong.
# The float64 bounds below cannot see an error far below half a unit (a series cut one term short, a reduction left out);
# the bits can.
# ---------------------------------------------------------------------------------------
def _horner(z, coefficients):
    p = np.full_like(z, coefficients[0])
    for c in coefficients[1:]:
        p = p * z + c
    return p


def _sincos_spec(x):
    f = np.float32
    fk = np.floor(x * f(0.636619772) + f(0.5))
    q = fk.astype(np.int32) & 3
    r = x - fk * f(1.5703125)
    r = r - fk * f(4.837512969970703125e-4)
    r = r - fk * f(7.54978995489188216e-8)
    z = r * r
    ps = ((f(-1.9515295891e-4) * z + f(8.3321608736e-3)) * z - f(1.6666654611e-1)) * z * r + r
    pc = ((f(2.443315711809948e-5) * z - f(1.388731625493765e-3)) * z + f(4.166664568298827e-2)) * z * z
    pc = pc - f(0.5) * z
    pc = pc + f(1.0)
    return np.stack([np.choose(q, [ps, pc, -ps, -pc]), np.choose(q, [pc, -ps, -pc, ps])], axis=1)


def _log2_spec(x):
    """pto_log2 of positive, finite, normal float64."""
    bits = x.view(np.uint64)
    e = ((bits >> np.uint64(52)) & np.uint64(0x7ff)).astype(np.int64) - 1023
    m = ((bits & np.uint64(0x000fffffffffffff)) | np.uint64(0x3ff0000000000000)).view(np.float64)
    fold = m > 1.4142135623730951
    m, e = np.where(fold, m * 0.5, m), np.where(fold, e + 1, e)
    f = m - 1.0
    s = f / (2.0 + f)
    ln = 2.0 * s * _horner(s * s, [1.0 / k for k in range(21, 0, -2)])
    return e.astype(np.float64) + ln * 1.4426950408889634


def _exp2_spec(t):
    """pto_exp2 of |t| <= 300."""
    k = np.floor(t + 0.5)
    r = (t - k) * 0.6931471805599453
    fact = [6227020800.0, 479001600.0, 39916800.0, 3628800.0, 362880.0, 40320.0, 5040.0, 720.0, 120.0, 24.0, 6.0]
    p = _horner(r, [1.0 / d for d in fact] + [0.5, 1.0, 1.0])
    return p * np.ldexp(1.0, k.astype(np.int64))


def _pow_spec(x, y):
    """pto_powf past its special cases: positive finite x other than 1, y neither 0 nor NaN."""
    with np.errstate(all="ignore"):
        t = y.astype(np.float64) * _log2_spec(x.astype(np.float64))
        return _exp2_spec(np.minimum(np.maximum(t, -300.0), 300.0)).astype(np.float32)


def _atan_reduced(lo, hi):
    a = lo / hi
    reduce = a > 0.4142135623730951
    t = np.where(reduce, (a - 1.0) / (a + 1.0), a)
    r = t * _horner(t * t, [(-1.0 if k % 4 == 3 else 1.0) / k for k in range(23, 0, -2)])
    return np.where(reduce, 0.7853981633974483 + r, r)


def _atan2_spec(yf, xf):
    with np.errstate(all="ignore"):
        y, x = yf.astype(np.float64), xf.astype(np.float64)
        ax, ay = np.where(x < 0, -x, x), np.where(y < 0, -y, y)
        hi, lo = np.where(ax < ay, ay, ax), np.where(ax < ay, ax, ay)
        r = _atan_reduced(lo, hi)
        r = np.where(ay > ax, 1.5707963267948966 - r, r)
        r = np.where(x < 0, 3.141592653589793 - r, r)
        r = np.where(y < 0, -r, r)
        return np.where(hi == 0, np.float32(0.0), r.astype(np.float32))


def _asin_spec(xf):
    with np.errstate(all="ignore"):
        x = xf.astype(np.float64)
        x = np.where(x > 1, 1.0, x)
        x = np.where(x < -1, -1.0, x)
        ax, ay = np.sqrt((1.0 - x) * (1.0 + x)), np.where(x < 0, -x, x)
        hi, lo = np.where(ax < ay, ay, ax), np.where(ax < ay, ax, ay)
        r = _atan_reduced(lo, hi)
        r = np.where(ay > ax, 1.5707963267948966 - r, r)
        r = np.where(x < 0, -r, r)
        return np.where(hi > 0, r.astype(np.float32), np.where(np.isnan(xf), xf, np.float32(0.0)))


def _same_bits(a, b):
    return util.bits_equal_or_both_nan(_bits(a), _bits(b))


# ---------------------------------------------------------------------------------------
# 1. sincos_ on its whole caller domain
# ---------------------------------------------------------------------------------------
def _sincos_sets():
    k = np.arange(LATTICE, dtype=np.float32)
    a = (np.float32(2.0) * PT_PI) * (k * np.float32(2.0 ** -23))  # SampleGGX: phi = 2.0 * PI * u.y, u.y = rnd()
    b = np.concatenate([_floats_between(0.5, 3 * np.pi / 4 + 1e-3), -_floats_between(0.5, np.pi / 4 + 1e-3)])
    rng = np.random.default_rng(101)
    mant = np.concatenate([np.uint32([0, 1, 0x7fffff, 0x400000]), rng.integers(0, 1 << 23, 4092, dtype=np.uint32)])
    c = np.concatenate([np.uint32(e << 23) | mant for e in range(126)])  # every exponent below 0.5; exponent 0: denormals
    c = _f32(np.concatenate([c, c | np.uint32(0x80000000), np.uint32([0, 0x80000000])]))
    return {"A": a, "B": b, "C": c}


def test_sincos_against_float64(pkg, orc):
    """sincos_ where its callers use it: A, every phi SampleGGX can form (2^23); B, every float of the concentric disk's range
    [0.5, 3 pi / 4] and -[0.5, pi / 4] with the quadrant switches k = 0 -> 1 -> 2 (23 M); C, 4096 mantissas at every exponent
    below 0.5, both signs, denormals, +-0.  Nothing beyond [-pi / 4 - 1e-3, 2 pi], the domain the kernel states: outside it the
    float-to-int conversion of the quadrant differs between host and device on overflow, and no caller goes there."""
    worst = {}
    for name, x in _sincos_sets().items():
        sin_err = cos_err = excess = 0.0
        for lo in range(0, len(x), CHUNK):
            xs = x[lo:lo + CHUNK]
            out = _oracle(pkg, orc, "sincos", _rows(xs))
            s, c, x64 = out[:, 0].astype(np.float64), out[:, 1].astype(np.float64), xs.astype(np.float64)
            assert (np.abs(out) <= np.float32(1.0)).all(), f"set {name}: |sin| or |cos| above 1"
            if name != "B":
                assert _same_bits(out, _sincos_spec(xs)).all(), f"set {name}: not the bits of the definition restated in numpy"
            sin_err = max(sin_err, float(np.abs(s - np.sin(x64)).max()))
            cos_err = max(cos_err, float(np.abs(c - np.cos(x64)).max()))
            excess = max(excess, float((s * s + c * c - 1.0).max()))
        worst[name] = (len(x), sin_err, cos_err, excess)
        print(f"sincos set {name}: {len(x)} inputs, max |s - sin| {sin_err:.3e}, max |c - cos| {cos_err:.3e}, max s^2 + c^2 - 1 {excess:.3e}")
    for name, (_, sin_err, cos_err, excess) in worst.items():
        assert sin_err <= SIN_MAX_ABS_ERR and cos_err <= COS_MAX_ABS_ERR and excess <= UNIT_CIRCLE_EXCESS, (name, worst[name])
    zero = _oracle(pkg, orc, "sincos", np.uint32([[0], [0x80000000]])).view(np.uint32)
    assert (zero == np.float32([0.0, 1.0]).view(np.uint32)).all(), "sincos_(+-0) is (+0, 1)"


@pytest.mark.gpu
def test_sincos_device_equals_oracle(pkg, orc, gpu_renderer):
    """Sets A, B, C of test_sincos_against_float64 and D: NaNs and the infinities, bit for bit (two NaNs are equal)."""
    t0 = time.perf_counter()
    sets = _sincos_sets()
    sets["D"] = _f32([0x7fc00000, 0xffc00000, 0x7f800001, 0x7fffffff, 0x7f800000, 0xff800000])
    rows = bad = 0
    for name, x in sets.items():
        d = _device_differs(pkg, orc, gpu_renderer, "sincos", _rows(x))
        assert d == 0, f"set {name}: {d} output words differ"
        rows, bad = rows + len(x), bad + d
    _report("test_sincos_device_equals_oracle", t0, rows, bad)


# ---------------------------------------------------------------------------------------
# 2. pow_, log2_, exp2_
# ---------------------------------------------------------------------------------------
PQ_M1, PQ_M2 = np.float32(2610.0 / 4096.0 / 4.0), np.float32(2523.0 / 4096.0 * 128.0)  # exact in binary32
POW_SPECIAL_X = _f32([0, 0x80000000, 0x3f800000, 1, 0x007fffff, 0x7f800000, 0x7fc00000, 0xbf800000])  # 0 -0 1 denormals inf NaN -1
POW_SPECIAL_Y = _f32([0, 0x80000000, 1, 0x80000001, 0x007fffff, 0x7f800000, 0xff800000, 0x7fc00000])


def _positive_halfs():
    """Every positive finite binary16 value, as binary32."""
    return np.arange(1, 0x7c00, dtype=np.uint16).view(np.float16).astype(np.float32)


def _pow_sets():
    rng = np.random.default_rng(202)
    h = _positive_halfs()
    exps = np.float32([2.4, 1.0 / 2.4, PQ_M1, PQ_M2, 5.0, 0.5])  # sRGB decode / encode, PQ encode, Schlick, sqrt-like
    a = np.stack([np.tile(h, len(exps)), np.repeat(exps, len(h))], axis=1)
    c8 = np.arange(256, dtype=np.float32)
    b = np.stack([(c8 / np.float32(255.0) + np.float32(0.055)) / np.float32(1.055), np.full(256, 2.4, np.float32)], axis=1)
    # Beer-Lambert: pow(AttenuationColor, t / AttenuationDistance)
    n = 1 << 20
    cx = rng.uniform(0.0, 1.5, n).astype(np.float32)
    cy = (10.0 ** rng.uniform(-6, 6, n)).astype(np.float32) / (10.0 ** rng.uniform(-6, 6, n)).astype(np.float32)
    sx, sy = np.meshgrid(POW_SPECIAL_X, POW_SPECIAL_Y, indexing="ij")
    m = len(POW_SPECIAL_X) * 64
    c = np.concatenate([np.stack([cx, cy], axis=1),
                        np.stack([sx.ravel(), sy.ravel()], axis=1),
                        np.stack([np.repeat(POW_SPECIAL_X, 64), np.tile(cy[:64], len(POW_SPECIAL_X))], axis=1),
                        np.stack([np.tile(cx[:64], len(POW_SPECIAL_Y)), np.repeat(POW_SPECIAL_Y, 64)], axis=1)])
    assert len(c) == n + 64 + m + len(POW_SPECIAL_Y) * 64
    # wide: any positive finite bit pattern (denormals too), y = +-uniform * 10^[-3, 3]
    n = 1 << 22
    dx = _f32(rng.integers(1, 0x7f800000, n, dtype=np.uint32))
    dy = (rng.uniform(-1.0, 1.0, n) * 10.0 ** rng.uniform(-3, 3, n)).astype(np.float32)
    return {"A": a, "B": b, "C": c, "D": np.stack([dx, dy], axis=1)}


def _lod_sets():
    rng = np.random.default_rng(203)
    mant = np.concatenate([np.uint32([0, 1, 0x7fffff, 0x3504f3, 0x3504f4]), rng.integers(0, 1 << 23, 8187, dtype=np.uint32)])
    lo, hi = int(np.float32(1e-18).view(np.uint32)) >> 23, int(np.float32(1e18).view(np.uint32)) >> 23
    s = _f32(np.concatenate([np.uint32(e << 23) | mant for e in range(lo, hi + 1)]))
    s = np.concatenate([s[(s >= np.float32(1e-18)) & (s <= np.float32(1e18))], _floats_between(0.99, 1.01)])
    return s


def _pow_check(x, y, got, label):
    """pow_'s results `got` against the special cases written in it and, everywhere else, float64 np.power.  Returns (largest error
    in ULP over the normal-range results, largest absolute error over the denormal-range results, rows that leave the normal range)."""
    x64, y64, g64 = x.astype(np.float64), y.astype(np.float64), got.astype(np.float64)
    gb = _bits(got)
    one = (y == 0) | (x == 1)  # before the NaN test: pow_(NaN, 0) = pow_(1, NaN) = 1
    nan = ~one & (np.isnan(x) | np.isnan(y) | (x < 0))
    zero = ~one & ~nan & (x == 0)
    inf = ~one & ~nan & np.isinf(x)
    assert (gb[one] == np.float32(1.0).view(np.uint32)).all(), f"{label}: y == 0 or x == 1 is 1"
    assert np.isnan(got[nan]).all(), f"{label}: a NaN argument or a negative base is NaN"
    assert (gb[zero] == np.where(y[zero] > 0, np.uint32(0), PINF)).all(), f"{label}: pow_(0, y) is y > 0 ? 0 : inf"
    assert (gb[inf] == np.where(y[inf] > 0, PINF, np.uint32(0))).all(), f"{label}: pow_(inf, y) is y > 0 ? inf : 0"
    rest = ~(one | nan | zero | inf)
    with np.errstate(all="ignore"):
        truth = np.power(x64[rest], y64[rest])
    g = g64[rest]
    assert (gb[rest] == _bits(_pow_spec(x[rest], y[rest]))).all(), f"{label}: not the bits of the definition restated in numpy"
    over = truth >= F32_ROUNDS_TO_INF
    assert np.isposinf(g[over]).all(), f"{label}: a result above FLT_MAX is inf"
    tiny = truth < F32_MIN_NORMAL
    normal = ~over & ~tiny
    ulp = float(util.ulp_error(g[normal], truth[normal]).max()) if normal.any() else 0.0
    den = float(np.abs(g[tiny] - truth[tiny]).max()) if tiny.any() else 0.0
    return ulp, den, int(over.sum() + tiny.sum())


def test_pow_and_log2_against_float64(pkg, orc):
    """pow_(x, y) = (float)exp2_(clamp(y * log2_(x), +-300)) in double, rounded once.  A: every positive finite binary16 value (what
    the sRGB and PQ encodes see after an f16Round) under every exponent the renderer uses; B: all 256 sRGB decode arguments; C:
    Beer-Lambert pow(colour, t / d) with t and d log-uniform over [1e-6, 1e6], and every special value of either argument;
    D: any positive finite bit pattern under y = +-uniform * 10^[-3, 3] -- about a quarter of the results leave the normal range
    through the +-300 clamp, overflow and the denormals; E: computeLod = log2_(sqrt(s^2)) on 8192 mantissas at every exponent of
    [1e-18, 1e18] and every float of [0.99, 1.01] (the m > sqrt 2 fold, results next to zero).
    Normal-range results: within ONE_ROUNDING_ULP of float64.  Denormal-range results: within half the smallest denormal -- the
    double-to-float conversion rounds, it does not flush.  Above FLT_MAX: inf.  The special cases as pow_ writes them."""
    for name, xy in _pow_sets().items():
        out = _oracle(pkg, orc, "pow", xy.view(np.uint32))[:, 0]
        ulp, den, outside = _pow_check(xy[:, 0], xy[:, 1], out, f"set {name}")
        print(f"pow set {name}: {len(xy)} pairs, {outside} results outside the normal range, max error {ulp:.8f} ULP, "
              f"max denormal-range error {den:.3e}")
        assert ulp <= ONE_ROUNDING_ULP, (name, ulp)
        assert den <= 2.0 ** -150 * (1 + 1e-6), (name, den)  # half the smallest denormal, and the kernel's own error in double
        if name == "D":
            assert outside > len(xy) // 8, "the wide set no longer reaches the clamp, the overflow and the denormals"
    s = _lod_sets()
    lod = _oracle(pkg, orc, "computeLod", _rows(s, 0.0, 0.0, 0.0))[:, 0]
    truth = np.log2(np.sqrt(s * s).astype(np.float64))  # both float32 operations are correctly rounded on either side
    assert (_bits(lod) == _bits(_log2_spec(np.sqrt(s * s).astype(np.float64)).astype(np.float32))).all(), "computeLod: not the definition's bits"
    ulp = float(util.ulp_error(lod, truth).max())
    print(f"computeLod set E: {len(s)} inputs, max error {ulp:.8f} ULP")
    assert ulp <= ONE_ROUNDING_ULP, ulp
    assert _oracle(pkg, orc, "computeLod", _rows(np.float32([1.0, 0.0]), 0.0, 0.0, 0.0)).view(np.uint32).tolist() == [[0], [0]]


@pytest.mark.gpu
def test_pow_and_log2_device_equals_oracle(pkg, orc, gpu_renderer):
    """Sets A - E of test_pow_and_log2_against_float64, and computeLod of 0, inf and NaN, bit for bit."""
    t0 = time.perf_counter()
    rows = 0
    for name, xy in _pow_sets().items():
        d = _device_differs(pkg, orc, gpu_renderer, "pow", xy.view(np.uint32))
        assert d == 0, f"pow set {name}: {d} results differ"
        rows += len(xy)
    s = np.concatenate([_lod_sets(), _f32([0, 0x80000000, 0x7f800000, 0x7fc00000])])
    d = _device_differs(pkg, orc, gpu_renderer, "computeLod", _rows(s, 0.0, 0.0, 0.0))
    assert d == 0, f"computeLod: {d} results differ"
    _report("test_pow_and_log2_device_equals_oracle", t0, rows + len(s), 0)


# ---------------------------------------------------------------------------------------
# 3. atan2_, asin_
# ---------------------------------------------------------------------------------------
ATAN_SPECIALS = _f32([0, 0x80000000, 1, 0x80000001, 0x007fffff, 0x7f800000, 0xff800000, 0x7fc00000, 0x3f800000, 0xbf800000])


def _step(x, k):
    """x moved k binary32 values away from zero (x positive or negative, not zero)."""
    return _f32((_bits(x).astype(np.int64) + k).astype(np.uint32))


def _atan_sets():
    rng = np.random.default_rng(303)
    n = 1 << 22
    a = (rng.normal(size=(n, 2)) * 10.0 ** rng.uniform(-30, 30, (n, 1))).astype(np.float32)
    # miss.rmiss: longitude = atan(dir.z, dir.x), latitude = asin(-dir.y)
    d = rng.normal(size=(1 << 20, 3))
    axes = np.array([(x, y, z) for x in (-1, 0, 1) for y in (-1, 0, 1) for z in (-1, 0, 1) if (x, y, z) != (0, 0, 0)], np.float64)
    d = np.concatenate([d, axes])
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    b = np.concatenate([np.stack([d[:, 2], d[:, 0]], axis=1), np.stack([-d[:, 1], d[:, 0]], axis=1)])
    # the a > tan(pi / 8) reduction and the |y| == |x| octant edge, in every octant
    hi = (rng.uniform(0.5, 2.0, 4096) * 10.0 ** rng.uniform(-10, 10, 4096)).astype(np.float32)
    lo0 = (hi.astype(np.float64) * np.tan(np.pi / 8)).astype(np.float32)
    lo = np.concatenate([_step(lo0, k) for k in (-2, -1, 0, 1, 2)] + [hi])
    hh = np.tile(hi, 6)
    c = np.concatenate([np.stack([sy * p, sx * q], axis=1) for p, q in ((lo, hh), (hh, lo)) for sy in (1, -1) for sx in (1, -1)]).astype(np.float32)
    # 2^16 more ratios rounded from tan(pi / 8) itself: a fifth of them lie within 2e-8 of the edge, where taking the other branch
    # moves the double result by no more than 1e-11 -- only the bits of the restated definition can tell
    hi = (rng.uniform(0.5, 2.0, 1 << 16) * 10.0 ** rng.uniform(-10, 10, 1 << 16)).astype(np.float32)
    lo = (hi.astype(np.float64) * np.tan(np.pi / 8)).astype(np.float32)
    c = np.concatenate([c] + [np.stack([sy * p, sx * q], axis=1) for p, q in ((lo, hi), (hi, lo)) for sy in (1, -1) for sx in (1, -1)]).astype(np.float32)
    # asin next to +-1: every float of [0.9999, 1], three beyond, 2
    e = np.concatenate([_floats_between(0.9999, _step(np.float32([1.0]), 3)[0]), np.float32([2.0])])
    e = np.concatenate([e, -e])
    dd = np.stack([e, np.ones_like(e)], axis=1)
    sy, sx = np.meshgrid(ATAN_SPECIALS, ATAN_SPECIALS, indexing="ij")
    return {"A": a, "B": b, "C": c, "D": dd, "E": np.stack([sy.ravel(), sx.ravel()], axis=1)}


def test_atan2_asin_against_float64(pkg, orc):
    """atan2_ and asin_ are double-precision kernels rounded once: within ONE_ROUNDING_ULP of np.arctan2 / np.arcsin(clip).
    A: pairs of any common magnitude; B: unit directions as missSkyboxTexCoords passes them, with the 26 axis and diagonal
    directions; C: both sides of the a > tan(pi / 8) reduction, 0, +-1 and +-2 floats from it, and |y| == |x|, in every octant;
    D: asin on every float of [0.9999, 1], three beyond, +-2; E: signed zeros, denormals, infinities, NaN in each slot.

    The special values are this project's definition and the device returns them too.  They are NOT all IEEE's:
    atan2_(+-0, +-0) = +0 whatever the signs (IEEE: atan2(0, -0) = pi, atan2(-0, -0) = -pi); y < 0 is false for -0, so
    atan2_(-0, x < 0) = +pi (IEEE: -pi) while atan2_(-0, x > 0) = -0 as in IEEE; atan2_(+-inf, +-inf) = NaN (IEEE: +-pi / 4,
    +-3 pi / 4); atan2_(NaN, +-0) = +0 (IEEE: NaN), every other NaN argument gives NaN; asin_(|x| > 1) = +-pi / 2 (IEEE: NaN).  A finite y over an infinite x, and an infinite y over a finite x, agree with IEEE up to the sign of a zero."""
    pi, hpi = np.float32(np.pi), np.float32(np.pi / 2)
    spec = _oracle(pkg, orc, "atanAsin", _rows(np.float32([0.0, 0.0, -0.0, np.inf, 2.0, -2.0, np.nan, -np.inf, 1.0]),
                                                np.float32([0.0, -0.0, -1.0, np.inf, 1.0, 1.0, 1.0, -np.inf, -np.inf])))
    assert _bits(spec[:3, 0]).tolist() == [0, 0, int(pi.view(np.uint32))], "atan2_(0, 0), atan2_(0, -0), atan2_(-0, -1)"
    assert np.isnan(spec[3, 0]) and np.isnan(spec[7, 0]) and np.isnan(spec[6]).all(), "atan2_(inf, inf), atan2_ / asin_(NaN)"
    assert spec[4, 1] == hpi and spec[5, 1] == -hpi and spec[3, 1] == hpi and spec[7, 1] == -hpi, "asin_(|x| > 1) = +-pi / 2"
    assert spec[8, 0] == pi, "atan2_(1, -inf) = pi"
    for name, yx in _atan_sets().items():
        out = _oracle(pkg, orc, "atanAsin", yx.view(np.uint32))
        y, x = yx[:, 0], yx[:, 1]
        assert _same_bits(out[:, 0], _atan2_spec(y, x)).all() and _same_bits(out[:, 1], _asin_spec(y)).all(), \
            f"set {name}: not the bits of the definition restated in numpy"
        # where IEEE and the definition above part: a zero y (its sign), both infinite, NaN
        plain = ~(np.isnan(y) | np.isnan(x) | (np.isinf(y) & np.isinf(x)) | (y == 0))
        with np.errstate(all="ignore"):
            at = util.ulp_error(out[plain, 0], np.arctan2(y[plain].astype(np.float64), x[plain].astype(np.float64)))
            ok = ~np.isnan(y)
            asn = util.ulp_error(out[ok, 1], np.arcsin(np.clip(y[ok].astype(np.float64), -1.0, 1.0)))
        zero_y = (y == 0) & ~np.isnan(x)
        want = np.where(x[zero_y] < 0, pi, np.where(x[zero_y] > 0, y[zero_y], np.float32(0.0)))
        assert (_bits(out[zero_y, 0]) == _bits(want)).all(), f"set {name}: atan2_(+-0, x) is +pi for x < 0, +-0 for x > 0, +0 for x == 0"
        nan_zero = np.isnan(y) & (x == 0)  # the hi == 0 test comes before anything else and a NaN never is the larger magnitude
        assert (_bits(out[nan_zero, 0]) == 0).all(), f"set {name}: atan2_(NaN, +-0) is +0"
        assert np.isnan(out[~plain & ~zero_y & ~nan_zero, 0]).all() and np.isnan(out[~ok, 1]).all(), f"set {name}: NaN cases"
        print(f"atan2 / asin set {name}: {len(yx)} pairs, max error atan2 {float(at.max()):.8f} ULP, asin {float(asn.max()):.8f} ULP")
        assert at.max() <= ONE_ROUNDING_ULP and asn.max() <= ONE_ROUNDING_ULP, (name, float(at.max()), float(asn.max()))


@pytest.mark.gpu
def test_atan2_asin_device_equals_oracle(pkg, orc, gpu_renderer):
    """Sets A - E of test_atan2_asin_against_float64, bit for bit (two NaNs are equal)."""
    t0 = time.perf_counter()
    rows = 0
    for name, yx in _atan_sets().items():
        d = _device_differs(pkg, orc, gpu_renderer, "atanAsin", yx.view(np.uint32))
        assert d == 0, f"set {name}: {d} output words differ"
        rows += len(yx)
    _report("test_atan2_asin_device_equals_oracle", t0, rows, 0)


# ---------------------------------------------------------------------------------------
# 4. the samplers built on them, on the RNG lattice
# ---------------------------------------------------------------------------------------
def _lattice_lines():
    """(label, u) for the lines of [0, 1)^2 the samplers are walked along; lat = k / 2^23."""
    lat = np.arange(LATTICE, dtype=np.float32) * np.float32(2.0 ** -23)
    some = lat[::8]  # 2^20 of them
    yield "(0, lat)", _rows(0.0, lat)
    yield "(lat, 0)", _rows(lat, 0.0)
    for u0 in (2.0 ** -23, 0.25, 0.5, 1.0 - 2.0 ** -23):
        yield f"({u0!r}, lat)", _rows(u0, some)
        yield f"(lat, {u0!r})", _rows(some, u0)
    yield "(lat, lat)", _rows(lat, lat)
    yield "(lat, 1 - 2^-23 - lat)", _rows(lat, lat[::-1])


def _ggx_sets():
    lat = np.arange(LATTICE, dtype=np.float32) * np.float32(2.0 ** -23)
    some = lat[::8]
    v = np.float64([0.3, -0.5, 0.8])
    v /= np.linalg.norm(v)
    g = np.float64([0.99, 0.0, 0.01])
    g /= np.linalg.norm(g)
    yield "V = normalize(0.3, -0.5, 0.8), alpha 0.25, u.x 0.5", _rows(0.5, lat, v[0], v[1], v[2], 0.25)
    yield "V = (0, 0, 1), alpha 1e-4, u.x 1 - 2^-23", _rows(1.0 - 2.0 ** -23, some, 0.0, 0.0, 1.0, 1e-4)
    yield "V = normalize(0.99, 0, 0.01), alpha 1, u.x 0", _rows(0.0, some, g[0], g[1], g[2], 1.0)


def test_samplers_on_the_rng_lattice(pkg, orc):
    """sampleUniformDiskConcentric, sampleCosineHemisphere and SampleGGX on what rnd() can return: u = (0, lat) and (lat, 0) in
    full, (u0, lat) and (lat, u0) on every eighth lattice value for u0 next to 0, at 0.25, at 0.5 (offset 0: the theta = pi / 2
    branch with a zero numerator) and next to 1, the diagonal and the anti-diagonal in full.

    x and y are always finite and z is never negative, but z IS NaN on part of the disk's rim: where a coordinate of u is
    exactly 0 the offset has magnitude 1, the point is (cos, sin) itself, and the kernel's sin^2 + cos^2 may exceed 1 by up to
    1.36e-7 (test_sincos_against_float64), so that 1 - x^2 - y^2 < 0.  That is the reference's own sqrt(1 - d.x * d.x - d.y * d.y)
    (common.glsl:189), and it is what the NaN restart of the sample loop absorbs.  The counts are pinned as measured on the
    oracle, the definition: a change of them is a change of the images."""
    for label, u in _lattice_lines():
        d = _oracle(pkg, orc, "sampleCosineHemisphere", u)
        uf = u.view(np.float32)
        assert np.isfinite(d[:, :2]).all(), f"{label}: x or y not finite"
        assert not (d[:, 2] < 0).any() and not np.isinf(d[:, 2]).any(), f"{label}: z negative or infinite"
        nan = np.isnan(d[:, 2])
        assert not (nan & (uf[:, 0] != 0) & (uf[:, 1] != 0)).any(), f"{label}: NaN away from the rim"
        print(f"sampleCosineHemisphere {label}: {len(u)} inputs, {int(nan.sum())} NaN z")
        assert int(nan.sum()) == HEMISPHERE_NANS.get(label, 0), (label, int(nan.sum()))
        if len(u) < LATTICE:  # the disk alone returns the same x, y
            disk = _oracle(pkg, orc, "sampleUniformDiskConcentric", u)
            assert (disk.view(np.uint32) == d[:, :2].view(np.uint32)).all(), label
    for label, rows in _ggx_sets():
        h = _oracle(pkg, orc, "SampleGGX", rows)
        assert np.isfinite(h).all(), f"SampleGGX {label}: not finite"
        err = float(np.abs(np.sqrt((h.astype(np.float64) ** 2).sum(axis=1)) - 1.0).max())
        print(f"SampleGGX {label}: {len(rows)} inputs, max | |H| - 1 | {err:.3e}")
        assert err <= 2e-7 and (h[:, 2] >= 0).all(), (label, err)


@pytest.mark.gpu
def test_samplers_device_equals_oracle(pkg, orc, gpu_renderer):
    """The lines of test_samplers_on_the_rng_lattice, bit for bit, and with that the same NaN counts."""
    t0 = time.perf_counter()
    rows = 0
    for label, u in _lattice_lines():
        for fn in ("sampleCosineHemisphere", "sampleUniformDiskConcentric"):
            d = _device_differs(pkg, orc, gpu_renderer, fn, u)
            assert d == 0, f"{fn} {label}: {d} output words differ"
        rows += 2 * len(u)
    for label, r in _ggx_sets():
        d = _device_differs(pkg, orc, gpu_renderer, "SampleGGX", r)
        assert d == 0, f"SampleGGX {label}: {d} output words differ"
        rows += len(r)
    _report("test_samplers_device_equals_oracle", t0, rows, 0)


# ---------------------------------------------------------------------------------------
# 5. the output stage on every binary16 value and on every rounding tie
# ---------------------------------------------------------------------------------------
TIE_W, TIE_H = 512, 496
NO_BLOOM = dict(exposure=1.0, bloom_intensity=0.0, bloom_threshold=1e6)  # a threshold above every input keeps the bloom at zero


def _tie_values():
    """For every non-negative finite binary16 value h: h, the binary32 midpoint between h and its successor, and the floats
    one step either side of the midpoint; then all of them negated -- without the four values of magnitude >= 65520, which round
    to infinity (253,948 values)."""
    h = np.arange(0, 0x7c00, dtype=np.uint16).view(np.float16).astype(np.float64)
    nxt = np.append(h[1:], 65536.0)
    mid = ((h + nxt) / 2).astype(np.float32)  # exact: 12 significant bits
    pos = np.stack([h.astype(np.float32), _step(mid, -1), mid, _step(mid, 1)], axis=1).ravel()
    pos = pos[pos < np.float32(65520.0)]
    v = np.concatenate([pos, -pos])
    assert len(v) == 253948
    return v


def _tie_image():
    v = _tie_values()
    flat = np.zeros(TIE_W * TIE_H, np.float32)
    flat[:len(v)] = v
    acc = np.ones((TIE_H, TIE_W, 4), np.float32)
    acc[..., :3] = flat.reshape(TIE_H, TIE_W, 1)
    return acc, len(v)


def _overflow_image():
    acc = np.ones((2, 2, 4), np.float32)  # small enough to skip the bloom chain
    acc[..., :3] = np.float32([65520.0, -65520.0, _step(np.float32([65520.0]), 1)[0], -_step(np.float32([65520.0]), 1)[0]]).reshape(2, 2, 1)
    return acc


def _srgb64(c):
    with np.errstate(all="ignore"):
        return np.where(c <= 0.0031308, 12.92 * c, 1.055 * np.power(np.maximum(c, 0.0), 1.0 / 2.4) - 0.055)


def test_output_stage_on_every_half_and_tie(pkg, orc):
    """One accumulation image holds every non-negative finite binary16 value, every binary32 midpoint between two of them (the
    ties of f16Round: to even, in the subnormals too), the floats either side of every midpoint, and the same negated.  The bloom
    threshold lies above every input: at a threshold of 1, level 0 of the bloom chain overflows binary16 in the upsample sum and
    inf * 0 = NaN floods the image through composition.comp, as it would in the reference.

    HDR mode: the RGBA32F output is the input rounded to binary16, by value; by bits too, except that the three inputs which
    round to -0 come out +0 (composition.comp adds the bloom term +0).  SDR mode: within one binary16 step of float64
    1 - exp(-h), and the sRGB8 image is floor(clip(srgb(c)) * 255 + 0.5) of the float64 sRGB curve at the stage's own linear
    value c, for every pixel.  The four inputs of magnitude >= 65520 come out as infinities (in an image too small to bloom)."""
    acc, n = _tie_image()
    x = acc[..., 0].ravel()
    want = x.astype(np.float16).astype(np.float32)
    hdr = orc.postprocess(acc, 1, tone_mapping=1, **NO_BLOOM)
    assert (hdr[..., 3] == 1).all() and (hdr[..., 0] == hdr[..., 1]).all() and (hdr[..., 0] == hdr[..., 2]).all()
    got = hdr[..., 0].ravel()
    assert (got == want).all(), "HDR mode: the output is not the input rounded to binary16"
    differ = np.flatnonzero(_bits(got) != _bits(want))
    minus_zero = np.flatnonzero(_bits(want) == 0x80000000)
    assert len(minus_zero) == 3 and (differ == minus_zero).all() and (_bits(got[differ]) == 0).all(), "only the three -0 come out +0"
    assert (orc.encode_output(hdr, 1).view(np.uint32) == hdr.view(np.uint32)).all()
    sdr = orc.postprocess(acc, 1, tone_mapping=0, **NO_BLOOM)
    c = sdr[..., 0].ravel()
    with np.errstate(over="ignore"):
        truth = 1.0 - np.exp(-want.astype(np.float64))  # -inf where it leaves binary16 (and float64)
        steps = np.abs(util.half_ordinal(c) - util.half_ordinal(truth))
    print(f"output stage: {n} values, SDR at most {int(steps.max())} binary16 steps from float64, "
          f"{int((steps == 1).sum())} values one step away")
    assert steps.max() <= 1
    srgb = orc.encode_output(sdr, 0)
    with np.errstate(invalid="ignore"):
        want8 = np.floor(np.clip(np.nan_to_num(_srgb64(sdr[..., :3].astype(np.float64)), neginf=0.0), 0.0, 1.0) * 255.0 + 0.5)
    bad = int((srgb[..., :3] != want8.astype(np.uint8)).sum())
    print(f"output stage: sRGB8 against the float64 curve: {bad} mismatches")
    assert bad == 0 and (srgb[..., 3] == 255).all()
    over = orc.postprocess(_overflow_image(), 1, tone_mapping=1, **NO_BLOOM)
    assert (over[..., 0].ravel() == np.float32([np.inf, -np.inf, np.inf, -np.inf])).all()


def _tonemap_rows():
    p = np.arange(1 << 16, dtype=np.uint16)
    return np.stack([p, p[::-1], p ^ np.uint16(0x8000)], axis=1).view(np.float16).astype(np.float32).view(np.uint32)


def test_tonemap_pixel_on_every_half(pkg, orc):
    """toneMapping.comp's 1 - exp(-c) on all 65536 binary16 patterns: NaN in, NaN out; +inf -> 1; -inf -> -inf; and every finite
    input within the two roundings of the definition -- exp_ is the double kernel rounded once (ONE_ROUNDING_ULP of exp(-c)),
    the subtraction from 1 rounds once more (half a unit of the result)."""
    rows = _tonemap_rows()
    c, out = rows.view(np.float32).ravel(), _oracle(pkg, orc, "toneMapPixel", rows).ravel()
    assert np.isnan(out[np.isnan(c)]).all() and not np.isnan(out[~np.isnan(c)]).any()
    assert (out[np.isposinf(c)] == 1).all() and np.isneginf(out[np.isneginf(c)]).all()
    fin = np.isfinite(c)
    with np.errstate(over="ignore"):
        e = np.exp(-c[fin].astype(np.float64))
    ok = e < F32_ROUNDS_TO_INF
    assert np.isneginf(out[fin][~ok]).all()
    e, got = e[ok], out[fin][ok].astype(np.float64)
    spacing = lambda t: np.ldexp(1.0, np.maximum(np.frexp(t)[1] - 1, -126) - 23)  # noqa: E731
    bound = ONE_ROUNDING_ULP * spacing(e) + 0.5 * spacing(1.0 - e)
    assert (np.abs(got - (1.0 - e)) <= bound).all()


@pytest.mark.gpu
def test_output_stage_device_equals_oracle(pkg, orc, gpu_renderer):
    """The images of test_output_stage_on_every_half_and_tie through ptx_postprocess / ptx_read_output in both tone-mapping modes
    and both output formats, and toneMapPixel on all 65536 binary16 patterns: the oracle's bits."""
    t0 = time.perf_counter()
    bad = 0
    for acc in (_tie_image()[0], _overflow_image()):
        r = pkg.Renderer()
        r.resize(acc.shape[1], acc.shape[0])
        r.write_accumulation(acc)
        for tone in (1, 0):
            r.postprocess(1, tone_mapping=tone, **NO_BLOOM)
            ref = orc.postprocess(acc, 1, tone_mapping=tone, **NO_BLOOM)
            d = int((~util.bits_equal_or_both_nan(r.read_output(pkg.OUTPUT_RGBA32F).view(np.uint32), ref.view(np.uint32))).sum())
            d += int((r.read_output(pkg.OUTPUT_RGBA8_SRGB) != orc.encode_output(ref, 0)).sum())
            assert d == 0, f"{acc.shape[1]} x {acc.shape[0]}, tone mapping {tone}: {d} output words differ"
            bad += d
            if tone == 1 and acc.shape[0] == 2:
                assert np.isinf(r.read_output(pkg.OUTPUT_RGBA32F)[..., :3]).all()
        r.close()
    d = _device_differs(pkg, orc, gpu_renderer, "toneMapPixel", _tonemap_rows())
    assert d == 0, f"toneMapPixel: {d} output words differ"
    _report("test_output_stage_device_equals_oracle", t0, TIE_W * TIE_H + 4 + (1 << 16), bad + d)
