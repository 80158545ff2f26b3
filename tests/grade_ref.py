"""CPU restatement of the display transform (include/ptx.h ptx_grade, steps 0 - 5; csrc/pt_grade.hpp), generic over a numpy dtype.

Written from the header's numbered steps.  Arithmetic conventions, the project's, in either dtype: every `/` of
the steps is a * (1 / b); pow and exp are evaluated in double precision and rounded to the dtype once, as tests/present_ref.py and
tests/test_transcendentals.py restate them; every store into an rgba16f image is a rounding to binary16.  The two divisions inside
srgbToLinear are IEEE quotients, as the header says.  Constants are the header's float literals, widened where the dtype is float64,
so that the float32 and the float64 instance differ in rounding alone.

In float32 and without pow / exp -- steps 1, 2a, 2c, the three rational curves, the LUT outside the sRGB domain -- every operation is
one IEEE operation in the stated order, and the device's result equals this one bit for bit."""
import numpy as np

CURVE_REFERENCE, CURVE_REINHARD, CURVE_HABLE, CURVE_ACES_FIT = range(4)
USE_LUT, LUT_SRGB_DOMAIN = 1, 2
SDR, HDR = 0, 1

HABLE = dict(A=0.15, B=0.50, C=0.10, D=0.20, E=0.02, F=0.30)
HABLE_EXPOSURE_BIAS, HABLE_WHITE = 2.0, 11.2
ACES_IN = (0.59719, 0.35458, 0.04823, 0.07600, 0.90834, 0.01566, 0.02840, 0.13383, 0.83777)
ACES_OUT = (1.60475, -0.53108, -0.07367, -0.10208, 1.10813, -0.00605, -0.00327, -0.07276, 1.07602)
ACES_A, ACES_B, ACES_C, ACES_D, ACES_E = 0.0245786, 0.000090537, 0.983729, 0.4329510, 0.238081

IDENTITY = dict(colour_matrix=(1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0), slope=(1.0, 1.0, 1.0), offset=(0.0, 0.0, 0.0), power=(1.0, 1.0, 1.0),
                saturation=1.0, curve=CURVE_REFERENCE, white_point=4.0)


def _k(x, dtype):
    """a float literal of the header in `dtype`"""
    return dtype(np.float32(x))


def _f16(x, dtype):
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(x).astype(np.float16).astype(dtype)


def _div(a, b, dtype):
    with np.errstate(all="ignore"):
        return np.asarray(a, dtype) * (dtype(1.0) / np.asarray(b, dtype))


def _pow(x, y, dtype):
    """pow_(x, y), x >= 0: a negative base is a NaN whatever the exponent"""
    x = np.asarray(x, np.float64)
    with np.errstate(all="ignore"):
        r = np.power(x, np.float64(y))
    return np.where(x < 0, np.nan, r).astype(dtype)


def _exp(x, dtype):
    with np.errstate(all="ignore"):
        return np.exp(np.asarray(x, np.float64)).astype(dtype)


def _max0(a, dtype):
    """max(a, 0) = a < 0 ? 0 : a"""
    with np.errstate(invalid="ignore"):
        return np.where(a < 0, dtype(0.0), a)


def _clamp01(a, dtype):
    """min(max(a, 0), 1), min(a, b) = b < a ? b : a; a NaN passes through"""
    a = _max0(a, dtype)
    with np.errstate(invalid="ignore"):
        return np.where(dtype(1.0) < a, dtype(1.0), a)


def luminance(c, dtype):
    return (_k(0.2126, dtype) * c[..., 0] + _k(0.7152, dtype) * c[..., 1]) + _k(0.0722, dtype) * c[..., 2]


def mat3(m, c, dtype):
    m = [dtype(np.float32(v)) for v in m]
    with np.errstate(all="ignore"):
        return np.stack([(m[3 * i] * c[..., 0] + m[3 * i + 1] * c[..., 1]) + m[3 * i + 2] * c[..., 2] for i in range(3)], axis=-1)


def compose(post, bloom0, bloom_intensity, dtype=np.float32):
    """Step 0 from the post-process image and bloom level 0."""
    post, bloom0 = np.asarray(post, dtype), np.asarray(bloom0, dtype)
    with np.errstate(all="ignore"):
        return _f16(bloom0 * (dtype(np.float32(bloom_intensity)) * _k(0.1, dtype)) + post * dtype(1.0), dtype)


def linear_to_srgb(x, dtype):
    with np.errstate(all="ignore"):
        return np.where(x <= _k(0.0031308, dtype), _k(12.92, dtype) * x,
                        _k(1.055, dtype) * _pow(x, np.float32(1.0) / np.float32(2.4), dtype) - _k(0.055, dtype))


def srgb_to_linear(x, dtype):
    with np.errstate(all="ignore"):
        return np.where(x <= _k(0.04045, dtype), x / _k(12.92, dtype), _pow((x + _k(0.055, dtype)) / _k(1.055, dtype), np.float32(2.4), dtype))


def curve_reference(v, dtype):
    return dtype(1.0) - _exp(-v, dtype)


def curve_reinhard(v, white_point, dtype):
    w = dtype(np.float32(white_point))
    with np.errstate(all="ignore"):
        return _div(v * (dtype(1.0) + _div(v, w * w, dtype)), dtype(1.0) + v, dtype)


def hable_f(x, dtype):
    A, B, C, D, E, F = (_k(HABLE[n], dtype) for n in "ABCDEF")
    with np.errstate(all="ignore"):
        return _div(x * (A * x + C * B) + D * E, x * (A * x + B) + D * F, dtype) - _div(E, F, dtype)


def curve_hable(v, dtype):
    with np.errstate(all="ignore"):
        return _div(hable_f(_k(HABLE_EXPOSURE_BIAS, dtype) * v, dtype), hable_f(_k(HABLE_WHITE, dtype), dtype), dtype)


def aces_rational(t, dtype):
    a, b, c, d, e = (_k(x, dtype) for x in (ACES_A, ACES_B, ACES_C, ACES_D, ACES_E))
    with np.errstate(all="ignore"):
        return _div(t * (t + a) - b, t * (c * t + d) + e, dtype)


def curve_aces_fit(v, dtype):
    t = mat3(ACES_IN, v, dtype)
    t = aces_rational(t, dtype)
    return _clamp01(mat3(ACES_OUT, t, dtype), dtype)


def lut_coordinates(x, n, dtype):
    """Step 4's index and fraction per channel of x in [0, 1] (or NaN: index 0, fraction NaN)."""
    with np.errstate(invalid="ignore"):
        s = x * dtype(n - 1)
        i = np.where(s >= 0, np.minimum(np.floor(s), n - 2), 0).astype(np.int64)
        return i, s - i.astype(dtype)


ORDERS = ("rgb", "rbg", "brg", "bgr", "gbr", "grb")


def lut_order(f):
    """The index into ORDERS per pixel: the header's >= comparisons in the header's order."""
    r, g, b = f[..., 0], f[..., 1], f[..., 2]
    with np.errstate(invalid="ignore"):
        first = np.where(g >= b, 0, np.where(r >= b, 1, 2))
        second = np.where(b >= g, 3, np.where(b >= r, 4, 5))
        return np.where(r >= g, first, second)


def lut_lookup(v, lut, srgb, dtype):
    """Step 4.  lut: N x N x N x 3 indexed [blue, green, red]."""
    lut = np.asarray(lut, np.float32)
    n = lut.shape[0]
    assert lut.shape == (n, n, n, 3)
    table = lut.astype(dtype)
    x = _clamp01(v, dtype)
    if srgb:
        x = linear_to_srgb(x, dtype)
    i, f = lut_coordinates(x, n, dtype)
    order = lut_order(f)
    axis = {"r": 0, "g": 1, "b": 2}
    hi, mid, lo = (np.empty(f.shape[:-1], dtype) for _ in range(3))
    step_a, step_b = np.zeros(i.shape, np.int64), np.zeros(i.shape, np.int64)
    for k, name in enumerate(ORDERS):
        sel = order == k
        p, q, s = (axis[ch] for ch in name)
        hi[sel], mid[sel], lo[sel] = f[..., p][sel], f[..., q][sel], f[..., s][sel]
        step_a[..., p][sel] = 1
        step_b[..., p][sel] = 1
        step_b[..., q][sel] = 1

    def entry(at):
        return table[at[..., 2], at[..., 1], at[..., 0]]

    v000, va, vb, v111 = entry(i), entry(i + step_a), entry(i + step_b), entry(i + 1)
    with np.errstate(all="ignore"):
        out = ((v000 * (dtype(1.0) - hi)[..., None] + va * (hi - mid)[..., None]) + vb * (mid - lo)[..., None]) + v111 * lo[..., None]
    if srgb:
        out = srgb_to_linear(out, dtype)
    return out


def _bits(values):
    return np.asarray(values, np.float32).view(np.uint32)


def steps_that_run(colour_matrix, slope, offset, power, saturation, mode, flags):
    """The skip rule: identity parameters, bit for bit."""
    return dict(matrix=(_bits(colour_matrix) != _bits(IDENTITY["colour_matrix"])).any(),
                slope_offset=(_bits(slope) != _bits((1, 1, 1))).any() or (_bits(offset) != 0).any(),
                power=(_bits(power) != _bits((1, 1, 1))).any(), saturation=_bits([saturation])[0] != _bits([1])[0],
                curve=mode == SDR, lut=mode == SDR and bool(flags & USE_LUT))


def grade(c, mode=SDR, colour_matrix=IDENTITY["colour_matrix"], slope=IDENTITY["slope"], offset=IDENTITY["offset"], power=IDENTITY["power"],
          saturation=IDENTITY["saturation"], curve=IDENTITY["curve"], white_point=IDENTITY["white_point"], flags=0, lut=None, dtype=np.float32):
    """Steps 1 - 5 on the composed colour of step 0, c: ... x 3, binary16-valued.  Returns ... x 4 of `dtype`, alpha 1."""
    v = np.asarray(c)[..., :3].astype(dtype)
    run = steps_that_run(colour_matrix, slope, offset, power, saturation, mode, flags)
    f32 = lambda t: np.asarray(t, np.float32).astype(dtype)  # noqa: E731
    with np.errstate(all="ignore"):
        if run["matrix"]:
            v = mat3(colour_matrix, v, dtype)
        if run["slope_offset"]:
            v = _max0(v * f32(slope) + f32(offset), dtype)
        if run["power"]:
            v = np.stack([_pow(v[..., k], np.float32(power[k]), dtype) for k in range(3)], axis=-1)
        if run["saturation"]:
            y = luminance(v, dtype)[..., None]
            v = y + (v - y) * dtype(np.float32(saturation))
        if run["curve"]:
            if curve == CURVE_REFERENCE:
                v = curve_reference(v, dtype)
            elif curve == CURVE_REINHARD:
                v = curve_reinhard(v, white_point, dtype)
            elif curve == CURVE_HABLE:
                v = curve_hable(v, dtype)
            else:
                assert curve == CURVE_ACES_FIT
                v = curve_aces_fit(v, dtype)
        if run["lut"]:
            v = lut_lookup(v, lut, bool(flags & LUT_SRGB_DOMAIN), dtype)
    out = np.ones(v.shape[:-1] + (4,), dtype)
    out[..., :3] = _f16(v, dtype)
    return out
