"""Display transform (include/ptx.h "Display transform": ptx_grade, ptx_grade_lut, ptx_present_graded; csrc/pt_grade.hpp,
docs/NEXT_ROWS.md section 22) against tests/grade_ref.py.

Step 0, the composed colour, is the oracle's orc.postprocess(..., tone_mapping=1), as in tests/test_present.py (the HDR mode passes
composition.comp's store through); one GPU test holds the device's against it.  Steps 1 - 5 are the numpy reference's.

Two kinds of cases.  EXACT: only steps 1, 2a, 2c, the three rational curves and a LUT outside the sRGB domain run -- every operation a
single IEEE float32 operation in the header's order -- and the device equals the float32 reference bit for bit (two NaNs count as equal).
AGAINST FLOAT64: the cases with pow or exp (CDL power, PTX_CURVE_REFERENCE, the sRGB domain), whose kernels are specified to a
tolerance and not to the bit.  The device may differ from the float64 reference by 8 x the maximum of |ref(float32) - ref(float64)|
of that case over the five frames, measured on the reference alone: the constants REF_F32_VS_F64 below, printed by

    python tests/test_grade.py

and recomputed by test_reference_float32_against_float64 without a GPU.

Frames: a synthetic sum at 1 x 1, 5 x 3, 33 x 22 (bloom intensity 0: the special values below reach the grade as written), 67 x 45 and
300 x 200 (bloom on: more than one workgroup, a partial last one).  Every frame of 15 pixels or more holds NaN and Inf (the output
stage's marker pixels), a negative channel, values above 1, exact greys (all three LUT fractions tie), every pair of equal channels
(two fractions tie), 0 and 1 (lattice points of every LUT; the largest frame also a pixel of 10^6, whose bloom is NaN; under Reinhard with w = 10^4 a grey of 1 lands on 0.5, an interior lattice
point of every odd N), and all six orders of three different channels."""
import ctypes as C
import os
import re
import sys
from decimal import Decimal

import numpy as np
import pytest

import grade_ref as R
import present_ref as PR

SAMPLES = 8
FRAMES = {"1x1": (1, 1, 0.0), "5x3": (5, 3, 0.0), "33x22": (33, 22, 0.0), "67x45": (67, 45, 0.35), "300x200": (300, 200, 0.35)}  # width, height, bloom intensity
OK, INVALID, NOT_READY = 0, 1, 5
WB = (1.2, -0.1, 0.05, -0.05, 0.95, 0.02, 0.01, -0.08, 1.4)
CDL = dict(slope=(1.1, 0.9, 1.0), offset=(0.01, -0.02, 0.0), saturation=1.3)
H, RH, HB, AC = R.CURVE_REFERENCE, R.CURVE_REINHARD, R.CURVE_HABLE, R.CURVE_ACES_FIT

# name -> (exact?, LUT size or None, mode, the desc's fields that are not the identity's)
CASES = {
    "matrix_reinhard": (True, None, R.SDR, dict(colour_matrix=WB, curve=RH, white_point=4.0)),
    "cdl_hable": (True, None, R.SDR, dict(CDL, curve=HB)),
    "saturation0_aces": (True, None, R.SDR, dict(saturation=0.0, curve=AC)),
    "lut2": (True, 2, R.SDR, dict(curve=RH, white_point=1e4, flags=R.USE_LUT)),
    "lut3": (True, 3, R.SDR, dict(curve=RH, white_point=1e4, flags=R.USE_LUT)),
    "lut17": (True, 17, R.SDR, dict(curve=RH, white_point=1e4, flags=R.USE_LUT)),
    "lut33": (True, 33, R.SDR, dict(curve=RH, white_point=1e4, flags=R.USE_LUT)),
    "lut65": (True, 65, R.SDR, dict(curve=RH, white_point=1e4, flags=R.USE_LUT)),
    "matrix_cdl_aces_lut17": (True, 17, R.SDR, dict(CDL, colour_matrix=WB, curve=AC, flags=R.USE_LUT)),
    "cdl_hable_lut33": (True, 33, R.SDR, dict(CDL, curve=HB, flags=R.USE_LUT)),
    "hdr_skips_curve_and_lut": (True, 17, R.HDR, dict(CDL, colour_matrix=WB, curve=HB, flags=R.USE_LUT)),
    "matrix_slope_reference": (False, None, R.SDR, dict(colour_matrix=WB, slope=(1.5, 1.0, 0.75), curve=H)),
    "power_hable": (False, None, R.SDR, dict(CDL, power=(0.9, 1.1, 2.0), saturation=0.9, curve=HB)),  # 0.1 Y + 0.9 v >= 0: clear of Hable's poles
    "srgb_lut17": (False, 17, R.SDR, dict(curve=RH, white_point=4.0, flags=R.USE_LUT | R.LUT_SRGB_DOMAIN)),
    "everything_reference_srgb_lut33": (False, 33, R.SDR, dict(CDL, colour_matrix=WB, power=(0.9, 1.0, 1.2), curve=H, flags=R.USE_LUT | R.LUT_SRGB_DOMAIN)),
    "hdr_power": (False, None, R.HDR, dict(power=(0.8, 1.0, 1.2), saturation=1.1)),
}
EXACT = [n for n, c in CASES.items() if c[0]]
AGAINST_F64 = [n for n, c in CASES.items() if not c[0]]

# case -> max |ref(float32) - ref(float64)| over the five frames, on the binary16 image
REF_F32_VS_F64 = {
    'matrix_slope_reference': 4.883e-04,
    'power_hable': 4.883e-04,
    'srgb_lut17': 4.883e-04,
    'everything_reference_srgb_lut33': 4.883e-04,
    'hdr_power': 9.766e-04,
}
# the screen path of test_present_graded_against_float64: (case, screen width, screen height) -> the same figure, blit included
REF_PRESENT_F32_VS_F64 = {
    ('matrix_cdl_aces_lut17', 100, 37): 1.465e-03,
    ('power_hable', 134, 90): 2.441e-04,
    ('srgb_lut17', 100, 37): 1.465e-03,
}
PRESENT_CASES = [("matrix_cdl_aces_lut17", 100, 37), ("power_hable", 134, 90), ("srgb_lut17", 100, 37)]

# per sample; the first fifteen are the whole 5 x 3 frame: greys, ties of two channels, a negative (b > g > r), r > g > b, the two markers, the
# four other orders of three different channels, a highlight
SPECIALS = [(1, 1, 1), (0, 0, 0), (0.5, 0.5, 0.5), (0.25, 0.25, 0.75), (0.75, 0.25, 0.25), (0.75, 0.75, 0.25), (-0.5, 0.25, 0.5), (3, 2, 1), (np.nan, 0, 0),
            (0, np.inf, 0), (1, 0.25, 0.5), (0.5, 0.25, 2), (0.1, 0.3, 0.2), (0.5, 1, 0.25), (40, 40, 40),
            (0.25, 0.75, 0.25), (0.25, 0.75, 0.75), (0.75, 0.25, 0.75), (2, 1, 0.5)]


# =====================================================================================================
# inputs and references: computed once, shared, left unchanged
# =====================================================================================================
_cache = {}


def _once(key, make):
    if key not in _cache:
        v = make()
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
        _cache[key] = v
    return _cache[key]


def _synthetic_sum(w, h):
    """A ramp with noise and a hot spot that blooms, and SPECIALS spread over the frame (a 1 x 1 frame is the grey of 1)."""
    rng = np.random.default_rng(w * 1000 + h)
    img = np.zeros((h, w, 4), np.float32)
    yy, xx = np.mgrid[0:h, 0:w]
    img[..., 0] = 0.05 + 1.6 * xx / w
    img[..., 1] = 0.02 + 0.9 * yy / h
    img[..., 2] = 0.3
    img[..., :3] += rng.uniform(0, 0.02, (h, w, 3))
    if w * h >= 1000:
        img[h // 3:h // 3 + 6, w // 2:w // 2 + 6, :3] = 40.0
    if w * h >= 60000:
        img[h - 10, 10, :3] = (1e6, 1, 1)  # Inf in the post-process image and NaN in the bloom chain around it: NaN reaches every step
    flat = img.reshape(-1, 4)
    n = w * h
    count = min(n, len(SPECIALS))
    for k in range(count):
        flat[(k * n) // count + (n // count) // 2 if n > count else k, :3] = SPECIALS[k]
    img[..., :3] *= SAMPLES
    img[..., 3] = 1.0
    return img


def _acc(frame):
    w, h, _ = FRAMES[frame]
    return _once(("acc", frame), lambda: _synthetic_sum(w, h))


def _post(frame):
    return dict(exposure=1.0, bloom_threshold=0.8, bloom_intensity=FRAMES[frame][2])


def _composed(orc, frame):
    return _once(("composed", frame), lambda: orc.postprocess(_acc(frame), SAMPLES, tone_mapping=1, **_post(frame)))


def _lut(n):
    """N x N x N x 3 [blue, green, red]: the identity lattice bent by noise, so that a wrong corner or weight shows"""
    def make():
        rng = np.random.default_rng(n)
        g = np.arange(n, dtype=np.float64) / (n - 1)
        ident = np.stack(np.broadcast_arrays(g[None, None, :], g[None, :, None], g[:, None, None]), axis=-1)
        return (0.7 * ident + 0.3 * rng.uniform(0, 1, (n, n, n, 3))).astype(np.float32)
    return _once(("lut", n), make)


def _ref(orc, case, frame, dtype):
    _, n, mode, fields = CASES[case]
    return _once(("ref", case, frame, np.dtype(dtype).name),
                 lambda: R.grade(_composed(orc, frame), mode=mode, lut=None if n is None else _lut(n), dtype=dtype, **fields))


def _same(a, b):
    """The same float32 bits, or both NaN."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def _gap(a32, b64):
    with np.errstate(all="ignore"):
        d = np.abs(np.asarray(a32, np.float64) - b64)
    return float(np.max(np.where(np.isfinite(d), d, 0.0)))


def _measure(orc, case):
    return max(_gap(_ref(orc, case, f, np.float32)[..., :3], _ref(orc, case, f, np.float64)[..., :3]) for f in FRAMES)


def _present_ref(orc, case, sw, sh, dtype, frame="67x45"):
    """ptx_present_graded without a UI in the SDR mode: blit, f16Round, steps 1 - 5."""
    _, n, mode, fields = CASES[case]

    def make():
        c = PR._f16(PR.blit(_composed(orc, frame)[..., :3].astype(dtype), sw, sh, dtype), dtype)
        return R.grade(c, mode=mode, lut=None if n is None else _lut(n), dtype=dtype, **fields)
    return _once(("present", case, sw, sh, np.dtype(dtype).name), make)


def _assert_close_to_float64(got, ref64, worst, what):
    got = np.asarray(got, np.float64)
    assert got.shape == ref64.shape and (got[..., 3] == 1).all(), what
    g, r = got[..., :3], ref64[..., :3]
    assert (np.isnan(g) == np.isnan(r)).all(), what
    with np.errstate(all="ignore"):
        d = np.where(np.isnan(r) | (g == r), 0.0, np.abs(g - r))
    print(what, "max |device - ref64| %.3e, measured on the reference %.3e" % (float(d.max()), worst))
    assert (d <= 8.0 * worst).all(), (what, float(d.max()), worst)


# =====================================================================================================
# without a GPU
# =====================================================================================================
def test_header_declares_and_package_exports_the_display_transform(pkg):
    header = open(os.path.join(pkg.REPO_DIR, "include", "ptx.h")).read()
    decls = {
        "ptx_grade": r"PTX_API int ptx_grade\(PtxRenderer \*r, const PtxGradeDesc \*d, uint32_t toneMappingMode\);",
        "ptx_grade_lut": r"PTX_API int ptx_grade_lut\(PtxRenderer \*r, uint32_t size, const float \*rgb /\* size\^3 \* 3, red fastest; NULL clears \*/\);",
        "ptx_present_graded": r"PTX_API int ptx_present_graded\(PtxRenderer \*r, const PtxPresentDesc \*desc\);",
    }
    lib = pkg.load_hip()
    for name, decl in decls.items():
        assert re.search(decl, header), name
        assert name in pkg.PTX_SYMBOLS and hasattr(lib, name), name
    assert "#define PTX_ABI_VERSION 5u" in header and "PTX_FN_COUNT = 38" in header  # additions only
    body = re.search(r"typedef struct PtxGradeDesc \{(.*?)\} PtxGradeDesc;", header, re.S)[1]
    fields = re.findall(r"(\w+)(?:\[\d\])?[,;]", re.sub(r"/\*.*?\*/", "", body))
    assert fields == ["colourMatrix", "slope", "offset", "power", "saturation", "curve", "whitePoint", "flags", "reserved"]
    D = pkg.GradeDesc
    assert C.sizeof(D) == 92 and [getattr(D, f).offset for f in fields] == [0, 36, 48, 60, 72, 76, 80, 84, 88]
    for k, name in enumerate(("REFERENCE", "REINHARD", "HABLE", "ACES_FIT")):
        assert re.search(r"PTX_CURVE_%s = %d\b" % (name, k), header) and getattr(pkg, "CURVE_" + name) == k == getattr(R, "CURVE_" + name)
    assert re.search(r"PTX_GRADE_USE_LUT = 1u", header) and re.search(r"PTX_GRADE_LUT_SRGB_DOMAIN = 2u", header)
    assert (pkg.GRADE_USE_LUT, pkg.GRADE_LUT_SRGB_DOMAIN) == (1, 2) == (R.USE_LUT, R.LUT_SRGB_DOMAIN)
    assert (pkg.GRADE_LUT_MIN_SIZE, pkg.GRADE_LUT_MAX_SIZE) == (2, 65)
    # the constants are written once, in the header, and the reference repeats them
    for name, value in [("PTX_HABLE_" + k, v) for k, v in R.HABLE.items()] + [("PTX_HABLE_EXPOSURE_BIAS", R.HABLE_EXPOSURE_BIAS), ("PTX_HABLE_WHITE", R.HABLE_WHITE),
                                                                              ("PTX_ACES_A", R.ACES_A), ("PTX_ACES_B", R.ACES_B), ("PTX_ACES_C", R.ACES_C),
                                                                              ("PTX_ACES_D", R.ACES_D), ("PTX_ACES_E", R.ACES_E)]:
        m = re.search(r"#define %s ([0-9.]+)f\b" % name, header)
        assert m and float(m[1]) == value, name
    for name, value in (("PTX_ACES_IN", R.ACES_IN), ("PTX_ACES_OUT", R.ACES_OUT)):
        m = re.search(r"#define %s \{([^}]*)\}" % name, header)
        assert m and tuple(float(t.strip().rstrip("f")) for t in m[1].split(",")) == value, name
    kernel = open(os.path.join(pkg.PKG_DIR, "csrc", "pt_grade.hpp")).read()
    assert "0.15f" not in kernel and "0.59719" not in kernel and "PTX_HABLE_A" in kernel and "PTX_ACES_IN" in kernel
    for name in ("k_compose_grade", "k_present_graded", "gradePixel"):
        assert name in kernel, name
    # the semantics are in the header as text: the reference is written from it
    for phrase in ("Display transform", "section 22", "0. COMPOSITION", "1. MATRIX", "c'_i = (m[3i] c.x + m[3i+1] c.y) + m[3i+2] c.z", "2a. SLOPE, OFFSET",
                   "2b. POWER", "2c. SATURATION", "Y + (v_k - Y) saturation", "3. CURVE", "v = (v (1 + v / (w w))) / (1 + v)", "f(2 v) / f(11.2)",
                   "(x (A x + C B) + D E) / (x (A x + B) + D F) - E / F", "4. LUT", "i_k = min((int)floor(s_k), N - 2)", "f_r >= f_g:  f_g >= f_b -> rgb",
                   "f_b >= f_g -> bgr", "((V000 (1 - f_hi) + V_a (f_hi - f_mid)) + V_b (f_mid - f_lo)) + V111 f_lo", "5. STORE", "SKIP RULE",
                   "the identity bit for bit", "ptx_resize keeps it, and the LUT", "PTX_GRADE_LUT_SRGB_DOMAIN without PTX_GRADE_USE_LUT",
                   "with no LUT set", "no accepted ptx_grade on this handle yet", "no AgX", "not dithered", "no local tone mapping", "sharded frames are refused"):
        assert phrase in header, phrase
    for method in ("grade", "set_lut", "present_graded"):
        assert callable(getattr(pkg.Renderer, method))
    assert callable(pkg.read_cube) and callable(pkg.white_balance_matrix)
    assert set(pkg.GRADE_DEFAULTS) == set(R.IDENTITY) and all(pkg.GRADE_DEFAULTS[k] == R.IDENTITY[k] for k in R.IDENTITY)
    host_header = open(os.path.join(pkg.REPO_DIR, "include", "ptx_host.h")).read()
    host = pkg.load_host()
    for name in ("pth_read_cube", "pth_white_balance_matrix"):
        assert name in host_header and name in pkg.PTH_SYMBOLS and hasattr(host, name), name
    adapter_h = open(os.path.join(pkg.PKG_DIR, "host", "RendererHip.h")).read()
    m = re.search(r"struct GradeSettings\s*\{\s*bool Enabled = false;\s*uint32_t Curve = (\d+);[^\n]*\n\s*float WhitePoint = ([0-9.]+)f;\s*float TemperatureKelvin = 0.0f;\s*"
                  r"float Slope\[3\] = \{ 1.0f, 1.0f, 1.0f \};\s*float Offset\[3\] = \{ 0.0f, 0.0f, 0.0f \};\s*float Power\[3\] = \{ 1.0f, 1.0f, 1.0f \};\s*"
                  r"float Saturation = 1.0f;\s*std::string LutFile;\s*bool LutSrgbDomain = false;\s*\};", adapter_h)
    assert m and int(m[1]) == pkg.GRADE_DEFAULTS["curve"] and float(m[2]) == pkg.GRADE_DEFAULTS["white_point"]
    adapter = open(os.path.join(pkg.PKG_DIR, "host", "RendererHip.cpp")).read()
    for call in ("ptx_grade(s_Renderer", "ptx_grade_lut(s_Renderer", "ptx_present_graded(s_Renderer"):
        assert call in adapter, call
    example = open(os.path.join(pkg.REPO_DIR, "examples", "render_scene.cpp")).read()
    for option in ("--curve", "--lut", "--temperature"):
        assert option in example, option


def test_known_answers_of_the_curves():
    for dtype in (np.float32, np.float64):
        one_ulp = np.finfo(dtype).eps
        for w in (0.5, 1.0, 4.0, 11.0):  # Reinhard at v = w: w (1 + 1 / w) / (1 + w) = 1
            assert abs(float(R.curve_reinhard(dtype(w), w, dtype)) - 1.0) <= one_ulp, (dtype, w)
        assert float(R.curve_reinhard(dtype(0.0), 4.0, dtype)) == 0.0
        # Hable at 2 v = 11.2: f / f.  v = 5.6f doubles to the float literal 11.2f exactly
        v = dtype(np.float32(5.6))
        assert dtype(np.float32(2.0)) * v == dtype(np.float32(11.2))
        assert float(R.curve_hable(v, dtype)) == 1.0
        assert abs(float(R.curve_hable(dtype(0.0), dtype))) <= 4 * one_ulp  # f(0) = D E / (D F) - E / F
        zero = R.curve_aces_fit(np.zeros((1, 3), dtype), dtype)
        assert (zero == 0).all()  # (0 - B) / E < 0 on every channel, rows of positive sums, clamped
        grey = R.curve_aces_fit(np.repeat(np.linspace(0.05, 4.0, 64).astype(dtype)[:, None], 3, axis=1), dtype)
        assert np.abs(grey - grey[:, :1]).max() <= 2e-5  # greys stay grey ...
    for rows in (R.ACES_IN, R.ACES_OUT):  # ... because every row of both matrices sums to 1
        for i in range(3):  # in decimal: the output matrix' last row sums to 0.99999 exactly, which binary arithmetic puts a hair beyond the bound
            assert abs(sum(Decimal(repr(v)) for v in rows[3 * i:3 * i + 3]) - 1) <= Decimal("1e-5"), (rows, i)
    assert float(R.curve_reference(np.float64(0.0), np.float64)) == 0.0 and abs(float(R.curve_reference(np.float64(1.0), np.float64)) - (1 - np.exp(-1))) < 1e-15


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_every_curve_is_monotone_on_4096_greys(dtype):
    g = np.linspace(0.0, 16.0, 4096).astype(dtype)
    grey = np.repeat(g[:, None], 3, axis=1)
    curves = {"reference": R.curve_reference(grey, dtype), "reinhard": R.curve_reinhard(grey, 4.0, dtype), "hable": R.curve_hable(grey, dtype),
              "aces": R.curve_aces_fit(grey, dtype)}
    for name, v in curves.items():
        d = np.diff(v.astype(np.float64), axis=0)
        # float32: a step down of one rounding where the curve is flat is not a turn
        assert (d >= (-2.0 * np.finfo(np.float32).eps if dtype == np.float32 else 0.0)).all(), (name, float(d.min()))
        assert v[-1, 0] > v[0, 0] and v[2048, 0] > v[16, 0], name
        out = R.grade(grey, curve=getattr(R, "CURVE_" + {"reference": "REFERENCE", "reinhard": "REINHARD", "hable": "HABLE", "aces": "ACES_FIT"}[name]), dtype=dtype)
        assert (np.diff(out[..., 0].astype(np.float64)) >= 0).all(), name  # and the binary16 image never steps down


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_lut_lattice_points_ties_and_the_identity_lattice(dtype):
    for n in (2, 3, 5, 17):
        lut = _lut(n)
        g = (np.arange(n) / (n - 1)).astype(dtype) if dtype == np.float64 else (np.arange(n, dtype=np.float32) * (np.float32(1) / np.float32(n - 1)))
        pts = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)  # [:, 0] red
        idx = np.stack(np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij"), axis=-1).reshape(-1, 3)
        i, f = R.lut_coordinates(pts, n, dtype)
        exact = (pts * dtype(n - 1) == idx).all(axis=1)  # k / (N - 1) * (N - 1) is k again for most k
        assert exact.mean() > 0.5 and exact[0] and exact[-1]
        got = R.lut_lookup(pts, lut, False, dtype)
        want = lut[idx[:, 2], idx[:, 1], idx[:, 0]].astype(dtype)
        assert (got[exact] == want[exact]).all(), n  # a lattice point returns its entry exactly
        if n == 2:
            assert (i == 0).all()  # one cell: every index is 0, x = 1 has fraction 1
    # the branch of a tie, per the header's order; V_a and V_b told apart by a LUT whose entry is its own lattice coordinate plus a mark
    n = 3
    lut = np.zeros((n, n, n, 3), np.float32)
    bb, gg, rr = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
    lut[..., 0] = rr + 10 * gg + 100 * bb
    cell = lambda r, g, b: np.float64(r + 10 * g + 100 * b)  # noqa: E731
    q = dtype(0.25)  # 0.25 * 2 = 0.5: fractions (0.5, 0.5, 0.5) etc. are exact
    ties = {
        (q, q, q): ("rgb", [cell(0, 0, 0) * 0.5, 0.0, 0.0, cell(1, 1, 1) * 0.5]),           # all equal: r >= g, g >= b
        (q, q, 0.0): ("rgb", [cell(0, 0, 0) * 0.5, 0.0, cell(1, 1, 0) * 0.5, 0.0]),         # f_r = f_g > f_b
        (q, q, 0.375): ("brg", [cell(0, 0, 0) * 0.25, cell(0, 0, 1) * 0.25, 0.0, cell(1, 1, 1) * 0.5]),  # f_r = f_g < f_b: r >= g, not g >= b, not r >= b
        (0.0, q, q): ("bgr", [cell(0, 0, 0) * 0.5, 0.0, cell(0, 1, 1) * 0.5, 0.0]),         # f_g = f_b > f_r: not r >= g, b >= g
        (q, 0.0, q): ("rbg", [cell(0, 0, 0) * 0.5, 0.0, cell(1, 0, 1) * 0.5, 0.0]),         # f_r = f_b > f_g: r >= g, not g >= b, r >= b
        (1.0, 1.0, 1.0): ("rgb", [0.0, 0.0, 0.0, cell(2, 2, 2)]),                           # x = 1: index N - 2, fraction 1
        (1.0, 0.5, 0.0): ("rgb", [0.0, cell(2, 1, 0), 0.0, 0.0]),
    }
    for x, (order, terms) in ties.items():
        x = np.asarray([x], dtype)
        i, f = R.lut_coordinates(x, n, dtype)
        assert R.ORDERS[int(R.lut_order(f)[0])] == order, (x, order)
        assert float(R.lut_lookup(x, lut, False, dtype)[0, 0]) == ((terms[0] + terms[1]) + terms[2]) + terms[3], (x, order)
    i, f = R.lut_coordinates(np.asarray([[1.0, 1.0, 1.0]], dtype), n, dtype)
    assert (i == n - 2).all() and (f == 1).all()
    # an identity lattice returns its input: the weights sum to 1 and the corners differ by the cell's size
    rng = np.random.default_rng(7)
    x = rng.uniform(0, 1, (4096, 3)).astype(dtype)
    for n in (2, 17, 65):
        g = np.arange(n, dtype=np.float64) / (n - 1)
        ident = np.stack(np.broadcast_arrays(g[None, None, :], g[None, :, None], g[:, None, None]), axis=-1).astype(np.float32)
        err = np.abs(R.lut_lookup(x, ident, False, dtype).astype(np.float64) - x).max()
        assert err <= 4 * np.finfo(np.float32).eps, (n, err)  # the table itself is float32 in both instances
    err = np.abs(R.lut_lookup(x, _ident(17), True, dtype).astype(np.float64) - x).max()  # and through the sRGB domain, where pow goes there and back
    assert err <= 2e-6, err


def _ident(n):
    g = np.arange(n, dtype=np.float64) / (n - 1)
    return np.stack(np.broadcast_arrays(g[None, None, :], g[None, :, None], g[:, None, None]), axis=-1).astype(np.float32)


def test_the_skip_rule_is_bit_for_bit():
    ident = R.IDENTITY
    run = lambda **kw: R.steps_that_run(**{**{k: ident[k] for k in ("colour_matrix", "slope", "offset", "power", "saturation")}, "mode": R.SDR, "flags": 0, **kw})  # noqa: E731
    assert not any(run()[k] for k in ("matrix", "slope_offset", "power", "saturation", "lut")) and run()["curve"]
    assert run(offset=(0.0, -0.0, 0.0))["slope_offset"] and run(slope=(1.0, np.nextafter(np.float32(1), np.float32(2)), 1.0))["slope_offset"]
    assert run(colour_matrix=(1, 0, 0, 0, 1, 0, 0, -0.0, 1))["matrix"] and run(power=(1, 1, 2))["power"] and run(saturation=0.0)["saturation"]
    assert not run(mode=R.HDR, flags=R.USE_LUT)["curve"] and not run(mode=R.HDR, flags=R.USE_LUT)["lut"] and run(flags=R.USE_LUT)["lut"]
    # an identity desc leaves negatives alone (step 2a's max does not run) and is the reference curve, then binary16
    c = np.float32([[-0.5, 0.25, 2.0]])
    assert (R.grade(c, dtype=np.float64)[0, :3] == (1 - np.exp(-np.float64(c[0]))).astype(np.float16)).all()
    assert (R.grade(c, mode=R.HDR)[0, :3] == c[0]).all()
    assert R.grade(c, slope=(1, 1, 1), offset=(0.0, -0.0, 0.0), mode=R.HDR)[0, 0] == 0  # -0 is not the identity: the max runs
    assert (R.compose(np.float32([1, 2, 3]), np.float32([10, 10, 10]), 0.35) == np.float32([1.35, 2.35, 3.35]).astype(np.float16)).all()


def test_white_balance_matrix_turns_the_source_white(pkg):
    def xyz(x, y):
        return np.float64([x / y, 1.0, (1 - x - y) / y])

    prim = np.stack([xyz(0.64, 0.33), xyz(0.30, 0.60), xyz(0.15, 0.06)], axis=1)
    white = xyz(0.3127, 0.3290)
    rgb_to_xyz = prim * np.linalg.solve(prim, white)[None, :]
    assert np.abs(rgb_to_xyz @ np.ones(3) - white).max() < 1e-14
    for T in (2000, 2856, 4500, 5000, 6504, 9000, 12000):
        u = (0.860117757 + 1.54118254e-4 * T + 1.28641212e-7 * T * T) / (1 + 8.42420235e-4 * T + 7.08145163e-7 * T * T)
        v = (0.317398726 + 4.22806245e-5 * T + 4.20481691e-8 * T * T) / (1 - 2.89741816e-5 * T + 1.61456053e-7 * T * T)
        x, y = 3 * u / (2 * u - 8 * v + 4), 2 * v / (2 * u - 8 * v + 4)
        source = np.linalg.solve(rgb_to_xyz, xyz(x, y))  # the linear-sRGB colour of the T-kelvin source
        m = pkg.white_balance_matrix(T)
        assert m.shape == (3, 3) and m.dtype == np.float32
        out = m.astype(np.float64) @ source
        assert np.abs(out - out[0]).max() <= 1e-5 and abs(out[0] - 1.0) <= 1e-5, (T, out)
        assert source[0] > source[2] if T <= 5000 else source[0] < source[2] if T >= 9000 else True  # a warm source is red-heavy, a cold one blue-heavy
    assert abs(x - 0.3127) > 1e-3  # 12000 K is not D65 ...
    d65 = pkg.white_balance_matrix(6504)
    assert np.abs(d65 - np.eye(3)).max() < 0.05  # ... and 6504 K nearly is
    assert (pkg.white_balance_matrix(0).view(np.uint32) == np.eye(3, dtype=np.float32).view(np.uint32)).all()  # the identity, which the grade skips
    for bad in (-1.0, 500.0, 20000.0, float("nan")):
        with pytest.raises(pkg.PtxError):
            pkg.white_balance_matrix(bad)


def _write_cube(path, lut, title="look", extra="", rows=None):
    n = lut.shape[0]
    flat = lut.reshape(-1, 3)
    with open(path, "w") as f:
        f.write("# a comment\nTITLE \"%s\"\n\nLUT_3D_SIZE %d\nDOMAIN_MIN 0.0 0.0 0.0\nDOMAIN_MAX 1.0 1.0 1.0\n%s" % (title, n, extra))
        for row in flat[:len(flat) if rows is None else rows]:
            f.write("%.9g %.9g %.9g\n" % tuple(row))
    return str(path)


def test_cube_reader(pkg, tmp_path):
    lut = _lut(5)
    got = pkg.read_cube(_write_cube(tmp_path / "ok.cube", lut))
    assert got.shape == (5, 5, 5, 3) and got.dtype == np.float32 and (got.view(np.uint32) == lut.view(np.uint32)).all()  # %.9g round-trips float32
    assert got[0, 0, 1, 0] == lut[0, 0, 1, 0] and (got[0, 0, 1] != got[1, 0, 0]).any()  # red fastest: [blue, green, red]
    assert (pkg.read_cube(_write_cube(tmp_path / "crlf.cube", lut, extra="# more\r\n")) == lut).all()
    bad = {
        "truncated": _write_cube(tmp_path / "t.cube", lut, rows=124),
        "one row too many": _write_cube(tmp_path / "m.cube", lut, extra="0 0 0\n"),
        "non-numeric": _write_cube(tmp_path / "n.cube", lut, extra="0.1 abc 0.3\n", rows=124),
        "two numbers": _write_cube(tmp_path / "2.cube", lut, extra="0.1 0.2\n", rows=124),
        "four numbers": _write_cube(tmp_path / "4.cube", lut, extra="0.1 0.2 0.3 0.4\n", rows=124),
        "not finite": _write_cube(tmp_path / "f.cube", lut, extra="0.1 nan 0.3\n", rows=124),
        "1-D": _write_cube(tmp_path / "1.cube", lut, extra="LUT_1D_SIZE 16\n"),
        "size twice": _write_cube(tmp_path / "s.cube", lut, extra="LUT_3D_SIZE 5\n"),
        "other domain": _write_cube(tmp_path / "d.cube", lut, extra="DOMAIN_MAX 2 2 2\n"),
        "missing": str(tmp_path / "nothing.cube"),
    }
    for name, text in (("oversized", "LUT_3D_SIZE 66\n"), ("size 1", "LUT_3D_SIZE 1\n0 0 0\n"), ("fractional size", "LUT_3D_SIZE 2.5\n"), ("no size", "0 0 0\n"),
                       ("huge", "LUT_3D_SIZE 100000\n0 0 0\n"), ("empty", "")):
        p = tmp_path / (name.replace(" ", "_") + ".cube")
        p.write_text(text)
        bad[name] = str(p)
    for name, path in bad.items():
        with pytest.raises(pkg.PtxError):
            pkg.read_cube(path)
        size = C.c_uint32(77)
        assert pkg.load_host().pth_read_cube(path.encode(), C.byref(size), None, 0) == INVALID, name
    # a buffer of the wrong size is refused, not overrun
    ok, size, small = str(tmp_path / "ok.cube").encode(), C.c_uint32(0), np.zeros(5 * 5 * 5 * 3 - 3, np.float32)
    assert pkg.load_host().pth_read_cube(ok, C.byref(size), small.ctypes.data, small.size) == INVALID and size.value == 5 and not small.any()


def test_reference_float32_against_float64(orc):
    """The measured figures behind every tolerance, recomputed: within a factor of 1.5 of the constants.  And the inputs are what the
    GPU tests assume."""
    assert set(REF_F32_VS_F64) == set(AGAINST_F64)
    for case in AGAINST_F64:
        got, want = _measure(orc, case), REF_F32_VS_F64[case]
        print(case, "max %.3e" % got)
        assert want > 0 and want / 1.5 <= got <= want * 1.5, (case, got, want)
    assert set(REF_PRESENT_F32_VS_F64) == set(PRESENT_CASES)
    for key in PRESENT_CASES:
        got, want = _gap(_present_ref(orc, *key, np.float32)[..., :3], _present_ref(orc, *key, np.float64)[..., :3]), REF_PRESENT_F32_VS_F64[key]
        print(key, "max %.3e" % got)
        assert want > 0 and want / 1.5 <= got <= want * 1.5, (key, got, want)
    for frame, (w, h, _) in FRAMES.items():
        c = _composed(orc, frame)[..., :3]
        if w * h == 1:
            assert (c == 1).all()
            continue
        assert np.isnan(c).any() == (frame == "300x200") and not np.isnan(c).all(axis=-1).mean() > 0.2  # the 10^6 pixel and its bloom
        assert (c[..., 0] >= 4096).any() and (c[..., 1] >= 4096).any() and (c > 1).any()  # the markers, highlights
        assert (c < 0).any() or FRAMES[frame][2] > 0  # a negative channel, where no bloom lifts it
        if FRAMES[frame][2] == 0.0:
            flat = c.reshape(-1, 3)
            for s in [s for s in SPECIALS[:w * h] if np.isfinite(s).all() and max(s) < 1e5]:
                assert (flat == np.float32(s).astype(np.float16)).all(axis=1).any(), (frame, s)
    # what reaches the LUT in the lattice cases: interior lattice points, ties of two and of three fractions, x = 1, every order
    for n in (3, 17, 33, 65):
        for frame in ("5x3", "33x22"):
            v = R.curve_reinhard(_composed(orc, frame)[..., :3].astype(np.float32), 1e4, np.float32).reshape(-1, 3)
            i, f = R.lut_coordinates(R._clamp01(v, np.float32), n, np.float32)
            ok = ~np.isnan(f).any(axis=1)
            assert ((f == 0).all(axis=1) & (i > 0).all(axis=1) & ok).any(), (n, frame)           # the grey of 1 -> 0.5
            assert ((f[:, 0] == f[:, 1]) & (f[:, 1] == f[:, 2]) & (f[:, 0] > 0) & (f[:, 0] < 1)).any() or n == 3
            assert ((f[:, 0] == f[:, 1]) & (f[:, 1] != f[:, 2]) & ok).any() and ((f[:, 1] == f[:, 2]) & (f[:, 0] != f[:, 1]) & ok).any()
            top = R.lut_coordinates(R.curve_aces_fit(_composed(orc, frame)[..., :3].astype(np.float32), np.float32).reshape(-1, 3), n, np.float32)
            assert ((top[1] == 1) & (top[0] == n - 2)).any()                                     # x = 1, where a curve saturates: the ACES cases
            # the order of the fractions is not the order of the channels once they fall into different cells: all six on the ramp, most on 15 pixels
            assert len(set(np.unique(R.lut_order(f)[ok]))) >= (6 if frame == "33x22" else 4), (n, frame)


# =====================================================================================================
# on the GPU
# =====================================================================================================
_handles = {}


def _fresh(pkg, frame, tone=0):
    import torch  # noqa: F401  (first, so the HIP library shares torch's HIP runtime)

    acc = _acc(frame)
    r = pkg.Renderer()
    r.resize(acc.shape[1], acc.shape[0])
    r.write_accumulation(acc)
    r.postprocess(SAMPLES, tone_mapping=tone, **_post(frame))
    return r


def _handle(pkg, frame):
    """One renderer per frame, its sum written and post-processed once."""
    if frame not in _handles:
        _handles[frame] = _fresh(pkg, frame)
    return _handles[frame]


def _kwargs(case):
    """Renderer.grade's arguments for a case."""
    _, n, mode, fields = CASES[case]
    kw = {k: v for k, v in fields.items() if k != "flags"}
    flags = fields.get("flags", 0)
    return dict(kw, tone_mapping=mode, use_lut=bool(flags & R.USE_LUT), lut_srgb_domain=bool(flags & R.LUT_SRGB_DOMAIN))


def _grade(pkg, r, case):
    n = CASES[case][1]
    if n is not None:
        r.set_lut(_lut(n))
    r.grade(**_kwargs(case))
    return r.read_output(pkg.OUTPUT_RGBA32F)


@pytest.mark.gpu
@pytest.mark.parametrize("frame", list(FRAMES))
def test_identity_desc_is_postprocess_and_step_0_is_the_oracle_s(pkg, orc, frame):
    r = _fresh(pkg, frame)
    for mode in (0, 1):
        r.postprocess(SAMPLES, tone_mapping=mode, **_post(frame))
        lin, srgb = r.read_output(pkg.OUTPUT_RGBA32F), r.read_output(pkg.OUTPUT_RGBA8_SRGB)
        if mode == 1:
            assert _same(lin, _composed(orc, frame)).all()  # step 0 of every reference below
        r.postprocess(SAMPLES, tone_mapping=1 - mode, **_post(frame))  # outLinear now holds the other mode's image
        r.grade(tone_mapping=mode)
        assert _same(r.read_output(pkg.OUTPUT_RGBA32F), lin).all(), mode
        assert (r.read_output(pkg.OUTPUT_RGBA8_SRGB) == srgb).all(), mode
    r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("frame", list(FRAMES))
@pytest.mark.parametrize("case", EXACT)
def test_grade_equals_the_float32_reference_bit_for_bit(pkg, orc, case, frame):
    got = _grade(pkg, _handle(pkg, frame), case)
    ref = _ref(orc, case, frame, np.float32)
    same = _same(got, ref)
    assert same.all(), (case, frame, int((~same).sum()), got[~same.all(axis=-1)][:4], ref[~same.all(axis=-1)][:4])


@pytest.mark.gpu
@pytest.mark.parametrize("frame", list(FRAMES))
@pytest.mark.parametrize("case", AGAINST_F64)
def test_grade_against_the_float64_reference(pkg, orc, case, frame):
    got = _grade(pkg, _handle(pkg, frame), case)
    _assert_close_to_float64(got, _ref(orc, case, frame, np.float64), REF_F32_VS_F64[case], (case, frame))


PAIRS = [("R8G8B8A8_SRGB", 0), ("B8G8R8A8_SRGB", 0), ("A2B10G10R10_UNORM", 1), ("R16G16B16A16_SFLOAT", 0), ("R16G16B16A16_SFLOAT", 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("fmt,hdr", PAIRS)
def test_present_graded_under_an_identity_desc_is_present(pkg, fmt, hdr):
    import test_present as TP

    r = _handle(pkg, "67x45")
    r.grade(tone_mapping=hdr)
    f = getattr(pkg, "PRESENT_" + fmt)
    for sw, sh, ui in ((67, 45, False), (100, 37, True), (134, 90, True), (1, 1, False)):
        image = TP._ui(sw, sh) if ui else None
        r.present(sw, sh, f, hdr, image)
        want = r.read_present()
        r.present_graded(sw, sh, f, hdr, image)
        got = r.read_present()
        assert got.dtype == want.dtype and (got.view(np.uint8) == want.view(np.uint8)).all(), (fmt, hdr, sw, sh)


@pytest.mark.gpu
def test_present_graded_follows_the_graded_image_in_every_format(pkg, orc):
    """At the frame's own size and without a UI the screen image is ptx_grade's: R16G16B16A16 its binary16 bits, the 8-bit formats
    ptx_read_output's sRGB8 image; under the UI and scaled, the packed formats are encodings of the device's own R16G16B16A16 image."""
    import test_present as TP

    r = _handle(pkg, "67x45")
    lin = _grade(pkg, r, "matrix_cdl_aces_lut17")
    srgb = r.read_output(pkg.OUTPUT_RGBA8_SRGB)
    assert (srgb == orc.encode_output(lin, 0)).all()  # ptx_read_output(RGBA8_SRGB) follows the graded image
    r.present_graded(67, 45, pkg.PRESENT_R16G16B16A16_SFLOAT, 0)
    half = r.read_present()
    assert _same(half.astype(np.float32), lin).all()
    r.present_graded(67, 45, pkg.PRESENT_R8G8B8A8_SRGB, 0)
    assert (r.read_present() == srgb).all()
    r.present_graded(67, 45, pkg.PRESENT_B8G8R8A8_SRGB, 0)
    assert (r.read_present() == srgb[..., [2, 1, 0, 3]]).all()
    r.present(67, 45, pkg.PRESENT_R8G8B8A8_SRGB, 0)
    assert (r.read_present() != srgb).any()  # and the plain call still shows the ungraded frame
    ui = TP._ui(100, 37)
    r.present_graded(100, 37, pkg.PRESENT_R16G16B16A16_SFLOAT, 0, ui)
    sdr = r.read_present().astype(np.float32)
    want = orc.encode_output(sdr, 0)
    r.present_graded(100, 37, pkg.PRESENT_R8G8B8A8_SRGB, 0, ui)
    assert (r.read_present() == want).all()
    r.present_graded(100, 37, pkg.PRESENT_B8G8R8A8_SRGB, 0, ui)
    assert (r.read_present() == want[..., [2, 1, 0, 3]]).all()
    r.present_graded(100, 37, pkg.PRESENT_R16G16B16A16_SFLOAT, 1, ui)
    hdr = r.read_present().astype(np.float32)
    r.present_graded(100, 37, pkg.PRESENT_A2B10G10R10_UNORM, 1, ui)
    assert (r.read_present() == PR.pack_a2b10g10r10(hdr)).all()
    # the HDR mode skips the curve and the LUT on the screen path too: the kept desc without them gives the same image
    kw = dict(_kwargs("matrix_cdl_aces_lut17"), tone_mapping=1)
    r.grade(**dict(kw, use_lut=False, curve=R.CURVE_REFERENCE))
    r.present_graded(100, 37, pkg.PRESENT_R16G16B16A16_SFLOAT, 1, ui)
    assert (r.read_present().view(np.uint16) == hdr.astype(np.float16).view(np.uint16)).all()


@pytest.mark.gpu
@pytest.mark.parametrize("case,sw,sh", PRESENT_CASES)
def test_present_graded_against_float64(pkg, orc, case, sw, sh):
    r = _handle(pkg, "67x45")
    _grade(pkg, r, case)
    r.present_graded(sw, sh, pkg.PRESENT_R16G16B16A16_SFLOAT, 0)
    _assert_close_to_float64(r.read_present(), _present_ref(orc, case, sw, sh, np.float64), REF_PRESENT_F32_VS_F64[(case, sw, sh)], (case, sw, sh))


@pytest.mark.gpu
def test_hdr_mode_skips_curve_and_lut_and_two_grades_in_a_row_match_a_fresh_handle(pkg, orc):
    r = _handle(pkg, "33x22")
    r.set_lut(_lut(17))
    a = dict(_kwargs("matrix_cdl_aces_lut17"), tone_mapping=1)
    r.grade(**a)
    with_them = r.read_output(pkg.OUTPUT_RGBA32F)
    r.grade(**dict(a, use_lut=False, curve=R.CURVE_HABLE))
    assert _same(r.read_output(pkg.OUTPUT_RGBA32F), with_them).all()
    r.grade(**dict(a, tone_mapping=0))
    assert not _same(r.read_output(pkg.OUTPUT_RGBA32F), with_them).all()
    # two grades in a row: the second reads the post-process image, not the first one's output
    first = _grade(pkg, r, "cdl_hable")
    second = _grade(pkg, r, "lut33")
    f = _fresh(pkg, "33x22")
    assert _same(_grade(pkg, f, "lut33"), second).all()
    f.close()
    f = _fresh(pkg, "33x22")
    assert _same(_grade(pkg, f, "cdl_hable"), first).all()
    f.close()
    # clearing the LUT: a desc that uses it is refused, the kept desc cannot present, and a new table brings both back
    r.set_lut(None)
    lib = pkg.load_hip()
    assert lib.ptx_present_graded(r.handle, C.byref(pkg.PresentDesc(33, 22, 0, 0, None, 0, 0))) == NOT_READY
    r.set_lut(_lut(33))
    r.present_graded(33, 22, pkg.PRESENT_R16G16B16A16_SFLOAT, 0)
    assert _same(r.read_present().astype(np.float32), second).all()


@pytest.mark.gpu
def test_grade_reads_what_the_denoised_and_the_metered_output_calls_left_and_touches_nothing_else(pkg):
    import torch  # noqa: F401

    w, h, spp = 67, 45, 2
    s = pkg.Scene("texture_test", 0.25)
    a, b = pkg.Renderer(), pkg.Renderer()
    a.upload(s)
    b.share_scene(a)  # b, the borrower, grades; a is the control that never does
    for r in (a, b):
        r.resize(w, h)
        for f in range(spp):
            r.render(s.uniform(w, h, bounces=3, sample_count=1, total_samples=f), s.lights)
        r.render_guides(s.uniform(w, h, bounces=3, sample_count=1, total_samples=spp))
        r.despike()
        r.temporal_accumulate(spp, *s.camera_matrices(w, h))
        r.denoise(spp)
        r.meter(spp)
    post = dict(exposure=1.0, bloom_threshold=0.8, bloom_intensity=0.35)
    kw = _kwargs("matrix_cdl_aces_lut17")
    fields = CASES["matrix_cdl_aces_lut17"][3]
    b.set_lut(_lut(17))
    outputs = []
    for call in (lambda r, mode: r.postprocess_denoised(1, tone_mapping=mode, **post), lambda r, mode: r.postprocess_metered(spp, tone_mapping=mode, **post),
                 lambda r, mode: r.postprocess_despiked(spp, tone_mapping=mode, **post)):
        call(b, 1)
        composed = b.read_output(pkg.OUTPUT_RGBA32F)
        call(b, 0)
        b.grade(**kw)
        got = b.read_output(pkg.OUTPUT_RGBA32F)
        assert _same(got, R.grade(composed, lut=_lut(17), **fields)).all()
        outputs.append(got)
    assert not _same(outputs[0], outputs[1]).all() and not _same(outputs[1], outputs[2]).all()
    b.present_graded(100, 37)
    # the sum, C, T, D, the guides and the meter's state are where they were; the next sample is the control's
    bits = lambda x: np.ascontiguousarray(x).view(np.uint32)  # noqa: E731
    assert (bits(a.readback()) == bits(b.readback())).all() and (bits(a.read_despiked()) == bits(b.read_despiked())).all()
    assert (bits(a.read_denoised()) == bits(b.read_denoised())).all() and (bits(a.read_temporal()) == bits(b.read_temporal())).all()
    for g in range(3):
        assert (bits(a.read_guide(g)) == bits(b.read_guide(g))).all(), g
    ma, mb = a.read_meter(bins=True), b.read_meter(bins=True)
    assert bytes(ma[0]) == bytes(mb[0]) and (ma[1] == mb[1]).all()
    for r in (a, b):
        r.render(s.uniform(w, h, bounces=3, sample_count=1, total_samples=spp), s.lights)
    assert (bits(a.readback()) == bits(b.readback())).all()
    for r in (b, a):
        r.close()
    s.close()


@pytest.mark.gpu
def test_resize_keeps_the_lut_and_the_desc(pkg, orc):
    r = _fresh(pkg, "33x22")
    want = _grade(pkg, r, "matrix_cdl_aces_lut17")
    lib = pkg.load_hip()
    r.resize(67, 45)
    d = pkg.GradeDesc()
    C.memmove(C.byref(d), C.byref(pkg.GradeDesc((C.c_float * 9)(*R.IDENTITY["colour_matrix"]), (C.c_float * 3)(1, 1, 1), (C.c_float * 3)(0, 0, 0), (C.c_float * 3)(1, 1, 1),
                                                1.0, 0, 4.0, 0, 0)), C.sizeof(d))
    assert lib.ptx_grade(r.handle, C.byref(d), 0) == NOT_READY  # nothing post-processed at this extent
    assert lib.ptx_present_graded(r.handle, C.byref(pkg.PresentDesc(33, 22, 0, 0, None, 0, 0))) == NOT_READY
    r.write_accumulation(_acc("67x45"))
    r.postprocess(SAMPLES, **_post("67x45"))
    r.present_graded(67, 45, pkg.PRESENT_R16G16B16A16_SFLOAT, 0)  # the kept desc and the LUT, without a new ptx_grade or ptx_grade_lut
    assert _same(r.read_present().astype(np.float32), _ref(orc, "matrix_cdl_aces_lut17", "67x45", np.float32)).all()
    r.resize(33, 22)
    r.write_accumulation(_acc("33x22"))
    r.postprocess(SAMPLES, **_post("33x22"))
    r.grade(**_kwargs("matrix_cdl_aces_lut17"))  # USE_LUT: the table set before the two ptx_resize
    assert _same(r.read_output(pkg.OUTPUT_RGBA32F), want).all()
    r.close()


def _cube_file(tmp_path):
    return _write_cube(tmp_path / "look.cube", _lut(5))


@pytest.mark.gpu
@pytest.mark.parametrize("with_lut", [0, 1])
def test_renderer_hip_with_grade_settings_on_is_the_same_calls_made_by_hand(pkg, tmp_path_factory, tmp_path, with_lut):
    """test_motion's driver (examples/motion_frame.cpp, compiled once per session) with GradeSettings on -- Hable's curve, 4500 K, a CDL
    grade, with_lut: a .cube file -- on the plain output path: the output image and the presented image of both frames equal
    ptx_postprocess, ptx_grade and ptx_present_graded made by hand, bit for bit, and differ from the ungraded ones."""
    import subprocess

    import test_motion as TM

    w, h, spp, depth, step = 67, 45, 2, 4, 0.37
    exe = TM._motion_frame_driver(pkg, tmp_path_factory)
    dump = tmp_path / "frames.bin"
    subprocess.check_call([exe, "animated_test", str(w), str(h), str(spp), str(depth), str(step), "0", str(dump), "0", "0", "0", "0", "1"] +
                          ([_cube_file(tmp_path)] if with_lut else []))
    raw = np.fromfile(dump, np.uint8)
    got = raw[:2 * 3 * h * w * 16].view(np.float32).reshape(2, 3, h, w, 4)
    screen = raw[2 * 3 * h * w * 16:].reshape(2, 37, 100, 4)
    s = pkg.Scene("animated_test", 0.25)
    s.update(0.0)
    r = pkg.Renderer()
    r.upload(s)
    r.resize(w, h)
    if with_lut:
        r.set_lut(pkg.read_cube(_cube_file(tmp_path)))
    for frame in range(2):
        if frame:
            assert s.update(step)
        it, bn = s.animation_state()
        r.update_animation(it, bn if len(bn) else None)
        r.reset()
        for f in range(spp):
            r.render(s.uniform(w, h, bounces=depth, sample_count=1, total_samples=f), s.lights)
        r.postprocess(spp, 1.0, 1.0, 1.0, pkg.TONE_MAPPING_SDR)
        plain = r.read_output(pkg.OUTPUT_RGBA32F)
        r.grade(colour_matrix=pkg.white_balance_matrix(4500.0), slope=(1.1, 1.0, 1.0), offset=(0.0, 0.01, 0.0), power=(1.0, 1.0, 0.9), saturation=1.2,
                curve=pkg.CURVE_HABLE, use_lut=bool(with_lut))
        out = r.read_output(pkg.OUTPUT_RGBA32F)
        assert _same(got[frame][0], r.readback()).all() and _same(got[frame][2], out).all(), frame
        assert not _same(out, plain).all()
        r.present_graded(100, 37)
        assert (screen[frame] == r.read_present()).all(), frame
    r.close()
    s.close()


@pytest.mark.gpu
def test_renderer_hip_with_grade_settings_off_is_the_plain_path(pkg, tmp_path_factory, tmp_path):
    import subprocess

    import test_motion as TM

    w, h, spp, depth, step = 67, 45, 2, 4, 0.37
    exe = TM._motion_frame_driver(pkg, tmp_path_factory)
    dump = tmp_path / "frames.bin"
    subprocess.check_call([exe, "animated_test", str(w), str(h), str(spp), str(depth), str(step), "0", str(dump), "0", "0", "0", "0", "0"])
    raw = np.fromfile(dump, np.uint8)
    got = raw[:2 * 3 * h * w * 16].view(np.float32).reshape(2, 3, h, w, 4)
    screen = raw[2 * 3 * h * w * 16:].reshape(2, 37, 100, 4)
    s = pkg.Scene("animated_test", 0.25)
    s.update(0.0)
    r = pkg.Renderer()
    r.upload(s)
    r.resize(w, h)
    for frame in range(2):
        if frame:
            assert s.update(step)
        it, bn = s.animation_state()
        r.update_animation(it, bn if len(bn) else None)
        r.reset()
        for f in range(spp):
            r.render(s.uniform(w, h, bounces=depth, sample_count=1, total_samples=f), s.lights)
        r.postprocess(spp, 1.0, 1.0, 1.0, pkg.TONE_MAPPING_SDR)
        assert _same(got[frame][2], r.read_output(pkg.OUTPUT_RGBA32F)).all(), frame
        r.present(100, 37)
        assert (screen[frame] == r.read_present()).all(), frame
    # a handle that was never graded holds no desc: the graded present call has nothing to apply
    assert pkg.load_hip().ptx_present_graded(r.handle, C.byref(pkg.PresentDesc(100, 37, 0, 0, None, 0, 0))) == NOT_READY
    r.close()
    s.close()


@pytest.mark.gpu
def test_refusals_leave_the_output_the_desc_and_the_lut_intact(pkg):
    import torch

    lib = pkg.load_hip()
    r = _fresh(pkg, "33x22")
    ident = R.IDENTITY

    def desc(**kw):
        f = dict(ident, flags=0, reserved=0)
        f.update(kw)
        return pkg.GradeDesc((C.c_float * 9)(*f["colour_matrix"]), (C.c_float * 3)(*f["slope"]), (C.c_float * 3)(*f["offset"]), (C.c_float * 3)(*f["power"]),
                             f["saturation"], f["curve"], f["white_point"], f["flags"], f["reserved"])

    pd = pkg.PresentDesc(33, 22, pkg.PRESENT_R16G16B16A16_SFLOAT, 0, None, 0, 0)
    # before anything: no desc kept, no LUT
    assert lib.ptx_present_graded(r.handle, C.byref(pd)) == NOT_READY
    assert lib.ptx_grade(r.handle, C.byref(desc(flags=1)), 0) == NOT_READY
    plain = r.read_output(pkg.OUTPUT_RGBA32F)
    assert _same(r.read_output(pkg.OUTPUT_RGBA32F), plain).all()
    want = _grade(pkg, r, "cdl_hable_lut33")
    r.present_graded(33, 22, pkg.PRESENT_R16G16B16A16_SFLOAT, 0)
    shown = r.read_present()

    def intact(what):
        assert _same(r.read_output(pkg.OUTPUT_RGBA32F), want).all(), what                       # the output image
        assert lib.ptx_present_graded(r.handle, C.byref(pd)) == OK, what                        # the kept desc, and the LUT it reads
        assert (r.read_present().view(np.uint16) == shown.view(np.uint16)).all(), what

    nan, inf = float("nan"), float("inf")
    m = list(ident["colour_matrix"])
    bad = {"curve 4": desc(curve=4), "flag bit 4": desc(flags=4), "flags 7": desc(flags=7), "reserved": desc(reserved=1),
           "sRGB domain without a LUT": desc(flags=2), "NaN in the matrix": desc(colour_matrix=m[:4] + [nan] + m[5:]),
           "Inf in the matrix": desc(colour_matrix=m[:8] + [inf]), "NaN slope": desc(slope=(1, nan, 1)), "Inf offset": desc(offset=(0, 0, -inf)),
           "NaN power": desc(power=(nan, 1, 1)), "Inf saturation": desc(saturation=inf), "NaN white point": desc(white_point=nan),
           "negative slope": desc(slope=(1, 1, -0.5)), "negative power": desc(power=(1, -1, 1)), "negative saturation": desc(saturation=-0.1),
           "Reinhard with w = 0": desc(curve=R.CURVE_REINHARD, white_point=0.0), "Reinhard with w < 0": desc(curve=R.CURVE_REINHARD, white_point=-4.0)}
    for what, d in bad.items():
        assert lib.ptx_grade(r.handle, C.byref(d), 0) == INVALID, what
        intact(what)
    assert lib.ptx_grade(r.handle, C.byref(desc()), 2) == INVALID  # an unknown mode
    assert lib.ptx_grade(r.handle, None, 0) == INVALID and lib.ptx_grade(None, C.byref(desc()), 0) == INVALID
    intact("null, mode")
    assert lib.ptx_grade(r.handle, C.byref(desc(white_point=-1.0)), 0) == OK  # the white point is Reinhard's alone
    _grade(pkg, r, "cdl_hable_lut33")
    intact("the same grade again")
    table = _lut(2)
    for size in (0, 1, 66, 1000):
        assert lib.ptx_grade_lut(r.handle, size, table.ctypes.data) == INVALID, size
        intact(("LUT size", size))
    assert lib.ptx_grade_lut(None, 2, table.ctypes.data) == INVALID
    # ptx_present_graded refuses what ptx_present refuses, flag bits 2 and 3 among it
    for d in (pkg.PresentDesc(0, 22, 3, 0, None, 0, 0), pkg.PresentDesc(33, 22, 4, 0, None, 0, 0), pkg.PresentDesc(33, 22, 3, 2, None, 0, 0),
              pkg.PresentDesc(33, 22, 3, 0, None, 2, 0), pkg.PresentDesc(33, 22, 3, 0, None, 3, 0), pkg.PresentDesc(33, 22, 3, 0, None, 0, 1),
              pkg.PresentDesc(33, 22, 0, 1, None, 0, 0), pkg.PresentDesc(33, 22, 2, 0, None, 0, 0)):
        assert lib.ptx_present_graded(r.handle, C.byref(d)) == INVALID, (d.width, d.format, d.toneMappingMode, d.flags, d.reserved)
        assert lib.ptx_present(r.handle, C.byref(d)) == INVALID
    assert lib.ptx_present_graded(r.handle, None) == INVALID
    intact("present refusals")
    # NOT_READY: a LUT desc with the LUT cleared (on a second handle: this one keeps its table), a bound shard buffer, a tile shard of several
    f = _fresh(pkg, "33x22")
    assert lib.ptx_grade(f.handle, C.byref(desc(flags=1)), 0) == NOT_READY and lib.ptx_grade(f.handle, C.byref(desc(flags=3)), 0) == NOT_READY
    assert _same(f.read_output(pkg.OUTPUT_RGBA32F), plain).all()
    f.close()
    r.set_tile_shard(0, 2, 8)
    assert lib.ptx_grade(r.handle, C.byref(desc()), 0) == NOT_READY and lib.ptx_present_graded(r.handle, C.byref(pd)) == NOT_READY
    shard = torch.zeros(r.shard_bytes(0) // 4, dtype=torch.float32, device="cuda")
    r.bind_shard_accumulation(shard.data_ptr(), r.shard_bytes(0))
    assert lib.ptx_grade(r.handle, C.byref(desc()), 0) == NOT_READY and lib.ptx_present_graded(r.handle, C.byref(pd)) == NOT_READY
    r.bind_shard_accumulation(0)
    assert _same(r.read_output(pkg.OUTPUT_RGBA32F), want).all()
    r.close()


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import __graft_entry__ as graft

    o = graft.load_oracle()
    o.build()
    print("REF_F32_VS_F64 = {")
    for name in AGAINST_F64:
        print("    %r: %.3e," % (name, _measure(o, name)))
    print("}")
    print("REF_PRESENT_F32_VS_F64 = {")
    for key in PRESENT_CASES:
        print("    %r: %.3e," % (key, _gap(_present_ref(o, *key, np.float32)[..., :3], _present_ref(o, *key, np.float64)[..., :3])))
    print("}")
