"""The enlarging screen path (include/ptx.h ptx_present_upscaled, csrc/pt_upscale.hpp; docs/NEXT_ROWS.md section 25) against
tests/upscale_ref.py.

Bit-exact legs.  Steps 2 - 5 are polynomial float32 in a written order, so on an R16G16B16A16 SDR surface without a UI the device is
held to float16(toneMapPixel of the oracle on the float32 reference's S), bit for bit, NaN positions included; the device's
toneMapPixel has the oracle's bits (tests/test_transcendentals.py).  The packed surface formats are the encodings of the device's own
R16G16B16A16 image.  A grade without pow is grade_ref's float32 instance on S, bit for bit.

Why not float64.  REF_F32_VS_F64 below is the reference's own float32 instance against its float64 instance of steps 2 - 5.  On the
finite frames the two differ on at most 0.1 % of the values by at most 0.8 % of the value (100 x 68 at sharpness 2; 0.4 % at 201 x 135,
where t sits on an integer in float64 and a rounding beside it in float32, and a weight of 1e-7 meets a 5000-valued marker pixel).  On
the frame whose T holds an Inf, at 201 x 135, 0.9 % of the values differ by up to 0.39 of the value: Inf x 0 is a NaN and becomes lo
where t is exactly 0, Inf x 1e-7 is an infinity and is clamped to lo or hi by its sign.  Both are what the header's text says; neither
instance is at fault, and the device is held to the float32 one.  test_reference_float32_against_float64 recomputes the table without
a GPU.

Tolerance of the UI and HDR10 legs.  present_ref.present (whose blit is the identity at equal extents) is applied to the float32 S
in float64; REF_TAIL_F32_VS_F64 holds, per case, what its float32 instance differs from that by on the binary16 image -- the gap of those
steps alone -- and the device may differ by 8 x that maximum, with a floor of one binary16 step, on at most 4 x that share of the
values: tests/test_present.py's rule.

Print both tables with

    python tests/test_upscale.py

All GPU tests and test_header_declares_and_package_exports_the_upscaled_screen_path fail on the parent commit; the tests of the
reference's properties exercise tests/upscale_ref.py alone."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

import grade_ref as G
import present_ref as R
import test_present as TP
import upscale_ref as U

W, H, SAMPLES, POST = TP.W, TP.H, TP.SAMPLES, TP.POST
SHARPNESS = (0.0, 0.5, 2.0)
# (frame, screen width, screen height): own size (sharpen only), 2 x (5 x 12 tiles), non-integer, one unfiltered axis each way, exact
# thirds (floor sits on integers), one more than the render extent (the widest source footprint of a tile), every tap clamped, 1 x 1
EXTENTS = [("frame", 67, 45), ("frame", 134, 90), ("frame", 100, 68), ("frame", 67, 90), ("frame", 134, 45), ("frame", 201, 135), ("frame", 68, 46),
           ("small", 300, 200), ("one", 5, 3)]
INF_EXTENTS = [("inf", sw, sh) for f, sw, sh in EXTENTS if f == "frame"]
CASES = [(f, sw, sh, s) for (f, sw, sh) in EXTENTS + INF_EXTENTS for s in SHARPNESS]
TAIL_SHARPNESS = 0.5
TAIL_CASES = [(f, sw, sh, ui, hdr) for (f, sw, sh) in EXTENTS for (ui, hdr) in ((False, True), (True, False), (True, True))]
# matrix + slope / offset + saturation + Hable: no pow, no exp
GRADE_NO_POW = dict(colour_matrix=(0.9, 0.1, 0.0, 0.05, 0.9, 0.05, 0.0, 0.2, 0.8), slope=(1.1, 0.9, 1.0), offset=(0.01, -0.02, 0.0), saturation=1.2,
                    curve=G.CURVE_HABLE)

# (frame, screen width, screen height, sharpness) -> (max |S32 - S64| / max(2^-14, |S64|) over the finite values, share of values that differ)
REF_F32_VS_F64 = {
    ('frame', 67, 45, 0.0): (0.000e+00, 0.000e+00),
    ('frame', 67, 45, 0.5): (0.000e+00, 0.000e+00),
    ('frame', 67, 45, 2.0): (0.000e+00, 0.000e+00),
    ('frame', 134, 90, 0.0): (9.643e-04, 1.106e-04),
    ('frame', 134, 90, 0.5): (1.936e-03, 1.382e-04),
    ('frame', 134, 90, 2.0): (2.042e-03, 1.658e-04),
    ('frame', 100, 68, 0.0): (9.443e-04, 4.412e-04),
    ('frame', 100, 68, 0.5): (1.890e-03, 7.843e-04),
    ('frame', 100, 68, 2.0): (7.628e-03, 9.804e-04),
    ('frame', 67, 90, 0.0): (0.000e+00, 0.000e+00),
    ('frame', 67, 90, 0.5): (0.000e+00, 0.000e+00),
    ('frame', 67, 90, 2.0): (0.000e+00, 0.000e+00),
    ('frame', 134, 45, 0.0): (0.000e+00, 0.000e+00),
    ('frame', 134, 45, 0.5): (0.000e+00, 0.000e+00),
    ('frame', 134, 45, 2.0): (0.000e+00, 0.000e+00),
    ('frame', 201, 135, 0.0): (9.737e-04, 4.299e-04),
    ('frame', 201, 135, 0.5): (1.946e-03, 4.054e-04),
    ('frame', 201, 135, 2.0): (3.610e-03, 6.633e-04),
    ('frame', 68, 46, 0.0): (0.000e+00, 0.000e+00),
    ('frame', 68, 46, 0.5): (0.000e+00, 0.000e+00),
    ('frame', 68, 46, 2.0): (0.000e+00, 0.000e+00),
    ('small', 300, 200, 0.0): (2.026e-03, 2.722e-04),
    ('small', 300, 200, 0.5): (4.175e-03, 4.278e-04),
    ('small', 300, 200, 2.0): (4.127e-03, 6.444e-04),
    ('one', 5, 3, 0.0): (0.000e+00, 0.000e+00),
    ('one', 5, 3, 0.5): (0.000e+00, 0.000e+00),
    ('one', 5, 3, 2.0): (0.000e+00, 0.000e+00),
    ('inf', 67, 45, 0.0): (0.000e+00, 0.000e+00),
    ('inf', 67, 45, 0.5): (0.000e+00, 0.000e+00),
    ('inf', 67, 45, 2.0): (0.000e+00, 0.000e+00),
    ('inf', 134, 90, 0.0): (5.035e-04, 2.764e-05),
    ('inf', 134, 90, 0.5): (1.010e-03, 2.764e-05),
    ('inf', 134, 90, 2.0): (1.018e-03, 8.292e-05),
    ('inf', 100, 68, 0.0): (9.033e-04, 5.392e-04),
    ('inf', 100, 68, 0.5): (1.812e-03, 9.314e-04),
    ('inf', 100, 68, 2.0): (2.954e-03, 1.569e-03),
    ('inf', 67, 90, 0.0): (0.000e+00, 0.000e+00),
    ('inf', 67, 90, 0.5): (0.000e+00, 0.000e+00),
    ('inf', 67, 90, 2.0): (0.000e+00, 0.000e+00),
    ('inf', 134, 45, 0.0): (0.000e+00, 0.000e+00),
    ('inf', 134, 45, 0.5): (0.000e+00, 0.000e+00),
    ('inf', 134, 45, 2.0): (0.000e+00, 0.000e+00),
    ('inf', 201, 135, 0.0): (3.856e-01, 3.759e-03),
    ('inf', 201, 135, 0.5): (3.881e-01, 7.727e-03),
    ('inf', 201, 135, 2.0): (3.959e-01, 8.648e-03),
    ('inf', 68, 46, 0.0): (8.071e-04, 1.066e-04),
    ('inf', 68, 46, 0.5): (1.630e-03, 3.197e-04),
    ('inf', 68, 46, 2.0): (2.517e-03, 2.131e-04),
}

# (frame, screen width, screen height, UI, HDR) -> (max |tail32(S32) - tail64(S32)| on the binary16 image, share of values that differ)
REF_TAIL_F32_VS_F64 = {
    ('frame', 67, 45, False, True): (4.883e-04, 4.754e-03),
    ('frame', 67, 45, True, False): (2.441e-04, 1.106e-04),
    ('frame', 67, 45, True, True): (4.883e-04, 5.196e-03),
    ('frame', 134, 90, False, True): (4.883e-04, 4.754e-03),
    ('frame', 134, 90, True, False): (0.000e+00, 0.000e+00),
    ('frame', 134, 90, True, True): (4.883e-04, 4.671e-03),
    ('frame', 100, 68, False, True): (4.883e-04, 4.804e-03),
    ('frame', 100, 68, True, False): (0.000e+00, 0.000e+00),
    ('frame', 100, 68, True, True): (4.883e-04, 4.755e-03),
    ('frame', 67, 90, False, True): (4.883e-04, 4.422e-03),
    ('frame', 67, 90, True, False): (0.000e+00, 0.000e+00),
    ('frame', 67, 90, True, True): (4.883e-04, 4.699e-03),
    ('frame', 134, 45, False, True): (4.883e-04, 4.478e-03),
    ('frame', 134, 45, True, False): (0.000e+00, 0.000e+00),
    ('frame', 134, 45, True, True): (4.883e-04, 5.196e-03),
    ('frame', 201, 135, False, True): (4.883e-04, 5.012e-03),
    ('frame', 201, 135, True, False): (0.000e+00, 0.000e+00),
    ('frame', 201, 135, True, True): (4.883e-04, 5.135e-03),
    ('frame', 68, 46, False, True): (9.766e-04, 5.648e-03),
    ('frame', 68, 46, True, False): (0.000e+00, 0.000e+00),
    ('frame', 68, 46, True, True): (9.766e-04, 6.500e-03),
    ('small', 300, 200, False, True): (9.766e-04, 4.767e-03),
    ('small', 300, 200, True, False): (4.883e-04, 5.556e-06),
    ('small', 300, 200, True, True): (9.766e-04, 4.589e-03),
    ('one', 5, 3, False, True): (0.000e+00, 0.000e+00),
    ('one', 5, 3, True, False): (0.000e+00, 0.000e+00),
    ('one', 5, 3, True, True): (0.000e+00, 0.000e+00),
}


# =====================================================================================================
# inputs and references: computed once, shared, left unchanged
# =====================================================================================================
_once = TP._once
_differs = TP._differs


def _acc(frame):
    def make():
        if frame in ("frame", "small"):
            return TP._acc(frame)
        if frame == "one":
            return np.array([[[0.7 * SAMPLES, 0.4 * SAMPLES, 0.3 * SAMPLES, 1.0]]], np.float32)
        a = TP._acc("frame").copy()  # "inf": a 3 x 3 hot spot beyond the binary16 range once bloom is added
        a[15:18, 33:36, :3] = 60000.0 * SAMPLES
        return a
    return _once(("up-acc", frame), make)


def _composed(orc, frame):
    """Step 1: the HDR mode of the oracle passes composition.comp's store through."""
    return _once(("up-composed", frame), lambda: orc.postprocess(_acc(frame), SAMPLES, tone_mapping=1, **POST))


def _S(orc, frame, sw, sh, sharpness, dtype=np.float32):
    return _once(("up-S", frame, sw, sh, sharpness, np.dtype(dtype).name), lambda: U.screen_image(_composed(orc, frame), sw, sh, sharpness, dtype))


def _tone_mapped(pkg, orc, s):
    """float16(toneMapPixel(S)) through the oracle, as H x W x 3 binary16 bit patterns."""
    fn = pkg.FN["toneMapPixel"]
    rows = np.ascontiguousarray(s, np.float32).reshape(-1, 3)
    out = orc.test_eval(fn, rows.view(np.uint32), 3).view(np.float32)
    with np.errstate(over="ignore"):
        return out.astype(np.float16).view(np.uint16).reshape(s.shape)


def _measure(orc, case):
    f, sw, sh, sharpness = case
    a, b = _S(orc, f, sw, sh, sharpness, np.float32).astype(np.float64), _S(orc, f, sw, sh, sharpness, np.float64)
    fin = np.isfinite(a) & np.isfinite(b)
    with np.errstate(all="ignore"):
        d = np.where(fin, np.abs(a - b) / np.maximum(2.0 ** -14, np.abs(b)), 0.0)
    return float(d.max()), float(_differs(a, b).mean())


def _tail(orc, case, dtype):
    f, sw, sh, ui, hdr = case
    return _once(("up-tail", case, np.dtype(dtype).name),
                 lambda: R.present(_S(orc, f, sw, sh, TAIL_SHARPNESS), TP._ui(sw, sh) if ui else None, sw, sh, hdr, dtype))


def _measure_tail(orc, case):
    a, b = _tail(orc, case, np.float32)[..., :3], _tail(orc, case, np.float64)[..., :3]
    with np.errstate(all="ignore"):
        d = np.abs(a.astype(np.float64) - b)
    return float(np.max(np.where(np.isfinite(d), d, 0.0))), float(_differs(a, b).mean())


# =====================================================================================================
# without a GPU
# =====================================================================================================
def test_header_declares_and_package_exports_the_upscaled_screen_path(pkg):
    header = open(os.path.join(pkg.REPO_DIR, "include", "ptx.h")).read()
    assert re.search(r"PTX_API int ptx_present_upscaled\(PtxRenderer \*r, const PtxPresentDesc \*desc, const PtxUpscaleDesc \*up\);", header)
    assert re.search(r"enum \{ PTX_UPSCALE_CATMULL_ROM = 0 \};", header) and re.search(r"enum \{ PTX_UPSCALE_GRADED = 1u \};", header)
    assert re.search(r"typedef struct PtxUpscaleDesc \{\s*uint32_t filter;[^}]*float\s+sharpness;[^}]*uint32_t flags;[^}]*uint32_t reserved;[^}]*\} PtxUpscaleDesc;", header)
    assert "#define PTX_ABI_VERSION 5u" in header and "PTX_FN_COUNT = 38" in header  # an addition
    for step in ("1. COMPOSED TEXEL", "2. AXIS SET-UP", "3. ROW PASS", "4. COLUMN PASS", "5. SHARPEN", "6. TONE OR GRADE, UI, HDR10, STORE", "SKIP RULE"):
        assert step in header, step
    for weight in ("w0 = ((-0.5f t + 1.0f) t - 0.5f) t", "w1 = ((1.5f t - 2.5f) t) t + 1.0f", "w2 = ((-1.5f t + 2.0f) t + 0.5f) t", "w3 = ((0.5f t - 0.5f) t) t"):
        assert weight in header, weight
    lib = pkg.load_hip()
    assert "ptx_present_upscaled" in pkg.PTX_SYMBOLS and hasattr(lib, "ptx_present_upscaled")
    assert pkg.ABI_VERSION == 5 and pkg.UPSCALE_CATMULL_ROM == 0 and pkg.UPSCALE_GRADED == 1
    d = pkg.UpscaleDesc
    assert C.sizeof(d) == 16 and (d.filter.offset, d.sharpness.offset, d.flags.offset, d.reserved.offset) == (0, 4, 8, 12)
    assert callable(pkg.Renderer.present_upscaled)
    adapter_h = open(os.path.join(pkg.PKG_DIR, "host", "RendererHip.h")).read()
    m = re.search(r"struct UpscaleSettings\s*\{\s*bool Enabled = false;\s*float Sharpness = ([0-9.]+)f;\s*\};", adapter_h)
    assert m and float(m[1]) == pkg.UPSCALE_DEFAULTS["sharpness"] == 0.5
    assert "SetSettings(const UpscaleSettings &settings)" in adapter_h
    adapter = open(os.path.join(pkg.PKG_DIR, "host", "RendererHip.cpp")).read()
    assert "ptx_present_upscaled(s_Renderer" in adapter and "PTX_UPSCALE_GRADED" in adapter
    assert "--upscale" in open(os.path.join(pkg.REPO_DIR, "examples", "render_scene.cpp")).read()
    assert "--upscale" in open(os.path.join(pkg.REPO_DIR, "tools", "screen_path_timing.py")).read()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_reference_axis_and_known_answers(dtype):
    rng = np.random.default_rng(3)
    img = rng.uniform(0, 4, (6, 8, 3)).astype(np.float16).astype(dtype)
    assert U.axis(8, 8, dtype) is None
    # 2 x: t alternates 0.75, 0.25; the weights are Catmull-Rom's and sum to 1; the taps at the edge are clamped
    taps, w = U.axis(8, 16, dtype)
    assert (taps[:, 0] == [0, 0, 0, 1]).all() and (taps[:, 1] == [0, 0, 1, 2]).all() and (taps[:, -1] == [6, 7, 7, 7]).all()
    assert (taps[1, 1:-1] == (np.arange(1, 15) - 1) // 2).all()
    assert np.abs(w.sum(axis=0) - 1).max() <= (1e-6 if dtype == np.float32 else 1e-15)
    assert (w[:, 1] == [dtype(-0.0703125), dtype(0.8671875), dtype(0.2265625), dtype(-0.0234375)]).all()  # t = 0.25, exact in binary
    # exact thirds of 3 x: t = 0 at the texel centres, where the weights are (0, 1, 0, 0) bit for bit in float64's exact thirds or not at all
    taps, w = U.axis(4, 12, dtype)
    assert (taps[1, 1::3] == [0, 1, 2, 3]).all()
    # a constant image is exact, at every extent and sharpness
    const = np.full((6, 8, 3), dtype(np.float16(0.3)))
    for sw, sh in ((8, 6), (16, 12), (11, 7), (8, 13), (24, 18)):
        for k in SHARPNESS:
            assert (U.screen_image(const, sw, sh, k, dtype) == const[0, 0, 0]).all(), (sw, sh, k)
    # own size with sharpness 0 is the identity; an unfiltered axis leaves its lines alone
    assert (U.screen_image(img, 8, 6, 0.0, dtype) == img).all()
    assert (U.enlarge(img, 8, 12, dtype)[:, 3] == U.enlarge(img[:, 3:4], 1, 12, dtype)[:, 0]).all()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_reference_stays_within_the_local_range(orc, dtype):
    """S lies within the range of the four central texels, the sharpened value within the five-tap range of S, on the frame with its
    5000-valued markers and on the frame whose T holds an Inf -- which produces no NaN."""
    for frame, sw, sh in (("frame", 134, 90), ("frame", 100, 68), ("frame", 201, 135), ("inf", 134, 90), ("inf", 100, 68), ("small", 300, 200)):
        t = _composed(orc, frame)[..., :3].astype(dtype)
        assert not np.isnan(t).any() and np.isinf(t).any() == (frame == "inf")
        s = U.enlarge(t, sw, sh, dtype)
        assert not np.isnan(s).any()
        (i, _), (j, _) = U.axis(t.shape[1], sw, dtype), U.axis(t.shape[0], sh, dtype)
        quad = np.stack([t[j[a]][:, i[b]] for a in (1, 2) for b in (1, 2)])
        f16 = lambda x: U._f16(x, dtype)  # noqa: E731
        assert (s >= f16(quad.min(axis=0))).all() and (s <= f16(quad.max(axis=0))).all(), (frame, sw, sh)
        for k in (0.5, 2.0):
            v = U.sharpen(s, k, dtype)
            assert not np.isnan(v).any()
            pad = np.pad(s, ((1, 1), (1, 1), (0, 0)), mode="edge")
            five = np.stack([s, pad[:-2, 1:-1], pad[2:, 1:-1], pad[1:-1, :-2], pad[1:-1, 2:]])
            assert (v >= five.min(axis=0)).all() and (v <= five.max(axis=0)).all(), (frame, sw, sh, k)
            assert (v != s).any()


def test_reference_sharpening_steepens_an_edge_monotonically():
    """A ramp between two plateaus: with growing sharpness every pixel moves away from the local mean and never back, the plateaus
    and the two extremes stay where they are, and nothing leaves [low, high]."""
    dtype = np.float32
    line = np.concatenate([np.full(6, 0.25), np.linspace(0.25, 2.0, 6)[1:-1], np.full(6, 2.0)]).astype(np.float16).astype(dtype)
    img = np.repeat(np.repeat(line[None, :, None], 5, axis=0), 3, axis=2)
    s = U.enlarge(img, 2 * img.shape[1], 5, dtype)
    prev = s
    mid = (s[:, :-2] + s[:, 2:]) / 2
    for k in (0.25, 0.5, 1.0, 2.0):
        v = U.sharpen(s, k, dtype)
        assert v.min() == s.min() and v.max() == s.max()
        assert (v[:, :8] == s[:, :8]).all() and (v[:, -8:] == s[:, -8:]).all()
        above = s[:, 1:-1] > mid
        assert (np.where(above, v[:, 1:-1] >= prev[:, 1:-1], v[:, 1:-1] <= prev[:, 1:-1])).all(), k
        assert (np.diff(v[2, :, 0]) >= 0).all()  # still monotone: no overshoot, no halo
        prev = v
    assert (prev != s).any()


def test_reference_float32_against_float64(orc):
    """The measured figures of the module's docstring, recomputed: within a factor of 1.5 of the constants."""
    assert set(REF_F32_VS_F64) == set(CASES) and set(REF_TAIL_F32_VS_F64) == set(TAIL_CASES)
    for table, measure, cases in ((REF_F32_VS_F64, _measure, CASES), (REF_TAIL_F32_VS_F64, _measure_tail, TAIL_CASES)):
        for case in cases:
            got, want = measure(orc, case), table[case]
            print(case, "max %.3e share %.3e" % got)
            for g, w in zip(got, want):
                assert w / 1.5 <= g <= w * 1.5 if w else g == 0.0, (case, got, want)
    assert max(share for _, share in REF_F32_VS_F64.values()) <= 0.01
    # the inputs are what the GPU tests assume
    for frame in ("frame", "inf", "small"):
        c = _composed(orc, frame)
        assert not np.isnan(c).any() and c[2, 3, 0] >= 4096 and c[4, 5, 1] >= 4096
    assert np.isinf(_composed(orc, "inf")[..., :3]).sum() >= 9 and np.isfinite(_composed(orc, "frame")).all()
    assert _composed(orc, "one").shape == (1, 1, 4)


# =====================================================================================================
# on the GPU
# =====================================================================================================
_handles = {}
_bits16 = TP._bits16


def _fresh(pkg, frame, tone=0):
    import torch  # noqa: F401  (first, so the HIP library shares torch's HIP runtime)

    acc = _acc(frame)
    r = pkg.Renderer()
    r.resize(acc.shape[1], acc.shape[0])
    r.write_accumulation(acc)
    r.postprocess(SAMPLES, tone_mapping=tone, **POST)
    return r


def _handle(pkg, frame):
    if frame not in _handles:
        _handles[frame] = _fresh(pkg, frame)
    return _handles[frame]


def _present(pkg, r, sw, sh, sharpness, fmt=None, hdr=False, ui=None, graded=False):
    r.present_upscaled(sw, sh, pkg.PRESENT_R16G16B16A16_SFLOAT if fmt is None else fmt, 1 if hdr else 0, ui, sharpness=sharpness, graded=graded)
    return r.read_present()


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-%dx%d-sharp%g" % c)
def test_device_equals_the_float32_reference_bit_for_bit(pkg, orc, case):
    frame, sw, sh, sharpness = case
    got = _present(pkg, _handle(pkg, frame), sw, sh, sharpness)
    want = _tone_mapped(pkg, orc, _S(orc, frame, sw, sh, sharpness))
    assert got.shape == (sh, sw, 4) and got.dtype == np.float16 and (_bits16(got)[..., 3] == 0x3c00).all()
    g = _bits16(got)[..., :3]
    nan_g, nan_w = np.isnan(got[..., :3]), np.isnan(want.view(np.float16))
    assert (nan_g == nan_w).all()
    bad = (g != want) & ~nan_g
    print(case, "values differing:", int(bad.sum()), "of", bad.size)
    assert not bad.any(), (case, int(bad.sum()), np.argwhere(bad)[:4].tolist())


@pytest.mark.gpu
@pytest.mark.parametrize("case", TAIL_CASES, ids=lambda c: "%s-%dx%d-ui%d-hdr%d" % c)
def test_ui_and_hdr10_against_the_float64_tail_on_the_float32_screen_image(pkg, orc, case):
    frame, sw, sh, ui, hdr = case
    got = _present(pkg, _handle(pkg, frame), sw, sh, TAIL_SHARPNESS, hdr=hdr, ui=TP._ui(sw, sh) if ui else None).astype(np.float64)
    ref = _tail(orc, case, np.float64)
    worst, share = REF_TAIL_F32_VS_F64[case]
    assert got.shape == ref.shape and (got[..., 3] == 1).all()
    with np.errstate(all="ignore"):
        d = np.abs(got - ref)[..., :3]
    tol = np.maximum(8.0 * worst, 2.0 ** -11 * np.maximum(1.0, np.abs(ref[..., :3])))
    differing = float(_differs(got[..., :3], ref[..., :3]).mean())
    print(case, "max |device - ref64| %.3e (measured on the reference %.3e), differing %.3e (%.3e)" % (float(np.nanmax(d)), worst, differing, share))
    assert np.isfinite(got).all() and (d <= tol).all(), (case, float(d.max()))
    assert differing <= 4.0 * share, (case, differing, share)


@pytest.mark.gpu
@pytest.mark.parametrize("extent", EXTENTS, ids=lambda e: "%s-%dx%d" % e)
def test_packed_formats_encode_the_device_s_own_screen_image(pkg, orc, extent):
    frame, sw, sh = extent
    r, ui = _handle(pkg, frame), TP._ui(sw, sh)
    sdr = _present(pkg, r, sw, sh, 0.5, ui=ui).astype(np.float32)
    want = orc.encode_output(sdr, 0)
    assert (_present(pkg, r, sw, sh, 0.5, pkg.PRESENT_R8G8B8A8_SRGB, ui=ui) == want).all()
    assert (_present(pkg, r, sw, sh, 0.5, pkg.PRESENT_B8G8R8A8_SRGB, ui=ui) == want[..., [2, 1, 0, 3]]).all()
    hdr = _present(pkg, r, sw, sh, 0.5, hdr=True, ui=ui).astype(np.float32)
    packed = _present(pkg, r, sw, sh, 0.5, pkg.PRESENT_A2B10G10R10_UNORM, hdr=True, ui=ui)
    assert packed.shape == (sh, sw) and packed.dtype == np.uint32 and (packed == R.pack_a2b10g10r10(hdr)).all()
    # without step 5 the kernel is another instantiation: its four stores hold one image too
    sdr0 = _present(pkg, r, sw, sh, 0.0).astype(np.float32)
    if (sw, sh) != _acc(frame).shape[1::-1]:
        assert (_present(pkg, r, sw, sh, 0.0, pkg.PRESENT_R8G8B8A8_SRGB) == orc.encode_output(sdr0, 0)).all()
        hdr0 = _present(pkg, r, sw, sh, 0.0, hdr=True).astype(np.float32)
        assert (_present(pkg, r, sw, sh, 0.0, pkg.PRESENT_A2B10G10R10_UNORM, hdr=True) == R.pack_a2b10g10r10(hdr0)).all()


@pytest.mark.gpu
def test_graded(pkg, orc):
    """PTX_UPSCALE_GRADED: an identity desc gives the ungraded bits; a desc without pow gives grade_ref's float32 instance on S."""
    r = _fresh(pkg, "frame")
    lib = pkg.load_hip()
    d, up = pkg.PresentDesc(134, 90, pkg.PRESENT_R16G16B16A16_SFLOAT, 0, None, 0, 0), pkg.UpscaleDesc(0, 0.5, pkg.UPSCALE_GRADED, 0)
    assert lib.ptx_present_upscaled(r.handle, C.byref(d), C.byref(up)) == 5  # no accepted ptx_grade yet
    r.grade()
    for sw, sh, sharpness, hdr in ((134, 90, 0.5, False), (100, 68, 0.0, False), (67, 45, 2.0, False), (100, 68, 0.5, True)):
        plain = _present(pkg, r, sw, sh, sharpness, hdr=hdr)
        assert (_bits16(_present(pkg, r, sw, sh, sharpness, hdr=hdr, graded=True)) == _bits16(plain)).all(), (sw, sh, sharpness, hdr)
    r.grade(**GRADE_NO_POW)
    for sw, sh, sharpness in ((134, 90, 0.5), (100, 68, 0.0), (201, 135, 2.0), (67, 45, 0.5)):
        got = _present(pkg, r, sw, sh, sharpness, graded=True)
        want = G.grade(_S(orc, "frame", sw, sh, sharpness), G.SDR, dtype=np.float32, **GRADE_NO_POW)
        with np.errstate(over="ignore"):
            assert (_bits16(got) == want.astype(np.float16).view(np.uint16)).all(), (sw, sh, sharpness)
        assert (_bits16(got) != _bits16(_present(pkg, r, sw, sh, sharpness))).any()
    # own size, sharpness 0: ptx_present_graded's launch
    r.present_graded(W, H, pkg.PRESENT_R16G16B16A16_SFLOAT)
    assert (_bits16(r.read_present()) == _bits16(_present(pkg, r, W, H, 0.0, graded=True))).all()
    r.close()


@pytest.mark.gpu
def test_own_size_with_sharpness_zero_is_ptx_present(pkg):
    r = _handle(pkg, "frame")
    ui = TP._ui(W, H)
    for fmt, hdr in ((pkg.PRESENT_R8G8B8A8_SRGB, False), (pkg.PRESENT_B8G8R8A8_SRGB, False), (pkg.PRESENT_R16G16B16A16_SFLOAT, False),
                     (pkg.PRESENT_R16G16B16A16_SFLOAT, True), (pkg.PRESENT_A2B10G10R10_UNORM, True)):
        r.present(W, H, fmt, int(hdr), ui)
        want = r.read_present()
        got = _present(pkg, r, W, H, 0.0, fmt, hdr=hdr, ui=ui)
        assert got.dtype == want.dtype and (got.view(np.uint8) == want.view(np.uint8)).all(), (fmt, hdr)
        # ... and with step 5 on it is another image
        assert (_present(pkg, r, W, H, 2.0, fmt, hdr=hdr, ui=ui).view(np.uint8) != want.view(np.uint8)).any()


@pytest.mark.gpu
def test_leaves_the_frame_alone_works_on_a_borrower_and_repeats(pkg):
    import torch  # noqa: F401

    scene = pkg.Scene("default")
    a, b = pkg.Renderer(), pkg.Renderer()
    a.upload(scene)
    b.share_scene(a)
    for r in (a, b):
        r.resize(W, H)
    u0, u1 = (scene.uniform(W, H, bounces=3, sample_count=1, total_samples=k) for k in (0, 1))
    a.render(u0, scene.lights)
    acc = a.readback()
    a.postprocess(1, **POST)
    b.write_accumulation(acc)
    b.postprocess(1, **POST)
    out, lin = a.read_output(pkg.OUTPUT_RGBA8_SRGB), a.read_output(pkg.OUTPUT_RGBA32F)
    ui = TP._ui(100, 68)
    img = _present(pkg, a, 100, 68, 0.5, ui=ui)
    img10 = _present(pkg, a, 134, 90, 2.0, pkg.PRESENT_A2B10G10R10_UNORM, hdr=True)
    assert (a.readback().view(np.uint32) == acc.view(np.uint32)).all()
    assert (a.read_output(pkg.OUTPUT_RGBA8_SRGB) == out).all() and (a.read_output(pkg.OUTPUT_RGBA32F).view(np.uint32) == lin.view(np.uint32)).all()
    # two calls in a row, of different extents, each give what the borrower -- a handle that never presented -- gives
    assert (_present(pkg, b, 134, 90, 2.0, pkg.PRESENT_A2B10G10R10_UNORM, hdr=True) == img10).all()
    assert (_bits16(_present(pkg, b, 100, 68, 0.5, ui=ui)) == _bits16(img)).all()
    assert (_bits16(_present(pkg, a, 100, 68, 0.5, ui=ui)) == _bits16(img)).all()
    # the image differs from the linear blit's, and the next sample is the one a handle that never presented renders
    a.present(100, 68, pkg.PRESENT_R16G16B16A16_SFLOAT, 0, ui)
    assert (_bits16(a.read_present()) != _bits16(img)).any()
    c = pkg.Renderer()
    c.share_scene(a)
    c.resize(W, H)
    c.write_accumulation(acc)
    a.render(u1, scene.lights)
    c.render(u1, scene.lights)
    assert (a.readback().view(np.uint32) == c.readback().view(np.uint32)).all()
    for r in (c, b, a):
        r.close()
    scene.close()


@pytest.mark.gpu
def test_state_resize_and_refusals(pkg):
    import torch

    lib = pkg.load_hip()
    r = _fresh(pkg, "frame")
    assert lib.ptx_present_bytes(r.handle) == 0 and not lib.ptx_device_present_ptr(r.handle)
    kept = _present(pkg, r, 100, 68, 0.5, pkg.PRESENT_B8G8R8A8_SRGB, ui=TP._ui(100, 68))
    assert lib.ptx_present_bytes(r.handle) == 100 * 68 * 4 and lib.ptx_device_present_ptr(r.handle)

    def call(handle=r.handle, up=True, width=100, height=68, fmt=pkg.PRESENT_R8G8B8A8_SRGB, mode=0, ui=None, flags=0, reserved=0, **over):
        u = dict(filter=0, sharpness=0.5, flags=0, reserved=0)
        u.update(over)
        d = pkg.PresentDesc(width, height, fmt, mode, ui, flags, reserved)
        return lib.ptx_present_upscaled(handle, C.byref(d), C.byref(pkg.UpscaleDesc(**u)) if up else None)

    def intact():
        assert (r.read_present() == kept).all() and lib.ptx_present_bytes(r.handle) == 100 * 68 * 4

    nan, inf = float("nan"), float("inf")
    # (1) what ptx_present refuses about desc, (2) what is wrong with up: the present image is read back after every single refusal
    bad = [dict(width=0), dict(height=0), dict(width=16385), dict(height=16385), dict(fmt=4), dict(mode=2), dict(flags=2), dict(reserved=1),
           dict(fmt=pkg.PRESENT_R8G8B8A8_SRGB, mode=1), dict(fmt=pkg.PRESENT_A2B10G10R10_UNORM, mode=0),
           dict(up=False), dict(filter=1), dict(filter=0xffffffff), dict(sharpness=nan), dict(sharpness=inf), dict(sharpness=-inf),
           dict(sharpness=-0.01), dict(sharpness=2.01)]
    for b in bad:
        assert call(**b) == 1, b
        intact()
    for u in (dict(flags=2), dict(flags=3), dict(reserved=1)):
        d = pkg.PresentDesc(100, 68, 0, 0, None, 0, 0)
        assert lib.ptx_present_upscaled(r.handle, C.byref(d), C.byref(pkg.UpscaleDesc(0, 0.5, u.get("flags", 0), u.get("reserved", 0)))) == 1, u
        intact()
    assert lib.ptx_present_upscaled(r.handle, None, C.byref(pkg.UpscaleDesc(0, 0.5, 0, 0))) == 1 and call(handle=None) == 1
    intact()
    # (4) a window below the render extent on either axis is ptx_present's; the limits of sharpness are accepted
    for b in (dict(width=66), dict(height=44), dict(width=1, height=1), dict(width=66, height=200)):
        assert call(**b) == 1, b
        intact()
    graded = pkg.UpscaleDesc(0, 0.5, pkg.UPSCALE_GRADED, 0)
    d = pkg.PresentDesc(100, 68, 0, 0, None, 0, 0)
    assert lib.ptx_present_upscaled(r.handle, C.byref(d), C.byref(graded)) == 5  # (3) no ptx_grade on this handle
    intact()
    assert call(sharpness=2.0) == 0 and call(sharpness=0.0) == 0 and call(sharpness=-0.0) == 0
    assert call(fmt=pkg.PRESENT_B8G8R8A8_SRGB, ui=TP._ui(100, 68).ctypes.data) == 0
    intact()
    # (3) before (4): a bound shard buffer and a resized handle are NOT_READY whatever the extent, (2) before (3)
    r.set_tile_shard(0, 2, 8)
    shard = torch.zeros(r.shard_bytes(0) // 4, dtype=torch.float32, device="cuda")
    r.bind_shard_accumulation(shard.data_ptr(), r.shard_bytes(0))
    assert call() == 5 and call(width=66) == 5 and call(sharpness=3.0) == 1
    intact()
    r.bind_shard_accumulation(0)
    assert call(fmt=pkg.PRESENT_B8G8R8A8_SRGB, ui=TP._ui(100, 68).ctypes.data) == 0  # a tile shard of several is refused under the grade alone
    assert lib.ptx_present_upscaled(r.handle, C.byref(d), C.byref(graded)) == 5
    r.set_tile_shard(0, 1, 32)
    intact()
    # ptx_resize: NOT_READY until the next output call, the present image stays readable; then the same image again
    r.resize(W, H)
    assert call() == 5 and call(width=66) == 5 and call(up=False) == 1
    with pytest.raises(pkg.PtxError, match="status 5"):
        r.present_upscaled(100, 68)
    intact()
    r.write_accumulation(_acc("frame"))
    assert call() == 5
    r.postprocess(SAMPLES, **POST)
    assert (_present(pkg, r, 100, 68, 0.5, pkg.PRESENT_B8G8R8A8_SRGB, ui=TP._ui(100, 68)) == kept).all()
    # a larger render extent turns the same window into a smaller one
    r.resize(101, 68)
    r.write_accumulation(np.ones((68, 101, 4), np.float32))
    r.postprocess(1, **POST)
    assert call() == 1 and lib.ptx_present(r.handle, C.byref(pkg.PresentDesc(100, 68, pkg.PRESENT_B8G8R8A8_SRGB, 0, None, 0, 0))) == 0
    r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("grade", [0, 1])
def test_renderer_hip_with_upscale_settings_on_is_the_same_call_made_by_hand(pkg, tmp_path_factory, tmp_path, grade):
    """test_motion's driver (examples/motion_frame.cpp, compiled once per session) with the upscale argument at 1: two frames of
    animated_test through RendererHip on the plain output path, each presented at 100 x 68 with UpscaleSettings on at their default.
    The presented images equal ptx_present_upscaled made by hand -- with PTX_UPSCALE_GRADED and the driver's grade where GradeSettings
    are on -- bit for bit, and differ from ptx_present's."""
    import subprocess

    import test_motion as TM

    w, h, spp, depth, step, sw, sh = W, H, 2, 4, 0.37, 100, 68
    exe = TM._motion_frame_driver(pkg, tmp_path_factory)
    dump = tmp_path / "frames.bin"
    subprocess.check_call([exe, "animated_test", str(w), str(h), str(spp), str(depth), str(step), "0", str(dump), "0", "0", "0", "0", str(grade), "-", "1"])
    raw = np.fromfile(dump, np.uint8)
    assert raw.size == 2 * 3 * h * w * 16 + 2 * sh * sw * 4
    screens = raw[2 * 3 * h * w * 16:].reshape(2, sh, sw, 4)
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
        if grade:
            r.grade(colour_matrix=pkg.white_balance_matrix(4500.0), slope=(1.1, 1.0, 1.0), offset=(0.0, 0.01, 0.0), power=(1.0, 1.0, 0.9), saturation=1.2,
                    curve=pkg.CURVE_HABLE)  # the driver's GradeSettings, as tests/test_grade.py repeats them
        got = _present(pkg, r, sw, sh, pkg.UPSCALE_DEFAULTS["sharpness"], pkg.PRESENT_R8G8B8A8_SRGB, graded=bool(grade))
        assert (got == screens[frame]).all(), frame
        r.present(sw, sh, pkg.PRESENT_R8G8B8A8_SRGB)
        assert (r.read_present() != screens[frame]).any()
    r.close()
    s.close()


def _print_tables():
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import __graft_entry__ as graft

    o = graft.load_oracle()
    o.build()
    print("REF_F32_VS_F64 = {")
    for case in CASES:
        print("    %r: (%.3e, %.3e)," % ((case,) + _measure(o, case)))
    print("}")
    print("REF_TAIL_F32_VS_F64 = {")
    for case in TAIL_CASES:
        print("    %r: (%.3e, %.3e)," % ((case,) + _measure_tail(o, case)))
    print("}")


if __name__ == "__main__":
    _print_tables()
