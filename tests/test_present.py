"""Row D15: the screen path (include/ptx.h ptx_present, csrc/pt_present.hpp) against tests/present_ref.py.

Bit-exact legs need no tolerance: a frame presented at its own size without a UI is ptx_read_output's image, and the packed
surface formats are the encodings of the device's own R16G16B16A16 result.

Tolerance of the rest.  The composed colour is the same bits on both sides (the oracle's, by test_output.py); what differs from the
float64 reference is float32 rounding in the blit, the tone mapping, the UI composition and the HDR10 encode, most of which the
rounding to binary16 at the next store hides.  Both bounds are therefore measured ON THE REFERENCE ALONE, per case, as its
float32 instance against its float64 instance on the binary16 image: the maximum difference and the share of values that differ
at all.  They are the constants REF_F32_VS_F64 below, printed by

    python tests/test_present.py

and test_reference_float32_against_float64 recomputes them without a GPU.  The device may differ from float64 by 8 x that
maximum, with a floor of one binary16 step (2^-11 max(1, |value|)), on at most 4 x that share of the values: the cap on the share
is what keeps the tolerance from hiding a wrong weight or constant."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

import present_ref as R

W, H = 67, 45          # the frame: odd, no multiple of a block, the last block of every screen extent partial
SMALL_W, SMALL_H = 7, 6  # below the bloom chain; 300 x 200 from it: many screen pixels share one clamped edge texel
SAMPLES = 8
POST = dict(exposure=1.0, bloom_threshold=0.8, bloom_intensity=0.35)
# (frame, screen width, screen height)
EXTENTS = [("frame", 67, 45), ("frame", 134, 90), ("frame", 33, 22), ("frame", 100, 37), ("frame", 67, 90), ("frame", 1, 1), ("small", 300, 200)]
CASES = [(f, sw, sh, ui, hdr) for (f, sw, sh) in EXTENTS for ui in (False, True) for hdr in (False, True)]

# (frame, screen width, screen height, UI, HDR) -> (max |ref(float32) - ref(float64)| on the binary16 image, share of values that differ)
REF_F32_VS_F64 = {
    ('frame', 67, 45, False, False): (0.000e+00, 0.000e+00),
    ('frame', 67, 45, False, True): (4.883e-04, 4.643e-03),
    ('frame', 67, 45, True, False): (0.000e+00, 0.000e+00),
    ('frame', 67, 45, True, True): (4.883e-04, 4.754e-03),
    ('frame', 134, 90, False, False): (0.000e+00, 0.000e+00),
    ('frame', 134, 90, False, True): (4.883e-04, 4.339e-03),
    ('frame', 134, 90, True, False): (0.000e+00, 0.000e+00),
    ('frame', 134, 90, True, True): (4.883e-04, 4.229e-03),
    ('frame', 33, 22, False, False): (2.441e-04, 4.591e-04),
    ('frame', 33, 22, False, True): (4.883e-04, 2.296e-03),
    ('frame', 33, 22, True, False): (2.441e-04, 4.591e-04),
    ('frame', 33, 22, True, True): (4.883e-04, 1.837e-03),
    ('frame', 100, 37, False, False): (4.883e-04, 9.009e-05),
    ('frame', 100, 37, False, True): (4.883e-04, 5.586e-03),
    ('frame', 100, 37, True, False): (4.883e-04, 9.009e-05),
    ('frame', 100, 37, True, True): (4.883e-04, 5.586e-03),
    ('frame', 67, 90, False, False): (0.000e+00, 0.000e+00),
    ('frame', 67, 90, False, True): (4.883e-04, 5.030e-03),
    ('frame', 67, 90, True, False): (0.000e+00, 0.000e+00),
    ('frame', 67, 90, True, True): (4.883e-04, 4.699e-03),
    ('frame', 1, 1, False, False): (0.000e+00, 0.000e+00),
    ('frame', 1, 1, False, True): (0.000e+00, 0.000e+00),
    ('frame', 1, 1, True, False): (0.000e+00, 0.000e+00),
    ('frame', 1, 1, True, True): (0.000e+00, 0.000e+00),
    ('small', 300, 200, False, False): (4.883e-04, 3.889e-05),
    ('small', 300, 200, False, True): (9.766e-04, 4.394e-03),
    ('small', 300, 200, True, False): (4.883e-04, 3.889e-05),
    ('small', 300, 200, True, True): (9.766e-04, 4.117e-03),
}


# =====================================================================================================
# inputs and references: computed once, shared, left unchanged
# =====================================================================================================
def _synthetic_sum(h, w, samples, seed=0):
    """test_output.py's running sum: a ramp with noise, a hot spot that blooms, a NaN and an Inf marker pixel."""
    rng = np.random.default_rng(seed)
    img = np.zeros((h, w, 4), np.float32)
    yy, xx = np.mgrid[0:h, 0:w]
    img[..., 0] = 0.2 + 0.6 * xx / w
    img[..., 1] = 0.1 + 0.5 * yy / h
    img[..., 2] = 0.3
    img[h // 3:h // 3 + 6, w // 2:w // 2 + 6, :3] = 40.0
    img[..., :3] += rng.uniform(0, 0.02, (h, w, 3))
    img[2, 3, 0] = np.nan   # -> (5000, 0, 0) marker, postprocess.comp:24-25
    img[4, 5, 1] = np.inf   # -> (0, 5000, 0) marker, :26-27
    img[..., :3] *= samples
    img[..., 3] = 1.0
    return img


UI_BYTES = np.array([0, 1, 5, 10, 11, 12, 40, 128, 254, 255], np.uint8)  # both sides of the sRGB threshold: 10 / 255 < 0.04044... < 11 / 255


def _ui_image(sw, sh):
    """Regions: alpha 0 (over colours that must not show), alpha 1, alpha 255 with colours on both sides of the sRGB threshold,
    a one-pixel line."""
    rng = np.random.default_rng(sw * 131 + sh)
    ui = np.zeros((sh, sw, 4), np.uint8)
    ui[..., :3] = rng.integers(0, 256, (sh, sw, 3))
    yy, xx = np.mgrid[0:sh, 0:sw]
    a1 = (slice(sh // 8, sh // 8 + max(1, sh // 4)), slice(sw // 8, sw // 8 + max(1, sw // 3)))
    ui[a1 + (3,)] = 1
    a255 = (slice(sh // 2, sh // 2 + max(1, sh // 4)), slice(sw // 3, sw // 3 + max(1, sw // 2)))
    for c in range(3):
        ui[a255 + (c,)] = UI_BYTES[(xx + 3 * yy + 4 * c) % len(UI_BYTES)][a255]
    ui[a255 + (3,)] = 255
    ui[(7 * sh) // 8, :, 3] = 200  # the line, over the random colours
    ui.setflags(write=False)
    return ui


_cache = {}


def _once(key, make):
    if key not in _cache:
        v = make()
        for a in (v if isinstance(v, tuple) else (v,)):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _cache[key] = v
    return _cache[key]


def _acc(frame):
    return _once(("acc", frame), lambda: _synthetic_sum(H, W, SAMPLES, seed=45) if frame == "frame" else _synthetic_sum(SMALL_H, SMALL_W, SAMPLES, seed=6))


def _composed(orc, frame):
    """Step 1: the HDR mode of the oracle passes composition.comp's store through."""
    return _once(("composed", frame), lambda: orc.postprocess(_acc(frame), SAMPLES, tone_mapping=1, **POST))


def _ui(sw, sh):
    return _once(("ui", sw, sh), lambda: _ui_image(sw, sh))


def _ref(orc, case, dtype):
    frame, sw, sh, ui, hdr = case
    return _once(("ref", case, np.dtype(dtype).name), lambda: R.present(_composed(orc, frame), _ui(sw, sh) if ui else None, sw, sh, hdr, dtype))


def _differs(a, b):
    """Values that are not the same number (two NaNs count as the same)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return ~((a == b) | (np.isnan(a) & np.isnan(b)))


def _measure(orc, case):
    a, b = _ref(orc, case, np.float32)[..., :3], _ref(orc, case, np.float64)[..., :3]
    with np.errstate(all="ignore"):
        d = np.abs(a.astype(np.float64) - b)
    return float(np.max(np.where(np.isfinite(d), d, 0.0))), float(_differs(a, b).mean())


# =====================================================================================================
# without a GPU
# =====================================================================================================
def test_header_declares_and_package_exports_the_screen_path(pkg):
    header = open(os.path.join(pkg.REPO_DIR, "include", "ptx.h")).read()
    for decl in (r"PTX_API int ptx_present\(PtxRenderer \*r, const PtxPresentDesc \*desc\);",
                 r"PTX_API int ptx_read_present\(PtxRenderer \*r, void \*host, size_t bytes\);",
                 r"PTX_API void \*ptx_device_present_ptr\(PtxRenderer \*r\);",
                 r"PTX_API size_t ptx_present_bytes\(const PtxRenderer \*r\);"):
        assert re.search(decl, header), decl
    lib = pkg.load_hip()
    for name in ("ptx_present", "ptx_read_present", "ptx_device_present_ptr", "ptx_present_bytes"):
        assert name in pkg.PTX_SYMBOLS
        assert hasattr(lib, name), name
    assert "#define PTX_ABI_VERSION 5u" in header and "PTX_FN_COUNT = 38" in header  # additions only
    assert pkg.ABI_VERSION == 5
    for k, name in enumerate(("R8G8B8A8_SRGB", "B8G8R8A8_SRGB", "A2B10G10R10_UNORM", "R16G16B16A16_SFLOAT")):
        assert re.search(r"PTX_PRESENT_%s = %d\b" % (name, k), header), name
        assert getattr(pkg, "PRESENT_" + name) == k
    assert re.search(r"PTX_PRESENT_UI_ON_DEVICE = 1u", header) and pkg.PRESENT_UI_ON_DEVICE == 1
    assert re.search(r"typedef struct PtxPresentDesc \{\s*uint32_t width, height;[^}]*uint32_t format;[^}]*uint32_t toneMappingMode;[^}]*"
                     r"const void \*ui;[^}]*uint32_t flags;[^}]*uint32_t reserved;[^}]*\} PtxPresentDesc;", header)
    assert C.sizeof(pkg.PresentDesc) == 32 and pkg.PresentDesc.ui.offset == 16 and pkg.PresentDesc.flags.offset == 24
    for method in ("present", "read_present"):
        assert callable(getattr(pkg.Renderer, method))
    host = open(os.path.join(pkg.PKG_DIR, "host", "RendererHip.h")).read()
    assert "Present(uint32_t width, uint32_t height, const uint8_t *ui" in host and "UpdateHdr(bool" in host and "ReadPresent()" in host


def test_reference_known_answers():
    """uiComposition.comp's two functions in float64 at points with known values."""
    f = lambda c: R.linear_to_hdr10(np.float64([c]), R.WHITE_POINT, np.float64)[0]  # noqa: E731
    assert np.abs(f([1, 1, 1]) - 0.58069).max() <= 1e-4  # BT.2408: 203 cd/m2 is 58 % PQ
    assert np.abs(f([10000 / 203] * 3) - 1.0).max() <= 1e-6
    assert f([0, 0, 0]).max() < 1e-6
    assert np.abs(f([1, 0, 0]) - np.float64([0.53255, 0.32702, 0.22007])).max() <= 1e-4  # the matrix' orientation
    s = lambda c: R.srgb_to_linear(np.float64(c), np.float64)  # noqa: E731
    t = 0.0404482362771082
    assert abs(float(s(t)) - float(s(np.nextafter(t, 0.0)))) <= 1e-6 and abs(float(s(t)) - t / 12.92) <= 1e-6
    assert float(s(0.0)) == 0.0 and float(s(1.0)) == 1.0
    assert float(s(10 / 255)) == (10 / 255) * (1 / 12.92) and float(s(11 / 255)) != (11 / 255) * (1 / 12.92)  # bytes 10 and 11 straddle it


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_reference_blit_properties(dtype):
    rng = np.random.default_rng(2)
    img = rng.uniform(0, 4, (6, 8, 3)).astype(np.float16).astype(dtype)
    # equal extents: the identity, bit for bit; also per axis
    assert (R.blit(img, 8, 6, dtype) == img).all() and R.blit_axis(8, 8, dtype) is None
    assert (R.blit(img, 16, 6, dtype)[:, 1::4] == (img[:, :-1] * dtype(0.75) + img[:, 1:] * dtype(0.25))[:, ::2]).all()
    # exact 2:1 reduction: the mean of each 2 x 2 block
    half = R.blit(img, 4, 3, dtype)
    mean = (img[0::2, 0::2] + img[0::2, 1::2] + img[1::2, 0::2] + img[1::2, 1::2]) / 4
    assert np.abs(half - mean).max() <= (1e-6 if dtype == np.float32 else 1e-14)
    i0, i1, t = R.blit_axis(8, 4, dtype)
    assert (i0 == [0, 2, 4, 6]).all() and (i1 == [1, 3, 5, 7]).all() and (t == 0.5).all()
    # 1:2 enlargement: interior weights 1/4 and 3/4, edge texels clamped
    i0, i1, t = R.blit_axis(8, 16, dtype)
    assert (t[1:-1:2] == 0.25).all() and (t[2:-1:2] == 0.75).all()
    assert (i0[1:-1] == (np.arange(1, 15) - 1) // 2).all() and (i1[1:-1] == i0[1:-1] + 1).all()
    assert i0[0] == 0 and i1[0] == 0 and i0[-1] == 7 and i1[-1] == 7
    twice = R.blit(img, 16, 12, dtype)
    assert (twice[0, 0] == img[0, 0]).all() and (twice[-1, -1] == img[-1, -1]).all()
    # a 1 x 1 screen reads the centre
    assert np.abs(R.blit(img, 1, 1, dtype)[0, 0] - (img[2, 3] + img[2, 4] + img[3, 3] + img[3, 4]) / 4).max() <= 1e-6
    odd = rng.uniform(0, 4, (5, 7, 3)).astype(dtype)
    assert np.abs(R.blit(odd, 1, 1, dtype)[0, 0] - odd[2, 3]).max() <= 1e-6


def test_reference_float32_against_float64(orc):
    """The measured figures behind every tolerance, recomputed: within a factor of 1.5 of the constants."""
    assert set(REF_F32_VS_F64) == set(CASES)
    for case in CASES:
        got, want = _measure(orc, case), REF_F32_VS_F64[case]
        print(case, "max %.3e share %.3e" % got)
        for g, w in zip(got, want):
            assert w / 1.5 <= g <= w * 1.5 if w else g == 0.0, (case, got, want)
    # the inputs are what the GPU tests assume: marker pixels present, the UI's regions present at every extent
    for frame in ("frame", "small"):
        c = _composed(orc, frame)
        assert np.isfinite(c).all() and c[2, 3, 0] >= 4096 and c[4, 5, 1] >= 4096
    for _, sw, sh in EXTENTS:
        a = _ui(sw, sh)[..., 3]
        assert (a > 0).any() and ((a == 0).any() or sw * sh == 1)
        if sw * sh > 1:
            assert (a == 1).any() and (a == 255).any() and (a == 200).any()
            on = _ui(sw, sh)[a == 255][:, :3]
            assert (on == 10).any() and (on == 11).any()


# =====================================================================================================
# on the GPU
# =====================================================================================================
_handles = {}


def _handle(pkg, frame, tone=0):
    """One renderer per frame, its sum written and post-processed once (SDR unless asked: present does not depend on it)."""
    import torch  # noqa: F401  (first, so the HIP library shares torch's HIP runtime)

    if frame not in _handles:
        acc = _acc(frame)
        r = pkg.Renderer()
        r.resize(acc.shape[1], acc.shape[0])
        r.write_accumulation(acc)
        r.postprocess(SAMPLES, tone_mapping=tone, **POST)
        _handles[frame] = r
    return _handles[frame]


def _fresh(pkg, frame, tone=0):
    import torch  # noqa: F401

    acc = _acc(frame)
    r = pkg.Renderer()
    r.resize(acc.shape[1], acc.shape[0])
    r.write_accumulation(acc)
    r.postprocess(SAMPLES, tone_mapping=tone, **POST)
    return r


def _present(pkg, r, case, fmt=None):
    frame, sw, sh, ui, hdr = case
    r.present(sw, sh, pkg.PRESENT_R16G16B16A16_SFLOAT if fmt is None else fmt, 1 if hdr else 0, _ui(sw, sh) if ui else None)
    return r.read_present()


def _bits16(a):
    assert a.dtype == np.float16
    return np.ascontiguousarray(a).view(np.uint16)


@pytest.mark.gpu
def test_own_size_without_ui_is_read_output(pkg):
    """Equal extents, no UI, SDR: the sRGB8 surface is ptx_read_output's sRGB8 image, BGRA its channel swap, R16G16B16A16 its
    RGBA32F image in binary16 -- and again after a ptx_postprocess in HDR mode: present does not depend on that call's mode."""
    r = _fresh(pkg, "frame", tone=0)
    srgb, lin = r.read_output(pkg.OUTPUT_RGBA8_SRGB), r.read_output(pkg.OUTPUT_RGBA32F)
    case = ("frame", W, H, False, False)
    for post_mode in (0, 1):
        r.postprocess(SAMPLES, tone_mapping=post_mode, **POST)
        rgba = _present(pkg, r, case, pkg.PRESENT_R8G8B8A8_SRGB)
        assert rgba.shape == (H, W, 4) and rgba.dtype == np.uint8 and (rgba == srgb).all(), post_mode
        assert (_present(pkg, r, case, pkg.PRESENT_B8G8R8A8_SRGB) == srgb[..., [2, 1, 0, 3]]).all(), post_mode
        half = _present(pkg, r, case)
        assert half.shape == (H, W, 4) and (_bits16(half) == _bits16(lin.astype(np.float16))).all(), post_mode
        assert (half.astype(np.float32).view(np.uint32) == lin.view(np.uint32)).all()
    r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("extent", EXTENTS, ids=lambda e: "%s-%dx%d" % e)
def test_packed_formats_encode_the_device_s_own_screen_image(pkg, orc, extent):
    """At every extent, with the UI, in both modes: the four store variants hold one image."""
    frame, sw, sh = extent
    r = _handle(pkg, frame)
    sdr = _present(pkg, r, (frame, sw, sh, True, False)).astype(np.float32)
    want = orc.encode_output(sdr, 0)
    assert (sdr[..., 3] == 1).all()
    assert (_present(pkg, r, (frame, sw, sh, True, False), pkg.PRESENT_R8G8B8A8_SRGB) == want).all()
    assert (_present(pkg, r, (frame, sw, sh, True, False), pkg.PRESENT_B8G8R8A8_SRGB) == want[..., [2, 1, 0, 3]]).all()
    hdr = _present(pkg, r, (frame, sw, sh, True, True)).astype(np.float32)
    packed = _present(pkg, r, (frame, sw, sh, True, True), pkg.PRESENT_A2B10G10R10_UNORM)
    assert packed.shape == (sh, sw) and packed.dtype == np.uint32 and (packed == R.pack_a2b10g10r10(hdr)).all()
    assert (packed >> 30 == 3).all()


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-%dx%d-ui%d-hdr%d" % c)
def test_screen_image_against_float64_reference(pkg, orc, case):
    frame, sw, sh, ui, hdr = case
    got = _present(pkg, _handle(pkg, frame), case).astype(np.float64)
    ref = _ref(orc, case, np.float64)
    worst, share = REF_F32_VS_F64[case]
    assert got.shape == ref.shape and (got[..., 3] == 1).all()
    with np.errstate(all="ignore"):
        d = np.abs(got - ref)[..., :3]
    tol = np.maximum(8.0 * worst, 2.0 ** -11 * np.maximum(1.0, np.abs(ref[..., :3])))
    differing = float(_differs(got[..., :3], ref[..., :3]).mean())
    print(case, "max |device - ref64| %.3e (measured on the reference %.3e), differing %.3e (%.3e)" % (float(np.nanmax(d)), worst, differing, share))
    assert np.isfinite(got).all() and (d <= tol).all(), (case, float(d.max()))
    assert differing <= 4.0 * share, (case, differing, share)
    if (sw, sh) == (W, H) and not ui:
        # the NaN / Inf marker pixels (5000 red, 5000 green) come out saturated: 1 after the SDR curve, beyond 10000 cd/m2 in PQ
        if hdr:
            assert got[2, 3, 0] > 1 and got[4, 5, 1] > 1
        else:
            assert got[2, 3, 0] == 1 and got[4, 5, 1] == 1 and (got[2, 3] == ref[2, 3]).all() and (got[4, 5] == ref[4, 5]).all()


@pytest.mark.gpu
def test_ui_placement(pkg):
    """A UI whose alpha is 0 everywhere is no UI; a UI in device memory is read in place and is the host image."""
    import torch

    r = _handle(pkg, "frame")
    for sw, sh, hdr in ((100, 37, False), (67, 45, True)):
        none = _present(pkg, r, ("frame", sw, sh, False, hdr))
        clear = _ui(sw, sh).copy()
        clear[..., 3] = 0
        r.present(sw, sh, pkg.PRESENT_R16G16B16A16_SFLOAT, int(hdr), clear)
        assert (_bits16(r.read_present()) == _bits16(none)).all()
        host = _present(pkg, r, ("frame", sw, sh, True, hdr))
        assert (_bits16(host) != _bits16(none)).any()
        dev = torch.from_numpy(_ui(sw, sh).copy()).cuda()
        r.present(sw, sh, pkg.PRESENT_R16G16B16A16_SFLOAT, int(hdr), dev)
        assert (_bits16(r.read_present()) == _bits16(host)).all()
        lib = pkg.load_hip()
        assert lib.ptx_present_bytes(r.handle) == sw * sh * 8 and lib.ptx_device_present_ptr(r.handle)


@pytest.mark.gpu
def test_present_leaves_the_frame_alone_and_works_on_a_borrower(pkg):
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
    out = a.read_output(pkg.OUTPUT_RGBA8_SRGB)
    lin = a.read_output(pkg.OUTPUT_RGBA32F)
    img_a = _present(pkg, a, ("frame", 100, 37, True, False))
    img_a10 = _present(pkg, a, ("frame", 100, 37, True, True), pkg.PRESENT_A2B10G10R10_UNORM)
    assert (a.readback().view(np.uint32) == acc.view(np.uint32)).all()
    assert (a.read_output(pkg.OUTPUT_RGBA8_SRGB) == out).all() and (a.read_output(pkg.OUTPUT_RGBA32F).view(np.uint32) == lin.view(np.uint32)).all()
    # the borrower presents the same frame; the handle that never presented renders the same next sample
    assert (_bits16(_present(pkg, b, ("frame", 100, 37, True, False))) == _bits16(img_a)).all()
    assert (_present(pkg, b, ("frame", 100, 37, True, True), pkg.PRESENT_A2B10G10R10_UNORM) == img_a10).all()
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
def test_present_state_and_refusals(pkg):
    import torch

    lib = pkg.load_hip()
    r = _fresh(pkg, "frame")
    with pytest.raises(pkg.PtxError, match="status 1"):
        r.read_present()
    probe = np.zeros(16, np.uint8)
    assert lib.ptx_read_present(r.handle, probe.ctypes.data, probe.nbytes) == 1  # before any present
    assert lib.ptx_present_bytes(r.handle) == 0 and not lib.ptx_device_present_ptr(r.handle)
    # two presents with different extents in a row each match a fresh handle's
    first = _present(pkg, r, ("frame", 134, 90, True, True))
    second = _present(pkg, r, ("frame", 33, 22, True, False), pkg.PRESENT_B8G8R8A8_SRGB)
    f = _fresh(pkg, "frame")
    assert (_present(pkg, f, ("frame", 33, 22, True, False), pkg.PRESENT_B8G8R8A8_SRGB) == second).all()
    f.close()
    f = _fresh(pkg, "frame")
    assert (_bits16(_present(pkg, f, ("frame", 134, 90, True, True))) == _bits16(first)).all()
    f.close()

    # every refusal returns its status and leaves the previous present image intact
    def desc(width=33, height=22, fmt=pkg.PRESENT_R8G8B8A8_SRGB, mode=0, ui=None, flags=0, reserved=0):
        return pkg.PresentDesc(width, height, fmt, mode, ui, flags, reserved)

    def intact():
        assert (r.read_present() == second).all() and lib.ptx_present_bytes(r.handle) == 33 * 22 * 4

    bad = [desc(width=0), desc(height=0), desc(width=16385), desc(height=16385), desc(fmt=4), desc(mode=2), desc(flags=2), desc(flags=3), desc(reserved=1),
           desc(fmt=pkg.PRESENT_R8G8B8A8_SRGB, mode=1), desc(fmt=pkg.PRESENT_B8G8R8A8_SRGB, mode=1), desc(fmt=pkg.PRESENT_A2B10G10R10_UNORM, mode=0)]
    for d in bad:
        assert lib.ptx_present(r.handle, C.byref(d)) == 1, (d.width, d.height, d.format, d.toneMappingMode, d.flags, d.reserved)
        intact()
    assert lib.ptx_present(r.handle, None) == 1
    small = np.zeros(33 * 22 * 4 - 4, np.uint8)
    large = np.zeros(33 * 22 * 4 + 4, np.uint8)
    for buf in (small, large):
        assert lib.ptx_read_present(r.handle, buf.ctypes.data, buf.nbytes) == 1 and not buf.any()
    assert lib.ptx_read_present(r.handle, None, 33 * 22 * 4) == 1
    intact()
    # a bound shard accumulation buffer: NOT_READY, as for the other calls that need the row-major frame
    r.set_tile_shard(0, 2, 8)
    shard = torch.zeros(r.shard_bytes(0) // 4, dtype=torch.float32, device="cuda")
    r.bind_shard_accumulation(shard.data_ptr(), r.shard_bytes(0))
    assert lib.ptx_present(r.handle, C.byref(desc())) == 5
    intact()
    r.bind_shard_accumulation(0)
    assert lib.ptx_present(r.handle, C.byref(desc(fmt=pkg.PRESENT_B8G8R8A8_SRGB, ui=_ui(33, 22).ctypes.data))) == 0
    intact()
    # ptx_resize: NOT_READY until the next ptx_postprocess; the present image stays readable
    r.resize(W, H)
    assert lib.ptx_present(r.handle, C.byref(desc())) == 5
    with pytest.raises(pkg.PtxError, match="status 5"):
        r.present(33, 22)
    intact()
    r.write_accumulation(_acc("frame"))
    assert lib.ptx_present(r.handle, C.byref(desc())) == 5
    r.postprocess(SAMPLES, **POST)
    assert (_present(pkg, r, ("frame", 33, 22, True, False), pkg.PRESENT_B8G8R8A8_SRGB) == second).all()
    r.close()


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import __graft_entry__ as graft

    o = graft.load_oracle()
    o.build()
    print("REF_F32_VS_F64 = {")
    for case in CASES:
        print("    %r: (%.3e, %.3e)," % ((case,) + _measure(o, case)))
    print("}")
