"""Noise metering (include/ptx.h "Noise metering": ptx_noise_halves, ptx_device_noise_half_ptr, ptx_noise_meter, ptx_read_noise;
csrc/pt_noise.hpp, docs/NEXT_ROWS.md section 26) against tests/noise_ref.py.

Tolerance: none.  Steps 1 - 5 are float32 operations in the header's order with the project's specified rcp and sqrt, both correctly
rounded on the arguments met, the sums of steps 6 and 7 are integers and the two divisions IEEE doubles -- so the device's result and
tile map equal the reference bit for bit on the device's own read-back of both halves.  The one place where bits are not compared is
the payload of a NaN in S = A + B, which IEEE 754 leaves open: there both sides have to be a NaN.  Extents: 1 x 1, 3 x 2, 33 x 9,
67 x 45, 130 x 70 and 300 x 200; the last two cross the 64-pixel block of a workgroup with ragged edges on both axes.

The statistical test (meanError at 64 + 64 frames below half of meanError at 4 + 4 frames of texture_test at 67 x 45; 1 / sqrt(n)
predicts a quarter): measured 0.2459 on the oracle's frames (0.06255 / 0.25437) and 0.2459 through the device."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

import noise_ref as NR

DETAIL = 0.25
SCENE = "texture_test"
EXTENTS = {"1x1": (1, 1), "3x2": (3, 2), "33x9": (33, 9), "67x45": (67, 45), "130x70": (130, 70), "300x200": (300, 200)}
W, H = EXTENTS["67x45"]
SHIFTS = (3, 4, 5, 6)
SAMPLES = ((1, 1), (4, 4), (3, 8))
EXPOSURES = (1.0, 2.75)
POST = dict(exposure=1.25, bloom_threshold=0.8, bloom_intensity=0.35)
OK, INVALID, NOT_READY = 0, 1, 5
FLOATS = ("meanError", "maxError")
INTS = ("tilesX", "tilesY", "converged", "counted", "black", "rejected", "valid", "calls")
f32 = np.float32


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_sum(got, want):
    """bit for bit, but for the payload of a NaN"""
    return ((_bits(got) == _bits(want)) | (np.isnan(got) & np.isnan(want))).all()


def _pair(a, b, h=1, w=1):
    """h x w halves whose every pixel is (a, a, a, 1) in half 0 and (b, b, b, 1) in half 1; a and b may be rgb triples"""
    A = np.ones((h, w, 4), np.float32)
    B = np.ones((h, w, 4), np.float32)
    A[..., :3] = a
    B[..., :3] = b
    return A, B


# =====================================================================================================
# without a GPU
# =====================================================================================================
def test_header_declares_and_package_exports_the_noise_metering(pkg):
    header = open(os.path.join(pkg.REPO_DIR, "include", "ptx.h")).read()
    decls = {
        "ptx_noise_halves": r"PTX_API int ptx_noise_halves\(PtxRenderer \*r, uint32_t enable\);",
        "ptx_device_noise_half_ptr": r"PTX_API void \*ptx_device_noise_half_ptr\(PtxRenderer \*r, uint32_t which\);",
        "ptx_noise_meter": r"PTX_API int ptx_noise_meter\(PtxRenderer \*r, const PtxNoiseDesc \*desc\);",
        "ptx_read_noise": r"PTX_API int ptx_read_noise\(PtxRenderer \*r, PtxNoiseResult \*out, float \*tileErrors /\* may be NULL \*/, size_t bytes\);",
    }
    lib = pkg.load_hip()
    for name, decl in decls.items():
        assert re.search(decl, header), name
        assert name in pkg.PTX_SYMBOLS
        assert hasattr(lib, name), name
    assert "#define PTX_ABI_VERSION 5u" in header and "PTX_FN_COUNT = 38" in header  # additions only
    body = re.search(r"typedef struct PtxNoiseDesc \{(.*?)\} PtxNoiseDesc;", header, re.S)[1]
    assert re.findall(r"(\w+)(?:\[2\])?[,;]", re.sub(r"/\*.*?\*/", "", body)) == ["samplesA", "samplesB", "exposure", "threshold", "tileShift", "flags", "reserved"]
    D = pkg.NoiseDesc
    assert C.sizeof(D) == 32 and [getattr(D, f).offset for f in ("samplesA", "samplesB", "exposure", "threshold", "tileShift", "flags", "reserved")] == [
        0, 4, 8, 12, 16, 20, 24]
    body = re.search(r"typedef struct PtxNoiseResult \{(.*?)\} PtxNoiseResult;", header, re.S)[1]
    assert tuple(re.findall(r"(\w+)[,;]", re.sub(r"/\*.*?\*/", "", body))) == FLOATS + INTS
    Rs = pkg.NoiseResult
    assert C.sizeof(Rs) == 40 and [getattr(Rs, f).offset for f in FLOATS + INTS] == list(range(0, 40, 4))
    assert [t for _, t in Rs._fields_] == [C.c_float] * 2 + [C.c_uint32] * 8
    assert re.search(r"PTX_NOISE_WRITE_SUM = 1u", header) and pkg.NOISE_WRITE_SUM == 1 == NR.WRITE_SUM
    # the semantics are in the header as text: the reference is written from it
    for phrase in ("Noise metering", "section 26", "1. SUM", "S = A + B, component by component, alpha included", "The binding is not changed", "2. SCALE FACTORS",
                   "sa = exposure * rcp((float)samplesA)", "st = exposure * rcp((float)(samplesA + samplesB))", "3. SCALED VALUES",
                   "D = (|a.r - b.r| + |a.g - b.g|) + |a.b - b.b|", "m = (c.r + c.g) + c.b", "4. CLASSES", "REJECTED iff any of the six input colour values, D or m is not finite",
                   "BLACK iff not rejected and not (m >= 2^-20)", "5. PER-PIXEL ERROR", "e = fmin(0.5f * (D / sqrt(m)), 255.0f)", "q = (uint32_t)(e * 65536.0f)",
                   "Dammertz, Hanika, Keller and Lensch", "6. PER TILE", "E_t = n_t ? (float)((double)Q_t / ((double)n_t * 65536.0)) : 0", "E_t <= threshold", "7. RESULT",
                   "meanError = (float)((double)SUM Q_t / ((double)SUM n_t * 65536.0))", "never synchronises", "works on a borrower",
                   "a refused call leaves the state, the tile map and the internal image intact", "is not the bits of one sum accumulated in frame order",
                   "unequal halves bias e", "no hierarchy", "sharded frames are refused", "no adaptive sampling", "ptx_resize drops them"):
        assert phrase in re.sub(r"\s*\n \*\s*", " ", header), phrase
    for method in ("noise_halves", "noise_half_ptr", "noise_meter", "read_noise"):
        assert callable(getattr(pkg.Renderer, method))
    # the adapter's defaults are the package's
    d = pkg.NOISE_DEFAULTS
    assert set(d) == {"threshold", "tile_shift", "check_every", "min_samples"}
    host = open(os.path.join(pkg.PKG_DIR, "host", "RendererHip.h")).read()
    m = re.search(r"struct NoiseSettings\s*\{\s*bool Enabled = false;\s*float Threshold = ([0-9.]+)f;\s*uint32_t TileShift = (\d+);\s*uint32_t CheckEvery = (\d+);\s*"
                  r"uint32_t MinSamples = (\d+);\s*\};", host)
    assert m, "NoiseSettings"
    assert (float(m[1]), int(m[2]), int(m[3]), int(m[4])) == (d["threshold"], d["tile_shift"], d["check_every"], d["min_samples"])
    assert d["tile_shift"] == 4 and d["check_every"] == 8 and "IsConverged()" in host and "GetNoise()" in host
    adapter = open(os.path.join(pkg.PKG_DIR, "host", "RendererHip.cpp")).read()
    for call in ("ptx_noise_halves(s_Renderer", "ptx_noise_meter(s_Renderer", "ptx_read_noise(s_Renderer", "ptx_device_noise_half_ptr(s_Renderer"):
        assert call in adapter, call
    assert "--noise-threshold" in open(os.path.join(pkg.REPO_DIR, "examples", "render_scene.cpp")).read()
    kernel = open(os.path.join(pkg.PKG_DIR, "csrc", "pt_noise.hpp")).read()
    for name in ("k_noise_tiles", "k_noise_resolve", "__shared__ unsigned long long tileQ"):
        assert name in kernel, name
    for parent in ("pt_meter.hpp", "pt_wavefront.hpp", "pt_post.hpp"):  # kernels in a file of their own
        assert "k_noise" not in open(os.path.join(pkg.PKG_DIR, "csrc", parent)).read()


def test_equal_halves_have_no_error_and_one_pixel_worked_out_by_hand():
    rng = np.random.default_rng(3)
    A = (2.0 ** rng.uniform(-6, 6, (H, W, 4))).astype(np.float32)
    for shift in SHIFTS:
        res, E, p = NR.meter(A, A, 5, 5, 1.5, 0.0, shift)
        assert res["meanError"] == 0 and res["maxError"] == 0 and not E.any() and res["converged"] == res["tilesX"] * res["tilesY"]
        assert res["valid"] == 1 and res["counted"] == W * H and res["black"] == 0 and res["rejected"] == 0 and not p["q"].any()
    # A = 4, B = 0 per channel, one sample each, exposure 1: a = 4, b = 0, S = 4, c = 4 * rcp(2) = 2; D = 12, m = 6;
    # e = 0.5 * (12 * rcp(sqrt(6))), in float32
    res, E, p = NR.meter(*_pair(4.0, 0.0), 1, 1, 1.0, 10.0, 3)
    root = np.sqrt(f32(6.0))
    e = f32(0.5) * (f32(12.0) * (f32(1.0) / root))
    assert p["D"][0, 0] == 12 and p["m"][0, 0] == 6 and p["e"][0, 0] == e and abs(float(e) - 6.0 / np.sqrt(6.0)) < 1e-6
    q = int(e * f32(65536.0))
    assert int(p["q"][0, 0]) == q == 160529
    assert res["meanError"] == E[0, 0] == f32(q / 65536.0) and res["maxError"] == E[0, 0] and res["converged"] == 1 and res["counted"] == 1
    assert NR.meter(*_pair(4.0, 0.0), 1, 1, 1.0, float(np.nextafter(E[0, 0], f32(0))), 3)[0]["converged"] == 0  # E_t <= threshold, to the bit
    assert NR.meter(*_pair(4.0, 0.0), 1, 1, 1.0, float(E[0, 0]), 3)[0]["converged"] == 1
    # the exposure scales D linearly and sqrt(m) by its root: e grows with sqrt(exposure)
    _, E4, _ = NR.meter(*_pair(4.0, 0.0), 1, 1, 4.0, 0.0, 3)
    assert abs(float(E4[0, 0]) / float(E[0, 0]) - 2.0) < 1e-5
    # unequal counts: the same means give no error (a = 6 / 3, b = 4 / 2)
    assert NR.meter(*_pair(6.0, 4.0), 3, 2, 1.0, 0.0, 3)[0]["maxError"] == 0


def test_the_clamp_the_rejected_and_the_black_class():
    one = lambda a, b, na=1, nb=1, ex=1.0: NR.meter(*_pair(a, b), na, nb, ex, 0.0, 3)
    # D large over m small: 16 in one sample against 0 in 2^24, so a = 16 and c = 16 / (2^24 + 1): D = 48, m = 2.9e-6, e = 14,189 before the clamp
    res, E, p = one(16.0, 0.0, nb=2 ** 24)
    assert p["D"][0, 0] == 48 and p["m"][0, 0] < 3e-6 and not p["black"][0, 0]
    assert p["e"][0, 0] == 255 and int(p["q"][0, 0]) == 255 * 65536 and E[0, 0] == 255 and res["maxError"] == 255
    for a, ex in ((1.0e12, 1.0), ((3.0e38, 0.0, 0.0), 0.5)):  # e grows with the root of the value; the second is 1.7e19 before the clamp, and finite
        res, E, p = one(a, 0.0, ex=ex)
        assert np.isfinite(p["D"][0, 0]) and int(p["q"][0, 0]) == 255 * 65536 and res["rejected"] == 0
    # NaN or an infinity in either half is rejected, and so is a finite pair whose sum overflows
    for a, b in ((np.nan, 1.0), (1.0, np.nan), (np.inf, 1.0), (1.0, np.inf), (-np.inf, 1.0), (1.0, -np.inf), (3.0e38, 3.0e38), ((np.nan, 1.0, 1.0), 1.0),
                 (1.0, (1.0, 1.0, np.inf))):
        res, E, p = one(a, b)
        assert p["rejected"][0, 0] and not p["black"][0, 0] and not p["counted"][0, 0] and int(p["q"][0, 0]) == 0, (a, b)
        assert res["rejected"] == 1 and res["counted"] == 0 and res["valid"] == 0 and res["meanError"] == 0 and res["maxError"] == 0
        assert E[0, 0] == 0 and res["converged"] == 1  # an all-rejected tile has E_t = 0 and is converged
    A, B = _pair(1.0, 1.0)
    A[0, 0, 3] = np.nan  # alpha is summed, not classified
    assert NR.meter(A, B, 1, 1)[0]["rejected"] == 0
    # a scaled value that overflows where the inputs are finite: D is not finite
    assert one(3.0e38, 1.0, ex=4.0)[0]["rejected"] == 1
    # black: zeros of either sign, negatives, denormals
    for a, b in ((0.0, 0.0), (-0.0, -0.0), (0.0, -0.0), (-1.0, -2.0), (-3.0, 1.0), (1e-41, 1e-41), (1e-41, 0.0), (1e-30, 1e-30)):
        res, E, p = one(a, b)
        assert p["black"][0, 0] and p["counted"][0, 0] and not p["rejected"][0, 0] and int(p["q"][0, 0]) == 0, (a, b)
        assert res["black"] == 1 and res["counted"] == 1 and res["valid"] == 1 and res["maxError"] == 0
    # m one ulp either side of 2^-20: only green is lit and equal in both halves, one sample each, so m = (g + g) * 0.5 = g exactly
    edge = f32(2.0 ** -20)
    for g, black in ((np.nextafter(edge, f32(0)), True), (edge, False), (np.nextafter(edge, f32(1)), False)):
        res, E, p = one((0.0, g, 0.0), (0.0, g, 0.0))
        assert p["m"][0, 0] == g and bool(p["black"][0, 0]) == black and res["black"] == int(black), g


def test_ragged_tiles_at_67_by_45_counted_by_hand():
    rng = np.random.default_rng(5)
    A = (2.0 ** rng.uniform(-3, 3, (H, W, 4))).astype(np.float32)
    B = (A * rng.uniform(0.5, 1.5, (H, W, 4))).astype(np.float32)
    A[0:8, 0:8, 0] = np.nan  # the first 8 x 8 pixels are rejected: a whole tile of tileShift 3
    p = NR.pixels(A, B, 2, 2, 1.0)
    by_hand = {3: (9, 6, [8, 8, 8, 8, 8, 8, 8, 8, 3], [8, 8, 8, 8, 8, 5]), 4: (5, 3, [16, 16, 16, 16, 3], [16, 16, 13]), 5: (3, 2, [32, 32, 3], [32, 13]),
               6: (2, 1, [64, 3], [45])}
    for shift, (tx, ty, widths, heights) in by_hand.items():
        res, E, q = NR.meter(A, B, 2, 2, 1.0, 0.05, shift)
        assert (res["tilesX"], res["tilesY"]) == (tx, ty) == E.shape[::-1] and sum(widths) == W and sum(heights) == H
        area = np.outer(heights, widths)
        area[0, 0] -= 64
        assert (q["N"] == area).all() and res["counted"] == W * H - 64 and res["rejected"] == 64
        x0 = y0 = 0
        total = 0
        for j, hh in enumerate(heights):
            x0 = 0
            for i, ww in enumerate(widths):
                Q = int(p["q"][y0:y0 + hh, x0:x0 + ww].sum())
                assert Q == q["Q"][j, i] and E[j, i] == (f32(Q / (int(area[j, i]) * 65536.0)) if area[j, i] else 0)
                total += Q
                x0 += ww
            y0 += hh
        assert res["meanError"] == f32(total / ((W * H - 64) * 65536.0)) and res["maxError"] == E.max()
        assert res["converged"] == int((E <= f32(0.05)).sum())
    assert NR.meter(A, B, 2, 2, 1.0, 0.0, 3)[1][0, 0] == 0  # the all-rejected tile
    # an all-rejected image
    A[...] = np.inf
    res, E, _ = NR.meter(A, B, 2, 2, 1.0, 0.0, 4)
    assert res["valid"] == 0 and res["meanError"] == 0 and res["maxError"] == 0 and res["counted"] == 0 and res["rejected"] == W * H and res["converged"] == 15


def test_the_error_of_the_oracles_frames_falls_with_the_samples(pkg, orc):
    """meanError at 64 + 64 frames below half of meanError at 4 + 4: measured 0.2459 (0.06255 / 0.25437), where 1 / sqrt(n) predicts 0.25"""
    s = pkg.Scene(SCENE, DETAIL)
    osc = orc.OracleScene(s.desc, build_bvh=True)
    u = s.uniform(W, H, bounces=4)
    half = [np.zeros((H, W, 4), np.float32) for _ in range(2)]
    mean = {}
    for f in range(128):
        u.TotalSamples = f
        osc.render(u, s.lights, W, H, accum=half[f & 1])
        if f + 1 in (8, 128):
            mean[f + 1] = float(NR.meter(half[0], half[1], (f + 1) // 2, (f + 1) // 2, 1.0, 0.02, 4)[0]["meanError"])
    print(f"meanError {mean[8]:.6g} at 4 + 4 frames, {mean[128]:.6g} at 64 + 64: ratio {mean[128] / mean[8]:.4f}")
    assert mean[8] > 0 and mean[128] < 0.5 * mean[8]


# =====================================================================================================
# on the GPU
# =====================================================================================================
_state = {}


def _gpu(pkg):
    """(scene, renderer) of SCENE, uploaded once"""
    import torch  # noqa: F401  (first, so the HIP library shares torch's HIP runtime)

    if "main" not in _state:
        s = pkg.Scene(SCENE, DETAIL)
        r = pkg.Renderer()
        r.upload(s)
        _state["main"] = (s, r)
    return _state["main"]


def _bind(r, which):
    """half 0 / 1, or None: the internal image"""
    if which is None:
        r.bind_accumulation(0, 0)
    else:
        assert r.noise_half_ptr(which)
        r.bind_accumulation(r.noise_half_ptr(which), r.width * r.height * 16)


def _write_halves(r, A, B):
    r.noise_halves(True)
    for which, img in enumerate((A, B)):
        _bind(r, which)
        r.write_accumulation(img)
    _bind(r, None)


def _read_halves(r):
    out = []
    for which in range(2):
        _bind(r, which)
        out.append(r.readback())
    _bind(r, None)
    return out


def _plain(pkg, w, h, A=None, B=None):
    """a handle with no scene: ptx_noise_meter needs none"""
    import torch  # noqa: F401

    f = pkg.Renderer()
    f.resize(w, h)
    if A is not None:
        _write_halves(f, A, B)
    return f


def _synthetic_halves(h, w, seed=23):
    """Halves with everything the steps have a clause for.  Positions wrap, so every extent gets what fits."""
    rng = np.random.default_rng(seed)
    A = (2.0 ** rng.uniform(-12, 12, (h, w, 4))).astype(np.float32)
    B = (A * (2.0 ** rng.normal(0.0, 0.5, (h, w, 4)))).astype(np.float32)
    B[::3, ::2] = A[::3, ::2]                                  # pixels without error
    A[..., 3], B[..., 3] = 2.0, 3.0
    fa, fb = A.reshape(-1, 4), B.reshape(-1, 4)
    cases = []
    for e in range(-30, -9):                                    # every power of two over twenty octaves, +- 3 ulps, on both sides of 2^-20
        g = f32(2.0 ** e)
        for _ in range(3):
            g = np.nextafter(g, f32(0))
        for _ in range(7):
            cases.append(((0.0, g, 0.0), (0.0, g, 0.0)))      # m = g at one sample each
            cases.append(((g, 0.0, 0.0), (0.0, 0.0, g)))      # ... and with D = m
            g = np.nextafter(g, f32(np.inf))
    nan, inf = np.nan, np.inf
    cases += [((nan, 1, 1), (1, 1, 1)), ((1, 1, 1), (1, nan, 1)), ((inf, 1, 1), (1, 1, 1)), ((1, 1, 1), (1, 1, -inf)), ((inf, 0, 0), (-inf, 0, 0)),
              ((3e38,) * 3, (3e38,) * 3), ((3e38, 0, 0), (0, 0, 0)), ((1e12,) * 3, (0,) * 3), ((0,) * 3, (1e12,) * 3), ((4,) * 3, (0,) * 3),
              ((0,) * 3, (0,) * 3), ((-0.0,) * 3, (-0.0,) * 3), ((-1,) * 3, (-2,) * 3), ((-3,) * 3, (1,) * 3), ((1e-41,) * 3, (1e-41,) * 3), ((1e-41,) * 3, (0,) * 3),
              ((1e-30,) * 3, (1e-30,) * 3), ((1e-3, 2e-3, 5e-4), (1.5e-3, 1e-3, 7e-4))]
    for k, (a, b) in enumerate(cases):
        at = (5 + 7 * k) % len(fa)
        fa[at, :3], fb[at, :3] = a, b
    A[h // 2:, : max(1, w // 5), :3] = 0.0                     # a black region
    B[h // 2:, : max(1, w // 5), :3] = 0.0
    if h >= 16 and w >= 24:                                    # an all-rejected tile of tileShift 3
        A[8:16, 16:24, 1] = np.inf
    A.view(np.uint32)[0, 0, 3] = 0x7FC0BEEF                    # a NaN in alpha is summed and nothing else
    return A, B


_halves = {}


def _device_halves(pkg, extent, kind):
    """The device's own read-back of both halves: synthetic, or texture_test rendered by alternating bindings with na frames in half 0 and nb
    in half 1 (kind = (na, nb)).  Computed once and left unchanged."""
    key = (extent, kind)
    if key not in _halves:
        s, r = _gpu(pkg)
        w, h = EXTENTS[extent]
        r.set_tile_shard(0, 1, 32)
        r.resize(w, h)
        if kind == "synthetic":
            _write_halves(r, *_synthetic_halves(h, w))
        else:
            r.noise_halves(True)
            u = s.uniform(w, h, bounces=4)
            left = list(kind)
            for f in range(sum(kind)):
                which = f & 1 if left[f & 1] else 1 - (f & 1)
                left[which] -= 1
                _bind(r, which)
                u.TotalSamples = f
                r.render(u, s.lights)
        _halves[key] = tuple(_read_halves(r))
        for img in _halves[key]:
            img.setflags(write=False)
        r.noise_halves(False)
    return _halves[key]


def _assert_same(r, want, E, what):
    res, tiles = r.read_noise(tile_errors=True)
    got = {k: getattr(res, k) for k in INTS}
    assert got == {k: int(want[k]) for k in INTS}, (what, got, want)
    for k in FLOATS:
        g, v = f32(getattr(res, k)), f32(want[k])
        assert g.view(np.uint32) == v.view(np.uint32), (what, k, float(g), float(v))
    assert tiles.shape == E.shape and (_bits(tiles) == _bits(E)).all(), (what, np.argwhere(_bits(tiles) != _bits(E))[:8])
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["render", "synthetic"])
@pytest.mark.parametrize("extent", list(EXTENTS))
def test_noise_meter_equals_the_reference_bit_for_bit(pkg, extent, kind):
    w, h = EXTENTS[extent]
    calls = 0
    r = _plain(pkg, w, h)
    seen = dict(black=0, rejected=0, clamped=0, unconverged=0)
    for na, nb in SAMPLES:
        A, B = _device_halves(pkg, extent, "synthetic" if kind == "synthetic" else (na, nb))
        _write_halves(r, A, B)
        got = _read_halves(r)
        assert (_bits(got[0]) == _bits(A)).all() and (_bits(got[1]) == _bits(B)).all()
        for exposure, shift in itertools.product(EXPOSURES, SHIFTS):
            _, E, p = NR.meter(A, B, na, nb, exposure, 0.0, shift)
            positive = np.sort(E[E > 0])
            exact = float(positive[len(positive) // 2]) if len(positive) else 0.25  # a threshold that equals a tile's E_t exactly
            for threshold in (0.0, 0.05, exact):
                calls += 1
                want = NR.meter(A, B, na, nb, exposure, threshold, shift, calls=calls)[0]
                r.noise_meter(na, nb, exposure, threshold, shift)
                _assert_same(r, want, E, (extent, kind, na, nb, exposure, shift, threshold))
                seen["unconverged"] += want["tilesX"] * want["tilesY"] - want["converged"]
            if len(positive):
                assert int((E <= f32(exact)).sum()) > int((E < f32(exact)).sum())
            seen["black"] += want["black"]
            seen["rejected"] += want["rejected"]
            seen["clamped"] += int((p["q"] == 255 * 65536).sum())
    print(f"{extent} {kind}: {calls} calls; over them {seen}")
    if w * h >= 297:
        assert seen["unconverged"] > 0
        if kind == "synthetic":
            assert seen["black"] > 0 and seen["rejected"] > 0 and seen["clamped"] > 0
    got = _read_halves(r)
    assert (_bits(got[0]) == _bits(A)).all() and (_bits(got[1]) == _bits(B)).all()  # the halves are only read
    r.close()


@pytest.mark.gpu
def test_write_sum_forms_a_plus_b_in_the_internal_image_and_the_output_stage_reads_it(pkg):
    w, h = EXTENTS["130x70"]
    for kind, (na, nb) in (("synthetic", (3, 8)), ((4, 4), (4, 4))):
        A, B = _device_halves(pkg, "130x70", kind)
        with np.errstate(all="ignore"):
            S = (A + B).astype(np.float32)
        r = _plain(pkg, w, h, A, B)
        marker = np.full((h, w, 4), 7.25, np.float32)
        r.write_accumulation(marker)  # the internal image: nothing is bound
        r.noise_meter(na, nb, 1.0, 0.05, 4)
        assert (_bits(r.readback()) == _bits(marker)).all()  # without the flag it keeps its bits
        plain = r.read_noise(tile_errors=True)
        _bind(r, 1)
        r.noise_meter(na, nb, 1.0, 0.05, 4, write_sum=True)
        assert r.accum_ptr() == r.noise_half_ptr(1)  # the binding is not changed
        _bind(r, None)
        assert _same_sum(r.readback(), S), kind
        flagged = r.read_noise(tile_errors=True)
        assert bytes(plain[0])[:36] == bytes(flagged[0])[:36] and flagged[0].calls == 2 and (_bits(plain[1]) == _bits(flagged[1])).all()
        got = _read_halves(r)
        assert (_bits(got[0]) == _bits(A)).all() and (_bits(got[1]) == _bits(B)).all()
        if kind != "synthetic":  # postprocess behind it is a fresh handle's postprocess of write_accumulation(A + B)
            assert (_bits(r.readback()) == _bits(S)).all()
            r.postprocess(na + nb, **POST)
            f = _plain(pkg, w, h)
            f.write_accumulation(S)
            f.postprocess(na + nb, **POST)
            assert (_bits(r.read_output(pkg.OUTPUT_RGBA32F)) == _bits(f.read_output(pkg.OUTPUT_RGBA32F))).all()
            assert not f.noise_half_ptr(0)
            f.close()
        r.close()


@pytest.mark.gpu
def test_alternating_bindings_leave_ptx_render_alone(pkg):
    s, r = _gpu(pkg)
    r.set_tile_shard(0, 1, 32)
    r.resize(W, H)
    u = s.uniform(W, H, bounces=4)

    def own(frames):
        """a fresh sum of those frames in the handle's own image"""
        _bind(r, None)
        r.reset()
        for f in frames:
            u.TotalSamples = f
            r.render(u, s.lights)
        return r.readback()
    evens, odds = own((0, 2, 4)), own((1, 3, 5))
    r.noise_halves(True)
    for f in range(6):
        _bind(r, f & 1)
        u.TotalSamples = f
        r.render(u, s.lights)
    A, B = _read_halves(r)
    assert (_bits(A) == _bits(evens)).all() and (_bits(B) == _bits(odds)).all()
    assert (_bits(A) != _bits(B)).any()
    # ... and a block of ptx_render_frames into whichever half is bound
    _bind(r, None)
    r.reset()
    r.render_frames(u, s.lights, 0, 3)
    first = r.readback()
    r.reset()
    r.render_frames(u, s.lights, 3, 3)
    second = r.readback()
    r.noise_halves(True)  # zeroes them again
    _bind(r, 0)
    r.render_frames(u, s.lights, 0, 3)
    _bind(r, 1)
    r.render_frames(u, s.lights, 3, 3)
    A, B = _read_halves(r)
    assert (_bits(A) == _bits(first)).all() and (_bits(B) == _bits(second)).all()
    # ptx_reset_accumulation acts on the bound half alone
    _bind(r, 0)
    r.reset()
    A2, B2 = _read_halves(r)
    assert not A2.any() and (_bits(B2) == _bits(B)).all()
    r.noise_halves(False)


@pytest.mark.gpu
def test_nothing_else_is_touched_and_two_meters_in_a_row_match_a_fresh_handle(pkg):
    s, main = _gpu(pkg)
    A, B = _device_halves(pkg, "67x45", (4, 4))
    u = s.uniform(W, H, bounces=4)
    r = pkg.Renderer()  # a borrower: the call needs no scene of its own
    r.share_scene(main)
    r.resize(W, H)
    _write_halves(r, A, B)
    marker = np.full((H, W, 4), 0.5, np.float32)
    r.write_accumulation(marker)
    r.render_guides(u)
    r.despike()
    before = [r.readback(), r.read_despiked()] + [r.read_guide(k) for k in range(3)] + _read_halves(r)
    calls = (dict(exposure=1.0, threshold=0.05, tile_shift=3), dict(exposure=2.0, threshold=0.3, tile_shift=5))
    f = _plain(pkg, W, H, A, B)
    only = _plain(pkg, W, H, A, B)
    for p in calls:
        r.noise_meter(4, 4, **p)
        f.noise_meter(4, 4, **p)
    only.noise_meter(4, 4, **calls[1])
    a, at = r.read_noise(tile_errors=True)
    b, bt = f.read_noise(tile_errors=True)
    c, ct = only.read_noise(tile_errors=True)
    assert bytes(a) == bytes(b) and (_bits(at) == _bits(bt)).all() and a.calls == 2
    assert bytes(a)[:36] == bytes(c)[:36] and (_bits(at) == _bits(ct)).all() and c.calls == 1
    want, E, _ = NR.meter(A, B, 4, 4, **calls[1], calls=2)
    _assert_same(r, want, E, "borrower")
    after = [r.readback(), r.read_despiked()] + [r.read_guide(k) for k in range(3)] + _read_halves(r)
    for k, (x, y) in enumerate(zip(before, after)):
        assert (_bits(x) == _bits(y)).all(), k
    for x in (r, f, only):
        x.close()
    # the next ptx_render continues a half as if nothing had happened
    main.set_tile_shard(0, 1, 32)
    main.resize(W, H)
    main.noise_halves(True)

    def path_traced(between=None):
        for which in range(2):
            _bind(main, which)
            main.reset()
        for k in range(4):
            if between and k == 3:
                between()
            _bind(main, k & 1)
            u.TotalSamples = k
            main.render(u, s.lights)
        return _read_halves(main)
    two = path_traced()
    again = path_traced(between=lambda: main.noise_meter(2, 1, write_sum=True))
    assert all((_bits(x) == _bits(y)).all() for x, y in zip(two, again))
    main.noise_halves(False)


@pytest.mark.gpu
def test_resize_drops_the_halves_and_disabling_returns_the_binding(pkg):
    lib = pkg.load_hip()
    A, B = _device_halves(pkg, "33x9", "synthetic")
    w, h = EXTENTS["33x9"]
    r = _plain(pkg, w, h)
    out = pkg.NoiseResult()
    assert not r.noise_half_ptr(0) and not r.noise_half_ptr(1) and lib.ptx_read_noise(r.handle, C.byref(out), None, 0) == NOT_READY
    internal = r.accum_ptr()
    _write_halves(r, A, B)
    assert r.noise_half_ptr(0) and r.noise_half_ptr(1) and r.noise_half_ptr(0) != r.noise_half_ptr(1) and not r.noise_half_ptr(2)
    assert internal not in (r.noise_half_ptr(0), r.noise_half_ptr(1))
    r.noise_meter(1, 1)
    r.noise_meter(1, 1)
    assert r.read_noise().calls == 2
    # ptx_noise_halves(0) with a half bound returns the binding
    _bind(r, 1)
    assert r.accum_ptr() == r.noise_half_ptr(1)
    r.noise_halves(False)
    assert r.accum_ptr() == internal and not r.noise_half_ptr(0) and not r.noise_half_ptr(1)
    assert r.read_noise().calls == 2  # the last result stays readable
    r.noise_halves(False)  # nothing to do
    # enabling zeroes them, and again where they exist
    r.noise_halves(True)
    assert not any(x.any() for x in _read_halves(r))
    _write_halves(r, A, B)
    r.noise_halves(True)
    assert not any(x.any() for x in _read_halves(r))
    # ptx_resize drops them, as it unbinds, and restarts calls
    _bind(r, 0)
    r.resize(w + 3, h + 2)
    assert not r.noise_half_ptr(0) and not r.noise_half_ptr(1) and r.accum_ptr() and lib.ptx_read_noise(r.handle, C.byref(out), None, 0) == NOT_READY
    assert lib.ptx_noise_meter(r.handle, C.byref(pkg.NoiseDesc(1, 1, 1.0, 0.0, 4, 0))) == NOT_READY
    r.noise_halves(True)
    r.noise_meter(1, 1)
    res = r.read_noise()
    assert res.calls == 1 and res.valid == 1 and res.black == (w + 3) * (h + 2) == res.counted and (res.tilesX, res.tilesY) == (3, 1)
    r.close()


@pytest.mark.gpu
def test_refusals_leave_the_state_the_tile_map_and_the_internal_image_intact(pkg):
    import torch

    lib = pkg.load_hip()
    A, B = _device_halves(pkg, "67x45", (3, 8))
    r = _plain(pkg, W, H, A, B)
    marker = np.full((H, W, 4), 3.5, np.float32)
    r.write_accumulation(marker)
    r.noise_meter(3, 8, 1.0, 0.05, 3)
    state = r.read_noise(tile_errors=True)
    flag = pkg.NOISE_WRITE_SUM

    def desc(**kw):
        d = dict(samplesA=3, samplesB=8, exposure=1.0, threshold=0.05, tileShift=4, flags=flag, reserved=(0, 0))
        d.update(kw)
        return pkg.NoiseDesc(d["samplesA"], d["samplesB"], d["exposure"], d["threshold"], d["tileShift"], d["flags"], (C.c_uint32 * 2)(*d["reserved"]))

    def intact(what):
        now = r.read_noise(tile_errors=True)
        assert bytes(now[0]) == bytes(state[0]) and (_bits(now[1]) == _bits(state[1])).all(), what
        _bind(r, None)
        assert (_bits(r.readback()) == _bits(marker)).all(), what
    bad = [dict(samplesA=0), dict(samplesB=0), dict(samplesA=2 ** 24 + 1), dict(samplesB=2 ** 24 + 1), dict(exposure=np.nan), dict(exposure=np.inf), dict(exposure=0.0),
           dict(exposure=-1.0), dict(threshold=np.nan), dict(threshold=np.inf), dict(threshold=-0.5), dict(tileShift=2), dict(tileShift=7), dict(flags=2), dict(flags=flag | 4),
           dict(reserved=(1, 0)), dict(reserved=(0, 1))]
    for kw in bad:
        assert lib.ptx_noise_meter(r.handle, C.byref(desc(**kw))) == INVALID, kw
        intact(kw)
    assert lib.ptx_noise_meter(r.handle, None) == INVALID and lib.ptx_noise_meter(None, C.byref(desc())) == INVALID
    intact("null")
    assert lib.ptx_noise_halves(None, 1) == INVALID and lib.ptx_noise_halves(r.handle, 2) == INVALID and not lib.ptx_device_noise_half_ptr(None, 0)
    intact("halves")
    # the largest counts are accepted: the check is against 2^24
    assert lib.ptx_noise_meter(r.handle, C.byref(desc(samplesA=2 ** 24, samplesB=2 ** 24, flags=0))) == OK
    assert lib.ptx_noise_meter(r.handle, C.byref(desc(samplesA=3, samplesB=8, tileShift=3, flags=0))) == OK
    again = r.read_noise(tile_errors=True)
    assert bytes(again[0])[:36] == bytes(state[0])[:36] and again[0].calls == 3 and (_bits(again[1]) == _bits(state[1])).all()
    state = again
    # ptx_read_noise
    out = pkg.NoiseResult()
    tiles = np.zeros_like(state[1])
    assert lib.ptx_read_noise(r.handle, None, None, 0) == INVALID and lib.ptx_read_noise(None, C.byref(out), None, 0) == INVALID
    for nbytes in (0, tiles.nbytes - 4, tiles.nbytes + 4):
        assert lib.ptx_read_noise(r.handle, C.byref(out), tiles.ctypes.data, nbytes) == INVALID
    assert not tiles.any()
    intact("read")
    # NOT_READY, in ptx_meter's order: a bound shard buffer, a tile shard with world size > 1, no halves; an invalid argument comes first
    r.set_tile_shard(0, 2, 8)
    assert lib.ptx_noise_meter(r.handle, C.byref(desc())) == NOT_READY and b"one tile shard of" in lib.ptx_last_error(r.handle)
    assert lib.ptx_noise_meter(r.handle, C.byref(desc(tileShift=9))) == INVALID
    shard = torch.zeros(r.shard_bytes(0) // 4, dtype=torch.float32, device="cuda")
    lib.ptx_bind_shard_accumulation(r.handle, shard.data_ptr(), shard.numel() * 4)
    assert lib.ptx_noise_meter(r.handle, C.byref(desc())) == NOT_READY and b"shard buffer" in lib.ptx_last_error(r.handle)
    lib.ptx_bind_shard_accumulation(r.handle, None, 0)
    r.set_tile_shard(0, 1, 32)
    intact("shard")
    r.noise_halves(False)
    assert lib.ptx_noise_meter(r.handle, C.byref(desc())) == NOT_READY and b"ptx_noise_halves" in lib.ptx_last_error(r.handle)
    now = r.read_noise(tile_errors=True)
    assert bytes(now[0]) == bytes(state[0]) and (_bits(now[1]) == _bits(state[1])).all()
    assert (_bits(r.readback()) == _bits(marker)).all()
    r.close()
    fresh = pkg.Renderer()  # no image: ptx_resize has not been called
    assert lib.ptx_noise_halves(fresh.handle, 1) == NOT_READY and lib.ptx_noise_meter(fresh.handle, C.byref(desc())) == NOT_READY
    assert lib.ptx_noise_halves(fresh.handle, 0) == OK and lib.ptx_read_noise(fresh.handle, C.byref(out), None, 0) == NOT_READY
    fresh.close()


def _driver_frames(pkg, tmp_path_factory, tmp_path, spp, noise):
    """test_motion's driver (examples/motion_frame.cpp, compiled once per session) with the noise argument given: two frames of
    animated_test, each presented at 100 x 37 too, and the trailer"""
    import subprocess

    import test_motion as TM

    exe = TM._motion_frame_driver(pkg, tmp_path_factory)
    dump = tmp_path / "frames.bin"
    subprocess.check_call([exe, "animated_test", str(W), str(H), str(spp), "4", "0.37", "0", str(dump), "0", "0", "0", "0", "0", "-", "0", str(noise)])
    raw = np.fromfile(dump, np.uint8)
    images = 6 * W * H * 16
    screens = 2 * 100 * 37 * 4
    assert len(raw) == images + screens + 2 * 44 + 4
    frames = raw[:images].view(np.float32).reshape(2, 3, H, W, 4)
    screen = raw[images:images + screens].reshape(2, 37, 100, 4)
    trailer = raw[images + screens:]
    results = [pkg.NoiseResult.from_buffer_copy(trailer[44 * k:44 * k + 40].tobytes()) for k in range(2)]
    converged = [int(trailer[44 * k + 40:44 * k + 44].view(np.uint32)[0]) for k in range(2)]
    return frames, screen, results, converged, int(trailer[88:92].view(np.uint32)[0])


def _posed(pkg, s, r, frame, step=0.37):
    if frame:
        assert s.update(step)
    it, bn = s.animation_state()
    r.update_animation(it, bn if len(bn) else None)


@pytest.mark.gpu
def test_renderer_hip_with_noise_settings_on_is_the_same_calls_made_by_hand(pkg, tmp_path_factory, tmp_path):
    """RendererHip with NoiseSettings { Enabled, CheckEvery 4, MinSamples 4 } over 16 render calls a frame: half (call parity) is bound
    before every ptx_render, the halves are metered after calls 4, 8, 12 and 16 on PostProcessSettings::Exposure, and ReadAccumulationImage,
    SaveOutput and Present each meter with PTX_NOISE_WRITE_SUM and read the internal image.  The result GetNoise() returns, the sum, the
    output image and the presented image equal the same calls made by hand, bit for bit."""
    spp = 16
    frames, screen, results, converged, halves = _driver_frames(pkg, tmp_path_factory, tmp_path, spp, 1)
    assert halves == 1
    d = pkg.NOISE_DEFAULTS
    s = pkg.Scene("animated_test", DETAIL)
    s.update(0.0)
    r = pkg.Renderer()
    r.upload(s)
    r.resize(W, H)
    calls = 0
    for frame in range(2):
        _posed(pkg, s, r, frame)
        r.noise_halves(True)  # ResetAccumulationImage
        n = [0, 0]
        for f in range(spp):
            _bind(r, f & 1)
            r.render(s.uniform(W, H, bounces=4, sample_count=1, total_samples=f), s.lights)
            n[f & 1] += 1
            if (f + 1) % 4 == 0:
                r.noise_meter(n[0], n[1], 1.0, d["threshold"], d["tile_shift"])
                calls += 1
        res, tiles = r.read_noise(tile_errors=True)
        assert bytes(res) == bytes(results[frame]) and res.calls == calls and res.valid == 1, frame
        assert converged[frame] == int(res.converged == res.tilesX * res.tilesY)
        A, B = _read_halves(r)
        want, E, _ = NR.meter(A, B, 8, 8, 1.0, d["threshold"], d["tile_shift"], calls=calls)
        _assert_same(r, want, E, frame)
        for k in range(3):  # ReadAccumulationImage, SaveOutput, Present
            r.noise_meter(8, 8, 1.0, d["threshold"], d["tile_shift"], write_sum=True)
            calls += 1
            _bind(r, None)
            if k == 0:
                S = r.readback()
                assert (_bits(S) == _bits(A + B)).all() and (_bits(frames[frame][0]) == _bits(S)).all(), frame
            else:
                r.postprocess(spp, 1.0, 1.0, 1.0, pkg.TONE_MAPPING_SDR)
            if k == 1:
                assert (_bits(frames[frame][2]) == _bits(r.read_output(pkg.OUTPUT_RGBA32F))).all(), frame
            if k == 2:
                r.present(100, 37)
                assert (r.read_present() == screen[frame]).all(), frame
            _bind(r, 0)
        print(f"frame {frame}: meanError {res.meanError:.6g} maxError {res.maxError:.6g}, {res.converged} of {res.tilesX * res.tilesY} tiles converged")
    r.close()


@pytest.mark.gpu
def test_renderer_hip_with_noise_settings_off_is_the_plain_path(pkg, tmp_path_factory, tmp_path):
    """The same driver with the noise argument given as 0: ptx_render into the internal image and ptx_postprocess on it, as before
    NoiseSettings existed, and the handle holds no halves at the end."""
    spp = 2
    frames, screen, results, converged, halves = _driver_frames(pkg, tmp_path_factory, tmp_path, spp, 0)
    assert halves == 0 and converged == [0, 0] and all(bytes(x) == bytes(40) for x in results)
    s = pkg.Scene("animated_test", DETAIL)
    s.update(0.0)
    r = pkg.Renderer()
    r.upload(s)
    r.resize(W, H)
    for frame in range(2):
        _posed(pkg, s, r, frame)
        r.reset()
        for f in range(spp):
            r.render(s.uniform(W, H, bounces=4, sample_count=1, total_samples=f), s.lights)
        r.postprocess(spp, 1.0, 1.0, 1.0, pkg.TONE_MAPPING_SDR)
        assert (_bits(frames[frame][0]) == _bits(r.readback())).all() and (_bits(frames[frame][2]) == _bits(r.read_output(pkg.OUTPUT_RGBA32F))).all(), frame
        r.present(100, 37)
        assert (r.read_present() == screen[frame]).all(), frame
    assert not r.noise_half_ptr(0) and not r.noise_half_ptr(1)
    r.close()


@pytest.mark.gpu
def test_the_error_falls_with_the_samples_on_the_device(pkg):
    """meanError at 64 + 64 frames below half of meanError at 4 + 4, through the device: measured 0.2459"""
    s, r = _gpu(pkg)
    r.set_tile_shard(0, 1, 32)
    r.resize(W, H)
    r.noise_halves(True)
    u = s.uniform(W, H, bounces=4)
    mean = {}
    for f in range(128):
        _bind(r, f & 1)
        u.TotalSamples = f
        r.render(u, s.lights)
        if f + 1 in (8, 128):
            r.noise_meter((f + 1) // 2, (f + 1) // 2, 1.0, 0.02, 4)
            res = r.read_noise()
            mean[f + 1] = float(res.meanError)
            assert res.valid == 1 and res.rejected == 0
    print(f"meanError {mean[8]:.6g} at 4 + 4 frames, {mean[128]:.6g} at 64 + 64: ratio {mean[128] / mean[8]:.4f}")
    assert mean[8] > 0 and mean[128] < 0.5 * mean[8]
    r.noise_halves(False)
