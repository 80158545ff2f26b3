"""Local exposure (include/ptx.h "Local exposure": ptx_local_exposure, ptx_read_local_exposure, ptx_device_local_exposure_ptr,
ptx_postprocess_local; csrc/pt_local_exposure.hpp, docs/NEXT_ROWS.md section 23) against tests/local_exposure_ref.py.

Tolerance for G: none.  Everything up to the base B is integer, B is one float64 division, the gain two float64 operations and the
project's exp2, restated in tests/meter_ref.py -- so the device's G equals the reference bit for bit on the device's own read-back
image.  ptx_postprocess_local is held to the plain output call bit for bit wherever G is one value over a region, and to
tests/bloom_ref.py under that file's tolerance rule where the bloom mixes pixels of different gains.

Extents: 1 x 1, 5 x 3 (every cell ragged), 67 x 45, 130 x 70 at s = 6 (3 x 2 cells, the last ragged; 3 x 2 workgroups of k_local_splat),
300 x 200 at s = 3 (38 x 25 cells: k_local_gain stages its largest 6 x 3 neighbourhood) and at s = 5."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import bloom_ref as BR
import local_exposure_ref as LR
import meter_ref as MR

DETAIL = 0.25
SCENE = "default"
CASES = {"1x1-s5": (1, 1, 5), "5x3-s3": (5, 3, 3), "67x45-s5": (67, 45, 5), "67x45-s4": (67, 45, 4), "130x70-s6": (130, 70, 6), "300x200-s3": (300, 200, 3),
         "300x200-s5": (300, 200, 5)}
W, H = 67, 45
POST = dict(exposure=1.25, bloom_threshold=0.8, bloom_intensity=0.35)
OK, INVALID, NOT_READY = 0, 1, 5
KEY = float(np.log2(0.18))
FIELDS = ("source", "totalSamples", "cellShift", "pivotLog2", "highlightContrast", "shadowContrast", "maxStops", "flags", "reserved")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _grey(h, w, value):
    """a grey H x W x 4 image: Y is the value to within an ulp or two"""
    S = np.empty((h, w, 4), np.float32)
    S[..., :3] = np.asarray(value, np.float32)[..., None] if np.ndim(value) else np.float32(value)
    S[..., 3] = 1.0
    return S


def _log2(G):
    return np.log2(G.astype(np.float64))


# =====================================================================================================
# without a GPU
# =====================================================================================================
def test_header_declares_and_package_exports_the_local_exposure(pkg):
    header = open(os.path.join(pkg.REPO_DIR, "include", "ptx.h")).read()
    decls = {
        "ptx_local_exposure": r"PTX_API int ptx_local_exposure\(PtxRenderer \*r, const PtxLocalExposureDesc \*desc\);",
        "ptx_read_local_exposure": r"PTX_API int ptx_read_local_exposure\(PtxRenderer \*r, void \*host, size_t bytes\);",
        "ptx_device_local_exposure_ptr": r"PTX_API void \*ptx_device_local_exposure_ptr\(PtxRenderer \*r\);",
        "ptx_postprocess_local": r"PTX_API int ptx_postprocess_local\(PtxRenderer \*r, const PtxPostProcessingUniformData \*u, uint32_t toneMappingMode,\s*"
                                 r"uint32_t source, uint32_t metered /\* 0 or 1 \*/\);",
    }
    lib = pkg.load_hip()
    for name, decl in decls.items():
        assert re.search(decl, header), name
        assert name in pkg.PTX_SYMBOLS
        assert hasattr(lib, name), name
    assert "#define PTX_ABI_VERSION 5u" in header and "PTX_FN_COUNT = 38" in header  # additions only
    body = re.search(r"typedef struct PtxLocalExposureDesc \{(.*?)\} PtxLocalExposureDesc;", header, re.S)[1]
    assert tuple(re.findall(r"^\s*(?:uint32_t|float)\s+(\w+);", body, re.M)) == FIELDS
    D = pkg.LocalExposureDesc
    assert C.sizeof(D) == 36 and [getattr(D, f).offset for f in FIELDS] == list(range(0, 36, 4))
    assert re.search(r"PTX_LOCAL_EXPOSURE_PIVOT_METERED = 1u", header) and pkg.LOCAL_EXPOSURE_PIVOT_METERED == 1 == LR.PIVOT_METERED
    # the semantics are in the header as text: the reference is written from it
    for phrase in ("Local exposure", "section 23", "1. LUMINANCE AND CLASSES", "2. FIXED-POINT LOG", "l = clamp((int)(bits(Y) >> 15) - 888 * 32, 0, 8191)",
                   "3. SPLAT", "cx = x >> s, cy = y >> s, z = l >> 8", "Both arrays are uint32", "4. BLUR", "4096 * 8191 * 64 = 2,147,221,504 < 2^32", "5. SLICE",
                   "u = 2x + 1 - 2^s", "v = 2l + 1 - 256", "z0 = v >> 9, fz = v & 511, z1 = min(z0 + 1, 31)", "B = (double)N / (double)D / 256 - 16", "6. GAIN",
                   "c = d > 0 ? highlightContrast : shadowContrast", "G(p) = (float)exp2(g)", "A BLACK or REJECTED pixel gets G(p) = 1", "7. OUTPUT",
                   "Exposure_p = (u->Exposure * m) * G(p)", "exactly 1.0f", "no halo", "a refused call leaves G intact", "ptx_resize drops G and the grid",
                   "no detail-strength control", "the pass count is", "32 octaves", "sharded frames are refused"):
        assert phrase in header, phrase
    for method in ("local_exposure", "read_local_exposure", "local_exposure_ptr", "postprocess_local"):
        assert callable(getattr(pkg.Renderer, method))
    # the adapter's defaults are the package's, and nobody claims they are tuned
    d = pkg.LOCAL_EXPOSURE_DEFAULTS
    assert d == dict(cell_shift=5, pivot_log2=-2.473931, highlight_contrast=0.6, shadow_contrast=0.8, max_stops=4.0)
    assert np.float32(d["pivot_log2"]) == np.float32(np.log2(0.18))
    host = open(os.path.join(pkg.PKG_DIR, "host", "RendererHip.h")).read()
    m = re.search(r"struct LocalExposureSettings\s*\{\s*bool Enabled = false;\s*uint32_t CellShift = (\d+);\s*float PivotLog2 = (-?[0-9.]+)f;[^\n]*\n\s*"
                  r"float HighlightContrast = ([0-9.]+)f;\s*float ShadowContrast = ([0-9.]+)f;\s*float MaxStops = ([0-9.]+)f;\s*\};", host)
    assert m, "LocalExposureSettings"
    assert (int(m[1]), float(m[2]), float(m[3]), float(m[4]), float(m[5])) == tuple(d.values())
    assert "tuned" in host and "tuned" in open(os.path.join(pkg.PKG_DIR, "__init__.py")).read()
    adapter = open(os.path.join(pkg.PKG_DIR, "host", "RendererHip.cpp")).read()
    for call in ("ptx_local_exposure(s_Renderer", "ptx_postprocess_local(s_Renderer"):
        assert call in adapter, call
    assert "--local-exposure" in open(os.path.join(pkg.REPO_DIR, "examples", "render_scene.cpp")).read()
    kernel = open(os.path.join(pkg.PKG_DIR, "csrc", "pt_local_exposure.hpp")).read()
    for name in ("k_local_splat", "k_local_blur", "k_local_gain", "__shared__"):
        assert name in kernel, name
    assert "k_postprocess_local" in open(os.path.join(pkg.PKG_DIR, "csrc", "pt_post.hpp")).read()


def test_known_answers_a_both_contrasts_at_one_give_unit_gain():
    rng = np.random.default_rng(3)
    S = (2.0 ** rng.uniform(-18, 18, (40, 50, 4))).astype(np.float32)
    S[3, 4, :3] = np.nan
    S[5, 6, :3] = -1.0
    for pivot in (KEY, 5.0, -30.0):
        G, d = LR.gain(S, 2, 4, pivot, 1.0, 1.0, 4.0)
        assert (_bits(G) == 0x3F800000).all() and not d["counted"][3, 4] and not d["counted"][5, 6]
    G, _ = LR.gain(S, 2, 4, KEY, 0.3, 1.7, 0.0)  # ... and so does maxStops = 0
    assert (_bits(G) == 0x3F800000).all()


def test_known_answers_b_a_constant_image_has_one_known_gain_and_the_worst_cell_fits_32_bits():
    for value, s, shape in ((0.18, 5, (45, 67)), (1.0, 3, (9, 20)), (3.7, 6, (70, 130)), (2.0 ** -17, 4, (5, 3)), (1e9, 5, (33, 31)), (1.0, 5, (1, 1))):
        S = _grey(*shape, value)
        G, d = LR.gain(S, 1, s, KEY, 0.6, 0.8, 4.0)
        l = int(d["l"][0, 0])
        assert (d["l"] == l).all() and (d["B"] == l / 256.0 - 16.0).all(), value  # exactly: the division N / D is l's
        dist = (l / 256.0 - 16.0) - float(np.float32(KEY))
        g = min(max((float(np.float32(0.6 if dist > 0 else 0.8)) - 1.0) * dist, -4.0), 4.0)
        assert (_bits(G) == _bits(np.float32(MR.exp2_spec(g)))).all(), value
    # l by hand: Y = 1 is 16 octaves above 2^-16, Y = 1.5 half an octave further in the piecewise-linear log
    assert LR.fixed_log(np.array([1.0, 1.5, 2.0 ** -16, 2.0 ** -17, 2.0 ** 16, 3e38], np.float32))[1].tolist() == [4096, 4224, 0, 0, 8191, 8191]
    # the bound of step 4 on its worst case: a full 64 x 64 cell of the largest l, alone in its grid, so every clamped neighbour is itself
    S = _grey(64, 64, 3e38)
    _, d = LR.gain(S, 1, 6)
    total, cnt = d["blurred_sum"], d["blurred_cnt"]
    assert (total == LR.blur(d["sum"])).all() and d["sum"].max() == 4096 * 8191
    # along x and y every neighbour is the cell itself (16 of it); along z slice 30 is empty and the clamped neighbour is slice 31 (3 of it)
    assert total.max() == 4096 * 8191 * 48 <= 4096 * 8191 * 64 == 2147221504 < 2 ** 32 and cnt.max() == 4096 * 48


def test_known_answers_c_a_power_of_two_shifts_the_base_by_that_many_stops():
    rng = np.random.default_rng(9)
    S = _grey(40, 52, 2.0 ** rng.uniform(-4, 4, (40, 52)))
    S[7, 9, :3] = 0.0
    _, base = LR.gain(S, 1, 3)
    for k in (-9, -1, 1, 3, 9):
        _, d = LR.gain(S * np.float32(2.0 ** k), 1, 3)
        assert (d["l"][d["counted"]] == base["l"][base["counted"]] + 256 * k).all() and (d["counted"] == base["counted"]).all()
        # N gains 256 k D exactly; the quotient is rounded once more at another magnitude, 2^-53 of at most 8191
        assert np.abs((d["B"] - base["B"])[d["counted"]] - k).max() <= 2.0 ** -40


def test_known_answers_d_two_plateaus_three_octaves_apart_get_their_own_gain_up_to_the_edge():
    for s, octaves, cut in ((3, 3, 21), (5, 3, 33), (4, 7, 16), (3, -3, 5)):
        lo, hi = 0.05, 0.05 * 2.0 ** octaves
        S = _grey(40, 70, lo)
        S[:, cut:, :3] = np.float32(hi)
        G, _ = LR.gain(S, 1, s, KEY, 0.5, 0.75, 6.0)
        for region, value in ((np.s_[:, :cut], lo), (np.s_[:, cut:], hi)):
            alone, _ = LR.gain(_grey(1, 1, value), 1, s, KEY, 0.5, 0.75, 6.0)
            assert (_bits(G[region]) == _bits(alone[0, 0])).all(), (s, octaves)  # the other plateau does not reach it: no halo
    # two octaves apart the blurred slices meet, and the edge shows: the limit is where the header puts it
    S = _grey(40, 70, 0.05)
    S[:, 33:, :3] = np.float32(0.2)
    G, _ = LR.gain(S, 1, 5, KEY, 0.5, 0.75, 6.0)
    assert len(np.unique(G[:, :33])) > 1


def test_known_answers_e_the_fixed_point_log_against_numpy_log2_on_a_luminance_ramp():
    """The piecewise-linear log2 e + m lies in [0, 0.0861] below log2 Y, and l / 256 - 16 is that value with m cut to eight bits: in
    [0, 1 / 256) below it.  The header's 0.0861 is the first figure; on a constant image the gain therefore moves by at most
    |c - 1| (0.0861 + 1 / 256) stops against the exact logarithm.  Both parts are asserted, on 2^16 luminances across [2^-16, 2^16) and on
    every one of the 8,192 steps, where the second part vanishes."""
    Y = (2.0 ** np.linspace(-16, 16, 65536, endpoint=False)).astype(np.float32)
    counted, l = LR.fixed_log(Y)
    assert counted.all() and (np.diff(l) >= 0).all() and l[0] == 0 and l[-1] == 8191
    mant, expo = np.frexp(Y.astype(np.float64))
    linear = (expo - 1) + (2.0 * mant - 1.0)  # e + m
    exact = np.log2(Y.astype(np.float64))
    gap = exact - linear
    assert gap.min() >= -1e-12 and gap.max() <= LR.LOG_GAP and gap.max() > 0.086
    cut = linear - (l / 256.0 - 16.0)
    assert cut.min() >= 0.0 and cut.max() < 1.0 / 256.0
    steps = np.ldexp(1.0 + (np.arange(8192) % 256) / 256.0, np.arange(8192) // 256 - 16).astype(np.float32)  # the lower end of every step: exact in float32
    counted, ls = LR.fixed_log(steps)
    assert counted.all() and (ls == np.arange(8192)).all()
    on_steps = np.log2(steps.astype(np.float64)) - (ls / 256.0 - 16.0)
    assert on_steps.min() >= 0.0 and on_steps.max() <= LR.LOG_GAP
    assert np.abs(np.diff(on_steps)).max() <= 1.5 / 256.0  # smooth: no jump at an octave's end either
    # through the whole stage: constant images along the ramp against the gain of the exact logarithm
    for c in (0.6, 0.25, 1.5):
        for y in Y[:: 4099]:
            S = np.zeros((2, 3, 4), np.float32)
            S[..., 1] = np.float32(y) / np.float32(0.7152)
            G, d = LR.gain(S, 1, 5, 0.0, c, c, 64.0)
            ideal = (float(np.float32(c)) - 1.0) * float(np.log2(np.float64(d["Y"][0, 0])))
            assert abs(float(_log2(G)[0, 0]) - ideal) <= abs(float(np.float32(c)) - 1.0) * (LR.LOG_GAP + 1.0 / 256.0) + 2.0 ** -22, (c, y)


def test_two_textured_plateaus_keep_their_detail_and_move_together():
    """Two plateaus five octaves apart, each with a texture of +-4 % that stays inside its octave's slice.  B(p) is a weighted mean of
    the l of the pixel's own plateau (the other one shares no slice with it), so it lies within that plateau's [l_min, l_max]; two
    pixels away from the edges see whole cells of equal counts, where B is the bilinear interpolation of the cell means and one
    pixel's step moves 1 / 2^s of the weight between two of them.  Hence: neighbouring interior pixels' gains differ by at most
    |c - 1| (l_max - l_min) / 256 / 2^s stops -- their ratio is unchanged to that -- and the plateaus' mean gains differ by (c - 1) times
    the five octaves to within |c - 1| times the texture's range."""
    s, c, cut, octaves = 4, 0.6, 96, 5
    rng = np.random.default_rng(23)
    h, w = 96, 192
    tex = 1.0 + rng.uniform(-0.04, 0.04, (h, w))
    value = np.where(np.arange(w)[None, :] < cut, 0.35, 0.35 * 2.0 ** octaves) * tex
    S = _grey(h, w, value)
    G, d = LR.gain(S, 1, s, -6.0, c, c, 16.0)  # the pivot below both: one contrast
    lg = _log2(G)
    cm1 = abs(float(np.float32(c)) - 1.0)
    means = []
    for x0, x1 in ((0, cut), (cut, w)):
        l = d["l"][:, x0:x1]
        assert len(np.unique(l >> 8)) == 1
        spread = (l.max() - l.min()) / 256.0
        assert 0.08 < spread < 0.13
        B = d["B"][:, x0:x1]
        assert B.min() >= l.min() / 256.0 - 16.0 and B.max() <= l.max() / 256.0 - 16.0
        inner = lg[2 << s: h - (2 << s), x0 + (2 << s): x1 - (2 << s)]
        bound = cm1 * spread / (1 << s) + 2.0 ** -22
        assert np.abs(np.diff(inner, axis=1)).max() <= bound and np.abs(np.diff(inner, axis=0)).max() <= bound
        assert np.abs(np.diff(np.log2(value[:, x0:x1]), axis=1)).max() > 20 * bound  # the texture itself is far larger
        means.append((inner.mean(), spread))
    moved = means[1][0] - means[0][0]
    assert abs(moved - (float(np.float32(c)) - 1.0) * octaves) <= cm1 * max(means[0][1], means[1][1]) + 2.0 ** -22
    assert moved < -1.9  # the scene's five octaves become three


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


def _specials(S):
    """NaN, Inf, negative, zero and denormal pixels; positions wrap, so every extent gets what fits"""
    h, w = S.shape[:2]

    def put(y, x, rgb):
        S[y % h, x % w, 0:3] = rgb
    if h * w >= 12:
        put(2, 3, (np.nan, 1.0, 1.0))
        put(4, 5, (1.0, np.inf, 1.0))
        put(6, 2, (np.inf, -np.inf, 0.0))
        put(8, 9, (-3.0, -2.0, -1.0))
        put(1, 1, (1e-41, 1e-41, 1e-41))
        put(9, 1, (-0.0, -0.0, -0.0))
        put(0, 7, (0.0, 0.0, 0.0))
        put(5, 12, 3e38)
    return S


def _synthetic(h, w, seed=31):
    """A frame spanning 40 octaves: a smooth diagonal ramp from 2^-20 to 2^20 under a texture of +-1 stop, with an opening of
    2^12 in an interior of 2^-3, so that cells hold several slices and slices at both ends of the range are clamped"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    ramp = -20.0 + 40.0 * (xx + yy) / max(1, w + h - 2)
    S = (2.0 ** (ramp[..., None] + rng.uniform(-1, 1, (h, w, 4)))).astype(np.float32)
    if h >= 20 and w >= 20:
        S[h // 4: h // 2, w // 4: w // 2, :3] = (2.0 ** (-3 + rng.uniform(-0.2, 0.2, (h // 2 - h // 4, w // 2 - w // 4, 3)))).astype(np.float32)
        S[h // 3: h // 3 + 5, w // 3: w // 3 + 7, :3] = np.float32(2.0 ** 12)
    S[..., 3] = 2.0
    return _specials(S)


_sums = {}


def _sum(pkg, w, h, kind):
    """The frame of `kind` (render8, synthetic) at w x h, with the special pixels in"""
    key = (w, h, kind)
    if key not in _sums:
        if kind == "synthetic":
            _sums[key] = _synthetic(h, w)
        else:
            s, r = _gpu(pkg)
            r.set_tile_shard(0, 1, 32)
            r.resize(w, h)
            u = s.uniform(w, h, bounces=4)
            for f in range(8):
                u.TotalSamples = f
                r.render(u, s.lights)
            _sums[key] = _specials(r.readback())
    return _sums[key]


def _plain(pkg, w, h, S=None):
    """a handle with no scene: ptx_local_exposure needs none"""
    import torch  # noqa: F401

    f = pkg.Renderer()
    f.resize(w, h)
    if S is not None:
        f.write_accumulation(S)
    return f


def _borrower(pkg, w, h, S=None, u=None):
    b = pkg.Renderer()
    b.share_scene(_gpu(pkg)[1])
    b.resize(w, h)
    if S is not None:
        b.write_accumulation(S)
    if u is not None:
        b.render_guides(u)
    return b


PARAMS = (dict(pivot_log2=KEY, highlight_contrast=0.6, shadow_contrast=0.8, max_stops=4.0),
          dict(pivot_log2=1.5, highlight_contrast=0.0, shadow_contrast=2.0, max_stops=2.5),
          dict(pivot_log2=-4.0, highlight_contrast=1.75, shadow_contrast=0.25, max_stops=40.0))
METER = dict(key_log2=KEY, low_permille=10, high_permille=10)


def _assert_gain(r, S, total_samples, what, cur=None, denoised=False, **p):
    G = r.read_local_exposure()
    ref, d = LR.gain(S, total_samples, cur=cur, denoised=denoised, **p)
    same = _bits(G) == _bits(ref)
    assert same.all(), (what, int((~same).sum()), np.argwhere(~same)[:4].tolist(), G[~same][:4], ref[~same][:4])
    return G, d


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["synthetic", "render8"])
@pytest.mark.parametrize("case", list(CASES))
def test_gain_equals_the_reference_bit_for_bit(pkg, case, kind):
    w, h, s = CASES[case]
    S = _sum(pkg, w, h, kind)
    ts = 8 if kind == "render8" else 1
    r = _plain(pkg, w, h, S)
    for p in PARAMS:
        r.local_exposure(ts, cell_shift=s, **p)
        G, d = _assert_gain(r, S, ts, (case, kind, p), cell_shift=s, **p)
    if w * h >= 3000:
        assert (~d["counted"]).sum() >= 6 and (G[~d["counted"]] == 1).all() and len(np.unique(G)) > 100
        if kind == "synthetic":
            assert d["l"][d["counted"]].min() == 0 and d["l"][d["counted"]].max() == 8191  # both ends of the range are clamped
    # the pivot on the display's side: the meter's cur comes off it, on the device
    m = MR.Meter()
    r.meter(ts, **METER)
    m.meter(S, ts, **METER)
    if m.result["valid"]:
        assert r.read_meter().log2Exposure == m.result["log2Exposure"] and m.cur != 0.0
    r.local_exposure(ts, cell_shift=s, pivot_metered=True, **PARAMS[0])
    _assert_gain(r, S, ts, (case, kind, "metered"), cell_shift=s, cur=m.cur, **PARAMS[0])
    assert (_bits(r.readback()) == _bits(S)).all()  # the image is only read
    assert r.local_exposure_ptr()
    r.close()


@pytest.mark.gpu
def test_the_three_sources_and_a_borrower(pkg):
    s, _ = _gpu(pkg)
    S = _sum(pkg, W, H, "render8")
    u = s.uniform(W, H, bounces=4)
    r = _borrower(pkg, W, H, S, u)
    r.despike(radius=1, rank=2, gain=1.5, min_taps=3)
    r.denoise(8, 2, 1.5, 0.3, 0.03)
    Cc, D = r.read_despiked(), r.read_denoised()
    assert (_bits(Cc) != _bits(S)).any()
    p = dict(PARAMS[0], cell_shift=4)
    seen = []
    for source, image in ((pkg.METER_SUM, S), (pkg.METER_DESPIKED, Cc), (pkg.METER_DENOISED, D)):
        r.local_exposure(8, source=source, **p)
        G, _ = _assert_gain(r, image, 8, source, denoised=source == pkg.METER_DENOISED, **p)
        seen.append(G)
        # two calls in a row are a fresh handle's: nothing of the first call is left in the grid
        r.local_exposure(8, source=source, **dict(p, cell_shift=6))
        r.local_exposure(8, source=source, **p)
        f = _plain(pkg, W, H, image)
        f.local_exposure(1 if source == pkg.METER_DENOISED else 8, **p)
        assert (_bits(r.read_local_exposure()) == _bits(f.read_local_exposure())).all() and (_bits(G) == _bits(f.read_local_exposure())).all(), source
        f.close()
    assert (_bits(seen[0]) != _bits(seen[2])).any()
    for image, read in ((S, r.readback), (Cc, r.read_despiked), (D, r.read_denoised)):
        assert (_bits(image) == _bits(read())).all()
    r.close()


def _plateaus(h, w):
    """four plateaus, each at least three octaves from the others, in quadrants that are no multiple of a cell"""
    S = _grey(h, w, 0.004)
    S[: h // 2 + 3, w // 2 - 5:, :3] = np.float32(0.06)
    S[h // 2 + 3:, : w // 2 - 5, :3] = np.float32(0.9)
    S[h // 2 + 3:, w // 2 - 5:, :3] = (9.0, 11.0, 7.0)
    regions = (np.s_[: h // 2 + 3, : w // 2 - 5], np.s_[: h // 2 + 3, w // 2 - 5:], np.s_[h // 2 + 3:, : w // 2 - 5], np.s_[h // 2 + 3:, w // 2 - 5:])
    return S, regions


@pytest.mark.gpu
def test_postprocess_local_with_unit_gain_is_the_plain_call_and_the_metered_one(pkg):
    s, _ = _gpu(pkg)
    S = _sum(pkg, W, H, "synthetic")
    u = s.uniform(W, H, bounces=4)
    r = _borrower(pkg, W, H, S, u)
    r.despike(radius=1, rank=2, gain=1.5, min_taps=3)
    r.denoise(2, 2, 1.5, 0.3, 0.03)
    r.meter(2, key_log2=1.0, low_permille=50, high_permille=50)
    assert r.read_meter().exposure != 1.0
    screens = ((W, H, pkg.PRESENT_R8G8B8A8_SRGB, 0), (100, 37, pkg.PRESENT_R16G16B16A16_SFLOAT, 0))
    for source, plain in ((pkg.METER_SUM, r.postprocess), (pkg.METER_DESPIKED, r.postprocess_despiked), (pkg.METER_DENOISED, r.postprocess_denoised)):
        r.local_exposure(2, source=source, highlight_contrast=1.0, shadow_contrast=1.0)
        assert (_bits(r.read_local_exposure()) == 0x3F800000).all()
        for tone in (pkg.TONE_MAPPING_SDR, pkg.TONE_MAPPING_HDR):
            for metered in (False, True):
                r.postprocess_local(2, tone_mapping=tone, source=source, metered=metered, **POST)
                got = [r.read_output(pkg.OUTPUT_RGBA32F), r.read_output(pkg.OUTPUT_RGBA8_SRGB)]
                for sw, sh, fmt, mode in screens:
                    r.present(sw, sh, fmt, mode)
                    got.append(r.read_present())
                if metered:
                    r.postprocess_metered(2, tone_mapping=tone, source=source, **POST)
                else:
                    plain(2, tone_mapping=tone, **POST)
                want = [r.read_output(pkg.OUTPUT_RGBA32F), r.read_output(pkg.OUTPUT_RGBA8_SRGB)]
                for sw, sh, fmt, mode in screens:
                    r.present(sw, sh, fmt, mode)
                    want.append(r.read_present())
                for k, (a, b) in enumerate(zip(got, want)):
                    assert a.dtype == b.dtype and (a.view(np.uint8) == b.view(np.uint8)).all(), (source, tone, metered, k)
    r.close()


@pytest.mark.gpu
def test_postprocess_local_without_bloom_is_the_plain_call_at_each_plateau_s_exposure(pkg):
    """A bloom threshold above every value leaves the bloom images zero, so a pixel's output depends on that pixel alone: every pixel of
    a plateau equals plain ptx_postprocess at Exposure = float(float(Exposure m) G) of that plateau, bit for bit; ptx_read_output in both
    formats, ptx_grade and ptx_present follow."""
    w, h = 130, 70
    S, regions = _plateaus(h, w)
    post = dict(exposure=1.25, bloom_threshold=1e6, bloom_intensity=0.35)
    p = dict(cell_shift=3, pivot_log2=KEY, highlight_contrast=0.5, shadow_contrast=0.7, max_stops=5.0)
    r, f = _plain(pkg, w, h, S), _plain(pkg, w, h, S)
    r.meter(1, **METER)
    m = np.float32(r.read_meter().exposure)
    assert m != 1.0
    for metered in (False, True):
        r.local_exposure(1, pivot_metered=metered, **p)
        G = r.read_local_exposure()
        gains = [G[reg] for reg in regions]
        assert all(len(np.unique(g)) == 1 for g in gains) and len({float(g[0, 0]) for g in gains}) == 4  # (d): one gain a plateau, up to its edges
        for tone in (pkg.TONE_MAPPING_SDR, pkg.TONE_MAPPING_HDR):
            r.postprocess_local(1, tone_mapping=tone, metered=metered, **post)
            got = (r.read_output(pkg.OUTPUT_RGBA32F), r.read_output(pkg.OUTPUT_RGBA8_SRGB))
            r.grade(tone, saturation=0.5, curve=pkg.CURVE_REINHARD)
            got += (r.read_output(pkg.OUTPUT_RGBA32F),)
            r.present(w, h, pkg.PRESENT_R16G16B16A16_SFLOAT if tone else pkg.PRESENT_R8G8B8A8_SRGB, tone)
            got += (r.read_present().reshape(h, w, -1),)
            for reg, g in zip(regions, gains):
                e = (np.float32(post["exposure"]) * (m if metered else np.float32(1.0))) * g[0, 0]
                f.postprocess(1, tone_mapping=tone, **dict(post, exposure=float(e)))
                want = (f.read_output(pkg.OUTPUT_RGBA32F), f.read_output(pkg.OUTPUT_RGBA8_SRGB))
                f.grade(tone, saturation=0.5, curve=pkg.CURVE_REINHARD)
                want += (f.read_output(pkg.OUTPUT_RGBA32F),)
                f.present(w, h, pkg.PRESENT_R16G16B16A16_SFLOAT if tone else pkg.PRESENT_R8G8B8A8_SRGB, tone)
                want += (f.read_present().reshape(h, w, -1),)
                for k, (a, b) in enumerate(zip(got, want)):
                    assert (a[reg].view(np.uint8) == b[reg].view(np.uint8)).all(), (metered, tone, k)
    r.close()
    f.close()


@pytest.mark.gpu
def test_postprocess_local_with_bloom_against_the_float64_bloom_reference(pkg):
    """tests/bloom_ref.py fed the per-pixel exposure float(Exposure G(p)), under tests/test_bloom.py's rule: the device may be off the
    float64 reference by 8 times what the float32 reference is off it, or by half a binary16 ulp (2^-11 relative, of at least 1)."""
    w, h = 67, 45
    S = _sum(pkg, w, h, "render8").copy()
    S[np.abs(S[..., :3]).max(axis=-1) > 1e30] = 1.0  # NaN, Inf and 3e38: the markers of non-finite pixels have tests/test_bloom.py's leg of their own
    S[~np.isfinite(S).all(axis=-1)] = 1.0
    S[..., :3] *= np.float32(6.0)  # bright enough for the knee
    r = _plain(pkg, w, h, S)
    p = dict(cell_shift=3, pivot_log2=0.0, highlight_contrast=0.4, shadow_contrast=1.6, max_stops=3.0)
    r.local_exposure(8, **p)
    G, _ = _assert_gain(r, S, 8, "bloom", **p)
    assert len(np.unique(G)) > 50
    post = dict(exposure=1.25, bloom_threshold=0.8, bloom_intensity=3.0)
    r.postprocess_local(8, tone_mapping=pkg.TONE_MAPPING_HDR, **post)
    got = r.read_output(pkg.OUTPUT_RGBA32F)
    per_pixel = (np.float32(post["exposure"]) * G)[..., None]
    ref64 = BR.composed(S, 8, per_pixel, post["bloom_threshold"], post["bloom_intensity"], np.float64)
    ref32 = BR.composed(S, 8, per_pixel, post["bloom_threshold"], post["bloom_intensity"], np.float32).astype(np.float64)
    worst = float(np.abs(ref32 - ref64).max())
    d = np.abs(got[..., :3].astype(np.float64) - ref64)
    tol = np.maximum(8.0 * worst, 2.0 ** -11 * np.maximum(1.0, np.abs(ref64)))
    print("max |device - ref64| %.3e, float32 reference %.3e" % (float(d.max()), worst))
    assert np.isfinite(got).all() and (got[..., 3] == 1).all() and (d <= tol).all(), float(d.max())
    flat = BR.composed(S, 8, post["exposure"], post["bloom_threshold"], post["bloom_intensity"], np.float64)
    assert np.abs(flat - ref64).max() > 0.1  # the gain is in the picture
    r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("leg", ["sum", "denoised"])
def test_renderer_hip_with_local_exposure_settings_on_is_the_same_calls_made_by_hand(pkg, tmp_path_factory, tmp_path, leg):
    """test_motion's driver (examples/motion_frame.cpp, compiled once per session) with the exposure argument at 2: ExposureSettings and
    LocalExposureSettings on.  Two frames of animated_test through RendererHip; the sum and the output image of both equal ptx_meter,
    ptx_local_exposure with PTX_LOCAL_EXPOSURE_PIVOT_METERED at the adapter's defaults and ptx_postprocess_local (metered) made by hand,
    bit for bit, on the sum and -- with the denoiser on -- on the denoised image, and differ from the metered call's.  Without the
    denoiser the driver saves every frame twice, the second time with the time step used up."""
    import subprocess

    import test_motion as TM

    w, h, spp, depth, step = W, H, 2, 4, 0.37
    denoiser = int(leg == "denoised")
    exe = TM._motion_frame_driver(pkg, tmp_path_factory)
    dump = tmp_path / "frames.bin"
    subprocess.check_call([exe, "animated_test", str(w), str(h), str(spp), str(depth), str(step), "0", str(dump), "0", "0", str(denoiser), "2"])
    got = np.fromfile(dump, np.float32).reshape(2, 3, h, w, 4)
    s = pkg.Scene("animated_test", DETAIL)
    s.update(0.0)
    r = pkg.Renderer()
    r.upload(s)
    if denoiser:
        r.track_motion(True)
    r.resize(w, h)
    source = pkg.METER_DENOISED if denoiser else pkg.METER_SUM
    for frame in range(2):
        if frame:
            assert s.update(step)
        it, bn = s.animation_state()
        r.update_animation(it, bn if len(bn) else None)
        r.reset()
        for f in range(spp):
            r.render(s.uniform(w, h, bounces=depth, sample_count=1, total_samples=f), s.lights)
        if denoiser:
            r.render_guides_motion(s.uniform(w, h, bounces=depth, sample_count=1, total_samples=spp))
            view, proj = s.camera_matrices(w, h)
            r.temporal_accumulate_motion(spp, view, proj, max_history=32.0, normal_threshold=0.3, position_threshold=0.03)
            r.denoise_temporal(iterations=3, sigma_color=1.5, sigma_normal=0.3, sigma_position=0.03)
        for dt in (step,) if denoiser else (step, 0.0):  # the driver's second SaveOutput of the frame
            r.meter(spp, delta_seconds=dt, source=source)
            r.local_exposure(spp, source=source, pivot_metered=True)  # LOCAL_EXPOSURE_DEFAULTS are the adapter's (the header test holds them together)
            r.postprocess_local(spp, 1.0, 1.0, 1.0, pkg.TONE_MAPPING_SDR, source=source, metered=True)
        S, out = r.readback(), r.read_output(pkg.OUTPUT_RGBA32F)
        assert (_bits(got[frame][0]) == _bits(S)).all() and (_bits(got[frame][2]) == _bits(out)).all(), frame
        G = r.read_local_exposure()
        assert len(np.unique(G)) > 50
        r.postprocess_metered(spp, 1.0, 1.0, 1.0, pkg.TONE_MAPPING_SDR, source=source)
        assert (_bits(r.read_output(pkg.OUTPUT_RGBA32F)) != _bits(out)).any()
    r.close()


@pytest.mark.gpu
def test_resize_drops_the_gain_and_refusals_leave_it_intact(pkg):
    import torch

    s, _ = _gpu(pkg)
    S = _sum(pkg, W, H, "render8")
    r = pkg.Renderer()  # an owner of its own: tile shards and bound buffers are refused on it
    r.upload(s)
    r.resize(W, H)
    lib = r.lib
    post = pkg.PostProcessingUniformData(8, 1.0, 1.0, 1.0)
    host = np.empty((H, W), np.float32)
    # the accessors before any ptx_local_exposure
    assert lib.ptx_read_local_exposure(r.handle, host.ctypes.data, host.nbytes) == NOT_READY and not lib.ptx_device_local_exposure_ptr(r.handle)
    assert lib.ptx_postprocess_local(r.handle, C.byref(post), 0, 0, 0) == NOT_READY
    r.write_accumulation(S)

    def call(handle=r.handle, **over):
        p = dict(source=0, totalSamples=8, cellShift=4, pivotLog2=KEY, highlightContrast=0.6, shadowContrast=0.8, maxStops=4.0, flags=0, reserved=0)
        p.update(over)
        d = pkg.LocalExposureDesc(**p)
        return lib.ptx_local_exposure(handle, C.byref(d))

    assert call(flags=1) == NOT_READY and not r.local_exposure_ptr()  # PIVOT_METERED without a meter
    assert call() == OK
    kept = r.read_local_exposure()
    assert len(np.unique(kept)) > 50

    def intact():
        assert (_bits(r.read_local_exposure()) == _bits(kept)).all()

    nan, inf = float("nan"), float("inf")
    bad = [dict(source=3), dict(totalSamples=0), dict(cellShift=2), dict(cellShift=7), dict(cellShift=0), dict(cellShift=4000000000), dict(flags=2), dict(flags=3),
           dict(reserved=1), dict(highlightContrast=-0.01), dict(highlightContrast=2.01), dict(shadowContrast=-1.0), dict(shadowContrast=3.0), dict(maxStops=-0.5)]
    bad += [{f: v} for f in ("pivotLog2", "highlightContrast", "shadowContrast", "maxStops") for v in (nan, inf, -inf)]
    for b in bad:  # G is read back after every single refusal, before anything is accepted again
        assert call(**b) == INVALID, b
        intact()
    for refused in (lambda: lib.ptx_local_exposure(r.handle, None), lambda: call(handle=None),
                    lambda: lib.ptx_read_local_exposure(r.handle, None, host.nbytes), lambda: lib.ptx_read_local_exposure(None, host.ctypes.data, host.nbytes),
                    lambda: lib.ptx_read_local_exposure(r.handle, host.ctypes.data, host.nbytes - 4),
                    lambda: lib.ptx_postprocess_local(r.handle, None, 0, 0, 0), lambda: lib.ptx_postprocess_local(None, C.byref(post), 0, 0, 0),
                    lambda: lib.ptx_postprocess_local(r.handle, C.byref(post), 2, 0, 0), lambda: lib.ptx_postprocess_local(r.handle, C.byref(post), 0, 3, 0),
                    lambda: lib.ptx_postprocess_local(r.handle, C.byref(post), 0, 0, 2)):
        assert refused() == INVALID
        intact()
    assert not lib.ptx_device_local_exposure_ptr(None)
    # a source that does not exist (no C, no D), a meter that does not exist
    for refused in (lambda: call(source=1), lambda: call(source=2), lambda: call(flags=1), lambda: lib.ptx_postprocess_local(r.handle, C.byref(post), 0, 1, 0),
                    lambda: lib.ptx_postprocess_local(r.handle, C.byref(post), 0, 2, 0), lambda: lib.ptx_postprocess_local(r.handle, C.byref(post), 0, 0, 1)):
        assert refused() == NOT_READY
        intact()
    assert lib.ptx_postprocess_local(r.handle, C.byref(post), 0, 0, 0) == OK
    # a tile shard of a larger world, a bound shard buffer
    r.set_tile_shard(0, 2, 8)
    assert call() == NOT_READY and lib.ptx_postprocess_local(r.handle, C.byref(post), 0, 0, 0) == NOT_READY
    intact()
    shard = torch.zeros(r.shard_bytes(0) // 4, dtype=torch.float32, device="cuda")
    r.bind_shard_accumulation(shard.data_ptr(), r.shard_bytes(0))
    assert call() == NOT_READY and lib.ptx_postprocess_local(r.handle, C.byref(post), 0, 0, 0) == NOT_READY
    intact()
    r.bind_shard_accumulation(0)
    r.set_tile_shard(0, 1, 32)
    intact()
    # the limits themselves are accepted
    assert call(cellShift=3, highlightContrast=0.0, shadowContrast=2.0, maxStops=0.0) == OK and call(cellShift=6, highlightContrast=2.0, shadowContrast=0.0) == OK
    # no image
    fresh = pkg.Renderer()
    assert call(handle=fresh.handle) == NOT_READY and lib.ptx_read_local_exposure(fresh.handle, host.ctypes.data, host.nbytes) == NOT_READY
    fresh.close()
    # ptx_resize drops G: the accessors and the output call are back where they were, C of the old extent does not count
    r.despike()
    assert call(source=1) == OK and r.local_exposure_ptr()
    r.resize(W, H)
    assert not r.local_exposure_ptr() and lib.ptx_read_local_exposure(r.handle, host.ctypes.data, host.nbytes) == NOT_READY
    assert lib.ptx_postprocess_local(r.handle, C.byref(post), 0, 0, 0) == NOT_READY and call(source=1) == NOT_READY
    r.write_accumulation(S)
    assert call() == OK
    intact()  # and the same call on the same image at the new extent gives the same G
    r.close()
