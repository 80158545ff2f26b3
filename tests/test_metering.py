"""Exposure metering (include/ptx.h "Exposure metering": ptx_meter, ptx_read_meter, ptx_device_meter_ptr, ptx_meter_reset,
ptx_postprocess_metered; csrc/pt_meter.hpp, docs/NEXT_ROWS.md section 21) against tests/meter_ref.py.

Tolerance: none.  Bins and counters are integers; avgLog2, targetLog2 and log2Exposure come from IEEE double operations in the order the
header states, and exposure goes through the project's exp2 kernel, restated in the reference as tests/test_transcendentals.py
restates it -- so the device's result equals the reference bit for bit on the device's own read-back image.  Extents: 1 x 1, 3 x 2,
33 x 9, 67 x 45, 300 x 200 and 1024 x 600: 2,400 workgroups' worth of pixels over a grid capped at 1,024, so that workgroups stride."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

import meter_ref as MR

DETAIL = 0.25
SCENE = "texture_test"
EXTENTS = {"1x1": (1, 1), "3x2": (3, 2), "33x9": (33, 9), "67x45": (67, 45), "300x200": (300, 200), "1024x600": (1024, 600)}
W, H = EXTENTS["67x45"]
POST = dict(exposure=1.25, bloom_threshold=0.8, bloom_intensity=0.35)
OK, INVALID, NOT_READY = 0, 1, 5
INTS = ("counted", "kept", "black", "rejected", "under", "over", "valid", "calls")
FLOATS = ("exposure", "log2Exposure", "avgLog2", "targetLog2")
KEY = float(np.log2(0.18))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _const(h, w, value, alpha=1.0):
    S = np.empty((h, w, 4), np.float32)
    S[..., 0:3] = value
    S[..., 3] = alpha
    return S


def _grey(y, n=1):
    """1 x n pixels whose luminance is exactly the float32 y: only green is lit and 0.7152f g is searched for y"""
    y = np.float32(y)
    g = np.float32(y) / np.float32(0.7152)
    for _ in range(64):
        got = np.float32(0.7152) * g
        if got == y:
            break
        g = np.nextafter(g, np.float32(np.inf) if got < y else np.float32(-np.inf))
    assert np.float32(0.7152) * g == y, y
    S = np.zeros((1, n, 4), np.float32)
    S[..., 1] = g
    return S


# =====================================================================================================
# without a GPU
# =====================================================================================================
def test_header_declares_and_package_exports_the_exposure_metering(pkg):
    header = open(os.path.join(pkg.REPO_DIR, "include", "ptx.h")).read()
    decls = {
        "ptx_meter": r"PTX_API int ptx_meter\(PtxRenderer \*r, const PtxMeterDesc \*desc\);",
        "ptx_read_meter": r"PTX_API int ptx_read_meter\(PtxRenderer \*r, PtxMeterResult \*out, uint32_t \*bins256 /\* may be NULL \*/\);",
        "ptx_device_meter_ptr": r"PTX_API void \*ptx_device_meter_ptr\(PtxRenderer \*r\);",
        "ptx_meter_reset": r"PTX_API int ptx_meter_reset\(PtxRenderer \*r\);",
        "ptx_postprocess_metered": r"PTX_API int ptx_postprocess_metered\(PtxRenderer \*r, const PtxPostProcessingUniformData \*u, uint32_t toneMappingMode, uint32_t source\);",
    }
    lib = pkg.load_hip()
    for name, decl in decls.items():
        assert re.search(decl, header), name
        assert name in pkg.PTX_SYMBOLS
        assert hasattr(lib, name), name
    assert "#define PTX_ABI_VERSION 5u" in header and "PTX_FN_COUNT = 38" in header  # additions only
    desc_fields = ("source", "mode", "totalSamples", "region", "lowPermille", "highPermille", "keyLog2", "compensation", "minLog2Exposure", "maxLog2Exposure",
                   "speedUp", "speedDown", "deltaSeconds", "flags", "reserved")
    body = re.search(r"typedef struct PtxMeterDesc \{(.*?)\} PtxMeterDesc;", header, re.S)[1]
    assert tuple(re.findall(r"^\s*(?:uint32_t|float)\s+(\w+)(?:\[4\])?;", body, re.M)) == desc_fields
    D = pkg.MeterDesc
    assert C.sizeof(D) == 72 and [getattr(D, f).offset for f in desc_fields] == [0, 4, 8, 12, 28, 32, 36, 40, 44, 48, 52, 56, 60, 64, 68]
    body = re.search(r"typedef struct PtxMeterResult \{(.*?)\} PtxMeterResult;", header, re.S)[1]
    assert tuple(re.findall(r"^\s*(?:uint32_t|float)\s+(\w+);", body, re.M)) == FLOATS + INTS
    Rs = pkg.MeterResult
    assert C.sizeof(Rs) == 48 and [getattr(Rs, f).offset for f in FLOATS + INTS] == list(range(0, 48, 4))
    assert (pkg.METER_SUM, pkg.METER_DESPIKED, pkg.METER_DENOISED) == (0, 1, 2) == (MR.SUM, MR.DESPIKED, MR.DENOISED)
    assert (pkg.METER_AVERAGE, pkg.METER_CENTRE, pkg.METER_REGION) == (0, 1, 2) == (MR.AVERAGE, MR.CENTRE, MR.REGION)
    for k, name in enumerate(("PTX_METER_SUM", "PTX_METER_DESPIKED", "PTX_METER_DENOISED")):
        assert re.search(rf"{name} = {k}\b", header)
    for k, name in enumerate(("PTX_METER_AVERAGE", "PTX_METER_CENTRE", "PTX_METER_REGION")):
        assert re.search(rf"{name} = {k}\b", header)
    # the semantics are in the header as text: the reference is written from it
    for phrase in ("Exposure metering", "section 21", "1. LUMINANCE", "(0.2126f c.r + 0.7152f c.g) + 0.0722f c.b", "2. CLASSES", "REJECTED iff Y is not finite",
                   "BLACK iff Y <= 0 or Y < 2^-126", "3. BIN", "k = bits(Y) >> 20", "i = k - 888", "Y = 1 lands in bin 128", "4. WEIGHT",
                   "wx = 1 + [W <= 4x + 2 <= 3W] + [3W <= 8x + 4 <= 5W]", "a pixel of weight 0 belongs to no class", "reaches 2^32 is refused", "5. TRIM",
                   "kept_i = max(0, min(P_i + n_i, N - hi) - max(P_i, lo))", "6. MEAN", "log2(1 + (2j + 1) / 16)", "/ (double)K - 16", "7. TARGET", "8. ADAPTATION",
                   "1.4426950408889634", "cur = cur + (target - cur) a", "9. STATE", "never synchronises", "6.25 %", "32 octaves", "sharded frames are refused",
                   "no scotopic shift", "A refused call leaves the state and the", "ptx_resize resets the state"):
        assert phrase in header, phrase
    for method in ("meter", "read_meter", "meter_ptr", "meter_reset", "postprocess_metered"):
        assert callable(getattr(pkg.Renderer, method))
    # the adapter's defaults are the package's
    d = pkg.METER_DEFAULTS
    assert set(d) == {"mode", "key_log2", "compensation", "min_log2_exposure", "max_log2_exposure", "speed_up", "speed_down", "low_permille", "high_permille"}
    host = open(os.path.join(pkg.PKG_DIR, "host", "RendererHip.h")).read()
    m = re.search(r"struct ExposureSettings\s*\{\s*bool Enabled = false;\s*uint32_t Mode = (\d+);[^\n]*\n\s*float KeyLog2 = (-?[0-9.]+)f;[^\n]*\n\s*"
                  r"float Compensation = (-?[0-9.]+)f;\s*float MinLog2Exposure = (-?[0-9.]+)f;\s*float MaxLog2Exposure = (-?[0-9.]+)f;\s*"
                  r"float SpeedUp = ([0-9.]+)f;\s*float SpeedDown = ([0-9.]+)f;\s*uint32_t LowPermille = (\d+);\s*uint32_t HighPermille = (\d+);\s*\};", host)
    assert m, "ExposureSettings"
    assert (int(m[1]), float(m[2]), float(m[3]), float(m[4]), float(m[5]), float(m[6]), float(m[7]), int(m[8]), int(m[9])) == (
        d["mode"], d["key_log2"], d["compensation"], d["min_log2_exposure"], d["max_log2_exposure"], d["speed_up"], d["speed_down"], d["low_permille"],
        d["high_permille"])
    assert np.float32(d["key_log2"]) == np.float32(np.log2(0.18)) and d["low_permille"] + d["high_permille"] < 1000
    adapter = open(os.path.join(pkg.PKG_DIR, "host", "RendererHip.cpp")).read()
    for call in ("ptx_meter(s_Renderer", "ptx_postprocess_metered(s_Renderer"):
        assert call in adapter, call
    assert "--auto-exposure" in open(os.path.join(pkg.REPO_DIR, "examples", "render_scene.cpp")).read()
    kernel = open(os.path.join(pkg.PKG_DIR, "csrc", "pt_meter.hpp")).read()
    for name in ("k_meter_histogram", "k_meter_resolve", "__shared__ uint32_t hist"):
        assert name in kernel, name
    assert "k_postprocess_metered" in open(os.path.join(pkg.PKG_DIR, "csrc", "pt_post.hpp")).read()


def test_the_eight_sub_bin_logarithms_of_the_header_are_the_nearest_doubles(pkg):
    header = open(os.path.join(pkg.REPO_DIR, "include", "ptx.h")).read()
    kernel = open(os.path.join(pkg.PKG_DIR, "csrc", "pt_meter.hpp")).read()
    for j in range(8):
        lit = re.search(rf"T_{j} = (0x1\.[0-9a-f]+p-\d)", header)[1]
        want = float(np.log2(np.float64(1.0) + np.float64(2 * j + 1) / 16.0))
        assert float.fromhex(lit) == want == MR.T[j], j
        assert lit in kernel, j


def test_known_answers_of_the_classes_and_bins():
    f = np.float32

    def one(y):
        rej, blk, cnt, b, un, ov = MR.classify(np.array([y], np.float32))
        return bool(rej[0]), bool(blk[0]), bool(cnt[0]), int(b[0]), bool(un[0]), bool(ov[0])
    assert one(1.0) == (False, False, True, 128, False, False)
    assert one(2.0 ** -16) == (False, False, True, 0, False, False)
    assert one(np.nextafter(f(2.0 ** -16), f(0))) == (False, False, True, 0, True, False)
    assert one(2.0 ** 16) == (False, False, True, 255, False, True)
    assert one(np.nextafter(f(2.0 ** 16), f(0))) == (False, False, True, 255, False, False)
    for y in (np.nan, np.inf, -np.inf):
        assert one(y)[:3] == (True, False, False), y
    for y in (0.0, -0.0, -1.0, -1e-30, -3e38, 1e-39, 1e-45, np.nextafter(f(2.0 ** -126), f(0))):
        assert one(y)[:3] == (False, True, False), y
    assert one(2.0 ** -126) == (False, False, True, 0, True, False)
    assert one(3e38) == (False, False, True, 255, False, True)
    for j in range(1, 8):  # the seven sub-bin edges, and the value one ulp below each
        edge = f(1.0 + j / 8.0)
        assert one(edge)[3] == 128 + j and one(np.nextafter(edge, f(0)))[3] == 128 + j - 1
    for e in range(-16, 16):  # exact powers of two open their octave
        assert one(2.0 ** e)[3:] == (8 * (e + 16), False, False)
    # through the whole of steps 1 - 4: a pixel whose luminance is exactly y
    for y, b in ((1.0, 128), (0.25, 112), (1.125, 129), (2.0 ** -16, 0), (1024.0, 208)):
        bins, counters, dec = MR.histogram(_grey(y), 1)
        assert dec["Y"][0, 0] == f(y) and bins[b] == 1 and bins.sum() == 1 and not any(counters.values()), y
    bins, counters, _ = MR.histogram(_grey(8.0), 8)  # the sum of eight samples of luminance 1
    assert bins[128] == 1
    S = np.array([[[np.nan, 1, 1, 1], [1, np.inf, 1, 1], [np.inf, -np.inf, 0, 1], [0, 0, 0, 1], [-1, -1, -1, 1], [1e-41, 1e-41, 1e-41, 1], [1, 1, 1, np.nan]]], np.float32)
    bins, counters, dec = MR.histogram(S, 1)
    assert counters == dict(black=3, rejected=3, under=0, over=0) and bins.sum() == 1  # alpha is not looked at


def test_a_constant_image_is_exposed_to_within_the_widest_sub_bin():
    m = MR.Meter()
    for value in (0.18, 0.17, 0.19, 0.2, 0.13, 0.12, 3.7, 1e-3):
        m.reset()
        S = _const(5, 7, value)
        m.meter(S, 1, key_log2=np.log2(value))
        y = float(MR.luminance(S, 1)[0, 0])
        # the exposure is 2^key over the centre of y's sub-bin where value / y would be exact: off by at most 1.0625, the width of
        # the widest sub-bin over its centre
        ratio = float(m.result["exposure"]) * y / value
        assert 1 / 1.0625 <= ratio <= 1.0625, (value, ratio)
        assert m.result["valid"] == 1 and m.result["counted"] == 35 == m.result["kept"]
    m.reset()
    m.meter(_const(5, 7, 0.18), 1, key_log2=np.log2(0.18))
    assert abs(float(m.result["exposure"]) - 1) <= 0.0625


def test_the_trim_drops_outliers_and_keeps_n_minus_lo_minus_hi():
    # 2,000 pixels, half at luminance 0.25 and half at 0.5; in the hot frame ten of the brighter half (0.5 %) sit at 2^15
    plain = np.concatenate([_grey(0.25, 1000), _grey(0.5, 1000)], axis=1)
    hot = plain.copy()
    hot[0, 1990:] = _grey(2.0 ** 15, 10)[0]
    a, b, c = MR.Meter(), MR.Meter(), MR.Meter()
    da = a.meter(hot, 1, low_permille=10, high_permille=10)
    db = b.meter(plain, 1, low_permille=10, high_permille=10)
    dc = c.meter(hot, 1)
    # 20 of 2,000 go at either end: the ten hot pixels and ten at 0.5 in one frame, twenty at 0.5 in the other
    assert a.result["kept"] == b.result["kept"] == 1960 and da["kept"] == db["kept"] and da["kept"][112] == da["kept"][120] == 980 and da["kept"][248] == 0
    assert da["avg"] == db["avg"] and a.result["avgLog2"] == b.result["avgLog2"]
    assert c.result["kept"] == 2000 and dc["kept"][248] == 10 and dc["avg"] > da["avg"] + 0.05  # untrimmed they move the mean
    rng = np.random.default_rng(21)
    S = (0.05 + rng.random((40, 50, 4))).astype(np.float32)
    for lo, hi in itertools.product((0, 1, 10, 333, 400, 999), repeat=2):
        if lo + hi >= 1000:
            continue
        for img in (hot, S, S[:3, :5], S[:1, :1]):
            bins, _, _ = MR.histogram(img, 1)
            N, l, h, kept = MR.trim(bins, lo, hi)
            assert sum(kept) == N - l - h and all(0 <= k <= n for k, n in zip(kept, bins)), (lo, hi)


def test_adaptation_follows_the_rates_and_an_all_black_frame_keeps_the_exposure():
    dark, bright = _const(4, 4, 0.01), _const(4, 4, 4.0)
    m = MR.Meter()
    m.meter(dark, 1)
    first = m.cur
    assert m.result["log2Exposure"] == np.float32(first) == m.result["targetLog2"]  # the first valid call jumps
    m.meter(bright, 1, delta_seconds=0.0, speed_up=5.0, speed_down=5.0)
    assert m.cur == first and m.result["targetLog2"] < m.result["log2Exposure"]  # deltaSeconds = 0 leaves cur unchanged
    d = m.meter(bright, 1, delta_seconds=1e6, speed_up=5.0, speed_down=5.0)
    assert m.cur == d["target"]  # ... and 10^6 seconds reach the target exactly
    for cur, target_img in ((-7.3, dark), (6.1, bright), (0.1, dark), (1e-9, bright)):
        m.cur = cur
        d = m.meter(target_img, 1, delta_seconds=1e6, speed_up=0.5, speed_down=0.5)
        assert m.cur == d["target"], cur
    # falling uses speedDown, rising speedUp
    m.reset()
    m.meter(dark, 1)
    top = m.cur
    d = m.meter(bright, 1, delta_seconds=0.1, speed_up=0.0, speed_down=2.0)
    a = 1.0 - MR.exp2_spec(((-float(np.float32(0.1))) * 2.0) * 1.4426950408889634)
    assert d["target"] < top and m.cur == top + (d["target"] - top) * a
    low = m.cur
    m.meter(bright, 1, delta_seconds=0.1, speed_up=2.0, speed_down=0.0)
    assert m.cur == low  # falling at speedDown = 0: nothing moves
    d = m.meter(dark, 1, delta_seconds=0.1, speed_up=2.0, speed_down=0.0)
    assert d["target"] > low and m.cur == low + (d["target"] - low) * a
    # K = 0
    before = dict(m.result)
    m.meter(_const(4, 4, 0.0), 1, delta_seconds=1.0)
    assert m.result["valid"] == 0 and m.result["kept"] == 0 and m.result["black"] == 16 and m.result["calls"] == before["calls"] + 1
    assert all(m.result[k] == before[k] for k in FLOATS)
    fresh = MR.Meter()
    fresh.meter(_const(4, 4, np.nan), 1)
    assert fresh.result["valid"] == 0 and fresh.result["exposure"] == 1 and fresh.result["log2Exposure"] == 0 and fresh.result["rejected"] == 16
    fresh.meter(dark, 1, delta_seconds=0.0)
    assert fresh.cur == first  # still the first VALID call: it jumps
    # the clamp of step 7
    m.reset()
    m.meter(dark, 1, min_log2_exposure=-1.0, max_log2_exposure=2.0)
    assert m.cur == 2.0
    m.reset()
    m.meter(bright, 1, min_log2_exposure=-1.0, max_log2_exposure=2.0)
    assert m.cur == -1.0 and m.result["exposure"] == np.float32(0.5)


def test_scaling_by_a_power_of_two_moves_the_mean_by_the_exponent():
    rng = np.random.default_rng(5)
    S = np.repeat((2.0 ** rng.uniform(-5, 5, (30, 41, 1))).astype(np.float32), 4, axis=2)  # grey: Y is the value to within an ulp or two
    for lo, hi, mode in ((0, 0, MR.AVERAGE), (10, 10, MR.CENTRE), (400, 400, MR.AVERAGE)):
        base = MR.Meter().meter(S, 1, low_permille=lo, high_permille=hi, mode=mode)
        for k in (-9, -1, 1, 3, 9):
            d = MR.Meter().meter(S * np.float32(2.0 ** k), 1, low_permille=lo, high_permille=hi, mode=mode)
            assert not d["under"].any() and not d["over"].any() and (d["bin"] == base["bin"] + 8 * k).all()  # no pixel leaves the range
            # double rounding in step 6: (A + frac) / K carries 2^-53 of at most 32, far inside 2^-40 of k; no bit equality is claimed
            assert abs((d["avg"] - base["avg"]) - k) <= 2.0 ** -40 * abs(k), (lo, hi, mode, k)


def test_centre_weights_written_out_by_hand():
    assert MR.centre_weight(8).tolist() == [1, 1, 2, 3, 3, 2, 1, 1]
    assert MR.centre_weight(5).tolist() == [1, 2, 3, 2, 1]
    assert MR.centre_weight(3).tolist() == [1, 3, 1]
    assert MR.centre_weight(1).tolist() == [3] and MR.centre_weight(2).tolist() == [2, 2]
    w8 = np.array([1, 1, 2, 3, 3, 2, 1, 1])
    assert (MR.weights(8, 8, MR.CENTRE) == w8[:, None] * w8[None, :]).all() and MR.weights(8, 8, MR.CENTRE)[3:5, 3:5].tolist() == [[9, 9], [9, 9]]
    assert MR.weights(3, 5, MR.CENTRE).tolist() == [[1, 2, 3, 2, 1], [3, 6, 9, 6, 3], [1, 2, 3, 2, 1]]  # 5 wide, 3 high
    assert MR.weights(3, 5, MR.REGION, (1, 3, 0, 2)).tolist() == [[0, 1, 1, 0, 0], [0, 1, 1, 0, 0], [0, 0, 0, 0, 0]]
    bins, counters, _ = MR.histogram(_const(3, 5, 1.0), 1, MR.CENTRE)
    assert bins.sum() == 45 and counters["black"] == 0
    bins, counters, _ = MR.histogram(_const(3, 5, 0.0), 1, MR.REGION, (1, 3, 0, 2))
    assert bins.sum() == 0 and counters["black"] == 4  # a pixel of weight 0 belongs to no class


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


def _synthetic_sum(h, w, seed=17):
    """A sum with everything the steps have a clause for.  Positions wrap, so every extent gets what fits."""
    rng = np.random.default_rng(seed)
    S = (2.0 ** rng.uniform(-20, 20, (h, w, 4))).astype(np.float32)  # below 2^-16 and above 2^16 among them
    S[..., 3] = 2.0
    S[: max(1, h // 3), w // 2:, 0:3] *= -1.0                   # negative values
    S[h // 3: h // 3 + 2, 0:3, 0:3] = np.float32(1e-41)         # denormals
    S[h // 2:, : max(1, w // 4), 0:3] = 0.0                     # black
    f = np.float32
    ladder = []
    for e in (-17, -16, -15, -3, 0, 1, 7, 15, 16, 17):           # exact powers of two, and every sub-bin edge of their octaves, +- 3 ulps
        for j in range(8):
            g = f(2.0 ** e * (1 + j / 8)) / f(0.7152)
            for _ in range(3):
                g = np.nextafter(g, f(0))
            for _ in range(7):
                ladder.append(g)
                g = np.nextafter(g, f(np.inf))
    flat = S.reshape(-1, 4)
    for k, g in enumerate(ladder):  # only green is lit: Y = 0.7152f g, within an ulp or two of the edge on either side
        flat[(7 + 3 * k) % len(flat), 0:3] = (0.0, g, 0.0)

    def put(y, x, rgb):
        S[y % h, x % w, 0:3] = rgb
    put(2, 3, (np.nan, 1.0, 1.0))
    put(4, 5, (1.0, np.inf, 1.0))
    put(6, 2, (np.inf, -np.inf, 0.0))
    put(8, 9, (-np.inf, 0.0, 0.0))
    put(5, 12, 3e38)
    put(9, 1, (-0.0, -0.0, -0.0))
    S.view(np.uint32)[2 % h, 3 % w, 0] = 0x7FC0BEEF
    return S


_sums = {}


def _sum(pkg, extent, kind):
    """The device's own read-back sum of `kind` at `extent` (render1, render8, constant, synthetic)"""
    key = (extent, kind)
    if key not in _sums:
        s, r = _gpu(pkg)
        w, h = EXTENTS[extent]
        r.set_tile_shard(0, 1, 32)
        r.resize(w, h)
        u = s.uniform(w, h, bounces=4)
        if kind == "synthetic":
            r.write_accumulation(_synthetic_sum(h, w))
        elif kind == "constant":
            r.write_accumulation(_const(h, w, (0.3, 0.7, 0.1)))
        else:
            for f in range(int(kind[6:])):
                u.TotalSamples = f
                r.render(u, s.lights)
        _sums[key] = r.readback()
    return _sums[key]


def _plain(pkg, w, h, S=None):
    """a handle with no scene: ptx_meter needs none"""
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


def _configs(w, h):
    """three modes (a region that touches the image's edges, and where the extent has an inside one that misses them) x trims
    {0 / 0, 10 / 10, 400 / 400} x totalSamples {1, 8, 3}; the time step, the rates and the limits change along the way, so that the
    sequence also walks the adaptation"""
    modes = [(MR.AVERAGE, (0, 0, 0, 0)), (MR.CENTRE, (0, 0, 0, 0)), (MR.REGION, (0, max(1, w // 2), 0, h))]
    if w >= 3 and h >= 3:
        modes.append((MR.REGION, (1, w - 1, 1, h - 1)))
    for k, ((mode, region), (lo, hi), ts) in enumerate(itertools.product(modes, ((0, 0), (10, 10), (400, 400)), (1, 8, 3))):
        yield dict(total_samples=ts, mode=mode, region=region, low_permille=lo, high_permille=hi, delta_seconds=(0.0, 0.016, 0.5, 2.0, 40.0)[k % 5],
                   key_log2=(KEY, 0.0, -1.5)[k % 3], compensation=(0.0, 0.5)[k % 2], speed_up=(1.0, 3.0, 0.25)[k % 3], speed_down=(3.0, 0.5)[k % 2],
                   min_log2_exposure=-8.0 if k % 7 else -0.5, max_log2_exposure=8.0 if k % 4 else 1.0)


def _assert_same(r, ref, what):
    """the device's result and bins against the reference's, bit for bit"""
    res, bins = r.read_meter(bins=True)
    got = {k: getattr(res, k) for k in INTS}
    want = {k: int(ref.result[k]) for k in INTS}
    assert got == want, (what, got, want)
    assert (bins.astype(np.int64) == ref.bins).all(), (what, np.flatnonzero(bins != ref.bins)[:8])
    for k in FLOATS:
        g, v = np.float32(getattr(res, k)), np.float32(ref.result[k])
        assert g.view(np.uint32) == v.view(np.uint32), (what, k, float(g), float(v))
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["render1", "render8", "constant", "synthetic"])
@pytest.mark.parametrize("extent", list(EXTENTS))
def test_meter_equals_the_reference_bit_for_bit(pkg, extent, kind):
    S = _sum(pkg, extent, kind)
    w, h = EXTENTS[extent]
    r = _plain(pkg, w, h, S)
    ref = MR.Meter()
    valid = 0
    for p in _configs(w, h):
        r.meter(**p)
        ref.meter(S, **p)
        res = _assert_same(r, ref, (extent, kind, p))
        valid += res.valid
    print(f"{extent} {kind}: {ref.result['calls']} calls, {valid} valid; last: counted {ref.result['counted']} black {ref.result['black']} rejected "
          f"{ref.result['rejected']} under {ref.result['under']} over {ref.result['over']} exposure {float(ref.result['exposure']):.6g}")
    if kind == "constant" or w * h >= 15:
        assert valid > 0
    if kind == "synthetic" and w * h >= 3000:
        assert all(ref.result[k] > 0 for k in ("black", "rejected", "under", "over"))
    assert (_bits(r.readback()) == _bits(S)).all()  # the image is only read
    r.close()


@pytest.mark.gpu
def test_a_sequence_of_changing_sums_pins_the_adaptation_and_reset_and_resize_restart_it(pkg):
    frames = [_sum(pkg, "67x45", k) for k in ("render1", "constant", "render8", "synthetic")]
    samples = (1, 1, 8, 2)
    r = _plain(pkg, W, H)
    ref = MR.Meter()
    p = dict(key_log2=KEY, speed_up=1.5, speed_down=4.0, low_permille=20, high_permille=20, mode=MR.CENTRE)
    seen = []
    for S, ts, dt in zip(frames, samples, (0.3, 0.05, 0.2, 0.1)):
        r.write_accumulation(S)
        r.meter(ts, delta_seconds=dt, **p)
        ref.meter(S, ts, delta_seconds=dt, **p)
        res = _assert_same(r, ref, ts)
        seen.append((res.log2Exposure, res.targetLog2))
    assert len(set(e for e, _ in seen)) == 4 and ref.result["calls"] == 4  # it moved every time ...
    assert seen[0][0] == seen[0][1] and all(e != t for e, t in seen[1:])    # ... the first call by jumping, the others part of the way
    jumped = MR.Meter()
    jumped.meter(frames[3], 2, **p)
    assert ref.result["log2Exposure"] != jumped.result["log2Exposure"]
    # ptx_meter_reset: the state of a fresh handle, and the next call jumps
    r.meter_reset()
    ref.reset()
    _assert_same(r, ref, "reset")
    r.meter(2, delta_seconds=0.1, **p)
    _assert_same(r, jumped, "after the reset")
    # ptx_resize does the same
    r.resize(W, H)
    _assert_same(r, ref, "resize")
    r.write_accumulation(frames[3])
    r.meter(2, delta_seconds=0.1, **p)
    _assert_same(r, jumped, "after the resize")
    # an all-black frame leaves the exposure alone, and so does a rejected one
    for value in (0.0, np.nan):
        r.write_accumulation(_const(H, W, value))
        r.meter(2, delta_seconds=1.0, **p)
        jumped.meter(_const(H, W, value), 2, delta_seconds=1.0, **p)
        assert _assert_same(r, jumped, value).valid == 0
    r.close()


@pytest.mark.gpu
def test_the_three_sources_are_the_images_the_output_calls_read(pkg):
    s, _ = _gpu(pkg)
    S = _sum(pkg, "67x45", "render8")
    u = s.uniform(W, H, bounces=4)
    r = _borrower(pkg, W, H, S, u)
    p = dict(key_log2=KEY, low_permille=10, high_permille=10, mode=MR.CENTRE)
    r.despike()
    r.denoise(8, 2, 1.5, 0.3, 0.03)
    Cc, D = r.read_despiked(), r.read_denoised()
    assert (_bits(Cc) != _bits(S)).any()
    for source, image, ts, fresh_ts in ((pkg.METER_SUM, S, 8, 8), (pkg.METER_DESPIKED, Cc, 8, 8), (pkg.METER_DENOISED, D, 8, 1)):
        r.meter_reset()
        r.meter(ts, source=source, **p)
        f = _plain(pkg, W, H, image)  # a fresh handle whose sum is that image; the denoised one holds the mean
        f.meter(fresh_ts, **p)
        ref = MR.Meter()
        ref.meter(image, ts, denoised=source == pkg.METER_DENOISED, **p)
        got = _assert_same(r, ref, source)
        _assert_same(f, ref, source)
        assert got.valid == 1
        f.close()
    r.close()


@pytest.mark.gpu
def test_postprocess_metered_multiplies_the_exposure_in_on_the_device(pkg):
    s, _ = _gpu(pkg)
    S = _sum(pkg, "67x45", "synthetic")
    u = s.uniform(W, H, bounces=4)
    r = _borrower(pkg, W, H, S, u)
    r.despike(radius=1, rank=2, gain=1.5, min_taps=3)
    r.denoise(2, 2, 1.5, 0.3, 0.03)
    images = {pkg.METER_SUM: S, pkg.METER_DESPIKED: r.read_despiked(), pkg.METER_DENOISED: r.read_denoised()}
    screens = ((W, H, pkg.PRESENT_R8G8B8A8_SRGB, 0), (100, 37, pkg.PRESENT_R16G16B16A16_SFLOAT, 0), (134, 90, pkg.PRESENT_A2B10G10R10_UNORM, 1))
    for source, image in images.items():
        r.meter(2, source=source, key_log2=1.0, low_permille=50, high_permille=50)
        e = r.read_meter().exposure
        assert e != 1.0 and np.isfinite(e) and e > 0
        f = _plain(pkg, W, H, image)
        host = dict(POST, exposure=float(np.float32(POST["exposure"]) * np.float32(e)))  # the float product, on the host
        for tone in (pkg.TONE_MAPPING_SDR, pkg.TONE_MAPPING_HDR):
            r.postprocess_metered(2, tone_mapping=tone, source=source, **POST)
            f.postprocess(1 if source == pkg.METER_DENOISED else 2, tone_mapping=tone, **host)
            for fmt in (pkg.OUTPUT_RGBA8_SRGB, pkg.OUTPUT_RGBA32F):
                a, b = r.read_output(fmt), f.read_output(fmt)
                assert a.dtype == b.dtype and (a.view(np.uint8) == b.view(np.uint8)).all(), (source, tone, fmt)
            for sw, sh, fmt, mode in screens:
                r.present(sw, sh, fmt, mode)
                f.present(sw, sh, fmt, mode)
                assert (r.read_present().view(np.uint8) == f.read_present().view(np.uint8)).all(), (source, tone, sw, sh, fmt)
        # the exposure does something, and with a reset state the call is the plain one
        r.postprocess_metered(2, source=source, **POST)
        metered = r.read_output(pkg.OUTPUT_RGBA32F)
        r.meter_reset()
        r.postprocess_metered(2, source=source, **POST)
        unit = r.read_output(pkg.OUTPUT_RGBA32F)
        (r.postprocess, r.postprocess_despiked, r.postprocess_denoised)[source](2, **POST)
        assert (_bits(unit) == _bits(r.read_output(pkg.OUTPUT_RGBA32F))).all(), source
        assert (_bits(unit) != _bits(metered)).any(), source
        f.close()
    r.close()


@pytest.mark.gpu
def test_nothing_else_is_touched_and_two_meters_in_a_row_match_a_fresh_handle(pkg):
    s, main = _gpu(pkg)
    S = _sum(pkg, "67x45", "render1")
    u = s.uniform(W, H, bounces=4)
    view, proj = s.camera_matrices(W, H)
    r = _borrower(pkg, W, H, S, u)
    r.despike()
    r.temporal_accumulate(1, view, proj, max_history=8.0, normal_threshold=0.3, position_threshold=0.03)
    r.denoise(1, 2, 1.5, 0.3, 0.03)
    before = [r.readback(), r.read_despiked(), r.read_temporal(), r.read_denoised()] + [r.read_guide(k) for k in range(3)]
    calls = (dict(mode=MR.CENTRE, key_log2=KEY), dict(mode=MR.REGION, region=(3, 40, 2, 30), low_permille=100, high_permille=50, delta_seconds=0.25))
    for source in (pkg.METER_SUM, pkg.METER_DESPIKED, pkg.METER_DENOISED):
        r.meter_reset()
        f = _plain(pkg, W, H, before[(0, 1, 3)[source]])
        for p in calls:
            r.meter(1, source=source, **p)
            f.meter(1, **p)
        a, ab = r.read_meter(bins=True)
        b, bb = f.read_meter(bins=True)
        assert bytes(a) == bytes(b) and (ab == bb).all() and a.calls == 2, source
        f.close()
    assert r.meter_ptr()
    after = [r.readback(), r.read_despiked(), r.read_temporal(), r.read_denoised()] + [r.read_guide(k) for k in range(3)]
    for k, (x, y) in enumerate(zip(before, after)):
        assert (_bits(x) == _bits(y)).all(), k
    r.close()
    # the next ptx_render continues the sum as if nothing had happened
    main.set_tile_shard(0, 1, 32)
    main.resize(W, H)
    up = s.uniform(W, H, bounces=4)

    def path_traced(n, between=None):
        main.reset()
        for k in range(n):
            if between and k == n - 1:
                between()
            up.TotalSamples = k
            main.render(up, s.lights)
        return main.readback()
    two = path_traced(2)
    again = path_traced(2, between=lambda: main.meter(1))
    assert (_bits(two) == _bits(again)).all()
    one = path_traced(1)
    ref = MR.Meter()
    ref.meter(one, 1, **{k: v for k, v in pkg.METER_DEFAULTS.items()})
    main.meter_reset()
    main.meter(1)  # the package's defaults are the call's
    _assert_same(main, ref, "defaults")
    main.meter_reset()


@pytest.mark.gpu
def test_a_borrower_and_a_bound_image(pkg):
    import torch

    s, _ = _gpu(pkg)
    w, h = EXTENTS["33x9"]
    b = _borrower(pkg, w, h)
    u = s.uniform(w, h, bounces=4)
    b.render(u, s.lights)
    S = b.readback()
    p = dict(key_log2=KEY, mode=MR.CENTRE, low_permille=10, high_permille=10, speed_up=2.0, speed_down=0.75)
    ref = MR.Meter()
    b.meter(1, **p)
    ref.meter(S, 1, **p)
    _assert_same(b, ref, "borrower")
    # a bound image is the sum
    bound = torch.from_numpy(_synthetic_sum(h, w, seed=5)).cuda()
    b.bind_accumulation(bound.data_ptr(), bound.numel() * 4)
    b.meter(3, delta_seconds=0.2, **p)
    ref.meter(bound.cpu().numpy(), 3, delta_seconds=0.2, **p)
    _assert_same(b, ref, "bound")
    b.postprocess_metered(3, **POST)
    f = _plain(pkg, w, h, bound.cpu().numpy())
    f.postprocess(3, **dict(POST, exposure=float(np.float32(POST["exposure"]) * ref.result["exposure"])))
    assert (_bits(b.read_output(pkg.OUTPUT_RGBA32F)) == _bits(f.read_output(pkg.OUTPUT_RGBA32F))).all()
    assert b.meter_ptr()
    b.bind_accumulation(0, 0)
    f.close()
    b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("leg", ["sum", "despiked", "denoised"])
def test_renderer_hip_with_exposure_settings_on_is_the_same_calls_made_by_hand(pkg, tmp_path_factory, tmp_path, leg):
    """test_motion's driver (examples/motion_frame.cpp, compiled once per session) with ExposureSettings on: two frames of
    animated_test through RendererHip, each announced with OnUpdate(0.37).  The adapter meters the image it is about to post-process:
    the sum; with FireflySettings on the despiked image; with the denoiser, the temporal settings and motion vectors on the denoised
    one.  The sum, T (where there is one) and the output image of both frames equal ptx_meter at the adapter's defaults followed by
    ptx_postprocess_metered made by hand, bit for bit -- the second frame adapts from the first -- and the output differs from the
    plain call's.  Without the denoiser the driver saves every frame twice: the second SaveOutput finds the time step used up, meters
    with deltaSeconds = 0 and gives the first one's image."""
    import subprocess

    import test_motion as TM

    w, h, spp, depth, step = W, H, 2, 4, 0.37
    despike, denoiser = int(leg == "despiked"), int(leg == "denoised")
    exe = TM._motion_frame_driver(pkg, tmp_path_factory)
    dump = tmp_path / "frames.bin"
    subprocess.check_call([exe, "animated_test", str(w), str(h), str(spp), str(depth), str(step), "0", str(dump), "0", str(despike), str(denoiser), "1"])
    got = np.fromfile(dump, np.float32).reshape(2, 3, h, w, 4)
    s = pkg.Scene("animated_test", DETAIL)
    s.update(0.0)
    r = pkg.Renderer()
    r.upload(s)
    if denoiser:
        r.track_motion(True)
    r.resize(w, h)
    source = {"sum": pkg.METER_SUM, "despiked": pkg.METER_DESPIKED, "denoised": pkg.METER_DENOISED}[leg]
    exposures = []
    for frame in range(2):
        if frame:
            assert s.update(step)
        it, bn = s.animation_state()
        r.update_animation(it, bn if len(bn) else None)
        r.reset()
        for f in range(spp):
            r.render(s.uniform(w, h, bounces=depth, sample_count=1, total_samples=f), s.lights)
        if despike:
            r.despike()
        if denoiser:
            r.render_guides_motion(s.uniform(w, h, bounces=depth, sample_count=1, total_samples=spp))
            view, proj = s.camera_matrices(w, h)
            r.temporal_accumulate_motion(spp, view, proj, max_history=32.0, normal_threshold=0.3, position_threshold=0.03)
            r.denoise_temporal(iterations=3, sigma_color=1.5, sigma_normal=0.3, sigma_position=0.03)
        r.meter(spp, delta_seconds=step, source=source)  # METER_DEFAULTS are the adapter's (the header test holds them together)
        r.postprocess_metered(spp, 1.0, 1.0, 1.0, pkg.TONE_MAPPING_SDR, source=source)
        first = r.read_meter()
        if not denoiser:  # the driver's second SaveOutput of the frame
            r.meter(spp, delta_seconds=0.0, source=source)
            r.postprocess_metered(spp, 1.0, 1.0, 1.0, pkg.TONE_MAPPING_SDR, source=source)
        S, out = r.readback(), r.read_output(pkg.OUTPUT_RGBA32F)
        assert (_bits(got[frame][0]) == _bits(S)).all() and (_bits(got[frame][2]) == _bits(out)).all(), frame
        if denoiser:
            assert (_bits(got[frame][1]) == _bits(r.read_temporal())).all(), frame
        res = r.read_meter()
        assert res.valid == 1 and res.calls == (frame + 1) * (1 if denoiser else 2)
        assert res.exposure == first.exposure and res.log2Exposure == first.log2Exposure  # deltaSeconds = 0 moved nothing
        exposures.append(res.exposure)
        (r.postprocess_denoised if denoiser else r.postprocess_despiked if despike else r.postprocess)(spp, 1.0, 1.0, 1.0, pkg.TONE_MAPPING_SDR)
        assert (_bits(r.read_output(pkg.OUTPUT_RGBA32F)) != _bits(out)).any()
    print(f"{leg}: metered exposures of the two frames {exposures}")
    assert exposures[0] != exposures[1]
    r.close()


@pytest.mark.gpu
def test_renderer_hip_with_exposure_settings_off_is_the_plain_path(pkg, tmp_path_factory, tmp_path):
    """The same driver with the exposure argument given as 0: ptx_postprocess on the sum, as before ExposureSettings existed."""
    import subprocess

    import test_motion as TM

    w, h, spp, depth, step = W, H, 2, 4, 0.37
    exe = TM._motion_frame_driver(pkg, tmp_path_factory)
    dump = tmp_path / "frames.bin"
    subprocess.check_call([exe, "animated_test", str(w), str(h), str(spp), str(depth), str(step), "0", str(dump), "0", "0", "0", "0"])
    got = np.fromfile(dump, np.float32).reshape(2, 3, h, w, 4)
    s = pkg.Scene("animated_test", DETAIL)
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
        assert (_bits(got[frame][0]) == _bits(r.readback())).all() and (_bits(got[frame][2]) == _bits(r.read_output(pkg.OUTPUT_RGBA32F))).all(), frame
    assert not r.meter_ptr()  # and nothing was allocated for a meter nobody called
    r.close()


@pytest.mark.gpu
def test_refusals_leave_the_state_and_the_bins_intact(pkg):
    import torch

    s, _ = _gpu(pkg)
    S = _sum(pkg, "67x45", "render8")
    r = pkg.Renderer()  # an owner of its own: tile shards and bound buffers are refused on it
    r.upload(s)
    r.resize(W, H)
    lib = r.lib
    post = pkg.PostProcessingUniformData(8, 1.0, 1.0, 1.0)
    out = pkg.MeterResult()
    # the accessors before any ptx_meter
    assert lib.ptx_read_meter(r.handle, C.byref(out), None) == NOT_READY and not lib.ptx_device_meter_ptr(r.handle)
    assert lib.ptx_postprocess_metered(r.handle, C.byref(post), 0, 0) == NOT_READY
    assert lib.ptx_meter_reset(r.handle) == OK and not lib.ptx_device_meter_ptr(r.handle)
    r.write_accumulation(S)
    r.meter(8, key_log2=KEY, mode=MR.CENTRE)
    r.meter(8, key_log2=KEY, mode=MR.CENTRE, delta_seconds=0.1, compensation=1.0)
    kept, kept_bins = r.read_meter(bins=True)
    assert kept.valid == 1 and kept.calls == 2

    def intact():
        now, bins = r.read_meter(bins=True)
        assert bytes(now) == bytes(kept) and (bins == kept_bins).all()

    def call(handle=r.handle, **over):
        p = dict(source=0, mode=0, totalSamples=8, region=(0, 0, 0, 0), lowPermille=0, highPermille=0, keyLog2=0.0, compensation=0.0, minLog2Exposure=-8.0,
                 maxLog2Exposure=8.0, speedUp=1.0, speedDown=1.0, deltaSeconds=0.1, flags=0, reserved=0)
        p.update(over)
        p["region"] = (C.c_uint32 * 4)(*p["region"])
        d = pkg.MeterDesc(**p)
        return lib.ptx_meter(handle, C.byref(d))

    nan, inf = float("nan"), float("inf")
    bad = [dict(source=3), dict(mode=3), dict(totalSamples=0), dict(lowPermille=1000), dict(lowPermille=500, highPermille=500), dict(highPermille=4000000000, lowPermille=4000000000),
           dict(minLog2Exposure=1.0, maxLog2Exposure=0.5), dict(speedUp=-1.0), dict(speedDown=-0.5), dict(deltaSeconds=-1e-3), dict(flags=1), dict(reserved=1)]
    bad += [{f: v} for f in ("keyLog2", "compensation", "minLog2Exposure", "maxLog2Exposure", "speedUp", "speedDown", "deltaSeconds") for v in (nan, inf, -inf)]
    bad += [dict(mode=2, region=g) for g in ((0, 0, 0, 0), (5, 5, 0, H), (6, 5, 0, H), (0, W, 7, 7), (0, W + 1, 0, H), (0, W, 0, H + 1), (W, W + 1, 0, 1))]
    for b in bad:  # state and bins are read back after every single refusal, before anything is accepted again
        assert call(**b) == INVALID, b
        intact()
    for refused in (lambda: lib.ptx_meter(r.handle, None), lambda: call(handle=None), lambda: lib.ptx_read_meter(r.handle, None, None),
                    lambda: lib.ptx_read_meter(None, C.byref(out), None), lambda: lib.ptx_meter_reset(None),
                    lambda: lib.ptx_postprocess_metered(r.handle, None, 0, 0), lambda: lib.ptx_postprocess_metered(None, C.byref(post), 0, 0),
                    lambda: lib.ptx_postprocess_metered(r.handle, C.byref(post), 2, 0), lambda: lib.ptx_postprocess_metered(r.handle, C.byref(post), 0, 3)):
        assert refused() == INVALID
        intact()
    assert not lib.ptx_device_meter_ptr(None)
    # a source that does not exist: no C, no D
    for refused in (lambda: call(source=1), lambda: call(source=2), lambda: lib.ptx_postprocess_metered(r.handle, C.byref(post), 0, 1),
                    lambda: lib.ptx_postprocess_metered(r.handle, C.byref(post), 0, 2)):
        assert refused() == NOT_READY
        intact()
    # a tile shard of a larger world, a bound shard buffer
    r.set_tile_shard(0, 2, 8)
    assert call() == NOT_READY
    intact()
    shard = torch.zeros(r.shard_bytes(0) // 4, dtype=torch.float32, device="cuda")
    r.bind_shard_accumulation(shard.data_ptr(), r.shard_bytes(0))
    assert call() == NOT_READY
    intact()
    assert lib.ptx_postprocess_metered(r.handle, C.byref(post), 0, 0) == NOT_READY
    intact()
    r.bind_shard_accumulation(0)
    r.set_tile_shard(0, 1, 32)
    intact()
    # the whole image and its last pixel are regions: accepted, so the state moves on
    assert call(mode=2, region=(0, W, 0, H)) == OK and call(mode=2, region=(W - 1, W, H - 1, H)) == OK
    assert r.read_meter().calls == 4
    # no image
    fresh = pkg.Renderer()
    assert call(handle=fresh.handle) == NOT_READY and call(handle=fresh.handle, mode=2, region=(0, 1, 0, 1)) == NOT_READY
    assert lib.ptx_read_meter(fresh.handle, C.byref(out), None) == NOT_READY
    fresh.close()
    # C and D of an older extent do not count
    r.despike()
    assert call(source=1) == OK
    r.resize(W, H)
    assert call(source=1) == NOT_READY and call(source=2) == NOT_READY
    now = r.read_meter()
    assert now.exposure == 1.0 and now.calls == 0  # ptx_resize reset the state; the refusals behind it left it so
    r.close()


@pytest.mark.gpu
def test_the_overflow_bound_of_step_4_is_refused(pkg):
    """9 W H reaches 2^32 at 477,218,589 pixels: 32768 x 14564 is refused in PTX_METER_CENTRE and taken in PTX_METER_AVERAGE, where
    the device's bins of a constant image hold every pixel (the only test of an index past 2^28; 7.6 GB, a few tens of milliseconds)."""
    import torch  # noqa: F401

    w, h = 32768, 14564
    assert 9 * w * h >= 2 ** 32 > 9 * w * (h - 1)
    r = pkg.Renderer()
    r.resize(w, h)
    d = pkg.MeterDesc(0, 1, 1, (C.c_uint32 * 4)(0, 0, 0, 0), 0, 0, 0.0, 0.0, -8.0, 8.0, 1.0, 1.0, 0.0, 0, 0)
    assert r.lib.ptx_meter(r.handle, C.byref(d)) == INVALID and not r.meter_ptr()
    r.meter(1, mode=MR.AVERAGE)
    res, bins = r.read_meter(bins=True)
    assert res.black == w * h and res.counted == 0 and res.valid == 0 and not bins.any()  # ptx_resize zeroed the sum
    assert r.lib.ptx_meter(r.handle, C.byref(d)) == INVALID  # ... and with a state to lose: intact
    again, bins_again = r.read_meter(bins=True)
    assert bytes(again) == bytes(res) and (bins_again == bins).all()
    r.resize(w, h - 1)
    assert r.lib.ptx_meter(r.handle, C.byref(d)) == OK
    res = r.read_meter()
    assert res.black == int(MR.centre_weight(h - 1).sum()) * int(MR.centre_weight(w).sum()) and res.calls == 1
    r.close()
