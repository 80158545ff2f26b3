"""Variance-guided denoising (include/ptx.h ptx_temporal_accumulate_moments / ptx_denoise_variance, csrc/pt_variance.hpp,
docs/NEXT_ROWS.md section 16) against tests/variance_ref.py.

Tolerance.  As in test_temporal: the reference runs on the device's own read-back sums and guides in float32 and in float64, and a
quantity's bound is measured ON THE REFERENCE ALONE inside the test: 8 x max |ref(float32) - ref(float64)| of that quantity in that
very case, with a floor of 2^-20 max(1, |value|).  A pixel on which the two runs of the reference decide differently (a tap, found or
not, known or not, the L_M >= 4 branch, the vt = 0 rule), or which took such a pixel in through a tap, is left out; the share left out
is capped at 4 x the share the reference alone leaves out on the CPU's own sequences (REFERENCE_LEFT_OUT) and at 2 % of the valid
pixels.  Pixels that are not valid must hold the mean bit for bit."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import denoise_ref as R
import temporal_ref as TR
import test_temporal as TT
import util
import variance_ref as VR

W, H = TT.W, TT.H
TD = dict(max_history=6.0, normal_threshold=0.3, position_threshold=0.03)  # five frames: both branches of the estimate run
SN, SP = 0.3, 0.03
SIGMAS = (0.5, 2.0)
FRAMES = 5
LEFT_OUT_CAP = 0.02
POST = TT.POST
# Measured on the CPU (test_reference_gap_and_left_out_share_on_the_cpu_sequences recomputes them): over CPU_SEQUENCES at 67 x 45 on
# first-hit guides computed without a GPU and the synthetic sum, the largest |ref32 - ref64| per quantity and the largest share of
# valid pixels the comparable_* masks leave out of any quantity.
# The hot pixel of the synthetic sum (3000 over the albedo floor: luminances up to 3e5, squares up to 1e11) sets the first three.
REFERENCE_GAP = {"mu1": 1.6e-3, "mu2": 9.0, "V0": 0.8, "D": 9.0e-4}  # measured 1.28e-3, 7.44, 0.596, 6.78e-4
REFERENCE_LEFT_OUT = 0.005  # measured 0.0041 (8 of 1938 pixels, after the jump, in the chain); the filter's stage leaves nothing out


_bits = TT._bits


# =====================================================================================================
# without a GPU
# =====================================================================================================
def test_header_declares_and_package_exports_the_variance_stage(pkg):
    header = open(os.path.join(pkg.REPO_DIR, "include", "ptx.h")).read()
    decls = {
        "ptx_temporal_accumulate_moments": r"PTX_API int ptx_temporal_accumulate_moments\(PtxRenderer \*r, const PtxTemporalDesc \*desc\);",
        "ptx_read_moments": r"PTX_API int ptx_read_moments\(PtxRenderer \*r, void \*host, size_t bytes\);",
        "ptx_denoise_variance": r"PTX_API int ptx_denoise_variance\(PtxRenderer \*r, const PtxDenoiseDesc \*desc\);",
        "ptx_read_variance": r"PTX_API int ptx_read_variance\(PtxRenderer \*r, void \*host, size_t bytes\);",
    }
    lib = pkg.load_hip()
    for name, decl in decls.items():
        assert re.search(decl, header), name
        assert name in pkg.PTX_SYMBOLS
        assert hasattr(lib, name), name
    assert "#define PTX_ABI_VERSION 5u" in header and "PTX_FN_COUNT = 38" in header  # additions only
    assert C.sizeof(pkg.DenoiseDesc) == 28 and C.sizeof(pkg.TemporalDesc) == 152  # no struct changed
    # the semantics are in the header as text: the reference is written from it
    for phrase in ("l = (0.2126 c.x + 0.7152 c.y) + 0.0722 c.z", "M = M_h + (mu - M_h) / L_M", "UNKNOWN (L_M = 0)", "DROPS the moment history",
                   "where L_M(p) >= 4, v = mu2 - mu1 mu1", "7 x 7 window", "sum w = 0 gives v = 0", "V_0 = v where v is finite and > 0, else 0",
                   "1/4 (centre), 1/8 (edges), 1/16 (corners)", "the tap does NOT count if d > 0 and vt(p) = 0", "e_l = d^2 / (sigmaLuminance^2 vt(p))",
                   "V_{i+1}(p) = sum w^2 V_i(q) / (sum w)^2", "NOT halved", "no epsilon and no square root"):
        assert phrase in header, phrase
    for method in ("temporal_accumulate_moments", "read_moments", "denoise_variance", "read_variance"):
        assert callable(getattr(pkg.Renderer, method))
    d = pkg.VARIANCE_DENOISE_DEFAULTS
    assert set(d) == {"iterations", "sigma_luminance", "sigma_normal", "sigma_position"}
    assert 1 <= d["iterations"] <= 6 and d["sigma_luminance"] > 0 and d["sigma_normal"] > 0 and d["sigma_position"] > 0
    host = open(os.path.join(pkg.PKG_DIR, "host", "RendererHip.h")).read()
    assert re.search(r"struct VarianceSettings\s*\{\s*bool Enabled = false;", host) and "SetSettings(const VarianceSettings &" in host


PF = TT._plane_frame


def _lum64(c):
    return (np.float64(np.float32(0.2126)) * c[..., 0] + np.float64(np.float32(0.7152)) * c[..., 1]) + np.float64(np.float32(0.0722)) * c[..., 2]


def _acc(S, frame, hist, mom, flags=0, dtype=np.float64, samples=2, **over):
    g, view, proj = frame
    p = dict(max_history=32.0, normal_threshold=0.3, position_threshold=0.03)
    p.update(over)
    return VR.accumulate(S, *g, samples, view, proj, hist, mom, p["max_history"], p["normal_threshold"], p["position_threshold"], flags, dtype)


def _box(a, r=VR.WINDOW):
    """The mean of `a` over the (2r + 1)^2 window clipped to the image, by loops"""
    h, w = a.shape
    out = np.zeros_like(a)
    for y in range(h):
        for x in range(w):
            out[y, x] = a[max(0, y - r):y + r + 1, max(0, x - r):x + r + 1].mean()
    return out


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_a_constant_image_has_its_moments_no_variance_and_stays_constant(dtype):
    h, w = 9, 12
    frame = PF(h, w, albedo=(0.8, 0.5, 0.25))
    S = np.zeros((h, w, 4), np.float32)
    S[..., 0:3], S[..., 3] = (1.0, 0.5, 0.25), 2
    c = np.float64([0.5, 0.25, 0.125]) / np.float64(np.float32([0.8, 0.5, 0.25]))
    l = _lum64(c)
    hist = mom = None
    eps = np.finfo(dtype).eps
    for k in range(5):
        T, hist, mom, d = _acc(S, frame, hist, mom, dtype=dtype)
        assert mom.m1.dtype == np.dtype(dtype) and (mom.L == k + 1).all() and d["known"].all()
        assert np.abs(mom.m1 - l).max() <= 8 * eps and np.abs(mom.m2 - l * l).max() <= 8 * eps
        for sl in SIGMAS:
            D, V0 = VR.denoise_variance(T, *frame[0], mom, 3, sl, SN, SP, dtype)
            if dtype == np.float64 or k < 3:  # float32: mu2 - mu1^2 is rounding noise of either sign; what is positive is tiny
                assert (V0 <= 64 * eps).all()
            assert np.abs(D[..., 0:3] - T[..., 0:3]).max() <= 16 * eps and (D[..., 3] == 1).all()


def test_still_camera_moments_are_the_means_and_the_variance_is_numpy_s():
    h, w = 8, 11
    frame = PF(h, w)
    sums = [TT._noise_sum(h, w, k) for k in range(6)]
    ls = [_lum64(s[..., 0:3].astype(np.float64) / 2) for s in sums]
    hist = mom = None
    for k in range(6):
        T, hist, mom, _ = _acc(sums[k], frame, hist, mom, max_history=6.0)
        m1, m2 = np.mean(ls[:k + 1], axis=0), np.mean(np.square(ls[:k + 1]), axis=0)
        assert (mom.L == k + 1).all() and np.abs(mom.m1 - m1).max() <= 1e-14 and np.abs(mom.m2 - m2).max() <= 1e-14
        V0, d = VR.estimate(T, *frame[0], mom, SN, SP)
        if k + 1 >= 4:
            assert d["long"].all() and not d["wtaps"].any()
            assert np.abs(V0 - np.var(ls[:k + 1], axis=0)).max() <= 1e-14
        else:  # flat guides: every weight is 1, the window is a box clipped to the image
            assert not d["long"].any() and d["wtaps"][3, 5].all() and d["wtaps"][0, 0].sum() == 16
            want = _box(mom.m2) - _box(mom.m1) ** 2
            assert (want > 0).all() and np.abs(V0 - want).max() <= 1e-14


def _flat_case(h, w, lum_image, variance, L=5.0):
    """T of grey pixels with the luminances `lum_image` on flat white guides, and moments that say `variance` everywhere"""
    g = R.plane_guides(h, w)
    T = np.zeros((h, w, 4), np.float64)
    T[..., 0:3] = (lum_image / sum(np.float64(np.float32(v)) for v in VR.LUM))[..., None]
    T[..., 3] = L
    mom = VR.Moments(lum_image.copy(), lum_image ** 2 + variance, np.full((h, w), L))
    return T.astype(np.float32), g, mom


def test_flat_guides_and_a_huge_sigma_shrink_the_variance_by_the_kernel_s_square_sum():
    h, w = 13, 15
    rng = np.random.default_rng(3)
    T, g, mom = _flat_case(h, w, rng.uniform(0.2, 0.8, (h, w)), 0.0)
    V0 = np.full((h, w), 0.37)
    Ds, Vs, dec = VR.filter_all(T, *g, V0, 2, 1e9, SN, SP)
    assert abs(sum(v * v for v in R.H5) - 35.0 / 128.0) == 0
    assert np.abs(Vs[0][2:-2, 2:-2] / 0.37 - (35.0 / 128.0) ** 2).max() <= 1e-12 and dec[0]["ftaps"][2:-2, 2:-2].all()
    assert (Vs[0] >= Vs[0][6, 7] - 1e-15).all()  # the edges lose taps: less averaging, never more
    # ... and the colour is the plain B3 blur there
    c = T[..., 0].astype(np.float64)
    want = sum(R.H5[dy + 2] * R.H5[dx + 2] * c[2 + dy:h - 2 + dy, 2 + dx:w - 2 + dx] for dy in range(-2, 3) for dx in range(-2, 3))
    assert np.abs(Ds[0][2:-2, 2:-2, 0] - want).max() <= 1e-9


def test_a_step_of_ten_standard_deviations_blocks_the_blur_and_a_tenth_of_one_does_not():
    h, w = 9, 16
    sd = 0.05
    for step, blocked in ((10.0 * sd, True), (0.1 * sd, False)):
        l = np.full((h, w), 0.4)
        l[:, w // 2:] += step
        T, g, mom = _flat_case(h, w, l, sd * sd)
        V0, d = VR.estimate(T, *g, mom, SN, SP)
        assert d["long"].all() and np.abs(V0 - sd * sd).max() <= 1e-12
        D = VR.filter_all(T, *g, V0, 1, 1.0, SN, SP)[0][0]
        moved = np.abs(D[..., 0].astype(np.float64) - T[..., 0].astype(np.float64))[:, w // 2 - 1:w // 2 + 1].max() / (step / sum(VR.LUM))
        assert (moved < 1e-30) if blocked else (moved > 0.2), (step, moved)


def test_zero_variance_keeps_a_pixel_that_differs_to_itself():
    h, w = 8, 10
    rng = np.random.default_rng(5)
    T, g, mom = _flat_case(h, w, rng.uniform(0.2, 0.8, (h, w)), 0.0)
    V0, _ = VR.estimate(T, *g, mom, SN, SP)
    assert (V0 <= 1e-15).all()
    V0[:] = 0.0
    Ds, Vs, dec = VR.filter_all(T, *g, V0, 3, 0.5, SN, SP)
    for i in range(3):
        centre_only = np.zeros(25, bool)
        centre_only[12] = True
        assert (dec[i]["ftaps"] == centre_only).all() and (Vs[i] == 0).all()
        assert dec[i]["vzero"].any() and (i > 0 or dec[i]["vzero"][4, 5].sum() == 24)  # every other tap inside the image was turned away
        assert np.abs(Ds[i][..., 0:3] - T[..., 0:3]).max() <= 1e-15
    # two pixels with the same luminance still share: d = 0 needs no variance
    T[3, 4] = T[3, 5]
    D = VR.filter_all(T, *g, V0, 1, 0.5, SN, SP)
    assert D[2][0]["ftaps"][3, 4].sum() == 2 and D[2][0]["ftaps"][3, 5].sum() == 2


def _moving_noise_frames(h, w, n, scale=1.0, max_k=0.4):
    frames = []
    for k in range(n):
        g, view, proj = PF(h, w, max_k * k, 0.3 * max_k * k, albedo=(0.9, 0.6, 0.3))
        S = TT._noise_sum(h, w, 10 + k)
        S[..., 0:3] *= np.float32(scale)
        frames.append((S, *g, 2, view, proj, 0))
    return frames


def _pipeline(frames, iterations, sl, dtype, plain=()):
    Ts, Ms, dec = VR.run_sequence(frames, 6.0, 0.3, 0.03, dtype, plain)
    g = frames[-1][1:4]
    V0, e = VR.estimate(Ts[-1], *g, Ms[-1], SN, SP, dtype)
    Ds, Vs, f = VR.filter_all(Ts[-1], *g, V0, iterations, sl, SN, SP, dtype)
    return Ts, Ms, V0, Ds, (dec, e, f)


@pytest.mark.parametrize("k", [6, -6])
def test_a_sum_scaled_by_a_power_of_two_scales_the_result_exactly(k):
    h, w = 10, 13
    for n in (2, 5):  # the window branch and the long branch
        T, M, V0, D, dec = _pipeline(_moving_noise_frames(h, w, n), 3, 0.5, np.float64)
        _, Ms, V0s, Dss, decs = _pipeline(_moving_noise_frames(h, w, n, 2.0 ** k), 3, 0.5, np.float64)
        assert (dec[1]["long"].any()) == (n == 5) and (V0 > 0).all()
        assert (Ms[-1].m1 == M[-1].m1 * 2.0 ** k).all() and (Ms[-1].m2 == M[-1].m2 * 4.0 ** k).all() and (V0s == V0 * 4.0 ** k).all()
        for a, b in zip(D, Dss):
            assert (b[..., 0:3] == a[..., 0:3] * 2.0 ** k).all()
            assert (np.abs(a[..., 0:3] - T[-1][..., 0:3]) > 1e-3).any()  # the filter did something


def test_misses_and_non_finite_pixels_pass_through_and_enter_nothing():
    h, w = 12, 14
    frames = _moving_noise_frames(h, w, 3)
    miss = np.zeros((h, w), bool)
    miss[:, 11:] = True
    for f in frames:
        R.set_miss(f[1:4], miss)
    S = frames[1][0]
    S[3, 4, 1], S[6, 7, 2], S[8, 2, 0], S[2, 12, 0] = np.nan, np.inf, -np.inf, np.nan
    S2 = frames[2][0]
    S2[5, 5, 0] = np.nan
    Ts, Ms, V0, Ds, dec = _pipeline(frames, 3, 0.5, np.float32)
    for y, x in ((3, 4), (6, 7), (8, 2)):
        assert Ms[1].L[y, x] == 0 and Ms[1].m1[y, x] == 0 and Ms[1].m2[y, x] == 0
    assert (Ms[2].L[miss] == 0).all() and Ms[2].L[5, 5] == 0
    hit = ~miss
    hit[5, 5] = False
    for M in Ms:
        assert np.isfinite(M.image()).all()
    assert np.isfinite(V0).all() and (V0[~hit] == 0).all() and (V0[hit] > 0).all()
    m = R.mean_of(S2, 2, np.float32)
    for D in Ds:
        assert np.isfinite(D[hit]).all()
        assert (_bits(D[..., 0:3])[~hit] == _bits(m)[~hit]).all() and (D[..., 3] == 1).all()
    # the pixels around a marker of the frame before lost a tap and went on with the others
    assert (dec[0][2]["mtaps"][hit].sum(axis=-1) >= 1).all() and (dec[0][2]["mtaps"].sum(axis=-1)[hit] < 4).any()


def test_a_pixel_whose_squared_luminance_overflows_is_unknown_and_takes_the_window_s_variance():
    h, w = 9, 11
    frames = _moving_noise_frames(h, w, 5, max_k=0.0)  # a still camera
    for f in frames:
        f[0][4, 5, 0:3] = 4e19  # mean 2e19, l^2 = inf in float32, finite in float64
    Ts, Ms, V0, Ds, dec = _pipeline(frames, 2, 0.5, np.float32)
    for k, M in enumerate(Ms):
        assert M.L[4, 5] == 0 and M.m2[4, 5] == 0 and np.isfinite(M.image()).all()
        others = np.ones((h, w), bool)
        others[4, 5] = False
        assert (M.L[others] == k + 1).all()
    assert np.isfinite(Ts[-1][4, 5]).all() and Ts[-1][4, 5, 3] == 5  # the colour is fine
    e = dec[1]
    assert not e["long"][4, 5] and e["long"].sum() == h * w - 1 and e["wtaps"][4, 5].sum() == 48 and not e["wtaps"][4, 5, 24]
    m1, m2 = Ms[-1].m1.astype(np.float64), Ms[-1].m2.astype(np.float64)
    win = np.ones((h, w), bool)
    win[4, 5] = False
    sel = np.zeros((h, w), bool)
    sel[1:8, 2:9] = True
    sel &= win
    want = m2[sel].mean() - m1[sel].mean() ** 2
    assert abs(V0[4, 5] - want) <= 1e-5 * want and np.isfinite(V0).all() and np.isfinite(Ds[-1][win]).all()
    _, Ms64, _, _, _ = _pipeline(frames, 2, 0.5, np.float64)
    assert Ms64[-1].L[4, 5] == 5  # float64 holds 4e38: the two runs decide differently here, which is what comparable_* reports


def test_reset_restarts_both_histories_and_a_plain_call_the_moments_only():
    h, w = 8, 10
    frames = _moving_noise_frames(h, w, 5)
    reset = [f if k != 2 else f[:7] + (TR.RESET,) for k, f in enumerate(frames)]
    Ts, Ms, _ = VR.run_sequence(reset, 6.0, 0.3, 0.03, np.float64)
    Tf, Mf, _ = VR.run_sequence(frames[2:], 6.0, 0.3, 0.03, np.float64)
    for k in range(3):
        assert (Ts[2 + k] == Tf[k]).all() and (Ms[2 + k].image() == Mf[k].image()).all()
    assert (Ms[2].L == 1).all() and (Ms[1].L[2:-2, 2:-2] == 2).all()
    # a plain call in between: T and the colour history go on, the moments restart on the next moments call
    Tp, Mp, _ = VR.run_sequence(frames, 6.0, 0.3, 0.03, np.float64, plain=(2,))
    Ta, Ma, _ = VR.run_sequence(frames, 6.0, 0.3, 0.03, np.float64)
    for k in range(5):
        assert (Tp[k] == Ta[k]).all()
    assert Mp[2] is None and (Mp[3].L == 1).all() and (Ta[3][2:-2, 2:-2, 3] > 3).all()
    l = _lum64(frames[3][0][..., 0:3].astype(np.float64) / 2 / np.float64(np.float32([0.9, 0.6, 0.3])))
    assert np.abs(Mp[3].m1 - l).max() <= 1e-14 and (Mp[4].L[2:-2, 2:-2] == 2).all()


# ---- the camera sequences of the GPU tests, and what the reference alone says about them ------------------------------------------------

CPU_SEQUENCES = ("still", "subpixel", "turn_dolly", "jump")


def _poses(scene, kind, w, h):
    if kind == "jump":
        p = TT._poses(scene, kind, w, h)
        return p + p[-1:]
    return TT._poses(scene, kind, w, h, frames=FRAMES)


def _iteration_counts(extent):
    return (1, 3, 6) if extent == "33x22" else (1, 3, 5)


def _reference(frames, iterations, plain=(), device=None):
    """Both runs of the reference, in two stages.  The chain: ptx_temporal_accumulate_moments over the sequence, each run keeping its own
    histories -- 'T<k>' per frame, 'mu1', 'mu2', 'LM' of the last frame.  The filter on the last frame: 'V0' and 'D<sigma>/<iterations>',
    both runs from the SAME float32 T and moments -- `device`'s (T, moments image) as read back, or the float32 chain's: what the
    chain's tolerance let through is not charged to the filter a second time, and a decision of the chain that went the other way
    does not spread over the whole frame through five iterations of taps.  Returns {name: (ref32, ref64, comparable)} and the valid
    pixels of the last frame."""
    T32, M32, d32 = VR.run_sequence(frames, TD["max_history"], TD["normal_threshold"], TD["position_threshold"], np.float32, plain)
    T64, M64, d64 = VR.run_sequence(frames, TD["max_history"], TD["normal_threshold"], TD["position_threshold"], np.float64, plain)
    keepM = VR.comparable_moments(d32, d64)
    keepT = TR.comparable_pixels(d32, d64)
    q = {}
    for k in range(len(frames)):
        q["T%d" % k] = (T32[k], T64[k], keepT[k])
    a, b = M32[-1].image(), M64[-1].image()
    q["mu1"], q["mu2"], q["LM"] = (a[..., 0], b[..., 0], keepM[-1]), (a[..., 1], b[..., 1], keepM[-1]), (a[..., 2], b[..., 2], keepM[-1])
    Tin, Min = device if device is not None else (T32[-1], a)
    g = frames[-1][1:4]
    run = {}
    for dt in (np.float32, np.float64):
        mom = VR.Moments(Min[..., 0].astype(dt), Min[..., 1].astype(dt), Min[..., 2].astype(dt))
        V0, e = VR.estimate(Tin, *g, mom, SN, SP, dt)
        run[dt] = (V0, e, {sl: VR.filter_all(Tin, *g, V0, max(iterations), sl, SN, SP, dt) for sl in SIGMAS})
    (V32, e32, f32), (V64, e64, f64) = run[np.float32], run[np.float64]
    valid = e64["valid"]
    keepV = VR.comparable_estimate(np.ones(valid.shape, bool), e32, e64)
    q["V0"] = (V32, V64, keepV)
    for sl in SIGMAS:
        keepD = VR.comparable_filter(keepV, f32[sl][2], f64[sl][2])
        for it in iterations:
            q["D%g/%d" % (sl, it)] = (f32[sl][0][it - 1][..., 0:3], f64[sl][0][it - 1][..., 0:3], keepD[it - 1])
    for name, (a, b, keep) in q.items():  # a value that overflows float32 alone (3e38 over an albedo below 1) is a decision as well
        alike = np.isfinite(a) == np.isfinite(b)
        q[name] = (a, b, keep & (alike if a.ndim == 2 else alike.all(axis=-1)))
    return q, valid, e64


def _gap_and_share(q, valid):
    gaps, share = {}, 0.0
    for name, (a, b, keep) in q.items():
        k = keep if a.ndim == 2 else keep[..., None]
        k = k & (valid if a.ndim == 2 else valid[..., None])
        fin = k & np.isfinite(a) & np.isfinite(b)
        with np.errstate(all="ignore"):
            gaps[name] = float(np.abs(a.astype(np.float64) - b)[fin].max()) if fin.any() else 0.0
        if valid.any():
            share = max(share, float((valid & ~keep).sum()) / float(valid.sum()))
    return gaps, share


def _check_against_reference(frames, got, iterations, label, plain=()):
    """got: the implementation's images under the names of _reference, and 'M' the moment image of the last frame"""
    q, valid, _ = _reference(frames, iterations, plain, (got["T%d" % (len(frames) - 1)], got["M"]))
    gaps, share = _gap_and_share(q, valid)
    print(f"{label}: {int(valid.sum())} valid pixels in the last frame, left out at most {share:.5f}")
    assert share <= min(LEFT_OUT_CAP, 4 * REFERENCE_LEFT_OUT), (label, share)
    m = got["T%d" % (len(frames) - 1)][..., 0:3]  # T holds the mean where a pixel is not valid (the T<k> rows check that)
    for name, (a, b, keep) in q.items():
        G = got[name]
        assert G.dtype == np.float32 and G.shape == b.shape, name
        if name.startswith("T"):
            fv = R.valid_mask(frames[int(name[1:])][0], frames[int(name[1:])][1], frames[int(name[1:])][2], frames[int(name[1:])][4], np.float64)
        else:
            fv = valid
        if name.startswith("D"):  # pixels that are not valid hold T, which holds the mean there, bit for bit
            assert (_bits(G)[~fv] == _bits(m)[~fv]).all(), (label, name)
        elif not name.startswith("T"):
            assert (G[~fv] == 0).all(), (label, name)
        cmp = keep & fv
        cmp = cmp if G.ndim == 2 else np.broadcast_to(cmp[..., None], G.shape)
        assert (np.isfinite(G) == np.isfinite(b))[cmp].all() and (np.isnan(G) == np.isnan(b))[cmp].all(), (label, name)
        fin = cmp & np.isfinite(b)
        if not fin.any():
            continue
        with np.errstate(all="ignore"):
            err = np.abs(G.astype(np.float64) - b)[fin]
        tol = np.maximum(8.0 * gaps[name], 2.0 ** -20 * np.maximum(1.0, np.abs(b[fin])))
        print(f"{label} {name}: max |gpu - ref64| {err.max():.3e}, max |ref32 - ref64| {gaps[name]:.3e}, largest value {np.abs(b[fin]).max():.3e}, "
              f"compared {int(fin.sum())} values")
        assert (err <= tol).all(), (label, name, float(err.max()), gaps[name])
    return gaps, share


def test_reference_gap_and_left_out_share_on_the_cpu_sequences(pkg, orc):
    """What the tolerance and the cap rest on, measured without a GPU: the camera sequences of the GPU tests on first-hit guides from
    the debug view's reference and a synthetic sum, five frames under maxHistory 6 so that both branches of the estimate run."""
    scene = pkg.Scene(TT.SCENE, TT.DETAIL)
    worst, share = {k: 0.0 for k in REFERENCE_GAP}, 0.0
    for kind in CPU_SEQUENCES:
        frames = []
        for f, (p, d) in enumerate(_poses(scene, kind, W, H)):
            scene.set_camera_pose(p, d)
            g = TT._cpu_guides(pkg, orc, scene, W, H)
            frames.append((TT._synthetic_sum(H, W, g[2], 100 + f), *g, 1, *scene.camera_matrices(W, H), 0))
        q, valid, e64 = _reference(frames, (1, 3, 5))
        gaps, s = _gap_and_share(q, valid)
        long = e64["long"]
        print(f"{kind}: left out {s:.5f} of {int(valid.sum())} valid pixels ({int(long.sum())} on the long branch); gaps " +
              ", ".join(f"{k} {v:.3e}" for k, v in gaps.items()))
        assert long.any() and ((valid & ~long).any() or kind == "still"), kind  # both branches of the estimate
        for k in worst:
            worst[k] = max([worst[k]] + [v for name, v in gaps.items() if name.startswith(k)])
        share = max(share, s)
    print("measured:", worst, share)
    for k, v in worst.items():
        assert REFERENCE_GAP[k] / 4 <= v <= REFERENCE_GAP[k], (k, v)
    assert REFERENCE_LEFT_OUT / 4 <= share <= REFERENCE_LEFT_OUT <= 0.005 and 4 * REFERENCE_LEFT_OUT <= LEFT_OUT_CAP


@pytest.mark.parametrize("name", ["default", "texture_test"])
def test_variance_guided_beats_temporal_alone_and_the_fixed_sigma_chain(pkg, orc, name):
    """The quality table of docs/NEXT_ROWS.md section 16 (tools/temporal_quality.py): section 14's sequence of 8 frames of 4 spp
    against the oracle's 192 spp at the last pose.  At VARIANCE_DENOISE_DEFAULTS the variance-guided result is closer than T alone
    and closer than T filtered at TEMPORAL_DENOISE_DEFAULTS, on both scenes with one setting."""
    truth = np.load(os.path.join(util.GOLDEN_DIR, "temporal_truth.npz"))[name].astype(np.float32)
    _, frames = TR.quality_sequence(pkg, orc, name)
    t, cd, vd = pkg.TEMPORAL_DEFAULTS, pkg.TEMPORAL_DENOISE_DEFAULTS, pkg.VARIANCE_DENOISE_DEFAULTS
    Ts, Ms, _ = VR.run_sequence(frames, t["max_history"], t["normal_threshold"], t["position_threshold"], np.float32)
    T, g = Ts[-1], frames[-1][1:4]
    chained = R.denoise(T, *g, 1, cd["iterations"], cd["sigma_color"], cd["sigma_normal"], cd["sigma_position"], np.float32)
    D, V0 = VR.denoise_variance(T, *g, Ms[-1], vd["iterations"], vd["sigma_luminance"], vd["sigma_normal"], vd["sigma_position"], np.float32)
    tmp_err, chn_err, var_err = R.relative_l2(T, truth), R.relative_l2(chained, truth), R.relative_l2(D, truth)
    print(f"{name}: relative L2 error temporal {tmp_err:.4f}, fixed-sigma chain {chn_err:.4f}, variance-guided {var_err:.4f}")
    assert np.isfinite(D).all() and np.isfinite(V0).all()
    assert var_err < tmp_err and var_err < chn_err


# =====================================================================================================
# on the GPU
# =====================================================================================================
EXTENTS = {"67x45": (67, 45), "1x1": (1, 1), "5x3": (5, 3), "33x22": (33, 22), "300x200": (300, 200)}
GPU_CASES = [("67x45", k) for k in CPU_SEQUENCES] + [("1x1", "still"), ("5x3", "subpixel"), ("33x22", "turn_dolly"), ("300x200", "turn_dolly")]
MARKED = (H // 3, 2 * W // 3)  # the 3e38 pixel of the synthetic frames


def _filter_outputs(r, got, iterations):
    """Every (sigmaLuminance, iterations) of a case on the handle's current T and moments, under the names of _reference"""
    T, M = r.read_temporal(), r.read_moments()
    got["M"], got["mu1"], got["mu2"], got["LM"] = M, M[..., 0], M[..., 1], M[..., 2]
    for sl in SIGMAS:
        for it in iterations:
            r.denoise_variance(it, sl, SN, SP)
            D = r.read_denoised()
            assert (D[..., 3] == 1).all()
            got["D%g/%d" % (sl, it)] = np.ascontiguousarray(D[..., 0:3])
            V0 = r.read_variance()
            assert "V0" not in got or (_bits(V0) == _bits(got["V0"])).all()  # the estimate does not depend on either
            got["V0"] = V0
    assert (_bits(r.read_temporal()) == _bits(T)).all() and (_bits(r.read_moments()) == _bits(M)).all()  # both are inputs


def _run(pkg, extent, kind, synthetic=False, scale=1.0, marked=False, plain=()):
    """One sequence through ptx_temporal_accumulate_moments on the scene's handle, with a borrower making the plain call in lockstep"""
    s, r = TT._gpu(pkg)
    w, h = EXTENTS[extent]
    r.set_tile_shard(0, 1, 32)
    r.resize(w, h)  # drops the histories of the case before
    b = TT._borrower(pkg, r, w, h)
    frames, got = [], {}
    for f, pose in enumerate(_poses(s, kind, w, h)):
        frame, u = TT._render_frame(s, r, w, h, pose, f, synthetic)
        if marked:
            frame[0][MARKED][0:3] = 3e38
        if scale != 1.0:
            frame[0][..., 0:3] *= np.float32(scale)
        if marked or scale != 1.0:
            r.write_accumulation(frame[0])
        frames.append(frame)
        if f in plain:
            r.temporal_accumulate(frame[4], frame[5], frame[6], **TD)
        else:
            r.temporal_accumulate_moments(frame[4], frame[5], frame[6], **TD)
        T = r.read_temporal()
        b.write_accumulation(frame[0])
        b.render_guides(u)
        b.temporal_accumulate(frame[4], frame[5], frame[6], **TD)
        assert (_bits(T) == _bits(b.read_temporal())).all(), (extent, kind, f)  # T and L are the plain call's, bit for bit
        got["T%d" % f] = T
        assert (_bits(r.readback()) == _bits(frame[0])).all()  # the sum is an input
        for k in range(3):
            assert (_bits(r.read_guide(k)) == _bits(frame[1 + k])).all()  # ... and so are the guides
    b.close()
    return r, frames, got


@pytest.mark.gpu
@pytest.mark.parametrize("case", GPU_CASES, ids=lambda c: "%s-%s" % c)
def test_moments_variance_and_filter_against_float64_reference(pkg, case):
    extent, kind = case
    r, frames, got = _run(pkg, extent, kind)
    _filter_outputs(r, got, _iteration_counts(extent))
    _check_against_reference(frames, got, _iteration_counts(extent), "%s %s" % case)
    valid = R.valid_mask(got["T4"], frames[-1][1], frames[-1][2], 1, np.float32)
    LM = got["LM"]
    if extent in ("67x45", "300x200"):
        assert valid.sum() > 200 and (~valid).sum() > 20 and (got["V0"][valid] > 0).mean() > 0.9
        changed = (_bits(got["D0.5/3"]) != _bits(got["T4"][..., 0:3])).any(axis=-1)
        assert changed[valid].mean() > 0.9 and not changed[~valid].any()
    if kind == "still":
        assert (LM[valid] == 5).all()
    if kind in ("subpixel", "turn_dolly") and extent in ("67x45", "300x200"):  # both branches of the estimate
        assert (LM[valid] >= 4).mean() > 0.5 and ((LM[valid] > 0) & (LM[valid] < 4)).any()


@pytest.mark.gpu
def test_synthetic_frames_with_markers_a_hot_pixel_and_a_3e38_pixel(pkg):
    r, frames, got = _run(pkg, "67x45", "subpixel", synthetic=True, marked=True)
    _filter_outputs(r, got, (1, 3, 5))
    _check_against_reference(frames, got, (1, 3, 5), "synthetic subpixel")
    assert got["LM"][MARKED] == 0 and got["LM"][2, 3] == 0 and got["LM"][4, 5] == 0  # l l overflows; not valid; not valid
    rest = np.ones((H, W), bool)
    rest[2, 3] = rest[4, 5] = rest[MARKED] = False
    for name, D in got.items():
        if name.startswith("D"):
            assert np.isnan(D[2, 3, 0]) and np.isposinf(D[4, 5, 1]) and np.isfinite(D[rest]).all(), name  # the markers keep to themselves
    assert np.isfinite(got["V0"]).all() and np.isfinite(got["M"]).all()


@pytest.mark.gpu
def test_a_sum_scaled_by_64_gives_the_result_scaled_by_64(pkg):
    r, frames, got = _run(pkg, "67x45", "subpixel", synthetic=True)
    _filter_outputs(r, got, (1, 3, 5))
    _, _, big = _run(pkg, "67x45", "subpixel", synthetic=True, scale=64.0)
    _filter_outputs(r, big, (1, 3, 5))
    back = {}
    for name, a in big.items():
        k = 64.0 ** 2 if name in ("mu2", "V0") else 1.0 if name == "LM" else 64.0
        back[name] = (a / np.float32(k)).astype(np.float32)
        if name.startswith("T"):
            back[name][..., 3] = a[..., 3]
    back["M"] = np.stack([back["mu1"], back["mu2"], back["LM"], np.zeros_like(back["LM"])], axis=-1)
    _check_against_reference(frames, back, (1, 3, 5), "scaled by 64")
    for name in sorted(got):
        if name != "M":
            fin = np.isfinite(got[name])
            same = (_bits(back[name])[fin] == _bits(got[name])[fin])
            print(f"scaled by 64, {name}: {'bit for bit' if same.all() else '%d of %d values differ' % ((~same).sum(), same.size)}")


@pytest.mark.gpu
def test_moved_geometry_restarts_its_moments_and_the_background_keeps_them(pkg):
    s, r = TT._gpu(pkg, "animated_test")
    r.resize(W, H)
    pose = TT._base_pose(s, W, H)[0:2]
    frames, got = [], {}
    for f in range(2):
        if f:
            assert s.update(0.37)
            r.update_animation(*s.animation_state())
        frame, _ = TT._render_frame(s, r, W, H, pose, f)
        frames.append(frame)
        r.temporal_accumulate_moments(frame[4], frame[5], frame[6], **TD)
        got["T%d" % f] = r.read_temporal()
    _filter_outputs(r, got, (1, 3))
    f0, f1 = frames
    _check_against_reference(frames, got, (1, 3), "animated_test")
    both = R.valid_mask(f1[0], f1[1], f1[2], 1, np.float32) & R.valid_mask(f0[0], f0[1], f0[2], 1, np.float32)
    unmoved = both & (_bits(f0[1]) == _bits(f1[1])).all(axis=-1) & (_bits(f0[2]) == _bits(f1[2])).all(axis=-1)
    shift = np.abs(((f1[2][..., 0:3].astype(np.float64) - f0[2][..., 0:3]) * f1[1][..., 0:3]).sum(axis=-1))
    moved = both & (shift > 2 * TD["position_threshold"] * f1[2][..., 3])
    assert unmoved.sum() > 200 and moved.sum() > 20
    assert (got["LM"][unmoved] == 2).all() and (got["LM"][moved] == 1).all()


@pytest.mark.gpu
def test_the_output_stage_follows_and_the_path_tracer_does_not_notice(pkg):
    r, frames, got = _run(pkg, "67x45", "subpixel", synthetic=True)
    S = frames[-1][0]
    r.denoise_variance(3, 0.5, SN, SP)
    D = r.read_denoised()
    g = pkg.Renderer()
    g.resize(W, H)
    g.write_accumulation(D)
    for tone in (pkg.TONE_MAPPING_SDR, pkg.TONE_MAPPING_HDR):
        r.postprocess_denoised(7, tone_mapping=tone, **POST)
        g.postprocess(1, tone_mapping=tone, **POST)
        for fmt in (pkg.OUTPUT_RGBA8_SRGB, pkg.OUTPUT_RGBA32F):
            a, b = r.read_output(fmt), g.read_output(fmt)
            assert a.dtype == b.dtype and (a.view(np.uint8) == b.view(np.uint8)).all(), (tone, fmt)
        for sw, sh, fmt, mode in ((W, H, pkg.PRESENT_R8G8B8A8_SRGB, 0), (100, 37, pkg.PRESENT_R16G16B16A16_SFLOAT, 0)):
            r.present(sw, sh, fmt, mode)
            g.present(sw, sh, fmt, mode)
            assert (r.read_present().view(np.uint8) == g.read_present().view(np.uint8)).all(), (tone, sw, sh, fmt)
    g.close()
    out = r.read_output(pkg.OUTPUT_RGBA32F)
    assert out[2, 3, 0] >= 1 and out[4, 5, 1] >= 1  # the NaN / Inf pixels still get postprocess.comp's markers
    assert (_bits(r.readback()) == _bits(S)).all() and (_bits(r.read_temporal()) == _bits(got["T4"])).all()
    # the older entry points compute what they did: ptx_denoise_temporal on this T is ptx_denoise on a copy of it
    f = TT._borrower(pkg, r, W, H)
    f.write_accumulation(got["T4"])
    s = TT._gpu(pkg)[0]
    u = s.uniform(W, H, bounces=4, sample_count=1, total_samples=4)
    f.render_guides(u)
    r.denoise_temporal(2, 0.5, SN, SP)
    f.denoise(1, 2, 0.5, SN, SP)
    assert (_bits(r.read_denoised()) == _bits(f.read_denoised())).all()
    f.close()
    # the next ptx_render continues the sum as if nothing had happened
    r.resize(W, H)
    up = s.uniform(W, H, bounces=4)

    def path_traced(n):
        r.reset()
        for k in range(n):
            up.TotalSamples = k
            r.render(up, s.lights)
        return r.readback()
    two, three = path_traced(2), path_traced(3)
    assert (_bits(path_traced(2)) == _bits(two)).all()
    r.render_guides(up)
    view, proj = s.camera_matrices(W, H)
    r.temporal_accumulate_moments(2, view, proj, **TD)
    r.temporal_accumulate_moments(2, view, proj, **TD)
    r.denoise_variance()
    assert (_bits(r.readback()) == _bits(two)).all()
    up.TotalSamples = 2
    r.render(up, s.lights)
    assert (_bits(r.readback()) == _bits(three)).all()


def _replay(b, frames, flags=None, plain=()):
    """The frames' own sums and uniforms on another handle: (T, moments or None) per frame"""
    out = []
    for k, (frame, u) in enumerate(frames):
        b.write_accumulation(frame[0])
        b.render_guides(u)
        call = b.temporal_accumulate if k in plain else b.temporal_accumulate_moments
        call(frame[4], frame[5], frame[6], flags=flags[k] if flags else 0, **TD)
        out.append((b.read_temporal(), None if k in plain else b.read_moments()))
    return out


def _same(a, b):
    return all((_bits(x) == _bits(y)).all() for x, y in zip(a, b) if x is not None or y is not None)


@pytest.mark.gpu
def test_borrower_reset_plain_call_in_between_and_resize(pkg):
    s, r = TT._gpu(pkg)
    r.set_tile_shard(0, 1, 32)
    r.resize(W, H)
    lib = r.lib
    poses = _poses(s, "turn_dolly", W, H)
    frames = [TT._render_frame(s, r, W, H, p, f) for f, p in enumerate(poses)]
    own = _replay(r, frames[0:2] + frames[2:5], flags=[0, 0, pkg.TEMPORAL_RESET, 0, 0])
    r.denoise_variance(3, 0.5, SN, SP)
    D, V0 = r.read_denoised(), r.read_variance()
    # a borrower computes what its owner does; two sequences separated by RESET are two fresh handles'
    for seq, want in ((frames[0:2], own[0:2]), (frames[2:5], own[2:5])):
        b = TT._borrower(pkg, r, W, H)
        for a, c in zip(_replay(b, seq), want):
            assert _same(a, c)
        if len(seq) == 3:
            b.denoise_variance(3, 0.5, SN, SP)
            assert (_bits(b.read_denoised()) == _bits(D)).all() and (_bits(b.read_variance()) == _bits(V0)).all()
        b.close()
    assert (own[2][1][..., 2] <= 1).all() and (own[4][1][..., 2] > 2).any()
    # a plain call in between: T goes on as if nothing had happened, the stage is refused until the next moments call, which restarts M
    buf = np.zeros((H, W, 4), np.float32)
    vbuf = np.zeros((H, W), np.float32)
    dd = pkg.DenoiseDesc(1, 2, 0.5, SN, SP, 0, 0)
    r.resize(W, H)
    mixed = _replay(r, frames[0:3], plain=(2,))
    assert lib.ptx_read_moments(r.handle, buf.ctypes.data, buf.nbytes) == 5 and lib.ptx_denoise_variance(r.handle, C.byref(dd)) == 5 and not buf.any()
    mixed += _replay(r, frames[3:5])
    b = TT._borrower(pkg, r, W, H)
    straight = _replay(b, frames)
    b.close()
    for k in range(5):
        assert (_bits(mixed[k][0]) == _bits(straight[k][0])).all(), k
    valid = mixed[3][0][..., 3] > 0
    assert (mixed[3][1][..., 2][valid] == 1).all() and (mixed[3][0][..., 3][valid] > 2).any() and (mixed[4][1][..., 2] > 1).any()
    fr = [f[0] for f in frames]
    Tm, Mm, _ = VR.run_sequence(fr, TD["max_history"], TD["normal_threshold"], TD["position_threshold"], np.float64, plain=(2,))
    ok = valid & np.isfinite(Mm[3].m1)
    assert np.abs(mixed[3][1][..., 0] - Mm[3].m1)[ok].max() <= 2.0 ** -20 * max(1.0, float(np.abs(Mm[3].m1[ok]).max()))  # M = mu of the frame: no history in it
    r.denoise_variance(2, 0.5, SN, SP)
    # ptx_resize drops everything
    r.resize(W, H)
    assert lib.ptx_read_moments(r.handle, buf.ctypes.data, buf.nbytes) == 5 and lib.ptx_read_variance(r.handle, vbuf.ctypes.data, vbuf.nbytes) == 5
    assert lib.ptx_denoise_variance(r.handle, C.byref(dd)) == 5 and not buf.any() and not vbuf.any()
    again = _replay(r, frames[4:5])
    assert (again[0][1][..., 2] <= 1).all() and (again[0][0][..., 3] <= 1).all()


@pytest.mark.gpu
def test_refusals_leave_d_t_and_both_histories_intact(pkg):
    import torch

    s, r = TT._gpu(pkg)
    r.set_tile_shard(0, 1, 32)
    r.resize(W, H)
    lib = r.lib
    poses = _poses(s, "subpixel", W, H)
    frames = [TT._render_frame(s, r, W, H, p, f) for f, p in enumerate(poses[0:3])]
    T, M = _replay(r, frames[0:2])[-1]
    r.denoise_variance(2, 0.5, SN, SP)
    D, V0 = r.read_denoised(), r.read_variance()
    view, proj = frames[2][0][5], frames[2][0][6]

    def desc(total=1, mh=6.0, nt=0.3, pt=0.03, flags=0, reserved=0):
        d = pkg.TemporalDesc()
        d.View[:], d.Proj[:] = [float(v) for v in view], [float(v) for v in proj]
        d.totalSamples, d.maxHistory, d.normalThreshold, d.positionThreshold, d.flags, d.reserved = total, mh, nt, pt, flags, reserved
        return d

    def intact():
        assert (_bits(r.read_temporal()) == _bits(T)).all() and (_bits(r.read_moments()) == _bits(M)).all()
        assert (_bits(r.read_denoised()) == _bits(D)).all() and (_bits(r.read_variance()) == _bits(V0)).all()

    nan, inf = float("nan"), float("inf")
    bad = [desc(total=0), desc(mh=0.5), desc(mh=nan), desc(mh=inf), desc(nt=0.0), desc(nt=nan), desc(pt=-0.03), desc(pt=inf), desc(flags=2), desc(flags=0x80000000),
           desc(reserved=1)]
    for d in bad:
        assert lib.ptx_temporal_accumulate_moments(r.handle, C.byref(d)) == 1
    assert lib.ptx_temporal_accumulate_moments(r.handle, None) == 1 and lib.ptx_denoise_variance(r.handle, None) == 1
    buf, vbuf = np.zeros((H, W, 4), np.float32), np.zeros((H, W), np.float32)
    assert lib.ptx_read_moments(r.handle, None, buf.nbytes) == 1 and lib.ptx_read_variance(r.handle, None, vbuf.nbytes) == 1
    assert lib.ptx_read_moments(r.handle, buf.ctypes.data, buf.nbytes - 16) == 1 and lib.ptx_read_variance(r.handle, vbuf.ctypes.data, buf.nbytes) == 1
    assert lib.ptx_read_variance(r.handle, vbuf.ctypes.data, vbuf.nbytes - 4) == 1 and not buf.any() and not vbuf.any()
    dd = lambda **kw: pkg.DenoiseDesc(**{**dict(totalSamples=1, iterations=2, sigmaColor=0.5, sigmaNormal=SN, sigmaPosition=SP, flags=0, reserved=0), **kw})  # noqa: E731
    for d in (dd(iterations=0), dd(iterations=7), dd(sigmaColor=0.0), dd(sigmaColor=-1.0), dd(sigmaColor=nan), dd(sigmaColor=inf), dd(sigmaNormal=0.0),
              dd(sigmaPosition=nan), dd(flags=1), dd(reserved=1)):
        assert lib.ptx_denoise_variance(r.handle, C.byref(d)) == 1
    intact()
    # a tile shard of a larger world, a bound shard accumulation buffer
    r.set_tile_shard(0, 2, 8)
    assert lib.ptx_temporal_accumulate_moments(r.handle, C.byref(desc())) == 5 and lib.ptx_denoise_variance(r.handle, C.byref(dd())) == 5
    shard = torch.zeros(r.shard_bytes(0) // 4, dtype=torch.float32, device="cuda")
    r.bind_shard_accumulation(shard.data_ptr(), r.shard_bytes(0))
    assert lib.ptx_temporal_accumulate_moments(r.handle, C.byref(desc())) == 5 and lib.ptx_denoise_variance(r.handle, C.byref(dd())) == 5
    r.bind_shard_accumulation(0)
    r.set_tile_shard(0, 1, 32)
    intact()
    # no image; an image without guides; guides without an accumulate; a plain accumulate
    fresh = pkg.Renderer()
    assert lib.ptx_temporal_accumulate_moments(fresh.handle, C.byref(desc())) == 5 and lib.ptx_denoise_variance(fresh.handle, C.byref(dd())) == 5
    fresh.share_scene(r)
    fresh.resize(W, H)
    assert lib.ptx_temporal_accumulate_moments(fresh.handle, C.byref(desc())) == 5
    fresh.render_guides(frames[2][1])
    assert lib.ptx_read_moments(fresh.handle, buf.ctypes.data, buf.nbytes) == 5 and lib.ptx_read_variance(fresh.handle, vbuf.ctypes.data, vbuf.nbytes) == 5
    assert lib.ptx_denoise_variance(fresh.handle, C.byref(dd())) == 5
    assert lib.ptx_temporal_accumulate(fresh.handle, C.byref(desc())) == 0 and lib.ptx_denoise_variance(fresh.handle, C.byref(dd())) == 5
    fresh.close()
    # the histories are intact as well: the third frame gives what a handle that never saw a refusal gives
    third = _replay(r, frames[2:3])[0]
    b = TT._borrower(pkg, r, W, H)
    assert _same(_replay(b, frames)[-1], third) and (third[1][..., 2] > 2).any()
    b.close()
    assert lib.ptx_denoise_variance(r.handle, C.byref(dd(totalSamples=0))) == 0  # the desc's count is ignored: T is a mean
