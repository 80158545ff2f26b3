"""Temporal accumulation (include/ptx.h ptx_temporal_accumulate / ptx_denoise_temporal, csrc/pt_temporal.hpp, docs/NEXT_ROWS.md
section 14) against tests/temporal_ref.py.

Tolerance.  The reference runs on the device's own read-back sums and guides, frame by frame, and keeps its own history in float32
and in float64.  The bound of a case is measured ON THE REFERENCE ALONE, inside the test: 8 x max |ref(float32) - ref(float64)| over
the frames of that very case, with a floor of 2^-20 max(1, |value|).  The accumulation takes decisions (which texel, which taps
count, found or not); a pixel on which the two runs of the reference decide differently, or whose history came through such a pixel,
is left out (temporal_ref.comparable_pixels).  That is a condition, not a measurement: its share is capped at 4 x the share the
reference alone leaves out on the CPU's own sequences (REFERENCE_LEFT_OUT) and never above 2 % of the valid pixels.
Pixels that are not valid must hold the mean bit for bit."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import denoise_ref as R
import temporal_ref as TR
import util

W, H = 67, 45
DETAIL = 0.25
SCENE = "texture_test"
TD = dict(max_history=3.0, normal_threshold=0.3, position_threshold=0.03)  # the cap is reached inside a four-frame sequence
POST = dict(exposure=1.0, bloom_threshold=0.8, bloom_intensity=0.35)
LEFT_OUT_CAP = 0.02
# Measured on the CPU (test_reference_gap_and_left_out_share_on_the_cpu_sequences recomputes both): over the camera sequences below at
# 67 x 45 on first-hit guides computed without a GPU, the largest |ref32 - ref64| of T.rgb and the largest share of valid pixels that
# comparable_pixels leaves out in a frame.
REFERENCE_GAP = 4.0e-3  # measured 2.7e-3, on values up to 3e5 (the synthetic sum's hot pixel over the albedo floor)
REFERENCE_LEFT_OUT = 0.005  # measured 0.0041 (8 of 1938 pixels, after the jump); every other sequence leaves nothing out


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# =====================================================================================================
# without a GPU
# =====================================================================================================
def test_header_declares_and_package_exports_the_temporal_stage(pkg):
    header = open(os.path.join(pkg.REPO_DIR, "include", "ptx.h")).read()
    decls = {
        "ptx_temporal_accumulate": r"PTX_API int ptx_temporal_accumulate\(PtxRenderer \*r, const PtxTemporalDesc \*desc\);",
        "ptx_read_temporal": r"PTX_API int ptx_read_temporal\(PtxRenderer \*r, void \*host, size_t bytes\);",
        "ptx_device_temporal_ptr": r"PTX_API void \*ptx_device_temporal_ptr\(PtxRenderer \*r\);",
        "ptx_denoise_temporal": r"PTX_API int ptx_denoise_temporal\(PtxRenderer \*r, const PtxDenoiseDesc \*desc\);",
    }
    lib = pkg.load_hip()
    for name, decl in decls.items():
        assert re.search(decl, header), name
        assert name in pkg.PTX_SYMBOLS
        assert hasattr(lib, name), name
    assert "#define PTX_ABI_VERSION 5u" in header and "PTX_FN_COUNT = 38" in header  # additions only
    assert re.search(r"PTX_TEMPORAL_RESET = 1\b", header) and pkg.TEMPORAL_RESET == 1 and TR.RESET == 1
    assert re.search(r"typedef struct PtxTemporalDesc \{\s*float View\[16\], Proj\[16\];[^}]*uint32_t totalSamples;[^}]*float maxHistory;[^}]*"
                     r"float normalThreshold;[^}]*float positionThreshold;[^}]*uint32_t flags;[^}]*uint32_t reserved;[^}]*\} PtxTemporalDesc;", header)
    D = pkg.TemporalDesc
    assert C.sizeof(D) == 152 and D.Proj.offset == 64 and D.totalSamples.offset == 128 and D.maxHistory.offset == 132 and D.reserved.offset == 148
    # the semantics are in the header as text: the reference is written from it
    for phrase in ("SAME-CAMERA RULE", "x0 = floor(u)", ">= 1/64", "L = min(L_h + 1, maxHistory)", "c_acc = c_h + (c(p) - c_h) / L", "112 bytes per pixel",
                   "no per-object motion vectors", "CALLER's duty"):
        assert phrase in header, phrase
    for method in ("temporal_accumulate", "read_temporal", "temporal_ptr", "denoise_temporal"):
        assert callable(getattr(pkg.Renderer, method))
    t, d = pkg.TEMPORAL_DEFAULTS, pkg.TEMPORAL_DENOISE_DEFAULTS
    assert t == dict(max_history=32.0, normal_threshold=0.3, position_threshold=0.03)
    assert 1 <= d["iterations"] <= 6 and d["sigma_color"] >= 0 and d["sigma_normal"] > 0 and d["sigma_position"] > 0
    hosth = open(os.path.join(pkg.REPO_DIR, "include", "ptx_host.h")).read()
    assert re.search(r"PTX_API int pth_scene_camera_matrices\(PthScene \*s, uint32_t width, uint32_t height, float view\[16\], float proj\[16\]\);", hosth)
    assert "pth_scene_camera_matrices" in pkg.PTH_SYMBOLS and hasattr(pkg.load_host(), "pth_scene_camera_matrices")
    host = open(os.path.join(pkg.PKG_DIR, "host", "RendererHip.h")).read()
    assert "struct TemporalSettings" in host and "SetSettings(const TemporalSettings &" in host
    assert re.search(r"struct TemporalSettings\s*\{\s*bool Enabled = false;", host)
    cam = open(os.path.join(pkg.PKG_DIR, "host", "Camera.h")).read()
    assert "GetViewMatrix" in cam and "GetProjectionMatrix" in cam


def test_camera_matrices_are_the_inverses_of_the_uniform_s(pkg):
    s = pkg.Scene("default", DETAIL)
    for pose in (None, ((1.0, 2.0, -3.0), (0.3, -0.2, 0.9))):
        if pose:
            s.set_camera_pose(*pose)
        u = s.uniform(W, H)
        view, proj = s.camera_matrices(W, H)
        assert view.dtype == np.float32 and view.shape == (16,) and proj.shape == (16,)
        V, P = view.reshape(4, 4).T.astype(np.float64), proj.reshape(4, 4).T.astype(np.float64)
        Vi, Pi = [np.frombuffer(m, np.float32).reshape(4, 4).T.astype(np.float64) for m in (u.ViewInverse, u.ProjInverse)]
        assert np.abs(V @ Vi - np.eye(4)).max() <= 1e-5 and np.abs(P @ Pi - np.eye(4)).max() <= 1e-5
        # the convention of the header: w is the view depth, and a primary ray's pixel centre comes back
        assert (P[3] == (0, 0, 1, 0)).all()
        xy = np.float64([[10, 7], [0, 0], [W - 1, H - 1]])
        ndc = (xy + 0.5) / (W, H) * 2 - 1
        target = (Pi @ np.stack([ndc[:, 0], ndc[:, 1], np.ones(3), np.ones(3)])).T
        d = target[:, 0:3] / np.linalg.norm(target[:, 0:3], axis=1, keepdims=True)
        world = Vi[0:3, 3] + (Vi[0:3, 0:3] @ (d * 4.0).T).T
        uu, vv, ok = TR.project(view, proj, world, W, H, np.float64)
        assert ok.all() and np.abs(uu - xy[:, 0]).max() <= 1e-3 and np.abs(vv - xy[:, 1]).max() <= 1e-3


PX, DIST = 0.01, 5.0


def _plane_frame(h, w, kx=0.0, ky=0.0, **kw):
    """denoise_ref.plane_guides -- pixel (x, y) sees the world point -PX (x + kx, y + ky, 0) -- and the small look-at / perspective
    camera that sees it so: head-on from DIST away, one pixel's footprint PX on the plane.  Returns (guides, view, proj)."""
    g = R.plane_guides(h, w, distance=DIST, pixel=PX, **kw)
    g[1][..., 0] -= np.float32(kx * PX)
    g[1][..., 1] -= np.float32(ky * PX)
    eye = np.float64([(0.5 - w / 2 - kx) * PX, (0.5 - h / 2 - ky) * PX, -DIST])
    view = TR.look_at(eye, eye + (0.0, 0.0, 1.0), up=(0.0, -1.0, 0.0))
    proj = TR.perspective(2.0 * np.arctan(PX * h / (2.0 * DIST)), w, h)
    return g, view, proj


def _noise_sum(h, w, seed, samples=2):
    S = np.zeros((h, w, 4), np.float32)
    S[..., 0:3] = np.random.default_rng(seed).uniform(0.1, 1.0, (h, w, 3)) * samples
    S[..., 3] = samples
    return S


def _acc(S, frame, hist, flags=0, dtype=np.float64, samples=2, **over):
    g, view, proj = frame
    p = dict(max_history=32.0, normal_threshold=0.3, position_threshold=0.03)
    p.update(over)
    return TR.accumulate(S, *g, samples, view, proj, hist, p["max_history"], p["normal_threshold"], p["position_threshold"], flags, dtype)


def test_plane_camera_projects_every_pixel_onto_itself():
    h, w = 9, 13
    g, view, proj = _plane_frame(h, w, 2.0, 1.0)
    u, v, ok = TR.project(view, proj, g[1][..., 0:3].astype(np.float64), w, h, np.float64)
    yy, xx = np.mgrid[0:h, 0:w]
    assert ok.all() and np.abs(u - xx).max() <= 1e-3 and np.abs(v - yy).max() <= 1e-3


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_still_camera_averages_and_then_decays(dtype):
    """L = k and c_acc = the mean of the frames; past maxHistory the exponential average with weight 1 / maxHistory.  The albedo is
    demodulated and put back, its last channel from below the floor."""
    h, w = 7, 10
    frame = _plane_frame(h, w, albedo=(0.8, 0.5, 0.004))
    sums = [_noise_sum(h, w, k) for k in range(6)]
    means = [s[..., 0:3].astype(np.float64) / 2 for s in sums]
    eps = np.finfo(dtype).eps
    hist = None
    for k in range(4):
        T, hist, d = _acc(sums[k], frame, hist, dtype=dtype, max_history=4.0)
        assert T.dtype == np.dtype(dtype) and (T[..., 3] == k + 1).all() and d["same_camera"] == (k > 0)
        assert np.abs(T[..., 0:3] - np.mean(means[:k + 1], axis=0)).max() <= 32 * eps
    ema = np.mean(means[:4], axis=0)
    for k in (4, 5):
        T, hist, _ = _acc(sums[k], frame, hist, dtype=dtype, max_history=4.0)
        ema = ema + (means[k] - ema) / 4
        assert (T[..., 3] == 4).all() and np.abs(T[..., 0:3] - ema).max() <= 32 * eps


def test_one_pixel_pan_shifts_the_history_by_one_pixel():
    h, w = 6, 11
    s0, s1 = _noise_sum(h, w, 1), _noise_sum(h, w, 2)
    T0, hist, _ = _acc(s0, _plane_frame(h, w, 0.0), None)
    T1, _, d = _acc(s1, _plane_frame(h, w, 1.0), hist)  # pixel x now sees what pixel x + 1 saw
    assert not d["same_camera"]
    c1 = s1[..., 0:3].astype(np.float64) / 2
    # the float32 matrices put u within 1e-4 of the integer, on either side of floor's edge: the answer holds to that weight
    assert np.abs(T1[:, :-1, 0:3] - (T0[:, 1:, 0:3] + c1[:, :-1]) / 2).max() <= 2e-4 and np.abs(T1[:, :-1, 3] - 2).max() <= 2e-4
    assert (T1[:, -1, 3] == 1).all() and (T1[:, -1, 0:3] == c1[:, -1]).all()  # the entering column


def test_half_pixel_pan_is_the_two_tap_mean():
    h, w = 6, 11
    s0, s1 = _noise_sum(h, w, 1), _noise_sum(h, w, 2)
    T0, hist, _ = _acc(s0, _plane_frame(h, w, 0.0), None)
    T1, _, d = _acc(s1, _plane_frame(h, w, 0.5), hist)
    c1 = s1[..., 0:3].astype(np.float64) / 2
    two = (T0[:, :-1, 0:3] + T0[:, 1:, 0:3]) / 2
    assert np.abs(T1[:, :-1, 0:3] - (two + c1[:, :-1]) / 2).max() <= 2e-4
    # the last column has one of its two taps inside the image: weight 1/2 >= 1/64, renormalised
    assert np.abs(T1[:, -1, 0:3] - (T0[:, -1, 0:3] + c1[:, -1]) / 2).max() <= 2e-4 and (np.abs(T1[..., 3] - 2) <= 1e-12).all()


def test_coverage_below_one_64th_is_no_history():
    """A pan by 0.9 pixels both ways: the corner pixel has one tap inside the image, of weight 0.1 x 0.1 < 1/64; its neighbours along
    the edges have 0.1 >= 1/64."""
    h, w = 6, 8
    T0, hist, _ = _acc(_noise_sum(h, w, 1), _plane_frame(h, w), None)
    T1, _, d = _acc(_noise_sum(h, w, 2), _plane_frame(h, w, 0.9, 0.9), hist)
    L = T1[..., 3]
    assert L[-1, -1] == 1 and not d["found"][-1, -1] and d["taps"][-1, -1].sum() == 1
    assert (np.abs(np.delete(L.ravel(), h * w - 1) - 2) <= 1e-9).all() and d["found"].sum() == h * w - 1


def test_normal_step_or_plane_offset_restarts_exactly_the_affected_pixels():
    h, w = 8, 12
    s0, s1 = _noise_sum(h, w, 1), _noise_sum(h, w, 2)
    part = np.zeros((h, w), bool)
    part[2:5, 3:9] = True
    for change in ("normal", "offset", "small offset"):
        f0, f1 = _plane_frame(h, w), _plane_frame(h, w)
        if change == "normal":
            f1[0][0][part, 0:3] = np.float32([0.0, np.sin(0.4), np.cos(0.4)])  # |dn| = 2 sin 0.2 = 0.397 > 0.3
        elif change == "offset":
            f1[0][1][part, 2] += np.float32(0.031 * DIST)  # along the normal, just above positionThreshold t
        else:
            f1[0][1][part, 2] += np.float32(0.029 * DIST)
        _, hist, _ = _acc(s0, f0, None)
        T1, _, d = _acc(s1, f1, hist)
        assert d["same_camera"]
        restarted = part if change != "small offset" else np.zeros_like(part)
        assert (T1[..., 3][restarted] == 1).all() and (T1[..., 3][~restarted] == 2).all(), change
        assert (T1[restarted][:, 0:3] == s1[restarted][:, 0:3].astype(np.float64) / 2).all()


def test_a_point_behind_the_previous_camera_has_no_history():
    h, w = 6, 9
    g, view, proj = _plane_frame(h, w)
    eye = np.float64([0.0, 0.0, -DIST])
    away = TR.look_at(eye, eye - (0.0, 0.0, 1.0), up=(0.0, -1.0, 0.0))  # the plane lies behind this camera: clip.w = -DIST
    _, hist, _ = _acc(_noise_sum(h, w, 1), (g, away, proj), None)
    T1, _, d = _acc(_noise_sum(h, w, 2), (g, view, proj), hist)
    assert (T1[..., 3] == 1).all() and (d["cell"] == -2 ** 31).all() and not d["found"].any() and d["used_history"]
    # ... the same history under the camera that sees the plane is found everywhere
    hist.view = view.copy()
    hist.view[12] += np.float32(1e-6)  # not the same camera bit for bit: the points are projected
    T2, _, d2 = _acc(_noise_sum(h, w, 2), (g, view, proj), hist)
    assert not d2["same_camera"] and d2["found"].all()


def test_camera_jump_and_reset_start_a_new_history():
    h, w = 6, 9
    s = [_noise_sum(h, w, k) for k in range(4)]
    near = _plane_frame(h, w)
    T0, hist, _ = _acc(s[0], near, None)
    T1, hist1, _ = _acc(s[1], near, hist)
    far = _plane_frame(h, w, 400.0, -250.0)  # another part of the plane: every point projects far outside the previous image
    Tj, _, d = _acc(s[2], far, hist1)
    fresh, _, _ = _acc(s[2], far, None)
    assert (Tj[..., 3] == 1).all() and (Tj == fresh).all() and not d["found"].any()
    Tr, histr, dr = _acc(s[2], near, hist1, flags=TR.RESET)  # the same camera, told to forget
    fresh, _, _ = _acc(s[2], near, None)
    assert (Tr == fresh).all() and not dr["used_history"]
    T3, _, _ = _acc(s[3], near, histr)
    assert (T3[..., 3] == 2).all() and np.abs(T3[..., 0:3] - (s[2][..., 0:3].astype(np.float64) + s[3][..., 0:3]) / 4).max() <= 1e-14


def test_misses_and_non_finite_pixels_pass_through_and_contaminate_nothing():
    h, w = 10, 14
    s0, s1 = _noise_sum(h, w, 1), _noise_sum(h, w, 2)
    f0, f1 = _plane_frame(h, w, albedo=(0.5, 0.5, 0.005)), _plane_frame(h, w, 0.5, 0.5, albedo=(0.5, 0.5, 0.005))
    miss = np.zeros((h, w), bool)
    miss[:, 10:] = True
    for f in (f0, f1):
        R.set_miss(f[0], miss)
    s0[3, 4, 1], s0[6, 7, 2], s0[8, 2, 0] = np.nan, np.inf, -np.inf
    s0[2, 12, 0] = np.nan  # in the miss region
    s0[5, 5, 2] = 3e38  # valid, but its demodulated colour overflows float32: a history that is not finite
    T0, hist, _ = _acc(s0, f0, None, dtype=np.float32)
    m0 = R.mean_of(s0, 2, np.float32)
    bad = [(3, 4), (6, 7), (8, 2)]
    for y, x in bad:
        assert (T0[y, x, 0:3].view(np.uint32) == m0[y, x].view(np.uint32)).all() and T0[y, x, 3] == 0 and hist.L[y, x] == 0
    assert (T0[miss][:, 0:3].view(np.uint32) == m0[miss].view(np.uint32)).all() and (T0[miss][:, 3] == 0).all()
    assert T0[5, 5, 3] == 1 and np.isinf(hist.c[5, 5, 2])
    T1, _, d = _acc(s1, f1, hist, dtype=np.float32)
    hit = ~miss
    assert np.isfinite(T1[hit]).all() and (T1[miss][:, 3] == 0).all()  # no tap took a NaN, an Inf or the overflowed history in
    for y, x in bad + [(5, 5)]:  # the four pixels around whose taps each of them is: three taps left, renormalised
        for yy, xx in ((y, x), (y - 1, x), (y, x - 1), (y - 1, x - 1)):
            assert d["taps"][yy, xx].sum() == 3 and d["found"][yy, xx] and T1[yy, xx, 3] == 2


# ---- the camera sequences of the GPU tests, and what the reference alone says about them ------------------------------------------------

def _rot_y(d, deg):
    a = np.radians(deg)
    return np.float64([d[0] * np.cos(a) + d[2] * np.sin(a), d[1], -d[0] * np.sin(a) + d[2] * np.cos(a)])


_base = {}


def _base_pose(scene, w, h):
    """(position, direction, right, proj) of the scene's camera as the scene was made: the sequences move it"""
    if scene.name not in _base:
        fresh = type(scene)(scene.name, DETAIL)
        _base[scene.name] = TR.scene_pose(fresh, w, h)
    return _base[scene.name]


def _poses(scene, kind, w, h, frames=4):
    """[(position, direction)] of a sequence around the scene's own camera.  `footprint`: a pixel's width at the scene's typical
    depth.  A pan exactly along the camera's right axis leaves v on the integers and one of exactly one footprint puts u there, where
    float32 and float64 floor differently: the pans go a little up as well, and the one-pixel pan is 3 % off the grid."""
    pos, fwd, right = _base_pose(scene, w, h)
    up = np.cross(fwd, right)
    proj = scene.camera_matrices(w, h)[1]
    footprint = 2.0 * 7.0 / (float(proj[5]) * h)
    if kind == "still":
        return [(pos, fwd)] * frames
    if kind == "pan1":
        return [(pos + (right * 1.03 + up * 0.21) * (footprint * f), fwd) for f in range(frames)]
    if kind == "subpixel":
        return [(pos + (right * 0.37 + up * 0.29) * (footprint * f), fwd) for f in range(frames)]
    if kind == "turn_dolly":
        return [(pos + fwd * (0.15 * f) + right * (0.05 * f), _rot_y(fwd, 1.3 * f)) for f in range(frames)]
    if kind == "jump":
        there, back = pos * (1.0, 1.0, -1.0), fwd * (-1.0, 1.0, -1.0)  # the scene (around the origin) from its other side
        return [(pos, fwd), (pos, fwd), (there, back), (there, back)]
    if kind == "turn180":
        mid = np.float64([0.0, 1.0, 0.0])  # in the middle of the scene, above its objects: either direction sees some
        return [(mid, fwd), (mid, fwd * (-1.0, 1.0, -1.0)), (mid, fwd)]
    raise KeyError(kind)


SEQUENCES = ("still", "pan1", "subpixel", "turn_dolly", "jump", "turn180")
GPU_CASES = [("67x45", k) for k in SEQUENCES] + [("1x1", "subpixel"), ("1x1", "still"), ("5x3", "subpixel"), ("5x3", "turn_dolly"), ("300x200", "turn_dolly"),
                                                ("300x200", "still")]
EXTENTS = {"67x45": (67, 45), "1x1": (1, 1), "5x3": (5, 3), "300x200": (300, 200)}


def _synthetic_sum(h, w, albedo, seed, samples=1):
    """albedo x a smooth light x noise, with a hot pixel, a NaN and an Inf marker pixel"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    light = np.stack([0.4 + 0.5 * xx / w, 0.3 + 0.6 * yy / h, 0.5 + 0.0 * xx], axis=-1)
    S = np.zeros((h, w, 4), np.float32)
    S[..., 0:3] = albedo[..., 0:3] * light * rng.uniform(0.2, 1.8, (h, w, 3))
    S[(h // 2) % h, (w // 3) % w, 0:3] = 3000.0
    S[2 % h, 3 % w, 0] = np.nan
    S[4 % h, 5 % w, 1] = np.inf
    S[..., 0:3] *= samples
    S[..., 3] = samples
    return S


def _check_against_reference(frames, got, label):
    """frames as temporal_ref.run_sequence takes them, got: the implementation's T per frame (None: the reference alone).  Returns
    (largest |ref32 - ref64| of the case, largest share of valid pixels left out in a frame)."""
    t32, d32 = TR.run_sequence(frames, TD["max_history"], TD["normal_threshold"], TD["position_threshold"], np.float32)
    t64, d64 = TR.run_sequence(frames, TD["max_history"], TD["normal_threshold"], TD["position_threshold"], np.float64)
    keep = TR.comparable_pixels(d32, d64)
    worst, share = 0.0, 0.0
    for k in range(len(frames)):
        valid = d64[k]["valid"]
        fin = keep[k][..., None] & np.isfinite(t64[k]) & np.isfinite(t32[k])
        if fin.any():
            worst = max(worst, float(np.abs(t32[k].astype(np.float64) - t64[k])[fin].max()))
        if valid.any():
            share = max(share, float((valid & ~keep[k]).sum()) / float(valid.sum()))
    if got is None:
        return worst, share
    assert share <= min(LEFT_OUT_CAP, 4 * REFERENCE_LEFT_OUT), (label, share)
    for k, T in enumerate(got):
        valid, b = d64[k]["valid"], t64[k]
        assert T.shape == b.shape and T.dtype == np.float32
        # pixels that are not valid hold the mean and L = 0, bit for bit, whatever class they have
        m = R.mean_of(frames[k][0], frames[k][4], np.float32)
        assert (_bits(T[..., 0:3])[~valid] == _bits(m)[~valid]).all() and (T[..., 3][~valid] == 0).all(), (label, k)
        cmp = keep[k] & valid
        fin = cmp[..., None] & np.isfinite(b)
        assert (np.isfinite(T) == np.isfinite(b))[cmp].all(), (label, k)
        err = np.abs(T.astype(np.float64) - b)[fin]
        tol = np.maximum(8.0 * worst, 2.0 ** -20 * np.maximum(1.0, np.abs(b[fin])))
        if err.size:
            print(f"{label} frame {k}: max |gpu - ref64| {err.max():.3e}, max |ref32 - ref64| of the case {worst:.3e}, left out {int((valid & ~keep[k]).sum())} of "
                  f"{int(valid.sum())} valid pixels, mean L {T[..., 3][valid].mean():.3f}, largest value {np.abs(b[fin]).max():.3e}")
            assert (err <= tol).all(), (label, k, float(err.max()), worst)
    return worst, share


def _cpu_guides(pkg, orc, scene, w, h):
    try:
        return R.cpu_guides(pkg, orc, scene, w, h)
    except KeyError:  # no pixel was hit: the debug view's reference has no position to report
        g = [np.zeros((h, w, 4), np.float32) for _ in range(3)]
        R.set_miss(g, np.ones((h, w), bool))
        return g


def test_reference_gap_and_left_out_share_on_the_cpu_sequences(pkg, orc):
    """What the tolerance and the cap rest on, measured without a GPU: the camera sequences of the GPU tests on first-hit guides from
    the debug view's reference and a synthetic sum.  The steps are chosen so that the reference alone stays inside the cap."""
    scene = pkg.Scene(SCENE, DETAIL)
    worst, share = 0.0, 0.0
    for kind in SEQUENCES:
        frames = []
        for f, (p, d) in enumerate(_poses(scene, kind, W, H)):
            scene.set_camera_pose(p, d)
            g = _cpu_guides(pkg, orc, scene, W, H)
            frames.append((_synthetic_sum(H, W, g[2], 100 + f), *g, 1, *scene.camera_matrices(W, H), 0))
        a, b = _check_against_reference(frames, None, kind)
        L = TR.run_sequence(frames, TD["max_history"], TD["normal_threshold"], TD["position_threshold"], np.float64)[0]
        print(f"{kind}: max |ref32 - ref64| {a:.3e}, left out {b:.5f}; valid pixels per frame {[int((t[..., 3] > 0).sum()) for t in L]}, "
              f"of them restarted {[int((t[..., 3] == 1).sum()) for t in L]}")
        worst, share = max(worst, a), max(share, b)
    assert REFERENCE_GAP / 4 <= worst <= REFERENCE_GAP and REFERENCE_LEFT_OUT / 4 <= share <= REFERENCE_LEFT_OUT and 4 * REFERENCE_LEFT_OUT <= LEFT_OUT_CAP


@pytest.mark.parametrize("name", ["default", "texture_test"])
def test_accumulation_beats_the_frame_and_the_chain_beats_the_spatial_filter(pkg, orc, name):
    """The quality table of docs/NEXT_ROWS.md section 14 (tools/temporal_quality.py): 8 frames of 4 spp of the CPU oracle under a
    camera sliding sideways.  Against the oracle's own 192 spp at the last pose (tests/golden/temporal_truth.npz, other samples) the
    accumulated frame is closer than the raw one, and the accumulated frame filtered at TEMPORAL_DENOISE_DEFAULTS closer than the raw
    frame filtered at DENOISE_DEFAULTS."""
    truth = np.load(os.path.join(util.GOLDEN_DIR, "temporal_truth.npz"))[name].astype(np.float32)
    assert truth.shape == (TR.QUALITY_H, TR.QUALITY_W, 3)
    _, frames = TR.quality_sequence(pkg, orc, name)
    t, dd, cd = pkg.TEMPORAL_DEFAULTS, pkg.DENOISE_DEFAULTS, pkg.TEMPORAL_DENOISE_DEFAULTS
    T = TR.run_sequence(frames, t["max_history"], t["normal_threshold"], t["position_threshold"], np.float32)[0][-1]
    S, nrm, pos, alb, spp = frames[-1][0:5]
    spatial = R.denoise(S, nrm, pos, alb, spp, dd["iterations"], dd["sigma_color"], dd["sigma_normal"], dd["sigma_position"], np.float32)
    chained = R.denoise(T, nrm, pos, alb, 1, cd["iterations"], cd["sigma_color"], cd["sigma_normal"], cd["sigma_position"], np.float32)
    raw_err, tmp_err = R.relative_l2(S[..., 0:3] / spp, truth), R.relative_l2(T, truth)
    spa_err, chn_err = R.relative_l2(spatial, truth), R.relative_l2(chained, truth)
    print(f"{name}: relative L2 error raw {raw_err:.4f}, spatial {spa_err:.4f}, temporal {tmp_err:.4f}, temporal + spatial {chn_err:.4f}")
    assert np.isfinite(T[..., 0:3]).all() and tmp_err < raw_err
    assert np.isfinite(chained).all() and chn_err < spa_err


# =====================================================================================================
# on the GPU
# =====================================================================================================
_state = {}


def _gpu(pkg, name=SCENE):
    """(scene, renderer) of `name`, uploaded once"""
    import torch  # noqa: F401  (first, so the HIP library shares torch's HIP runtime)

    if name not in _state:
        s = pkg.Scene(name, DETAIL)
        r = pkg.Renderer()
        r.upload(s)
        _state[name] = (s, r)
    return _state[name]


def _render_frame(s, r, w, h, pose, f, synthetic=False):
    """One 1-spp frame at `pose`: the device's own sum and guides, read back.  Returns the reference's frame tuple and the uniform."""
    s.set_camera_pose(*pose)
    u = s.uniform(w, h, bounces=4, sample_count=1, total_samples=f)
    r.render_guides(u)
    g = [r.read_guide(k) for k in range(3)]
    if synthetic:
        S = _synthetic_sum(h, w, g[2], 7 + f)
        r.write_accumulation(S)
    else:
        r.reset()
        r.render(u, s.lights)
        S = r.readback()
    view, proj = s.camera_matrices(w, h)
    return (S, *g, 1, view, proj, 0), u


def _accumulate(r, frame, flags=0):
    r.temporal_accumulate(frame[4], frame[5], frame[6], flags=flags, **TD)
    return r.read_temporal()


def _run(pkg, extent, kind, synthetic=False):
    s, r = _gpu(pkg)
    w, h = EXTENTS[extent]
    r.set_tile_shard(0, 1, 32)
    r.resize(w, h)  # drops the history of the case before
    frames, got = [], []
    for f, pose in enumerate(_poses(s, kind, w, h)):
        frame, _ = _render_frame(s, r, w, h, pose, f, synthetic)
        frames.append(frame)
        got.append(_accumulate(r, frame))
        assert (_bits(r.readback()) == _bits(frame[0])).all()  # the sum is an input
        for k in range(3):
            assert (_bits(r.read_guide(k)) == _bits(frame[1 + k])).all()  # ... and so are the guides
    return frames, got


@pytest.mark.gpu
@pytest.mark.parametrize("case", GPU_CASES, ids=lambda c: "%s-%s" % c)
def test_accumulation_against_float64_reference(pkg, case):
    extent, kind = case
    frames, got = _run(pkg, extent, kind)
    _check_against_reference(frames, got, "%s %s" % case)
    L = [T[..., 3] for T in got]
    valid = [R.valid_mask(f[0], f[1], f[2], 1, np.float32) for f in frames]
    if extent in ("67x45", "300x200"):
        assert all(v.sum() > 200 and (~v).sum() > 20 for v in valid[:1]), "the frame must have accumulated and passed-through pixels"
        assert (L[0][valid[0]] == 1).all()
    if kind == "still":  # the same-camera variant: L = k up to the cap, nothing restarts
        for k in range(len(L)):
            both = valid[k] & valid[0]
            assert (L[k][both] == min(k + 1.0, TD["max_history"])).all(), k
    if kind in ("pan1", "subpixel", "turn_dolly") and extent in ("67x45", "300x200"):
        assert (L[1][valid[1]] > 1).mean() > 0.5 and (L[-1][valid[-1]] > 2).mean() > 0.5  # the history is found on most of the frame
    if kind == "turn_dolly" and extent == "300x200":  # four live taps: lengths between the integers
        frac = L[2][valid[2]]
        assert ((frac > 2.01) & (frac < 2.99)).any()
    if kind == "jump":
        assert (L[1][valid[1]] == 2).all() and (L[2][valid[2]] == 1).mean() > 0.5 and (L[3][valid[3]] >= 2).all() and valid[2].sum() > 200
    if kind == "turn180":  # what the camera sees after turning back lies behind the camera of the frame before
        assert (L[2][valid[2]] == 1).all() and valid[2].sum() > 200


@pytest.mark.gpu
def test_synthetic_frames_with_markers_and_a_hot_pixel(pkg):
    frames, got = _run(pkg, "67x45", "subpixel", synthetic=True)
    _check_against_reference(frames, got, "synthetic subpixel")
    for T in got:
        assert np.isnan(T[2, 3, 0]) and np.isposinf(T[4, 5, 1]) and T[2, 3, 3] == 0 and T[4, 5, 3] == 0
        rest = np.ones((H, W), bool)
        rest[2, 3] = rest[4, 5] = False
        assert np.isfinite(T[rest]).all()  # the markers keep to themselves


@pytest.mark.gpu
def test_moved_geometry_restarts_and_the_background_keeps_its_length(pkg):
    s, r = _gpu(pkg, "animated_test")
    r.resize(W, H)
    pose = _base_pose(s, W, H)[0:2]
    f0, _ = _render_frame(s, r, W, H, pose, 0)
    got = [_accumulate(r, f0)]
    assert s.update(0.37)
    r.update_animation(*s.animation_state())
    f1, _ = _render_frame(s, r, W, H, pose, 1)
    got.append(_accumulate(r, f1))
    _check_against_reference([f0, f1], got, "animated_test")
    valid = R.valid_mask(f1[0], f1[1], f1[2], 1, np.float32) & R.valid_mask(f0[0], f0[1], f0[2], 1, np.float32)
    unmoved = valid & (_bits(f0[1]) == _bits(f1[1])).all(axis=-1) & (_bits(f0[2]) == _bits(f1[2])).all(axis=-1)
    shift = np.abs(((f1[2][..., 0:3].astype(np.float64) - f0[2][..., 0:3]) * f1[1][..., 0:3]).sum(axis=-1))
    moved = valid & (shift > 2 * TD["position_threshold"] * f1[2][..., 3])
    print(f"animated_test: {int(unmoved.sum())} pixels with the same guides, {int(moved.sum())} moved along their normal")
    assert unmoved.sum() > 200 and moved.sum() > 20
    assert (got[1][..., 3][unmoved] == 2).all() and (got[1][..., 3][moved] == 1).all()


def _borrower(pkg, owner, w, h):
    b = pkg.Renderer()
    b.share_scene(owner)
    b.resize(w, h)
    return b


def _replay(b, frames, flags=None):
    """The frames' own sums and uniforms on another handle"""
    out = []
    for k, (frame, u) in enumerate(frames):
        b.write_accumulation(frame[0])
        b.render_guides(u)
        out.append(_accumulate(b, frame, flags[k] if flags else 0))
    return out


@pytest.mark.gpu
def test_borrower_reset_and_resize(pkg):
    """A borrower computes what its owner does; two sequences on one handle separated by RESET are two fresh handles; ptx_resize
    drops T and the history."""
    s, r = _gpu(pkg)
    r.set_tile_shard(0, 1, 32)
    r.resize(W, H)
    poses = _poses(s, "turn_dolly", W, H)
    frames = [_render_frame(s, r, W, H, p, f) for f, p in enumerate(poses)]
    own = _replay(r, frames[0:2] + frames[2:4], flags=[0, 0, pkg.TEMPORAL_RESET, 0])
    assert r.temporal_ptr()
    for seq, want in ((frames[0:2], own[0:2]), (frames[2:4], own[2:4])):
        b = _borrower(pkg, r, W, H)
        for a, c in zip(_replay(b, seq), want):
            assert (_bits(a) == _bits(c)).all()
        b.close()
    assert (own[2][..., 3] <= 1).all() and (own[3][..., 3] > 1).any()
    # RESET on a still camera as well: the same-camera variant is not taken without a history
    still = _replay(r, [frames[3], frames[3]], flags=[0, pkg.TEMPORAL_RESET])
    assert (still[0][..., 3] > 1).any() and (still[1][..., 3] <= 1).all()
    # ptx_resize
    lib, buf = r.lib, np.zeros((H, W, 4), np.float32)
    r.resize(W, H)
    dd = pkg.DenoiseDesc(1, 2, 0.0, 0.3, 0.03, 0, 0)
    assert not r.temporal_ptr() and lib.ptx_read_temporal(r.handle, buf.ctypes.data, buf.nbytes) == 5 and not buf.any()
    assert lib.ptx_denoise_temporal(r.handle, C.byref(dd)) == 5
    again = _replay(r, frames[3:4])  # no history survived: a first frame
    assert (again[0][..., 3] <= 1).all() and (_bits(again[0]) == _bits(still[1])).all()


@pytest.mark.gpu
def test_denoise_temporal_is_denoise_on_a_copy_of_t_and_the_output_stage_follows(pkg):
    s, r = _gpu(pkg)
    r.set_tile_shard(0, 1, 32)
    r.resize(W, H)
    poses = _poses(s, "subpixel", W, H)
    frames = [_render_frame(s, r, W, H, p, f, synthetic=True) for f, p in enumerate(poses[0:3])]
    T = _replay(r, frames)[-1]
    S, u = frames[-1][0][0], frames[-1][1]
    f = _borrower(pkg, r, W, H)
    f.write_accumulation(T)
    f.render_guides(u)
    for params in ((3, 0.5, 0.3, 0.03), (2, 0.0, 0.3, 0.05), (1, 1.5, 0.5, 0.02)):
        r.denoise_temporal(*params)
        f.denoise(1, *params)
        D = r.read_denoised()
        assert (_bits(D) == _bits(f.read_denoised())).all(), params
        assert (D[..., 3] == 1).all()
    assert (_bits(r.read_temporal()) == _bits(T)).all() and (_bits(r.readback()) == _bits(S)).all()  # T and the sum are inputs
    assert (_bits(D) != _bits(T))[..., 0:3].any(axis=-1).sum() > 200
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
    out = r.read_output(pkg.OUTPUT_RGBA32F)
    assert out[2, 3, 0] >= 1 and out[4, 5, 1] >= 1  # the NaN / Inf pixels still get postprocess.comp's markers
    # the plain filter still reads the sum: ptx_denoise did not change
    r.denoise(1, 3, 0.5, 0.3, 0.03)
    f.write_accumulation(S)
    f.denoise(1, 3, 0.5, 0.3, 0.03)
    assert (_bits(r.read_denoised()) == _bits(f.read_denoised())).all()
    f.close()
    g.close()


@pytest.mark.gpu
def test_the_path_tracer_does_not_notice(pkg):
    s, r = _gpu(pkg)
    r.set_tile_shard(0, 1, 32)
    r.resize(W, H)
    pose = _base_pose(s, W, H)[0:2]
    s.set_camera_pose(*pose)
    up = s.uniform(W, H, bounces=4)

    def path_traced(frames):
        r.reset()
        for f in range(frames):
            up.TotalSamples = f
            r.render(up, s.lights)
        return r.readback()
    two, three = path_traced(2), path_traced(3)
    assert (_bits(path_traced(2)) == _bits(two)).all()
    r.render_guides(up)
    view, proj = s.camera_matrices(W, H)
    r.temporal_accumulate(2, view, proj, **TD)
    r.temporal_accumulate(2, view, proj, **TD)
    r.denoise_temporal()
    assert (_bits(r.readback()) == _bits(two)).all()
    up.TotalSamples = 2
    r.render(up, s.lights)  # the next ptx_render continues the sum as if nothing had happened
    assert (_bits(r.readback()) == _bits(three)).all()


@pytest.mark.gpu
def test_refusals_leave_t_and_the_history_intact(pkg):
    import torch

    s, r = _gpu(pkg)
    r.set_tile_shard(0, 1, 32)
    r.resize(W, H)
    lib = r.lib
    poses = _poses(s, "subpixel", W, H)
    frames = [_render_frame(s, r, W, H, p, f) for f, p in enumerate(poses[0:3])]
    T = _replay(r, frames[0:2])[-1]
    view, proj = frames[2][0][5], frames[2][0][6]

    def desc(total=1, mh=3.0, nt=0.3, pt=0.03, flags=0, reserved=0):
        d = pkg.TemporalDesc()
        d.View[:], d.Proj[:] = [float(v) for v in view], [float(v) for v in proj]
        d.totalSamples, d.maxHistory, d.normalThreshold, d.positionThreshold, d.flags, d.reserved = total, mh, nt, pt, flags, reserved
        return d

    def intact():
        assert (_bits(r.read_temporal()) == _bits(T)).all()

    nan, inf = float("nan"), float("inf")
    bad = [desc(total=0), desc(mh=0.5), desc(mh=0.0), desc(mh=-1.0), desc(mh=nan), desc(mh=inf), desc(nt=0.0), desc(nt=-0.3), desc(nt=nan), desc(nt=inf),
           desc(pt=0.0), desc(pt=-0.03), desc(pt=nan), desc(pt=inf), desc(flags=2), desc(flags=3), desc(flags=0x80000000), desc(reserved=1)]
    for d in bad:
        assert lib.ptx_temporal_accumulate(r.handle, C.byref(d)) == 1, (d.totalSamples, d.maxHistory, d.normalThreshold, d.positionThreshold, d.flags, d.reserved)
    assert lib.ptx_temporal_accumulate(r.handle, None) == 1 and lib.ptx_denoise_temporal(r.handle, None) == 1
    buf = np.zeros((H, W, 4), np.float32)
    assert lib.ptx_read_temporal(r.handle, None, buf.nbytes) == 1
    assert lib.ptx_read_temporal(r.handle, buf.ctypes.data, buf.nbytes + 16) == 1 and lib.ptx_read_temporal(r.handle, buf.ctypes.data, buf.nbytes - 16) == 1
    assert not buf.any()
    dd = lambda **kw: pkg.DenoiseDesc(**{**dict(totalSamples=1, iterations=2, sigmaColor=0.0, sigmaNormal=0.3, sigmaPosition=0.03, flags=0, reserved=0), **kw})  # noqa: E731
    for d in (dd(iterations=0), dd(iterations=7), dd(sigmaColor=-1.0), dd(sigmaNormal=0.0), dd(sigmaPosition=nan), dd(flags=1), dd(reserved=1)):
        assert lib.ptx_denoise_temporal(r.handle, C.byref(d)) == 1
    intact()
    # a tile shard of a larger world, a bound shard accumulation buffer
    r.set_tile_shard(0, 2, 8)
    assert lib.ptx_temporal_accumulate(r.handle, C.byref(desc())) == 5 and lib.ptx_denoise_temporal(r.handle, C.byref(dd())) == 5
    shard = torch.zeros(r.shard_bytes(0) // 4, dtype=torch.float32, device="cuda")
    r.bind_shard_accumulation(shard.data_ptr(), r.shard_bytes(0))
    assert lib.ptx_temporal_accumulate(r.handle, C.byref(desc())) == 5 and lib.ptx_denoise_temporal(r.handle, C.byref(dd())) == 5
    r.bind_shard_accumulation(0)
    assert lib.ptx_temporal_accumulate(r.handle, C.byref(desc())) == 5
    r.set_tile_shard(0, 1, 32)
    intact()
    # no image; an image without guides; guides without an accumulate
    fresh = pkg.Renderer()
    assert lib.ptx_temporal_accumulate(fresh.handle, C.byref(desc())) == 5
    fresh.share_scene(r)
    fresh.resize(W, H)
    assert lib.ptx_temporal_accumulate(fresh.handle, C.byref(desc())) == 5
    fresh.render_guides(frames[2][1])
    assert lib.ptx_read_temporal(fresh.handle, buf.ctypes.data, buf.nbytes) == 5 and not lib.ptx_device_temporal_ptr(fresh.handle)
    assert lib.ptx_denoise_temporal(fresh.handle, C.byref(dd())) == 5
    fresh.close()
    # the history is intact as well: the third frame gives what a handle that never saw a refusal gives
    third = _replay(r, frames[2:3])[0]
    b = _borrower(pkg, r, W, H)
    assert (_bits(_replay(b, frames)[-1]) == _bits(third)).all() and (third[..., 3] > 2).any()
    b.close()
    assert lib.ptx_denoise_temporal(r.handle, C.byref(dd(totalSamples=0))) == 0  # the desc's count is ignored: T is a mean
