"""Motion guides (include/ptx.h ptx_track_motion, ptx_render_guides_motion, ptx_temporal_accumulate_motion; docs/NEXT_ROWS.md
section 17): the pose bookkeeping, the two motion images against the float64 reference of tests/motion_ref.py, the identities that
hold bit for bit, the accumulation through the motion guides against its reference, and everything that must not notice.
"""
import os
import re

import numpy as np
import pytest

import debug_view_ref as DV
import denoise_ref as R
import motion_ref as M
import temporal_ref as TR
import test_skinning as SK  # skin_lab, its poses and the vertex-count labs
import test_temporal as TT  # the plane frames, the camera sequences and the synthetic sum
import util

W, H = 67, 45
DETAIL = 0.25
TD = dict(max_history=3.0, normal_threshold=0.3, position_threshold=0.03)
PX = TT.PX
LEFT_OUT_CAP = 0.02
# what tests/motion_ref.py alone says about the sequences of the GPU tests (test_reference_gap_and_left_out_share_on_the_cpu_sequences):
# the largest |float32 - float64| of T, and the largest share of valid pixels on which the two precisions decide a tap differently
REFERENCE_GAP = 2.0e-3  # measured 1.31e-3 (animated_test under the sub-pixel pan: the synthetic sum's hot pixel over the albedo floor)
REFERENCE_LEFT_OUT = 0.0  # measured 0: on these poses the two precisions decide every tap alike, so the GPU test leaves nothing out
ANIMATION_STEPS = (0.37, 0.37)  # Scene.update between the three poses of animated_test


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _known(img):
    return img[..., 3] == 1


# =====================================================================================================
# without a GPU
# =====================================================================================================

def test_header_declares_and_package_exports_the_motion_guides(pkg):
    header = open(os.path.join(pkg.REPO_DIR, "include", "ptx.h")).read()
    capi = open(os.path.join(pkg.PKG_DIR, "csrc", "ptx_capi.hip")).read()
    assert "#define PTX_ABI_VERSION 5u" in header and re.search(r"PTX_FN_COUNT = 38\b", header) and pkg.ABI_VERSION == 5
    for decl in ("PTX_API int ptx_track_motion(PtxRenderer *r, int enable);",
                 "PTX_API int ptx_render_guides_motion(PtxRenderer *r, const PtxRaygenUniformData *uniform);",
                 "PTX_API int ptx_read_motion(PtxRenderer *r, uint32_t which, void *host, size_t bytes);",
                 "PTX_API void *ptx_device_motion_ptr(PtxRenderer *r, uint32_t which);",
                 "PTX_API int ptx_temporal_accumulate_motion(PtxRenderer *r, const PtxTemporalDesc *desc, uint32_t withMoments);"):
        assert decl in header, decl
        name = re.search(r"(ptx_\w+)\(", decl).group(1)
        assert name in pkg.PTX_SYMBOLS and re.search(r"^(int |void \*)%s\(" % name, capi, re.M), name
    assert re.search(r"PTX_MOTION_POSITION = 0,.*\n\s*PTX_MOTION_NORMAL = 1,.*\n\s*PTX_MOTION_COUNT = 2", header)
    assert (pkg.MOTION_POSITION, pkg.MOTION_NORMAL) == (0, 1)
    for method in ("track_motion", "render_guides_motion", "read_motion", "motion_ptr", "temporal_accumulate_motion"):
        assert callable(getattr(pkg.Renderer, method))
    # the host adapter: off by default, and on it calls the two new functions in the plain pair's place
    host_h = open(os.path.join(pkg.PKG_DIR, "host", "RendererHip.h")).read()
    host_cpp = open(os.path.join(pkg.PKG_DIR, "host", "RendererHip.cpp")).read()
    assert re.search(r"struct TemporalSettings\s*\{\s*bool Enabled = false;[^}]*bool MotionVectors = false;", host_h)
    for call in ("ptx_track_motion(s_Renderer", "ptx_render_guides_motion(s_Renderer", "ptx_temporal_accumulate_motion(s_Renderer"):
        assert call in host_cpp, call
    # the rules the reference is written from
    for phrase in ("h == S - 1 and the snapshot is valid", "never through the triangle's place in", "x~ bit-equal to", "takes no history"):
        assert phrase in header, phrase


def _acc(S, frame, xprev, nprev, hist, dtype=np.float64, samples=2, **over):
    g, view, proj = frame
    p = dict(max_history=32.0, normal_threshold=0.3, position_threshold=0.03)
    p.update(over)
    return M.accumulate_motion(S, *g, xprev, nprev, samples, view, proj, hist, p["max_history"], p["normal_threshold"], p["position_threshold"], 0, dtype)


def _known_images(g, dx=(0.0, 0.0, 0.0), normal=None):
    """(X_prev, N_prev) with w = 1: the position guide moved by dx and the normal guide (or `normal`)"""
    x, n = g[1].copy(), g[0].copy()
    x[..., 0:3] += np.float32(dx)
    x[..., 3] = 1.0
    if normal is not None:
        n[..., 0:3] = np.float32(normal)
    return x, n


def test_translated_quad_shifts_its_history_by_the_known_offset():
    """A plane sliding in itself under a still camera: the point pixel x shows was at pixel x + 1"""
    h, w = 6, 11
    s0, s1 = TT._noise_sum(h, w, 1), TT._noise_sum(h, w, 2)
    frame = TT._plane_frame(h, w)
    T0, hist, _ = _acc(s0, frame, *_known_images(frame[0]), None)
    T1, _, d = _acc(s1, frame, *_known_images(frame[0], dx=(-PX, 0.0, 0.0)), hist)
    assert not d["at_pixel"].any()
    c1 = s1[..., 0:3].astype(np.float64) / 2
    assert np.abs(T1[:, :-1, 0:3] - (T0[:, 1:, 0:3] + c1[:, :-1]) / 2).max() <= 2e-4 and np.abs(T1[:, :-1, 3] - 2).max() <= 2e-4
    assert (T1[:, -1, 3] == 1).all() and (T1[:, -1, 0:3] == c1[:, -1]).all()  # its previous place lies outside the image
    # the plain call sees the same guides in both frames: it takes the history of pixel x itself
    P1 = TR.accumulate(s1, *frame[0], 2, frame[1], frame[2], hist, 32.0, 0.3, 0.03)[0]
    assert np.abs(P1[..., 0:3] - (T0[..., 0:3] + c1) / 2).max() <= 1e-12


def test_quad_rotated_about_its_own_normal_keeps_its_length():
    h, w = 16, 16
    frame = TT._plane_frame(h, w)
    g = frame[0]
    centre = g[1][h // 2, w // 2, 0:3].astype(np.float64)
    a = 0.2
    rot = np.float64([[np.cos(a), np.sin(a), 0], [-np.sin(a), np.cos(a), 0], [0, 0, 1]])
    x = g[1].copy()
    x[..., 0:3] = ((g[1][..., 0:3].astype(np.float64) - centre) @ rot.T + centre).astype(np.float32)
    x[..., 3] = 1.0
    _, hist, _ = _acc(TT._noise_sum(h, w, 1), frame, *_known_images(g), None)
    T1, _, d = _acc(TT._noise_sum(h, w, 2), frame, x, _known_images(g)[1], hist)
    inner = np.zeros((h, w), bool)
    inner[5:11, 5:11] = True
    assert d["found"][inner].all() and np.abs(T1[..., 3][inner] - 2).max() <= 1e-9
    assert d["at_pixel"].sum() <= 1  # the centre alone may stay where it was


def test_tilt_beyond_the_normal_threshold_keeps_its_length_with_n_prev_and_restarts_without():
    """The quad tilts by 0.5 rad in one frame, |n1 - n0| = 0.49 > 0.3: looked up with the PREVIOUS normal the history is found, with
    the current normal in its place it is not.  This is the point of N_prev."""
    h, w = 8, 10
    f0 = TT._plane_frame(h, w)
    a = 0.5
    rot = np.float64([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    g1 = [x.copy() for x in f0[0]]
    g1[0][..., 0:3] = (rot @ np.float64([0, 0, 1])).astype(np.float32)
    g1[1][..., 0:3] = (f0[0][1][..., 0:3].astype(np.float64) @ rot.T).astype(np.float32)
    f1 = (g1, f0[1], f0[2])
    _, hist, _ = _acc(TT._noise_sum(h, w, 1), f0, *_known_images(f0[0]), None)
    xprev, nprev = _known_images(f0[0])  # where the points were, and how they faced
    T, _, d = _acc(TT._noise_sum(h, w, 2), f1, xprev, nprev, hist)
    moved = (_bits(g1[1][..., 0:3]) != _bits(f0[0][1][..., 0:3])).any(axis=-1)
    assert moved.sum() >= h * w - w and d["found"].all() and np.abs(T[..., 3] - 2).max() <= 1e-9
    T, _, d = _acc(TT._noise_sum(h, w, 2), f1, xprev, _known_images(g1)[1], hist)  # n_p in the place of N_prev
    assert not d["found"].any() and (T[..., 3] == 1).all()


def test_unknown_motion_restarts():
    h, w = 5, 7
    frame = TT._plane_frame(h, w)
    s1 = TT._noise_sum(h, w, 2)
    _, hist, _ = _acc(TT._noise_sum(h, w, 1), frame, *_known_images(frame[0]), None)
    x, n = _known_images(frame[0])
    x[..., 3] = n[..., 3] = 0.0
    x[1, 2, 3] = n[1, 2, 3] = 1.0
    T, nxt, d = _acc(s1, frame, x, n, hist)
    one = np.zeros((h, w), bool)
    one[1, 2] = True
    assert (T[..., 3][~one] == 1).all() and T[1, 2, 3] == 2 and (d["found"] == one).all()
    assert (T[..., 0:3][~one] == (s1[..., 0:3].astype(np.float64) / 2)[~one]).all()
    assert (nxt.x == frame[0][1][..., 0:3]).all()  # what is stored is the current position


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("pan", [0.0, 0.5])
def test_static_scene_is_the_plain_reference_exactly(dtype, pan):
    h, w = 6, 9
    f0, f1 = TT._plane_frame(h, w), TT._plane_frame(h, w, pan)
    s0, s1 = TT._noise_sum(h, w, 1), TT._noise_sum(h, w, 2)
    _, hm, _ = _acc(s0, f0, *_known_images(f0[0]), None, dtype=dtype)
    _, hp, _ = TR.accumulate(s0, *f0[0], 2, f0[1], f0[2], None, 32.0, 0.3, 0.03, 0, dtype)
    Tm, nm, dm = _acc(s1, f1, *_known_images(f1[0]), hm, dtype=dtype)
    Tp, npl, dp = TR.accumulate(s1, *f1[0], 2, f1[1], f1[2], hp, 32.0, 0.3, 0.03, 0, dtype)
    assert dp["same_camera"] == (pan == 0.0) and dm["at_pixel"].all() == (pan == 0.0)
    assert Tm.dtype == np.dtype(dtype) and Tm.tobytes() == Tp.tobytes()
    assert nm.c.tobytes() == npl.c.tobytes() and nm.L.tobytes() == npl.L.tobytes() and (dm["found"] == dp["found"]).all()


def test_revealed_background_restarts():
    """An object one unit in front of the plane leaves: the pixels it covered show the background, whose own previous place holds the
    object's history"""
    h, w = 8, 12
    part = np.zeros((h, w), bool)
    part[2:5, 3:9] = True
    f0 = TT._plane_frame(h, w)
    g0 = [x.copy() for x in f0[0]]
    g0[1][part, 2] -= 1.0
    f1 = TT._plane_frame(h, w)
    _, hist, _ = _acc(TT._noise_sum(h, w, 1), (g0, f0[1], f0[2]), *_known_images(g0), None)
    T, _, d = _acc(TT._noise_sum(h, w, 2), f1, *_known_images(f1[0]), hist)
    assert (T[..., 3][part] == 1).all() and (T[..., 3][~part] == 2).all() and (d["found"] == ~part).all()


# ---- the scenes of the GPU tests, as the reference reads them -----------------------------------------------------------------------

class _Animated:
    """animated_test at its three poses: the scene object, and per pose the instance transforms and bones"""

    def __init__(self, pkg):
        self.scene = pkg.Scene("animated_test", DETAIL)
        self.states = [self.scene.animation_state()]
        for step in ANIMATION_STEPS:
            assert self.scene.update(step)
            self.states.append(self.scene.animation_state())
        self.desc = self.scene.desc

    def camera(self, w, h, kind="still"):
        """[(uniform, view, proj)] per pose"""
        out = []
        for p, d in TT._poses(self.scene, kind, w, h, frames=len(self.states)):
            self.scene.set_camera_pose(p, d)
            out.append((self.scene.uniform(w, h), *self.scene.camera_matrices(w, h)))
        return out


class _Soup:
    """A scene from arrays (skin_lab, the vertex-count labs, the quads) and its poses"""

    def __init__(self, pkg, soup, states):
        self.soup, self.desc, self.states = soup, soup.desc, states
        self.cam = pkg.Scene("default", DETAIL)

    def camera(self, w, h, kind="still"):
        self.cam.set_camera_pose((0.0, 9.0, 20.0), (0.0, -0.25, -1.0))
        one = (self.cam.uniform(w, h), *self.cam.camera_matrices(w, h))
        return [one] * len(self.states)


def _quads():
    """A floor and a wall of quads: every leaf that holds a pair has hits on its second triangle"""
    out = []
    for j in range(3):
        for i in range(4):
            x, y = -4.0 + 2.0 * i, 1.0 + 2.0 * j
            out.append(util.quad_mesh([(x, y, 0.0), (x + 1.9, y, 0.0), (x + 1.9, y + 1.9, 0.3), (x, y + 1.9, 0.3)], np.cross((1.9, 0, 0), (0, 1.9, 0.3)) / np.linalg.norm(np.cross((1.9, 0, 0), (0, 1.9, 0.3)))))
    return out


def _move(transform, angle, shift):
    m = np.float64(transform).reshape(3, 4)
    return SK._affine(SK._rotation((0.2, 1.0, 0.1), angle) @ m[:, :3], m[:, 3] + np.float64(shift)).reshape(12)


_cases = {}


def _case(pkg, name):
    if name in _cases:
        return _cases[name]
    if name == "animated_test":
        c = _Animated(pkg)
    elif name == "skin_lab":
        lab = SK.skin_lab(pkg)
        c = _Soup(pkg, lab, [(SK.pose_instances(lab, p), SK.pose_bones(p)) for p in SK.POSES])
    elif name.startswith("count"):
        lab = SK.count_lab(pkg, int(name[5:]))
        it = lab.instances["Transform"].copy()
        c = _Soup(pkg, lab, [(it, SK.pose_bones(0)), (np.stack([it[0], _move(it[1], 0.2, (0.3, 0.1, -0.2))]), SK.pose_bones(1))])
    elif name == "quads":
        floor = util.quad_mesh([(-16, -1, -16), (-16, -1, 16), (16, -1, 16), (16, -1, -16)], (0, 1, 0))
        soup = util.TriangleSoup(pkg, [[floor], _quads()], material=util.mr_material(color=(0.7, 0.6, 0.5)))
        it = soup.instances["Transform"].copy()
        c = _Soup(pkg, soup, [(it, None), (np.stack([it[0], _move(it[1], 0.15, (0.4, 0.2, 0.5))]), None),
                              (np.stack([it[0], _move(it[1], 0.3, (0.9, 0.1, 0.8))]), None)])
    else:  # a scene of the package whose instances the test moves itself (texture_test, alpha_test: kernel modes 1 and 2)
        c = _Soup(pkg, pkg.Scene(name, DETAIL), None)
        it = c.soup.animation_state()[0]
        moved = it.copy()
        for i in range(len(moved)):
            moved[i] = _move(it[i], 0.05 * (i % 3), (0.11 * ((i % 4) - 1.5), 0.0, 0.07 * ((i % 3) - 1)))
        c.states = [(it, None), (moved, None)]
        c.cam = c.soup
        c.camera = lambda w, h, kind="still", c=c: [(c.soup.uniform(w, h), *c.soup.camera_matrices(w, h))] * 2
    _cases[name] = c
    return c


_refs = {}


def _ref_pose(orc, c, name, k, dtype):
    """(RefScene, skinned block in dtype) of pose k"""
    if (name, k) not in _refs:
        it, bn = c.states[k]
        _refs[(name, k)] = DV.RefScene(orc, c.desc, it, bn if bn is not None and len(bn) else None)
    rs = _refs[(name, k)]
    bn = c.states[k][1]
    return rs, M.skinned_block(rs, bn, dtype)


def _ref_motion(orc, c, name, k, prev, uniform, w, h, dtype):
    key = ("motion", name, k, prev, w, h, np.dtype(dtype).name, bytes(uniform))
    if key not in _refs:
        cur = _ref_pose(orc, c, name, k, dtype)
        was = _ref_pose(orc, c, name, prev, dtype) if prev is not None else (None, None)
        _refs[key] = M.motion_guides(*cur, *was, uniform, w, h, dtype)
    return _refs[key]


def _check_chain(frames, got, label):
    """test_temporal._check_against_reference for chains through the motion guides; frames as motion_ref.run_sequence takes them"""
    t32, d32 = M.run_sequence(frames, TD["max_history"], TD["normal_threshold"], TD["position_threshold"], np.float32)
    t64, d64 = M.run_sequence(frames, TD["max_history"], TD["normal_threshold"], TD["position_threshold"], np.float64)
    keep = M.comparable_pixels(d32, d64)
    worst, share = 0.0, 0.0
    for k in range(len(frames)):
        valid = d64[k]["valid"]
        fin = keep[k][..., None] & np.isfinite(t64[k]) & np.isfinite(t32[k])
        if fin.any():
            worst = max(worst, float(np.abs(t32[k].astype(np.float64) - t64[k])[fin].max()))
        if valid.any():
            share = max(share, float((valid & ~keep[k]).sum()) / float(valid.sum()))
    if got is None:
        return worst, share, t64
    assert share <= min(LEFT_OUT_CAP, 4 * REFERENCE_LEFT_OUT), (label, share)
    for k, T in enumerate(got):
        valid, b = d64[k]["valid"], t64[k]
        assert T.shape == b.shape and T.dtype == np.float32
        m = R.mean_of(frames[k][0], frames[k][6], np.float32)
        assert (_bits(T[..., 0:3])[~valid] == _bits(m)[~valid]).all() and (T[..., 3][~valid] == 0).all(), (label, k)
        cmp = keep[k] & valid
        fin = cmp[..., None] & np.isfinite(b)
        assert (np.isfinite(T) == np.isfinite(b))[cmp].all(), (label, k)
        err = np.abs(T.astype(np.float64) - b)[fin]
        tol = np.maximum(8.0 * worst, 2.0 ** -20 * np.maximum(1.0, np.abs(b[fin])))
        if err.size:
            print(f"{label} frame {k}: max |gpu - ref64| {err.max():.3e}, max |ref32 - ref64| of the case {worst:.3e}, left out "
                  f"{int((valid & ~keep[k]).sum())} of {int(valid.sum())} valid pixels, mean L {T[..., 3][valid].mean():.3f}")
            assert (err <= tol).all(), (label, k, float(err.max()), worst)
    return worst, share, t64


CHAINS = [("animated_test", "still", (W, H)), ("animated_test", "subpixel", (W, H)), ("skin_lab", "still", (W, H)),
          ("animated_test", "subpixel", (1, 1)), ("animated_test", "subpixel", (5, 3))]


def test_reference_gap_and_left_out_share_on_the_cpu_sequences(pkg, orc):
    """What the accumulation's tolerance and cap rest on, measured without a GPU: the sequences of the GPU test on the reference's
    own guides (float32) and a synthetic sum.  The poses are chosen so that the reference alone stays inside the cap."""
    worst, share = 0.0, 0.0
    for name, kind, (w, h) in CHAINS:
        c = _case(pkg, name)
        cams = c.camera(w, h, kind)
        frames = []
        for k, (u, view, proj) in enumerate(cams):
            n, x, xp, npv = _ref_motion(orc, c, name, k, k - 1 if k else None, u, w, h, np.float32)
            alb = np.ones((h, w, 4), np.float32)
            alb[..., 0:3] = (0.8, 0.5, 0.3)
            R.set_miss([n, x, alb], n[..., 3] != 1)
            frames.append((TT._synthetic_sum(h, w, alb, 100 + k), n, x, alb, xp, npv, 1, view, proj, 0))
        a, b, t64 = _check_chain(frames, None, name)
        L = [t[..., 3] for t in t64]
        print(f"{name} {kind}: max |ref32 - ref64| {a:.3e}, left out {b:.5f}; valid {[int((x > 0).sum()) for x in L]}, restarted {[int((x == 1).sum()) for x in L]}")
        assert w * h < 100 or ((L[1] > 1.5).sum() > 0.5 * (L[1] > 0).sum()), "most of the frame keeps its history"
        worst, share = max(worst, a), max(share, b)
    assert REFERENCE_GAP / 4 <= worst <= REFERENCE_GAP and REFERENCE_LEFT_OUT / 4 <= share <= REFERENCE_LEFT_OUT and 4 * REFERENCE_LEFT_OUT <= LEFT_OUT_CAP


QUALITY_SPP, QUALITY_TRUTH_SPP, QUALITY_BOUNCES = 2, 96, 4


def test_animated_geometry_is_closer_to_the_truth_through_the_motion_guides(pkg, orc):
    """The quality table of docs/NEXT_ROWS.md section 17: animated_test at its three poses under a still camera, 2 spp per frame from
    the CPU oracle, no demodulation (albedo 1).  On the pixels test_temporal's moved-geometry test calls moved, the chain through the
    motion guides ends closer to the oracle's own 96 spp of the last pose (other samples) than the plain chain, which restarts
    there; and it carries a history on them."""
    c = _case(pkg, "animated_test")
    cams = c.camera(W, H)
    lights = c.scene.lights
    plain, motion, sums = [], [], []
    for k, (u, view, proj) in enumerate(cams):
        it, bn = c.states[k]
        osc = orc.OracleScene(c.desc, build_bvh=True, instance_transforms=it, bones=bn if len(bn) else None)
        S = np.zeros((H, W, 4), np.float32)
        for f in range(QUALITY_SPP):
            osc.render(c.scene.uniform(W, H, bounces=QUALITY_BOUNCES, sample_count=1, total_samples=k * QUALITY_SPP + f), lights, W, H, accum=S)
        if k == len(cams) - 1:
            truth = np.zeros((H, W, 4), np.float32)
            for f in range(QUALITY_TRUTH_SPP):
                osc.render(c.scene.uniform(W, H, bounces=QUALITY_BOUNCES, sample_count=1, total_samples=1000 + f), lights, W, H, accum=truth)
        osc.close()
        n, x, xp, npv = _ref_motion(orc, c, "animated_test", k, k - 1 if k else None, u, W, H, np.float32)
        alb = np.ones((H, W, 4), np.float32)
        R.set_miss([n, x, alb], n[..., 3] != 1)
        sums.append(S)
        plain.append((S, n, x, alb, QUALITY_SPP, view, proj, 0))
        motion.append((S, n, x, alb, xp, npv, QUALITY_SPP, view, proj, 0))
    t = pkg.TEMPORAL_DEFAULTS
    Tp = TR.run_sequence(plain, t["max_history"], t["normal_threshold"], t["position_threshold"], np.float32)[0][-1]
    Tm = M.run_sequence(motion, t["max_history"], t["normal_threshold"], t["position_threshold"], np.float32)[0][-1]
    (n0, x0), (n1, x1) = plain[-2][1:3], plain[-1][1:3]
    valid = (Tp[..., 3] > 0) & (n0[..., 3] == 1)
    shift = np.abs(((x1[..., 0:3].astype(np.float64) - x0[..., 0:3]) * n1[..., 0:3]).sum(axis=-1))
    moved = valid & (shift > 2 * t["position_threshold"] * x1[..., 3])
    want = truth[..., 0:3] / QUALITY_TRUTH_SPP

    def err(img, mask):
        a, b = img[..., 0:3][mask].astype(np.float64), want[mask].astype(np.float64)
        return float(np.linalg.norm(a - b) / np.linalg.norm(b))

    raw = sums[-1] / QUALITY_SPP
    print(f"animated_test: {int(moved.sum())} moved of {int(valid.sum())} valid pixels; relative L2 on the moved pixels: raw {err(raw, moved):.4f}, "
          f"plain chain {err(Tp, moved):.4f}, motion chain {err(Tm, moved):.4f}; mean L there {Tp[..., 3][moved].mean():.3f} / {Tm[..., 3][moved].mean():.3f}; "
          f"on all valid pixels: raw {err(raw, valid):.4f}, plain {err(Tp, valid):.4f}, motion {err(Tm, valid):.4f}")
    assert moved.sum() > 20 and (Tp[..., 3][moved] == 1).all()
    assert err(Tm, moved) < err(Tp, moved) and Tm[..., 3][moved].mean() > 1


# =====================================================================================================
# on the GPU
# =====================================================================================================
_gpu_state = {}


def _gpu(pkg, name, fresh=False):
    """(case, renderer) of `name`: uploaded once, tracking on, at pose 0.  fresh: a renderer of its own."""
    import torch  # noqa: F401  (first, so the HIP library shares torch's HIP runtime)

    c = _case(pkg, name)
    if fresh or name not in _gpu_state:
        r = pkg.Renderer()
        r.upload(c.desc)
        if fresh:
            return c, r
        _gpu_state[name] = r
    r = _gpu_state[name]
    r.track_motion(False)
    _pose(r, c, 0)
    r.track_motion(True)
    return c, r


def _pose(r, c, k, rebuild=False):
    it, bn = c.states[k]
    r.update_animation(it, bn if bn is not None and len(bn) else None, rebuild=rebuild)


def _images(r):
    return [r.read_guide(k) for k in range(3)] + [r.read_motion(k) for k in range(2)]


def _accumulate(r, S, cam, motion=True, moments=False, flags=0):
    r.write_accumulation(S)
    if motion:
        r.temporal_accumulate_motion(1, cam[1], cam[2], flags=flags, moments=moments, **TD)
    elif moments:
        r.temporal_accumulate_moments(1, cam[1], cam[2], flags=flags, **TD)
    else:
        r.temporal_accumulate(1, cam[1], cam[2], flags=flags, **TD)
    return r.read_temporal()


def _sequence(r, c, w, h, kind="still", rebuild=False):
    """The case's poses in turn, each with motion guides and an accumulate through them.  Returns [(five images, S, T)] and cameras."""
    r.resize(w, h)
    cams = c.camera(w, h, kind)
    out = []
    for k, cam in enumerate(cams):
        if k:
            _pose(r, c, k, rebuild)
        r.render_guides_motion(cam[0])
        img = _images(r)
        S = TT._synthetic_sum(h, w, img[2], 7 + k)
        out.append((img, S, _accumulate(r, S, cam)))
    return out, cams


GUIDE_CASES = ["animated_test", "skin_lab", "quads", "texture_test", "alpha_test", "count3", "count255", "count258", "count513"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", GUIDE_CASES)
def test_motion_guides_against_float64_reference(pkg, orc, name):
    c, r = _gpu(pkg, name)
    seq, cams = _sequence(r, c, W, H)
    for k, (img, _, _) in enumerate(seq):
        prev = k - 1 if k else None  # the first frame has no history: unknown
        r32 = _ref_motion(orc, c, name, k, prev, cams[k][0], W, H, np.float32)
        r64 = _ref_motion(orc, c, name, k, prev, cams[k][0], W, H, np.float64)
        hit = r64[0][..., 3] == 1
        assert hit.sum() > 200
        if name == "quads":  # what the case is for: hits on the second triangle of a quad, on the moving wall (pairs 1 ...)
            _, pair, prim, _, _, _ = M.primary_hits(_ref_pose(orc, c, name, k, np.float32)[0], cams[k][0], W, H)
            second = (prim % 2 == 1) & (pair >= 1)
            print(f"quads pose {k}: {int(second.sum())} of {int((pair >= 1).sum())} hits on the wall lie on a second triangle")
            assert second.sum() > 100 and ((prim % 2 == 0) & (pair >= 1)).sum() > 100
        for which, (got, a, b) in enumerate(zip([img[0], img[1], img[3], img[4]], r32, r64)):
            if name == "texture_test" and which in (0, 3):
                continue  # its normal maps are images: material.Normal is no constant the reference could state; positions and flags stand
            gap =float(np.abs(a.astype(np.float64) - b)[..., 0:3].max())
            err = np.abs(got.astype(np.float64) - b)[..., 0:3]
            tol = np.maximum(8.0 * gap, 2.0 ** -20 * np.maximum(1.0, np.abs(b[..., 0:3])))
            print(f"{name} pose {k} image {which}: max |gpu - ref64| {err.max():.3e}, max |ref32 - ref64| {gap:.3e}, hits {int(hit.sum())}")
            assert (err <= tol).all(), (name, k, which, float(err.max()), gap)
        # the flags and the misses, bit for bit
        want_w = np.where(hit, 0.0 if prev is None else 1.0, 0.0).astype(np.float32)
        for m in (img[3], img[4]):
            assert (_bits(m[..., 3]) == _bits(want_w)).all() and (_bits(m[~hit]) == 0).all(), (name, k)
        if prev is None:  # unknown: the guides themselves
            assert (_bits(img[3][..., 0:3]) == _bits(img[1][..., 0:3])).all() and (_bits(img[4][..., 0:3]) == _bits(img[0][..., 0:3])).all()
        else:
            still = hit & (_bits(img[3][..., 0:3]) == _bits(img[1][..., 0:3])).all(axis=-1)
            print(f"{name} pose {k}: {int(still.sum())} of {int(hit.sum())} hits did not move")
            assert name.startswith("count") or (hit & ~still).sum() > 20, "the pose must move something"


@pytest.mark.gpu
def test_refit_and_rebuild_give_the_same_five_images(pkg):
    runs = []
    for rebuild in (False, True):
        c, r = _gpu(pkg, "animated_test", fresh=True)
        r.track_motion(True)
        runs.append(_sequence(r, c, W, H, rebuild=rebuild)[0])
        r.close()
    a, b = runs
    for (ia, _, ta), (ib, _, tb) in zip(a, b):
        for x, y in zip(ia + [ta], ib + [tb]):
            assert (_bits(x) == _bits(y)).all()
    assert _known(a[1][0][3]).sum() > 200


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["animated_test", "texture_test", "alpha_test"])
def test_identities_of_the_guide_pass(pkg, name):
    """The three guides are ptx_render_guides' in every kernel mode; with no update since the history's pose X_prev and N_prev are
    the position and normal guides on hits, bit for bit."""
    c, r = _gpu(pkg, name)
    r.resize(W, H)
    cam = c.camera(W, H)[0]
    r.render_guides(cam[0])
    plain = [r.read_guide(k) for k in range(3)]
    with pytest.raises(pkg.PtxError, match="status 5"):
        r.read_motion(0)
    _pose(r, c, 1)
    for step in range(2):  # after an update without a history: unknown; then at the history's pose
        cam = c.camera(W, H)[1]
        r.render_guides(cam[0])
        plain = [r.read_guide(k) for k in range(3)]
        r.render_guides_motion(cam[0])
        img = _images(r)
        for k in range(3):
            assert (_bits(img[k]) == _bits(plain[k])).all(), (name, k)
        hit = img[0][..., 3] == 1
        assert hit.sum() > 200
        for m, g in ((img[3], img[1]), (img[4], img[0])):
            assert (_bits(m[..., 0:3]) == _bits(g[..., 0:3])).all() and (m[..., 3][hit] == step).all() and (m[..., 3][~hit] == 0).all(), (name, step)
        _accumulate(r, TT._synthetic_sum(H, W, img[2], 3), cam)
    assert r.motion_ptr(0) and r.motion_ptr(1) and not r.motion_ptr(2)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["still", "pan1"])
@pytest.mark.parametrize("moments", [False, True])
def test_accumulate_motion_is_the_plain_call_without_an_update(pkg, kind, moments):
    """On a borrower, against its owner's plain calls on the same sums"""
    c, r = _gpu(pkg, "animated_test")
    r.resize(W, H)
    b = pkg.Renderer()
    b.share_scene(r)
    b.resize(W, H)
    cams = c.camera(W, H, kind)
    for k, cam in enumerate(cams + cams[-1:]):
        r.render_guides(cam[0])
        b.render_guides_motion(cam[0])
        S = TT._synthetic_sum(H, W, r.read_guide(2), 40 + k)
        Tp, Tm = _accumulate(r, S, cam, motion=False, moments=moments), _accumulate(b, S, cam, moments=moments)
        assert (_bits(Tp) == _bits(Tm)).all(), (kind, k)
        if moments:
            assert (_bits(r.read_moments()) == _bits(b.read_moments())).all(), (kind, k)
    assert (Tm[..., 3] > 1).sum() > 200
    b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case", CHAINS, ids=lambda c: "%s-%s-%dx%d" % (c[0], c[1], *c[2]))
def test_accumulation_against_float64_reference(pkg, case):
    name, kind, (w, h) = case
    c, r = _gpu(pkg, name)
    seq, cams = _sequence(r, c, w, h, kind)
    frames = [(S, img[0], img[1], img[2], img[3], img[4], 1, cams[k][1], cams[k][2], 0) for k, (img, S, _) in enumerate(seq)]
    _check_chain(frames, [T for _, _, T in seq], "%s %s %dx%d" % (name, kind, w, h))
    if name != "animated_test" or (w, h) != (W, H):
        return
    # the plain chain on the same guides and sums: what moved restarts there and keeps its length here
    b = pkg.Renderer()
    b.share_scene(r)
    b.resize(w, h)
    plain = []
    _pose(r, c, 0)
    for k, cam in enumerate(cams[0:2]):
        if k:
            _pose(r, c, k)
        b.render_guides(cam[0])
        plain.append(_accumulate(b, seq[k][1], cam, motion=False))
    (i0, _, _), (i1, _, T1) = seq[0], seq[1]
    valid = (T1[..., 3] > 0) & (seq[0][2][..., 3] > 0)
    shift = np.abs(((i1[1][..., 0:3].astype(np.float64) - i0[1][..., 0:3]) * i1[0][..., 0:3]).sum(axis=-1))
    moved = valid & (shift > 2 * TD["position_threshold"] * i1[1][..., 3])
    unmoved = valid & (_bits(i0[0]) == _bits(i1[0])).all(axis=-1) & (_bits(i0[1]) == _bits(i1[1])).all(axis=-1)
    print(f"animated_test {kind}: {int(moved.sum())} moved pixels, of them L = 1 under the plain call {int((plain[1][..., 3][moved] == 1).sum())}, "
          f"L = 2 through the motion guides {int((T1[..., 3][moved] == 2).sum())}; {int(unmoved.sum())} unmoved")
    assert moved.sum() > 20
    if kind == "still":
        assert (plain[1][..., 3][moved] == 1).all() and unmoved.sum() > 200
        assert (T1[..., 3][moved] == 2).mean() > 0.5
        assert (_bits(T1)[unmoved] == _bits(plain[1])[unmoved]).all() and (T1[..., 3][unmoved] == 2).all()
    else:
        assert (T1[..., 3][moved] > 1.5).mean() > 0.5
    b.close()


@pytest.mark.gpu
def test_serial_rule(pkg):
    c, r = _gpu(pkg, "animated_test")
    r.resize(W, H)
    cam = c.camera(W, H)[0]

    def frame(who, seed, motion=True):
        who.render_guides_motion(cam[0])
        img = _images(who)
        return img, _accumulate(who, TT._synthetic_sum(H, W, img[2], seed), cam, motion=motion)

    img, T = frame(r, 1)  # the first call after ptx_track_motion, no history: unknown
    hit = img[0][..., 3] == 1
    assert hit.sum() > 200 and (img[3][..., 3] == 0).all() and (T[..., 3][T[..., 3] > 0] == 1).all()
    b = pkg.Renderer()  # a borrower with a history of its own, made at pose 0
    b.share_scene(r)
    b.resize(W, H)
    frame(b, 2)
    _pose(r, c, 1)
    img, T = frame(r, 3)  # one update: the snapshot
    assert (img[3][..., 3][img[0][..., 3] == 1] == 1).all() and (T[..., 3] == 2).sum() > 200
    _pose(r, c, 2)
    _pose(r, c, 1)
    img, T = frame(r, 4)  # two updates between the frames: unknown
    assert (img[3][..., 3] == 0).all() and (T[..., 3][T[..., 3] > 0] == 1).all()
    img, T = frame(b, 5)  # the borrower's history is three updates old
    assert (img[3][..., 3] == 0).all() and (T[..., 3][T[..., 3] > 0] == 1).all()
    _pose(r, c, 2)
    img, T = frame(b, 6)  # ... and now one: the borrower follows its own cadence
    assert (img[3][..., 3][img[0][..., 3] == 1] == 1).all() and (T[..., 3] == 2).sum() > 200
    # a plain accumulate moves the history's pose, and the next motion call follows it
    r.render_guides(cam[0])
    _accumulate(r, TT._synthetic_sum(H, W, r.read_guide(2), 7), cam, motion=False)
    img, T = frame(r, 8)
    moved = (_bits(img[3][..., 0:3]) != _bits(img[1][..., 0:3])).any(axis=-1)
    assert (img[3][..., 3][img[0][..., 3] == 1] == 1).all() and not moved.any() and (T[..., 3] == 2).sum() > 200
    # tracking enabled only after the update: nobody kept the pose
    r.track_motion(False)
    _pose(r, c, 1)
    r.track_motion(True)
    img, T = frame(r, 9)
    assert (img[3][..., 3] == 0).all() and (T[..., 3][T[..., 3] > 0] == 1).all()
    b.close()


@pytest.mark.gpu
def test_nothing_else_notices(pkg):
    """A path-traced frame and the update itself are the same with tracking on and off; ptx_resize drops the motion images"""
    c = _case(pkg, "animated_test")
    out = []
    for track in (False, True):
        _, r = _gpu(pkg, "animated_test", fresh=True)
        r.resize(W, H)
        if track:
            r.track_motion(True)
        _pose(r, c, 1)
        u = c.scene.uniform(W, H, bounces=4, sample_count=1, total_samples=0)
        r.render(u, c.scene.lights)
        st = r.stats()
        out.append((r.readback(), (st.pathSamples, st.segments, st.shadowRays, st.retries)))
        if track:
            r.render_guides_motion(u)
            assert r.motion_ptr(0)
            r.resize(W, H)
            assert not r.motion_ptr(0)
            with pytest.raises(pkg.PtxError, match="status 5"):
                r.read_motion(0)
        r.close()
    assert (_bits(out[0][0]) == _bits(out[1][0])).all() and out[0][1] == out[1][1]


@pytest.mark.gpu
def test_refusals_leave_the_images_and_the_history_intact(pkg):
    c, r = _gpu(pkg, "animated_test")
    seq, cams = _sequence(r, c, W, H)
    cam = cams[-1]
    # the sequence's last accumulate moved the history to the current pose; its motion guides lead back to the pose before
    with pytest.raises(pkg.PtxError, match="status 5"):
        r.temporal_accumulate_motion(1, cam[1], cam[2], **TD)
    assert (_bits(r.read_temporal()) == _bits(seq[-1][2])).all()
    r.render_guides_motion(cam[0])
    before = _images(r) + [r.read_temporal()]
    b = pkg.Renderer()
    b.share_scene(r)
    b.resize(W, H)
    with pytest.raises(pkg.PtxError, match="status 1"):  # a borrower does not decide about tracking
        b.track_motion(True)
    with pytest.raises(pkg.PtxError, match="status 1"):
        r.temporal_accumulate_motion(1, cam[1], cam[2], moments=2, **TD)
    for bad in (dict(TD, max_history=0.5), dict(TD, normal_threshold=0.0), dict(TD, position_threshold=float("nan"))):
        with pytest.raises(pkg.PtxError, match="status 1"):
            r.temporal_accumulate_motion(1, cam[1], cam[2], **bad)
    with pytest.raises(pkg.PtxError, match="status 1"):
        r.temporal_accumulate_motion(0, cam[1], cam[2], **TD)
    after = _images(r) + [r.read_temporal()]
    for x, y in zip(before, after):
        assert (_bits(x) == _bits(y)).all()
    T = _accumulate(r, TT._synthetic_sum(H, W, before[2], 90), cam)
    assert (T[..., 3] >= 2).sum() > 200
    r.render_guides(cam[0])  # a plain guide pass makes the motion guides stale
    with pytest.raises(pkg.PtxError, match="status 5"):
        r.temporal_accumulate_motion(1, cam[1], cam[2], **TD)
    with pytest.raises(pkg.PtxError, match="status 5"):
        r.read_motion(1)
    assert (_bits(r.read_temporal()) == _bits(T)).all()
    r.track_motion(False)  # tracking off: the guide pass is refused, on the owner and on the borrower
    for who in (r, b):
        with pytest.raises(pkg.PtxError, match="status 5"):
            who.render_guides_motion(cam[0])
    assert (_bits(r.read_temporal()) == _bits(T)).all() and (_bits(r.read_guide(1)) == _bits(before[1])).all()
    fresh = pkg.Renderer()
    with pytest.raises(pkg.PtxError, match="status 5"):  # no scene
        fresh.track_motion(True)
    fresh.close()
    b.close()


# ---- the host adapter ----------------------------------------------------------------------------------------------------------------

_driver = {}


def _motion_frame_driver(pkg, tmp_path_factory):
    """examples/motion_frame.cpp compiled against RendererHip and the HIP library, once; the sources in parallel"""
    import subprocess

    if "exe" not in _driver:
        out = tmp_path_factory.mktemp("motion_frame")
        host = pkg.PKG_DIR + "/host"
        sources = [pkg.REPO_DIR + "/examples/motion_frame.cpp"] + [f"{host}/{f}.cpp" for f in (
            "Scene", "Camera", "ExampleScenes", "OutputSaver", "TextureImporter", "JpegDecoder", "SceneImporter", "SceneDescription", "FbxReader", "ObjReader",
            "RendererHip")]
        objects = [str(out / (os.path.basename(s) + ".o")) for s in sources]
        jobs = [subprocess.Popen(["g++", "-std=c++20", "-O2", "-c", s, f"-I{host}", "-o", o]) for s, o in zip(sources, objects)]
        assert all(j.wait() == 0 for j in jobs)
        exe = str(out / "motion_frame")
        subprocess.check_call(["g++"] + objects + [f"-L{pkg.PKG_DIR}", "-lptx_hip", f"-Wl,-rpath,{pkg.PKG_DIR}", "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
        _driver["exe"] = exe
    return _driver["exe"]


@pytest.mark.gpu
@pytest.mark.parametrize("variance", [0, 1])
def test_renderer_hip_with_motion_vectors_is_the_same_calls_made_by_hand(pkg, tmp_path_factory, tmp_path, variance):
    """Two frames of animated_test through RendererHip with DenoiserSettings, TemporalSettings and MotionVectors on (variance: with the
    VarianceSettings too), the settings made BEFORE the upload, the pose moved in between: T and the output image of both frames
    equal ptx_track_motion, ptx_render_guides_motion, ptx_temporal_accumulate_motion, the filter and the output stage called by hand
    with the adapter's defaults, bit for bit -- and the second frame keeps a history on what moved."""
    import subprocess
    import torch  # noqa: F401

    w, h, spp, depth, step = W, H, 2, 4, 0.37
    exe = _motion_frame_driver(pkg, tmp_path_factory)
    dump = tmp_path / "frames.bin"
    subprocess.check_call([exe, "animated_test", str(w), str(h), str(spp), str(depth), str(step), str(variance), str(dump)])
    got = np.fromfile(dump, np.float32).reshape(2, 3, h, w, 4)
    s = pkg.Scene("animated_test", DETAIL)
    s.update(0.0)
    r = pkg.Renderer()
    r.upload(s)
    r.track_motion(True)
    it, bn = s.animation_state()
    r.update_animation(it, bn if len(bn) else None)  # the pose Scene::Update(0) leaves: the driver poses its first frame so too
    r.resize(w, h)
    lengths = []
    for frame in range(2):
        if frame:
            assert s.update(step)
            it, bn = s.animation_state()
            r.update_animation(it, bn if len(bn) else None)
        r.reset()
        for f in range(spp):
            r.render(s.uniform(w, h, bounces=depth, sample_count=1, total_samples=f), s.lights)
        r.render_guides_motion(s.uniform(w, h, bounces=depth, sample_count=1, total_samples=spp))
        view, proj = s.camera_matrices(w, h)
        r.temporal_accumulate_motion(spp, view, proj, max_history=32.0, normal_threshold=0.3, position_threshold=0.03, moments=bool(variance))
        if variance:
            r.denoise_variance(iterations=3, sigma_luminance=0.75, sigma_normal=0.3, sigma_position=0.03)
        else:
            r.denoise_temporal(iterations=3, sigma_color=1.5, sigma_normal=0.3, sigma_position=0.03)
        r.postprocess_denoised(spp, 1.0, 1.0, 1.0, pkg.TONE_MAPPING_SDR)
        S, T, out = r.readback(), r.read_temporal(), r.read_output(pkg.OUTPUT_RGBA32F)
        differ = [int((_bits(a) != _bits(b)).any(axis=-1).sum()) for a, b in zip(got[frame], (S, T, out))]
        print(f"variance {variance} frame {frame}: pixels differing in the sum, T and the output image {differ}")
        assert differ == [0, 0, 0], (variance, frame)
        lengths.append(T[..., 3])
        if frame:
            x_prev, x = r.read_motion(pkg.MOTION_POSITION), r.read_guide(pkg.GUIDE_POSITION)
            moved = (x_prev[..., 3] == 1) & (_bits(x_prev[..., 0:3]) != _bits(x[..., 0:3])).any(axis=-1)
    assert (lengths[0][lengths[0] > 0] == 1).all() and (lengths[1] == 2).sum() > 200
    assert moved.sum() > 20 and (lengths[1][moved] == 2).mean() > 0.5  # the snapshot was there: tracking was on before the update
    r.close()
