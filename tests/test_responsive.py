"""The responsive temporal history (include/ptx.h ptx_temporal_accumulate_responsive, csrc/pt_responsive.hpp, docs/NEXT_ROWS.md
section 19) against tests/responsive_ref.py.

Tolerance.  As tests/test_temporal.py: the reference runs on the device's own read-back sums and guides and keeps its own histories
in float32 and in float64.  T, F and (with MOMENTS) the moment history are held to 8 x the largest |ref(float32) - ref(float64)| of
that very quantity in that very case, with a floor of 2^-20 max(1, |value|); the colour history has no read-back of its own and is
held through the T of the frames after it.  A pixel on which the two runs of the reference decide differently -- a tap, found or
not, clamped or not, which side -- or whose history or window came through such a pixel is left out
(responsive_ref.comparable_pixels); the share left out is capped at 4 x the share the reference alone leaves out on the CPU's own
sequences (REFERENCE_LEFT_OUT) and at 2 % of the valid pixels.  Pixels that are not valid hold the mean bit for bit."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import denoise_ref as R
import responsive_ref as RR
import temporal_ref as TR
import util
import variance_ref as VR

W, H = 67, 45
DETAIL = 0.25
SCENE = "texture_test"
TD = dict(max_history=3.0, normal_threshold=0.3, position_threshold=0.03)
RD = dict(fast_history=2.0, clamp_sigma=1.5)
NEVER = 1e30  # a clampSigma under which no box is ever left
SHADOW = 4.0  # the lighting step of the sequences: the sum scaled by 4 inside the half-plane x >= w / 2 from the third frame on
LEFT_OUT_CAP = 0.02
# Measured on the CPU (test_reference_gap_and_left_out_share_on_the_cpu_sequences recomputes both): over the sequences below at 67 x 45
# on first-hit guides computed without a GPU, the largest |ref32 - ref64| of T.rgb and the largest share of valid pixels that
# comparable_pixels leaves out in a frame.
REFERENCE_GAP = 1.0e-3  # measured 8.5e-4, on values up to 3e5 (the synthetic sum's hot pixel over the albedo floor); 9.4e-5 on rendered sums
REFERENCE_LEFT_OUT = 0.0006  # measured 0.00054 (21 of 39,160 pixels, 300 x 200 under the sub-pixel pan); every other sequence leaves nothing out
IDENT = np.eye(4, dtype=np.float32).reshape(16)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# =====================================================================================================
# without a GPU
# =====================================================================================================
def test_header_declares_and_package_exports_the_responsive_call(pkg):
    header = open(os.path.join(pkg.REPO_DIR, "include", "ptx.h")).read()
    decls = {
        "ptx_temporal_accumulate_responsive": r"PTX_API int ptx_temporal_accumulate_responsive\(PtxRenderer \*r, const PtxTemporalDesc \*desc, "
                                              r"const PtxResponsiveDesc \*responsive\);",
        "ptx_read_fast_history": r"PTX_API int ptx_read_fast_history\(PtxRenderer \*r, void \*host, size_t bytes\);",
        "ptx_device_fast_history_ptr": r"PTX_API void \*ptx_device_fast_history_ptr\(PtxRenderer \*r\);",
    }
    lib = pkg.load_hip()
    for name, decl in decls.items():
        assert re.search(decl, header), name
        assert name in pkg.PTX_SYMBOLS
        assert hasattr(lib, name), name
    assert "#define PTX_ABI_VERSION 5u" in header and "PTX_FN_COUNT = 38" in header  # additions only
    assert re.search(r"enum \{ PTX_RESPONSIVE_MOMENTS = 1, PTX_RESPONSIVE_MOTION = 2 \};", header)
    assert (pkg.RESPONSIVE_MOMENTS, pkg.RESPONSIVE_MOTION) == (1, 2) == (RR.MOMENTS, RR.MOTION)
    assert re.search(r"typedef struct PtxResponsiveDesc \{\s*float fastHistory;[^}]*float clampSigma;[^}]*uint32_t flags;[^}]*uint32_t reserved;[^}]*\} "
                     r"PtxResponsiveDesc;", header)
    D = pkg.ResponsiveDesc
    assert C.sizeof(D) == 16 and (D.fastHistory.offset, D.clampSigma.offset, D.flags.offset, D.reserved.offset) == (0, 4, 8, 12)
    # the semantics are in the header as text: the reference is written from it
    for phrase in ("FAST HISTORY", "L_F = min(sum w L_F'(q) / sum w_F + 1, fastHistory)", "F = F_h + (c - F_h) / L_F", "L > 1", "5 x 5", "n >= 1",
                   "var = sum (F(q) - mu)^2 / n", "lo = mu - clampSigma sigma", "c' = min(max(c_acc, lo), hi)", "L_out = min(L, L_F(p))",
                   "L_M becomes min(L_M, L_F(p))", "32 more bytes", "DROPS the fast history", "sqrt_ of csrc/pt_device.hpp", "section 19"):
        assert phrase in header, phrase
    assert "a moving light still lags" not in header
    for method in ("temporal_accumulate_responsive", "read_fast_history", "fast_history_ptr"):
        assert callable(getattr(pkg.Renderer, method))
    d = pkg.RESPONSIVE_DEFAULTS
    assert set(d) == {"fast_history", "clamp_sigma"} and 1 <= d["fast_history"] <= pkg.TEMPORAL_DEFAULTS["max_history"] and d["clamp_sigma"] > 0
    state = open(os.path.join(pkg.PKG_DIR, "csrc", "pt_chain_state.hpp")).read()
    assert "fastLive" in state and "Accumulate accumulate(bool moments, bool reset, bool fast = false)" in state
    assert os.path.exists(os.path.join(pkg.PKG_DIR, "csrc", "pt_responsive.hpp"))


def _plane(h, w, **kw):
    return R.plane_guides(h, w, distance=5.0, pixel=0.01, **kw)


def _const_sum(h, w, value, samples=2):
    S = np.zeros((h, w, 4), np.float32)
    S[..., 0:3] = np.float32(value) * samples
    S[..., 3] = samples
    return S


def _noise_sum(h, w, seed, samples=2):
    S = np.zeros((h, w, 4), np.float32)
    S[..., 0:3] = np.random.default_rng(seed).uniform(0.1, 1.0, (h, w, 3)) * samples
    S[..., 3] = samples
    return S


def _frames_of(sums, guides, samples=2, flags=None):
    return [(S, *guides, samples, IDENT, IDENT, flags[k] if flags else 0) for k, S in enumerate(sums)]


def _seq(frames, dtype, fast_history, clamp_sigma, max_history=32.0, rflags=0, plain=()):
    return RR.run_sequence(frames, max_history, 0.3, 0.03, fast_history, clamp_sigma, dtype, rflags, plain)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_first_reset_and_max_history_1_calls_are_the_base_call(dtype):
    """Consequence (a), in the reference: no pixel has L > 1, so pass B is the identity"""
    h, w = 9, 13
    g = _plane(h, w, albedo=(0.8, 0.5, 0.004))
    sums = [_noise_sum(h, w, k) for k in range(4)]
    flags = [0, 0, TR.RESET, 0]
    frames = _frames_of(sums, g, flags=flags)
    T, _, F, _, dec = _seq(frames, dtype, 2.0, 0.5)
    base = TR.run_sequence(frames, 32.0, 0.3, 0.03, dtype)[0]
    for k in (0, 2):
        assert (T[k] == base[k]).all() and not dec[k]["acts"].any() and (F[k].L == 1).all()
    assert dec[1]["acts"].all() and dec[1]["clamped"].any()  # ... and it is not where there is a history
    T1 = _seq(frames, dtype, 1.0, 0.5, max_history=1.0)[0]
    b1 = TR.run_sequence(frames, 1.0, 0.3, 0.03, dtype)[0]
    assert all((a == b).all() for a, b in zip(T1, b1))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_fast_history_as_long_as_the_long_one_is_the_colour_history(dtype):
    """Consequence (b): the same operations on the same operands, bit for bit, while nothing is clamped"""
    h, w = 8, 11
    g = _plane(h, w, albedo=(0.8, 0.5, 0.004))
    frames = _frames_of([_noise_sum(h, w, 10 + k) for k in range(6)], g)
    T, hist, F, _, dec = _seq(frames, dtype, 4.0, NEVER, max_history=4.0)
    base = TR.run_sequence(frames, 4.0, 0.3, 0.03, dtype)[0]
    for k in range(6):
        assert not dec[k]["clamped"].any() and (T[k] == base[k]).all()
        assert (F[k].c == hist[k].c).all() and (F[k].L == hist[k].L).all() and (F[k].L == min(k + 1, 4)).all()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_a_step_of_a_constant_frame(dtype):
    """Colour 1 for 8 calls, then 3.  fastHistory 1: the first call after the change returns 3 and L = 1.  fastHistory 4: F is constant
    over every window, so c' = F(p) (consequence (c)) and T follows F's series 3 - 2 (3/4)^k, exact in binary, with L = L_F = 4."""
    h, w = 7, 9
    g = _plane(h, w)
    frames = _frames_of([_const_sum(h, w, 1.0)] * 8 + [_const_sum(h, w, 3.0)] * 4, g)
    T, _, F, _, dec = _seq(frames, dtype, 1.0, 1.0)
    assert (T[7][..., 0:3] == 1).all() and (T[7][..., 3] == 8).all() and not dec[7]["clamped"].any()
    assert (T[8][..., 0:3] == 3).all() and (T[8][..., 3] == 1).all() and dec[8]["clamped"].all()
    T, _, F, _, dec = _seq(frames, dtype, 4.0, 1.0)
    assert (T[7][..., 0:3] == 1).all() and (T[7][..., 3] == 8).all() and (F[7].L == 4).all()
    for k in range(1, 5):
        want = 3.0 - 2.0 * 0.75 ** k
        assert (T[7 + k][..., 0:3] == want).all() and (F[7 + k].c == want).all(), k
        assert (T[7 + k][..., 3] == 4).all() and (F[7 + k].L == 4).all() and dec[7 + k]["clamped"].all(), k


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_one_differing_pixel_widens_the_boxes_of_its_24_neighbours(dtype):
    h, w, d = 11, 12, 5.0
    F = np.zeros((h, w, 3), dtype)
    F[5, 6] = d
    LF = np.full((h, w), 2, dtype)
    c = np.full((h, w, 3), 0.25, dtype)  # inside a widened box, outside a box of zero width
    c_out, L_out, dec = RR.clamp(c, np.full((h, w), 3, dtype), F, LF, np.ones((h, w), bool), 1.0, dtype)
    near = np.zeros((h, w), bool)
    near[3:8, 4:9] = True
    mu, sigma = d / 25, d * np.sqrt(24.0) / 25
    assert mu - sigma < 0.25 < mu + sigma
    assert (dec["clamped"] == ~near).all() and (c_out[near] == 0.25).all() and (c_out[~near] == 0).all()
    assert (L_out[near] == 3).all() and (L_out[~near] == 2).all()
    # ... by exactly mu +- sigma: a value just outside is brought to the bound
    c2 = np.full((h, w, 3), 2.0, dtype)
    c_out2, _, dec2 = RR.clamp(c2, np.full((h, w), 3, dtype), F, LF, np.ones((h, w), bool), 1.0, dtype)
    assert dec2["clamped"].all() and np.abs(c_out2[near] - (mu + sigma)).max() <= 8 * np.finfo(dtype).eps * (mu + sigma)
    # the window at the image's corner has 9 taps, at an edge 15, inside 25
    n = dec["wtaps"].sum(axis=-1)
    assert n[0, 0] == n[-1, -1] == n[0, -1] == 9 and n[0, 5] == n[5, 0] == 15 and n[5, 5] == 25 and n[1, 1] == 16


def test_misses_non_finite_pixels_and_unknown_f_take_part_in_no_window():
    h, w = 10, 14
    g = _plane(h, w)
    miss = np.zeros((h, w), bool)
    miss[:, 10:] = True
    R.set_miss(g, miss)
    g[2][6, 7, 2] = 0.001  # below the albedo floor
    sums = [_noise_sum(h, w, 1), _noise_sum(h, w, 2)]
    for S in sums:
        S[3, 4, 1] = np.nan  # not valid: zeros in F
        S[6, 7, 2] = 3e38  # valid, but its demodulated mean overflows float32: F is not finite, stored as zeros, L_F = 0
    T, hist, F, _, dec = _seq(_frames_of(sums, g), np.float32, 2.0, 1.0)
    for k in (0, 1):
        assert (F[k].L[miss] == 0).all() and (F[k].c[miss] == 0).all() and F[k].L[3, 4] == 0 and F[k].L[6, 7] == 0 and (F[k].c[6, 7] == 0).all()
        assert np.isfinite(F[k].c).all() and dec[k]["valid"][6, 7] and not dec[k]["known_F"][6, 7]
    d = dec[1]
    n = d["wtaps"].sum(axis=-1)
    assert n[3, 2] == 24 and n[7, 6] == 24 and n[5, 6] == 23  # the window holds the NaN pixel, the unknown one, both
    assert n[2, 9] == 5 * 3 and n[0, 9] == 3 * 3  # the miss columns count for nobody
    assert not d["acts"][3, 4] and not d["acts"][6, 7] and not d["acts"][miss].any()
    rest = d["valid"].copy()
    rest[6, 7] = False
    assert np.isfinite(T[1][rest]).all() and d["clamped"].any()  # no box took a NaN or an Inf in


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_a_centre_with_unknown_f_is_not_clamped(dtype):
    h, w = 7, 8
    F, LF = np.zeros((h, w, 3), dtype), np.full((h, w), 2, dtype)
    LF[3, 4] = 0
    c = np.full((h, w, 3), 9.0, dtype)  # far outside every box
    c_out, L_out, dec = RR.clamp(c, np.full((h, w), 3, dtype), F, LF, np.ones((h, w), bool), 1.0, dtype)
    assert not dec["acts"][3, 4] and not dec["clamped"][3, 4] and (c_out[3, 4] == 9).all() and L_out[3, 4] == 3
    rest = np.ones((h, w), bool)
    rest[3, 4] = False
    assert dec["clamped"][rest].all() and (c_out[rest] == 0).all() and (L_out[rest] == 2).all()
    assert dec["wtaps"].sum(axis=-1)[3, 3] == 24 and dec["wtaps"].sum(axis=-1)[3, 4] == 0


def test_a_pixel_without_history_is_not_clamped():
    h, w = 8, 10
    g0, g1 = _plane(h, w), _plane(h, w)
    part = np.zeros((h, w), bool)
    part[2:5, 3:8] = True
    g1[0][part, 0:3] = np.float32([0.0, np.sin(0.4), np.cos(0.4)])  # the normal test fails there: L = 1
    S0, S1 = _const_sum(h, w, 1.0), _const_sum(h, w, 1.0)
    S1[part, 0:3] = 50.0  # far outside every box
    frames = [(S0, *g0, 2, IDENT, IDENT, 0), (S1, *g1, 2, IDENT, IDENT, 0)]
    T, _, F, _, dec = _seq(frames, np.float64, 2.0, 1.0)
    assert (T[1][..., 3][part] == 1).all() and not dec[1]["acts"][part].any() and (T[1][part][:, 0:3] == 25).all()
    assert dec[1]["acts"][~part].all() and (F[1].L[part] == 1).all()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_moments_follow_the_base_call_and_their_length_follows_on_clamped_pixels_only(dtype):
    h, w = 9, 12
    g = _plane(h, w, albedo=(0.8, 0.5, 0.004))
    sums = [_noise_sum(h, w, 20 + k) for k in range(5)]
    for S in sums[3:]:
        S[:, w // 2:, 0:3] *= 4
    frames = _frames_of(sums, g)
    T, _, F, M, dec = _seq(frames, dtype, 2.0, 1.0, max_history=4.0, rflags=RR.MOMENTS)
    Tn, _, Fn, Mn, decn = _seq(frames, dtype, 2.0, NEVER, max_history=4.0, rflags=RR.MOMENTS)
    base = VR.run_sequence(frames, 4.0, 0.3, 0.03, dtype)
    seen = 0
    for k in range(5):
        assert not decn[k]["clamped"].any()
        assert (Tn[k] == base[0][k]).all() and (Mn[k].image() == base[1][k].image()).all()  # pass A is the moments call
        cl = dec[k]["clamped"]
        seen += int(cl.sum())
        if k == 0:
            continue
        # one call from a common start: the lengths drop on the clamped pixels, the moments themselves are kept
        Tk, _, Fk, Mk, dk = RR.accumulate(*frames[k][0:7], *_state_after(frames[:k], dtype, 2.0, NEVER, 4.0), 4.0, 0.3, 0.03, 2.0, 1.0, 0, RR.MOMENTS, None, dtype)
        c = dk["clamped"]
        assert (Mk.m1 == Mn[k].m1).all() and (Mk.m2 == Mn[k].m2).all()
        assert (Mk.L[~c] == Mn[k].L[~c]).all() and (Mk.L[c] == np.minimum(Mn[k].L[c], Fk.L[c])).all()
        assert (Tk[..., 3][c] == np.minimum(Tn[k][..., 3][c], Fk.L[c])).all() and (Tk[..., 3][~c] == Tn[k][..., 3][~c]).all()
    assert seen > 20


def _state_after(frames, dtype, fast_history, clamp_sigma, max_history):
    """(history, fast, moments) after a MOMENTS sequence"""
    _, hist, F, M, _ = _seq(frames, dtype, fast_history, clamp_sigma, max_history=max_history, rflags=RR.MOMENTS)
    return hist[-1], F[-1], M[-1]


def test_a_plain_call_drops_the_fast_history():
    h, w = 6, 8
    frames = _frames_of([_noise_sum(h, w, k) for k in range(3)], _plane(h, w))
    T, hist, F, _, dec = _seq(frames, np.float64, 2.0, 1.0, plain=(1,))
    cl = dec[2]["clamped"]  # F restarts on the colour history as it stands: L = 3 where the new box holds it, L_F = 1 where not
    assert F[1] is None and (F[2].L == 1).all() and (hist[2].L[~cl] == 3).all() and (hist[2].L[cl] == 1).all() and cl.any() and not cl.all()
    assert (F[2].c == frames[2][0][..., 0:3].astype(np.float64) * 0.5).all()


# ---- the sequences of the GPU tests, and what the reference alone says about them ------------------------------------------------------

def _rot_y(d, deg):
    a = np.radians(deg)
    return np.float64([d[0] * np.cos(a) + d[2] * np.sin(a), d[1], -d[0] * np.sin(a) + d[2] * np.cos(a)])


_base = {}


def _base_pose(pkg, name, w, h):
    if name not in _base:
        _base[name] = TR.scene_pose(pkg.Scene(name, DETAIL), w, h)
    return _base[name]


FRAMES = 5


def _poses(pkg, scene, kind, w, h, frames=FRAMES):
    """test_temporal's sequences: a still camera, the sub-pixel pan (a little up as well: off the grid) and the turn with a dolly.
    (Its jump is not among them: a pixel the two runs of the reference decide differently takes its 5 x 5 neighbours with it, frame
    after frame, and the eight such pixels after the jump grow to a fifth of the image -- over the condition on the inputs.)"""
    pos, fwd, right = _base_pose(pkg, scene.name, w, h)
    up = np.cross(fwd, right)
    footprint = 2.0 * 7.0 / (float(scene.camera_matrices(w, h)[1][5]) * h)
    if kind == "still":
        return [(pos, fwd)] * frames
    if kind == "subpixel":
        return [(pos + (right * 0.37 + up * 0.29) * (footprint * f), fwd) for f in range(frames)]
    if kind == "turn_dolly":
        return [(pos + fwd * (0.15 * f) + right * (0.05 * f), _rot_y(fwd, 1.3 * f)) for f in range(frames)]
    raise KeyError(kind)


def _synthetic_sum(h, w, albedo, seed, markers=True):
    """albedo x a smooth light x noise; with a hot pixel, a NaN and an Inf marker pixel"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    light = np.stack([0.4 + 0.5 * xx / w, 0.3 + 0.6 * yy / h, 0.5 + 0.0 * xx], axis=-1)
    S = np.zeros((h, w, 4), np.float32)
    S[..., 0:3] = albedo[..., 0:3] * light * rng.uniform(0.2, 1.8, (h, w, 3))
    if markers:
        S[(h // 2) % h, (w // 3) % w, 0:3] = 3000.0
        S[2 % h, 3 % w, 0] = np.nan
        S[4 % h, 5 % w, 1] = np.inf
    S[..., 3] = 1
    return S


def _shadow(S, k):
    """The lighting step: from the third frame on the half-plane x >= w / 2 is four times as bright"""
    S = np.array(S, np.float32)
    if k >= 2:
        S[:, S.shape[1] // 2:, 0:3] *= np.float32(SHADOW)
    return S


def _compare(frames, got, label, rflags=0, plain=(), rd=RD):
    """frames as responsive_ref.run_sequence takes them; got: per frame (T, F or None, M or None) of the implementation (None: the
    reference alone).  Returns (largest |ref32 - ref64| of T in the case, largest share of valid pixels left out in a frame)."""
    a = RR.run_sequence(frames, TD["max_history"], TD["normal_threshold"], TD["position_threshold"], rd["fast_history"], rd["clamp_sigma"], np.float32, rflags, plain)
    b = RR.run_sequence(frames, TD["max_history"], TD["normal_threshold"], TD["position_threshold"], rd["fast_history"], rd["clamp_sigma"], np.float64, rflags, plain)
    keep = RR.comparable_pixels(a[4], b[4])

    def images(run, k):
        return [run[0][k], None if run[2][k] is None else run[2][k].image(), None if run[3][k] is None else run[3][k].image()]

    worst, share, clamped = [0.0, 0.0, 0.0], 0.0, 0
    for k in range(len(frames)):
        valid = b[4][k]["valid"]
        for q, (x, y) in enumerate(zip(images(a, k), images(b, k))):
            if y is None:
                continue
            fin = keep[k][..., None] & np.isfinite(x) & np.isfinite(y)
            if fin.any():
                with np.errstate(all="ignore"):
                    worst[q] = max(worst[q], float(np.abs(x.astype(np.float64) - y)[fin].max()))
        if valid.any():
            share = max(share, float((valid & ~keep[k]).sum()) / float(valid.sum()))
        clamped += int(b[4][k].get("clamped", np.zeros(1, bool)).sum())
    if got is None:
        return worst[0], share, clamped, b
    assert share <= min(LEFT_OUT_CAP, 4 * REFERENCE_LEFT_OUT), (label, share)
    for k, imgs in enumerate(got):
        valid = b[4][k]["valid"]
        m = R.mean_of(frames[k][0], frames[k][4], np.float32)
        for q, (G, y) in enumerate(zip(imgs, images(b, k))):
            if y is None:
                assert G is None, (label, k, q)
                continue
            assert G.shape == y.shape and G.dtype == np.float32
            if q == 0:  # pixels that are not valid hold the mean and L = 0, bit for bit, whatever class they have
                assert (_bits(G[..., 0:3])[~valid] == _bits(m)[~valid]).all() and (G[..., 3][~valid] == 0).all(), (label, k)
            else:
                assert (_bits(G)[~valid] == 0).all(), (label, k, q)
            cmp = keep[k] & valid
            fin = cmp[..., None] & np.isfinite(y)
            assert (np.isfinite(G) == np.isfinite(y))[cmp].all(), (label, k, q)
            with np.errstate(all="ignore"):
                err = np.abs(G.astype(np.float64) - y)[fin]
            tol = np.maximum(8.0 * worst[q], 2.0 ** -20 * np.maximum(1.0, np.abs(y[fin])))
            if err.size:
                print(f"{label} frame {k} {'TFM'[q]}: max |gpu - ref64| {err.max():.3e}, max |ref32 - ref64| of the case {worst[q]:.3e}, left out "
                      f"{int((valid & ~keep[k]).sum())} of {int(valid.sum())} valid pixels, clamped {int(b[4][k].get('clamped', np.zeros(1, bool)).sum())}, "
                      f"largest value {np.abs(y[fin]).max():.3e}")
                assert (err <= tol).all(), (label, k, q, float(err.max()), worst[q])
    return worst[0], share, clamped, b


def _cpu_guides(pkg, orc, scene, w, h):
    try:
        return R.cpu_guides(pkg, orc, scene, w, h)
    except KeyError:  # no pixel was hit
        g = [np.zeros((h, w, 4), np.float32) for _ in range(3)]
        R.set_miss(g, np.ones((h, w), bool))
        return g


SEQUENCES = ("still", "subpixel", "turn_dolly")


def test_reference_gap_and_left_out_share_on_the_cpu_sequences(pkg, orc):
    """What the tolerance and the cap rest on, measured without a GPU: the sequences of the GPU tests on first-hit guides from the
    debug view's reference and the oracle's own 1-spp sums (the synthetic sum with its markers where the GPU test takes it), with the
    lighting step.  CONDITION ON THE INPUTS: the reference alone leaves out at most 0.5 % of the valid pixels on every sequence, a
    quarter of the 2 % cap.  (The turn with a dolly does not meet it at 300 x 200 -- one tap decision in the second frame grows, window
    by window, to 429 of 38,840 pixels in the fifth -- so the large extent runs under the still camera and the sub-pixel pan.)"""
    scene = pkg.Scene(SCENE, DETAIL)
    worst, share, rendered = 0.0, 0.0, {}
    for (w, h), kind, rflags, markers in [((W, H), k, f, False) for k in SEQUENCES for f in (0, RR.MOMENTS)] + [((W, H), "subpixel", 0, True)] + \
                                        [((300, 200), "still", 0, False), ((300, 200), "subpixel", 0, False), ((1, 1), "still", 0, False),
                                         ((5, 3), "subpixel", 0, False), ((33, 9), "still", 0, False), ((33, 9), "turn_dolly", RR.MOMENTS, False)]:
        frames, sums = [], []
        for f, (p, d) in enumerate(_poses(pkg, scene, kind, w, h)):
            scene.set_camera_pose(p, d)
            if (w, kind, f) not in rendered:
                g = _cpu_guides(pkg, orc, scene, w, h)
                rendered[(w, kind, f)] = (g, None if kind == "still" and f >= 2 else TR.render_oracle_sum(orc, scene, w, h, 1, f))
            g, S = rendered[(w, kind, f)]
            if markers:
                S = _synthetic_sum(h, w, g[2], 7 + f)
            elif S is None:
                S = sums[f - 2]
            sums.append(S)
            frames.append((_shadow(S, f), *g, 1, *scene.camera_matrices(w, h), 0))
        a, b, clamped, run = _compare(frames, None, kind, rflags)
        print(f"{w} x {h} {kind} flags {rflags} markers {markers}: max |ref32 - ref64| {a:.3e}, left out {b:.5f}, clamped pixels over the sequence {clamped}; "
              f"valid per frame {[int(d['valid'].sum()) for d in run[4]]}")
        assert (clamped > 100 or w * h < 3000) and b <= 0.005, (kind, rflags, b)
        worst, share = max(worst, a), max(share, b)
    assert REFERENCE_GAP / 4 <= worst <= REFERENCE_GAP and REFERENCE_LEFT_OUT / 4 <= share <= REFERENCE_LEFT_OUT and 4 * REFERENCE_LEFT_OUT <= LEFT_OUT_CAP


def _quality(pkg, frames, truth):
    """Relative L2 errors of the last frame: (raw, spatial filter, plain temporal, plain + filter, responsive, responsive + filter)"""
    t, dd, cd, rd = pkg.TEMPORAL_DEFAULTS, pkg.DENOISE_DEFAULTS, pkg.TEMPORAL_DENOISE_DEFAULTS, pkg.RESPONSIVE_DEFAULTS
    S, nrm, pos, alb, spp = frames[-1][0:5]
    T = TR.run_sequence(frames, t["max_history"], t["normal_threshold"], t["position_threshold"], np.float32)[0][-1]
    Tr = RR.run_sequence(frames, t["max_history"], t["normal_threshold"], t["position_threshold"], rd["fast_history"], rd["clamp_sigma"], np.float32)[0][-1]
    assert np.isfinite(Tr[..., 0:3]).all()
    spatial = R.denoise(S, nrm, pos, alb, spp, dd["iterations"], dd["sigma_color"], dd["sigma_normal"], dd["sigma_position"], np.float32)
    chain = [R.denoise(x, nrm, pos, alb, 1, cd["iterations"], cd["sigma_color"], cd["sigma_normal"], cd["sigma_position"], np.float32) for x in (T, Tr)]
    return [R.relative_l2(x, truth) for x in (S[..., 0:3] / spp, spatial, T, chain[0], Tr, chain[1])]


def test_a_moving_light_is_followed_sooner_than_by_the_plain_call(pkg, orc):
    """The quality table of docs/NEXT_ROWS.md section 19 (tools/temporal_quality.py --responsive): 12 frames of 4 spp of the CPU oracle
    on animated_test under a still camera, the point light stepping to the far end of its track after the eighth frame, or sliding
    there a twelfth per frame.  Against the oracle's own 192 spp with the light at its last position
    (tests/golden/responsive_truth.npz, other samples) the responsive call at RESPONSIVE_DEFAULTS is closer than the plain one at the
    last frame, with and without the filter at TEMPORAL_DENOISE_DEFAULTS."""
    truth = np.load(os.path.join(util.GOLDEN_DIR, "responsive_truth.npz"))["light"].astype(np.float32)
    assert truth.shape == (TR.QUALITY_H, TR.QUALITY_W, 3)
    shared = RR.light_scene(pkg, orc)
    for kind in RR.LIGHT_SEQUENCES:
        raw, spa, tmp, chn, rsp, rch = _quality(pkg, RR.light_sequence(shared, pkg, kind), truth)
        print(f"{kind}: relative L2 error raw {raw:.4f}, spatial {spa:.4f}, temporal {tmp:.4f}, temporal + spatial {chn:.4f}, responsive {rsp:.4f}, "
              f"responsive + spatial {rch:.4f}")
        assert rsp < tmp and rch < chn, kind


@pytest.mark.parametrize("name", ["default", "texture_test"])
def test_the_controls_keep_what_the_plain_call_gives_them(pkg, orc, name):
    """Section 14's sliding-camera sequences, where nothing changes and the clamp can only do harm or suppress fireflies: the relations
    section 14's test asserts for the plain call hold for the responsive one -- the accumulated frame is closer than the raw one, and
    filtered at TEMPORAL_DENOISE_DEFAULTS closer than the raw frame filtered at DENOISE_DEFAULTS."""
    truth = np.load(os.path.join(util.GOLDEN_DIR, "temporal_truth.npz"))[name].astype(np.float32)
    raw, spa, tmp, chn, rsp, rch = _quality(pkg, TR.quality_sequence(pkg, orc, name)[1], truth)
    print(f"{name}: relative L2 error raw {raw:.4f}, spatial {spa:.4f}, temporal {tmp:.4f}, temporal + spatial {chn:.4f}, responsive {rsp:.4f}, "
          f"responsive + spatial {rch:.4f}")
    assert rsp < raw and rch < spa


# =====================================================================================================
# on the GPU
# =====================================================================================================
_state = {}
EXTENTS = {"67x45": (67, 45), "1x1": (1, 1), "5x3": (5, 3), "33x9": (33, 9), "300x200": (300, 200)}


def _gpu(pkg, name=SCENE):
    """(scene, renderer) of `name`, uploaded once"""
    import torch  # noqa: F401  (first, so the HIP library shares torch's HIP runtime)

    if name not in _state:
        s = pkg.Scene(name, DETAIL)
        r = pkg.Renderer()
        r.upload(s)
        _state[name] = (s, r)
    return _state[name]


_frames_cache = {}


def _frames(pkg, extent, kind, synthetic=False):
    """[(frame tuple, uniform)] of one sequence: the device's own 1-spp sums and guides, read back once and shared by the tests.  The
    still camera renders two frames, the later ones take the sum of two frames earlier; every frame from the third on has the
    lighting step."""
    key = (extent, kind, synthetic)
    if key not in _frames_cache:
        s, r = _gpu(pkg)
        w, h = EXTENTS[extent]
        r.set_tile_shard(0, 1, 32)
        r.resize(w, h)
        out, sums = [], []
        for f, pose in enumerate(_poses(pkg, s, kind, w, h)):
            s.set_camera_pose(*pose)
            u = s.uniform(w, h, bounces=4, sample_count=1, total_samples=f)
            r.render_guides(u)
            g = [r.read_guide(k) for k in range(3)]
            if synthetic:
                S = _synthetic_sum(h, w, g[2], 7 + f)
            elif kind == "still" and f >= 2:
                S = sums[f - 2]
            else:
                r.reset()
                r.render(u, s.lights)
                S = r.readback()
            sums.append(S)
            out.append(((_shadow(S, f), *g, 1, *s.camera_matrices(w, h), 0), u))
        _frames_cache[key] = out
    return _frames_cache[key]


def _call(r, frame, rflags=0, flags=0, rd=RD, td=TD):
    r.temporal_accumulate_responsive(frame[4], frame[5], frame[6], flags=flags, responsive_flags=rflags, **td, **rd)


def _base_call(r, frame, rflags=0, flags=0, td=TD):
    if rflags & RR.MOTION:
        r.temporal_accumulate_motion(frame[4], frame[5], frame[6], flags=flags, moments=bool(rflags & RR.MOMENTS), **td)
    elif rflags & RR.MOMENTS:
        r.temporal_accumulate_moments(frame[4], frame[5], frame[6], flags=flags, **td)
    else:
        r.temporal_accumulate(frame[4], frame[5], frame[6], flags=flags, **td)


def _read(r, rflags, fast=True):
    return (r.read_temporal(), r.read_fast_history() if fast else None, r.read_moments() if rflags & RR.MOMENTS else None)


def _replay(r, frames, rflags=0, flags=None, rd=RD, td=TD, base=False, motion=False):
    """The frames' own sums and uniforms on handle r: per frame (T, F, M)"""
    out = []
    for k, (frame, u) in enumerate(frames):
        r.write_accumulation(frame[0])
        (r.render_guides_motion if motion else r.render_guides)(u)
        if base:
            _base_call(r, frame, rflags, flags[k] if flags else 0, td)
        else:
            _call(r, frame, rflags, flags[k] if flags else 0, rd, td)
        out.append(_read(r, rflags, fast=not base))
    return out


def _handle(pkg, w, h, name=SCENE):
    b = pkg.Renderer()
    b.share_scene(_gpu(pkg, name)[1])
    b.resize(w, h)
    return b


GPU_CASES = [("67x45", "still", 0), ("67x45", "subpixel", 0), ("67x45", "turn_dolly", 0), ("67x45", "still", RR.MOMENTS), ("67x45", "subpixel", RR.MOMENTS),
             ("1x1", "still", 0), ("5x3", "subpixel", 0), ("33x9", "still", 0), ("33x9", "turn_dolly", RR.MOMENTS), ("300x200", "still", 0),
             ("300x200", "subpixel", 0)]


@pytest.mark.gpu
@pytest.mark.parametrize("case", GPU_CASES, ids=lambda c: "%s-%s-%d" % c)
def test_sequences_against_float64_reference(pkg, case):
    """On a borrower, with a moving shadow edge from the third frame on"""
    extent, kind, rflags = case
    frames = _frames(pkg, extent, kind)
    w, h = EXTENTS[extent]
    b = _handle(pkg, w, h)
    got = _replay(b, frames, rflags)
    assert b.fast_history_ptr()
    for frame, _ in frames[-1:]:
        assert (_bits(b.readback()) == _bits(frame[0])).all()  # the sum is an input
        for k in range(3):
            assert (_bits(b.read_guide(k)) == _bits(frame[1 + k])).all()  # ... and so are the guides
    b.close()
    _, _, clamped, ref = _compare([f for f, _ in frames], got, "%s %s %d" % case, rflags)
    if extent in ("67x45", "300x200"):
        assert clamped > 100
    if kind == "still" and extent == "67x45" and not rflags:
        # the first frame after the change: L = min(L, L_F) on exactly the pixels the reference clamps, 3 on the others
        d, T, F = ref[4][2], got[2][0], got[2][1]
        keep = RR.comparable_pixels(RR.run_sequence([f for f, _ in frames], TD["max_history"], TD["normal_threshold"], TD["position_threshold"], RD["fast_history"],
                                                    RD["clamp_sigma"], np.float32)[4], ref[4])[2] & d["valid"]
        assert (T[..., 3][keep & d["clamped"]] == np.minimum(3, F[..., 3])[keep & d["clamped"]]).all() and (T[..., 3][keep & ~d["clamped"]] == 3).all()
        lit = np.zeros((h, w), bool)
        lit[:, w // 2:] = True
        share = [float(d["clamped"][keep & m].mean()) for m in (lit, ~lit)]
        print(f"clamped on the first frame after the change: {share[0]:.3f} of the lit half, {share[1]:.3f} of the untouched half")
        assert (T[..., 3][keep & ~lit] == 3).mean() > 0.5 and d["clamped"][keep & lit].sum() > 20


@pytest.mark.gpu
def test_synthetic_frames_with_markers_and_a_hot_pixel(pkg):
    frames = _frames(pkg, "67x45", "subpixel", synthetic=True)
    b = _handle(pkg, W, H)
    got = _replay(b, frames)
    b.close()
    _compare([f for f, _ in frames], got, "synthetic subpixel")
    for T, F, _ in got:
        assert np.isnan(T[2, 3, 0]) and np.isposinf(T[4, 5, 1]) and T[2, 3, 3] == 0 and T[4, 5, 3] == 0
        assert not F[2, 3].any() and not F[4, 5].any()
        rest = np.ones((H, W), bool)
        rest[2, 3] = rest[4, 5] = False
        assert np.isfinite(T[rest]).all() and np.isfinite(F).all()  # the markers keep to themselves


def _motion_frames(pkg, w, h):
    """animated_test across one ptx_update_animation with tracking on: two frames at time 0, the update, two more; synthetic sums
    with the lighting step; the device's own guides and motion guides, read back"""
    key = ("motion", w, h)
    if key not in _frames_cache:
        import torch  # noqa: F401

        s = pkg.Scene("animated_test", DETAIL)
        r = pkg.Renderer()
        r.upload(s)
        r.track_motion(True)
        r.resize(w, h)
        view, proj = s.camera_matrices(w, h)
        out, states = [], []
        for f in range(4):
            if f == 2:
                assert s.update(0.37)
                r.update_animation(*s.animation_state())
            states.append(s.animation_state() if f >= 2 else None)
            u = s.uniform(w, h, bounces=4, sample_count=1, total_samples=f)
            r.render_guides_motion(u)
            g = [r.read_guide(k) for k in range(3)] + [r.read_motion(k) for k in range(2)]
            S = _shadow(_synthetic_sum(h, w, g[2], 50 + f, markers=False), f)
            r.write_accumulation(S)
            r.temporal_accumulate_motion(1, view, proj, **TD)  # moves the history's pose along, as the runs under test will
            out.append(((S, g[0], g[1], g[2], 1, view, proj, 0, g[3], g[4]), u))
        r.close()
        _frames_cache[key] = (out, states)
    return _frames_cache[key]


def _motion_replay(pkg, w, h, rflags, base=False, rd=RD):
    frames, states = _motion_frames(pkg, w, h)
    s = pkg.Scene("animated_test", DETAIL)
    r = pkg.Renderer()
    r.upload(s)
    r.track_motion(True)
    r.resize(w, h)
    out = []
    for k, (frame, u) in enumerate(frames):
        if k == 2:
            r.update_animation(*states[k])
        r.write_accumulation(frame[0])
        r.render_guides_motion(u)
        for which in range(2):
            assert (_bits(r.read_motion(which)) == _bits(frame[8 + which])).all()
        if base:
            _base_call(r, frame, rflags)
        else:
            _call(r, frame, rflags, rd=rd)
        out.append(_read(r, rflags, fast=not base))
    r.close()
    return frames, out


@pytest.mark.gpu
@pytest.mark.parametrize("rflags", [RR.MOTION, RR.MOTION | RR.MOMENTS])
def test_motion_sequences_against_float64_reference(pkg, rflags):
    frames, got = _motion_replay(pkg, W, H, rflags)
    _, _, clamped, ref = _compare([f for f, _ in frames], got, "animated_test flags %d" % rflags, rflags)
    moved = (_bits(frames[2][0][8][..., 0:3]) != _bits(frames[2][0][2][..., 0:3])).any(axis=-1) & (frames[2][0][8][..., 3] == 1)
    print(f"animated_test: {int(moved.sum())} pixels moved, of them {int((got[2][0][..., 3][moved] > 1).sum())} kept their history; clamped {clamped}")
    assert moved.sum() > 20 and (got[2][0][..., 3][moved] > 1).sum() > 10 and clamped > 100


@pytest.mark.gpu
@pytest.mark.parametrize("rflags", [0, RR.MOMENTS, RR.MOTION, RR.MOTION | RR.MOMENTS])
def test_a_box_never_left_is_the_base_call_bit_for_bit(pkg, rflags):
    """clampSigma 1e30: T and the read-back histories are the base call's on a fresh handle; with fastHistory == maxHistory as well,
    F is the colour history: float32(F max(albedo, 0.01)) == T.rgb and L_F == T.w"""
    same = dict(fast_history=TD["max_history"], clamp_sigma=NEVER)
    if rflags & RR.MOTION:
        frames, base = _motion_replay(pkg, W, H, rflags, base=True)
        runs = [_motion_replay(pkg, W, H, rflags, rd=rd)[1] for rd in (dict(RD, clamp_sigma=NEVER), same)]
    else:
        frames = _frames(pkg, "67x45", "turn_dolly")
        handles = [_handle(pkg, W, H) for _ in range(3)]
        base = _replay(handles[0], frames, rflags, base=True)
        runs = [_replay(hd, frames, rflags, rd=rd) for hd, rd in zip(handles[1:], (dict(RD, clamp_sigma=NEVER), same))]
        for hd in handles:
            hd.close()
    for run in runs:
        for k, ((T, F, M), (Tb, _, Mb)) in enumerate(zip(run, base)):
            assert (_bits(T) == _bits(Tb)).all(), (rflags, k)
            if rflags & RR.MOMENTS:
                assert (_bits(M) == _bits(Mb)).all(), (rflags, k)
    assert (base[-1][0][..., 3] > 2).sum() > 200
    for k, (T, F, _) in enumerate(runs[1]):
        a = np.maximum(frames[k][0][3][..., 0:3], np.float32(0.01))
        valid = T[..., 3] > 0
        assert (_bits(F[..., 0:3] * a)[valid] == _bits(T[..., 0:3])[valid]).all() and (_bits(F[..., 3]) == _bits(T[..., 3])).all(), (rflags, k)


@pytest.mark.gpu
def test_first_and_reset_calls_and_sequences_separated_by_reset(pkg):
    frames = _frames(pkg, "67x45", "turn_dolly")
    r, b = _handle(pkg, W, H), _handle(pkg, W, H)
    flags = [0, 0, pkg.TEMPORAL_RESET, 0, 0]
    own = _replay(r, frames, flags=flags)
    base = _replay(b, frames, flags=flags, base=True)
    for k in (0, 2):  # a first call and a RESET call are the base call's
        assert (_bits(own[k][0]) == _bits(base[k][0])).all() and (own[k][0][..., 3] <= 1).all()
        valid = own[k][0][..., 3] > 0
        assert (own[k][1][..., 3][valid] == 1).all() and not own[k][1][~valid].any()
    r.close()
    b.close()
    for seq, want in ((frames[0:2], own[0:2]), (frames[2:5], own[2:5])):  # two sequences on one handle are two fresh handles'
        f = _handle(pkg, W, H)
        for a, c in zip(_replay(f, seq), want):
            assert (_bits(a[0]) == _bits(c[0])).all() and (_bits(a[1]) == _bits(c[1])).all()
        f.close()
    assert (own[4][0][..., 3] > 1).any() and any((_bits(o[0]) != _bits(p[0])).any() for o, p in zip(own, base))


@pytest.mark.gpu
def test_a_plain_call_in_between_drops_the_fast_history(pkg):
    frames = _frames(pkg, "67x45", "subpixel")
    r = _handle(pkg, W, H)
    lib, buf = r.lib, np.zeros((H, W, 4), np.float32)
    assert lib.ptx_read_fast_history(r.handle, buf.ctypes.data, buf.nbytes) == 5 and not r.fast_history_ptr()
    got = _replay(r, frames[0:2])
    (frame, u) = frames[2]
    r.write_accumulation(frame[0])
    r.render_guides(u)
    _base_call(r, frame)
    plain = r.read_temporal()
    assert lib.ptx_read_fast_history(r.handle, buf.ctypes.data, buf.nbytes) == 5 and not buf.any() and not r.fast_history_ptr()
    after = _replay(r, frames[3:4])[0]
    valid = after[0][..., 3] > 0
    assert valid.sum() > 200 and (after[1][..., 3][valid] == 1).all() and (after[0][..., 3] > 2).any()  # F restarts, the colour history stands
    r.close()
    want = [g for g in got] + [(plain, None, None), after]
    _compare([f for f, _ in frames[0:4]], want, "plain call in between", plain=(2,))


@pytest.mark.gpu
def test_the_filters_follow_unchanged_and_the_path_tracer_does_not_notice(pkg):
    s, main = _gpu(pkg)
    frames = _frames(pkg, "67x45", "subpixel")
    r = _handle(pkg, W, H)
    T, F, M = _replay(r, frames[0:4], RR.MOMENTS)[-1]
    S, u = frames[3][0][0], frames[3][1]
    f = _handle(pkg, W, H)  # ptx_denoise_temporal: a borrower's ptx_denoise on a copy of T
    f.write_accumulation(T)
    f.render_guides(u)
    for params in ((3, 0.5, 0.3, 0.03), (1, 1.5, 0.5, 0.02)):
        r.denoise_temporal(*params)
        f.denoise(1, *params)
        assert (_bits(r.read_denoised()) == _bits(f.read_denoised())).all(), params
    g = _handle(pkg, W, H)  # ptx_denoise_variance: no call writes a moment history, so the copy of T and of the moments is a second run's
    for x, y in zip(_replay(g, frames[0:4], RR.MOMENTS)[-1], (T, F, M)):
        assert (_bits(x) == _bits(y)).all()
    r.denoise_variance()
    g.denoise_variance()
    D = r.read_denoised()
    assert (_bits(D) == _bits(g.read_denoised())).all() and (_bits(r.read_variance()) == _bits(g.read_variance())).all() and (D[..., 3] == 1).all()
    # ... and against calls that are not the responsive one: under a box that is never left T and the moments are the plain moments
    # call's, and the filter behind them gives what it gives behind that call on another handle
    v, q = _handle(pkg, W, H), _handle(pkg, W, H)
    Tv, _, Mv = _replay(v, frames[0:4], RR.MOMENTS, rd=dict(RD, clamp_sigma=NEVER))[-1]
    Tq, _, Mq = _replay(q, frames[0:4], RR.MOMENTS, base=True)[-1]
    assert (_bits(Tv) == _bits(Tq)).all() and (_bits(Mv) == _bits(Mq)).all()
    for params in ((3, 0.75, 0.3, 0.03), (1, 1.5, 0.5, 0.02)):
        v.denoise_variance(*params)
        q.denoise_variance(*params)
        assert (_bits(v.read_denoised()) == _bits(q.read_denoised())).all() and (_bits(v.read_variance()) == _bits(q.read_variance())).all(), params
    v.close()
    q.close()
    # every image is an input to the filters
    assert (_bits(r.read_temporal()) == _bits(T)).all() and (_bits(r.read_moments()) == _bits(M)).all() and (_bits(r.read_fast_history()) == _bits(F)).all()
    assert (_bits(r.readback()) == _bits(S)).all()
    for k in range(3):
        assert (_bits(r.read_guide(k)) == _bits(frames[3][0][1 + k])).all()
    for hd in (r, f, g):
        hd.close()
    # the next ptx_render continues the sum as if nothing had happened
    main.set_tile_shard(0, 1, 32)
    main.resize(W, H)
    s.set_camera_pose(*_poses(pkg, s, "still", W, H)[0])
    up = s.uniform(W, H, bounces=4)

    def path_traced(n):
        main.reset()
        for k in range(n):
            up.TotalSamples = k
            main.render(up, s.lights)
        return main.readback()
    two, three = path_traced(2), path_traced(3)
    path_traced(2)
    main.render_guides(up)
    view, proj = s.camera_matrices(W, H)
    for _ in range(2):
        main.temporal_accumulate_responsive(2, view, proj, **TD, **RD)
    assert (_bits(main.readback()) == _bits(two)).all()
    up.TotalSamples = 2
    main.render(up, s.lights)
    assert (_bits(main.readback()) == _bits(three)).all()


@pytest.mark.gpu
def test_resize_and_refusals_leave_everything_intact(pkg):
    import torch

    s, main = _gpu(pkg)
    frames = _frames(pkg, "67x45", "subpixel")
    r = pkg.Renderer()  # an owner of its own: tile shards and bound buffers are refused on it
    r.upload(s)
    r.resize(W, H)
    lib = r.lib
    T, F, M = _replay(r, frames[0:2], RR.MOMENTS)[-1]
    r.denoise_variance()
    D = r.read_denoised()
    frame = frames[2][0]

    def desc(mh=3.0, flags=0):
        d = pkg.TemporalDesc()
        d.View[:], d.Proj[:] = [float(v) for v in frame[5]], [float(v) for v in frame[6]]
        d.totalSamples, d.maxHistory, d.normalThreshold, d.positionThreshold, d.flags, d.reserved = 1, mh, 0.3, 0.03, flags, 0
        return d

    def rdesc(fh=2.0, cs=1.5, flags=1, reserved=0):
        return pkg.ResponsiveDesc(fh, cs, flags, reserved)

    def call(d, rd):
        return lib.ptx_temporal_accumulate_responsive(r.handle, None if d is None else C.byref(d), None if rd is None else C.byref(rd))

    def intact():
        assert (_bits(r.read_temporal()) == _bits(T)).all() and (_bits(r.read_fast_history()) == _bits(F)).all() and (_bits(r.read_moments()) == _bits(M)).all()
        assert (_bits(r.read_denoised()) == _bits(D)).all()

    nan, inf = float("nan"), float("inf")
    for rd in (rdesc(fh=0.5), rdesc(fh=0.0), rdesc(fh=nan), rdesc(fh=inf), rdesc(fh=3.5), rdesc(cs=0.0), rdesc(cs=-1.0), rdesc(cs=nan), rdesc(cs=inf),
               rdesc(flags=4), rdesc(flags=0x80000001), rdesc(reserved=1)):
        assert call(desc(), rd) == 1, (rd.fastHistory, rd.clampSigma, rd.flags, rd.reserved)
    assert call(desc(), None) == 1 and call(None, rdesc()) == 1 and call(desc(mh=0.5), rdesc(fh=0.5)) == 1 and call(desc(flags=2), rdesc()) == 1
    assert lib.ptx_temporal_accumulate_responsive(None, C.byref(desc()), C.byref(rdesc())) == 1
    buf = np.zeros((H, W, 4), np.float32)
    assert lib.ptx_read_fast_history(r.handle, None, buf.nbytes) == 1
    assert lib.ptx_read_fast_history(r.handle, buf.ctypes.data, buf.nbytes + 16) == 1 and lib.ptx_read_fast_history(r.handle, buf.ctypes.data, buf.nbytes - 16) == 1
    assert not buf.any()
    intact()
    # the base call's refusals, with its codes: stale motion guides, a tile shard of a larger world, a bound shard buffer
    assert call(desc(), rdesc(flags=2)) == 5 and call(desc(), rdesc(flags=3)) == 5
    r.set_tile_shard(0, 2, 8)
    assert call(desc(), rdesc()) == 5
    shard = torch.zeros(r.shard_bytes(0) // 4, dtype=torch.float32, device="cuda")
    r.bind_shard_accumulation(shard.data_ptr(), r.shard_bytes(0))
    assert call(desc(), rdesc()) == 5
    r.bind_shard_accumulation(0)
    r.set_tile_shard(0, 1, 32)
    intact()
    fresh = pkg.Renderer()
    rd, d = rdesc(), desc()
    assert lib.ptx_temporal_accumulate_responsive(fresh.handle, C.byref(d), C.byref(rd)) == 5  # no image
    fresh.share_scene(r)
    fresh.resize(W, H)
    assert lib.ptx_temporal_accumulate_responsive(fresh.handle, C.byref(d), C.byref(rd)) == 5  # no guides
    assert lib.ptx_read_fast_history(fresh.handle, buf.ctypes.data, buf.nbytes) == 5 and not lib.ptx_device_fast_history_ptr(fresh.handle)
    fresh.close()
    # the histories are intact as well: the third frame gives what a handle that never saw a refusal gives
    third = _replay(r, frames[2:3], RR.MOMENTS)[0]
    b = _handle(pkg, W, H)
    want = _replay(b, frames[0:3], RR.MOMENTS)[-1]
    b.close()
    for x, y in zip(third, want):
        assert (_bits(x) == _bits(y)).all()
    assert (third[0][..., 3] > 1).any()
    # ptx_resize drops everything
    r.resize(W, H)
    assert lib.ptx_read_fast_history(r.handle, buf.ctypes.data, buf.nbytes) == 5 and not r.fast_history_ptr() and not r.temporal_ptr()
    again = _replay(r, frames[2:3], RR.MOMENTS)[0]
    valid = again[0][..., 3] > 0
    assert (again[0][..., 3] <= 1).all() and (again[1][..., 3][valid] == 1).all()
    r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("variance", [0, 1])
def test_renderer_hip_with_responsive_on_is_the_same_calls_made_by_hand(pkg, tmp_path_factory, tmp_path, variance):
    """test_motion's driver (examples/motion_frame.cpp, compiled once per session) with TemporalSettings::Responsive on as well: two
    frames of animated_test through RendererHip, the pose moved in between.  The sum, T and the output image of both frames equal
    ptx_render_guides_motion, ptx_temporal_accumulate_responsive with PTX_RESPONSIVE_MOTION (and MOMENTS) at the adapter's defaults,
    the filter and the output stage called by hand, bit for bit; the second frame has a history, and the clamp changed it."""
    import subprocess

    import test_motion as TM

    w, h, spp, depth, step = W, H, 2, 4, 0.37
    exe = TM._motion_frame_driver(pkg, tmp_path_factory)
    dump = tmp_path / "frames.bin"
    subprocess.check_call([exe, "animated_test", str(w), str(h), str(spp), str(depth), str(step), str(variance), str(dump), "1"])
    got = np.fromfile(dump, np.float32).reshape(2, 3, h, w, 4)
    host = open(os.path.join(pkg.PKG_DIR, "host", "RendererHip.h")).read()
    assert re.search(r"bool Responsive = false;\s*float FastHistory = 2\.0f;\s*float ClampSigma = 1\.0f;", host)
    assert pkg.RESPONSIVE_DEFAULTS == dict(fast_history=2.0, clamp_sigma=1.0)
    rflags = RR.MOTION | (RR.MOMENTS if variance else 0)
    s = pkg.Scene("animated_test", DETAIL)
    s.update(0.0)
    runs = []
    for responsive in (True, False):
        r = pkg.Renderer()
        r.upload(s) if responsive else r.share_scene(runs[0][0])
        if responsive:
            r.track_motion(True)
        r.resize(w, h)
        runs.append((r, []))
    owner, base = runs[0][0], runs[1][0]
    for frame in range(2):
        if frame:
            assert s.update(step)
        it, bn = s.animation_state()
        owner.update_animation(it, bn if len(bn) else None)
        for r, out in runs:
            r.reset()
            for f in range(spp):
                r.render(s.uniform(w, h, bounces=depth, sample_count=1, total_samples=f), s.lights)
            r.render_guides_motion(s.uniform(w, h, bounces=depth, sample_count=1, total_samples=spp))
            view, proj = s.camera_matrices(w, h)
            if r is owner:
                r.temporal_accumulate_responsive(spp, view, proj, responsive_flags=rflags)  # TEMPORAL_DEFAULTS, RESPONSIVE_DEFAULTS
            else:
                r.temporal_accumulate_motion(spp, view, proj, moments=bool(variance))
            if variance:
                r.denoise_variance(iterations=3, sigma_luminance=0.75, sigma_normal=0.3, sigma_position=0.03)
            else:
                r.denoise_temporal(iterations=3, sigma_color=1.5, sigma_normal=0.3, sigma_position=0.03)
            r.postprocess_denoised(spp, 1.0, 1.0, 1.0, pkg.TONE_MAPPING_SDR)
            out.append((r.readback(), r.read_temporal(), r.read_output(pkg.OUTPUT_RGBA32F)))
        differ = [int((_bits(a) != _bits(b)).any(axis=-1).sum()) for a, b in zip(got[frame], runs[0][1][frame])]
        print(f"variance {variance} frame {frame}: pixels differing in the sum, T and the output image {differ}")
        assert differ == [0, 0, 0], (variance, frame)
    T1, plain1 = runs[0][1][1][1], runs[1][1][1][1]
    assert (_bits(runs[0][1][0][1]) == _bits(runs[1][1][0][1])).all()  # a first frame is the base call's
    changed = (_bits(T1) != _bits(plain1)).any(axis=-1)
    print(f"second frame: {int((T1[..., 3] > 1).sum())} pixels with a history, {int(changed.sum())} differ from the base call's")
    assert (plain1[..., 3] == 2).sum() > 200 and changed.sum() > 20
    base.close()
    owner.close()
