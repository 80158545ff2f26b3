"""The temporal accumulation (include/ptx.h ptx_temporal_accumulate, docs/NEXT_ROWS.md section 14) restated in numpy from the
header's text, generic over float32 / float64.  Nothing here is derived from the kernel.

    m(p) = S(p).rgb / totalSamples;  a_p = max(albedo_p, 0.01) per channel;  c(p) = m(p) / a_p
    valid p: hit (normal.w == 1), m(p) finite, n_p finite, t_p = position.w > 0 and finite
    history (of the previous call): H, L', N', X' per pixel, View', Proj'
    for a valid p with a history and without RESET
        clip = Proj' (View' (x_p, 1));  none if clip.w <= 0 or u or v is not finite
        u = (clip.x / clip.w 0.5 + 0.5) W - 0.5,  v = (clip.y / clip.w 0.5 + 0.5) H - 0.5
        (View', Proj') == (View, Proj) bit for bit: one tap of weight 1 at p itself, no projection
        taps (x0 + i, y0 + j), x0 = floor(u), y0 = floor(v), bilinear weights; a tap q counts if it is inside, L'(q) > 0, H(q) is
        finite, |n_p - N'(q)|^2 <= normalThreshold^2 and |dot(n_p, X'(q) - x_p)| <= positionThreshold t_p
        found iff sum w >= 1/64;  c_h = sum w H / sum w, L_h = sum w L' / sum w, L = min(L_h + 1, maxHistory),
        c_acc = c_h + (c - c_h) / L
    otherwise c_acc = c, L = 1
    T = (c_acc a, L) on valid pixels, (m, 0) elsewhere; the next history is c_acc, L (0 where not valid), n, x
"""
import numpy as np

import denoise_ref as R

RESET = 1
FOUND_FLOOR = 1.0 / 64.0


class History:
    """What one call leaves for the next, in the reference's own number format"""

    def __init__(self, c, L, n, x, view, proj):
        self.c, self.L, self.n, self.x = c, L, n, x
        self.view, self.proj = np.array(view, np.float32).reshape(16), np.array(proj, np.float32).reshape(16)


def _mul(m, x, y, z, w):
    """M (x, y, z, w) for a column-major M, summed left to right"""
    return [((m[i] * x + m[4 + i] * y) + m[8 + i] * z) + m[12 + i] * w for i in range(4)]


def project(view, proj, x, width, height, dtype):
    """(u, v, ok) of the world points x (..., 3) in the camera (view, proj): pixel coordinates with centres at integers"""
    view, proj = [dtype(f) for f in np.asarray(view, np.float32).reshape(16)], [dtype(f) for f in np.asarray(proj, np.float32).reshape(16)]
    with np.errstate(all="ignore"):
        e = _mul(view, x[..., 0], x[..., 1], x[..., 2], dtype(1))
        cl = _mul(proj, *e)
        u = (cl[0] / cl[3] * dtype(0.5) + dtype(0.5)) * dtype(width) - dtype(0.5)
        v = (cl[1] / cl[3] * dtype(0.5) + dtype(0.5)) * dtype(height) - dtype(0.5)
        ok = (cl[3] > 0) & np.isfinite(u) & np.isfinite(v)
    return u, v, ok


def accumulate(S, normal, position, albedo, total_samples, view, proj, history, max_history, normal_threshold, position_threshold, flags=0,
               dtype=np.float64):
    """One call: (T as an (H, W, 4) array of `dtype`, the next History, decisions).  `decisions` holds what the call decided per pixel:
    'cell' (H, W, 2) the texel (x0, y0) the gather started from (-2^31 where nothing was projected), 'taps' (H, W, 4) which taps
    counted (the same-camera rule has tap 0 alone, at p), 'found' (H, W), 'valid' (H, W), and for the call as a whole 'used_history'
    and 'same_camera'."""
    assert total_samples > 0 and max_history >= 1 and normal_threshold > 0 and position_threshold > 0 and flags in (0, RESET)
    h, w = np.asarray(S).shape[:2]
    m = R.mean_of(S, total_samples, dtype)
    valid = R.valid_mask(S, normal, position, total_samples, dtype)
    n = np.asarray(normal, np.float32)[..., 0:3].astype(dtype)
    x = np.asarray(position, np.float32)[..., 0:3].astype(dtype)
    t = np.asarray(position, np.float32)[..., 3].astype(dtype)
    a = np.maximum(np.asarray(albedo, np.float32)[..., 0:3].astype(dtype), dtype(np.float32(R.ALBEDO_FLOOR)))
    view, proj = np.array(view, np.float32).reshape(16), np.array(proj, np.float32).reshape(16)
    nt2 = dtype(np.float32(normal_threshold)) * dtype(np.float32(normal_threshold))
    pt = dtype(np.float32(position_threshold))
    cell = np.full((h, w, 2), -2 ** 31, np.int64)
    taps = np.zeros((h, w, 4), bool)
    found = np.zeros((h, w), bool)
    used, same = history is not None and not (flags & RESET), False
    with np.errstate(all="ignore"):
        c = np.where(valid[..., None], m / a, m)
        c_acc, L = c.copy(), np.where(valid, dtype(1), dtype(0))
        if used:
            assert history.c.dtype == np.dtype(dtype) and history.c.shape == (h, w, 3)
            same = bool((history.view.view(np.uint32) == view.view(np.uint32)).all() and (history.proj.view(np.uint32) == proj.view(np.uint32)).all())
            yy, xx = np.mgrid[0:h, 0:w]
            if same:
                candidates = [(yy, xx, np.ones((h, w), dtype), valid)]
            else:
                u, v, ok = project(history.view, history.proj, x, w, h, dtype)
                ok &= valid
                x0f, y0f = np.floor(u), np.floor(v)
                fx, fy = u - x0f, v - y0f
                # what lies outside the image by more than a texel has no tap inside it: keep the integers small
                ok &= (x0f >= -1) & (x0f <= w) & (y0f >= -1) & (y0f <= h)
                x0, y0 = np.where(ok, x0f, -2 ** 31).astype(np.int64), np.where(ok, y0f, -2 ** 31).astype(np.int64)
                cell[..., 0], cell[..., 1] = x0, y0
                candidates = []
                for j in (0, 1):
                    for i in (0, 1):
                        qx, qy = x0 + i, y0 + j
                        inside = ok & (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
                        wgt = (fx if i else dtype(1) - fx) * (fy if j else dtype(1) - fy)
                        candidates.append((np.where(inside, qy, 0), np.where(inside, qx, 0), wgt, inside))
            num, lnum, den = np.zeros((h, w, 3), dtype), np.zeros((h, w), dtype), np.zeros((h, w), dtype)
            for k, (qy, qx, wgt, inside) in enumerate(candidates):
                Hq, Lq, Nq, Xq = history.c[qy, qx], history.L[qy, qx], history.n[qy, qx], history.x[qy, qx]
                dn = n - Nq
                plane = (n * (Xq - x)).sum(axis=-1)
                counts = inside & (Lq > 0) & np.isfinite(Hq).all(axis=-1) & ((dn * dn).sum(axis=-1) <= nt2) & (np.abs(plane) <= pt * t)
                taps[..., k] = counts
                wk = np.where(counts, wgt, dtype(0))
                num = num + wk[..., None] * np.where(counts[..., None], Hq, dtype(0))
                lnum = lnum + wk * np.where(counts, Lq, dtype(0))
                den = den + wk
            found = valid & (den >= dtype(FOUND_FLOOR))
            safe = np.where(found, den, dtype(1))
            c_h, L_h = num / safe[..., None], lnum / safe
            L_new = np.minimum(L_h + dtype(1), dtype(np.float32(max_history)))
            blended = c_h + (c - c_h) / np.where(found, L_new, dtype(1))[..., None]
            c_acc = np.where(found[..., None], blended, c)
            L = np.where(found, L_new, L)
        T = np.zeros((h, w, 4), dtype)
        T[..., 0:3] = np.where(valid[..., None], c_acc * a, m)
        T[..., 3] = L
    assert T.dtype == np.dtype(dtype) and c_acc.dtype == np.dtype(dtype) and L.dtype == np.dtype(dtype)
    nxt = History(np.where(valid[..., None], c_acc, dtype(0)), L, n, x, view, proj)
    return T, nxt, {"cell": cell, "taps": taps, "found": found, "valid": valid, "used_history": used, "same_camera": same}


def same_decisions(d32, d64):
    """(H, W) bool: the pixels on which two runs of the reference took every accept / found decision alike"""
    return (d32["cell"] == d64["cell"]).all(axis=-1) & (d32["taps"] == d64["taps"]).all(axis=-1) & (d32["found"] == d64["found"]) & (d32["valid"] == d64["valid"])


def run_sequence(frames, max_history, normal_threshold, position_threshold, dtype):
    """frames: [(S, normal, position, albedo, total_samples, view, proj, flags)].  Returns ([T], [decisions]) of one history chain."""
    hist, out, dec = None, [], []
    for S, nrm, pos, alb, n, view, proj, flags in frames:
        T, hist, d = accumulate(S, nrm, pos, alb, n, view, proj, hist, max_history, normal_threshold, position_threshold, flags, dtype)
        out.append(T)
        dec.append(d)
    return out, dec


# ---- a small camera of the test's own: forward matrices in the convention of the header (column-major, w = view depth) ------------

def look_at(eye, target, up=(0.0, 1.0, 0.0)):
    eye, target, up = np.float64(eye), np.float64(target), np.float64(up)
    f = target - eye
    f /= np.linalg.norm(f)
    s = np.cross(up, f)
    s /= np.linalg.norm(s)
    u = np.cross(f, s)
    m = np.eye(4)
    m[0, 0:3], m[1, 0:3], m[2, 0:3] = s, u, f
    m[0, 3], m[1, 3], m[2, 3] = -s @ eye, -u @ eye, -f @ eye
    return np.float32(m.T.reshape(16))  # column-major


def perspective(fov_y, width, height, near=0.1, far=100.0):
    hh = 1.0 / np.tan(0.5 * fov_y)
    m = np.zeros((4, 4))
    m[0, 0], m[1, 1] = hh * height / width, hh
    m[2, 2], m[2, 3], m[3, 2] = far / (far - near), -far * near / (far - near), 1.0
    return np.float32(m.T.reshape(16))


def comparable_pixels(dec32, dec64):
    """Per frame of one history chain, the (H, W) mask of pixels on which a float32 implementation can be held to the float64
    reference: the two runs of the reference agree on every decision there, in this frame, and in the frames before it on every
    pixel this one's history came from (a pixel read through a tap that was itself left out is left out)."""
    out, prev = [], None
    for a, b in zip(dec32, dec64):
        keep = same_decisions(a, b)
        if b["used_history"] and prev is not None:
            h, w = keep.shape
            if b["same_camera"]:
                keep &= prev
            else:
                x0, y0 = b["cell"][..., 0], b["cell"][..., 1]
                for j in (0, 1):
                    for i in (0, 1):
                        qx, qy = x0 + i, y0 + j
                        inside = (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
                        keep &= ~inside | prev[np.where(inside, qy, 0), np.where(inside, qx, 0)]
        out.append(keep)
        prev = keep
    return out


# ---- the quality sequence shared by tools/temporal_quality.py and the quality test: a camera sliding sideways over a static scene ----

QUALITY_W, QUALITY_H, QUALITY_DETAIL, QUALITY_BOUNCES = 134, 90, 0.25, 4
QUALITY_FRAMES, QUALITY_SPP, QUALITY_TRUTH_SPP = 8, 4, 192
QUALITY_STEPS = {"default": 0.02, "texture_test": 0.05, "alpha_test": 0.05}  # the slide per frame, in scene units
QUALITY_TRUTH_FIRST_SAMPLE = 1000  # the truth's RNG frames start here: it shares no sample with the sequence


def scene_pose(scene, w, h):
    """(position, direction, right) of the scene's active camera, from the uniform it hands the renderer"""
    vi = np.frombuffer(scene.uniform(w, h).ViewInverse, np.float32).reshape(4, 4).T.astype(np.float64)
    return vi[0:3, 3], vi[0:3, 2], vi[0:3, 0]


def render_oracle_sum(orc, scene, w, h, spp, first):
    """One sample per launch, RNG frame = `first` + launch index, with the scene's camera as it stands"""
    osc = orc.OracleScene(scene.desc, build_bvh=True)
    acc = np.zeros((h, w, 4), np.float32)
    for f in range(first, first + spp):
        osc.render(scene.uniform(w, h, bounces=QUALITY_BOUNCES, sample_count=1, total_samples=f), scene.lights, w, h, accum=acc)
    return acc


def quality_sequence(pkg, orc, name, frames=QUALITY_FRAMES):
    """[(S, normal, position, albedo, spp, view, proj, 0)] of the sliding camera on scene `name`, rendered by the CPU oracle with
    first-hit guides from the debug view's reference; the scene is left at the last pose."""
    w, h = QUALITY_W, QUALITY_H
    scene = pkg.Scene(name, QUALITY_DETAIL)
    pos, fwd, right = scene_pose(scene, w, h)
    out = []
    for f in range(frames):
        scene.set_camera_pose(pos + right * (QUALITY_STEPS[name] * f), fwd)
        S = render_oracle_sum(orc, scene, w, h, QUALITY_SPP, f * QUALITY_SPP)
        view, proj = scene.camera_matrices(w, h)
        out.append((S, *R.cpu_guides(pkg, orc, scene, w, h), QUALITY_SPP, view, proj, 0))
    return scene, out
