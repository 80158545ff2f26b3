"""The responsive temporal history (include/ptx.h ptx_temporal_accumulate_responsive, docs/NEXT_ROWS.md section 19) restated in
numpy from the header's text, generic over float32 / float64.  Nothing here is derived from the kernels.

    pass A: the base call the flags name (temporal_ref.accumulate, motion_ref.accumulate_motion; with MOMENTS the moment history
        of variance_ref.accumulate) -- T, the colour history and every tap decision are its own -- and beside it the fast history
        F' = (F.rgb, L_F) along the same taps with the same weights:
        a colour tap q counts for F iff L_F'(q) > 0 and F'(q) is finite; found_F iff sum w_F >= 1/64:
        F_h = sum w F' / sum w_F, L_F = min(sum w L_F' / sum w_F + 1, fastHistory), F = F_h + (c - F_h) / L_F; else F = c, L_F = 1
        F not finite: zeros are stored, F is unknown (L_F = 0); a pixel that is not valid stores zeros
    pass B, on a valid p with L > 1, L_F(p) > 0 and c_acc finite:
        the 5 x 5 window of this call's F, a tap counts iff it is inside the image and L_F(q) > 0 (n >= 1: the centre)
        per channel, two passes row by row: mu = sum F / n, var = sum (F - mu)^2 / n, sigma = sqrt(var),
        lo = mu - clampSigma sigma, hi = mu + clampSigma sigma, c' = lo where c_acc < lo, hi where c_acc > hi, else c_acc
        clamped iff c_acc < lo or c_acc > hi in some channel: L_out = min(L, L_F), and with MOMENTS and L_M > 0, L_M = min(L_M, L_F)
        T = (c' a, L_out), the colour history's own entry (c', L_out)

Every clamp decision is reported per pixel ('clamped', 'acts', 'wtaps'), so that a float32 implementation is held to the float64
run only where the reference's own two runs decide alike (comparable_pixels)."""
import numpy as np

import denoise_ref as R
import temporal_ref as TR
import variance_ref as VR

MOMENTS, MOTION = 1, 2  # PTX_RESPONSIVE_*
HALO = 2  # the window is 5 x 5
OFFSETS = [(dy, dx) for dy in range(-HALO, HALO + 1) for dx in range(-HALO, HALO + 1)]

# ---- the lighting sequences of tools/temporal_quality.py --responsive and of the quality test: animated_test at time 0, a still camera,
# the geometry never updated, the point light moved along its own track (ExampleScenes.cpp: x from -1 to 2.5 at y = 3, z = -1).
# light_step: 8 frames with the light where the scene puts it, then 4 with it at the far end of the track; light_slide: 12 frames, one
# twelfth of the way further each, ending there too.  The truth is the oracle's 192 spp with the light at LIGHT_X_TO.
LIGHT_SCENE = "animated_test"
LIGHT_FRAMES, LIGHT_STEP_AT = 12, 8
LIGHT_X_FROM, LIGHT_X_TO = -1.0, 2.5
LIGHT_SEQUENCES = ("light_step", "light_slide")


class Fast:
    """The fast history in the reference's own number format: c (H, W, 3) and L (H, W)"""

    def __init__(self, c, L):
        self.c, self.L = c, L

    def image(self):
        out = np.zeros(self.L.shape + (4,), self.L.dtype)
        out[..., 0:3], out[..., 3] = self.c, self.L
        return out


def _candidates(d, history, x_lookup, w, h, dtype):
    """The taps the base call looked at, rebuilt from its decisions in its order and with its weights: [(qy, qx, weight)].  Slot k is
    d['taps'][..., k]; a pixel that took the tap at p under the same-camera rule has it in slot 0."""
    yy, xx = np.mgrid[0:h, 0:w]
    if d["same_camera"]:
        return [(yy, xx, np.ones((h, w), dtype))]
    with np.errstate(all="ignore"):
        u, v, _ = TR.project(history.view, history.proj, x_lookup, w, h, dtype)
        x0, y0 = d["cell"][..., 0], d["cell"][..., 1]
        ok = x0 != -2 ** 31
        fx, fy = u - np.floor(u), v - np.floor(v)
        at = d.get("at_pixel", np.zeros((h, w), bool))
        out = []
        for j in (0, 1):
            for i in (0, 1):
                qx, qy = x0 + i, y0 + j
                inside = ok & (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
                wgt = (fx if i else dtype(1) - fx) * (fy if j else dtype(1) - fy)
                qy, qx = np.where(inside, qy, 0), np.where(inside, qx, 0)
                if i == 0 and j == 0:
                    qy, qx, wgt = np.where(at, yy, qy), np.where(at, xx, qx), np.where(at, dtype(1), wgt)
                out.append((qy, qx, wgt))
    return out


def carry(prev, prev_L, cur, candidates, taps, valid, cap, dtype):
    """One more history along the colour's taps: `prev` (H, W, k) with the lengths prev_L (None: no such history), `cur` this frame's
    value.  Returns (values, L, the taps that counted (H, W, 4), found, known); unknown and not valid pixels hold zeros."""
    h, w, k = cur.shape
    mt, found = np.zeros((h, w, 4), bool), np.zeros((h, w), bool)
    with np.errstate(all="ignore"):
        out, L = cur.copy(), np.ones((h, w), dtype)
        if prev is not None:
            assert prev.dtype == np.dtype(dtype) and prev_L.dtype == np.dtype(dtype)
            num, ln, den = np.zeros((h, w, k), dtype), np.zeros((h, w), dtype), np.zeros((h, w), dtype)
            for s, (qy, qx, wgt) in enumerate(candidates):
                v, Lq = prev[qy, qx], prev_L[qy, qx]
                counts = taps[..., s] & (Lq > 0) & np.isfinite(v).all(axis=-1)
                mt[..., s] = counts
                wk = np.where(counts, wgt, dtype(0))
                num = num + wk[..., None] * np.where(counts[..., None], v, dtype(0))
                ln = ln + wk * np.where(counts, Lq, dtype(0))
                den = den + wk
            found = valid & (den >= dtype(TR.FOUND_FLOOR))
            safe = np.where(found, den, dtype(1))
            hv = num / safe[..., None]
            Lf = np.where(found, np.minimum(ln / safe + dtype(1), dtype(np.float32(cap))), dtype(1))
            out, L = np.where(found[..., None], hv + (cur - hv) / Lf[..., None], cur), Lf
        known = valid & np.isfinite(out).all(axis=-1)
        out, L = np.where(known[..., None], out, dtype(0)), np.where(known, L, dtype(0))
    assert out.dtype == np.dtype(dtype) and L.dtype == np.dtype(dtype)
    return out, L, mt, found, known


def clamp(c_acc, L, F, LF, valid, clamp_sigma, dtype):
    """Pass B on arrays of `dtype`: (c', L_out, decisions) with 'acts', 'clamped' (H, W) and 'wtaps' (H, W, 25) the window's taps that
    counted on the pixels pass B acts on, row-major over (dy, dx)."""
    h, w = L.shape
    ks = dtype(np.float32(clamp_sigma))
    with np.errstate(all="ignore"):
        acts = valid & (L > 1) & (LF > 0) & np.isfinite(c_acc).all(axis=-1)
        known = LF > 0
        wtaps = np.zeros((h, w, len(OFFSETS)), bool)
        total, n = np.zeros((h, w, 3), dtype), np.zeros((h, w), dtype)
        for k, (dy, dx) in enumerate(OFFSETS):
            counts = R._shift(known, dy, dx, False)
            wtaps[..., k] = counts & acts
            total = total + np.where(counts[..., None], R._shift(F, dy, dx, 0), dtype(0))
            n = n + np.where(counts, dtype(1), dtype(0))
        safe = np.where(n > 0, n, dtype(1))
        mu = total / safe[..., None]
        sq = np.zeros((h, w, 3), dtype)
        for dy, dx in OFFSETS:
            counts = R._shift(known, dy, dx, False)
            dev = R._shift(F, dy, dx, 0) - mu
            sq = sq + np.where(counts[..., None], dev * dev, dtype(0))
        sigma = np.sqrt(sq / safe[..., None])
        lo, hi = mu - ks * sigma, mu + ks * sigma
        below, above = acts[..., None] & (c_acc < lo), acts[..., None] & (c_acc > hi)
        clamped = (below | above).any(axis=-1)
        c_out = np.where(below, lo, np.where(above, hi, c_acc))
        L_out = np.where(clamped, np.minimum(L, LF), L)
    assert c_out.dtype == np.dtype(dtype) and L_out.dtype == np.dtype(dtype)
    return c_out, L_out, {"acts": acts, "clamped": clamped, "wtaps": wtaps, "below": below, "above": above}


def accumulate(S, normal, position, albedo, total_samples, view, proj, history, fast, moments, max_history, normal_threshold, position_threshold,
               fast_history, clamp_sigma, flags=0, responsive_flags=0, motion=None, dtype=np.float64):
    """One ptx_temporal_accumulate_responsive: (T, the next History, the next Fast, the next Moments or None, decisions).
    `history`, `fast`, `moments`: what the previous call left (None: none -- for `fast`, also after a call that was not responsive).
    `motion`: (X_prev, N_prev) of the motion guides under MOTION.  The decisions are the base call's plus 'ftaps', 'found_F',
    'known_F', with MOMENTS 'mtaps', 'found_M', 'known', and pass B's 'acts', 'clamped', 'wtaps'."""
    assert fast_history >= 1 and fast_history <= max_history and clamp_sigma > 0 and not (responsive_flags & ~(MOMENTS | MOTION))
    if responsive_flags & MOTION:
        import motion_ref as MR

        T, nxt, d = MR.accumulate_motion(S, normal, position, albedo, motion[0], motion[1], total_samples, view, proj, history, max_history,
                                         normal_threshold, position_threshold, flags, dtype)
        x_lookup = np.asarray(motion[0], np.float32)[..., 0:3].astype(dtype)
    else:
        T, nxt, d = TR.accumulate(S, normal, position, albedo, total_samples, view, proj, history, max_history, normal_threshold, position_threshold, flags, dtype)
        x_lookup = np.asarray(position, np.float32)[..., 0:3].astype(dtype)
    h, w = T.shape[:2]
    valid = d["valid"]
    m = R.mean_of(S, total_samples, dtype)
    a = np.maximum(np.asarray(albedo, np.float32)[..., 0:3].astype(dtype), dtype(np.float32(R.ALBEDO_FLOOR)))
    with np.errstate(all="ignore"):
        c = np.where(valid[..., None], m / a, m)
        cand = _candidates(d, history, x_lookup, w, h, dtype) if d["used_history"] else []
        use = d["used_history"]
        Fc, FL, ftaps, found_F, known_F = carry(fast.c if use and fast is not None else None, fast.L if use and fast is not None else None, c, cand, d["taps"],
                                                valid, fast_history, dtype)
        d = dict(d, ftaps=ftaps, found_F=found_F, known_F=known_F)
        mom = None
        if responsive_flags & MOMENTS:
            l = VR.lum(c, dtype)
            mu = np.stack([l, l * l], axis=-1)
            have = use and moments is not None
            M, ML, mtaps, found_M, known = carry(np.stack([moments.m1, moments.m2], axis=-1) if have else None, moments.L if have else None, mu, cand, d["taps"],
                                                 valid, max_history, dtype)
            d = dict(d, mtaps=mtaps, found_M=found_M, known=known)
        # pass B
        c_out, L_out, dec = clamp(nxt.c, nxt.L, Fc, FL, valid, clamp_sigma, dtype)
        d = dict(d, **dec)
        if responsive_flags & MOMENTS:
            ML = np.where(dec["clamped"] & (ML > 0), np.minimum(ML, FL), ML)
            mom = VR.Moments(M[..., 0], M[..., 1], ML)
        T = T.copy()
        T[..., 0:3] = np.where(valid[..., None], c_out * a, m)
        T[..., 3] = L_out
    nxt = TR.History(c_out, L_out, nxt.n, nxt.x, nxt.view, nxt.proj)
    assert T.dtype == np.dtype(dtype)
    return T, nxt, Fast(Fc, FL), mom, d


def run_sequence(frames, max_history, normal_threshold, position_threshold, fast_history, clamp_sigma, dtype, responsive_flags=0, plain=()):
    """frames as temporal_ref.run_sequence takes them, under MOTION with (X_prev, N_prev) appended to each; `plain`: the indices of the
    frames given to the base call alone, which drops the fast history.  Returns ([T], [History], [Fast or None], [Moments or None],
    [decisions])."""
    hist, fast, mom, out = None, None, None, ([], [], [], [], [])
    for k, frame in enumerate(frames):
        S, nrm, pos, alb, n, view, proj, flags = frame[0:8]
        motion = frame[8:10] if responsive_flags & MOTION else None
        if k in plain:
            assert not responsive_flags
            T, hist, d = TR.accumulate(S, nrm, pos, alb, n, view, proj, hist, max_history, normal_threshold, position_threshold, flags, dtype)
            fast = mom = None
        else:
            T, hist, fast, mom, d = accumulate(S, nrm, pos, alb, n, view, proj, hist, fast, mom, max_history, normal_threshold, position_threshold, fast_history,
                                               clamp_sigma, flags, responsive_flags, motion, dtype)
        for lst, v in zip(out, (T, hist, fast, mom, d)):
            lst.append(v)
    return out


_PASS_B = ("acts", "clamped", "wtaps", "below", "above")


def _same(a, b, keys):
    same = np.ones(b["valid"].shape, bool)
    for key in keys:
        if key in b:
            eq = a[key] == b[key]
            same &= eq if eq.ndim == 2 else eq.all(axis=-1)
    return same


def comparable_pixels(dec32, dec64):
    """Per frame the (H, W) mask of pixels on which a float32 implementation can be held to the float64 run: the two runs of the
    reference decide alike there, pass A's decisions are alike on every pixel of its 5 x 5 window (whose F sets the box), and in the
    frames before all of this holds on every pixel its history came from."""
    out, prev = [], None
    for a, b in zip(dec32, dec64):
        keep = TR.same_decisions(a, b) & _same(a, b, ("at_pixel", "found_F", "known_F", "found_M", "known", "ftaps", "mtaps"))
        if b["used_history"] and prev is not None:
            h, w = keep.shape
            if b["same_camera"]:
                keep &= prev
            else:
                if "at_pixel" in b:
                    keep &= ~b["at_pixel"] | prev
                x0, y0 = b["cell"][..., 0], b["cell"][..., 1]
                for j in (0, 1):
                    for i in (0, 1):
                        qx, qy = x0 + i, y0 + j
                        inside = (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
                        keep &= ~inside | prev[np.where(inside, qy, 0), np.where(inside, qx, 0)]
        if "acts" in b:  # pass B reads pass A's F of every window tap
            passA = keep.copy()
            keep &= _same(a, b, _PASS_B)
            for k, (dy, dx) in enumerate(OFFSETS):
                took = a["wtaps"][..., k] | b["wtaps"][..., k]
                keep &= ~took | R._shift(passA, dy, dx, True)
        out.append(keep)
        prev = keep
    return out


def light_position(pkg, scene_lights, x):
    """A copy of the scene's lights block with the first point light at x on its track"""
    import ctypes as C

    out = pkg.LightsUbo()
    C.memmove(C.byref(out), C.byref(scene_lights), C.sizeof(out))
    assert out.LightCount >= 1 and abs(out.Lights[0].Position[0] - LIGHT_X_FROM) < 1e-6, "the scene's light is not where the sequences start"
    out.Lights[0].Position[0] = float(x)
    return out


def light_x(kind, f):
    if kind == "light_step":
        return LIGHT_X_FROM if f < LIGHT_STEP_AT else LIGHT_X_TO
    return LIGHT_X_FROM + (LIGHT_X_TO - LIGHT_X_FROM) * (f + 1) / LIGHT_FRAMES


def light_scene(pkg, orc):
    """(scene, oracle scene, guides, view, proj): what the lighting sequences and their truth share"""
    w, h = TR.QUALITY_W, TR.QUALITY_H
    scene = pkg.Scene(LIGHT_SCENE, TR.QUALITY_DETAIL)
    return scene, orc.OracleScene(scene.desc, build_bvh=True), bind_pose_guides(pkg, orc, scene, w, h), *scene.camera_matrices(w, h)


def bind_pose_guides(pkg, orc, scene, w, h):
    """denoise_ref.cpu_guides for a scene with animated geometry that was never updated: the skinned block is the bind pose's"""
    import debug_view_ref as DV
    import motion_ref as MR

    u, dark = scene.uniform(w, h), R.dark_lights(pkg, scene.lights)
    rs = DV.RefScene(orc, scene.desc)
    nrm = DV.render(rs, u, dark, w, h, DV.MODE_NORMAL, 0, np.float32, MR.skinned_block(rs, None, np.float32))
    d, keep = R.without_emission(pkg, scene.desc)
    rs = DV.RefScene(orc, d)
    col = DV.render(rs, u, dark, w, h, DV.MODE_COLOR, DV.HIT_DISABLE_SHADOWS, np.float64, MR.skinned_block(rs, None, np.float64))
    g = [np.zeros((h, w, 4), np.float32) for _ in range(3)]
    g[0][..., 0:3], g[0][..., 3] = nrm["image"][..., 0:3], 1.0
    g[1][..., 0:3], g[1][..., 3] = nrm["position"], nrm["t"]
    with np.errstate(all="ignore"):
        g[2][..., 0:3], g[2][..., 3] = col["image"][..., 0:3] / 0.1, 1.0
    R.set_miss(g, ~nrm["hit"])
    return g


def render_lit(shared, pkg, x, spp, first):
    """The oracle's sum of `spp` samples, RNG frames from `first`, with the light at x"""
    scene, osc = shared[0], shared[1]
    w, h = TR.QUALITY_W, TR.QUALITY_H
    lights = light_position(pkg, scene.lights, x)
    acc = np.zeros((h, w, 4), np.float32)
    for f in range(first, first + spp):
        osc.render(scene.uniform(w, h, bounces=TR.QUALITY_BOUNCES, sample_count=1, total_samples=f), lights, w, h, accum=acc)
    return acc


def light_sequence(shared, pkg, kind):
    """[(S, normal, position, albedo, spp, view, proj, 0)] of one lighting sequence, 4 spp per frame"""
    _, _, guides, view, proj = shared
    return [(render_lit(shared, pkg, light_x(kind, f), TR.QUALITY_SPP, f * TR.QUALITY_SPP), *guides, TR.QUALITY_SPP, view, proj, 0) for f in range(LIGHT_FRAMES)]
