"""Variance-guided denoising (include/ptx.h ptx_temporal_accumulate_moments / ptx_denoise_variance, docs/NEXT_ROWS.md section 16)
restated in numpy from the header's text, generic over float32 / float64.  Nothing here is derived from the kernels.

    moments (beside temporal_ref.accumulate, whose T and colour history are untouched):
        l = (0.2126 c.x + 0.7152 c.y) + 0.0722 c.z of this frame's demodulated mean c, mu = (l, l l)
        a colour tap q counts for the moments iff L_M'(q) > 0 and mu1'(q), mu2'(q) are finite; found_M iff sum w_M >= 1/64:
        M_h = sum w mu' / sum w_M, L_M = min(sum w L_M' / sum w_M + 1, maxHistory), M = M_h + (mu - M_h) / L_M; else M = mu, L_M = 1
        M not finite: (0, 0, 0) is stored, the moments are unknown; a pixel that is not valid stores zeros
    estimate (valid: the denoiser's with m = T.rgb):
        L_M(p) >= 4: v = mu2 - mu1 mu1; else a 7 x 7 window of the taps inside, valid and with L_M(q) > 0,
        w = exp(-(|n_p - n_q|^2 / sigmaNormal^2 + (dot(n_p, x_q - x_p) / (sigmaPosition t_p))^2)), the centre with w = 1 iff known,
        m1 = sum w mu1 / sum w, m2 = sum w mu2 / sum w, v = m2 - m1 m1, sum w = 0: v = 0;  V_0 = v if finite and > 0 else 0
    filter, iteration i, s = 2^i, valid p:
        vt = 3 x 3 mean of V_i, weights 1/4, 1/8, 1/16 over the taps inside and valid, over the weights that count
        taps as the denoiser's; d = |lum c_i(p) - lum c_i(q)|, e_l = 0 if d = 0, no tap if d > 0 and vt = 0, else d^2 / (sigmaLuminance^2 vt)
        w = h h exp(-(e_l + normal term + position term)); c_{i+1} = sum w c_i / sum w; V_{i+1} = sum w^2 V_i / (sum w)^2
    D = c_N a on valid pixels, m elsewhere; alpha 1

Every function reports what it decided per pixel, so that a float32 implementation is held to the float64 run only where the
reference's own two runs decide alike (comparable_*)."""
import numpy as np

import denoise_ref as R
import temporal_ref as TR

LUM = (0.2126, 0.7152, 0.0722)
LONG_HISTORY = 4.0
WINDOW = 3  # the estimate's window is 7 x 7
G3 = (0.25, 0.5, 0.25)  # the prefilter: 1/4 centre, 1/8 edges, 1/16 corners


def lum(c, dtype):
    k = [dtype(np.float32(v)) for v in LUM]
    return (k[0] * c[..., 0] + k[1] * c[..., 1]) + k[2] * c[..., 2]


class Moments:
    """The moment history in the reference's own number format: (H, W) arrays"""

    def __init__(self, m1, m2, L):
        self.m1, self.m2, self.L = m1, m2, L

    def image(self):
        out = np.zeros(self.m1.shape + (4,), self.m1.dtype)
        out[..., 0], out[..., 1], out[..., 2] = self.m1, self.m2, self.L
        return out


def _colour_candidates(history, view, proj, x, valid, w, h, dtype):
    """The taps temporal_ref.accumulate looked at, in its order and with its weights: [(qy, qx, weight, inside)]"""
    view, proj = np.array(view, np.float32).reshape(16), np.array(proj, np.float32).reshape(16)
    same = bool((history.view.view(np.uint32) == view.view(np.uint32)).all() and (history.proj.view(np.uint32) == proj.view(np.uint32)).all())
    yy, xx = np.mgrid[0:h, 0:w]
    if same:
        return [(yy, xx, np.ones((h, w), dtype), valid)]
    with np.errstate(all="ignore"):
        u, v, ok = TR.project(history.view, history.proj, x, w, h, dtype)
        ok &= valid
        x0f, y0f = np.floor(u), np.floor(v)
        fx, fy = u - x0f, v - y0f
        ok &= (x0f >= -1) & (x0f <= w) & (y0f >= -1) & (y0f <= h)
        x0, y0 = np.where(ok, x0f, -2 ** 31).astype(np.int64), np.where(ok, y0f, -2 ** 31).astype(np.int64)
        out = []
        for j in (0, 1):
            for i in (0, 1):
                qx, qy = x0 + i, y0 + j
                inside = ok & (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
                wgt = (fx if i else dtype(1) - fx) * (fy if j else dtype(1) - fy)
                out.append((np.where(inside, qy, 0), np.where(inside, qx, 0), wgt, inside))
    return out


def accumulate(S, normal, position, albedo, total_samples, view, proj, history, moments, max_history, normal_threshold, position_threshold, flags=0,
               dtype=np.float64):
    """One ptx_temporal_accumulate_moments: (T, the next History, the next Moments, decisions).  T, the History and the colour's
    decisions are temporal_ref.accumulate's own; `moments` None: no moment history (the first call, or a plain call came in between).
    The decisions gain 'mtaps' (H, W, 4) which taps counted for the moments, 'found_M' and 'known' (H, W)."""
    T, nxt, d = TR.accumulate(S, normal, position, albedo, total_samples, view, proj, history, max_history, normal_threshold, position_threshold, flags, dtype)
    h, w = T.shape[:2]
    valid = d["valid"]
    m = R.mean_of(S, total_samples, dtype)
    a = np.maximum(np.asarray(albedo, np.float32)[..., 0:3].astype(dtype), dtype(np.float32(R.ALBEDO_FLOOR)))
    x = np.asarray(position, np.float32)[..., 0:3].astype(dtype)
    mtaps, found = np.zeros((h, w, 4), bool), np.zeros((h, w), bool)
    with np.errstate(all="ignore"):
        c = np.where(valid[..., None], m / a, m)
        l = lum(c, dtype)
        mu1, mu2 = l, l * l
        M1, M2, LM = mu1.copy(), mu2.copy(), np.ones((h, w), dtype)
        if d["used_history"] and moments is not None:
            assert moments.m1.dtype == np.dtype(dtype)
            n1, n2, ln, den = (np.zeros((h, w), dtype) for _ in range(4))
            for k, (qy, qx, wgt, inside) in enumerate(_colour_candidates(history, view, proj, x, valid, w, h, dtype)):
                q1, q2, qL = moments.m1[qy, qx], moments.m2[qy, qx], moments.L[qy, qx]
                counts = d["taps"][..., k] & (qL > 0) & np.isfinite(q1) & np.isfinite(q2)
                mtaps[..., k] = counts
                wk = np.where(counts, wgt, dtype(0))
                n1, n2, ln, den = n1 + wk * np.where(counts, q1, dtype(0)), n2 + wk * np.where(counts, q2, dtype(0)), ln + wk * np.where(counts, qL, dtype(0)), den + wk
            found = valid & (den >= dtype(TR.FOUND_FLOOR))
            safe = np.where(found, den, dtype(1))
            h1, h2 = n1 / safe, n2 / safe
            Lf = np.where(found, np.minimum(ln / safe + dtype(1), dtype(np.float32(max_history))), dtype(1))
            M1, M2, LM = np.where(found, h1 + (mu1 - h1) / Lf, mu1), np.where(found, h2 + (mu2 - h2) / Lf, mu2), Lf
        known = valid & np.isfinite(M1) & np.isfinite(M2)
        zero = dtype(0)
        out = Moments(np.where(known, M1, zero), np.where(known, M2, zero), np.where(known, LM, zero))
    assert out.m1.dtype == np.dtype(dtype) and out.L.dtype == np.dtype(dtype)
    d = dict(d, mtaps=mtaps, found_M=found, known=known)
    return T, nxt, out, d


def run_sequence(frames, max_history, normal_threshold, position_threshold, dtype, plain=()):
    """frames as temporal_ref.run_sequence takes them; `plain`: the indices of the frames given to the plain call, which drops the
    moment history.  Returns ([T], [Moments or None], [decisions])."""
    hist, mom, Ts, Ms, dec = None, None, [], [], []
    for k, (S, nrm, pos, alb, n, view, proj, flags) in enumerate(frames):
        if k in plain:
            T, hist, d = TR.accumulate(S, nrm, pos, alb, n, view, proj, hist, max_history, normal_threshold, position_threshold, flags, dtype)
            mom = None
        else:
            T, hist, mom, d = accumulate(S, nrm, pos, alb, n, view, proj, hist, mom, max_history, normal_threshold, position_threshold, flags, dtype)
        Ts.append(T)
        Ms.append(mom)
        dec.append(d)
    return Ts, Ms, dec


def comparable_moments(dec32, dec64):
    """temporal_ref.comparable_pixels, with the moments' own decisions added: per frame the (H, W) mask of pixels on which a float32
    implementation's T and moments can be held to the float64 run"""
    out, prev = [], None
    colour = TR.comparable_pixels(dec32, dec64)
    for k, (a, b) in enumerate(zip(dec32, dec64)):
        keep = colour[k].copy()
        if "mtaps" in b:
            keep &= (a["mtaps"] == b["mtaps"]).all(axis=-1) & (a["found_M"] == b["found_M"]) & (a["known"] == b["known"])
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


def _guides(normal, position, albedo, dtype):
    n = np.asarray(normal, np.float32)[..., 0:3].astype(dtype)
    x = np.asarray(position, np.float32)[..., 0:3].astype(dtype)
    t = np.asarray(position, np.float32)[..., 3].astype(dtype)
    a = np.maximum(np.asarray(albedo, np.float32)[..., 0:3].astype(dtype), dtype(np.float32(R.ALBEDO_FLOOR)))
    return n, x, t, a


def _edge_terms(n, x, t, nq, xq, sn, sp):
    dn = n - nq
    plane = ((n * (xq - x)).sum(axis=-1)) / (sp * t)
    return (dn * dn).sum(axis=-1) / (sn * sn) + plane * plane


def estimate(T, normal, position, albedo, moments, sigma_normal, sigma_position, dtype=np.float64):
    """(V_0 (H, W), decisions): 'valid', 'long' (the L_M >= 4 branch), 'wtaps' (H, W, 49) the window's taps that counted (row-major
    over dy, dx; all False on the long branch)"""
    assert sigma_normal > 0 and sigma_position > 0
    valid = R.valid_mask(T, normal, position, 1, dtype)
    n, x, t, _ = _guides(normal, position, albedo, dtype)
    sn, sp = dtype(np.float32(sigma_normal)), dtype(np.float32(sigma_position))
    m1, m2, L = moments.m1.astype(dtype), moments.m2.astype(dtype), moments.L.astype(dtype)
    h, w = valid.shape
    long = valid & (L >= dtype(LONG_HISTORY))
    wtaps = np.zeros((h, w, (2 * WINDOW + 1) ** 2), bool)
    with np.errstate(all="ignore"):
        known = valid & (L > 0)
        s1, s2, den = np.where(known, m1, dtype(0)), np.where(known, m2, dtype(0)), np.where(known, dtype(1), dtype(0))
        k = -1
        for dy in range(-WINDOW, WINDOW + 1):
            for dx in range(-WINDOW, WINDOW + 1):
                k += 1
                if dx == 0 and dy == 0:
                    wtaps[..., k] = known & ~long
                    continue
                counts = valid & ~long & R._shift(known, dy, dx, False)
                if not counts.any():
                    continue
                wtaps[..., k] = counts
                e = _edge_terms(n, x, t, R._shift(n, dy, dx, 0), R._shift(x, dy, dx, 0), sn, sp)
                wq = np.where(counts, np.exp(-np.where(counts, e, 0)), dtype(0))
                s1, s2, den = s1 + wq * R._shift(m1, dy, dx, 0), s2 + wq * R._shift(m2, dy, dx, 0), den + wq
        some = den != 0
        safe = np.where(some, den, dtype(1))
        a1, a2 = s1 / safe, s2 / safe
        v = np.where(long, m2 - m1 * m1, np.where(some, a2 - a1 * a1, dtype(0)))
        V0 = np.where(valid & np.isfinite(v) & (v > 0), v, dtype(0))
    assert V0.dtype == np.dtype(dtype)
    return V0, {"valid": valid, "long": long, "wtaps": wtaps}


def filter_all(T, normal, position, albedo, V0, iterations, sigma_luminance, sigma_normal, sigma_position, dtype=np.float64):
    """([D after 1 iteration, ..., D after `iterations`], [V_1, ..., V_N], [decisions of iteration i]): 'ftaps' (H, W, 25) the taps that
    counted (row-major over dy, dx, the centre included on valid pixels), 'vzero' (H, W, 25) the taps the vt = 0 rule turned away."""
    assert 1 <= iterations <= 6 and sigma_luminance > 0 and sigma_normal > 0 and sigma_position > 0
    m = R.mean_of(T, 1, dtype)
    valid = R.valid_mask(T, normal, position, 1, dtype)
    n, x, t, a = _guides(normal, position, albedo, dtype)
    hk = [dtype(v) for v in R.H5]
    g3 = [dtype(v) for v in G3]
    sl, sn, sp = dtype(np.float32(sigma_luminance)), dtype(np.float32(sigma_normal)), dtype(np.float32(sigma_position))
    Ds, Vs, decs = [], [], []
    with np.errstate(all="ignore"):
        c = np.where(valid[..., None], m / a, m)
        V = np.where(valid, V0.astype(dtype), dtype(0))
        for i in range(iterations):
            s = 1 << i
            vs, gs = V * g3[1] * g3[1], np.full(valid.shape, g3[1] * g3[1], dtype)
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    if dx == 0 and dy == 0:
                        continue
                    vq = R._shift(valid, dy, dx, False)
                    g = np.where(vq, g3[dx + 1] * g3[dy + 1], dtype(0))
                    vs, gs = vs + np.where(vq, R._shift(V, dy, dx, 0), dtype(0)) * g, gs + g
            vt = vs / gs
            lp = lum(c, dtype)
            c0w = hk[2] * hk[2]
            num, den, vnum = c * c0w, np.full(valid.shape, c0w, dtype), V * (c0w * c0w)
            ftaps, vzero = np.zeros(valid.shape + (25,), bool), np.zeros(valid.shape + (25,), bool)
            k = -1
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    k += 1
                    if dx == 0 and dy == 0:
                        ftaps[..., k] = valid
                        continue
                    vq = valid & R._shift(valid, dy * s, dx * s, False)
                    if not vq.any():
                        continue
                    cq, Vq = R._shift(c, dy * s, dx * s, 0), R._shift(V, dy * s, dx * s, 0)
                    vq = vq & np.isfinite(cq).all(axis=-1)
                    dl = np.abs(lp - lum(cq, dtype))
                    turned = vq & (dl > 0) & (vt == 0)
                    vzero[..., k] = turned
                    el = np.where(dl == 0, dtype(0), (dl * dl) / ((sl * sl) * vt))
                    e = el + _edge_terms(n, x, t, R._shift(n, dy * s, dx * s, 0), R._shift(x, dy * s, dx * s, 0), sn, sp)
                    ok = vq & ~turned & (e >= 0)
                    ftaps[..., k] = ok
                    wq = np.where(ok, (hk[dx + 2] * hk[dy + 2]) * np.exp(-np.where(ok, e, 0)), dtype(0))
                    num = num + wq[..., None] * np.where(ok[..., None], cq, dtype(0))
                    vnum = vnum + (wq * wq) * np.where(ok, Vq, dtype(0))
                    den = den + wq
            c = np.where(valid[..., None], num / den[..., None], c)
            V = np.where(valid, vnum / (den * den), dtype(0))
            out = np.ones(valid.shape + (4,), dtype)
            out[..., 0:3] = np.where(valid[..., None], c * a, m)
            assert out.dtype == np.dtype(dtype) and V.dtype == np.dtype(dtype)
            Ds.append(out)
            Vs.append(V)
            decs.append({"ftaps": ftaps, "vzero": vzero})
    return Ds, Vs, decs


def denoise_variance(T, normal, position, albedo, moments, iterations, sigma_luminance, sigma_normal, sigma_position, dtype=np.float64):
    """One ptx_denoise_variance: (D, V_0)"""
    V0, _ = estimate(T, normal, position, albedo, moments, sigma_normal, sigma_position, dtype)
    return filter_all(T, normal, position, albedo, V0, iterations, sigma_luminance, sigma_normal, sigma_position, dtype)[0][-1], V0


def _took(keep, taps, offsets):
    """keep(p) and keep(q) for every tap q = p + offset that counted"""
    out = keep.copy()
    for k, (dy, dx) in enumerate(offsets):
        if taps[..., k].any():
            out &= ~taps[..., k] | R._shift(keep, dy, dx, True)  # a tap outside the image never counted
    return out


def comparable_estimate(keep, e32, e64):
    """The pixels whose V_0 can be held to the float64 run: `keep` (comparable_moments of the last frame) there and on every window tap
    either run took, and the two runs on the same branch with the same taps"""
    offsets = [(dy, dx) for dy in range(-WINDOW, WINDOW + 1) for dx in range(-WINDOW, WINDOW + 1)]
    same = keep & (e32["valid"] == e64["valid"]) & (e32["long"] == e64["long"]) & (e32["wtaps"] == e64["wtaps"]).all(axis=-1)
    return _took(same, e32["wtaps"] | e64["wtaps"], offsets)


def comparable_filter(keep, f32, f64):
    """Per iteration, the pixels whose D can be held to the float64 run: `keep` (comparable_estimate) carried through the taps that
    counted and the prefilter's 3 x 3, and the two runs alike in every tap decision"""
    out = []
    for i, (a, b) in enumerate(zip(f32, f64)):
        s = 1 << i
        same = keep & (a["ftaps"] == b["ftaps"]).all(axis=-1) & (a["vzero"] == b["vzero"]).all(axis=-1)
        same = _took(same, a["ftaps"] | b["ftaps"], [(dy * s, dx * s) for dy in range(-2, 3) for dx in range(-2, 3)])
        near = np.ones(keep.shape + (9,), bool)  # the prefilter reads V_i of every neighbour inside the image
        keep = _took(same, near, [(dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1)])
        out.append(keep)
    return out
