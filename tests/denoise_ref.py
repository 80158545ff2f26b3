"""The denoiser's filter (include/ptx.h ptx_denoise, docs/NEXT_ROWS.md section 13) restated in numpy from its text, generic over
float32 / float64.  Nothing here is derived from the kernel.

    h = (1/16, 1/4, 3/8, 1/4, 1/16);  m(p) = S(p).rgb / totalSamples;  a_p = max(albedo_p, 0.01) per channel
    valid p: hit (normal.w == 1), m(p) finite, n_p finite, t_p = position.w > 0 and finite
    c_0 = m / a on valid pixels, m elsewhere
    c_{i+1}(p) = sum w_q c_i(q) / sum w_q over q = p + 2^i (dx, dy), dx, dy in -2 .. 2, on valid p; c_i(p) elsewhere
        centre: w = h[2] h[2] by rule; any other tap only if q is inside, valid, c_i(q) finite and e >= 0
        w = h[dx+2] h[dy+2] exp(-e)
        e = |c_i(p) - c_i(q)|^2 / (sigmaColor 2^-i)^2 + |n_p - n_q|^2 / sigmaNormal^2 + (dot(n_p, x_q - x_p) / (sigmaPosition t_p))^2
    D = c_N a on valid pixels, m elsewhere; alpha 1
"""
import numpy as np

H5 = (1.0 / 16.0, 1.0 / 4.0, 3.0 / 8.0, 1.0 / 4.0, 1.0 / 16.0)
ALBEDO_FLOOR = 0.01
GUIDE_NORMAL, GUIDE_POSITION, GUIDE_ALBEDO = 0, 1, 2
MISS = {GUIDE_NORMAL: (0.0, 0.0, 0.0, 0.0), GUIDE_POSITION: (0.0, 0.0, 0.0, 0.0), GUIDE_ALBEDO: (1.0, 1.0, 1.0, 1.0)}


def _shift(a, oy, ox, fill):
    """out[y, x] = a[y + oy, x + ox] where that is inside the image, `fill` elsewhere"""
    h, w = a.shape[:2]
    out = np.full_like(a, fill)
    y0, y1, x0, x1 = max(0, -oy), min(h, h - oy), max(0, -ox), min(w, w - ox)
    if y0 < y1 and x0 < x1:
        out[y0:y1, x0:x1] = a[y0 + oy:y1 + oy, x0 + ox:x1 + ox]
    return out


def mean_of(S, total_samples, dtype):
    """postprocess.comp:22 divides by multiplying with the reciprocal"""
    return np.asarray(S, np.float32)[..., 0:3].astype(dtype) * (dtype(1) / dtype(total_samples))


def valid_mask(S, normal, position, total_samples, dtype=np.float64):
    m = mean_of(S, total_samples, dtype)
    n, t = np.asarray(normal, np.float32), np.asarray(position, np.float32)[..., 3]
    with np.errstate(all="ignore"):
        return (n[..., 3] == 1) & np.isfinite(m).all(axis=-1) & np.isfinite(n[..., 0:3]).all(axis=-1) & (t > 0) & np.isfinite(t)


def denoise_all(S, normal, position, albedo, total_samples, iterations, sigma_color, sigma_normal, sigma_position, dtype=np.float64):
    """[D after 1 iteration, D after 2, ..., D after `iterations`], each an (H, W, 4) array of `dtype`: iteration i does not depend
    on how many follow it, so one run serves every count."""
    assert 1 <= iterations <= 6 and total_samples > 0 and sigma_color >= 0 and sigma_normal > 0 and sigma_position > 0
    m = mean_of(S, total_samples, dtype)
    valid = valid_mask(S, normal, position, total_samples, dtype)
    n = np.asarray(normal, np.float32)[..., 0:3].astype(dtype)
    x = np.asarray(position, np.float32)[..., 0:3].astype(dtype)
    t = np.asarray(position, np.float32)[..., 3].astype(dtype)
    a = np.maximum(np.asarray(albedo, np.float32)[..., 0:3].astype(dtype), dtype(np.float32(ALBEDO_FLOOR)))
    h = [dtype(v) for v in H5]
    sn, sp = dtype(np.float32(sigma_normal)), dtype(np.float32(sigma_position))
    results = []
    with np.errstate(all="ignore"):
        c = np.where(valid[..., None], m / a, m)
        for i in range(iterations):
            s = 1 << i
            sc = dtype(np.float32(sigma_color)) * dtype(2.0 ** -i)
            num = c * (h[2] * h[2])
            den = np.full(valid.shape, h[2] * h[2], dtype)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    if dx == 0 and dy == 0:
                        continue
                    vq = _shift(valid, dy * s, dx * s, False)  # inside the image and valid
                    if not vq.any():
                        continue
                    cq, nq, xq = _shift(c, dy * s, dx * s, 0), _shift(n, dy * s, dx * s, 0), _shift(x, dy * s, dx * s, 0)
                    dn = n - nq
                    plane = ((n * (xq - x)).sum(axis=-1)) / (sp * t)
                    e = (dn * dn).sum(axis=-1) / (sn * sn) + plane * plane
                    if sigma_color > 0:
                        dc = c - cq
                        e = (dc * dc).sum(axis=-1) / (sc * sc) + e
                    ok = vq & np.isfinite(cq).all(axis=-1) & (e >= 0)
                    w = np.where(ok, (h[dx + 2] * h[dy + 2]) * np.exp(-np.where(ok, e, 0)), dtype(0))
                    num = num + w[..., None] * np.where(ok[..., None], cq, dtype(0))
                    den = den + w
            c = np.where(valid[..., None], num / den[..., None], c)
            out = np.ones(valid.shape + (4,), dtype)
            out[..., 0:3] = np.where(valid[..., None], c * a, m)
            assert out.dtype == np.dtype(dtype)
            results.append(out)
    return results


def denoise(S, normal, position, albedo, total_samples, iterations, sigma_color, sigma_normal, sigma_position, dtype=np.float64):
    return denoise_all(S, normal, position, albedo, total_samples, iterations, sigma_color, sigma_normal, sigma_position, dtype)[-1]


def plane_guides(h, w, normal=(0.0, 0.0, 1.0), distance=5.0, albedo=(1.0, 1.0, 1.0), pixel=0.01):
    """Synthetic guides of one plane through the origin seen head-on: position = pixel * (x, y) in the plane, hit everywhere."""
    nrm = np.zeros((h, w, 4), np.float32)
    nrm[..., 0:3], nrm[..., 3] = np.float32(normal), 1.0
    pos = np.zeros((h, w, 4), np.float32)
    yy, xx = np.mgrid[0:h, 0:w]
    n = np.float64(normal)
    u = np.cross(n, [0.0, 1.0, 0.0] if abs(n[1]) < 0.9 else [1.0, 0.0, 0.0])
    u /= np.linalg.norm(u)
    v = np.cross(n, u)
    pos[..., 0:3] = (xx[..., None] * u + yy[..., None] * v) * pixel
    pos[..., 3] = distance
    alb = np.ones((h, w, 4), np.float32)
    alb[..., 0:3] = np.float32(albedo)
    return nrm, pos, alb


def set_miss(guides, mask):
    for which, g in enumerate(guides):
        g[mask] = np.float32(MISS[which])


def relative_l2(img, truth):
    a, b = np.asarray(img, np.float64)[..., 0:3], np.asarray(truth, np.float64)[..., 0:3]
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def without_emission(pkg, desc):
    """(a copy of the scene description whose materials emit nothing, the arrays it points to)"""
    import ctypes as C

    d = pkg.SceneDesc()
    C.memmove(C.byref(d), C.byref(desc), C.sizeof(d))
    keep = []
    for field, count in (("metallicRoughnessMaterials", d.metallicRoughnessMaterialCount), ("specularGlossinessMaterials", d.specularGlossinessMaterialCount),
                         ("phongMaterials", d.phongMaterialCount)):
        if count:
            mats = np.frombuffer((C.c_uint8 * (count * 96)).from_address(getattr(d, field)), np.float32).reshape(count, 24).copy()
            mats[:, 0:4] = 0.0  # EmissiveColor, EmissiveIntensity
            keep.append(mats)
            setattr(d, field, mats.ctypes.data)
    return d, keep


def dark_lights(pkg, lights):
    """The scene's lights with every colour zero (the directions stay: a zero direction has no normalize())"""
    import ctypes as C

    out = pkg.LightsUbo()
    C.memmove(C.byref(out), C.byref(lights), C.sizeof(out))
    out.Directional.Color[:] = (0.0, 0.0, 0.0)
    for k in range(64):
        out.Lights[k].Color[:] = (0.0, 0.0, 0.0)
    return out


def cpu_guides(pkg, orc, scene, w, h):
    """ptx_render_guides without a GPU, from the debug view's reference (tests/debug_view_ref.py): its Normal mode, the position and
    hit distance of the primary hit, and the base colour as (Color mode without emission, light colours or shadows) / 0.1."""
    import debug_view_ref as DV

    u, dark = scene.uniform(w, h), dark_lights(pkg, scene.lights)
    nrm = DV.render(DV.RefScene(orc, scene.desc), u, dark, w, h, DV.MODE_NORMAL, 0, np.float32)
    d, keep = without_emission(pkg, scene.desc)
    col = DV.render(DV.RefScene(orc, d), u, dark, w, h, DV.MODE_COLOR, DV.HIT_DISABLE_SHADOWS, np.float64)
    g = [np.zeros((h, w, 4), np.float32) for _ in range(3)]
    g[GUIDE_NORMAL][..., 0:3], g[GUIDE_NORMAL][..., 3] = nrm["image"][..., 0:3], 1.0
    g[GUIDE_POSITION][..., 0:3], g[GUIDE_POSITION][..., 3] = nrm["position"], nrm["t"]
    with np.errstate(all="ignore"):
        g[GUIDE_ALBEDO][..., 0:3], g[GUIDE_ALBEDO][..., 3] = col["image"][..., 0:3] / 0.1, 1.0
    set_miss(g, ~nrm["hit"])
    return g
