"""Local exposure (include/ptx.h "Local exposure", ptx_local_exposure) in numpy integers and float64, written from the header's steps
1 - 7.  Steps 1 and 2 are tests/meter_ref.py's luminance and classes; steps 2 - 5 are int64 operations (exact: every value stays below
2^55); step 5's division and step 6 are float64 operations, one per expression, so nothing is contracted; exp2 is meter_ref.exp2_spec,
the project's specified kernel.  The device's G is held to this bit for bit (tests/test_local_exposure.py)."""
import numpy as np

import meter_ref as MR

PIVOT_METERED = 1
SLICES = 32
LOG_GAP = 0.0861  # the largest distance of the piecewise-linear log2 e + m below log2((1 + m) 2^e): 0.08607 at m = 1 / ln 2 - 1


def fixed_log(Y):
    """Steps 1 - 2 on float32 luminances: (counted, l); l = clamp((int)(bits(Y) >> 15) - 888 * 32, 0, 8191) is meaningful where counted"""
    Y = np.ascontiguousarray(Y, np.float32)
    _, _, counted, _, _, _ = MR.classify(Y)
    l = np.clip((Y.view(np.uint32) >> 15).astype(np.int64) - 888 * 32, 0, 8191)
    return counted, l


def splat(l, counted, s):
    """Step 3: sum[cy][cx][z], cnt[cy][cx][z] as int64 (they fit uint32: asserted)"""
    h, w = l.shape
    nx, ny = -(-w // (1 << s)), -(-h // (1 << s))
    y, x = np.nonzero(counted)
    lv = l[y, x]
    total, cnt = np.zeros((ny, nx, SLICES), np.int64), np.zeros((ny, nx, SLICES), np.int64)
    np.add.at(total, (y >> s, x >> s, lv >> 8), lv)
    np.add.at(cnt, (y >> s, x >> s, lv >> 8), 1)
    assert total.max(initial=0) < 2 ** 32 and cnt.max(initial=0) <= 4096
    return total, cnt


def blur(a):
    """Step 4: one 1-2-1 pass along x, y and z, clamp to edge, integers, nothing divided"""
    a = np.asarray(a, np.int64)
    for axis in (1, 0, 2):
        pad = [(0, 0)] * 3
        pad[axis] = (1, 1)
        p = np.pad(a, pad, mode="edge")
        lo, mid, hi = (np.take(p, range(k, k + a.shape[axis]), axis=axis) for k in range(3))
        a = lo + 2 * mid + hi
    assert a.max(initial=0) < 2 ** 32
    return a


def taps(p, shift, last):
    """Step 5 along one axis for coordinates p (pixels with shift = s, or l with shift = 8): u = 2p + 1 - 2^shift; (c0, c1, f)"""
    u = 2 * np.asarray(p, np.int64) + 1 - (1 << shift)
    neg = u < 0
    c0 = np.where(neg, 0, u >> (shift + 1))
    f = np.where(neg, 0, u & ((2 << shift) - 1))
    c1 = np.where(neg, 0, np.minimum(c0 + 1, last))
    return c0, c1, f


def base(l, counted, s):
    """Steps 3 - 5: B as float64 (H x W; meaningful where counted), the splatted (sum, cnt) and the blurred ones"""
    h, w = l.shape
    raw = splat(l, counted, s)
    total, cnt = (blur(g) for g in raw)
    ny, nx = total.shape[:2]
    x0, x1, fx = taps(np.arange(w), s, nx - 1)
    y0, y1, fy = taps(np.arange(h), s, ny - 1)
    z0, z1, fz = taps(l, 8, SLICES - 1)
    full = 2 << s
    N, D = np.zeros((h, w), np.int64), np.zeros((h, w), np.int64)
    for cy, wy in ((y0, full - fy), (y1, fy)):
        for cx, wx in ((x0, full - fx), (x1, fx)):
            for cz, wz in ((z0, 512 - fz), (z1, fz)):
                wgt = wy[:, None] * wx[None, :] * wz
                N += wgt * total[cy[:, None], cx[None, :], cz]
                D += wgt * cnt[cy[:, None], cx[None, :], cz]
    assert N.max(initial=0) <= 2 ** 54 and (D[counted] > 0).all()
    with np.errstate(all="ignore"):
        B = N.astype(np.float64) / D.astype(np.float64) / 256.0 - 16.0
    return B, raw, (total, cnt)


def gain(S, total_samples, cell_shift=5, pivot_log2=-2.473931, highlight_contrast=0.6, shadow_contrast=0.8, max_stops=4.0, cur=None, denoised=False):
    """One accepted ptx_local_exposure on the H x W x 4 image S: (G as float32 H x W, per-pixel decisions).  cur: the meter state's
    double under PTX_LOCAL_EXPOSURE_PIVOT_METERED, None without the flag.  denoised: S is D, which holds the mean.  The float fields
    are taken as the float32 the descriptor holds."""
    f = lambda v: float(np.float32(v))  # noqa: E731
    Y = MR.luminance(S, 1 if denoised else total_samples)
    counted, l = fixed_log(Y)
    B, (total, cnt), (blurred_total, blurred_cnt) = base(l, counted, cell_shift)
    pv = f(pivot_log2)
    if cur is not None:
        pv = pv - float(cur)
    d = B - pv
    c = np.where(d > 0.0, f(highlight_contrast), f(shadow_contrast))
    g = (c - 1.0) * d
    g = np.minimum(np.maximum(g, -f(max_stops)), f(max_stops))
    g = np.minimum(np.maximum(g, -300.0), 300.0)
    G = np.ones(Y.shape, np.float32)
    values, inverse = np.unique(g[counted], return_inverse=True)
    G[counted] = np.array([MR.exp2_spec(float(v)) for v in values], np.float64).astype(np.float32)[inverse.reshape(-1)]
    return G, dict(Y=Y, counted=counted, l=l, B=B, g=np.where(counted, g, 0.0), sum=total, cnt=cnt, blurred_sum=blurred_total, blurred_cnt=blurred_cnt)
