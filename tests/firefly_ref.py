"""Firefly suppression (include/ptx.h "Firefly suppression", ptx_despike) in numpy, written from the header's ten steps; generic over
float32 and float64.  In float32 every operation is the one the header names, in its order, so the device's C is held to it bit for
bit; float64 is there to say what a clamp decision is worth (tests/test_fireflies.py).

The specified reciprocal, restated: 1 / Y correctly rounded, +-inf below 2^-126, +-0 above 2^126."""
import numpy as np

TINY = 2.0 ** -126  # the smallest normal float32
HUGE = 2.0 ** 126


def luminance(S, dtype=np.float32):
    """Step 1: Y = (0.2126 r + 0.7152 g) + 0.0722 b"""
    S = np.asarray(S)
    r, g, b = (S[..., k].astype(dtype) for k in range(3))
    with np.errstate(all="ignore"):
        return (dtype(0.2126) * r + dtype(0.7152) * g) + dtype(0.0722) * b


def rcp(y, dtype=np.float32):
    """1 / y correctly rounded on [2^-126, 2^126], +-inf below (zeros and denormals), +-0 above"""
    y = np.asarray(y, dtype)
    with np.errstate(all="ignore"):
        r = dtype(1.0) / y
        r = np.where(np.abs(y) < dtype(TINY), np.copysign(dtype(np.inf), y), r)
        r = np.where(np.abs(y) > dtype(HUGE), np.copysign(dtype(0.0), y), r)
    return r.astype(dtype)


def window(radius):
    """Step 3: the offsets (dy, dx) of the (2 radius + 1)^2 window without its centre, row by row"""
    return [(dy, dx) for dy in range(-radius, radius + 1) for dx in range(-radius, radius + 1) if (dy, dx) != (0, 0)]


def _shifted(Y, dy, dx):
    """Y(p + (dy, dx)), -inf where that is outside the image"""
    h, w = Y.shape
    out = np.full_like(Y, -np.inf)
    ys, yd = (slice(dy, h), slice(0, h - dy)) if dy >= 0 else (slice(0, h + dy), slice(-dy, h))
    xs, xd = (slice(dx, w), slice(0, w - dx)) if dx >= 0 else (slice(0, w + dx), slice(-dx, w))
    if h - abs(dy) > 0 and w - abs(dx) > 0:
        out[yd, xd] = Y[ys, xs]
    return out


def despike(S, radius, rank, min_taps, gain, dtype=np.float32):
    """(C, decisions) of ptx_despike on the H x W x 4 sum S.  C has S's alpha and, where nothing is clamped, S's bits (float32) or
    values (float64).  decisions: every per-pixel quantity a step of the header names."""
    assert radius in (1, 2) and 1 <= rank <= 4 and rank <= min_taps <= (2 * radius + 1) ** 2 - 1 and gain >= 1 and np.isfinite(gain)
    S = np.ascontiguousarray(S, np.float32)
    Y = luminance(S, dtype)
    counts = np.isfinite(Y)                                                       # step 2
    seen = np.where(counts, Y, dtype(-np.inf))
    taps = np.stack([_shifted(seen, dy, dx) for dy, dx in window(radius)], axis=-1)  # steps 3, 4: what does not count is -inf
    n = (taps > dtype(-np.inf)).sum(axis=-1)                                     # step 5
    ranked = -np.sort(-taps, axis=-1)                                            # step 6: descending, equal values separately
    h = ranked[..., rank - 1]
    with np.errstate(all="ignore"):
        gh = (dtype(gain) * h).astype(dtype)
        b = np.where(gh > dtype(0.0), gh, dtype(0.0)).astype(dtype)               # step 7
        enough = n >= min_taps
        normal = counts & (Y >= dtype(TINY))
        above = counts & (Y > b)
        clamped = counts & enough & normal & above                               # step 8
        s = (b * rcp(np.where(clamped, Y, dtype(1.0)), dtype)).astype(dtype)      # step 9
        C = S.astype(dtype).copy() if dtype is not np.float32 else S.copy()
        rgb = (S[..., 0:3].astype(dtype) * s[..., None]).astype(dtype)
    C[..., 0:3] = np.where(clamped[..., None], rgb, C[..., 0:3])                 # step 10: everything else is S
    return C, {"Y": Y, "counts": counts, "n": n, "h": h, "b": b, "enough": enough, "normal": normal, "above": above, "clamped": clamped, "scale": s}


def mean_of(C, total_samples):
    """The mean an H x W x 4 sum stands for: rgb / total_samples"""
    return np.asarray(C)[..., 0:3] / np.float32(total_samples)
