"""CPU restatement of the enlarging screen path (include/ptx.h ptx_present_upscaled, steps 2 - 5; csrc/pt_upscale.hpp), generic over
a numpy dtype.

Written from the header's numbered steps.  Step 1, the composed texel, is the oracle's orc.postprocess(..., tone_mapping=1), as in
tests/present_ref.py; step 6 is present_ref.present at equal extents (its blit is then the identity) or grade_ref.grade.  Every
operation of steps 2 - 5 is one IEEE operation in the stated order -- products, sums, comparisons and selections, one division a * (1 / b)
for the axis ratio, roundings to binary16 -- so in float32 the device's S equals this one bit for bit.  Constants are float32 literals,
widened where the dtype is float64, so that the two instances differ in rounding alone."""
import numpy as np


def _f16(x, dtype):
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(x).astype(np.float16).astype(dtype)


def _div(a, b, dtype):
    return dtype(a) * (dtype(1.0) / dtype(b))


def axis(src, dst, dtype):
    """Step 2 for every destination coordinate of one axis: (taps 4 x dst, weights 4 x dst), or None for an axis that is not filtered."""
    if src == dst:
        return None
    s = np.arange(dst).astype(dtype)
    x = (s + dtype(0.5)) * _div(src, dst, dtype) - dtype(0.5)
    x0 = np.floor(x)
    t = x - x0
    taps = np.stack([np.clip(x0 + dtype(k), 0, src - 1).astype(np.int64) for k in (-1, 0, 1, 2)])
    w0 = ((dtype(-0.5) * t + dtype(1.0)) * t - dtype(0.5)) * t
    w1 = ((dtype(1.5) * t - dtype(2.5)) * t) * t + dtype(1.0)
    w2 = ((dtype(-1.5) * t + dtype(2.0)) * t + dtype(0.5)) * t
    w3 = ((dtype(0.5) * t - dtype(0.5)) * t) * t
    return taps, np.stack([w0, w1, w2, w3])


def _select_min(new, running):
    with np.errstate(invalid="ignore"):
        return np.where(new < running, new, running)


def _select_max(new, running):
    with np.errstate(invalid="ignore"):
        return np.where(running < new, new, running)


def _clamp(v, lo, hi):
    """v >= lo ? v : lo, then v <= hi ? v : hi: a NaN becomes lo"""
    with np.errstate(invalid="ignore"):
        v = np.where(v >= lo, v, lo)
        return np.where(v <= hi, v, hi)


def taps4(a, b, c, d, w):
    """Steps 3 and 4: the weighted sum in its written order, clamped between the two central taps."""
    with np.errstate(all="ignore"):
        v = ((a * w[0] + b * w[1]) + c * w[2]) + d * w[3]
    return _clamp(v, _select_min(c, b), _select_max(c, b))


def enlarge(composed, sw, sh, dtype):
    """Steps 2 - 4: H x W x 3 binary16-valued T -> sh x sw x 3 S of `dtype`, binary16-valued."""
    t = np.asarray(composed)[..., :3].astype(dtype)
    h, w = t.shape[:2]
    assert sw >= w and sh >= h
    ax, ay = axis(w, sw, dtype), axis(h, sh, dtype)
    r = t
    if ax is not None:
        i, wt = ax
        r = taps4(t[:, i[0]], t[:, i[1]], t[:, i[2]], t[:, i[3]], wt[:, None, :, None])
    if ay is not None:
        j, wt = ay
        r = taps4(r[j[0]], r[j[1]], r[j[2]], r[j[3]], wt[:, :, None, None])
    return _f16(r, dtype)


def sharpen(s, sharpness, dtype):
    """Step 5 on the screen image S; sharpness as the float32 the desc holds.  Not called for +0."""
    s = np.asarray(s, dtype)
    k = dtype(np.float32(sharpness))
    n, sd = np.concatenate([s[:1], s[:-1]]), np.concatenate([s[1:], s[-1:]])
    wt, e = np.concatenate([s[:, :1], s[:, :-1]], axis=1), np.concatenate([s[:, 1:], s[:, -1:]], axis=1)
    with np.errstate(all="ignore"):
        m = ((n + sd) + (wt + e)) * dtype(0.25)
        v = s + (s - m) * k
    lo, hi = s, s
    for q in (n, sd, wt, e):
        lo, hi = _select_min(q, lo), _select_max(q, hi)
    v = _f16(_clamp(v, lo, hi), dtype)
    return np.where(np.isfinite(s), v, s)


def screen_image(composed, sw, sh, sharpness, dtype=np.float32):
    """Steps 2 - 5: what step 6 (tone or grade, UI, HDR10, store) is applied to.  sh x sw x 3 of `dtype`, binary16-valued."""
    s = enlarge(composed, sw, sh, dtype)
    if np.float32(sharpness).view(np.uint32) != 0:
        s = sharpen(s, sharpness, dtype)
    return s
