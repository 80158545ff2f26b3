"""Exposure metering (include/ptx.h "Exposure metering", ptx_meter) in numpy and Python integers, written from the header's steps 1 - 9.
Steps 1 - 4 are float32 and integer operations in the header's order; steps 5 - 8 are Python integers (exact) and Python floats (IEEE
doubles, one operation per expression, so nothing is contracted), so the device's result is held to this bit for bit
(tests/test_metering.py).  Every per-pixel decision is reported.

The project's kernels, restated: rcp is 1 / x correctly rounded on [2^-126, 2^126]; exp2 on |t| <= 300 is the fixed kernel of
csrc/pt_device.hpp (exp2_), as tests/test_transcendentals.py restates it."""
import math

import numpy as np

SUM, DESPIKED, DENOISED = 0, 1, 2
AVERAGE, CENTRE, REGION = 0, 1, 2
# step 6: the doubles nearest to log2(1 + (2j + 1) / 16), as the header spells them
T = [float.fromhex(h) for h in ("0x1.663f6fac91316p-4", "0x1.fbc16b902680ap-3", "0x1.91bba891f1709p-2", "0x1.0c10500d63aa6p-1",
                                "0x1.49a784bcd1b8bp-1", "0x1.82809d5be7073p-1", "0x1.b74948f5532dap-1", "0x1.e88c6b3626a73p-1")]


def exp2_spec(t):
    """exp2_ of |t| <= 300: k = floor(t + 0.5), Horner in (t - k) ln 2 over 1/13! ... 1/2!, 1, 1, times 2^k"""
    k = math.floor(t + 0.5)
    r = (t - k) * 0.6931471805599453
    p = 1.0 / 6227020800.0
    for d in (479001600.0, 39916800.0, 3628800.0, 362880.0, 40320.0, 5040.0, 720.0, 120.0, 24.0, 6.0):
        p = p * r + 1.0 / d
    for c in (0.5, 1.0, 1.0):
        p = p * r + c
    return p * math.ldexp(1.0, int(k))


def luminance(S, total_samples):
    """Step 1: c = S.rgb rcp((float)totalSamples), Y = (0.2126 c.r + 0.7152 c.g) + 0.0722 c.b, all float32"""
    S = np.ascontiguousarray(S, np.float32)
    f = np.float32
    with np.errstate(all="ignore"):
        rs = f(1.0) / f(total_samples)
        r, g, b = (S[..., k] * rs for k in range(3))
        return ((f(0.2126) * r + f(0.7152) * g) + f(0.0722) * b).astype(np.float32)


def classify(Y):
    """Steps 2 and 3 on float32 luminances: (rejected, black, counted, bin, under, over); bin is meaningful where counted"""
    Y = np.ascontiguousarray(Y, np.float32)
    bits = Y.view(np.uint32)
    rejected = ~np.isfinite(Y)
    with np.errstate(invalid="ignore"):
        black = ~rejected & ((Y <= 0) | (Y < np.float32(2.0 ** -126)))
    counted = ~rejected & ~black
    i = (bits >> 20).astype(np.int64) - 888
    under = counted & (i < 0)
    over = counted & (i > 255)
    return rejected, black, counted, np.clip(i, 0, 255), under, over


def centre_weight(n):
    """Step 4: 1 + [n <= 4x + 2 <= 3n] + [3n <= 8x + 4 <= 5n] for x = 0 ... n - 1, Python integers"""
    return np.array([1 + int(n <= 4 * x + 2 <= 3 * n) + int(3 * n <= 8 * x + 4 <= 5 * n) for x in range(n)], np.int64)


def weights(h, w, mode, region=(0, 0, 0, 0)):
    if mode == AVERAGE:
        return np.ones((h, w), np.int64)
    if mode == CENTRE:
        return centre_weight(h)[:, None] * centre_weight(w)[None, :]
    x0, x1, y0, y1 = region
    out = np.zeros((h, w), np.int64)
    out[y0:y1, x0:x1] = 1
    return out


def histogram(S, total_samples, mode=AVERAGE, region=(0, 0, 0, 0)):
    """Steps 1 - 4: the 256 bins and the class counters of the H x W x 4 image S, and the per-pixel decisions"""
    S = np.ascontiguousarray(S, np.float32)
    h, w = S.shape[:2]
    Y = luminance(S, total_samples)
    rejected, black, counted, b, under, over = classify(Y)
    wt = weights(h, w, mode, region)
    bins = np.bincount(b[counted], weights=wt[counted], minlength=256).astype(np.int64)  # doubles hold sums below 2^53 exactly
    total = lambda m: int(wt[m].sum())
    assert int(wt.sum()) < 2 ** 32
    return bins, dict(black=total(black), rejected=total(rejected), under=total(under), over=total(over)), \
        dict(Y=Y, rejected=rejected, black=black, counted=counted, bin=b, under=under, over=over, weight=wt)


def trim(bins, low_permille, high_permille):
    """Step 5: (N, lo, hi, kept_i) in Python integers"""
    n = [int(v) for v in bins]
    N = sum(n)
    lo, hi = N * low_permille // 1000, N * high_permille // 1000
    kept, P = [], 0
    for v in n:
        kept.append(max(0, min(P + v, N - hi) - max(P, lo)))
        P += v
    return N, lo, hi, kept


def mean_log2(kept):
    """Step 6: avg as a double, in the header's order"""
    K = sum(kept)
    A = sum(k * (i >> 3) for i, k in enumerate(kept))
    B = [sum(k for i, k in enumerate(kept) if (i & 7) == j) for j in range(8)]
    frac = float(B[0]) * T[0] + float(B[1]) * T[1]
    for j in range(2, 8):
        frac = frac + float(B[j]) * T[j]
    return (float(A) + frac) / float(K) - 16.0


def clamp(x, lo, hi):
    return min(max(x, lo), hi)


class Meter:
    """The device state of step 9 and ptx_meter on it.  `result` has PtxMeterResult's fields; `bins` the 256 bins; `cur` the double."""

    def __init__(self):
        self.reset()

    def reset(self):
        """ptx_meter_reset, ptx_resize"""
        self.result = dict(exposure=np.float32(1.0), log2Exposure=np.float32(0.0), avgLog2=np.float32(0.0), targetLog2=np.float32(0.0), counted=0, kept=0,
                           black=0, rejected=0, under=0, over=0, valid=0, calls=0)
        self.bins = np.zeros(256, np.int64)
        self.cur, self.started = 0.0, False

    def meter(self, S, total_samples, delta_seconds=0.0, mode=AVERAGE, region=(0, 0, 0, 0), low_permille=0, high_permille=0, key_log2=0.0, compensation=0.0,
              min_log2_exposure=-8.0, max_log2_exposure=8.0, speed_up=1.0, speed_down=1.0, denoised=False):
        """One accepted ptx_meter on the image S; denoised: S is D, which holds the mean, so 1 stands for total_samples.  The float
        fields are taken as the float32 the descriptor holds.  Returns the per-pixel decisions."""
        f = lambda v: float(np.float32(v))
        bins, counters, decisions = histogram(S, 1 if denoised else total_samples, mode, region)
        N, lo, hi, kept = trim(bins, low_permille, high_permille)
        K = sum(kept)
        assert K == N - lo - hi
        res = self.result
        res.update(counters, counted=N, kept=K, calls=res["calls"] + 1, valid=int(K > 0))
        self.bins = bins
        if K:
            avg = mean_log2(kept)                                                                    # step 6
            target = clamp((f(key_log2) - avg) + f(compensation), f(min_log2_exposure), f(max_log2_exposure))  # step 7
            if not self.started:                                                                     # step 8
                cur = target
            else:
                rate = f(speed_up) if target > self.cur else f(speed_down)
                a = 1.0 - exp2_spec(max(((-f(delta_seconds)) * rate) * 1.4426950408889634, -300.0))
                cur = target if a == 1.0 else self.cur + (target - self.cur) * a
            self.cur, self.started = cur, True
            res.update(avgLog2=np.float32(avg), targetLog2=np.float32(target), log2Exposure=np.float32(cur),
                       exposure=np.float32(exp2_spec(clamp(cur, -300.0, 300.0))))
            decisions.update(avg=avg, target=target)
        decisions.update(kept=kept, lo=lo, hi=hi)
        return decisions
