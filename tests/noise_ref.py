"""Noise metering (include/ptx.h "Noise metering", ptx_noise_meter) in numpy float32 and Python integers, written from the header's steps
1 - 7.  Steps 1 - 5 are float32 operations in the header's order, one numpy operation per header operation, so nothing is contracted;
steps 6 and 7 are Python integers (exact) and Python floats (IEEE doubles), so the device's result is held to this bit for bit
(tests/test_noise_meter.py).  Every per-pixel class and q is reported.

The project's kernels, restated: rcp is 1 / x correctly rounded (numpy's float32 division), as tests/meter_ref.py restates it; sqrt is
IEEE; a / b is a * rcp(b); fmin(a, b) = b < a ? b : a."""
import numpy as np

WRITE_SUM = 1
f32 = np.float32
BLACK_BELOW = f32(2.0 ** -20)


def rcp(x):
    with np.errstate(all="ignore"):
        return (f32(1.0) / np.asarray(x, f32)).astype(f32)


def scale_factors(samples_a, samples_b, exposure):
    """Step 2: sa, sb, st"""
    e = f32(exposure)
    return e * rcp(f32(samples_a)), e * rcp(f32(samples_b)), e * rcp(f32(samples_a + samples_b))


def pixels(A, B, samples_a, samples_b, exposure):
    """Steps 1 - 5 on the H x W x 4 halves: S, and per pixel rejected, black, counted and q (int64)"""
    A = np.ascontiguousarray(A, f32)
    B = np.ascontiguousarray(B, f32)
    sa, sb, st = scale_factors(samples_a, samples_b, exposure)
    with np.errstate(all="ignore"):
        S = (A + B).astype(f32)                                                      # step 1
        a, b, c = A[..., :3] * sa, B[..., :3] * sb, S[..., :3] * st                  # step 3
        d = np.abs(a - b)
        D = (d[..., 0] + d[..., 1]) + d[..., 2]
        m = (c[..., 0] + c[..., 1]) + c[..., 2]
        rejected = ~(np.isfinite(A[..., :3]).all(-1) & np.isfinite(B[..., :3]).all(-1) & np.isfinite(D) & np.isfinite(m))   # step 4
        black = ~rejected & ~(m >= BLACK_BELOW)
        counted = ~rejected
        live = counted & ~black
        ms = np.where(live, m, f32(1.0)).astype(f32)
        Ds = np.where(live, D, f32(0.0)).astype(f32)
        quotient = (Ds * rcp(np.sqrt(ms))).astype(f32)                                # step 5: D / sqrt(m) = D * rcp(sqrt(m))
        e = (f32(0.5) * quotient).astype(f32)
        e = np.where(f32(255.0) < e, f32(255.0), e).astype(f32)                       # fmin(e, 255)
        q = np.where(live, (e * f32(65536.0)).astype(f32).astype(np.int64), 0)
    assert int(q.max(initial=0)) < 2 ** 24
    return dict(S=S, D=D, m=m, rejected=rejected, black=black, counted=counted, e=np.where(live, e, f32(0.0)).astype(f32), q=q)


def tile_error(Q, n):
    """Step 6: E_t of one tile as a float32"""
    return f32(float(Q) / (float(n) * 65536.0)) if n else f32(0.0)


def meter(A, B, samples_a, samples_b, exposure=1.0, threshold=0.0, tile_shift=4, calls=1):
    """One accepted ptx_noise_meter: (result, tileErrors, per-pixel decisions).  `result` has PtxNoiseResult's fields; `calls` is what
    the device will have counted."""
    p = pixels(A, B, samples_a, samples_b, exposure)
    h, w = p["q"].shape
    side = 1 << tile_shift
    tx, ty = (w + side - 1) >> tile_shift, (h + side - 1) >> tile_shift
    E = np.zeros((ty, tx), f32)
    Q = np.zeros((ty, tx), object)
    N = np.zeros((ty, tx), np.int64)
    for j in range(ty):
        for i in range(tx):
            win = (slice(j * side, min(h, (j + 1) * side)), slice(i * side, min(w, (i + 1) * side)))
            Q[j, i] = sum(int(v) for v in p["q"][win].ravel())
            N[j, i] = int(p["counted"][win].sum())
            E[j, i] = tile_error(Q[j, i], N[j, i])
    thr = f32(threshold)
    n_all, q_all = int(N.sum()), sum(int(v) for v in Q.ravel())
    res = dict(meanError=f32(float(q_all) / (float(n_all) * 65536.0)) if n_all else f32(0.0), maxError=f32(E.max()) if n_all else f32(0.0),
               tilesX=tx, tilesY=ty, converged=int((E <= thr).sum()), counted=n_all, black=int(p["black"].sum()), rejected=int(p["rejected"].sum()),
               valid=int(n_all > 0), calls=calls)
    p.update(Q=Q, N=N)
    return res, E, p
