"""Adaptive sampling (include/ptx.h "Adaptive sampling": ptx_adaptive_plan, ptx_adaptive_clear, ptx_noise_meter_adaptive) in Python
integers and numpy float32, written from the header's text: steps 1 - 3 of ptx_adaptive_plan are integers only, and the adaptive meter
is tests/noise_ref.py's steps with every tile's own sample counts.  The device is held to this bit for bit (tests/test_adaptive.py)."""
import numpy as np

import noise_ref as NR

FROM_NOISE, FROM_MASK = 0, 1
f32 = np.float32


def tiling(w, h, shift):
    """tilesX, tilesY"""
    side = 1 << shift
    return (w + side - 1) >> shift, (h + side - 1) >> shift


def tile_pixels(w, h, shift):
    """tilesY x tilesX: the pixels of every tile that lie inside the image"""
    side = 1 << shift
    tx, ty = tiling(w, h, shift)
    return np.array([[min(side, w - i * side) * min(side, h - j * side) for i in range(tx)] for j in range(ty)], np.int64).reshape(ty, tx)


def dilated(seeds, dilate):
    """Step 2: active iff some seed lies within Chebyshev distance `dilate`, in tiles"""
    seeds = np.asarray(seeds, bool)
    ty, tx = seeds.shape
    active = np.zeros((ty, tx), bool)
    for j in range(ty):
        for i in range(tx):
            active[j, i] = any(seeds[y, x] for y in range(max(0, j - dilate), min(ty, j + dilate + 1)) for x in range(max(0, i - dilate), min(tx, i + dilate + 1)))
    return active


class Planner:
    """The handle's adaptive state: the counts, the plan in force (active is None without one) and the generation."""

    def __init__(self, w, h):
        self.w, self.h = w, h
        self.shift = 0
        self.counts = None   # 2 x tilesY x tilesX, Python integers held in int64
        self.active = None
        self.generation = 0

    def plan(self, shift, seeds, dilate=0, frames_a=0, frames_b=0):
        """One accepted ptx_adaptive_plan with the seeds given (from a mask, or `not converged` of a meter's records):
        (PtxAdaptivePlan's fields, the list)"""
        tx, ty = tiling(self.w, self.h, shift)
        if self.shift != shift:
            assert self.counts is None or (not self.counts.any() and (self.active is None or not (frames_a or frames_b))), "refused"
            self.counts = np.zeros((2, ty, tx), np.int64)
            self.active = None
            self.shift = shift
            self.generation = 0
        seeds = np.asarray(seeds).reshape(ty, tx) != 0
        was = np.ones((ty, tx), bool) if self.active is None else self.active          # step 1
        self.counts[0][was] += frames_a
        self.counts[1][was] += frames_b
        self.active = dilated(seeds, dilate)                                             # step 2
        ids = [j * tx + i for j in range(ty) for i in range(tx) if self.active[j, i]]    # step 3: ascending
        self.generation += 1
        pixels = int(tile_pixels(self.w, self.h, shift)[self.active].sum())
        return dict(tilesX=tx, tilesY=ty, activeTiles=len(ids), activePixels=pixels, seedTiles=int(seeds.sum()), generation=self.generation), np.array(ids, np.uint32)

    def clear(self):
        self.active = None

    def zero_counts(self):
        """ptx_noise_halves(1)"""
        if self.counts is not None:
            self.counts[...] = 0

    def pixel_mask(self):
        """H x W: the pixels of the plan's tiles (all without a plan)"""
        if self.active is None:
            return np.ones((self.h, self.w), bool)
        side = 1 << self.shift
        return np.kron(self.active, np.ones((side, side), bool))[: self.h, : self.w].astype(bool)


def tile_counts(counts, active, pending_a, pending_b):
    """COUNTS PER TILE: NA_t, NB_t (tilesY x tilesX, int64); active None: no plan in force, every tile is active"""
    on = np.ones(counts[0].shape, bool) if active is None else np.asarray(active, bool)
    return counts[0] + np.where(on, pending_a, 0), counts[1] + np.where(on, pending_b, 0)


def meter(A, B, counts, active, pending_a, pending_b, normalize_to, exposure=1.0, threshold=0.0, tile_shift=4, calls=1):
    """One accepted ptx_noise_meter_adaptive: (result, tileErrors, per-pixel decisions with the image PTX_NOISE_WRITE_SUM stores as
    `image`, Q, N and the per-tile sample counts NA, NB)."""
    A = np.ascontiguousarray(A, f32)
    B = np.ascontiguousarray(B, f32)
    h, w = A.shape[:2]
    side = 1 << tile_shift
    tx, ty = tiling(w, h, tile_shift)
    NA, NB = tile_counts(np.asarray(counts, np.int64).reshape(2, ty, tx), active, pending_a, pending_b)
    with np.errstate(all="ignore"):
        S = (A + B).astype(f32)
    image = S.copy()
    rejected = np.zeros((h, w), bool)
    black = np.zeros((h, w), bool)
    q = np.zeros((h, w), np.int64)
    E = np.zeros((ty, tx), f32)
    Q = np.zeros((ty, tx), object)
    N = np.zeros((ty, tx), np.int64)
    conv = np.zeros((ty, tx), bool)
    thr = f32(threshold)
    for j in range(ty):
        for i in range(tx):
            win = (slice(j * side, min(h, (j + 1) * side)), slice(i * side, min(w, (i + 1) * side)))
            na, nb = int(NA[j, i]), int(NB[j, i])
            n = na + nb
            if n != normalize_to and n != 0:
                k = (f32(normalize_to) * NR.rcp(f32(n))).astype(f32)
                with np.errstate(all="ignore"):
                    image[win] = (S[win] * k).astype(f32)
            if na == 0 or nb == 0:   # an unsampled half: every pixel rejected, the tile not converged
                rejected[win] = True
                Q[j, i] = 0
                continue
            p = NR.pixels(A[win], B[win], na, nb, exposure)
            rejected[win], black[win], q[win] = p["rejected"], p["black"], p["q"]
            Q[j, i] = sum(int(v) for v in p["q"].ravel())
            N[j, i] = int(p["counted"].sum())
            E[j, i] = NR.tile_error(Q[j, i], N[j, i])
            conv[j, i] = E[j, i] <= thr
    n_all, q_all = int(N.sum()), sum(int(v) for v in Q.ravel())
    res = dict(meanError=f32(float(q_all) / (float(n_all) * 65536.0)) if n_all else f32(0.0), maxError=f32(E.max()) if n_all else f32(0.0),
               tilesX=tx, tilesY=ty, converged=int(conv.sum()), counted=n_all, black=int(black.sum()), rejected=int(rejected.sum()),
               valid=int(n_all > 0), calls=calls)
    return res, E, dict(S=S, image=image, rejected=rejected, black=black, counted=~rejected, q=q, Q=Q, N=N, NA=NA, NB=NB, converged=conv)
