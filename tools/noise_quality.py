#!/usr/bin/env python3
"""What ptx_noise_meter's estimate is worth (docs/NEXT_ROWS.md section 26): for `default`, `texture_test` and `atrium_like` at a reduced
extent, meanError, maxError and the share of converged tiles at the package's defaults against the samples taken, beside the relative L2
error of the mean (A + B) / n against the mean of 4,096 samples of the same sequence.  The halves are accumulated by alternating
bindings, one frame per render call, as RendererHip does it.

--adaptive (docs/NEXT_ROWS.md section 27): instead, the path samples and the wall clock to "every tile converged" of the uniform render and of
the adaptive one with a margin of 0 and of 1 tile (a check every CheckEvery render calls from MinSamples on, as RendererHip does it), and
the relative L2 error of each stopped image against the same reference.

Not a test and no part of bench.py.  Usage: tools/noise_quality.py [--json FILE] [--extent W H] [--reference N] [--adaptive]"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402,F401  (first, so the HIP library shares torch's HIP runtime)
import __graft_entry__ as graft  # noqa: E402

SCENES = ("default", "texture_test", "atrium_like")
DEPTH = 4


def to_convergence(pkg, r, scene, w, h, cap, dilate):
    """One render to "every tile converged" (or `cap` samples): uniform (dilate None) or adaptive.  The stopped mean, and the figures."""
    import time

    d = pkg.NOISE_DEFAULTS
    every, shift = d["check_every"], d["tile_shift"]
    r.noise_halves(True)  # zeroes the halves and the counts
    r.adaptive_clear()
    u = scene.uniform(w, h, bounces=DEPTH)
    traced, active, n, counts = 0, w * h, 0, False
    res = None
    r.synchronize()
    t0 = time.perf_counter()
    while n < cap:
        r.bind_accumulation(r.noise_half_ptr(n & 1), w * h * 16)
        u.TotalSamples = n
        r.render(u, scene.lights)
        n += 1
        traced += active
        if n % every or n < d["min_samples"]:
            continue
        if dilate is None:
            r.noise_meter(n // 2, n // 2, 1.0, d["threshold"], shift)
        else:
            if counts:
                r.noise_meter_adaptive(every // 2, every // 2, n, 1.0, d["threshold"], shift)
                plan = r.adaptive_plan(shift, dilate=dilate, frames_a=every // 2, frames_b=every // 2)
            else:  # the first check: every tile has every sample
                r.noise_meter(n // 2, n // 2, 1.0, d["threshold"], shift)
                plan = r.adaptive_plan(shift, dilate=dilate, frames_a=n // 2, frames_b=n // 2)
            counts = True
            active = plan.activePixels
        res = r.read_noise()
        if res.converged == res.tilesX * res.tilesY:
            break
    r.synchronize()
    seconds = time.perf_counter() - t0
    if dilate is None:
        r.noise_meter(n // 2, n - n // 2, 1.0, d["threshold"], shift, write_sum=True)
    else:
        r.noise_meter_adaptive(0, 0, n, 1.0, d["threshold"], shift, write_sum=True)
    r.bind_accumulation(0, 0)
    mean = r.readback()[..., :3].astype(np.float64) / n
    r.adaptive_clear()
    return mean, {"dilate": dilate, "stop_samples": n, "converged": bool(res and res.converged == res.tilesX * res.tilesY), "path_samples": traced,
                  "samples_per_pixel": traced / (w * h), "seconds": seconds}


def adaptive_main(pkg, w, h, reference):
    out = {"extent": [w, h], "reference_samples": reference, "scenes": {}}
    for name in SCENES:
        scene = pkg.Scene(name, 0.25)
        r = pkg.Renderer()
        r.upload(scene)
        r.resize(w, h)
        u = scene.uniform(w, h, bounces=DEPTH)
        for f in range(reference):  # the reference: one sum of the same sequence
            u.TotalSamples = f
            r.render(u, scene.lights)
        ref = r.readback()[..., :3].astype(np.float64) / reference
        norm = max(float(np.linalg.norm(ref)), 1e-30)
        rows = []
        for dilate in (None, None, 0, 1):  # the first uniform run warms up and is dropped
            mean, row = to_convergence(pkg, r, scene, w, h, reference, dilate)
            row["rel_l2_to_reference"] = float(np.linalg.norm(mean - ref)) / norm
            rows.append(row)
        for row in rows[1:]:
            print(f"{name} {w}x{h}: {json.dumps(row)}", flush=True)
        out["scenes"][name] = rows[1:]
        r.close()
    return out


def main():
    pkg = graft.load_package()
    w, h = (int(sys.argv[sys.argv.index("--extent") + k]) for k in (1, 2)) if "--extent" in sys.argv else (320, 180)
    reference = int(sys.argv[sys.argv.index("--reference") + 1]) if "--reference" in sys.argv else 4096
    if "--adaptive" in sys.argv:
        out = adaptive_main(pkg, w, h, reference)
        if "--json" in sys.argv:
            with open(sys.argv[sys.argv.index("--json") + 1], "w") as f:
                json.dump(out, f, indent=1)
        return
    checkpoints = [n for n in (4, 8, 16, 32, 64, 128, 256, 512, 1024, 2048) if n < reference]
    d = pkg.NOISE_DEFAULTS
    out = {"extent": [w, h], "reference_samples": reference, "threshold": d["threshold"], "tile_shift": d["tile_shift"], "scenes": {}}
    for name in SCENES:
        scene = pkg.Scene(name, 0.25)
        r = pkg.Renderer()
        r.upload(scene)
        r.resize(w, h)
        r.noise_halves(True)
        u = scene.uniform(w, h, bounces=DEPTH)
        rows, means = [], {}
        for f in range(reference):
            r.bind_accumulation(r.noise_half_ptr(f & 1), w * h * 16)
            u.TotalSamples = f
            r.render(u, scene.lights)
            n = f + 1
            if n in checkpoints or n == reference:
                r.noise_meter(n // 2, n // 2, 1.0, d["threshold"], d["tile_shift"], write_sum=True)
                res = r.read_noise()
                r.bind_accumulation(0, 0)
                means[n] = r.readback()[..., :3].astype(np.float64) / n
                rows.append({"samples": n, "mean_error": res.meanError, "max_error": res.maxError, "converged_share": res.converged / (res.tilesX * res.tilesY),
                             "black": res.black, "rejected": res.rejected})
        ref = means[reference]
        norm = max(float(np.linalg.norm(ref)), 1e-30)
        for row in rows:
            row["rel_l2_to_reference"] = float(np.linalg.norm(means[row["samples"]] - ref)) / norm
            print(f"{name} {w}x{h}: {json.dumps(row)}", flush=True)
        out["scenes"][name] = rows
        r.close()
    if "--json" in sys.argv:
        with open(sys.argv[sys.argv.index("--json") + 1], "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
