#!/usr/bin/env python3
"""What ptx_noise_meter's estimate is worth (docs/NEXT_ROWS.md section 26): for `default`, `texture_test` and `atrium_like` at a reduced
extent, meanError, maxError and the share of converged tiles at the package's defaults against the samples taken, beside the relative L2
error of the mean (A + B) / n against the mean of 4,096 samples of the same sequence.  The halves are accumulated by alternating
bindings, one frame per render call, as RendererHip does it.

Not a test and no part of bench.py.  Usage: tools/noise_quality.py [--json FILE] [--extent W H] [--reference N]"""
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


def main():
    pkg = graft.load_package()
    w, h = (int(sys.argv[sys.argv.index("--extent") + k]) for k in (1, 2)) if "--extent" in sys.argv else (320, 180)
    reference = int(sys.argv[sys.argv.index("--reference") + 1]) if "--reference" in sys.argv else 4096
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
