#!/usr/bin/env python3
"""What an adaptive plan buys per render call (docs/NEXT_ROWS.md section 27): `chess_like` and `atrium_like` at 1920 x 1080, 8 frames per
ptx_render_frames call, depth 8, 16-pixel tiles, under mask plans of 100, 50, 25 and 10 % of the tiles -- once as one contiguous block of
tile rows from the top, once scattered as a checkerboard-like pattern (tile (i, j) is active iff (i + j) mod m < k, with k / m the share)
-- beside the unplanned call.  The 100 % plan against the unplanned call is the price of the list's indirection and of the schedule
hint that starts anew; the scattered plans against the blocks show what the loss of coherence costs.  Then the cost of
ptx_adaptive_plan itself, its synchronisation included (from a mask and from the meter's records), and of ptx_noise_meter_adaptive
beside ptx_noise_meter on the same halves.

Every figure is a device-synchronised wall-clock time: synchronise, enqueue the call, synchronise; every shape is warmed up first (two
calls, so that the second runs on the learnt schedule) and the figure is the median of 20 windows.

Not a test and no part of bench.py.  Usage: tools/adaptive_timing.py [--json FILE] [--extent W H] [--scenes a,b] [--windows N]"""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402,F401  (first, so the HIP library shares torch's HIP runtime)
import __graft_entry__ as graft  # noqa: E402

FRAMES, DEPTH, SHIFT = 8, 8, 4
SHARES = {100: (1, 1), 50: (1, 2), 25: (1, 4), 10: (1, 10)}


def window(r, call, windows):
    times = []
    for _ in range(windows):
        r.synchronize()
        t0 = time.perf_counter()
        call()
        r.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times)


def masks(tx, ty, share):
    k, m = SHARES[share]
    jj, ii = np.mgrid[0:ty, 0:tx]
    block = (np.arange(tx * ty).reshape(ty, tx) < round(tx * ty * k / m)).astype(np.uint8)
    scattered = (((ii + jj) % m) < k).astype(np.uint8)
    return {"block": block, "scattered": scattered}


def main():
    pkg = graft.load_package()
    w, h = (int(sys.argv[sys.argv.index("--extent") + k]) for k in (1, 2)) if "--extent" in sys.argv else (1920, 1080)
    scenes = sys.argv[sys.argv.index("--scenes") + 1].split(",") if "--scenes" in sys.argv else ["chess_like", "atrium_like"]
    windows = int(sys.argv[sys.argv.index("--windows") + 1]) if "--windows" in sys.argv else 20
    side = 1 << SHIFT
    tx, ty = (w + side - 1) // side, (h + side - 1) // side
    out = {"extent": [w, h], "frames_per_call": FRAMES, "depth": DEPTH, "tile_shift": SHIFT, "scenes": {}}
    for name in scenes:
        scene = pkg.Scene(name, 0.25)
        r = pkg.Renderer()
        r.upload(scene)
        r.resize(w, h)
        u = scene.uniform(w, h, bounces=DEPTH)
        call = lambda: r.render_frames(u, scene.lights, 0, FRAMES)
        rows = []

        def timed(label, plan=None):
            for _ in range(2):
                call()
            ms = window(r, call, windows)
            pixels = plan.activePixels if plan is not None else w * h
            row = {"plan": label, "active_tiles": plan.activeTiles if plan is not None else tx * ty, "active_pixels": pixels, "ms_per_call": ms,
                   "msamples_per_s": pixels * FRAMES / ms / 1e3}
            rows.append(row)
            print(f"{name} {w}x{h}: {json.dumps(row)}", flush=True)
        timed("none")
        for share in SHARES:
            for kind, mask in masks(tx, ty, share).items():
                if share == 100 and kind == "scattered":
                    continue
                timed(f"{share}% {kind}", r.adaptive_plan(SHIFT, mask=mask, dilate=0))
        r.adaptive_clear()
        timed("none again")
        # the calls themselves: on two halves of four frames each
        r.noise_halves(True)
        for f in range(8):
            r.bind_accumulation(r.noise_half_ptr(f & 1), w * h * 16)
            u.TotalSamples = f
            r.render(u, scene.lights)
        r.bind_accumulation(0, 0)
        half_mask = masks(tx, ty, 50)["scattered"]
        r.noise_meter(4, 4, 1.0, 0.02, SHIFT)
        r.adaptive_plan(SHIFT, mask=half_mask, dilate=1)
        calls = {
            "ptx_adaptive_plan from a mask, dilate 1": lambda: r.adaptive_plan(SHIFT, mask=half_mask, dilate=1),
            "ptx_adaptive_plan from the records, dilate 1": lambda: r.adaptive_plan(SHIFT, dilate=1),
            "ptx_noise_meter": lambda: r.noise_meter(4, 4, 1.0, 0.02, SHIFT),
            "ptx_noise_meter_adaptive": lambda: r.noise_meter_adaptive(4, 4, 8, 1.0, 0.02, SHIFT),
            "ptx_noise_meter, WRITE_SUM": lambda: r.noise_meter(4, 4, 1.0, 0.02, SHIFT, write_sum=True),
            "ptx_noise_meter_adaptive, WRITE_SUM": lambda: r.noise_meter_adaptive(4, 4, 8, 1.0, 0.02, SHIFT, write_sum=True),
        }
        for label, fn in calls.items():
            fn()
            row = {"call": label, "ms_per_call": window(r, fn, windows)}
            rows.append(row)
            print(f"{name} {w}x{h}: {json.dumps(row)}", flush=True)
        out["scenes"][name] = rows
        r.close()
    if "--json" in sys.argv:
        with open(sys.argv[sys.argv.index("--json") + 1], "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
