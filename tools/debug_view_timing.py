#!/usr/bin/env python3
"""Time the debug view against a one-sample, one-bounce path-traced frame (docs/EXPERIMENTS.md, "The debug view").

Per scene (atrium_like, chess_like) at 1920 x 1080: ptx_render_debug in the Color mode with shadows, and ptx_render with
SampleCount 1 and BounceCount 1, timed by the HIP events around the launch (PtxStats.lastRenderMs), median of 20 after 3 warm-ups,
the two alternating twice; then the Color mode without shadows, WorldPosition and Instance for where the time goes.  Prints the ray
counts beside every time.  Usage: tools/debug_view_timing.py [--json FILE]"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402,F401  (first, so the HIP library shares torch's HIP runtime)
import __graft_entry__ as graft  # noqa: E402

W, H, WARM_UP, RUNS = 1920, 1080, 3, 20


def main():
    pkg = graft.load_package()
    out = {}
    for name in ("atrium_like", "chess_like"):
        scene = pkg.Scene(name)
        lights = scene.lights
        r = pkg.Renderer()
        r.upload(scene)
        r.resize(W, H)
        u = scene.uniform(W, H, bounces=1, sample_count=1)

        def timed(launch):
            ms = []
            for k in range(WARM_UP + RUNS):
                launch(k)
                st = r.stats()
                ms.append(st.lastRenderMs)
            ms = np.array(ms[WARM_UP:])
            return {"median_ms": float(np.median(ms)), "min_ms": float(ms.min()), "max_ms": float(ms.max()),
                    "segments": int(st.segments), "shadowRays": int(st.shadowRays)}

        def path_trace(k):
            u.TotalSamples = k
            r.render(u, lights)

        rec = {"triangles": scene.triangle_count, "LightCount": int(lights.LightCount)}
        for rep in range(2):
            rec[f"path_trace_1spp_1bounce_{rep}"] = timed(path_trace)
            rec[f"debug_color_shadows_{rep}"] = timed(lambda k: r.render_debug(u, lights, pkg.DEBUG_MODE_COLOR))
        rec["debug_color_no_shadows"] = timed(lambda k: r.render_debug(u, lights, pkg.DEBUG_MODE_COLOR, 0, pkg.DEBUG_HIT_DISABLE_SHADOWS))
        rec["debug_world_position"] = timed(lambda k: r.render_debug(u, lights, pkg.DEBUG_MODE_WORLD_POSITION))
        rec["debug_instance"] = timed(lambda k: r.render_debug(u, lights, pkg.DEBUG_MODE_INSTANCE))
        out[name] = rec
        print(name, json.dumps(rec), flush=True)
        r.close()
    if "--json" in sys.argv:
        with open(sys.argv[sys.argv.index("--json") + 1], "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
