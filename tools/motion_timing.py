#!/usr/bin/env python3
"""Times what the motion guides add (docs/NEXT_ROWS.md section 17) at 1920 x 1080, on animated_test and on one heavy scene:
ptx_render_guides_motion beside ptx_render_guides (with the previous pose the current one, the snapshot, and unknown),
ptx_update_animation with tracking on beside tracking off, and ptx_temporal_accumulate_motion beside the plain and the moments call
(same camera, and two cameras a fraction of a pixel apart in turn so that every call gathers four taps).

The method is tools/screen_path_timing.py's: synchronise, enqueue the call `repeat` times, synchronise; `repeat` chosen per shape so
that a window lasts about five milliseconds, a warm-up first, the median of 20 windows divided by `repeat`.  ptx_update_animation
synchronises by itself and includes its refit.  The whole list is measured `--rounds` times over (5), so that the variants alternate;
a figure is the median of its rounds' medians and comes with their smallest and largest: differences inside that spread are not
differences.  On a checkout without the motion guides (the parent commit) the tool times the plain calls alone, which is how the
parent's figures of docs/NEXT_ROWS.md section 17 were taken, alternating with this tree's in one session.

Not a test and no part of bench.py.  Usage: tools/motion_timing.py [--json FILE] [--detail D] [--heavy SCENE] [--rounds N]"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402,F401  (first, so the HIP library shares torch's HIP runtime)
import __graft_entry__ as graft  # noqa: E402
from screen_path_timing import timed  # noqa: E402

W, H = 1920, 1080
TD = dict(max_history=32.0, normal_threshold=0.3, position_threshold=0.03)


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def poses(pkg, scene):
    """Two poses of the scene: its own animation where it has one, every instance nudged otherwise"""
    a = scene.animation_state()
    if scene.update(0.37):
        return a, scene.animation_state()
    it = a[0].copy()
    it[:, 3] += 0.01
    return a, (it, a[1])


def measure(pkg, scene, r):
    """One round: every call of the list once, in the order a frame makes them"""
    r.resize(W, H)
    u = scene.uniform(W, H, bounces=4)
    cams = [scene.camera_matrices(W, H)]
    pos, fwd, right = (np.frombuffer(u.ViewInverse, np.float32).reshape(4, 4).T[0:3, k].astype(np.float64) for k in (3, 2, 0))
    scene.set_camera_pose(pos + right * 0.002, fwd)
    cams.append(scene.camera_matrices(W, H))
    scene.set_camera_pose(pos, fwd)
    (it0, bn0), (it1, bn1) = poses(pkg, scene)
    bones = lambda b: b if b is not None and len(b) else None  # noqa: E731
    state = {"k": 0}

    def update():
        state["k"] ^= 1
        r.update_animation(it1 if state["k"] else it0, bones(bn1 if state["k"] else bn0))

    def accumulate(call, two_cameras):
        def go():
            state["k"] ^= 1
            call(1, *cams[state["k"] if two_cameras else 0], **TD)
        return go

    rec = {"triangles": int(r.stats().triangles)}
    rec["update_animation_untracked"] = timed(r, update)
    rec["render_guides"] = timed(r, lambda: r.render_guides(u))
    r.render(u, scene.lights)
    for label, two in (("same_camera", False), ("projected", True)):
        rec[f"temporal_accumulate_{label}"] = timed(r, accumulate(r.temporal_accumulate, two))
        rec[f"temporal_accumulate_moments_{label}"] = timed(r, accumulate(r.temporal_accumulate_moments, two))
    if not hasattr(r, "track_motion"):  # a checkout without the motion guides
        return rec
    r.track_motion(True)
    rec["update_animation_tracked"] = timed(r, update)
    r.resize(W, H)  # no history: unknown
    rec["render_guides_motion_unknown"] = timed(r, lambda: r.render_guides_motion(u))
    r.render(u, scene.lights)
    r.temporal_accumulate_motion(1, *cams[0], **TD)
    rec["render_guides_motion_same_pose"] = timed(r, lambda: r.render_guides_motion(u))
    for label, two in (("same_camera", False), ("projected", True)):
        rec[f"temporal_accumulate_motion_{label}"] = timed(r, accumulate(r.temporal_accumulate_motion, two))
        rec[f"temporal_accumulate_motion_moments_{label}"] = timed(r, accumulate(lambda *a, **k: r.temporal_accumulate_motion(*a, moments=True, **k), two))
    r.render_guides_motion(u)
    r.temporal_accumulate_motion(1, *cams[0], **TD)
    update()  # the history is one update old: the snapshot
    rec["render_guides_motion_snapshot"] = timed(r, lambda: r.render_guides_motion(u))
    r.track_motion(False)
    return rec


def rounds_of(pkg, name, detail, rounds):
    """{label: median, smallest and largest of the rounds' medians}"""
    scene = pkg.Scene(name, detail)
    r = pkg.Renderer()
    r.upload(scene)
    runs = [measure(pkg, scene, r) for _ in range(rounds)]
    r.close()
    out = {"triangles": runs[0]["triangles"]}
    for k, v in runs[0].items():
        if isinstance(v, dict):
            ms = np.array([run[k]["median_ms"] for run in runs])
            out[k] = {"median_ms": float(np.median(ms)), "min_ms": float(ms.min()), "max_ms": float(ms.max()), "rounds": rounds}
    return out


def main():
    pkg = graft.load_package()
    detail = float(arg("--detail", 1.0))
    rounds = int(arg("--rounds", 5))
    out = {name: rounds_of(pkg, name, detail, rounds) for name in ("animated_test", arg("--heavy", "atrium_like"))}
    for name, rec in out.items():
        print(f"{name} ({rec['triangles']} triangles) at {W}x{H}")
        for k, v in rec.items():
            if isinstance(v, dict):
                print(f"  {k:52s} {v['median_ms']:9.4f} ms  ({v['rounds']} rounds: {v['min_ms']:.4f} .. {v['max_ms']:.4f})")
    if "--json" in sys.argv:
        with open(arg("--json", None), "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
