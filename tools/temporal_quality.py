#!/usr/bin/env python3
"""Measures the temporal accumulation (docs/NEXT_ROWS.md section 14) and chooses the defaults of the filter behind it, without a
GPU: CPU-oracle renders of a camera sliding sideways over three scenes (8 frames of 4 spp, tests/temporal_ref.py's quality sequence),
first-hit guides from tests/debug_view_ref.py, the accumulation of tests/temporal_ref.py and the filter of tests/denoise_ref.py.  The
last frame is compared with a 192-spp render at its pose.

    python tools/temporal_quality.py            the relative L2 error of the last frame: raw, spatial filter, temporal, both
    python tools/temporal_quality.py --sweep    the chained filter over maxHistory x iterations x sigmaColor, best geometric mean first
    python tools/temporal_quality.py --write    (re)writes tests/golden/temporal_truth.npz, the 192-spp means as binary16

tests/test_temporal.py's quality test reads that file and recomputes the sequence; the file holds the two scenes that test uses
(a committed file stays below 100 KB), the truth of the third is rendered on every run of this tool.
"""
import argparse
import itertools
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import __graft_entry__ as graft  # noqa: E402
import denoise_ref as R  # noqa: E402
import temporal_ref as TR  # noqa: E402

SCENES = ("default", "texture_test", "alpha_test")
GOLDEN_SCENES = ("default", "texture_test")
TRUTH = os.path.join(REPO, "tests", "golden", "temporal_truth.npz")


def temporal(frames, max_history, t):
    T, dec = TR.run_sequence(frames, max_history, t["normal_threshold"], t["position_threshold"], np.float32)
    return T[-1], dec


def filtered(image, frame, samples, p):
    return R.denoise(image, frame[1], frame[2], frame[3], samples, p["iterations"], p["sigma_color"], p["sigma_normal"], p["sigma_position"], np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--write", action="store_true")
    args = ap.parse_args()
    pkg, orc = graft.load_package(), graft.load_oracle()
    orc.build()
    t0 = time.time()
    seqs, truth = {}, {}
    write = args.write or not os.path.exists(TRUTH)
    for name in SCENES:
        scene, seqs[name] = TR.quality_sequence(pkg, orc, name)
        if write or name not in GOLDEN_SCENES:  # the scene stands at the last pose
            S = TR.render_oracle_sum(orc, scene, TR.QUALITY_W, TR.QUALITY_H, TR.QUALITY_TRUTH_SPP, TR.QUALITY_TRUTH_FIRST_SAMPLE)
            truth[name] = (S[..., 0:3] / TR.QUALITY_TRUTH_SPP).astype(np.float16)
    print(f"sequences rendered in {time.time() - t0:.0f} s")
    if write:
        np.savez_compressed(TRUTH, **{n: truth[n] for n in GOLDEN_SCENES})
        print(f"wrote {TRUTH} ({os.path.getsize(TRUTH)} bytes)")
    truth.update(np.load(TRUTH).items())
    truth = {k: v.astype(np.float32) for k, v in truth.items()}
    td, dd, cd = pkg.TEMPORAL_DEFAULTS, pkg.DENOISE_DEFAULTS, pkg.TEMPORAL_DENOISE_DEFAULTS
    if not args.sweep:
        print(f"{TR.QUALITY_W} x {TR.QUALITY_H}, {TR.QUALITY_FRAMES} frames of {TR.QUALITY_SPP} spp against {TR.QUALITY_TRUTH_SPP} spp at the last pose")
        print(f"temporal {td}\nspatial alone {dd}\nchained {cd}")
        print("scene (step)            raw     spatial  temporal  chained  chained at the spatial defaults   mean L   restarted")
        for name in SCENES:
            last = seqs[name][-1]
            T, dec = temporal(seqs[name], td["max_history"], td)
            valid = dec[-1]["valid"]
            e = [R.relative_l2(last[0][..., 0:3] / TR.QUALITY_SPP, truth[name]), R.relative_l2(filtered(last[0], last, TR.QUALITY_SPP, dd), truth[name]),
                 R.relative_l2(T, truth[name]), R.relative_l2(filtered(T, last, 1, cd), truth[name]), R.relative_l2(filtered(T, last, 1, dd), truth[name])]
            print(f"  {name:14s}({TR.QUALITY_STEPS[name]:4.2f})  {e[0]:.4f}  {e[1]:.4f}   {e[2]:.4f}    {e[3]:.4f}   {e[4]:.4f}"
                  f"                            {T[..., 3][valid].mean():.2f}     {100.0 * (T[..., 3][valid] == 1).mean():.2f} %")
        return
    rows = []
    for mh in (8.0, 16.0, 32.0, 64.0):
        T = {n: temporal(seqs[n], mh, td)[0] for n in SCENES}
        for it, sc in itertools.product((1, 2, 3), (0.0, 0.5, 0.75, 1.0, 1.5)):
            p = dict(iterations=it, sigma_color=sc, sigma_normal=dd["sigma_normal"], sigma_position=dd["sigma_position"])
            e = [R.relative_l2(filtered(T[n], seqs[n][-1], 1, p), truth[n]) for n in SCENES]
            rows.append((float(np.exp(np.mean(np.log(e)))), mh, it, sc, e))
    rows.sort(key=lambda r: r[0])
    print("geometric mean  maxHistory  iterations  sigmaColor   " + "  ".join(SCENES))
    for score, mh, it, sc, e in rows:
        print(f"{score:.4f}          {mh:4.0f}        {it}           {sc:4.2f}         " + "  ".join(f"{v:.4f}" for v in e))


if __name__ == "__main__":
    main()
