#!/usr/bin/env python3
"""Chooses the denoiser's default parameters (docs/NEXT_ROWS.md section 13) without a GPU: CPU-oracle renders of three scenes at
4 spp against 512 spp, first-hit guides from tests/debug_view_ref.py, the filter of tests/denoise_ref.py.

    python tools/denoise_quality.py            the relative L2 error before / after at the package's defaults, per scene
    python tools/denoise_quality.py --sweep    the same over a grid of parameters, best mean improvement first
    python tools/denoise_quality.py --write    (re)writes tests/golden/denoise_truth_512spp.npz, the 512-spp means as binary16

tests/test_denoise.py's quality test reads that file and recomputes the 4-spp side.
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

SCENES = ("default", "texture_test", "alpha_test")
W, H, DETAIL, BOUNCES, LOW_SPP, HIGH_SPP = 134, 90, 0.25, 4, 4, 512
TRUTH = os.path.join(REPO, "tests", "golden", "denoise_truth_512spp.npz")


def render_sum(orc, scene, spp, first=0):
    """The canonical schedule: one sample per launch, RNG frame = launch index."""
    osc = orc.OracleScene(scene.desc, build_bvh=True)
    acc = np.zeros((H, W, 4), np.float32)
    for f in range(first, first + spp):
        osc.render(scene.uniform(W, H, bounces=BOUNCES, sample_count=1, total_samples=f), scene.lights, W, H, accum=acc)
    return acc


def errors(low, truth, guides, **params):
    den = R.denoise(low, *guides, LOW_SPP, params["iterations"], params["sigma_color"], params["sigma_normal"], params["sigma_position"], np.float32)
    return R.relative_l2(low[..., 0:3] / LOW_SPP, truth), R.relative_l2(den, truth)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--write", action="store_true")
    args = ap.parse_args()
    pkg, orc = graft.load_package(), graft.load_oracle()
    orc.build()
    scenes = {name: pkg.Scene(name, DETAIL) for name in SCENES}
    if args.write or not os.path.exists(TRUTH):
        t0 = time.time()
        # frames LOW_SPP .. : the truth shares no sample with the frame that is denoised
        truth = {name: (render_sum(orc, s, HIGH_SPP, first=LOW_SPP)[..., 0:3] / HIGH_SPP).astype(np.float16) for name, s in scenes.items()}
        np.savez_compressed(TRUTH, **truth)
        print(f"wrote {TRUTH} ({os.path.getsize(TRUTH)} bytes, {time.time() - t0:.0f} s)")
    truth = {k: v.astype(np.float32) for k, v in np.load(TRUTH).items()}
    low = {name: render_sum(orc, s, LOW_SPP) for name, s in scenes.items()}
    guides = {name: R.cpu_guides(pkg, orc, s, W, H) for name, s in scenes.items()}
    if not args.sweep:
        print(f"{W} x {H}, {LOW_SPP} spp against {HIGH_SPP} spp, defaults {pkg.DENOISE_DEFAULTS}")
        for name in SCENES:
            raw, den = errors(low[name], truth[name], guides[name], **pkg.DENOISE_DEFAULTS)
            print(f"  {name:14s} relative L2 error: raw {raw:.4f}  denoised {den:.4f}  ({raw / den:.2f} x)")
        return
    rows = []
    for it, sc, sn, sp in itertools.product((2, 3, 4, 5), (0.0, 1.0, 1.5, 2.0, 3.0, 4.0), (0.1, 0.3, 0.6), (0.01, 0.03, 0.1)):
        p = dict(iterations=it, sigma_color=sc, sigma_normal=sn, sigma_position=sp)
        e = [errors(low[n], truth[n], guides[n], **p) for n in SCENES]
        rows.append((float(np.mean([np.log(d / r) for r, d in e])), p, e))
    rows.sort(key=lambda r: r[0])
    for score, p, e in rows[:25]:
        print(f"{np.exp(score):.3f}  {p}  " + "  ".join(f"{r:.4f}->{d:.4f}" for r, d in e))


if __name__ == "__main__":
    main()
