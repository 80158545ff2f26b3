#!/usr/bin/env python3
"""Measures what the specular-chain guides (docs/NEXT_ROWS.md section 18) do to the denoised image and chooses the defaults of
ptx_render_guides_specular, without a GPU: CPU-oracle renders at 134 x 90, detail 0.25, depth 4, 4 spp (the recipe of
tools/denoise_quality.py), guides from tests/specular_guides_ref.py (maxBounces 0: the first-hit guides), the filter of
tests/denoise_ref.py and the accumulation of tests/temporal_ref.py.

    python tools/specular_guides_quality.py                    first-hit against specular guides at the package's defaults: the relative
                                                               L2 error on all pixels and on the pixels with bounces > 0, for the
                                                               spatial chain (`default` against tests/golden/denoise_truth_512spp.npz)
                                                               and the temporal + filter chain (the eight-frame sliding camera of
                                                               tests/temporal_ref.py against tests/golden/temporal_truth.npz)
    python tools/specular_guides_quality.py --specular-sweep   roughnessMax x maxBounces on `default` and `roughness_cubes`, ranked by the
                                                               geometric mean of the relative L2 error after the filter at DENOISE_DEFAULTS
    python tools/specular_guides_quality.py --write            (re)writes tests/golden/specular_truth_512spp.npz: roughness_cubes at 512 spp

tests/test_specular_guides.py's quality test recomputes the first mode's figures on the pixels with bounces > 0.
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
import debug_view_ref as DV  # noqa: E402
import denoise_ref as R  # noqa: E402
import specular_guides_ref as SR  # noqa: E402
import temporal_ref as TR  # noqa: E402

W, H, DETAIL, BOUNCES, LOW_SPP, HIGH_SPP = 134, 90, 0.25, 4, 4, 512
TRUTH = os.path.join(REPO, "tests", "golden", "denoise_truth_512spp.npz")
TEMPORAL_TRUTH = os.path.join(REPO, "tests", "golden", "temporal_truth.npz")
OWN_TRUTH = os.path.join(REPO, "tests", "golden", "specular_truth_512spp.npz")  # roughness_cubes, which the two files above lack
SWEEP_SCENES = ("default", "roughness_cubes")
SWEEP_ROUGHNESS, SWEEP_BOUNCES = (0.0, 0.05, 0.1, 0.2, 0.4), (1, 2, 4, 8)


def render_sum(orc, scene, spp, first=0):
    """The canonical schedule: one sample per launch, RNG frame = launch index."""
    osc = orc.OracleScene(scene.desc, build_bvh=True)
    acc = np.zeros((H, W, 4), np.float32)
    for f in range(first, first + spp):
        osc.render(scene.uniform(W, H, bounces=BOUNCES, sample_count=1, total_samples=f), scene.lights, W, H, accum=acc)
    return acc


def guides(orc, scene, max_bounces, roughness_max):
    """(the three guide images as float32, the chain length per pixel) of the scene at its current pose"""
    rs = DV.RefScene(orc, scene.desc)
    r = SR.render(rs, scene.uniform(W, H), W, H, max_bounces, roughness_max, np.float32)
    rs.close()
    return [r[k].astype(np.float32) for k in ("normal", "position", "albedo")], r["bounces"]


def relative_l2(img, truth, mask=None):
    a, b = np.asarray(img, np.float64)[..., 0:3], np.asarray(truth, np.float64)[..., 0:3]
    if mask is not None:
        a, b = a[mask], b[mask]
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def spatial(low, g, p):
    return R.denoise(low, *g, LOW_SPP, p["iterations"], p["sigma_color"], p["sigma_normal"], p["sigma_position"], np.float32)


def spatial_case(pkg, orc, max_bounces, roughness_max):
    """`default`, 4 spp against 512: (D with first-hit guides, D with specular guides, truth, the pixels with bounces > 0)"""
    scene = pkg.Scene("default", DETAIL)
    truth = np.load(TRUTH)["default"].astype(np.float32)
    low = render_sum(orc, scene, LOW_SPP)
    first, _ = guides(orc, scene, 0, 0.0)
    spec, bounces = guides(orc, scene, max_bounces, roughness_max)
    return spatial(low, first, pkg.DENOISE_DEFAULTS), spatial(low, spec, pkg.DENOISE_DEFAULTS), truth, bounces > 0


def temporal_case(pkg, orc, max_bounces, roughness_max):
    """The sliding camera on `default`, temporal accumulation + the filter behind it at the package's defaults, the last frame against
    192 spp: (D with first-hit guides, D with specular guides, truth, the pixels with bounces > 0 in the last frame)"""
    scene = pkg.Scene("default", TR.QUALITY_DETAIL)
    pos, fwd, right = TR.scene_pose(scene, W, H)
    td, cd = pkg.TEMPORAL_DEFAULTS, pkg.TEMPORAL_DENOISE_DEFAULTS
    seq = {"first": [], "specular": []}
    for f in range(TR.QUALITY_FRAMES):
        scene.set_camera_pose(pos + right * (TR.QUALITY_STEPS["default"] * f), fwd)
        S = TR.render_oracle_sum(orc, scene, W, H, TR.QUALITY_SPP, f * TR.QUALITY_SPP)
        view, proj = scene.camera_matrices(W, H)
        for kind, (cap, rmax) in (("first", (0, 0.0)), ("specular", (max_bounces, roughness_max))):
            g, bounces = guides(orc, scene, cap, rmax)
            seq[kind].append((S, *g, TR.QUALITY_SPP, view, proj, 0))
    out = []
    for kind in ("first", "specular"):
        T, _ = TR.run_sequence(seq[kind], td["max_history"], td["normal_threshold"], td["position_threshold"], np.float32)
        last = seq[kind][-1]
        out.append(R.denoise(T[-1], last[1], last[2], last[3], 1, cd["iterations"], cd["sigma_color"], cd["sigma_normal"], cd["sigma_position"], np.float32))
    truth = np.load(TEMPORAL_TRUTH)["default"].astype(np.float32)
    return out[0], out[1], truth, bounces > 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--specular-sweep", action="store_true")
    ap.add_argument("--write", action="store_true")
    args = ap.parse_args()
    pkg, orc = graft.load_package(), graft.load_oracle()
    orc.build()
    d = pkg.SPECULAR_GUIDES_DEFAULTS
    if args.write:
        t0 = time.time()
        s = pkg.Scene("roughness_cubes", DETAIL)
        np.savez_compressed(OWN_TRUTH, roughness_cubes=(render_sum(orc, s, HIGH_SPP, first=LOW_SPP)[..., 0:3] / HIGH_SPP).astype(np.float16))
        print(f"wrote {OWN_TRUTH} ({os.path.getsize(OWN_TRUTH)} bytes, {time.time() - t0:.0f} s)")
    if not args.specular_sweep:
        print(f"{W} x {H}, defaults {d}; relative L2 error, first-hit guides -> specular guides")
        for label, case in (("spatial chain (4 spp, DENOISE_DEFAULTS)", spatial_case), ("temporal + filter chain (8 frames of 4 spp)", temporal_case)):
            a, b, truth, chains = case(pkg, orc, d["max_bounces"], d["roughness_max"])
            print(f"  {label:46s} all pixels {relative_l2(a, truth):.4f} -> {relative_l2(b, truth):.4f}   "
                  f"the {int(chains.sum())} pixels with bounces > 0 {relative_l2(a, truth, chains):.4f} -> {relative_l2(b, truth, chains):.4f}")
        return
    truth = {"default": np.load(TRUTH)["default"].astype(np.float32), "roughness_cubes": np.load(OWN_TRUTH)["roughness_cubes"].astype(np.float32)}
    scenes = {n: pkg.Scene(n, DETAIL) for n in SWEEP_SCENES}
    low = {n: render_sum(orc, s, LOW_SPP) for n, s in scenes.items()}
    base = {n: relative_l2(spatial(low[n], guides(orc, scenes[n], 0, 0.0)[0], pkg.DENOISE_DEFAULTS), truth[n]) for n in SWEEP_SCENES}
    rows = []
    for rmax, cap in itertools.product(SWEEP_ROUGHNESS, SWEEP_BOUNCES):
        e = [relative_l2(spatial(low[n], guides(orc, scenes[n], cap, rmax)[0], pkg.DENOISE_DEFAULTS), truth[n]) for n in SWEEP_SCENES]
        rows.append((float(np.exp(np.mean(np.log(e)))), rmax, cap, e))
    rows.sort(key=lambda r: (r[0], r[2], r[1]))  # ties: fewer bounces, then the lower threshold
    print("first-hit guides: " + "  ".join(f"{n} {base[n]:.4f}" for n in SWEEP_SCENES))
    print("geometric mean  roughnessMax  maxBounces   " + "  ".join(SWEEP_SCENES))
    for score, rmax, cap, e in rows:
        print(f"{score:.4f}          {rmax:4.2f}          {cap}            " + "  ".join(f"{v:.4f}" for v in e))


if __name__ == "__main__":
    main()
