#!/usr/bin/env python3
"""Measures the temporal accumulation (docs/NEXT_ROWS.md section 14) and chooses the defaults of the filter behind it, without a
GPU: CPU-oracle renders of a camera sliding sideways over three scenes (8 frames of 4 spp, tests/temporal_ref.py's quality sequence),
first-hit guides from tests/debug_view_ref.py, the accumulation of tests/temporal_ref.py and the filter of tests/denoise_ref.py.  The
last frame is compared with a 192-spp render at its pose.

    python tools/temporal_quality.py            the relative L2 error of the last frame: raw, spatial filter, temporal, both
    python tools/temporal_quality.py --sweep    the chained filter over maxHistory x iterations x sigmaColor, best geometric mean first,
                                                then the variance-guided filter (section 16, tests/variance_ref.py) over iterations x
                                                sigmaLuminance at 8, 4, 2 and 1 frames of history
    python tools/temporal_quality.py --write    (re)writes tests/golden/temporal_truth.npz, the 192-spp means as binary16
    python tools/temporal_quality.py --responsive   the responsive history (section 19, tests/responsive_ref.py): two sequences with a
                                                moving light on animated_test and the three sliding-camera sequences as controls; the
                                                sweep fastHistory x clampSigma, best geometric mean first, and the table at
                                                RESPONSIVE_DEFAULTS; with --write also tests/golden/responsive_truth.npz

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
import variance_ref as VR  # noqa: E402
import responsive_ref as RR  # noqa: E402

SCENES = ("default", "texture_test", "alpha_test")
GOLDEN_SCENES = ("default", "texture_test")
TRUTH = os.path.join(REPO, "tests", "golden", "temporal_truth.npz")
RESPONSIVE_TRUTH = os.path.join(REPO, "tests", "golden", "responsive_truth.npz")
FAST_HISTORIES, CLAMP_SIGMAS = (2.0, 4.0, 8.0), (1.0, 1.5, 2.0, 3.0, 4.0)


def temporal(frames, max_history, t):
    T, dec = TR.run_sequence(frames, max_history, t["normal_threshold"], t["position_threshold"], np.float32)
    return T[-1], dec


def filtered(image, frame, samples, p):
    return R.denoise(image, frame[1], frame[2], frame[3], samples, p["iterations"], p["sigma_color"], p["sigma_normal"], p["sigma_position"], np.float32)


HISTORIES = (8, 4, 2, 1)  # frames of history: the last k frames of the sequence, so the pose and the truth stay
VARIANCE_ITERATIONS, VARIANCE_SIGMAS = (2, 3, 4, 5), (0.35, 0.5, 0.75, 1.0, 1.5, 2.0)


def moments(frames, t):
    """(T, moments, V_0) of the last frame after ptx_temporal_accumulate_moments over `frames`"""
    Ts, Ms, _ = VR.run_sequence(frames, t["max_history"], t["normal_threshold"], t["position_threshold"], np.float32)
    last = frames[-1]
    return Ts[-1], Ms[-1], VR.estimate(Ts[-1], last[1], last[2], last[3], Ms[-1], 0.3, 0.03, np.float32)[0]


def variance_guided(T, V0, frame, p, iterations=None):
    """D per iteration count up to p['iterations'] (or `iterations`)"""
    return VR.filter_all(T, frame[1], frame[2], frame[3], V0, iterations or p["iterations"], p["sigma_luminance"], p["sigma_normal"], p["sigma_position"],
                         np.float32)[0]


def responsive(frames, t, fast_history, clamp_sigma):
    """(T of the last frame, share of the valid pixels clamped per frame) of ptx_temporal_accumulate_responsive over `frames`"""
    T, _, _, _, dec = RR.run_sequence(frames, t["max_history"], t["normal_threshold"], t["position_threshold"], fast_history, clamp_sigma, np.float32)
    return T[-1], [float(d["clamped"].sum()) / max(1, int(d["valid"].sum())) for d in dec]


def responsive_main(pkg, orc, write):
    t0 = time.time()
    td, dd, cd = pkg.TEMPORAL_DEFAULTS, pkg.DENOISE_DEFAULTS, pkg.TEMPORAL_DENOISE_DEFAULTS
    shared = RR.light_scene(pkg, orc)
    seqs = {kind: RR.light_sequence(shared, pkg, kind) for kind in RR.LIGHT_SEQUENCES}
    truth = {}
    if write or not os.path.exists(RESPONSIVE_TRUTH):
        lit = RR.render_lit(shared, pkg, RR.LIGHT_X_TO, TR.QUALITY_TRUTH_SPP, TR.QUALITY_TRUTH_FIRST_SAMPLE)
        np.savez_compressed(RESPONSIVE_TRUTH, light=(lit[..., 0:3] / TR.QUALITY_TRUTH_SPP).astype(np.float16))
        print(f"wrote {RESPONSIVE_TRUTH} ({os.path.getsize(RESPONSIVE_TRUTH)} bytes)")
    light = np.load(RESPONSIVE_TRUTH)["light"].astype(np.float32)
    for kind in RR.LIGHT_SEQUENCES:
        truth[kind] = light
    # how much the two end positions differ: the 192-spp means with the light at either end
    start = RR.render_lit(shared, pkg, RR.LIGHT_X_FROM, TR.QUALITY_TRUTH_SPP, 2 * TR.QUALITY_TRUTH_FIRST_SAMPLE)[..., 0:3] / TR.QUALITY_TRUTH_SPP
    valid = shared[2][0][..., 3] == 1
    la, lb = VR.lum(start, np.float32)[valid], VR.lum(light, np.float32)[valid]
    with np.errstate(all="ignore"):
        ratio = np.maximum(la, lb) / np.minimum(la, lb)
    print(f"light at x = {RR.LIGHT_X_FROM} and at x = {RR.LIGHT_X_TO}: the luminance differs by more than a factor of 2 on {100.0 * (ratio > 2).mean():.1f} % of the "
          f"{int(valid.sum())} valid pixels")
    controls = np.load(TRUTH)
    for name in SCENES:
        scene, seqs[name] = TR.quality_sequence(pkg, orc, name)
        if name in controls:
            truth[name] = controls[name].astype(np.float32)
        else:
            S = TR.render_oracle_sum(orc, scene, TR.QUALITY_W, TR.QUALITY_H, TR.QUALITY_TRUTH_SPP, TR.QUALITY_TRUTH_FIRST_SAMPLE)
            truth[name] = (S[..., 0:3] / TR.QUALITY_TRUTH_SPP).astype(np.float16).astype(np.float32)
    names = list(RR.LIGHT_SEQUENCES) + list(SCENES)
    print(f"sequences rendered in {time.time() - t0:.0f} s")
    rows = []
    for fh, cs in itertools.product(FAST_HISTORIES, CLAMP_SIGMAS):
        e = [R.relative_l2(responsive(seqs[n], td, fh, cs)[0], truth[n]) for n in names]
        rows.append((float(np.exp(np.mean(np.log(e)))), fh, cs, e))
    rows.sort(key=lambda r: r[0])
    print(f"temporal {td}\ngeometric mean  fastHistory  clampSigma   " + "  ".join(names))
    for score, fh, cs, e in rows:
        print(f"{score:.4f}          {fh:4.0f}         {cs:4.2f}         " + "  ".join(f"{v:.4f}" for v in e))
    rd = pkg.RESPONSIVE_DEFAULTS
    print(f"head of the list: fast_history {rows[0][1]}, clamp_sigma {rows[0][2]}; RESPONSIVE_DEFAULTS {rd}\nchained {cd}, spatial alone {dd}")
    print("sequence        raw     spatial  temporal  chained  responsive  responsive chained   clamped, mean over the frames / last frame")
    for n in names:
        last = seqs[n][-1]
        spp = last[4]
        T = temporal(seqs[n], td["max_history"], td)[0]
        Tr, share = responsive(seqs[n], td, rd["fast_history"], rd["clamp_sigma"])
        e = [R.relative_l2(last[0][..., 0:3] / spp, truth[n]), R.relative_l2(filtered(last[0], last, spp, dd), truth[n]), R.relative_l2(T, truth[n]),
             R.relative_l2(filtered(T, last, 1, cd), truth[n]), R.relative_l2(Tr, truth[n]), R.relative_l2(filtered(Tr, last, 1, cd), truth[n])]
        print(f"  {n:14s}{e[0]:.4f}  {e[1]:.4f}   {e[2]:.4f}    {e[3]:.4f}   {e[4]:.4f}      {e[5]:.4f}               {100.0 * np.mean(share):.1f} % / {100.0 * share[-1]:.1f} %")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--write", action="store_true")
    ap.add_argument("--responsive", action="store_true")
    args = ap.parse_args()
    pkg, orc = graft.load_package(), graft.load_oracle()
    orc.build()
    if args.responsive:
        return responsive_main(pkg, orc, args.write)
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
    td, dd, cd, vd = pkg.TEMPORAL_DEFAULTS, pkg.DENOISE_DEFAULTS, pkg.TEMPORAL_DENOISE_DEFAULTS, pkg.VARIANCE_DENOISE_DEFAULTS
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
        print(f"variance-guided {vd}\nscene           frames of history   temporal  chained  variance-guided   pixels on the 7 x 7 window")
        for name in SCENES:
            for k in HISTORIES:
                frames = seqs[name][-k:]
                T, M, V0 = moments(frames, td)
                e = [R.relative_l2(T, truth[name]), R.relative_l2(filtered(T, frames[-1], 1, cd), truth[name]),
                     R.relative_l2(variance_guided(T, V0, frames[-1], vd)[-1], truth[name])]
                valid = R.valid_mask(T, frames[-1][1], frames[-1][2], 1, np.float32)
                print(f"  {name:14s}  {k}                 {e[0]:.4f}    {e[1]:.4f}   {e[2]:.4f}            {100.0 * (M.L[valid] < VR.LONG_HISTORY).mean():.1f} %")
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
    for k in HISTORIES:
        rows = []
        est = {n: moments(seqs[n][-k:], td) for n in SCENES}
        for sl in VARIANCE_SIGMAS:
            p = dict(sigma_luminance=sl, sigma_normal=vd["sigma_normal"], sigma_position=vd["sigma_position"])
            D = {n: variance_guided(est[n][0], est[n][2], seqs[n][-1], p, max(VARIANCE_ITERATIONS)) for n in SCENES}
            for it in VARIANCE_ITERATIONS:
                e = [R.relative_l2(D[n][it - 1], truth[n]) for n in SCENES]
                rows.append((float(np.exp(np.mean(np.log(e)))), it, sl, e))
        rows.sort(key=lambda r: r[0])
        print(f"variance-guided, {k} frames of history\ngeometric mean  iterations  sigmaLuminance   " + "  ".join(SCENES))
        for score, it, sl, e in rows:
            print(f"{score:.4f}          {it}           {sl:4.2f}             " + "  ".join(f"{v:.4f}" for v in e))


if __name__ == "__main__":
    main()
