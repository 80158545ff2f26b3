#!/usr/bin/env python3
"""Chooses the defaults of the firefly suppression (docs/NEXT_ROWS.md section 20) without a GPU: tools/denoise_quality.py's CPU-oracle
renders of three scenes against its 512-spp truth, at 1 and 4 spp, the rank clamp of tests/firefly_ref.py (unguided, float32) and
the filter of tests/denoise_ref.py at DENOISE_DEFAULTS behind it.

    python tools/firefly_quality.py             the table at DESPIKE_DEFAULTS: raw -> despiked / filter -> despiked + filter, pixels clamped
    python tools/firefly_quality.py --sweep     radius {1, 2} x rank {1 .. 4} x gain {1, 1.5, 2, 3}, minTaps a third of the window rounded
                                                up (and at least the rank), ranked by the geometric mean of the error behind the filter; then the winner's table
    python tools/firefly_quality.py --temporal  tools/temporal_quality.py's three sliding-camera sequences, last frame: plain temporal +
                                                filter against despiked -> temporal + filter (reported, not asserted)

tests/test_fireflies.py's quality test recomputes the 4-spp side of the table."""
import argparse
import itertools
import math
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tools"))

import __graft_entry__ as graft  # noqa: E402
import denoise_quality as DQ  # noqa: E402
import denoise_ref as R  # noqa: E402
import firefly_ref as FR  # noqa: E402

SPPS = (1, 4)
RADII, RANKS, GAINS = (1, 2), (1, 2, 3, 4), (1.0, 1.5, 2.0, 3.0)


def min_taps_of(radius, rank=1):
    """a third of the window, rounded up: 3 and 8 -- and never below the rank, which the call refuses (rank 4 at radius 1: 4)"""
    return max(math.ceil(((2 * radius + 1) ** 2 - 1) / 3), rank)


def despiked(S, p):
    return FR.despike(S, p["radius"], p["rank"], p["min_taps"], p["gain"], np.float32)


def filtered(S, guides, spp, dd):
    return R.denoise(S, *guides, spp, dd["iterations"], dd["sigma_color"], dd["sigma_normal"], dd["sigma_position"], np.float32)


def cell(S, truth, guides, spp, p, dd, base=None):
    """(raw, despiked, filter, despiked + filter, share clamped) -- relative L2 of the mean against the truth"""
    C, dec = despiked(S, p)
    raw, flt = base if base else (R.relative_l2(S[..., 0:3] / spp, truth), R.relative_l2(filtered(S, guides, spp, dd), truth))
    return raw, R.relative_l2(C[..., 0:3] / spp, truth), flt, R.relative_l2(filtered(C, guides, spp, dd), truth), float(dec["clamped"].mean())


def table(cases, p, dd, bases):
    print(f"{p}\nscene, spp          raw -> despiked / filter -> despiked + filter    pixels clamped")
    for key, (S, truth, guides, spp) in cases.items():
        raw, des, flt, both, share = cell(S, truth, guides, spp, p, dd, bases[key])
        print(f"  {key[0]:14s}{key[1]}   {raw:.4f} -> {des:.4f} / {flt:.4f} -> {both:.4f}                    {100.0 * share:.1f} %")


def temporal_table(pkg, orc, p):
    import temporal_quality as TQ
    import temporal_ref as TR

    td, cd = pkg.TEMPORAL_DEFAULTS, pkg.TEMPORAL_DENOISE_DEFAULTS
    print(f"{TR.QUALITY_W} x {TR.QUALITY_H}, {TR.QUALITY_FRAMES} frames of {TR.QUALITY_SPP} spp, last frame; temporal {td}, filter {cd}\n"
          "scene           temporal -> despiked + temporal / temporal + filter -> despiked + temporal + filter")
    stored = dict(np.load(TQ.TRUTH).items())
    for name in TQ.SCENES:
        scene, frames = TR.quality_sequence(pkg, orc, name)
        if name in stored:
            truth = stored[name].astype(np.float32)
        else:  # the scene stands at the last pose
            truth = TR.render_oracle_sum(orc, scene, TR.QUALITY_W, TR.QUALITY_H, TR.QUALITY_TRUTH_SPP, TR.QUALITY_TRUTH_FIRST_SAMPLE)[..., 0:3] / TR.QUALITY_TRUTH_SPP
        clean = [(despiked(f[0], p)[0],) + tuple(f[1:]) for f in frames]
        e = []
        for seq in (frames, clean):
            T = TQ.temporal(seq, td["max_history"], td)[0]
            e += [R.relative_l2(T, truth), R.relative_l2(TQ.filtered(T, seq[-1], 1, cd), truth)]
        print(f"  {name:14s}{e[0]:.4f} -> {e[2]:.4f} / {e[1]:.4f} -> {e[3]:.4f}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--temporal", action="store_true")
    args = ap.parse_args()
    pkg, orc = graft.load_package(), graft.load_oracle()
    orc.build()
    dd = pkg.DENOISE_DEFAULTS
    if args.temporal:
        return temporal_table(pkg, orc, pkg.DESPIKE_DEFAULTS)
    scenes = {name: pkg.Scene(name, DQ.DETAIL) for name in DQ.SCENES}
    truth = {k: v.astype(np.float32) for k, v in np.load(DQ.TRUTH).items()}
    guides = {name: R.cpu_guides(pkg, orc, s, DQ.W, DQ.H) for name, s in scenes.items()}
    cases = {}
    for name, s in scenes.items():
        osc = orc.OracleScene(s.desc, build_bvh=True)
        acc = np.zeros((DQ.H, DQ.W, 4), np.float32)
        for f in range(max(SPPS)):  # denoise_quality.render_sum's schedule: the 1-spp sum is the first launch of the 4-spp one
            osc.render(s.uniform(DQ.W, DQ.H, bounces=DQ.BOUNCES, sample_count=1, total_samples=f), s.lights, DQ.W, DQ.H, accum=acc)
            if f + 1 in SPPS:
                cases[(name, f + 1)] = (acc.copy(), truth[name], guides[name], f + 1)
    bases = {k: (R.relative_l2(S[..., 0:3] / spp, t), R.relative_l2(filtered(S, g, spp, dd), t)) for k, (S, t, g, spp) in cases.items()}
    p = dict(pkg.DESPIKE_DEFAULTS)
    if args.sweep:
        rows = []
        for radius, rank, gain in itertools.product(RADII, RANKS, GAINS):
            q = dict(radius=radius, rank=rank, gain=gain, min_taps=min_taps_of(radius, rank))
            e = [cell(*cases[k], q, dd, bases[k]) for k in cases]
            rows.append((float(np.exp(np.mean([np.log(c[3]) for c in e]))), q, e))
        rows.sort(key=lambda r: r[0])
        print(f"filter alone: geometric mean {float(np.exp(np.mean([np.log(b[1]) for b in bases.values()]))):.4f}")
        print("geometric mean behind the filter   parameters   " + "  ".join(f"{k[0]}@{k[1]}" for k in cases))
        for score, q, e in rows:
            print(f"{score:.4f}  {q}  " + "  ".join(f"{c[3]:.4f}" for c in e))
        p = rows[0][1]
        edge = [name for name, grid in (("radius", RADII), ("rank", RANKS), ("gain", GAINS)) if p[name] in (grid[0], grid[-1])]
        print(f"winner {p}" + (f": on the edge of the grid in {', '.join(edge)}" if edge else ": inside the grid"))
        if p != pkg.DESPIKE_DEFAULTS:
            print(f"NOTE: DESPIKE_DEFAULTS is {pkg.DESPIKE_DEFAULTS}")
    table(cases, p, dd, bases)


if __name__ == "__main__":
    main()
