#!/usr/bin/env python3
"""Times the calls between ptx_render and the window (docs/NEXT_ROWS.md sections 12, 13, 14 and 16): ptx_postprocess, ptx_present,
ptx_render_guides, ptx_temporal_accumulate and ptx_temporal_accumulate_moments (both variants each), ptx_denoise, ptx_denoise_temporal,
ptx_denoise_variance and ptx_postprocess_denoised at 1920 x 1080 and 3840 x 2160, beside one 8-spp step of chess_like.

Every figure is a device-synchronised wall-clock time: synchronise, enqueue the call `repeat` times, synchronise; `repeat` is chosen
per shape so that a window lasts about five milliseconds, every shape is warmed up first, and the figure is the median of 20
windows divided by `repeat`.  ptx_denoise is also given as a rate against its algorithmic traffic of 80 bytes per pixel and pass
(16 B in, 16 B out, 48 B of guides) -- a rate, not a measured bandwidth: the 25 taps are served by the caches.
ptx_temporal_accumulate likewise against 176 bytes per pixel (64 B of sum and guides and 48 B of history in, T and 48 B of history
out); its projected variant is called with two cameras a fraction of a pixel apart in turn, so that every call gathers four taps.
ptx_temporal_accumulate_moments adds 16 B of moment history in and out: 208 bytes per pixel.  ptx_denoise_variance is timed on a
history at its cap (every pixel takes mu2 - mu1^2) and, as `_restarted`, right after a PTX_TEMPORAL_RESET (every valid pixel takes
the 7 x 7 window); ptx_denoise_temporal at the same iteration counts stands beside it.

ptx_temporal_accumulate_responsive (section 19) is one call of two launches, accumulate and clamp; it stands right behind the plain call
of the same run, with the difference between the two, and against 240 bytes per pixel: the plain call's 176, 16 B of fast history in and
out, and the clamp's 16 B of fast history and 16 B of colour history in (a clamped pixel reads 16 B of albedo and writes 32 B more,
which the figure leaves out).  --temporal-only times nothing but the accumulate calls; --extent W H takes one extent in place of the
two.  The wall clock cannot take the call's two launches apart: a kernel trace of `--temporal-only --extent W H` (rocprofv3
--kernel-trace --stats, in a run of its own) gives k_responsive_clamp's and k_temporal_responsive's device times per extent.

ptx_despike (section 20) stands behind the responsive rows, and so in the --temporal-only run whose kernel trace holds
k_responsive_clamp: one launch per call at radius 1 and 2, against 37.25 and 43 bytes per pixel (16 B out, 16 B x (tile + halo) / tile in).

ptx_render_guides_specular (section 18) at the package's defaults stands beside ptx_render_guides of the same run on chess_like and on
`default`; --guides-only times nothing but the two guide passes.

ptx_meter and ptx_postprocess_metered (section 21): --meter times nothing but them, on the 8-spp chess_like sum and on a constant
frame (every lane of a wave on one bin: the contention case of the LDS atomics), with ptx_despike at radius 1 (the same 16 bytes per
pixel in) and ptx_postprocess of the same run beside them.  ptx_meter is given against its 16 algorithmic bytes per pixel -- a rate, not
a bandwidth: at 1920 x 1080 the 33 MB frame of a back-to-back run is served from the last-level cache.  A kernel trace of `--meter
--extent W H` gives k_meter_histogram's, k_meter_resolve's and k_despike<1>'s device times.

ptx_grade and ptx_present_graded (section 22): --grade times nothing but them, on the 8-spp chess_like frame behind one ptx_postprocess:
the identity desc, each curve, a CDL grade with and without power, and a 33^3 LUT in the linear and in the sRGB domain, with
ptx_postprocess and ptx_present of the same run beside them.  ptx_grade is one launch of k_compose_grade, which moves k_compose_tonemap's
40 bytes per pixel; a kernel trace of `--grade --extent W H` gives both kernels' device times.

ptx_local_exposure and ptx_postprocess_local (section 23): --local times nothing but them, with ptx_meter, ptx_postprocess and
ptx_postprocess_metered of the same run beside them, on the 8-spp chess_like sum and on a constant frame (every pixel of a cell in one
slice: up to 2^cellShift lanes of a wave on one LDS address, all 64 at cellShift 6 -- the contention case of k_local_splat), at every
cellShift.  ptx_local_exposure is given against 36 algorithmic bytes per pixel (16 B in for the splat, 16 B in and 4 B out for the
gain; the grid is noise beside them at cellShift 5) -- a rate, not a bandwidth.  A kernel trace of `--local --extent W H` gives
k_local_splat's, k_local_blur's, k_local_gain's and k_postprocess_local's device times.

ptx_present_upscaled (section 25): --upscale times nothing but it, at sharpness 0 and 0.5, with ptx_present at the same extents in the
same run beside it: the 8-spp chess_like frame rendered at 1920 x 1080 and shown at 3840 x 2160, and at 1280 x 720 shown at 2560 x 1440,
as an SDR sRGB8 and as an HDR10 surface.  --extent W H takes one render extent in place of the two; the screen is twice it on both axes.
A kernel trace of `--upscale --extent W H` gives k_present_upscaled's and k_present's device times.

ptx_noise_meter (section 26): --noise times nothing but it, with and without PTX_NOISE_WRITE_SUM at every tileShift, on two halves of four
chess_like frames each rendered by alternating bindings, with ptx_despike at radius 1 and ptx_meter of the same run beside it (the
neighbours that read 16 bytes per pixel).  It is given against 32 algorithmic bytes per pixel (both halves in) and 48 with the flag (S
out) -- a rate, not a bandwidth: the halves of a back-to-back run at 1920 x 1080 are 66 MB and fit the last-level cache, at 3840 x 2160
they are 265 MB and do not.  A kernel trace of `--noise --extent W H` gives k_noise_tiles', k_noise_resolve's, k_despike<1>'s and
k_meter_histogram's device times.

Not a test and no part of bench.py.  Usage: tools/screen_path_timing.py [--json FILE] [--detail D] [--guides-only] [--temporal-only] [--meter] [--grade [--desc NAME]] [--local] [--upscale] [--noise] [--extent W H]"""
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402,F401  (first, so the HIP library shares torch's HIP runtime)
import __graft_entry__ as graft  # noqa: E402

WINDOWS, WINDOW_MS, STEP_SPP, STEP_DEPTH = 20, 5.0, 8, 8
POST = dict(exposure=1.0, bloom_threshold=0.8, bloom_intensity=0.35)
DENOISE_BYTES_PER_PIXEL_AND_PASS = 80
TEMPORAL_BYTES_PER_PIXEL = 176
MOMENTS_BYTES_PER_PIXEL = 208
RESPONSIVE_BYTES_PER_PIXEL = 240
GRADE_BYTES_PER_PIXEL = 40  # 24 in (post-process image, bloom level 0), 16 out; the LUT's reads are cache hits
LOCAL_EXPOSURE_BYTES_PER_PIXEL = 36  # the sum twice (splat, gain) and G out; the grid is 2 x 16 B x 32 slices per cell
NOISE_BYTES_PER_PIXEL = {False: 32, True: 48}  # both halves in; S out with PTX_NOISE_WRITE_SUM; tile and workgroup records are noise beside them
METER_BYTES_PER_PIXEL = 16  # one load of the pixel; the slabs (1 MB at the most) and the state are noise beside it
# 16 B out and 16 B x (tile + halo) / tile in: the halo is 84 entries of 256 at radius 1 and 176 at radius 2
DESPIKE_BYTES_PER_PIXEL = {1: 16 + 16 * (256 + 84) / 256, 2: 16 + 16 * (256 + 176) / 256}


def timed(r, call):
    """Median over WINDOWS windows of the device-synchronised time of one call, in milliseconds."""
    def window(repeat):
        r.synchronize()
        t0 = time.perf_counter()
        for _ in range(repeat):
            call()
        r.synchronize()
        return (time.perf_counter() - t0) * 1e3 / repeat
    window(1)  # warm-up of the shape: allocations, code objects
    repeat = max(1, math.ceil(WINDOW_MS / max(window(2), 1e-3)))
    ms = np.array([window(repeat) for _ in range(WINDOWS)])
    return {"median_ms": float(np.median(ms)), "min_ms": float(ms.min()), "max_ms": float(ms.max()), "repeat": repeat}


def main():
    pkg = graft.load_package()
    detail = float(sys.argv[sys.argv.index("--detail") + 1]) if "--detail" in sys.argv else 1.0
    out = {}
    guides_only, temporal_only, meter_only = "--guides-only" in sys.argv, "--temporal-only" in sys.argv, "--meter" in sys.argv
    grade_only, local_only, upscale_only = "--grade" in sys.argv, "--local" in sys.argv, "--upscale" in sys.argv
    noise_only = "--noise" in sys.argv
    scenes = {name: pkg.Scene(name, detail) for name in (("chess_like",) if temporal_only or meter_only or grade_only or local_only or upscale_only or noise_only else ("chess_like", "default") if guides_only else
                                                          ("chess_like", "atrium_like", "default"))}
    renderers = {}
    for name, scene in scenes.items():
        renderers[name] = pkg.Renderer()
        renderers[name].upload(scene)
    extents = ((1920, 1080), (1280, 720)) if upscale_only else ((1920, 1080), (3840, 2160))
    if "--extent" in sys.argv:
        extents = ((int(sys.argv[sys.argv.index("--extent") + 1]), int(sys.argv[sys.argv.index("--extent") + 2])),)
    for w, h in extents:
        rec = {}
        scene, r = scenes["chess_like"], renderers["chess_like"]
        r.resize(w, h)
        u = scene.uniform(w, h, bounces=STEP_DEPTH)

        def specular_row(name, rg, ug):  # right behind the plain pass of the same scene
            t = timed(rg, lambda: rg.render_guides_specular(ug))
            t["ratio_to_render_guides"] = t["median_ms"] / rec[f"render_guides_{name}"]["median_ms"]
            rec[f"render_guides_specular_{name}"] = t

        def default_rows():
            sd, rd = scenes["default"], renderers["default"]
            rd.resize(w, h)
            ud = sd.uniform(w, h, bounces=STEP_DEPTH)
            rec["render_guides_default"] = timed(rd, lambda: rd.render_guides(ud))
            specular_row("default", rd, ud)
        if upscale_only:
            r.reset()
            r.render_frames(u, scene.lights, 0, STEP_SPP)
            sw, sh = 2 * w, 2 * h
            for surface, fmt, mode in (("sdr_srgb8", pkg.PRESENT_R8G8B8A8_SRGB, pkg.TONE_MAPPING_SDR), ("hdr10", pkg.PRESENT_A2B10G10R10_UNORM, pkg.TONE_MAPPING_HDR)):
                r.postprocess(STEP_SPP, tone_mapping=mode, **POST)
                base = timed(r, lambda: r.present(sw, sh, fmt, mode))
                rec[f"present_to_{sw}x{sh}_{surface}"] = base
                for sharpness in (0.0, 0.5):
                    t = timed(r, lambda: r.present_upscaled(sw, sh, fmt, mode, sharpness=sharpness))
                    t["ratio_to_present"] = t["median_ms"] / base["median_ms"]
                    rec[f"present_upscaled_to_{sw}x{sh}_{surface}_sharpness_{sharpness}"] = t
                rec[f"present_to_{sw}x{sh}_{surface}_again"] = timed(r, lambda: r.present(sw, sh, fmt, mode))
            out[f"{w}x{h}"] = rec
            for k, v in rec.items():
                print(f"{w}x{h} {k}: {json.dumps(v)}", flush=True)
            continue
        if grade_only:
            r.reset()
            r.render_frames(u, scene.lights, 0, STEP_SPP)
            rec["postprocess"] = timed(r, lambda: r.postprocess(STEP_SPP, **POST))
            rec["present_own_size"] = timed(r, lambda: r.present(w, h))
            n = 33
            g = np.arange(n, dtype=np.float32) / np.float32(n - 1)
            lut = np.stack(np.broadcast_arrays(g[None, None, :], g[None, :, None], g[:, None, None]), axis=-1) ** np.float32(0.9)
            r.set_lut(lut)
            cdl = dict(slope=(1.1, 0.9, 1.0), offset=(0.01, -0.02, 0.0), saturation=1.3)
            descs = {"identity": {}, "reinhard": dict(curve=pkg.CURVE_REINHARD), "hable": dict(curve=pkg.CURVE_HABLE), "aces_fit": dict(curve=pkg.CURVE_ACES_FIT),
                     "matrix_cdl_hable": dict(cdl, colour_matrix=pkg.white_balance_matrix(4500.0), curve=pkg.CURVE_HABLE),
                     "cdl_power_hable": dict(cdl, power=(0.9, 1.1, 1.2), curve=pkg.CURVE_HABLE),
                     "hable_lut33": dict(curve=pkg.CURVE_HABLE, use_lut=True), "hable_lut33_srgb_domain": dict(curve=pkg.CURVE_HABLE, use_lut=True, lut_srgb_domain=True)}
            if "--desc" in sys.argv:  # one desc alone, so that a kernel trace of the run shows k_compose_grade under that desc
                descs = {sys.argv[sys.argv.index("--desc") + 1]: descs[sys.argv[sys.argv.index("--desc") + 1]]}
            for name, d in descs.items():
                t = timed(r, lambda: r.grade(**d))
                t["algorithmic_GB_per_s"] = w * h * GRADE_BYTES_PER_PIXEL / (t["median_ms"] * 1e-3) / 1e9
                rec[f"grade_{name}"] = t
                rec[f"present_graded_own_size_{name}"] = timed(r, lambda: r.present_graded(w, h))
            out[f"{w}x{h}"] = rec
            for k, v in rec.items():
                print(f"{w}x{h} {k}: {json.dumps(v)}", flush=True)
            continue
        if local_only:
            r.reset()
            r.render_frames(u, scene.lights, 0, STEP_SPP)
            frames = {"chess_like_8spp": None, "constant": np.full((h, w, 4), 0.18 * STEP_SPP, np.float32)}
            for frame, image in frames.items():
                if image is not None:
                    r.write_accumulation(image)
                rec[f"meter_average_{frame}"] = timed(r, lambda: r.meter(STEP_SPP, delta_seconds=1.0 / 60))
                rec[f"postprocess_{frame}"] = timed(r, lambda: r.postprocess(STEP_SPP, **POST))
                rec[f"postprocess_metered_{frame}"] = timed(r, lambda: r.postprocess_metered(STEP_SPP, **POST))
                for shift in (3, 4, 5, 6):
                    t = timed(r, lambda: r.local_exposure(STEP_SPP, cell_shift=shift, pivot_metered=True))
                    t["algorithmic_GB_per_s"] = w * h * LOCAL_EXPOSURE_BYTES_PER_PIXEL / (t["median_ms"] * 1e-3) / 1e9
                    rec[f"local_exposure_shift_{shift}_{frame}"] = t
                r.local_exposure(STEP_SPP, pivot_metered=True)  # the package's defaults: cellShift 5
                G = r.read_local_exposure()
                rec[f"local_exposure_result_{frame}"] = {"min_gain": float(G.min()), "max_gain": float(G.max()), "exposure": r.read_meter().exposure}
                rec[f"postprocess_local_{frame}"] = timed(r, lambda: r.postprocess_local(STEP_SPP, metered=True, **POST))
            out[f"{w}x{h}"] = rec
            for k, v in rec.items():
                print(f"{w}x{h} {k}: {json.dumps(v)}", flush=True)
            continue
        if noise_only:
            half = STEP_SPP // 2
            r.noise_halves(True)
            for f in range(STEP_SPP):
                r.bind_accumulation(r.noise_half_ptr(f & 1), w * h * 16)
                u.TotalSamples = f
                r.render(u, scene.lights)
            r.bind_accumulation(0, 0)
            for write_sum in (False, True):
                for shift in (3, 4, 5, 6):
                    t = timed(r, lambda: r.noise_meter(half, half, POST["exposure"], tile_shift=shift, write_sum=write_sum))
                    t["algorithmic_GB_per_s"] = w * h * NOISE_BYTES_PER_PIXEL[write_sum] / (t["median_ms"] * 1e-3) / 1e9
                    rec[f"noise_meter_shift_{shift}{'_write_sum' if write_sum else ''}"] = t
            res = r.read_noise()
            rec["noise_result"] = {"mean_error": res.meanError, "max_error": res.maxError, "converged": res.converged, "tiles": res.tilesX * res.tilesY,
                                   "counted": res.counted, "black": res.black, "rejected": res.rejected}
            p1 = dict(pkg.DESPIKE_DEFAULTS, radius=1, min_taps=max(3, pkg.DESPIKE_DEFAULTS["rank"]))
            rec["despike_radius_1"] = timed(r, lambda: r.despike(**p1))  # on the internal image, which holds A + B now
            t = timed(r, lambda: r.meter(STEP_SPP, delta_seconds=1.0 / 60))
            t["algorithmic_GB_per_s"] = w * h * METER_BYTES_PER_PIXEL / (t["median_ms"] * 1e-3) / 1e9
            rec["meter_average"] = t
            r.noise_halves(False)
            out[f"{w}x{h}"] = rec
            for k, v in rec.items():
                print(f"{w}x{h} {k}: {json.dumps(v)}", flush=True)
            continue
        if meter_only:
            r.reset()
            r.render_frames(u, scene.lights, 0, STEP_SPP)
            p1 = dict(pkg.DESPIKE_DEFAULTS, radius=1, min_taps=max(3, pkg.DESPIKE_DEFAULTS["rank"]))
            rec["despike_radius_1"] = timed(r, lambda: r.despike(**p1))
            rec["postprocess"] = timed(r, lambda: r.postprocess(STEP_SPP, **POST))
            frames = {"chess_like_8spp": None, "constant": np.full((h, w, 4), 0.18 * STEP_SPP, np.float32)}
            for frame, image in frames.items():
                if image is not None:
                    r.write_accumulation(image)
                for mode, name in ((pkg.METER_AVERAGE, "average"), (pkg.METER_CENTRE, "centre"), (pkg.METER_REGION, "region_of_a_quarter")):
                    region = (w // 4, w // 4 + w // 2, h // 4, h // 4 + h // 2)
                    t = timed(r, lambda: r.meter(STEP_SPP, delta_seconds=1.0 / 60, mode=mode, region=region))
                    t["algorithmic_GB_per_s"] = w * h * METER_BYTES_PER_PIXEL * (0.25 if mode == pkg.METER_REGION else 1.0) / (t["median_ms"] * 1e-3) / 1e9
                    rec[f"meter_{name}_{frame}"] = t
                res = r.read_meter()
                rec[f"meter_result_{frame}"] = {"exposure": res.exposure, "avg_log2": res.avgLog2, "counted": res.counted, "black": res.black}
                rec[f"postprocess_metered_{frame}"] = timed(r, lambda: r.postprocess_metered(STEP_SPP, **POST))
            out[f"{w}x{h}"] = rec
            for k, v in rec.items():
                print(f"{w}x{h} {k}: {json.dumps(v)}", flush=True)
            continue
        if guides_only:
            rec["render_guides_chess_like"] = timed(r, lambda: r.render_guides(u))
            specular_row("chess_like", r, u)
            default_rows()
            out[f"{w}x{h}"] = rec
            for k, v in rec.items():
                print(f"{w}x{h} {k}: {json.dumps(v)}", flush=True)
            continue
        if not temporal_only:
            rec["render_8spp_step_chess_like"] = timed(r, lambda: r.render_frames(u, scene.lights, 0, STEP_SPP))
        r.reset()
        r.render_frames(u, scene.lights, 0, STEP_SPP)
        if not temporal_only:
            rec["postprocess"] = timed(r, lambda: r.postprocess(STEP_SPP, **POST))
        screens = [(w, h)] + ([(3840, 2160)] if (w, h) == (1920, 1080) else [])
        for sw, sh in ([] if temporal_only else screens):
            r.postprocess(STEP_SPP, tone_mapping=pkg.TONE_MAPPING_SDR, **POST)
            rec[f"present_to_{sw}x{sh}_sdr_srgb8"] = timed(r, lambda: r.present(sw, sh, pkg.PRESENT_R8G8B8A8_SRGB, pkg.TONE_MAPPING_SDR))
            r.postprocess(STEP_SPP, tone_mapping=pkg.TONE_MAPPING_HDR, **POST)
            rec[f"present_to_{sw}x{sh}_hdr10"] = timed(r, lambda: r.present(sw, sh, pkg.PRESENT_A2B10G10R10_UNORM, pkg.TONE_MAPPING_HDR))
        if not temporal_only:
            rec["render_guides_chess_like"] = timed(r, lambda: r.render_guides(u))
            specular_row("chess_like", r, u)
        r.render_guides(u)  # what follows is timed on first-hit guides, as it always was
        cams = [scene.camera_matrices(w, h)]
        pos, fwd, right = (np.frombuffer(u.ViewInverse, np.float32).reshape(4, 4).T[0:3, k].astype(np.float64) for k in (3, 2, 0))
        scene.set_camera_pose(pos + right * 0.002, fwd)
        cams.append(scene.camera_matrices(w, h))
        scene.set_camera_pose(pos, fwd)
        calls = [0]

        def accumulate(moving):
            calls[0] += 1
            r.temporal_accumulate(STEP_SPP, *cams[calls[0] % 2 if moving else 0])
        for key, moving in (("temporal_accumulate_same_camera", False), ("temporal_accumulate_projected", True)):
            t = timed(r, lambda: accumulate(moving))
            t["algorithmic_GB_per_s"] = w * h * TEMPORAL_BYTES_PER_PIXEL / (t["median_ms"] * 1e-3) / 1e9
            rec[key] = t

        def accumulate_responsive(moving, flags):
            calls[0] += 1
            r.temporal_accumulate_responsive(STEP_SPP, *cams[calls[0] % 2 if moving else 0], responsive_flags=flags)
        for key, moving, flags, base in (("temporal_accumulate_responsive_same_camera", False, 0, "temporal_accumulate_same_camera"),
                                         ("temporal_accumulate_responsive_projected", True, 0, "temporal_accumulate_projected"),
                                         ("temporal_accumulate_responsive_moments_projected", True, pkg.RESPONSIVE_MOMENTS, None)):
            t = timed(r, lambda: accumulate_responsive(moving, flags))
            t["algorithmic_GB_per_s"] = w * h * (RESPONSIVE_BYTES_PER_PIXEL + (32 if flags else 0)) / (t["median_ms"] * 1e-3) / 1e9
            if base:
                t["minus_plain_call_ms"] = t["median_ms"] - rec[base]["median_ms"]
            T = r.read_temporal()
            t["share_of_valid_pixels_below_max_history"] = float((T[..., 3][T[..., 3] > 0] < pkg.TEMPORAL_DEFAULTS["max_history"]).mean())
            rec[key] = t
        # ptx_despike (section 20) on the 8-spp sum, both radii at the package's rank, gain and a third of the window: one launch each
        for radius, min_taps in ((1, 3), (2, 8)):
            p = dict(pkg.DESPIKE_DEFAULTS, radius=radius, min_taps=max(min_taps, pkg.DESPIKE_DEFAULTS["rank"]))
            t = timed(r, lambda: r.despike(**p))
            t["algorithmic_GB_per_s"] = w * h * DESPIKE_BYTES_PER_PIXEL[radius] / (t["median_ms"] * 1e-3) / 1e9
            rec[f"despike_radius_{radius}"] = t
        if temporal_only:
            out[f"{w}x{h}"] = rec
            for k, v in rec.items():
                print(f"{w}x{h} {k}: {json.dumps(v)}", flush=True)
            continue

        def accumulate_moments(moving):
            calls[0] += 1
            r.temporal_accumulate_moments(STEP_SPP, *cams[calls[0] % 2 if moving else 0])
        for key, moving in (("temporal_accumulate_moments_projected", True), ("temporal_accumulate_moments_same_camera", False)):
            t = timed(r, lambda: accumulate_moments(moving))
            t["algorithmic_GB_per_s"] = w * h * MOMENTS_BYTES_PER_PIXEL / (t["median_ms"] * 1e-3) / 1e9
            rec[key] = t
        for it in (1, 3, 5):  # the history stands at its cap after the windows above
            rec[f"denoise_temporal_{it}_iterations"] = timed(r, lambda: r.denoise_temporal(iterations=it))
            rec[f"denoise_variance_{it}_iterations"] = timed(r, lambda: r.denoise_variance(iterations=it))
        r.temporal_accumulate_moments(STEP_SPP, *cams[0], flags=pkg.TEMPORAL_RESET)
        for it in (1, 3, 5):
            rec[f"denoise_variance_{it}_iterations_restarted"] = timed(r, lambda: r.denoise_variance(iterations=it))
        for it in (1, 3, 5):
            t = timed(r, lambda: r.denoise(STEP_SPP, iterations=it))
            t["algorithmic_GB_per_s"] = w * h * DENOISE_BYTES_PER_PIXEL_AND_PASS * it / (t["median_ms"] * 1e-3) / 1e9
            rec[f"denoise_{it}_iterations"] = t
        r.denoise(STEP_SPP)
        rec["postprocess_denoised"] = timed(r, lambda: r.postprocess_denoised(**POST))
        d = pkg.DENOISE_DEFAULTS
        frame = rec["render_guides_chess_like"]["median_ms"] + rec[f"denoise_{d['iterations']}_iterations"]["median_ms"]
        rec["guides_plus_default_denoise_share_of_8spp_step"] = frame / rec["render_8spp_step_chess_like"]["median_ms"]
        a, ra = scenes["atrium_like"], renderers["atrium_like"]
        ra.resize(w, h)
        ua = a.uniform(w, h, bounces=STEP_DEPTH)
        rec["render_guides_atrium_like"] = timed(ra, lambda: ra.render_guides(ua))
        default_rows()
        out[f"{w}x{h}"] = rec
        for k, v in rec.items():
            print(f"{w}x{h} {k}: {json.dumps(v)}", flush=True)
    for r in renderers.values():
        r.close()
    if "--json" in sys.argv:
        with open(sys.argv[sys.argv.index("--json") + 1], "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
