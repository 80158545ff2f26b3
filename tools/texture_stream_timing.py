#!/usr/bin/env python3
"""Time streamed texture uploads against the blocking upload (docs/EXPERIMENTS.md, "Streamed textures").

Per texture set (32 x 1024^2 and 4 x 4096^2, sRGB8 and RGBA32F), host clock from the first call to a device synchronise,
warm-up plus the median of five runs, the three variants alternating inside each run:
  (a) ptx_texture_upload x n + ptx_textures_commit, chains by k_stream_chain
  (b) the same on a handle created under PTX_STREAM_LEVELWISE=1 (k_blit_level per level)
  (c) the blocking ptx_scene_upload of the same description (its texture stage: the scene's geometry is a few triangles)
and (d) atrium_like with eight frames in flight, Msamples/s while the 1024^2 sRGB set streams in against nothing streaming.
Usage: tools/texture_stream_timing.py [--quick] [--skip-frames]"""
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

os.environ["GPU_MAX_HW_QUEUES"] = "17"  # eight two-stream frames in flight and the upload stream, before HIP starts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402

SRGB, F32 = 1, 2
RUNS = 5


def renderer_with(pkg, levelwise, **kw):
    os.environ["PTX_STREAM_LEVELWISE"] = "1" if levelwise else "0"  # read once, when the handle is created
    try:
        return pkg.Renderer(**kw)
    finally:
        del os.environ["PTX_STREAM_LEVELWISE"]


def texture_set(pkg, rng, count, extent, fmt):
    one = rng.uniform(0, 4, (extent, extent, 4)).astype(np.float32) if fmt == F32 else rng.integers(0, 256, (extent, extent, 4), dtype=np.uint8)
    images = [np.roll(one, 17 * k, axis=1).copy() for k in range(count)]  # distinct pages, one draw of random numbers
    return images, [pkg.TextureDesc(extent, extent, fmt, 1, a.ctypes.data) for a in images]


def with_textures(pkg, desc, table, keep_first=0):
    old = list((pkg.TextureDesc * desc.textureCount).from_address(desc.textures))[:keep_first] if keep_first else []
    arr = (pkg.TextureDesc * (len(old) + len(table)))(*old, *table)
    d = type(desc).from_buffer_copy(desc)
    d.textures, d.textureCount, d.forceFullTextureSize = C.addressof(arr), len(arr), 1
    return d, arr


def pending(pkg, table):
    return [pkg.TextureDesc(t.width, t.height, t.format, t.levels, None) for t in table]


def time_streamed(r, d_pending, table):
    r.upload_streamed(d_pending, None, build=False)
    r.synchronize()
    t0 = time.perf_counter()
    for i, t in enumerate(table):
        r.upload_texture(i, t)
    r.commit_textures()
    r.synchronize()
    return (time.perf_counter() - t0) * 1e3


def time_blocking(r, d_full, d_empty):
    r._check(r.lib.ptx_scene_upload(r.handle, C.byref(d_empty)))
    t_empty = time.perf_counter()
    r._check(r.lib.ptx_scene_upload(r.handle, C.byref(d_empty)))
    t_empty = time.perf_counter() - t_empty
    t0 = time.perf_counter()
    r._check(r.lib.ptx_scene_upload(r.handle, C.byref(d_full)))  # returns after its own stream synchronise
    return (time.perf_counter() - t0 - t_empty) * 1e3


def upload_table(pkg, quick):
    base = pkg.Scene("texture_test")
    rng = np.random.default_rng(3)
    fused, levelwise, blocking = renderer_with(pkg, False), renderer_with(pkg, True), pkg.Renderer()
    d_empty, keep0 = with_textures(pkg, base.desc, [])
    rows = []
    sets = ((4, 256), (2, 512)) if quick else ((32, 1024), (4, 4096))
    for count, extent in sets:
        for fmt in (SRGB, F32):
            images, table = texture_set(pkg, rng, count, extent, fmt)
            d_full, keep1 = with_textures(pkg, base.desc, table)
            d_pend, keep2 = with_textures(pkg, base.desc, pending(pkg, table))
            times = {"fused": [], "levelwise": [], "blocking": []}
            for run in range(RUNS + 1):  # the first run warms every shape up
                a, b, c = time_streamed(fused, d_pend, table), time_streamed(levelwise, d_pend, table), time_blocking(blocking, d_full, d_empty)
                if run:
                    times["fused"].append(a), times["levelwise"].append(b), times["blocking"].append(c)
            med = {k: statistics.median(v) for k, v in times.items()}
            rows.append((count, extent, "sRGB8" if fmt == SRGB else "RGBA32F", med, {k: (min(v), max(v)) for k, v in times.items()}))
            print(f"{count} x {extent}^2 {rows[-1][2]}: per texture, ms: " +
                  ", ".join(f"{k} {med[k] / count:.3f} ({times_[0] / count:.3f} .. {times_[1] / count:.3f})" for k, times_ in rows[-1][4].items()), flush=True)
            del images
    for r in (fused, levelwise, blocking):
        r.close()
    return rows


def frames_in_flight(pkg, quick):
    scene = pkg.Scene("atrium_like", 0.05 if quick else 1.0)
    W, H, spp, steps = (320, 180, 8, 16) if quick else (1920, 1080, 8, 64)
    rng = np.random.default_rng(4)
    images, table = texture_set(pkg, rng, 8 if quick else 32, 256 if quick else 1024, SRGB)
    own = scene.desc.textureCount
    d_pend, keep = with_textures(pkg, scene.desc, pending(pkg, table), keep_first=own)
    owner = pkg.Renderer()
    owner.upload_streamed(d_pend, None)
    ring = [owner] + [pkg.Renderer() for _ in range(7)]
    for r in ring:
        if r is not owner:
            r.share_scene(owner)
        r.resize(W, H)
    u, lights = scene.uniform(W, H, bounces=8), scene.lights
    result = {}

    def run(stream_in):
        nxt = 0
        t0 = time.perf_counter()
        for step in range(steps):
            ring[step % len(ring)].render_frames(u, lights, step * spp, spp)
            if stream_in and nxt < len(table) and step % 2 == 1:
                owner.upload_texture(own + nxt, table[nxt])
                nxt += 1
        if stream_in:
            owner.commit_textures()
        for r in ring:
            r.synchronize()
        return W * H * spp * steps / (time.perf_counter() - t0) / 1e6

    run(False)  # warm-up: the bounce schedule is learnt by the first launches
    for run_ in range(RUNS):
        result.setdefault("idle", []).append(run(False))
        if run_ == 0:  # a texture is streamed in once in its life: the streaming run is one run per process
            result["streaming"] = [run(True)]
    for r in reversed(ring):
        r.close()
    print(f"atrium_like {W}x{H} x {spp} spp, 8 frames in flight: {statistics.median(result['idle']):.0f} Msamples/s idle "
          f"({min(result['idle']):.0f} .. {max(result['idle']):.0f}), {result['streaming'][0]:.0f} while {len(table)} textures stream in", flush=True)
    return result


def main():
    import torch  # noqa: F401  (one HIP runtime in the process)

    pkg = graft.load_package()
    quick = "--quick" in sys.argv
    upload_table(pkg, quick)
    if "--skip-frames" not in sys.argv:
        frames_in_flight(pkg, quick)


if __name__ == "__main__":
    main()
