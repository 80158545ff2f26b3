#!/usr/bin/env python3
"""Times the upload of block-compressed textures (docs/NEXT_ROWS.md section 15) against the RGBA8 route on the same blocks.

Cases: one 4096 x 4096 BC1 texture with its full chain, the same in BC3, 256 textures of 512 x 512 BC1 through the blocking
upload (ptx_scene_upload) and the same 256 through the streamed one (ptx_scene_upload_streamed, 256 ptx_texture_upload, one
ptx_textures_commit).  Per case:
  rgba8     the route before the block formats: the host decodes the DDS file to RGBA8 (TextureImporter::DecodeDds through
            pth_decode_image, timed on its own) and uploads 4 B per texel with the file's chain; decode + upload is the baseline
  blocks    the blocks as they are, k_decode_bc with one thread per texel
  rows      the same with one thread per block row and four stores (PTX_BC_MAPPING=rows, read when the handle is created)
Algorithmic bytes per texel: 0.5 (BC1) / 1 (BC3) in and 16 out for the block route, 4 in over the bus, 4 + 16 on the device
for RGBA8.

Every figure is a device-synchronised wall-clock time: the upload calls return after their stream has drained, the streamed case
ends with ptx_synchronize.  Median of 20 after a warm-up (the host decode: median of 5).  The scene around the textures is
texture_test's geometry, the same in every column.  Not a test and no part of bench.py.
Usage: tools/bc_upload_timing.py [--json FILE] [--quick]"""
import ctypes as C
import json
import os
import struct
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402,F401  (first, so the HIP library shares torch's HIP runtime)
import __graft_entry__ as graft  # noqa: E402

REPEATS, DECODE_REPEATS = 20, 5
BLOCK_BYTES = {3: 8, 4: 8, 5: 16, 6: 16}
TWIN = {3: 0, 4: 1, 5: 1, 6: 0}


def full_levels(w, h):
    return max(w, h).bit_length()


def chain_bytes(w, h, fmt):
    return sum(((max(w >> l, 1) + 3) // 4) * ((max(h >> l, 1) + 3) // 4) for l in range(full_levels(w, h))) * BLOCK_BYTES[fmt]


def dds_file(blocks, w, h, fmt):
    levels = full_levels(w, h)
    hdr = struct.pack("<4s7I44x", b"DDS ", 124, 0x1007 | 0x20000, h, w, 0, 0, levels)
    hdr += struct.pack("<2I4s5I", 32, 4, b"DXT1" if BLOCK_BYTES[fmt] == 8 else b"DXT5", 0, 0, 0, 0, 0) + struct.pack("<5I", 0x1000, 0, 0, 0, 0)
    return hdr + bytes(blocks)


def median_ms(call, repeats):
    call()  # warm-up: allocations, code objects
    ms = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        call()
        ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms))


def main():
    pkg = graft.load_package()
    host = pkg.load_host()
    quick = "--quick" in sys.argv
    big, many, side = (1024, 16, 128) if quick else (4096, 256, 512)
    rng = np.random.default_rng(1)
    scene = pkg.Scene("texture_test")
    renderers = {}
    for name, mapping in (("blocks", None), ("rows", "rows")):
        if mapping:
            os.environ["PTX_BC_MAPPING"] = mapping
        renderers[name] = pkg.Renderer()
        os.environ.pop("PTX_BC_MAPPING", None)

    def desc_of(table):
        arr = (pkg.TextureDesc * len(table))(*table)
        d = type(scene.desc).from_buffer_copy(scene.desc)
        d.textures, d.textureCount, d.textureMemoryBudget, d.forceFullTextureSize = C.addressof(arr), len(table), 2**64 - 1, 1
        return d, arr

    def blocking(r, d):
        def call():
            r._check(r.lib.ptx_scene_upload(r.handle, C.byref(d)))
        return call

    def streamed(r, pending, table):
        def call():
            r._check(r.lib.ptx_scene_upload_streamed(r.handle, C.byref(pending), None))
            for i, t in enumerate(table):
                r._check(r.lib.ptx_texture_upload(r.handle, i, C.byref(t)))
            r.commit_textures()
            r.synchronize()
        return call

    out = {}
    for case, (w, h, fmt, count, stream) in {
        f"one_{big}x{big}_bc1": (big, big, 4, 1, False), f"one_{big}x{big}_bc3": (big, big, 5, 1, False),
        f"{many}x_{side}x{side}_bc1_blocking": (side, side, 4, many, False), f"{many}x_{side}x{side}_bc1_streamed": (side, side, 4, many, True),
    }.items():
        levels = full_levels(w, h)
        texels = sum(max(w >> l, 1) * max(h >> l, 1) for l in range(levels))
        blocks = [rng.integers(0, 256, chain_bytes(w, h, fmt), dtype=np.uint8) for _ in range(count)]
        files = [dds_file(b, w, h, fmt) for b in blocks]
        rgba = [np.empty(texels * 4, np.uint8) for _ in range(count)]
        info = (C.c_uint32 * 4)()

        def decode():
            for f, px in zip(files, rgba):
                if host.pth_decode_image(f, len(f), info, px.ctypes.data, px.nbytes):
                    raise RuntimeError(host.pth_last_error().decode())
        rec = {"texels": texels * count, "block_bytes": sum(len(b) for b in blocks), "rgba8_bytes": texels * 4 * count}
        rec["host_decode_ms"] = median_ms(decode, DECODE_REPEATS)
        tables = {"rgba8": [pkg.TextureDesc(w, h, TWIN[fmt], levels, px.ctypes.data) for px in rgba],
                  "blocks": [pkg.TextureDesc(w, h, fmt, levels, b.ctypes.data) for b in blocks]}
        for column, r, table in (("rgba8", renderers["blocks"], tables["rgba8"]), ("blocks", renderers["blocks"], tables["blocks"]),
                                 ("rows", renderers["rows"], tables["blocks"])):
            d, keep = desc_of(table)
            if stream:
                pending, keep2 = desc_of([pkg.TextureDesc(t.width, t.height, t.format, t.levels, None) for t in table])
                rec[f"{column}_upload_ms"] = median_ms(streamed(r, pending, table), REPEATS)
            else:
                rec[f"{column}_upload_ms"] = median_ms(blocking(r, d), REPEATS)
        rec["rgba8_route_ms"] = rec["host_decode_ms"] + rec["rgba8_upload_ms"]
        rec["speedup_blocks"] = rec["rgba8_route_ms"] / rec["blocks_upload_ms"]
        out[case] = rec
        print(f"{case:34s} host decode {rec['host_decode_ms']:9.2f} ms + rgba8 upload {rec['rgba8_upload_ms']:9.2f} ms = {rec['rgba8_route_ms']:9.2f} ms | "
              f"blocks {rec['blocks_upload_ms']:9.2f} ms | rows {rec['rows_upload_ms']:9.2f} ms | x{rec['speedup_blocks']:.1f}", flush=True)
    for r in renderers.values():
        r.close()
    if "--json" in sys.argv:
        with open(sys.argv[sys.argv.index("--json") + 1], "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
