"""The frame's hand-over (csrc/pt_frame_host.hpp, FrameState / OutputState) and the shard geometry it is filled from
(csrc/pt_shard_layout.hpp).

Without a GPU: shardLayout as a stand-alone host program, plain and under the address / undefined-behaviour sanitizers, against the
numpy wording of include/ptx.h (util.shard_entries) on every case of util.SHARD_CASES and three tiny shapes.

On the GPU, at 40x24 with 8-pixel tiles and three ranks: what tests/test_shard_gather.py (test_state_machine_of_a_bound_shard,
test_bind_accumulation_uses_the_callers_image) and tests/test_gpu_parity.py (test_pipelined_readback_paths) leave open about
which call drops which part of the frame's state.  Every buffer the device writes lies between sentinel guards."""
import functools
import os
import subprocess

import numpy as np
import pytest

import util

W, H, WORLD, TILE = 40, 24, 3, 8
SENTINEL = np.uint32(util.SHARD_SENTINEL)
GUARD = 64  # sentinel entries (16 bytes each) either side of a buffer
TINY = [(1, 1, 1, 8), (8, 8, 3, 8), (9, 17, 2, 16)]  # one pixel; one tile for three ranks: two own nothing; ragged both ways

_PROGRAM = r"""
#include "pt_shard_layout.hpp"
#include <cstdio>
#include <cstdlib>
int main(int argc, char **argv) // W H world tile, four numbers per case
{
    for (int i = 1; i + 3 < argc; i += 4)
    {
        const uint32_t w = (uint32_t)strtoul(argv[i], nullptr, 10), h = (uint32_t)strtoul(argv[i + 1], nullptr, 10);
        const uint32_t world = (uint32_t)strtoul(argv[i + 2], nullptr, 10), tile = (uint32_t)strtoul(argv[i + 3], nullptr, 10);
        for (uint32_t rank = 0; rank < world; rank++)
        {
            const ShardLayout s = shardLayout(w, h, rank, world, tile);
            printf("%u %u %u %u %u %u %u %u %u %u\n", w, h, world, tile, rank, s.tilesX, s.numTiles, s.ownedTiles, s.slotsPerFrame, s.ownedPixels);
        }
    }
    return 0;
}
"""


@functools.lru_cache(maxsize=None)
def _reference(w, h, rank, world, tile):
    """(owned tiles, entries, entries inside the image) of one rank's message, from util.shard_entries; computed once"""
    e = util.shard_entries(w, h, rank, world, tile)
    return len(e) // tile ** 2, len(e), int((e >= 0).sum())


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]], ids=["plain", "asan-ubsan"])
def test_shard_layout_header_alone_against_the_numpy_wording(pkg, tmp_path, flags):
    """pt_shard_layout.hpp compiles with the host compiler and nothing else, and for every rank of every case its ownedTiles,
    slotsPerFrame and ownedPixels are those of util.shard_entries; no rank's message is longer than rank 0's."""
    src, exe = tmp_path / "layout.cpp", tmp_path / "layout"
    src.write_text(_PROGRAM)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *flags, "-I", os.path.join(pkg.PKG_DIR, "csrc"), str(src), "-o", str(exe)])
    cases = list(util.SHARD_CASES) + TINY
    done = subprocess.run([str(exe)] + [str(v) for c in cases for v in c], capture_output=True, text=True, timeout=120)
    assert done.returncode == 0 and not done.stderr, done.stderr
    got = {}
    for line in done.stdout.split("\n")[:-1]:
        v = [int(x) for x in line.split()]
        got[tuple(v[:5])] = v[5:]
    assert len(got) == sum(c[2] for c in cases)
    for case in cases:
        w, h, world, tile = case
        slots = []
        for rank in range(world):
            tiles_x, num_tiles, owned, per_frame, pixels = got[case + (rank,)]
            assert (tiles_x, num_tiles) == (-(-w // tile), -(-w // tile) * -(-h // tile)), case
            assert (owned, per_frame, pixels) == _reference(w, h, rank, world, tile), (case, rank)
            slots.append(per_frame)
        assert max(slots) == slots[0], case
    assert [got[(8, 8, 3, 8, r)][2] for r in range(3)] == [1, 0, 0]


# ---------------------------------------------------------------------------------------
# the device
# ---------------------------------------------------------------------------------------
def _sentinel_tensor(entries, device="cuda", pinned=False):
    """(tensor of GUARD + entries + GUARD float4 entries filled with the sentinel, address of entry GUARD)"""
    import torch

    t = torch.full(((entries + 2 * GUARD) * 4,), int(SENTINEL), dtype=torch.int32, device=device)
    t = (t.pin_memory() if pinned else t).view(torch.float32)
    torch.cuda.synchronize()
    return t, t.data_ptr() + GUARD * 16


def _inside(t, entries):
    """The `entries` entries between the guards as uint32[entries, 4], after checking that the guards are intact."""
    import torch

    got = t.view(torch.int32).cpu().numpy().view(np.uint32).reshape(-1, 4)
    assert (got[:GUARD] == SENTINEL).all() and (got[GUARD + entries:] == SENTINEL).all(), "a store outside the buffer"
    return got[GUARD:GUARD + entries]


def _pattern(w, h):
    p = np.full((h, w, 4), -7.0, np.float32)
    p[..., 1] = np.arange(w, dtype=np.float32)
    p[..., 2] = np.arange(h, dtype=np.float32)[:, None]
    return p


@pytest.fixture(scope="module")
def scene_owner(pkg):
    import torch  # noqa: F401  (first, so the HIP library shares torch's HIP runtime)

    scene = pkg.Scene("default")
    owner = pkg.Renderer()
    owner.upload(scene)
    yield scene, owner
    owner.close()


@pytest.mark.gpu
def test_shard_bytes_of_every_rank_and_of_a_handle_without_a_frame(pkg):
    r = pkg.Renderer()
    try:
        r.set_tile_shard(1, WORLD, TILE)
        assert [r.shard_bytes(k) for k in range(WORLD + 1)] == [0] * (WORLD + 1), "no extent yet: no shard"
        r.resize(W, H)
        assert [r.shard_bytes(k) for k in range(WORLD)] == [16 * len(util.shard_entries(W, H, k, WORLD, TILE)) for k in range(WORLD)]
        assert r.shard_bytes(WORLD) == 0
    finally:
        r.close()


@pytest.mark.gpu
def test_only_a_changed_tile_shard_drops_the_bound_shard_buffer(pkg, scene_owner):
    """The same three values keep the binding (ptx_readback stays refused with PTX_ERROR_NOT_READY); another tile size alone drops
    it, and the frame that ptx_readback then returns is the internal image, which the render into the bound buffer never touched."""
    scene, owner = scene_owner
    rank = 1
    entries = len(util.shard_entries(W, H, rank, WORLD, TILE))
    buf, ptr = _sentinel_tensor(entries)
    pattern = _pattern(W, H)
    r = pkg.Renderer()
    try:
        r.share_scene(owner)
        r.resize(W, H)
        r.set_tile_shard(rank, WORLD, TILE)
        r.write_accumulation(pattern)
        r.bind_shard_accumulation(ptr, 16 * entries)
        r.reset()
        r.render_frames(scene.uniform(W, H, bounces=2), scene.lights, 0, 2)
        r.synchronize()
        message = _inside(buf, entries).copy()
        assert (message.view(np.float32)[:, 3] == 1).all(), "the render went somewhere else"
        r.set_tile_shard(rank, WORLD, TILE)
        with pytest.raises(pkg.PtxError, match="status 5"):
            r.readback()
        r.set_tile_shard(rank, WORLD, 2 * TILE)
        assert (r.readback().view(np.uint32) == pattern.view(np.uint32)).all()
        r.reset()  # ... and it is the internal image that a reset clears now
        assert (r.readback() == 0).all()
        assert (_inside(buf, entries) == message).all()
    finally:
        r.close()


@pytest.mark.gpu
def test_resize_returns_to_an_internal_image_and_leaves_the_present_image(pkg):
    """After ptx_bind_accumulation a ptx_resize to another extent accumulates in an internal image of the new size again, the
    output stage wants a new ptx_postprocess, and the screen keeps showing what was presented."""
    lib = pkg.load_hip()
    image, ptr = _sentinel_tensor(W * H)
    pattern = _pattern(W, H)
    r = pkg.Renderer()
    try:
        r.resize(W, H)
        r.bind_accumulation(ptr, W * H * 16)
        assert r.accum_ptr() == ptr and lib.ptx_accum_bytes(r.handle) == W * H * 16
        r.write_accumulation(pattern)
        r.postprocess(1)
        r.read_output()
        r.present(33, 22)
        shown, shown_bytes = r.read_present(), r.present_bytes()
        assert shown_bytes == 33 * 22 * 4 and shown.any()
        w2, h2 = 24, 16
        r.resize(w2, h2)
        assert r.accum_ptr() not in (0, ptr) and lib.ptx_accum_bytes(r.handle) == w2 * h2 * 16
        assert (r.readback() == 0).all()
        with pytest.raises(pkg.PtxError, match="status 5"):
            r.read_output()
        assert r.present_bytes() == shown_bytes and (r.read_present() == shown).all()
        r.write_accumulation(_pattern(w2, h2))
        r.postprocess(1)
        assert r.read_output().shape == (h2, w2, 4)
        assert r.present_bytes() == shown_bytes and (r.read_present() == shown).all()
        assert (_inside(image, W * H) == pattern.view(np.uint32).reshape(-1, 4)).all(), "the caller's image changed after it was unbound"
    finally:
        r.close()


@pytest.mark.gpu
def test_two_readbacks_in_flight_end_with_one_readback_end(pkg, scene_owner):
    """Two ptx_readback_begin into two page-locked buffers with a render between them, one ptx_readback_end after both: the first
    buffer holds the frame before that render and the second the frame after it, bit for bit what blocking read-backs at the
    same points of the same schedule give on a second handle."""
    scene, owner = scene_owner
    u, lights = scene.uniform(W, H, bounces=2), scene.lights
    a, b = pkg.Renderer(), pkg.Renderer()
    pinned = [_sentinel_tensor(W * H, device="cpu", pinned=True) for _ in range(2)]
    try:
        for r in (a, b):
            r.share_scene(owner)
            r.resize(W, H)
        b.render_frames(u, lights, 0, 2)
        before = b.readback()
        b.render_frames(u, lights, 2, 2)
        after = b.readback()
        assert not (before.view(np.uint32) == after.view(np.uint32)).all()
        a.render_frames(u, lights, 0, 2)
        a.readback_begin(pinned[0][1], W * H * 16)
        a.render_frames(u, lights, 2, 2)
        a.readback_begin(pinned[1][1], W * H * 16)
        a.readback_end()
        assert (_inside(pinned[0][0], W * H) == before.view(np.uint32).reshape(-1, 4)).all()
        assert (_inside(pinned[1][0], W * H) == after.view(np.uint32).reshape(-1, 4)).all()
    finally:
        a.close()
        b.close()
