"""The tile-shard gather path at every world size, tile size and image shape the project names, and at
the edges of its index arithmetic.

The N-rank step is emulated in ONE process on one GPU: a shard renderer is an ordinary handle with set_tile_shard(rank, world,
tile); N of them, each bound (ptx_bind_shard_accumulation) to its slice of one device tensor, write what IS the receive buffer
of the gather.  That buffer is compared bit for bit with (a) the whole-frame render of an unsharded handle and (b) the layout
include/ptx.h documents, stated in plain numpy (util.shard_entries / util.gather_index); ptx_unpack_shards then composes the
frame from it.  Every buffer the device may write lies inside a tensor that was filled with a sentinel (a quiet NaN with a
recognisable payload) and has sentinel padding after every slice: a store one entry too far shows as a changed sentinel.

The tests without the `gpu` mark guard the numpy reference itself (and close the chain to the oracle on two small cases)."""
import numpy as np
import pytest

import util

CASES = list(util.SHARD_CASES)
FULL_SIZE = [c for c in CASES if c[0] * c[1] >= 1920 * 1080]
SMALL = [c for c in CASES if c not in FULL_SIZE]
EMPTY_RANKS = [c for c in CASES if util.SHARD_CASES[c][4] > 0]
FRAME_COUNTS = (1, 2, 3, 4, 8, 12)  # frames per wave of k_accumulate: 1, 2, 1, 4, 8, 4
SENTINEL = np.uint32(util.SHARD_SENTINEL)
GUARD = 64  # sentinel entries (16 bytes each) in front of the first slice and behind the last
PAD = 37    # sentinel entries between a rank's largest possible message and the next slice: an odd stride, as the ABI allows


def _id(c):
    return "%dx%d-world%d-tile%d" % c


def _layout(W, H, world, tile):
    entries = [util.shard_entries(W, H, r, world, tile) for r in range(world)]
    return entries, max(len(e) for e in entries)


# ---------------------------------------------------------------------------------------
# the reference itself (no GPU)
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_layout_reference_maps_are_inverse_and_cover_the_image(pkg, case):
    """shard_entries (message entry -> pixel) and gather_index (pixel -> entry of the receive buffer) were written
    independently from the wording of include/ptx.h: they must be inverse to each other, the entries of all ranks must be every
    pixel exactly once, and they must agree with the package's own owned_tiles / shard_mask.  The properties each case is in
    the matrix for (util.SHARD_CASES) are asserted, so that a changed case cannot silently lose its edge."""
    W, H, world, tile = case
    tiles_x, tiles_y, fewest, most, empty, outside = util.SHARD_CASES[case]
    entries, largest = _layout(W, H, world, tile)
    owned = [len(e) // (tile * tile) for e in entries]
    assert (-(-W // tile), -(-H // tile)) == (tiles_x, tiles_y)
    assert (min(owned), max(owned), owned.count(0)) == (fewest, most, empty)
    assert sum(int((e < 0).sum()) for e in entries) == outside
    assert sum(owned) == tiles_x * tiles_y and largest == most * tile * tile
    seen = np.zeros(W * H, np.int64)
    for stride in (largest, largest + PAD):
        G = util.gather_index(W, H, world, tile, stride)
        assert G.shape == (W * H,) and G.min() >= 0 and len(np.unique(G)) == W * H
        for r, e in enumerate(entries):
            at = np.flatnonzero(e >= 0)
            assert (G[e[at]] == r * stride + at).all(), f"rank {r}: the two maps are not inverse"
        # ... and no other pixel reads a rank's slice
        assert np.bincount(G // stride, minlength=world).tolist() == [int((e >= 0).sum()) for e in entries]
    for r, e in enumerate(entries):
        assert len(e) == len(pkg.owned_tiles(W, H, r, world, tile)) * tile * tile
        mask = np.zeros(W * H, bool)
        mask[e[e >= 0]] = True
        assert (mask.reshape(H, W) == pkg.shard_mask(W, H, r, world, tile)).all()
        np.add.at(seen, e[e >= 0], 1)
    assert (seen == 1).all(), "every pixel must be exactly one entry of exactly one rank"
    if case == (1920, 1080, 8, 32):  # equal tiles per rank, unequal pixels
        px = [int((e >= 0).sum()) for e in entries]
        assert (min(px), max(px)) == (259072, 259328)
    if case == (328, 200, 7, 64):
        px = [int((e >= 0).sum()) for e in entries]
        assert 5120 in px and 12800 in px
    if case == (33, 257, 6, 16):
        assert min(int((e >= 0).sum()) for e in entries) == 128
    # the 32-bit products of k_gather_frame and slotPixel stay below 2^32 at the largest shapes
    assert world * (largest + PAD) < 2 ** 32 and W * H * 16 < 2 ** 32


@pytest.mark.parametrize("case", [(200, 120, 3, 32), (96, 54, 8, 32)], ids=_id)
def test_layout_reference_composes_the_oracles_shards(pkg, orc, case):
    """The oracle closes the chain: its shard renders, packed with shard_entries and composed with gather_index, are its whole
    frame bit for bit (one ragged case with unequal shards, one with ranks that own nothing)."""
    W, H, world, tile = case
    scene = pkg.Scene("default")
    osc = orc.OracleScene(scene.desc)
    u = scene.uniform(W, H, bounces=3)
    whole, _ = osc.render(u, scene.lights, W, H)
    entries, largest = _layout(W, H, world, tile)
    stride = largest + PAD
    recv = np.full((world * stride, 4), SENTINEL, np.uint32)
    for r, e in enumerate(entries):
        part, st = osc.render(u, scene.lights, W, H, shard=pkg.TileShard(r, world, tile))
        assert (st.pathSamples == 0) == (len(e) == 0)
        flat = part.view(np.uint32).reshape(-1, 4)
        recv[r * stride:r * stride + len(e)] = np.where((e >= 0)[:, None], flat[np.maximum(e, 0)], 0)
    got = recv[util.gather_index(W, H, world, tile, stride)].reshape(H, W, 4)
    assert (got == whole.view(np.uint32)).all()
    assert (whole[..., 3] == 1).all()


# ---------------------------------------------------------------------------------------
# the device (one MI355X, one process)
# ---------------------------------------------------------------------------------------
def _sentinel_tensor(entries, device="cuda", pinned=False):
    import torch

    t = torch.full((entries * 4,), int(SENTINEL), dtype=torch.int32, device=device)
    return (t.pin_memory() if pinned else t).view(torch.float32)


def _bits(t):
    import torch

    return t.view(torch.int32).cpu().numpy().view(np.uint32)


def _counters(st):
    return (st.pathSamples, st.segments, st.shadowRays, st.retries)


class _Pool:
    """ONE scene owner at a time (one upload and one tree; the whole-frame reference is rendered on it) and the rank handles of
    ONE flavour at a time (single_stream or not), re-used from case to case: about a dozen handles alive."""

    def __init__(self, pkg):
        self.pkg, self.owners, self.ranks, self.flavour = pkg, {}, [], None

    def owner(self, name, detail):
        if (name, detail) not in self.owners:
            for _, r in self.owners.values():  # (its borrowers are given the new owner before they render again)
                r.close()
            scene = self.pkg.Scene(name, detail)
            r = self.pkg.Renderer()
            r.upload(scene)
            self.owners = {(name, detail): (scene, r)}
        return self.owners[(name, detail)]

    def rank_handles(self, n, single_stream):
        if self.flavour != single_stream:
            for h in self.ranks:
                h.close()
            self.ranks, self.flavour = [], single_stream
        while len(self.ranks) < n:
            self.ranks.append(self.pkg.Renderer(single_stream=single_stream))
        return self.ranks[:n]

    def close(self):
        for h in self.ranks:
            h.close()
        for _, r in self.owners.values():
            r.close()
        self.ranks, self.owners = [], {}


@pytest.fixture(scope="module")
def pool(pkg):
    import torch  # noqa: F401  (first, so the HIP library shares torch's HIP runtime)

    p = _Pool(pkg)
    yield p
    p.close()


def _render_batches(scene, W, H, depth, batches):
    u, lights = scene.uniform(W, H, bounces=depth), scene.lights

    def render(h):
        for first, n in batches:
            h.render_frames(u, lights, first, n)
    return render


def whole_frame(owner, W, H, render, backend=0):
    """The reference: the same launches on an unsharded handle.  Returns (image, counters of each launch that reported them or
    of the last one)."""
    owner.set_backend(backend)
    owner.set_tile_shard(0, 1, 32)
    owner.resize(W, H)
    per_launch = render(owner)
    img = owner.readback()
    assert np.isfinite(img).all() and (img[..., 3] == 1).all()
    return img, per_launch if per_launch else [_counters(owner.stats())]


class Gathered:
    pass


def emulate_gather(pkg, pool, owner, W, H, world, tile, render, backend=0, single_stream=True, reuse_handle=False):
    """The N-rank step in one process: one handle per rank borrows the owner's scene, is resized, given its shard and bound to
    its slice of ONE device tensor (GUARD sentinel entries, then `world` slices of largest + PAD entries, then GUARD again);
    reset, render, synchronize.  reuse_handle: ONE handle takes the ranks in turn (a ptx_set_tile_shard that changes the shard
    unbinds).  Returns the tensor, the layout and the counters per rank."""
    import torch

    g = Gathered()
    g.W, g.H, g.world, g.tile = W, H, world, tile
    g.entries, g.largest = _layout(W, H, world, tile)
    g.stride = g.largest + PAD
    g.buf = _sentinel_tensor(2 * GUARD + world * g.stride)
    torch.cuda.synchronize()
    g.ptr = lambda r: g.buf.data_ptr() + (GUARD + r * g.stride) * 16
    g.handles = pool.rank_handles(1 if reuse_handle else world, single_stream)
    g.counters = [None] * world
    g.shard_bytes = []
    for r in range(world):
        h = g.handles[0 if reuse_handle else r]
        if not reuse_handle or r == 0:
            h.share_scene(owner)
            h.set_backend(backend)
            h.resize(W, H)
        h.set_tile_shard(r, world, tile)
        g.shard_bytes.append(h.shard_bytes(r))
        assert [h.shard_bytes(k) for k in range(world)] == [16 * len(e) for e in g.entries]
        assert h.shard_bytes(world) == 0
        h.bind_shard_accumulation(g.ptr(r), g.shard_bytes[r])  # exactly the bytes required: 0 for a rank that owns nothing
        h.reset()
        per_launch = render(h)
        if reuse_handle:
            h.synchronize()
            g.counters[r] = per_launch if per_launch else [_counters(h.stats())]
        else:
            g.counters[r] = per_launch
    for r in range(world):
        if not reuse_handle:
            g.handles[r].synchronize()
            if not g.counters[r]:
                g.counters[r] = [_counters(g.handles[r].stats())]
    return g


def check_message(g, ref):
    """Assertion 1: slice r is the documented layout of the reference frame, 0.0 where a ragged tile leaves the image, and the
    sentinel everywhere behind shard_bytes(r)."""
    got = _bits(g.buf).reshape(-1, 4)
    flat = ref.view(np.uint32).reshape(-1, 4)
    assert (got[:GUARD] == SENTINEL).all() and (got[GUARD + g.world * g.stride:] == SENTINEL).all(), "a store outside every slice"
    for r, e in enumerate(g.entries):
        part = got[GUARD + r * g.stride:GUARD + (r + 1) * g.stride]
        assert g.shard_bytes[r] == 16 * len(e)
        want = np.where((e >= 0)[:, None], flat[np.maximum(e, 0)], np.uint32(0))
        bad = np.flatnonzero((part[:len(e)] != want).any(axis=1))
        assert not len(bad), (f"rank {r}: {len(bad)} of {len(e)} entries differ from the documented layout, first entry {bad[0]} "
                              f"(pixel {e[bad[0]]}): {part[bad[0]]} != {want[bad[0]]}")
        assert (part[len(e):] == SENTINEL).all(), f"rank {r}: something was written behind its {len(e)} entries"


def check_counters(g, ref_counters):
    total = np.sum([np.array(c, np.int64) for c in g.counters], axis=0)
    assert (total == np.array(ref_counters, np.int64)).all(), f"counters summed over the ranks {total.tolist()} != the whole frame's {ref_counters}"
    for r, e in enumerate(g.entries):
        if not len(e):
            assert all(c == (0, 0, 0, 0) for c in g.counters[r]), f"rank {r} owns nothing but reports {g.counters[r]}"


def compact(g):
    """The receive buffer with stride == the largest shard (what bench.py allocates): the messages copied as a gather would."""
    import torch

    t = _sentinel_tensor(g.world * g.largest + GUARD)
    if g.largest:
        t[:g.world * g.largest * 4].view(g.world, g.largest * 4).copy_(
            g.buf[GUARD * 4:(GUARD + g.world * g.stride) * 4].view(g.world, g.stride * 4)[:, :g.largest * 4])
    torch.cuda.synchronize()
    return t, t.data_ptr(), g.largest * 16


def check_one_launch_composes(pkg, g, ref, strides=("padded", "largest")):
    """Assertion 2: ptx_unpack_shards on a separate, unbound handle -- device image only, host frame only (the device image
    untouched), both -- with a padded stride and with stride == largest shard."""
    import torch

    W, H, nbytes = g.W, g.H, g.W * g.H * 16
    c = pkg.Renderer()
    c.resize(W, H)
    c.set_tile_shard(0, g.world, g.tile)
    pattern = np.full((H, W, 4), -7.0, np.float32)
    pattern[..., 1] = np.arange(W, dtype=np.float32)
    rb = ref.view(np.uint32)
    try:
        for which in strides:
            keep, src, stride_bytes = (g.buf, g.buf.data_ptr() + GUARD * 16, g.stride * 16) if which == "padded" else compact(g)
            c.write_accumulation(pattern)
            c.unpack_shards(src, stride_bytes, True)  # (a) the device image only
            assert (c.readback().view(np.uint32) == rb).all(), f"{which} stride: the device image is not the reference"
            c.write_accumulation(pattern)
            host = _sentinel_tensor(W * H, device="cpu", pinned=True)
            c.unpack_shards(src, stride_bytes, False, host.data_ptr(), nbytes)  # (b) the host's frame only
            c.readback_end()
            assert (_bits(host).reshape(H, W, 4) == rb).all(), f"{which} stride: the host's frame is not the reference"
            assert (c.readback() == pattern).all(), "to_device_image=False must leave the device image alone"
            host2 = _sentinel_tensor(W * H, device="cpu", pinned=True)
            c.unpack_shards(src, stride_bytes, True, host2.data_ptr(), nbytes)  # (c) both
            c.readback_end()
            assert (_bits(host2).reshape(H, W, 4) == rb).all() and (c.readback().view(np.uint32) == rb).all()
            del keep
    finally:
        c.close()


def check_older_forms(pkg, g, ref, owner, render, backend=0):
    """Assertion 3: ptx_pack_shard of a row-major shard render gives the bytes of the bound message; on a bound handle it is a
    copy (or, into the bound buffer itself, nothing); N ptx_unpack_shard launches and the _host form compose the same frame."""
    import torch

    W, H, world, tile = g.W, g.H, g.world, g.tile
    before = _bits(g.buf).copy()
    msg = before.reshape(-1, 4)
    rb = ref.view(np.uint32)
    rm = pkg.Renderer(backend=backend)
    rm.share_scene(owner)
    rm.resize(W, H)
    c = pkg.Renderer()
    c.resize(W, H)
    c.set_tile_shard(0, world, tile)
    c.write_accumulation(np.full((H, W, 4), -7.0, np.float32))
    ch = pkg.Renderer()
    ch.resize(W, H)
    ch.set_tile_shard(0, world, tile)
    host = _sentinel_tensor(W * H, device="cpu", pinned=True)
    try:
        for r, e in enumerate(g.entries):
            n = len(e)
            mine = msg[GUARD + r * g.stride:GUARD + r * g.stride + n]
            if len(g.handles) == world:  # the rank's handle is still bound
                h = g.handles[r]
                copy = _sentinel_tensor(n + GUARD)
                torch.cuda.synchronize()
                h.pack_shard(copy.data_ptr())
                h.pack_shard(g.ptr(r))
                h.synchronize()
                got = _bits(copy).reshape(-1, 4)
                assert (got[:n] == mine).all() and (got[n:] == SENTINEL).all(), f"rank {r}: pack_shard of a bound handle is not a copy of the message"
            rm.set_tile_shard(r, world, tile)
            rm.reset()
            render(rm)
            img = rm.readback()
            mask = pkg.shard_mask(W, H, r, world, tile)
            assert (img.view(np.uint32)[mask] == rb[mask]).all() and (img[~mask] == 0).all()
            packed = _sentinel_tensor(n + GUARD)
            torch.cuda.synchronize()
            rm.pack_shard(packed.data_ptr())
            rm.synchronize()
            got = _bits(packed).reshape(-1, 4)
            assert (got[:n] == mine).all() and (got[n:] == SENTINEL).all(), f"rank {r}: pack_shard of the row-major render differs from the bound message"
            c.unpack_shard(r, packed.data_ptr())
            ch.unpack_shard(r, g.ptr(r), host.data_ptr(), W * H * 16)
            c.synchronize()
            ch.synchronize()
        ch.readback_end()
        assert (c.readback().view(np.uint32) == rb).all(), "N unpack_shard launches do not compose the reference"
        assert (_bits(host).reshape(H, W, 4) == rb).all() and (ch.readback().view(np.uint32) == rb).all()
        assert (_bits(g.buf) == before).all(), "pack_shard into the bound buffer must be a no-op"
    finally:
        for x in (rm, c, ch):
            x.close()


def _single_stream_for(case):
    return CASES.index(case) % 3 != 2  # a rank of a job runs on one stream: two thirds of the matrix


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(SMALL, key=lambda c: not _single_stream_for(c)), ids=_id)
def test_small_shapes_every_frame_count(pkg, pool, case):
    """Every small row of the matrix on chess_like at low detail, depth 5, for 1, 2, 3, 4, 8 and 12 frames (k_accumulate's lane
    shuffles for 1 / 2 / 4 / 8 frames per wave writing shard-major): the message is the documented layout of the whole-frame
    render, the counters add up, one ptx_unpack_shards launch composes the frame, and (at 4 frames) the older forms agree.
    World 16 goes through ONE re-used handle."""
    W, H, world, tile = case
    scene, owner = pool.owner("chess_like", 0.05)
    for frames in FRAME_COUNTS:
        render = _render_batches(scene, W, H, 5, [(0, frames)])
        ref, ref_counters = whole_frame(owner, W, H, render)
        g = emulate_gather(pkg, pool, owner, W, H, world, tile, render, single_stream=_single_stream_for(case), reuse_handle=(world == 16))
        check_message(g, ref)
        check_counters(g, ref_counters[-1])
        check_one_launch_composes(pkg, g, ref, strides=("padded", "largest") if frames in (1, 8) else ("largest",))
        if frames == 4:
            check_older_forms(pkg, g, ref, owner, render)


@pytest.mark.gpu
@pytest.mark.parametrize("case", FULL_SIZE, ids=_id)
def test_full_size_shapes(pkg, pool, case):
    """BASELINE configs[3] and [4] and the strong-scaling frame at the sizes they ship for: 4 and 8 ranks at 1920x1080, 8 ranks
    at 3840x2160 with tiles of 32 and 16; one frame at depth 4 exercises every index."""
    W, H, world, tile = case
    scene, owner = pool.owner("chess_like", 0.05)
    render = _render_batches(scene, W, H, 4, [(0, 2 if W == 1920 else 1)])
    ref, ref_counters = whole_frame(owner, W, H, render)
    g = emulate_gather(pkg, pool, owner, W, H, world, tile, render, single_stream=True)
    check_message(g, ref)
    check_counters(g, ref_counters[-1])
    check_one_launch_composes(pkg, g, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("name,detail,case", [("atrium_like", 0.2, (1920, 1080, 4, 32)), ("atrium_like", 0.2, (328, 200, 7, 64)),
                                              ("materials_test", 1.0, (200, 120, 3, 32))], ids=lambda v: _id(v) if isinstance(v, tuple) else str(v))
def test_textured_and_material_sorted_scenes(pkg, pool, name, detail, case):
    """atrium_like is textured and alpha-tested (k_shade<true>, the ALPHA traversal kernels); materials_test goes through the
    material-sorted shade queue, whose length depends on the shard."""
    W, H, world, tile = case
    scene, owner = pool.owner(name, detail)
    render = _render_batches(scene, W, H, 6, [(0, 1 if W == 1920 else 4)])
    ref, ref_counters = whole_frame(owner, W, H, render)
    g = emulate_gather(pkg, pool, owner, W, H, world, tile, render, single_stream=False)
    check_message(g, ref)
    check_counters(g, ref_counters[-1])
    check_one_launch_composes(pkg, g, ref, strides=("largest",))


@pytest.mark.gpu
@pytest.mark.parametrize("case", [(200, 120, 3, 32), (96, 54, 8, 32)], ids=_id)
def test_device_whole_frame_is_the_oracles(pkg, orc, pool, case):
    """The chain new test -> device whole frame -> oracle, closed inside this file on two small cases."""
    W, H, world, tile = case
    scene, owner = pool.owner("chess_like", 0.05)
    ref, _ = whole_frame(owner, W, H, _render_batches(scene, W, H, 5, [(0, 2)]))
    osc = orc.OracleScene(scene.desc)
    want = np.zeros((H, W, 4), np.float32)
    for f in range(2):
        osc.render(scene.uniform(W, H, bounces=5, total_samples=f), scene.lights, W, H, accum=want)
    assert (ref.view(np.uint32) == want.view(np.uint32)).all()


@pytest.mark.gpu
@pytest.mark.parametrize("backend,depth", [(0, 5), (1, 5), (0, 0), (1, 0)], ids=["wavefront", "megakernel", "wavefront-0-bounces", "megakernel-0-bounces"])
@pytest.mark.parametrize("case", [(200, 120, 3, 32), (328, 200, 5, 8), (640, 360, 8, 128)], ids=_id)
def test_every_accumulate_call_site_adds_onto_the_bound_shard(pkg, pool, case, backend, depth):
    """renderImpl reaches k_accumulate from three places (zero bounces, the megakernel backend, the wavefront path), and the
    wavefront path is driven from the host on the first launch of a shape and hinted afterwards.  Frames 0-3 and then 4-7
    into the same bound buffer without a reset -- the second batch runs the hinted schedule AND adds onto existing entries --
    must be the reference's 8 frames."""
    W, H, world, tile = case
    scene, owner = pool.owner("chess_like", 0.05)
    ref, _ = whole_frame(owner, W, H, _render_batches(scene, W, H, depth, [(0, 8)]), backend=backend)
    _, last = whole_frame(owner, W, H, _render_batches(scene, W, H, depth, [(0, 4), (4, 4)]), backend=backend)
    g = emulate_gather(pkg, pool, owner, W, H, world, tile, _render_batches(scene, W, H, depth, [(0, 4), (4, 4)]), backend=backend)
    owner.set_backend(0)
    check_message(g, ref)
    check_counters(g, last[-1])
    check_one_launch_composes(pkg, g, ref, strides=("largest",))


@pytest.mark.gpu
def test_multi_sample_launch_under_a_bound_shard(pkg, pool):
    """SampleCount = 3 in one ptx_render (the restart queue): message, frame and counters."""
    W, H, world, tile = 328, 200, 7, 64
    scene, owner = pool.owner("chess_like", 0.05)
    u, lights = scene.uniform(W, H, bounces=6, sample_count=3, total_samples=0), scene.lights

    def render(h):
        h.render(u, lights)
        return [_counters(h.stats())]

    ref, ref_counters = whole_frame(owner, W, H, render)
    assert ref_counters[0][0] == W * H * 3 + ref_counters[0][3]
    g = emulate_gather(pkg, pool, owner, W, H, world, tile, render)
    check_message(g, ref)
    check_counters(g, ref_counters)
    check_one_launch_composes(pkg, g, ref, strides=("largest",))


@pytest.mark.gpu
def test_nan_inf_restarts_under_a_bound_shard(pkg, pool):
    """The set-up of test_nan_inf_samples_restart_like_the_reference (a point light of infinite colour: samples that come out
    NaN / Inf restart) with eight ranks at 96x54, two of which own nothing: launch by launch the counters summed over the ranks
    are the whole frame's, and so is the composed frame."""
    W, H, world, tile = 96, 54, 8, 32
    scene, owner = pool.owner("default", 1.0)
    lights = scene.lights
    lights.LightCount = 12
    for i in range(12):
        for k in range(3):
            lights.Lights[i].Color[k] = float("inf") if i == 0 else 0.0
        lights.Lights[i].Position[0], lights.Lights[i].Position[1], lights.Lights[i].Position[2] = 1.0, -2.0, 0.5
        lights.Lights[i].AttenuationConstant = 1.0

    def render(h):
        out = []
        for f, sc_ in enumerate((1, 1, 3)):
            h.render(scene.uniform(W, H, bounces=4, sample_count=sc_, total_samples=f), lights)
            out.append(_counters(h.stats()))
        return out

    ref, ref_counters = whole_frame(owner, W, H, render)
    assert all(c[3] > 0 for c in ref_counters), "the scene must provoke restarts"
    g = emulate_gather(pkg, pool, owner, W, H, world, tile, render)
    check_message(g, ref)
    check_counters(g, ref_counters)
    check_one_launch_composes(pkg, g, ref, strides=("largest",))


@pytest.mark.gpu
@pytest.mark.parametrize("case", EMPTY_RANKS, ids=_id)
def test_ranks_that_own_nothing(pkg, pool, case):
    """More ranks than tiles: render, reset, bind (a valid pointer, 0 required bytes), pack and stats of a rank without tiles
    all succeed, it reports no samples and writes nothing, and the composed frame is still the reference."""
    import torch

    W, H, world, tile = case
    scene, owner = pool.owner("chess_like", 0.05)
    render = _render_batches(scene, W, H, 4, [(0, 2)])
    ref, ref_counters = whole_frame(owner, W, H, render)
    g = emulate_gather(pkg, pool, owner, W, H, world, tile, render, reuse_handle=(world == 16))
    empty = [r for r, e in enumerate(g.entries) if not len(e)]
    assert len(empty) == util.SHARD_CASES[case][4] > 0
    check_message(g, ref)
    check_counters(g, ref_counters[-1])
    check_older_forms(pkg, g, ref, owner, render)
    h = g.handles[0]
    h.set_tile_shard(empty[0], world, tile)
    other = _sentinel_tensor(GUARD)
    torch.cuda.synchronize()
    assert h.shard_bytes(empty[0]) == 0
    h.bind_shard_accumulation(other.data_ptr(), 0)
    h.reset()
    render(h)
    h.pack_shard(other.data_ptr())
    h.pack_shard(g.ptr(empty[0]))
    h.synchronize()
    assert _counters(h.stats()) == (0, 0, 0, 0)
    h.bind_shard_accumulation(0)
    h.pack_shard(other.data_ptr())  # the row-major form of an empty shard
    h.synchronize()
    assert (_bits(other) == SENTINEL).all()
    check_message(g, ref)
    check_one_launch_composes(pkg, g, ref)


@pytest.mark.gpu
def test_state_machine_of_a_bound_shard(pkg, pool):
    """include/ptx.h on ptx_bind_shard_accumulation: the calls that need the row-major frame return PTX_ERROR_NOT_READY (5) and
    change nothing until NULL is bound again; ptx_resize and a ptx_set_tile_shard that changes the shard unbind, an identical
    one does not; bad buffers, strides and shards are refused by host-side checks before anything is launched."""
    import torch

    W, H, world, tile = 200, 120, 3, 32
    scene, owner = pool.owner("chess_like", 0.05)
    render = _render_batches(scene, W, H, 4, [(0, 2)])
    ref, _ = whole_frame(owner, W, H, render)
    g = emulate_gather(pkg, pool, owner, W, H, world, tile, render)
    check_message(g, ref)
    before = _bits(g.buf).copy()
    h = g.handles[1]
    pinned = _sentinel_tensor(W * H, device="cpu", pinned=True)
    for call in (h.readback, lambda: h.readback_begin(pinned.data_ptr(), W * H * 16), lambda: h.postprocess(2),
                 lambda: h.write_accumulation(np.ones((H, W, 4), np.float32))):
        with pytest.raises(pkg.PtxError, match="status 5"):
            call()
    h.readback_end()
    h.synchronize()
    assert (_bits(pinned) == SENTINEL).all() and (_bits(g.buf) == before).all()
    # the no-read-back branch of a job's step: the owner of the frame, itself bound, composes it into its own device image
    h.unpack_shards(g.buf.data_ptr() + GUARD * 16, g.stride * 16, True)
    h.synchronize()
    with pytest.raises(pkg.PtxError, match="status 5"):
        h.readback()
    h.set_tile_shard(1, world, tile)  # identical: still bound
    with pytest.raises(pkg.PtxError, match="status 5"):
        h.readback()
    h.bind_shard_accumulation(0)
    assert (h.readback().view(np.uint32) == ref.view(np.uint32)).all()
    h.postprocess(2)
    h.write_accumulation(ref)
    assert (_bits(g.buf) == before).all()
    # a changed shard unbinds: the next render goes to the row-major image, not to the buffer
    h.bind_shard_accumulation(g.ptr(1), g.shard_bytes[1])
    h.set_tile_shard(2, world, tile)
    h.reset()
    render(h)
    img = h.readback()
    mask = pkg.shard_mask(W, H, 2, world, tile)
    assert (img.view(np.uint32)[mask] == ref.view(np.uint32)[mask]).all() and (img[~mask] == 0).all()
    # resize unbinds
    h.bind_shard_accumulation(g.ptr(2), g.shard_bytes[2])
    h.resize(W, H)
    assert (h.readback() == 0).all()
    render(h)
    assert (h.readback().view(np.uint32)[mask] == ref.view(np.uint32)[mask]).all()
    assert (_bits(g.buf) == before).all()
    # refused before anything is launched
    h.set_tile_shard(0, world, tile)
    need = h.shard_bytes(0)
    assert need == g.shard_bytes[0] > 16
    src, stride_bytes, nbytes = g.buf.data_ptr() + GUARD * 16, g.stride * 16, W * H * 16
    pageable = np.zeros(W * H * 4, np.float32)
    for bad in (lambda: h.bind_shard_accumulation(g.ptr(0), need - 16),
                lambda: h.unpack_shards(src, g.largest * 16 - 16, True),
                lambda: h.unpack_shards(src, stride_bytes + 8, True),
                lambda: h.unpack_shards(src, stride_bytes, False),  # no target at all
                lambda: h.unpack_shards(src, stride_bytes, False, pinned.data_ptr(), nbytes - 16),
                lambda: h.unpack_shards(src, stride_bytes, False, pageable.ctypes.data, nbytes),
                lambda: h.unpack_shard(0, src, pinned.data_ptr(), nbytes - 16),
                lambda: h.unpack_shard(0, src, pageable.ctypes.data, nbytes),
                lambda: h.unpack_shard(world, src),
                lambda: h.set_tile_shard(0, world, 0), lambda: h.set_tile_shard(0, world, 12), lambda: h.set_tile_shard(0, world, 2048),
                lambda: h.set_tile_shard(world, world, tile), lambda: h.set_tile_shard(0, 0, tile)):
        with pytest.raises(pkg.PtxError, match="status 1"):
            bad()
    h.synchronize()
    assert (_bits(pinned) == SENTINEL).all() and (_bits(g.buf) == before).all() and (pageable == 0).all()
    assert (h.readback().view(np.uint32)[mask] == ref.view(np.uint32)[mask]).all()
    fresh = pkg.Renderer()
    with pytest.raises(pkg.PtxError, match="status 5"):  # nothing to bind to before ptx_resize
        fresh.bind_shard_accumulation(g.ptr(0), need)
    fresh.close()


@pytest.mark.gpu
def test_bind_accumulation_uses_the_callers_image(pkg, pool):
    """ptx_bind_accumulation: a caller-owned tensor as the row-major accumulation image receives the render; readback,
    postprocess and unpack_shards(to_device_image=True) use it; a wrong size is refused; NULL returns to the internal image;
    resize drops the binding."""
    import torch

    W, H, world, tile = 200, 120, 3, 32
    scene, owner = pool.owner("chess_like", 0.05)
    render = _render_batches(scene, W, H, 4, [(0, 3)])
    ref, _ = whole_frame(owner, W, H, render)
    owner.postprocess(3)
    want_out = owner.read_output()
    rb = ref.view(np.uint32)
    image = _sentinel_tensor(GUARD + W * H + GUARD)
    torch.cuda.synchronize()
    ptr, nbytes = image.data_ptr() + GUARD * 16, W * H * 16

    def inside():
        got = _bits(image).reshape(-1, 4)
        assert (got[:GUARD] == SENTINEL).all() and (got[GUARD + W * H:] == SENTINEL).all()
        return got[GUARD:GUARD + W * H].reshape(H, W, 4)

    h = pkg.Renderer()
    with pytest.raises(pkg.PtxError, match="status 5"):
        h.bind_accumulation(ptr, nbytes)  # before ptx_resize
    h.share_scene(owner)
    h.resize(W, H)
    for wrong in (nbytes - 16, nbytes + 16, 0):
        with pytest.raises(pkg.PtxError, match="status 1"):
            h.bind_accumulation(ptr, wrong)
    h.bind_accumulation(ptr, nbytes)
    assert h.accum_ptr() == ptr
    h.reset()
    render(h)
    h.synchronize()
    assert (inside() == rb).all(), "the bound tensor did not receive the render"
    assert (h.readback().view(np.uint32) == rb).all()
    h.postprocess(3)
    assert (h.read_output() == want_out).all()
    # the gathered frame composed into the caller's image
    g = emulate_gather(pkg, pool, owner, W, H, world, tile, render)
    h.reset()
    h.synchronize()
    assert (inside() == 0).all()
    h.set_tile_shard(0, world, tile)
    h.unpack_shards(g.buf.data_ptr() + GUARD * 16, g.stride * 16, True)
    h.synchronize()
    assert (inside() == rb).all()
    # NULL: back to the internal image (cleared by ptx_resize, never rendered to)
    h.bind_accumulation(0, 0)
    assert h.accum_ptr() not in (0, ptr)
    assert (h.readback() == 0).all()
    h.write_accumulation(np.full((H, W, 4), 3.0, np.float32))
    assert (inside() == rb).all()
    # resize drops the binding
    h.bind_accumulation(ptr, nbytes)
    h.resize(W, H)
    assert h.accum_ptr() != ptr
    h.set_tile_shard(0, 1, 32)
    render(h)
    assert (h.readback().view(np.uint32) == rb).all()
    assert (inside() == rb).all()
    h.close()
