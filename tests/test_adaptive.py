"""Adaptive sampling (include/ptx.h "Adaptive sampling": ptx_adaptive_plan, ptx_read_adaptive, ptx_adaptive_clear,
ptx_noise_meter_adaptive; csrc/pt_adaptive.hpp, docs/NEXT_ROWS.md section 27) against tests/adaptive_ref.py.

Tolerance: none.  The plan is integers only; a planned render adds to a pixel of an active tile what the unplanned render adds (the
random numbers are a function of pixel, width and frame alone, k_accumulate adds in frame order) and touches no other pixel; the
adaptive meter is ptx_noise_meter's float32 operations with every tile's own factors, formed with the correctly rounded rcp.  The one
place where bits are not compared is the payload of a NaN in a stored sum, as in tests/test_noise_meter.py.

The threshold of the loop test is the median tile error of the oracle's 8 + 8 frames of `default` at 130 x 70, depth 2, 16-pixel tiles:
LOOP_THRESHOLD, pinned with the line that printed it."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import adaptive_ref as AR
import noise_ref as NR

EXTENTS = {"1x1": (1, 1), "3x2": (3, 2), "33x9": (33, 9), "67x45": (67, 45), "130x70": (130, 70), "300x200": (300, 200)}
W, H = EXTENTS["67x45"]
SHIFTS = (3, 4, 5, 6)
DILATES = (0, 1, 2)
FRAMES = ((0, 0), (1, 1), (3, 2), (0, 5), (8, 8), (2, 0))  # what successive plans commit
SCENES = {"default": 1.0, "texture_test": 0.25, "alpha_test": 1.0}  # kernel modes 0 (opaque), 1 (textured), 2 (any-hit stages)
POST = dict(exposure=1.25, bloom_threshold=0.8, bloom_intensity=0.35)
OK, INVALID, NOT_READY = 0, 1, 5
PLAN_FIELDS = ("tilesX", "tilesY", "activeTiles", "activePixels", "seedTiles", "generation")
NOISE_INTS = ("tilesX", "tilesY", "converged", "counted", "black", "rejected", "valid", "calls")
STAT_FIELDS = ("pathSamples", "segments", "shadowRays", "retries")
# python -c "import sys; sys.path[:0] = ['tests', '.']; import __graft_entry__ as g, test_adaptive as T; print(repr(T._loop_median(g.load_package(), g.load_oracle())))"
LOOP_THRESHOLD = 0.00568312406539917
LOOP_EXTENT, LOOP_DEPTH, LOOP_SHIFT, LOOP_WARMUP = (130, 70), 2, 4, 16
f32 = np.float32


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_sum(got, want):
    """bit for bit, but for the payload of a NaN"""
    return ((_bits(got) == _bits(want)) | (np.isnan(got) & np.isnan(want))).all()


def _masks(tx, ty, seed=0):
    rng = np.random.default_rng(seed + 17 * tx + ty)
    single = np.zeros((ty, tx), np.uint8)
    single[ty // 2, tx // 2] = 1
    last = np.zeros((ty, tx), np.uint8)
    last[-1, -1] = 1
    jj, ii = np.mgrid[0:ty, 0:tx]
    # the random mask's seeds are bytes of every non-zero value: they reach the device as they are, and mask[t] != 0 decides
    return {"random": ((rng.random((ty, tx)) < 0.3) * rng.integers(1, 256, (ty, tx))).astype(np.uint8), "empty": np.zeros((ty, tx), np.uint8), "full": np.ones((ty, tx), np.uint8),
            "single": single, "last": last, "checkerboard": ((ii + jj) & 1).astype(np.uint8)}


def _loop_halves(pkg, orc):
    """the oracle's LOOP_WARMUP frames of `default`, even frames in half 0 and odd ones in half 1"""
    w, h = LOOP_EXTENT
    s = pkg.Scene("default", SCENES["default"])
    osc = orc.OracleScene(s.desc, build_bvh=True)
    u = s.uniform(w, h, bounces=LOOP_DEPTH)
    half = [np.zeros((h, w, 4), np.float32) for _ in range(2)]
    for f in range(LOOP_WARMUP):
        u.TotalSamples = f
        osc.render(u, s.lights, w, h, accum=half[f & 1])
    return half


def _loop_median(pkg, orc):
    half = _loop_halves(pkg, orc)
    E = NR.meter(half[0], half[1], LOOP_WARMUP // 2, LOOP_WARMUP // 2, 1.0, 0.0, LOOP_SHIFT)[1]
    return float(np.sort(E.ravel())[E.size // 2])


# =====================================================================================================
# without a GPU
# =====================================================================================================
def test_header_declares_and_package_exports_adaptive_sampling(pkg):
    header = open(os.path.join(pkg.REPO_DIR, "include", "ptx.h")).read()
    decls = {
        "ptx_adaptive_plan": r"PTX_API int ptx_adaptive_plan\(PtxRenderer \*r, const PtxAdaptiveDesc \*desc, PtxAdaptivePlan \*out\);",
        "ptx_read_adaptive": r"PTX_API int ptx_read_adaptive\(PtxRenderer \*r, PtxAdaptivePlan \*out, uint32_t \*tiles, size_t tileBytes, uint32_t \*counts, size_t countBytes\);",
        "ptx_adaptive_clear": r"PTX_API int ptx_adaptive_clear\(PtxRenderer \*r\);",
        "ptx_noise_meter_adaptive": r"PTX_API int ptx_noise_meter_adaptive\(PtxRenderer \*r, const PtxAdaptiveMeterDesc \*desc\);",
    }
    lib = pkg.load_hip()
    for name, decl in decls.items():
        assert re.search(decl, header), name
        assert name in pkg.PTX_SYMBOLS
        assert hasattr(lib, name), name
    assert "#define PTX_ABI_VERSION 5u" in header and "PTX_FN_COUNT = 38" in header  # additions only
    names = lambda struct: re.findall(r"(\w+)(?:\[2\])?[,;]", re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), header, re.S)[1]))
    fields = ["tileShift", "source", "mask", "dilate", "framesA", "framesB", "flags", "reserved"]
    assert names("PtxAdaptiveDesc") == fields
    D = pkg.AdaptiveDesc
    assert C.sizeof(D) == 40 and [getattr(D, f).offset for f in fields] == [0, 4, 8, 16, 20, 24, 28, 32]
    assert tuple(names("PtxAdaptivePlan")) == PLAN_FIELDS
    P = pkg.AdaptivePlan
    assert C.sizeof(P) == 24 and [getattr(P, f).offset for f in PLAN_FIELDS] == list(range(0, 24, 4)) and all(t is C.c_uint32 for _, t in P._fields_)
    fields = ["pendingA", "pendingB", "normalizeTo", "exposure", "threshold", "tileShift", "flags", "reserved"]
    assert names("PtxAdaptiveMeterDesc") == fields
    M = pkg.AdaptiveMeterDesc
    assert C.sizeof(M) == 36 and [getattr(M, f).offset for f in fields] == list(range(0, 32, 4))
    assert dict(M._fields_)["exposure"] is C.c_float and dict(M._fields_)["threshold"] is C.c_float
    assert re.search(r"PTX_ADAPTIVE_FROM_NOISE = 0u, PTX_ADAPTIVE_FROM_MASK = 1u", header)
    assert (pkg.ADAPTIVE_FROM_NOISE, pkg.ADAPTIVE_FROM_MASK) == (0, 1) == (AR.FROM_NOISE, AR.FROM_MASK)
    # the semantics are in the header as text: the reference is written from it
    flat = re.sub(r"\s*\n \*\s*", " ", header)
    for phrase in ("Adaptive sampling", "section 27", "1. COMMIT", "countA[t] += framesA and countB[t] += framesB", "With no plan in force every tile counts as active",
                   "2. SEED AND DILATE", "marks it not converged", "t is a seed iff mask[t] != 0", "max(|tx - sx|, |ty - sy|) <= dilate", "3. COMPACT", "in ascending order, by a scan",
                   "no atomic's arrival order can show in it", "a ragged tile counts less", "two slots never own one pixel", "every other pixel keeps its bits",
                   "activePixels * frames * SampleCount plus retries", "An empty plan (activeTiles = 0) renders and accumulates nothing", "SYNCHRONOUS",
                   "a refused call leaves the plan, the counts and the list intact", "sharded frames are refused", "starts anew with every plan",
                   "COUNTS PER TILE", "NA_t = countA[t] + (active(t) ? pendingA : 0)", "with no plan in force every tile is active", "STEP 2 PER TILE",
                   "sa_t = exposure * rcp((float)NA_t)", "st_t = exposure * rcp((float)N_t)", "a tile with NA_t == 0 or NB_t == 0 has all its pixels REJECTED and is not converged",
                   "An unsampled tile never freezes", "stores S where N_t == normalizeTo or N_t == 0, and S * k_t elsewhere", "k_t = (float)normalizeTo * rcp((float)N_t)",
                   "alpha included", "ptx_read_noise reads it", "The counts stay"):
        assert phrase in flat, phrase
    assert "there is no adaptive sampling" not in flat
    for method in ("adaptive_plan", "read_adaptive", "adaptive_clear", "noise_meter_adaptive"):
        assert callable(getattr(pkg.Renderer, method))
    kernel = open(os.path.join(pkg.PKG_DIR, "csrc", "pt_adaptive.hpp")).read()
    for name in ("k_adaptive_plan", "k_noise_tiles_adaptive", "__shfl_up"):
        assert name in kernel, name
    assert "atomic" not in re.sub(r"//.*", "", kernel)
    assert "k_adaptive" not in open(os.path.join(pkg.PKG_DIR, "csrc", "pt_wavefront.hpp")).read()
    # the adapter's defaults are the package's
    assert pkg.ADAPTIVE_DEFAULTS == dict(dilate=1)
    host = open(os.path.join(pkg.PKG_DIR, "host", "RendererHip.h")).read()
    m = re.search(r"struct AdaptiveSettings\s*\{\s*bool Enabled = false;\s*uint32_t Dilate = (\d+);\s*\};", host)
    assert m and int(m[1]) == pkg.ADAPTIVE_DEFAULTS["dilate"]
    adapter = open(os.path.join(pkg.PKG_DIR, "host", "RendererHip.cpp")).read()
    for call in ("ptx_adaptive_plan(s_Renderer", "ptx_noise_meter_adaptive(s_Renderer", "ptx_adaptive_clear(s_Renderer"):
        assert call in adapter, call
    assert "--adaptive" in open(os.path.join(pkg.REPO_DIR, "examples", "render_scene.cpp")).read()


def test_the_plan_by_hand_at_67_by_45():
    by_hand = {3: (9, 6, [8] * 8 + [3], [8] * 5 + [5]), 4: (5, 3, [16] * 4 + [3], [16, 16, 13]), 5: (3, 2, [32, 32, 3], [32, 13]), 6: (2, 1, [64, 3], [45])}
    for shift, (tx, ty, widths, heights) in by_hand.items():
        assert AR.tiling(W, H, shift) == (tx, ty) and sum(widths) == W and sum(heights) == H
        area = np.outer(heights, widths)
        assert (AR.tile_pixels(W, H, shift) == area).all()
        # one seed in a corner, on an edge and in the middle, dilate 0, 1 and 2: the active tiles are the clipped square around it
        for sy, sx in {(0, 0), (ty - 1, tx - 1), (0, tx // 2), (ty // 2, 0), (ty // 2, tx // 2)}:
            for dilate in DILATES:
                mask = np.zeros((ty, tx), np.uint8)
                mask[sy, sx] = 7
                plan, ids = AR.Planner(W, H).plan(shift, mask, dilate)
                ys, xs = range(max(0, sy - dilate), min(ty, sy + dilate + 1)), range(max(0, sx - dilate), min(tx, sx + dilate + 1))
                want = [y * tx + x for y in ys for x in xs]
                assert list(ids) == want and sorted(set(want)) == want and plan["activeTiles"] == len(want) and plan["seedTiles"] == 1
                assert plan["activePixels"] == sum(int(area[y, x]) for y in ys for x in xs)
                assert (plan["tilesX"], plan["tilesY"], plan["generation"]) == (tx, ty, 1)
        # the ragged corner alone
        last = np.zeros((ty, tx), np.uint8)
        last[-1, -1] = 1
        assert AR.Planner(W, H).plan(shift, last)[0]["activePixels"] == widths[-1] * heights[-1]
        # an empty mask and a full one
        p = AR.Planner(W, H)
        plan, ids = p.plan(shift, np.zeros((ty, tx)), 2)
        assert plan["activeTiles"] == 0 == plan["activePixels"] == plan["seedTiles"] and len(ids) == 0 and not p.pixel_mask().any()
        plan, ids = p.plan(shift, np.ones((ty, tx)), 0)
        assert plan["activeTiles"] == tx * ty and plan["activePixels"] == W * H and list(ids) == list(range(tx * ty)) and p.pixel_mask().all() and plan["generation"] == 2
    # the commit rule over three plans in a row, 16-pixel tiles: no plan = all tiles, then the plan being replaced
    p = AR.Planner(W, H)
    first = np.zeros((3, 5), np.uint8)
    first[0, 0] = first[2, 4] = 1
    p.plan(4, first, 0, 8, 8)                      # the warm-up frames enter every tile's counts
    assert (p.counts == 8).all()
    second = np.zeros((3, 5), np.uint8)
    second[1, 2] = 1
    p.plan(4, second, 1, 3, 2)                     # rendered under `first`: its two tiles only
    want = np.full((2, 3, 5), 8)
    want[0][first != 0] += 3
    want[1][first != 0] += 2
    assert (p.counts == want).all()
    p.plan(4, np.zeros((3, 5)), 0, 0, 5)           # rendered under `second` dilated by 1: the 3 x 3 block round (1, 2)
    want[1, 0:3, 1:4] += 5
    assert (p.counts == want).all() and p.active is not None and not p.active.any()
    p.plan(4, np.ones((3, 5)), 0, 9, 9)            # rendered under an empty plan: nothing
    assert (p.counts == want).all()
    p.clear()
    p.plan(4, first, 0, 1, 0)                      # cleared: every tile again
    want[0] += 1
    assert (p.counts == want).all()
    p.zero_counts()
    assert not p.counts.any() and p.generation == 5


def test_the_adaptive_meter_on_the_reference():
    rng = np.random.default_rng(11)
    A = (2.0 ** rng.uniform(-3, 3, (H, W, 4))).astype(np.float32)
    B = (A * rng.uniform(0.5, 1.5, (H, W, 4))).astype(np.float32)
    for shift in SHIFTS:
        tx, ty = AR.tiling(W, H, shift)
        # equal counts everywhere reproduce noise_ref's result bit for bit, with the counts committed, pending or both
        want, E, p = NR.meter(A, B, 5, 3, 1.5, 0.05, shift, calls=4)
        for committed, pending in (((5, 3), (0, 0)), ((0, 0), (5, 3)), ((2, 1), (3, 2))):
            counts = np.stack([np.full((ty, tx), committed[0]), np.full((ty, tx), committed[1])])
            for active in (None, np.ones((ty, tx), bool)):
                got, Eg, q = AR.meter(A, B, counts, active, pending[0], pending[1], 8, 1.5, 0.05, shift, calls=4)
                assert {k: (f32(v).tobytes() if isinstance(v, np.floating) else v) for k, v in got.items()} == {
                    k: (f32(v).tobytes() if isinstance(v, np.floating) else v) for k, v in want.items()}
                assert (_bits(Eg) == _bits(E)).all() and (q["q"] == p["q"]).all() and (_bits(q["image"]) == _bits(p["S"])).all()  # n_t == normalizeTo: S as it is
    # a tile with a zero count in either half is rejected and not converged, whatever its pixels hold; the others are unchanged
    shift = 4
    tx, ty = AR.tiling(W, H, shift)
    counts = np.full((2, ty, tx), 4)
    counts[:, 0, 0] = 0            # never sampled
    counts[1, 1, 2] = 0            # half 1 never sampled
    counts[:, 2, 4] = (6, 2)       # more frames than the rest
    got, E, q = AR.meter(A, A, counts, None, 0, 0, 8, 1.0, 10.0, shift)
    assert got["converged"] == tx * ty - 2 and not q["converged"][0, 0] and not q["converged"][1, 2] and E[0, 0] == 0 and E[1, 2] == 0
    assert got["rejected"] == 16 * 16 * 2 and q["rejected"][:16, :16].all() and q["rejected"][16:32, 32:48].all() and got["counted"] == W * H - 512
    # with pending frames only the active tiles receive them: an inactive unsampled tile stays unsampled
    active = np.ones((ty, tx), bool)
    active[0, 0] = False
    got2, _, q2 = AR.meter(A, A, counts, active, 1, 1, 10, 1.0, 10.0, shift)
    assert not q2["converged"][0, 0] and q2["converged"][1, 2] and q2["NA"][0, 0] == 0 and q2["NA"][1, 2] == 5 and q2["NB"][1, 2] == 1 and got2["converged"] == tx * ty - 1
    # k_t is skipped exactly where n_t == normalizeTo (and where n_t == 0)
    S = (A + A).astype(np.float32)
    img = q["image"]
    assert (_bits(img[:16, :16]) == _bits(S[:16, :16])).all()                              # n_t = 0
    assert (_bits(img[0:16, 16:32]) == _bits(S[0:16, 16:32])).all()                        # n_t = 8 = normalizeTo
    assert (_bits(img[32:, 64:]) == _bits(S[32:, 64:])).all()                              # 6 + 2 = 8 too
    assert (_bits(img[16:32, 32:48]) == _bits((S[16:32, 32:48] * f32(2.0)).astype(f32))).all()   # n_t = 4: k_t = 8 * rcp(4) = 2, alpha included
    k = f32(7.0) * (f32(1.0) / f32(3.0))
    third = AR.meter(A, A, np.full((2, ty, tx), 1), None, 1, 0, 7, 1.0, 10.0, shift)[2]["image"]   # n_t = 3: k_t = 7 * rcp(3), rounded twice
    assert (_bits(third) == _bits((S * k).astype(f32))).all() and k != f32(7.0 / 3.0)


def test_the_loop_threshold_splits_the_oracles_tiles(pkg, orc):
    """LOOP_THRESHOLD is the median E_t of the oracle's 8 + 8 frames; on those frames alone it leaves at least a quarter of the tiles
    seeded and at least a quarter unseeded"""
    half = _loop_halves(pkg, orc)
    res, E, _ = NR.meter(half[0], half[1], LOOP_WARMUP // 2, LOOP_WARMUP // 2, 1.0, LOOP_THRESHOLD, LOOP_SHIFT)
    tiles = res["tilesX"] * res["tilesY"]
    seeded = tiles - res["converged"]
    print(f"median E_t {float(np.sort(E.ravel())[E.size // 2])!r}; {seeded} of {tiles} tiles seeded at {LOOP_THRESHOLD!r}")
    assert f32(LOOP_THRESHOLD) == np.sort(E.ravel())[E.size // 2]
    assert 4 * seeded >= tiles and 4 * (tiles - seeded) >= tiles


# =====================================================================================================
# on the GPU
# =====================================================================================================
_state = {}


def _gpu(pkg, scene="default"):
    """(scene, renderer) of `scene`, uploaded once; the renderer comes back unsharded, at 67 x 45, without halves, plan or counts"""
    import torch  # noqa: F401  (first, so the HIP library shares torch's HIP runtime)

    if scene not in _state:
        s = pkg.Scene(scene, SCENES[scene])
        r = pkg.Renderer()
        r.upload(s)
        _state[scene] = (s, r)
    s, r = _state[scene]
    r.set_backend(pkg.BACKEND_WAVEFRONT)
    r.set_tile_shard(0, 1, 32)
    r.resize(W, H)
    return s, r


def _plain(pkg, w, h):
    """a handle with no scene: the plan and the meter need none"""
    import torch  # noqa: F401

    f = pkg.Renderer()
    f.resize(w, h)
    return f


def _bind(r, which):
    """half 0 / 1, or None: the internal image"""
    if which is None:
        r.bind_accumulation(0, 0)
    else:
        assert r.noise_half_ptr(which)
        r.bind_accumulation(r.noise_half_ptr(which), r.width * r.height * 16)


def _write_halves(r, A, B):
    for which, img in enumerate((A, B)):
        _bind(r, which)
        r.write_accumulation(img)
    _bind(r, None)


def _read_halves(r):
    out = []
    for which in range(2):
        _bind(r, which)
        out.append(r.readback())
    _bind(r, None)
    return out


def _plan_fields(p):
    return {k: int(getattr(p, k)) for k in PLAN_FIELDS}


def _assert_plan(r, got, want, ids, ref, what):
    assert _plan_fields(got) == want, (what, _plan_fields(got), want)
    plan, tiles, counts = r.read_adaptive()
    assert _plan_fields(plan) == want, what
    assert tiles.dtype == np.uint32 and list(tiles) == list(ids), (what, tiles[:16], ids[:16])
    assert (counts.astype(np.int64) == ref.counts).all(), (what, np.argwhere(counts != ref.counts)[:8])


def _assert_noise(r, want, E, what):
    res, tiles = r.read_noise(tile_errors=True)
    got = {k: getattr(res, k) for k in NOISE_INTS}
    assert got == {k: int(want[k]) for k in NOISE_INTS}, (what, got, want)
    for k in ("meanError", "maxError"):
        g, v = f32(getattr(res, k)), f32(want[k])
        assert g.view(np.uint32) == v.view(np.uint32), (what, k, float(g), float(v))
    assert tiles.shape == E.shape and (_bits(tiles) == _bits(E)).all(), (what, np.argwhere(_bits(tiles) != _bits(E))[:8])
    return res


def _pattern(h, w):
    """a known image: every pixel its own finite, non-zero bits"""
    p = (np.arange(h * w * 4, dtype=np.float32).reshape(h, w, 4) * f32(0.0078125) + f32(0.25)).astype(np.float32)
    p[..., 3] = 3.0
    return p


@pytest.mark.gpu
@pytest.mark.parametrize("extent", list(EXTENTS))
def test_plan_from_a_mask_equals_the_reference(pkg, extent):
    w, h = EXTENTS[extent]
    r = _plain(pkg, w, h)
    calls = 0
    for shift in SHIFTS:
        r.resize(w, h)  # drops the plan and the counts of the last tile size
        ref = AR.Planner(w, h)
        tx, ty = AR.tiling(w, h, shift)
        for dilate in DILATES:
            for name, mask in _masks(tx, ty, dilate).items():
                fa, fb = FRAMES[calls % len(FRAMES)]
                calls += 1
                got = r.adaptive_plan(shift, mask=mask, dilate=dilate, frames_a=fa, frames_b=fb)
                want, ids = ref.plan(shift, mask, dilate, fa, fb)
                _assert_plan(r, got, want, ids, ref, (extent, shift, dilate, name))
        assert ref.counts.any() or tx * ty == 1
        # ptx_adaptive_clear: the next commit reaches every tile; ptx_noise_halves(1) zeroes the counts and keeps the plan
        r.adaptive_clear()
        assert r.read_adaptive()[0].activeTiles == 0
        ref.clear()
        got = r.adaptive_plan(shift, mask=_masks(tx, ty)["checkerboard"], dilate=0, frames_a=7, frames_b=1)
        want, ids = ref.plan(shift, _masks(tx, ty)["checkerboard"], 0, 7, 1)
        _assert_plan(r, got, want, ids, ref, (extent, shift, "after clear"))
        r.noise_halves(True)
        ref.zero_counts()
        _assert_plan(r, got, want, ids, ref, (extent, shift, "halves"))
        got = r.adaptive_plan(shift, mask=_masks(tx, ty)["full"], dilate=0, frames_a=2, frames_b=3)
        want, ids = ref.plan(shift, _masks(tx, ty)["full"], 0, 2, 3)
        _assert_plan(r, got, want, ids, ref, (extent, shift, "after halves"))
    r.close()


@pytest.mark.gpu
def test_plan_from_the_noise_meters_records_equals_the_reference(pkg):
    s, r = _gpu(pkg, "texture_test")
    r.noise_halves(True)
    u = s.uniform(W, H, bounces=3)
    for f in range(8):
        _bind(r, f & 1)
        u.TotalSamples = f
        r.render(u, s.lights)
    _bind(r, None)
    lib = pkg.load_hip()
    seeded = 0
    for shift in SHIFTS:
        r.noise_meter(4, 4, 1.0, 0.0, shift)
        E = r.read_noise(tile_errors=True)[1]
        threshold = float(np.sort(E.ravel())[E.size // 2])
        ref = AR.Planner(W, H)
        for k, dilate in enumerate(DILATES):
            r.noise_meter(4, 4, 1.0, threshold if k != 2 else 0.0, shift)
            res, E = r.read_noise(tile_errors=True)
            seeds = ~(E <= f32(threshold if k != 2 else 0.0))
            assert int(seeds.sum()) == res.tilesX * res.tilesY - res.converged
            fa, fb = FRAMES[k + 1]
            got = r.adaptive_plan(shift, dilate=dilate, frames_a=fa, frames_b=fb)
            want, ids = ref.plan(shift, seeds, dilate, fa, fb)
            _assert_plan(r, got, want, ids, ref, (shift, dilate))
            seeded += want["seedTiles"]
        # a meter of another tile size is refused as a source, and leaves everything as it was
        other = 3 if shift != 3 else 4
        r.noise_meter(4, 4, 1.0, 0.0, other)
        d = pkg.AdaptiveDesc(shift, pkg.ADAPTIVE_FROM_NOISE, None, 0, 0, 0, 0, (C.c_uint32 * 2)(0, 0))
        assert lib.ptx_adaptive_plan(r.handle, C.byref(d), C.byref(pkg.AdaptivePlan())) == NOT_READY
        _assert_plan(r, got, want, ids, ref, (shift, "refused"))
        r.noise_halves(True)  # zero counts: the next tile size is accepted
        r.adaptive_clear()
        for f in range(8):
            _bind(r, f & 1)
            u.TotalSamples = f
            r.render(u, s.lights)
        _bind(r, None)
    assert seeded > 0
    r.noise_halves(False)


def _variants(pkg):
    """(name, frames per call or None for ptx_render, calls, SampleCount, BounceCount, backend)"""
    return (("render", None, 3, 1, 3, pkg.BACKEND_WAVEFRONT), ("frames8", 8, 1, 1, 3, pkg.BACKEND_WAVEFRONT), ("restart", None, 2, 3, 3, pkg.BACKEND_WAVEFRONT),
            ("bounce0", None, 2, 1, 0, pkg.BACKEND_WAVEFRONT), ("megakernel", None, 2, 1, 3, pkg.BACKEND_MEGAKERNEL))


def _render_variant(r, s, w, h, variant, first, plan=None):
    """the variant's calls from frame `first` on; with a plan every call's pathSamples is checked"""
    name, block, calls, sc, depth, backend = variant
    r.set_backend(backend)
    u = s.uniform(w, h, bounces=depth, sample_count=sc)
    stats = []
    for k in range(calls):
        if block:
            r.render_frames(u, s.lights, first + k * block, block)
        else:
            u.TotalSamples = first + k
            r.render(u, s.lights)
        st = r.stats()
        stats.append({f: int(getattr(st, f)) for f in STAT_FIELDS})
        if plan is not None:
            assert st.pathSamples == plan.activePixels * (block or 1) * sc + st.retries, (name, k, st.pathSamples, plan.activePixels, st.retries)
    return stats


def _planned_render_cases(pkg, r, s, w, h, shifts=(3, 6), variants=None):
    pattern = _pattern(h, w)
    touched = 0
    for shift in shifts:
        tx, ty = AR.tiling(w, h, shift)
        mask = _masks(tx, ty, 5)["random"]
        mask[-1, -1] = 1            # the ragged corner takes part ...
        mask[0, 0] = 0 if tx * ty > 1 else 1   # ... and the first tile does not
        for variant in variants or _variants(pkg):
            first = 5
            r.adaptive_clear()
            r.write_accumulation(pattern)
            _render_variant(r, s, w, h, variant, first)
            full = r.readback()                      # the pattern plus a fresh sum of those frames
            ref = AR.Planner(w, h)
            plan = r.adaptive_plan(shift, mask=mask, dilate=0)
            want, ids = ref.plan(shift, mask, 0)
            assert _plan_fields(plan)["activePixels"] == want["activePixels"] and 0 < plan.activeTiles
            r.write_accumulation(pattern)
            _render_variant(r, s, w, h, variant, first, plan)
            got = r.readback()
            inside = ref.pixel_mask()
            expect = np.where(inside[..., None], full, pattern)
            assert (_bits(got) == _bits(expect)).all(), (variant[0], shift, np.argwhere((_bits(got) != _bits(expect)).any(-1))[:8])
            assert (_bits(full)[inside] != _bits(pattern)[inside]).any()
            touched += int(inside.sum())
    r.adaptive_clear()
    r.set_backend(pkg.BACKEND_WAVEFRONT)
    return touched


@pytest.mark.gpu
@pytest.mark.parametrize("extent", ["67x45", "130x70"])
@pytest.mark.parametrize("scene", list(SCENES))
def test_a_planned_render_is_the_full_render_where_it_is_active_and_nothing_elsewhere(pkg, scene, extent):
    w, h = EXTENTS[extent]
    s, r = _gpu(pkg, scene)
    r.resize(w, h)
    assert _planned_render_cases(pkg, r, s, w, h) > 0


@pytest.mark.gpu
def test_a_planned_render_with_primary_rays_from_k_generate(pkg, monkeypatch):
    """PTX_FIRST_BOUNCE=0, as tests/test_first_bounce.py selects it: the variable is read when the handle is created"""
    import torch  # noqa: F401

    monkeypatch.setenv("PTX_FIRST_BOUNCE", "0")
    s = pkg.Scene("texture_test", SCENES["texture_test"])
    r = pkg.Renderer()
    r.upload(s)
    r.resize(W, H)
    assert _planned_render_cases(pkg, r, s, W, H, variants=_variants(pkg)[:3]) > 0
    r.close()


@pytest.mark.gpu
def test_a_full_plan_is_the_unplanned_render_and_an_empty_plan_renders_nothing(pkg):
    s, r = _gpu(pkg)
    pattern = _pattern(H, W)
    for shift in (3, 5):
        tx, ty = AR.tiling(W, H, shift)
        for variant in _variants(pkg):
            r.adaptive_clear()
            r.write_accumulation(pattern)
            stats = _render_variant(r, s, W, H, variant, 2)
            full = r.readback()
            plan = r.adaptive_plan(shift, mask=np.ones((ty, tx)), dilate=0)
            assert plan.activeTiles == tx * ty and plan.activePixels == W * H
            r.write_accumulation(pattern)
            assert _render_variant(r, s, W, H, variant, 2, plan) == stats, variant[0]
            assert (_bits(r.readback()) == _bits(full)).all(), variant[0]
            plan = r.adaptive_plan(shift, mask=np.zeros((ty, tx)), dilate=2)
            assert plan.activeTiles == 0 and plan.activePixels == 0
            r.write_accumulation(pattern)
            for st in _render_variant(r, s, W, H, variant, 2, plan):
                assert st["pathSamples"] == 0 and st["segments"] == 0, variant[0]
            assert (_bits(r.readback()) == _bits(pattern)).all(), variant[0]
    r.adaptive_clear()
    r.set_backend(pkg.BACKEND_WAVEFRONT)


@pytest.mark.gpu
def test_nothing_leaks_from_a_plan(pkg):
    import torch

    lib = pkg.load_hip()
    s, r = _gpu(pkg, "texture_test")
    u = s.uniform(W, H, bounces=3)
    fresh = pkg.Renderer()
    fresh.share_scene(r)
    fresh.resize(W, H)
    tx, ty = AR.tiling(W, H, 3)
    mask = _masks(tx, ty)["checkerboard"]
    out = pkg.AdaptivePlan()

    def plain(x, frame=4):
        x.reset()
        u.TotalSamples = frame
        x.render(u, s.lights)
        return x.readback()
    want = plain(fresh)
    plan = r.adaptive_plan(3, mask=mask, dilate=0)
    assert 0 < plan.activeTiles < tx * ty
    assert (_bits(plain(r)) != _bits(want)).any()
    # the guide pass, the debug view and the output stage keep the frame
    r.write_accumulation(want)
    r.render_guides(u)
    fresh.render_guides(u)
    for k in range(3):
        assert (_bits(r.read_guide(k)) == _bits(fresh.read_guide(k))).all(), k
    r.postprocess(1, **POST)
    fresh.postprocess(1, **POST)
    assert (_bits(r.read_output(pkg.OUTPUT_RGBA32F)) == _bits(fresh.read_output(pkg.OUTPUT_RGBA32F))).all()
    r.render_debug(u, s.lights, pkg.DEBUG_MODE_NORMAL)
    fresh.render_debug(u, s.lights, pkg.DEBUG_MODE_NORMAL)
    assert (_bits(r.readback()) == _bits(fresh.readback())).all()
    want = plain(fresh)
    # after ptx_adaptive_clear the next ptx_render is a fresh handle's
    r.adaptive_clear()
    assert (_bits(plain(r)) == _bits(want)).all()
    # ptx_resize, a change of the shard and ptx_noise_halves(0) drop the plan and the counts
    for drop in ("resize", "shard", "halves", "same shard"):
        plan = r.adaptive_plan(3, mask=mask, dilate=0, frames_a=1, frames_b=1)
        assert (_bits(plain(r)) != _bits(want)).any() and lib.ptx_read_adaptive(r.handle, C.byref(out), None, 0, None, 0) == OK
        if drop == "resize":
            r.resize(W, H)
        elif drop == "shard":
            r.set_tile_shard(0, 1, 16)
        elif drop == "halves":
            r.noise_halves(True)
            assert lib.ptx_read_adaptive(r.handle, C.byref(out), None, 0, None, 0) == OK and not r.read_adaptive()[2].any() and out.activeTiles == plan.activeTiles
            r.noise_halves(False)
        else:
            r.set_tile_shard(0, 1, 16)  # no change: the plan stays
            assert lib.ptx_read_adaptive(r.handle, C.byref(out), None, 0, None, 0) == OK and out.activeTiles == plan.activeTiles
            r.adaptive_clear()
            assert r.read_adaptive()[2].all()  # the counts stay
            r.set_tile_shard(0, 1, 32)
        assert (_bits(plain(r)) == _bits(want)).all(), drop
        assert lib.ptx_read_adaptive(r.handle, C.byref(out), None, 0, None, 0) == NOT_READY, drop
    # binding a shard buffer ends the plan, the counts stay
    r.adaptive_plan(3, mask=mask, dilate=0, frames_a=1, frames_b=0)
    shard = torch.zeros(r.shard_bytes(0) // 4, dtype=torch.float32, device="cuda")
    r.bind_shard_accumulation(shard.data_ptr(), shard.numel() * 4)
    r.bind_shard_accumulation(0, 0)
    assert r.read_adaptive()[0].activeTiles == 0 and (r.read_adaptive()[2][0] == 1).all()
    assert (_bits(plain(r)) == _bits(want)).all()
    r.resize(W, H)
    # a borrower of a shared scene plans and renders
    plan = fresh.adaptive_plan(3, mask=mask, dilate=0)
    ref = AR.Planner(W, H)
    ref.plan(3, mask, 0)
    pattern = _pattern(H, W)
    fresh.write_accumulation(pattern)
    u.TotalSamples = 4
    fresh.render(u, s.lights)
    inside = ref.pixel_mask()[..., None]
    got = fresh.readback()
    assert (_bits(got)[~inside[..., 0]] == _bits(pattern)[~inside[..., 0]]).all() and (_bits(got)[inside[..., 0]] != _bits(pattern)[inside[..., 0]]).any()
    assert fresh.stats().pathSamples == plan.activePixels + fresh.stats().retries
    fresh.close()


def _hand_counts(r, ref, shift, tx, ty, seed):
    """counts set by hand through mask plans: some tiles never sampled, one half of some never sampled, the rest unequal"""
    rng = np.random.default_rng(seed)
    first = (rng.random((ty, tx)) < 0.8).astype(np.uint8)
    second = (rng.random((ty, tx)) < 0.5).astype(np.uint8)
    third = (rng.random((ty, tx)) < 0.5).astype(np.uint8)
    for mask, (fa, fb) in ((first, (0, 0)), (second, (2, 2)), (third, (3, 0)), (first, (0, 1))):
        got = r.adaptive_plan(shift, mask=mask, dilate=0, frames_a=fa, frames_b=fb)
        ref.plan(shift, mask, 0, fa, fb)
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("extent", ["67x45", "300x200"])
def test_adaptive_meter_equals_the_reference_on_synthetic_halves_with_hand_set_counts(pkg, extent):
    import test_noise_meter as TN

    w, h = EXTENTS[extent]
    A, B = TN._synthetic_halves(h, w)
    r = _plain(pkg, w, h)
    seen = dict(zero=0, scaled=0, plain=0, unconverged=0)
    for shift in SHIFTS:
        r.resize(w, h)  # drops the counts of the last tile size, and the meter counts its calls anew
        calls = 0
        r.noise_halves(True)
        _write_halves(r, A, B)
        A, B = _read_halves(r)
        ref = AR.Planner(w, h)
        tx, ty = AR.tiling(w, h, shift)
        _hand_counts(r, ref, shift, tx, ty, shift)
        assert (r.read_adaptive()[2].astype(np.int64) == ref.counts).all()
        marker = np.full((h, w, 4), 7.25, np.float32)
        r.write_accumulation(marker)
        # _hand_counts leaves NA_t = 2 [first] + 3 [second] and NB_t = 2 [first] + [third] with `first` in force: every normalizeTo below is some tile's N_t
        for pending, normalize_to, exposure, threshold, planned in (((1, 1), 7, 1.0, 0.05, True), ((0, 0), 5, 2.75, 0.3, True), ((2, 1), 7, 1.0, 0.0, False)):
            if not planned:
                r.adaptive_clear()
                ref.clear()
            calls += 1
            want, E, p = AR.meter(A, B, ref.counts, ref.active, pending[0], pending[1], normalize_to, exposure, threshold, shift, calls=calls)
            r.noise_meter_adaptive(pending[0], pending[1], normalize_to, exposure, threshold, shift)
            _assert_noise(r, want, E, (extent, shift, pending, normalize_to))
            assert (_bits(r.readback()) == _bits(marker)).all()  # without the flag the internal image keeps its bits
            _bind(r, 1)
            r.noise_meter_adaptive(pending[0], pending[1], normalize_to, exposure, threshold, shift, write_sum=True)
            assert r.accum_ptr() == r.noise_half_ptr(1)  # the binding is not changed
            _bind(r, None)
            calls += 1
            want["calls"] = calls
            _assert_noise(r, want, E, (extent, shift, pending, normalize_to, "write_sum"))
            image = r.readback()
            assert _same_sum(image, p["image"]), (extent, shift, pending, normalize_to)
            n = p["NA"] + p["NB"]
            seen["zero"] += int(((p["NA"] == 0) | (p["NB"] == 0)).sum())
            seen["scaled"] += int(((n != normalize_to) & (n != 0)).sum())
            seen["plain"] += int((n == normalize_to).sum())
            seen["unconverged"] += want["tilesX"] * want["tilesY"] - want["converged"]
            r.write_accumulation(marker)
        # ptx_noise_meter itself on the same halves still gives what it gave
        r.noise_meter(3, 8, 1.0, 0.05, shift)
        want, E, _ = NR.meter(A, B, 3, 8, 1.0, 0.05, shift, calls=calls + 1)
        _assert_noise(r, want, E, (extent, shift, "ptx_noise_meter"))
        got = _read_halves(r)
        assert (_bits(got[0]) == _bits(A)).all() and (_bits(got[1]) == _bits(B)).all()  # the halves are only read
    print(f"{extent}: tiles over all calls {seen}")
    assert all(v > 0 for v in seen.values()), seen
    r.close()


@pytest.mark.gpu
def test_adaptive_meter_equals_the_reference_on_halves_rendered_under_two_plans(pkg):
    w, h = EXTENTS["130x70"]
    s, r = _gpu(pkg)
    r.resize(w, h)
    r.noise_halves(True)
    u = s.uniform(w, h, bounces=3)
    shift = 4
    tx, ty = AR.tiling(w, h, shift)
    ref = AR.Planner(w, h)
    frame = 0

    def render(pairs):
        nonlocal frame
        for _ in range(2 * pairs):
            _bind(r, frame & 1)
            u.TotalSamples = frame
            r.render(u, s.lights)
            frame += 1
        _bind(r, None)
    render(2)
    masks = _masks(tx, ty, 3)
    r.adaptive_plan(shift, mask=masks["random"], dilate=1, frames_a=2, frames_b=2)
    ref.plan(shift, masks["random"], 1, 2, 2)
    render(2)
    r.adaptive_plan(shift, mask=masks["checkerboard"], dilate=0, frames_a=2, frames_b=2)
    ref.plan(shift, masks["checkerboard"], 0, 2, 2)
    render(1)
    assert (r.read_adaptive()[2].astype(np.int64) == ref.counts).all() and len(np.unique(ref.counts)) > 1
    A, B = _read_halves(r)
    total = frame
    want, E, p = AR.meter(A, B, ref.counts, ref.active, 1, 1, total, POST["exposure"], 0.05, shift)
    assert int((p["NA"] + p["NB"]).max()) == total and int((p["NA"] + p["NB"]).min()) < total
    r.noise_meter_adaptive(1, 1, total, POST["exposure"], 0.05, shift, write_sum=True)
    _assert_noise(r, want, E, "rendered")
    image = r.readback()
    assert (_bits(image) == _bits(p["image"])).all()
    # ptx_postprocess behind it is a fresh handle's on write_accumulation of that image
    r.postprocess(total, **POST)
    f = _plain(pkg, w, h)
    f.write_accumulation(p["image"])
    f.postprocess(total, **POST)
    assert (_bits(r.read_output(pkg.OUTPUT_RGBA32F)) == _bits(f.read_output(pkg.OUTPUT_RGBA32F))).all()
    f.close()
    # every tile's own mean: image / total is (A + B) / n_t up to the two roundings of k_t
    side = 1 << shift
    n = np.kron(p["NA"] + p["NB"], np.ones((side, side), np.int64))[:h, :w]
    assert np.allclose(image[..., :3] / total, (A + B)[..., :3] / n[..., None], rtol=1e-6, atol=0)
    # each half at every pixel is a fresh sum of exactly the frames its tile took part in
    r.adaptive_clear()
    r.noise_halves(False)
    schedule = [(0, 4, np.ones((ty, tx), bool)), (4, 8, AR.dilated(masks["random"] != 0, 1)), (8, 10, masks["checkerboard"] != 0)]
    for which, got in enumerate((A, B)):
        expect = np.zeros((h, w, 4), np.float32)
        # per distinct set of frames: render that set uniformly into a fresh image and take the tiles with exactly that set
        sets = {}
        for j in range(ty):
            for i in range(tx):
                frames = tuple(fr for lo, hi, act in schedule if act[j, i] for fr in range(lo, hi) if (fr & 1) == which)
                sets.setdefault(frames, []).append((j, i))
        for frames, tiles in sets.items():
            r.reset()
            for fr in frames:
                u.TotalSamples = fr
                r.render(u, s.lights)
            img = r.readback()
            for j, i in tiles:
                win = (slice(j * side, min(h, (j + 1) * side)), slice(i * side, min(w, (i + 1) * side)))
                expect[win] = img[win]
        assert (_bits(got) == _bits(expect)).all(), which


@pytest.mark.gpu
def test_refusals_leave_the_plan_the_counts_the_list_the_noise_state_and_the_internal_image_intact(pkg):
    import torch

    import test_noise_meter as TN

    lib = pkg.load_hip()
    A, B = TN._synthetic_halves(H, W)
    r = _plain(pkg, W, H)
    r.noise_halves(True)
    _write_halves(r, A, B)
    marker = np.full((H, W, 4), 3.5, np.float32)
    r.write_accumulation(marker)
    tx, ty = AR.tiling(W, H, 4)
    mask = np.ascontiguousarray(_masks(tx, ty)["checkerboard"])
    r.adaptive_plan(4, mask=mask, dilate=0, frames_a=2, frames_b=3)
    r.adaptive_plan(4, mask=mask, dilate=1, frames_a=1, frames_b=1)
    r.noise_meter_adaptive(1, 1, 7, 1.0, 0.05, 4)
    state = (r.read_adaptive(), r.read_noise(tile_errors=True))
    out = pkg.AdaptivePlan()

    def intact(what):
        plan, tiles, counts = r.read_adaptive()
        assert bytes(plan) == bytes(state[0][0]) and (tiles == state[0][1]).all() and (counts == state[0][2]).all(), what
        res, E = r.read_noise(tile_errors=True)
        assert bytes(res) == bytes(state[1][0]) and (_bits(E) == _bits(state[1][1])).all(), what
        _bind(r, None)
        assert (_bits(r.readback()) == _bits(marker)).all(), what

    def desc(**kw):
        d = dict(tileShift=4, source=pkg.ADAPTIVE_FROM_MASK, mask=mask.ctypes.data, dilate=1, framesA=1, framesB=1, flags=0, reserved=(0, 0))
        d.update(kw)
        return pkg.AdaptiveDesc(d["tileShift"], d["source"], d["mask"], d["dilate"], d["framesA"], d["framesB"], d["flags"], (C.c_uint32 * 2)(*d["reserved"]))

    def mdesc(**kw):
        d = dict(pendingA=1, pendingB=1, normalizeTo=7, exposure=1.0, threshold=0.05, tileShift=4, flags=pkg.NOISE_WRITE_SUM, reserved=(0, 0))
        d.update(kw)
        return pkg.AdaptiveMeterDesc(d["pendingA"], d["pendingB"], d["normalizeTo"], d["exposure"], d["threshold"], d["tileShift"], d["flags"], (C.c_uint32 * 2)(*d["reserved"]))
    plan = lambda d: lib.ptx_adaptive_plan(r.handle, C.byref(d), C.byref(out))
    meter = lambda d: lib.ptx_noise_meter_adaptive(r.handle, C.byref(d))
    for kw in (dict(tileShift=2), dict(tileShift=7), dict(source=2), dict(flags=1), dict(reserved=(1, 0)), dict(reserved=(0, 1)), dict(dilate=3), dict(framesA=2 ** 24 + 1),
               dict(framesB=2 ** 24 + 1), dict(mask=None)):
        assert plan(desc(**kw)) == INVALID, kw
        intact(kw)
    assert lib.ptx_adaptive_plan(None, C.byref(desc()), C.byref(out)) == INVALID and lib.ptx_adaptive_plan(r.handle, None, C.byref(out)) == INVALID
    assert lib.ptx_adaptive_plan(r.handle, C.byref(desc()), None) == INVALID and lib.ptx_adaptive_clear(None) == INVALID
    intact("null")
    for kw in (dict(pendingA=2 ** 24 + 1), dict(pendingB=2 ** 24 + 1), dict(normalizeTo=0), dict(normalizeTo=2 ** 25 + 1), dict(exposure=np.nan), dict(exposure=np.inf),
               dict(exposure=0.0), dict(exposure=-1.0), dict(threshold=np.nan), dict(threshold=np.inf), dict(threshold=-0.5), dict(tileShift=2), dict(tileShift=7),
               dict(flags=2), dict(flags=5), dict(reserved=(1, 0)), dict(reserved=(0, 1))):
        assert meter(mdesc(**kw)) == INVALID, kw
        intact(kw)
    assert lib.ptx_noise_meter_adaptive(None, C.byref(mdesc())) == INVALID and lib.ptx_noise_meter_adaptive(r.handle, None) == INVALID
    intact("meter null")
    # a tile size that differs from the counts' own, while they are not zero; FROM_NOISE after a meter of another tile size
    small = np.ones(54, np.uint8)  # the 9 x 6 tiles of tileShift 3
    assert plan(desc(tileShift=3, mask=small.ctypes.data)) == NOT_READY and b"not all zero" in lib.ptx_last_error(r.handle)
    intact("plan tileShift")
    assert meter(mdesc(tileShift=5)) == NOT_READY and b"counts are of tileShift 4" in lib.ptx_last_error(r.handle)
    intact("meter tileShift")
    assert plan(desc(tileShift=5, source=pkg.ADAPTIVE_FROM_NOISE, mask=None)) == NOT_READY and b"accepted meter call" in lib.ptx_last_error(r.handle)
    intact("noise tileShift")
    for wrong in (np.ones(tx * ty - 1, np.uint8), np.ones((ty + 1, tx)), np.ones(0)):  # the wrapper: never a copy from a smaller array
        with pytest.raises(pkg.PtxError):
            r.adaptive_plan(4, mask=wrong, dilate=0)
    intact("mask size")
    # ptx_read_adaptive
    tiles, counts = np.zeros_like(state[0][1]), np.zeros_like(state[0][2])
    assert lib.ptx_read_adaptive(None, C.byref(out), None, 0, None, 0) == INVALID and lib.ptx_read_adaptive(r.handle, None, None, 0, None, 0) == INVALID
    for nbytes in (0, tiles.nbytes - 4, tiles.nbytes + 4):
        assert lib.ptx_read_adaptive(r.handle, C.byref(out), tiles.ctypes.data, nbytes, None, 0) == INVALID
    for nbytes in (0, counts.nbytes - 4, counts.nbytes + 4):
        assert lib.ptx_read_adaptive(r.handle, C.byref(out), None, 0, counts.ctypes.data, nbytes) == INVALID
    assert not tiles.any() and not counts.any()
    intact("read")
    # NOT_READY, in ptx_noise_meter's order: a tile shard with world size > 1, a bound shard buffer; an invalid argument comes first
    r.set_tile_shard(0, 1, 32)  # no change: nothing is dropped
    intact("same shard")
    fresh = pkg.Renderer()  # no image
    assert lib.ptx_adaptive_plan(fresh.handle, C.byref(desc()), C.byref(out)) == NOT_READY and lib.ptx_noise_meter_adaptive(fresh.handle, C.byref(mdesc())) == NOT_READY
    assert lib.ptx_adaptive_plan(fresh.handle, C.byref(desc(dilate=9)), C.byref(out)) == INVALID
    assert lib.ptx_read_adaptive(fresh.handle, C.byref(out), None, 0, None, 0) == NOT_READY and lib.ptx_adaptive_clear(fresh.handle) == OK
    fresh.resize(W, H)
    # no halves, then no counts, then no accepted meter
    assert lib.ptx_noise_meter_adaptive(fresh.handle, C.byref(mdesc())) == NOT_READY and b"ptx_noise_halves" in lib.ptx_last_error(fresh.handle)
    fresh.noise_halves(True)
    assert lib.ptx_noise_meter_adaptive(fresh.handle, C.byref(mdesc())) == NOT_READY and b"ptx_adaptive_plan" in lib.ptx_last_error(fresh.handle)
    assert lib.ptx_adaptive_plan(fresh.handle, C.byref(desc(source=pkg.ADAPTIVE_FROM_NOISE, mask=None)), C.byref(out)) == NOT_READY
    assert lib.ptx_read_adaptive(fresh.handle, C.byref(out), None, 0, None, 0) == NOT_READY  # a refused call makes nothing
    # a sharded frame and a bound shard buffer
    fresh.set_tile_shard(0, 2, 8)
    assert lib.ptx_adaptive_plan(fresh.handle, C.byref(desc()), C.byref(out)) == NOT_READY and b"one tile shard of" in lib.ptx_last_error(fresh.handle)
    assert lib.ptx_adaptive_plan(fresh.handle, C.byref(desc(tileShift=9)), C.byref(out)) == INVALID
    shard = torch.zeros(fresh.shard_bytes(0) // 4, dtype=torch.float32, device="cuda")
    lib.ptx_bind_shard_accumulation(fresh.handle, shard.data_ptr(), shard.numel() * 4)
    assert lib.ptx_adaptive_plan(fresh.handle, C.byref(desc()), C.byref(out)) == NOT_READY and b"shard buffer" in lib.ptx_last_error(fresh.handle)
    lib.ptx_bind_shard_accumulation(fresh.handle, None, 0)
    fresh.set_tile_shard(0, 1, 32)
    # with all counts zero and nothing to commit another tile size is accepted, and the largest arguments are
    assert lib.ptx_adaptive_plan(fresh.handle, C.byref(desc(framesA=0, framesB=0)), C.byref(out)) == OK and out.generation == 1
    assert lib.ptx_adaptive_plan(fresh.handle, C.byref(desc(tileShift=3, mask=small.ctypes.data, framesA=0, framesB=0)), C.byref(out)) == OK
    assert (out.tilesX, out.tilesY, out.activeTiles) == (9, 6, 54)
    assert lib.ptx_adaptive_plan(fresh.handle, C.byref(desc(tileShift=4, framesA=1, framesB=0)), C.byref(out)) == NOT_READY  # a plan in force and frames to commit
    assert lib.ptx_adaptive_plan(fresh.handle, C.byref(desc(tileShift=3, mask=small.ctypes.data, framesA=2 ** 24, framesB=2 ** 24, dilate=2)), C.byref(out)) == OK
    assert lib.ptx_noise_meter_adaptive(fresh.handle, C.byref(mdesc(tileShift=3, pendingA=2 ** 24, pendingB=2 ** 24, normalizeTo=2 ** 25))) == OK
    fresh.close()
    intact("another handle")
    r.close()


@pytest.mark.gpu
def test_the_loop_closes(pkg):
    """8 + 8 uniform frames of `default`, a meter at LOOP_THRESHOLD, a plan from its records, eight planned render calls: each reports
    exactly activePixels samples, and each half at every pixel is a fresh sum of exactly the frames that pixel took part in"""
    w, h = LOOP_EXTENT
    s, r = _gpu(pkg)
    r.resize(w, h)
    r.noise_halves(True)
    u = s.uniform(w, h, bounces=LOOP_DEPTH)
    for f in range(LOOP_WARMUP):
        _bind(r, f & 1)
        u.TotalSamples = f
        r.render(u, s.lights)
    half = LOOP_WARMUP // 2
    r.noise_meter(half, half, 1.0, LOOP_THRESHOLD, LOOP_SHIFT)
    res, E = r.read_noise(tile_errors=True)
    plan = r.adaptive_plan(LOOP_SHIFT, dilate=1, frames_a=half, frames_b=half)
    tiles = plan.tilesX * plan.tilesY
    print(f"{tiles - res.converged} of {tiles} tiles seeded, {plan.activeTiles} active with the margin, {plan.activePixels} of {w * h} pixels")
    assert plan.seedTiles == tiles - res.converged and 0 < plan.activeTiles < tiles
    ref = AR.Planner(w, h)
    want, ids = ref.plan(LOOP_SHIFT, ~(E <= f32(LOOP_THRESHOLD)), 1, half, half)
    _assert_plan(r, plan, want, ids, ref, "loop")
    for f in range(LOOP_WARMUP, LOOP_WARMUP + 8):
        _bind(r, f & 1)
        u.TotalSamples = f
        r.render(u, s.lights)
        st = r.stats()
        assert st.pathSamples - st.retries == plan.activePixels, f
    A, B = _read_halves(r)
    # the adaptive meter sees the counts: warm-up everywhere, four more per half on the plan's tiles
    r.noise_meter_adaptive(4, 4, LOOP_WARMUP + 8, 1.0, LOOP_THRESHOLD, LOOP_SHIFT)
    want, E2, p = AR.meter(A, B, ref.counts, ref.active, 4, 4, LOOP_WARMUP + 8, 1.0, LOOP_THRESHOLD, LOOP_SHIFT, calls=2)
    _assert_noise(r, want, E2, "loop meter")
    assert set(np.unique(p["NA"])) == {half, half + 4}
    r.adaptive_clear()
    r.noise_halves(False)
    inside = ref.pixel_mask()[..., None]
    for which, got in enumerate((A, B)):
        sums = []
        for last in (LOOP_WARMUP, LOOP_WARMUP + 8):
            r.reset()
            for f in range(which, last, 2):
                u.TotalSamples = f
                r.render(u, s.lights)
            sums.append(r.readback())
        assert (_bits(got) == _bits(np.where(inside, sums[1], sums[0]))).all(), which


def _driver_frames(pkg, tmp_path_factory, tmp_path, spp, noise, adaptive):
    """tests/test_motion.py's driver (examples/motion_frame.cpp, compiled once per session) with the noise and adaptive arguments given:
    two frames of animated_test, each presented at 100 x 37 too, the noise trailer and the adaptive one"""
    import subprocess

    import test_motion as TM

    exe = TM._motion_frame_driver(pkg, tmp_path_factory)
    dump = tmp_path / "frames.bin"
    subprocess.check_call([exe, "animated_test", str(W), str(H), str(spp), "4", "0.37", "0", str(dump), "0", "0", "0", "0", "0", "-", "0", str(noise), str(adaptive)])
    raw = np.fromfile(dump, np.uint8)
    images = 6 * W * H * 16
    screens = 2 * 100 * 37 * 4
    assert len(raw) == images + screens + 2 * 44 + 4 + 2 * 24
    frames = raw[:images].view(np.float32).reshape(2, 3, H, W, 4)
    screen = raw[images:images + screens].reshape(2, 37, 100, 4)
    trailer = raw[images + screens:]
    results = [pkg.NoiseResult.from_buffer_copy(trailer[44 * k:44 * k + 40].tobytes()) for k in range(2)]
    converged = [int(trailer[44 * k + 40:44 * k + 44].view(np.uint32)[0]) for k in range(2)]
    plans = [pkg.AdaptivePlan.from_buffer_copy(trailer[92 + 24 * k:92 + 24 * k + 24].tobytes()) for k in range(2)]
    return frames, screen, results, converged, int(trailer[88:92].view(np.uint32)[0]), plans


def _posed(s, r, frame, step=0.37):
    if frame:
        assert s.update(step)
    it, bn = s.animation_state()
    r.update_animation(it, bn if len(bn) else None)


@pytest.mark.gpu
def test_renderer_hip_with_adaptive_settings_on_is_the_same_calls_made_by_hand(pkg, tmp_path_factory, tmp_path):
    """RendererHip with NoiseSettings { Enabled, Threshold 0.05, CheckEvery 4, MinSamples 4 } and AdaptiveSettings { Enabled, Dilate 0 }
    (the driver's adaptive argument 1: a threshold and a margin at which the plans of this small frame are partial) over 16 render
    calls a frame: after calls 4, 8, 12 and 16 the halves are metered -- by ptx_noise_meter while the handle holds no counts, by
    ptx_noise_meter_adaptive with the pending samples afterwards -- and ptx_adaptive_plan(FROM_NOISE) commits the pending samples and plans
    the calls that follow; ReadAccumulationImage, SaveOutput and Present meter with PTX_NOISE_WRITE_SUM and normalizeTo 16.  Two frames,
    so eight checks, the second frame's first on counts ResetAccumulationImage zeroed.  Everything equals the same calls made by hand."""
    spp = 16
    frames, screen, results, converged, halves, plans = _driver_frames(pkg, tmp_path_factory, tmp_path, spp, 1, 1)
    assert halves == 1
    d = pkg.NOISE_DEFAULTS
    thr, shift, dilate = 0.05, d["tile_shift"], 0
    s = pkg.Scene("animated_test", 0.25)
    s.update(0.0)
    r = pkg.Renderer()
    r.upload(s)
    r.resize(W, H)
    counts = False
    partial = 0
    for frame in range(2):
        _posed(s, r, frame)
        r.noise_halves(True)  # ResetAccumulationImage: the halves and the counts are zeroed, the plan is cleared
        if counts:
            r.adaptive_clear()
        n, pending = [0, 0], [0, 0]
        traced = 0
        for f in range(spp):
            _bind(r, f & 1)
            r.render(s.uniform(W, H, bounces=4, sample_count=1, total_samples=f), s.lights)
            traced += r.stats().pathSamples
            n[f & 1] += 1
            pending[f & 1] += 1
            if (f + 1) % 4 == 0:
                if counts:
                    r.noise_meter_adaptive(pending[0], pending[1], n[0] + n[1], 1.0, thr, shift)
                else:
                    r.noise_meter(n[0], n[1], 1.0, thr, shift)
                plan = r.adaptive_plan(shift, dilate=dilate, frames_a=pending[0], frames_b=pending[1])
                if f + 1 < spp:  # render calls follow under this plan
                    partial += int(0 < plan.activeTiles < plan.tilesX * plan.tilesY)
                counts = True
                pending = [0, 0]
        res = r.read_noise()
        assert bytes(res) == bytes(results[frame]) and res.valid == 1, frame
        assert converged[frame] == int(res.converged == res.tilesX * res.tilesY)
        assert bytes(plan) == bytes(plans[frame]) and bytes(r.read_adaptive()[0]) == bytes(plans[frame]), frame
        print(f"frame {frame}: {res.converged} of {res.tilesX * res.tilesY} tiles converged, {plan.activeTiles} active; {traced} path samples of {spp * W * H}")
        assert traced < spp * W * H, frame  # fewer path samples than the uniform render's
        for k in range(3):  # ReadAccumulationImage, SaveOutput, Present
            r.noise_meter_adaptive(0, 0, spp, 1.0, thr, shift, write_sum=True)
            _bind(r, None)
            if k == 0:
                assert (_bits(frames[frame][0]) == _bits(r.readback())).all(), frame
            else:
                r.postprocess(spp, 1.0, 1.0, 1.0, pkg.TONE_MAPPING_SDR)
            if k == 1:
                assert (_bits(frames[frame][2]) == _bits(r.read_output(pkg.OUTPUT_RGBA32F))).all(), frame
            if k == 2:
                r.present(100, 37)
                assert (r.read_present() == screen[frame]).all(), frame
            _bind(r, 0)
    assert partial > 0  # pending samples went to some tiles and not to others
    r.close()


@pytest.mark.gpu
def test_renderer_hip_with_adaptive_settings_off_is_todays_noise_path(pkg, tmp_path_factory, tmp_path):
    """The same driver with the adaptive argument given as 0: the noise path of tests/test_noise_meter.py by hand, and the handle holds
    no counts at the end; with the noise argument 0 as well AdaptiveSettings alone do nothing"""
    spp = 8
    frames, screen, results, converged, halves, plans = _driver_frames(pkg, tmp_path_factory, tmp_path, spp, 1, 0)
    assert halves == 1 and all(bytes(p) == bytes(24) for p in plans)
    d = pkg.NOISE_DEFAULTS
    s = pkg.Scene("animated_test", 0.25)
    s.update(0.0)
    r = pkg.Renderer()
    r.upload(s)
    r.resize(W, H)
    for frame in range(2):
        _posed(s, r, frame)
        r.noise_halves(True)
        for f in range(spp):
            _bind(r, f & 1)
            r.render(s.uniform(W, H, bounces=4, sample_count=1, total_samples=f), s.lights)
            if (f + 1) % 4 == 0:
                r.noise_meter((f + 1) // 2, (f + 1) // 2, 1.0, d["threshold"], d["tile_shift"])
        res = r.read_noise()
        assert bytes(res) == bytes(results[frame]), frame
        for k in range(2):  # ReadAccumulationImage, SaveOutput
            r.noise_meter(spp // 2, spp // 2, 1.0, d["threshold"], d["tile_shift"], write_sum=True)
            _bind(r, None)
            if k == 0:
                assert (_bits(frames[frame][0]) == _bits(r.readback())).all(), frame
            else:
                r.postprocess(spp, 1.0, 1.0, 1.0, pkg.TONE_MAPPING_SDR)
                assert (_bits(frames[frame][2]) == _bits(r.read_output(pkg.OUTPUT_RGBA32F))).all(), frame
            _bind(r, 0)
        r.noise_meter(spp // 2, spp // 2, 1.0, d["threshold"], d["tile_shift"], write_sum=True)  # Present's
    r.close()
    frames, screen, results, converged, halves, plans = _driver_frames(pkg, tmp_path_factory, tmp_path, 2, 0, 1)
    assert halves == 0 and all(bytes(p) == bytes(24) for p in plans) and all(bytes(x) == bytes(40) for x in results)
