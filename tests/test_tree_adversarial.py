"""The tree build (pt_bvh_build.hpp) and the traversal (pt_bvh.hpp) on geometry chosen to reach the branches friendly scenes
do not: leaf and tile counts at the sort / scan block boundaries (up to 16,384 references a radix pass scans its 256 counters per
2,048-reference tile in one block; from 16,385 on -- more than 8 tiles -- in three kernels: sizes 16,383 - 16,385, and 18,433 = nine
tiles and one reference), zero-area triangles, exact duplicates and shared centroids
(PLOC ties, equal-t ties that must go to the smallest id), coplanar overlaps far from the ray origin (the case the traversal's
cull slack is for -- with today's box padding these scenes do not need it: they also pass with a slack of 1.0), scenes scaled by powers of two and moved far from the origin, flat scenes, slivers, a tiny cluster inside a huge box, and
nested triangles deep enough to spill the traversal stack into its global region or past it.

Every scene is generated here by seeded numpy.  The reference for every closest hit is the oracle's brute force (no tree),
compared bit for bit; the CPU tests check the oracle's own tree and the exactness of power-of-two scaling, the GPU tests
the HIP tree under every builder switch, after a refit, in rendered images, and the stack depth the walks reach.

Not covered on purpose: nearly degenerate triangles (edge cross product a rounding residue, area ~1e-8, e.g. three vertices
made "collinear" by float32 arithmetic).  They are live, but the triangle test accepts points far outside their boxes, so
brute force reports hits that no tree walk reaches (seen on the oracle's tree: 14 of 4,800 rays).  The zero-area scenes
here are built exactly collinear or with a repeated vertex."""
import numpy as np
import pytest

import util

DEEP_RATIO, DEEP_STEP = 0.93, 1e-4
SIZES = (1, 2, 3, 4, 5, 17, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 4097, 16383, 16384, 16385,
         18433)
SCALE_EXPONENTS = (-40, -20, 20, 40)
EXACT_EXPONENTS = (-20, 20, 40)  # at 2^-40 cancelling products of the triangle test leave the normal range (measured on the oracle)


# ---------------------------------------------------------------------------------------
# scenes: (models, instances or None, ray box lo, hi); models = list of models = lists of (n, 3, 3) meshes
# ---------------------------------------------------------------------------------------
def _random_tris(rng, n, lo=-4.0, hi=4.0, size=(0.2, 0.8)):
    c = rng.uniform(lo, hi, (n, 1, 3))
    e = rng.normal(size=(n, 3, 3))
    e /= np.linalg.norm(e, axis=2, keepdims=True)
    return (c + e * rng.uniform(*size, (n, 1, 1))).astype(np.float32)


def _degenerate(tris, every):
    """Every `every`-th triangle made zero-area, alternately by a repeated vertex and by three collinear vertices (on a line
    along x, so that the edge cross product vanishes exactly in float32)."""
    t = tris.copy()
    for j, i in enumerate(range(0, len(t), every)):
        if j % 2:
            t[i, 2] = t[i, 0]
        else:
            t[i, 1:3] = t[i, 0]
            t[i, 1, 0] += np.float32(0.5)
            t[i, 2, 0] += np.float32(0.25)
    return t


def _translate(x):
    m = util.IDENTITY_3X4.copy()
    m[[3, 7, 11]] = x
    return m


def _nested(n):
    """Triangles nested towards the shared corner at the origin: T_k has legs DEEP_RATIO^k along x and y and sits at
    z = k DEEP_STEP, so each smaller one lies a little nearer to a ray coming down the z axis.  A closest-hit walk down to the
    corner enters the cluster of the smaller ones first and keeps the larger siblings on its stack: about one entry per
    triangle."""
    s = DEEP_RATIO ** np.arange(n)
    z = np.arange(n) * DEEP_STEP
    t = np.zeros((n, 3, 3))
    t[:, :, 2] = z[:, None]
    t[:, 1, 0] = s
    t[:, 2, 1] = s
    return t.astype(np.float32)


def _fan(n, r=1.0):
    """n triangles turned about one shared centroid in the plane z = 0, all overlapping, every box nearly the same.  The
    float32 centroids differ only by rounding (~1e-8); k_morton quantises over the bounds of the centroids themselves, so
    it spreads those residues over the whole curve: the codes are distinct but carry no spatial order.  (Identical Morton
    codes come from dup512, whose boxes are bit-identical.)"""
    a = np.arange(n) * (2 * np.pi / 3 / n)
    t = np.zeros((n, 3, 3))
    for k in range(3):
        t[:, k, 0] = r * np.cos(a + k * 2 * np.pi / 3)
        t[:, k, 1] = r * np.sin(a + k * 2 * np.pi / 3)
    return t.astype(np.float32)


def _quad(x0, y0, x1, y1, z):
    return np.float32([[[x0, y0, z], [x1, y0, z], [x1, y1, z]], [[x1, y1, z], [x0, y1, z], [x0, y0, z]]])


DUP_TRIANGLE = np.float32([[[-1, -1, 0], [1, -1, 0.2], [0, 1, -0.1]]])


def make_scene(name):
    rng = np.random.default_rng(sum(map(ord, name)))
    if name.startswith("sizes_"):
        n = int(name.split("_")[1])
        return [[_random_tris(rng, n)]], None, -5.0, 5.0
    if name == "inert_third":
        return [[_degenerate(_random_tris(rng, 257), 3)]], None, -5.0, 5.0
    if name == "inert_all":
        return [[_degenerate(_random_tris(rng, 100), 1)]], None, -5.0, 5.0
    if name == "inert_one_live":
        t = _degenerate(_random_tris(rng, 101), 1)
        t[50] = np.float32([[-1, -1, 0.5], [1, -1, 0.5], [0, 1, 0.5]])
        return [[t]], None, -5.0, 5.0
    if name.startswith("dup"):
        # exact duplicates of one triangle across two meshes and two instances
        one = np.repeat(DUP_TRIANGLE, int(name[3:]) // 4, axis=0)
        return [[one, one]], [(0, util.IDENTITY_3X4), (0, util.IDENTITY_3X4)], -3.0, 3.0
    if name == "fan512":
        return [[_fan(512)]], None, -2.0, 2.0
    if name == "coplanar_far":
        # overlapping coplanar quads in three instances of three models, at 100-1000 units from every ray origin (box -8..8)
        quads = [_quad(-300, -300, 300, 300, 0), _quad(-290.5, -310, 310, 290.25, 0), _quad(-200, -200, 250, 250, 0)]
        inst = [(k, _translate((0.0, 0.0, 400.0))) for k in range(3)] + [(0, _translate((0.0, 0.0, -150.0))),
                                                                        (2, _translate((0.0, 0.0, -150.0)))]
        return [[q] for q in quads], inst, -8.0, 8.0
    if name == "coplanar_near":
        quads = [_quad(-2, -2, 2, 2, 0), _quad(-1.5, -2.5, 2.5, 1.5, 0), _quad(-1, -1, 1, 1, 0)]
        return [[q] for q in quads], [(k, util.IDENTITY_3X4) for k in range(3)] + [(1, util.IDENTITY_3X4)], -3.0, 3.0
    if name == "flat":
        t = _random_tris(rng, 1500)
        t[:, :, 2] = 0.0
        return [[t]], None, -5.0, 5.0
    if name == "slivers":
        c = rng.uniform(-4, 4, (1500, 1, 3))
        a = rng.normal(size=(1500, 3))
        a /= np.linalg.norm(a, axis=1, keepdims=True)
        b = np.cross(a, rng.normal(size=(1500, 3)))
        b /= np.linalg.norm(b, axis=1, keepdims=True)
        t = np.stack([c[:, 0], c[:, 0] + 10 * a, c[:, 0] + 5 * a + 1e-4 * b], axis=1)
        return [[t.astype(np.float32)]], None, -6.0, 6.0
    if name == "tiny_in_huge":
        big = np.float32([[[-1e4, -1e4, 0], [1e4, -1e4, 0], [0, 1e4, 3e3]]])
        small = _random_tris(rng, 2000, -2.0, 2.0, size=(5e-4, 1e-3))
        return [[big, small]], None, -2.5, 2.5
    if name == "deep_spill":
        return [[_nested(40)]], None, 0.0, 0.5
    if name == "deep_160":
        return [[_nested(160)]], None, 0.0, 0.5
    raise KeyError(name)


SCENES = ([f"sizes_{n}" for n in SIZES] + ["inert_third", "inert_all", "inert_one_live", "dup512", "fan512", "coplanar_far",
                                           "coplanar_near", "flat", "slivers", "tiny_in_huge", "deep_spill", "deep_160"])
VARIANT_SCENES = ["dup512", "fan512", "coplanar_far", "coplanar_near", "flat", "slivers", "tiny_in_huge", "deep_spill"]


def soup(pkg, name, scale=1.0, offset=0.0):
    models, inst, lo, hi = make_scene(name)
    models = [[(m * np.float32(scale) + np.float32(offset)).astype(np.float32) for m in model] for model in models]
    if inst is not None and scale != 1.0:
        inst = [(k, np.float32(x) * np.float32([1, 1, 1, scale] * 3)) for k, x in inst]
    return util.TriangleSoup(pkg, models, inst), lo, hi


def live_mask(T):
    """Triangles whose float32 edge cross product does not vanish: what the builder keeps in the tree (k_tri_setup)."""
    w = np.float32(T)
    return (np.cross(w[:, 1] - w[:, 0], w[:, 2] - w[:, 0]) != 0).any(axis=1)


def live_count(T):
    return int(live_mask(T).sum())


# ---------------------------------------------------------------------------------------
# rays
# ---------------------------------------------------------------------------------------
def _aimed(o, target, tmin=1e-5, tmax=1e4):
    d = np.float64(target) - np.float64(o)
    n = np.linalg.norm(d, axis=1, keepdims=True)
    ok = n[:, 0] > 0
    rays = np.zeros((int(ok.sum()), 8), np.float32)
    rays[:, 0:3] = o[ok]
    rays[:, 3] = tmin
    rays[:, 4:7] = d[ok] / n[ok]
    rays[:, 7] = tmax
    return rays


def scene_rays(name, T, lo, hi, n_random=3000, seed=5):
    """Random rays from the scene's box plus rays aimed at centroids, vertices and edge midpoints, axis-parallel rays through
    vertex planes, directions with signed zeros and subnormals, and the targeted rays of the deep scenes."""
    rng = np.random.default_rng(seed)
    parts = [util.random_rays(rng, n_random, lo, hi)]
    live = np.flatnonzero(live_mask(T))
    if len(T):
        pick = rng.choice(len(T), size=min(len(T), 400), replace=False)
        P = T[pick]
        targets = np.concatenate([P.mean(axis=1), P[:, 0], P[:, 1], P[:, 2], 0.5 * (P[:, 0] + P[:, 1]), 0.5 * (P[:, 1] + P[:, 2])])
        o = rng.uniform(lo, hi, (len(targets), 3))
        parts.append(_aimed(o, targets))
        # axis-parallel rays whose origin lies exactly in a vertex plane: along z through (vx, vy), along x through (vy, vz)
        v = np.float32(P[:, 0])
        m = len(v)
        ax = np.zeros((2 * m, 8), np.float32)
        ax[:m, 0:2], ax[:m, 2], ax[:m, 6] = v[:, 0:2], v[:, 2] + 3.0, -1.0
        ax[m:, 1:3], ax[m:, 0], ax[m:, 4] = v[:, 1:3], v[:, 0] - 3.0, 1.0
        ax[:, 3], ax[:, 7] = 1e-5, 1e4
        parts.append(ax)
        # signed zeros and subnormals in the direction
        c = np.float32(P.mean(axis=1))
        odd = np.zeros((4 * m, 8), np.float32)
        sub = np.float32(1e-40)
        dirs = np.float32([[0.0, -0.0, -1.0], [-0.0, 0.0, 1.0], [sub, -sub, -1.0], [-sub, 0.0, 1.0]])
        for k in range(4):
            odd[k * m:(k + 1) * m, 0:3] = c - dirs[k] * np.float32(3.0)
            odd[k * m:(k + 1) * m, 4:7] = dirs[k]
        odd[:, 3], odd[:, 7] = 1e-5, 1e4
        parts.append(odd)
    if name.startswith("deep"):
        parts.append(deep_rays(T, 500, rng))
    rays = np.concatenate(parts)
    return rays, len(live)


def deep_rays(T, n, rng):
    """Rays from above straight down (and slightly tilted) through the smallest triangle of a nested scene: they hit them all."""
    s = float(T[-1, 1, 0])
    rays = np.zeros((n, 8), np.float32)
    rays[:, 0:2] = rng.uniform(0.05 * s, 0.3 * s, (n, 2))
    rays[:, 2] = 1.0
    rays[:, 3], rays[:, 7] = 1e-5, 1e4
    rays[:, 6] = -1.0
    rays[n // 2:, 4:6] = rng.uniform(-0.05, 0.05, (n - n // 2, 2)) * s
    rays[:, 4:7] /= np.linalg.norm(rays[:, 4:7], axis=1, keepdims=True)
    return rays


def interval_rays(rays, want):
    """For rays with a hit at t: tmax = t (excluded: tmin < t < tmax is strict), tmax = nextafter(t, +inf), tmin = t and
    tmin = nextafter(t, -inf)."""
    h = np.flatnonzero(want["tri"] != 0xFFFFFFFF)[:300]
    t = want["t"][h].astype(np.float32)
    out = np.repeat(rays[h][None], 4, axis=0)
    out[0, :, 7] = t
    out[1, :, 7] = np.nextafter(t, np.float32(np.inf))
    out[2, :, 3] = t
    out[3, :, 3] = np.nextafter(t, np.float32(-np.inf))
    out[3, :, 7] = np.maximum(out[3, :, 7], np.nextafter(t, np.float32(np.inf)))
    return out.reshape(-1, 8)


def all_rays(orc, name, desc):
    T = util.world_triangles(desc)
    _, _, lo, hi = make_scene(name)
    rays, nlive = scene_rays(name, T, lo, hi)
    osc = orc.OracleScene(desc, build_bvh=False)
    want = osc.trace_closest(rays, brute_force=True)
    osc.close()
    rays = np.concatenate([rays, interval_rays(rays, want)])
    min_hits = 0 if nlive == 0 else min(200, nlive)
    return rays, min_hits, nlive


# ---------------------------------------------------------------------------------------
# CPU: the scenes themselves, the oracle's tree, exact scaling
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCENES)
def test_oracle_tree_matches_bruteforce(pkg, orc, name):
    """The oracle's binned-SAH tree (what the image parity tests render with) against its own brute force, bit for bit."""
    s, _, _ = soup(pkg, name)
    rays, min_hits, nlive = all_rays(orc, name, s.desc)
    osc = orc.OracleScene(s.desc, build_bvh=True)
    got, got_any = osc.trace_closest(rays), osc.trace_any(rays)
    osc.close()
    ref = orc.OracleScene(s.desc, build_bvh=False)
    want, want_any = ref.trace_closest(rays, brute_force=True), ref.trace_any(rays, brute_force=True)
    ref.close()
    assert (got["tri"] == want["tri"]).all(), int((got["tri"] != want["tri"]).sum())
    for f in ("t", "u", "v"):
        assert (got[f].view(np.uint32) == want[f].view(np.uint32)).all(), f
    assert ((got_any != 0) == (want_any != 0)).all()
    assert int((want["tri"] != 0xFFFFFFFF).sum()) >= min_hits
    if nlive == 0:
        assert (want["tri"] == 0xFFFFFFFF).all()


def test_duplicates_tie_to_the_smallest_id(pkg, orc):
    """512 copies of one triangle: every hit is the first copy (global id 0), whatever the direction."""
    s, lo, hi = soup(pkg, "dup512")
    rays, _, _ = all_rays(orc, "dup512", s.desc)
    osc = orc.OracleScene(s.desc, build_bvh=False)
    want = osc.trace_closest(rays, brute_force=True)
    osc.close()
    h = want["tri"] != 0xFFFFFFFF
    assert h.sum() > 500 and (want["tri"][h] == 0).all()


def scaling_rays(T, lo, hi):
    """Random rays and rays aimed at centroids.  Rays aimed exactly at vertices and edges, or with subnormal direction
    components, are left out: their cancelling products fall below the normal range at 2^-40 (measured: 50 of 9,000 rays of
    the full set change their triangle there), where scaling is no longer exact."""
    rng = np.random.default_rng(6)
    pick = rng.choice(len(T), size=400, replace=False)
    return np.concatenate([util.random_rays(rng, 3000, lo, hi), _aimed(rng.uniform(lo, hi, (400, 3)), T[pick].mean(axis=1))])


@pytest.mark.parametrize("k", EXACT_EXPONENTS)
def test_power_of_two_scaling_is_exact_on_the_oracle(pkg, orc, k):
    """The triangle test is exact under scaling by 2^k (while no product leaves the normal range): the scene, the ray
    origins, tmin and tmax scaled by 2^k give the same triangles, the same u and v bits and t scaled by exactly 2^k."""
    base, lo, hi = soup(pkg, "sizes_1025")
    rays = scaling_rays(util.world_triangles(base.desc), lo, hi)
    osc = orc.OracleScene(base.desc, build_bvh=False)
    want = osc.trace_closest(rays, brute_force=True)
    osc.close()
    f = np.float32(2.0 ** k)
    s, _, _ = soup(pkg, "sizes_1025", scale=f)
    sr = rays.copy()
    sr[:, [0, 1, 2, 3, 7]] *= f
    for bvh in (False, True):
        osc = orc.OracleScene(s.desc, build_bvh=bvh)
        got = osc.trace_closest(sr, brute_force=not bvh)
        osc.close()
        assert (got["tri"] == want["tri"]).all(), int((got["tri"] != want["tri"]).sum())
        h = want["tri"] != 0xFFFFFFFF
        assert h.sum() > 1000
        for fld in ("u", "v"):
            assert (got[fld][h].view(np.uint32) == want[fld][h].view(np.uint32)).all(), fld
        assert (got["t"][h] == want["t"][h] * f).all()


@pytest.mark.parametrize("offset", [1e3, 1e5])
def test_translated_scene_against_float64(pkg, orc, offset):
    """The random scene moved 1e3 and 1e5 units from the origin (in the vertices: float32 world space), rays moved with it:
    the oracle's brute force against the float64 Moeller-Trumbore within the tolerances of test_analytic's check."""
    s, lo, hi = soup(pkg, "sizes_1025", offset=offset)
    T = util.world_triangles(s.desc)
    rays = util.random_rays(np.random.default_rng(8), 2000, lo + offset, hi + offset)
    osc = orc.OracleScene(s.desc, build_bvh=False)
    got = osc.trace_closest(rays, brute_force=True)
    osc.close()
    # The second pass of the triangle test starts from o + t1 d rounded to the coordinates' ulp (6e-5 at 1e3, 8e-3 at 1e5):
    # t is good to a few of those ulps (measured 1.3e-4 at t = 4.6, offset 1e3), the barycentrics to that over the edge.
    # At 1e3 the bounds stay tight (t within 5e-4, u / v within 3e-3).  At 1e5 an ulp is 1 - 4 % of these triangles' edges, so
    # the barycentric bounds widen to ~0.3 and say little there: what 1e5 checks is the hit / miss rule, the same nearest
    # triangle on 98 % of the hits and t within 8 ulps.
    ulp = float(np.spacing(np.float32(offset + hi)))
    hits, agree, close = util.check_closest_against_float64(T, rays, got, t_slack=8 * ulp, bary_slack=8 * ulp / 0.2)
    assert hits > 300 and agree > 0.98 * hits, (hits, agree, close)


def test_scene_recipes(pkg):
    """The deep scenes are what their names claim: nested, every triangle containing the corner rays' footprint."""
    def tris(name):
        s = soup(pkg, name)[0]
        return util.world_triangles(s.desc)

    for name, n in (("deep_spill", 40), ("deep_160", 160)):
        T = tris(name)
        assert len(T) == n and live_count(T) == n
        assert (np.diff(T[:, 1, 0]) < 0).all() and (np.diff(T[:, 0, 2]) > 0).all()
    assert live_count(tris("inert_third")) == 257 - 86
    assert live_count(tris("inert_all")) == 0
    assert live_count(tris("inert_one_live")) == 1
    fan = tris("fan512")
    c = fan.mean(axis=1)
    assert np.abs(c).max() < 1e-6                               # one centroid up to rounding
    dup = tris("dup512")
    assert len(dup) == 512 and (dup == dup[0]).all()            # bit-identical boxes, hence identical Morton codes


# ---------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------
def _renderer(pkg, desc):
    r = pkg.Renderer()
    r.upload(desc)
    err = r.lib.ptx_last_error(r.handle).decode()
    assert "reinsertion" not in err, err
    return r


def _check_scene(pkg, orc, name, label=""):
    s, _, _ = soup(pkg, name)
    rays, min_hits, nlive = all_rays(orc, name, s.desc)
    r = _renderer(pkg, s.desc)
    try:
        assert r.stats().treeTriangles == nlive
        util.check_trace_against_bruteforce(r, orc, s.desc, rays, min_hits, label=f"{name} {label}")
    finally:
        r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", SCENES)
def test_tree_matches_bruteforce(pkg, orc, name):
    import torch  # noqa: F401

    _check_scene(pkg, orc, name)


VARIANTS = [{"PTX_BUILDER": "lbvh"}, {"PTX_REINSERT": "0"}, {"PTX_COLLAPSE": "0"}, {"PTX_SPLIT_BUDGET": "0.5"}, {"PTX_NODE_LAYOUT": "1"},
            {"PTX_PLOC_RADIUS": "1"}]


@pytest.mark.gpu
@pytest.mark.parametrize("env", VARIANTS, ids=lambda e: ",".join(f"{k}={v}" for k, v in e.items()))
def test_builder_variants_match_bruteforce(pkg, orc, monkeypatch, env):
    import torch  # noqa: F401

    for k, v in env.items():
        monkeypatch.setenv(k, v)
    for name in VARIANT_SCENES:
        _check_scene(pkg, orc, name, label=str(env))


@pytest.mark.gpu
@pytest.mark.parametrize("k", SCALE_EXPONENTS)
def test_scaled_scene_matches_unscaled_on_the_gpu(pkg, orc, k):
    """The tree over the scene scaled by 2^k (boxes padded by an absolute floor at 2^-40, quantised with power-of-two scales
    at 2^40) returns the oracle's brute force, and where scaling is exact the unscaled hits: same ids, same u and v bits,
    t times 2^k."""
    import torch  # noqa: F401

    base, lo, hi = soup(pkg, "sizes_1025")
    rays, min_hits = scaling_rays(util.world_triangles(base.desc), lo, hi), 1000
    r = _renderer(pkg, base.desc)
    h0, i0 = r.trace_rays(rays)
    r.close()
    f = np.float32(2.0 ** k)
    s, _, _ = soup(pkg, "sizes_1025", scale=f)
    sr = rays.copy()
    sr[:, [0, 1, 2, 3, 7]] *= f
    r = _renderer(pkg, s.desc)
    try:
        util.check_trace_against_bruteforce(r, orc, s.desc, sr, min_hits, label=f"2^{k}")
        h1, i1 = r.trace_rays(sr)
    finally:
        r.close()
    if k not in EXACT_EXPONENTS:
        return
    assert (i1 == i0).all()
    hit = i0[:, 0] != 0xFFFFFFFF
    assert (h1[hit, 1:3].view(np.uint32) == h0[hit, 1:3].view(np.uint32)).all()
    assert (h1[hit, 0] == h0[hit, 0] * f).all()


@pytest.mark.gpu
@pytest.mark.parametrize("offset", [1e3, 1e5])
def test_translated_scene_matches_bruteforce(pkg, orc, offset):
    import torch  # noqa: F401

    s, lo, hi = soup(pkg, "sizes_1025", offset=offset)
    rays, min_hits, _ = all_rays(orc, "sizes_1025", s.desc)
    rays[:, 0:3] += np.float32(offset)  # the box of all_rays is the untranslated one
    r = _renderer(pkg, s.desc)
    try:
        util.check_trace_against_bruteforce(r, orc, s.desc, rays, 300, label=f"+{offset}")
    finally:
        r.close()


@pytest.mark.gpu
def test_refit_matches_rebuild_and_bruteforce(pkg, orc):
    """Two instances (the duplicates' model and the flat model) refitted after their transforms are swapped, one scaled by
    2^-20 and one moved by 1e4: the refitted tree, a rebuilt tree and the oracle's brute force of that pose agree."""
    import torch  # noqa: F401

    dup = make_scene("dup512")[0][0][0]
    flat = make_scene("flat")[0][0][0]
    a = _translate((3.0, 0.0, 0.0))
    b = _translate((-3.0, 1.0, 0.0))
    s = util.TriangleSoup(pkg, [[dup], [flat]], [(0, a), (1, b)])
    r = _renderer(pkg, s.desc)
    rng = np.random.default_rng(17)
    try:
        util.check_trace_against_bruteforce(r, orc, s.desc, util.random_rays(rng, 3000, -6.0, 6.0), 200, label="initial")
        small = b.copy()
        small[[0, 1, 2, 4, 5, 6, 8, 9, 10]] *= np.float32(2.0 ** -20)
        far = a.copy()
        far[[3, 7, 11]] += np.float32(1e4)
        for pose in (np.stack([b, a]), np.stack([small, far]), np.stack([far, small])):
            r.update_animation(pose, rebuild=False)
            # rays at both instances: random from each one's box, and aimed at the world-space centroids
            T = util.world_triangles(s.desc, instance_transforms=pose)
            c = T.mean(axis=1)
            away = rng.normal(size=c.shape)
            away /= np.linalg.norm(away, axis=1, keepdims=True)
            # at least 0.05 away: the scaled instance's triangles are 1e-6 across, and tmin is 1e-5
            o = c + away * np.maximum(np.abs(T - c[:, None]).max(axis=(1, 2)) * 4, 0.05)[:, None]
            rays = np.concatenate([_aimed(o, c), util.random_rays(rng, 1000, pose[0][[3, 7, 11]] - 6, pose[0][[3, 7, 11]] + 6),
                                   util.random_rays(rng, 1000, pose[1][[3, 7, 11]] - 6, pose[1][[3, 7, 11]] + 6)])
            util.check_trace_against_bruteforce(r, orc, s.desc, rays, 500, instance_transforms=pose, label="refit")
            h_refit, i_refit = r.trace_rays(rays)
            r.update_animation(pose, rebuild=True)
            h_re, i_re = r.trace_rays(rays)
            assert (i_refit == i_re).all() and (h_refit.view(np.uint32) == h_re.view(np.uint32)).all()
    finally:
        r.close()


def _render_scene(pkg, orc, desc, pos, look, backend, W=48, H=32, depth=4, frames=2):
    cam = pkg.Scene("default")
    cam.set_camera_pose(np.float32(pos), np.float32(look))
    lights = cam.lights
    r = pkg.Renderer(backend=backend)
    r.upload(desc)
    r.resize(W, H)
    osc = orc.OracleScene(desc, build_bvh=True)
    ref = np.zeros((H, W, 4), np.float32)
    try:
        for f in range(frames):
            u = cam.uniform(W, H, bounces=depth, sample_count=1, total_samples=f)
            r.render(u, lights)
            st = r.stats()
            _, ost = osc.render(u, lights, W, H, accum=ref)
            assert (st.segments, st.shadowRays) == (ost.segments, ost.shadowRays), "segment counts differ"
        img = r.readback()
    finally:
        r.close()
        osc.close()
    return img, ref


@pytest.mark.gpu
@pytest.mark.parametrize("backend", [0, 1])
@pytest.mark.parametrize("name,pos,look", [("coplanar_near", (0.3, -0.2, 3.0), (0.0, 0.1, -1.0)),
                                           ("dup512", (0.1, 0.0, 3.0), (0.0, -0.1, -1.0)),
                                           ("deep_spill", (0.06, 0.05, 0.25), (-0.1, -0.1, -1.0))])
def test_images_match_oracle(pkg, orc, name, pos, look, backend):
    """The render kernels' stacks (closest, shadow, tail; the megakernel's) on coplanar ties, on 512 duplicates and on a tree
    that spills."""
    import torch  # noqa: F401

    s, _, _ = soup(pkg, name)
    img, ref = _render_scene(pkg, orc, s.desc, pos, look, backend)
    assert np.isfinite(img).all() and (img[..., :3] != 0).any()
    assert (img.view(np.uint32) == ref.view(np.uint32)).all(), int((img.view(np.uint32) != ref.view(np.uint32)).any(axis=-1).sum())


def _deepest(pkg, desc, rays):
    r = _renderer(pkg, desc)
    try:
        hits, ids = r.trace_rays(rays, 3)  # diagnostic mode 3: (deepest stack position, node visits)
    finally:
        r.close()
    return hits, ids


def _dup_rays(lo, hi, n=500):
    rng = np.random.default_rng(2)
    return _aimed(rng.uniform(lo, hi, (n, 3)), np.repeat(np.float64(DUP_TRIANGLE[0].mean(axis=0))[None], n, axis=0))


@pytest.mark.gpu
@pytest.mark.parametrize("name,low,high", [("deep_spill", 17, 64), ("deep_160", 17, 96), ("dup512", 1, 64)])
def test_walks_reach_the_expected_stack_depth(pkg, orc, name, low, high):
    """The deepest stack position (ptx_trace_rays mode 3) of rays through the nested scenes and the duplicates.  deep_spill
    goes past the 16 LDS entries into the global region and stays within the megakernel's 64; deep_160 needs the global
    region and stays within the 96 of the wavefront kernels (the builder keeps it shallower than one entry per triangle:
    54 measured).  512 duplicates are a balanced subtree: a chain -- one PLOC merge per iteration -- would need 511."""
    import torch  # noqa: F401

    s, lo, hi = soup(pkg, name)
    rays = _dup_rays(lo, hi) if name.startswith("dup") else deep_rays(util.world_triangles(s.desc), 500, np.random.default_rng(2))
    hits, ids = _deepest(pkg, s.desc, rays)
    depth = int(ids[:, 0].max())
    print(f"{name}: deepest stack position {depth}")
    assert low <= depth <= high, depth
    assert (hits[:, 3] == 1).all()
