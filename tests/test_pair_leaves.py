"""Pair leaves (pt_bvh_build.hpp, "pair leaves"): the two triangles of a quad share one leaf.  What a ray hits must not depend
on it: closest hits (triangle, t, u, v) and occlusion equal the oracle's brute force bit for bit, and images equal the oracle's,
with pairing on (the default) and with PTX_PAIR_LEAVES=0.  The scenes here share vertex indices between the triangles of a quad
(as the stand-ins' meshes do), so that pairs form, and every test checks how many pair leaves the build made (PTX_VERBOSE)."""
import re

import numpy as np
import pytest

import util
import test_tree_adversarial as adv

PAIR_MODES = ["1", "0"]


def _mesh(positions, indices):
    p = np.asarray(positions, np.float32)
    return {"positions": p, "indices": np.asarray(indices, np.uint32).reshape(-1), "normal": np.float32([0, 0, 1]),
            "uv": np.zeros((len(p), 2), np.float32)}


def _grid(nx, ny, z=0.0):
    """nx x ny quads in the plane z, each written as (a, d, c), (a, c, b) like the stand-ins' grid surfaces: one long run of
    links per row (neighbouring quads share an edge too), which parity must split into the quads."""
    xs, ys = np.linspace(-1.5, 1.5, nx + 1), np.linspace(-1.0, 1.0, ny + 1)
    p = [(x, y, z + 0.05 * x * y) for y in ys for x in xs]
    idx = []
    for j in range(ny):
        for i in range(nx):
            a, b, c, d = j * (nx + 1) + i, j * (nx + 1) + i + 1, (j + 1) * (nx + 1) + i + 1, (j + 1) * (nx + 1) + i
            idx += [a, d, c, a, c, b]
    return _mesh(p, idx)


def _strip(n, z, degenerate=None):
    """A zig-zag strip of n triangles (k, k+1, k+2): n - 1 links in one run; `degenerate`: that triangle made zero-area by a
    repeated index, which cuts the run in two."""
    p = [(-1.5 + 0.4 * k, 0.6 * (k % 2) - 0.3, z) for k in range(n + 2)]
    idx = []
    for k in range(n):
        t = [k, k + 1, k + 2] if k % 2 == 0 else [k + 1, k, k + 2]
        if k == degenerate:
            t = [k, k, k + 2]
        idx += t
    return _mesh(p, idx)


def _quad(z=0.0, s=1.0):
    return _mesh([(-s, -s, z), (s, -s, z), (s, s, z), (-s, s, z)], [0, 1, 2, 2, 3, 0])


def _dup_quads(n):
    """n coincident quads over the SAME four vertices: one run of 2n - 1 links (every neighbour shares two indices) and the
    bit-identical boxes of the PLOC tie case."""
    q = _quad(0.2, 0.8)
    return _mesh(q["positions"], np.tile(q["indices"], n))


def _scene(pkg, name):
    """(soup, expected pair leaves)"""
    if name == "grid":
        return util.TriangleSoup(pkg, [[_grid(7, 5)]]), 35
    if name == "odd_runs":     # 7 triangles: 3 pairs and a single; 9 with a zero-area 5th: (0 1) (2 3) | inert | (5 6) (7 8)
        return util.TriangleSoup(pkg, [[_strip(7, 0.0), _strip(9, 0.5, degenerate=4)]]), 3 + 4
    if name == "dup_quads":
        return util.TriangleSoup(pkg, [[_dup_quads(96)]]), 96
    if name == "across_pairs":
        # two meshes with one triangle each over the same edge (two (instance, mesh) pairs: no pair leaf), and one quad model
        # instanced twice (one pair leaf per instance)
        a = _mesh([(-1, -1, 0), (1, -1, 0), (1, 1, 0)], [0, 1, 2])
        b = _mesh([(-1, -1, 0), (1, 1, 0), (-1, 1, 0)], [0, 1, 2])
        inst = [(0, util.IDENTITY_3X4), (1, adv._translate((0.0, 0.0, 0.4))), (1, adv._translate((0.3, 0.2, -0.4)))]
        return util.TriangleSoup(pkg, [[a, b], [_quad()]], inst), 2
    if name == "mixed_opacity":
        # a non-opaque quad beside an opaque one over the same vertices: only the opaque one pairs
        s = util.TriangleSoup(pkg, [[_quad(0.0), _quad(0.0, 0.7), _grid(3, 2, 0.3)]])
        s.geometries["IsOpaque"][0] = 0
        return s, 1 + 6
    if name == "one_quad":
        return util.TriangleSoup(pkg, [[_quad()]]), 1
    raise KeyError(name)


SCENES = ["grid", "odd_runs", "dup_quads", "across_pairs", "mixed_opacity", "one_quad"]


def _pair_leaves(err):
    """The pair-leaf count of the last build logged under PTX_VERBOSE (0: the build made none)."""
    m = re.findall(r"\[ptx\] pair leaves: (\d+) \((\d+) of (\d+) tree triangles paired\)", err)
    return (int(m[-1][0]), int(m[-1][2])) if m else (0, None)


def _rays(desc, rng, n=3000):
    """Rays aimed at the centroids of random triangles from around the scene, plus random rays through its box."""
    T = util.world_triangles(desc)
    c = T[rng.integers(0, len(T), n)].mean(axis=1)
    o = c + rng.normal(size=c.shape) * 1.5
    lo, hi = T.reshape(-1, 3).min(axis=0) - 1.0, T.reshape(-1, 3).max(axis=0) + 1.0
    return np.concatenate([adv._aimed(o, c), util.random_rays(rng, n, lo, hi)])


@pytest.mark.gpu
@pytest.mark.parametrize("pair", PAIR_MODES)
@pytest.mark.parametrize("name", SCENES)
def test_paired_scenes_match_bruteforce(pkg, orc, monkeypatch, capfd, name, pair):
    """Closest hits and occlusion bit for bit against brute force, the expected number of pair leaves, and no stack overflow
    (ptx_trace_rays fails on one)."""
    import torch  # noqa: F401

    monkeypatch.setenv("PTX_PAIR_LEAVES", pair)
    monkeypatch.setenv("PTX_VERBOSE", "1")
    s, want_pairs = _scene(pkg, name)
    capfd.readouterr()
    r = adv._renderer(pkg, s.desc)
    try:
        got, _ = _pair_leaves(capfd.readouterr().err)
        assert got == (want_pairs if pair == "1" else 0), f"{name}: {got} pair leaves"
        util.check_trace_against_bruteforce(r, orc, s.desc, _rays(s.desc, np.random.default_rng(11)), 1000, label=f"{name} pairs={pair}")
    finally:
        r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("pair", PAIR_MODES)
def test_refit_recomputes_pair_boxes(pkg, orc, monkeypatch, pair):
    """Two instances of a paired grid refitted through sheared, scaled and far-moved poses: the union boxes of the pairs are
    recomputed, and the refitted tree equals brute force and a rebuilt tree."""
    import torch  # noqa: F401

    monkeypatch.setenv("PTX_PAIR_LEAVES", pair)
    s = util.TriangleSoup(pkg, [[_grid(9, 6), _dup_quads(8)]], [(0, util.IDENTITY_3X4), (0, adv._translate((0.0, 0.0, 2.0)))])
    r = adv._renderer(pkg, s.desc)
    rng = np.random.default_rng(23)
    try:
        shear = util.IDENTITY_3X4.copy()
        shear[[1, 2, 4, 8]] = (1.5, -0.7, 0.2, 0.9)
        stretch = adv._translate((3.0, -1.0, 0.5))
        stretch[[0, 5, 10]] = (4.0, 0.25, 2.0)
        for pose in (np.stack([shear, stretch]), np.stack([stretch, adv._translate((0.0, 0.0, 1e3))])):
            r.update_animation(pose, rebuild=False)
            T = util.world_triangles(s.desc, instance_transforms=pose)
            c = T[rng.integers(0, len(T), 2000)].mean(axis=1)
            rays = adv._aimed(c + rng.normal(size=c.shape), c)
            util.check_trace_against_bruteforce(r, orc, s.desc, rays, 1000, instance_transforms=pose, label=f"refit pairs={pair}")
            h_refit, i_refit = r.trace_rays(rays)
            r.update_animation(pose, rebuild=True)
            h_re, i_re = r.trace_rays(rays)
            assert (i_refit == i_re).all() and (h_refit.view(np.uint32) == h_re.view(np.uint32)).all()
    finally:
        r.close()


STAND_INS = ["chess_like", "temple_like", "atrium_like", "street_like", "alpha_test"]


@pytest.mark.gpu
@pytest.mark.parametrize("pair", PAIR_MODES)
@pytest.mark.parametrize("name", STAND_INS)
def test_stand_ins_match_bruteforce_and_oracle_images(pkg, orc, monkeypatch, capfd, name, pair):
    """Reduced-detail stand-ins: closest hits and occlusion against brute force, and a rendered image against the oracle."""
    import torch  # noqa: F401

    monkeypatch.setenv("PTX_PAIR_LEAVES", pair)
    monkeypatch.setenv("PTX_VERBOSE", "1")
    scene = pkg.Scene(name, 0.1)
    capfd.readouterr()
    r = pkg.Renderer()
    r.upload(scene)
    try:
        got, slots = _pair_leaves(capfd.readouterr().err)
        if pair == "0":
            assert got == 0
        util.check_trace_against_bruteforce(r, orc, scene.desc, _rays(scene.desc, np.random.default_rng(5), 1500), 500,
                                            label=f"{name} pairs={pair}")
    finally:
        r.close()
    img, ref = util.render_pair(pkg, orc, name, 0.25, 48, 32, 1, 3)
    assert (img.view(np.uint32) == ref.view(np.uint32)).all(), f"{name} PTX_PAIR_LEAVES={pair}: image differs from the oracle"


@pytest.mark.gpu
def test_chess_like_pairs_most_triangles(pkg, monkeypatch, capfd):
    """Pairing is active: most of chess_like's triangles are quads and end up in pair leaves (99 % at full detail)."""
    import torch  # noqa: F401

    monkeypatch.setenv("PTX_VERBOSE", "1")
    scene = pkg.Scene("chess_like", 0.25)
    capfd.readouterr()
    r = pkg.Renderer()
    r.upload(scene)
    r.close()
    got, slots = _pair_leaves(capfd.readouterr().err)
    print(f"chess_like (detail 0.25): {got} pair leaves, {2 * got} of {slots} tree triangles paired")
    assert slots and 2 * got >= 0.8 * slots
