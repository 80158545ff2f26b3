"""Skinning and ptx_update_animation against tests/skin_ref.py: linear-blend skinning written from the definition in numpy, float64
as the reference and float32 as the yardstick of the tolerance.  The scene, "skin_lab", is laid out so that no offset of the upload
plan is accidentally zero or unique, its vertices take every route through k_skin / skinVertex (weight classes a - g below), and its
bones scale, shear and mirror.

Tolerance (the rule of tests/test_debug_view.py).  Measured ON THE REFERENCE ALONE, never on k_skin or skinVertex:
tol = 8 x max |ref(float32) - ref(float64)|, floor 2^-20 max(1, |value|).  SKIN_F32_VS_F64 holds the maxima of skin_vertices per
pose and attribute over skin_lab's vertices, VIEW_F32_VS_F64 those of the debug-view reference per pose and mode over the 67 x 45
image; both are 1.25 x the measured values (numpy's float32 sums depend on the SIMD width of the CPU they run on; the constant must
hold on any), rounded up to two digits, printed by

    python tests/test_skinning.py

and test_tolerance_constants_cover_the_measurements recomputes them without a GPU."""
import os
import sys

import numpy as np
import pytest

import debug_view_ref as R
import skin_ref as S
import util

W, H = 67, 45
OUT_OF_RANGE = (9, 64, 0xFFFFFFFF)  # bone indices no pose reaches: the largest bone array of these tests has nine rows
CLASS_NAMES = {0: "a: one bone at 1, ignored slots behind it", 1: "b: two bones at 1/2", 2: "c: four bones at 1/4", 3: "d: sum below 1",
               4: "e: sum passing 1 early", 5: "f: exactly 1 after three slots", 6: "g: an out-of-range index in a slot that runs",
               7: "h: the 16 x 16 grid, two bones at k/16 and 1 - k/16"}
POSES = (0, 1, 2)
BONE_COUNT = 6

# (pose, attribute) -> 1.25 x max |skin_vertices(float32) - skin_vertices(float64)| over skin_lab's animated vertices
SKIN_F32_VS_F64 = {
    (0, 'position'): 5.2e-07,
    (0, 'normal'): 9.3e-08,
    (0, 'tangent'): 1.2e-07,
    (0, 'bitangent'): 1.4e-07,
    (1, 'position'): 4.2e-07,
    (1, 'normal'): 1.4e-07,
    (1, 'tangent'): 9.6e-08,
    (1, 'bitangent'): 1.2e-07,
    (2, 'position'): 4.7e-07,
    (2, 'normal'): 1.3e-07,
    (2, 'tangent'): 9.2e-08,
    (2, 'bitangent'): 1.1e-07,
}
# (pose or "bind", mode) -> 1.25 x max |debug_view_ref(float32) - debug_view_ref(float64)| over the 67 x 45 image of skin_lab
VIEW_F32_VS_F64 = {
    (0, 1): 2.1e-06,
    (0, 2): 2.5e-07,
    (0, 3): 1.1e-07,
    (1, 1): 2.1e-06,
    (1, 2): 2.0e-07,
    (1, 3): 1.4e-07,
    (2, 1): 2.1e-06,
    (2, 2): 2.3e-07,
    (2, 3): 1.3e-07,
    ('bind', 1): 2.1e-06,
    ('bind', 2): 1.8e-07,
    ('bind', 3): 9.1e-08,
}
ATTRIBUTES = {"position": slice(0, 3), "normal": slice(5, 8), "tangent": slice(8, 11), "bitangent": slice(11, 14)}
VIEW_MODES = (R.MODE_WORLD_POSITION, R.MODE_NORMAL, R.MODE_TEXTURE_COORDS)
NORMAL_TEXEL = (0.8, 0.35, 0.9, 1.0)  # a tilted constant: tangent and bitangent reach the Normal view


# =====================================================================================================
# the scene
# =====================================================================================================
def _rotation(axis, angle):
    a = np.float64(axis) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def _affine(linear, translation=(0, 0, 0)):
    return np.hstack([np.float64(linear), np.float64(translation).reshape(3, 1)]).astype(np.float32).reshape(12)


def pose_bones(pose):
    """Six bones, translations within +-8: a rotation; a rotation with translation; non-uniform scale (0.5, 2, 1.25) with
    rotation; a shear; a mirrored bone; a near-identity.  None is singular."""
    rng = np.random.default_rng(100 + pose)
    rot = lambda: _rotation(rng.normal(size=3), rng.uniform(0.3, 2.8))  # noqa: E731
    shift = lambda: rng.uniform(-3.0, 3.0, 3)  # noqa: E731
    shear = np.array([[1, 0.6, 0], [0, 1, -0.4], [0.3, 0, 1]]) + rng.uniform(-0.1, 0.1, (3, 3))
    return np.stack([_affine(rot()), _affine(rot(), shift()), _affine(rot() @ np.diag([0.5, 2.0, 1.25]), shift()), _affine(shear, shift()),
                     _affine(rot() @ np.diag([-1.0, 1.0, 1.0]), shift()), _affine(np.eye(3) + rng.uniform(-1e-3, 1e-3, (3, 3)), rng.uniform(-0.05, 0.05, 3))])


def _class_slots(c, rng):
    """(bone indices, weights) of weight class c; every weight a multiple of 1/64."""
    p = rng.permutation(BONE_COUNT)
    out = rng.choice(OUT_OF_RANGE, 3)
    return {0: ((p[0], out[0], out[1], out[2]), (1, 1 / 2, 1 / 4, 1 / 8)),
            1: ((p[0], p[1], p[2], p[3]), (1 / 2, 1 / 2, 0, 0)),
            2: ((p[0], p[1], p[2], p[3]), (1 / 4, 1 / 4, 1 / 4, 1 / 4)),
            3: ((p[0], p[1], p[2], p[3]), (3 / 8, 1 / 4, 0, 0)),
            4: ((p[0], p[1], p[2], p[3]), (3 / 4, 1 / 2, 1 / 2, 1 / 4)),
            5: ((p[0], p[1], p[2], p[3]), (1 / 2, 1 / 4, 1 / 4, 1 / 2)),
            6: ((p[0], out[0], p[1], p[2]), (1 / 2, 1 / 4, 1 / 4, 1 / 4))}[c]


def _random_triangles(rng, n, lo, hi, size):
    """Well-shaped triangles in random planes: corners about 120 degrees apart on a circle of radius 0.7 - 1 x size."""
    c = rng.uniform(lo, hi, (n, 1, 3))
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    v = np.cross(u, rng.normal(size=(n, 3)))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    angle = rng.uniform(0, 2 * np.pi, (n, 1)) + np.arange(3) * (2 * np.pi / 3) + rng.uniform(-0.4, 0.4, (n, 3))
    radius = size * rng.uniform(0.7, 1.0, (n, 3))
    return (c + (radius * np.cos(angle))[..., None] * u[:, None] + (radius * np.sin(angle))[..., None] * v[:, None]).astype(np.float32)


def _class_soup(rng, classes, lo, hi, size):
    """One animated mesh of own-vertex triangles, triangle k of class classes[k]: its three vertices share bones and weights, so
    the posed triangle is an affine image of the authored one and stays small."""
    tris = _random_triangles(rng, len(classes), lo, hi, size)
    slots = [_class_slots(c, rng) for c in classes]
    idx = np.repeat(np.array([s[0] for s in slots], np.uint32), 3, axis=0)
    wts = np.repeat(np.array([s[1] for s in slots], np.float32), 3, axis=0)
    assert (wts * 64 == np.round(wts * 64)).all()
    return S.animated_rows(tris, idx, wts, np.repeat(classes, 3))


def _grid(n=16, half=3.0):
    """An indexed n x n grid in the plane y = 0 facing +y, skinned by bones 0 and 1 at weights that slide along x."""
    x = np.linspace(-half, half, n, dtype=np.float32)
    px, pz = np.meshgrid(x, x, indexing="ij")
    pos = np.stack([px, np.zeros_like(px), pz], axis=-1).reshape(-1, 3)
    i, j = np.meshgrid(np.arange(n - 1), np.arange(n - 1), indexing="ij")
    v = lambda a, b: (a * n + b).reshape(-1)  # noqa: E731
    idx = np.stack([v(i, j), v(i, j + 1), v(i + 1, j), v(i + 1, j), v(i, j + 1), v(i + 1, j + 1)], axis=1).reshape(-1).astype(np.uint32)
    mesh = {"positions": pos, "indices": idx, "normal": np.float32([0, 1, 0]), "uv": ((pos[:, [0, 2]] + half) / (2 * half)).astype(np.float32)}
    k = np.repeat(np.arange(n), n)  # the column along x
    wts = np.stack([(n - k) / n, k / n, np.zeros(n * n), np.zeros(n * n)], axis=1).astype(np.float32)  # column 0: weight 1 in the first slot
    idx4 = np.tile(np.uint32([0, 1, 5, 5]), (n * n, 1))
    return S.animated_rows(mesh, idx4, wts, np.full(n * n, 7))


def _floor_and_clutter(rng, half, y, n):
    floor = np.float32([[[-half, y, half], [half, y, half], [half, y, -half]], [[half, y, -half], [-half, y, -half], [-half, y, half]]])
    return np.concatenate([floor, _random_triangles(rng, n, (-half, y + 0.4, -half), (half, y + 1.5, half), 0.8)])


MESH_TRANSFORM = _affine(_rotation((0.2, 1.0, 0.1), 0.7) * 1.1, (0.5, 1.0, -0.5))
UNMIRRORED_THIRD = _affine(_rotation((1, 0, 0.2), 0.5), (1.0, 3.0, -7.0))
MIRRORED_THIRD = _affine(_rotation((1, 0, 0.2), 0.5) @ np.diag([-1.0, 1.0, 1.0]), (1.0, 3.0, -7.0))


def skin_lab(pkg, mirrored=True):
    """Static mesh first (staticVertexCount != 0); model A with two animated geometries, the second at non-zero offsets into the
    animated arrays and under a non-identity mesh transform, instanced three times (translation; non-uniform scale with rotation;
    mirrored); model B, an indexed grid of exactly 256 vertices, instanced once."""
    rng = np.random.default_rng(2024)
    static = _floor_and_clutter(rng, 16.0, -4.0, 40)
    a0 = _class_soup(rng, np.repeat(np.arange(7), 5), (-2, -2, -2), (2, 2, 2), 1.3)
    a1 = _class_soup(rng, np.repeat(np.arange(7), 3), (-2, -2, -2), (2, 2, 2), 1.3)
    models = [[(static, 0)], [(a0, 0), (a1, 1)], [(_grid(), 0)]]
    instances = [(0, util.IDENTITY_3X4),
                 (1, _affine(np.eye(3), (-8.0, 3.0, 0.0))),
                 (1, _affine(_rotation((0.3, 1, 0), 1.1) @ np.diag([1.5, 0.7, 1.2]), (8.0, 3.0, 1.0))),
                 (1, MIRRORED_THIRD if mirrored else UNMIRRORED_THIRD),
                 (2, _affine(_rotation((0, 0, 1), 0.2), (0.0, 0.5, 5.0)))]
    return S.SkinnedSoup(pkg, models, instances, transforms=np.stack([util.IDENTITY_3X4, MESH_TRANSFORM]),
                         material=util.mr_material(color=(0.8, 0.7, 0.6), roughness=0.7), normal_texel=NORMAL_TEXEL)


def pose_instances(soup, pose):
    """Instance transforms of a pose: pose 0 keeps the scene's; the others move every instance but the static one."""
    it = soup.instances["Transform"].copy()
    if pose:
        rng = np.random.default_rng(200 + pose)
        for i in range(1, len(it)):
            m = np.float64(it[i]).reshape(3, 4)
            r = _rotation(rng.normal(size=3), rng.uniform(0.1, 0.6))
            it[i] = _affine(r @ m[:, :3], m[:, 3] + rng.uniform(-1.0, 1.0, 3))
    return it


def count_lab(pkg, skinned_vertices):
    """A floor and one soup of `skinned_vertices` / 3 skinned triangles, the classes in turn: k_skin's block edge."""
    assert skinned_vertices % 3 == 0
    rng = np.random.default_rng(skinned_vertices)
    n = skinned_vertices // 3
    soup = _class_soup(rng, np.arange(n) % 7, (-3, -2, -3), (3, 2, 3), 0.9)
    return S.SkinnedSoup(pkg, [[(_floor_and_clutter(rng, 16.0, -4.0, 4), 0)], [(soup, 0)]], [(0, util.IDENTITY_3X4), (1, _affine(np.eye(3), (0.5, 2.0, 0.0)))])


SKINNED_COUNTS = (3, 255, 258, 513)  # with the 256 of model B: one short of k_skin's 256-thread block, exact, one over, two blocks plus one

_cache = {}


def _lab(pkg):
    if "lab" not in _cache:
        _cache["lab"] = skin_lab(pkg)
    return _cache["lab"]


def _camera(pkg):
    if "camera" not in _cache:
        cam = pkg.Scene("default", 0.25)
        cam.set_camera_pose((0.0, 9.0, 20.0), (0.0, -0.25, -1.0))
        _cache["camera"] = cam.uniform(W, H)
    return _cache["camera"]


def aimed_rays(T, tri_class, rng, per_class, scattered):
    """`per_class` rays at interior points of triangles of every class (and of the static mesh, class -1) from random directions,
    then `scattered` random rays from above: (rays, the class each ray was aimed at; -2 for the scattered ones)."""
    rays, aim = [], []
    for c in np.unique(tri_class):
        ids = rng.choice(np.flatnonzero(tri_class == c), per_class)
        b = rng.dirichlet((2.0, 2.0, 2.0), per_class)
        point = np.einsum("nk,nki->ni", b, T[ids])
        d = rng.normal(size=(per_class, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        r = np.zeros((per_class, 8), np.float32)
        r[:, 0:3], r[:, 3], r[:, 4:7], r[:, 7] = point - d * rng.uniform(4.0, 12.0, (per_class, 1)), 1e-5, d, 1e4
        rays.append(r)
        aim.append(np.full(per_class, c))
    r = util.random_rays(rng, scattered, -12.0, 12.0)
    r[:, 1] = np.abs(r[:, 1]) + 6.0
    rays.append(r)
    aim.append(np.full(scattered, -2))
    rays, aim = np.concatenate(rays), np.concatenate(aim)
    # A ray that meets a triangle at a grazing angle, or a triangle that a blend of unlike bones has flattened to a sliver, has an
    # ill-conditioned hit: an error of the vertices is magnified by 1 / cos in t and by 1 / altitude in u and v.  Such rays are
    # not cast (decided in float64, on the reference's triangles alone; the hit minimum per class still holds afterwards).
    normal = np.cross(T[:, 1] - T[:, 0], T[:, 2] - T[:, 0])
    edge = np.stack([np.linalg.norm(T[:, k] - T[:, (k + 1) % 3], axis=1) for k in range(3)]).max(axis=0)
    sliver = np.linalg.norm(normal, axis=1) < 0.1 * np.maximum(edge, 1e-300)  # the altitude on the longest edge, world units
    normal /= np.maximum(np.linalg.norm(normal, axis=1, keepdims=True), 1e-300)
    keep = np.ones(len(rays), bool)
    for k in range(len(rays)):
        near = util.moller_trumbore_f64(T, rays[k])[4] > -1e-3
        keep[k] = not (sliver[near].any() or (np.abs(normal[near] @ np.float64(rays[k, 4:7])) < 0.1).any())
    return rays[keep], aim[keep]


def _skin_tolerance(pose, want):
    """Per value of an (n, 14) block: 8 x the measured float32 / float64 maximum of its attribute, floor 2^-20 max(1, |value|)."""
    tol = 2.0 ** -20 * np.maximum(1.0, np.abs(want))
    for name, cols in ATTRIBUTES.items():
        tol[:, cols] = np.maximum(tol[:, cols], 8.0 * SKIN_F32_VS_F64[(pose, name)])
    return tol


def _measure_skin(pkg, pose):
    lab = _lab(pkg)
    a, b = S.skin_vertices(lab.animated_vertices, pose_bones(pose), np.float32), S.skin_vertices(lab.animated_vertices, pose_bones(pose), np.float64)
    return {name: float(np.abs(a[:, cols].astype(np.float64) - b[:, cols]).max()) for name, cols in ATTRIBUTES.items()}


def _pose(pkg, pose):
    """(bones, instance transforms) of a pose of skin_lab; "bind": as uploaded."""
    return (None, None) if pose == "bind" else (pose_bones(pose), pose_instances(_lab(pkg), pose))


def _view_ref(pkg, orc, pose, mode, dtype):
    """The debug-view reference of skin_lab in a pose: computed once, shared and left unchanged."""
    key = ("view", pose, mode, np.dtype(dtype).name)
    if key not in _cache:
        lab = _lab(pkg)
        bones, it = _pose(pkg, pose)
        if ("rs", pose) not in _cache:
            _cache[("rs", pose)] = R.RefScene(orc, lab.desc, instance_transforms=it, bones=bones)
        block, _ = S.posed_vertices(lab, bones, dtype, it)
        _cache[key] = R.render(_cache[("rs", pose)], _camera(pkg), pkg.LightsUbo(), W, H, mode, 0, dtype, posed=block)
        _cache[key]["image"].setflags(write=False)
    return _cache[key]


def _measure_view(pkg, orc, pose, mode):
    a, b = _view_ref(pkg, orc, pose, mode, np.float32), _view_ref(pkg, orc, pose, mode, np.float64)
    return float(np.abs(a["image"].astype(np.float64) - b["image"]).max())


def _view_tolerance(pkg, orc, pose, mode):
    b = _view_ref(pkg, orc, pose, mode, np.float64)["image"]
    return np.maximum(8.0 * VIEW_F32_VS_F64[(pose, mode)], 2.0 ** -20 * np.maximum(1.0, np.abs(b)))


# =====================================================================================================
# without a GPU
# =====================================================================================================
def test_skin_reference_on_hand_computed_vertices():
    """skin_vertices against values worked out by hand: the scale bone sends the normal through the inverse transpose; the weights
    stop counting once they have reached 1; an index past the array is the identity; nothing is normalised after the sum."""
    bones = np.stack([_affine(np.diag([2.0, 1.0, 1.0]), (1, 0, 0)), _affine(_rotation((0, 0, 1), np.pi / 2), (0, 0, 5))])
    rows = np.zeros(4, S.ANIMATED_VERTEX_DT)
    rows["Position"], rows["TexCoords"] = (1, 1, 0), (0.25, 0.75)
    s = np.sqrt(0.5)
    rows["Normal"], rows["Tangent"], rows["Bitangent"] = (s, s, 0), (s, -s, 0), (0, 0, 1)
    rows["BoneIndices"] = [(0, 1, 1, 1), (0, 1, 0, 0), (1, 2, 0, 0), (1, 0, 0, 0)]
    rows["BoneWeights"] = [(1, 1, 1, 1), (0.5, 0.5, 0.5, 0.5), (0.5, 0.5, 0, 0), (0.25, 0.5, 0, 0)]
    for dtype, eps in ((np.float32, 1e-6), (np.float64, 1e-14)):
        out = S.skin_vertices(rows, bones, dtype)
        assert out.dtype == dtype and (out[:, 3:5] == np.float32([0.25, 0.75])).all()
        n0, t0 = np.float64([0.5, 1, 0]) / np.sqrt(1.25), np.float64([2, -1, 0]) / np.sqrt(5.0)  # through diag(1/2, 1, 1) and diag(2, 1, 1)
        p0, p1 = np.float64([3, 1, 0]), np.float64([-1, 1, 5])
        n1, t1 = np.float64([-s, s, 0]), np.float64([s, s, 0])
        assert np.allclose(out[0], np.concatenate([p0, [0.25, 0.75], n0, t0, [0, 0, 1]]), atol=eps, rtol=0)
        assert np.allclose(out[1], np.concatenate([(p0 + p1) / 2, [0.25, 0.75], (n0 + n1) / 2, (t0 + t1) / 2, [0, 0, 1]]), atol=eps, rtol=0)
        assert np.allclose(out[2], np.concatenate([(p1 + [1, 1, 0]) / 2, [0.25, 0.75], (n1 + [s, s, 0]) / 2, (t1 + [s, -s, 0]) / 2, [0, 0, 1]]), atol=eps, rtol=0)
        assert np.allclose(out[3], np.concatenate([p1 / 4 + p0 / 2, [0.25, 0.75], n1 / 4 + n0 / 2, t1 / 4 + t0 / 2, [0, 0, 0.75]]), atol=eps, rtol=0)


def test_skin_lab_leaves_no_offset_at_zero(pkg):
    lab = _lab(pkg)
    g = lab.geometries
    assert list(g["IsAnimated"]) == [0, 1, 1, 1] and lab.desc.vertexCount == 126 and lab.desc.animatedVertexCount == 105 + 63 + 256
    assert g["VertexOffset"][2] == 105 and g["IndexOffset"][2] == 105 and g["VertexLength"][3] == 256 and g["IndexLength"][3] == 15 * 15 * 6
    assert lab.meshes["TransformIndex"][2] == 1 and not np.array_equal(lab.transforms[1], util.IDENTITY_3X4)
    dets = [np.linalg.det(np.float64(x).reshape(3, 4)[:, :3]) for x in lab.instances["Transform"]]
    assert list(lab.instances["ModelIndex"]) == [0, 1, 1, 1, 2] and dets[3] < 0 < min(dets[1], dets[2]) and abs(dets[2] - 1.26) < 1e-3
    src = lab.skin_source()
    assert len(src) == 3 * 168 + 256 and (np.bincount(src)[:168] == 3).all() and (np.bincount(src)[168:] == 1).all()
    assert set(np.unique(lab.triangle_class())) == set(range(-1, 8))
    for pose in POSES:
        b = pose_bones(pose).reshape(-1, 3, 4)
        d = np.linalg.det(np.float64(b[:, :, :3]))
        assert len(b) == BONE_COUNT and (np.abs(d) > 0.5).all() and d[4] < 0 and (np.abs(b[:, :, 3]) <= 8).all()
    assert [count_lab(pkg, n).desc.animatedVertexCount for n in SKINNED_COUNTS] == list(SKINNED_COUNTS)


def test_tolerance_constants_cover_the_measurements(pkg, orc):
    """Every constant behind a tolerance is at least what the reference's own float32 and float64 instances differ by, and not
    more than twice that: a bound that has gone stale in either direction fails here."""
    assert set(SKIN_F32_VS_F64) == {(p, a) for p in POSES for a in ATTRIBUTES}
    assert set(VIEW_F32_VS_F64) == {(p, m) for p in POSES + ("bind",) for m in VIEW_MODES}
    for pose in POSES:
        for name, got in _measure_skin(pkg, pose).items():
            assert 0.5 * SKIN_F32_VS_F64[(pose, name)] <= got <= SKIN_F32_VS_F64[(pose, name)], (pose, name, got)
    for key in VIEW_F32_VS_F64:
        got = _measure_view(pkg, orc, *key)
        assert 0.5 * VIEW_F32_VS_F64[key] <= got <= VIEW_F32_VS_F64[key], (key, got)


@pytest.mark.parametrize("pose", POSES)
def test_oracle_skinned_vertices_against_reference(pkg, orc, pose):
    """The oracle's skinned vertex block (skinVertex) against skin_vertices in float64, attribute by attribute and class by class,
    in the device's order: one copy per (instance, animated mesh) pair."""
    lab = _lab(pkg)
    bones = pose_bones(pose)
    want, _ = S.posed_vertices(lab, bones, np.float64)
    osc = orc.OracleScene(lab.desc, build_bvh=False, bones=bones)
    got = osc.skinned_vertices()
    osc.close()
    assert got.shape == want.shape == (3 * 168 + 256, 14)
    err, tol = np.abs(got.astype(np.float64) - want), _skin_tolerance(pose, want)
    cls = lab.vertex_class[lab.skin_source()]
    for c, label in CLASS_NAMES.items():
        sel = cls == c
        assert sel.sum() >= 27
        for name, cols in ATTRIBUTES.items():
            worst = (err[sel][:, cols] / tol[sel][:, cols]).max()
            assert worst <= 1.0, f"pose {pose}, class {label}: {name} is off by {worst:.3g} x the tolerance"
    assert (got[:, 3:5] == want[:, 3:5]).all(), "texture coordinates are copied"
    # classes d and e leave their sums short of or beyond unit length; nothing renormalises them
    length = np.linalg.norm(got[:, 5:8], axis=1)
    assert (length[cls == 3] < 0.63).all() and (length[cls == 0] > 0.999).all()


def test_oracle_bind_pose_and_empty_bone_array(pkg, orc):
    """Without bones the block holds the attributes as authored; an empty bone array skins with the identity in every slot, which
    scales the vertices whose weights do not sum to 1."""
    lab = _lab(pkg)
    osc = orc.OracleScene(lab.desc, build_bvh=False)
    assert (osc.skinned_vertices() == S.posed_vertices(lab, None, np.float32)[0]).all()
    osc.close()
    osc = orc.OracleScene(lab.desc, build_bvh=False, bones=np.zeros((0, 12), np.float32))
    got = osc.skinned_vertices()
    osc.close()
    ident = np.tile(util.IDENTITY_3X4, (BONE_COUNT, 1))
    for bones in (np.zeros((0, 12), np.float32), ident):
        want = S.posed_vertices(lab, bones, np.float64)[0]
        assert (np.abs(got - want) <= 2.0 ** -20 * np.maximum(1.0, np.abs(want))).all()
    cls = lab.vertex_class[lab.skin_source()]
    bind = S.posed_vertices(lab, None, np.float64)[0]
    assert np.allclose(got[cls == 3, 0:3], 0.625 * bind[cls == 3, 0:3], atol=1e-5) and np.allclose(got[cls == 4, 0:3], 1.25 * bind[cls == 4, 0:3], atol=1e-5)


def _closest_hits_case(pkg, orc, lab, bones, it, seed, per_class, class_hits, floor_hits, label):
    _, T = S.posed_vertices(lab, bones, np.float64, it)
    tri_class = lab.triangle_class()
    rays, aim = aimed_rays(T, tri_class, np.random.default_rng(seed), per_class, 200)
    osc = orc.OracleScene(lab.desc, build_bvh=True, instance_transforms=it, bones=bones)
    got = osc.trace_closest(rays)
    brute = osc.trace_closest(rays, brute_force=True)
    osc.close()
    assert (got == brute).all()
    hit = got["tri"] != 0xFFFFFFFF
    for c in np.unique(tri_class):
        n = int((tri_class[got["tri"][hit]] == c).sum())
        assert n >= (floor_hits if c < 0 else class_hits), f"{label}: only {n} hits on class {CLASS_NAMES.get(c, 'static')}"
    hits, agree, close = util.check_closest_against_float64(T, rays, got)
    assert hits >= hit.sum() - 5 and agree >= 0.98 * hits, (label, hits, agree, close)
    return rays


@pytest.mark.parametrize("pose", POSES)
def test_oracle_closest_hits_against_float64_triangles(pkg, orc, pose):
    """Closest hits of the oracle's posed scene against Moeller-Trumbore in float64 over the reference's posed triangles: every
    weight class, the static mesh, all three instances of model A and the grid, each with a minimum of hits.  No t_slack: the
    scene stays within 40 units of the origin, where the bounds of check_closest_against_float64 hold as they are."""
    lab = _lab(pkg)
    _closest_hits_case(pkg, orc, lab, pose_bones(pose), pose_instances(lab, pose), 10 + pose, 120, 40, 100, f"pose {pose}")


@pytest.mark.parametrize("count", SKINNED_COUNTS)
def test_oracle_closest_hits_at_the_skinned_vertex_counts(pkg, orc, count):
    lab = count_lab(pkg, count)
    per_class = 80 if count > 3 else 40
    for pose in POSES:
        _closest_hits_case(pkg, orc, lab, pose_bones(pose), None, 20 + pose, per_class, per_class // 2, 40, f"{count} vertices, pose {pose}")


@pytest.mark.parametrize("pose", POSES + ("bind",))
def test_debug_view_reference_on_posed_scenes(pkg, orc, pose):
    """The extended reference's own float32 and float64 instances agree on skin_lab within the tolerance, see animated geometry of
    every class, and place the world position on the pixel's ray."""
    lab = _lab(pkg)
    tri_class = lab.triangle_class()
    for mode in VIEW_MODES:
        a, b = _view_ref(pkg, orc, pose, mode, np.float32), _view_ref(pkg, orc, pose, mode, np.float64)
        assert (np.abs(a["image"].astype(np.float64) - b["image"]) <= _view_tolerance(pkg, orc, pose, mode)).all(), mode
        assert (a["hit"] == b["hit"]).all() and b["hit"].any() and not b["hit"].all()
    seen = np.bincount(tri_class[b["tri"][b["hit"]]] + 1, minlength=9)
    print(f"pose {pose}: pixels per class (static first) {seen}")
    assert (seen >= 4).all() and seen[1:].sum() >= 300, seen
    ref = _view_ref(pkg, orc, pose, R.MODE_WORLD_POSITION, np.float64)
    P, hit = ref["image"][..., 0:3], ref["hit"]
    on_ray = ref["origin"].astype(np.float64) + ref["t"].astype(np.float64)[..., None] * ref["direction"].astype(np.float64)
    assert (np.abs(P - on_ray).max(axis=-1)[hit] <= 2.0 ** -18 * np.maximum(1.0, np.maximum(np.abs(P).max(axis=-1), ref["t"]))[hit]).all()


# =====================================================================================================
# on the GPU
# =====================================================================================================
CLEAR = np.float32([0.2, 0.2, 0.2, 1.0])


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _renderer(pkg, desc, width=W, height=H):
    import torch  # noqa: F401  (first, so the HIP library shares torch's HIP runtime)

    r = pkg.Renderer()
    r.upload(desc)
    r.resize(width, height)
    return r


def _lab_rays(pkg, lab, bones, it, seed, per_class=120):
    _, T = S.posed_vertices(lab, bones, np.float64, it)
    rays, _ = aimed_rays(T, lab.triangle_class(), np.random.default_rng(seed), per_class, 200)
    assert len(rays) <= 6000
    return T, rays


def _as_oracle_record(desc, hits, ids):
    got = np.zeros(len(hits), dtype=[("t", "f4"), ("u", "f4"), ("v", "f4"), ("tri", "u4")])
    got["t"], got["u"], got["v"], got["tri"] = hits[:, 0], hits[:, 1], hits[:, 2], util.global_ids(desc, ids)
    return got


def _check_posed_trace(pkg, orc, r, lab, bones, it, seed, label, min_hits=100, per_class=40):
    """ptx_trace_rays of the renderer as it stands against the oracle's brute force over the scene posed by (it, bones), bit for
    bit, and against the reference's float64 triangles.  Returns (hits, ids)."""
    T, rays = _lab_rays(pkg, lab, bones, it, seed, per_class)
    util.check_trace_against_bruteforce(r, orc, lab.desc, rays, min_hits, instance_transforms=it, label=label, bones=bones)
    hits, ids = r.trace_rays(rays)
    n, agree, _ = util.check_closest_against_float64(T, rays, _as_oracle_record(lab.desc, hits, ids))
    assert agree >= 0.98 * n, (label, n, agree)
    return hits, ids


@pytest.mark.gpu
@pytest.mark.parametrize("scene", ("lab",) + SKINNED_COUNTS)
def test_trace_parity_after_update(pkg, orc, scene):
    """After ptx_update_animation: ptx_trace_rays equals the oracle's brute force bit for bit, agrees with Moeller-Trumbore in
    float64 over the reference's posed triangles, and a refit answers like a rebuild -- for three poses, on skin_lab and at the
    skinned-vertex counts around k_skin's block size."""
    lab = _lab(pkg) if scene == "lab" else count_lab(pkg, scene)
    r = _renderer(pkg, lab.desc)
    for pose in POSES:
        bones, it = pose_bones(pose), pose_instances(lab, pose) if scene == "lab" else None
        r.update_animation(it, bones)
        refit = _check_posed_trace(pkg, orc, r, lab, bones, it, 30 + pose, f"{scene}, pose {pose}, refit", 300 if scene == "lab" else 100, 120)
        r.update_animation(it, bones, rebuild=True)
        rebuilt = _check_posed_trace(pkg, orc, r, lab, bones, it, 30 + pose, f"{scene}, pose {pose}, rebuild", 300 if scene == "lab" else 100, 120)
        assert (refit[1] == rebuilt[1]).all() and (_bits(refit[0]) == _bits(rebuilt[0])).all(), (scene, pose)
    r.close()


def _check_views(pkg, orc, r, pose):
    """WorldPosition, TextureCoords and Normal of the renderer as it stands within the tolerance of the float64 reference in that
    pose, no pixel left out; the three id modes bit for bit; the world position on the pixel's ray."""
    u, lights = _camera(pkg), pkg.LightsUbo()
    for mode in VIEW_MODES:
        ref = _view_ref(pkg, orc, pose, mode, np.float64)
        r.render_debug(u, lights, mode)
        img = r.readback()
        hit = ref["hit"]
        err = np.abs(img.astype(np.float64) - ref["image"])
        tol = _view_tolerance(pkg, orc, pose, mode)
        print(f"pose {pose}, mode {mode}: max |gpu - ref64| {err.max():.3e}, worst error / tolerance {(err / tol).max():.3f}, constant for max |ref32 - ref64| {VIEW_F32_VS_F64[(pose, mode)]:.1e}")
        assert (err <= tol).all(), (pose, mode, float((err / tol).max()))
        assert (_bits(img)[~hit] == _bits(CLEAR)).all() and (img[..., 3] == 1.0).all()
        if mode == R.MODE_WORLD_POSITION:  # independent of the vertex data
            o, d, t = ref["origin"].astype(np.float64), ref["direction"].astype(np.float64), ref["t"].astype(np.float64)
            P = img[..., 0:3].astype(np.float64)
            off = np.abs(P - (o + t[..., None] * d)).max(axis=-1)
            assert (off[hit] <= 2.0 ** -18 * np.maximum(1.0, np.maximum(np.abs(P).max(axis=-1), t))[hit]).all()
    for mode in (R.MODE_GEOMETRY, R.MODE_PRIMITIVE, R.MODE_INSTANCE):
        ref = _view_ref(pkg, orc, pose, mode, np.float32)
        r.render_debug(u, lights, mode)
        assert (_bits(r.readback()) == _bits(ref["image"])).all(), (pose, mode)


@pytest.mark.gpu
def test_attributes_through_the_debug_view(pkg, orc):
    """Position, texture coordinates and the normal-mapped normal of skinned vertices as the debug view shows them, in bind pose
    straight after the upload and after the update to each pose.  The 1 x 1 normal texture is a tilted constant, so the skinned
    tangent and bitangent reach the pixel."""
    lab = _lab(pkg)
    r = _renderer(pkg, lab.desc)
    _check_views(pkg, orc, r, "bind")
    for pose in POSES:
        bones, it = _pose(pkg, pose)
        r.update_animation(it, bones)
        _check_views(pkg, orc, r, pose)
    r.close()


def _culled_reference(lab, T, it, o, d):
    """Per pixel the global triangle a primary ray with back-face culling hits, by Moeller-Trumbore in float64 (-1: none), and
    whether the pixel is decided: no candidate within 1e-4 (barycentric) of an edge or within 1e-4 of edge-on, and no other
    front-facing hit within 1e-3 of the nearest.  Back-facing (include/ptx.h, PTX_DEBUG_RAYGEN_CULL_BACK_FACES): in the space of
    the model, i.e. dot(cross(p1 - p0, p2 - p0), d) > 0 on the world-space triangle, reversed for a mirroring instance."""
    inst = np.concatenate([np.full(int(g["IndexLength"]) // 3, i) for i, _, g in lab.pairs()])  # the instance of every triangle
    mirrored = np.array([np.linalg.det(np.float64(x).reshape(3, 4)[:, :3]) < 0 for x in np.asarray(it).reshape(-1, 12)])[inst]
    normal = np.cross(T[:, 1] - T[:, 0], T[:, 2] - T[:, 0])
    normal /= np.linalg.norm(normal, axis=1, keepdims=True)
    tri, decided = np.full(len(o), -1, np.int64), np.ones(len(o), bool)
    v0, e1, e2 = T[:, 0], T[:, 1] - T[:, 0], T[:, 2] - T[:, 0]
    for lo in range(0, len(o), 512):  # util.moller_trumbore_f64 for 512 rays at a time
        oo, dd = np.float64(o[lo:lo + 512])[:, None], np.float64(d[lo:lo + 512])[:, None]
        pv = np.cross(dd, e2)
        with np.errstate(divide="ignore", invalid="ignore"):
            inv = 1.0 / np.einsum("tj,ntj->nt", e1, pv)
            sv = oo - v0
            bu = np.einsum("ntj,ntj->nt", sv, pv) * inv
            qv = np.cross(sv, e1)
            bv = np.einsum("ntj,ntj->nt", qv, np.broadcast_to(dd, qv.shape)) * inv
            t = np.einsum("tj,ntj->nt", e2, qv) * inv
            margin = np.minimum(np.minimum(bu, bv), 1 - bu - bv)
            inside = (margin >= 0) & (t > 1e-5) & (t < 1e4)
            facing = dd[:, 0] @ normal.T
            front = inside & ((facing > 0) == mirrored)
            unsure = (margin > -1e-4) & (t > 0) & ((margin < 1e-4) | (np.abs(facing) < 1e-4))
            tf = np.where(front, t, np.inf)
            k = np.argmin(tf, axis=1)
            nearest = tf[np.arange(len(k)), k]
            second = np.partition(tf, 1, axis=1)[:, 1]
            hit = np.isfinite(nearest)
            tri[lo:lo + 512] = np.where(hit, k, -1)
            decided[lo:lo + 512] = np.where(hit, ~(unsure & (t < nearest[:, None] + 1e-3)).any(axis=1) & ~(second - nearest <= 1e-3), ~unsure.any(axis=1))
    return tri, decided, inst


@pytest.mark.gpu
def test_mirror_sign_refresh(pkg, orc):
    """ptx_update_animation refreshes the winding sign that back-face culling reads: uploaded un-mirrored,
    the third instance of model A is then mirrored by an update and un-mirrored by another."""
    lab = skin_lab(pkg, mirrored=False)
    bones = pose_bones(0)
    before, after = lab.instances["Transform"].copy(), lab.instances["Transform"].copy()
    after[3] = MIRRORED_THIRD
    u, lights = _camera(pkg), pkg.LightsUbo()
    o, d, _, _ = R.primary_rays(orc, u, W, H)
    rs = R.RefScene(orc, lab.desc)
    r = _renderer(pkg, lab.desc)
    r.update_animation(before, bones)

    def culled():
        out = []
        for mode in (R.MODE_GEOMETRY, R.MODE_PRIMITIVE, R.MODE_INSTANCE):
            r.render_debug(u, lights, mode, pkg.DEBUG_RAYGEN_CULL_BACK_FACES)
            out.append(r.readback())
        return out

    def check(imgs, it, label):
        _, T = S.posed_vertices(lab, bones, np.float64, it)
        tri, decided, inst = _culled_reference(lab, T, it, o, d)
        assert decided.mean() > 0.97, (label, decided.mean())
        h = tri >= 0
        p = np.searchsorted(rs.first, tri[h], side="right") - 1
        for img, ident in zip(imgs, (rs.pair[p, 1], tri[h] - rs.first[p], rs.pair[p, 0])):
            want = np.tile(CLEAR, (W * H, 1))
            want[h, 0:3] = R.random_color(ident)
            same = (_bits(img).reshape(-1, 4) == _bits(want)).all(axis=-1)
            assert same[decided].all(), f"{label}: {int((~same & decided).sum())} decided pixels show another triangle"
        touched = np.zeros(W * H, bool)
        touched[h] = inst[tri[h]] == 3
        return touched, decided

    first = culled()
    touched, decided = check(first, before, "un-mirrored")
    r.update_animation(after, None)  # instances only: the bones stay
    second = culled()
    touched2, decided2 = check(second, after, "mirrored")
    touched, decided = touched | touched2, decided & decided2
    differs = (_bits(first[1]) != _bits(second[1])).any(axis=-1).reshape(-1)
    assert (differs & touched).sum() >= 20, "the mirrored instance must show other faces"
    assert not (differs & ~touched & decided).any(), "nothing else may change"
    r.update_animation(before, None)
    third = culled()
    assert all((_bits(a) == _bits(b)).all() for a, b in zip(first, third))
    r.close()


def _lights(pkg):
    lights = pkg.LightsUbo()
    lights.LightCount = 1
    lights.Directional.Color[:] = (1.0, 0.9, 0.8)
    lights.Directional.Direction[:] = (0.3, -1.0, 0.2)
    lights.Lights[0].Color[:] = (40.0, 40.0, 50.0)
    lights.Lights[0].Position[:] = (0.5, 9.0, 6.0)
    lights.Lights[0].AttenuationConstant, lights.Lights[0].AttenuationLinear, lights.Lights[0].AttenuationQuadratic = 1.0, 0.1, 0.02
    return lights


PW, PH = 64, 36


def _path_uniform(pkg):
    if "path_uniform" not in _cache:
        cam = pkg.Scene("default", 0.25)
        cam.set_camera_pose((0.0, 9.0, 20.0), (0.0, -0.25, -1.0))
        _cache["path_uniform"] = cam.uniform(PW, PH, bounces=2, sample_count=2)
    return _cache["path_uniform"]


def _check_path_traced(pkg, orc, r, lab, bones, it, label):
    """One 64 x 36, 2-bounce, 2-sample frame of the renderer as it stands against the oracle posed by (it, bones), bit for bit."""
    u, lights = _path_uniform(pkg), _lights(pkg)
    osc = orc.OracleScene(lab.desc, instance_transforms=it, bones=bones)
    ref, ost = osc.render(u, lights, PW, PH)
    osc.close()
    r.reset()
    r.render(u, lights)
    st = r.stats()
    img = r.readback()
    assert (st.segments, st.shadowRays) == (ost.segments, ost.shadowRays), label
    assert (_bits(img) == _bits(ref)).all(), f"{label}: {int((_bits(img) != _bits(ref)).any(axis=-1).sum())} pixels differ"
    assert np.isfinite(ref).all() and (ref[..., 0:3] > 0).any()
    return img


@pytest.mark.gpu
def test_call_sequences(pkg, orc):
    """The branches of ptx_update_animation, each against the oracle posed the same way."""
    lab = _lab(pkg)
    r = _renderer(pkg, lab.desc, PW, PH)
    b = [pose_bones(p) for p in POSES]
    it = [pose_instances(lab, p) for p in POSES]
    # an update before the first render
    r.update_animation(it[1], b[1])
    _check_path_traced(pkg, orc, r, lab, b[1], it[1], "update before the first render")
    _check_posed_trace(pkg, orc, r, lab, b[1], it[1], 40, "update before the first render")
    # bones only, then instances only: each keeps the other half
    r.update_animation(None, b[2])
    _check_posed_trace(pkg, orc, r, lab, b[2], it[1], 41, "bones only")
    r.update_animation(it[0], None)
    _check_posed_trace(pkg, orc, r, lab, b[2], it[0], 42, "instances only")
    # two updates in a row: the last wins
    r.update_animation(it[1], b[0])
    r.update_animation(it[2], b[1])
    _check_posed_trace(pkg, orc, r, lab, b[1], it[2], 43, "two updates in a row")
    # the bone array grows to nine rows (the extra three unused), shrinks to two (indices 2 .. 5 out of range: the identity), and
    # comes back
    r.update_animation(it[0], b[0])
    six = _check_posed_trace(pkg, orc, r, lab, b[0], it[0], 44, "six bones")
    nine = np.concatenate([b[0], pose_bones(7)[1:4]])
    r.update_animation(None, nine)
    grown = _check_posed_trace(pkg, orc, r, lab, nine, it[0], 44, "nine bones")
    assert (six[1] == grown[1]).all() and (_bits(six[0]) == _bits(grown[0])).all()
    r.update_animation(None, b[0][:2])
    _check_posed_trace(pkg, orc, r, lab, b[0][:2], it[0], 45, "two bones")
    _check_path_traced(pkg, orc, r, lab, b[0][:2], it[0], "two bones")
    r.update_animation(None, b[0])
    again = _check_posed_trace(pkg, orc, r, lab, b[0], it[0], 44, "six bones again")
    assert (six[1] == again[1]).all() and (_bits(six[0]) == _bits(again[0])).all()
    # an empty bone array skins with the identity: not the bind pose, where the weights do not sum to 1
    empty = np.zeros((0, 12), np.float32)
    r.update_animation(None, empty)
    none = _check_posed_trace(pkg, orc, r, lab, empty, it[0], 46, "empty bone array")
    ident = np.tile(util.IDENTITY_3X4, (BONE_COUNT, 1))
    r.update_animation(None, ident)
    unit = _check_posed_trace(pkg, orc, r, lab, ident, it[0], 46, "identity bones")
    assert (none[1] == unit[1]).all() and (_bits(none[0]) == _bits(unit[0])).all()
    r.close()


@pytest.mark.gpu
def test_borrower_sees_the_owners_pose(pkg, orc):
    lab = _lab(pkg)
    owner = _renderer(pkg, lab.desc, PW, PH)
    borrower = pkg.Renderer()
    borrower.share_scene(owner)
    borrower.resize(PW, PH)
    bones, it = pose_bones(1), pose_instances(lab, 1)
    owner.update_animation(it, bones)
    a = _check_posed_trace(pkg, orc, owner, lab, bones, it, 50, "owner")
    c = _check_posed_trace(pkg, orc, borrower, lab, bones, it, 50, "borrower")
    assert (a[1] == c[1]).all() and (_bits(a[0]) == _bits(c[0])).all()
    img = _check_path_traced(pkg, orc, owner, lab, bones, it, "owner")
    assert (_bits(_check_path_traced(pkg, orc, borrower, lab, bones, it, "borrower")) == _bits(img)).all()
    with pytest.raises(pkg.PtxError):
        borrower.update_animation(it, bones)
    with pytest.raises(pkg.PtxError):
        borrower.update_animation(None, bones)
    c = _check_posed_trace(pkg, orc, borrower, lab, bones, it, 50, "borrower after the refused update")
    assert (a[1] == c[1]).all() and (_bits(a[0]) == _bits(c[0])).all()
    borrower.close()
    owner.close()


@pytest.mark.gpu
@pytest.mark.parametrize("backend", (0, 1), ids=("wavefront", "megakernel"))
def test_path_tracer_on_skinned_geometry(pkg, orc, backend):
    """One 64 x 36, 2-bounce, 2-sample render of skin_lab per pose matches the oracle bit for bit: k_tri_setup's shading records and
    k_shade with skinned normals shorter and longer than unit length (classes d and e)."""
    import torch  # noqa: F401

    lab = _lab(pkg)
    r = pkg.Renderer(backend=backend)
    r.upload(lab.desc)
    r.resize(PW, PH)
    _check_path_traced(pkg, orc, r, lab, None, None, "bind pose")
    for pose in POSES:
        bones, it = pose_bones(pose), pose_instances(lab, pose)
        r.update_animation(it, bones)
        _check_path_traced(pkg, orc, r, lab, bones, it, f"pose {pose}")
    r.close()


if __name__ == "__main__":  # prints SKIN_F32_VS_F64 and VIEW_F32_VS_F64
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import __graft_entry__ as graft

    def round_up(x):
        """1.25 x, to two significant digits, upwards"""
        x = 1.25 * x
        e = int(np.floor(np.log10(x))) - 1
        return float(f"{np.ceil(x / 10.0 ** e) * 10.0 ** e:.1e}")

    pkg_, orc_ = graft.load_package(), graft.load_oracle()
    orc_.build()
    print("SKIN_F32_VS_F64 = {")
    for pose_ in POSES:
        for name_, got_ in _measure_skin(pkg_, pose_).items():
            print(f"    ({pose_!r}, {name_!r}): {round_up(got_):.1e},")
    print("}\nVIEW_F32_VS_F64 = {")
    for pose_ in POSES + ("bind",):
        for mode_ in VIEW_MODES:
            print(f"    ({pose_!r}, {mode_}): {round_up(_measure_view(pkg_, orc_, pose_, mode_)):.1e},")
    print("}")
