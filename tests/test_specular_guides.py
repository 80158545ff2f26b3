"""The specular-chain guide pass (include/ptx.h ptx_render_guides_specular, csrc/pt_denoise.hpp k_render_guides_specular,
docs/NEXT_ROWS.md section 18) against tests/specular_guides_ref.py.

Bit-exact legs need no tolerance: a pixel whose chain has no bounce holds the plain pass's bits, maxBounces = 0 is the plain pass,
tile shards write what the whole frame writes, and everything behind the pass computes what it computed from the same guide bits.

Tolerance against the reference.  The device runs float32; the bound is measured ON THE REFERENCE ALONE, per case: 8 x max
|ref(float32) - ref(float64)| over the pixels of that very case on which both precisions decide alike, floor 2^-20 max(1, |value|).
Pixels on which the device decides differently from the float64 reference (another triangle at some bounce, another class, another
chain length -- read from the device's SURFACE image and from a ptx_trace_rays replay of the reference's own rays), or on which the
two precisions of the reference do, are left out; their share is capped."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import denoise_ref as DR
import specular_guides_ref as SR
import util

W, H = 67, 45
DETAIL = 0.25
EPS32, EPS64 = float(np.finfo(np.float32).eps), float(np.finfo(np.float64).eps)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# =====================================================================================================
# hand-made scenes
# =====================================================================================================
class _Hand:
    """A TriangleSoup with one metallic-roughness material per mesh, and a pinhole camera on it."""

    def __init__(self, pkg, quads, materials, position, direction):
        self.soup = util.TriangleSoup(pkg, [list(quads)])
        self.materials = np.ascontiguousarray(np.stack(materials), np.float32)
        # The default normal texel (128 / 255, 128 / 255, 1) tilts the shading normal by 0.004: a 1 x 1 scene texture holds the flat
        # normal exactly, so that a planar mirror is one to the last bit (and the scene runs the textured variant of the kernel)
        self.texel = np.float32([0.5, 0.5, 1.0, 1.0]).reshape(1, 1, 4)
        self.texture = (pkg.TextureDesc * 1)(pkg.TextureDesc(1, 1, pkg.TEXTURE_RGBA32F, 1, self.texel.ctypes.data))
        self.soup.desc.textures, self.soup.desc.textureCount = C.addressof(self.texture), 1
        self.materials.view(np.uint32)[:, 21] = 9  # the normal slot: the first scene texture
        self.soup.materials = self.materials
        self.soup.meshes["MaterialId"] = np.arange(len(materials), dtype=np.uint32) << 8  # (index << 8) | metallic-roughness
        self.soup.desc.metallicRoughnessMaterials, self.soup.desc.metallicRoughnessMaterialCount = self.materials.ctypes.data, len(materials)
        self.desc = self.soup.desc
        self.cam = pkg.Scene("default", DETAIL)  # lends its camera and its lights
        self.lights = self.cam.lights
        self.pose(position, direction)

    def pose(self, position, direction):
        self.cam.set_camera_pose(position, direction)

    def uniform(self, w=W, h=H, **kw):
        return self.cam.uniform(w, h, **kw)

    def camera_matrices(self, w=W, h=H):
        return self.cam.camera_matrices(w, h)


def _quad(centre, normal, e1, half1, half2=None):
    """A planar quad around `centre`: unit normal, unit in-plane e1 (orthogonal to it), half extents along e1 and normal x e1."""
    n, e1, c = np.float64(normal), np.float64(e1), np.float64(centre)
    n, e1 = n / np.linalg.norm(n), e1 / np.linalg.norm(e1)
    e2 = np.cross(n, e1)
    a, b = e1 * half1, e2 * (half1 if half2 is None else half2)
    return util.quad_mesh([c - a - b, c + a - b, c + a + b, c - a + b], n)


MIRROR_COLOUR, DIFFUSE_COLOUR, GLASS_COLOUR = (0.9, 0.8, 0.7), (0.3, 0.6, 0.5), (0.9, 0.95, 1.0)
DIFFUSE_N = np.float64([0.3, 0.0, -1.0]) / np.linalg.norm([0.3, 0.0, -1.0])
DIFFUSE_C = np.float64([0.0, 0.0, 9.0])
MIRROR_CAMERA = ((0.3, 0.2, 6.0), (0.0, 0.0, -1.0))
MIRROR_EXTENT = 16.0  # no coordinate and no path length of the mirror scene exceeds it


def mirror_scene(pkg, mirror_roughness=0.0):
    """A mirror in the plane z = 0 facing +z, seen from z = 6; behind the camera, at z = 9, a tilted diffuse quad faces it.  Primary
    rays that miss the mirror leave the scene."""
    mirror = _quad((0, 0, 0), (0, 0, 1), (1, 0, 0), 2.0, 1.5)
    diffuse = _quad(DIFFUSE_C, DIFFUSE_N, (1.0, 0.0, 0.3), 7.0)
    return _Hand(pkg, [mirror, diffuse], [util.mr_material(color=MIRROR_COLOUR, roughness=mirror_roughness, metalness=1.0),
                                          util.mr_material(color=DIFFUSE_COLOUR, roughness=0.8)], *MIRROR_CAMERA)


def facing_mirrors_scene(pkg):
    """Two mirrors face each other across z = 0 and z = 8 with the camera between them: no chain ends before the cap."""
    a = _quad((0, 0, 0), (0, 0, 1), (1, 0, 0), 200.0)
    b = _quad((0, 0, 8), (0, 0, -1), (1, 0, 0), 200.0)
    m = util.mr_material(color=(0.9, 0.9, 0.9), roughness=0.0, metalness=1.0)
    return _Hand(pkg, [a, b], [m, m], (0.1, 0.2, 4.0), (0.05, 0.02, -1.0))


def glass_slab_scene(pkg):
    """A slab of glass (Ior 1.5) between z = 0 and z = -1, its faces wound outwards, in front of a diffuse wall at z = -3."""
    front = _quad((0, 0, 0), (0, 0, 1), (1, 0, 0), 30.0)
    back = _quad((0, 0, -1), (0, 0, -1), (1, 0, 0), 30.0)
    wall = _quad((0, 0, -3), (0, 0, 1), (1, 0, 0), 60.0)
    glass = util.mr_material(color=GLASS_COLOUR, roughness=0.0, transmission=1.0, ior=1.5)
    return _Hand(pkg, [front, back, wall], [glass, glass, util.mr_material(color=DIFFUSE_COLOUR, roughness=0.8)], (0.2, 0.1, 4.0), (0.2, 0.1, -1.0))


def sky_mirror_scene(pkg):
    """A mirror tilted up at the sky: its reflection leaves the scene."""
    return _Hand(pkg, [_quad((0, 0, 0), (0, 0.6, 1), (1, 0, 0), 2.0)], [util.mr_material(color=MIRROR_COLOUR, roughness=0.0, metalness=1.0)],
                 (0.0, 0.0, 6.0), (0.0, 0.0, -1.0))


def _ref(orc, scene, max_bounces, roughness_max=0.0, dtype=np.float64, w=W, h=H):
    import debug_view_ref as DV

    rs = DV.RefScene(orc, scene.desc)
    try:
        return SR.render(rs, scene.uniform(w, h), w, h, max_bounces, roughness_max, dtype)
    finally:
        rs.close()


# =====================================================================================================
# without a GPU
# =====================================================================================================
def test_header_declares_and_package_exports_the_specular_pass(pkg):
    header = open(os.path.join(pkg.REPO_DIR, "include", "ptx.h")).read()
    decls = {
        "ptx_render_guides_specular": r"PTX_API int\s+ptx_render_guides_specular\(PtxRenderer \*r, const PtxRaygenUniformData \*uniform, const PtxSpecularGuidesDesc \*desc\);",
        "ptx_read_specular_guide": r"PTX_API int\s+ptx_read_specular_guide\(PtxRenderer \*r, uint32_t which, void \*host, size_t bytes\);",
        "ptx_device_specular_guide_ptr": r"PTX_API void \*ptx_device_specular_guide_ptr\(PtxRenderer \*r, uint32_t which\);",
    }
    lib = pkg.load_hip()
    for name, decl in decls.items():
        assert re.search(decl, header), name
        assert name in pkg.PTX_SYMBOLS
        assert hasattr(lib, name), name
    assert "#define PTX_ABI_VERSION 5u" in header and "PTX_FN_COUNT = 38" in header and "PTX_GUIDE_COUNT = 3" in header  # additions only
    assert re.search(r"PTX_SPECULAR_SURFACE = 0\b", header) and re.search(r"PTX_SPECULAR_COUNT = 1\b", header)
    assert re.search(r"typedef struct PtxSpecularGuidesDesc \{\s*uint32_t maxBounces;[^}]*float\s+roughnessMax;[^}]*uint32_t flags;[^}]*uint32_t reserved;[^}]*\} "
                     r"PtxSpecularGuidesDesc;", header)
    for phrase in ("N_guide", "N_cont", "total internal reflection", "ESCAPED", "BIT-EXACTNESS", "bounces + 16 class"):
        assert phrase in header, phrase
    assert C.sizeof(pkg.SpecularGuidesDesc) == 16 and pkg.SpecularGuidesDesc.roughnessMax.offset == 4 and pkg.SpecularGuidesDesc.reserved.offset == 12
    assert pkg.SPECULAR_SURFACE == 0 == SR.SPECULAR_SURFACE
    for method in ("render_guides_specular", "read_specular_guide", "specular_guide_ptr"):
        assert callable(getattr(pkg.Renderer, method))
    d = pkg.SPECULAR_GUIDES_DEFAULTS
    assert 1 <= d["max_bounces"] <= 8 and 0 <= d["roughness_max"] < 1


def test_reference_planar_mirror_known_answers(pkg, orc):
    """Tolerance: the float64 reference is float64 throughout (it intersects the triangle the oracle names again), and every answer is
    a few dozen float64 operations on values up to the scene's extent: 64 eps64 x the extent for points and lengths, 16 eps64 for the
    unit normal and the colour product.
    One term is the pass's own and is taken out before the geometry is checked: T sums ray PARAMETERS, and the primary direction rd0
    is unit to float32 rounding only, so the first segment enters T as its length / |rd0| (later directions are normalised in the
    working precision).  The geometric path length is T + length1 (1 - 1 / |rd0|)."""
    s = mirror_scene(pkg)
    r = _ref(orc, s, 4)
    one = r["bounces"] == 1
    assert one.sum() > 300 and (r["cls"][one] == SR.CLASS_SURFACE).all() and (r["bounces"] <= 1).all()
    assert (r["tri"][one][:, 0] < 2).all() and (r["tri"][one][:, 1] >= 2).all() and (r["tri"][one][:, 2:] == SR.NO_TRI).all()
    x, T = r["position"][one][:, 0:3], r["position"][one][:, 3]
    n = np.float64(np.float32(DIFFUSE_N))
    n /= np.linalg.norm(n)
    ro, rd0, first = r["origins"][0][one], r["directions"][0][one], r["surface"][one][:, 0:3]
    norm0 = np.linalg.norm(rd0, axis=1)
    assert np.abs(norm0 - 1).max() <= 2 * EPS32 and (np.float64(np.float32(ro)) == ro).all()
    length1 = np.linalg.norm(first - ro, axis=1)
    assert np.abs(x - (ro + rd0 / norm0[:, None] * T[:, None])).max() <= 16 * EPS64 * MIRROR_EXTENT  # the stored point is ro + normalize(rd0) T
    T = T + length1 * (1 - 1 / norm0)  # the geometric length
    x = ro + rd0 / norm0[:, None] * T[:, None]
    unfolded = x * np.float64([1, 1, -1])  # reflected across the mirror's plane z = 0
    # the plane of the very triangle that was hit: the quad's four float32 corners are coplanar to a float32 ulp only
    corners = util.world_triangles(s.desc)[r["tri"][one][:, 1]]
    plane_n = np.cross(corners[:, 1] - corners[:, 0], corners[:, 2] - corners[:, 0])
    plane_n /= np.linalg.norm(plane_n, axis=1, keepdims=True)
    assert np.abs(((unfolded - corners[:, 0]) * plane_n).sum(axis=1)).max() <= 64 * EPS64 * MIRROR_EXTENT
    back = r["normal"][one][:, 0:3] * np.float64([1, 1, -1])
    assert np.abs(back - n).max() <= 16 * EPS64 and (r["normal"][one][:, 3] == 1).all()
    assert np.abs(first[:, 2]).max() <= 16 * EPS64 * MIRROR_EXTENT  # the first hit lies on the mirror
    two_segments = np.linalg.norm(first - ro, axis=1) + np.linalg.norm(unfolded - first, axis=1)
    assert np.abs(T - two_segments).max() <= 64 * EPS64 * MIRROR_EXTENT
    want = np.float64(np.float32(MIRROR_COLOUR)) * np.float64(np.float32(DIFFUSE_COLOUR))
    assert np.abs(r["albedo"][one][:, 0:3] - want).max() <= 16 * EPS64 and (r["albedo"][one][:, 3] == 1).all()
    assert (r["surface"][one][:, 3] == 1).all()
    # a primary miss: the plain pass's miss, and an empty surface word
    miss = ~r["hit"]
    assert miss.sum() > 300 and not r["normal"][miss].any() and not r["position"][miss].any() and (r["albedo"][miss] == 1).all() and not r["surface"][miss].any()
    assert r["segments"] == W * H + int(one.sum())


@pytest.mark.parametrize("cap", [1, 2, 8])
def test_reference_facing_mirrors_stop_at_the_cap(pkg, orc, cap):
    r = _ref(orc, facing_mirrors_scene(pkg), cap)
    assert r["hit"].all() and (r["bounces"] == cap).all() and (r["cls"] == SR.CLASS_CAPPED).all()
    assert (r["surface"][..., 3] == cap + 16).all() and (r["normal"][..., 3] == 1).all()
    assert np.abs(np.abs(r["normal"][..., 2]) - 1).max() <= 16 * EPS64
    # every segment but the first crosses the gap of 8 at the primary ray's slope
    # (the first segment enters T as a ray parameter of the primary direction, which is unit to float32 rounding only: z0 / |dz|)
    d, z0 = r["directions"][0], r["origins"][0][..., 2]
    slope = np.linalg.norm(d, axis=-1) / np.abs(d[..., 2])
    want = z0 / np.abs(d[..., 2]) + slope * 8.0 * cap
    assert np.abs(r["position"][..., 3] - want).max() <= 64 * EPS64 * want.max()  # float64 sums of float64 lengths
    assert np.abs(r["albedo"][..., 0] - np.float64(np.float32(0.9)) ** (cap + 1)).max() <= 16 * EPS64


def test_reference_glass_slab(pkg, orc):
    s = glass_slab_scene(pkg)
    r = _ref(orc, s, 4)
    assert r["hit"].all() and (r["bounces"] == 2).all() and (r["cls"] == SR.CLASS_SURFACE).all()
    d0, d1, d2 = (r["directions"][k] for k in range(3))
    # Snell in float64 with the material's Eta, which the path tracer defines in float32: 1 / 1.5 rounded on the way in, 1.5 on the
    # way out.  The faces are z planes, so refract() scales the tangential part by Eta; the primary direction is refracted as it is
    # traced, unit to float32 rounding only: r = (Eta d0.xy, -sqrt(1 - Eta^2 (1 - d0.z^2))), normalised.  From the unit d1 on the exit
    # is Snell exactly.  So the exit direction is the entry direction up to 1.5 x float32(1 / 1.5) = 1 + 2e-8 and |d0| - 1 = 6e-8:
    # each step to 16 eps64, the round trip to 4 eps32.
    eta_in = np.float64(np.float32(1.0) / np.float32(1.5))
    r1 = np.concatenate([eta_in * d0[..., 0:2], -np.sqrt(1 - eta_in * eta_in * (1 - d0[..., 2:3] ** 2))], axis=-1)
    assert np.abs(d1 - r1 / np.linalg.norm(r1, axis=-1, keepdims=True)).max() <= 16 * EPS64
    assert np.abs(d2[..., 0:2] - 1.5 * d1[..., 0:2]).max() <= 16 * EPS64 and np.abs(np.linalg.norm(d2, axis=-1) - 1).max() <= 16 * EPS64
    assert (d2[..., 2] < 0).all() and np.abs(d2 - d0 / np.linalg.norm(d0, axis=-1, keepdims=True)).max() <= 4 * EPS32
    assert np.abs(r["normal"][..., 0:3] - np.float64([0, 0, 1])).max() <= 16 * EPS64  # refraction does not unfold the normal
    want = np.float64(np.float32(GLASS_COLOUR)) ** 2 * np.float64(np.float32(DIFFUSE_COLOUR))
    assert np.abs(r["albedo"][..., 0:3] - want).max() <= 16 * EPS64
    # inside the slab at a grazing angle: total internal reflection at every face, so the chain runs to the cap and the tint stays 1
    import debug_view_ref as DV

    rs = DV.RefScene(orc, s.desc)
    o = np.float32([[0.0, 0.0, -0.5], [1.0, 2.0, -0.4]])
    d = np.float32([[0.9, 0.1, 0.2], [-0.8, 0.3, -0.25]])
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    off = np.float32([[0.001, 0, 0], [0, 0.001, 0]])
    c = SR.chain(rs, o, d, d + off[0], d + off[1], 3, 0.0, np.float64)
    rs.close()
    assert (c["bounces"] == 3).all() and (c["cls"] == SR.CLASS_CAPPED).all() and (c["tri"] < 4).all() and (c["tri"] >= 0).all()
    assert np.abs(c["albedo"][:, 0:3] - np.float64(np.float32(GLASS_COLOUR))).max() <= 16 * EPS64  # tint 1 x the last face's colour
    assert np.abs(np.abs(c["normal"][:, 2]) - 1).max() <= 16 * EPS64 and np.abs(c["normal"][:, 0:2]).max() <= 16 * EPS64


def test_reference_mirror_facing_the_sky_escapes(pkg, orc):
    r = _ref(orc, sky_mirror_scene(pkg), 4)
    esc = r["hit"]
    assert esc.sum() > 200 and (r["cls"][esc] == SR.CLASS_ESCAPED).all() and (r["bounces"][esc] == 1).all()
    assert not r["normal"][esc].any() and not r["position"][esc].any() and (r["albedo"][esc] == 1).all()  # a miss to every consumer
    assert (r["surface"][esc][:, 3] == 1 + 32).all() and np.abs(r["surface"][esc][:, 0:3]).max() > 0.5
    assert (r["tri"][esc][:, 1] == SR.MISS).all()


def test_reference_roughness_threshold(pkg, orc):
    at = np.float32(0.125)
    above = np.nextafter(at, np.float32(1))
    followed = _ref(orc, mirror_scene(pkg, mirror_roughness=float(at)), 4, roughness_max=float(at))
    stays = _ref(orc, mirror_scene(pkg, mirror_roughness=float(above)), 4, roughness_max=float(at))
    on_mirror = followed["hit"]
    assert on_mirror.sum() > 300 and (followed["bounces"][on_mirror] == 1).all()
    assert (stays["hit"] == on_mirror).all() and (stays["bounces"] == 0).all() and (stays["cls"] == SR.CLASS_SURFACE).all()
    assert np.abs(stays["albedo"][on_mirror][:, 0:3] - np.float64(np.float32(MIRROR_COLOUR))).max() <= 16 * EPS64


@pytest.mark.parametrize("name", ["default", "alpha_test"])
def test_reference_without_bounces_is_the_plain_pass(pkg, orc, name):
    """Normal and position: the float32 reference runs the expressions of tests/debug_view_ref.py, bit for bit.  Albedo: cpu_guides
    takes it from a FLOAT64 run of the debug view on the oracle's float32 hit records (whose footprint, and with it the filtered
    texel, differs from the float32 run's), as (colour x float32(0.1)) / 0.1 rounded to float32: it is compared with this reference's
    float64 run on the same hit records (oracle_hits), from which it differs by the factor 1 + 1.5e-8 and one rounding to float32 on
    either side: 2 ulp."""
    import debug_view_ref as DV

    scene = pkg.Scene(name, DETAIL)
    want = DR.cpu_guides(pkg, orc, scene, W, H)
    rs = DV.RefScene(orc, scene.desc)
    got = SR.render(rs, scene.uniform(W, H), W, H, 0, 0.5, np.float32)
    got64 = SR.render(rs, scene.uniform(W, H), W, H, 0, 0.5, np.float64, oracle_hits=True)
    rs.close()
    hit = got["hit"]
    assert hit.sum() > 500 and (got["bounces"] == 0).all() and (got64["bounces"] == 0).all()
    assert (_bits(got["normal"]) == _bits(want[DR.GUIDE_NORMAL])).all() and (_bits(got["position"]) == _bits(want[DR.GUIDE_POSITION])).all()
    a, b = np.float64(np.float32(got64["albedo"])), np.float64(want[DR.GUIDE_ALBEDO])
    print(f"{name}: albedo differs by at most {float(np.nanmax(np.abs(a - b) / np.maximum(np.abs(b), 1e-30)) / EPS32):.2f} ulp")
    assert (np.abs(a - b) <= 2 * EPS32 * np.abs(b)).all()
    assert (got["surface"][hit][:, 0:3] == got["position"][hit][:, 0:3]).all() and np.isin(got["surface"][hit][:, 3], (0, 16)).all()


# =====================================================================================================
# the cases of the GPU tests, and the reference's own gap on them (no GPU)
# =====================================================================================================
CARD_COLOUR = (1.0, 0.5, 0.5)


def alpha_scene(pkg):
    """The mirror scene with two alpha-tested cards over a 2 x 2 texture (alpha 1 / 0.25): one between the camera and the mirror's
    left half -- where its alpha is low the mirror is seen through it and takes its tint -- and one in front of the reflected
    surface, which the continuation ray meets: the any-hit stage runs on it, and the diffuse quad behind picks up a decal."""
    mirror = _quad((0, 0, 0), (0, 0, 1), (1, 0, 0), 2.0, 1.5)
    diffuse = _quad(DIFFUSE_C, DIFFUSE_N, (1.0, 0.0, 0.3), 7.0)
    near = _quad((-0.7, 0.1, 3.0), (0, 0, 1), (1, 0, 0), 0.8, 0.9)
    far = _quad((0.5, -0.3, 7.5), (0, 0, -1), (1, 0, 0), 2.5, 2.0)
    card = util.mr_material(color=CARD_COLOUR, roughness=0.9)
    s = _Hand(pkg, [mirror, diffuse, near, far], [util.mr_material(color=MIRROR_COLOUR, roughness=0.0, metalness=1.0),
                                                  util.mr_material(color=DIFFUSE_COLOUR, roughness=0.8), card, card], *MIRROR_CAMERA)
    s.card_texels = np.float32([[[0.2, 0.9, 0.4, 1.0], [0.9, 0.3, 0.2, 0.25]], [[0.5, 0.5, 0.9, 0.25], [0.8, 0.8, 0.1, 1.0]]])
    s.texture = (pkg.TextureDesc * 2)(pkg.TextureDesc(1, 1, pkg.TEXTURE_RGBA32F, 1, s.texel.ctypes.data),
                                      pkg.TextureDesc(2, 2, pkg.TEXTURE_RGBA32F, 1, s.card_texels.ctypes.data))
    s.desc.textures, s.desc.textureCount = C.addressof(s.texture), 2
    s.materials.view(np.uint32)[2:4, 20] = 10  # the colour slot of the cards: the second scene texture
    s.soup.geometries["IsOpaque"][2:4] = 0
    return s


class _Case:
    """One scene of the GPU tests with its pass parameters; the references are computed once and shared."""

    def __init__(self, pkg, name):
        self.name = name
        self.pose_state = None
        if name == "mirror":
            self.scene, self.cap, self.rmax = mirror_scene(pkg), 4, 0.0
        elif name == "alpha":
            self.scene, self.cap, self.rmax = alpha_scene(pkg), 4, 0.0
        else:
            detail, self.cap, self.rmax = {"default": (DETAIL, 8, 0.1), "roughness_cubes": (DETAIL, 4, 0.3), "chess_like": (0.1, 2, 0.1),
                                           "animated_test": (DETAIL, 4, 0.3)}[name]
            self.scene = pkg.Scene(name, detail)
            if name == "animated_test":
                assert self.scene.update(0.37)
                self.pose_state = self.scene.animation_state()
        self.refs = {}

    def uniform(self, w=W, h=H):
        return self.scene.uniform(w, h)

    def ref(self, orc, dtype, cap=None, w=W, h=H):
        import debug_view_ref as DV

        cap = self.cap if cap is None else cap
        key = (np.dtype(dtype).name, cap, w, h)
        if key not in self.refs:
            it, bn = self.pose_state if self.pose_state else (None, None)
            rs = DV.RefScene(orc, self.scene.desc, it, bn if bn is not None and len(bn) else None)
            # skinned vertices are the oracle's own float32 block in either precision
            posed = rs.osc.skinned_vertices().astype(dtype) if self.pose_state else None
            self.refs[key] = SR.render(rs, self.uniform(w, h), w, h, cap, self.rmax, dtype, posed)
            rs.close()
        return self.refs[key]

    def gap(self, orc, cap=None, w=W, h=H):
        """(max |ref32 - ref64| per image over the pixels both decide alike, the share of hit pixels they decide differently, that mask)"""
        r32, r64 = self.ref(orc, np.float32, cap, w, h), self.ref(orc, np.float64, cap, w, h)
        differ = SR.decisions_differ(r32, r64) | (r32["hit"] != r64["hit"])
        hit = r64["hit"]
        return SR.max_gap(r32, r64, ~differ), float(differ[hit].sum()) / max(1, int(hit.sum())), differ


CASE_NAMES = ["default", "roughness_cubes", "chess_like", "animated_test", "mirror", "alpha"]
_cases = {}


def _case(pkg, name):
    if name not in _cases:
        _cases[name] = _Case(pkg, name)
    return _cases[name]


# What the tolerance and the cap of the GPU comparison rest on, measured without a GPU at 67 x 45 with each case's parameters and
# recomputed by test_reference_own_gap: max |ref32 - ref64| of (normal, position, albedo, surface) over the pixels on which the two
# precisions decide alike, and the share of hit pixels on which they do not.  The float64 run intersects every hit triangle again, so the
# gap holds the float32 error of the oracle's hit records (on chess_like's small far triangles that error dominates the normal).
REFERENCE_GAP = {
    "default": ((2.324e-07, 2.200e-06, 2.875e-08, 1.518e-06), 0.00000),  # 1845 hit pixels, bounces [1634, 72, 66, 51, 20, 2], classes [1819, 0, 26]
    "roughness_cubes": ((1.475e-07, 2.484e-06, 0.000e+00, 2.384e-06), 0.00000),  # 1256 hit pixels, bounces [1075, 148, 23, 9, 1], classes [1091, 0, 165]
    "chess_like": ((4.082e-03, 5.888e-04, 3.109e-08, 1.328e-05), 0.00000),  # 2626 hit pixels, bounces [2491, 90, 45], classes [2582, 7, 37]
    "animated_test": ((2.007e-06, 2.356e-06, 1.431e-08, 2.356e-06), 0.00000),  # 1767 hit pixels, bounces [1730, 37], classes [1747, 0, 20]
    "mirror": ((3.785e-08, 2.512e-06, 7.153e-09, 6.312e-07), 0.00000),  # 972 hit pixels, bounces [0, 972], classes [972, 0, 0]
    "alpha": ((3.785e-08, 2.512e-06, 2.493e-07, 6.312e-07), 0.00000),  # 1399 hit pixels, bounces [815, 584], classes [1399, 0, 0]
}
REFERENCE_SHARE_LIMIT = 0.005  # the condition on every scene and camera of the GPU tests


@pytest.mark.parametrize("name", CASE_NAMES)
def test_reference_own_gap(pkg, orc, name):
    c = _case(pkg, name)
    gaps, share, differ = c.gap(orc)
    r64 = c.ref(orc, np.float64)
    print(f'    "{name}": (({", ".join("%.3e" % g for g in gaps)}), {share:.5f}),  # {int(r64["hit"].sum())} hit pixels, bounces {np.bincount(r64["bounces"][r64["hit"]]).tolist()}, '
          f'classes {np.bincount(r64["cls"][r64["hit"]], minlength=3).tolist()}')
    assert share <= REFERENCE_SHARE_LIMIT, (name, share)
    assert (r64["bounces"][r64["hit"]] > 0).sum() > 30, "the case must have chains"
    want_gaps, want_share = REFERENCE_GAP[name]
    assert abs(share - want_share) <= 1e-5
    for g, w in zip(gaps, want_gaps):
        assert w / 2 <= g <= 2 * w or (g == 0 and w == 0), (name, gaps)  # the recorded figures, up to the libm of the machine
    if name == "alpha":  # the cards do what they are there for
        first, second = r64["tri"][..., 0], r64["tri"][..., 1]
        assert ((first >= 4) & (first < 6)).sum() > 50, "pixels end on the near card where it is opaque"
        assert (np.abs(r64["albedo"][..., 0:3] - np.float64(np.float32(MIRROR_COLOUR)) * np.float64(np.float32(DIFFUSE_COLOUR))).max(axis=-1)[r64["bounces"] == 1] > 1e-3).sum() > 50
        assert ((second >= 6) & (second < 8)).sum() > 20, "continuation rays end on the far card where it is opaque"
    if name == "chess_like":
        assert (r64["cls"] == SR.CLASS_CAPPED).sum() >= 5
    if name == "roughness_cubes":
        assert (r64["cls"] == SR.CLASS_ESCAPED).sum() > 10


# =====================================================================================================
# on the GPU
# =====================================================================================================
_renderers = {}
SIZES = {"67x45": (67, 45), "1x1": (1, 1), "5x3": (5, 3), "300x200": (300, 200)}
SIZE_CASES = [(n, "67x45") for n in CASE_NAMES] + [("default", s) for s in ("1x1", "5x3", "300x200")]


def _renderer(pkg, name, w=W, h=H):
    """One renderer per case, uploaded once (and posed once); resized where the extent differs."""
    import torch  # noqa: F401  (first, so the HIP library shares torch's HIP runtime)

    c = _case(pkg, name)
    if name not in _renderers:
        r = pkg.Renderer()
        r.upload(c.scene if isinstance(c.scene, pkg.Scene) else c.scene.desc)
        if c.pose_state:
            it, bn = c.pose_state
            r.update_animation(it, bn if len(bn) else None)
        r.resize(W, H)
        _renderers[name] = r
    r = _renderers[name]
    r.set_tile_shard(0, 1, 32)
    if (r.width, r.height) != (w, h):
        r.resize(w, h)
    return c, r


def _plain(r, u):
    r.render_guides(u)
    return [r.read_guide(k) for k in range(3)]


def _specular(r, u, cap, rmax):
    r.render_guides_specular(u, max_bounces=cap, roughness_max=rmax)
    return [r.read_guide(k) for k in range(3)] + [r.read_specular_guide(0)]


def _word(surface):
    """(bounces, class) of the SURFACE image"""
    w = surface[..., 3].astype(np.int64)
    return w % 16, w // 16


@pytest.mark.gpu
@pytest.mark.parametrize("name,size", SIZE_CASES)
def test_zero_bounces_is_the_plain_pass(pkg, name, size):
    w, h = SIZES[size]
    c, r = _renderer(pkg, name, w, h)
    u = c.uniform(w, h)
    plain = _plain(r, u)
    got = _specular(r, u, 0, 0.5)
    for a, b in zip(got, plain):
        assert (_bits(a) == _bits(b)).all()
    hit = plain[0][..., 3] == 1
    b, cls = _word(got[3])
    assert (b == 0).all() and (cls[~hit] == 0).all() and np.isin(cls[hit], (0, 1)).all() and not got[3][~hit].any()
    assert (_bits(got[3][..., 0:3])[hit] == _bits(plain[1][..., 0:3])[hit]).all()
    st = r.stats()
    assert (st.pathSamples, st.segments, st.shadowRays, st.retries) == (w * h, w * h, 0, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("cap", [1, 3, 8])
@pytest.mark.parametrize("name,size", SIZE_CASES)
def test_pixels_without_a_bounce_hold_the_plain_bits(pkg, name, size, cap):
    w, h = SIZES[size]
    c, r = _renderer(pkg, name, w, h)
    u = c.uniform(w, h)
    plain = _plain(r, u)
    got = _specular(r, u, cap, c.rmax)
    b, cls = _word(got[3])
    still = (b == 0) & (cls != SR.CLASS_ESCAPED)
    for a, p in zip(got, plain):
        assert (_bits(a)[still] == _bits(p)[still]).all()
    hit = plain[0][..., 3] == 1
    assert (b[~hit] == 0).all() and (b <= cap).all() and (cls <= 2).all()
    assert ((cls == SR.CLASS_CAPPED) <= (b == cap)).all() and ((cls == SR.CLASS_ESCAPED) <= (b > 0)).all()
    esc = cls == SR.CLASS_ESCAPED
    assert not got[0][esc].any() and not got[1][esc].any() and (got[2][esc] == 1).all()  # a miss to every consumer
    if size == "67x45":
        assert (b > 0).sum() > 30, "the case must have chains"
    # segments = sum over the owned pixels of 1 + bounces, from the device's own image
    st = r.stats()
    assert (st.pathSamples, st.segments, st.shadowRays, st.retries) == (w * h, w * h + int(b.sum()), 0, 0)


def _replay_differs(pkg, c, r, r64):
    """Per pixel: ptx_trace_rays on the float64 reference's own rays names another triangle than the reference at some bounce."""
    out = np.zeros(r64["hit"].shape, bool)
    for k in range(r64["rays"].shape[0]):
        traced = r64["tri"][..., k] != SR.NO_TRI
        if not traced.any():
            break
        hits, ids = r.trace_rays(r64["rays"][k][traced])
        got = util.global_ids(c.scene.desc, ids).astype(np.int64)
        got[hits[:, 3] == 0] = SR.MISS
        out[traced] |= got != r64["tri"][..., k][traced]
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASE_NAMES)
def test_against_float64_reference(pkg, orc, name):
    c, r = _renderer(pkg, name)
    got = _specular(r, c.uniform(), c.cap, c.rmax)
    gaps, ref_share, ref_differ = c.gap(orc)
    r64 = c.ref(orc, np.float64)
    b, cls = _word(got[3])
    dev_hit = (got[0][..., 3] == 1) | (cls == SR.CLASS_ESCAPED)
    differ = ref_differ | (dev_hit != r64["hit"]) | (b != r64["bounces"]) | (cls != r64["cls"]) | _replay_differs(pkg, c, r, r64)
    hit = r64["hit"]
    share = float(differ[hit].sum()) / float(hit.sum())
    print(f"{name}: left out {int(differ[hit].sum())} of {int(hit.sum())} hit pixels ({share:.5f}; the reference alone {ref_share:.5f}), {int((differ & ~hit).sum())} other pixels")
    keep = ~differ
    worst = []
    for which, (a, ref, gap) in enumerate(zip(got, SR.images(r64), gaps)):
        err = np.abs(a.astype(np.float64) - ref)
        worst.append(float(err[keep].max()))
        print(f"{name} image {which}: max |gpu - ref64| {worst[-1]:.3e}, max |ref32 - ref64| of the case {gap:.3e}")
    assert share <= min(4 * ref_share, 0.02), (name, share, ref_share)
    for which, (a, ref, gap) in enumerate(zip(got, SR.images(r64), gaps)):
        tol = np.maximum(8.0 * gap, 2.0 ** -20 * np.maximum(1.0, np.abs(ref)))
        assert (np.abs(a.astype(np.float64) - ref)[keep] <= tol[keep]).all(), (name, which, worst[which], gap)
    st = r.stats()
    if not differ.any():
        assert st.segments == r64["segments"]


@pytest.mark.gpu
def test_planar_mirror_properties_on_the_device(pkg):
    """The statements of test_reference_planar_mirror_known_answers on the device's float32 images.  Bounds: the unfolded point and T
    come out of some ten dependent float32 operations on values up to the scene's extent, each half an ulp of it: 16 eps32 x extent on
    top of the reference's 16; the unit normal and the colour product are a few roundings of values below 1: 8 eps32."""
    c, r = _renderer(pkg, "mirror")
    nrm, pos, alb, srf = _specular(r, c.uniform(), 4, 0.0)
    b, cls = _word(srf)
    one = b == 1
    assert one.sum() > 300 and (cls[one] == SR.CLASS_SURFACE).all() and (b <= 1).all()
    n = np.float64(np.float32(DIFFUSE_N))
    n /= np.linalg.norm(n)
    x, T = np.float64(pos[one][:, 0:3]), np.float64(pos[one][:, 3])
    unfolded = x * np.float64([1, 1, -1])
    assert np.abs((unfolded - DIFFUSE_C) @ n).max() <= 32 * EPS32 * MIRROR_EXTENT
    assert np.abs(np.float64(nrm[one][:, 0:3]) * np.float64([1, 1, -1]) - n).max() <= 8 * EPS32 and (nrm[one][:, 3] == 1).all()
    first = np.float64(srf[one][:, 0:3])
    assert np.abs(first[:, 2]).max() <= 32 * EPS32 * MIRROR_EXTENT
    two_segments = np.linalg.norm(first - np.float64(np.float32(MIRROR_CAMERA[0])), axis=1) + np.linalg.norm(unfolded - first, axis=1)
    assert np.abs(T - two_segments).max() <= 32 * EPS32 * MIRROR_EXTENT
    want = np.float64(np.float32(MIRROR_COLOUR)) * np.float64(np.float32(DIFFUSE_COLOUR))
    assert np.abs(np.float64(alb[one][:, 0:3]) - want).max() <= 8 * EPS32 and (alb[one][:, 3] == 1).all()


@pytest.mark.gpu
@pytest.mark.parametrize("world", [2, 3])
def test_tile_shards_write_their_own_pixels(pkg, world):
    c, r = _renderer(pkg, "default")
    u = c.uniform()
    whole = _specular(r, u, c.cap, c.rmax)
    wb, _ = _word(whole[3])
    fresh = pkg.Renderer()
    fresh.share_scene(r)
    fresh.resize(W, H)
    union = [np.zeros((H, W, 4), np.float32) for _ in range(4)]
    seen = np.zeros((H, W), bool)
    for rank in range(world):
        # a handle that has rendered nothing yet: what a rank does not own stays all zeros
        one = pkg.Renderer()
        one.share_scene(r)
        one.resize(W, H)
        one.set_tile_shard(rank, world, 16)
        part = _specular(one, u, c.cap, c.rmax)
        own = pkg.shard_mask(W, H, rank, world, 16)
        st = one.stats()
        assert (st.pathSamples, st.segments) == (own.sum(), own.sum() + int(wb[own].sum()))
        for k in range(4):
            assert not part[k][~own].any()
            assert (_bits(part[k])[own] == _bits(whole[k])[own]).all()
            union[k][own] = part[k][own]
        one.close()
        assert not (seen & own).any()
        seen |= own
        # ... and on a handle that holds a whole frame the others keep what they held
        fresh.set_tile_shard(0, 1, 32)
        before = _specular(fresh, u, 0, 0.0)
        fresh.set_tile_shard(rank, world, 16)
        after = _specular(fresh, u, c.cap, c.rmax)
        for k in range(4):
            assert (_bits(after[k])[~own] == _bits(before[k])[~own]).all() and (_bits(after[k])[own] == _bits(whole[k])[own]).all()
    fresh.close()
    assert seen.all()
    for k in range(4):
        assert (_bits(union[k]) == _bits(whole[k])).all()


TD = dict(max_history=3.0, normal_threshold=0.3, position_threshold=0.03)


def _check_temporal(frames, got, label):
    """tests/test_temporal.py's comparison with temporal_ref: its tolerance, its caps, and its accumulation parameters, which are this file's"""
    import test_temporal as TT

    assert TT.TD == TD
    return TT._check_against_reference(frames, got, label)


def _frame(c, r, f, cap, rmax):
    """One 1-spp frame at the scene's current pose: (S, the device's guides, 1, view, proj, 0) as temporal_ref takes it, the surface image"""
    u = c.scene.uniform(W, H, bounces=4, sample_count=1, total_samples=f)
    r.reset()
    r.render(u, c.scene.lights)
    S = r.readback()
    g = _specular(r, u, cap, rmax)
    view, proj = c.scene.camera_matrices(W, H)
    return (S, g[0], g[1], g[2], 1, view, proj, 0), g[3]


@pytest.mark.gpu
def test_downstream_is_untouched(pkg):
    """With maxBounces = 0 the guides are the plain pass's bits, so every stage behind computes the plain chain's bits; after a real
    pass the filter and the accumulation are the references' on the device's own guides; the accumulation and the next ptx_render
    never notice."""
    c, r = _renderer(pkg, "default")
    lights = c.scene.lights
    up = c.scene.uniform(W, H, bounces=4)

    def chain_outputs(handle, guides):
        handle.reset()
        for f in range(2):
            up.TotalSamples = f
            handle.render(up, lights)
        S = handle.readback()
        guides(handle)
        view, proj = c.scene.camera_matrices(W, H)
        out = {"S": S}
        handle.denoise(2)
        out["denoise"] = handle.read_denoised()
        handle.temporal_accumulate(2, view, proj, **TD)
        out["temporal"] = handle.read_temporal()
        handle.temporal_accumulate_moments(2, view, proj, **TD)
        handle.denoise_variance()
        out["variance"] = handle.read_denoised()
        out["after"] = handle.readback()
        up.TotalSamples = 2
        handle.render(up, lights)
        out["next"] = handle.readback()
        return out

    u = c.uniform()
    other = pkg.Renderer()
    other.share_scene(r)
    other.resize(W, H)
    plain = chain_outputs(other, lambda h: h.render_guides(u))
    other.close()
    r.resize(W, H)  # a fresh chain
    zero = chain_outputs(r, lambda h: h.render_guides_specular(u, max_bounces=0, roughness_max=0.1))
    for k in plain:
        assert (_bits(plain[k]) == _bits(zero[k])).all(), k
    r.resize(W, H)
    real = chain_outputs(r, lambda h: h.render_guides_specular(u, max_bounces=c.cap, roughness_max=c.rmax))
    for k in ("S", "after", "next"):
        assert (_bits(plain[k]) == _bits(real[k])).all(), k  # the accumulation and the next ptx_render are a handle's that never ran the pass
    assert (_bits(real["denoise"]) != _bits(plain["denoise"])).any()
    g = [r.read_guide(k) for k in range(3)]
    d = pkg.DENOISE_DEFAULTS
    args = (real["S"], *g, 2, d["iterations"], d["sigma_color"], d["sigma_normal"], d["sigma_position"])
    d32, d64 = DR.denoise(*args, np.float32), DR.denoise(*args, np.float64)
    fin = np.isfinite(d64)
    gap = float(np.abs(d32.astype(np.float64) - d64)[fin].max())
    tol = np.maximum(8.0 * gap, 2.0 ** -20 * np.maximum(1.0, np.abs(d64)))
    print(f"filter after the specular pass: max |gpu - ref64| {np.abs(real['denoise'].astype(np.float64) - d64)[fin].max():.3e}, max |ref32 - ref64| {gap:.3e}")
    assert (np.abs(real["denoise"].astype(np.float64) - d64)[fin] <= tol[fin]).all()
    view, proj = c.scene.camera_matrices(W, H)
    _check_temporal([(real["S"], *g, 2, view, proj, 0)], [real["temporal"]], "accumulation after the specular pass")


@pytest.mark.gpu
def test_reflections_keep_their_history_under_a_pan(pkg, orc):
    """Three 1-spp frames of the mirror scene under a sideways move that shifts the mirror's image by about a pixel (1.37 across and,
    so that the reprojected rows do not land on pixel centres where floor() is a coin toss between two precisions, 0.31 up): the virtual point
    is fixed in the world, so the history is found, and a pixel that showed the reflection in all three frames (and whose taps did:
    two pixels inside the mirror's outline) has the full history, 3 -- up to the rounding of the length's weighted mean, 4 eps32 x 3.
    T is temporal_ref's on the device's own guides, within test_temporal's tolerances."""
    import debug_view_ref as DV

    c, r = _renderer(pkg, "mirror")
    r.resize(W, H)
    o, d, _, _ = DV.primary_rays(orc, c.uniform(), W, H)
    dn = d / np.linalg.norm(d, axis=1, keepdims=True)
    mid = (H // 2) * W + W // 2
    step = float(np.arccos(np.clip(dn[mid] @ dn[mid + 1], -1, 1))) * 6.0  # one pixel at the mirror's distance
    frames, surfaces, got = [], [], []
    try:
        for f in range(3):
            p = MIRROR_CAMERA[0]
            c.scene.pose((p[0] + f * 1.37 * step, p[1] + f * 0.31 * step, p[2]), MIRROR_CAMERA[1])
            frame, srf = _frame(c, r, f, 4, 0.0)
            frames.append(frame)
            surfaces.append(srf)
            view, proj = frame[5], frame[6]
            r.temporal_accumulate(1, view, proj, **TD)
            got.append(r.read_temporal())
    finally:
        c.scene.pose(*MIRROR_CAMERA)
    _check_temporal(frames, got, "mirror pan")
    inner = np.ones((H, W), bool)
    for srf in surfaces:
        m = _word(srf)[0] == 1
        e = m.copy()
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                sh = np.zeros_like(m)
                sh[max(0, dy):H + min(0, dy), max(0, dx):W + min(0, dx)] = m[max(0, -dy):H + min(0, -dy), max(0, -dx):W + min(0, -dx)]
                e &= sh
        inner &= e
    L = got[2][..., 3]
    print(f"mirror pan of {step:.4f}: {int(inner.sum())} pixels inside the mirror in all three frames, history {L[inner].min():.6f} .. {L[inner].max():.6f}")
    assert inner.sum() > 200
    assert np.abs(L[inner] - 3.0).max() <= 4 * EPS32 * 3


@pytest.mark.gpu
def test_borrower_pending_textures_resize_and_motion(pkg):
    c, r = _renderer(pkg, "default")
    u = c.uniform()
    whole = _specular(r, u, c.cap, c.rmax)
    assert r.specular_guide_ptr(0) and not r.specular_guide_ptr(1)
    # a borrower renders its owner's scene
    b = pkg.Renderer()
    b.share_scene(r)
    b.resize(W, H)
    for a, w in zip(_specular(b, u, c.cap, c.rmax), whole):
        assert (_bits(a) == _bits(w)).all()
    # ptx_resize drops the fourth image with the guides
    buf = np.zeros((H, W, 4), np.float32)
    b.resize(W, H)
    assert b.lib.ptx_read_specular_guide(b.handle, 0, buf.ctypes.data, buf.nbytes) == 5 and not b.specular_guide_ptr(0)
    assert b.lib.ptx_read_guide(b.handle, 0, buf.ctypes.data, buf.nbytes) == 5
    b.render_guides(u)  # a plain pass brings the three guides back, not the fourth image
    assert b.lib.ptx_read_specular_guide(b.handle, 0, buf.ctypes.data, buf.nbytes) == 5 and b.lib.ptx_read_guide(b.handle, 0, buf.ctypes.data, buf.nbytes) == 0
    b.close()
    # pending streamed textures sample their stand-ins: the pass on the scene without its textures (materials_test: textured, with
    # mirrors and glass, every metal or glass followed)
    s = pkg.Scene("materials_test", DETAIL)
    u, cap, rmax = s.uniform(W, H), 4, 1.0
    t = pkg.Renderer()
    t.upload(s)
    t.resize(W, H)
    textured = _specular(t, u, cap, rmax)
    t.close()
    assert (_word(textured[3])[0] > 0).sum() > 100
    d = pkg.SceneDesc()
    C.memmove(C.byref(d), C.byref(s.desc), C.sizeof(d))
    tex = (pkg.TextureDesc * d.textureCount).from_address(d.textures)
    pending = (pkg.TextureDesc * d.textureCount)(*[pkg.TextureDesc(t.width, t.height, t.format, t.levels, None) for t in tex])
    d.textures = C.addressof(pending)
    p = pkg.Renderer()
    p.upload_streamed(d)
    p.resize(W, H)
    got = _specular(p, u, cap, rmax)
    p.close()
    none = pkg.SceneDesc()
    C.memmove(C.byref(none), C.byref(s.desc), C.sizeof(none))
    none.textures, none.textureCount = None, 0
    q = pkg.Renderer()
    q.upload(none)
    q.resize(W, H)
    for a, w in zip(got, _specular(q, u, cap, rmax)):
        assert (_bits(a) == _bits(w)).all()
    q.close()
    assert (_bits(got[2]) != _bits(textured[2])).any()


@pytest.mark.gpu
def test_motion_accumulate_after_a_specular_pass_as_after_a_plain_one(pkg):
    """To the chain the pass is a plain guide pass: the motion images go stale, and ptx_temporal_accumulate_motion answers as it does
    after ptx_render_guides; a motion pass afterwards makes them fresh again."""
    c, r = _renderer(pkg, "animated_test")
    u = c.uniform()
    r.track_motion(True)
    r.resize(W, H)
    view, proj = c.scene.camera_matrices(W, H)
    desc = r._temporal_desc(1, view, proj, TD["max_history"], TD["normal_threshold"], TD["position_threshold"], 0)
    lib = r.lib
    r.render_guides_motion(u)
    assert lib.ptx_temporal_accumulate_motion(r.handle, C.byref(desc), 0) == 0
    r.render_guides(u)
    after_plain = lib.ptx_temporal_accumulate_motion(r.handle, C.byref(desc), 0)
    message = r.last_error() if hasattr(r, "last_error") else None
    r.render_guides_motion(u)
    assert lib.ptx_temporal_accumulate_motion(r.handle, C.byref(desc), 0) == 0
    r.render_guides_specular(u, max_bounces=4, roughness_max=0.3)
    after_specular = lib.ptx_temporal_accumulate_motion(r.handle, C.byref(desc), 0)
    assert after_plain == after_specular == 5
    if message is not None:
        assert r.last_error() == message
    buf = np.zeros((H, W, 4), np.float32)
    assert lib.ptx_read_motion(r.handle, 0, buf.ctypes.data, buf.nbytes) == 5  # stale, as after a plain pass
    r.render_guides_motion(u)
    assert lib.ptx_temporal_accumulate_motion(r.handle, C.byref(desc), 0) == 0
    r.track_motion(False)


@pytest.mark.gpu
def test_specular_pass_refusals(pkg):
    import torch

    c, r = _renderer(pkg, "default")
    u = c.uniform()
    lib = r.lib
    buf = np.zeros((H, W, 4), np.float32)
    D = pkg.SpecularGuidesDesc
    good = D(4, 0.1, 0, 0)
    fresh = pkg.Renderer()
    assert lib.ptx_render_guides_specular(fresh.handle, C.byref(u), C.byref(good)) == 5  # no scene, no tree, no image
    fresh.resize(W, H)
    assert lib.ptx_render_guides_specular(fresh.handle, C.byref(u), C.byref(good)) == 5
    assert lib.ptx_read_specular_guide(fresh.handle, 0, buf.ctypes.data, buf.nbytes) == 5 and not lib.ptx_device_specular_guide_ptr(fresh.handle, 0)
    fresh.close()
    r.resize(W, H)  # drops the images of earlier tests
    assert lib.ptx_read_specular_guide(r.handle, 0, buf.ctypes.data, buf.nbytes) == 5
    r.render_guides(u)
    assert lib.ptx_read_specular_guide(r.handle, 0, buf.ctypes.data, buf.nbytes) == 5  # a plain pass brings no fourth image
    held = _specular(r, u, 4, 0.1)
    view, proj = c.scene.camera_matrices(W, H)
    r.temporal_accumulate(1, view, proj, **TD)
    T = r.read_temporal()

    def intact():
        got = [r.read_guide(k) for k in range(3)] + [r.read_specular_guide(0)]
        return all((_bits(a) == _bits(b)).all() for a, b in zip(got, held)) and (_bits(r.read_temporal()) == _bits(T)).all() and bool(r.specular_guide_ptr(0))

    nan, inf = float("nan"), float("inf")
    for bad in (D(9, 0.1, 0, 0), D(0xFFFFFFFF, 0.1, 0, 0), D(4, -0.001, 0, 0), D(4, nan, 0, 0), D(4, inf, 0, 0), D(4, -inf, 0, 0), D(4, 0.1, 1, 0), D(4, 0.1, 0, 1)):
        assert lib.ptx_render_guides_specular(r.handle, C.byref(u), C.byref(bad)) == 1, (bad.maxBounces, bad.roughnessMax, bad.flags, bad.reserved)
        assert intact()
    assert lib.ptx_render_guides_specular(r.handle, C.byref(u), None) == 1 and lib.ptx_render_guides_specular(r.handle, None, C.byref(good)) == 1
    assert lib.ptx_render_guides_specular(None, C.byref(u), C.byref(good)) == 1 and intact()
    shard = torch.zeros(r.shard_bytes(0) // 4, dtype=torch.float32, device="cuda")
    r.bind_shard_accumulation(shard.data_ptr(), shard.numel() * 4)
    assert lib.ptx_render_guides_specular(r.handle, C.byref(u), C.byref(good)) == 5
    r.bind_shard_accumulation(0)
    assert intact()
    assert lib.ptx_read_specular_guide(r.handle, 1, buf.ctypes.data, buf.nbytes) == 1 and lib.ptx_read_specular_guide(r.handle, 0, None, buf.nbytes) == 1
    assert lib.ptx_read_specular_guide(r.handle, 0, buf.ctypes.data, buf.nbytes - 16) == 1 and not buf.any()
    assert lib.ptx_read_guide(r.handle, 3, buf.ctypes.data, buf.nbytes) == 1 and not lib.ptx_device_guide_ptr(r.handle, 3)  # the old pair keeps refusing it
    assert lib.ptx_read_specular_guide(r.handle, 0, buf.ctypes.data, buf.nbytes) == 0 and buf.any()
    # the accepted limits
    for ok in (D(8, 0.0, 0, 0), D(0, 3.0e38, 0, 0)):
        assert lib.ptx_render_guides_specular(r.handle, C.byref(u), C.byref(ok)) == 0


# =====================================================================================================
# quality, without a GPU
# =====================================================================================================
# tools/specular_guides_quality.py at SPECULAR_GUIDES_DEFAULTS on `default`, 134 x 90: the relative L2 error against the committed
# truths on the 850 pixels with bounces > 0, (first-hit guides, specular guides).  The spatial chain gains; the temporal + filter chain
# LOSES a little (docs/NEXT_ROWS.md section 18 discusses why): a finding about the method, asserted in the direction it was measured.
QUALITY_SPATIAL = (0.3984, 0.2135)
QUALITY_TEMPORAL = (0.2486, 0.2527)


def test_quality_on_the_pixels_with_chains(pkg, orc):
    import importlib.util

    spec = importlib.util.spec_from_file_location("specular_guides_quality", os.path.join(pkg.REPO_DIR, "tools", "specular_guides_quality.py"))
    Q = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(Q)
    d = pkg.SPECULAR_GUIDES_DEFAULTS
    for label, case, want in (("spatial", Q.spatial_case, QUALITY_SPATIAL), ("temporal + filter", Q.temporal_case, QUALITY_TEMPORAL)):
        first, specular, truth, chains = case(pkg, orc, d["max_bounces"], d["roughness_max"])
        got = (Q.relative_l2(first, truth, chains), Q.relative_l2(specular, truth, chains))
        print(f"{label}: {int(chains.sum())} pixels with bounces > 0, relative L2 error {got[0]:.4f} with first-hit guides, {got[1]:.4f} with specular guides; "
              f"all pixels {Q.relative_l2(first, truth):.4f} -> {Q.relative_l2(specular, truth):.4f}")
        assert chains.sum() > 500 and np.isfinite(specular).all()
        assert abs(got[0] - want[0]) <= 0.002 and abs(got[1] - want[1]) <= 0.002, (label, got)  # the recorded figures, to the table's digits
        assert (got[1] < got[0]) == (want[1] < want[0]), (label, got)  # the direction that was measured
    assert QUALITY_SPATIAL[1] < QUALITY_SPATIAL[0] and QUALITY_TEMPORAL[1] > QUALITY_TEMPORAL[0]
