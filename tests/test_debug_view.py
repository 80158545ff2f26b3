"""Row D16: the debug view (include/ptx.h ptx_render_debug, csrc/pt_debug_view.hpp) against tests/debug_view_ref.py.

Tolerance.  The hit (t, u, v, triangle) is the same bits on both sides by the project's standing parity; what differs is float32
evaluation order in arithmetic no fixture pins.  The bound is therefore measured ON THE REFERENCE ALONE: per mode and scene
tol = 8 x max |ref(float32) - ref(float64)| over the image, with a floor of 2^-20 max(1, |value|).  The maxima are the constants
REF_F32_VS_F64 below, printed by

    python tests/test_debug_view.py

and test_reference_float32_against_float64 recomputes them without a GPU."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

import debug_view_ref as R
import util

W, H = 67, 45  # the last block of the launch is partial, the last tiles ragged
DETAIL = 0.25
NO_SHADOWS = R.HIT_DISABLE_SHADOWS

# (scene, mode, hit group flags) -> max |ref(float32) - ref(float64)| over the 67 x 45 image
REF_F32_VS_F64 = {
    ('texture_test', 1, 0): 4.917e-07,
    ('texture_test', 2, 0): 6.459e-07,
    ('texture_test', 3, 0): 6.007e-07,
    ('texture_test', 4, 0): 1.379e-06,
    ('materials_test', 1, 0): 4.926e-07,
    ('materials_test', 2, 0): 4.368e-06,
    ('materials_test', 3, 0): 4.519e-07,
    ('materials_test', 4, 0): 1.142e-06,
    ('default', 1, 0): 3.776e-07,
    ('default', 2, 0): 6.168e-08,
    ('default', 3, 0): 8.382e-08,
    ('default', 4, 0): 7.215e-07,
    ('texture_test', 0, 8): 2.688e-05,
    ('materials_test', 0, 8): 5.974e-02,
    ('alpha_test', 0, 8): 5.157e-06,
    ('reuse_mesh_cubes', 0, 8): 3.010e-07,
    ('roughness_cubes', 0, 8): 5.352e-07,
    ('default', 0, 0): 2.235e-08,
    ('alpha_test', 0, 0): 1.399e-03,
}
# the image cases of the GPU tests
VALUE_CASES = [(s, m, 0) for s in ("texture_test", "materials_test", "default")
               for m in (R.MODE_WORLD_POSITION, R.MODE_NORMAL, R.MODE_TEXTURE_COORDS, R.MODE_MIPS)]
COLOR_CASES = [(s, R.MODE_COLOR, NO_SHADOWS) for s in ("texture_test", "materials_test", "alpha_test", "reuse_mesh_cubes", "roughness_cubes")]
SHADOW_CASES = [(s, R.MODE_COLOR, 0) for s in ("default", "alpha_test")]
ALL_CASES = VALUE_CASES + COLOR_CASES + SHADOW_CASES

_scenes, _refs = {}, {}


def _scene(pkg, orc, name):
    if name not in _scenes:
        s = pkg.Scene(name, DETAIL)
        _scenes[name] = (s, R.RefScene(orc, s.desc), s.uniform(W, H), s.lights)
    return _scenes[name]


def _ref(pkg, orc, name, mode, flags, dtype):
    """Computed once, shared and left unchanged."""
    key = (name, mode, flags, np.dtype(dtype).name)
    if key not in _refs:
        s, rs, u, lights = _scene(pkg, orc, name)
        _refs[key] = R.render(rs, u, lights, W, H, mode, flags, dtype)
        _refs[key]["image"].setflags(write=False)
    return _refs[key]


def _measure(pkg, orc, case):
    a, b = _ref(pkg, orc, *case, np.float32), _ref(pkg, orc, *case, np.float64)
    with np.errstate(all="ignore"):
        d = np.abs(a["image"].astype(np.float64) - b["image"])
    return float(np.max(np.where(np.isfinite(d), d, 0.0)))


def _tol(pkg, orc, case):
    b = _ref(pkg, orc, *case, np.float64)["image"]
    return np.maximum(8.0 * REF_F32_VS_F64[case], 2.0 ** -20 * np.maximum(1.0, np.abs(b)))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# =====================================================================================================
# without a GPU
# =====================================================================================================
def test_header_declares_and_package_exports_the_debug_view(pkg):
    header = open(os.path.join(pkg.REPO_DIR, "include", "ptx.h")).read()
    for name, args in (("ptx_render_debug", r"PtxRenderer \*r, const PtxRaygenUniformData \*uniform, const PtxLightsUbo \*lights, const PtxDebugViewDesc \*view"),
                       ("ptx_test_debug_eval", r"PtxRenderer \*r, uint32_t which, const float \*in, float \*out, uint32_t n")):
        assert re.search(r"PTX_API int " + name + r"\(" + args + r"\);", header), name
        assert name in pkg.PTX_SYMBOLS
        assert hasattr(pkg.load_hip(), name), name
    assert "#define PTX_ABI_VERSION 5u" in header and "PTX_FN_COUNT = 38" in header  # additions only
    assert re.search(r"typedef struct PtxDebugViewDesc \{\s*uint32_t renderMode;[^}]*uint32_t raygenFlags;[^}]*uint32_t hitGroupFlags;[^}]*uint32_t reserved;[^}]*\} PtxDebugViewDesc;", header)
    for k, name in enumerate(("COLOR", "WORLD_POSITION", "NORMAL", "TEXTURE_COORDS", "MIPS", "GEOMETRY", "PRIMITIVE", "INSTANCE")):
        assert re.search(r"PTX_DEBUG_MODE_%s = %d\b" % (name, k), header), name
        assert getattr(pkg, "DEBUG_MODE_" + name) == k
    for name, v in (("RAYGEN_FORCE_OPAQUE", 1), ("RAYGEN_CULL_BACK_FACES", 2), ("HIT_DISABLE_COLOR_TEXTURE", 1), ("HIT_DISABLE_NORMAL_TEXTURE", 2),
                    ("HIT_DISABLE_MIP_MAPS", 4), ("HIT_DISABLE_SHADOWS", 8)):
        assert re.search(r"PTX_DEBUG_%s = %du" % (name, v), header), name
        assert getattr(pkg, "DEBUG_" + name) == v
    assert C.sizeof(pkg.DebugViewDesc) == 16
    for method in ("render_debug", "test_debug_eval"):
        assert callable(getattr(pkg.Renderer, method))
    host = open(os.path.join(pkg.PKG_DIR, "host", "RendererHip.h")).read()
    assert "SetDebugRaytracingPipeline(uint32_t renderMode" in host and "SetPathTracingPipeline()" in host


HASH_KNOWN_ANSWERS = {  # x -> hash, r, g, b (float bits); rcp(255) = 0x3b808081
    0: (0x10AFE506, 0x3D808081, 0x3F2FAFB0, 0x3F65E5E7),
    1: (0x969E1BA8, 0x3F169697, 0x3F1E9E9F, 0x3DD8D8DA),
    2: (0x1C8C3169, 0x3DE0E0E2, 0x3F0C8C8D, 0x3E44C4C6),
    1000: (0xCF6C1480, 0x3F4FCFD1, 0x3ED8D8DA, 0x3DA0A0A1),
}


def test_hash_known_answers():
    assert (np.float32(1.0) / np.float32(255.0)).view(np.uint32) == 0x3B808081
    for x, (h, r, g, b) in HASH_KNOWN_ANSWERS.items():
        assert int(R.hash_u32([x])[0]) == h
        assert [int(v) for v in _bits(R.random_color([x]))[0]] == [r, g, b]


def test_reference_float32_against_float64(pkg, orc):
    """The measured maxima behind every tolerance have not more than doubled, and the shadow-edge rule holds for the reference's own two
    instances: with shadows a pixel beyond the bound lies at an occlusion edge, and such pixels are at most 1 % of the hit pixels."""
    assert set(REF_F32_VS_F64) == set(ALL_CASES)
    for case in ALL_CASES:
        got = _measure(pkg, orc, case)
        assert got <= 2.0 * REF_F32_VS_F64[case], (case, got, REF_F32_VS_F64[case])
    for case in SHADOW_CASES:
        a, b = _ref(pkg, orc, *case, np.float32), _ref(pkg, orc, *case, np.float64)
        beyond = (np.abs(a["image"].astype(np.float64) - b["image"]) > _tol(pkg, orc, case)).any(axis=-1)
        assert not (beyond & ~R.shadow_edge_mask(b)).any(), case
        assert int(beyond.sum()) * 100 <= int(b["hit"].sum()), case
        assert b["occluded"].any() and not b["occluded"][:, b["hit"]].all(), "the scene must have lit and shadowed pixels"


def test_reference_light_model_limits():
    """debugClosestHit.rchit:111-141 at points with known values: a metal has no diffuse term; light from behind contributes nothing."""
    N = np.float64([[0, 0, 1]])
    up = R.light_contribution(np.float64([[0, 0, -1]]), np.ones((1, 3)), np.ones(1), N, N, np.float64([[0.5, 0.25, 1.0]]), np.float64([1.0]), np.float64([0.0]), np.float64)
    # head-on, roughness 1, dielectric: NDF = 1 / pi, G = 1, F = 0.04 -> (0.96 c / pi + 0.04 / (4 pi))
    assert np.allclose(up[0], 0.96 * np.float64([0.5, 0.25, 1.0]) / R.PI + 0.01 / R.PI, rtol=1e-6)
    back = R.light_contribution(np.float64([[0, 0, 1]]), np.ones((1, 3)), np.ones(1), np.float64([[0.6, 0, 0.8]]), N, np.ones((1, 3)), np.float64([0.5]), np.float64([0.0]), np.float64)
    assert (back == 0).all()


# =====================================================================================================
# on the GPU
# =====================================================================================================
_renderers = {}


def _renderer(pkg, orc, name):
    """One renderer per scene, uploaded once."""
    import torch  # noqa: F401  (first, so the HIP library shares torch's HIP runtime)

    if name not in _renderers:
        r = pkg.Renderer()
        r.upload(_scene(pkg, orc, name)[0])
        r.resize(W, H)
        _renderers[name] = r
    return _renderers[name]


def _debug(pkg, orc, name, mode, raygen=0, hit=0, lights=None):
    s, rs, u, sl = _scene(pkg, orc, name)
    r = _renderer(pkg, orc, name)
    r.render_debug(u, sl if lights is None else lights, mode, raygen, hit)
    return r.readback()


def _light_inputs():
    rng = np.random.default_rng(16)
    n = 20000
    unit = lambda x: x / np.linalg.norm(x, axis=1, keepdims=True)  # noqa: E731
    inp = np.zeros((n, 18), np.float32)
    inp[:, 0:3] = rng.normal(size=(n, 3)) * rng.uniform(0.1, 10.0, (n, 1))
    inp[:, 3:6] = rng.uniform(0.0, 5.0, (n, 3))
    inp[:, 6] = rng.uniform(0.0, 1.0, n)
    N = unit(rng.normal(size=(n, 3)))
    V = unit(rng.normal(size=(n, 3)))
    # grazing N.V and N.L: V, the light direction, or both nearly in the tangent plane
    g = np.arange(n) % 8
    tang = unit(np.cross(N, rng.normal(size=(n, 3))))
    eps = rng.uniform(-1e-3, 1e-3, (n, 1))
    V = np.where((g == 1)[:, None] | (g == 3)[:, None], unit(tang + eps * N), V)
    inp[:, 0:3] = np.where((g == 2)[:, None] | (g == 3)[:, None], -unit(np.cross(N, tang) + eps * N) * 3.0, inp[:, 0:3])
    inp[:, 7:10], inp[:, 10:13] = V, N
    inp[:, 13:16] = rng.uniform(0.0, 1.0, (n, 3))
    inp[:, 16] = rng.uniform(0.0, 1.0, n)
    inp[::11, 16] = 0.0
    inp[5::11, 16] = 1.0
    inp[:, 17] = rng.choice(np.float32([0.0, 0.5, 1.0]), n)
    inp[0, 0:3], inp[0, 7:10], inp[0, 10:13] = (0, 0, 2), (0, 0, 1), (0, 0, 1)  # V = -L: H = normalize(0)
    inp[1, 0:3] = 0.0                                                         # no light direction at all
    return inp


@pytest.mark.gpu
def test_debug_eval(pkg, gpu_renderer):
    ids = np.concatenate([np.uint32([0, 1, 2, 1000, 0xFFFFFFFF]), np.random.default_rng(5).integers(0, 1 << 32, 4091, dtype=np.uint64).astype(np.uint32)])
    got = gpu_renderer.test_debug_eval(pkg.DEBUG_EVAL_RANDOM_COLOR, ids)
    assert (got == _bits(R.random_color(ids))).all()
    for k, x in enumerate((0, 1, 2, 1000)):
        assert [int(v) for v in got[k]] == list(HASH_KNOWN_ANSWERS[x][1:])

    inp = _light_inputs()
    args = (inp[:, 0:3], inp[:, 3:6], inp[:, 6], inp[:, 7:10], inp[:, 10:13], inp[:, 13:16], inp[:, 16], inp[:, 17])
    f32, f64 = R.light_contribution(*args, np.float32), R.light_contribution(*args, np.float64)
    got = gpu_renderer.test_debug_eval(pkg.DEBUG_EVAL_LIGHT_CONTRIBUTION, inp).view(np.float32)
    assert (np.isnan(got) == np.isnan(f32)).all() and (np.isinf(got) == np.isinf(f32)).all()
    fin = np.isfinite(f32) & np.isfinite(f64)
    assert fin.sum() > 0.99 * fin.size and not fin[0].any()
    bound = 8.0 * np.abs(f32.astype(np.float64) - f64)[fin].max()
    err = np.abs(got.astype(np.float64) - f64)[fin]
    print(f"light contribution: max |gpu - f64| {err.max():.3e}, bound {bound:.3e}, largest value {np.abs(f64[fin]).max():.3e}")
    assert err.max() <= bound


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["reuse_mesh_cubes", "default", "animated_test"])
def test_id_modes(pkg, orc, name):
    s, rs, u, lights = _scene(pkg, orc, name)
    for mode in (R.MODE_GEOMETRY, R.MODE_PRIMITIVE, R.MODE_INSTANCE):
        ref = _ref(pkg, orc, name, mode, 0, np.float32)
        img = _debug(pkg, orc, name, mode)
        assert ref["hit"].any() and not ref["hit"].all()
        assert (_bits(img) == _bits(ref["image"])).all(), mode  # hits: getRandomColor of the oracle's id; misses: the miss colour; alpha 1
        if mode == R.MODE_INSTANCE:
            colours = np.unique(_bits(img)[ref["hit"]][:, 0:3], axis=0)
            assert len(colours) == len(np.unique(ref["ids"][ref["hit"]]))
            assert len(colours) > 1 or s.desc.instanceCount == 1


@pytest.mark.gpu
@pytest.mark.parametrize("case", VALUE_CASES, ids=lambda c: f"{c[0]}-{c[1]}")
def test_value_modes(pkg, orc, case):
    name, mode, flags = case
    ref = _ref(pkg, orc, name, mode, flags, np.float64)
    img = _debug(pkg, orc, name, mode)
    hit = ref["hit"]
    err = np.abs(img.astype(np.float64) - ref["image"])
    print(f"{case}: max |gpu - ref64| {err.max():.3e}, measured max |ref32 - ref64| {REF_F32_VS_F64[case]:.3e}")
    assert (err <= _tol(pkg, orc, case)).all()
    assert (_bits(img)[~hit] == _bits(np.float32([0.2, 0.2, 0.2, 1.0]))).all() and (img[..., 3] == 1.0).all()
    if mode == R.MODE_WORLD_POSITION:  # independent of the vertex data: the point lies on the ray
        o, d, t = ref["origin"].astype(np.float64), ref["direction"].astype(np.float64), ref["t"].astype(np.float64)
        P = img[..., 0:3].astype(np.float64)
        off = np.abs(P - (o + t[..., None] * d)).max(axis=-1)
        assert (off[hit] <= 2.0 ** -18 * np.maximum(1.0, np.maximum(np.abs(P).max(axis=-1), t))[hit]).all()
    if mode == R.MODE_MIPS:
        flat = _debug(pkg, orc, name, mode, hit=pkg.DEBUG_HIT_DISABLE_MIP_MAPS)
        assert (flat[hit][:, 0:3] == 1.0).all() and (_bits(flat)[~hit] == _bits(img)[~hit]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("case", COLOR_CASES, ids=lambda c: c[0])
def test_color_without_shadows(pkg, orc, case):
    name, mode, flags = case
    s, rs, u, lights = _scene(pkg, orc, name)
    ref = _ref(pkg, orc, name, mode, flags, np.float64)
    img = _debug(pkg, orc, name, mode, hit=flags)
    hit = ref["hit"]
    err = np.abs(img.astype(np.float64) - ref["image"])
    print(f"{case}: max |gpu - ref64| on hits {err[hit].max():.3e}, measured max |ref32 - ref64| {REF_F32_VS_F64[case]:.3e}")
    assert (err <= _tol(pkg, orc, case))[hit].all()  # no exception and no cap
    assert (img[..., 3] == 1.0).all() and hit.any() and not hit.all()
    st = _renderer(pkg, orc, name).stats()
    assert (st.pathSamples, st.segments, st.shadowRays, st.retries) == (W * H, W * H, 0, 0)
    miss = rs.osc.test_miss(ref["direction"][~hit].view(np.uint32)).view(np.float32)[:, 0:3]
    if s.desc.skyboxKind == 2:  # the cube sky is miss.rmiss:32's lookup
        assert (_bits(img)[~hit][:, 0:3] == _bits(miss)).all()
    elif s.desc.skyboxKind == 1:  # the 2-D sky is miss.rmiss's lookup WITHOUT hdrToLdr: m = c / (1 + max c) inverted
        m = miss.astype(np.float64)
        M = m.max(axis=1) / (1.0 - m.max(axis=1))
        c = m * (1.0 + M)[:, None]
        ok = M <= 8.0
        assert ok.sum() > 100
        assert (np.abs(img[~hit][:, 0:3] - c) <= (8.0 * 2.0 ** -24 * (1.0 + M) ** 2)[:, None] * np.abs(c) + 1e-30)[ok].all()
    else:
        assert (_bits(img)[~hit] == _bits(np.float32([0.2, 0.2, 0.2, 1.0]))).all()
    if name == "alpha_test":  # the decal tint is in the picture
        has, rgba = R._decals(rs, ref["origin"].reshape(-1, 3), ref["direction"].reshape(-1, 3), ref["t"].reshape(-1), hit.reshape(-1))
        assert has.sum() > 20 and (rgba[has][:, 3] > 0).any()


@pytest.mark.gpu
@pytest.mark.parametrize("case", SHADOW_CASES, ids=lambda c: c[0])
def test_color_with_shadows(pkg, orc, case):
    name, mode, flags = case
    ref = _ref(pkg, orc, name, mode, flags, np.float64)
    img = _debug(pkg, orc, name, mode)
    st = _renderer(pkg, orc, name).stats()
    assert (st.pathSamples, st.segments, st.shadowRays, st.retries) == (W * H, ref["segments"], ref["shadow_rays"], 0)
    beyond = (np.abs(img.astype(np.float64) - ref["image"]) > _tol(pkg, orc, case)).any(axis=-1)
    print(f"{case}: {int(beyond.sum())} pixels beyond the bound, {int(ref['hit'].sum())} hit pixels")
    assert not (beyond & ~R.shadow_edge_mask(ref)).any()
    assert int(beyond.sum()) * 100 <= int(ref["hit"].sum())


def _camera(pkg, position, direction):
    cam = pkg.Scene("default", DETAIL)
    cam.set_camera_pose(position, direction)
    return cam.uniform(W, H)


def _desc_renderer(pkg, desc):
    import torch  # noqa: F401

    r = pkg.Renderer()
    r.upload(desc)
    r.resize(W, H)
    return r


def _soup_renderer(pkg, soup):
    return _desc_renderer(pkg, soup.desc)


@pytest.mark.gpu
def test_shadows_on_a_hand_made_scene(pkg, orc):
    """A floor, an occluder above it, one point light and the directional light: lit pixels are the shadows-disabled render,
    fully shadowed ones the ambient term alone."""
    floor = util.quad_mesh([[-4, 0, 4], [4, 0, 4], [4, 0, -4], [-4, 0, -4]], [0, 1, 0])
    occluder = util.quad_mesh([[-1, 1, 1], [1, 1, 1], [1, 1, -1], [-1, 1, -1]], [0, 1, 0])
    soup = util.TriangleSoup(pkg, [[floor], [occluder]], material=util.mr_material(color=(0.8, 0.6, 0.4), roughness=0.6))
    u = _camera(pkg, (0.0, 5.0, 8.0), (0.0, -0.5, -0.8))
    lights = pkg.LightsUbo()
    lights.LightCount = 1
    lights.Directional.Color[:] = (1.0, 0.9, 0.8)
    lights.Directional.Direction[:] = (0.3, -1.0, 0.2)
    lights.Lights[0].Color[:] = (4.0, 4.0, 5.0)
    lights.Lights[0].Position[:] = (0.2, 4.0, 0.1)
    lights.Lights[0].AttenuationConstant, lights.Lights[0].AttenuationLinear, lights.Lights[0].AttenuationQuadratic = 1.0, 0.1, 0.02
    dark = pkg.LightsUbo()  # no point light and a directional light without colour: what is left is Color * 0.1 + Emissive
    dark.Directional.Direction[:] = (0.3, -1.0, 0.2)
    rs = R.RefScene(orc, soup.desc)
    ref = R.render(rs, u, lights, W, H, R.MODE_COLOR, 0, np.float32)
    r = _soup_renderer(pkg, soup)
    r.render_debug(u, lights, pkg.DEBUG_MODE_COLOR)
    img = r.readback()
    st = r.stats()
    assert (st.segments, st.shadowRays) == (ref["segments"], ref["shadow_rays"]) and ref["shadow_rays"] == 2 * int(ref["hit"].sum())
    r.render_debug(u, lights, pkg.DEBUG_MODE_COLOR, 0, pkg.DEBUG_HIT_DISABLE_SHADOWS)
    unshadowed = r.readback()
    r.render_debug(u, dark, pkg.DEBUG_MODE_COLOR, 0, pkg.DEBUG_HIT_DISABLE_SHADOWS)
    ambient = r.readback()
    r.close()
    lit, shadowed = ref["hit"] & ~ref["occluded"].any(axis=0), ref["hit"] & ref["occluded"].all(axis=0)
    assert lit.sum() > 200 and shadowed.sum() > 10 and (ref["hit"] & ~lit & ~shadowed).sum() > 10
    assert (_bits(img)[lit] == _bits(unshadowed)[lit]).all()
    assert (_bits(img)[shadowed] == _bits(ambient)[shadowed]).all()
    assert (img[shadowed][:, 0:3] < unshadowed[shadowed][:, 0:3]).all()
    assert (_bits(ambient)[ref["hit"]][:, 0:3] == _bits(np.float32([0.8, 0.6, 0.4]) * np.float32(0.1))).all()


def _copy_desc(pkg, desc):
    d = pkg.SceneDesc()
    C.memmove(C.byref(d), C.byref(desc), C.sizeof(d))
    return d


@pytest.mark.gpu
def test_texture_flags(pkg, orc):
    """DisableColorTexture / DisableNormalTexture = the same scene with the materials' colour / normal indices set to the defaults."""
    s, rs, u, lights = _scene(pkg, orc, "texture_test")
    assert s.desc.specularGlossinessMaterialCount == 0 and s.desc.phongMaterialCount == 0
    flagged = {f: _debug(pkg, orc, "texture_test", R.MODE_COLOR, hit=f) for f in (pkg.DEBUG_HIT_DISABLE_COLOR_TEXTURE, pkg.DEBUG_HIT_DISABLE_NORMAL_TEXTURE)}
    plain = _debug(pkg, orc, "texture_test", R.MODE_COLOR)
    for flag, slot, default in ((pkg.DEBUG_HIT_DISABLE_COLOR_TEXTURE, 20, 0), (pkg.DEBUG_HIT_DISABLE_NORMAL_TEXTURE, 21, 1)):
        mats = rs.materials[0].copy()
        assert (mats.view(np.uint32)[:, slot] >= 9).any(), "the scene must use the slot"
        mats.view(np.uint32)[:, slot] = default
        d = _copy_desc(pkg, s.desc)
        d.metallicRoughnessMaterials = mats.ctypes.data
        r = _desc_renderer(pkg, d)
        r.render_debug(u, lights, pkg.DEBUG_MODE_COLOR)
        want = r.readback()
        r.close()
        assert (_bits(flagged[flag]) == _bits(want)).all(), flag
        assert (_bits(flagged[flag]) != _bits(plain)).any(), flag


@pytest.mark.gpu
def test_force_opaque(pkg, orc):
    """ForceOpaque = the same scene with every geometry opaque (shadow rays keep their any-hit stage, so: without shadows)."""
    s, rs, u, lights = _scene(pkg, orc, "alpha_test")
    geos = rs.a["geometries"].copy()
    assert (geos["IsOpaque"] == 0).any()
    geos["IsOpaque"] = 1
    d = _copy_desc(pkg, s.desc)
    d.geometries = geos.ctypes.data
    r = _desc_renderer(pkg, d)
    for mode, hit in ((R.MODE_COLOR, NO_SHADOWS), (R.MODE_WORLD_POSITION, 0), (R.MODE_PRIMITIVE, 0)):
        r.render_debug(u, lights, mode, 0, hit)
        want = r.readback()
        got = _debug(pkg, orc, "alpha_test", mode, raygen=pkg.DEBUG_RAYGEN_FORCE_OPAQUE, hit=hit)
        assert (_bits(got) == _bits(want)).all(), mode
        assert (_bits(got) != _bits(_debug(pkg, orc, "alpha_test", mode, hit=hit))).any(), mode
    r.close()


MIRROR_X = np.float32([-1, 0, 0, 0.5, 0, 1, 0, 0.2, 0, 0, 1, 0.1])  # negative determinant: x -> 0.5 - x


def _facing_quads():
    """Quads in planes z = const, facing +z or -z, some behind others."""
    def quad(cx, cy, z, half, front):
        c = [[cx - half, cy - half, z], [cx + half, cy - half, z], [cx + half, cy + half, z], [cx - half, cy + half, z]]
        return util.quad_mesh(c if front else c[::-1], [0, 0, 1 if front else -1])
    a = [quad(-2.0, 1.0, 0.0, 1.0, True), quad(-2.2, 1.1, -1.0, 1.4, False), quad(-2.0, -1.2, 0.0, 0.9, False), quad(-2.1, -1.0, -1.5, 1.3, True)]
    b = [quad(1.5, 0.8, 0.5, 0.8, True), quad(1.6, 0.9, -0.5, 1.2, False), quad(1.5, -1.0, 0.2, 0.7, False), quad(1.4, -1.1, -0.8, 1.1, True)]
    return a, b


@pytest.mark.gpu
def test_cull_back_faces(pkg, orc):
    """For a pinhole camera a planar quad is back-facing for every pixel or for none: culling = deleting those quads.  Facing is
    decided in the model's space: a mirrored instance keeps the winding of its model."""
    a, b = _facing_quads()
    shift = np.float32([1, 0, 0, 2.6, 0, 1, 0, 0, 0, 0, 1, -0.3])
    instances = [(0, util.IDENTITY_3X4), (1, util.IDENTITY_3X4), (1, MIRROR_X), (0, shift)]
    soup = util.TriangleSoup(pkg, [a, b], instances)
    eye = np.float64([0.2, 0.3, 9.0])
    u = _camera(pkg, tuple(eye), (0.0, 0.0, -1.0))
    # the facing rule, in float64: back-facing iff dot(cross(p1 - p0, p2 - p0), d) > 0 in the model's space = the world-space test times
    # the sign of the instance's determinant
    T = util.world_triangles(soup.desc)
    first = util.pair_first(soup.desc)
    meshes = [(i, k) for i, (m, _) in enumerate(instances) for k in range(4)]
    back, world_back = [], []
    for p, (i, k) in enumerate(meshes):
        sign = np.sign(np.linalg.det(np.float64(instances[i][1]).reshape(3, 4)[:, :3]))
        facing = [np.cross(t[1] - t[0], t[2] - t[0]) @ (t.mean(axis=0) - eye) for t in T[first[p]:first[p + 1]]]
        assert all(f > 1e-3 for f in facing) or all(f < -1e-3 for f in facing)
        back.append(sign * facing[0] > 0)
        world_back.append(facing[0] > 0)
    back, world_back = np.array(back).reshape(len(instances), 4), np.array(world_back).reshape(len(instances), 4)
    assert back[2].any() and not back[2].all(), "the mirrored instance has quads on both sides of the rule"
    assert (back[2] == back[1]).all() and (world_back[2] != back[2]).all(), "a mirrored instance keeps the winding of its model, not of the world"
    # the same scene without the back-facing quads: one model per instance
    models = [[(a, b)[m][k] for k in range(4) if not back[i, k]] for i, (m, _) in enumerate(instances)]
    kept = util.TriangleSoup(pkg, models, [(i, x) for i, (_, x) in enumerate(instances)])
    r, rk = _soup_renderer(pkg, soup), _soup_renderer(pkg, kept)
    r.render_debug(u, pkg.LightsUbo(), pkg.DEBUG_MODE_WORLD_POSITION, pkg.DEBUG_RAYGEN_CULL_BACK_FACES)
    culled = r.readback()
    r.render_debug(u, pkg.LightsUbo(), pkg.DEBUG_MODE_WORLD_POSITION)
    unculled = r.readback()
    rk.render_debug(u, pkg.LightsUbo(), pkg.DEBUG_MODE_WORLD_POSITION)
    want = rk.readback()
    rk.render_debug(u, pkg.LightsUbo(), pkg.DEBUG_MODE_WORLD_POSITION, pkg.DEBUG_RAYGEN_CULL_BACK_FACES)
    assert (_bits(rk.readback()) == _bits(want)).all()  # nothing left to cull
    r.close()
    rk.close()
    assert (_bits(culled) == _bits(want)).all()
    assert (_bits(culled) != _bits(unculled)).any(axis=-1).sum() > 100


@pytest.mark.gpu
def test_cull_back_faces_on_a_closed_box(pkg, orc):
    """Outward-wound and seen from outside, nothing is culled; from inside, everything."""
    q = util.quad_mesh
    box = [q([[-1, -1, 1], [1, -1, 1], [1, 1, 1], [-1, 1, 1]], [0, 0, 1]), q([[1, -1, -1], [-1, -1, -1], [-1, 1, -1], [1, 1, -1]], [0, 0, -1]),
           q([[1, -1, 1], [1, -1, -1], [1, 1, -1], [1, 1, 1]], [1, 0, 0]), q([[-1, -1, -1], [-1, -1, 1], [-1, 1, 1], [-1, 1, -1]], [-1, 0, 0]),
           q([[-1, 1, 1], [1, 1, 1], [1, 1, -1], [-1, 1, -1]], [0, 1, 0]), q([[-1, -1, -1], [1, -1, -1], [1, -1, 1], [-1, -1, 1]], [0, -1, 0])]
    r = _soup_renderer(pkg, util.TriangleSoup(pkg, [box]))
    outside = _camera(pkg, (2.5, 2.0, 4.0), (-0.5, -0.4, -0.8))
    imgs = []
    for raygen in (0, pkg.DEBUG_RAYGEN_CULL_BACK_FACES):
        r.render_debug(outside, pkg.LightsUbo(), pkg.DEBUG_MODE_WORLD_POSITION, raygen)
        imgs.append(r.readback())
    assert (_bits(imgs[0]) == _bits(imgs[1])).all()
    clear = _bits(np.float32([0.2, 0.2, 0.2, 1.0]))
    assert 200 < (_bits(imgs[0]) != clear).any(axis=-1).sum() < W * H
    inside = _camera(pkg, (0.1, 0.0, 0.2), (0.3, 0.2, -0.9))
    r.render_debug(inside, pkg.LightsUbo(), pkg.DEBUG_MODE_WORLD_POSITION)
    assert (_bits(r.readback()) != clear).any(axis=-1).all()
    r.render_debug(inside, pkg.LightsUbo(), pkg.DEBUG_MODE_WORLD_POSITION, pkg.DEBUG_RAYGEN_CULL_BACK_FACES)
    assert (_bits(r.readback()) == clear).all()
    r.close()


@pytest.mark.gpu
def test_tile_shards_borrower_and_output(pkg, orc):
    s, rs, u, lights = _scene(pkg, orc, "texture_test")
    whole = _debug(pkg, orc, "texture_test", R.MODE_COLOR)
    r = _renderer(pkg, orc, "texture_test")
    sentinel = np.full((H, W, 4), util.SHARD_SENTINEL, np.uint32).view(np.float32)
    union = np.zeros((H, W), bool)
    for rank in range(3):
        r.set_tile_shard(rank, 3, 16)
        r.write_accumulation(sentinel)
        r.render_debug(u, lights, pkg.DEBUG_MODE_COLOR)
        img = r.readback()
        own = pkg.shard_mask(W, H, rank, 3, 16)
        assert r.stats().pathSamples == own.sum()
        assert (_bits(img)[own] == _bits(whole)[own]).all() and (_bits(img)[~own] == util.SHARD_SENTINEL).all()
        assert not (union & own).any()
        union |= own
    assert union.all()
    r.set_tile_shard(0, 1, 32)
    # a borrower renders its owner's scene
    b = pkg.Renderer()
    b.share_scene(r)
    b.resize(W, H)
    b.render_debug(u, lights, pkg.DEBUG_MODE_COLOR)
    assert (_bits(b.readback()) == _bits(whole)).all()
    b.close()
    # the frame is one sample to the output stage
    r.render_debug(u, lights, pkg.DEBUG_MODE_COLOR)
    r.postprocess(1)
    assert (_bits(r.read_output(pkg.OUTPUT_RGBA32F)) == _bits(orc.postprocess(whole, 1))).all()


@pytest.mark.gpu
def test_the_view_leaves_no_state_behind(pkg, orc):
    s, rs, u, lights = _scene(pkg, orc, "alpha_test")
    r = _renderer(pkg, orc, "alpha_test")
    up = s.uniform(W, H, bounces=4)

    def path_traced():
        r.reset()
        for f in range(2):
            up.TotalSamples = f
            r.render(up, lights)
        return r.readback()
    before = path_traced()
    r.render_debug(u, lights, pkg.DEBUG_MODE_COLOR)
    r.render_debug(u, lights, pkg.DEBUG_MODE_INSTANCE, pkg.DEBUG_RAYGEN_CULL_BACK_FACES | pkg.DEBUG_RAYGEN_FORCE_OPAQUE)
    after = path_traced()
    assert (_bits(before) == _bits(after)).all() and np.isfinite(before).all() and (before[..., 0:3] > 0).any()


@pytest.mark.gpu
def test_refusals_leave_the_image_untouched(pkg, orc):
    import torch

    s, rs, u, lights = _scene(pkg, orc, "default")
    r = _renderer(pkg, orc, "default")
    sentinel = np.full((H, W, 4), util.SHARD_SENTINEL, np.uint32).view(np.float32)
    r.write_accumulation(sentinel)

    def refused(status, view, ubo=lights, renderer=r):
        rc = renderer.lib.ptx_render_debug(renderer.handle, C.byref(u), C.byref(ubo), C.byref(view))
        assert rc == status, (rc, renderer.lib.ptx_last_error(renderer.handle))
    for view in (pkg.DebugViewDesc(8, 0, 0, 0), pkg.DebugViewDesc(0, 4, 0, 0), pkg.DebugViewDesc(0, 0, 16, 0), pkg.DebugViewDesc(0, 0, 0, 1),
                 pkg.DebugViewDesc(0xFFFFFFFF, 0, 0, 0)):
        refused(1, view)
    many = pkg.LightsUbo()
    many.LightCount = 65
    refused(1, pkg.DebugViewDesc(0, 0, 0, 0), many)
    assert r.lib.ptx_render_debug(r.handle, C.byref(u), C.byref(lights), None) == 1
    shard = torch.zeros(r.shard_bytes(0) // 4, dtype=torch.float32, device="cuda")
    r.bind_shard_accumulation(shard.data_ptr(), shard.numel() * 4)
    refused(5, pkg.DebugViewDesc(0, 0, 0, 0))
    r.bind_shard_accumulation(0)
    assert (_bits(r.readback()) == util.SHARD_SENTINEL).all()
    fresh = pkg.Renderer()
    refused(5, pkg.DebugViewDesc(0, 0, 0, 0), renderer=fresh)  # no scene, no tree, no image
    fresh.resize(W, H)
    refused(5, pkg.DebugViewDesc(0, 0, 0, 0), renderer=fresh)
    fresh.close()
    r.render_debug(u, lights, pkg.DEBUG_MODE_COLOR)  # and the handle still works
    assert (_bits(r.readback()) != util.SHARD_SENTINEL).all()


@pytest.mark.gpu
def test_pending_streamed_textures_sample_their_stand_ins(pkg, orc):
    """A scene uploaded with every texture pending renders the debug view of the scene whose textures are the stand-ins."""
    s, rs, u, lights = _scene(pkg, orc, "texture_test")
    d = _copy_desc(pkg, s.desc)
    tex = (pkg.TextureDesc * d.textureCount).from_address(d.textures)
    pending = (pkg.TextureDesc * d.textureCount)(*[pkg.TextureDesc(t.width, t.height, t.format, t.levels, None) for t in tex])
    d.textures = C.addressof(pending)
    r = pkg.Renderer()
    r.upload_streamed(d)
    r.resize(W, H)
    r.render_debug(u, lights, pkg.DEBUG_MODE_COLOR, 0, NO_SHADOWS)
    got = r.readback()
    r.close()
    none = _copy_desc(pkg, s.desc)
    none.textures, none.textureCount = None, 0  # indices >= 9 then sample the white placeholder
    r = _desc_renderer(pkg, none)
    r.render_debug(u, lights, pkg.DEBUG_MODE_COLOR, 0, NO_SHADOWS)
    assert (_bits(got) == _bits(r.readback())).all()
    r.close()


if __name__ == "__main__":  # prints REF_F32_VS_F64
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import __graft_entry__ as graft

    pkg_, orc_ = graft.load_package(), graft.load_oracle()
    orc_.build()
    for case_ in ALL_CASES:
        print(f"    {case_!r}: {_measure(pkg_, orc_, case_):.3e},")
