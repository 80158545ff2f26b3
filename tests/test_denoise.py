"""The denoiser (include/ptx.h ptx_render_guides / ptx_denoise / ptx_postprocess_denoised, csrc/pt_denoise.hpp, docs/NEXT_ROWS.md
section 13) against tests/denoise_ref.py.

Bit-exact legs need no tolerance: the normal and position guides are the debug view's Normal and WorldPosition images, the albedo
guide is the material's colour, the output stage on the denoised image is the output stage on a copy of it.

Tolerance of the filter.  The filter gets the device's own read-back guides, so both sides start from the same bits; what differs
from the float64 reference is float32 rounding in the weights and the sums.  The bound is measured ON THE REFERENCE ALONE, per case,
inside the test: 8 x max |ref(float32) - ref(float64)| over the image of that very case, with a floor of 2^-20 max(1, |value|).
Pixels that are not finite must match in class and position exactly."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import denoise_ref as R
import util

W, H = 67, 45  # the frame of the neighbouring tests: odd, no multiple of a workgroup tile
DETAIL = 0.25
SAMPLES = 8
POST = dict(exposure=1.0, bloom_threshold=0.8, bloom_intensity=0.35)
SIGMA_NORMAL, SIGMA_POSITION = 0.3, 0.05
SIGMA_COLORS = (0.0, 1.5)
# frame -> (width, height, iteration counts checked).  1 x 1: nothing but the centre tap; 5 x 3: smaller than the footprint at step
# 1; 33 x 22 with six iterations: step 32 exceeds an extent; 300 x 200: 10 x 25 workgroup tiles whose halos meet
FRAMES = {"67x45": (67, 45, (1, 3, 5)), "1x1": (1, 1, (1, 3, 5)), "5x3": (5, 3, (1, 3, 5)), "33x22": (33, 22, (1, 3, 6)), "300x200": (300, 200, (1, 3, 5))}
FILTER_CASES = [(f, i) for f in ("67x45", "1x1", "5x3", "33x22") for i in ("render1", "render8", "synthetic", "impulse")] + \
               [("300x200", "render1"), ("300x200", "synthetic")]
FILTER_SCENE = "texture_test"


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# =====================================================================================================
# without a GPU
# =====================================================================================================
def test_header_declares_and_package_exports_the_denoiser(pkg):
    header = open(os.path.join(pkg.REPO_DIR, "include", "ptx.h")).read()
    decls = {
        "ptx_render_guides": r"PTX_API int ptx_render_guides\(PtxRenderer \*r, const PtxRaygenUniformData \*uniform\);",
        "ptx_read_guide": r"PTX_API int ptx_read_guide\(PtxRenderer \*r, uint32_t which, void \*host, size_t bytes\);",
        "ptx_device_guide_ptr": r"PTX_API void \*ptx_device_guide_ptr\(PtxRenderer \*r, uint32_t which\);",
        "ptx_denoise": r"PTX_API int ptx_denoise\(PtxRenderer \*r, const PtxDenoiseDesc \*desc\);",
        "ptx_read_denoised": r"PTX_API int ptx_read_denoised\(PtxRenderer \*r, void \*host, size_t bytes\);",
        "ptx_device_denoised_ptr": r"PTX_API void \*ptx_device_denoised_ptr\(PtxRenderer \*r\);",
        "ptx_postprocess_denoised": r"PTX_API int ptx_postprocess_denoised\(PtxRenderer \*r, const PtxPostProcessingUniformData \*uniform, uint32_t toneMappingMode\);",
    }
    lib = pkg.load_hip()
    for name, decl in decls.items():
        assert re.search(decl, header), name
        assert name in pkg.PTX_SYMBOLS
        assert hasattr(lib, name), name
    assert "#define PTX_ABI_VERSION 5u" in header and "PTX_FN_COUNT = 38" in header  # additions only
    assert pkg.ABI_VERSION == 5
    for k, name in enumerate(("NORMAL", "POSITION", "ALBEDO")):
        assert re.search(r"PTX_GUIDE_%s = %d\b" % (name, k), header), name
        assert getattr(pkg, "GUIDE_" + name) == k and getattr(R, "GUIDE_" + name) == k
    assert re.search(r"typedef struct PtxDenoiseDesc \{\s*uint32_t totalSamples;[^}]*uint32_t iterations;[^}]*float sigmaColor;[^}]*float sigmaNormal;[^}]*"
                     r"float sigmaPosition;[^}]*uint32_t flags;[^}]*uint32_t reserved;[^}]*\} PtxDenoiseDesc;", header)
    assert C.sizeof(pkg.DenoiseDesc) == 28 and pkg.DenoiseDesc.sigmaColor.offset == 8 and pkg.DenoiseDesc.reserved.offset == 24
    for method in ("render_guides", "read_guide", "denoise", "read_denoised", "postprocess_denoised"):
        assert callable(getattr(pkg.Renderer, method))
    d = pkg.DENOISE_DEFAULTS
    assert 1 <= d["iterations"] <= 6 and d["sigma_color"] >= 0 and d["sigma_normal"] > 0 and d["sigma_position"] > 0
    host = open(os.path.join(pkg.PKG_DIR, "host", "RendererHip.h")).read()
    assert "struct DenoiserSettings" in host and "SetSettings(const DenoiserSettings &" in host and "bool Enabled = false" in host
    assert "--denoise" in open(os.path.join(pkg.REPO_DIR, "examples", "render_scene.cpp")).read()


def _plane_sum(h, w, value=(0.5, 0.25, 1.0), samples=SAMPLES):
    S = np.zeros((h, w, 4), np.float32)
    S[..., 0:3] = np.float32(value) * samples
    S[..., 3] = samples
    return S


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_reference_keeps_a_constant_image(dtype):
    g = R.plane_guides(19, 23, albedo=(0.8, 0.5, 0.004))  # the last channel is below the albedo floor
    for sc in (0.0, 0.7):
        for D in R.denoise_all(_plane_sum(19, 23), *g, SAMPLES, 5, sc, SIGMA_NORMAL, SIGMA_POSITION, dtype):
            assert D.dtype == np.dtype(dtype) and (D[..., 3] == 1).all()
            assert np.abs(D[..., 0:3] - np.float64([0.5, 0.25, 1.0])).max() <= 16 * np.finfo(dtype).eps


def test_reference_impulse_response_is_the_b3_spline():
    """One plane, no colour term: every weight is h (x) h, so one iteration answers an impulse with h (x) h and two with its
    convolution with the same kernel spread two pixels apart."""
    n, c = 21, 10
    g = R.plane_guides(n, n)
    S = np.zeros((n, n, 4), np.float32)
    S[c, c, 0:3] = (1.0, 2.0, 4.0)
    one, two = R.denoise_all(S, *g, 1, 2, 0.0, SIGMA_NORMAL, SIGMA_POSITION, np.float64)
    h = np.float64(R.H5)
    k1 = np.zeros((n, n))
    k1[c - 2:c + 3, c - 2:c + 3] = np.outer(h, h)
    assert np.abs(one[..., 0] - k1).max() <= 1e-15 and np.abs(one[..., 2] - 4 * k1).max() <= 1e-15
    k2 = np.zeros((n, n))
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            k2 += h[dy + 2] * h[dx + 2] * np.roll(np.roll(k1, 2 * dy, axis=0), 2 * dx, axis=1)
    assert np.abs(two[..., 1] - 2 * k2).max() <= 1e-15
    assert abs(one[..., 0].sum() - 1) <= 1e-14 and abs(two[..., 0].sum() - 1) <= 1e-14  # away from the border the filter keeps the sum


def test_reference_renormalises_at_the_border():
    """An impulse in the corner: the centre weight 9/64 over the weights inside the image, (3/8 + 1/4 + 1/16)^2 = 121/256."""
    g = R.plane_guides(9, 9)
    S = np.zeros((9, 9, 4), np.float32)
    S[0, 0, 0:3] = 1.0
    D = R.denoise(S, *g, 1, 1, 0.0, SIGMA_NORMAL, SIGMA_POSITION, np.float64)
    assert abs(D[0, 0, 0] - 36.0 / 121.0) <= 1e-15
    # (0, 1) sees the impulse through h[1] h[2] over (3/8 + 1/4 + 1/16) (1/4 + 3/8 + 1/4 + 1/16)
    assert abs(D[0, 1, 0] - (0.25 * 0.375) / ((11.0 / 16.0) * (15.0 / 16.0))) <= 1e-15


@pytest.mark.parametrize("sigma", [0.01, 0.1, 0.3])
def test_reference_edges_block_the_blur(sigma):
    """A step in the normal (|n_p - n_q|^2 = 2) or a plane offset of 40 sigma t keeps the two halves apart to e^-(2 / sigma^2) or
    better; the same step under a wide sigma is blurred."""
    h, w = 12, 16
    S = _plane_sum(h, w, (1.0, 1.0, 1.0))
    S[:, w // 2:, 0:3] = 0.0
    left = np.ones((h, w), bool)
    left[:, w // 2:] = False
    nrm, pos, alb = R.plane_guides(h, w)
    nrm[~left, 0:3] = (1.0, 0.0, 0.0)
    D = R.denoise(S, nrm, pos, alb, SAMPLES, 3, 0.0, sigma, 1e3, np.float64)
    bound = np.exp(-2.0 / sigma ** 2) * 25
    assert np.abs(D[left][:, 0:3] - 1).max() <= bound and np.abs(D[~left][:, 0:3]).max() <= bound
    blurred = R.denoise(S, nrm, pos, alb, SAMPLES, 3, 0.0, 1e3, 1e3, np.float64)
    assert 0.3 < blurred[h // 2, w // 2 - 1, 0] < 0.7
    nrm, pos, alb = R.plane_guides(h, w, distance=2.0)
    pos[~left, 2] += 40 * sigma * 2.0  # along the normal
    D = R.denoise(S, nrm, pos, alb, SAMPLES, 3, 0.0, 1e3, sigma, np.float64)
    assert np.abs(D[left][:, 0:3] - 1).max() <= 1e-300 and np.abs(D[~left][:, 0:3]).max() <= 1e-300
    blurred = R.denoise(S, nrm, pos, alb, SAMPLES, 3, 0.0, 1e3, 1e3, np.float64)
    assert 0.3 < blurred[h // 2, w // 2 - 1, 0] < 0.7


def test_reference_colour_term_keeps_a_hot_pixel_to_itself():
    g = R.plane_guides(11, 11)
    S = _plane_sum(11, 11, (0.5, 0.5, 0.5))
    S[5, 5, 0:3] = 1000.0 * SAMPLES
    spread = R.denoise(S, *g, SAMPLES, 2, 0.0, SIGMA_NORMAL, SIGMA_POSITION, np.float64)
    kept = R.denoise(S, *g, SAMPLES, 2, 1.0, SIGMA_NORMAL, SIGMA_POSITION, np.float64)
    assert spread[5, 6, 0] > 10 and abs(kept[5, 6, 0] - 0.5) <= 1e-12 and kept[5, 5, 0] == 1000.0


def test_reference_misses_and_non_finite_pixels_pass_through():
    rng = np.random.default_rng(3)
    h, w = 14, 18
    S = _plane_sum(h, w, (0.5, 0.5, 0.5))
    S[..., 0:3] += rng.uniform(0, 1, (h, w, 3)).astype(np.float32)
    g = list(R.plane_guides(h, w, albedo=(0.5, 0.5, 0.5)))
    miss = np.zeros((h, w), bool)
    miss[:, 12:] = True
    R.set_miss(g, miss)
    S[3, 4, 1], S[6, 7, 2], S[8, 2, 0] = np.nan, np.inf, -np.inf
    S[2, 14, 0] = np.nan  # in the miss region
    D = R.denoise(S, *g, SAMPLES, 3, 0.0, SIGMA_NORMAL, SIGMA_POSITION, np.float64)
    m = R.mean_of(S, SAMPLES, np.float64)
    assert (D[miss][:, 0:3].view(np.uint64) == m[miss].view(np.uint64)).all()  # untouched, the NaN included
    for y, x in ((3, 4), (6, 7), (8, 2)):
        assert (D[y, x, 0:3].view(np.uint64) == m[y, x].view(np.uint64)).all()  # the centre survives with its class
    rest = ~miss
    for y, x in ((3, 4), (6, 7), (8, 2)):
        rest[y, x] = False
    assert np.isfinite(D[rest]).all()  # ... and no tap took it in
    # the hit pixels next to the miss region saw none of it: the same image cropped at the boundary gives the same values
    crop = R.denoise(S[:, :12], *[x[:, :12] for x in g], SAMPLES, 3, 0.0, SIGMA_NORMAL, SIGMA_POSITION, np.float64)
    assert (crop.view(np.uint64) == D[:, :12].view(np.uint64)).all()
    # a pixel whose normal or hit distance is not finite is no tap and is not filtered either
    g[R.GUIDE_NORMAL][5, 5, 0] = np.nan
    g[R.GUIDE_POSITION][9, 9, 3] = 0.0
    D2 = R.denoise(S, *g, SAMPLES, 1, 0.0, SIGMA_NORMAL, SIGMA_POSITION, np.float64)
    assert (D2[5, 5, 0:3] == m[5, 5]).all() and (D2[9, 9, 0:3] == m[9, 9]).all() and np.isfinite(D2[4:7, 4:7]).all()


QUALITY_W, QUALITY_H, QUALITY_LOW_SPP = 134, 90, 4


@pytest.mark.parametrize("name", ["default", "texture_test", "alpha_test"])
def test_defaults_reduce_the_error_of_a_low_sample_frame(pkg, orc, name):
    """The quality table of docs/NEXT_ROWS.md section 13 (tools/denoise_quality.py): a 4-spp frame of the CPU oracle, denoised by the
    reference at the package's default parameters with first-hit guides computed on the CPU, is closer to the 512-spp mean
    (tests/golden/denoise_truth_512spp.npz, other samples) than the raw frame is."""
    truth = np.load(os.path.join(util.GOLDEN_DIR, "denoise_truth_512spp.npz"))[name].astype(np.float32)
    assert truth.shape == (QUALITY_H, QUALITY_W, 3)
    scene = pkg.Scene(name, DETAIL)
    osc = orc.OracleScene(scene.desc, build_bvh=True)
    low = np.zeros((QUALITY_H, QUALITY_W, 4), np.float32)
    for f in range(QUALITY_LOW_SPP):
        osc.render(scene.uniform(QUALITY_W, QUALITY_H, bounces=4, sample_count=1, total_samples=f), scene.lights, QUALITY_W, QUALITY_H, accum=low)
    guides = R.cpu_guides(pkg, orc, scene, QUALITY_W, QUALITY_H)
    d = pkg.DENOISE_DEFAULTS
    den = R.denoise(low, *guides, QUALITY_LOW_SPP, d["iterations"], d["sigma_color"], d["sigma_normal"], d["sigma_position"], np.float32)
    raw_err, den_err = R.relative_l2(low[..., 0:3] / QUALITY_LOW_SPP, truth), R.relative_l2(den, truth)
    print(f"{name}: relative L2 error raw {raw_err:.4f}, denoised {den_err:.4f}")
    assert np.isfinite(den).all() and den_err < raw_err


# =====================================================================================================
# on the GPU: the guide pass
# =====================================================================================================
_scenes, _renderers = {}, {}


def _scene(pkg, name):
    if name not in _scenes:
        s = pkg.Scene(name, DETAIL)
        _scenes[name] = (s, s.uniform(W, H), s.lights)
    return _scenes[name]


def _renderer(pkg, name):
    """One renderer per scene, uploaded once."""
    import torch  # noqa: F401  (first, so the HIP library shares torch's HIP runtime)

    if name not in _renderers:
        r = pkg.Renderer()
        r.upload(_scene(pkg, name)[0])
        r.resize(W, H)
        _renderers[name] = r
    return _renderers[name]


def _guides(r, u):
    r.render_guides(u)
    return [r.read_guide(k) for k in range(3)]


def _primary_rays(pkg, r, u, w, h):
    """The device's own constructPrimaryRay through the pixel centres, as ptx_trace_rays takes them."""
    y, x = np.divmod(np.arange(w * h, dtype=np.uint32), np.uint32(w))
    inp = np.zeros((w * h, 38), np.float32)
    iu = inp.view(np.uint32)
    iu[:, 0], iu[:, 1], iu[:, 2], iu[:, 3] = x, y, w, h
    inp[:, 4:6] = 0.5
    inp[:, 6:22] = np.frombuffer(u.ViewInverse, np.float32)
    inp[:, 22:38] = np.frombuffer(u.ProjInverse, np.float32)
    out = r.test_eval(pkg.FN["constructPrimaryRay"], inp).view(np.float32)
    rays = np.zeros((w * h, 8), np.float32)
    rays[:, 0:3], rays[:, 3], rays[:, 4:7], rays[:, 7] = out[:, 0:3], 1e-5, out[:, 3:6], 1e4
    return rays


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["default", "texture_test", "alpha_test", "reuse_mesh_cubes", "animated_test"])
def test_normal_and_position_guides_are_the_debug_view_s(pkg, name):
    s, u, lights = _scene(pkg, name)
    r = _renderer(pkg, name)
    if name == "animated_test":
        assert s.update(0.37)
        r.update_animation(*s.animation_state())
    hits, _ = r.trace_rays(_primary_rays(pkg, r, u, W, H))
    hit = (hits[:, 3] != 0).reshape(H, W)
    assert hit.any() and not hit.all()
    nrm, pos, alb = _guides(r, u)
    st = r.stats()
    assert (st.pathSamples, st.segments, st.shadowRays, st.retries) == (W * H, W * H, 0, 0)
    for guide, mode in ((nrm, pkg.DEBUG_MODE_NORMAL), (pos, pkg.DEBUG_MODE_WORLD_POSITION)):
        r.render_debug(u, lights, mode)
        want = r.readback()
        assert (_bits(guide)[hit][:, 0:3] == _bits(want)[hit][:, 0:3]).all(), mode
    assert (_bits(nrm)[hit][:, 3] == _bits(np.float32(1.0))).all()
    assert (_bits(pos)[..., 3][hit] == _bits(hits[:, 0]).reshape(H, W)[hit]).all()  # w = the hit distance
    assert (_bits(alb)[hit][:, 3] == _bits(np.float32(1.0))).all() and np.isfinite(alb).all()
    assert (_bits(nrm)[~hit] == 0).all() and (_bits(pos)[~hit] == 0).all() and (_bits(alb)[~hit] == _bits(np.float32(1.0))).all()
    assert abs(np.linalg.norm(nrm[hit][:, 0:3].astype(np.float64), axis=1) - 1).max() <= 1e-6


def _camera(pkg, position, direction, w=W, h=H):
    cam = pkg.Scene("default", DETAIL)
    cam.set_camera_pose(position, direction)
    return cam.uniform(w, h)


FLAT_COLOURS = np.float32([[0.8, 0.6, 0.4], [0.005, 1.5, 0.25], [0.0, 1.0, 0.1]])  # below the filter's floor, above one, zero: stored as they are


@pytest.mark.gpu
def test_albedo_guide_on_flat_materials(pkg):
    import torch  # noqa: F401

    def quad(cx, cy, z, half):
        return util.quad_mesh([[cx - half, cy - half, z], [cx + half, cy - half, z], [cx + half, cy + half, z], [cx - half, cy + half, z]], [0, 0, 1])
    soup = util.TriangleSoup(pkg, [[quad(-2.0, 0.5, 0.0, 1.2), quad(1.5, 0.8, 0.5, 1.0), quad(0.0, -1.2, -1.0, 1.6)]])
    soup.materials = np.stack([util.mr_material(color=tuple(c), roughness=0.5) for c in FLAT_COLOURS])
    soup.meshes["MaterialId"] = np.arange(3, dtype=np.uint32) << 8  # (index << 8) | metallic-roughness
    soup.desc.metallicRoughnessMaterials, soup.desc.metallicRoughnessMaterialCount = soup.materials.ctypes.data, 3
    u = _camera(pkg, (0.2, 0.3, 9.0), (0.0, 0.0, -1.0))
    r = pkg.Renderer()
    r.upload(soup.desc)
    r.resize(W, H)
    hits, ids = r.trace_rays(_primary_rays(pkg, r, u, W, H))
    hit, mesh = (hits[:, 3] != 0).reshape(H, W), ids[:, 0].reshape(H, W)
    nrm, pos, alb = _guides(r, u)
    r.close()
    assert all(((mesh == k) & hit).sum() > 30 for k in range(3)) and (~hit).sum() > 30
    assert (_bits(alb)[hit][:, 0:3] == _bits(FLAT_COLOURS)[mesh[hit]]).all() and (alb[..., 3] == 1).all()
    assert (_bits(alb)[~hit] == _bits(np.float32(1.0))).all() and (_bits(nrm)[~hit] == 0).all() and (_bits(pos)[~hit] == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["texture_test", "alpha_test"])
def test_albedo_guide_on_textured_scenes(pkg, name):
    """Without emission, light colours and shadows the debug view's Color mode is material.Color * 0.1 (+ 0 + finite x 0)."""
    import torch  # noqa: F401

    s, u, lights = _scene(pkg, name)
    d, keep = R.without_emission(pkg, s.desc)
    dark = R.dark_lights(pkg, lights)
    r = pkg.Renderer()
    r.upload(d)
    r.resize(W, H)
    nrm, pos, alb = _guides(r, u)
    r.render_debug(u, dark, pkg.DEBUG_MODE_COLOR, 0, pkg.DEBUG_HIT_DISABLE_SHADOWS)
    img = r.readback()
    r.close()
    hit = nrm[..., 3] == 1
    finite = np.isfinite(img[..., 0:3]).all(axis=-1) & hit
    print(f"{name}: {int(hit.sum())} hit pixels, {int(finite.sum())} of them finite in the debug view")
    assert hit.sum() > 200 and finite.sum() * 100 >= 99 * hit.sum()
    want = alb[..., 0:3] * np.float32(0.1)
    assert want.dtype == np.float32 and (_bits(img[..., 0:3])[finite] == _bits(want)[finite]).all()
    assert len(np.unique(_bits(alb)[hit][:, 0:3], axis=0)) > 8, "the scene's albedo must come from its textures"
    # emission is no part of the albedo: the scene as it is has the same guides
    own = _guides(_renderer(pkg, name), u)
    for a, b in zip(own, (nrm, pos, alb)):
        assert (_bits(a) == _bits(b)).all()
    if name == "alpha_test":  # the decal tint is in the albedo: the same scene with every geometry opaque differs
        geos = util.desc_arrays(s.desc)["geometries"].copy()
        assert (geos["IsOpaque"] == 0).any()
        geos["IsOpaque"] = 1
        o = pkg.SceneDesc()
        C.memmove(C.byref(o), C.byref(s.desc), C.sizeof(o))
        o.geometries = geos.ctypes.data
        ro = pkg.Renderer()
        ro.upload(o)
        ro.resize(W, H)
        opaque = _guides(ro, u)
        ro.close()
        assert (_bits(opaque[R.GUIDE_ALBEDO]) != _bits(alb)).any(axis=-1).sum() > 20


@pytest.mark.gpu
def test_guide_pass_behaviour(pkg):
    """Stats per tile shard, a borrower, pending streamed textures, and nothing of the path tracer's is touched."""
    s, u, lights = _scene(pkg, "texture_test")
    r = _renderer(pkg, "texture_test")
    up = s.uniform(W, H, bounces=4)

    def path_traced():
        r.reset()
        for f in range(2):
            up.TotalSamples = f
            r.render(up, lights)
        return r.readback()
    before = path_traced()
    whole = _guides(r, u)
    assert (_bits(r.readback()) == _bits(before)).all()  # the accumulation image is not touched
    assert r.guide_ptr(0) and r.guide_ptr(1) - r.guide_ptr(0) == W * H * 16 and r.guide_ptr(2) - r.guide_ptr(1) == W * H * 16 and not r.guide_ptr(3)
    up.TotalSamples = 2
    r.render(up, lights)
    third = r.readback()
    assert (_bits(path_traced()) == _bits(before)).all()  # ... nor the next ptx_render
    up.TotalSamples = 2
    r.render(up, lights)
    assert (_bits(r.readback()) == _bits(third)).all()
    # tile shards: the owned pixels are written, the others keep what they held
    union = np.zeros((H, W), bool)
    for rank in range(3):
        r.set_tile_shard(rank, 3, 16)
        part = _guides(r, u)
        own = pkg.shard_mask(W, H, rank, 3, 16)
        st = r.stats()
        assert (st.pathSamples, st.segments, st.shadowRays) == (own.sum(), own.sum(), 0)
        for a, b in zip(part, whole):
            assert (_bits(a) == _bits(b)).all()
        union |= own
    assert union.all()
    r.set_tile_shard(0, 1, 32)
    # a borrower renders its owner's scene
    b = pkg.Renderer()
    b.share_scene(r)
    b.resize(W, H)
    for a, c in zip(_guides(b, u), whole):
        assert (_bits(a) == _bits(c)).all()
    b.close()
    # pending streamed textures sample their stand-ins: the guides of the scene without its textures
    d = pkg.SceneDesc()
    C.memmove(C.byref(d), C.byref(s.desc), C.sizeof(d))
    tex = (pkg.TextureDesc * d.textureCount).from_address(d.textures)
    pending = (pkg.TextureDesc * d.textureCount)(*[pkg.TextureDesc(t.width, t.height, t.format, t.levels, None) for t in tex])
    d.textures = C.addressof(pending)
    p = pkg.Renderer()
    p.upload_streamed(d)
    p.resize(W, H)
    got = _guides(p, u)
    p.close()
    none = pkg.SceneDesc()
    C.memmove(C.byref(none), C.byref(s.desc), C.sizeof(none))
    none.textures, none.textureCount = None, 0
    q = pkg.Renderer()
    q.upload(none)
    q.resize(W, H)
    for a, c in zip(got, _guides(q, u)):
        assert (_bits(a) == _bits(c)).all()
    q.close()
    assert (_bits(got[R.GUIDE_ALBEDO]) != _bits(whole[R.GUIDE_ALBEDO])).any()


@pytest.mark.gpu
def test_guide_pass_refusals(pkg):
    import torch

    s, u, lights = _scene(pkg, "default")
    r = _renderer(pkg, "default")
    lib = r.lib
    buf = np.zeros((H, W, 4), np.float32)
    fresh = pkg.Renderer()
    assert lib.ptx_render_guides(fresh.handle, C.byref(u)) == 5  # no scene, no tree, no image
    fresh.resize(W, H)
    assert lib.ptx_render_guides(fresh.handle, C.byref(u)) == 5
    assert lib.ptx_read_guide(fresh.handle, 0, buf.ctypes.data, buf.nbytes) == 5 and not lib.ptx_device_guide_ptr(fresh.handle, 0)
    fresh.close()
    r.resize(W, H)  # drops the guides of earlier tests
    assert lib.ptx_read_guide(r.handle, 0, buf.ctypes.data, buf.nbytes) == 5
    assert lib.ptx_render_guides(r.handle, None) == 1
    shard = torch.zeros(r.shard_bytes(0) // 4, dtype=torch.float32, device="cuda")
    r.bind_shard_accumulation(shard.data_ptr(), shard.numel() * 4)
    assert lib.ptx_render_guides(r.handle, C.byref(u)) == 5
    r.bind_shard_accumulation(0)
    assert lib.ptx_read_guide(r.handle, 0, buf.ctypes.data, buf.nbytes) == 5 and not buf.any()
    r.render_guides(u)
    assert lib.ptx_read_guide(r.handle, 3, buf.ctypes.data, buf.nbytes) == 1
    assert lib.ptx_read_guide(r.handle, 0, None, buf.nbytes) == 1
    assert lib.ptx_read_guide(r.handle, 0, buf.ctypes.data, buf.nbytes - 16) == 1 and not buf.any()
    assert lib.ptx_read_guide(r.handle, 0, buf.ctypes.data, buf.nbytes) == 0 and buf.any()


# =====================================================================================================
# on the GPU: the filter
# =====================================================================================================
def _synthetic_sum(h, w, guides, samples=SAMPLES):
    """A noisy frame: albedo x a smooth light + noise, a hot pixel, a NaN and an Inf marker pixel (where the frame has room)."""
    rng = np.random.default_rng(h * 1000 + w)
    yy, xx = np.mgrid[0:h, 0:w]
    light = np.stack([0.4 + 0.5 * xx / w, 0.3 + 0.6 * yy / h, 0.5 + 0.0 * xx], axis=-1)
    S = np.zeros((h, w, 4), np.float32)
    S[..., 0:3] = guides[R.GUIDE_ALBEDO][..., 0:3] * light * rng.uniform(0.2, 1.8, (h, w, 3))
    S[(h // 2) % h, (w // 3) % w, 0:3] = 3000.0
    S[2 % h, 3 % w, 0] = np.nan
    S[4 % h, 5 % w, 1] = np.inf
    S[..., 0:3] *= samples
    S[..., 3] = samples
    return S


def _impulse_sum(h, w):
    S = np.zeros((h, w, 4), np.float32)
    S[h // 2, w // 2, 0:3] = np.float32([1.0, 2.0, 3.0]) * SAMPLES
    S[..., 3] = SAMPLES
    return S


_filter = {"frame": None, "guides": None, "sums": {}}


def _filter_state(pkg, frame, which):
    """The filter's renderer at `frame` (resized when the frame changes: guides rendered and read back once) with the sum `which`
    in its accumulation image.  Returns (renderer, guides, sum)."""
    s = _scene(pkg, FILTER_SCENE)[0]
    r = _renderer(pkg, FILTER_SCENE)
    w, h, _ = FRAMES[frame]
    if _filter["frame"] != frame or r.width != w or r.height != h:
        r.set_tile_shard(0, 1, 32)
        r.resize(w, h)
        _filter.update(frame=frame, guides=_guides(r, s.uniform(w, h)), sums={})
        for g in _filter["guides"]:
            g.setflags(write=False)
    guides, sums = _filter["guides"], _filter["sums"]
    if which not in sums:
        if which.startswith("render"):
            r.reset()
            for f in range(int(which[6:])):
                r.render(s.uniform(w, h, bounces=4, sample_count=1, total_samples=f), s.lights)
            sums[which] = r.readback()
        else:
            sums[which] = _synthetic_sum(h, w, guides) if which == "synthetic" else _impulse_sum(h, w)
        sums[which].setflags(write=False)
    r.write_accumulation(sums[which])
    return r, guides, sums[which]


def _samples_of(which):
    return int(which[6:]) if which.startswith("render") else SAMPLES


def _same_class(a, b):
    return (np.isnan(a) == np.isnan(b)).all() and (np.isposinf(a) == np.isposinf(b)).all() and (np.isneginf(a) == np.isneginf(b)).all()


@pytest.mark.gpu
@pytest.mark.parametrize("case", FILTER_CASES, ids=lambda c: "%s-%s" % c)
def test_filter_against_float64_reference(pkg, case):
    frame, which = case
    w, h, counts = FRAMES[frame]
    r, guides, S = _filter_state(pkg, frame, which)
    n = _samples_of(which)
    hit = guides[R.GUIDE_NORMAL][..., 3] == 1
    if frame in ("67x45", "300x200"):
        assert hit.sum() > 200 and (~hit).sum() > 20, "the frame must have filtered and passed-through pixels"
    for sc in SIGMA_COLORS:
        ref32 = R.denoise_all(S, *guides, n, max(counts), sc, SIGMA_NORMAL, SIGMA_POSITION, np.float32)
        ref64 = R.denoise_all(S, *guides, n, max(counts), sc, SIGMA_NORMAL, SIGMA_POSITION, np.float64)
        for it in counts:
            r.denoise(n, it, sc, SIGMA_NORMAL, SIGMA_POSITION)
            got = r.read_denoised()
            a, b = ref32[it - 1], ref64[it - 1]
            assert got.shape == b.shape and (got[..., 3] == 1).all()
            assert _same_class(a, b) and _same_class(got, b), (case, sc, it)
            fin = np.isfinite(b)
            worst = float(np.abs(a.astype(np.float64) - b)[fin].max())
            tol = np.maximum(8.0 * worst, 2.0 ** -20 * np.maximum(1.0, np.abs(b[fin])))
            err = np.abs(got.astype(np.float64)[fin] - b[fin])
            print(f"{case} sigmaColor {sc} iterations {it}: max |gpu - ref64| {err.max():.3e}, max |ref32 - ref64| {worst:.3e}, largest value {np.abs(b[fin]).max():.3e}")
            assert (err <= tol).all(), (case, sc, it, float(err.max()), worst)
            # pixels that are not filtered hold the mean, bit for bit
            valid = R.valid_mask(S, guides[0], guides[1], n, np.float32)
            assert (_bits(got[..., 0:3])[~valid] == _bits(R.mean_of(S, n, np.float32))[~valid]).all()
    assert (_bits(r.readback()) == _bits(S)).all()  # the sum is an input
    for k in range(3):
        assert (_bits(r.read_guide(k)) == _bits(guides[k])).all()  # ... and so are the guides


@pytest.mark.gpu
def test_filter_at_the_default_parameters_smooths_a_real_frame(pkg):
    r, guides, S = _filter_state(pkg, "67x45", "render1")
    r.denoise(1)
    got = r.read_denoised()
    d = pkg.DENOISE_DEFAULTS
    ref = R.denoise(S, *guides, 1, d["iterations"], d["sigma_color"], d["sigma_normal"], d["sigma_position"], np.float64)
    ref32 = R.denoise(S, *guides, 1, d["iterations"], d["sigma_color"], d["sigma_normal"], d["sigma_position"], np.float32)
    worst = float(np.abs(ref32.astype(np.float64) - ref).max())
    assert (np.abs(got - ref) <= np.maximum(8.0 * worst, 2.0 ** -20 * np.maximum(1.0, np.abs(ref)))).all()
    assert (_bits(got) != _bits(S)).any(axis=-1).sum() > 200


@pytest.mark.gpu
def test_denoised_output_stage_and_present(pkg):
    """ptx_postprocess_denoised = ptx_postprocess(TotalSamples 1) on a copy of the denoised image; ptx_present follows either."""
    r, guides, S = _filter_state(pkg, "67x45", "synthetic")
    r.denoise(SAMPLES, 3, 1.5, SIGMA_NORMAL, SIGMA_POSITION)
    D = r.read_denoised()
    assert r.denoised_ptr()
    f = pkg.Renderer()
    f.resize(W, H)
    f.write_accumulation(D)
    for tone in (pkg.TONE_MAPPING_SDR, pkg.TONE_MAPPING_HDR):
        r.postprocess_denoised(7, tone_mapping=tone, **POST)  # the uniform's TotalSamples is ignored: the image is a mean
        f.postprocess(1, tone_mapping=tone, **POST)
        for fmt in (pkg.OUTPUT_RGBA8_SRGB, pkg.OUTPUT_RGBA32F):
            a, b = r.read_output(fmt), f.read_output(fmt)
            assert a.dtype == b.dtype and (a.view(np.uint8) == b.view(np.uint8)).all(), (tone, fmt)
        for sw, sh, fmt, mode in ((W, H, pkg.PRESENT_R8G8B8A8_SRGB, 0), (100, 37, pkg.PRESENT_R16G16B16A16_SFLOAT, 0), (134, 90, pkg.PRESENT_A2B10G10R10_UNORM, 1)):
            r.present(sw, sh, fmt, mode)
            f.present(sw, sh, fmt, mode)
            a, b = r.read_present(), f.read_present()
            assert (a.view(np.uint8) == b.view(np.uint8)).all(), (tone, sw, sh, fmt)
    out = r.read_output(pkg.OUTPUT_RGBA32F)
    assert out[2, 3, 0] >= 1 and out[4, 5, 1] >= 1  # the NaN / Inf pixels still get postprocess.comp's markers
    f.close()
    assert (_bits(r.readback()) == _bits(S)).all() and (_bits(r.read_denoised()) == _bits(D)).all()
    # the plain output stage still reads the sum
    r.postprocess(SAMPLES, **POST)
    f = pkg.Renderer()
    f.resize(W, H)
    f.write_accumulation(S)
    f.postprocess(SAMPLES, **POST)
    assert (_bits(r.read_output(pkg.OUTPUT_RGBA32F)) == _bits(f.read_output(pkg.OUTPUT_RGBA32F))).all()
    f.close()


def _borrower(pkg, owner, S, u):
    b = pkg.Renderer()
    b.share_scene(owner)
    b.resize(S.shape[1], S.shape[0])
    b.write_accumulation(S)
    b.render_guides(u)
    return b


@pytest.mark.gpu
def test_two_denoise_calls_in_a_row_match_fresh_handles(pkg):
    r, guides, S = _filter_state(pkg, "67x45", "render8")
    u = _scene(pkg, FILTER_SCENE)[0].uniform(W, H)
    calls = ((8, 3, 0.0, SIGMA_NORMAL, SIGMA_POSITION), (8, 4, 1.5, 0.5, 0.02), (8, 1, 0.0, SIGMA_NORMAL, SIGMA_POSITION))
    got = []
    for c in calls:  # odd and even iteration counts: the result changes its buffer
        r.denoise(*c)
        got.append(r.read_denoised())
    assert (_bits(got[0]) != _bits(got[1])).any()
    for c, g in zip(calls, got):
        b = _borrower(pkg, r, S, u)
        b.denoise(*c)
        assert (_bits(b.read_denoised()) == _bits(g)).all(), c
        b.close()


@pytest.mark.gpu
def test_resize_drops_the_guides_and_the_denoised_image(pkg):
    r, guides, S = _filter_state(pkg, "33x22", "synthetic")
    lib = r.lib
    r.denoise(SAMPLES, 2)
    assert r.guide_ptr(0) and r.denoised_ptr()
    r.resize(33, 22)
    _filter["frame"] = None
    buf = np.zeros((22, 33, 4), np.float32)
    post = pkg.PostProcessingUniformData(1, 1.0, 1.0, 1.0)
    d = pkg.DenoiseDesc(SAMPLES, 2, 0.0, SIGMA_NORMAL, SIGMA_POSITION, 0, 0)
    assert not r.guide_ptr(0) and not r.denoised_ptr()
    assert lib.ptx_read_guide(r.handle, 0, buf.ctypes.data, buf.nbytes) == 5
    assert lib.ptx_read_denoised(r.handle, buf.ctypes.data, buf.nbytes) == 5 and not buf.any()
    assert lib.ptx_denoise(r.handle, C.byref(d)) == 5
    assert lib.ptx_postprocess_denoised(r.handle, C.byref(post), 0) == 5
    r.render_guides(_scene(pkg, FILTER_SCENE)[0].uniform(33, 22))
    assert lib.ptx_read_denoised(r.handle, buf.ctypes.data, buf.nbytes) == 5  # guides alone are no denoised image
    assert lib.ptx_postprocess_denoised(r.handle, C.byref(post), 0) == 5
    r.write_accumulation(S)
    r.denoise(SAMPLES, 2)
    assert lib.ptx_postprocess_denoised(r.handle, C.byref(post), 0) == 0


@pytest.mark.gpu
def test_denoise_refusals_leave_the_denoised_image_intact(pkg):
    import torch

    r, guides, S = _filter_state(pkg, "67x45", "synthetic")
    lib = r.lib
    r.denoise(SAMPLES, 3, 1.5, SIGMA_NORMAL, SIGMA_POSITION)
    D = r.read_denoised()

    def desc(total=SAMPLES, iterations=2, sc=0.0, sn=SIGMA_NORMAL, sp=SIGMA_POSITION, flags=0, reserved=0):
        return pkg.DenoiseDesc(total, iterations, sc, sn, sp, flags, reserved)

    def intact():
        assert (_bits(r.read_denoised()) == _bits(D)).all()

    nan, inf = float("nan"), float("inf")
    bad = [desc(iterations=0), desc(iterations=7), desc(iterations=0xFFFFFFFF), desc(total=0), desc(sc=-1.0), desc(sc=nan), desc(sc=inf), desc(sn=0.0),
           desc(sn=-0.3), desc(sn=nan), desc(sn=inf), desc(sp=0.0), desc(sp=-0.05), desc(sp=nan), desc(sp=inf), desc(flags=1), desc(reserved=1)]
    for d in bad:
        assert lib.ptx_denoise(r.handle, C.byref(d)) == 1, (d.totalSamples, d.iterations, d.sigmaColor, d.sigmaNormal, d.sigmaPosition, d.flags, d.reserved)
    assert lib.ptx_denoise(r.handle, None) == 1
    intact()
    buf = np.zeros((H, W, 4), np.float32)
    assert lib.ptx_read_denoised(r.handle, None, buf.nbytes) == 1
    assert lib.ptx_read_denoised(r.handle, buf.ctypes.data, buf.nbytes + 16) == 1 and not buf.any()
    post = pkg.PostProcessingUniformData(1, 1.0, 1.0, 1.0)
    assert lib.ptx_postprocess_denoised(r.handle, None, 0) == 1 and lib.ptx_postprocess_denoised(r.handle, C.byref(post), 2) == 1
    # a bound shard accumulation buffer, a tile shard of a larger world
    r.set_tile_shard(0, 2, 8)
    assert lib.ptx_denoise(r.handle, C.byref(desc())) == 5
    shard = torch.zeros(r.shard_bytes(0) // 4, dtype=torch.float32, device="cuda")
    r.bind_shard_accumulation(shard.data_ptr(), r.shard_bytes(0))
    assert lib.ptx_denoise(r.handle, C.byref(desc())) == 5
    r.bind_shard_accumulation(0)
    assert lib.ptx_denoise(r.handle, C.byref(desc())) == 5
    r.set_tile_shard(0, 1, 32)
    intact()
    # no image; an image without guides
    fresh = pkg.Renderer()
    assert lib.ptx_denoise(fresh.handle, C.byref(desc())) == 5
    fresh.resize(W, H)
    assert lib.ptx_denoise(fresh.handle, C.byref(desc())) == 5
    assert lib.ptx_read_denoised(fresh.handle, buf.ctypes.data, buf.nbytes) == 5 and not lib.ptx_device_denoised_ptr(fresh.handle)
    fresh.close()
    assert lib.ptx_denoise(r.handle, C.byref(desc())) == 0  # and the handle still works
    assert (_bits(r.read_denoised()) != _bits(D)).any()
