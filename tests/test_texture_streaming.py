"""Streamed scene textures (ptx_scene_upload_streamed / ptx_texture_upload / ptx_textures_commit / ptx_texture_residency):
a frame sees, for every texture, either exactly its 1 x 1 stand-in or exactly what a blocking upload of the same description
produces, and which of the two is fixed by the order of the calls.  Everything is compared bit for bit.  The oracle of a
pending state is the oracle run on a copy of the description in which each pending texture is a 1 x 1 RGBA8 texture holding
the stand-in's bytes (ShaderRendererTypes.incl:49-56), in the format of the stand-in's type."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import util

UNORM, SRGB, F32 = 0, 1, 2
W, H, SPP, DEPTH = 64, 48, 2, 4

# shader index -> (the texel as the reference writes it, little-endian RGBA; image format of that texture type)
STAND_IN = {
    0: (0xFFFFFFFF, SRGB),   # DefaultTextureColor
    1: (0xFFFF8080, UNORM),  # DefaultTextureNormal
    2: (0xFFFFFFFF, UNORM),  # DefaultTextureRoughness
    3: (0xFFFFFFFF, UNORM),  # DefaultTextureMetalness
    4: (0x00000000, SRGB),   # DefaultTextureEmissive
    5: (0xFFFFFFFF, SRGB),   # DefaultTextureSpecular
    6: (0x00000000, UNORM),  # DefaultTextureGlossiness
    7: (0x00000000, UNORM),  # DefaultTextureShininess
    8: (0xFFFFFFFF, SRGB),   # the placeholder: an opaque white colour texture
}
# the default of each of the five texture slots per material type; a colour texture waits behind the placeholder (Renderer.cpp:426-428)
SLOT_STAND_INS = {"mr": (4, 8, 1, 2, 3), "sg": (4, 8, 1, 5, 6), "phong": (4, 8, 1, 5, 7)}


def _inputs(idx, u, v, dudx=0.0, dvdx=0.0, dudy=0.0, dvdy=0.0):
    a = np.zeros((len(u), 7), np.float32)
    a.view(np.uint32)[:, 0] = idx
    a[:, 1], a[:, 2], a[:, 3], a[:, 4], a[:, 5], a[:, 6] = u, v, dudx, dvdx, dudy, dvdy
    return a


def _random_lookups(seed, n, first, last):
    """The generator of test_sampler_matches_oracle_bitexact over the shader indices first .. last - 1."""
    rng = np.random.default_rng(seed)
    idx = rng.integers(first, last, n).astype(np.uint32)
    uv = rng.uniform(-2.5, 3.5, (n, 2)).astype(np.float32)
    g = (10.0 ** rng.uniform(-5, 0.5, (n, 4)) * rng.choice([-1, 1], (n, 4))).astype(np.float32)
    g[:50] = 0
    g[50:60, 0] = np.nan
    g[60:70, 3] = np.inf
    uv[70:80, 0] = np.nan
    uv[80:90, 1] = 1e30
    return _inputs(idx, uv[:, 0], uv[:, 1], g[:, 0], g[:, 1], g[:, 2], g[:, 3])


def _textures(pkg, desc):
    return list((pkg.TextureDesc * desc.textureCount).from_address(desc.textures)) if desc.textureCount else []


def _with_textures(pkg, desc, table, budget=None):
    """A copy of `desc` with the texture table `table` (a list of TextureDesc); returns (desc, what must stay alive)."""
    arr = (pkg.TextureDesc * max(len(table), 1))()
    for i, t in enumerate(table):
        arr[i] = pkg.TextureDesc(t.width, t.height, t.format, t.levels, t.data)
    d = type(desc).from_buffer_copy(desc)
    d.textures = C.addressof(arr)
    d.textureCount = len(table)
    if budget is not None:
        d.textureMemoryBudget = budget
    return d, arr


def _pending_desc(pkg, desc, pending):
    table = _textures(pkg, desc)
    return _with_textures(pkg, desc, [pkg.TextureDesc(t.width, t.height, t.format, t.levels, None if i in pending else t.data) for i, t in enumerate(table)])


def _stand_in_desc(pkg, desc, pending, stand_in):
    """The description the oracle renders for a state in which the textures `pending` wait behind their stand-ins."""
    table = _textures(pkg, desc)
    texels = np.array([STAND_IN[int(k)][0] for k in stand_in], "<u4")
    out = []
    for i, t in enumerate(table):
        if i in pending:
            out.append(pkg.TextureDesc(1, 1, STAND_IN[int(stand_in[i])][1], 1, texels[i:].ctypes.data))
        else:
            out.append(t)
    d, arr = _with_textures(pkg, desc, out)
    return d, (arr, texels)


def _stand_ins_by_type(desc):
    """What Renderer.cpp:426-428 computes: per scene texture the placeholder if a material uses it as its colour texture, else
    the default of the slot that names it (a texture nothing names: the placeholder)."""
    n = desc.textureCount
    out = np.full(n, 8, np.uint32)
    for ptr, count, first, kind in ((desc.metallicRoughnessMaterials, desc.metallicRoughnessMaterialCount, 19, "mr"),
                                    (desc.specularGlossinessMaterials, desc.specularGlossinessMaterialCount, 18, "sg"),
                                    (desc.phongMaterials, desc.phongMaterialCount, 18, "phong")):
        if not ptr or not count:
            continue
        words = np.frombuffer((C.c_uint8 * (count * 96)).from_address(ptr), np.uint32).reshape(count, 24)
        for slot in (0, 2, 3, 4, 1):  # the colour slot last: it wins
            for idx in words[:, first + slot]:
                if 9 <= idx < 9 + n:
                    out[idx - 9] = SLOT_STAND_INS[kind][slot]
    return out


def _status(excinfo):
    return int(re.match(r"status (\d+)", str(excinfo.value)).group(1))


def _same(a, b):
    return bool((np.ascontiguousarray(a).view(np.uint32) == np.ascontiguousarray(b).view(np.uint32)).all())


def _frame(r, scene):
    """One launch of the tests' frame on `r` (accumulation cleared first): image and the counters the oracle also keeps."""
    r.resize(W, H)
    r.render(scene.uniform(W, H, bounces=DEPTH, sample_count=SPP), scene.lights)
    img = r.readback()
    st = r.stats()
    return img, (st.segments, st.shadowRays, st.retries, st.pathSamples)


_oracle_frames = {}


def _oracle_frame(orc, scene, desc, key):
    if key not in _oracle_frames:
        img, st = orc.OracleScene(desc).render(scene.uniform(W, H, bounces=DEPTH, sample_count=SPP), scene.lights, W, H)
        _oracle_frames[key] = (img, (st.segments, st.shadowRays, st.retries, st.pathSamples))
    return _oracle_frames[key]


def _upload_all(pkg, r, desc, order):
    table = _textures(pkg, desc)
    for i in order:
        r.upload_texture(i, table[i])


class _TexturedScene:
    """texture_test with every texture pending behind the stand-in of its type, and the descriptions of the mixed states."""

    def __init__(self, pkg, name="texture_test"):
        self.pkg = pkg
        self.scene = pkg.Scene(name)
        self.full = self.scene.desc
        self.n = self.full.textureCount
        self.stand_in = _stand_ins_by_type(self.full)
        self.keep = []

    def pending(self, which=None):
        d, keep = _pending_desc(self.pkg, self.full, set(range(self.n)) if which is None else set(which))
        self.keep.append(keep)
        return d

    def state(self, pending):
        d, keep = _stand_in_desc(self.pkg, self.full, set(pending), self.stand_in)
        self.keep.append(keep)
        return d


# ---------------------------------------------------------------------------------------
# 8. no GPU
# ---------------------------------------------------------------------------------------
def test_header_declares_and_package_exports_the_entry_points(pkg):
    header = open(os.path.join(pkg.REPO_DIR, "include", "ptx.h")).read()
    for name, args in (("ptx_scene_upload_streamed", r"PtxRenderer \*r, const PtxSceneDesc \*scene, const uint32_t \*standIn"),
                       ("ptx_texture_upload", r"PtxRenderer \*r, uint32_t index, const PtxTextureDesc \*desc"),
                       ("ptx_textures_commit", r"PtxRenderer \*r, uint32_t \*committed"),
                       ("ptx_texture_residency", r"PtxRenderer \*r, uint32_t \*resident, uint32_t \*pending")):
        assert re.search(r"PTX_API int " + name + r"\(" + args + r"\);", header), name
        assert name in pkg.PTX_SYMBOLS
        assert hasattr(pkg.load_hip(), name), name
    assert "#define PTX_ABI_VERSION 5u" in header  # additions only
    for method in ("upload_streamed", "upload_texture", "commit_textures", "texture_residency"):
        assert callable(getattr(pkg.Renderer, method))


def test_stand_in_bytes_decode_to_the_fixed_texels(pkg, orc):
    """The byte table above, as 1 x 1 textures of the stand-in's format, samples as sampleTexture(idx) of pt_device.hpp."""
    s = pkg.Scene("texture_test")
    texels = np.array([STAND_IN[k][0] for k in range(9)], "<u4")
    d, keep = _with_textures(pkg, s.desc, [pkg.TextureDesc(1, 1, STAND_IN[k][1], 1, texels[k:].ctypes.data) for k in range(9)])
    u = np.float32([0.0, 0.3, 7.5])
    got = orc.OracleScene(d, build_bvh=False).test_texture(_inputs(np.repeat(np.arange(9, 18), 3), np.tile(u, 9), np.tile(u, 9), dudx=0.1, dvdy=0.2))
    want = np.ones((9, 4), np.float32)
    want[1, :2] = np.float32(128.0) / np.float32(255.0)
    want[[4, 6, 7]] = 0.0
    assert _same(got.reshape(9, 3, 4), np.repeat(want[:, None], 3, axis=1))


# ---------------------------------------------------------------------------------------
# 1 - 3. texture_test: pending, streamed, partial
# ---------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("backend", [0, 1])
def test_pending_scene_equals_oracle_of_the_stand_in_scene(pkg, orc, backend):
    ts = _TexturedScene(pkg)
    assert sorted(set(ts.stand_in)) == [1, 2, 3, 4, 8]  # texture_test has a texture of every metallic-roughness slot
    r = pkg.Renderer(backend=backend)
    r.upload_streamed(ts.pending(), ts.stand_in)
    assert r.texture_residency() == (0, ts.n)
    stand = ts.state(range(ts.n))
    img, counters = _frame(r, ts.scene)
    ref, ref_counters = _oracle_frame(orc, ts.scene, stand, "texture_test/pending")
    assert counters == ref_counters
    assert _same(img, ref)
    osc = orc.OracleScene(stand, build_bvh=False)
    inp = _random_lookups(5, 20000, 9, 17)
    for implicit in (False, True):
        assert _same(r.test_texture(inp, implicit), osc.test_texture(inp, implicit)), implicit
    r.close()


@pytest.mark.gpu
def test_streamed_equals_blocking_equals_oracle(pkg, orc):
    ts = _TexturedScene(pkg)
    r = pkg.Renderer()
    r.upload_streamed(ts.pending(), ts.stand_in)
    assert r.texture_residency() == (0, ts.n)
    _upload_all(pkg, r, ts.full, reversed(range(ts.n)))
    # uploaded, not committed: nothing a frame sees has changed
    assert r.texture_residency() == (0, ts.n)
    img, counters = _frame(r, ts.scene)
    ref, ref_counters = _oracle_frame(orc, ts.scene, ts.state(range(ts.n)), "texture_test/pending")
    assert counters == ref_counters and _same(img, ref)
    assert r.commit_textures() == ts.n
    assert r.texture_residency() == (ts.n, 0)
    assert r.commit_textures() == 0
    img, counters = _frame(r, ts.scene)
    ref, ref_counters = _oracle_frame(orc, ts.scene, ts.full, "texture_test/full")
    assert counters == ref_counters and _same(img, ref)
    blocking = pkg.Renderer()
    blocking.upload(ts.scene)
    assert blocking.texture_residency() == (ts.n, 0)
    bimg, bcounters = _frame(blocking, ts.scene)
    assert bcounters == counters and _same(bimg, img)
    osc = orc.OracleScene(ts.full, build_bvh=False)
    inp = _random_lookups(5, 20000, 9, 17)
    for implicit in (False, True):
        a = r.test_texture(inp, implicit)
        assert _same(a, blocking.test_texture(inp, implicit)) and _same(a, osc.test_texture(inp, implicit)), implicit
    blocking.close()
    r.close()


@pytest.mark.gpu
def test_partial_and_incremental_commits(pkg, orc):
    ts = _TexturedScene(pkg)
    r = pkg.Renderer()
    r.upload_streamed(ts.pending(), ts.stand_in)
    first, rest = list(range(0, ts.n, 2)), list(range(1, ts.n, 2))
    _upload_all(pkg, r, ts.full, first)
    assert r.commit_textures() == len(first)
    assert r.texture_residency() == (len(first), len(rest))
    mixed = ts.state(rest)
    img, counters = _frame(r, ts.scene)
    ref, ref_counters = _oracle_frame(orc, ts.scene, mixed, "texture_test/odd pending")
    assert counters == ref_counters and _same(img, ref)
    inp = _random_lookups(6, 5000, 9, 17)
    assert _same(r.test_texture(inp), orc.OracleScene(mixed, build_bvh=False).test_texture(inp))
    _upload_all(pkg, r, ts.full, rest)
    assert r.commit_textures() == len(rest)
    assert r.texture_residency() == (ts.n, 0)
    img, counters = _frame(r, ts.scene)
    ref, ref_counters = _oracle_frame(orc, ts.scene, ts.full, "texture_test/full")
    assert counters == ref_counters and _same(img, ref)
    r.close()


@pytest.mark.gpu
def test_a_texture_that_came_with_its_data_is_resident_at_once(pkg, orc):
    ts = _TexturedScene(pkg)
    r = pkg.Renderer()
    rest = list(range(1, ts.n, 2))
    r.upload_streamed(ts.pending(rest), ts.stand_in)
    assert r.texture_residency() == (ts.n - len(rest), len(rest))
    img, counters = _frame(r, ts.scene)
    ref, ref_counters = _oracle_frame(orc, ts.scene, ts.state(rest), "texture_test/odd pending")
    assert counters == ref_counters and _same(img, ref)
    r.close()


# ---------------------------------------------------------------------------------------
# 4. the chain kernel at the shapes where it can go wrong
# ---------------------------------------------------------------------------------------
_SHAPES = [(1, 1), (2, 2), (64, 64), (128, 64), (256, 1), (96, 96), (65, 33), (160, 96)]
# per-texture budgets of test_upload_rules_match_oracle_bitexact (_BUDGET_32 / 6 and _BUDGET_32 // 5 / 6): 8-bit textures are
# held to 32 and 8 texels across, float textures to 16 and 4
_BUDGETS = (6000, 1200)


def _chain_cases():
    """(id, width, height, format, levels in the data, budget, texels): one-texture scenes."""
    rng = np.random.default_rng(41)
    cases = []
    for w, h in _SHAPES:
        for fmt in (UNORM, SRGB, F32):
            data = rng.uniform(0, 4, (h, w, 4)).astype(np.float32) if fmt == F32 else rng.integers(0, 256, (h, w, 4)).astype(np.uint8)
            cases.append((f"{w}x{h}-{('unorm', 'srgb', 'f32')[fmt]}", w, h, fmt, 1, 2**64 - 1, data.reshape(-1)))
    bad = rng.uniform(0, 4, (8, 8, 4)).astype(np.float32)
    bad[2, 3, 0], bad[5, 6, 1], bad[7, 0, 3] = np.inf, np.nan, -np.inf
    cases.append(("8x8-f32-nonfinite", 8, 8, F32, 1, 2**64 - 1, bad.reshape(-1)))
    for w, h in ((100, 60), (256, 256)):
        for budget in _BUDGETS:
            cases.append((f"{w}x{h}-srgb-budget{budget}", w, h, SRGB, 1, budget, rng.integers(0, 256, (h, w, 4)).astype(np.uint8).reshape(-1)))
    cases.append(("100x60-f32-budget6000", 100, 60, F32, 1, 6000, rng.uniform(0, 4, (60, 100, 4)).astype(np.float32).reshape(-1)))
    # files that carry their own complete chain: used level by level; under a budget from the level that fits
    chain = lambda w, h: np.concatenate([rng.integers(0, 256, (max(h >> l, 1), max(w >> l, 1), 4)).astype(np.uint8).reshape(-1)  # noqa: E731
                                         for l in range(int(np.log2(max(w, h))) + 1)])
    cases.append(("8x8-unorm-filechain", 8, 8, UNORM, 4, 2**64 - 1, chain(8, 8)))
    cases.append(("64x64-srgb-filechain-budget6000", 64, 64, SRGB, 7, 6000, chain(64, 64)))
    return cases


_CASES = _chain_cases()


def _chain_lookups(w, h, seed):
    """Texel centres of every level with the gradients of that level's LOD (2^l texels per pixel), plus 5000 random lookups:
    the extents are those of the unscaled image, so a scaled texture is met between its levels as well."""
    rng = np.random.default_rng(seed)
    rows = []
    levels = int(np.log2(max(w, h))) + 1
    for l in range(levels):
        lw, lh = max(w >> l, 1), max(h >> l, 1)
        ys, xs = np.mgrid[0:lh, 0:lw]
        xs, ys = xs.reshape(-1), ys.reshape(-1)
        if len(xs) > 4096:
            pick = rng.choice(len(xs), 4096, replace=False)
            xs, ys = xs[pick], ys[pick]
        rows.append(_inputs(9, (xs + 0.5) / lw, (ys + 0.5) / lh, dudx=np.float32(2.0 ** l / w), dvdy=np.float32(2.0 ** l / h)))
    rows.append(_random_lookups(seed + 1, 5000, 9, 10))
    return np.concatenate(rows)


def _chain_desc(pkg, base, case):
    _, w, h, fmt, levels, budget, data = case
    return _with_textures(pkg, base.desc, [pkg.TextureDesc(w, h, fmt, levels, data.ctypes.data)], budget=budget)


def _streamed_chain(pkg, r, base, case, inp):
    d, keep = _chain_desc(pkg, base, case)
    pend, keep2 = _pending_desc(pkg, d, {0})
    r.upload_streamed(pend, None, build=False)
    r.upload_texture(0, _textures(pkg, d)[0])
    assert r.commit_textures() == 1
    return r.test_texture(inp), r.test_texture(inp, True)


def _levelwise_child(out_path):
    """Runs in a child process started with PTX_STREAM_LEVELWISE=1 (the library reads its switches when a handle is created)."""
    import conftest

    pkg = conftest.graft.load_package()
    import torch  # noqa: F401

    base = pkg.Scene("texture_test")
    r = pkg.Renderer()
    out = {}
    for k, case in enumerate(_CASES):
        a, b = _streamed_chain(pkg, r, base, case, _chain_lookups(case[1], case[2], 100 + k))
        out[f"grad{k}"], out[f"lod0_{k}"] = a, b
    r.close()
    np.savez(out_path, **out)


@pytest.fixture(scope="module")
def levelwise_results(pkg, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("levelwise") / "levelwise.npz")
    here = os.path.dirname(os.path.abspath(__file__))
    code = f"import sys; sys.path.insert(0, {here!r}); import test_texture_streaming as t; t._levelwise_child({out!r})"
    env = dict(os.environ, PTX_STREAM_LEVELWISE="1")
    done = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stderr[-2000:]
    return np.load(out)


@pytest.fixture(scope="module")
def fused_renderer(pkg):
    import torch  # noqa: F401

    before = os.environ.get("PTX_STREAM_LEVELWISE")
    os.environ["PTX_STREAM_LEVELWISE"] = "0"
    try:
        r = pkg.Renderer()
    finally:
        if before is None:
            del os.environ["PTX_STREAM_LEVELWISE"]
        else:
            os.environ["PTX_STREAM_LEVELWISE"] = before
    yield r
    r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(len(_CASES)), ids=[c[0] for c in _CASES])
def test_chain_fused_and_levelwise_equal_blocking_and_oracle(pkg, orc, gpu_renderer, fused_renderer, levelwise_results, k):
    case = _CASES[k]
    base = pkg.Scene("texture_test")
    inp = _chain_lookups(case[1], case[2], 100 + k)
    d, keep = _chain_desc(pkg, base, case)
    osc = orc.OracleScene(d, build_bvh=False)
    want = osc.test_texture(inp), osc.test_texture(inp, True)
    gpu_renderer._check(gpu_renderer.lib.ptx_scene_upload(gpu_renderer.handle, C.byref(d)))
    blocking = gpu_renderer.test_texture(inp), gpu_renderer.test_texture(inp, True)
    fused = _streamed_chain(pkg, fused_renderer, base, case, inp)
    levelwise = levelwise_results[f"grad{k}"], levelwise_results[f"lod0_{k}"]
    for name, got in (("blocking", blocking), ("fused", fused), ("levelwise", levelwise)):
        for which in (0, 1):
            ok = util.bits_equal_or_both_nan(got[which], want[which])  # (how the sampler tests compare non-finite results)
            assert ok.all(), f"{case[0]}, {name}: {int((~ok).any(axis=1).sum())} of {len(inp)} lookups differ from the oracle (implicit LOD {which})"
            assert (got[which] == blocking[which]).all() or "nonfinite" in case[0], f"{case[0]}, {name} differs from the blocking upload"


# ---------------------------------------------------------------------------------------
# 5. any-hit: the colour textures of non-opaque geometry
# ---------------------------------------------------------------------------------------
def _check_rays_and_frame(pkg, orc, r, ts, desc, key, label):
    rays = util.random_rays(np.random.default_rng(21), 8000, -4.0, 4.0)
    rays[:, 1] = np.abs(rays[:, 1])
    if key + "/rays" not in _oracle_frames:
        osc = orc.OracleScene(desc, build_bvh=False)
        _oracle_frames[key + "/rays"] = (osc.trace_closest(rays, brute_force=True), osc.trace_any(rays, brute_force=True))
    ref, occ_ref = _oracle_frames[key + "/rays"]
    hits, ids = r.trace_rays(rays, any_hit=False)
    gid = util.global_ids(desc, ids)
    assert (gid == ref["tri"]).all(), f"{label}: {int((gid != ref['tri']).sum())} rays hit a different triangle"
    h = gid != 0xFFFFFFFF
    assert h.sum() > 2000
    for k, f in enumerate(("t", "u", "v")):
        assert _same(hits[h, k], ref[f][h]), (label, f)
    occ, _ = r.trace_rays(rays, any_hit=True)
    assert ((occ[:, 3] != 0) == (occ_ref != 0)).all(), label
    img, counters = _frame(r, ts.scene)
    want, want_counters = _oracle_frame(orc, ts.scene, desc, key)
    assert counters == want_counters and _same(img, want), label
    return ref, occ_ref


@pytest.mark.gpu
def test_any_hit_pending_then_committed_after_the_build(pkg, orc):
    ts = _TexturedScene(pkg, "alpha_test")
    assert ts.n and (ts.stand_in == 8).all()  # alpha_test's textures are colour textures
    r = pkg.Renderer()
    r.upload_streamed(ts.pending(), ts.stand_in)
    pend = _check_rays_and_frame(pkg, orc, r, ts, ts.state(range(ts.n)), "alpha_test/pending", "pending")
    _upload_all(pkg, r, ts.full, range(ts.n))
    assert r.commit_textures() == ts.n
    full = _check_rays_and_frame(pkg, orc, r, ts, ts.full, "alpha_test/full", "committed")
    # the stand-in is opaque where the textures cut holes: the two states must differ for the test to mean anything
    assert (pend[0]["tri"] != full[0]["tri"]).any() and (pend[1] != full[1]).any()
    it, _ = ts.scene.animation_state()
    r.update_animation(instance_transforms=it)  # a refit with unchanged transforms rewrites the any-hit records
    _check_rays_and_frame(pkg, orc, r, ts, ts.full, "alpha_test/full", "refit after the commit")
    r.close()


@pytest.mark.gpu
def test_any_hit_committed_before_the_build(pkg, orc):
    ts = _TexturedScene(pkg, "alpha_test")
    r = pkg.Renderer()
    r.upload_streamed(ts.pending(), ts.stand_in, build=False)
    _upload_all(pkg, r, ts.full, range(ts.n))
    assert r.commit_textures() == ts.n
    r._check(r.lib.ptx_build_accel(r.handle))
    _check_rays_and_frame(pkg, orc, r, ts, ts.full, "alpha_test/full", "committed before the build")
    r.close()


# ---------------------------------------------------------------------------------------
# 6. a borrower sees the owner's commits, from its next frame on
# ---------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["texture_test", "alpha_test"])
def test_borrower_follows_the_owners_commit(pkg, orc, name):
    ts = _TexturedScene(pkg, name)
    owner, borrower = pkg.Renderer(), pkg.Renderer()
    owner.upload_streamed(ts.pending(), ts.stand_in)
    borrower.share_scene(owner)
    assert borrower.texture_residency() == (0, ts.n)
    img, counters = _frame(borrower, ts.scene)
    ref, ref_counters = _oracle_frame(orc, ts.scene, ts.state(range(ts.n)), name + "/pending")
    assert counters == ref_counters and _same(img, ref)
    with pytest.raises(pkg.PtxError) as e:
        borrower.upload_texture(0, _textures(pkg, ts.full)[0])
    assert _status(e) == 1
    with pytest.raises(pkg.PtxError) as e:
        borrower.commit_textures()
    assert _status(e) == 1
    _upload_all(pkg, owner, ts.full, range(ts.n))
    assert owner.commit_textures() == ts.n
    assert borrower.texture_residency() == (ts.n, 0)
    borrower.reset()
    img, counters = _frame(borrower, ts.scene)
    ref, ref_counters = _oracle_frame(orc, ts.scene, ts.full, name + "/full")
    assert counters == ref_counters and _same(img, ref)
    owner.close()
    with pytest.raises(pkg.PtxError) as e:  # a borrower without its owner has no scene
        borrower.upload_texture(0, _textures(pkg, ts.full)[0])
    assert _status(e) == 5
    borrower.close()


# ---------------------------------------------------------------------------------------
# 7. refusals leave the handle as it was
# ---------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refusals_leave_the_handle_as_it_was(pkg, orc):
    ts = _TexturedScene(pkg)
    table = _textures(pkg, ts.full)
    r = pkg.Renderer()
    r.upload_streamed(ts.pending(), ts.stand_in)
    r.upload_texture(2, table[2])
    pending_img, _ = _frame(r, ts.scene)
    assert _same(pending_img, _oracle_frame(orc, ts.scene, ts.state(range(ts.n)), "texture_test/pending")[0])
    t = table[1]
    refused = {
        "wrong extent": (1, pkg.TextureDesc(t.width + 1, t.height, t.format, t.levels, t.data)),
        "wrong format": (1, pkg.TextureDesc(t.width, t.height, UNORM if t.format == SRGB else SRGB, t.levels, t.data)),
        "wrong level count": (1, pkg.TextureDesc(t.width, t.height, t.format, 3, t.data)),
        "null data": (1, pkg.TextureDesc(t.width, t.height, t.format, t.levels, None)),
        "index equal to textureCount": (ts.n, table[ts.n - 1]),
        "a second upload of the same index": (2, table[2]),
    }
    for why, (index, desc) in refused.items():
        with pytest.raises(pkg.PtxError) as e:
            r.upload_texture(index, desc)
        assert _status(e) == 1, why
        assert r.texture_residency() == (0, ts.n), why
        assert _same(_frame(r, ts.scene)[0], pending_img), why
    bad = ts.stand_in.copy()
    bad[3] = 9
    with pytest.raises(pkg.PtxError) as e:
        r.upload_streamed(ts.pending(), bad)
    assert _status(e) == 1
    assert r.texture_residency() == (0, ts.n) and _same(_frame(r, ts.scene)[0], pending_img)
    # the refused calls have not disturbed the upload that was accepted
    assert r.commit_textures() == 1
    assert _same(_frame(r, ts.scene)[0], _oracle_frame(orc, ts.scene, ts.state(set(range(ts.n)) - {2}), "texture_test/all but 2 pending")[0])
    with pytest.raises(pkg.PtxError) as e:
        r.upload_texture(2, table[2])  # committed: not pending any more
    assert _status(e) == 1
    # after a plain upload there is nothing to stream into
    r.upload(ts.scene)
    full_img, _ = _frame(r, ts.scene)
    with pytest.raises(pkg.PtxError) as e:
        r.upload_texture(1, table[1])
    assert _status(e) == 1
    with pytest.raises(pkg.PtxError) as e:
        r.commit_textures()
    assert _status(e) == 1
    assert r.texture_residency() == (ts.n, 0)
    assert _same(_frame(r, ts.scene)[0], full_img) and _same(full_img, _oracle_frame(orc, ts.scene, ts.full, "texture_test/full")[0])
    r.close()
