"""The oracle against the golden vectors generated from the REFERENCE's own GLSL
(tools/gen_golden.py; inputs include the grids of Path-Tracing-Tests/TestData.h)."""
import os

import numpy as np
import pytest

import util

# golden_libm is the INDEPENDENT build of the reference's GLSL text: glibc's sinf / cosf / powf / atan2f / asinf / expf and
# IEEE division, where the oracle (and golden_fixed) use the fixed polynomial kernels and the specified division
# a * rcp(b) (oracle/pt_oracle_math.h: <= 1.5 ULP, inside GLSL's 2.5-ULP latitude).  Functions that neither divide nor call a
# transcendental must agree bit for bit; the others within a few ULP (amplified where the GLSL subtracts nearly equal
# numbers, e.g. sqrt(1 - x^2 - y^2) at the rim of the disk, or intersects a ray differential with a grazing plane).
# Tolerance: |oracle - libm| / max(1, |libm|).
TOLERANCE = {"SchlickFresnel": 1e-6, "SampleGGX": 2e-6, "evaluateBSDF": 1e-6, "sampleBSDF": 5e-6,
             "sampleUniformDiskConcentric": 1e-6, "sampleCosineHemisphere": 2e-4, "constructPrimaryRayLens": 1e-6,
             "sampleLight": 1e-6, "missSkyboxTexCoords": 2e-7, "toneMapPixel": 2e-7,
             # division only (exact until round 5, when `/` became a * rcp(b)):
             "GGXDistribution": 5e-7, "Lambda": 5e-7, "GGXSmith": 5e-7, "DielectricFresnel": 5e-7, "EvaluateReflection": 5e-7,
             "EvaluateRefraction": 5e-7, "constructPrimaryRay": 1e-6, "computeDpDxy": 3e-6, "computeReflectedDifferentialRays": 1e-6,
             "computeRefractedDifferentialRays": 1e-6, "hdrToLdr": 5e-7, "postprocessPixel": 1e-6, "sampleMaterial": 1e-6,
             # normalize only (exact until round 6, when normalize(v) became v * rsq(dot): ONE rounding of 1 / sqrt where the libm
             # build rounds the root and then the reciprocal)
             "computeTangentSpace": 2e-7}
EXACT_WITH_LIBM = {"sampleLobePdfs", "rng", "offsetRayOriginSelfIntersection", "offsetRayOriginShadowTerminator",
                   "computeDpnDuv", "computeDerivatives", "computeLod", "compositionPixel"}


def test_oracle_bitexact_against_reference_glsl(orc):
    """Every restated function reproduces the reference's GLSL body bit for bit when the GLSL
    builtins follow the same arithmetic conventions (golden_fixed)."""
    for name, (fn, inp, exp) in util.load_golden("fixed").items():
        out = orc.test_eval(fn, inp, exp.shape[1])
        ok = util.bits_equal_or_both_nan(out, exp)
        assert ok.all(), f"{name}: {int((~ok).sum())} outputs differ"


def test_oracle_against_reference_glsl_with_libm(orc):
    """Same GLSL bodies with glibc's transcendentals and IEEE division: exact where neither is involved, within a small
    tolerance otherwise (independent check of the polynomial kernels and of the division convention)."""
    for name, (fn, inp, exp) in util.load_golden("libm").items():
        out = orc.test_eval(fn, inp, exp.shape[1])
        if name in EXACT_WITH_LIBM:
            assert util.bits_equal_or_both_nan(out, exp).all(), name
            continue
        assert name in TOLERANCE, f"{name}: neither exact nor toleranced"
        of, ef = out.view(np.float32), exp.view(np.float32)
        if name == "sampleBSDF":  # last column is the RNG state (integer): must be exact
            assert (out[:, 7] == exp[:, 7]).all()
            of, ef = of[:, :7], ef[:, :7]
        finite = np.isfinite(ef) & np.isfinite(of)
        assert (np.isfinite(ef) == np.isfinite(of)).mean() > 0.99
        err = np.abs(of[finite].astype(np.float64) - ef[finite]) / np.maximum(1.0, np.abs(ef[finite]))
        assert err.max() <= TOLERANCE[name], f"{name}: {err.max()}"


def test_oracle_raygen_loop_against_reference_main(orc):
    """Stage level: raygen.rgen's main() -- compiled from the reference's text with the trace calls scripted -- against
    the oracle's raygenPixel driven by the same script: the stored pixel, the number of primary and shadow trace calls
    and a hash of every ray handed to them.  Covers the draws per sample (pixel jitter, lens), the order of the radiance /
    throughput updates, the 0.001 gates, roulette, paths that end on a miss, and the NaN / inf restart of the sample loop."""
    import json
    import os

    for mode in ("fixed", "libm"):
        with util.open_golden(f"golden_stage_{mode}.json") as f:
            c = json.load(f)["raygenMain"]
        inp = np.array(c["in"], np.uint32).reshape(-1, c["nin"])
        exp = np.array(c["out"], np.uint32).reshape(-1, c["nout"])
        out = orc.test_raygen(inp)
        lens = inp[:, 7] != 0
        # exact in the fixed build; the libm build divides by IEEE (every case: the pixel coordinates are divided by the
        # resolution) and draws thin-lens cases through glibc's sin / cos: within a tolerance there
        exact = np.ones(len(inp), bool) if mode == "fixed" else np.zeros(len(inp), bool)
        ok = util.bits_equal_or_both_nan(out, exp).all(axis=1)
        assert ok[exact].all(), f"{mode}: {int((~ok[exact]).sum())} of {int(exact.sum())} cases differ"
        assert (out[:, 4:6] == exp[:, 4:6]).all(), "trace call counts"
        of, ef = out[~exact, :3].view(np.float32), exp[~exact, :3].view(np.float32)
        assert np.allclose(of, ef, rtol=1e-5, atol=1e-6)
        # the cases do exercise what they are meant to
        if mode == "fixed":
            calls0, calls1 = exp[:, 4].astype(int), exp[:, 5].astype(int)
            assert calls0.max() >= 12 and (calls0 == 0).any() and calls1.max() >= 3 and lens.sum() >= 50
            restarted = calls0 > inp[:, 5].astype(int) * np.maximum(inp[:, 6].astype(int), 1)
            assert restarted.sum() >= 5, "some scripts must poison a sample and make the loop start over"


def _one_triangle_scene(pkg, words):
    """PtxSceneDesc + lights of one closestHitMain case: a triangle with identity transforms, one material of the case's
    model, five 1 x 1 float textures (a lookup returns the texel, whatever the coordinates), 0..3 point lights."""
    import ctypes as C

    class Tex(C.Structure):
        _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("format", C.c_uint32), ("levels", C.c_uint32), ("data", C.c_void_p)]

    f = words.view(np.float32)
    keep = {}
    keep["v"] = np.ascontiguousarray(f[0:42])
    keep["i"] = np.uint32([0, 1, 2])
    ident = np.float32([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0])
    keep["t"] = ident.copy()
    if len(words) >= 174:  # closestHitMainTransformed: rows of the mesh transform, then of the instance transform
        keep["t"] = np.ascontiguousarray(f[150:162])
        ident = np.ascontiguousarray(f[162:174])
    keep["g"] = np.zeros(1, util.GEOMETRY_DT)
    keep["g"][0] = (0, 3, 0, 3, 1, 0, (0, 0))
    mtype, flip = int(words[42]), int(words[43])
    image = words[44:68].copy()
    first = 19 if mtype == 0 else 18  # the five texture indices of the 96-byte record (include/ptx.h)
    image[first:first + 5] += 9       # scene textures follow the nine default ones
    keep["m"] = image
    keep["mesh"] = np.zeros(1, util.MESH_DT)
    keep["mesh"][0] = (0, mtype, 0)
    keep["model"] = np.zeros(1, util.MODEL_DT)
    keep["model"][0] = (0, 1)
    keep["inst"] = np.zeros(1, util.INSTANCE_DT)
    keep["inst"][0] = (0, ident)
    keep["texels"] = [np.ascontiguousarray(f[68 + 4 * k:72 + 4 * k]) for k in range(5)]
    keep["tex"] = (Tex * 5)(*[Tex(1, 1, 2, 1, t.ctypes.data) for t in keep["texels"]])
    d = pkg.SceneDesc()
    d.vertices, d.vertexCount = keep["v"].ctypes.data, 3
    d.indices, d.indexCount = keep["i"].ctypes.data, 3
    d.transforms, d.transformCount = keep["t"].ctypes.data, 1
    d.geometries, d.geometryCount = keep["g"].ctypes.data, 1
    for k, (ptr, cnt) in enumerate((("metallicRoughnessMaterials", "metallicRoughnessMaterialCount"), ("specularGlossinessMaterials", "specularGlossinessMaterialCount"),
                                     ("phongMaterials", "phongMaterialCount"))):
        if k == mtype:
            setattr(d, ptr, keep["m"].ctypes.data)
            setattr(d, cnt, 1)
    d.meshes, d.meshCount = keep["mesh"].ctypes.data, 1
    d.models, d.modelCount = keep["model"].ctypes.data, 1
    d.instances, d.instanceCount = keep["inst"].ctypes.data, 1
    d.textures, d.textureCount = C.addressof(keep["tex"]), 5
    d.dxNormalTextures = flip
    d.textureMemoryBudget = 2**64 - 1
    L = pkg.LightsUbo()
    L.LightCount = int(words[88])
    for k in range(3):
        L.Directional.Direction[k], L.Directional.Color[k] = f[89 + k], f[92 + k]
    for n in range(3):
        b = 95 + 9 * n
        for k in range(3):
            L.Lights[n].Position[k], L.Lights[n].Color[k] = f[b + k], f[b + 3 + k]
        L.Lights[n].AttenuationConstant, L.Lights[n].AttenuationLinear, L.Lights[n].AttenuationQuadratic = f[b + 6], f[b + 7], f[b + 8]
    return d, L, keep


def test_oracle_closest_hit_against_reference_main(orc, pkg):
    """Stage level: closestHit.rchit's main() -- the reference's text over a one-triangle vertex buffer, with its own
    vertex fetch, interpolation and transform() -- against the oracle's closestHit on the same triangle, material, lights,
    hit and incoming payload: every payload field bit for bit (fixed build; the libm build within the tolerance of its
    transcendentals).  Covers the order of the RNG draws (BSDF lobe, then three for the light), hits from inside
    (flipped frame, Beer-Lambert on the hit distance, refracted origin and differential rays), the decal mix, the
    roughness ratchet, all three material models with DX normal maps, 0..3 point lights + the directional one."""
    import json
    import os

    for mode in ("fixed", "libm"):
        with util.open_golden(f"golden_stage_{mode}.json") as f:
            c = json.load(f)["closestHitMain"]
        inp = np.array(c["in"], np.uint32).reshape(-1, c["nin"])
        exp = np.array(c["out"], np.uint32).reshape(-1, c["nout"])
        assert inp.shape[1] == 150 and exp.shape[1] == 35 and len(inp) >= 300
        bad = loose = 0
        inside = refracted = decals = 0
        for row, want in zip(inp, exp):
            d, L, keep = _one_triangle_scene(pkg, row)
            got = orc.OracleScene(d, build_bvh=False).test_closest_hit(L, row[122:150])[0]
            wf = want.view(np.float32)
            inside += int(wf[10] != 0 and keep["m"].view(np.float32)[11 if int(row[42]) == 0 else 21] > 0)
            decals += int(row[133:134].view(np.float32)[0] != -1.0)
            if mode == "fixed":
                bad += int(not util.bits_equal_or_both_nan(got, want).all())
            else:
                assert got[14] == want[14], "RNG state"
                gf = got.view(np.float32)
                fin = np.isfinite(wf) & np.isfinite(gf)
                assert (np.isfinite(wf) == np.isfinite(gf)).all()
                err = np.abs(gf[fin].astype(np.float64) - wf[fin]) / np.maximum(1.0, np.abs(wf[fin]))
                err[14] = 0.0
                # one case of the 360 is ill-conditioned (a sampled refraction at the edge of its domain: Bsdf and Pdf come out
                # NEGATIVE, differences of nearly equal terms): there the last bit of a normalize() -- one rounding in rsq, two in
                # the libm build's 1 / sqrt -- shows as 4e-3; every other case stays inside the tolerance of the transcendentals
                loose += int(err.max() >= 2e-4)
                assert err.max() < 5e-3, float(err.max())
        assert bad == 0, f"{bad} of {len(inp)} payloads differ"
        assert loose <= 1
        assert decals >= 20


def test_oracle_closest_hit_with_transforms_bitexact(orc, pkg):
    """The ONE documented arithmetic deviation, quantified.  transform() (sampling.glsl:5-15) takes the normal through
    transpose(inverse(mat4(transform))) -- a 4 x 4 inverse per vertex; the oracle and the HIP kernels use the cofactor inverse
    of the 3 x 3 linear part (DevPair::Rinv), which is the same matrix in exact arithmetic.  Stage-level cases from the
    reference's closestHit.rchit text with a rotated, NON-UNIFORMLY scaled and translated mesh AND instance (the shim's
    4 x 4 cofactor inverse) against the oracle's closestHit on the same words.

    Until round 5 this was the one documented deviation (the shim divided every cofactor by the determinant, the oracle
    multiplied by its reciprocal: 107 of 240 cases bit-identical, the rest within 2e-6 ... 1.5e-4).  With the specified division
    a / b := a * rcp(b) both ARE cofactor * rcp(det), and for an affine matrix the 4 x 4 cofactors reduce to the 3 x 3 ones by
    products with 1 and sums with 0: every case is bit-identical now, and the test says so.  (-s prints the distribution.)"""
    import json
    import os

    with util.open_golden("golden_stage_fixed.json") as f:
        c = json.load(f)["closestHitMainTransformed"]
    inp = np.array(c["in"], np.uint32).reshape(-1, c["nin"])
    exp = np.array(c["out"], np.uint32).reshape(-1, c["nout"])
    assert inp.shape[1] == 174 and exp.shape[1] == 35 and len(inp) >= 200
    worst = []
    exact = 0
    for row, want in zip(inp, exp):
        d, L, keep = _one_triangle_scene(pkg, row)
        # the scales really are non-uniform: the normal matrix is not the rotation
        lin = row[150:162].view(np.float32).reshape(3, 4)[:, :3].astype(np.float64)
        sv = np.linalg.svd(lin, compute_uv=False)
        assert sv[0] / sv[-1] > 1.02
        got = orc.OracleScene(d, build_bvh=False).test_closest_hit(L, row[122:150])[0]
        assert got[14] == want[14], "RNG state"
        gf, wf = got.view(np.float32).astype(np.float64), want.view(np.float32).astype(np.float64)
        assert (np.isfinite(gf) == np.isfinite(wf)).all()
        fin = np.isfinite(wf)
        fin[14] = False
        err = np.abs(gf[fin] - wf[fin]) / np.maximum(1.0, np.abs(wf[fin]))
        worst.append(float(err.max()))
        exact += int(util.bits_equal_or_both_nan(got, want).all())
    worst = np.array(worst)
    print(f"closestHitMainTransformed: {len(worst)} cases, {exact} bit-identical, median of the worst field {np.median(worst):.2e}, "
          f"99th percentile {np.quantile(worst, 0.99):.2e}, max {worst.max():.2e}")
    assert exact == len(worst) and worst.max() == 0.0


def test_oracle_any_hit_against_reference_mains(orc, pkg):
    """Stage level: anyhit.rahit's and occlusionAnyhit.rahit's main() from the reference's text against the oracle's
    any-hit decisions for one candidate: ignored by the closest-hit query (alpha < 0.5), ignored by the shadow query
    (alpha < 1), and the decal the payload holds afterwards (replaced only by a nearer candidate)."""
    import ctypes as C
    import json
    import os

    with util.open_golden("golden_stage_fixed.json") as f:
        c = json.load(f)["anyHitMain"]
    inp = np.array(c["in"], np.uint32).reshape(-1, c["nin"])
    exp = np.array(c["out"], np.uint32).reshape(-1, c["nout"])
    assert len(inp) >= 300 and 0.2 < exp[:, 0].mean() < 0.8 and exp[:, 1].mean() > exp[:, 0].mean()
    replaced = 0
    for row, want in zip(inp, exp):
        # the closestHitMain scene builder wants 122 words: vertices, type, flag, material, five texels, lights
        words = np.zeros(150, np.uint32)
        words[0:42] = row[0:42]
        words[42] = row[42]
        words[44:68] = row[43:67]
        words[44 + (20 if int(row[42]) == 0 else 19)] = 1  # ColorIdx -> the second one-texel texture
        words[72:76] = row[67:71]
        d, L, keep = _one_triangle_scene(pkg, words)
        keep["g"][0]["IsOpaque"] = 0  # the any-hit stages run for non-opaque geometry only
        got = orc.OracleScene(d, build_bvh=False).test_any_hit(row[71:79])[0]
        assert util.bits_equal_or_both_nan(got[None], want[None]).all(), (row[71:79].view(np.float32), got, want)
        replaced += int(got[2] != row[74])
    assert replaced >= 50


def test_oracle_miss_against_reference_main(orc, pkg):
    """Stage level: miss.rmiss's main() from the reference's text against the oracle's miss stage: the clear colour, a
    2-D sky through hdrToLdr, a cube sky as it is, and Pdf = -1 in every case (one-texel sky images: the lookup itself is
    the sampler's business)."""
    import ctypes as C
    import json
    import os

    class Tex(C.Structure):
        _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("format", C.c_uint32), ("levels", C.c_uint32), ("data", C.c_void_p)]

    with util.open_golden("golden_stage_fixed.json") as f:
        c = json.load(f)["missMain"]
    inp = np.array(c["in"], np.uint32).reshape(-1, c["nin"])
    exp = np.array(c["out"], np.uint32).reshape(-1, c["nout"])
    assert len(inp) >= 90 and set(inp[:, 0].tolist()) == {0, 1, 2}
    for row, want in zip(inp, exp):
        texel = np.ascontiguousarray(row[4:8].view(np.float32))
        kind = int(row[0])
        sky = (Tex * 6)(*[Tex(1, 1, 2, 1, texel.ctypes.data) for _ in range(6)])
        d = pkg.SceneDesc()
        d.skyboxKind = kind
        d.skybox = C.addressof(sky) if kind else None
        got = orc.OracleScene(d, build_bvh=False).test_miss(row[1:4])[0]
        if kind == 2:  # the seamless bilinear blend of six equal 1 x 1 faces returns the texel up to the rounding of its lerps
            assert np.allclose(got.view(np.float32), want.view(np.float32), rtol=3e-7, atol=0), (got.view(np.float32), want.view(np.float32))
        else:
            assert (got == want).all(), (kind, got.view(np.float32), want.view(np.float32))


def test_reference_test_properties(orc):
    """The three properties the reference's own tests assert (ShadingTest.cpp: finite outputs on
    the TestData.h grids; BsdfTest.cpp:34-40: lobe weights sum to 1 within 4 ULP)."""
    g = util.load_golden("fixed")
    grids = {"GGXDistribution": 6, "Lambda": 6, "GGXSmith": 6, "DielectricFresnel": 4, "SchlickFresnel": 2,
             "EvaluateReflection": 54, "EvaluateRefraction": 108, "SampleGGX": 24}
    for name, n in grids.items():
        fn, inp, exp = g[name]
        out = orc.test_eval(fn, inp[:n], exp.shape[1]).view(np.float32)
        assert np.isfinite(out).all(), name
    fn, inp, exp = g["sampleLobePdfs"]
    assert inp.shape[0] == 125
    s = orc.test_eval(fn, inp, 4).view(np.float32).sum(axis=1, dtype=np.float32)
    assert np.all(np.abs(s - 1.0) <= 4 * np.finfo(np.float32).eps)


def test_rng_known_answers(orc, pkg):
    """jenkinsHash / initRng / xorshift / uintToFloat computed by hand from common.glsl:133-165."""
    def jenkins(x):
        x = (x + (x << 10)) & 0xFFFFFFFF
        x ^= x >> 6
        x = (x + (x << 3)) & 0xFFFFFFFF
        x ^= x >> 11
        x = (x + (x << 15)) & 0xFFFFFFFF
        return x

    cases = [(0, 0, 1920, 0), (1919, 1079, 1920, 7), (3839, 2159, 3840, 1023), (17, 5, 512, 3)]
    inp = np.array(cases, dtype=np.uint32)
    out = orc.test_eval(pkg.FN["rng"], inp, 5)
    for (px, py, w, frame), row in zip(cases, out):
        st = jenkins((px + py * w) ^ jenkins(frame))
        assert row[0] == st
        for k in range(4):
            st ^= (st << 13) & 0xFFFFFFFF
            st ^= st >> 17
            st ^= (st << 5) & 0xFFFFFFFF
            f = np.array([0x3F800000 | (st >> 9)], dtype=np.uint32).view(np.float32)[0] - np.float32(1.0)
            assert row[1 + k] == np.array([f], np.float32).view(np.uint32)[0]
            assert 0.0 <= f < 1.0


def test_analytic_checks(orc, pkg):
    """Checks the reference lacks: sampled-direction pdf consistency and normalised lobes."""
    rng = np.random.default_rng(3)
    n = 2000
    # sampleBSDF's pdf must equal evaluateBSDF's pdf for the direction it returned
    mat = np.zeros((n, 8), np.float32)
    mat[:, 0:3] = rng.uniform(0.1, 1.0, (n, 3))
    mat[:, 3] = rng.uniform(0.05, 1.0, n)
    mat[:, 4] = rng.choice([0.0, 1.0, 0.5], n)
    mat[:, 5] = rng.choice([0.0, 1.0, 0.3], n)
    mat[:, 6] = rng.choice([1.5, 1 / 1.5], n).astype(np.float32)
    V = rng.normal(size=(n, 3)).astype(np.float32)
    V[:, 2] = np.abs(V[:, 2]) + 0.05
    V /= np.linalg.norm(V, axis=1, keepdims=True)
    seeds = rng.integers(1, 2**32 - 1, n, dtype=np.uint32).view(np.float32).reshape(-1, 1)
    sb = orc.test_eval(pkg.FN["sampleBSDF"], np.concatenate([mat, V, seeds], axis=1), 8).view(np.float32)
    L = sb[:, 0:3]
    ok = np.isfinite(L).all(axis=1)
    ev = orc.test_eval(pkg.FN["evaluateBSDF"], np.concatenate([mat, V, L], axis=1)[ok], 4).view(np.float32)
    assert (ev[:, 3].view(np.uint32) == sb[ok, 3].view(np.uint32)).all()
    assert (ev[:, 0:3].view(np.uint32) == sb[ok, 4:7].view(np.uint32)).all()
    # cosine-hemisphere samples lie on the unit hemisphere; disk samples inside the unit disk
    u = rng.uniform(0, 1, (n, 2)).astype(np.float32)
    d = orc.test_eval(pkg.FN["sampleCosineHemisphere"], u, 3).view(np.float32)
    assert np.abs(np.linalg.norm(d, axis=1) - 1).max() < 2e-3 and (d[:, 2] >= 0).all()
    k = orc.test_eval(pkg.FN["sampleUniformDiskConcentric"], u, 2).view(np.float32)
    assert (np.linalg.norm(k, axis=1) <= 1 + 1e-6).all()
    # tangent frames are orthonormal
    nrm = rng.normal(size=(n, 3)).astype(np.float32)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    t = orc.test_eval(pkg.FN["computeTangentSpace"], nrm, 9).view(np.float32).reshape(-1, 3, 3)
    gram = np.einsum("nij,nkj->nik", t, t)
    assert np.abs(gram - np.eye(3)).max() < 1e-5


def test_golden_fixtures_regenerate_byte_for_byte_from_the_reference(tmp_path, orc):
    """The committed fixtures ARE what tools/gen_golden.py makes of the reference's shader text: where the reference tree is
    present the generator runs into a scratch directory, elsewhere the generators build() compiled from that text into oracle/_ref
    (oracle.build_ref) run, and every archive must come out byte-identical to tests/golden/.  A fixture edited by hand, a
    generator that drifted from the committed vectors, or a reference that changed under them fails here."""
    import gzip
    import subprocess
    import sys

    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    gen = os.path.join(repo, "tools", "gen_golden.py")
    sys.path.insert(0, os.path.join(repo, "tools"))
    import gen_golden

    if os.path.isdir(gen_golden.REF):
        cmd = [sys.executable, gen, "--out", str(tmp_path)]
    elif all(os.path.exists(os.path.join(orc.REF_DIR, "golden_" + m)) for m, _ in gen_golden.MODES):
        cmd = [sys.executable, gen, "--from-bin", orc.REF_DIR, "--out", str(tmp_path)]
    else:
        pytest.skip("neither the reference tree nor the generators compiled from it (oracle/_ref) are present")
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    made = sorted(f for f in os.listdir(tmp_path) if f.endswith(".json") or f.endswith(".json.gz"))
    committed = sorted(f for f in os.listdir(util.GOLDEN_DIR) if f.endswith(".json.gz"))
    assert committed and [m if m.endswith(".gz") else m + ".gz" for m in made] == committed, (made, committed)
    for m in made:
        new = open(os.path.join(tmp_path, m), "rb").read()
        new = gzip.decompress(new) if m.endswith(".gz") else new
        old = gzip.decompress(open(os.path.join(util.GOLDEN_DIR, m if m.endswith(".gz") else m + ".gz"), "rb").read())
        assert new == old, f"{m}: regenerated vectors differ from the committed fixture"


def test_specified_division_is_what_the_header_says(orc, pkg):
    """oracle/pt_oracle_math.h pto_rcp / pto_div (the `/` of the shader path): against the definition restated in numpy on all 2^23
    mantissas, every exponent, denormals, infinities and NaNs; the reciprocal is the correctly rounded one inside
    [2^-126, 2^126] (checked against float64), flushed outside; a / b stays within 1.5 ULP of the exact quotient -- inside the
    2.5 ULP GLSL grants a division."""
    b = util.reciprocal_inputs()
    rng = np.random.default_rng(5)
    a = rng.uniform(-4.0, 4.0, len(b)).astype(np.float32)
    out = orc.test_eval(pkg.FN["divide"], np.stack([a.view(np.uint32), b], axis=1), 2)
    spec = util.reciprocal_spec(b.view(np.float32))
    assert util.bits_equal_or_both_nan(out[:, 0], spec.view(np.uint32)).all()
    bf = b.view(np.float32)
    inside = np.isfinite(bf) & (np.abs(bf) >= np.float32(1.17549435e-38)) & (np.abs(bf) <= np.float32(8.50705917e37))
    exact = 1.0 / bf[inside].astype(np.float64)
    got = out[:, 0].view(np.float32)[inside]
    assert (got == exact.astype(np.float32)).all()  # float64 -> float32 of 1 / b: the correctly rounded reciprocal
    with np.errstate(all="ignore"):
        q = out[:, 1].view(np.float32)[inside].astype(np.float64)
        want = a[inside].astype(np.float64) / bf[inside].astype(np.float64)
        normal = np.abs(want) >= 1.17549435e-38
        ulp = np.spacing(np.abs(want[normal]).astype(np.float32)).astype(np.float64)
        assert (np.abs(q[normal] - want[normal]) <= 1.5 * ulp).all()
    outside = ~inside & ~np.isnan(bf)
    assert (np.isinf(out[:, 0].view(np.float32)[outside & (np.abs(bf) < 1)])).all()
    assert (out[:, 0].view(np.float32)[outside & (np.abs(bf) > 1)] == 0).all()


def _division_corner_pairs():
    """(a, b) pairs where a * rcp(b) is NOT the IEEE quotient's value (stated in pt_oracle_math.h): a zero numerator over a zero or
    denormal divisor (0 * inf = NaN; IEEE: 0 / denormal = 0), an infinite numerator over |b| > 2^126 (inf * 0 = NaN; IEEE: inf),
    x / x for |x| > 2^126 (x * 0 = 0; IEEE: 1) and for denormal x (inf; IEEE: 1)."""
    f = np.float32
    den = f(1e-40)
    big = f(1.5e38)
    a = np.array([0.0, -0.0, 0.0, 0.0, np.inf, -np.inf, big, -big, den, 1.0, 3.0, 0.0], np.float32)
    b = np.array([den, den, 0.0, -den, big, big, big, big, den, den, big, 2.0], np.float32)
    return a, b


def test_specified_division_corner_cases_are_the_stated_ones(orc, pkg):
    """The corner cases the a * rcp(b) convention answers differently from IEEE `/` are part of the specification (round-5
    advice): NaN for 0 / (zero or denormal) and inf / (|b| > 2^126), 0 for x / x beyond 2^126, inf for finite / denormal.  GLSL
    lets an implementation flush denormal operands, under which 0 / denormal IS 0 / 0; a NaN that reaches a pixel is what
    raygen.rgen:99-112 rejects (the launch's samples restart), so it cannot stay in the accumulation image."""
    a, b = _division_corner_pairs()
    out = orc.test_eval(pkg.FN["divide"], np.stack([a.view(np.uint32), b.view(np.uint32)], axis=1), 2)[:, 1].view(np.float32)
    assert np.isnan(out[:6]).all()                  # 0 / denormal, -0 / denormal, 0 / 0, 0 / -denormal, +-inf / big
    assert (out[6:8] == 0).all()                    # x / x, |x| > 2^126
    assert np.isinf(out[8]) and np.isinf(out[9])    # denormal / denormal, 1 / denormal
    assert out[10] == 0 and out[11] == 0            # 3 / big flushes to zero; 0 / 2 = 0 as ever


def test_specified_rsq_is_the_correctly_rounded_reciprocal_square_root(orc, pkg):
    """oracle/pt_oracle_math.h pto_rsq -- normalize(v) = v * rsq(dot(v, v)), inversesqrt = rsq (round 6): on the positive normal range
    it is the correctly rounded 1 / sqrt(x), checked against EXACT 128-bit integer arithmetic on all 2^24 (mantissa, exponent parity)
    classes (1 / sqrt(4^k x) = 2^-k / sqrt(x)); the device's float sequence (v_rsq_f32 seed + one compensated Newton step with the
    second-order term) run on the CPU from every seed the hardware's 1 ULP allows lands on the same float, so the definition does not
    depend on the seed.  Outside: +-inf for +-0 and denormals, +0 for +inf, NaN for negative numbers and NaN.  Inside GLSL's 2 ULP."""
    wrong, seed_dependent = orc.rsq_selfcheck()
    assert wrong == 0 and seed_dependent == 0
    f = np.float32
    x = np.array([0.0, -0.0, 1e-40, -1e-40, np.inf, -np.inf, -1.0, np.nan, 1.0, 4.0, 0.25, 2.0, 3.4028235e38, 1.17549435e-38], np.float32)
    out = orc.test_eval(pkg.FN["rsq"], x.view(np.uint32).reshape(-1, 1), 1)[:, 0].view(np.float32)
    assert out[0] == np.inf and out[1] == -np.inf and out[2] == np.inf and out[3] == -np.inf and out[4] == 0 and not np.signbit(out[4])
    assert np.isnan(out[5:8]).all()
    assert (out[8:11] == f([1.0, 0.5, 2.0])).all() and out[11] == f(0.70710678118654752) and out[12] == f(1.0 / np.sqrt(np.float64(f(3.4028235e38))))
    assert out[13] == f(2.0 ** 63)
    # every exponent, random mantissas: against float64 (1 / sqrt in double, rounded once -- exactly what the definition says)
    rng = np.random.default_rng(9)
    bits = ((np.arange(1, 255, dtype=np.uint32).repeat(4000) << 23) | rng.integers(0, 1 << 23, 254 * 4000, dtype=np.uint32)).astype(np.uint32)
    got = orc.test_eval(pkg.FN["rsq"], bits.reshape(-1, 1), 1)[:, 0].view(np.float32)
    want = (1.0 / np.sqrt(bits.view(np.float32).astype(np.float64))).astype(np.float32)
    assert (got == want).all()
    # normalize keeps unit length to 1 ULP-ish and agrees with the IEEE-divided form to 1.5 ULP
    v = rng.normal(size=(20000, 3)).astype(np.float32) * np.float32(10.0) ** rng.integers(-15, 15, (20000, 1)).astype(np.float32)
    d = ((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]).astype(np.float32) + v[:, 2] * v[:, 2]).astype(np.float32)
    r = orc.test_eval(pkg.FN["rsq"], d.view(np.uint32).reshape(-1, 1), 1)[:, 0].view(np.float32)
    n = v * r[:, None]
    assert np.abs(np.linalg.norm(n.astype(np.float64), axis=1) - 1.0).max() < 3e-7
