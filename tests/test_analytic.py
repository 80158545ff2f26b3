"""Independent evidence for the stage-level code of the oracle (raygen.rgen / closestHit.rchit restated by reading, with
no golden vectors in the reference to pin them): closed-form and quadrature checks computed here in float64 from the
PUBLISHED formulas, not from the oracle's own functions.

  * closed forms of the metallic lobe at alpha = 1 (albedo 1 - ln 2, pdf mass 1 / 2) and energy / pdf-mass bounds of the
    whole mixture (bsdf.glsl:72-103 with the lobe weights of :62-70): physical where the reference's BSDF is (entering
    side, no transmission), a characterisation of its quirks elsewhere (clamped D, eta^2 on leaving refractions),
  * Helmholtz reciprocity of the reflection lobes,
  * a direct-light pixel in closed form: Lambert-like plane, one directional light, N dark point lights, BounceCount 1:
    checks the 1 / (N + 1) light-selection normalisation (sampling.glsl:27-28) and that NEE uses the PRE-update
    throughput (raygen.rgen:79-84),
  * Beer-Lambert through a glass slab against a constant sky: F + (1 - F)^2 a / (1 - F a) with
    a = AttenuationColor^(T / AttenuationDistance) (closestHit.rchit:123-128), which also exercises Fresnel lobe
    selection, the refracted-origin offset and Russian roulette (raygen.rgen:86-93) as an unbiased estimator.
"""
import ctypes as C

import numpy as np
import pytest

import util

PI = np.pi


# ---------------------------------------------------------------------------------------
# function level: quadrature over the sphere of directions
# ---------------------------------------------------------------------------------------
def _sphere_grid(n_theta=400, n_phi=256):
    """Midpoint rule in (cos theta, phi) over the full sphere: directions and the solid angle of a cell."""
    ct = (np.arange(2 * n_theta) + 0.5) / (2 * n_theta) * 2.0 - 1.0
    ph = (np.arange(n_phi) + 0.5) / n_phi * 2.0 * PI
    CT, PH = np.meshgrid(ct, ph, indexing="ij")
    st = np.sqrt(1.0 - CT * CT)
    L = np.stack([st * np.cos(PH), st * np.sin(PH), CT], axis=-1).reshape(-1, 3)
    return L.astype(np.float32), (2.0 / (2 * n_theta)) * (2.0 * PI / n_phi)


def _evaluate(orc, pkg, color, rough, metal, trans, eta, V, L):
    n = L.shape[0]
    mat = np.zeros((n, 8), np.float32)
    mat[:, 0:3], mat[:, 3], mat[:, 4], mat[:, 5], mat[:, 6] = color, rough, metal, trans, eta
    Vn = np.broadcast_to(np.asarray(V, np.float32), (n, 3))
    out = orc.test_eval(pkg.FN["evaluateBSDF"], np.concatenate([mat, Vn, L], axis=1), 4).view(np.float32)
    return out[:, 0:3].astype(np.float64), out[:, 3].astype(np.float64)


def _view(theta_deg):
    t = np.radians(theta_deg)
    return np.float32([np.sin(t), 0.0, np.cos(t)])


def test_metallic_lobe_closed_forms(pkg, orc):
    """alpha = 1 (roughness 1), V = normal, white metal: D = 1 / pi, G1(V) = 1, G1(L) = 2 cos / (1 + cos), F = 1, so
      albedo = int D G / (4 V.z) dw = 1 - ln 2           (shading.glsl:56-77 integrated by hand)
      int pdf = 1 / 2                                     (VNDF mass whose reflection stays above the horizon: sin^2 45)
    and neither depends on eta (the metallic lobe has no dielectric Fresnel)."""
    L, dw = _sphere_grid()
    res = []
    for eta in (1.0 / 1.5, 1.5):
        f, pdf = _evaluate(orc, pkg, 1.0, 1.0, 1.0, 0.0, eta, _view(0.0), L)
        res.append((f.sum(axis=0) * dw, pdf.sum() * dw))
    assert np.abs(res[0][0] - (1.0 - np.log(2.0))).max() <= 2e-3 and abs(res[0][1] - 0.5) <= 2e-3
    assert np.allclose(res[0][0], res[1][0], rtol=0, atol=1e-12) and res[0][1] == res[1][1]


@pytest.mark.parametrize("metal,trans", [(0.0, 0.0), (1.0, 0.0), (0.5, 0.0), (0.0, 1.0), (0.3, 0.6)])
def test_white_furnace_and_pdf_mass(pkg, orc, metal, trans):
    """Energy and pdf mass of the whole mixture (bsdf.glsl:72-103).  The reference's BSDF is not a textbook one -- D is
    clamped to 1 (shading.glsl:13), the lobe weights follow the Fresnel term of the half vector OF L (so the "mixture" is
    not a convex combination of densities), a leaving refraction (eta > 1) carries the eta^2 radiance factor -- so the
    bounds below are the physical one where it applies and a characterisation elsewhere; a restatement that dropped a
    cosine, a 1 / pi or a lobe weight would leave them by integer factors."""
    L, dw = _sphere_grid()
    for rough in (0.3, 0.5, 0.8, 1.0):
        for theta in (0.0, 35.0, 60.0, 80.0):
            V = _view(theta)
            for eta in (1.0 / 1.5, 1.5):
                f, pdf = _evaluate(orc, pkg, 1.0, rough, metal, trans, eta, V, L)
                assert np.isfinite(f).all() and np.isfinite(pdf).all() and (f >= 0).all() and (pdf >= 0).all()
                albedo = (f.sum(axis=0) * dw).max()  # evaluateBSDF already carries the cosine (bsdf.glsl:14, shading.glsl:76)
                mass = pdf.sum() * dw
                up = L[:, 2] > 0
                if trans == 0.0:
                    assert f[~up].max() == 0.0 and pdf[~up].max() == 0.0      # nothing below the surface
                    if eta < 1.0:
                        assert 0.25 <= albedo <= 1.03, (rough, theta, albedo)  # entering side: energy conserving (1 + quadrature)
                    assert albedo <= 1.08 and 0.25 <= mass <= 1.12, (rough, theta, eta, albedo, mass)
                else:
                    assert f[~up].sum() > 0.0                                     # the transmissive lobe is below
                    bound = 1.03 if eta < 1.0 else 2.25 * 1.03                    # eta^2 on the way out
                    assert albedo <= bound and mass <= 2.25 * 1.06, (rough, theta, eta, albedo, mass)
                if rough <= 0.3 and metal == 1.0:
                    assert mass < 0.35   # the documented quirk: the clamped D under-counts a sharp lobe (pi alpha^2 = 0.025)


def test_reflection_lobes_are_reciprocal(pkg, orc):
    rng = np.random.default_rng(4)
    n = 4000
    V = rng.normal(size=(n, 3)).astype(np.float32)
    L = rng.normal(size=(n, 3)).astype(np.float32)
    for A in (V, L):
        A[:, 2] = np.abs(A[:, 2]) + 0.05
        A /= np.linalg.norm(A, axis=1, keepdims=True)
    mat = np.zeros((n, 8), np.float32)
    mat[:, 0:3] = rng.uniform(0.1, 1.0, (n, 3))
    mat[:, 3] = rng.uniform(0.2, 1.0, n)
    mat[:, 4] = rng.choice([0.0, 0.4, 1.0], n)
    mat[:, 6] = 1.0 / 1.5
    a = orc.test_eval(pkg.FN["evaluateBSDF"], np.concatenate([mat, V, L], axis=1), 4).view(np.float32)[:, :3].astype(np.float64)
    b = orc.test_eval(pkg.FN["evaluateBSDF"], np.concatenate([mat, L, V], axis=1), 4).view(np.float32)[:, :3].astype(np.float64)
    fa, fb = a / L[:, 2:3], b / V[:, 2:3]   # strip the cosine of the outgoing side
    assert np.abs(fa - fb).max() <= 2e-5 * max(1.0, np.abs(fa).max())


# ---------------------------------------------------------------------------------------
# image level: hand-built scenes with closed-form pixels
# ---------------------------------------------------------------------------------------
def _hand_scene(pkg, quads, material):
    """Quads in world space (corners, normal), one mesh each, all with one material."""
    return util.TriangleSoup(pkg, [[util.quad_mesh(c, n) for c, n in quads]], material=material)


def _lights(pkg, color, direction, dark_point_lights=0):
    l = pkg.LightsUbo()
    l.LightCount = dark_point_lights
    for k in range(3):
        l.Directional.Color[k] = color[k]
        l.Directional.Direction[k] = direction[k]
    for i in range(dark_point_lights):  # colour 0: selected with probability 1 / (N + 1) each, contribute nothing
        l.Lights[i].Position[0], l.Lights[i].Position[1], l.Lights[i].Position[2] = 1.0 + i, 5.0, 2.0
        l.Lights[i].AttenuationConstant = 1.0
    return l


def _fresnel(cos_i, eta):
    s2 = eta * eta * (1 - cos_i * cos_i)
    if s2 > 1:
        return 1.0
    ct = np.sqrt(max(1 - s2, 0.0))
    rs = (eta * ct - cos_i) / (eta * ct + cos_i)
    rp = (eta * cos_i - ct) / (eta * cos_i + ct)
    return (rs * rs + rp * rp) / 2


@pytest.mark.parametrize("dark_lights", [0, 3])
def test_direct_light_pixel_in_closed_form(pkg, orc, dark_lights):
    # a plane y = 0 facing +y, camera above it looking down at an angle, one directional light.  The quad is kept small on
    # purpose: offsetRayOriginShadowTerminator (ray.glsl:109-131) returns P + sum b_i (P - v_i), which is P only in exact
    # arithmetic -- on 100-unit triangles its rounding error (1e-5) puts 4 % of the shadow origins below the plane, and
    # those rays hit the plane itself past tmin = 1e-5.  Reference behaviour, reproduced; not what this test is about.
    S = 6.0
    plane = ([[-S, 0, -S], [-S, 0, S], [S, 0, S], [S, 0, -S]], [0, 1, 0])
    albedo = np.float64([0.8, 0.5, 0.3])
    hs = _hand_scene(pkg, [plane], util.mr_material(color=albedo, roughness=1.0))
    osc = orc.OracleScene(hs.desc)
    cam = pkg.Scene("default")
    pos, look = np.float32([0.0, 3.0, -4.0]), np.float32([0.0, -0.6, 0.8])
    cam.set_camera_pose(pos, look)
    E, ldir = np.float64([3.0, 2.5, 2.0]), np.float64([0.3, -1.0, 0.2])
    lights = _lights(pkg, E, ldir, dark_lights)
    W = H = 33
    spp = 1024 if dark_lights == 0 else 4096
    u = cam.uniform(W, H, bounces=1, sample_count=spp)
    img, st = osc.render(u, lights, W, H)
    assert st.retries == 0
    got = img[H // 2, W // 2, :3].astype(np.float64) / spp
    if dark_lights:
        # the 1 / (N + 1) selection pdf makes the estimate independent of N: same frame with the directional light alone
        ref, _ = osc.render(u, _lights(pkg, E, ldir, 0), W, H)
        c = slice(H // 2 - 5, H // 2 + 6)
        ratio = img[c, c, :3].astype(np.float64).sum() / ref[c, c, :3].astype(np.float64).sum()
        assert abs(ratio - 1) <= 0.01, ratio                          # 121 pixels x 4096 samples: sigma ~ 0.25 %
    # closed form at the central pixel: V = -look, L = -ldir, n = +y (the default normal texel tilts it by 0.4 %)
    V = -look.astype(np.float64) / np.linalg.norm(look)
    Lw = -ldir / np.linalg.norm(ldir)
    cv, cl = V[1], Lw[1]
    Hh = (V + Lw) / np.linalg.norm(V + Lw)
    F = _fresnel(abs(V @ Hh), 1 / 1.5)
    G = (2 * cv / (1 + cv)) * (2 * cl / (1 + cl))                # Smith, alpha = 1: Lambda = (1 / cos - 1) / 2
    expect = E * ((1 - F) * albedo * cl / PI + F * (1 / PI) * G / (4 * cv))
    # The shadow ray starts at payload.Position (raygen.rgen:81), the origin of the CONTINUATION ray: when the glossy lobe
    # reflects below the horizon (bsdf.Direction.z < 0 counts as "refracted", closestHit.rchit:131-142) that origin is
    # pushed under the surface and the plane shadows its own direct light.  Probability of that, by quadrature over the
    # visible normals (alpha = 1: D = 1 / pi, Dv = G1(V) max(V.H, 0) D / V.z), lobe chosen with probability F(V.H):
    n_t, n_p = 1000, 720
    ch = (np.arange(n_t) + 0.5) / n_t
    phh = (np.arange(n_p) + 0.5) / n_p * 2 * PI
    CH, PHH = np.meshgrid(ch, phh, indexing="ij")
    sh = np.sqrt(1 - CH * CH)
    Hx, Hy, Hz = sh * np.cos(PHH), sh * np.sin(PHH), CH              # local frame: z = normal
    Vl = np.float64([np.sqrt(1 - cv * cv), 0.0, cv])
    vh = Vl[0] * Hx + Vl[1] * Hy + Vl[2] * Hz
    dvis = (2 * cv / (1 + cv)) * np.maximum(vh, 0) / PI / cv
    s2 = (1 / 1.5) ** 2 * (1 - vh * vh)
    ct = np.sqrt(np.maximum(1 - s2, 0))
    Fh = (((ct / 1.5 - vh) / (ct / 1.5 + vh)) ** 2 + ((vh / 1.5 - ct) / (vh / 1.5 + ct)) ** 2) / 2
    below = (2 * vh * Hz - cv) < 0
    dwh = (1.0 / n_t) * (2 * PI / n_p)
    assert abs(dvis.sum() * dwh - 1) < 2e-3                            # the visible-normal density is normalised
    p_below = float((dvis * Fh * below).sum() * dwh)
    assert 0.01 < p_below < 0.08
    expect = expect * (1 - p_below)
    tol = 0.02 if dark_lights == 0 else 0.12                       # one pixel, 4096 Bernoulli(1/4) samples: sigma ~ 2.7 %
    assert np.abs(got / expect - 1).max() <= tol, (got, expect)


def test_beer_lambert_slab_in_closed_form(pkg, orc):
    # a glass slab 0 <= z <= T facing the camera (looking down +z from z = -5), nothing else: every path ends in the sky
    T, S = 0.5, 40.0
    front = ([[-S, -S, 0], [-S, S, 0], [S, S, 0], [S, -S, 0]], [0, 0, -1])   # outward normals, winding to match
    back = ([[-S, -S, T], [S, -S, T], [S, S, T], [-S, S, T]], [0, 0, 1])
    att_color, att_dist = np.float64([0.3, 0.6, 0.9]), 0.4
    glass = util.mr_material(color=(1, 1, 1), roughness=0.0, transmission=1.0, ior=1.5, att_color=att_color, att_dist=att_dist)
    hs = _hand_scene(pkg, [front, back], glass)
    osc = orc.OracleScene(hs.desc)
    cam = pkg.Scene("default")
    cam.set_camera_pose(np.float32([0.0, 0.0, -5.0]), np.float32([0.0, 0.0, 1.0]))
    lights = _lights(pkg, (0, 0, 0), (0, -1, 0))
    W = H = 65
    spp = 256
    u = cam.uniform(W, H, bounces=24, sample_count=spp)
    img, st = osc.render(u, lights, W, H)
    assert st.retries == 0 and np.isfinite(img).all()
    c = slice(H // 2 - 3, H // 2 + 4)
    got = img[c, c, :3].astype(np.float64).mean(axis=(0, 1)) / spp     # 49 pixels within 2.5 degrees of the normal
    sky = np.float64([0.08, 0.09, 0.1])
    F = 0.04                                                            # ((1 - 1.5) / (1 + 1.5))^2 at normal incidence, both ways
    a = att_color ** (T / att_dist)
    expect = sky * (F + (1 - F) ** 2 * a / (1 - F * a))               # k internal reflections: (1 - F)^2 a (F a)^k, every exit sees the sky
    assert np.abs(got / expect - 1).max() <= 0.03, (got, expect, got / sky)
    # without attenuation the slab is invisible against a constant sky (white furnace through two interfaces)
    clear = util.mr_material(color=(1, 1, 1), roughness=0.0, transmission=1.0, ior=1.5)
    hs2 = _hand_scene(pkg, [front, back], clear)
    img2, _ = orc.OracleScene(hs2.desc).render(u, lights, W, H)
    got2 = img2[c, c, :3].astype(np.float64).mean(axis=(0, 1)) / spp
    assert np.abs(got2 / sky - 1).max() <= 0.02, got2 / sky


def test_closest_hit_query_against_float64_geometry(pkg, orc):
    """The ray / triangle test and the closest-hit rule are the Vulkan driver's work in the reference, restated here by
    reading -- so an independent check: the oracle's brute-force query on a real scene against a float64 Moeller-Trumbore
    over the same world-space triangles, written from the textbook formula.  Hit / miss agrees except where the float64
    barycentrics sit within 1e-5 of an edge; the nearest triangle agrees except between hits closer than 1e-4 of t;
    t, u, v agree to float precision."""
    scene = pkg.Scene("chess_like", 0.05)
    d = scene.desc
    T = util.world_triangles(d)  # world-space triangles in the global order (instance, mesh, primitive)
    assert len(T) == scene.triangle_count and len(T) < 200000
    rng = np.random.default_rng(21)
    rays = util.random_rays(rng, 3000, -6.0, 6.0)
    got = orc.OracleScene(d, build_bvh=False).trace_closest(rays, brute_force=True)
    hits, agree, close = util.check_closest_against_float64(T, rays, got)
    assert hits > 500 and agree > 0.98 * hits, (hits, agree, close)
