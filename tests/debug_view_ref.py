"""CPU restatement of the debug view (Shaders/Debug/*, include/ptx.h ptx_render_debug), generic over a numpy dtype.

Everything the oracle already specifies comes from the oracle's entry points, in float32 whatever the dtype: the primary ray and
the offset directions (PTX_FN_PRIMARY_RAY), the hit (trace_closest), the shadow queries (trace_any), the texture footprint
(PTX_FN_DPN_DUV / DP_DXY / DERIVATIVES / COMPUTE_LOD), the texels (test_texture) and the material sample (PTX_FN_SAMPLE_MATERIAL),
the cube sky (test_miss).  The rest -- vertex interpolation and transform, the shadow-terminator point, the light model, the
hash -- is numpy in `dtype`: float32 restates the arithmetic of the kernel up to evaluation order, float64 is what both
approximate.  The difference between the two is what the tolerance of tests/test_debug_view.py is measured from.  Never calls
the HIP library."""
import ctypes as C

import numpy as np

import util

(MODE_COLOR, MODE_WORLD_POSITION, MODE_NORMAL, MODE_TEXTURE_COORDS, MODE_MIPS, MODE_GEOMETRY, MODE_PRIMITIVE, MODE_INSTANCE) = range(8)
HIT_DISABLE_COLOR_TEXTURE, HIT_DISABLE_NORMAL_TEXTURE, HIT_DISABLE_MIP_MAPS, HIT_DISABLE_SHADOWS = 1, 2, 4, 8
FN_PRIMARY_RAY, FN_DPN_DUV, FN_DP_DXY, FN_DERIVATIVES, FN_COMPUTE_LOD, FN_SAMPLE_MATERIAL = 16, 22, 23, 24, 27, 34
CLEAR_COLOR = (0.2, 0.2, 0.2)  # debugMiss.rmiss:36
DIRECTIONAL_LIGHT_DISTANCE = 100000.0  # sampling.glsl:3
PI = 3.14159265359  # common.glsl:3
MISS = 0xFFFFFFFF


# ---- debugClosestHit.rchit:143-162 ------------------------------------------------------------------------
def hash_u32(x):
    x = np.asarray(x, np.uint64) & 0xFFFFFFFF
    x = (x * 0x1ECA7D79) & 0xFFFFFFFF
    x ^= x >> 20
    x = ((x << 8) | (x >> 24)) & 0xFFFFFFFF
    x = ~x & 0xFFFFFFFF
    x ^= (x << 5) & 0xFFFFFFFF
    x = (x + 0x10AFE4E7) & 0xFFFFFFFF
    return x.astype(np.uint32)


def random_color(x):
    """getRandomColor in the project's arithmetic: byte * rcp(255), float32."""
    h = hash_u32(x)
    rcp255 = np.float32(1.0) / np.float32(255.0)
    return np.stack([((h >> s) & 0xFF).astype(np.float32) * rcp255 for s in (24, 16, 8)], axis=-1)


# ---- small vector helpers in the project's conventions ----------------------------------------------------
def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _div(a, b):
    """a / b := a * rcp(b)"""
    with np.errstate(all="ignore"):
        return a * (np.ones_like(b) / b)


def _normalize(a):
    """a * rsq(dot(a, a)), rsq correctly rounded"""
    with np.errstate(all="ignore"):
        d = _dot(a, a)
        r = (1.0 / np.sqrt(d.astype(np.float64))).astype(a.dtype)
        return a * r[..., None]


def _mix(x, y, a):
    return x * (1 - a) + y * a


# ---- debugClosestHit.rchit:71-141 ---------------------------------------------------------------------------
def light_contribution(light_dir, light_color, attenuation, V, N, color, roughness, metalness, dtype):
    c = lambda x: np.asarray(x).astype(dtype)  # noqa: E731
    light_dir, light_color, attenuation, V, N, color, roughness, metalness = map(c, (light_dir, light_color, attenuation, V, N, color, roughness, metalness))
    one, zero, pi = dtype(1), dtype(0), dtype(np.float32(PI))
    with np.errstate(all="ignore"):
        L = -_normalize(light_dir)
        H = _normalize(V + L)
        radiance = light_color * attenuation[..., None]
        F0 = _mix(dtype(np.float32(0.04)), color, metalness[..., None])
        a = roughness * roughness
        a2 = a * a
        NdotH = np.maximum(_dot(N, H), zero)
        denom = NdotH * NdotH * (a2 - one) + one
        denom = pi * denom * denom
        NDF = _div(a2, np.maximum(denom, dtype(np.float32(0.0001))))
        NdotV, NdotL = np.maximum(_dot(N, V), zero), np.maximum(_dot(N, L), zero)
        r = roughness + one
        k = _div(r * r, np.full_like(r, 8))
        G = _div(NdotL, NdotL * (one - k) + k) * _div(NdotV, NdotV * (one - k) + k)
        x = np.clip(one - np.maximum(_dot(H, V), zero), zero, one)
        x2 = x * x
        F = F0 + (one - F0) * (x2 * x2 * x)[..., None]
        numerator = F * (NDF * G)[..., None]
        denominator = (dtype(4) * NdotV) * NdotL
        specular = _div(numerator, np.maximum(denominator, dtype(np.float32(0.0001)))[..., None])
        kD = (one - F) * (one - metalness)[..., None]
        return ((_div(kD * color, pi) + specular) * radiance) * NdotL[..., None]


# ---- the scene as the reference reads it ------------------------------------------------------------------------
class RefScene:
    """The per-pair tables of a PtxSceneDesc and its oracle; with `instance_transforms` (n x 12) / `bones` (m x 12), of the
    scene posed that way (ptx_update_animation)."""

    def __init__(self, orc, desc, instance_transforms=None, bones=None):
        self.orc, self.desc = orc, desc
        self.osc = orc.OracleScene(desc, build_bvh=True, instance_transforms=instance_transforms, bones=bones)
        a = util.desc_arrays(desc)
        if instance_transforms is not None:
            a["instances"] = a["instances"].copy()
            a["instances"]["Transform"] = np.asarray(instance_transforms, np.float32).reshape(-1, 12)
        a["animated_indices"] = util._view(desc.animatedIndices, desc.animatedIndexCount, np.dtype("u4"))
        self.a = a
        self.first = util.pair_first(desc)
        rows = []
        for i, inst in enumerate(a["instances"]):
            m = a["models"][inst["ModelIndex"]]
            for k in range(m["MeshCount"]):
                rec = a["meshes"][m["MeshOffset"] + k]
                rows.append((i, k, int(rec["GeometryIndex"]), int(rec["MaterialId"]), int(rec["TransformIndex"])))
        self.pair = np.array(rows, np.int64).reshape(-1, 5)  # instance, geometry index inside the model, geometry, material id, transform
        # first vertex of every pair's copy in the skinned vertex block: one copy per instanced animated mesh, in pair order
        g = a["geometries"][self.pair[:, 2]]
        length = np.where(g["IsAnimated"] != 0, g["VertexLength"], 0).astype(np.int64)
        self.skinned_first = np.cumsum(length) - length
        f4 = np.dtype("f4")
        self.materials = [util._view(desc.metallicRoughnessMaterials, desc.metallicRoughnessMaterialCount * 24, f4).reshape(-1, 24),
                          util._view(desc.specularGlossinessMaterials, desc.specularGlossinessMaterialCount * 24, f4).reshape(-1, 24),
                          util._view(desc.phongMaterials, desc.phongMaterialCount * 24, f4).reshape(-1, 24)]

    def close(self):
        self.osc.close()

    def pair_matrix(self, dtype):
        """world = A_instance * A_mesh * x per pair: (n, 3, 4)"""
        out = np.zeros((len(self.pair), 3, 4), dtype)
        for p, (i, _, _, _, tr) in enumerate(self.pair):
            ai = np.vstack([self.a["instances"][i]["Transform"].astype(dtype).reshape(3, 4), np.array([0, 0, 0, 1], dtype)])
            am = np.vstack([self.a["transforms"][tr].astype(dtype).reshape(3, 4), np.array([0, 0, 0, 1], dtype)])
            out[p] = (ai @ am)[:3]
        return out

    def material_record(self, material_id):
        """(type, 24-dword record, the five texture indices in slot order) of each material id"""
        mtype, mindex = material_id & 0xFF, material_id >> 8
        rec = np.zeros((len(material_id), 24), np.float32)
        idx = np.zeros((len(material_id), 5), np.uint32)
        for t in range(3):
            sel = mtype == t
            if sel.any():
                rec[sel] = self.materials[t][mindex[sel]]
                first = 19 if t == 0 else 18  # PtxMetallicRoughnessMaterial / the other two (include/ptx.h)
                idx[sel] = rec[sel].view(np.uint32)[:, first:first + 5]
        return mtype.astype(np.uint32), rec, idx

    def texels(self, idx, uv, dv, implicit_lod=False):
        """textureGrad(textures[idx], uv, dv.xy, dv.zw) (or texture() at the base level): scene textures through the oracle's sampler,
        the fixed 1x1 slots and the placeholder as constants (ShaderRendererTypes.incl:49-56)"""
        n = len(idx)
        inp = np.zeros((n, 7), np.float32)
        inp.view(np.uint32)[:, 0] = idx
        inp[:, 1:3] = uv
        inp[:, 3:7] = dv
        out = self.osc.test_texture(inp, implicit_lod=implicit_lod).view(np.float32).copy()
        scene = (idx >= 9) & (idx - 9 < self.desc.textureCount)
        fixed = np.ones((n, 4), np.float32)
        fixed[idx == 1, 0:2] = np.float32(128.0) / np.float32(255.0)
        fixed[(idx == 4) | (idx == 6) | (idx == 7)] = 0.0
        out[~scene] = fixed[~scene]
        return out


def primary_rays(orc, uniform, W, H):
    """debugRaygen.rgen:25 for every pixel, row-major: origin, direction, rx direction, ry direction (float32)"""
    y, x = np.divmod(np.arange(W * H, dtype=np.uint32), np.uint32(W))
    inp = np.zeros((W * H, 38), np.float32)
    iu = inp.view(np.uint32)
    iu[:, 0], iu[:, 1], iu[:, 2], iu[:, 3] = x, y, W, H
    inp[:, 4:6] = 0.5
    inp[:, 6:22] = np.frombuffer(uniform.ViewInverse, np.float32)
    inp[:, 22:38] = np.frombuffer(uniform.ProjInverse, np.float32)
    out = orc.test_eval(FN_PRIMARY_RAY, inp, 18).view(np.float32)
    return out[:, 0:3].copy(), out[:, 3:6].copy(), out[:, 9:12].copy(), out[:, 15:18].copy()


def _decals(rs, o, d, hit_t, hit_sel):
    """debugAnyhit.rahit:37-64 by brute force: per hit pixel the colour (rgba) of the nearest candidate with alpha < 0.5 in front
    of the hit, among the triangles of non-opaque geometry; (has decal, rgba)."""
    geo = rs.a["geometries"]
    nonopaque = np.flatnonzero(geo["IsOpaque"][rs.pair[:, 2]] == 0)
    n = len(hit_t)
    has, rgba = np.zeros(n, bool), np.zeros((n, 4), np.float32)
    if not len(nonopaque):
        return has, rgba
    assert not geo["IsAnimated"][rs.pair[nonopaque, 2]].any(), "decals over animated geometry are not restated"
    T = util.world_triangles(rs.desc, rs.a["instances"]["Transform"])
    ids = np.concatenate([np.arange(rs.first[p], rs.first[p + 1]) for p in nonopaque])
    pair_of = np.concatenate([np.full(rs.first[p + 1] - rs.first[p], p) for p in nonopaque])
    Tn = T[ids]
    cand = []  # (pixel, triangle position in ids, t, u, v)
    for k in np.flatnonzero(hit_sel):
        ray = np.concatenate([o[k], [1e-5], d[k], [hit_t[k]]])
        inside, t, u, v, _ = util.moller_trumbore_f64(Tn, ray)
        for j in np.flatnonzero(inside):
            cand.append((k, j, t[j], u[j], v[j]))
    if not cand:
        return has, rgba
    c = np.array(cand)
    pix, j = c[:, 0].astype(np.int64), c[:, 1].astype(np.int64)
    p = pair_of[j]
    prim = ids[j] - rs.first[p]
    g = geo[rs.pair[p, 2]]
    vi = rs.a["indices"][(g["IndexOffset"].astype(np.int64) + 3 * prim)[:, None] + np.arange(3)] + g["VertexOffset"].astype(np.int64)[:, None]
    uv3 = rs.a["vertices"][vi][:, :, 3:5]
    u, v = c[:, 3].astype(np.float32), c[:, 4].astype(np.float32)
    b = np.stack([np.float32(1) - u - v, u, v], axis=1)
    uv = (uv3[:, 0] * b[:, 0:1] + uv3[:, 1] * b[:, 1:2]) + uv3[:, 2] * b[:, 2:3]
    mtype, rec, idx = rs.material_record(rs.pair[p, 3])
    color = rs.texels(idx[:, 1], uv, np.zeros((len(uv), 4), np.float32), implicit_lod=True) * rec[:, 4:8]
    ignored = color[:, 3] < 0.5
    order = np.lexsort((ids[j], c[:, 2]))
    for q in order[::-1]:  # the nearest is written last
        if ignored[q]:
            has[pix[q]] = True
            rgba[pix[q]] = color[q]
    return has, rgba


def render(rs, uniform, lights, W, H, mode, hit_flags=0, dtype=np.float32, posed=None):
    """One debug frame of the whole image.  `posed`: the skinned vertex block in `dtype` (tests/skin_ref.py posed_vertices), what
    hits on animated geometry read their vertices from.  Returns a dict: image (H, W, 4) in `dtype`; hit (H, W) bool; occluded
    (1 + LightCount, H, W) bool, the reference's own occlusion masks (Color mode with shadows); segments / shadow_rays, the counts
    ptx_get_stats reports; t, tri of the primary hits."""
    orc, osc, desc = rs.orc, rs.osc, rs.desc
    n = W * H
    o, d, rxd, ryd = primary_rays(orc, uniform, W, H)
    rays = np.zeros((n, 8), np.float32)
    rays[:, 0:3], rays[:, 3], rays[:, 4:7], rays[:, 7] = o, 1e-5, d, 1e4
    hits = osc.trace_closest(rays)
    hit = hits["tri"] != MISS
    img = np.zeros((n, 4), dtype)
    img[:, 3] = 1
    nl = int(lights.LightCount)
    res = {"hit": hit.reshape(H, W), "occluded": np.zeros((1 + nl, H, W), bool), "segments": n, "shadow_rays": 0,
           "t": hits["t"].reshape(H, W), "tri": hits["tri"].reshape(H, W), "direction": d.reshape(H, W, 3), "origin": o.reshape(H, W, 3)}
    # debugMiss.rmiss:18-37
    if desc.skyboxKind == 2:
        img[~hit, 0:3] = osc.test_miss(d[~hit].view(np.uint32)).view(np.float32)[:, 0:3]
    elif desc.skyboxKind == 1:
        # the 2-D sky without hdrToLdr: miss.rmiss's value m = c / (1 + max c) inverted, c = m (1 + M), M = max m / (1 - max m)
        m = osc.test_miss(d[~hit].view(np.uint32)).view(np.float32)[:, 0:3].astype(np.float64)
        mx = m.max(axis=1, keepdims=True)
        with np.errstate(all="ignore"):
            img[~hit, 0:3] = (m * (1 + mx / (1 - mx))).astype(dtype)
    else:
        img[~hit, 0:3] = np.array(CLEAR_COLOR, np.float32).astype(dtype)
    h = np.flatnonzero(hit)
    if not len(h):
        res["image"] = img.reshape(H, W, 4)
        return res
    tri = hits["tri"][h].astype(np.int64)
    p = np.searchsorted(rs.first, tri, side="right") - 1
    prim = tri - rs.first[p]
    if mode >= MODE_GEOMETRY:  # debugClosestHit.rchit:256-264
        ident = rs.pair[p, 1] if mode == MODE_GEOMETRY else prim if mode == MODE_PRIMITIVE else rs.pair[p, 0]
        img[h, 0:3] = random_color(ident).astype(dtype)
        res["ids"] = np.full(n, -1, np.int64)
        res["ids"][h] = ident
        res["ids"] = res["ids"].reshape(H, W)
        res["image"] = img.reshape(H, W, 4)
        return res

    # :166-184 vertex fetch, interpolation, transform
    u, v = hits["u"][h].astype(dtype), hits["v"][h].astype(dtype)
    b = np.stack([dtype(1) - u - v, u, v], axis=1)
    g = rs.a["geometries"][rs.pair[p, 2]]
    anim = g["IsAnimated"] != 0
    corner = (g["IndexOffset"].astype(np.int64) + 3 * prim)[:, None] + np.arange(3)
    vtx = np.zeros((len(h), 3, 14), dtype)  # position, uv, normal, tangent, bitangent
    vtx[~anim] = rs.a["vertices"][rs.a["indices"][corner[~anim]] + g["VertexOffset"].astype(np.int64)[~anim, None]].astype(dtype)
    if anim.any():
        assert posed is not None and posed.dtype == np.dtype(dtype), "hits on animated geometry need the posed vertex block"
        vtx[anim] = posed[rs.a["animated_indices"][corner[anim]] + rs.skinned_first[p[anim], None]]
    M = rs.pair_matrix(dtype)[p]
    A, tr = M[:, :, 0:3], M[:, :, 3]
    Ainv_t = np.linalg.inv(A.astype(np.float64)).astype(dtype).transpose(0, 2, 1)  # the normal transform: inverse transpose

    def interp(x):
        return (x[:, 0] * b[:, 0:1] + x[:, 1] * b[:, 1:2]) + x[:, 2] * b[:, 2:3]

    def xf_point(x):
        return np.einsum("nij,nj->ni", A, x) + tr

    def xf_vector(x):
        return _normalize(np.einsum("nij,nj->ni", A, x))

    def xf_normal(x):
        return _normalize(np.einsum("nij,nj->ni", Ainv_t, x))

    P, uv = xf_point(interp(vtx[:, :, 0:3])), interp(vtx[:, :, 3:5])
    Nv, Tv, Bv = xf_normal(interp(vtx[:, :, 5:8])), xf_vector(interp(vtx[:, :, 8:11])), xf_vector(interp(vtx[:, :, 11:14]))
    P3 = np.stack([xf_point(vtx[:, k, 0:3]) for k in range(3)], axis=1)
    N3 = np.stack([xf_normal(vtx[:, k, 5:8]) for k in range(3)], axis=1)
    res["position"] = np.zeros((n, 3), dtype)
    res["position"][h] = P
    res["position"] = res["position"].reshape(H, W, 3)
    if mode == MODE_WORLD_POSITION:
        img[h, 0:3] = P
    elif mode == MODE_TEXTURE_COORDS:
        img[h, 0:2] = uv
    if mode in (MODE_WORLD_POSITION, MODE_TEXTURE_COORDS):
        res["image"] = img.reshape(H, W, 4)
        return res

    # :186-191 the texture footprint, through the oracle's functions
    f32 = lambda x: np.ascontiguousarray(x, np.float32)  # noqa: E731
    m = len(h)
    inp = np.zeros((m, 30), np.float32)
    for k in range(3):
        inp[:, 8 * k:8 * k + 3], inp[:, 8 * k + 3:8 * k + 6], inp[:, 8 * k + 6:8 * k + 8] = f32(P3[:, k]), f32(N3[:, k]), vtx[:, k, 3:5]
    inp[:, 24:27], inp[:, 27:30] = f32(Tv), f32(Bv)
    dpn = orc.test_eval(FN_DPN_DUV, inp, 12).view(np.float32)
    inp = np.zeros((m, 24), np.float32)
    inp[:, 0:3], inp[:, 3:6], inp[:, 6:9] = f32(P), o[h], f32(_normalize(d[h]))
    inp[:, 9:12], inp[:, 12:15], inp[:, 15:18], inp[:, 18:21], inp[:, 21:24] = o[h], rxd[h], o[h], ryd[h], f32(Nv)
    dpxy = orc.test_eval(FN_DP_DXY, inp, 6).view(np.float32)
    if hit_flags & HIT_DISABLE_MIP_MAPS:
        deriv = np.zeros((m, 4), np.float32)
    else:
        deriv = orc.test_eval(FN_DERIVATIVES, np.ascontiguousarray(np.concatenate([dpxy, dpn[:, 0:6]], axis=1)), 4).view(np.float32).copy()
    if mode == MODE_MIPS:  # :254
        lod = orc.test_eval(FN_COMPUTE_LOD, deriv, 1).view(np.float32)[:, 0].astype(dtype)
        img[h, 0:3] = (dtype(np.float32(0.1)) * lod + dtype(1))[:, None]
        res["image"] = img.reshape(H, W, 4)
        return res

    # :195 the material
    mtype, rec, idx = rs.material_record(rs.pair[p, 3])
    if hit_flags & HIT_DISABLE_COLOR_TEXTURE:
        idx[:, 1] = 0
    if hit_flags & HIT_DISABLE_NORMAL_TEXTURE:
        idx[:, 2] = 1
    inp = np.zeros((m, 47), np.float32)
    iu = inp.view(np.uint32)
    iu[:, 0], iu[:, 1], iu[:, 2] = mtype, 0, 1 if desc.dxNormalTextures else 0
    inp[:, 3:27] = rec
    for k in range(5):
        inp[:, 27 + 4 * k:31 + 4 * k] = rs.texels(idx[:, k], f32(uv), deriv)
    ms = orc.test_eval(FN_SAMPLE_MATERIAL, inp, 17).view(np.float32)
    emissive, color, nmap = ms[:, 0:3].astype(dtype), ms[:, 3:6].astype(dtype), ms[:, 6:9].astype(dtype)
    roughness, metalness = ms[:, 9].astype(dtype), ms[:, 10].astype(dtype)
    # :197-198 the decal
    has, rgba = _decals(rs, o, d, hits["t"], hit)
    has, rgba = has[h], rgba[h].astype(dtype)
    color = np.where(has[:, None], _mix(color, rgba[:, 0:3], rgba[:, 3:4]), color)
    # :200-202
    V = -_normalize(d[h].astype(dtype))
    N = _normalize(Nv + ((Tv * nmap[:, 0:1] + Bv * nmap[:, 1:2]) + Nv * nmap[:, 2:3]))
    if mode == MODE_NORMAL:
        img[h, 0:3] = N
        res["image"] = img.reshape(H, W, 4)
        return res

    # :204-237
    total = color * dtype(np.float32(0.1)) + emissive
    tu, tv, tw = P - P3[:, 0], P - P3[:, 1], P - P3[:, 2]
    tu = tu - N3[:, 0] * np.minimum(dtype(0), _dot(tu, N3[:, 0]))[:, None]
    tv = tv - N3[:, 1] * np.minimum(dtype(0), _dot(tv, N3[:, 1]))[:, None]
    tw = tw - N3[:, 2] * np.minimum(dtype(0), _dot(tw, N3[:, 2]))[:, None]
    Pp = ((P + tu * b[:, 0:1]) + tv * b[:, 1:2]) + tw * b[:, 2:3]
    shadows = not (hit_flags & HIT_DISABLE_SHADOWS)

    def occluded(light_dir, dist):
        r = np.zeros((m, 8), np.float32)
        r[:, 0:3], r[:, 3], r[:, 4:7], r[:, 7] = f32(Pp), 1e-5, f32(-_normalize(light_dir)), f32(dist)
        return osc.trace_any(r) != 0

    occ = np.zeros((1 + nl, m), bool)
    ddir = np.broadcast_to(np.array(lights.Directional.Direction, np.float32).astype(dtype), (m, 3))
    if shadows:
        occ[0] = occluded(ddir, np.full(m, DIRECTIONAL_LIGHT_DISTANCE, np.float32))
    lc = light_contribution(ddir, np.broadcast_to(np.array(lights.Directional.Color, np.float32), (m, 3)), np.ones(m, np.float32), V, N, color,
                            roughness, metalness, dtype)
    total = total + np.where(occ[0][:, None], dtype(0), lc)
    for k in range(nl):
        L = lights.Lights[k]
        ldir = Pp - np.array(L.Position, np.float32).astype(dtype)
        dist = np.sqrt(_dot(ldir, ldir))
        att = _div(np.ones_like(dist), (dtype(np.float32(L.AttenuationConstant)) + dist * dtype(np.float32(L.AttenuationLinear))) +
                   (dist * dist) * dtype(np.float32(L.AttenuationQuadratic)))
        if shadows:
            occ[1 + k] = occluded(ldir, dist)
        lc = light_contribution(ldir, np.broadcast_to(np.array(L.Color, np.float32), (m, 3)), att, V, N, color, roughness, metalness, dtype)
        total = total + np.where(occ[1 + k][:, None], dtype(0), lc)
    img[h, 0:3] = total
    res["image"] = img.reshape(H, W, 4)
    full = np.zeros((1 + nl, n), bool)
    full[:, h] = occ
    res["occluded"] = full.reshape(1 + nl, H, W)
    res["shadow_rays"] = (1 + nl) * m if shadows else 0
    return res


def shadow_edge_mask(res):
    """Pixels within one pixel (8-neighbourhood) of a place where the reference's occlusion mask of some light differs from a
    4-neighbour's -- where a last-bit difference in the shadow ray's origin may flip a light."""
    occ, hit = res["occluded"], res["hit"]
    H, W = hit.shape
    edge = np.zeros((H, W), bool)
    for m in occ:
        dx = m[:, 1:] != m[:, :-1]
        dy = m[1:, :] != m[:-1, :]
        edge[:, 1:] |= dx
        edge[:, :-1] |= dx
        edge[1:, :] |= dy
        edge[:-1, :] |= dy
    grown = edge.copy()
    for sy in (-1, 0, 1):
        for sx in (-1, 0, 1):
            src = edge[max(0, -sy):H - max(0, sy), max(0, -sx):W - max(0, sx)]
            grown[max(0, sy):H - max(0, -sy), max(0, sx):W - max(0, -sx)] |= src
    return grown


def tolerance(ref32, ref64, measured_max=None):
    """Per-pixel bound: 8 x max |ref(float32) - ref(float64)| over the image (or the recorded maximum), floor 2^-20 max(1, |value|)."""
    a, b = ref32["image"].astype(np.float64), ref64["image"]
    with np.errstate(all="ignore"):
        diff = np.abs(a - b)
    mx = float(np.nanmax(np.where(np.isfinite(diff), diff, 0.0))) if measured_max is None else measured_max
    return np.maximum(8.0 * mx, 2.0 ** -20 * np.maximum(1.0, np.abs(b)))
