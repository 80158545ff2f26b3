"""CPU restatement of the specular-chain guide pass (include/ptx.h ptx_render_guides_specular, docs/NEXT_ROWS.md section 18), generic
over a numpy dtype and written from the header's text.

Built the way tests/debug_view_ref.py is built, whose scene tables and helpers it imports: what the oracle already specifies comes
from the oracle's entry points, in float32 whatever the dtype -- the primary ray and its offset directions, which triangle a ray hits
(trace_closest, any-hit stage included; the float32 run also takes its t, u, v, the float64 run intersects the named triangle
again), the texture footprint (PTX_FN_DPN_DUV / DP_DXY / DERIVATIVES), the texels, the material sample (PTX_FN_SAMPLE_MATERIAL, with the inside flag), the propagated offset rays (PTX_FN_REFLECTED / REFRACTED_DIFFERENTIALS) and the
self-intersection offset (PTX_FN_OFFSET_RAY_ORIGIN).  The rest -- vertex interpolation and transform, the two normals, the class
decision, reflect / refract, the shadow-terminator origin, T, M and the tint -- is numpy in `dtype`.  float32 restates the kernel up
to evaluation order, float64 is what both approximate; the gap between the two is what the tolerance of
tests/test_specular_guides.py is measured from.  Never calls the HIP library.

chain() shades an arbitrary ray batch; render() feeds it the primary rays of a frame.  Beside the four images both return, per ray
and bounce, the triangle that was hit, and per ray the class and the chain length, so that a test can tell "decided differently"
from "computed differently"."""
import numpy as np

import debug_view_ref as DV
from debug_view_ref import _dot, _mix, _normalize

FN_OFFSET_RAY_ORIGIN, FN_REFLECTED_DIFFERENTIALS, FN_REFRACTED_DIFFERENTIALS = 15, 25, 26
SPECULAR_SURFACE = 0
CLASS_SURFACE, CLASS_CAPPED, CLASS_ESCAPED = range(3)
NO_TRI = -1  # tri[ray, bounce] where no ray was traced; a traced ray that missed holds MISS
MISS = int(DV.MISS)
T_MIN, T_MAX = 1e-5, 1e4


def _f32(x):
    return np.ascontiguousarray(x, np.float32)


def _shadow_terminator(P, P3, N3, b, refracted, dtype):
    """offsetRayOriginShadowTerminator (tracing.glsl / pt_device.hpp), the corner normals negated for a refracted ray"""
    N3 = np.where(refracted[:, None, None], -N3, N3)
    out = P
    for k in range(3):
        t = P - P3[:, k]
        t = t - N3[:, k] * np.minimum(dtype(0), _dot(t, N3[:, k]))[:, None]
        out = out + t * b[:, k:k + 1]
    return out


def _shade(rs, o, d, diff, hits, first, dtype, posed, oracle_hits=False):
    """Steps 1 and 2 of the header text for m rays that hit.  o, d: (m, 3) in dtype; diff: (m, 12) float32, the offset rays (origin
    and direction of x, then of y); hits: the oracle's records; first: the hit is a primary ray's (the plain pass's expressions:
    nothing flipped in the footprint)."""
    orc = rs.orc
    m = len(hits)
    tri = hits["tri"].astype(np.int64)
    p = np.searchsorted(rs.first, tri, side="right") - 1
    prim = tri - rs.first[p]
    g = rs.a["geometries"][rs.pair[p, 2]]
    anim = g["IsAnimated"] != 0
    corner = (g["IndexOffset"].astype(np.int64) + 3 * prim)[:, None] + np.arange(3)
    vtx = np.zeros((m, 3, 14), dtype)
    vtx[~anim] = rs.a["vertices"][rs.a["indices"][corner[~anim]] + g["VertexOffset"].astype(np.int64)[~anim, None]].astype(dtype)
    if anim.any():
        assert posed is not None and posed.dtype == np.dtype(dtype), "hits on animated geometry need the posed vertex block"
        vtx[anim] = posed[rs.a["animated_indices"][corner[anim]] + rs.skinned_first[p[anim], None]]
    M = rs.pair_matrix(dtype)[p]
    A, tr = M[:, :, 0:3], M[:, :, 3]
    Ainv_t = np.linalg.inv(A.astype(np.float64)).astype(dtype).transpose(0, 2, 1)

    def xf_point(x):
        return np.einsum("nij,nj->ni", A, x) + tr

    def xf_vector(x):
        return _normalize(np.einsum("nij,nj->ni", A, x))

    def xf_normal(x):
        return _normalize(np.einsum("nij,nj->ni", Ainv_t, x))

    P3 = np.stack([xf_point(vtx[:, k, 0:3]) for k in range(3)], axis=1)
    N3 = np.stack([xf_normal(vtx[:, k, 5:8]) for k in range(3)], axis=1)
    # The hit record.  float32: the oracle's t, u, v, which are what the kernel's traversal returns.  Above float32 the oracle only
    # says WHICH triangle: the ray is intersected with it again in `dtype`, so that the float64 run is float64 throughout and the gap
    # between the two runs holds the float32 error of the hit record as well (oracle_hits: the oracle's record all the same, which is
    # how tests/denoise_ref.py cpu_guides builds its float64 albedo).
    if np.dtype(dtype) == np.float32 or oracle_hits:
        t, u, v = hits["t"].astype(dtype), hits["u"].astype(dtype), hits["v"].astype(dtype)
    else:
        e1, e2 = P3[:, 1] - P3[:, 0], P3[:, 2] - P3[:, 0]
        nn = np.cross(e1, e2)
        t = _dot(P3[:, 0] - o, nn) / _dot(d, nn)
        w = (o + d * t[:, None]) - P3[:, 0]
        u, v = _dot(np.cross(w, e2), nn) / _dot(nn, nn), _dot(np.cross(e1, w), nn) / _dot(nn, nn)
    b = np.stack([dtype(1) - u - v, u, v], axis=1)

    def interp(x):
        return (x[:, 0] * b[:, 0:1] + x[:, 1] * b[:, 1:2]) + x[:, 2] * b[:, 2:3]

    P, uv = xf_point(interp(vtx[:, :, 0:3])), interp(vtx[:, :, 3:5])
    Nv, Tv, Bv = xf_normal(interp(vtx[:, :, 5:8])), xf_vector(interp(vtx[:, :, 8:11])), xf_vector(interp(vtx[:, :, 11:14]))
    gn = _normalize(np.cross(P3[:, 1] - P3[:, 0], P3[:, 2] - P3[:, 0]))
    inside = _dot(gn, d) > 0
    gn = np.where(inside[:, None], -gn, gn)  # facing the ray
    flip = inside & ~first  # the footprint's frame: closestHit flips it, the plain pass does not
    sgn = np.where(flip, dtype(-1), dtype(1))[:, None]
    # the texture footprint, through the oracle's functions
    inp = np.zeros((m, 30), np.float32)
    for k in range(3):
        inp[:, 8 * k:8 * k + 3], inp[:, 8 * k + 3:8 * k + 6], inp[:, 8 * k + 6:8 * k + 8] = _f32(P3[:, k]), _f32(N3[:, k]), vtx[:, k, 3:5]
    inp[:, 24:27], inp[:, 27:30] = _f32(Tv * sgn), _f32(Bv * sgn)
    dpn = orc.test_eval(DV.FN_DPN_DUV, inp, 12).view(np.float32)
    inp = np.zeros((m, 24), np.float32)
    inp[:, 0:3], inp[:, 9:21], inp[:, 21:24] = _f32(P), diff, _f32(Nv * sgn)
    dpxy = orc.test_eval(DV.FN_DP_DXY, inp, 6).view(np.float32)
    deriv = orc.test_eval(DV.FN_DERIVATIVES, np.ascontiguousarray(np.concatenate([dpxy, dpn[:, 0:6]], axis=1)), 4).view(np.float32).copy()
    # the material, sampled with the inside flag
    mtype, rec, idx = rs.material_record(rs.pair[p, 3])
    inp = np.zeros((m, 47), np.float32)
    iu = inp.view(np.uint32)
    iu[:, 0], iu[:, 1], iu[:, 2] = mtype, inside.astype(np.uint32), 1 if rs.desc.dxNormalTextures else 0
    inp[:, 3:27] = rec
    for k in range(5):
        inp[:, 27 + 4 * k:31 + 4 * k] = rs.texels(idx[:, k], _f32(uv), deriv)
    ms = orc.test_eval(DV.FN_SAMPLE_MATERIAL, inp, 17).view(np.float32)
    color, nmap = ms[:, 3:6].astype(dtype), ms[:, 6:9].astype(dtype)
    # the decal mix
    has, rgba = DV._decals(rs, _f32(o), _f32(d), hits["t"], np.ones(m, bool))
    rgba = rgba.astype(dtype)
    color = np.where(has[:, None], _mix(color, rgba[:, 0:3], rgba[:, 3:4]), color)
    n_guide = _normalize(Nv + ((Tv * nmap[:, 0:1] + Bv * nmap[:, 1:2]) + Nv * nmap[:, 2:3]))
    n_cont = np.where(inside[:, None], -n_guide, n_guide)  # the flipped frame negates every term
    return dict(P=P, P3=P3, N3=N3, b=b, gn=gn, inside=inside, Nv_cont=np.where(inside[:, None], -Nv, Nv), deriv=deriv, dndu=dpn[:, 6:9], dndv=dpn[:, 9:12],
                color=color, roughness=ms[:, 9].copy(), metalness=ms[:, 10].copy(), transmission=ms[:, 11].copy(), eta=ms[:, 12].astype(dtype),
                n_guide=n_guide, n_cont=n_cont, t=t)


def chain(rs, o, d, rxd, ryd, max_bounces, roughness_max, dtype=np.float32, posed=None, oracle_hits=False):
    """The pass for a batch of n rays (float32 origin, direction and the two offset directions, which start at the origin).  Returns
    a dict of (n, ...) arrays: normal, position, albedo, surface (n, 4) in `dtype`; hit (the primary ray hit); bounces; cls; tri
    (n, max_bounces + 1): the triangle per traced segment, MISS for a traced miss, NO_TRI where nothing was traced; rays
    (max_bounces + 1, n, 8) float32: what was traced per segment (zeros where nothing was), origins and directions
    (max_bounces + 1, n, 3) the same rays in `dtype`; segments: rays traced in all."""
    osc, orc = rs.osc, rs.orc
    n = len(o)
    roughness_max = np.float32(roughness_max)
    o0, d0 = o.astype(dtype), d.astype(dtype)
    co, cd = o0.copy(), d0.copy()
    diff = np.concatenate([_f32(o), _f32(rxd), _f32(o), _f32(ryd)], axis=1)
    T = np.zeros(n, dtype)
    M = np.broadcast_to(np.eye(3, dtype=dtype), (n, 3, 3)).copy()
    tint = np.ones((n, 3), dtype)
    out = {k: np.zeros((n, 4), dtype) for k in ("normal", "position", "albedo", "surface")}
    out["albedo"][:] = 1
    bounces, cls = np.zeros(n, np.int64), np.zeros(n, np.int64)
    tris = np.full((n, max_bounces + 1), NO_TRI, np.int64)
    rays_log = np.zeros((max_bounces + 1, n, 8), np.float32)
    origins, dirs = np.zeros((max_bounces + 1, n, 3), dtype), np.zeros((max_bounces + 1, n, 3), dtype)
    hit0 = np.zeros(n, bool)
    act = np.arange(n)
    segments = 0
    for bounce in range(max_bounces + 1):
        if not len(act):
            break
        rays = np.zeros((len(act), 8), np.float32)
        rays[:, 0:3], rays[:, 3], rays[:, 4:7], rays[:, 7] = _f32(co[act]), T_MIN, _f32(cd[act]), T_MAX
        rays_log[bounce, act] = rays
        origins[bounce, act], dirs[bounce, act] = co[act], cd[act]
        segments += len(act)
        hits = osc.trace_closest(rays)
        tris[act, bounce] = hits["tri"]
        got = hits["tri"] != DV.MISS
        gone = act[~got]
        if bounce:  # escaped: the guides stay a miss's, the surface word says so
            cls[gone] = CLASS_ESCAPED
            out["surface"][gone, 3] = (bounces[gone] + 16 * CLASS_ESCAPED).astype(dtype)
        act, hits = act[got], hits[got]
        if not len(act):
            break
        if bounce == 0:
            hit0[act] = True
        with np.errstate(all="ignore"):
            s = _shade(rs, co[act], cd[act], diff[act], hits, np.full(len(act), bounce == 0), dtype, posed, oracle_hits)
            if bounce == 0:
                out["surface"][act, 0:3] = s["P"]
            mirror = s["metalness"] >= np.float32(0.5)
            followed = (s["roughness"] <= roughness_max) & (mirror | (s["transmission"] >= np.float32(0.5)))
            stop = ~followed | (bounce == max_bounces)
            e = act[stop]
            if bounce == 0:  # the plain pass's values
                out["normal"][e, 0:3], out["position"][e, 0:3], out["position"][e, 3] = s["n_guide"][stop], s["P"][stop], s["t"][stop]
                out["albedo"][e, 0:3] = s["color"][stop]
            else:
                Te = T[e] + s["t"][stop]
                out["normal"][e, 0:3] = np.einsum("nij,nj->ni", M[e], s["n_guide"][stop])
                out["position"][e, 0:3], out["position"][e, 3] = o0[e] + _normalize(d0[e]) * Te[:, None], Te
                out["albedo"][e, 0:3] = tint[e] * s["color"][stop]
            out["normal"][e, 3] = 1
            out["albedo"][e, 3] = 1
            cls[e] = np.where(followed[stop], CLASS_CAPPED, CLASS_SURFACE)
            out["surface"][e, 3] = (bounces[e] + 16 * cls[e]).astype(dtype)
            # step 4 for the rest
            go = ~stop
            a = act[go]
            if not len(a):
                break
            k = {key: val[go] for key, val in s.items()}
            din, nc, eta = cd[a], k["n_cont"], k["eta"]
            glass = ~mirror[go]
            dn = _dot(nc, din)
            kk = dtype(1) - eta * eta * (dtype(1) - dn * dn)
            refr = din * eta[:, None] - nc * (eta * dn + np.sqrt(np.maximum(kk, 0)))[:, None]
            refracted = glass & ~(kk < 0) & (refr != 0).any(axis=1)
            refl = din - nc * (dtype(2) * dn)[:, None]
            dout = _normalize(np.where(refracted[:, None], refr, refl))
            origin_st = _shadow_terminator(k["P"], k["P3"], k["N3"], k["b"], refracted, dtype)
            inp = np.concatenate([_f32(k["P"]), _f32(-k["gn"])], axis=1)
            origin_si = orc.test_eval(FN_OFFSET_RAY_ORIGIN, inp, 3).view(np.float32).astype(dtype)
            origin = np.where(refracted[:, None], origin_si, origin_st)
            tinted = refracted | ~glass  # total internal reflection leaves the tint alone
            tint[a] = np.where(tinted[:, None], tint[a] * k["color"], tint[a])
            Mn = np.einsum("nij,nj->ni", M[a], nc)
            M[a] = np.where(refracted[:, None, None], M[a], M[a] - (dtype(2) * Mn)[:, :, None] * nc[:, None, :])
            # the offset rays, as closestHit propagates them
            inp = np.zeros((len(a), 35), np.float32)
            inp[:, 0:4], inp[:, 4:7], inp[:, 7:10], inp[:, 10:13], inp[:, 13:16] = k["deriv"], _f32(k["Nv_cont"]), _f32(origin_st), _f32(-din), _f32(dout)
            inp[:, 16:19], inp[:, 19:22], inp[:, 22:34], inp[:, 34] = k["dndu"], k["dndv"], diff[a], _f32(eta)
            new = np.zeros((len(a), 12), np.float32)
            if (~refracted).any():
                new[~refracted] = orc.test_eval(FN_REFLECTED_DIFFERENTIALS, np.ascontiguousarray(inp[~refracted, 0:34]), 12).view(np.float32)
            if refracted.any():
                new[refracted] = orc.test_eval(FN_REFRACTED_DIFFERENTIALS, np.ascontiguousarray(inp[refracted]), 12).view(np.float32)
            diff[a] = new
            co[a], cd[a] = origin, dout
            T[a] = T[a] + k["t"]
            bounces[a] += 1
            act = a
    out.update(hit=hit0, bounces=bounces, cls=cls, tri=tris, rays=rays_log, origins=origins, directions=dirs, segments=segments)
    return out


def render(rs, uniform, W, H, max_bounces, roughness_max, dtype=np.float32, posed=None, oracle_hits=False):
    """One frame: chain() on the primary rays through the pixel centres, the arrays reshaped to (H, W, ...)."""
    o, d, rxd, ryd = DV.primary_rays(rs.orc, uniform, W, H)
    res = chain(rs, o, d, rxd, ryd, max_bounces, roughness_max, dtype, posed, oracle_hits)
    for k, v in list(res.items()):
        if k in ("rays", "origins", "directions"):
            res[k] = v.reshape(v.shape[0], H, W, v.shape[-1])
        elif isinstance(v, np.ndarray):
            res[k] = v.reshape((H, W) + v.shape[1:])
    return res


def decisions_differ(a, b):
    """Per pixel: the two results hit a different triangle at some bounce, or ended in another class, or after another length."""
    return (a["tri"] != b["tri"]).any(axis=-1) | (a["cls"] != b["cls"]) | (a["bounces"] != b["bounces"])


def images(res):
    return [res["normal"], res["position"], res["albedo"], res["surface"]]


def max_gap(r32, r64, where):
    """max |ref32 - ref64| per image over the pixels of `where`"""
    out = []
    for a, b in zip(images(r32), images(r64)):
        with np.errstate(all="ignore"):
            df = np.abs(a.astype(np.float64) - b)[where]
        out.append(float(df.max()) if df.size else 0.0)
    return out
