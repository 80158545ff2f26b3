"""The motion guides and the accumulation through them (include/ptx.h ptx_render_guides_motion, ptx_temporal_accumulate_motion;
docs/NEXT_ROWS.md section 17), restated in numpy from the header text.  Generic over float32 and float64.

The current pose's primary hits come from the oracle (debug_view_ref.RefScene, osc.trace_closest: tri -> pair, prim, u, v), the
previous pose's vertices from a second RefScene and, for animated geometry, its skinned vertex block in the reference's own number
format (skin_ref.skin_vertices).  material.Normal is evaluated once per hit at uv = 0 without derivatives: scenes whose normal
texture is absent or 1 x 1 have no other value, and the reference is good for those alone.
"""
import numpy as np

import debug_view_ref as DV
import denoise_ref as R
import skin_ref as S
import temporal_ref as TR
import util

MOTION_POSITION, MOTION_NORMAL = 0, 1


def skinned_block(rs, bones, dtype):
    """The skinned vertex block of RefScene `rs` posed by `bones` (None: the bind pose) in the device's order -- one copy per
    (instance, animated mesh) pair, in pair order -- as rows of 14 values in `dtype`; None for a scene without animated geometry."""
    n = int(rs.desc.animatedVertexCount)
    if not n:
        return None
    animated = util._view(rs.desc.animatedVertices, n, S.ANIMATED_VERTEX_DT)
    g = rs.a["geometries"][rs.pair[:, 2]]
    src = [np.arange(x["VertexOffset"], x["VertexOffset"] + x["VertexLength"]) for x in g if x["IsAnimated"]]
    if not src:
        return None
    rows = S.bind_vertices(animated, dtype) if bones is None or not len(bones) else S.skin_vertices(animated, bones, dtype)
    return rows[np.concatenate(src)]


def primary_hits(rs, uniform, W, H):
    """(hit mask (n), pair, prim, u, v of the hits) of the primary rays of the whole image, row-major"""
    o, d, _, _ = DV.primary_rays(rs.orc, uniform, W, H)
    rays = np.zeros((W * H, 8), np.float32)
    rays[:, 0:3], rays[:, 3], rays[:, 4:7], rays[:, 7] = o, 1e-5, d, 1e4
    hits = rs.osc.trace_closest(rays)
    hit = hits["tri"] != DV.MISS
    tri = hits["tri"][hit].astype(np.int64)
    p = np.searchsorted(rs.first, tri, side="right") - 1
    return hit, p, tri - rs.first[p], hits["u"][hit], hits["v"][hit], hits["t"]


def material_normal(rs, p):
    """material.Normal of the pairs p: the oracle's sampleMaterial on the texels at uv = 0 (see the module's note)"""
    mtype, rec, idx = rs.material_record(rs.pair[p, 3])
    m = len(p)
    inp = np.zeros((m, 47), np.float32)
    iu = inp.view(np.uint32)
    iu[:, 0], iu[:, 1], iu[:, 2] = mtype, 0, 1 if rs.desc.dxNormalTextures else 0
    inp[:, 3:27] = rec
    zero2, zero4 = np.zeros((m, 2), np.float32), np.zeros((m, 4), np.float32)
    for k in range(5):
        inp[:, 27 + 4 * k:31 + 4 * k] = rs.texels(idx[:, k], zero2, zero4)
    return rs.orc.test_eval(DV.FN_SAMPLE_MATERIAL, inp, 17).view(np.float32)[:, 6:9].copy()


def surface(rs, posed, p, prim, u, v, nmap, dtype):
    """(Position, shading normal) of the points (pair p, prim, u, v) in the pose RefScene `rs` describes, `posed` its skinned block
    in `dtype`: the header's steps 1 - 4."""
    u, v = u.astype(dtype), v.astype(dtype)
    b = np.stack([dtype(1) - u - v, u, v], axis=1)
    g = rs.a["geometries"][rs.pair[p, 2]]
    anim = g["IsAnimated"] != 0
    corner = (g["IndexOffset"].astype(np.int64) + 3 * prim)[:, None] + np.arange(3)
    vtx = np.zeros((len(p), 3, 14), dtype)
    vtx[~anim] = rs.a["vertices"][rs.a["indices"][corner[~anim]] + g["VertexOffset"].astype(np.int64)[~anim, None]].astype(dtype)
    if anim.any():
        assert posed is not None and posed.dtype == np.dtype(dtype)
        vtx[anim] = posed[rs.a["animated_indices"][corner[anim]] + rs.skinned_first[p[anim], None]]
    M = rs.pair_matrix(dtype)[p]
    A, tr = M[:, :, 0:3], M[:, :, 3]
    Ainv_t = np.linalg.inv(A.astype(np.float64)).astype(dtype).transpose(0, 2, 1)

    def interp(x):
        return (x[:, 0] * b[:, 0:1] + x[:, 1] * b[:, 1:2]) + x[:, 2] * b[:, 2:3]

    P = np.einsum("nij,nj->ni", A, interp(vtx[:, :, 0:3])) + tr
    Nv = DV._normalize(np.einsum("nij,nj->ni", Ainv_t, interp(vtx[:, :, 5:8])))
    Tv = DV._normalize(np.einsum("nij,nj->ni", A, interp(vtx[:, :, 8:11])))
    Bv = DV._normalize(np.einsum("nij,nj->ni", A, interp(vtx[:, :, 11:14])))
    nm = nmap.astype(dtype)
    N = DV._normalize(Nv + ((Tv * nm[:, 0:1] + Bv * nm[:, 1:2]) + Nv * nm[:, 2:3]))
    return P, N


def motion_guides(rs_cur, posed_cur, rs_prev, posed_prev, uniform, W, H, dtype):
    """(normal guide, position guide, X_prev, N_prev), (H, W, 4) in `dtype`, of the current pose (rs_cur, posed_cur) seen through
    `uniform`; rs_prev None: the motion is unknown."""
    hit, p, prim, u, v, t = primary_hits(rs_cur, uniform, W, H)
    out = [np.zeros((W * H, 4), dtype) for _ in range(4)]
    if hit.any():
        nmap = material_normal(rs_cur, p)
        P, N = surface(rs_cur, posed_cur, p, prim, u, v, nmap, dtype)
        out[0][hit, 0:3], out[0][hit, 3] = N, 1
        out[1][hit, 0:3], out[1][hit, 3] = P, t[hit].astype(dtype)
        if rs_prev is None:
            out[2][hit, 0:3], out[3][hit, 0:3] = P, N
        else:
            Pp, Np = surface(rs_prev, posed_prev, p, prim, u, v, nmap, dtype)
            out[2][hit, 0:3], out[2][hit, 3] = Pp, 1
            out[3][hit, 0:3], out[3][hit, 3] = Np, 1
    return [a.reshape(H, W, 4) for a in out]


def accumulate_motion(S_, normal, position, albedo, x_prev, n_prev, total_samples, view, proj, history, max_history, normal_threshold,
                      position_threshold, flags=0, dtype=np.float64):
    """temporal_ref.accumulate with steps 1 and 2 run on (x~, n~) = (x_prev.xyz, n_prev.xyz): x~ is projected, the taps are tested
    against n~ and x~; one tap of weight 1 at p needs equal matrices and x~ bit-equal to x_p, any other pixel is projected; a pixel
    whose x_prev.w is not 1 takes no history.  Returns what temporal_ref.accumulate returns; decisions['taps'] slot 0 is the tap at p
    where the same-camera rule applied ('at_pixel')."""
    assert total_samples > 0 and max_history >= 1 and normal_threshold > 0 and position_threshold > 0 and flags in (0, TR.RESET)
    h, w = np.asarray(S_).shape[:2]
    m = R.mean_of(S_, total_samples, dtype)
    valid = R.valid_mask(S_, normal, position, total_samples, dtype)
    n = np.asarray(normal, np.float32)[..., 0:3].astype(dtype)
    x = np.asarray(position, np.float32)[..., 0:3].astype(dtype)
    t = np.asarray(position, np.float32)[..., 3].astype(dtype)
    xm32, nm32 = np.asarray(x_prev, np.float32), np.asarray(n_prev, np.float32)
    xt, nt = xm32[..., 0:3].astype(dtype), nm32[..., 0:3].astype(dtype)
    known = xm32[..., 3] == 1
    a = np.maximum(np.asarray(albedo, np.float32)[..., 0:3].astype(dtype), dtype(np.float32(R.ALBEDO_FLOOR)))
    view, proj = np.array(view, np.float32).reshape(16), np.array(proj, np.float32).reshape(16)
    nt2 = dtype(np.float32(normal_threshold)) * dtype(np.float32(normal_threshold))
    pt = dtype(np.float32(position_threshold))
    cell = np.full((h, w, 2), -2 ** 31, np.int64)
    taps = np.zeros((h, w, 4), bool)
    found = np.zeros((h, w), bool)
    at_pixel = np.zeros((h, w), bool)
    used, same = history is not None and not (flags & TR.RESET), False
    with np.errstate(all="ignore"):
        c = np.where(valid[..., None], m / a, m)
        c_acc, L = c.copy(), np.where(valid, dtype(1), dtype(0))
        if used:
            same = bool((history.view.view(np.uint32) == view.view(np.uint32)).all() and (history.proj.view(np.uint32) == proj.view(np.uint32)).all())
            look = valid & known
            yy, xx = np.mgrid[0:h, 0:w]
            if same:
                at_pixel = look & (xm32[..., 0:3].view(np.uint32) == np.asarray(position, np.float32)[..., 0:3].view(np.uint32)).all(axis=-1)
            u, v, ok = TR.project(history.view, history.proj, xt, w, h, dtype)
            ok &= look & ~at_pixel
            x0f, y0f = np.floor(u), np.floor(v)
            fx, fy = u - x0f, v - y0f
            ok &= (x0f >= -1) & (x0f <= w) & (y0f >= -1) & (y0f <= h)
            x0, y0 = np.where(ok, x0f, -2 ** 31).astype(np.int64), np.where(ok, y0f, -2 ** 31).astype(np.int64)
            cell[..., 0], cell[..., 1] = x0, y0
            candidates = []
            for j in (0, 1):
                for i in (0, 1):
                    qx, qy = x0 + i, y0 + j
                    inside = ok & (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
                    wgt = (fx if i else dtype(1) - fx) * (fy if j else dtype(1) - fy)
                    if i == 0 and j == 0:  # the tap at p of the same-camera rule shares slot 0: no pixel has both
                        qy, qx, wgt, inside = np.where(at_pixel, yy, qy), np.where(at_pixel, xx, qx), np.where(at_pixel, dtype(1), wgt), inside | at_pixel
                    candidates.append((np.where(inside, qy, 0), np.where(inside, qx, 0), wgt, inside))
            num, lnum, den = np.zeros((h, w, 3), dtype), np.zeros((h, w), dtype), np.zeros((h, w), dtype)
            for k, (qy, qx, wgt, inside) in enumerate(candidates):
                Hq, Lq, Nq, Xq = history.c[qy, qx], history.L[qy, qx], history.n[qy, qx], history.x[qy, qx]
                dn = nt - Nq
                plane = (nt * (Xq - xt)).sum(axis=-1)
                counts = inside & (Lq > 0) & np.isfinite(Hq).all(axis=-1) & ((dn * dn).sum(axis=-1) <= nt2) & (np.abs(plane) <= pt * t)
                taps[..., k] = counts
                wk = np.where(counts, wgt, dtype(0))
                num = num + wk[..., None] * np.where(counts[..., None], Hq, dtype(0))
                lnum = lnum + wk * np.where(counts, Lq, dtype(0))
                den = den + wk
            found = valid & (den >= dtype(TR.FOUND_FLOOR))
            safe = np.where(found, den, dtype(1))
            c_h, L_h = num / safe[..., None], lnum / safe
            L_new = np.minimum(L_h + dtype(1), dtype(np.float32(max_history)))
            blended = c_h + (c - c_h) / np.where(found, L_new, dtype(1))[..., None]
            c_acc = np.where(found[..., None], blended, c)
            L = np.where(found, L_new, L)
        T = np.zeros((h, w, 4), dtype)
        T[..., 0:3] = np.where(valid[..., None], c_acc * a, m)
        T[..., 3] = L
    nxt = TR.History(np.where(valid[..., None], c_acc, dtype(0)), L, n, x, view, proj)  # the CURRENT normal and position
    return T, nxt, {"cell": cell, "taps": taps, "found": found, "valid": valid, "used_history": used, "same_camera": False, "at_pixel": at_pixel}


def run_sequence(frames, max_history, normal_threshold, position_threshold, dtype):
    """frames: [(S, normal, position, albedo, x_prev, n_prev, total_samples, view, proj, flags)]; ([T], [decisions]) of one chain"""
    hist, out, dec = None, [], []
    for S_, nrm, pos, alb, xp, npv, n, view, proj, flags in frames:
        T, hist, d = accumulate_motion(S_, nrm, pos, alb, xp, npv, n, view, proj, hist, max_history, normal_threshold, position_threshold, flags, dtype)
        out.append(T)
        dec.append(d)
    return out, dec


def comparable_pixels(dec32, dec64):
    """temporal_ref.comparable_pixels for chains of accumulate_motion: a pixel is kept where the two precisions decided alike, here
    and on every pixel its history came from -- the tap at p under the same-camera rule, the four texels of its cell otherwise."""
    out, prev = [], None
    for a, b in zip(dec32, dec64):
        keep = TR.same_decisions(a, b) & (a["at_pixel"] == b["at_pixel"])
        if b["used_history"] and prev is not None:
            h, w = keep.shape
            keep &= ~b["at_pixel"] | prev
            x0, y0 = b["cell"][..., 0], b["cell"][..., 1]
            for j in (0, 1):
                for i in (0, 1):
                    qx, qy = x0 + i, y0 + j
                    inside = (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
                    keep &= ~inside | prev[np.where(inside, qy, 0), np.where(inside, qx, 0)]
        out.append(keep)
        prev = keep
    return out
