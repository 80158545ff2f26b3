"""An independent reference for texel production and the any-hit alpha test, in numpy from the specifications: the sRGB
transfer functions (IEC 61966-2-1 as the Vulkan specification quotes them), the linear vkCmdBlitImage (Vulkan "Image
Copies with Scaling": texel centres scaled into the source, clamp-to-edge, bilinear weights), the UNORM / sRGB 8-bit
conversions, the mip chain dimensions, the upload rules of docs/NEXT_ROWS.md section 7 and a repeat-addressed bilinear alpha.
Every function is generic over the float dtype: float64 is the reference, float32 measures the reference's own rounding.
Nothing here is taken from the kernels or from the oracle."""
import numpy as np

UNORM, SRGB, F32 = 0, 1, 2
MAX_EXTENT = 4096
UNLIMITED = 2**64 - 1


# ---------------------------------------------------------------------------------------
# transfer functions and the 8-bit conversions
# ---------------------------------------------------------------------------------------
def srgb_to_linear(c):
    c = np.asarray(c)
    dt = c.dtype.type
    return np.where(c <= dt(0.04045), c / dt(12.92), ((c + dt(0.055)) / dt(1.055)) ** dt(2.4))


def linear_to_srgb(x):
    x = np.asarray(x)
    dt = x.dtype.type
    return np.where(x <= dt(0.0031308), x * dt(12.92), dt(1.055) * np.maximum(x, dt(0)) ** (dt(1) / dt(2.4)) - dt(0.055))


def decode(texels, fmt, dtype=np.float64):
    """(h, w, 4) bytes (or float texels) -> linear values of `dtype`: b / 255, colour channels of an sRGB image through the
    transfer function, alpha linear."""
    if fmt == F32:
        return np.asarray(texels, np.float32).astype(dtype)
    c = np.asarray(texels).astype(dtype) / dtype(255)
    if fmt == SRGB:
        c = np.concatenate([srgb_to_linear(c[..., :3]), c[..., 3:]], axis=-1)
    return c


def encode_units(lin, fmt):
    """Linear values -> the value about to be stored, in code units (0 ... 255), before the rounding."""
    dt = lin.dtype.type
    c = lin
    if fmt == SRGB:
        c = np.concatenate([linear_to_srgb(lin[..., :3]), lin[..., 3:]], axis=-1)
    return np.clip(c, dt(0), dt(1)) * dt(255)


def quantise(v):
    """floor(v + 1/2) of a value in code units."""
    return np.floor(v + v.dtype.type(0.5)).astype(np.int64)


# ---------------------------------------------------------------------------------------
# the linear blit
# ---------------------------------------------------------------------------------------
def _axis(sn, dn, dt):
    x = (np.arange(dn).astype(dt) + dt(0.5)) * (dt(sn) / dt(dn)) - dt(0.5)
    x0 = np.floor(x)
    a = x - x0
    i0 = np.clip(x0, 0, sn - 1).astype(np.int64)
    i1 = np.clip(x0 + 1, 0, sn - 1).astype(np.int64)
    return i0, i1, a


def blit(src, dw, dh):
    """The linear vkCmdBlitImage of a whole image onto a dw x dh one.  src: (sh, sw, 4) linear values of any float dtype."""
    dt = src.dtype.type
    sh, sw = src.shape[:2]
    i0, i1, ax = _axis(sw, dw, dt)
    j0, j1, ay = _axis(sh, dh, dt)
    ax, ay = ax[None, :, None], ay[:, None, None]
    top = src[j0][:, i0] * (dt(1) - ax) + src[j0][:, i1] * ax
    bot = src[j1][:, i0] * (dt(1) - ax) + src[j1][:, i1] * ax
    return top * (dt(1) - ay) + bot * ay


def blit_step(texels, fmt, dw, dh, dtype=np.float64):
    """One upload-time blit of stored texels: decode, filter, re-encode.  Returns (v, code): the pre-quantisation value in code
    units and floor(v + 1/2) for the 8-bit formats; (values, values) for float texels."""
    out = blit(decode(texels, fmt, dtype), dw, dh)
    if fmt == F32:
        return out, out
    v = encode_units(out, fmt)
    return v, quantise(v)


# ---------------------------------------------------------------------------------------
# chain dimensions and the upload rules
# ---------------------------------------------------------------------------------------
def chain_dims(w, h):
    levels = int(np.floor(np.log2(max(w, h)))) + 1
    return [(max(w >> l, 1), max(h >> l, 1)) for l in range(levels)]


def chain_bytes(extent, fmt):
    texels = 0
    e = extent
    while e:
        texels += e * e
        e >>= 1
    return texels * (16 if fmt == F32 else 4)


def max_extent(fmt, budget_share, force_full=False):
    """The largest square extent, from 4096 down by halving, whose full mip chain fits the per-texture share."""
    e = MAX_EXTENT
    if force_full or budget_share >= UNLIMITED:
        return e
    while e > 1 and chain_bytes(e, fmt) > budget_share:
        e //= 2
    return e


def planned_extent(w, h, fmt, budget_share, force_full=False, file_levels=1):
    """What an upload of a w x h image with `file_levels` levels in its data becomes: a dict with the uploaded `extent`, the
    integer `scale`, the number of `halvings` of level 0 and whether one more blit to the exact extent follows (`final_blit`),
    and `skipped`, the number of leading file levels a complete file chain gives up instead (None: the file chain is not used;
    0: used as it is)."""
    mx = max_extent(fmt, budget_share, force_full)
    scale = max(-(-w // mx), -(-h // mx))
    ew, eh = max(w // scale, 1), max(h // scale, 1)
    plan = dict(extent=(ew, eh), scale=scale, halvings=0, final_blit=False, skipped=None)
    levels = len(chain_dims(ew, eh))
    if scale == 1:
        if file_levels == levels and levels > 1:
            plan["skipped"] = 0
        return plan
    skip = file_levels - levels
    if skip > 0 and (max(w >> skip, 1), max(h >> skip, 1)) == (ew, eh):
        plan["skipped"] = skip
        return plan
    k = 0
    while max(w >> (k + 1), 1) >= ew and max(h >> (k + 1), 1) >= eh and (max(w >> k, 1), max(h >> k, 1)) != (ew, eh):
        k += 1
    plan["halvings"] = k
    plan["final_blit"] = (max(w >> k, 1), max(h >> k, 1)) != (ew, eh)
    return plan


def scaled_steps(w, h, plan):
    """The extents the scaled-down path passes through after level 0."""
    steps = [(max(w >> k, 1), max(h >> k, 1)) for k in range(1, plan["halvings"] + 1)]
    if plan["final_blit"]:
        steps.append(plan["extent"])
    return steps


# ---------------------------------------------------------------------------------------
# the any-hit alpha
# ---------------------------------------------------------------------------------------
def alpha_at(alpha_level0, w, h, tu, tv, factor):
    """texture(colour texture, uv).a * colour factor's alpha at the base level: bilinear with repeat addressing.
    alpha_level0: (h, w) decoded alphas of the working dtype; tu, tv of the same dtype.  Returns (alpha, all_one): all_one
    marks the lookups whose whole footprint is 1 -- with a factor of 1 their alpha is exactly 1."""
    dt = alpha_level0.dtype.type
    tu, tv = np.asarray(tu, alpha_level0.dtype), np.asarray(tv, alpha_level0.dtype)
    if w == 1 and h == 1:
        a = np.full(tu.shape, alpha_level0[0, 0])
        return a * dt(factor), a == dt(1)
    x, y = tu * dt(w) - dt(0.5), tv * dt(h) - dt(0.5)
    x0, y0 = np.floor(x), np.floor(y)
    ax, ay = x - x0, y - y0
    i0, j0 = np.mod(x0.astype(np.int64), w), np.mod(y0.astype(np.int64), h)
    i1, j1 = np.mod(i0 + 1, w), np.mod(j0 + 1, h)
    t00, t10, t01, t11 = alpha_level0[j0, i0], alpha_level0[j0, i1], alpha_level0[j1, i0], alpha_level0[j1, i1]
    top = t00 * (dt(1) - ax) + t10 * ax
    bot = t01 * (dt(1) - ax) + t11 * ax
    a = top * (dt(1) - ay) + bot * ay
    one = (t00 == 1) & (t10 == 1) & (t01 == 1) & (t11 == 1)
    a = np.where(one, dt(1), a)
    return a * dt(factor), one


CLOSEST_THRESHOLD, SHADOW_THRESHOLD = 0.5, 1.0  # a closest ray ignores alpha < 0.5, a shadow ray alpha < 1


def barycentrics_f64(tri, rays):
    """Moeller-Trumbore in float64 of rays (n, 8) against ONE triangle (3, 3), vectorised over the rays -- the formulas of
    util.moller_trumbore_f64, which is vectorised over the triangles: (inside, t, u, v)."""
    o, d = np.float64(rays[:, 0:3]), np.float64(rays[:, 4:7])
    tmin, tmax = np.float64(rays[:, 3]), np.float64(rays[:, 7])
    v0, e1, e2 = tri[0], tri[1] - tri[0], tri[2] - tri[0]
    p = np.cross(d, e2)
    det = p @ e1
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = 1.0 / det
        s = o - v0
        u = np.einsum("ij,ij->i", s, p) * inv
        q = np.cross(s, e1)
        v = np.einsum("ij,ij->i", q, d) * inv
        t = (q @ e2) * inv
    inside = (u >= 0) & (v >= 0) & (u + v <= 1) & (t > tmin) & (t < tmax) & (np.abs(det) > 1e-300)
    return inside, t, u, v
