"""CPU restatement of the bloom chain of the output stage (include/ptx.h ptx_postprocess, csrc/pt_post.hpp k_postprocess,
k_bloom_downsample, k_bloom_upsample, k_compose_tonemap in HDR mode), generic over a numpy dtype.

Written from the reference's shader text -- postprocess.comp:22-36, bloomDownsample.comp:28-55, bloomUpsample.comp:28-53,
composition.comp:22 -- from the dispatch loops of Renderer.cpp:955-1063 and from the Vulkan specification's texel filtering
("Texel Coordinate Systems", "Texel Filtering": linear filter, clamp to edge) and mip extents ("Image Mip Level Sizing"); not
from the project's kernels or its oracle.  Images are H x W x C arrays, any C: the tests use the channels as independent cases.

Arithmetic conventions, the project's, in either dtype: a / b is a * (1 / b); literal constants and the
uniform's float32 values are taken in the dtype.  Every store into one of the reference's rgba16f images is a rounding to
binary16 (astype(np.float16)).

Tap tables, in source texels relative to the destination texel's centre (x to the right, y down the array; the shader's +y):

    down, weight          up, weight / 16
    g . h . i   y = -2    g h i   y = -1    1 2 1
    . l . m .   y = -1    d e f   y =  0    2 4 2
    d . e . f   y =  0    a b c   y = +1    1 2 1
    . j . k .   y = +1
    a . b . c   y = +2
    e 0.125; a c g i 0.03125 each; b d f h 0.0625 each; j k l m 0.125 each: they sum to 1.

A destination centre of a 2:1 step lies on a corner of four source texels, so every down tap is the mean of a 2 x 2 block; of a
1:2 step a quarter texel off a source centre, so every up tap weighs two texels 3/4 and 1/4 per axis."""
import numpy as np

MAX_BLOOM_MIP_LEVEL = 12  # ShaderRendererTypes.incl MaxBloomMipmapLevel
KNEE = 0.5                # postprocess.comp:30


def _f16(x, dtype):
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(x).astype(np.float16).astype(dtype)


def _rcp(b, dtype):
    return dtype(1.0) / np.asarray(b, dtype)


def levels_used(W, H):
    """The (h, w) extents of the mips that take part, level 0 first.  The image has floor(log2(max(W, H))) + 1 mips
    (Image.cpp:14-17); mips 0 .. min(levels - 3, MaxBloomMipmapLevel) - 1 are written by the down loop and read by the up
    loop (Renderer.cpp:955-1000).  Below five mips `levels - 3` would leave no second level or wrap around: level 0 alone takes
    part, the project's documented reading."""
    W, H = int(W), int(H)
    assert W >= 1 and H >= 1
    levels = max(W, H).bit_length()  # floor(log2(m)) + 1
    n = min(levels - 3, MAX_BLOOM_MIP_LEVEL) if levels >= 5 else 1
    return [(max(1, H >> l), max(1, W >> l)) for l in range(n)]


def _axis(coord, size, dtype):
    """Linear filter along one axis: normalised coordinates -> texel i0, texel i1, weight of i1.  Unnormalised u = s * size, the
    pair is floor(u - 0.5) and the next texel, the weight frac(u - 0.5); clamp to edge clamps the indices."""
    x = np.asarray(coord, dtype) * dtype(size) - dtype(0.5)
    x0 = np.floor(x)
    a = x - x0
    i0 = np.clip(x0, 0, size - 1).astype(np.int64)
    i1 = np.clip(x0 + dtype(1.0), 0, size - 1).astype(np.int64)
    return i0, i1, a


def tap(img, u, v, dtype=np.float64):
    """texture(sampler, (u[i], v[j])) for every pair: u holds the x coordinates (n values), v the y coordinates (m values), the
    result is m x n x C.  tau = (p00 (1 - a) + p10 a)(1 - b) + (p01 (1 - a) + p11 a) b: along x first, then along y."""
    img = np.asarray(img, dtype)
    h, w = img.shape[:2]
    ix0, ix1, a = _axis(np.atleast_1d(u), w, dtype)
    iy0, iy1, b = _axis(np.atleast_1d(v), h, dtype)
    a, b = a[None, :, None], b[:, None, None]
    one = dtype(1.0)
    with np.errstate(invalid="ignore", over="ignore"):
        top = img[iy0][:, ix0] * (one - a) + img[iy0][:, ix1] * a
        bot = img[iy1][:, ix0] * (one - a) + img[iy1][:, ix1] * a
        return top * (one - b) + bot * b


def _uv(dst_shape, dtype):
    """(vec2(dstCoords) + 0.5) / vec2(dstSize)"""
    dh, dw = dst_shape
    u = (np.arange(dw).astype(dtype) + dtype(0.5)) * _rcp(dw, dtype)
    v = (np.arange(dh).astype(dtype) + dtype(0.5)) * _rcp(dh, dtype)
    return u, v


def down(src, dst_shape, dtype=np.float64):
    """bloomDownsample.comp: level i -> the (h, w) of level i + 1."""
    src = np.asarray(src, dtype)
    sh, sw = src.shape[:2]
    tx, ty = _rcp(sw, dtype), _rcp(sh, dtype)  # srcTexelSize
    u, v = _uv(dst_shape, dtype)
    t = lambda ox, oy: tap(src, u + dtype(ox) * tx, v + dtype(oy) * ty, dtype)  # noqa: E731
    with np.errstate(invalid="ignore", over="ignore"):
        a, b, c = t(-2, 2), t(0, 2), t(2, 2)
        d, e, f = t(-2, 0), t(0, 0), t(2, 0)
        g, h, i = t(-2, -2), t(0, -2), t(2, -2)
        j, k, l, m = t(-1, 1), t(1, 1), t(-1, -1), t(1, -1)
        out = e * dtype(0.125)
        out = out + (((a + c) + g) + i) * dtype(0.03125)
        out = out + (((b + d) + f) + h) * dtype(0.0625)
        out = out + (((j + k) + l) + m) * dtype(0.125)
    return _f16(out, dtype)


def up(src, dst, dtype=np.float64):
    """bloomUpsample.comp: the 3 x 3 tent of level i added onto level i - 1 (`dst`, which is returned anew)."""
    src, dst = np.asarray(src, dtype), np.asarray(dst, dtype)
    sh, sw = src.shape[:2]
    x, y = _rcp(sw, dtype), _rcp(sh, dtype)
    u, v = _uv(dst.shape[:2], dtype)
    zero = dtype(0.0)
    t = lambda ox, oy: tap(src, u + ox, v + oy, dtype)  # noqa: E731
    with np.errstate(invalid="ignore", over="ignore"):
        a, b, c = t(-x, y), t(zero, y), t(x, y)
        d, e, f = t(-x, zero), t(zero, zero), t(x, zero)
        g, h, i = t(-x, -y), t(zero, -y), t(x, -y)
        out = e * dtype(4.0)
        out = out + (((b + d) + f) + h) * dtype(2.0)
        out = out + (((a + c) + g) + i)
        out = out * (dtype(1.0) / dtype(16.0))
        return _f16(dst + out, dtype)


def chain(bloom0, dtype=np.float64):
    """Level 0 after the down loop (i = 0 .. n - 2) and the up loop (i = n - 1 .. 1), Renderer.cpp:958-1038."""
    bloom0 = np.asarray(bloom0, dtype)
    extents = levels_used(bloom0.shape[1], bloom0.shape[0])
    mips = [bloom0]
    for shape in extents[1:]:
        mips.append(down(mips[-1], shape, dtype))
    for i in range(len(mips) - 1, 0, -1):
        mips[i - 1] = up(mips[i], mips[i - 1], dtype)
    return mips[0]


def prefilter(acc, samples, exposure, threshold, dtype=np.float64):
    """postprocess.comp:22-36 and its two stores: H x W x (3|4) running sum -> (post-process colour, bloom colour), binary16-valued."""
    color = np.asarray(acc, np.float32)[..., :3].astype(dtype)
    exposure, threshold = dtype(np.float32(exposure)), dtype(np.float32(threshold))
    with np.errstate(all="ignore"):
        color = color * _rcp(np.float32(np.uint32(samples)), dtype) * exposure
        color = np.where(np.isnan(color).any(axis=-1, keepdims=True), np.array([5000.0, 0.0, 0.0], dtype), color)
        color = np.where(np.isinf(color).any(axis=-1, keepdims=True), np.array([0.0, 5000.0, 0.0], dtype), color)
        knee = dtype(KNEE)
        br = np.maximum(color[..., 0], np.maximum(color[..., 1], color[..., 2]))
        cx, cy, cz = threshold - knee, knee * dtype(2.0), dtype(0.25) * _rcp(knee, dtype)
        rq = np.clip(br - cx, dtype(0.0), cy)
        rq = cz * rq * rq
        scale = np.maximum(rq, br - threshold) * _rcp(np.maximum(br, dtype(0.0001)), dtype)
        bloom = color * scale[..., None]
    return _f16(color, dtype), _f16(bloom, dtype)


def composed(acc, samples, exposure, threshold, intensity, dtype=np.float64):
    """The colour that the HDR mode passes through: composition.comp:22 on the post-process image and level 0 of the chain,
    H x W x 3 of `dtype`, binary16-valued."""
    post, bloom0 = prefilter(acc, samples, exposure, threshold, dtype)
    bloom0 = chain(bloom0, dtype)
    with np.errstate(all="ignore"):
        k = dtype(np.float32(intensity)) * dtype(0.1)
        return _f16(bloom0 * k + post * dtype(1.0), dtype)
