"""CPU restatement of the screen path (include/ptx.h ptx_present, csrc/pt_present.hpp), generic over a numpy dtype.

Written from the reference's shader text (uiComposition.comp, toneMapping.comp) and the Vulkan specification's linear blit
with clamp to edge; steps 2 - 4 of the screen path.  Step 1, the composed colour, is the oracle's
orc.postprocess(..., tone_mapping=1): the HDR mode passes composition.comp's result through.

Arithmetic conventions, the project's, in either dtype: a / b is a * (1 / b); pow and exp are evaluated in
double precision and rounded to the dtype once.  Every store into the reference's rgba16f screen image is a rounding to binary16
(astype(np.float16)): after the blit, after tone mapping, after the UI composition."""
import numpy as np

WHITE_POINT = 203.0  # BT.2408 reference white, uiComposition.comp:58


def _f16(x, dtype):
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(x).astype(np.float16).astype(dtype)


def _div(a, b, dtype):
    return np.asarray(a, dtype) * (dtype(1.0) / np.asarray(b, dtype))


def _pow(x, y, dtype):
    with np.errstate(all="ignore"):
        return np.power(np.asarray(x, np.float64), np.float64(dtype(y))).astype(dtype)


def _exp(x, dtype):
    with np.errstate(all="ignore"):
        return np.exp(np.asarray(x, np.float64)).astype(dtype)


def srgb_to_linear(c, dtype=np.float64):
    """uiComposition.comp:40-47: mix(c / 12.92, pow((c + 0.055) / 1.055, 2.4), step(0.0404482362771082, c))."""
    c = np.asarray(c, dtype)
    low = _div(c, dtype(12.92), dtype)
    high = _pow(_div(c + dtype(0.055), dtype(1.055), dtype), 2.4, dtype)
    return np.where(c >= dtype(0.0404482362771082), high, low)


# uiComposition.comp:17-22: the three initialiser lists are the matrix' columns and the colour multiplies from the left, so
# output channel i is the dot product of the colour with the i-th triple
FROM_709_TO_2020 = ((0.6274040, 0.3292820, 0.0433136), (0.0690970, 0.9195400, 0.0113612), (0.0163916, 0.0880132, 0.8955950))


def linear_to_hdr10(color, white_point=WHITE_POINT, dtype=np.float64):
    """uiComposition.comp:15-37."""
    color = np.asarray(color, dtype)
    r, g, b = color[..., 0], color[..., 1], color[..., 2]
    c = np.stack([r * dtype(m[0]) + g * dtype(m[1]) + b * dtype(m[2]) for m in FROM_709_TO_2020], axis=-1)
    with np.errstate(all="ignore"):
        c = c * _div(dtype(white_point), dtype(10000.0), dtype)
        m1, m2 = dtype(2610.0 / 4096.0 / 4), dtype(2523.0 / 4096.0 * 128)
        c1, c2, c3 = dtype(3424.0 / 4096.0), dtype(2413.0 / 4096.0 * 32), dtype(2392.0 / 4096.0 * 32)
        cp = _pow(np.abs(c), m1, dtype)
        return _pow(_div(c1 + c2 * cp, dtype(1.0) + c3 * cp, dtype), m2, dtype)


def blit_axis(src, dst, dtype):
    """Texel indices and the weight of the second for every destination coordinate of one axis; None for an axis that is not
    filtered (equal extents)."""
    if src == dst:
        return None
    s = np.arange(dst).astype(dtype)
    x = (s + dtype(0.5)) * _div(dtype(src), dtype(dst), dtype) - dtype(0.5)
    x0 = np.floor(x)
    t = x - x0
    i0 = np.clip(x0, 0, src - 1).astype(np.int64)
    i1 = np.clip(x0 + 1, 0, src - 1).astype(np.int64)
    return i0, i1, t


def blit(img, screen_w, screen_h, dtype):
    """vkCmdBlitImage(eLinear), H x W x C -> screen_h x screen_w x C: a * (1 - t) + b * t, first along x, then along y."""
    img = np.asarray(img, dtype)
    h, w = img.shape[:2]
    ax, ay = blit_axis(w, screen_w, dtype), blit_axis(h, screen_h, dtype)
    with np.errstate(all="ignore"):
        if ax is not None:
            i0, i1, t = ax
            t = t[None, :, None]
            img = img[:, i0] * (dtype(1.0) - t) + img[:, i1] * t
        if ay is not None:
            i0, i1, t = ay
            t = t[:, None, None]
            img = img[i0] * (dtype(1.0) - t) + img[i1] * t
    return img


def tone_map(c, hdr, dtype):
    """toneMapping.comp:19-21."""
    return c if hdr else dtype(1.0) - _exp(-c, dtype)


def present(composed, ui, screen_w, screen_h, hdr, dtype=np.float64):
    """Steps 2 - 4: composed H x W x (3|4) binary16-valued colour, ui None or screen_h x screen_w x 4 uint8 -> the screen image,
    screen_h x screen_w x 4 of `dtype`, binary16-valued, alpha 1."""
    c = np.asarray(composed)[..., :3].astype(dtype)
    c = _f16(blit(c, screen_w, screen_h, dtype), dtype)
    c = _f16(tone_map(c, hdr, dtype), dtype)
    if ui is not None:
        ui = np.asarray(ui)
        assert ui.shape == (screen_h, screen_w, 4) and ui.dtype == np.uint8
        u = _div(ui[..., :3].astype(dtype), dtype(255.0), dtype)
        over = srgb_to_linear(u, dtype) * dtype(0.99) + c * dtype(0.01)
        c = np.where(ui[..., 3:4] > 0, over, c)
    if hdr:
        c = linear_to_hdr10(c, WHITE_POINT, dtype)
    out = np.ones((screen_h, screen_w, 4), dtype)
    out[..., :3] = _f16(c, dtype)
    return out


def pack_a2b10g10r10(img):
    """R | G << 10 | B << 20 | 3 << 30 of floor(clamp(c, 0, 1) * 1023 + 0.5), NaN -> 0."""
    c = np.asarray(img)[..., :3].astype(np.float32)
    with np.errstate(invalid="ignore"):
        q = np.floor(np.clip(np.where(np.isnan(c), np.float32(0), c), 0, 1) * np.float32(1023) + np.float32(0.5)).astype(np.uint32)
    return q[..., 0] | q[..., 1] << np.uint32(10) | q[..., 2] << np.uint32(20) | np.uint32(3 << 30)
