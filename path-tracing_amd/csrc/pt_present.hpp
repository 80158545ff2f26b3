// pt_present.hpp -- the screen path (row D15) on the device: what turns the post-processed frame into the swapchain image.
//
//   Renderer::RecordPostProcessCommands' final blit (Renderer.cpp:1075-1085)   composed rgba16f image -> ScreenImage at the
//                                                                              swapchain's extent, vkCmdBlitImage(eLinear)
//   toneMapping.comp on ScreenImage (:1138-1151)                               HDR mode iff Swapchain::IsHdr()
//   uiComposition.comp:49-63 (:1160-1168)                                      UI over the frame, BT.2020 / ST 2084 encode
//   the blit into the swapchain image (:1174-1191)                             the store in the surface's format
//
// One body, presentPixel, under k_present (and k_present_graded of pt_grade.hpp, with the grade where the tone mapping stands), one
// thread per SCREEN pixel in row-major order: up to four taps of the post-process image and bloom
// level 0 in (composition.comp is evaluated per tap, as the reference blits the composed image), one word of the UI image, one
// 4- or 8-byte store out.  The tone-mapping mode and the surface format are template parameters; whether an axis is filtered
// and whether there is a UI image are wave-uniform arguments.  No LDS, no scratch.  Every store of the reference into an rgba16f
// image is an f16Round here, as in pt_post.hpp.
//
// The blit is the Vulkan specification's linear filter with clamp to edge (unnormalised coordinate (s + 0.5) * W / SW - 0.5,
// weights from its fraction), not a bit-match of any GPU's fixed-function filter; k_blit_level takes the same stance.  An axis
// whose screen extent equals the render extent is NOT filtered (one texel, no arithmetic): W * rcp(W) is not 1 for every W, and
// a frame shown at its own size comes through bit for bit.
#pragma once

#include "pt_post.hpp"

namespace ptd
{

// uiComposition.comp:40-47.  The shader's own function and threshold, not srgbToLinear of pt_device.hpp (0.04045);
// mix(low, high, step(threshold, c)) with a 0 / 1 weight is the selection.
PT_DEV float uiSrgbToLinear(float c)
{
    return c >= 0.0404482362771082f ? pow_(div_(c + 0.055f, 1.055f), 2.4f) : div_(c, 12.92f);
}

// uiComposition.comp:15-37.  `color * from709to2020` is a row vector times a matrix whose initialiser lists are its columns:
// output channel i is the dot product of the colour with the i-th listed triple.  m1, m2, c1, c2, c3 are exact in binary32.
PT_DEV float pqEncode(float c)
{
    const float m1 = 2610.0f / 4096.0f / 4.0f, m2 = 2523.0f / 4096.0f * 128.0f;
    const float c1 = 3424.0f / 4096.0f, c2 = 2413.0f / 4096.0f * 32.0f, c3 = 2392.0f / 4096.0f * 32.0f;
    const float cp = pow_(abs_(c), m1);
    return pow_(div_(c1 + c2 * cp, 1.0f + c3 * cp), m2);
}
PT_DEV f3 linearToHdr10(f3 color, float whitePoint)
{
    f3 c = F3(color.x * 0.6274040f + color.y * 0.3292820f + color.z * 0.0433136f,
              color.x * 0.0690970f + color.y * 0.9195400f + color.z * 0.0113612f,
              color.x * 0.0163916f + color.y * 0.0880132f + color.z * 0.8955950f);
    c = c * div_(whitePoint, 10000.0f);
    return F3(pqEncode(c.x), pqEncode(c.y), pqEncode(c.z));
}

// bits of a float that already is a binary16 value (f16Round's result)
PT_DEV uint32_t f16Bits(float f)
{
    const uint32_t x = __float_as_uint(f), sign = (x >> 16) & 0x8000u, ax = x & 0x7fffffffu;
    if (ax >= 0x7f800000u)
        return sign | (ax > 0x7f800000u ? 0x7e00u : 0x7c00u);
    if (ax < 0x38800000u) // half subnormal: a multiple of 2^-24
        return sign | (uint32_t)(__uint_as_float(ax) * 16777216.0f);
    return sign | ((ax - 0x38000000u) >> 13);
}

PT_DEV uint32_t quantize10(float x) // UNORM10: NaN -> 0, as quantize8 treats it; binary16 value * 1023 is exact in binary32
{
    if (!(x > 0.0f))
        return 0u;
    if (x > 1.0f)
        x = 1.0f;
    return (uint32_t)__builtin_floorf(x * 1023.0f + 0.5f);
}

constexpr uint32_t kPresentBlock = 256;

struct PresentArgs
{
    const float *post, *bloom0;      // what ptx_postprocess left: post-process image and bloom level 0 after the upsample chain
    const uint32_t *ui;              // RGBA8 UNORM at the screen extent, or null (alpha 0 everywhere)
    void *out;                       // SW * SH texels of the surface format
    PtxPostProcessingUniformData u;  // of that ptx_postprocess
    uint32_t W, H, SW, SH;           // render and screen extent
};

// composition.comp's store at render pixel (x, y)
PT_DEV f3 presentTexel(const PresentArgs &a, uint32_t x, uint32_t y)
{
    const size_t i = ((size_t)y * a.W + x) * 3;
    return f16Round(compositionPixel(F3(a.post[i], a.post[i + 1], a.post[i + 2]), F3(a.bloom0[i], a.bloom0[i + 1], a.bloom0[i + 2]), a.u));
}

// one axis of the blit: texel indices and the weight of the second
PT_DEV void presentAxis(uint32_t s, uint32_t srcExtent, uint32_t dstExtent, uint32_t &i0, uint32_t &i1, float &t)
{
    const float x = ((float)s + 0.5f) * div_((float)srcExtent, (float)dstExtent) - 0.5f;
    const float x0 = __builtin_floorf(x), m = (float)(srcExtent - 1);
    t = x - x0;
    i0 = (uint32_t)clamp_(x0, 0.0f, m);
    i1 = (uint32_t)clamp_(x0 + 1.0f, 0.0f, m);
}

PT_DEV f3 presentRow(const PresentArgs &a, bool filterX, uint32_t ix0, uint32_t ix1, float ax, uint32_t y)
{
    const f3 l = presentTexel(a, ix0, y);
    if (!filterX)
        return l;
    const f3 r = presentTexel(a, ix1, y);
    return l * (1.0f - ax) + r * ax;
}

// The scaling blit at screen pixel (sx, sy): the value ScreenImage is about to store, not yet rounded
PT_DEV f3 presentBlit(const PresentArgs &a, uint32_t sx, uint32_t sy)
{
    const bool filterX = a.SW != a.W, filterY = a.SH != a.H;
    uint32_t ix0 = sx, ix1 = sx, iy0 = sy, iy1 = sy;
    float ax = 0.0f, ay = 0.0f;
    if (filterX)
        presentAxis(sx, a.W, a.SW, ix0, ix1, ax);
    if (filterY)
        presentAxis(sy, a.H, a.SH, iy0, iy1, ay);
    f3 c = presentRow(a, filterX, ix0, ix1, ax, iy0);
    if (filterY)
    {
        const f3 bot = presentRow(a, filterX, ix0, ix1, ax, iy1);
        c = c * (1.0f - ay) + bot * ay;
    }
    return c;
}

// Screen pixel p = sy * SW + sx from `tone` on: c is ScreenImage's binary16-valued texel.  `tone` is what stands between the blit and
// the UI and returns a binary16-valued colour: ToneMap (pt_post.hpp) in k_present, the grade in k_present_graded (pt_grade.hpp).
template <uint32_t FORMAT, bool HDR, class Tone> PT_DEV void presentStore(const PresentArgs &a, const Tone &tone, uint32_t p, f3 c)
{
    c = tone(c);     // toneMapping.comp on ScreenImage, or the grade
    if (a.ui)        // uiComposition.comp:53-62
    {
        const uint32_t t = a.ui[p];
        if (t >> 24)
        {
            const f3 ui = F3(uiSrgbToLinear(div_((float)(t & 255u), 255.0f)), uiSrgbToLinear(div_((float)((t >> 8) & 255u), 255.0f)),
                             uiSrgbToLinear(div_((float)((t >> 16) & 255u), 255.0f)));
            c = ui * 0.99f + c * 0.01f;
        }
    }
    if (HDR)
        c = linearToHdr10(c, 203.0f);
    c = f16Round(c);
    if (FORMAT == PTX_PRESENT_R16G16B16A16_SFLOAT)
        static_cast<uint2 *>(a.out)[p] = make_uint2(f16Bits(c.x) | f16Bits(c.y) << 16, f16Bits(c.z) | 0x3c00u << 16);
    else if (FORMAT == PTX_PRESENT_A2B10G10R10_UNORM)
        static_cast<uint32_t *>(a.out)[p] = quantize10(c.x) | quantize10(c.y) << 10 | quantize10(c.z) << 20 | 3u << 30;
    else
    {
        const uint32_t r8 = quantize8(linearToSrgb(c.x)), g8 = quantize8(linearToSrgb(c.y)), b8 = quantize8(linearToSrgb(c.z));
        static_cast<uint32_t *>(a.out)[p] = FORMAT == PTX_PRESENT_B8G8R8A8_SRGB ? (b8 | g8 << 8 | r8 << 16 | 255u << 24) : (r8 | g8 << 8 | b8 << 16 | 255u << 24);
    }
}

// One screen pixel, from the blit to the store.  The two halves above are k_present_upscaled's too (pt_upscale.hpp), which puts its
// own enlargement where the blit stands; inlined here they assemble to the one function's instructions, a few of them in another
// order at the store (docs/NEXT_ROWS.md section 25 has the comparison).
template <uint32_t FORMAT, bool HDR, class Tone> PT_DEV void presentPixel(const PresentArgs &a, const Tone &tone)
{
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; // SW * SH <= 2^28
    if (p >= a.SW * a.SH)
        return;
    const f3 c = f16Round(presentBlit(a, p % a.SW, p / a.SW)); // ScreenImage after the blit
    presentStore<FORMAT, HDR>(a, tone, p, c);
}

template <uint32_t FORMAT, bool HDR> __global__ void __launch_bounds__(kPresentBlock) k_present(PresentArgs a)
{
    presentPixel<FORMAT, HDR>(a, ToneMap{ HDR ? PTX_TONE_MAPPING_HDR : PTX_TONE_MAPPING_SDR });
}

} // namespace ptd
