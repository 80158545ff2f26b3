// pt_bc.hpp -- block-compressed scene textures (docs/NEXT_ROWS.md section 15): BC1 / BC3 / BC5 blocks are uploaded as the file
// holds them and decoded on the device, in one pass, into the pool the render kernels sample.  The decoded values are the bits the
// RGBA8 route (host decode to RGBA8, k_decode_texels) gives for the same blocks; nothing behind the pool knows the difference.
// The block layout and the palette rules are the text of include/ptx.h (PtxTextureFormat).
#pragma once

#include "pt_device.hpp"

PT_DEV bool bcIsSrgb(uint32_t format) { return format == PTX_TEXTURE_BC1_SRGB || format == PTX_TEXTURE_BC3_SRGB; }

// One channel of a BC4 block (the alpha block of BC3, each half of BC5) at texel i = 4 * (y & 3) + (x & 3): two end points, 48 bits
// of 3-bit codes; eight values with a0 > a1, six values and 0 / 255 otherwise.  Integer arithmetic, floor division.
PT_DEV uint32_t bc4Value(uint32_t w0, uint32_t w1, uint32_t i)
{
    const uint32_t a0 = w0 & 255u, a1 = (w0 >> 8) & 255u;
    const uint64_t bits = (uint64_t)(w0 >> 16) | ((uint64_t)w1 << 16);
    const uint32_t c = (uint32_t)(bits >> (3u * i)) & 7u;
    if (c == 0u)
        return a0;
    if (c == 1u)
        return a1;
    if (a0 > a1)
        return ((8u - c) * a0 + (c - 1u) * a1) / 7u;
    if (c >= 6u)
        return c == 6u ? 0u : 255u;
    return ((6u - c) * a0 + (c - 1u) * a1) / 5u;
}

// The colour block of BC1 / BC3 at texel i, as R | G << 8 | B << 16 | A << 24: two RGB565 end points expanded by bit replication,
// 32 bits of 2-bit codes.  Four colours with c0 > c1 (always for BC3: punchThrough = false), three colours and transparent
// black otherwise.
PT_DEV uint32_t bc1Texel(uint32_t w0, uint32_t w1, uint32_t i, bool punchThrough)
{
    const uint32_t c0 = w0 & 0xffffu, c1 = w0 >> 16;
    const uint32_t code = (w1 >> (2u * i)) & 3u;
    const bool four = c0 > c1 || !punchThrough;
    uint32_t p0[3], p1[3];
    p0[0] = (c0 >> 11) & 31u; p0[1] = (c0 >> 5) & 63u; p0[2] = c0 & 31u;
    p1[0] = (c1 >> 11) & 31u; p1[1] = (c1 >> 5) & 63u; p1[2] = c1 & 31u;
    p0[0] = (p0[0] << 3) | (p0[0] >> 2); p0[1] = (p0[1] << 2) | (p0[1] >> 4); p0[2] = (p0[2] << 3) | (p0[2] >> 2);
    p1[0] = (p1[0] << 3) | (p1[0] >> 2); p1[1] = (p1[1] << 2) | (p1[1] >> 4); p1[2] = (p1[2] << 3) | (p1[2] >> 2);
    uint32_t out = 0xff000000u;
    if (code == 3u && !four)
        return 0u;
#pragma unroll
    for (uint32_t k = 0; k < 3u; k++)
    {
        uint32_t v;
        if (code == 0u)
            v = p0[k];
        else if (code == 1u)
            v = p1[k];
        else if (!four)
            v = (p0[k] + p1[k]) / 2u;
        else if (code == 2u)
            v = (2u * p0[k] + p1[k]) / 3u;
        else
            v = (p0[k] + 2u * p1[k]) / 3u;
        out |= v << (8u * k);
    }
    return out;
}

// Texel i of one block (two dwords for BC1, four for BC3 / BC5), as the RGBA8 word the host decoder would have produced.
template <uint32_t FORMAT> PT_DEV uint32_t bcTexel8(const uint32_t *w, uint32_t i)
{
    if (FORMAT == PTX_TEXTURE_BC1_UNORM || FORMAT == PTX_TEXTURE_BC1_SRGB)
        return bc1Texel(w[0], w[1], i, true);
    if (FORMAT == PTX_TEXTURE_BC3_SRGB)
        return (bc1Texel(w[2], w[3], i, false) & 0x00ffffffu) | bc4Value(w[0], w[1], i) << 24;
    return bc4Value(w[0], w[1], i) | bc4Value(w[2], w[3], i) << 8 | 0xff000000u; // BC5: R, G, B = 0, A = 1
}

// ... and that word as k_decode_texels takes it: the sRGB table for the colour channels of the _SRGB formats, c / 255 otherwise.
template <uint32_t FORMAT> PT_DEV float4 bcDecoded(uint32_t p, const float *__restrict__ srgbLut)
{
    float4 r;
    if (FORMAT == PTX_TEXTURE_BC1_SRGB || FORMAT == PTX_TEXTURE_BC3_SRGB)
    {
        r.x = srgbLut[p & 255u]; r.y = srgbLut[(p >> 8) & 255u]; r.z = srgbLut[(p >> 16) & 255u];
    }
    else
    {
        r.x = (float)(p & 255u) / 255.0f; r.y = (float)((p >> 8) & 255u) / 255.0f; r.z = (float)((p >> 16) & 255u) / 255.0f;
    }
    r.w = (float)(p >> 24) / 255.0f;
    return r;
}

// All levels of ONE texture in one launch.  A work item is a texel (ROWS = false: row-major within a level, a wave stores 1 KiB
// of contiguous float4 and the four lanes of a block row read the same 8 / 16 bytes) or the four texels of one row of one block
// (ROWS = true: row-major over (y, block column), four stores per thread).  The level of an item is found from the <= 16 chain
// offsets by compares against kernel arguments (no indexed array: nothing goes to scratch).  Texels of a partial block that fall
// outside the level are never stored.
struct BcDecodeArgs
{
    uint32_t width, height, levels; // of the image as it is kept: level 0 may be a later level of the file
    uint32_t items;                 // work items of all levels
    uint32_t itemFirst[16];         // first work item of level l; 0xffffffff from `levels` on
    uint32_t blockFirst[16];        // byte offset of level l's blocks behind `blocks`
    uint32_t decodedFirst[16];      // the renderTable's levelOffset[l]
};

template <uint32_t FORMAT, bool ROWS>
__global__ __launch_bounds__(256) void k_decode_bc(BcDecodeArgs a, const uint8_t *__restrict__ blocks, const float *__restrict__ srgbLut, float4 *__restrict__ decoded)
{
    constexpr uint32_t kBlockBytes = (FORMAT == PTX_TEXTURE_BC1_UNORM || FORMAT == PTX_TEXTURE_BC1_SRGB) ? 8u : 16u;
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= a.items)
        return;
    uint32_t level = 0, first = 0, blockFirst = a.blockFirst[0], out = a.decodedFirst[0];
#pragma unroll
    for (uint32_t l = 1; l < 16u; l++)
        if (k >= a.itemFirst[l])
        {
            level = l; first = a.itemFirst[l]; blockFirst = a.blockFirst[l]; out = a.decodedFirst[l];
        }
    const uint32_t w = levelDim(a.width, level), bw = (w + 3u) >> 2;
    const uint32_t j = k - first;
    const uint32_t perRow = ROWS ? bw : w;
    const uint32_t y = j / perRow, c = j - y * perRow; // c: texel column, or block column
    const uint32_t bx = ROWS ? c : c >> 2;
    const uint8_t *b = blocks + blockFirst + ((size_t)(y >> 2) * bw + bx) * kBlockBytes;
    uint32_t word[4];
    if (kBlockBytes == 8u)
    {
        const uint2 v = *reinterpret_cast<const uint2 *>(b);
        word[0] = v.x; word[1] = v.y; word[2] = word[3] = 0u;
    }
    else
    {
        const uint4 v = *reinterpret_cast<const uint4 *>(b);
        word[0] = v.x; word[1] = v.y; word[2] = v.z; word[3] = v.w;
    }
    if (ROWS)
    {
        float4 *row = decoded + out + (size_t)y * w + 4u * bx;
#pragma unroll
        for (uint32_t i = 0; i < 4u; i++)
            if (4u * bx + i < w)
                row[i] = bcDecoded<FORMAT>(bcTexel8<FORMAT>(word, 4u * (y & 3u) + i), srgbLut);
    }
    else
        decoded[out + (size_t)y * w + c] = bcDecoded<FORMAT>(bcTexel8<FORMAT>(word, 4u * (y & 3u) + (c & 3u)), srgbLut);
}
