// pt_upscale.hpp -- the enlarging screen path on the device (docs/NEXT_ROWS.md section 25; semantics: include/ptx.h
// ptx_present_upscaled, steps 1 - 6): a separable Catmull-Rom enlargement of the composed frame with a per-axis anti-ringing clamp,
// a clamped unsharp mask at the screen extent, then the screen path's own tail (presentStore of pt_present.hpp).
//
//   k_present_upscaled<FORMAT, HDR, SHARPEN, ToneArgs>   one launch; a workgroup of 256 threads owns a 32 x 8 tile of screen pixels
//                                                        and, when SHARPEN, its one-pixel halo (clamped to the screen's edge)
//
//   stage 1  the source footprint of tile plus halo is composed once per texel (presentTexel) into LDS.  Its origin and end are the
//            first tap of the first column (row) and the last tap of the last one, from the same float expression as the per-pixel
//            taps (upscaleAxis), which is monotone in the screen coordinate: every tap of every pixel of the tile lies between them.
//            The taps are clamped to the image before the origin is subtracted, so the edge clamp is applied by staging.
//   stage 2  the row pass, once per (source row, screen column), into LDS as float32 (R is not rounded)
//   stage 3  the column pass per screen pixel, halo included, f16Round: S.  With SHARPEN it goes into LDS over the texels, which are
//            dead by then; without, it stays in the thread's registers
//   stage 4  the unsharp mask on S and its four neighbours, then presentStore: tone or grade, UI, HDR10, store
//
// Footprint.  A tile with its halo spans 34 screen columns; W / SW < 1 on a filtered axis, so the first and the last differ by less
// than 33 in source coordinates (33 * 16383 / 16384 plus 2^-10 of rounding at the largest extent), their floors by at most 33, and
// with one tap before and two behind the footprint is at most 37 texels wide and 13 high; 38 x 14 are reserved.  An axis that is not
// filtered needs the 34 (10) texels themselves.  The loops run over the footprint's own extent, cut to the reserved one.
//
// LDS (SHARPEN / not): texels 14 x 38 x 3 floats = 6,384 B / 12 x 36 x 3 = 5,184 B, rows 14 x 34 x 3 = 5,712 B / 12 x 32 x 3 = 4,608 B:
// 12,096 B / 9,792 B a workgroup, under the 20 KB at which eight workgroups share a compute unit's 160 KB.  The texels are kept as
// float32 and not as 3 x 16 bits: the 3 KB saved would not raise the occupancy, and every tap would pay a conversion.  Three floats
// per texel put neighbouring texels three banks apart, which 64 banks serve without a conflict; two screen columns that share a tap
// read one address.  No scratch.
#pragma once

#include "pt_grade.hpp"

namespace ptd
{

constexpr uint32_t kUpscaleTileX = 32, kUpscaleTileY = 8, kUpscaleBlock = kUpscaleTileX * kUpscaleTileY;

// step 2: the four taps and weights of screen coordinate s on a filtered axis
PT_DEV void upscaleAxis(uint32_t s, uint32_t srcExtent, uint32_t dstExtent, uint32_t (&i)[4], float (&w)[4])
{
    const float x = ((float)s + 0.5f) * div_((float)srcExtent, (float)dstExtent) - 0.5f;
    const float x0 = __builtin_floorf(x), m = (float)(srcExtent - 1), t = x - x0;
    i[0] = (uint32_t)clamp_(x0 + -1.0f, 0.0f, m);
    i[1] = (uint32_t)clamp_(x0 + 0.0f, 0.0f, m);
    i[2] = (uint32_t)clamp_(x0 + 1.0f, 0.0f, m);
    i[3] = (uint32_t)clamp_(x0 + 2.0f, 0.0f, m);
    w[0] = ((-0.5f * t + 1.0f) * t - 0.5f) * t;
    w[1] = ((1.5f * t - 2.5f) * t) * t + 1.0f;
    w[2] = ((-1.5f * t + 2.0f) * t + 0.5f) * t;
    w[3] = ((0.5f * t - 0.5f) * t) * t;
}

// steps 3 and 4: the weighted sum in its written order, clamped between the two central taps; a NaN becomes the lower one
PT_DEV float upscaleTaps(float a, float b, float c, float d, const float (&w)[4])
{
    float v = ((a * w[0] + b * w[1]) + c * w[2]) + d * w[3];
    const float lo = c < b ? c : b, hi = b < c ? c : b;
    v = v >= lo ? v : lo;
    return v <= hi ? v : hi;
}

// step 5 on one channel: c is S at the pixel, n, s, w, e S at its neighbours
PT_DEV float upscaleSharpen(float c, float n, float s, float w, float e, float sharpness)
{
    if (!(abs_(c) <= 3.402823466e38f))
        return c;
    const float m = ((n + s) + (w + e)) * 0.25f;
    float v = c + (c - m) * sharpness;
    float lo = c, hi = c;
    lo = n < lo ? n : lo; hi = hi < n ? n : hi;
    lo = s < lo ? s : lo; hi = hi < s ? s : hi;
    lo = w < lo ? w : lo; hi = hi < w ? w : hi;
    lo = e < lo ? e : lo; hi = hi < e ? e : hi;
    v = v >= lo ? v : lo;
    v = v <= hi ? v : hi;
    return f16Round(v);
}

// what stands between S and the UI, from the kernel's last argument: ToneMap itself, or the grade's arguments
PT_DEV ToneMap upscaleTone(const ToneMap &t) { return t; }
PT_DEV Grade upscaleTone(const GradeArgs &g) { return Grade{ g }; }

template <uint32_t FORMAT, bool HDR, bool SHARPEN, class ToneArgs>
__global__ void __launch_bounds__(kUpscaleBlock) k_present_upscaled(PresentArgs a, float sharpness, ToneArgs toneArgs)
{
    constexpr uint32_t HALO = SHARPEN ? 1u : 0u;
    constexpr uint32_t COLS = kUpscaleTileX + 2u * HALO, ROWS = kUpscaleTileY + 2u * HALO; // screen pixels a workgroup computes S for
    constexpr uint32_t SRCX = COLS + 4u, SRCY = ROWS + 4u;                                 // the reserved source footprint
    static_assert(COLS * ROWS <= SRCX * SRCY, "S lies over the texels");
    __shared__ float texel[SRCY * SRCX * 3u]; // stage 1; stage 3 writes S over it, COLS to a row
    __shared__ float rowPass[SRCY * COLS * 3u];

    const uint32_t tid = threadIdx.x;
    const uint32_t tileX = blockIdx.x * kUpscaleTileX, tileY = blockIdx.y * kUpscaleTileY; // inside the screen: the grid is ceil(SW / 32) x ceil(SH / 8)
    const bool filterX = a.SW != a.W, filterY = a.SH != a.H;
    // the screen columns and rows S is needed at, the halo clamped to the screen's edge
    const uint32_t col0 = tileX ? tileX - HALO : 0u, row0 = tileY ? tileY - HALO : 0u;
    const uint32_t colEnd = tileX + kUpscaleTileX - 1u + HALO, rowEnd = tileY + kUpscaleTileY - 1u + HALO;
    const uint32_t col1 = colEnd < a.SW ? colEnd : a.SW - 1u, row1 = rowEnd < a.SH ? rowEnd : a.SH - 1u;
    const uint32_t ncols = col1 - col0 + 1u, nrows = row1 - row0 + 1u; // <= COLS, ROWS
    // the source footprint [ox, ex] x [oy, ey]
    uint32_t ox = col0, ex = col1, oy = row0, ey = row1;
    {
        uint32_t i[4];
        float w[4];
        if (filterX)
        {
            upscaleAxis(col0, a.W, a.SW, i, w);
            ox = i[0];
            upscaleAxis(col1, a.W, a.SW, i, w);
            ex = i[3];
        }
        if (filterY)
        {
            upscaleAxis(row0, a.H, a.SH, i, w);
            oy = i[0];
            upscaleAxis(row1, a.H, a.SH, i, w);
            ey = i[3];
        }
    }
    const uint32_t fw = ex - ox + 1u < SRCX ? ex - ox + 1u : SRCX, fh = ey - oy + 1u < SRCY ? ey - oy + 1u : SRCY;

    // stage 1: ox + lx <= ex <= W - 1 and oy + ly <= ey <= H - 1
    for (uint32_t k = tid; k < fw * fh; k += kUpscaleBlock)
    {
        const uint32_t ly = k / fw, lx = k - ly * fw;
        const f3 c = presentTexel(a, ox + lx, oy + ly);
        float *t = &texel[(ly * SRCX + lx) * 3u];
        t[0] = c.x; t[1] = c.y; t[2] = c.z;
    }
    __syncthreads();

    // stage 2: R at (source row ly, screen column col0 + cx); an unfiltered x has ox = col0 and the texel itself
    for (uint32_t k = tid; k < fh * ncols; k += kUpscaleBlock)
    {
        const uint32_t ly = k / ncols, cx = k - ly * ncols;
        const float *row = &texel[ly * SRCX * 3u];
        float *out = &rowPass[(ly * COLS + cx) * 3u];
        if (filterX)
        {
            uint32_t i[4];
            float w[4];
            upscaleAxis(col0 + cx, a.W, a.SW, i, w);
            const float *t0 = &row[(i[0] - ox) * 3u], *t1 = &row[(i[1] - ox) * 3u], *t2 = &row[(i[2] - ox) * 3u], *t3 = &row[(i[3] - ox) * 3u];
            out[0] = upscaleTaps(t0[0], t1[0], t2[0], t3[0], w);
            out[1] = upscaleTaps(t0[1], t1[1], t2[1], t3[1], w);
            out[2] = upscaleTaps(t0[2], t1[2], t2[2], t3[2], w);
        }
        else
        {
            const float *t = &row[cx * 3u];
            out[0] = t[0]; out[1] = t[1]; out[2] = t[2];
        }
    }
    __syncthreads();

    // stage 3: S at (col0 + cx, row0 + cy); an unfiltered y has oy = row0 and R itself
    const auto columnPass = [&](uint32_t cx, uint32_t cy) {
        if (filterY)
        {
            uint32_t j[4];
            float w[4];
            upscaleAxis(row0 + cy, a.H, a.SH, j, w);
            const float *r0 = &rowPass[((j[0] - oy) * COLS + cx) * 3u], *r1 = &rowPass[((j[1] - oy) * COLS + cx) * 3u];
            const float *r2 = &rowPass[((j[2] - oy) * COLS + cx) * 3u], *r3 = &rowPass[((j[3] - oy) * COLS + cx) * 3u];
            return f16Round(F3(upscaleTaps(r0[0], r1[0], r2[0], r3[0], w), upscaleTaps(r0[1], r1[1], r2[1], r3[1], w), upscaleTaps(r0[2], r1[2], r2[2], r3[2], w)));
        }
        const float *r = &rowPass[(cy * COLS + cx) * 3u];
        return f16Round(F3(r[0], r[1], r[2]));
    };
    const uint32_t tx = tid % kUpscaleTileX, ty = tid / kUpscaleTileX;
    const uint32_t sx = tileX + tx, sy = tileY + ty;
    const bool inside = sx < a.SW && sy < a.SH;
    f3 c = F3(0.0f, 0.0f, 0.0f);
    if (SHARPEN)
    {
        float *S = texel; // every read of the texels lies before the barrier above
        for (uint32_t k = tid; k < nrows * ncols; k += kUpscaleBlock)
        {
            const uint32_t cy = k / ncols, cx = k - cy * ncols;
            const f3 s = columnPass(cx, cy);
            float *o = &S[(cy * COLS + cx) * 3u];
            o[0] = s.x; o[1] = s.y; o[2] = s.z;
        }
        __syncthreads();
        // stage 4: the neighbours, clamped to the screen's edge, lie in [col0, col1] x [row0, row1]
        if (inside)
        {
            const uint32_t x = sx - col0, y = sy - row0;
            const uint32_t xw = (sx ? sx - 1u : 0u) - col0, xe = (sx + 1u < a.SW ? sx + 1u : sx) - col0;
            const uint32_t yn = (sy ? sy - 1u : 0u) - row0, ys = (sy + 1u < a.SH ? sy + 1u : sy) - row0;
            const float *pc = &S[(y * COLS + x) * 3u], *pn = &S[(yn * COLS + x) * 3u], *ps = &S[(ys * COLS + x) * 3u];
            const float *pw = &S[(y * COLS + xw) * 3u], *pe = &S[(y * COLS + xe) * 3u];
            c = F3(upscaleSharpen(pc[0], pn[0], ps[0], pw[0], pe[0], sharpness), upscaleSharpen(pc[1], pn[1], ps[1], pw[1], pe[1], sharpness),
                   upscaleSharpen(pc[2], pn[2], ps[2], pw[2], pe[2], sharpness));
        }
    }
    else if (inside)
        c = columnPass(tx, ty); // col0 = tileX, row0 = tileY
    if (inside)
        presentStore<FORMAT, HDR>(a, upscaleTone(toneArgs), sy * a.SW + sx, c);
}

} // namespace ptd
