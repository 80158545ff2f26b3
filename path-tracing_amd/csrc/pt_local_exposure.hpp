// pt_local_exposure.hpp -- local exposure between the meter and the output stage (docs/NEXT_ROWS.md section 23; semantics:
// include/ptx.h ptx_local_exposure, steps 1 - 7): a bilateral grid over the fixed-point log2 of the luminance gives every pixel the
// smooth base layer under it, and a gain G(p) that compresses the base's distance from a pivot; ptx_postprocess_local multiplies G
// into Exposure per pixel (k_postprocess_local, pt_post.hpp).  Three kernels, host side in pt_output_host.hpp:
//
//   k_local_splat   one workgroup of 256 threads per 64 x 64-pixel block, sixteen pixels a thread (a wave is 64 pixels of one row, so
//                   every load is 1 KB contiguous; the sixteen loads are issued before the first is used: out-of-image pixels load a
//                   clamped address and are predicated at the atomic).  The block's (64 >> s)^2 cells x 32 slices live in LDS as one
//                   64-bit word each, count in the high half and sum of l in the low half, filled with one 64-bit LDS integer
//                   atomic per counted pixel (a cell holds at most 4,096 pixels: the low half stays below 2^25 and never carries).
//                   64 is a multiple of every cell size, so a cell belongs to one workgroup, which writes all 32 slices of it,
//                   zeros included, with plain 8-byte vector stores: no global atomics, nothing to zero between calls.
//   k_local_blur    ONE launch for the three 1-2-1 passes.  Why not three: the arithmetic is integer, so the tensor product of the
//                   three clamped passes is the same number in any order, and at the sizes the stage runs at (60 x 34 x 32 cells at
//                   1080p, s = 5: 0.5 MB) a launch costs more than the pass it carries.  A thread owns one (cell, slice): it sums the
//                   3 x 3 neighbours of its slice with weights (1 2 1) x (1 2 1) (nine 8-byte loads, 32 consecutive slices per
//                   half-wave: 256 B rows), then takes the slices above and below from the neighbouring lanes of its half-wave
//                   (__shfl_up / __shfl_down of width 32 hand a lane its own value at the ends: the clamp to the edge).  No LDS, no
//                   intermediate grid.
//   k_local_gain    one thread per pixel on the chain's 32 x 8 tiles.  The cells the tile's taps can touch -- at most 6 x 3 at s = 3,
//                   2 x 2 at s = 6 -- x 32 slices are staged in LDS (4,608 B) by the whole workgroup, then eight taps, two 64-bit
//                   sums, one float64 division, one exp2 and a 4-byte store per pixel.
//
// LDS atomics: the lanes of a wave that meet on one address are the pixels of one row that share a cell and a slice: up to 2^s of
// them, all 64 at s = 6 on a constant image, the worst case measured in section 23.  Every intermediate of the blur fits 32 bits:
// 4096 x 8191 x 64 = 2,147,221,504.  -ffp-contract=off keeps the products and the division of step 5 and 6 operations of their own.
#pragma once

#include "pt_meter.hpp"

constexpr int kLocalSplatThreads = 256;
constexpr uint32_t kLocalBlockShift = 6;  // k_local_splat: a workgroup takes 64 x 64 pixels
constexpr uint32_t kLocalSlices = 32;     // one per octave of [2^-16, 2^16)
constexpr uint32_t kLocalMinShift = 3, kLocalMaxShift = 6;
constexpr uint32_t kLocalStageCellsX = 6, kLocalStageCellsY = 3; // k_local_gain: the cells a 32 x 8 tile's taps reach at kLocalMinShift
static_assert(kLocalMaxShift <= kLocalBlockShift, "a cell must not straddle two workgroups of k_local_splat");
static_assert(4096ull * 8191ull * 64ull < (1ull << 32), "the blurred sums are uint32");

// steps 1 and 2: l of a COUNTED pixel, -1 for a BLACK or REJECTED one
PT_DEV int localLog(float4 s, float rs)
{
    const float Y = luminance_(F3(s.x * rs, s.y * rs, s.z * rs));
    const uint32_t bits = __float_as_uint(Y), e = bits >> 23; // sign and exponent field
    if ((e & 0xffu) == 0xffu || e - 1u >= 254u)
        return -1; // NaN, +-Inf; the sign set, zero or a denormal
    const int l = (int)(bits >> 15) - 888 * 32;
    return l < 0 ? 0 : l > 8191 ? 8191 : l;
}

struct LocalSplatArgs
{
    const float4 *source;
    uint2 *grid; // [ny][nx][32]: x the sum of l, y the count
    uint32_t width, height, shift, nx, ny;
    float totalSamples; // (float)totalSamples
};

__global__ void __launch_bounds__(kLocalSplatThreads) k_local_splat(LocalSplatArgs a)
{
    __shared__ unsigned long long cell[(1u << (2u * (kLocalBlockShift - kLocalMinShift))) * kLocalSlices]; // 16 KB at s = 3
    const uint32_t t = threadIdx.x, s = a.shift;
    const uint32_t sideShift = kLocalBlockShift - s, words = kLocalSlices << (2u * sideShift); // cells along a side, as a shift
    for (uint32_t i = t; i < words; i += kLocalSplatThreads)
        cell[i] = 0ull;
    __syncthreads();
    const float rs = rcp_(a.totalSamples);
    const uint32_t lx = t & 63u, x = (blockIdx.x << kLocalBlockShift) + lx, xc = x < a.width ? x : a.width - 1u;
    constexpr uint32_t kRows = (1u << kLocalBlockShift) / (kLocalSplatThreads / 64u); // 16 rows a thread, four rows apart
    float4 v[kRows];
#pragma unroll
    for (uint32_t k = 0; k < kRows; k++)
    {
        const uint32_t y = (blockIdx.y << kLocalBlockShift) + (t >> 6) + 4u * k, yc = y < a.height ? y : a.height - 1u;
        v[k] = a.source[(size_t)yc * a.width + xc]; // always inside the image; a pixel outside it is dropped below
    }
#pragma unroll
    for (uint32_t k = 0; k < kRows; k++)
    {
        const uint32_t ly = (t >> 6) + 4u * k, y = (blockIdx.y << kLocalBlockShift) + ly;
        const int l = localLog(v[k], rs);
        if (l >= 0 && x < a.width && y < a.height)
            atomicAdd(&cell[(((ly >> s) << sideShift) + (lx >> s)) * kLocalSlices + ((uint32_t)l >> 8)], (1ull << 32) | (unsigned long long)l);
    }
    __syncthreads();
    for (uint32_t i = t; i < words; i += kLocalSplatThreads)
    {
        const uint32_t c = i >> 5, cx = (blockIdx.x << sideShift) + (c & ((1u << sideShift) - 1u)), cy = (blockIdx.y << sideShift) + (c >> sideShift);
        if (cx < a.nx && cy < a.ny)
        {
            const unsigned long long w = cell[i];
            a.grid[((size_t)cy * a.nx + cx) * kLocalSlices + (i & 31u)] = make_uint2((uint32_t)w, (uint32_t)(w >> 32));
        }
    }
}

// step 4.  entries = nx ny 32, a multiple of 32: a half-wave is the 32 slices of one cell, or wholly past the end
__global__ void __launch_bounds__(256) k_local_blur(const uint2 *__restrict__ in, uint2 *__restrict__ out, uint32_t nx, uint32_t ny)
{
    const size_t entries = (size_t)nx * ny * kLocalSlices, i = (size_t)blockIdx.x * 256u + threadIdx.x;
    const bool valid = i < entries;
    const size_t c = valid ? i >> 5 : 0u;
    const uint32_t z = (uint32_t)i & 31u, cy = (uint32_t)(c / nx), cx = (uint32_t)(c - (size_t)cy * nx);
    const uint32_t xs[3] = { cx ? cx - 1u : 0u, cx, cx + 1u < nx ? cx + 1u : nx - 1u };
    const uint32_t ys[3] = { cy ? cy - 1u : 0u, cy, cy + 1u < ny ? cy + 1u : ny - 1u };
    uint32_t sum = 0u, cnt = 0u;
#pragma unroll
    for (int j = 0; j < 3; j++)
#pragma unroll
        for (int k = 0; k < 3; k++)
        {
            const uint2 e = in[((size_t)ys[j] * nx + xs[k]) * kLocalSlices + z];
            const uint32_t w = (j == 1 ? 2u : 1u) * (k == 1 ? 2u : 1u);
            sum += w * e.x;
            cnt += w * e.y;
        }
    // along z: lane z - 1 and lane z + 1 of the half-wave; at slice 0 and 31 the shuffles return the lane's own value
    const uint32_t sumBelow = __shfl_up(sum, 1, 32), sumAbove = __shfl_down(sum, 1, 32);
    const uint32_t cntBelow = __shfl_up(cnt, 1, 32), cntAbove = __shfl_down(cnt, 1, 32);
    if (valid)
        out[i] = make_uint2(sumBelow + 2u * sum + sumAbove, cntBelow + 2u * cnt + cntAbove);
}

struct LocalGainArgs
{
    const float4 *source;
    const uint2 *grid;      // the blurred grid
    float *gain;            // G
    const double *meterCur; // PTX_LOCAL_EXPOSURE_PIVOT_METERED: the meter state's cur; otherwise null
    uint32_t width, height, shift, nx, ny;
    float totalSamples, pivotLog2, highlightContrast, shadowContrast, maxStops;
};

// step 5, one axis: the two taps' cells and the second tap's weight of a coordinate given as 2 p + 1 (a pixel, or l) and the cell's
// size 2^s (or 256): u = 2 p + 1 - 2^s, unsigned throughout (2 p + 1 fits 32 bits: p < 2^31)
PT_DEV void localTaps(uint32_t twicePlusOne, uint32_t shift, uint32_t last, uint32_t &c0, uint32_t &c1, uint32_t &f)
{
    if (twicePlusOne < (1u << shift)) // u < 0
    {
        c0 = c1 = 0u;
        f = 0u;
        return;
    }
    const uint32_t u = twicePlusOne - (1u << shift);
    c0 = u >> (shift + 1u);
    f = u & ((2u << shift) - 1u);
    c1 = c0 + 1u < last ? c0 + 1u : last;
}

__global__ void __launch_bounds__(kDenoiseTileX *kDenoiseTileY) k_local_gain(LocalGainArgs a)
{
    __shared__ uint2 stage[kLocalStageCellsX * kLocalStageCellsY * kLocalSlices];
    const uint32_t s = a.shift, t = threadIdx.y * kDenoiseTileX + threadIdx.x;
    const uint32_t x0 = blockIdx.x * kDenoiseTileX, y0 = blockIdx.y * kDenoiseTileY;
    const uint32_t xl = x0 + kDenoiseTileX - 1u < a.width ? x0 + kDenoiseTileX - 1u : a.width - 1u;
    const uint32_t yl = y0 + kDenoiseTileY - 1u < a.height ? y0 + kDenoiseTileY - 1u : a.height - 1u;
    // the cells between the first tap of the tile's first pixel and the second tap of its last one, along x and y
    uint32_t cxa, cxb, cya, cyb, unused0, unused1;
    localTaps(2u * x0 + 1u, s, a.nx - 1u, cxa, unused0, unused1);
    localTaps(2u * xl + 1u, s, a.nx - 1u, unused0, cxb, unused1);
    localTaps(2u * y0 + 1u, s, a.ny - 1u, cya, unused0, unused1);
    localTaps(2u * yl + 1u, s, a.ny - 1u, unused0, cyb, unused1);
    uint32_t ncx = cxb - cxa + 1u, ncy = cyb - cya + 1u;
    ncx = ncx < kLocalStageCellsX ? ncx : kLocalStageCellsX; // they are: s >= kLocalMinShift.  The clamp keeps `stage` in bounds whatever s is
    ncy = ncy < kLocalStageCellsY ? ncy : kLocalStageCellsY;
    for (uint32_t i = t; i < ncx * ncy * kLocalSlices; i += kDenoiseTileX * kDenoiseTileY)
    {
        const uint32_t c = i >> 5, ly = c / ncx, lx = c - ly * ncx;
        stage[i] = a.grid[((size_t)(cya + ly) * a.nx + (cxa + lx)) * kLocalSlices + (i & 31u)];
    }
    __syncthreads(); // every thread of the workgroup gets here
    const uint32_t x = x0 + threadIdx.x, y = y0 + threadIdx.y;
    if (x >= a.width || y >= a.height)
        return;
    const size_t p = (size_t)y * a.width + x;
    const int l = localLog(a.source[p], rcp_(a.totalSamples));
    float G = 1.0f;
    if (l >= 0)
    {
        uint32_t cx[2], cy[2], cz[2], fx, fy, fz;
        localTaps(2u * x + 1u, s, a.nx - 1u, cx[0], cx[1], fx);
        localTaps(2u * y + 1u, s, a.ny - 1u, cy[0], cy[1], fy);
        localTaps(2u * (uint32_t)l + 1u, 8u, kLocalSlices - 1u, cz[0], cz[1], fz);
        const uint32_t wx[2] = { (2u << s) - fx, fx }, wy[2] = { (2u << s) - fy, fy }, wz[2] = { 512u - fz, fz };
        uint64_t N = 0ull, D = 0ull;
#pragma unroll
        for (int j = 0; j < 2; j++)
#pragma unroll
            for (int i = 0; i < 2; i++)
            {
                uint32_t lx = cx[i] - cxa, ly = cy[j] - cya;
                lx = lx < ncx ? lx : ncx - 1u; // never taken (the staged range covers every tap of the tile): bounds only
                ly = ly < ncy ? ly : ncy - 1u;
                const uint2 *col = stage + (ly * ncx + lx) * kLocalSlices;
#pragma unroll
                for (int k = 0; k < 2; k++)
                {
                    const uint2 e = col[cz[k]];
                    const uint64_t w = (uint64_t)(wx[i] * wy[j] * wz[k]); // at most 2^7 2^7 2^9
                    N += w * e.x;
                    D += w * e.y;
                }
            }
        const double B = (double)N / (double)D / 256.0 - 16.0;
        // step 6
        double pv = (double)a.pivotLog2;
        if (a.meterCur)
            pv = pv - *a.meterCur;
        const double d = B - pv;
        const double c = d > 0.0 ? (double)a.highlightContrast : (double)a.shadowContrast;
        const double g = meterClamp(meterClamp((c - 1.0) * d, -(double)a.maxStops, (double)a.maxStops), -300.0, 300.0);
        G = (float)exp2_(g);
    }
    a.gain[p] = G;
}
