// pt_adaptive.hpp -- adaptive sampling of an offline render (docs/NEXT_ROWS.md section 27; semantics: include/ptx.h ptx_adaptive_plan,
// steps 1 - 3, and ptx_noise_meter_adaptive): the tile records of the noise meter, or a mask of the host's, become the sorted list of
// tiles the next render calls cover (slotPixel, pt_wavefront.hpp, reads it), and per tile and half the frames rendered so far are
// counted.  Host side in pt_output_host.hpp, state: OutputState::AdaptiveState.
//
//   k_adaptive_plan            ONE workgroup of 1,024 threads, integers only, four phases with a barrier between them:
//                              commit (the counts of the tiles active in the plan being replaced grow by the frames rendered under it)
//                              and seed (a flag per tile from the record or the mask), thread i taking tiles i, i + 1024, ...;
//                              dilate (a tile is active iff a seed lies within `dilate` tiles of it: at most 25 byte loads);
//                              compact: a blocked scan -- thread i owns the tiles [i per, (i + 1) per), per = ceil(numTiles / 1024),
//                              counts its active ones, the counts are scanned by wave shuffles and across the 16 waves through LDS,
//                              and the thread writes its tiles' ids from its offset on.  The list is ascending because the blocks
//                              are, whatever order the waves run in: no global atomic.  A 4K frame with 8-pixel tiles has 129,600
//                              tiles, 127 per thread.
//   k_noise_tiles_adaptive<W>  k_noise_tiles' body (pt_noise.hpp, noiseTilesBody) with the scale factors and the normalisation
//                              factor of step 1 taken per tile from LDS, where the first 64 threads put them.
//
// LDS: 192 B in k_adaptive_plan; k_noise_tiles_adaptive: k_noise_tiles' 784 B + 1,280 B.  All device memory is written with the
// compiler's ordinary vector stores.
#pragma once

#include "pt_noise.hpp"

constexpr int kAdaptiveBlock = 1024;
constexpr uint32_t kAdaptiveWaves = kAdaptiveBlock / 64;

struct AdaptiveArgs
{
    uint32_t *countA, *countB;  // frames per tile in half 0 / half 1
    uint8_t *active;            // per tile: in the plan in force (read by the commit, then rewritten)
    uint8_t *seed;              // per tile: scratch of this call
    const NoiseTile *records;   // PTX_ADAPTIVE_FROM_NOISE: the last meter's tile records, else null
    const uint8_t *mask;        // PTX_ADAPTIVE_FROM_MASK: the device copy of the host's mask, else null
    uint32_t *list;             // the active tile ids, ascending
    PtxAdaptivePlan *plan;
    uint32_t width, height, tileShift, tilesX, tilesY;
    uint32_t hadPlan, framesA, framesB, dilate, generation;
};

// the in-image pixels of tile i
PT_DEV uint32_t adaptiveTilePixels(const AdaptiveArgs &a, uint32_t i)
{
    const uint32_t side = 1u << a.tileShift, x0 = (i % a.tilesX) << a.tileShift, y0 = (i / a.tilesX) << a.tileShift;
    const uint32_t w = a.width - x0 < side ? a.width - x0 : side, h = a.height - y0 < side ? a.height - y0 : side;
    return w * h;
}

__global__ void __launch_bounds__(kAdaptiveBlock) k_adaptive_plan(AdaptiveArgs a)
{
    __shared__ uint32_t waveTiles[kAdaptiveWaves], wavePixels[kAdaptiveWaves], waveSeeds[kAdaptiveWaves];
    const uint32_t t = threadIdx.x, n = a.tilesX * a.tilesY;
    // 1. commit, and the seeds of 2.
    for (uint32_t i = t; i < n; i += kAdaptiveBlock)
    {
        if (!a.hadPlan || a.active[i])
        {
            a.countA[i] += a.framesA;
            a.countB[i] += a.framesB;
        }
        a.seed[i] = a.records ? (a.records[i].converged ? 0 : 1) : (a.mask[i] ? 1 : 0);
    }
    __syncthreads();
    // 2. dilate
    const uint32_t d = a.dilate;
    for (uint32_t i = t; i < n; i += kAdaptiveBlock)
    {
        const uint32_t tx = i % a.tilesX, ty = i / a.tilesX;
        const uint32_t x0 = tx > d ? tx - d : 0u, x1 = tx + d < a.tilesX ? tx + d : a.tilesX - 1u;
        const uint32_t y0 = ty > d ? ty - d : 0u, y1 = ty + d < a.tilesY ? ty + d : a.tilesY - 1u;
        uint32_t any = 0u;
        for (uint32_t y = y0; y <= y1; y++)
            for (uint32_t x = x0; x <= x1; x++)
                any |= a.seed[y * a.tilesX + x];
        a.active[i] = any ? 1 : 0;
    }
    __syncthreads();
    // 3. compact
    const uint32_t per = (n + kAdaptiveBlock - 1u) / kAdaptiveBlock;
    const uint32_t first = t * per < n ? t * per : n, last = first + per < n ? first + per : n;
    uint32_t tiles = 0u, pixels = 0u, seeds = 0u;
    for (uint32_t i = first; i < last; i++)
    {
        seeds += a.seed[i];
        if (a.active[i])
        {
            tiles++;
            pixels += adaptiveTilePixels(a, i);
        }
    }
    uint32_t scan = tiles; // inclusive over the wave
    const uint32_t lane = t & 63u, wave = t >> 6;
#pragma unroll
    for (int s = 1; s < 64; s <<= 1)
    {
        const uint32_t o = __shfl_up(scan, s, 64);
        scan += lane >= (uint32_t)s ? o : 0u;
    }
#pragma unroll
    for (int s = 32; s > 0; s >>= 1)
    {
        pixels += __shfl_down(pixels, s, 64);
        seeds += __shfl_down(seeds, s, 64);
    }
    if (lane == 63u)
        waveTiles[wave] = scan;
    if (lane == 0u)
    {
        wavePixels[wave] = pixels;
        waveSeeds[wave] = seeds;
    }
    __syncthreads();
    uint32_t at = scan - tiles;
    for (uint32_t w = 0u; w < wave; w++)
        at += waveTiles[w];
    for (uint32_t i = first; i < last; i++)
        if (a.active[i])
            a.list[at++] = i;
    if (t != 0u)
        return;
    PtxAdaptivePlan out;
    out.tilesX = a.tilesX;
    out.tilesY = a.tilesY;
    out.activeTiles = out.activePixels = out.seedTiles = 0u;
    for (uint32_t w = 0u; w < kAdaptiveWaves; w++)
    {
        out.activeTiles += waveTiles[w];
        out.activePixels += wavePixels[w];
        out.seedTiles += waveSeeds[w];
    }
    out.generation = a.generation;
    *a.plan = out;
}

// ptx_noise_meter_adaptive: what k_noise_tiles gets, and the counts
struct AdaptiveNoiseArgs
{
    NoiseArgs noise;               // sa, sb and st are unused: they are per tile
    const uint32_t *countA, *countB;
    const uint8_t *active;         // null: no plan in force, every tile is active
    uint32_t pendingA, pendingB, normalizeTo;
    float exposure;
};

template <bool WRITE_SUM>
__global__ void __launch_bounds__(kNoiseBlock) k_noise_tiles_adaptive(AdaptiveNoiseArgs a)
{
    __shared__ NoiseTileScale scale[64];
    const uint32_t t = threadIdx.x, s = a.noise.tileShift, perSide = kNoiseBlockSide >> s;
    if (t < 64u)
    {
        NoiseTileScale v;
        v.sa = v.sb = v.st = 0.0f;
        v.k = 1.0f;
        v.flags = 1u; // an unsampled half: every pixel rejected
        const uint32_t tx = blockIdx.x * perSide + (t & (perSide - 1u)), ty = blockIdx.y * perSide + (t >> (kNoiseBlockShift - s));
        if (t < perSide * perSide && tx < a.noise.tilesX && ty < a.noise.tilesY)
        {
            const size_t at = (size_t)ty * a.noise.tilesX + tx;
            const bool on = !a.active || a.active[at];
            const uint32_t nA = a.countA[at] + (on ? a.pendingA : 0u), nB = a.countB[at] + (on ? a.pendingB : 0u), n = nA + nB;
            if (nA && nB)
            {
                v.sa = a.exposure * rcp_((float)nA);
                v.sb = a.exposure * rcp_((float)nB);
                v.st = a.exposure * rcp_((float)n);
                v.flags = 0u;
            }
            if (n != a.normalizeTo && n != 0u)
            {
                v.k = (float)a.normalizeTo * rcp_((float)n);
                v.flags |= 2u;
            }
        }
        scale[t] = v;
    }
    noiseTilesBody<WRITE_SUM, true>(a.noise, scale);
}
