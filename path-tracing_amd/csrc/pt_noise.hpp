// pt_noise.hpp -- noise metering of an offline render (docs/NEXT_ROWS.md section 26; semantics: include/ptx.h ptx_noise_meter, steps
// 1 - 7): the two half-sums a host accumulates by alternating ptx_bind_accumulation give a per-tile error estimate in the units of the
// displayed mean, and with it a stopping condition.  Two kernels, host side in pt_output_host.hpp:
//
//   k_noise_tiles<WRITE_SUM>  one workgroup of 256 threads owns one 64 x 64 block of pixels, which is 1 ... 64 whole tiles whatever
//                             tileShift is.  Wave w takes rows 4 i + w, i = 0 ... 15: lane c reads pixel c of the row from both halves,
//                             so every wave-load is one contiguous 1 KB row segment, and four rows' loads are issued before the first
//                             is used.  A thread adds its q and its counted flag in registers while its rows stay in one tile row
//                             (2^tileShift / 4 iterations; at most 16 x 2^24 = 2^28: 32 bits) and then adds them to Q_t and n_t in LDS
//                             with integer atomics; the three class counters go to LDS once per thread.  The first 64 threads then
//                             do step 6 for a tile each and store E_t and the record (Q_t, n_t, converged) with plain stores: every
//                             tile has exactly one writer.  The same wave sums Q_t and the converged flags and takes the maximum of
//                             E_t over the block's tiles with wave shuffles and stores one record of eight words per workgroup: no
//                             global atomic, nothing to zero between calls, no slab.
//   k_noise_resolve           one workgroup of 1,024 threads sums the per-workgroup records (four in flight per thread: a 4K frame has
//                             2,040 of them, so two rounds), reduces per wave by shuffles and across waves by LDS atomics, does the
//                             float64 division of step 7 and writes the result.  It reads no tile record: the per-workgroup records
//                             carry the block's Q, converged count and maximum already, which is 64 KB at 4K where the tile records of
//                             8-pixel tiles are 2.6 MB -- too much for one workgroup to stream.
//
// LDS: 784 B in k_noise_tiles, 32 B in the resolve.  All device memory is written with the compiler's ordinary vector stores.
// -ffp-contract=off keeps every product and sum of steps 2 - 5 an operation of its own; the double divisions are the compiler's IEEE
// sequence (v_div_scale_f64, v_rcp_f64, v_fma_f64 ..., v_div_fmas_f64, v_div_fixup_f64).
#pragma once

#include "pt_meter.hpp"

constexpr int kNoiseBlock = 256;
constexpr uint32_t kNoiseBlockShift = 6u; // a workgroup's block of pixels is 64 x 64
constexpr uint32_t kNoiseBlockSide = 1u << kNoiseBlockShift;
constexpr uint32_t kNoiseRowsPerPass = kNoiseBlock / kNoiseBlockSide; // 4: one row per wave
constexpr uint32_t kNoiseBatch = 4u;                                   // passes whose loads are in flight together
constexpr uint32_t kNoiseRecordWords = 8u; // Q low, Q high, counted, black, rejected, converged, bits of max E_t, 0
constexpr int kNoiseResolveBlock = 1024;
static_assert(kNoiseBlockSide == 64u && kNoiseRowsPerPass == 4u, "a wave reads one 64-pixel row segment");
static_assert(kNoiseBlockSide % (kNoiseRowsPerPass * kNoiseBatch) == 0u, "whole batches");

// one tile: what steps 6 and 7 sum, and the flag; E_t lies beside it in the tile map ptx_read_noise copies out
struct NoiseTile
{
    unsigned long long Q;
    uint32_t n, converged;
};
static_assert(sizeof(NoiseTile) == 16, "NoiseTile layout");

struct NoiseArgs
{
    const float4 *halfA, *halfB;
    float4 *sum;        // the internal accumulation image (PTX_NOISE_WRITE_SUM), or unused
    NoiseTile *tiles;   // tilesX x tilesY
    float *tileErrors;  // tilesX x tilesY
    uint32_t *records;  // gridDim.x x gridDim.y x kNoiseRecordWords
    uint32_t width, height, tileShift, tilesX, tilesY;
    float sa, sb, st, threshold; // step 2, formed on the host with the same rcp
};

PT_DEV bool noiseFinite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// What ptx_noise_meter_adaptive knows per tile (pt_adaptive.hpp): step 2 from the tile's own counts, the factor step 1 stores S with,
// and flags: 1 a half without a sample (every pixel rejected, the tile not converged), 2 S is stored as S * k
struct NoiseTileScale
{
    float sa, sb, st, k;
    uint32_t flags;
};

// steps 3 - 5 for one pixel: 0 counted, 1 black, 2 rejected; q is 0 unless counted and not black
PT_DEV uint32_t noisePixel(const float4 &A, const float4 &B, const float4 &S, float sa, float sb, float st, uint32_t &q)
{
    const float ar = A.x * sa, ag = A.y * sa, ab = A.z * sa;
    const float br = B.x * sb, bg = B.y * sb, bb = B.z * sb;
    const float cr = S.x * st, cg = S.y * st, cb = S.z * st;
    const float D = (abs_(ar - br) + abs_(ag - bg)) + abs_(ab - bb);
    const float m = (cr + cg) + cb;
    q = 0u;
    if (!(noiseFinite(A.x) && noiseFinite(A.y) && noiseFinite(A.z) && noiseFinite(B.x) && noiseFinite(B.y) && noiseFinite(B.z) && noiseFinite(D) && noiseFinite(m)))
        return 2u;
    if (!(m >= 9.5367431640625e-07f)) // 2^-20
        return 1u;
    const float e = fmin_(0.5f * div_(D, sqrt_(m)), 255.0f);
    q = (uint32_t)(e * 65536.0f);
    return 0u;
}

// The body of k_noise_tiles and, with ADAPTIVE, of k_noise_tiles_adaptive (pt_adaptive.hpp), which has filled `scale` for the
// block's tiles before it calls this: the barrier below orders those stores too.
template <bool WRITE_SUM, bool ADAPTIVE>
PT_DEV void noiseTilesBody(const NoiseArgs &a, const NoiseTileScale *scale)
{
    __shared__ unsigned long long tileQ[64];
    __shared__ uint32_t tileN[64];
    __shared__ uint32_t classes[3]; // counted, black, rejected
    const uint32_t t = threadIdx.x, c = t & (kNoiseBlockSide - 1u), w = t >> kNoiseBlockShift;
    if (t < 64u)
    {
        tileQ[t] = 0ull;
        tileN[t] = 0u;
    }
    if (t < 3u)
        classes[t] = 0u;
    __syncthreads();
    const uint32_t s = a.tileShift, perSide = kNoiseBlockSide >> s; // tiles along a side of the block: 8, 4, 2, 1
    const uint32_t x = blockIdx.x * kNoiseBlockSide + c, y0 = blockIdx.y * kNoiseBlockSide + w;
    const bool inX = x < a.width;
    const uint32_t xc = inX ? x : a.width - 1u; // a lane outside the image loads the row's last pixel and drops it: no load behind a branch
    const uint32_t ltx = c >> s;
    uint32_t counted = 0u, black = 0u, rejected = 0u;
    uint32_t accQ = 0u, accN = 0u, accRow = 0u; // this thread's partial of tile (ltx, accRow)
    for (uint32_t pass = 0u; pass < kNoiseBlockSide / kNoiseRowsPerPass; pass += kNoiseBatch)
    {
        float4 A[kNoiseBatch], B[kNoiseBatch];
#pragma unroll
        for (uint32_t j = 0u; j < kNoiseBatch; j++)
        {
            const uint32_t y = y0 + (pass + j) * kNoiseRowsPerPass, yc = y < a.height ? y : a.height - 1u;
            const size_t at = (size_t)yc * a.width + xc;
            A[j] = a.halfA[at];
            B[j] = a.halfB[at];
        }
#pragma unroll
        for (uint32_t j = 0u; j < kNoiseBatch; j++)
        {
            const uint32_t ly = w + (pass + j) * kNoiseRowsPerPass, y = blockIdx.y * kNoiseBlockSide + ly;
            const uint32_t lty = ly >> s;
            if (lty != accRow) // the same for every lane of the wave
            {
                if (accN | accQ)
                {
                    atomicAdd(&tileQ[accRow * perSide + ltx], (unsigned long long)accQ);
                    atomicAdd(&tileN[accRow * perSide + ltx], accN);
                }
                accQ = 0u;
                accN = 0u;
                accRow = lty;
            }
            if (!inX || y >= a.height)
                continue;
            const float4 S = make_float4(A[j].x + B[j].x, A[j].y + B[j].y, A[j].z + B[j].z, A[j].w + B[j].w); // step 1
            uint32_t q, cls;
            if (ADAPTIVE)
            {
                const NoiseTileScale v = scale[lty * perSide + ltx];
                if (WRITE_SUM)
                    a.sum[(size_t)y * a.width + x] = (v.flags & 2u) ? make_float4(S.x * v.k, S.y * v.k, S.z * v.k, S.w * v.k) : S;
                q = 0u;
                cls = (v.flags & 1u) ? 2u : noisePixel(A[j], B[j], S, v.sa, v.sb, v.st, q);
            }
            else
            {
                if (WRITE_SUM)
                    a.sum[(size_t)y * a.width + x] = S;
                cls = noisePixel(A[j], B[j], S, a.sa, a.sb, a.st, q);
            }
            if (cls == 2u)
                rejected++;
            else
            {
                counted++;
                black += cls;
                accN++;
                accQ += q;
            }
        }
    }
    if (accN | accQ)
    {
        atomicAdd(&tileQ[accRow * perSide + ltx], (unsigned long long)accQ);
        atomicAdd(&tileN[accRow * perSide + ltx], accN);
    }
    if (counted)
        atomicAdd(&classes[0], counted);
    if (black)
        atomicAdd(&classes[1], black);
    if (rejected)
        atomicAdd(&classes[2], rejected);
    __syncthreads();
    if (t >= 64u) // the first wave: a tile per lane
        return;
    unsigned long long Q = 0ull;
    uint32_t conv = 0u, eBits = 0u;
    const uint32_t tx = blockIdx.x * perSide + (t & (perSide - 1u)), ty = blockIdx.y * perSide + (t >> (kNoiseBlockShift - s));
    if (t < perSide * perSide && tx < a.tilesX && ty < a.tilesY)
    {
        Q = tileQ[t];
        const uint32_t n = tileN[t];
        const float E = n ? (float)((double)Q / ((double)n * 65536.0)) : 0.0f; // step 6
        conv = E <= a.threshold ? 1u : 0u;
        if (ADAPTIVE && (scale[t].flags & 1u)) // an unsampled tile never freezes
            conv = 0u;
        eBits = __float_as_uint(E); // E >= 0 and never a NaN: the order of the bits is the order of the values
        NoiseTile rec;
        rec.Q = Q;
        rec.n = n;
        rec.converged = conv;
        const size_t at = (size_t)ty * a.tilesX + tx;
        a.tiles[at] = rec;
        a.tileErrors[at] = E;
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1)
    {
        Q += __shfl_down(Q, d, 64);
        conv += __shfl_down(conv, d, 64);
        const uint32_t o = __shfl_down(eBits, d, 64);
        eBits = o > eBits ? o : eBits;
    }
    if (t == 0u)
    {
        uint32_t *rec = a.records + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * kNoiseRecordWords;
        uint4 lo, hi;
        lo.x = (uint32_t)Q; lo.y = (uint32_t)(Q >> 32); lo.z = classes[0]; lo.w = classes[1];
        hi.x = classes[2]; hi.y = conv; hi.z = eBits; hi.w = 0u;
        reinterpret_cast<uint4 *>(rec)[0] = lo;
        reinterpret_cast<uint4 *>(rec)[1] = hi;
    }
}

template <bool WRITE_SUM>
__global__ void __launch_bounds__(kNoiseBlock) k_noise_tiles(NoiseArgs a)
{
    noiseTilesBody<WRITE_SUM, false>(a, nullptr);
}

struct NoiseResolveArgs
{
    const uint32_t *records;
    uint32_t recordCount;
    PtxNoiseResult *result;
    uint32_t tilesX, tilesY, calls;
};

__global__ void __launch_bounds__(kNoiseResolveBlock) k_noise_resolve(NoiseResolveArgs a)
{
    __shared__ unsigned long long accQ;
    __shared__ uint32_t acc[5]; // counted, black, rejected, converged, bits of the maximum
    const uint32_t t = threadIdx.x;
    if (t == 0u)
        accQ = 0ull;
    if (t < 5u)
        acc[t] = 0u;
    __syncthreads();
    unsigned long long Q = 0ull;
    uint32_t counted = 0u, black = 0u, rejected = 0u, conv = 0u, eBits = 0u;
    const auto add = [&](const uint4 &lo, const uint4 &hi) {
        Q += (unsigned long long)lo.x | ((unsigned long long)lo.y << 32);
        counted += lo.z;
        black += lo.w;
        rejected += hi.x;
        conv += hi.y;
        eBits = hi.z > eBits ? hi.z : eBits;
    };
    const uint4 *rec = reinterpret_cast<const uint4 *>(a.records);
    constexpr uint32_t kBatch = 4u;
    uint32_t i = t;
    for (; i + (kBatch - 1u) * kNoiseResolveBlock < a.recordCount; i += kBatch * kNoiseResolveBlock)
    {
        uint4 lo[kBatch], hi[kBatch];
#pragma unroll
        for (uint32_t j = 0u; j < kBatch; j++)
        {
            lo[j] = rec[2u * (size_t)(i + j * kNoiseResolveBlock)];
            hi[j] = rec[2u * (size_t)(i + j * kNoiseResolveBlock) + 1u];
        }
#pragma unroll
        for (uint32_t j = 0u; j < kBatch; j++)
            add(lo[j], hi[j]);
    }
    for (; i < a.recordCount; i += kNoiseResolveBlock)
        add(rec[2u * (size_t)i], rec[2u * (size_t)i + 1u]);
#pragma unroll
    for (int d = 32; d > 0; d >>= 1)
    {
        Q += __shfl_down(Q, d, 64);
        counted += __shfl_down(counted, d, 64);
        black += __shfl_down(black, d, 64);
        rejected += __shfl_down(rejected, d, 64);
        conv += __shfl_down(conv, d, 64);
        const uint32_t o = __shfl_down(eBits, d, 64);
        eBits = o > eBits ? o : eBits;
    }
    if ((t & 63u) == 0u) // integer sums and a maximum: no order to depend on
    {
        atomicAdd(&accQ, Q);
        atomicAdd(&acc[0], counted);
        atomicAdd(&acc[1], black);
        atomicAdd(&acc[2], rejected);
        atomicAdd(&acc[3], conv);
        atomicMax(&acc[4], eBits);
    }
    __syncthreads();
    if (t != 0u)
        return;
    PtxNoiseResult res;
    const uint32_t n = acc[0];
    res.meanError = n ? (float)((double)accQ / ((double)n * 65536.0)) : 0.0f; // step 7
    res.maxError = n ? __uint_as_float(acc[4]) : 0.0f;
    res.tilesX = a.tilesX;
    res.tilesY = a.tilesY;
    res.converged = acc[3];
    res.counted = n;
    res.black = acc[1];
    res.rejected = acc[2];
    res.valid = n ? 1u : 0u;
    res.calls = a.calls;
    *a.result = res;
}
