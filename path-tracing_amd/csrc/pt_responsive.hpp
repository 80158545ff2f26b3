// pt_responsive.hpp -- the responsive temporal history (docs/NEXT_ROWS.md section 19; semantics: include/ptx.h
// ptx_temporal_accumulate_responsive): a second, short history F beside the long one, and a clamp of the long one into the box F spans
// around the pixel.  Two kernels, host side in pt_chain_host.hpp, both on k_denoise's 32 x 8 tiles with one thread per pixel:
//
//   k_temporal_responsive<SAME_CAMERA, MOMENTS, MOTION>  k_temporal's pixel (temporalPixel, pt_temporal.hpp: the same expressions, so T
//                                    and the colour history are the base call's bits) carrying one more history image, (F.rgb, L_F),
//                                    along its taps; with MOMENTS the moment history rides along too, MomentHistory as it is
//   k_responsive_clamp<MOMENTS>      the 5 x 5 window of this call's F: the tile and a halo of 2 staged in LDS (36 x 12 float4, 6,912 B),
//                                    two sweeps of 25 LDS reads, and on a clamped pixel three 16-byte rewrites of the pixel's own entries
//
// The clamp is the chain's first stage that stages a tile: the 25 taps of neighbouring lanes overlap 24 / 25.  A sweep reads every
// tap's whole entry, whether it counts or not, and selects: as compiled (checked in the assembly, both variants) the kernel holds 49
// ds_read_b128 at constant offsets from the thread's own entry -- 24 + 25; the centre of the first sweep is read ahead of the early
// exit as one ds_read_b32 (L_F) and one ds_read_b96 -- two ds_write_b128 and no branch inside a sweep.  Written with `if (L_F > 0)`
// around the sums it compiled to 25 ds_read_b32 and 49 ds_read_b96 with a branch per tap; without the compiler barrier between the
// sweeps to 25 reads kept in 108 VGPRs and 4 waves.  ds_read_b128's four 16-lane groups ({0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} of
// each half-wave) each lie in one row of the tile and read 16 different consecutive entries, that is 16 different 16-byte slots
// modulo the 256-byte bank row, every bank once: conflict-free by the bank rule whatever the row pitch is, 576 B included.  The one
// ds_read_b32 is 4-way (lanes l, l + 8, l + 16, l + 24 of a half-wave meet on (4 l + 3) mod 32).  In global memory the tile's two loads,
// the colour history's load and the two rewrites are 16-byte accesses; the compiler narrows the albedo to 12 bytes and the moments'
// read and rewrite to L_M's 4.  float32 in the order the header states.
#pragma once

#include "pt_variance.hpp"

// ---- pass A: the fast history ---------------------------------------------------------------------------------------------------------

struct FastHistory
{
    const float4 *in; // (F.rgb, L_F) of the previous responsive call; nullptr: none (no history, RESET, or a call that was not responsive in between)
    float4 *out;
    float fastHistory;
    f3 acc = F3s(0.0f);
    float lacc = 0.0f, wsum = 0.0f;

    // q counted for the colour: it counts here if its F is known and finite
    PT_DEV void tap(uint32_t q, float w)
    {
        if (!in)
            return;
        const float4 f = in[q];
        if (!(f.w > 0.0f) || !finite3_(F3(f.x, f.y, f.z)))
            return;
        acc = acc + F3(f.x, f.y, f.z) * w;
        lacc = lacc + f.w * w;
        wsum = wsum + w;
    }
    // the colour's blend (temporalPixel), operation for operation
    PT_DEV void store(uint32_t p, f3 c)
    {
        f3 F = c;
        float L = 1.0f;
        if (wsum >= 0.015625f) // 1 / 64
        {
            const float inv = rcp_(wsum);
            const f3 fh = acc * inv;
            L = fmin_(lacc * inv + 1.0f, fastHistory);
            F = fh + (c - fh) * rcp_(L);
        }
        out[p] = finite3_(F) ? make_float4(F.x, F.y, F.z, L) : make_float4(0.0f, 0.0f, 0.0f, 0.0f); // L_F = 0: unknown, no tap takes it
    }
    PT_DEV void storeNotValid(uint32_t p) { out[p] = make_float4(0.0f, 0.0f, 0.0f, 0.0f); }
};

// F and the moments along the same taps
struct FastAndMoments
{
    FastHistory fast;
    MomentHistory moments;
    PT_DEV void tap(uint32_t q, float w) { fast.tap(q, w); moments.tap(q, w); }
    PT_DEV void store(uint32_t p, f3 c) { fast.store(p, c); moments.store(p, c); }
    PT_DEV void storeNotValid(uint32_t p) { fast.storeNotValid(p); moments.storeNotValid(p); }
};

// F's pointers and the moments' are kernel arguments of their own: TemporalArgs does not grow
struct ResponsiveHistories
{
    const float4 *fastIn;
    float4 *fastOut;
    const float4 *momentsIn; // MOMENTS
    float4 *momentsOut;
    float fastHistory;
};

template <bool SAME_CAMERA, bool MOMENTS, bool MOTION>
__global__ void __launch_bounds__(kDenoiseTileX *kDenoiseTileY) k_temporal_responsive(TemporalArgs a, ResponsiveHistories h, TemporalMotion motion)
{
    FastHistory f;
    f.in = h.fastIn;
    f.out = h.fastOut;
    f.fastHistory = h.fastHistory;
    if constexpr (MOMENTS)
    {
        FastAndMoments both;
        both.fast = f;
        both.moments.in = h.momentsIn;
        both.moments.out = h.momentsOut;
        both.moments.maxHistory = a.maxHistory;
        temporalPixel<SAME_CAMERA, FastAndMoments, MOTION>(a, both, &motion);
    }
    else
        temporalPixel<SAME_CAMERA, FastHistory, MOTION>(a, f, &motion);
}

// ---- pass B: the clamp ----------------------------------------------------------------------------------------------------------------

constexpr int kClampHalo = 2;                                  // the window is 5 x 5
constexpr int kClampPitch = kDenoiseTileX + 2 * kClampHalo;    // 36 entries, 576 B
constexpr int kClampRows = kDenoiseTileY + 2 * kClampHalo;     // 12
constexpr int kClampEntries = kClampPitch * kClampRows;        // 432

struct ResponsiveClampArgs
{
    const float4 *fast;   // (F.rgb, L_F) of this call
    float4 *temporal;     // T, as pass A wrote it
    float4 *history;      // (c_acc, L), the first image of the colour history pass A wrote
    float4 *moments;      // (mu1, mu2, L_M, 0) as pass A wrote it (MOMENTS)
    const float4 *albedo; // the guide
    uint32_t width, height;
    float clampSigma;
};

template <bool MOMENTS>
__global__ void __launch_bounds__(kDenoiseTileX *kDenoiseTileY) k_responsive_clamp(ResponsiveClampArgs a)
{
    __shared__ float4 tile[kClampEntries];
    const int tx = (int)threadIdx.x, ty = (int)threadIdx.y;
    const int x0 = (int)(blockIdx.x * kDenoiseTileX) - kClampHalo, y0 = (int)(blockIdx.y * kDenoiseTileY) - kClampHalo;
    // 432 entries by 256 threads: two rounds, the second with 176 of them.  Outside the image: zeros, L_F = 0, in no window.
#pragma unroll
    for (int e = ty * kDenoiseTileX + tx; e < kClampEntries; e += kDenoiseTileX * kDenoiseTileY)
    {
        const int ly = e / kClampPitch, lx = e - ly * kClampPitch;
        const int gx = x0 + lx, gy = y0 + ly;
        float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (gx >= 0 && gx < (int)a.width && gy >= 0 && gy < (int)a.height)
            v = a.fast[(size_t)gy * a.width + (size_t)gx];
        tile[e] = v;
    }
    __syncthreads(); // every thread of the workgroup gets here: those outside the image leave only now
    const int x = x0 + kClampHalo + tx, y = y0 + kClampHalo + ty;
    if (x >= (int)a.width || y >= (int)a.height)
        return;
    const size_t p = (size_t)y * a.width + (size_t)x;
    const float4 *win = tile + ty * kClampPitch + tx; // the window's corner (-2, -2); the centre is win[2 * kClampPitch + 2]
    const float4 h = a.history[p];
    const f3 c = F3(h.x, h.y, h.z);
    const float LF = win[kClampHalo * kClampPitch + kClampHalo].w;
    if (!(h.w > 1.0f) || !(LF > 0.0f) || !finite3_(c))
        return;
    f3 sum = F3s(0.0f);
    float n = 0.0f;
#pragma unroll
    for (int j = 0; j <= 2 * kClampHalo; j++)
#pragma unroll
        for (int i = 0; i <= 2 * kClampHalo; i++)
        {
            // the whole entry, whether it counts or not, and a select: one 16-byte LDS read per tap and no branch
            const float4 f = win[j * kClampPitch + i];
            const bool counts = f.w > 0.0f;
            const f3 with = sum + F3(f.x, f.y, f.z);
            sum = F3(counts ? with.x : sum.x, counts ? with.y : sum.y, counts ? with.z : sum.z);
            n = counts ? n + 1.0f : n;
        }
    const float invN = rcp_(n);
    const f3 mu = sum * invN;
    // the second sweep reads the tile again: kept in registers across the two, the 25 entries cost 100 VGPRs and half the waves
    asm volatile("" ::: "memory");
    f3 sq = F3s(0.0f);
#pragma unroll
    for (int j = 0; j <= 2 * kClampHalo; j++)
#pragma unroll
        for (int i = 0; i <= 2 * kClampHalo; i++)
        {
            const float4 f = win[j * kClampPitch + i];
            const bool counts = f.w > 0.0f;
            const f3 d = F3(f.x, f.y, f.z) - mu;
            const f3 with = sq + d * d;
            sq = F3(counts ? with.x : sq.x, counts ? with.y : sq.y, counts ? with.z : sq.z);
        }
    const f3 var = sq * invN;
    const f3 half = F3(sqrt_(var.x), sqrt_(var.y), sqrt_(var.z)) * a.clampSigma;
    const f3 lo = mu - half, hi = mu + half;
    // comparisons: a bound that is not a number clamps nothing
    const bool clamped = c.x < lo.x || c.x > hi.x || c.y < lo.y || c.y > hi.y || c.z < lo.z || c.z > hi.z;
    if (!clamped)
        return; // T and the histories hold (c_acc a_p, L) and (c_acc, L) already
    const f3 cc = F3(c.x < lo.x ? lo.x : (c.x > hi.x ? hi.x : c.x), c.y < lo.y ? lo.y : (c.y > hi.y ? hi.y : c.y), c.z < lo.z ? lo.z : (c.z > hi.z ? hi.z : c.z));
    const float L = fmin_(h.w, LF);
    const f3 t = cc * albedoFloor(a.albedo[p]);
    a.temporal[p] = make_float4(t.x, t.y, t.z, L);
    a.history[p] = make_float4(cc.x, cc.y, cc.z, L);
    if constexpr (MOMENTS)
    {
        float4 m = a.moments[p];
        if (m.z > 0.0f)
        {
            m.z = fmin_(m.z, LF);
            a.moments[p] = m;
        }
    }
}
