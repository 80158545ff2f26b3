// pt_despike.hpp -- firefly suppression ahead of the chain and the output stage (docs/NEXT_ROWS.md section 20; semantics: include/ptx.h
// ptx_despike): every pixel's luminance is capped at `gain` times the `rank`-th largest luminance among its neighbours.  One kernel,
// host side in pt_chain_host.hpp, on k_denoise's 32 x 8 tiles with one thread per pixel:
//
//   k_despike<RADIUS>   the (2 RADIUS + 1)^2 window without its centre, over luminances only: the tile and a halo of RADIUS staged in
//                       LDS as one float per pixel ((32 + 2 R) x (8 + 2 R): 1,360 B at R = 1, 1,728 B at R = 2), a pixel that does not
//                       count (outside the image, luminance not finite) as -inf, which loses every comparison and is told from a
//                       counting one by one compare.  Every interior thread loads its own S(p) once, keeps it in registers and stages
//                       its luminance; the halo follows in a second round (84 / 176 of the 256 threads), rows first, then the side
//                       columns.  One barrier that every thread reaches.  The scan is fully unrolled and holds no branch: per tap one
//                       LDS read, one compare for n and a four-register insertion network (4 max, 3 min) that keeps the four largest
//                       in order, equal values separately; `rank` picks the register afterwards, the same for the whole wave.
//
// LDS by the bank rule (4-byte accesses: bank = word address mod 32, conflicts within a 32-lane half-wave only).  A half-wave is one tile
// row: 32 consecutive floats, for the own-pixel write and for every tap's read (a constant offset from the thread's own entry), so 32
// different banks whatever the row pitch is -- no conflict.  Halo round, R = 2 (pitch 36): the two top rows are entries 0 .. 71 and the
// two bottom rows start 288 entries (= 0 mod 32) after them, so lanes stay consecutive modulo 32 across the gap: none; the side columns
// put four lanes on a row at words {0, 1, 34, 35} + 36 j, banks {0, 1, 2, 3} + 4 j modulo 32 over eight rows: all 32 different, none.
// R = 1 (pitch 34): the bottom row starts 272 entries (= 16 mod 32) after the top one, so in the one half-wave that straddles the gap
// two lanes of the top row meet two of the bottom row: 2-way on two banks, once per workgroup; the side columns, words {0, 33} + 34 j,
// are 16 different banks.  Global memory: one 16-byte load and one 16-byte store per pixel, plus the halo's loads.  float32 in the order
// the header states.
#pragma once

#include "pt_variance.hpp"

struct DespikeArgs
{
    const float4 *sum; // S
    float4 *out;       // C
    uint32_t width, height;
    uint32_t rank;    // 1 .. 4
    uint32_t minTaps; // rank .. (2 R + 1)^2 - 1
    float gain;       // >= 1, finite
};

// the luminance a window sees: -inf where the pixel does not count
PT_DEV float despikeLuminance(float4 s)
{
    const float y = luminance_(F3(s.x, s.y, s.z));
    return finite_(y) ? y : -__builtin_inff();
}

// fmax_ / fmin_ of the network as v_max_f32 / v_min_f32.  No operand is a NaN (the staging took them out), so the two forms give the
// same number; they may differ in the sign of a zero, which never reaches C: a bound of either zero is +0 (step 7 of the header).  As
// compare and select every one of the seven cost v_cmp, a wait state and v_cndmask: 192 + 201 + 226 s_nop in the two kernels against
// 272 v_max / v_min.
PT_DEV float despikeMax(float a, float b) { return __builtin_fmaxf(a, b); }
PT_DEV float despikeMin(float a, float b) { return __builtin_fminf(a, b); }

template <int RADIUS>
__global__ void __launch_bounds__(kDenoiseTileX *kDenoiseTileY) k_despike(DespikeArgs a)
{
    constexpr int kPitch = kDenoiseTileX + 2 * RADIUS, kRows = kDenoiseTileY + 2 * RADIUS;
    constexpr int kHaloRowEntries = 2 * RADIUS * kPitch;                       // the rows above and below the tile, whole
    constexpr int kHaloEntries = kHaloRowEntries + 2 * RADIUS * kDenoiseTileY; // ... and the columns left and right of it
    static_assert(kHaloEntries <= kDenoiseTileX * kDenoiseTileY, "one halo entry per thread at the most");
    __shared__ float lum[kPitch * kRows];
    const int tx = (int)threadIdx.x, ty = (int)threadIdx.y;
    const int x0 = (int)(blockIdx.x * kDenoiseTileX) - RADIUS, y0 = (int)(blockIdx.y * kDenoiseTileY) - RADIUS;
    const int x = x0 + RADIUS + tx, y = y0 + RADIUS + ty;
    const bool inside = x < (int)a.width && y < (int)a.height;
    const size_t p = (size_t)y * a.width + (size_t)x;
    // round one: the thread's own pixel, which stays in registers
    float4 s = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    float Y = -__builtin_inff();
    if (inside)
    {
        s = a.sum[p];
        Y = despikeLuminance(s);
    }
    lum[(ty + RADIUS) * kPitch + tx + RADIUS] = Y;
    // round two: the halo, one entry per thread
    const int t = ty * kDenoiseTileX + tx;
    if (t < kHaloEntries)
    {
        int lx, ly;
        if (t < kHaloRowEntries)
        {
            ly = t / kPitch;
            lx = t - ly * kPitch;
            ly += ly >= RADIUS ? kDenoiseTileY : 0;
        }
        else
        {
            const int u = t - kHaloRowEntries, c = u % (2 * RADIUS);
            ly = RADIUS + u / (2 * RADIUS);
            lx = c < RADIUS ? c : c + kDenoiseTileX;
        }
        const int gx = x0 + lx, gy = y0 + ly;
        float v = -__builtin_inff();
        if (gx >= 0 && gx < (int)a.width && gy >= 0 && gy < (int)a.height)
            v = despikeLuminance(a.sum[(size_t)gy * a.width + (size_t)gx]);
        lum[ly * kPitch + lx] = v;
    }
    __syncthreads(); // every thread of the workgroup gets here: those outside the image leave only now
    if (!inside)
        return;
    const float *win = lum + ty * kPitch + tx; // the window's corner (-R, -R)
    float m1 = -__builtin_inff(), m2 = m1, m3 = m1, m4 = m1; // the four largest, m1 >= m2 >= m3 >= m4
    uint32_t n = 0;
#pragma unroll
    for (int j = 0; j <= 2 * RADIUS; j++)
#pragma unroll
        for (int i = 0; i <= 2 * RADIUS; i++)
        {
            if (i == RADIUS && j == RADIUS)
                continue; // (compile time: the centre is in no window)
            float v = win[j * kPitch + i];
            n += v > -__builtin_inff() ? 1u : 0u;
            float lo = despikeMin(m1, v);
            m1 = despikeMax(m1, v);
            v = lo;
            lo = despikeMin(m2, v);
            m2 = despikeMax(m2, v);
            v = lo;
            lo = despikeMin(m3, v);
            m3 = despikeMax(m3, v);
            m4 = despikeMax(m4, lo);
        }
    const float h = a.rank == 1u ? m1 : a.rank == 2u ? m2 : a.rank == 3u ? m3 : m4;
    const float gh = a.gain * h;
    const float b = gh > 0.0f ? gh : 0.0f;
    // Y is -inf where p does not count, which fails both comparisons
    const bool clamped = n >= a.minTaps && Y >= 1.17549435e-38f && Y > b;
    const float scale = div_(b, Y);
    a.out[p] = clamped ? make_float4(s.x * scale, s.y * scale, s.z * scale, s.w) : s;
}
