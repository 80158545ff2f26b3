// pt_temporal.hpp -- temporal accumulation (docs/NEXT_ROWS.md section 14; semantics: include/ptx.h ptx_temporal_accumulate): the
// history of the previous frames, found by projecting the position guide into the previous camera, blended with the current
// frame's demodulated mean ahead of the filter.  One kernel, host side in pt_chain_host.hpp; its per-pixel body, temporalPixel, is
// also k_temporal_moments' (pt_variance.hpp), which carries the luminance moments along the same taps:
//
//   k_temporal<SAME_CAMERA>  one thread per pixel; reads the sum and the three guides of its pixel and up to four taps of the three
//                            history images (one tap, at the pixel itself, when the camera did not move); writes T and the three
//                            images of the next history
//   k_temporal_motion<SAME_CAMERA>  the same pixel looking its history up through the motion guides (docs/NEXT_ROWS.md section 17):
//                            two more float4 reads, and under the same camera a per-pixel choice between the tap at the pixel
//                            itself and the projected four
//
// Every access is a 16-byte float4 and nothing is staged in LDS: the four taps of neighbouring lanes overlap in L1 / L2.  The
// arithmetic is float32 in the order the header states; nothing here is compared with a reference bit for bit.
#pragma once

#include "pt_denoise.hpp"

constexpr uint32_t kTemporalHistoryImages = 3; // (c_acc, L), (n, 0), (x, t)

struct TemporalArgs
{
    const float4 *sum;      // the accumulation image (running sum)
    const float4 *normal;   // the guides
    const float4 *position;
    const float4 *albedo;
    const float4 *histIn;   // the previous history: (c_acc, L), (n, 0), (x, t), `pixels` apart; nullptr: none, or PTX_TEMPORAL_RESET
    float4 *histOut;        // the next history, in the same form
    float4 *out;            // T
    uint32_t width, height, pixels;
    float totalSamples;
    float maxHistory;
    float normalThreshold2; // normalThreshold^2, the float32 product
    float positionThreshold;
    float view[16], proj[16]; // View' and Proj' of the previous history (unused by SAME_CAMERA and without a history)
};

// out = M (x, y, z, w), column-major, summed left to right
PT_DEV void temporalMul(const float *m, float x, float y, float z, float w, float &ox, float &oy, float &oz, float &ow)
{
    ox = ((m[0] * x + m[4] * y) + m[8] * z) + m[12] * w;
    oy = ((m[1] * x + m[5] * y) + m[9] * z) + m[13] * w;
    oz = ((m[2] * x + m[6] * y) + m[10] * z) + m[14] * w;
    ow = ((m[3] * x + m[7] * y) + m[11] * z) + m[15] * w;
}

// One tap inside the image with the bilinear weight w: its share of the sums if it counts, and whether it did
PT_DEV bool temporalTap(const TemporalArgs &a, uint32_t q, float w, f3 nP, f3 xP, float planeBound, f3 &acc, float &lacc, float &wsum)
{
    const float4 h = a.histIn[q];
    if (!(h.w > 0.0f) || !finite3_(F3(h.x, h.y, h.z)))
        return false;
    const float4 nq = a.histIn[(size_t)a.pixels + q];
    const float4 xq = a.histIn[2 * (size_t)a.pixels + q];
    const f3 dn = nP - F3(nq.x, nq.y, nq.z);
    const float plane = dot(nP, F3(xq.x, xq.y, xq.z) - xP);
    if (!(dot(dn, dn) <= a.normalThreshold2) || !(abs_(plane) <= planeBound)) // a NaN fails either
        return false;
    acc = acc + F3(h.x, h.y, h.z) * w;
    lacc = lacc + h.w * w;
    wsum = wsum + w;
    return true;
}

// What a kernel carries along the colour's taps: tap(q, w) after every tap that counted for the colour, then exactly one of
// store(p, c) on a valid pixel (c: this frame's demodulated mean) and storeNotValid(p).  k_temporal carries nothing;
// k_temporal_moments (pt_variance.hpp) the luminance moments.
struct TemporalColourOnly
{
    PT_DEV void tap(uint32_t, float) {}
    PT_DEV void store(uint32_t, f3) {}
    PT_DEV void storeNotValid(uint32_t) {}
};

// The motion guides of ptx_temporal_accumulate_motion (docs/NEXT_ROWS.md section 17): (x~, known) and (n~, known) per pixel, the
// surface point and its normal in the pose of the history.  A kernel argument of its own: TemporalArgs does not grow.
struct TemporalMotion
{
    const float4 *position, *normal;
};

// MOTION: the history is looked up with (x~, n~) in place of (x_p, n_p) -- projected, and tested against the taps -- and a pixel
// whose motion is not known takes none.  What is blended and what is stored for the next call stay the current pixel's.
template <bool SAME_CAMERA, class Extra, bool MOTION = false>
PT_DEV void temporalPixel(const TemporalArgs &a, Extra &extra, const TemporalMotion *motion = nullptr)
{
    const int x = (int)(blockIdx.x * kDenoiseTileX + threadIdx.x), y = (int)(blockIdx.y * kDenoiseTileY + threadIdx.y);
    if (x >= (int)a.width || y >= (int)a.height)
        return;
    const uint32_t p = (uint32_t)y * a.width + (uint32_t)x;
    const float4 np = a.normal[p];
    const float4 xp = a.position[p];
    const float4 s = a.sum[p];
    const f3 mean = F3(s.x, s.y, s.z) / a.totalSamples;
    if (!denoiseValid(mean, np, xp.w))
    {
        const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        a.out[p] = make_float4(mean.x, mean.y, mean.z, 0.0f);
        a.histOut[p] = zero; // L = 0: no tap of the next call
        a.histOut[(size_t)a.pixels + p] = zero;
        a.histOut[2 * (size_t)a.pixels + p] = zero;
        extra.storeNotValid(p);
        return;
    }
    const f3 al = albedoFloor(a.albedo[p]);
    const f3 c = F3(div_(mean.x, al.x), div_(mean.y, al.y), div_(mean.z, al.z));
    const f3 nP = F3(np.x, np.y, np.z), xP = F3(xp.x, xp.y, xp.z);
    f3 cAcc = c;
    float L = 1.0f;
    // where the history is looked up, and with which normal; under the same camera, whether at the pixel itself
    f3 nH = nP, xH = xP;
    bool look = a.histIn != nullptr, atPixel = SAME_CAMERA;
    if constexpr (MOTION)
    {
        if (look)
        {
            const float4 mx = motion->position[p], mn = motion->normal[p];
            look = mx.w == 1.0f;
            xH = F3(mx.x, mx.y, mx.z);
            nH = F3(mn.x, mn.y, mn.z);
            // the same-camera rule asks for x~ bit-equal to x_p as well: a point that moved is projected like any other
            atPixel = SAME_CAMERA && __float_as_uint(mx.x) == __float_as_uint(xp.x) && __float_as_uint(mx.y) == __float_as_uint(xp.y) &&
                      __float_as_uint(mx.z) == __float_as_uint(xp.z);
        }
    }
    if (look)
    {
        const float planeBound = a.positionThreshold * xp.w;
        f3 acc = F3s(0.0f);
        float lacc = 0.0f, wsum = 0.0f;
        if (atPixel)
        {
            if (temporalTap(a, p, 1.0f, nH, xH, planeBound, acc, lacc, wsum))
                extra.tap(p, 1.0f);
        }
        else
        {
            float vx, vy, vz, vw, cx, cy, cz, cw;
            temporalMul(a.view, xH.x, xH.y, xH.z, 1.0f, vx, vy, vz, vw);
            temporalMul(a.proj, vx, vy, vz, vw, cx, cy, cz, cw);
            if (cw > 0.0f)
            {
                const float inv = rcp_(cw);
                const float u = ((cx * inv) * 0.5f + 0.5f) * (float)a.width - 0.5f;
                const float v = ((cy * inv) * 0.5f + 0.5f) * (float)a.height - 0.5f;
                // outside (-1, W) x (-1, H) no tap with a weight is inside the image; a NaN fails the test, and what passes fits an int
                if (u > -1.0f && u < (float)a.width && v > -1.0f && v < (float)a.height)
                {
                    const float fx0 = __builtin_floorf(u), fy0 = __builtin_floorf(v);
                    const float fx = u - fx0, fy = v - fy0;
                    const int x0 = (int)fx0, y0 = (int)fy0;
#pragma unroll
                    for (int j = 0; j < 2; j++)
                    {
                        const int qy = y0 + j;
                        if (qy < 0 || qy >= (int)a.height)
                            continue;
#pragma unroll
                        for (int i = 0; i < 2; i++)
                        {
                            const int qx = x0 + i;
                            if (qx < 0 || qx >= (int)a.width)
                                continue;
                            const float w = (i ? fx : 1.0f - fx) * (j ? fy : 1.0f - fy);
                            const uint32_t q = (uint32_t)qy * a.width + (uint32_t)qx;
                            if (temporalTap(a, q, w, nH, xH, planeBound, acc, lacc, wsum))
                                extra.tap(q, w);
                        }
                    }
                }
            }
        }
        if (wsum >= 0.015625f) // 1 / 64
        {
            const float inv = rcp_(wsum);
            const f3 ch = acc * inv;
            L = fmin_(lacc * inv + 1.0f, a.maxHistory);
            cAcc = ch + (c - ch) * rcp_(L);
        }
    }
    const f3 t = cAcc * al;
    a.out[p] = make_float4(t.x, t.y, t.z, L);
    a.histOut[p] = make_float4(cAcc.x, cAcc.y, cAcc.z, L);
    a.histOut[(size_t)a.pixels + p] = make_float4(nP.x, nP.y, nP.z, 0.0f);
    a.histOut[2 * (size_t)a.pixels + p] = xp;
    extra.store(p, c);
}

template <bool SAME_CAMERA>
__global__ void __launch_bounds__(kDenoiseTileX *kDenoiseTileY) k_temporal(TemporalArgs a)
{
    TemporalColourOnly none;
    temporalPixel<SAME_CAMERA>(a, none);
}

template <bool SAME_CAMERA>
__global__ void __launch_bounds__(kDenoiseTileX *kDenoiseTileY) k_temporal_motion(TemporalArgs a, TemporalMotion motion)
{
    TemporalColourOnly none;
    temporalPixel<SAME_CAMERA, TemporalColourOnly, true>(a, none, &motion);
}
