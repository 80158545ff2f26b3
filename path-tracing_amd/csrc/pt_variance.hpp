// pt_variance.hpp -- variance-guided denoising (docs/NEXT_ROWS.md section 16; semantics: include/ptx.h ptx_temporal_accumulate_moments
// and ptx_denoise_variance): the first two luminance moments accumulated beside the colour history, a per-pixel variance from them,
// and an a-trous filter whose colour weight is measured in that variance.  Three kernels, host side in pt_chain_host.hpp, all on
// k_denoise's 32 x 8 tiles with one thread per pixel:
//
//   k_temporal_moments<SAME_CAMERA>  k_temporal's pixel (temporalPixel, pt_temporal.hpp: the same expressions, so T and the colour
//                                    history are the same bits) carrying one more history image, (mu1, mu2, L_M, 0), along its taps
//   k_variance_estimate              V_0 from the moments -- mu2 - mu1^2 where L_M >= 4, a 7 x 7 edge-weighted window elsewhere --
//                                    and the filter's input P_0 = (c_0.rgb, V_0): T demodulated, V = -1 on a pixel that is not valid
//   k_denoise_variance<LAST>         one iteration over P_i -> P_{i+1}: a tap is one 16-byte load of (c_i.rgb, V_i) whose sign carries
//                                    the validity that k_denoise keeps in w, and the normal and position of the taps that pass it
//
// The estimate writes P_0 itself, so the filter has no first-launch variant: k_denoise's FIRST exists to demodulate, and here that
// happened a launch earlier.  Nothing is staged in LDS (the 7 x 7 window runs only where the history is shorter than four frames).
// float32 in the order the header states; the weights use the hardware's exp2 as k_denoise's do.
#pragma once

#include "pt_temporal.hpp"

PT_DEV float luminance_(f3 c) { return (0.2126f * c.x + 0.7152f * c.y) + 0.0722f * c.z; }

// ---- the moments --------------------------------------------------------------------------------------------------------------------

struct MomentHistory
{
    const float4 *in; // (mu1, mu2, L_M, 0) of the previous moments call; nullptr: none (no history, RESET, or a plain call in between)
    float4 *out;
    float maxHistory;
    float m1 = 0.0f, m2 = 0.0f, lacc = 0.0f, wsum = 0.0f;

    // q counted for the colour: it counts here if its moments are known and finite
    PT_DEV void tap(uint32_t q, float w)
    {
        if (!in)
            return;
        const float4 m = in[q];
        if (!(m.z > 0.0f) || !finite_(m.x) || !finite_(m.y))
            return;
        m1 = m1 + m.x * w;
        m2 = m2 + m.y * w;
        lacc = lacc + m.z * w;
        wsum = wsum + w;
    }
    PT_DEV void store(uint32_t p, f3 c)
    {
        const float l = luminance_(c);
        float M1 = l, M2 = l * l, L = 1.0f;
        if (wsum >= 0.015625f) // 1 / 64
        {
            const float inv = rcp_(wsum);
            const float h1 = m1 * inv, h2 = m2 * inv;
            L = fmin_(lacc * inv + 1.0f, maxHistory);
            const float invL = rcp_(L);
            M1 = h1 + (M1 - h1) * invL;
            M2 = h2 + (M2 - h2) * invL;
        }
        const bool known = finite_(M1) && finite_(M2);
        out[p] = known ? make_float4(M1, M2, L, 0.0f) : make_float4(0.0f, 0.0f, 0.0f, 0.0f); // L_M = 0: unknown, no tap takes it
    }
    PT_DEV void storeNotValid(uint32_t p) { out[p] = make_float4(0.0f, 0.0f, 0.0f, 0.0f); }
};

template <bool SAME_CAMERA>
__global__ void __launch_bounds__(kDenoiseTileX *kDenoiseTileY) k_temporal_moments(TemporalArgs a, const float4 *momentsIn, float4 *momentsOut)
{
    MomentHistory m;
    m.in = momentsIn;
    m.out = momentsOut;
    m.maxHistory = a.maxHistory;
    temporalPixel<SAME_CAMERA>(a, m);
}

// ... through the motion guides (ptx_temporal_accumulate_motion with withMoments = 1)
template <bool SAME_CAMERA>
__global__ void __launch_bounds__(kDenoiseTileX *kDenoiseTileY) k_temporal_moments_motion(TemporalArgs a, const float4 *momentsIn, float4 *momentsOut,
                                                                                          TemporalMotion motion)
{
    MomentHistory m;
    m.in = momentsIn;
    m.out = momentsOut;
    m.maxHistory = a.maxHistory;
    temporalPixel<SAME_CAMERA, MomentHistory, true>(a, m, &motion);
}

// ---- the estimate and the filter ----------------------------------------------------------------------------------------------------

struct VarianceArgs
{
    const float4 *temporal; // T (the estimate)
    const float4 *moments;  // (mu1, mu2, L_M, 0) (the estimate)
    float *variance;        // V_0, one float per pixel (the estimate)
    const float4 *src;      // P_i = (c_i.rgb, V_i >= 0) on a valid pixel, (m, -1) elsewhere (the filter)
    float4 *dst;            // P_0 (the estimate), P_{i+1}, or the denoised mean with alpha 1 (the last launch)
    const float4 *normal;   // the guides
    const float4 *position;
    const float4 *albedo;
    uint32_t width, height;
    int32_t step;              // 2^i
    float invSigmaLuminance2;  // 1 / sigmaLuminance^2
    float invSigmaNormal2;     // 1 / sigmaNormal^2
    float invSigmaPosition;    // 1 / sigmaPosition
};

constexpr int kVarianceWindow = 3; // the estimate's window is 7 x 7

// section 13's normal and position terms of the tap q seen from p
PT_DEV float varianceEdgeTerms(const VarianceArgs &a, f3 nP, f3 xP, float invDepth, float4 nq, float4 xq)
{
    const f3 dn = nP - F3(nq.x, nq.y, nq.z);
    const float plane = dot(nP, F3(xq.x, xq.y, xq.z) - xP) * invDepth;
    return dot(dn, dn) * a.invSigmaNormal2 + plane * plane;
}

__global__ void __launch_bounds__(kDenoiseTileX *kDenoiseTileY) k_variance_estimate(VarianceArgs a)
{
    const int x = (int)(blockIdx.x * kDenoiseTileX + threadIdx.x), y = (int)(blockIdx.y * kDenoiseTileY + threadIdx.y);
    if (x >= (int)a.width || y >= (int)a.height)
        return;
    const uint32_t p = (uint32_t)y * a.width + (uint32_t)x;
    const float4 np = a.normal[p];
    const float4 xp = a.position[p];
    const float4 t = a.temporal[p];
    const f3 mean = F3(t.x, t.y, t.z);
    if (!denoiseValid(mean, np, xp.w))
    {
        a.variance[p] = 0.0f;
        a.dst[p] = make_float4(mean.x, mean.y, mean.z, -1.0f);
        return;
    }
    const f3 al = albedoFloor(a.albedo[p]);
    const f3 c = F3(div_(mean.x, al.x), div_(mean.y, al.y), div_(mean.z, al.z));
    const float4 mp = a.moments[p];
    float v;
    if (mp.z >= 4.0f)
        v = mp.y - mp.x * mp.x;
    else
    {
        const float invDepth = a.invSigmaPosition * rcp_(xp.w);
        const f3 nP = F3(np.x, np.y, np.z), xP = F3(xp.x, xp.y, xp.z);
        const bool known = mp.z > 0.0f;
        float m1 = known ? mp.x : 0.0f, m2 = known ? mp.y : 0.0f, wsum = known ? 1.0f : 0.0f; // the centre, by rule
#pragma unroll 1
        for (int dy = -kVarianceWindow; dy <= kVarianceWindow; dy++)
        {
            const int qy = y + dy;
            if (qy < 0 || qy >= (int)a.height)
                continue;
#pragma unroll 1
            for (int dx = -kVarianceWindow; dx <= kVarianceWindow; dx++)
            {
                const int qx = x + dx;
                if ((dx == 0 && dy == 0) || qx < 0 || qx >= (int)a.width)
                    continue;
                const uint32_t q = (uint32_t)qy * a.width + (uint32_t)qx;
                const float4 mq = a.moments[q];
                if (!(mq.z > 0.0f))
                    continue;
                const float4 nq = a.normal[q];
                const float4 xq = a.position[q];
                const float4 tq = a.temporal[q];
                if (!denoiseValid(F3(tq.x, tq.y, tq.z), nq, xq.w))
                    continue;
                const float e = varianceEdgeTerms(a, nP, xP, invDepth, nq, xq);
                const float w = __builtin_amdgcn_exp2f(e * -1.44269504f); // a NaN e gives a NaN v, which is stored as 0
                m1 = m1 + mq.x * w;
                m2 = m2 + mq.y * w;
                wsum = wsum + w;
            }
        }
        v = 0.0f;
        if (wsum != 0.0f)
        {
            const float inv = rcp_(wsum);
            m1 = m1 * inv;
            m2 = m2 * inv;
            v = m2 - m1 * m1;
        }
    }
    const float v0 = (finite_(v) && v > 0.0f) ? v : 0.0f;
    a.variance[p] = v0;
    a.dst[p] = make_float4(c.x, c.y, c.z, v0);
}

// One thread per pixel.  V_i stays finite and >= 0 on a valid pixel: V_0 is, and V_{i+1} is a mean of V_i with the weights
// w^2 / (sum w)^2 <= 1 over a sum w that holds the centre's 9/64 -- so the sign of P.w is the validity for every i.
template <bool LAST>
__global__ void __launch_bounds__(kDenoiseTileX *kDenoiseTileY) k_denoise_variance(VarianceArgs a)
{
    const int x = (int)(blockIdx.x * kDenoiseTileX + threadIdx.x), y = (int)(blockIdx.y * kDenoiseTileY + threadIdx.y);
    if (x >= (int)a.width || y >= (int)a.height)
        return;
    const uint32_t p = (uint32_t)y * a.width + (uint32_t)x;
    const float4 pp = a.src[p];
    const f3 cp = F3(pp.x, pp.y, pp.z);
    const bool valid = pp.w >= 0.0f;
    f3 out = cp;
    float vOut = pp.w;
    if (valid)
    {
        // the prefilter: the 3 x 3 mean of V_i over the neighbours inside the image and valid
        const float gk[3] = { 0.25f, 0.5f, 0.25f }; // 1/4 centre, 1/8 edges, 1/16 corners
        float vsum = pp.w * 0.25f, gsum = 0.25f;
#pragma unroll
        for (int dy = -1; dy <= 1; dy++)
        {
            const int qy = y + dy;
            if (qy < 0 || qy >= (int)a.height)
                continue;
#pragma unroll
            for (int dx = -1; dx <= 1; dx++)
            {
                const int qx = x + dx;
                if ((dx == 0 && dy == 0) || qx < 0 || qx >= (int)a.width)
                    continue;
                const float vq = a.src[(uint32_t)qy * a.width + (uint32_t)qx].w;
                if (!(vq >= 0.0f))
                    continue;
                const float g = gk[dx + 1] * gk[dy + 1];
                vsum = vsum + vq * g;
                gsum = gsum + g;
            }
        }
        const float vt = vsum * rcp_(gsum);
        const float invVar = a.invSigmaLuminance2 * rcp_(vt); // unused where vt = 0
        const float lp = luminance_(cp);

        const float hk[5] = { 0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f };
        const float4 np = a.normal[p];
        const float4 xp = a.position[p];
        const float invDepth = a.invSigmaPosition * rcp_(xp.w);
        const f3 nP = F3(np.x, np.y, np.z), xP = F3(xp.x, xp.y, xp.z);
        f3 acc = cp * (0.375f * 0.375f); // the centre tap, by rule
        float wsum = 0.375f * 0.375f;
        float vacc = pp.w * ((0.375f * 0.375f) * (0.375f * 0.375f));
#pragma unroll
        for (int dy = -2; dy <= 2; dy++)
        {
            const int qy = y + dy * a.step;
            if (qy < 0 || qy >= (int)a.height)
                continue;
#pragma unroll
            for (int dx = -2; dx <= 2; dx++)
            {
                const int qx = x + dx * a.step;
                if ((dx == 0 && dy == 0) || qx < 0 || qx >= (int)a.width)
                    continue;
                const uint32_t q = (uint32_t)qy * a.width + (uint32_t)qx;
                const float4 pq = a.src[q];
                const f3 cq = F3(pq.x, pq.y, pq.z);
                if (!(pq.w >= 0.0f) || !finite3_(cq))
                    continue;
                const float d = abs_(lp - luminance_(cq));
                float el = 0.0f;
                if (d != 0.0f) // a NaN d goes on and fails e >= 0
                {
                    if (vt == 0.0f)
                        continue;
                    el = (d * d) * invVar;
                }
                const float e = el + varianceEdgeTerms(a, nP, xP, invDepth, a.normal[q], a.position[q]);
                if (!(e >= 0.0f)) // a NaN
                    continue;
                const float w = (hk[dx + 2] * hk[dy + 2]) * __builtin_amdgcn_exp2f(e * -1.44269504f);
                acc = acc + cq * w;
                vacc = vacc + pq.w * (w * w);
                wsum = wsum + w;
            }
        }
        const float inv = rcp_(wsum);
        out = acc * inv;
        vOut = vacc * (inv * inv);
    }
    if (LAST)
    {
        if (valid)
            out = out * albedoFloor(a.albedo[p]);
        a.dst[p] = make_float4(out.x, out.y, out.z, 1.0f);
    }
    else
        a.dst[p] = make_float4(out.x, out.y, out.z, vOut);
}
