// pt_grade.hpp -- the display transform on the device (docs/NEXT_ROWS.md section 22; semantics: include/ptx.h ptx_grade, steps 0 - 5):
// a colour matrix, an ASC CDL grade, one of four tone curves and a tetrahedral 3-D LUT in the place of the output stage's last step.
//
//   k_compose_grade        k_compose_tonemap with gradePixel where toneMapPixel stands: 24 B in, 16 B out per pixel, grid-stride.
//   k_present_graded<F, H> k_present with gradePixel where toneMapPixel stands.
// Both bodies are the older kernels' own, composeStore (pt_post.hpp) and presentPixel (pt_present.hpp), which take the step between the
// composed colour and the UI as a functor: Grade here.  Those two files know nothing of the grade.  tests/test_grade.py holds each
// pair together: under an identity desc the two kernels give the same bits.
//
// Which steps run is decided on the host (the skip rule of the header) and arrives as bits of GradeArgs::steps, a kernel argument:
// every branch on it is a scalar branch, and a wave never diverges on the grade.  The four curves share one kernel; the registers
// are those of the heaviest step, pow_ (double precision), which steps 2b and the sRGB domain of the LUT use.
//
// The LUT is read from global memory as the host wrote it, 12 B per entry, red fastest: four lattice points per pixel at
// data-dependent addresses, of which V000 and V111 do not depend on the order of the fractions and are issued ahead of the
// comparisons.  At N = 33 the table is 431 KB and stays in the L2: the lookup adds 0.011 ms to the kernel's 0.015 ms at 1080p and
// 0.040 to 0.066 ms at 2160p (docs/NEXT_ROWS.md section 22, cost), two fifths of the kernel and not most of it.  The LDS-staged form
// was not built: it fits only N <= 17 (59 KB a workgroup), and staging 59 KB for the 1,000 pixels a workgroup of the grid handles at
// 1080p moves more bytes than the 48 B per pixel of lookups it saves, at two workgroups a compute unit.  No LDS, no scratch.
// All indices are bounded by construction: i_k <= N - 2 after the min, so i_k + 1 <= N - 1 on every axis, and a NaN reads entry 0.
#pragma once

#include "pt_present.hpp"
#include "pt_variance.hpp" // luminance_

namespace ptd
{

enum : uint32_t
{
    GRADE_STEP_MATRIX = 1u,       // step 1
    GRADE_STEP_SLOPE_OFFSET = 2u, // step 2a
    GRADE_STEP_POWER = 4u,        // step 2b
    GRADE_STEP_SATURATION = 8u,   // step 2c
    GRADE_STEP_CURVE = 16u,       // step 3: the SDR mode
    GRADE_STEP_LUT = 32u,         // step 4: the SDR mode with PTX_GRADE_USE_LUT
    GRADE_STEP_LUT_SRGB = 64u     // ... in the sRGB domain
};

struct GradeArgs
{
    float m[9];                            // PtxGradeDesc::colourMatrix
    float slope[3], offset[3], power[3];
    float saturation, whitePoint;
    uint32_t curve, steps;                 // PTX_CURVE_*, GRADE_STEP_*
    const float *lut;                      // N^3 x 3 floats, or null without GRADE_STEP_LUT
    uint32_t lutSize;                      // N
};

PT_DEV f3 gradeMat3(const float *m, f3 c) // rows: (m[3i] x + m[3i+1] y) + m[3i+2] z
{
    return F3((m[0] * c.x + m[1] * c.y) + m[2] * c.z, (m[3] * c.x + m[4] * c.y) + m[5] * c.z, (m[6] * c.x + m[7] * c.y) + m[8] * c.z);
}

PT_DEV float curveReinhard(float v, float w2) { return div_(v * (1.0f + div_(v, w2)), 1.0f + v); }

PT_DEV float hableF(float x)
{
    const float A = PTX_HABLE_A, B = PTX_HABLE_B, C = PTX_HABLE_C, D = PTX_HABLE_D, E = PTX_HABLE_E, F = PTX_HABLE_F;
    return div_(x * (A * x + C * B) + D * E, x * (A * x + B) + D * F) - div_(E, F);
}
PT_DEV float curveHable(float v, float fWhite) { return div_(hableF(PTX_HABLE_EXPOSURE_BIAS * v), fWhite); }

PT_DEV float acesRational(float t)
{
    return div_(t * (t + PTX_ACES_A) - PTX_ACES_B, t * (PTX_ACES_C * t + PTX_ACES_D) + PTX_ACES_E);
}
PT_DEV f3 curveAcesFit(f3 v)
{
    const float in[9] = PTX_ACES_IN, out[9] = PTX_ACES_OUT;
    f3 t = gradeMat3(in, v);
    t = F3(acesRational(t.x), acesRational(t.y), acesRational(t.z));
    t = gradeMat3(out, t);
    return F3(clamp_(t.x, 0.0f, 1.0f), clamp_(t.y, 0.0f, 1.0f), clamp_(t.z, 0.0f, 1.0f));
}

// one axis of step 4: lattice index and fraction of x in [0, 1] (or NaN: index 0, fraction NaN)
PT_DEV void lutAxis(float x, uint32_t N, uint32_t &i, float &f)
{
    const float s = x * (float)(N - 1u);
    i = 0u;
    if (s >= 0.0f)
    {
        i = (uint32_t)__builtin_floorf(s);
        if (i > N - 2u)
            i = N - 2u;
    }
    f = s - (float)i;
}

PT_DEV f3 lutEntry(const float *__restrict__ lut, uint32_t at) { return F3(lut[at], lut[at + 1u], lut[at + 2u]); }

PT_DEV f3 lutTetrahedral(f3 v, const float *__restrict__ lut, uint32_t N, bool srgb)
{
    f3 x = F3(clamp_(v.x, 0.0f, 1.0f), clamp_(v.y, 0.0f, 1.0f), clamp_(v.z, 0.0f, 1.0f));
    if (srgb)
        x = F3(linearToSrgb(x.x), linearToSrgb(x.y), linearToSrgb(x.z));
    uint32_t ir, ig, ib;
    float fr, fg, fb;
    lutAxis(x.x, N, ir, fr);
    lutAxis(x.y, N, ig, fg);
    lutAxis(x.z, N, ib, fb);
    const uint32_t dr = 3u, dg = 3u * N, db = 3u * N * N; // one step along each axis, in floats
    const uint32_t base = ir * dr + ig * dg + ib * db;    // <= 3 (N^3 - 1) - (dr + dg + db): at most 823,872 at N = 65
    const f3 v000 = lutEntry(lut, base), v111 = lutEntry(lut, base + dr + dg + db);
    uint32_t da, dab; // the steps to V_a and V_b
    float hi, mid, lo;
    if (fr >= fg)
    {
        if (fg >= fb)      { hi = fr; mid = fg; lo = fb; da = dr; dab = dr + dg; } // rgb
        else if (fr >= fb) { hi = fr; mid = fb; lo = fg; da = dr; dab = dr + db; } // rbg
        else               { hi = fb; mid = fr; lo = fg; da = db; dab = db + dr; } // brg
    }
    else
    {
        if (fb >= fg)      { hi = fb; mid = fg; lo = fr; da = db; dab = db + dg; } // bgr
        else if (fb >= fr) { hi = fg; mid = fb; lo = fr; da = dg; dab = dg + db; } // gbr
        else               { hi = fg; mid = fr; lo = fb; da = dg; dab = dg + dr; } // grb
    }
    const f3 va = lutEntry(lut, base + da), vb = lutEntry(lut, base + dab);
    f3 out = ((v000 * (1.0f - hi) + va * (hi - mid)) + vb * (mid - lo)) + v111 * lo;
    if (srgb)
        out = F3(srgbToLinear(out.x), srgbToLinear(out.y), srgbToLinear(out.z));
    return out;
}

// steps 1 - 5 on the composed colour c of step 0
PT_DEV f3 gradePixel(f3 c, const GradeArgs &g)
{
    if (g.steps & GRADE_STEP_MATRIX)
        c = gradeMat3(g.m, c);
    if (g.steps & GRADE_STEP_SLOPE_OFFSET)
        c = F3(fmax_(c.x * g.slope[0] + g.offset[0], 0.0f), fmax_(c.y * g.slope[1] + g.offset[1], 0.0f), fmax_(c.z * g.slope[2] + g.offset[2], 0.0f));
    if (g.steps & GRADE_STEP_POWER)
        c = F3(pow_(c.x, g.power[0]), pow_(c.y, g.power[1]), pow_(c.z, g.power[2]));
    if (g.steps & GRADE_STEP_SATURATION)
    {
        const float Y = luminance_(c);
        c = F3(Y + (c.x - Y) * g.saturation, Y + (c.y - Y) * g.saturation, Y + (c.z - Y) * g.saturation);
    }
    if (g.steps & GRADE_STEP_CURVE)
    {
        if (g.curve == PTX_CURVE_REFERENCE)
            c = toneMapPixel(c, PTX_TONE_MAPPING_SDR);
        else if (g.curve == PTX_CURVE_REINHARD)
        {
            const float w2 = g.whitePoint * g.whitePoint;
            c = F3(curveReinhard(c.x, w2), curveReinhard(c.y, w2), curveReinhard(c.z, w2));
        }
        else if (g.curve == PTX_CURVE_HABLE)
        {
            const float fWhite = hableF(PTX_HABLE_WHITE);
            c = F3(curveHable(c.x, fWhite), curveHable(c.y, fWhite), curveHable(c.z, fWhite));
        }
        else
            c = curveAcesFit(c);
    }
    if (g.steps & GRADE_STEP_LUT)
        c = lutTetrahedral(c, g.lut, g.lutSize, (g.steps & GRADE_STEP_LUT_SRGB) != 0u);
    return f16Round(c);
}

// the tone step of composeStore (pt_post.hpp) and presentPixel (pt_present.hpp): gradePixel rounds by itself
struct Grade
{
    const GradeArgs &g;
    PT_DEV f3 operator()(f3 c) const { return gradePixel(c, g); }
};

__global__ void k_compose_grade(const float *__restrict__ post, const float *__restrict__ bloom0, uint32_t n, PtxPostProcessingUniformData u, GradeArgs g,
                                float4 *__restrict__ out)
{
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
        composeStore(post, bloom0, i, u, Grade{ g }, out);
}

// the blit's store is step 0; the host leaves the curve and the LUT out of g.steps in the HDR mode
template <uint32_t FORMAT, bool HDR> __global__ void __launch_bounds__(kPresentBlock) k_present_graded(PresentArgs a, GradeArgs g)
{
    presentPixel<FORMAT, HDR>(a, Grade{ g });
}

} // namespace ptd
