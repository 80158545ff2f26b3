// pt_denoise.hpp -- the denoiser (docs/NEXT_ROWS.md section 13): the one stage the reference does not have (it relies on accumulation;
// DESIGN.md section 9 names this exception).  Three kernels, host side in pt_chain_host.hpp:
//
//   k_render_guides  one primary ray through the centre of every owned pixel, exactly the debug view's (debugViewBody,
//                    pt_debug_view.hpp), storing the first hit's shading normal, world position + hit distance and base colour;
//                    <MODE, true> (ptx_render_guides_motion, docs/NEXT_ROWS.md section 17) also where the hit was, and which way its
//                    normal pointed, in the pose the temporal history was made from
//   k_render_guides_specular  the same pass following mirrors and glass to the first surface that is neither, storing that surface's
//                    guides and, in a fourth image, the first hit and the chain's length and class (ptx_render_guides_specular,
//                    docs/NEXT_ROWS.md section 18)
//   k_denoise        one iteration of the edge-avoiding a-trous filter (a 5 x 5 B3-spline stencil dilated by `step`) over the
//                    demodulated mean, guided by those three images; the first launch demodulates, the last remodulates
//
// The arithmetic is float32 and nothing here is compared with an oracle bit for bit: the filter's weights use the hardware's
// exp2 (v_exp_f32) with the log2(e) factor folded into the exponent.
#pragma once

#include "pt_wavefront.hpp"

// ---- the guide pass ----------------------------------------------------------------------------------------

// What k_render_guides<MODE, true> gets beside the scene: the pose the renderer's temporal history was made from, and the two images
// it writes.  A kernel argument of its own -- SceneView and TraceScene do not grow for a pass most launches never run.
struct PrevPose
{
    const DevPair *pairs;      // the DevPair table of that pose: the scene's own, or the snapshot ptx_update_animation kept
    const PtxVertex *skinned;  // vertices[firstSkinned ...] of that pose; nullptr: the vertex buffer itself holds them
    uint32_t firstSkinned;     // the first index of the vertex buffer that k_skin writes
    uint32_t known;            // 0: the pose is not known; the images hold (x_p, 0) and (n_p, 0) on hits
    float4 *position, *normal; // PTX_MOTION_POSITION, PTX_MOTION_NORMAL
};

// The hit's surface point and shading normal in the previous pose.  The triangle is found through (pair, prim), never through the
// slot: a rebuild between the two poses reorders slots.  Vertices as writeShadeTri fetches them, then renderGuidesBody's own
// expressions in its order -- where neither the pair's transform nor its vertices changed, the same operations on the same bits.
PT_DEV void motionGuides(const SceneView &sv, const PrevPose &prev, const Hit &h, f3 bary, f3 materialNormal, float4 gp, float4 gn, float4 &mx,
                         float4 &mn)
{
    if (!prev.known)
    {
        mx = make_float4(gp.x, gp.y, gp.z, 0.0f);
        mn = make_float4(gn.x, gn.y, gn.z, 0.0f);
        return;
    }
    const DevPair pr = prev.pairs[h.pair];
    Vtx o[3];
    for (int k = 0; k < 3; k++)
    {
        const uint32_t vi = pr.vertexOffset + sv.indices[pr.indexOffset + h.prim * 3 + k];
        o[k] = loadVertex(prev.skinned && vi >= prev.firstSkinned ? &prev.skinned[vi - prev.firstSkinned] : &sv.vertices[vi]);
    }
    Vtx ov;
    ov.Position = interp3(o[0].Position, o[1].Position, o[2].Position, bary);
    ov.Normal = interp3(o[0].Normal, o[1].Normal, o[2].Normal, bary);
    ov.Tangent = interp3(o[0].Tangent, o[1].Tangent, o[2].Tangent, bary);
    ov.Bitangent = interp3(o[0].Bitangent, o[1].Bitangent, o[2].Bitangent, bary);
    const Vtx vertex = transformVertex(pr, ov);
    mat3 TBN;
    TBN.c0 = vertex.Tangent;
    TBN.c1 = vertex.Bitangent;
    TBN.c2 = vertex.Normal;
    const f3 N = normalize(vertex.Normal + mul(TBN, materialNormal));
    mx = make_float4(vertex.Position.x, vertex.Position.y, vertex.Position.z, 1.0f);
    mn = make_float4(N.x, N.y, N.z, 1.0f);
}

// debugRaygen.rgen:22-40 + debugClosestHit.rchit:164-202 without flags: the values of the debug view's Normal and WorldPosition
// modes and the material's colour after the decal mix, from ONE traversal.  Every expression is the debug view's, in its order:
// the normal and position images are the same bits as ptx_render_debug's.
//
// MOTION (ptx_render_guides_motion, docs/NEXT_ROWS.md section 17): two more images from the same traversal -- where the hit's
// surface point was and which way its normal pointed in the pose `prev` describes (motionGuides above).
template <int MODE, bool MOTION = false>
PT_DEV void renderGuidesBody(const LaunchParams &p, const SceneView &sv, const TraceScene &sc, float4 *__restrict__ gNormal,
                             float4 *__restrict__ gPosition, float4 *__restrict__ gAlbedo, uint32_t *__restrict__ counters, uint32_t *spill,
                             const PrevPose *prev = nullptr)
{
    constexpr bool TEX = MODE >= 1, ALPHA = MODE == 2;
    PT_DECLARE_STACK(st, PT_TAIL_LDS, spill)
    uint32_t nPix = 0;
    for (uint32_t s = blockIdx.x * blockDim.x + threadIdx.x; s < p.slotsPerFrame; s += gridDim.x * blockDim.x)
    {
        const uint32_t pixel = slotPixel(p, s);
        if (pixel == kNoPixel)
            continue;
        f3 ro, rd, rx, ry;
        constructPrimaryRay<true>(pixel % p.width, pixel / p.width, p.width, p.height, p.u.ViewInverse, p.u.ProjInverse, F2(0.5f, 0.5f), ro, rd, rx, ry);
        Hit h;
        Decal decal = noDecal();
        nPix++;
        const bool hit = traceRay<false, false, ALPHA>(sc, ro, rd, 0.00001f, 10000.0f, st, h, nullptr, nullptr, ALPHA ? &decal : nullptr);
        float4 gn = make_float4(0.0f, 0.0f, 0.0f, 0.0f), gp = gn, ga = make_float4(1.0f, 1.0f, 1.0f, 1.0f);
        float4 mx = gn, mn = gn; // MOTION: a miss stores zeros
        if (hit)
        {
            const f3 bary = F3(1.0f - h.u - h.v, h.u, h.v);
            const DevPair pr = sv.pairs[h.pair];
            const TriVertices tv3 = loadTriangle(&sv.shadeTris[h.slot]);
            Vtx ov;
            ov.Position = interp3(tv3.o[0].Position, tv3.o[1].Position, tv3.o[2].Position, bary);
            ov.Normal = interp3(tv3.o[0].Normal, tv3.o[1].Normal, tv3.o[2].Normal, bary);
            ov.Tangent = interp3(tv3.o[0].Tangent, tv3.o[1].Tangent, tv3.o[2].Tangent, bary);
            ov.Bitangent = interp3(tv3.o[0].Bitangent, tv3.o[1].Bitangent, tv3.o[2].Bitangent, bary);
            const Vtx vertex = transformVertex(pr, ov);
            const f2 uv0 = tv3.uv[0], uv1 = tv3.uv[1], uv2 = tv3.uv[2];
            const f2 texCoords = F2((uv0.x * bary.x + uv1.x * bary.y) + uv2.x * bary.z, (uv0.y * bary.x + uv1.y * bary.y) + uv2.y * bary.z);
            const f3 P3[3] = { tv3.worldPosition[0], tv3.worldPosition[1], tv3.worldPosition[2] };
            const f3 N3[3] = { tv3.worldNormal[0], tv3.worldNormal[1], tv3.worldNormal[2] };
            const f2 UV3[3] = { uv0, uv1, uv2 };
            f3 dpdu, dpdv, dndu, dndv, dpdx, dpdy;
            computeDpnDuv(P3, N3, UV3, vertex.Tangent, vertex.Bitangent, dpdu, dpdv, dndu, dndv);
            computeDpDxy(vertex.Position, ro, rx, ro, ry, vertex.Normal, dpdx, dpdy);
            const f4 derivatives = computeDerivatives(dpdx, dpdy, dpdu, dpdv);
            MaterialSample material = sampleMaterial<TEX>(sv, pr.materialId, texCoords, derivatives, false, false, false);
            if (ALPHA && decal.dist != -1.0f && h.t > decal.dist)
            {
                const f4 c = hitBaseColor(sv, decal.pair, decal.slot, decal.u, decal.v);
                material.Color = mix(material.Color, rgb(c), c.w);
            }
            mat3 TBN;
            TBN.c0 = vertex.Tangent;
            TBN.c1 = vertex.Bitangent;
            TBN.c2 = vertex.Normal;
            const f3 N = normalize(vertex.Normal + mul(TBN, material.Normal));
            gn = make_float4(N.x, N.y, N.z, 1.0f);
            gp = make_float4(vertex.Position.x, vertex.Position.y, vertex.Position.z, h.t);
            ga = make_float4(material.Color.x, material.Color.y, material.Color.z, 1.0f);
            if constexpr (MOTION)
                motionGuides(sv, *prev, h, bary, material.Normal, gp, gn, mx, mn);
        }
        gNormal[pixel] = gn;
        gPosition[pixel] = gp;
        gAlbedo[pixel] = ga;
        if constexpr (MOTION)
        {
            prev->position[pixel] = mx;
            prev->normal[pixel] = mn;
        }
    }
    if (st.overflow)
        atomicAdd(&counters[C_OVERFLOW], 1u);
    waveAddCounter(&counters[C_SEGMENTS], nPix);
    waveAddCounter(&counters[C_SAMPLES], nPix);
}

// k_debug_view's class of kernel (the sampler and a traversal) and its occupancy attribute; register and scratch figures of the
// three variants: docs/NEXT_ROWS.md section 13.
#ifndef PT_GUIDES_ATTR
#define PT_GUIDES_ATTR __attribute__((amdgpu_waves_per_eu(2, 2)))
#endif
// MOTION adds one trailing argument, the PrevPose: the pack is empty for the plain pass, whose argument list stays what it was.
template <int MODE, bool MOTION = false, class... Prev>
__global__ void __launch_bounds__(kBlock) k_render_guides(LaunchParams p, SceneView sv, TraceScene sc, float4 *gNormal, float4 *gPosition,
                                                           float4 *gAlbedo, uint32_t *counters, uint32_t *spill, Prev... prev);
#define PT_GUIDES_KERNEL(MODE)                                                                                                          \
    template <>                                                                                                                         \
    __global__ void __launch_bounds__(kBlock) PT_GUIDES_ATTR k_render_guides<MODE>(LaunchParams p, SceneView sv, TraceScene sc, float4 *gNormal, \
                                                                                   float4 *gPosition, float4 *gAlbedo, uint32_t *counters,  \
                                                                                   uint32_t *spill)                                      \
    {                                                                                                                                   \
        renderGuidesBody<MODE>(p, sv, sc, gNormal, gPosition, gAlbedo, counters, spill);                                                \
    }                                                                                                                                   \
    template <>                                                                                                                         \
    __global__ void __launch_bounds__(kBlock) PT_GUIDES_ATTR k_render_guides<MODE, true>(LaunchParams p, SceneView sv, TraceScene sc,      \
                                                                                         float4 *gNormal, float4 *gPosition, float4 *gAlbedo, \
                                                                                         uint32_t *counters, uint32_t *spill, PrevPose prev) \
    {                                                                                                                                   \
        renderGuidesBody<MODE, true>(p, sv, sc, gNormal, gPosition, gAlbedo, counters, spill, &prev);                                   \
    }
PT_GUIDES_KERNEL(0)
PT_GUIDES_KERNEL(1)
PT_GUIDES_KERNEL(2)
#undef PT_GUIDES_KERNEL

// ---- the specular-chain guide pass (ptx_render_guides_specular, docs/NEXT_ROWS.md section 18) ---------------

// What one lane carries from hit to hit: the ray, its offset rays (TEX variants), the summed length, the product of the mirrors'
// reflections (rows: (M v)_i = dot(m_i, v)), the product of the followed surfaces' colours.
struct SpecularChain
{
    f3 o, d;
    DiffRays diff;
    float T;
    f3 m0, m1, m2;
    f3 tint;
    uint32_t bounces;
};

// The hit as steps 1 and 2 of the header text shade it.  bounces == 0: renderGuidesBody's expressions in its order (the footprint from
// the unflipped frame and the primary's offset rays); later: closestHit's (pt_device.hpp), which flips the frame first where the
// hit is from inside.  `vertex` comes back unflipped; nGuide, nCont and the footprint's by-products go to the continuation.
struct SpecularHit
{
    Vtx vertex;
    TriVertices tri;
    f3 bary, geometricNormal; // the normal facing the ray
    bool inside;
    MaterialSample material;
    f4 derivatives;
    f3 dndu, dndv;
    f3 nGuide, nCont;
};

template <bool TEX, bool ALPHA>
PT_DEV void specularShadeHit(const SceneView &sv, const SpecularChain &c, const Hit &h, const Decal &decal, SpecularHit &s)
{
    s.bary = F3(1.0f - h.u - h.v, h.u, h.v);
    const DevPair pr = sv.pairs[h.pair];
    s.tri = loadTriangle(&sv.shadeTris[h.slot]);
    const TriVertices &tv3 = s.tri;
    Vtx ov;
    ov.Position = interp3(tv3.o[0].Position, tv3.o[1].Position, tv3.o[2].Position, s.bary);
    ov.Normal = interp3(tv3.o[0].Normal, tv3.o[1].Normal, tv3.o[2].Normal, s.bary);
    ov.Tangent = interp3(tv3.o[0].Tangent, tv3.o[1].Tangent, tv3.o[2].Tangent, s.bary);
    ov.Bitangent = interp3(tv3.o[0].Bitangent, tv3.o[1].Bitangent, tv3.o[2].Bitangent, s.bary);
    s.vertex = transformVertex(pr, ov);
    s.inside = dot(tv3.geometricNormal, c.d) > 0.0f;
    s.geometricNormal = s.inside ? -tv3.geometricNormal : tv3.geometricNormal;
    Vtx flipped = s.vertex; // the continuation's frame
    if (s.inside)
    {
        flipped.Normal = -flipped.Normal;
        flipped.Tangent = -flipped.Tangent;
        flipped.Bitangent = -flipped.Bitangent;
    }
    const Vtx &fp = c.bounces ? flipped : s.vertex; // the footprint's frame: the plain pass flips nothing
    const f2 uv0 = tv3.uv[0], uv1 = tv3.uv[1], uv2 = tv3.uv[2];
    const f2 texCoords = F2((uv0.x * s.bary.x + uv1.x * s.bary.y) + uv2.x * s.bary.z, (uv0.y * s.bary.x + uv1.y * s.bary.y) + uv2.y * s.bary.z);
    const f3 P3[3] = { tv3.worldPosition[0], tv3.worldPosition[1], tv3.worldPosition[2] };
    const f3 N3[3] = { tv3.worldNormal[0], tv3.worldNormal[1], tv3.worldNormal[2] };
    const f2 UV3[3] = { uv0, uv1, uv2 };
    f3 dpdu, dpdv, dpdx, dpdy;
    computeDpnDuv(P3, N3, UV3, fp.Tangent, fp.Bitangent, dpdu, dpdv, s.dndu, s.dndv);
    computeDpDxy(s.vertex.Position, c.diff.rxOrigin, c.diff.rxDirection, c.diff.ryOrigin, c.diff.ryDirection, fp.Normal, dpdx, dpdy);
    s.derivatives = computeDerivatives(dpdx, dpdy, dpdu, dpdv);
    s.material = sampleMaterial<TEX>(sv, pr.materialId, texCoords, s.derivatives, s.inside, false, false);
    if (ALPHA && decal.dist != -1.0f && h.t > decal.dist)
    {
        const f4 dc = hitBaseColor(sv, decal.pair, decal.slot, decal.u, decal.v);
        s.material.Color = mix(s.material.Color, rgb(dc), dc.w);
    }
    mat3 TBN;
    TBN.c0 = s.vertex.Tangent;
    TBN.c1 = s.vertex.Bitangent;
    TBN.c2 = s.vertex.Normal;
    s.nGuide = normalize(s.vertex.Normal + mul(TBN, s.material.Normal));
    s.nCont = s.inside ? -s.nGuide : s.nGuide; // the flipped frame negates every term of the sum: the same bits, negated
}

// Step 4 of the header text: the continuation ray of a hit that is followed -- mirror, refraction, or total internal reflection (a
// mirror that leaves the tint alone).  The offset rays follow as closestHit propagates them.
template <bool TEX>
PT_DEV void specularContinue(SpecularChain &c, const SpecularHit &s, float t)
{
    const TriVertices &tv3 = s.tri;
    const f3 flippedNormal = s.inside ? -s.vertex.Normal : s.vertex.Normal;
    f3 r = F3s(0.0f);
    const bool glass = !(s.material.Metalness >= 0.5f);
    if (glass)
        r = refract(c.d, s.nCont, s.material.Eta);
    const bool refracted = glass && !(r.x == 0.0f && r.y == 0.0f && r.z == 0.0f);
    const f3 rayOrigin = offsetRayOriginShadowTerminator(s.vertex.Position, tv3.worldPosition[0], tv3.worldNormal[0], tv3.worldPosition[1], tv3.worldNormal[1],
                                                         tv3.worldPosition[2], tv3.worldNormal[2], s.bary, refracted);
    f3 dir, origin;
    if (refracted)
    {
        dir = normalize(r);
        origin = offsetRayOriginSelfIntersection(s.vertex.Position, -s.geometricNormal);
        c.tint = c.tint * s.material.Color;
    }
    else
    {
        dir = normalize(reflect(c.d, s.nCont));
        origin = rayOrigin;
        if (!glass)
            c.tint = c.tint * s.material.Color;
        const f3 n = s.nCont; // M <- M (I - 2 n n^T)
        const float a0 = 2.0f * dot(c.m0, n), a1 = 2.0f * dot(c.m1, n), a2 = 2.0f * dot(c.m2, n);
        c.m0 = c.m0 - n * a0;
        c.m1 = c.m1 - n * a1;
        c.m2 = c.m2 - n * a2;
    }
    if constexpr (TEX)
    {
        if (refracted)
            computeRefractedDifferentialRays(s.derivatives, flippedNormal, rayOrigin, -c.d, dir, s.dndu, s.dndv, s.material.Eta, c.diff);
        else
            computeReflectedDifferentialRays(s.derivatives, flippedNormal, rayOrigin, -c.d, dir, s.dndu, s.dndv, c.diff);
    }
    c.o = origin;
    c.d = dir;
    c.T = c.T + t;
    c.bounces++;
}

// One traversal and one shading site, run once per segment: the primary ray enters the loop like every continuation ray, so a lane
// whose chain ended waits, results in registers, until the wave's longest chain is done, and stores once.
template <int MODE>
PT_DEV void renderGuidesSpecularBody(const LaunchParams &p, const SceneView &sv, const TraceScene &sc, float4 *__restrict__ gNormal,
                                     float4 *__restrict__ gPosition, float4 *__restrict__ gAlbedo, float4 *__restrict__ gSurface, uint32_t maxBounces,
                                     float roughnessMax, uint32_t *__restrict__ counters, uint32_t *spill)
{
    constexpr bool TEX = MODE >= 1, ALPHA = MODE == 2;
    PT_DECLARE_STACK(st, PT_TAIL_LDS, spill)
    uint32_t nPix = 0, nRays = 0;
    for (uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x; slot < p.slotsPerFrame; slot += gridDim.x * blockDim.x)
    {
        const uint32_t pixel = slotPixel(p, slot);
        if (pixel == kNoPixel)
            continue;
        f3 ro, rd, rx, ry;
        constructPrimaryRay<true>(pixel % p.width, pixel / p.width, p.width, p.height, p.u.ViewInverse, p.u.ProjInverse, F2(0.5f, 0.5f), ro, rd, rx, ry);
        SpecularChain c;
        c.o = ro;
        c.d = rd;
        c.diff.rxOrigin = ro;
        c.diff.rxDirection = rx;
        c.diff.ryOrigin = ro;
        c.diff.ryDirection = ry;
        c.T = 0.0f;
        c.m0 = F3(1.0f, 0.0f, 0.0f);
        c.m1 = F3(0.0f, 1.0f, 0.0f);
        c.m2 = F3(0.0f, 0.0f, 1.0f);
        c.tint = F3s(1.0f);
        c.bounces = 0u;
        nPix++;
        float4 gn = make_float4(0.0f, 0.0f, 0.0f, 0.0f), gp = gn, gs = gn, ga = make_float4(1.0f, 1.0f, 1.0f, 1.0f);
        for (;;)
        {
            Hit h;
            Decal decal = noDecal();
            nRays++;
            if (!traceRay<false, false, ALPHA>(sc, c.o, c.d, 0.00001f, 10000.0f, st, h, nullptr, nullptr, ALPHA ? &decal : nullptr))
            {
                if (c.bounces) // escaped: a miss to every consumer
                    gs.w = (float)c.bounces + 32.0f;
                break;
            }
            SpecularHit s;
            specularShadeHit<TEX, ALPHA>(sv, c, h, decal, s);
            if (c.bounces == 0u)
                gs = make_float4(s.vertex.Position.x, s.vertex.Position.y, s.vertex.Position.z, 0.0f);
            const bool followed = s.material.Roughness <= roughnessMax && (s.material.Metalness >= 0.5f || s.material.Transmission >= 0.5f);
            if (c.bounces == maxBounces || !followed)
            {
                if (c.bounces == 0u) // the plain pass's values, bit for bit
                {
                    gn = make_float4(s.nGuide.x, s.nGuide.y, s.nGuide.z, 1.0f);
                    gp = make_float4(s.vertex.Position.x, s.vertex.Position.y, s.vertex.Position.z, h.t);
                    ga = make_float4(s.material.Color.x, s.material.Color.y, s.material.Color.z, 1.0f);
                }
                else
                {
                    const float T = c.T + h.t;
                    const f3 x = ro + normalize(rd) * T;
                    const f3 al = c.tint * s.material.Color;
                    gn = make_float4(dot(c.m0, s.nGuide), dot(c.m1, s.nGuide), dot(c.m2, s.nGuide), 1.0f);
                    gp = make_float4(x.x, x.y, x.z, T);
                    ga = make_float4(al.x, al.y, al.z, 1.0f);
                }
                gs.w = (float)c.bounces + (followed ? 16.0f : 0.0f);
                break;
            }
            specularContinue<TEX>(c, s, h.t);
        }
        gNormal[pixel] = gn;
        gPosition[pixel] = gp;
        gAlbedo[pixel] = ga;
        gSurface[pixel] = gs;
    }
    if (st.overflow)
        atomicAdd(&counters[C_OVERFLOW], 1u);
    waveAddCounter(&counters[C_SEGMENTS], nRays);
    waveAddCounter(&counters[C_SAMPLES], nPix);
}

// The plain pass's class of kernel and its occupancy attribute; register and scratch figures: docs/NEXT_ROWS.md section 18.
template <int MODE>
__global__ void __launch_bounds__(kBlock) k_render_guides_specular(LaunchParams p, SceneView sv, TraceScene sc, float4 *gNormal, float4 *gPosition,
                                                                    float4 *gAlbedo, float4 *gSurface, uint32_t maxBounces, float roughnessMax,
                                                                    uint32_t *counters, uint32_t *spill);
#define PT_GUIDES_SPECULAR_KERNEL(MODE)                                                                                                 \
    template <>                                                                                                                         \
    __global__ void __launch_bounds__(kBlock) PT_GUIDES_ATTR k_render_guides_specular<MODE>(                                            \
        LaunchParams p, SceneView sv, TraceScene sc, float4 *gNormal, float4 *gPosition, float4 *gAlbedo, float4 *gSurface, uint32_t maxBounces, \
        float roughnessMax, uint32_t *counters, uint32_t *spill)                                                                         \
    {                                                                                                                                   \
        renderGuidesSpecularBody<MODE>(p, sv, sc, gNormal, gPosition, gAlbedo, gSurface, maxBounces, roughnessMax, counters, spill);     \
    }
PT_GUIDES_SPECULAR_KERNEL(0)
PT_GUIDES_SPECULAR_KERNEL(1)
PT_GUIDES_SPECULAR_KERNEL(2)
#undef PT_GUIDES_SPECULAR_KERNEL

// ---- the filter --------------------------------------------------------------------------------------------

struct DenoiseArgs
{
    const float4 *sum;      // the accumulation image (running sum)
    const float4 *src;      // c_i of the previous launch: rgb, w = 1 on a valid pixel and 0 elsewhere (unused by the first launch)
    float4 *dst;            // c_{i+1} in the same form, or the denoised mean with alpha 1 (the last launch)
    const float4 *normal;   // the guides
    const float4 *position;
    const float4 *albedo;
    uint32_t width, height;
    int32_t step;           // 2^i
    float totalSamples;
    float invSigmaColor2;   // 1 / (sigmaColor 2^-i)^2; 0: no colour term
    float invSigmaNormal2;  // 1 / sigmaNormal^2
    float invSigmaPosition; // 1 / sigmaPosition
};

constexpr int kDenoiseTileX = 32, kDenoiseTileY = 8; // 256 threads; a row of the tile is 512 contiguous bytes of every image

PT_DEV bool finite_(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }
PT_DEV bool finite3_(f3 c) { return finite_(c.x) && finite_(c.y) && finite_(c.z); }
PT_DEV f3 albedoFloor(float4 a) { return F3(fmax_(a.x, 0.01f), fmax_(a.y, 0.01f), fmax_(a.z, 0.01f)); }
PT_DEV bool denoiseValid(f3 mean, float4 n, float t)
{
    return n.w == 1.0f && finite3_(mean) && finite_(n.x) && finite_(n.y) && finite_(n.z) && t > 0.0f && finite_(t);
}

// c_0 of pixel q: the mean, divided by the floored albedo where the pixel is valid
PT_DEV f3 denoiseInput(const DenoiseArgs &a, uint32_t q, float4 nq, float tq, bool &valid)
{
    const float4 s = a.sum[q];
    const f3 mean = F3(s.x, s.y, s.z) / a.totalSamples;
    valid = denoiseValid(mean, nq, tq);
    if (!valid)
        return mean;
    const f3 al = albedoFloor(a.albedo[q]);
    return F3(div_(mean.x, al.x), div_(mean.y, al.y), div_(mean.z, al.z));
}

// One tap that passed the tests on q itself (inside the image, valid, finite colour): its weight, and its share of the sums
PT_DEV void denoiseTap(const DenoiseArgs &a, f3 cp, f3 nP, f3 xP, float invDepth, f3 cq, float4 nq, float4 xq, float hh, f3 &acc, float &wsum)
{
    const f3 dn = nP - F3(nq.x, nq.y, nq.z);
    const float plane = dot(nP, F3(xq.x, xq.y, xq.z) - xP) * invDepth;
    float e = dot(dn, dn) * a.invSigmaNormal2 + plane * plane;
    if (a.invSigmaColor2 != 0.0f)
    {
        const f3 dc = cp - cq;
        e = dot(dc, dc) * a.invSigmaColor2 + e;
    }
    if (!(e >= 0.0f)) // a NaN
        return;
    const float w = hh * __builtin_amdgcn_exp2f(e * -1.44269504f);
    acc = acc + cq * w;
    wsum = wsum + w;
}

PT_DEV void denoiseStore(const DenoiseArgs &a, uint32_t p, f3 out, bool valid, bool last)
{
    if (last)
    {
        if (valid)
            out = out * albedoFloor(a.albedo[p]);
        a.dst[p] = make_float4(out.x, out.y, out.z, 1.0f);
    }
    else
        a.dst[p] = make_float4(out.x, out.y, out.z, valid ? 1.0f : 0.0f);
}

// One thread per pixel.  A tap costs 16 B of colour and, where that says the pixel is valid, 32 B of normal and position; the
// first launch also reads the sum and the albedo of every tap.  Nothing is staged in LDS: the 25 taps of neighbouring threads
// overlap in L1 / L2 (docs/NEXT_ROWS.md section 13, cost).
template <bool FIRST, bool LAST>
__global__ void __launch_bounds__(kDenoiseTileX *kDenoiseTileY) k_denoise(DenoiseArgs a)
{
    const int x = (int)(blockIdx.x * kDenoiseTileX + threadIdx.x), y = (int)(blockIdx.y * kDenoiseTileY + threadIdx.y);
    if (x >= (int)a.width || y >= (int)a.height)
        return;
    const uint32_t p = (uint32_t)y * a.width + (uint32_t)x;
    const float4 np = a.normal[p];
    const float4 xp = a.position[p];
    bool valid;
    f3 cp;
    if (FIRST)
        cp = denoiseInput(a, p, np, xp.w, valid);
    else
    {
        const float4 c = a.src[p];
        cp = F3(c.x, c.y, c.z);
        valid = c.w != 0.0f;
    }
    f3 out = cp;
    if (valid)
    {
        const float hk[5] = { 0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f };
        const float invDepth = a.invSigmaPosition * rcp_(xp.w);
        const f3 nP = F3(np.x, np.y, np.z), xP = F3(xp.x, xp.y, xp.z);
        f3 acc = cp * (0.375f * 0.375f); // the centre tap, by rule
        float wsum = 0.375f * 0.375f;
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
                float4 nq, xq;
                f3 cq;
                bool qValid;
                if (FIRST)
                {
                    nq = a.normal[q];
                    xq = a.position[q];
                    cq = denoiseInput(a, q, nq, xq.w, qValid);
                }
                else
                {
                    const float4 c = a.src[q];
                    cq = F3(c.x, c.y, c.z);
                    qValid = c.w != 0.0f;
                }
                if (!qValid || !finite3_(cq))
                    continue;
                if (!FIRST)
                {
                    nq = a.normal[q];
                    xq = a.position[q];
                }
                denoiseTap(a, cp, nP, xP, invDepth, cq, nq, xq, hk[dx + 2] * hk[dy + 2], acc, wsum);
            }
        }
        out = acc * rcp_(wsum);
    }
    denoiseStore(a, p, out, valid, LAST);
}
