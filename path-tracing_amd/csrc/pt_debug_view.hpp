// pt_debug_view.hpp -- the debug ray-tracing pipeline (row D16): Shaders/Debug/debugRaygen.rgen, debugAnyhit.rahit, debugMiss.rmiss
// and debugClosestHit.rchit restated as ONE kernel (host side: renderDebug / testDebugEval in pt_runtime.hpp).
//
// The reference binds this pipeline instead of the path tracer's for its interactive preview
// (Renderer::SetDebugRaytracingPipeline, Renderer.cpp:579-610, :769-772): every pixel casts one primary ray through its centre,
// shades the hit with rasteriser-style direct light (ambient + a Cook-Torrance term per light, each behind its own shadow ray)
// or shows one attribute of the hit, and OVERWRITES the image.  Everything it shares with the path tracer is the path tracer's
// code (pt_device.hpp, pt_bvh.hpp); what is restated here is what only this stage has.
#pragma once

#include "pt_wavefront.hpp"

struct DebugView // the specialisation constants of the four shaders (DebugShaderTypes.incl:13-39) as kernel arguments
{
    uint32_t renderMode;    // s_RenderMode, PTX_DEBUG_MODE_*
    uint32_t raygenFlags;   // s_RaygenFlags; CullBackFaces selects the kernel variant too
    uint32_t hitGroupFlags; // s_HitGroupFlags; DxNormalTextures is SceneView::dxNormalTextures
};

// ---- debugClosestHit.rchit:71-141 ------------------------------------------------------------------------

constexpr float kDebugPi = 3.14159265359f; // common.glsl:3

PT_DEV float debugDistributionGGX(f3 N, f3 H, float roughness) // :71-83
{
    const float a = roughness * roughness;
    const float a2 = a * a;
    const float NdotH = fmax_(dot(N, H), 0.0f);
    const float NdotH2 = NdotH * NdotH;
    float denom = NdotH2 * (a2 - 1.0f) + 1.0f;
    denom = (kDebugPi * denom) * denom;
    return div_(a2, fmax_(denom, 0.0001f));
}

PT_DEV float debugGeometrySchlickGGX(float NdotV, float roughness) // :85-94
{
    const float r = roughness + 1.0f;
    const float k = div_(r * r, 8.0f);
    return div_(NdotV, NdotV * (1.0f - k) + k);
}

PT_DEV float debugGeometrySmith(f3 N, f3 V, f3 L, float roughness) // :96-104
{
    const float NdotV = fmax_(dot(N, V), 0.0f);
    const float NdotL = fmax_(dot(N, L), 0.0f);
    const float ggx2 = debugGeometrySchlickGGX(NdotV, roughness);
    const float ggx1 = debugGeometrySchlickGGX(NdotL, roughness);
    return ggx1 * ggx2;
}

PT_DEV f3 debugFresnelSchlick(float cosTheta, f3 F0) // :106-109, pow(x, 5) in the product form of SchlickFresnel
{
    const float x = clamp_(1.0f - cosTheta, 0.0f, 1.0f);
    const float x2 = x * x;
    return F0 + (F3s(1.0f) - F0) * (x2 * x2 * x);
}

// DDDcomputeLightContribution, :111-141 (its `position` argument and the reflection vector R are unused there)
PT_DEV f3 debugLightContribution(f3 lightDir, f3 lightColor, float attenuation, f3 V, f3 N, f3 color, float roughness, float metalness)
{
    const f3 L = -normalize(lightDir);
    const f3 H = normalize(V + L);
    const f3 radiance = lightColor * attenuation;
    const f3 F0 = mix(F3s(0.04f), color, metalness);
    const float NDF = debugDistributionGGX(N, H, roughness);
    const float G = debugGeometrySmith(N, V, L, roughness);
    const f3 F = debugFresnelSchlick(fmax_(dot(H, V), 0.0f), F0);
    const f3 numerator = F * (NDF * G);
    const float denominator = (4.0f * fmax_(dot(N, V), 0.0f)) * fmax_(dot(N, L), 0.0f);
    const f3 specular = numerator / fmax_(denominator, 0.0001f);
    f3 kD = F3s(1.0f) - F;
    kD = kD * (1.0f - metalness);
    const float NdotL = fmax_(dot(N, L), 0.0f);
    return (((kD * color) / kDebugPi + specular) * radiance) * NdotL;
}

// :143-162
PT_DEV uint32_t debugHash(uint32_t x)
{
    x *= 0x1eca7d79u;
    x ^= x >> 20;
    x = (x << 8) | (x >> 24);
    x = ~x;
    x ^= x << 5;
    x += 0x10afe4e7u;
    return x;
}
PT_DEV f3 debugRandomColor(uint32_t x)
{
    const uint32_t rand = debugHash(x);
    return F3(div_((float)((rand & 0xff000000u) >> 24), 255.0f), div_((float)((rand & 0x00ff0000u) >> 16), 255.0f),
              div_((float)((rand & 0x0000ff00u) >> 8), 255.0f));
}

// ---- debugMiss.rmiss:18-37 -------------------------------------------------------------------------------

PT_DEV f3 debugMissColor(const SceneView &sv, f3 rayDir)
{
    if (sv.skyKind == PTX_SKYBOX_2D)
        return skybox2DLookup(sv, rayDir); // :29, no hdrToLdr here
    if (sv.skyKind == PTX_SKYBOX_CUBE)
        return rgb(sampleCube(sv.tex, sv.tex.textures + sv.tex.textureCount, rayDir)); // :33 = miss.rmiss:32
    return F3(0.2f, 0.2f, 0.2f); // :36
}

// ---- debugClosestHit.rchit:164-266 -----------------------------------------------------------------------

struct DebugCounters
{
    uint32_t nSeg = 0, nShadow = 0, nPix = 0;
};

// checkOccluded, :57-69: the pipeline's occlusion hit group is the path tracer's (Renderer.cpp:584-589)
template <bool ALPHA>
PT_DEV bool debugOccluded(const TraceScene &sc, Stack &st, f3 lightDir, f3 position, float dist, DebugCounters &dc)
{
    Hit sh;
    dc.nShadow++;
    return traceRay<true, false, ALPHA>(sc, position, -normalize(lightDir), 0.00001f, dist, st, sh);
}

template <int MODE>
PT_DEV f4 debugClosestHit(const SceneView &sv, const TraceScene &sc, const DebugPair *pairIds, const DebugView &dv, Stack &st, f3 rayO,
                          f3 rayD, f3 rxDirection, f3 ryDirection, const Hit &h, const Decal &decal, DebugCounters &dc)
{
    constexpr bool TEX = MODE >= 1, ALPHA = MODE == 2;
    f3 out = F3s(0.0f);
    const uint32_t mode = dv.renderMode;
    if (mode >= PTX_DEBUG_MODE_GEOMETRY) // :256-264: the ids need nothing of the vertex
    {
        // (values, not a conditional over lvalues: that one selects between a pointer into the table and one to h.prim, which then lives in scratch)
        const uint32_t instance = pairIds[h.pair].instance, geometry = pairIds[h.pair].geometry, prim = h.prim;
        uint32_t id = instance;
        if (mode == PTX_DEBUG_MODE_GEOMETRY)
            id = geometry;
        if (mode == PTX_DEBUG_MODE_PRIMITIVE)
            id = prim;
        out = debugRandomColor(id);
    }
    else
    {
        const f3 bary = F3(1.0f - h.u - h.v, h.u, h.v); // :166
        const DevPair pr = sv.pairs[h.pair];
        const TriVertices tv3 = loadTriangle(&sv.shadeTris[h.slot]);
        Vtx ov; // :171 getInterpolatedVertex
        ov.Position = interp3(tv3.o[0].Position, tv3.o[1].Position, tv3.o[2].Position, bary);
        ov.Normal = interp3(tv3.o[0].Normal, tv3.o[1].Normal, tv3.o[2].Normal, bary);
        ov.Tangent = interp3(tv3.o[0].Tangent, tv3.o[1].Tangent, tv3.o[2].Tangent, bary);
        ov.Bitangent = interp3(tv3.o[0].Bitangent, tv3.o[1].Bitangent, tv3.o[2].Bitangent, bary);
        const Vtx vertex = transformVertex(pr, ov); // :172; isHitFromInside is always false here: nothing is flipped
        const f2 uv0 = tv3.uv[0], uv1 = tv3.uv[1], uv2 = tv3.uv[2];
        const f2 texCoords = F2((uv0.x * bary.x + uv1.x * bary.y) + uv2.x * bary.z, (uv0.y * bary.x + uv1.y * bary.y) + uv2.y * bary.z);
        if (mode == PTX_DEBUG_MODE_WORLD_POSITION) // :245
            out = vertex.Position;
        else if (mode == PTX_DEBUG_MODE_TEXTURE_COORDS) // :251
            out = F3(texCoords.x, texCoords.y, 0.0f);
        else
        {
            // :178-191 the transformed corners (precomputed per triangle, ShadeTri) and the texture footprint: both offset rays
            // start at the ray's origin (debugRaygen.rgen:26-27 keeps their directions only)
            const f3 P3[3] = { tv3.worldPosition[0], tv3.worldPosition[1], tv3.worldPosition[2] };
            const f3 N3[3] = { tv3.worldNormal[0], tv3.worldNormal[1], tv3.worldNormal[2] };
            const f2 UV3[3] = { uv0, uv1, uv2 };
            f3 dpdu, dpdv, dndu, dndv, dpdx, dpdy;
            computeDpnDuv(P3, N3, UV3, vertex.Tangent, vertex.Bitangent, dpdu, dpdv, dndu, dndv);
            computeDpDxy(vertex.Position, rayO, rxDirection, rayO, ryDirection, vertex.Normal, dpdx, dpdy);
            f4 derivatives;
            derivatives.x = derivatives.y = derivatives.z = derivatives.w = 0.0f;
            if (!(dv.hitGroupFlags & PTX_DEBUG_HIT_DISABLE_MIP_MAPS))
                derivatives = computeDerivatives(dpdx, dpdy, dpdu, dpdv);
            if (mode == PTX_DEBUG_MODE_MIPS) // :254
                out = F3s(0.1f * computeLod(derivatives) + 1.0f);
            else
            {
                MaterialSample material = sampleMaterial<TEX>(sv, pr.materialId, texCoords, derivatives, false,
                                                              (dv.hitGroupFlags & PTX_DEBUG_HIT_DISABLE_COLOR_TEXTURE) != 0u,
                                                              (dv.hitGroupFlags & PTX_DEBUG_HIT_DISABLE_NORMAL_TEXTURE) != 0u); // :195
                if (ALPHA && decal.dist != -1.0f && h.t > decal.dist) // :197-198
                {
                    const f4 c = hitBaseColor(sv, decal.pair, decal.slot, decal.u, decal.v);
                    material.Color = mix(material.Color, rgb(c), c.w);
                }
                const f3 V = -normalize(rayD); // :200-202
                mat3 TBN;
                TBN.c0 = vertex.Tangent;
                TBN.c1 = vertex.Bitangent;
                TBN.c2 = vertex.Normal;
                const f3 N = normalize(vertex.Normal + mul(TBN, material.Normal));
                if (mode == PTX_DEBUG_MODE_NORMAL) // :248
                    out = N;
                else
                {
                    // :204-237.  (The reference traces the shadow rays in every mode and throws the light away in seven of them;
                    // here they are traced where they can be seen.)
                    f3 totalLight = material.Color * 0.1f + material.EmissiveColor;
                    const f3 Pp = offsetRayOriginShadowTerminator(vertex.Position, P3[0], N3[0], P3[1], N3[1], P3[2], N3[2], bary, false); // :206-218
                    const bool shadowsDisabled = (dv.hitGroupFlags & PTX_DEBUG_HIT_DISABLE_SHADOWS) != 0u;
                    const PtxLightsUbo *ubo = sv.lights;
                    const f3 dirDirection = ld3(ubo->Directional.Direction);
                    if (shadowsDisabled || !debugOccluded<ALPHA>(sc, st, dirDirection, Pp, 100000.0f, dc)) // DirectionalLightDistance, sampling.glsl:3
                        totalLight = totalLight + debugLightContribution(dirDirection, ld3(ubo->Directional.Color), 1.0f, V, N, material.Color,
                                                                         material.Roughness, material.Metalness);
                    const uint32_t lightCount = ubo->LightCount;
#pragma nounroll
                    for (uint32_t lightIndex = 0; lightIndex < lightCount; lightIndex++)
                    {
                        const PtxPointLight *light = &ubo->Lights[lightIndex];
                        const f3 lightDirection = Pp - ld3(light->Position);
                        const float dist = length(lightDirection);
                        const float attenuation = div_(1.0f, (light->AttenuationConstant + dist * light->AttenuationLinear) + (dist * dist) * light->AttenuationQuadratic);
                        if (shadowsDisabled || !debugOccluded<ALPHA>(sc, st, lightDirection, Pp, dist, dc))
                            totalLight = totalLight + debugLightContribution(lightDirection, ld3(light->Color), attenuation, V, N, material.Color,
                                                                             material.Roughness, material.Metalness);
                    }
                    out = totalLight;
                }
            }
        }
    }
    f4 r;
    r.x = out.x; r.y = out.y; r.z = out.z; r.w = 1.0f;
    return r;
}

// debugRaygen.rgen:22-40 for the slots of the current tile shard, a thread per slot at a time (the grid is capped at the threads the
// global part of the traversal stack has room for, like k_trace_rays; the loop covers the rest).
// MODE: the scene's kernel mode, as in runPath (0: opaque, fixed 1x1 textures; 1: + the sampler; 2: + the any-hit stages).
template <int MODE, bool CULL>
PT_DEV void debugViewBody(const LaunchParams &p, const SceneView &sv, const TraceScene &sc, const DebugPair *pairIds, const DebugView &dv,
                          float4 *__restrict__ image, uint32_t *__restrict__ counters, uint32_t *spill)
{
    constexpr bool ALPHA = MODE == 2;
    PT_DECLARE_STACK(st, PT_TAIL_LDS, spill)
    DebugCounters dc;
    const bool forceOpaque = (dv.raygenFlags & PTX_DEBUG_RAYGEN_FORCE_OPAQUE) != 0u; // :32-33
    for (uint32_t s = blockIdx.x * blockDim.x + threadIdx.x; s < p.slotsPerFrame; s += gridDim.x * blockDim.x)
    {
        const uint32_t pixel = slotPixel(p, s);
        if (pixel == kNoPixel)
            continue;
        f3 ro, rd, rx, ry;
        constructPrimaryRay<true>(pixel % p.width, pixel / p.width, p.width, p.height, p.u.ViewInverse, p.u.ProjInverse, F2(0.5f, 0.5f), ro, rd, rx, ry); // :25
        Hit h;
        Decal decal = noDecal(); // :28 payload.DecalDist = -1
        bool hit;
        dc.nSeg++;
        dc.nPix++;
        if (ALPHA && !forceOpaque) // :37, tmin / tmax of ray.glsl
            hit = traceRay<false, false, ALPHA, CULL>(sc, ro, rd, 0.00001f, 10000.0f, st, h, nullptr, nullptr, &decal, nullptr, pairIds);
        else
            hit = traceRay<false, false, false, CULL>(sc, ro, rd, 0.00001f, 10000.0f, st, h, nullptr, nullptr, nullptr, nullptr, pairIds);
        f4 c;
        if (hit)
            c = debugClosestHit<MODE>(sv, sc, pairIds, dv, st, ro, rd, rx, ry, h, decal, dc);
        else
        {
            const f3 m = debugMissColor(sv, rd);
            c.x = m.x; c.y = m.y; c.z = m.z; c.w = 1.0f;
        }
        image[pixel] = make_float4(c.x, c.y, c.z, c.w); // :39 imageStore: stored, not added
    }
    if (st.overflow)
        atomicAdd(&counters[C_OVERFLOW], 1u);
    waveAddCounter(&counters[C_SEGMENTS], dc.nSeg);
    waveAddCounter(&counters[C_HITS], dc.nShadow);
    waveAddCounter(&counters[C_SAMPLES], dc.nPix);
}

// The kernel carries the sampler (up to five textureGrad of up to sixteen taps) and a traversal: k_tail<1>'s class.  Register and
// scratch figures of the six variants: docs/EXPERIMENTS.md.
#ifndef PT_DEBUG_VIEW_ATTR
#define PT_DEBUG_VIEW_ATTR __attribute__((amdgpu_waves_per_eu(2, 2)))
#endif
#ifndef PT_DEBUG_VIEW_TEX_ATTR
#define PT_DEBUG_VIEW_TEX_ATTR __attribute__((amdgpu_waves_per_eu(2, 2)))
#endif
template <int MODE, bool CULL>
__global__ void __launch_bounds__(kBlock) k_debug_view(LaunchParams p, SceneView sv, TraceScene sc, const DebugPair *pairIds, DebugView dv,
                                                        float4 *image, uint32_t *counters, uint32_t *spill);
#define PT_DEBUG_VIEW_KERNEL(MODE, CULL, ATTR)                                                                                                  \
    template <>                                                                                                                                 \
    __global__ void __launch_bounds__(kBlock) ATTR k_debug_view<MODE, CULL>(LaunchParams p, SceneView sv, TraceScene sc, const DebugPair *pairIds, \
                                                                           DebugView dv, float4 *image, uint32_t *counters, uint32_t *spill)  \
    {                                                                                                                                           \
        debugViewBody<MODE, CULL>(p, sv, sc, pairIds, dv, image, counters, spill);                                                              \
    }
PT_DEBUG_VIEW_KERNEL(0, false, PT_DEBUG_VIEW_ATTR)
PT_DEBUG_VIEW_KERNEL(0, true, PT_DEBUG_VIEW_ATTR)
PT_DEBUG_VIEW_KERNEL(1, false, PT_DEBUG_VIEW_TEX_ATTR)
PT_DEBUG_VIEW_KERNEL(1, true, PT_DEBUG_VIEW_TEX_ATTR)
PT_DEBUG_VIEW_KERNEL(2, false, PT_DEBUG_VIEW_TEX_ATTR)
PT_DEBUG_VIEW_KERNEL(2, true, PT_DEBUG_VIEW_TEX_ATTR)
#undef PT_DEBUG_VIEW_KERNEL

// ptx_test_debug_eval: the two functions above over n packed inputs
__global__ void k_test_debug_eval(uint32_t which, const float *__restrict__ in, float *__restrict__ out, uint32_t n)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n)
        return;
    f3 r;
    if (which == 0u)
    {
        const float *a = in + (size_t)i * 18;
        r = debugLightContribution(F3(a[0], a[1], a[2]), F3(a[3], a[4], a[5]), a[6], F3(a[7], a[8], a[9]), F3(a[10], a[11], a[12]),
                                   F3(a[13], a[14], a[15]), a[16], a[17]);
    }
    else
        r = debugRandomColor(__float_as_uint(in[i]));
    out[(size_t)i * 3] = r.x;
    out[(size_t)i * 3 + 1] = r.y;
    out[(size_t)i * 3 + 2] = r.z;
}
