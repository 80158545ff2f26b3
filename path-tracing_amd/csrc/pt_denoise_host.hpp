// pt_denoise_host.hpp -- host side of the denoiser (kernels: pt_denoise.hpp; semantics: include/ptx.h, docs/NEXT_ROWS.md section 13).
// Included by pt_runtime.hpp: two stages on the render stream between ptx_render and the output stage, and their read-backs.
#pragma once

static float4 *guidePtr(PtxRenderer *r, uint32_t which)
{
    return r->guides.p + which * r->frame.pixels();
}

static float4 *motionPtr(PtxRenderer *r, uint32_t which)
{
    return r->motion.p + which * r->frame.pixels();
}

// ptx_render_guides: one launch, enqueued like ptx_render_debug's -- the counter block comes back with collectRender, which is
// where a traversal-stack overflow fails the stream.  `motion`: ptx_render_guides_motion -- the same launch of k_render_guides<MODE,
// true>, which also writes where every hit was in the pose the temporal history was made from (docs/NEXT_ROWS.md section 17).
static int renderGuides(PtxRenderer *r, const PtxRaygenUniformData *uniform, bool motion = false, const char *who = "ptx_render_guides")
{
    if (!r || !uniform)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "%s: null argument", who);
    if (!sceneUsable(r) || !imagePtr(r))
        return fail(r, PTX_ERROR_NOT_READY, "%s: need ptx_scene_upload (or ptx_share_scene), ptx_build_accel and ptx_resize first", who);
    if (r->frame.boundShard)
        return frameIsElsewhere(r, who);
    const SceneData &scene = sceneOf(r)->scene;
    if (motion && !scene.pose.enabled)
        return fail(r, PTX_ERROR_NOT_READY, "%s: the scene's owner does not track motion (ptx_track_motion)", who);
    HIP_TRY(r, hipSetDevice(r->device));
    const size_t n = r->frame.pixels();
    HIP_TRY(r, r->guides.alloc(n * PTX_GUIDE_COUNT));
    if (motion)
        HIP_TRY(r, r->motion.alloc(n * PTX_MOTION_COUNT));
    static const PtxLightsUbo noLights = {}; // the pass reads no light
    const LaunchParams p = makeParams(r, uniform, 0, 1);
    if (const int rc = beginLaunch(r, &noLights, p, 0))
        return rc;
    if (!r->guidesReady) // pixels of other ranks' tiles read as misses that were not hit: all zeros
        HIP_TRY(r, hipMemsetAsync(r->guides.p, 0, n * PTX_GUIDE_COUNT * sizeof(float4), r->stream));
    if (motion && !r->motionReady)
        HIP_TRY(r, hipMemsetAsync(r->motion.p, 0, n * PTX_MOTION_COUNT * sizeof(float4), r->stream));
    // the pose the history was made from: the current one, the one the last update replaced, or one nobody kept
    const uint64_t serial = scene.pose.serial, from = r->temporalHistoryIn >= 0 ? r->temporalPose : PtxRenderer::kNoPose;
    if (p.slotsPerFrame)
    {
        const SceneView sv = makeSceneView(r);
        const TraceScene sc = makeTraceScene(r);
        // at most kMaxPersistentThreads threads: the global part of the traversal stack is sized for that many
        const dim3 grid(gridFor(p.slotsPerFrame, kBlock, kMaxPersistentThreads / kBlock));
        if (motion)
        {
            PrevPose prev = {};
            const bool same = from == serial, snapshot = !same && scene.pose.snapshotValid && from != PtxRenderer::kNoPose && from + 1u == serial;
            prev.known = same || snapshot;
            prev.pairs = snapshot ? scene.pose.prevPairs.p : scene.pairs.p;
            prev.skinned = snapshot && scene.skinnedCount ? scene.pose.prevSkinned.p : nullptr;
            prev.firstSkinned = (uint32_t)std::min<uint64_t>(scene.staticVertexCount, 0xffffffffull);
            prev.position = motionPtr(r, PTX_MOTION_POSITION);
            prev.normal = motionPtr(r, PTX_MOTION_NORMAL);
            withMode(kernelMode(r), [&](auto M) {
                k_render_guides<decltype(M)::value, true><<<grid, kBlock, 0, r->stream>>>(p, sv, sc, guidePtr(r, PTX_GUIDE_NORMAL), guidePtr(r, PTX_GUIDE_POSITION),
                                                                                          guidePtr(r, PTX_GUIDE_ALBEDO), r->counters.p, r->spill.p, prev);
            });
        }
        else
            withMode(kernelMode(r), [&](auto M) {
                k_render_guides<decltype(M)::value><<<grid, kBlock, 0, r->stream>>>(p, sv, sc, guidePtr(r, PTX_GUIDE_NORMAL), guidePtr(r, PTX_GUIDE_POSITION),
                                                                                    guidePtr(r, PTX_GUIDE_ALBEDO), r->counters.p, r->spill.p);
            });
    }
    if (const int rc = endLaunch(r, { PendingLaunch::kDebugView })) // the counters are the kernel's own, as the debug view's
        return rc;
    r->guidesReady = true;
    r->guidesPose = serial;
    r->motionReady = motion; // a plain pass leaves the motion images behind the guides: stale
    r->motionFromPose = from;
    return PTX_OK;
}

// device -> host copy of one renderer-owned RGBA32F image of the render extent, synchronous
static int readFrameImage(PtxRenderer *r, const float4 *image, void *host, size_t bytes, const char *who)
{
    if (bytes != r->frame.bytes())
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "%s: buffer must be width*height*16 bytes", who);
    HIP_TRY(r, hipSetDevice(r->device));
    HIP_TRY(r, hipMemcpyAsync(host, image, bytes, hipMemcpyDeviceToHost, r->stream));
    HIP_TRY(r, hipStreamSynchronize(r->stream));
    return collectRender(r); // an error of the launch that produced the image surfaces with it
}

static int readGuide(PtxRenderer *r, uint32_t which, void *host, size_t bytes)
{
    if (!r || !host || which >= PTX_GUIDE_COUNT)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "ptx_read_guide: null argument or unknown guide %u", which);
    if (!r->guidesReady)
        return fail(r, PTX_ERROR_NOT_READY, "ptx_read_guide: call ptx_render_guides first");
    return readFrameImage(r, guidePtr(r, which), host, bytes, "ptx_read_guide");
}

static int readMotion(PtxRenderer *r, uint32_t which, void *host, size_t bytes)
{
    if (!r || !host || which >= PTX_MOTION_COUNT)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "ptx_read_motion: null argument or unknown image %u", which);
    if (!r->motionReady)
        return fail(r, PTX_ERROR_NOT_READY, "ptx_read_motion: call ptx_render_guides_motion first");
    return readFrameImage(r, motionPtr(r, which), host, bytes, "ptx_read_motion");
}

// The filter over the mean `source` / `totalSamples`: ptx_denoise passes the accumulation image and the desc's count (source null:
// the image is looked up after the checks, in their order), ptx_denoise_temporal (pt_temporal_host.hpp) T and 1.
static int denoise(PtxRenderer *r, const PtxDenoiseDesc *d, const float4 *source = nullptr, uint32_t totalSamples = 0u, const char *who = "ptx_denoise")
{
    if (!r || !d)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "%s: null argument", who);
    if (!source)
        totalSamples = d->totalSamples;
    const auto sigmaOk = [](float s) { return s >= 0.0f && s <= 3.402823466e38f; }; // finite and not negative (a NaN fails both)
    if (d->iterations < 1u || d->iterations > 6u || totalSamples == 0u || !sigmaOk(d->sigmaColor) || !sigmaOk(d->sigmaNormal) ||
        !sigmaOk(d->sigmaPosition) || d->sigmaNormal == 0.0f || d->sigmaPosition == 0.0f || d->flags != 0u || d->reserved != 0u)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "%s: need 1 <= iterations <= 6 (%u), totalSamples > 0 (%u), sigmaColor >= 0 (%g), sigmaNormal > 0 (%g), "
                    "sigmaPosition > 0 (%g), all finite, flags 0 (0x%x) and reserved 0 (%u)", who, d->iterations, totalSamples, (double)d->sigmaColor,
                    (double)d->sigmaNormal, (double)d->sigmaPosition, d->flags, d->reserved);
    if (!imagePtr(r))
        return fail(r, PTX_ERROR_NOT_READY, "%s: no accumulation image (call ptx_resize)", who);
    if (r->frame.boundShard)
        return frameIsElsewhere(r, who);
    if (!r->guidesReady)
        return fail(r, PTX_ERROR_NOT_READY, "%s: no guides for this extent (call ptx_render_guides)", who);
    if (r->frame.shard.worldSize > 1u)
        return fail(r, PTX_ERROR_NOT_READY, "%s: this renderer holds one tile shard of %u; the filter's taps cross tiles", who, r->frame.shard.worldSize);
    HIP_TRY(r, hipSetDevice(r->device));
    const size_t n = r->frame.pixels();
    HIP_TRY(r, r->denoisePing[0].alloc(n));
    if (d->iterations > 1u)
        HIP_TRY(r, r->denoisePing[1].alloc(n));
    DenoiseArgs a;
    a.sum = source ? source : imagePtr(r);
    a.normal = guidePtr(r, PTX_GUIDE_NORMAL);
    a.position = guidePtr(r, PTX_GUIDE_POSITION);
    a.albedo = guidePtr(r, PTX_GUIDE_ALBEDO);
    a.width = r->frame.width;
    a.height = r->frame.height;
    a.totalSamples = (float)totalSamples;
    a.invSigmaNormal2 = (float)(1.0 / ((double)d->sigmaNormal * d->sigmaNormal));
    a.invSigmaPosition = (float)(1.0 / (double)d->sigmaPosition);
    const dim3 block(kDenoiseTileX, kDenoiseTileY), grid((r->frame.width + kDenoiseTileX - 1) / kDenoiseTileX, (r->frame.height + kDenoiseTileY - 1) / kDenoiseTileY);
    for (uint32_t i = 0; i < d->iterations; i++)
    {
        a.src = i ? r->denoisePing[(i - 1u) & 1u].p : nullptr;
        a.dst = r->denoisePing[i & 1u].p;
        a.step = 1 << i;
        const double sc = (double)d->sigmaColor / (double)(1u << i);
        a.invSigmaColor2 = d->sigmaColor > 0.0f ? (float)(1.0 / (sc * sc)) : 0.0f;
        const bool first = i == 0u, last = i + 1u == d->iterations;
        if (first && last) k_denoise<true, true><<<grid, block, 0, r->stream>>>(a);
        else if (first) k_denoise<true, false><<<grid, block, 0, r->stream>>>(a);
        else if (last) k_denoise<false, true><<<grid, block, 0, r->stream>>>(a);
        else k_denoise<false, false><<<grid, block, 0, r->stream>>>(a);
    }
    HIP_TRY(r, hipGetLastError());
    r->denoisedIn = (int)((d->iterations - 1u) & 1u);
    return PTX_OK;
}

static int readDenoised(PtxRenderer *r, void *host, size_t bytes)
{
    if (!r || !host)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "ptx_read_denoised: null argument");
    if (r->denoisedIn < 0)
        return fail(r, PTX_ERROR_NOT_READY, "ptx_read_denoised: call ptx_denoise first");
    return readFrameImage(r, r->denoisePing[r->denoisedIn].p, host, bytes, "ptx_read_denoised");
}

// ptx_postprocess's chain on the denoised image, which holds the mean: TotalSamples = 1
static int postprocessDenoised(PtxRenderer *r, const PtxPostProcessingUniformData *uniform, uint32_t toneMappingMode)
{
    if (!r || !uniform || toneMappingMode > PTX_TONE_MAPPING_HDR)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "ptx_postprocess_denoised: bad argument");
    if (r->denoisedIn < 0)
        return fail(r, PTX_ERROR_NOT_READY, "ptx_postprocess_denoised: call ptx_denoise first");
    PtxPostProcessingUniformData u = *uniform;
    u.TotalSamples = 1u;
    return postprocessImage(r, r->denoisePing[r->denoisedIn].p, &u, toneMappingMode);
}
