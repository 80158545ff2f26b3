// pt_chain_host.hpp -- host side of the interactive chain, the stages on the render stream between ptx_render and the output stage:
// the guide pass (plain, with motion guides, following specular chains), the temporal accumulation (plain, with moments, through the
// motion guides, responsive), the three filters (on the accumulation image, on T, variance-guided on T) and their read-backs, and the firefly
// suppression in front of them (ptx_despike, the switch that puts its image in the sum's place).  The output calls on C and D are the output stage's
// (pt_output_host.hpp).  Kernels: pt_denoise.hpp, pt_temporal.hpp,
// pt_variance.hpp, pt_responsive.hpp, pt_despike.hpp; semantics: include/ptx.h, docs/NEXT_ROWS.md sections 13, 14 and 16 - 20; state: ChainState, the member `chain` of
// the handle, whose bookkeeping (pt_chain_state.hpp) is told of every accepted call.  Included by pt_runtime.hpp after
// pt_frame_host.hpp; every function takes a valid or null handle and returns a PTX_* code.
#pragma once

// What every stage behind the guide pass needs, in the order it is reported.  `taps`: whose taps cross tiles, "filter" or "history";
// `motion`: the call reads the motion guides.  `readsSum`: the call reads the accumulation image, so C in its place while
// ptx_chain_use_despiked is on (docs/NEXT_ROWS.md section 20): the last rung.
static int chainRefusal(PtxRenderer *r, const char *who, const char *taps, bool motion = false, bool readsSum = false)
{
    if (!imagePtr(r))
        return fail(r, PTX_ERROR_NOT_READY, "%s: no accumulation image (call ptx_resize)", who);
    if (r->frame.boundShard)
        return frameIsElsewhere(r, who);
    if (!r->chain.status.guidesReady)
        return fail(r, PTX_ERROR_NOT_READY, "%s: no guides for this extent (call ptx_render_guides)", who);
    if (motion && !r->chain.status.motionFresh())
        return fail(r, PTX_ERROR_NOT_READY, "%s: the motion guides are stale: a ptx_render_guides or an accumulate call came after the last "
                    "ptx_render_guides_motion", who);
    if (r->frame.shard.worldSize > 1u)
        return fail(r, PTX_ERROR_NOT_READY, "%s: this renderer holds one tile shard of %u; the %s's taps cross tiles", who, r->frame.shard.worldSize, taps);
    if (readsSum && r->chain.status.useDespiked && !r->chain.status.despikedReady)
        return fail(r, PTX_ERROR_NOT_READY, "%s: ptx_chain_use_despiked is on and there is no despiked image for this extent (call ptx_despike)", who);
    return PTX_OK;
}

// The image the accumulate calls and ptx_denoise read as the sum: C while ptx_chain_use_despiked is on (chainRefusal saw that it exists)
static const float4 *chainSum(const PtxRenderer *r)
{
    return r->chain.status.useDespiked ? r->chain.despikedImage.p : imagePtr(r);
}

// one thread per pixel in 32 x 8 tiles: the grid of every kernel behind the guide pass
static dim3 tileGrid(const PtxRenderer *r)
{
    return dim3((r->frame.width + kDenoiseTileX - 1) / kDenoiseTileX, (r->frame.height + kDenoiseTileY - 1) / kDenoiseTileY);
}
static const dim3 kTileBlock(kDenoiseTileX, kDenoiseTileY);

// DenoiseArgs, TemporalArgs, VarianceArgs
template <class Args> static void setGuides(const PtxRenderer *r, Args &a)
{
    a.normal = r->chain.guidePtr(PTX_GUIDE_NORMAL, r->frame.pixels());
    a.position = r->chain.guidePtr(PTX_GUIDE_POSITION, r->frame.pixels());
    a.albedo = r->chain.guidePtr(PTX_GUIDE_ALBEDO, r->frame.pixels());
}

// ---- the guide pass ----------------------------------------------------------------------------------------

// ptx_render_guides: one launch, enqueued like ptx_render_debug's -- the counter block comes back with collectRender, which is
// where a traversal-stack overflow fails the stream.  `motion`: ptx_render_guides_motion -- the same launch of k_render_guides<MODE,
// true>, which also writes where every hit was in the pose the temporal history was made from (docs/NEXT_ROWS.md section 17).
// `specular`: ptx_render_guides_specular's checked desc -- the same ladder and launch with k_render_guides_specular<MODE>, which follows
// near-delta surfaces and writes a fourth image (section 18); to the chain it is a plain guide pass.
static int renderGuides(PtxRenderer *r, const PtxRaygenUniformData *uniform, bool motion = false, const char *who = "ptx_render_guides",
                        const PtxSpecularGuidesDesc *specular = nullptr)
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
    ChainState &c = r->chain;
    const size_t n = r->frame.pixels();
    HIP_TRY(r, c.guides.alloc(n * PTX_GUIDE_COUNT));
    if (motion)
        HIP_TRY(r, c.motion.alloc(n * PTX_MOTION_COUNT));
    if (specular)
        HIP_TRY(r, c.specular.alloc(n * PTX_SPECULAR_COUNT));
    static const PtxLightsUbo noLights = {}; // the pass reads no light
    const LaunchParams p = makeParams(r, uniform, 0, 1);
    if (const int rc = beginLaunch(r, &noLights, p, 0))
        return rc;
    if (!c.status.guidesReady) // pixels of other ranks' tiles read as misses that were not hit: all zeros
        HIP_TRY(r, hipMemsetAsync(c.guides.p, 0, n * PTX_GUIDE_COUNT * sizeof(float4), r->stream));
    if (motion && !c.status.motionReady)
        HIP_TRY(r, hipMemsetAsync(c.motion.p, 0, n * PTX_MOTION_COUNT * sizeof(float4), r->stream));
    if (specular && !c.status.specularReady)
        HIP_TRY(r, hipMemsetAsync(c.specular.p, 0, n * PTX_SPECULAR_COUNT * sizeof(float4), r->stream));
    const uint64_t serial = scene.pose.serial;
    if (p.slotsPerFrame)
    {
        const SceneView sv = makeSceneView(r);
        const TraceScene sc = makeTraceScene(r);
        // at most kMaxPersistentThreads threads: the global part of the traversal stack is sized for that many
        const dim3 grid(gridFor(p.slotsPerFrame, kBlock, kMaxPersistentThreads / kBlock));
        const auto launch = [&](auto... prev) { // nothing, or the PrevPose of a motion pass
            withMode(kernelMode(r), [&](auto M) {
                k_render_guides<decltype(M)::value, sizeof...(prev) != 0><<<grid, kBlock, 0, r->stream>>>(
                    p, sv, sc, c.guidePtr(PTX_GUIDE_NORMAL, n), c.guidePtr(PTX_GUIDE_POSITION, n), c.guidePtr(PTX_GUIDE_ALBEDO, n), r->launch.counters.p, r->launch.spill.p, prev...);
            });
        };
        if (specular)
            withMode(kernelMode(r), [&](auto M) {
                k_render_guides_specular<decltype(M)::value><<<grid, kBlock, 0, r->stream>>>(
                    p, sv, sc, c.guidePtr(PTX_GUIDE_NORMAL, n), c.guidePtr(PTX_GUIDE_POSITION, n), c.guidePtr(PTX_GUIDE_ALBEDO, n),
                    c.specularPtr(PTX_SPECULAR_SURFACE, n), specular->maxBounces, specular->roughnessMax, r->launch.counters.p, r->launch.spill.p);
            });
        else if (motion)
        {
            // the pose the history was made from: the current one, the one the last update replaced, or one nobody kept
            const PrevPoseSource from = ChainStatus::prevPoseSource(c.status.historyPose(), serial, scene.pose.snapshotValid);
            const bool snapshot = from == PrevPoseSource::kSnapshot;
            PrevPose prev = {};
            prev.known = from != PrevPoseSource::kUnknown;
            prev.pairs = snapshot ? scene.pose.prevPairs.p : scene.pairs.p;
            prev.skinned = snapshot && scene.skinnedCount ? scene.pose.prevSkinned.p : nullptr;
            prev.firstSkinned = (uint32_t)std::min<uint64_t>(scene.staticVertexCount, 0xffffffffull);
            prev.position = c.motionPtr(PTX_MOTION_POSITION, n);
            prev.normal = c.motionPtr(PTX_MOTION_NORMAL, n);
            launch(prev);
        }
        else
            launch();
    }
    if (const int rc = endLaunch(r, { PendingLaunch::kDebugView })) // the counters are the kernel's own, as the debug view's
        return rc;
    c.status.guidesRendered(serial, motion);
    if (specular)
        c.status.specularRendered();
    return PTX_OK;
}

// ptx_render_guides_specular (docs/NEXT_ROWS.md section 18): the desc is checked first, the rest is renderGuides' own ladder and launch
static int renderGuidesSpecular(PtxRenderer *r, const PtxRaygenUniformData *uniform, const PtxSpecularGuidesDesc *d)
{
    const char *who = "ptx_render_guides_specular";
    if (!r || !uniform || !d)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "%s: null argument", who);
    if (d->maxBounces > 8u || !(d->roughnessMax >= 0.0f && d->roughnessMax <= 3.402823466e38f) || d->flags != 0u || d->reserved != 0u)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "%s: need maxBounces <= 8 (%u), roughnessMax >= 0 and finite (%g), flags 0 (0x%x) and reserved 0 (%u)", who,
                    d->maxBounces, (double)d->roughnessMax, d->flags, d->reserved);
    return renderGuides(r, uniform, false, who, d);
}

// device -> host copy of one renderer-owned image of the render extent with `texel` bytes per pixel, synchronous
static int readFrameImage(PtxRenderer *r, const void *image, void *host, size_t bytes, size_t texel, const char *who)
{
    if (bytes != r->frame.pixels() * texel)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "%s: buffer must be width*height*%zu bytes", who, texel);
    HIP_TRY(r, hipSetDevice(r->device));
    HIP_TRY(r, hipMemcpyAsync(host, image, bytes, hipMemcpyDeviceToHost, r->stream));
    HIP_TRY(r, hipStreamSynchronize(r->stream));
    return collectRender(r); // an error of the launch that produced the image surfaces with it
}

static int readGuide(PtxRenderer *r, uint32_t which, void *host, size_t bytes)
{
    if (!r || !host || which >= PTX_GUIDE_COUNT)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "ptx_read_guide: null argument or unknown guide %u", which);
    if (!r->chain.status.guidesReady)
        return fail(r, PTX_ERROR_NOT_READY, "ptx_read_guide: call ptx_render_guides first");
    return readFrameImage(r, r->chain.guidePtr(which, r->frame.pixels()), host, bytes, sizeof(float4), "ptx_read_guide");
}

static int readMotion(PtxRenderer *r, uint32_t which, void *host, size_t bytes)
{
    if (!r || !host || which >= PTX_MOTION_COUNT)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "ptx_read_motion: null argument or unknown image %u", which);
    if (!r->chain.status.motionReady)
        return fail(r, PTX_ERROR_NOT_READY, "ptx_read_motion: call ptx_render_guides_motion first");
    return readFrameImage(r, r->chain.motionPtr(which, r->frame.pixels()), host, bytes, sizeof(float4), "ptx_read_motion");
}

static int readSpecularGuide(PtxRenderer *r, uint32_t which, void *host, size_t bytes)
{
    if (!r || !host || which >= PTX_SPECULAR_COUNT)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "ptx_read_specular_guide: null argument or unknown image %u", which);
    if (!r->chain.status.specularReady)
        return fail(r, PTX_ERROR_NOT_READY, "ptx_read_specular_guide: call ptx_render_guides_specular first");
    return readFrameImage(r, r->chain.specularPtr(which, r->frame.pixels()), host, bytes, sizeof(float4), "ptx_read_specular_guide");
}

// ---- the temporal accumulation -----------------------------------------------------------------------------

// One stage between the guide pass and the filter.  `moments`: ptx_temporal_accumulate_moments -- the same stage with
// k_temporal_moments, which carries the moment history along; a plain call drops that history.
// `motion`: ptx_temporal_accumulate_motion -- the same stage with k_temporal_motion / k_temporal_moments_motion, which look the
// history up through the motion guides of the last ptx_render_guides_motion (docs/NEXT_ROWS.md section 17).
// `responsive`: ptx_temporal_accumulate_responsive's desc, checked here behind the base call's -- the same stage with
// k_temporal_responsive, which carries the fast history along, and k_responsive_clamp behind it (docs/NEXT_ROWS.md section 19); a
// call without it drops the fast history.
static int temporalAccumulate(PtxRenderer *r, const PtxTemporalDesc *d, bool moments = false, const char *who = "ptx_temporal_accumulate", bool motion = false,
                              const PtxResponsiveDesc *responsive = nullptr)
{
    if (!r || !d)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "%s: null argument", who);
    const auto positive = [](float v) { return v > 0.0f && v <= 3.402823466e38f; }; // finite and above zero (a NaN fails both)
    if (d->totalSamples == 0u || !(d->maxHistory >= 1.0f) || !positive(d->maxHistory) || !positive(d->normalThreshold) || !positive(d->positionThreshold) ||
        (d->flags & ~(uint32_t)PTX_TEMPORAL_RESET) != 0u || d->reserved != 0u)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "%s: need totalSamples > 0 (%u), maxHistory >= 1 (%g), normalThreshold > 0 (%g), "
                    "positionThreshold > 0 (%g), all finite, flags 0 or PTX_TEMPORAL_RESET (0x%x) and reserved 0 (%u)", who, d->totalSamples, (double)d->maxHistory,
                    (double)d->normalThreshold, (double)d->positionThreshold, d->flags, d->reserved);
    if (responsive && (!(responsive->fastHistory >= 1.0f) || !(responsive->fastHistory <= d->maxHistory) || !positive(responsive->clampSigma) ||
                       responsive->reserved != 0u)) // the flags chose `moments` and `motion`: temporalAccumulateResponsive
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "%s: need 1 <= fastHistory <= maxHistory (%g, %g), clampSigma > 0 and finite (%g) and reserved 0 (%u)", who,
                    (double)responsive->fastHistory, (double)d->maxHistory, (double)responsive->clampSigma, responsive->reserved);
    if (const int rc = chainRefusal(r, who, "history", motion, true))
        return rc;
    HIP_TRY(r, hipSetDevice(r->device));
    ChainState &c = r->chain;
    const size_t n = r->frame.pixels();
    HIP_TRY(r, c.temporalImage.alloc(n));
    for (int i = 0; i < 2; i++)
    {
        HIP_TRY(r, c.temporalHistory[i].alloc(n * kTemporalHistoryImages));
        if (moments)
            HIP_TRY(r, c.momentHistory[i].alloc(n));
        if (responsive)
            HIP_TRY(r, c.fastHistory[i].alloc(n));
    }
    ChainStatus next = c.status; // the call counts once its launch is accepted
    const ChainStatus::Accumulate h = next.accumulate(moments, (d->flags & PTX_TEMPORAL_RESET) != 0u, responsive != nullptr);
    TemporalArgs a;
    a.sum = chainSum(r);
    setGuides(r, a);
    a.histIn = h.useHistory ? c.temporalHistory[h.src].p : nullptr;
    a.histOut = c.temporalHistory[h.dst].p;
    a.out = c.temporalImage.p;
    a.width = r->frame.width;
    a.height = r->frame.height;
    a.pixels = (uint32_t)n;
    a.totalSamples = (float)d->totalSamples;
    a.maxHistory = d->maxHistory;
    a.normalThreshold2 = d->normalThreshold * d->normalThreshold;
    a.positionThreshold = d->positionThreshold;
    memcpy(a.view, c.temporalView, sizeof a.view);
    memcpy(a.proj, c.temporalProj, sizeof a.proj);
    const bool sameCamera = h.useHistory && !memcmp(d->View, c.temporalView, sizeof d->View) && !memcmp(d->Proj, c.temporalProj, sizeof d->Proj);
    const float4 *momentsIn = h.useMoments ? c.momentHistory[h.src].p : nullptr;
    float4 *momentsOut = c.momentHistory[h.dst].p;
    const TemporalMotion mo = { motion ? c.motionPtr(PTX_MOTION_POSITION, n) : nullptr, motion ? c.motionPtr(PTX_MOTION_NORMAL, n) : nullptr };
    const dim3 grid = tileGrid(r);
    if (responsive)
    {
        const ResponsiveHistories rh = { h.useFast ? c.fastHistory[h.src].p : nullptr, c.fastHistory[h.dst].p, momentsIn, momentsOut, responsive->fastHistory };
        ResponsiveClampArgs b;
        b.fast = c.fastHistory[h.dst].p;
        b.temporal = c.temporalImage.p;
        b.history = c.temporalHistory[h.dst].p;
        b.moments = momentsOut;
        b.albedo = a.albedo;
        b.width = a.width;
        b.height = a.height;
        b.clampSigma = responsive->clampSigma;
        withFlag(moments, [&](auto Moments) {
            constexpr bool mm = decltype(Moments)::value;
            withFlag(motion, [&](auto Motion) { withFlag(sameCamera, [&](auto Same) {
                k_temporal_responsive<decltype(Same)::value, mm, decltype(Motion)::value><<<grid, kTileBlock, 0, r->stream>>>(a, rh, mo);
            }); });
            k_responsive_clamp<mm><<<grid, kTileBlock, 0, r->stream>>>(b);
        });
    }
    else
        withFlag(moments, [&](auto Moments) { withFlag(motion, [&](auto Motion) { withFlag(sameCamera, [&](auto Same) {
            constexpr bool mm = decltype(Moments)::value, mv = decltype(Motion)::value, same = decltype(Same)::value;
            if constexpr (mm && mv) k_temporal_moments_motion<same><<<grid, kTileBlock, 0, r->stream>>>(a, momentsIn, momentsOut, mo);
            else if constexpr (mm) k_temporal_moments<same><<<grid, kTileBlock, 0, r->stream>>>(a, momentsIn, momentsOut);
            else if constexpr (mv) k_temporal_motion<same><<<grid, kTileBlock, 0, r->stream>>>(a, mo);
            else k_temporal<same><<<grid, kTileBlock, 0, r->stream>>>(a);
        }); }); });
    HIP_TRY(r, hipGetLastError());
    c.status = next;
    memcpy(c.temporalView, d->View, sizeof d->View);
    memcpy(c.temporalProj, d->Proj, sizeof d->Proj);
    return PTX_OK;
}

static int temporalAccumulateMotion(PtxRenderer *r, const PtxTemporalDesc *d, uint32_t withMoments)
{
    if (withMoments > 1u)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "ptx_temporal_accumulate_motion: withMoments is 0 or 1 (%u)", withMoments);
    return temporalAccumulate(r, d, withMoments != 0u, "ptx_temporal_accumulate_motion", true);
}

// ptx_temporal_accumulate_responsive: the flags choose the base call, whose name the refusals keep apart from the plain calls'
static int temporalAccumulateResponsive(PtxRenderer *r, const PtxTemporalDesc *d, const PtxResponsiveDesc *responsive)
{
    const char *who = "ptx_temporal_accumulate_responsive";
    if (!r || !d || !responsive)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "%s: null argument", who);
    if ((responsive->flags & ~(uint32_t)(PTX_RESPONSIVE_MOMENTS | PTX_RESPONSIVE_MOTION)) != 0u)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "%s: flags are PTX_RESPONSIVE_MOMENTS and PTX_RESPONSIVE_MOTION (0x%x)", who, responsive->flags);
    return temporalAccumulate(r, d, (responsive->flags & PTX_RESPONSIVE_MOMENTS) != 0u, who, (responsive->flags & PTX_RESPONSIVE_MOTION) != 0u, responsive);
}

static int readFastHistory(PtxRenderer *r, void *host, size_t bytes)
{
    if (!r || !host)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "ptx_read_fast_history: null argument");
    if (!r->chain.status.fastCurrent())
        return fail(r, PTX_ERROR_NOT_READY, "ptx_read_fast_history: the last accumulate call was not ptx_temporal_accumulate_responsive");
    return readFrameImage(r, r->chain.fastHistory[r->chain.status.historyIn].p, host, bytes, sizeof(float4), "ptx_read_fast_history");
}

static int readTemporal(PtxRenderer *r, void *host, size_t bytes)
{
    if (!r || !host)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "ptx_read_temporal: null argument");
    if (!r->chain.status.temporalReady)
        return fail(r, PTX_ERROR_NOT_READY, "ptx_read_temporal: call ptx_temporal_accumulate first");
    return readFrameImage(r, r->chain.temporalImage.p, host, bytes, sizeof(float4), "ptx_read_temporal");
}

static int readMoments(PtxRenderer *r, void *host, size_t bytes)
{
    if (!r || !host)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "ptx_read_moments: null argument");
    if (!r->chain.status.momentsCurrent())
        return fail(r, PTX_ERROR_NOT_READY, "ptx_read_moments: the last accumulate call was not ptx_temporal_accumulate_moments");
    return readFrameImage(r, r->chain.momentHistory[r->chain.status.historyIn].p, host, bytes, sizeof(float4), "ptx_read_moments");
}

// ---- the filters -------------------------------------------------------------------------------------------

// The filter over the mean `source` / `totalSamples`: ptx_denoise passes the accumulation image and the desc's count (source null:
// the image is looked up after the checks, in their order), ptx_denoise_temporal T and 1.
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
    if (const int rc = chainRefusal(r, who, "filter", false, !source))
        return rc;
    HIP_TRY(r, hipSetDevice(r->device));
    ChainState &c = r->chain;
    HIP_TRY(r, c.denoisePing[0].alloc(r->frame.pixels()));
    if (d->iterations > 1u)
        HIP_TRY(r, c.denoisePing[1].alloc(r->frame.pixels()));
    DenoiseArgs a;
    a.sum = source ? source : chainSum(r);
    setGuides(r, a);
    a.width = r->frame.width;
    a.height = r->frame.height;
    a.totalSamples = (float)totalSamples;
    a.invSigmaNormal2 = (float)(1.0 / ((double)d->sigmaNormal * d->sigmaNormal));
    a.invSigmaPosition = (float)(1.0 / (double)d->sigmaPosition);
    const dim3 grid = tileGrid(r);
    for (uint32_t i = 0; i < d->iterations; i++)
    {
        a.src = i ? c.denoisePing[(i - 1u) & 1u].p : nullptr;
        a.dst = c.denoisePing[i & 1u].p;
        a.step = 1 << i;
        const double sc = (double)d->sigmaColor / (double)(1u << i);
        a.invSigmaColor2 = d->sigmaColor > 0.0f ? (float)(1.0 / (sc * sc)) : 0.0f;
        withFlag(i == 0u, [&](auto First) { withFlag(i + 1u == d->iterations, [&](auto Last) {
            k_denoise<decltype(First)::value, decltype(Last)::value><<<grid, kTileBlock, 0, r->stream>>>(a);
        }); });
    }
    HIP_TRY(r, hipGetLastError());
    c.status.filtered(d->iterations);
    return PTX_OK;
}

// ptx_denoise's filter on T, which holds the mean: totalSamples = 1
static int denoiseTemporal(PtxRenderer *r, const PtxDenoiseDesc *d)
{
    if (!r || !d)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "ptx_denoise_temporal: null argument");
    if (!r->chain.status.temporalReady)
        return fail(r, PTX_ERROR_NOT_READY, "ptx_denoise_temporal: call ptx_temporal_accumulate first");
    return denoise(r, d, r->chain.temporalImage.p, 1u, "ptx_denoise_temporal");
}

// V_0 and P_0 from the estimate, then one launch per iteration: P_0 lies in denoisePing[1], iteration i writes denoisePing[i & 1], so
// the result lands where ptx_denoise's does
static int denoiseVariance(PtxRenderer *r, const PtxDenoiseDesc *d)
{
    const char *who = "ptx_denoise_variance";
    if (!r || !d)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "%s: null argument", who);
    const auto positive = [](float s) { return s > 0.0f && s <= 3.402823466e38f; }; // finite and above zero (a NaN fails both)
    if (d->iterations < 1u || d->iterations > 6u || !positive(d->sigmaColor) || !positive(d->sigmaNormal) || !positive(d->sigmaPosition) || d->flags != 0u ||
        d->reserved != 0u)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "%s: need 1 <= iterations <= 6 (%u), sigmaColor (read as sigmaLuminance) > 0 (%g), sigmaNormal > 0 (%g), "
                    "sigmaPosition > 0 (%g), all finite, flags 0 (0x%x) and reserved 0 (%u)", who, d->iterations, (double)d->sigmaColor, (double)d->sigmaNormal,
                    (double)d->sigmaPosition, d->flags, d->reserved);
    if (const int rc = chainRefusal(r, who, "filter"))
        return rc;
    ChainState &c = r->chain;
    if (!c.status.momentsCurrent())
        return fail(r, PTX_ERROR_NOT_READY, "%s: the last accumulate call must be ptx_temporal_accumulate_moments", who);
    HIP_TRY(r, hipSetDevice(r->device));
    HIP_TRY(r, c.denoisePing[0].alloc(r->frame.pixels()));
    HIP_TRY(r, c.denoisePing[1].alloc(r->frame.pixels()));
    HIP_TRY(r, c.varianceImage.alloc(r->frame.pixels()));
    VarianceArgs a;
    a.temporal = c.temporalImage.p;
    a.moments = c.momentHistory[c.status.historyIn].p;
    a.variance = c.varianceImage.p;
    a.src = nullptr;
    a.dst = c.denoisePing[1].p;
    setGuides(r, a);
    a.width = r->frame.width;
    a.height = r->frame.height;
    a.step = 1;
    a.invSigmaLuminance2 = (float)(1.0 / ((double)d->sigmaColor * d->sigmaColor));
    a.invSigmaNormal2 = (float)(1.0 / ((double)d->sigmaNormal * d->sigmaNormal));
    a.invSigmaPosition = (float)(1.0 / (double)d->sigmaPosition);
    const dim3 grid = tileGrid(r);
    k_variance_estimate<<<grid, kTileBlock, 0, r->stream>>>(a);
    for (uint32_t i = 0; i < d->iterations; i++)
    {
        a.src = c.denoisePing[(i + 1u) & 1u].p;
        a.dst = c.denoisePing[i & 1u].p;
        a.step = 1 << i;
        withFlag(i + 1u == d->iterations, [&](auto Last) { k_denoise_variance<decltype(Last)::value><<<grid, kTileBlock, 0, r->stream>>>(a); });
    }
    HIP_TRY(r, hipGetLastError());
    c.status.varianceFiltered(d->iterations);
    return PTX_OK;
}

static int readDenoised(PtxRenderer *r, void *host, size_t bytes)
{
    if (!r || !host)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "ptx_read_denoised: null argument");
    if (!r->chain.denoised())
        return fail(r, PTX_ERROR_NOT_READY, "ptx_read_denoised: call ptx_denoise first");
    return readFrameImage(r, r->chain.denoised(), host, bytes, sizeof(float4), "ptx_read_denoised");
}

static int readVariance(PtxRenderer *r, void *host, size_t bytes)
{
    if (!r || !host)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "ptx_read_variance: null argument");
    if (!r->chain.status.varianceReady)
        return fail(r, PTX_ERROR_NOT_READY, "ptx_read_variance: call ptx_denoise_variance first");
    return readFrameImage(r, r->chain.varianceImage.p, host, bytes, sizeof(float), "ptx_read_variance");
}

// ---- firefly suppression (docs/NEXT_ROWS.md section 20) ------------------------------------------------------------------------------

// ptx_despike: C from the sum as it stands, one launch.  No scene and no guides: the ladder is the image's own.
static int despike(PtxRenderer *r, const PtxDespikeDesc *d)
{
    const char *who = "ptx_despike";
    if (!r || !d)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "%s: null argument", who);
    const uint32_t window = d->radius == 1u ? 8u : 24u;
    if ((d->radius != 1u && d->radius != 2u) || d->rank < 1u || d->rank > 4u || d->minTaps < d->rank || d->minTaps > window ||
        !(d->gain >= 1.0f && d->gain <= 3.402823466e38f) || d->flags != 0u || d->reserved != 0u)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "%s: need radius 1 or 2 (%u), 1 <= rank <= 4 (%u), rank <= minTaps <= (2 radius + 1)^2 - 1 (%u), "
                    "gain >= 1 and finite (%g), flags 0 (0x%x) and reserved 0 (%u)", who, d->radius, d->rank, d->minTaps, (double)d->gain, d->flags, d->reserved);
    if (!imagePtr(r))
        return fail(r, PTX_ERROR_NOT_READY, "%s: no accumulation image (call ptx_resize)", who);
    if (r->frame.boundShard)
        return frameIsElsewhere(r, who);
    if (r->frame.shard.worldSize > 1u)
        return fail(r, PTX_ERROR_NOT_READY, "%s: this renderer holds one tile shard of %u; the window's taps cross tiles", who, r->frame.shard.worldSize);
    HIP_TRY(r, hipSetDevice(r->device));
    ChainState &c = r->chain;
    HIP_TRY(r, c.despikedImage.alloc(r->frame.pixels()));
    DespikeArgs a;
    a.sum = imagePtr(r);
    a.out = c.despikedImage.p;
    a.width = r->frame.width;
    a.height = r->frame.height;
    a.rank = d->rank;
    a.minTaps = d->minTaps;
    a.gain = d->gain;
    if (d->radius == 1u)
        k_despike<1><<<tileGrid(r), kTileBlock, 0, r->stream>>>(a);
    else
        k_despike<2><<<tileGrid(r), kTileBlock, 0, r->stream>>>(a);
    HIP_TRY(r, hipGetLastError());
    c.status.despiked();
    return PTX_OK;
}

static int readDespiked(PtxRenderer *r, void *host, size_t bytes)
{
    if (!r || !host)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "ptx_read_despiked: null argument");
    if (!r->chain.despiked())
        return fail(r, PTX_ERROR_NOT_READY, "ptx_read_despiked: call ptx_despike first");
    return readFrameImage(r, r->chain.despiked(), host, bytes, sizeof(float4), "ptx_read_despiked");
}

// ptx_chain_use_despiked: sticky, like ptx_track_motion; the calls that read the sum look at it when they are made
static int chainUseDespiked(PtxRenderer *r, int enable)
{
    if (!r)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "ptx_chain_use_despiked: null argument");
    r->chain.status.useDespiked = enable != 0;
    return PTX_OK;
}
