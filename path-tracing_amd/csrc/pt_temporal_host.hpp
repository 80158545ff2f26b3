// pt_temporal_host.hpp -- host side of the temporal accumulation (kernel: pt_temporal.hpp; semantics: include/ptx.h, docs/NEXT_ROWS.md
// section 14).  Included by pt_runtime.hpp after pt_denoise_host.hpp: one stage on the render stream between ptx_render_guides and
// the filter, its read-back, and the filter on its result.
#pragma once

// `moments`: ptx_temporal_accumulate_moments (pt_variance_host.hpp) -- the same stage with k_temporal_moments, which carries the
// moment history along; a plain call drops that history.
// `motion`: ptx_temporal_accumulate_motion -- the same stage with k_temporal_motion / k_temporal_moments_motion, which look the
// history up through the motion guides of the last ptx_render_guides_motion (docs/NEXT_ROWS.md section 17).
static int temporalAccumulate(PtxRenderer *r, const PtxTemporalDesc *d, bool moments = false, const char *who = "ptx_temporal_accumulate", bool motion = false)
{
    if (!r || !d)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "%s: null argument", who);
    const auto positive = [](float v) { return v > 0.0f && v <= 3.402823466e38f; }; // finite and above zero (a NaN fails both)
    if (d->totalSamples == 0u || !(d->maxHistory >= 1.0f) || !positive(d->maxHistory) || !positive(d->normalThreshold) || !positive(d->positionThreshold) ||
        (d->flags & ~(uint32_t)PTX_TEMPORAL_RESET) != 0u || d->reserved != 0u)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "%s: need totalSamples > 0 (%u), maxHistory >= 1 (%g), normalThreshold > 0 (%g), "
                    "positionThreshold > 0 (%g), all finite, flags 0 or PTX_TEMPORAL_RESET (0x%x) and reserved 0 (%u)", who, d->totalSamples, (double)d->maxHistory,
                    (double)d->normalThreshold, (double)d->positionThreshold, d->flags, d->reserved);
    if (!imagePtr(r))
        return fail(r, PTX_ERROR_NOT_READY, "%s: no accumulation image (call ptx_resize)", who);
    if (r->frame.boundShard)
        return frameIsElsewhere(r, who);
    if (!r->guidesReady)
        return fail(r, PTX_ERROR_NOT_READY, "%s: no guides for this extent (call ptx_render_guides)", who);
    // the motion images belong to the guides they were rendered with and lead back to the history as it stood then
    if (motion && (!r->motionReady || r->motionFromPose != (r->temporalHistoryIn >= 0 ? r->temporalPose : PtxRenderer::kNoPose)))
        return fail(r, PTX_ERROR_NOT_READY, "%s: the motion guides are stale: a ptx_render_guides or an accumulate call came after the last "
                    "ptx_render_guides_motion", who);
    if (r->frame.shard.worldSize > 1u)
        return fail(r, PTX_ERROR_NOT_READY, "%s: this renderer holds one tile shard of %u; the history's taps cross tiles", who,
                    r->frame.shard.worldSize);
    HIP_TRY(r, hipSetDevice(r->device));
    const size_t n = r->frame.pixels();
    HIP_TRY(r, r->temporalImage.alloc(n));
    HIP_TRY(r, r->temporalHistory[0].alloc(n * kTemporalHistoryImages));
    HIP_TRY(r, r->temporalHistory[1].alloc(n * kTemporalHistoryImages));
    if (moments)
    {
        HIP_TRY(r, r->momentHistory[0].alloc(n));
        HIP_TRY(r, r->momentHistory[1].alloc(n));
    }
    const bool useHistory = r->temporalHistoryIn >= 0 && !(d->flags & PTX_TEMPORAL_RESET);
    const int dst = r->temporalHistoryIn == 0 ? 1 : 0; // the history ping-pongs: a thread reads q while its neighbour writes it
    TemporalArgs a;
    a.sum = imagePtr(r);
    a.normal = guidePtr(r, PTX_GUIDE_NORMAL);
    a.position = guidePtr(r, PTX_GUIDE_POSITION);
    a.albedo = guidePtr(r, PTX_GUIDE_ALBEDO);
    a.histIn = useHistory ? r->temporalHistory[r->temporalHistoryIn].p : nullptr;
    a.histOut = r->temporalHistory[dst].p;
    a.out = r->temporalImage.p;
    a.width = r->frame.width;
    a.height = r->frame.height;
    a.pixels = (uint32_t)n;
    a.totalSamples = (float)d->totalSamples;
    a.maxHistory = d->maxHistory;
    a.normalThreshold2 = d->normalThreshold * d->normalThreshold;
    a.positionThreshold = d->positionThreshold;
    memcpy(a.view, r->temporalView, sizeof a.view);
    memcpy(a.proj, r->temporalProj, sizeof a.proj);
    const bool sameCamera = useHistory && !memcmp(d->View, r->temporalView, sizeof d->View) && !memcmp(d->Proj, r->temporalProj, sizeof d->Proj);
    const dim3 block(kDenoiseTileX, kDenoiseTileY), grid((r->frame.width + kDenoiseTileX - 1) / kDenoiseTileX, (r->frame.height + kDenoiseTileY - 1) / kDenoiseTileY);
    const TemporalMotion mo = { motion ? motionPtr(r, PTX_MOTION_POSITION) : nullptr, motion ? motionPtr(r, PTX_MOTION_NORMAL) : nullptr };
    if (moments)
    {
        // the moment history ping-pongs with the colour's; without a live one the moments restart on the colour history as it stands
        const float4 *momentsIn = useHistory && r->momentsLive ? r->momentHistory[r->temporalHistoryIn].p : nullptr;
        if (motion && sameCamera) k_temporal_moments_motion<true><<<grid, block, 0, r->stream>>>(a, momentsIn, r->momentHistory[dst].p, mo);
        else if (motion) k_temporal_moments_motion<false><<<grid, block, 0, r->stream>>>(a, momentsIn, r->momentHistory[dst].p, mo);
        else if (sameCamera) k_temporal_moments<true><<<grid, block, 0, r->stream>>>(a, momentsIn, r->momentHistory[dst].p);
        else k_temporal_moments<false><<<grid, block, 0, r->stream>>>(a, momentsIn, r->momentHistory[dst].p);
    }
    else if (motion && sameCamera) k_temporal_motion<true><<<grid, block, 0, r->stream>>>(a, mo);
    else if (motion) k_temporal_motion<false><<<grid, block, 0, r->stream>>>(a, mo);
    else if (sameCamera) k_temporal<true><<<grid, block, 0, r->stream>>>(a);
    else k_temporal<false><<<grid, block, 0, r->stream>>>(a);
    HIP_TRY(r, hipGetLastError());
    r->momentsLive = moments;
    r->temporalHistoryIn = dst;
    r->temporalReady = true;
    r->temporalPose = r->guidesPose; // the history now leads back to the pose its guides were rendered at
    memcpy(r->temporalView, d->View, sizeof d->View);
    memcpy(r->temporalProj, d->Proj, sizeof d->Proj);
    return PTX_OK;
}

static int temporalAccumulateMotion(PtxRenderer *r, const PtxTemporalDesc *d, uint32_t withMoments)
{
    if (withMoments > 1u)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "ptx_temporal_accumulate_motion: withMoments is 0 or 1 (%u)", withMoments);
    return temporalAccumulate(r, d, withMoments != 0u, "ptx_temporal_accumulate_motion", true);
}

static int readTemporal(PtxRenderer *r, void *host, size_t bytes)
{
    if (!r || !host)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "ptx_read_temporal: null argument");
    if (!r->temporalReady)
        return fail(r, PTX_ERROR_NOT_READY, "ptx_read_temporal: call ptx_temporal_accumulate first");
    return readFrameImage(r, r->temporalImage.p, host, bytes, "ptx_read_temporal");
}

// ptx_denoise's filter on T, which holds the mean: totalSamples = 1
static int denoiseTemporal(PtxRenderer *r, const PtxDenoiseDesc *d)
{
    if (!r || !d)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "ptx_denoise_temporal: null argument");
    if (!r->temporalReady)
        return fail(r, PTX_ERROR_NOT_READY, "ptx_denoise_temporal: call ptx_temporal_accumulate first");
    return denoise(r, d, r->temporalImage.p, 1u, "ptx_denoise_temporal");
}
