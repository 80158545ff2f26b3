// pt_variance_host.hpp -- host side of the variance-guided denoising (kernels: pt_variance.hpp; semantics: include/ptx.h,
// docs/NEXT_ROWS.md section 16).  Included by pt_runtime.hpp after pt_temporal_host.hpp, whose temporalAccumulate launches the
// moments kernel: here are the estimate and the filter on T, and the read-backs of the moments and V_0.
#pragma once

static int readMoments(PtxRenderer *r, void *host, size_t bytes)
{
    if (!r || !host)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "ptx_read_moments: null argument");
    if (!r->momentsLive)
        return fail(r, PTX_ERROR_NOT_READY, "ptx_read_moments: the last accumulate call was not ptx_temporal_accumulate_moments");
    return readFrameImage(r, r->momentHistory[r->temporalHistoryIn].p, host, bytes, "ptx_read_moments");
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
    if (!imagePtr(r))
        return fail(r, PTX_ERROR_NOT_READY, "%s: no accumulation image (call ptx_resize)", who);
    if (r->frame.boundShard)
        return frameIsElsewhere(r, who);
    if (!r->guidesReady)
        return fail(r, PTX_ERROR_NOT_READY, "%s: no guides for this extent (call ptx_render_guides)", who);
    if (r->frame.shard.worldSize > 1u)
        return fail(r, PTX_ERROR_NOT_READY, "%s: this renderer holds one tile shard of %u; the filter's taps cross tiles", who, r->frame.shard.worldSize);
    if (!r->temporalReady || !r->momentsLive)
        return fail(r, PTX_ERROR_NOT_READY, "%s: the last accumulate call must be ptx_temporal_accumulate_moments", who);
    HIP_TRY(r, hipSetDevice(r->device));
    const size_t n = r->frame.pixels();
    HIP_TRY(r, r->denoisePing[0].alloc(n));
    HIP_TRY(r, r->denoisePing[1].alloc(n));
    HIP_TRY(r, r->varianceImage.alloc(n));
    VarianceArgs a;
    a.temporal = r->temporalImage.p;
    a.moments = r->momentHistory[r->temporalHistoryIn].p;
    a.variance = r->varianceImage.p;
    a.src = nullptr;
    a.dst = r->denoisePing[1].p;
    a.normal = guidePtr(r, PTX_GUIDE_NORMAL);
    a.position = guidePtr(r, PTX_GUIDE_POSITION);
    a.albedo = guidePtr(r, PTX_GUIDE_ALBEDO);
    a.width = r->frame.width;
    a.height = r->frame.height;
    a.step = 1;
    a.invSigmaLuminance2 = (float)(1.0 / ((double)d->sigmaColor * d->sigmaColor));
    a.invSigmaNormal2 = (float)(1.0 / ((double)d->sigmaNormal * d->sigmaNormal));
    a.invSigmaPosition = (float)(1.0 / (double)d->sigmaPosition);
    const dim3 block(kDenoiseTileX, kDenoiseTileY), grid((r->frame.width + kDenoiseTileX - 1) / kDenoiseTileX, (r->frame.height + kDenoiseTileY - 1) / kDenoiseTileY);
    k_variance_estimate<<<grid, block, 0, r->stream>>>(a);
    for (uint32_t i = 0; i < d->iterations; i++)
    {
        a.src = r->denoisePing[(i + 1u) & 1u].p;
        a.dst = r->denoisePing[i & 1u].p;
        a.step = 1 << i;
        if (i + 1u == d->iterations) k_denoise_variance<true><<<grid, block, 0, r->stream>>>(a);
        else k_denoise_variance<false><<<grid, block, 0, r->stream>>>(a);
    }
    HIP_TRY(r, hipGetLastError());
    r->denoisedIn = (int)((d->iterations - 1u) & 1u);
    r->varianceReady = true;
    return PTX_OK;
}

static int readVariance(PtxRenderer *r, void *host, size_t bytes)
{
    if (!r || !host)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "ptx_read_variance: null argument");
    if (!r->varianceReady)
        return fail(r, PTX_ERROR_NOT_READY, "ptx_read_variance: call ptx_denoise_variance first");
    if (bytes != r->frame.pixels() * sizeof(float))
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "ptx_read_variance: buffer must be width*height*4 bytes");
    HIP_TRY(r, hipSetDevice(r->device));
    HIP_TRY(r, hipMemcpyAsync(host, r->varianceImage.p, bytes, hipMemcpyDeviceToHost, r->stream));
    HIP_TRY(r, hipStreamSynchronize(r->stream));
    return collectRender(r);
}
