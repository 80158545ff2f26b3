// pt_output_host.hpp -- the output stage (ptx_postprocess and its calls on C and D, ptx_read_output: row N4) and the screen path
// (ptx_present, ptx_read_present: row D15; docs/NEXT_ROWS.md section 12), the exposure metering in front of them (ptx_meter, ptx_read_meter,
// ptx_meter_reset, ptx_postprocess_metered: section 21), the display transform behind them (ptx_grade, ptx_grade_lut, ptx_present_graded:
// section 22), which runs the output stage's last kernel, or the screen path's, again with a grade in the place of the tone mapping, and
// the local exposure between the meter and the output stage (ptx_local_exposure, ptx_read_local_exposure, ptx_postprocess_local: section 23),
// and the enlarging screen path (ptx_present_upscaled: section 25), which is presentFrame with pt_upscale.hpp's kernel at its end,
// and the noise metering of an offline render's two half-sums (ptx_noise_halves, ptx_noise_meter, ptx_read_noise: section 26) with the
// adaptive sampling it steers (ptx_adaptive_plan, ptx_read_adaptive, ptx_adaptive_clear, ptx_noise_meter_adaptive: section 27).
// What the entry points share stands first: the source rule, the refusal ladder, the read-back's end, ptx_resize's part (section 24).
// Kernels: pt_post.hpp, pt_present.hpp, pt_meter.hpp, pt_grade.hpp, pt_local_exposure.hpp, pt_upscale.hpp, pt_noise.hpp, pt_adaptive.hpp; state: OutputState, the member `output` of the handle.
// Included by pt_runtime.hpp ahead of pt_frame_host.hpp, whose ptx_resize ends in outputResized; every function takes a valid or null
// handle and returns a PTX_* code.
#pragma once

static bool finiteFloat(float v) { return v >= -3.402823466e38f && v <= 3.402823466e38f; } // a NaN fails both

// The source rule: the image a PTX_METER_* source names, as the output call of that source reads it (null: it does not exist for this
// extent), and the sample count its values are divided by.  The sum and C are running sums of the caller's count; D holds the mean.
struct OutputSource
{
    const float4 *image;
    uint32_t totalSamples;
};
static OutputSource outputSource(const PtxRenderer *r, uint32_t source, uint32_t totalSamples)
{
    if (source == PTX_METER_SUM)
        return { imagePtr(r), totalSamples };
    if (source == PTX_METER_DESPIKED)
        return { r->chain.despiked(), totalSamples };
    return { r->chain.denoised(), 1u };
}

// What an entry point needs before its first allocation or launch, in the order it is reported (chainRefusal is the chain's)
enum : uint32_t
{
    NEEDS_OUTPUT = 1u,        // an accepted output call since the last ptx_resize / ptx_render_debug
    NEEDS_FRAME = 2u,         // the accumulation image, and in this renderer: no shard buffer bound
    NEEDS_ONE_SHARD = 4u,     // ... the whole frame, not one tile shard of several
    NEEDS_SOURCE = 8u,        // the image of `source`, in the words of an output call
    NEEDS_SOURCE_IMAGE = 16u, // ... or in those of ptx_meter and ptx_local_exposure
    NEEDS_METER = 32u,        // an accepted ptx_meter on this handle
    NEEDS_GAIN = 64u          // G: an accepted ptx_local_exposure since the last ptx_resize
};
static int outputRefusal(PtxRenderer *r, const char *who, uint32_t needs, uint32_t source = PTX_METER_SUM)
{
    if ((needs & NEEDS_OUTPUT) && !r->output.ready)
        return fail(r, PTX_ERROR_NOT_READY, "%s: call ptx_postprocess first", who);
    if ((needs & NEEDS_FRAME) && !imagePtr(r))
        return fail(r, PTX_ERROR_NOT_READY, "%s: no accumulation image (call ptx_resize)", who);
    if ((needs & NEEDS_FRAME) && r->frame.boundShard)
        return frameIsElsewhere(r, who);
    if ((needs & NEEDS_ONE_SHARD) && r->frame.shard.worldSize > 1u)
        return fail(r, PTX_ERROR_NOT_READY, "%s: this renderer holds one tile shard of %u", who, r->frame.shard.worldSize);
    if ((needs & (NEEDS_SOURCE | NEEDS_SOURCE_IMAGE)) && !outputSource(r, source, 1u).image)
    {
        const bool c = source == PTX_METER_DESPIKED;
        if (needs & NEEDS_SOURCE)
            return fail(r, PTX_ERROR_NOT_READY, "%s: call %s first", who, c ? "ptx_despike" : "ptx_denoise");
        return fail(r, PTX_ERROR_NOT_READY, "%s: no %s image for this extent (call %s first)", who, c ? "despiked" : "denoised", c ? "ptx_despike" : "ptx_denoise");
    }
    if ((needs & NEEDS_METER) && !r->output.meterState.p)
        return fail(r, PTX_ERROR_NOT_READY, "%s: call ptx_meter first", who);
    if ((needs & NEEDS_GAIN) && !r->output.localReady)
        return fail(r, PTX_ERROR_NOT_READY, "%s: call ptx_local_exposure first", who);
    return PTX_OK;
}

// the end of every synchronous read-back of this file: the last copy on the render stream, the wait, and what the launches left
static int readBack(PtxRenderer *r, void *host, const void *device, size_t bytes)
{
    HIP_TRY(r, hipMemcpyAsync(host, device, bytes, hipMemcpyDeviceToHost, r->stream));
    HIP_TRY(r, hipStreamSynchronize(r->stream));
    HIP_TRY(r, hipGetLastError());
    return PTX_OK;
}

// The bloom chain's levels for a W x H frame, laid end to end from `base` (null: the extents and the size alone).  Mips 0 .. maxMipLevel - 1
// take part, maxMipLevel = min(levels - 3, MaxBloomMipmapLevel) (Renderer.cpp:955-956).
struct BloomPlan
{
    BloomLevel level[13];
    uint32_t used;
    size_t floats; // of the whole chain
};
static BloomPlan bloomPlan(uint32_t W, uint32_t H, float *base)
{
    uint32_t levels = 1;
    for (uint32_t m = W > H ? W : H; m > 1; m >>= 1)
        levels++;
    BloomPlan b;
    b.used = levels >= 5 ? (levels - 3 < 12 ? levels - 3 : 12) : 1;
    b.floats = 0;
    for (uint32_t l = 0; l < b.used; l++)
    {
        b.level[l].w = (W >> l) ? (W >> l) : 1;
        b.level[l].h = (H >> l) ? (H >> l) : 1;
        b.level[l].rgb = base ? base + b.floats : nullptr;
        b.floats += (size_t)b.level[l].w * b.level[l].h * 3;
    }
    return b;
}

// Renderer::RecordPostProcessCommands + RecordSaveOutputCommands (Renderer.cpp:928-1085, :1204-1246)
// the chain on `source` (width x height running sums of uniform->TotalSamples samples): the accumulation image, or the denoised mean
// meterExposure: the device address of the metered exposure that ptx_postprocess_metered multiplies in (k_postprocess_metered), or none
// localGain: G of ptx_local_exposure, which ptx_postprocess_local multiplies in per pixel (k_postprocess_local), or none
static int postprocessImage(PtxRenderer *r, const float4 *source, const PtxPostProcessingUniformData *uniform, uint32_t toneMappingMode,
                            const float *meterExposure, const float *localGain)
{
    HIP_TRY(r, hipSetDevice(r->device));
    OutputState &o = r->output;
    const uint32_t W = r->frame.width, H = r->frame.height, n = W * H;
    HIP_TRY(r, o.postRgb.alloc((size_t)n * 3));
    HIP_TRY(r, o.bloomRgb.alloc(bloomPlan(W, H, nullptr).floats));
    HIP_TRY(r, o.outLinear.alloc(n));
    const BloomPlan b = bloomPlan(W, H, o.bloomRgb.p);
    const BloomLevel *L = b.level;
    if (localGain)
        k_postprocess_local<<<gridFor(n), kBlock, 0, r->stream>>>(source, n, *uniform, meterExposure, localGain, o.postRgb.p, L[0].rgb);
    else if (meterExposure)
        k_postprocess_metered<<<gridFor(n), kBlock, 0, r->stream>>>(source, n, *uniform, meterExposure, o.postRgb.p, L[0].rgb);
    else
        k_postprocess<<<gridFor(n), kBlock, 0, r->stream>>>(source, n, *uniform, o.postRgb.p, L[0].rgb);
    for (uint32_t i = 0; i + 1 < b.used; i++)
        k_bloom_downsample<<<gridFor((size_t)L[i + 1].w * L[i + 1].h), kBlock, 0, r->stream>>>(L[i], L[i + 1]);
    for (uint32_t i = b.used - 1; i > 0; i--)
        k_bloom_upsample<<<gridFor((size_t)L[i - 1].w * L[i - 1].h), kBlock, 0, r->stream>>>(L[i], L[i - 1]);
    k_compose_tonemap<<<gridFor(n), kBlock, 0, r->stream>>>(o.postRgb.p, L[0].rgb, n, *uniform, toneMappingMode, o.outLinear.p);
    HIP_TRY(r, hipGetLastError());
    o.postUniform = *uniform;
    o.ready = true;
    return PTX_OK;
}

// The five output calls are one: the chain on the image of `source`, which is all the plain call of that source needs (ptx_postprocess
// the sum in this renderer, ptx_postprocess_despiked C, ptx_postprocess_denoised D), with the metered exposure multiplied in on the
// device (`metered`: ptx_postprocess_metered) and G per pixel, Exposure = (uniform->Exposure x m) x G(p) (`local`: ptx_postprocess_local;
// G covers the frame, a shard's image does not)
static int postprocessSource(PtxRenderer *r, const char *who, const PtxPostProcessingUniformData *uniform, uint32_t toneMappingMode, uint32_t source,
                             bool metered = false, bool local = false)
{
    if (!r || !uniform || toneMappingMode > PTX_TONE_MAPPING_HDR || source > PTX_METER_DENOISED)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "%s: bad argument", who);
    const uint32_t needs = (source == PTX_METER_SUM ? NEEDS_FRAME : NEEDS_SOURCE) | (metered ? NEEDS_METER : 0u) | (local ? NEEDS_ONE_SHARD | NEEDS_GAIN : 0u);
    if (const int rc = outputRefusal(r, who, needs, source))
        return rc;
    const OutputSource s = outputSource(r, source, uniform->TotalSamples);
    PtxPostProcessingUniformData u = *uniform;
    u.TotalSamples = s.totalSamples;
    return postprocessImage(r, s.image, &u, toneMappingMode, metered ? &r->output.meterState.p->result.exposure : nullptr,
                            local ? r->output.localGain.p : nullptr);
}

static int postprocessLocal(PtxRenderer *r, const PtxPostProcessingUniformData *uniform, uint32_t toneMappingMode, uint32_t source, uint32_t metered)
{
    if (metered > 1u)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "ptx_postprocess_local: bad argument");
    return postprocessSource(r, "ptx_postprocess_local", uniform, toneMappingMode, source, metered != 0u, true);
}

// OutputSaver: blit of the tone-mapped image into its output image + readback (OutputSaver.cpp:64-86, :120-199)
static int readOutput(PtxRenderer *r, uint32_t outputFormat, void *host, size_t bytes)
{
    if (!r || !host || outputFormat > PTX_OUTPUT_RGBA32F)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "ptx_read_output: bad argument");
    if (const int rc = outputRefusal(r, "ptx_read_output", NEEDS_OUTPUT))
        return rc;
    const uint32_t n = r->frame.width * r->frame.height;
    const size_t want = (size_t)n * (outputFormat == PTX_OUTPUT_RGBA32F ? 16 : 4);
    if (bytes != want)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "ptx_read_output: buffer must be %zu bytes", want);
    HIP_TRY(r, hipSetDevice(r->device));
    if (outputFormat == PTX_OUTPUT_RGBA32F)
        return readBack(r, host, r->output.outLinear.p, bytes);
    HIP_TRY(r, r->output.outSrgb8.alloc(n));
    k_encode_srgb8<<<gridFor(n), kBlock, 0, r->stream>>>(r->output.outLinear.p, n, r->output.outSrgb8.p);
    return readBack(r, host, r->output.outSrgb8.p, bytes);
}

// the five (surface format, HDR) pairs presentFrame lets through, as compile-time constants: f(format, hdr)
template <typename F> static void withPresentFormat(uint32_t format, bool hdr, F &&f)
{
    switch (format)
    {
    case PTX_PRESENT_R8G8B8A8_SRGB: f(std::integral_constant<uint32_t, PTX_PRESENT_R8G8B8A8_SRGB>(), std::false_type()); break;
    case PTX_PRESENT_B8G8R8A8_SRGB: f(std::integral_constant<uint32_t, PTX_PRESENT_B8G8R8A8_SRGB>(), std::false_type()); break;
    case PTX_PRESENT_A2B10G10R10_UNORM: f(std::integral_constant<uint32_t, PTX_PRESENT_A2B10G10R10_UNORM>(), std::true_type()); break;
    default: withFlag(hdr, [&](auto Hdr) { f(std::integral_constant<uint32_t, PTX_PRESENT_R16G16B16A16_SFLOAT>(), Hdr); });
    }
}

static GradeArgs gradeArgs(const PtxRenderer *r, const PtxGradeDesc &d, bool hdr); // below: the display transform

// The screen path: RecordPostProcessCommands' final blit + RecordUICommands (Renderer.cpp:1075-1203) in one launch of k_present, or, for
// ptx_present_graded (`graded`, section 22), of k_present_graded with the desc the last accepted ptx_grade left.  ptx_present_upscaled
// (`upscaled`, section 25; `up` may be null and is then refused) takes the same road -- the desc's refusals, its own, the ladder, the
// image, the UI -- and ends in one launch of k_present_upscaled instead, unless its skip rule leaves exactly the plain launch.
static int presentFrame(PtxRenderer *r, const PtxPresentDesc *d, const char *who, bool graded, bool upscaled = false, const PtxUpscaleDesc *up = nullptr)
{
    if (!r || !d)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "%s: null argument", who);
    if (!d->width || !d->height || d->width > 16384u || d->height > 16384u)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "%s: bad screen extent %ux%u (1 .. 16384 each)", who, d->width, d->height);
    if (d->format > PTX_PRESENT_R16G16B16A16_SFLOAT || d->toneMappingMode > PTX_TONE_MAPPING_HDR || (d->flags & ~(uint32_t)PTX_PRESENT_UI_ON_DEVICE) || d->reserved)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "%s: unknown format %u, mode %u or flags 0x%x, or reserved != 0", who, d->format, d->toneMappingMode, d->flags);
    const bool hdr = d->toneMappingMode == PTX_TONE_MAPPING_HDR;
    if ((hdr && d->format <= PTX_PRESENT_B8G8R8A8_SRGB) || (!hdr && d->format == PTX_PRESENT_A2B10G10R10_UNORM))
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "%s: an 8-bit sRGB surface is SDR and A2B10G10R10 is HDR10 (Swapchain.cpp:317-340)", who);
    if (upscaled)
    {
        if (!up)
            return fail(r, PTX_ERROR_INVALID_ARGUMENT, "%s: null PtxUpscaleDesc", who);
        if (up->filter != PTX_UPSCALE_CATMULL_ROM || (up->flags & ~(uint32_t)PTX_UPSCALE_GRADED) || up->reserved)
            return fail(r, PTX_ERROR_INVALID_ARGUMENT, "%s: unknown filter %u or flags 0x%x, or reserved != 0 (%u)", who, up->filter, up->flags, up->reserved);
        if (!finiteFloat(up->sharpness) || up->sharpness < 0.0f || up->sharpness > 2.0f)
            return fail(r, PTX_ERROR_INVALID_ARGUMENT, "%s: need a finite sharpness in 0 .. 2 (%g)", who, (double)up->sharpness);
        graded = (up->flags & PTX_UPSCALE_GRADED) != 0u;
    }
    if (const int rc = outputRefusal(r, who, NEEDS_OUTPUT | NEEDS_FRAME | (graded ? NEEDS_ONE_SHARD : 0u)))
        return rc;
    OutputState &o = r->output;
    if (graded && !o.gradeSet)
        return fail(r, PTX_ERROR_NOT_READY, "%s: call ptx_grade first", who);
    if (graded && (o.gradeDesc.flags & PTX_GRADE_USE_LUT) && !o.gradeLut.p)
        return fail(r, PTX_ERROR_NOT_READY, "%s: the kept desc uses a LUT and the LUT has been cleared (ptx_grade_lut)", who);
    if (upscaled && (d->width < r->frame.width || d->height < r->frame.height))
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "%s: the screen extent %ux%u is below the render extent %ux%u on an axis (a smaller window is ptx_present's)", who,
                    d->width, d->height, r->frame.width, r->frame.height);
    // the skip rule: whether step 5 runs, bit for bit, and whether anything but the plain launch is left
    uint32_t sharpnessBits = 0u;
    if (upscaled)
        memcpy(&sharpnessBits, &up->sharpness, 4);
    const bool sharpen = sharpnessBits != 0u;
    const bool enlarge = upscaled && (sharpen || d->width != r->frame.width || d->height != r->frame.height);
    HIP_TRY(r, hipSetDevice(r->device));
    const uint32_t n = d->width * d->height;
    const size_t words = (size_t)n * (d->format == PTX_PRESENT_R16G16B16A16_SFLOAT ? 2 : 1);
    if (words > o.presentImage.n || !o.presentImage.p) // a failed allocation keeps the previous image
    {
        DevBuf<uint32_t> grown;
        HIP_TRY(r, grown.alloc(words));
        o.presentImage.swap(grown);
    }
    PresentArgs a;
    a.post = o.postRgb.p;
    a.bloom0 = o.bloomRgb.p; // level 0 of the chain
    a.ui = static_cast<const uint32_t *>(d->ui);
    a.out = o.presentImage.p;
    a.u = o.postUniform;
    a.W = r->frame.width; a.H = r->frame.height; a.SW = d->width; a.SH = d->height;
    if (d->ui && !(d->flags & PTX_PRESENT_UI_ON_DEVICE))
    {
        HIP_TRY(r, o.presentUi.alloc(n));
        HIP_TRY(r, hipMemcpyAsync(o.presentUi.p, d->ui, (size_t)n * 4, hipMemcpyHostToDevice, r->stream));
        a.ui = o.presentUi.p;
    }
    const uint32_t grid = (n + kPresentBlock - 1) / kPresentBlock;
    withPresentFormat(d->format, hdr, [&](auto Format, auto Hdr) {
        constexpr uint32_t format = decltype(Format)::value;
        constexpr bool isHdr = decltype(Hdr)::value;
        if (enlarge)
        {
            const dim3 tiles((d->width + kUpscaleTileX - 1) / kUpscaleTileX, (d->height + kUpscaleTileY - 1) / kUpscaleTileY); // <= 512 x 2048
            withFlag(sharpen, [&](auto Sharpen) {
                constexpr bool sh = decltype(Sharpen)::value;
                if (graded)
                    k_present_upscaled<format, isHdr, sh, GradeArgs><<<tiles, kUpscaleBlock, 0, r->stream>>>(a, up->sharpness, gradeArgs(r, o.gradeDesc, hdr));
                else
                    k_present_upscaled<format, isHdr, sh, ToneMap><<<tiles, kUpscaleBlock, 0, r->stream>>>(
                        a, up->sharpness, ToneMap{ isHdr ? (uint32_t)PTX_TONE_MAPPING_HDR : (uint32_t)PTX_TONE_MAPPING_SDR });
            });
        }
        else if (graded)
            k_present_graded<format, isHdr><<<grid, kPresentBlock, 0, r->stream>>>(a, gradeArgs(r, o.gradeDesc, hdr));
        else
            k_present<format, isHdr><<<grid, kPresentBlock, 0, r->stream>>>(a);
    });
    HIP_TRY(r, hipGetLastError());
    o.presentWidth = d->width;
    o.presentHeight = d->height;
    o.presentFormat = d->format;
    o.presentBytes = words * 4;
    return PTX_OK;
}

static int readPresent(PtxRenderer *r, void *host, size_t bytes)
{
    if (!r || !host)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "ptx_read_present: null argument");
    if (!r->output.presentBytes)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "ptx_read_present: nothing presented yet (call ptx_present)");
    if (bytes != r->output.presentBytes)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "ptx_read_present: buffer must be %zu bytes", r->output.presentBytes);
    HIP_TRY(r, hipSetDevice(r->device));
    return readBack(r, host, r->output.presentImage.p, bytes);
}

// ---- exposure metering (docs/NEXT_ROWS.md section 21; semantics: include/ptx.h ptx_meter; kernels: pt_meter.hpp) --------------------

// ptx_meter_reset, and ptx_resize's part in it: nothing to do while no ptx_meter has made a state
static int meterReset(PtxRenderer *r)
{
    if (!r)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "ptx_meter_reset: null argument");
    if (!r->output.meterState.p)
        return PTX_OK;
    HIP_TRY(r, hipSetDevice(r->device));
    k_meter_reset<<<1, kMeterBlock, 0, r->stream>>>(r->output.meterState.p);
    HIP_TRY(r, hipGetLastError());
    return PTX_OK;
}

// ptx_meter: the histogram's slabs, then one workgroup that sums them and moves the exposure.  Two launches, no synchronisation.
static int meter(PtxRenderer *r, const PtxMeterDesc *d)
{
    const char *who = "ptx_meter";
    if (!r || !d)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "%s: null argument", who);
    if (d->source > PTX_METER_DENOISED || d->mode > PTX_METER_REGION || !d->totalSamples || (uint64_t)d->lowPermille + d->highPermille >= 1000u ||
        d->flags != 0u || d->reserved != 0u)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "%s: need source <= 2 (%u), mode <= 2 (%u), totalSamples > 0 (%u), lowPermille + highPermille < 1000 "
                    "(%u + %u), flags 0 (0x%x) and reserved 0 (%u)", who, d->source, d->mode, d->totalSamples, d->lowPermille, d->highPermille, d->flags, d->reserved);
    if (!finiteFloat(d->keyLog2) || !finiteFloat(d->compensation) || !finiteFloat(d->minLog2Exposure) || !finiteFloat(d->maxLog2Exposure) ||
        !finiteFloat(d->speedUp) || !finiteFloat(d->speedDown) || !finiteFloat(d->deltaSeconds) || d->minLog2Exposure > d->maxLog2Exposure || d->speedUp < 0.0f ||
        d->speedDown < 0.0f || d->deltaSeconds < 0.0f)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "%s: need finite keyLog2 (%g) and compensation (%g), finite minLog2Exposure <= maxLog2Exposure (%g, %g), "
                    "finite speedUp, speedDown and deltaSeconds >= 0 (%g, %g, %g)", who, (double)d->keyLog2, (double)d->compensation, (double)d->minLog2Exposure,
                    (double)d->maxLog2Exposure, (double)d->speedUp, (double)d->speedDown, (double)d->deltaSeconds);
    if (const int rc = outputRefusal(r, who, NEEDS_FRAME))
        return rc;
    if (r->frame.shard.worldSize > 1u) // the ladder's rung, with the way out
        return fail(r, PTX_ERROR_NOT_READY, "%s: this renderer holds one tile shard of %u; sum the bins of ptx_read_meter across ranks on the host", who,
                    r->frame.shard.worldSize);
    // the header puts the checks against the extent between the frame's rungs and the source's
    const uint32_t W = r->frame.width, H = r->frame.height;
    const uint32_t *g = d->region;
    if (d->mode == PTX_METER_REGION && (g[0] >= g[1] || g[2] >= g[3] || g[1] > W || g[3] > H))
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "%s: the region [%u, %u) x [%u, %u) is empty or leaves the %u x %u image", who, g[0], g[1], g[2], g[3], W, H);
    // step 4: the largest total a counter can reach
    const uint64_t total = d->mode == PTX_METER_REGION ? (uint64_t)(g[1] - g[0]) * (g[3] - g[2]) : (uint64_t)W * H * (d->mode == PTX_METER_CENTRE ? 9u : 1u);
    if (total >= (1ull << 32))
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "%s: the weights of a %u x %u image can sum to %llu, which a 32-bit counter does not hold", who, W, H,
                    (unsigned long long)total);
    if (const int rc = outputRefusal(r, who, NEEDS_SOURCE_IMAGE, d->source))
        return rc;
    const OutputSource s = outputSource(r, d->source, d->totalSamples);
    HIP_TRY(r, hipSetDevice(r->device));
    OutputState &o = r->output;
    HIP_TRY(r, o.meterSlabs.alloc((size_t)kMeterGridCap * kMeterSlabWords));
    if (!o.meterState.p)
    {
        HIP_TRY(r, o.meterState.alloc(1));
        k_meter_reset<<<1, kMeterBlock, 0, r->stream>>>(o.meterState.p);
    }
    MeterArgs a;
    a.source = s.image;
    a.slabs = o.meterSlabs.p;
    a.n = W * H;
    a.width = W;
    a.height = H;
    a.totalSamples = (float)s.totalSamples;
    a.x0 = g[0]; a.x1 = g[1]; a.y0 = g[2]; a.y1 = g[3];
    const uint32_t grid = gridFor(a.n, kMeterBlock, kMeterGridCap);
    switch (d->mode)
    {
    case PTX_METER_AVERAGE: k_meter_histogram<PTX_METER_AVERAGE><<<grid, kMeterBlock, 0, r->stream>>>(a); break;
    case PTX_METER_CENTRE: k_meter_histogram<PTX_METER_CENTRE><<<grid, kMeterBlock, 0, r->stream>>>(a); break;
    default: k_meter_histogram<PTX_METER_REGION><<<grid, kMeterBlock, 0, r->stream>>>(a);
    }
    MeterResolveArgs v;
    v.slabs = o.meterSlabs.p;
    v.slabCount = grid;
    v.state = o.meterState.p;
    v.lowPermille = d->lowPermille;
    v.highPermille = d->highPermille;
    v.keyLog2 = d->keyLog2;
    v.compensation = d->compensation;
    v.minLog2Exposure = d->minLog2Exposure;
    v.maxLog2Exposure = d->maxLog2Exposure;
    v.speedUp = d->speedUp;
    v.speedDown = d->speedDown;
    v.deltaSeconds = d->deltaSeconds;
    k_meter_resolve<<<1, kMeterResolveBlock, 0, r->stream>>>(v);
    HIP_TRY(r, hipGetLastError());
    return PTX_OK;
}

static int readMeter(PtxRenderer *r, PtxMeterResult *out, uint32_t *bins256)
{
    if (!r || !out)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "ptx_read_meter: null argument");
    if (const int rc = outputRefusal(r, "ptx_read_meter", NEEDS_METER))
        return rc;
    HIP_TRY(r, hipSetDevice(r->device));
    const MeterState *st = r->output.meterState.p;
    if (!bins256)
        return readBack(r, out, &st->result, sizeof(PtxMeterResult));
    HIP_TRY(r, hipMemcpyAsync(out, &st->result, sizeof(PtxMeterResult), hipMemcpyDeviceToHost, r->stream));
    return readBack(r, bins256, st->bins, sizeof(st->bins));
}

// ---- display transform (docs/NEXT_ROWS.md section 22; semantics: include/ptx.h ptx_grade; kernels: pt_grade.hpp) ---------------------

// the skip rule: which steps of the header run for this desc and mode, decided here, bit for bit, and handed to the kernel as switches
static GradeArgs gradeArgs(const PtxRenderer *r, const PtxGradeDesc &d, bool hdr)
{
    const auto bits = [](float f) { uint32_t u; memcpy(&u, &f, 4); return u; };
    const uint32_t one = 0x3f800000u;
    GradeArgs g;
    uint32_t steps = 0u;
    for (int i = 0; i < 9; i++)
    {
        g.m[i] = d.colourMatrix[i];
        if (bits(d.colourMatrix[i]) != (i % 4 == 0 ? one : 0u))
            steps |= GRADE_STEP_MATRIX;
    }
    for (int k = 0; k < 3; k++)
    {
        g.slope[k] = d.slope[k]; g.offset[k] = d.offset[k]; g.power[k] = d.power[k];
        if (bits(d.slope[k]) != one || bits(d.offset[k]) != 0u)
            steps |= GRADE_STEP_SLOPE_OFFSET;
        if (bits(d.power[k]) != one)
            steps |= GRADE_STEP_POWER;
    }
    if (bits(d.saturation) != one)
        steps |= GRADE_STEP_SATURATION;
    if (!hdr)
    {
        steps |= GRADE_STEP_CURVE;
        if (d.flags & PTX_GRADE_USE_LUT)
            steps |= GRADE_STEP_LUT | (d.flags & PTX_GRADE_LUT_SRGB_DOMAIN ? GRADE_STEP_LUT_SRGB : 0u);
    }
    g.saturation = d.saturation;
    g.whitePoint = d.whitePoint;
    g.curve = d.curve;
    g.steps = steps;
    g.lut = steps & GRADE_STEP_LUT ? r->output.gradeLut.p : nullptr;
    g.lutSize = r->output.gradeLutSize;
    return g;
}

// ptx_grade: k_compose_tonemap's launch with k_compose_grade in its place, on what the last output call left
static int grade(PtxRenderer *r, const PtxGradeDesc *d, uint32_t toneMappingMode)
{
    const char *who = "ptx_grade";
    if (!r || !d)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "%s: null argument", who);
    if (d->curve > PTX_CURVE_ACES_FIT || toneMappingMode > PTX_TONE_MAPPING_HDR || (d->flags & ~(uint32_t)(PTX_GRADE_USE_LUT | PTX_GRADE_LUT_SRGB_DOMAIN)) ||
        d->reserved != 0u)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "%s: unknown curve %u, mode %u or flags 0x%x, or reserved != 0 (%u)", who, d->curve, toneMappingMode, d->flags,
                    d->reserved);
    bool ok = finiteFloat(d->saturation) && finiteFloat(d->whitePoint) && d->saturation >= 0.0f;
    for (int i = 0; i < 9; i++)
        ok = ok && finiteFloat(d->colourMatrix[i]);
    for (int k = 0; k < 3; k++)
        ok = ok && finiteFloat(d->slope[k]) && finiteFloat(d->offset[k]) && finiteFloat(d->power[k]) && d->slope[k] >= 0.0f && d->power[k] >= 0.0f;
    if (!ok)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "%s: every float field must be finite, and slope, power and saturation >= 0", who);
    if (d->curve == PTX_CURVE_REINHARD && !(d->whitePoint > 0.0f))
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "%s: PTX_CURVE_REINHARD needs whitePoint > 0 (%g)", who, (double)d->whitePoint);
    if ((d->flags & PTX_GRADE_LUT_SRGB_DOMAIN) && !(d->flags & PTX_GRADE_USE_LUT))
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "%s: PTX_GRADE_LUT_SRGB_DOMAIN needs PTX_GRADE_USE_LUT", who);
    if (const int rc = outputRefusal(r, who, NEEDS_OUTPUT | NEEDS_FRAME | NEEDS_ONE_SHARD))
        return rc;
    OutputState &o = r->output;
    if ((d->flags & PTX_GRADE_USE_LUT) && !o.gradeLut.p)
        return fail(r, PTX_ERROR_NOT_READY, "%s: PTX_GRADE_USE_LUT and no LUT set (call ptx_grade_lut)", who);
    HIP_TRY(r, hipSetDevice(r->device));
    const uint32_t n = r->frame.width * r->frame.height;
    const GradeArgs g = gradeArgs(r, *d, toneMappingMode == PTX_TONE_MAPPING_HDR);
    // postRgb, level 0 of bloomRgb and outLinear are those of the output call that set `ready`, at this extent
    k_compose_grade<<<gridFor(n), kBlock, 0, r->stream>>>(o.postRgb.p, o.bloomRgb.p, n, o.postUniform, g, o.outLinear.p);
    HIP_TRY(r, hipGetLastError());
    o.gradeDesc = *d;
    o.gradeSet = true;
    return PTX_OK;
}

// ptx_grade_lut: the table goes into a buffer of its own first and takes the old one's place once it has arrived, so a kernel still
// in flight reads the LUT it was launched with and a failed call leaves that LUT where it is
static int setGradeLut(PtxRenderer *r, uint32_t size, const float *rgb)
{
    const char *who = "ptx_grade_lut";
    if (!r)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "%s: null argument", who);
    if (rgb && (size < PTX_GRADE_LUT_MIN_SIZE || size > PTX_GRADE_LUT_MAX_SIZE))
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "%s: size %u outside %u .. %u", who, size, PTX_GRADE_LUT_MIN_SIZE, PTX_GRADE_LUT_MAX_SIZE);
    HIP_TRY(r, hipSetDevice(r->device));
    DevBuf<float> table;
    if (rgb)
    {
        const size_t count = (size_t)size * size * size * 3u;
        HIP_TRY(r, table.alloc(count));
        HIP_TRY(r, hipMemcpyAsync(table.p, rgb, count * sizeof(float), hipMemcpyHostToDevice, r->stream));
    }
    HIP_TRY(r, hipStreamSynchronize(r->stream)); // the copy has landed, and nothing in flight reads the table that is about to go
    r->output.gradeLut.swap(table);
    r->output.gradeLutSize = rgb ? size : 0u;
    return PTX_OK;
}

// ---- local exposure (docs/NEXT_ROWS.md section 23; semantics: include/ptx.h ptx_local_exposure; kernels: pt_local_exposure.hpp) -------

// ptx_local_exposure: splat, blur, gain.  Three launches, no synchronisation; every refusal comes before the first allocation or
// launch, so a refused call leaves G as it was.
static int localExposure(PtxRenderer *r, const PtxLocalExposureDesc *d)
{
    const char *who = "ptx_local_exposure";
    if (!r || !d)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "%s: null argument", who);
    if (d->source > PTX_METER_DENOISED || !d->totalSamples || d->cellShift < kLocalMinShift || d->cellShift > kLocalMaxShift ||
        (d->flags & ~(uint32_t)PTX_LOCAL_EXPOSURE_PIVOT_METERED) || d->reserved != 0u)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "%s: need source <= 2 (%u), totalSamples > 0 (%u), cellShift in 3 .. 6 (%u), no unknown flag (0x%x) and "
                    "reserved 0 (%u)", who, d->source, d->totalSamples, d->cellShift, d->flags, d->reserved);
    if (!finiteFloat(d->pivotLog2) || !finiteFloat(d->highlightContrast) || !finiteFloat(d->shadowContrast) || !finiteFloat(d->maxStops) ||
        d->highlightContrast < 0.0f || d->highlightContrast > 2.0f || d->shadowContrast < 0.0f || d->shadowContrast > 2.0f || d->maxStops < 0.0f)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "%s: need a finite pivotLog2 (%g), highlightContrast and shadowContrast in 0 .. 2 (%g, %g) and a finite "
                    "maxStops >= 0 (%g)", who, (double)d->pivotLog2, (double)d->highlightContrast, (double)d->shadowContrast, (double)d->maxStops);
    if (const int rc = outputRefusal(r, who, NEEDS_FRAME | NEEDS_ONE_SHARD | NEEDS_SOURCE_IMAGE, d->source))
        return rc;
    OutputState &o = r->output;
    const bool metered = (d->flags & PTX_LOCAL_EXPOSURE_PIVOT_METERED) != 0u;
    if (metered && !o.meterState.p)
        return fail(r, PTX_ERROR_NOT_READY, "%s: PTX_LOCAL_EXPOSURE_PIVOT_METERED and no accepted ptx_meter on this handle yet", who);
    const OutputSource src = outputSource(r, d->source, d->totalSamples);
    HIP_TRY(r, hipSetDevice(r->device));
    const uint32_t W = r->frame.width, H = r->frame.height, s = d->cellShift;
    const uint32_t nx = (W + (1u << s) - 1u) >> s, ny = (H + (1u << s) - 1u) >> s;
    const size_t entries = (size_t)nx * ny * kLocalSlices;
    // the grid grows with a smaller cellShift; G has one size per extent (ptx_resize releases both), so a G that exists is never reallocated
    HIP_TRY(r, o.localGrid.alloc(2u * entries));
    HIP_TRY(r, o.localGain.alloc((size_t)W * H));
    LocalSplatArgs a;
    a.source = src.image;
    a.grid = o.localGrid.p;
    a.width = W; a.height = H; a.shift = s; a.nx = nx; a.ny = ny;
    a.totalSamples = (float)src.totalSamples;
    const uint32_t block = 1u << kLocalBlockShift;
    k_local_splat<<<dim3((W + block - 1u) / block, (H + block - 1u) / block), kLocalSplatThreads, 0, r->stream>>>(a);
    k_local_blur<<<(uint32_t)((entries + 255u) / 256u), 256, 0, r->stream>>>(o.localGrid.p, o.localGrid.p + entries, nx, ny);
    LocalGainArgs g;
    g.source = src.image;
    g.grid = o.localGrid.p + entries;
    g.gain = o.localGain.p;
    g.meterCur = metered ? &o.meterState.p->cur : nullptr;
    g.width = W; g.height = H; g.shift = s; g.nx = nx; g.ny = ny;
    g.totalSamples = a.totalSamples;
    g.pivotLog2 = d->pivotLog2;
    g.highlightContrast = d->highlightContrast;
    g.shadowContrast = d->shadowContrast;
    g.maxStops = d->maxStops;
    k_local_gain<<<dim3((W + kDenoiseTileX - 1) / kDenoiseTileX, (H + kDenoiseTileY - 1) / kDenoiseTileY), dim3(kDenoiseTileX, kDenoiseTileY), 0, r->stream>>>(g);
    HIP_TRY(r, hipGetLastError());
    o.localReady = true;
    return PTX_OK;
}

static int readLocalExposure(PtxRenderer *r, void *host, size_t bytes)
{
    if (!r || !host)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "ptx_read_local_exposure: null argument");
    if (const int rc = outputRefusal(r, "ptx_read_local_exposure", NEEDS_GAIN))
        return rc;
    const size_t want = (size_t)r->frame.width * r->frame.height * sizeof(float);
    if (bytes != want)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "ptx_read_local_exposure: buffer must be %zu bytes", want);
    HIP_TRY(r, hipSetDevice(r->device));
    return readBack(r, host, r->output.localGain.p, bytes);
}

// ---- noise metering (docs/NEXT_ROWS.md section 26; semantics: include/ptx.h ptx_noise_meter; kernels: pt_noise.hpp) ------------------

// ptx_noise_halves: the two images a host binds in turn.  Nothing here touches the render path: a half is bound with
// ptx_bind_accumulation like any buffer of the caller's.
static void dropNoiseHalves(PtxRenderer *r)
{
    OutputState::NoiseState &s = r->output.noise;
    for (DevBuf<float4> &h : s.half)
    {
        if (h.p && r->frame.boundImage == h.p) // the binding returns to the internal image
            r->frame.boundImage = nullptr;
        h.release();
    }
}

// What ptx_resize, a ptx_set_tile_shard that changes the shard and ptx_noise_halves(0) do to adaptive sampling: plan and counts go.
static void dropAdaptive(PtxRenderer *r)
{
    OutputState::AdaptiveState &s = r->output.adaptive;
    s.counts.release();
    s.list.release();
    s.active.release();
    s.seed.release();
    s.mask.release();
    s.result.release();
    s.plan = {};
    s.tileShift = s.generation = 0u;
    s.planned = s.counted = false;
}

static int noiseHalves(PtxRenderer *r, uint32_t enable)
{
    const char *who = "ptx_noise_halves";
    if (!r || enable > 1u)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "%s: need a handle and enable 0 or 1", who);
    if (!enable)
    {
        if (r->output.noise.half[0].p || r->output.noise.half[1].p)
            HIP_TRY(r, hipSetDevice(r->device));
        dropNoiseHalves(r);
        dropAdaptive(r);
        return PTX_OK;
    }
    if (!r->frame.width)
        return fail(r, PTX_ERROR_NOT_READY, "%s: call ptx_resize first", who);
    HIP_TRY(r, hipSetDevice(r->device));
    OutputState::NoiseState &s = r->output.noise;
    for (DevBuf<float4> &h : s.half)
    {
        const hipError_t e = h.alloc(r->frame.pixels());
        if (e != hipSuccess)
        {
            dropNoiseHalves(r); // both or none
            HIP_TRY(r, e);
        }
    }
    for (DevBuf<float4> &h : s.half)
        HIP_TRY(r, hipMemsetAsync(h.p, 0, r->frame.bytes(), r->stream));
    OutputState::AdaptiveState &ad = r->output.adaptive;
    if (ad.tileShift) // the halves start over, and so do the frames counted in them
    {
        HIP_TRY(r, hipMemsetAsync(ad.counts.p, 0, 2u * (size_t)ad.numTiles() * sizeof(uint32_t), r->stream));
        ad.counted = false;
    }
    return PTX_OK;
}

// ptx_noise_meter: the tiles, then one workgroup that sums the workgroups' records.  Two launches, no synchronisation; every refusal
// comes before the first allocation or launch.
static int noiseMeter(PtxRenderer *r, const PtxNoiseDesc *d)
{
    const char *who = "ptx_noise_meter";
    if (!r || !d)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "%s: null argument", who);
    const uint32_t maxSamples = 1u << 24;
    if (!d->samplesA || d->samplesA > maxSamples || !d->samplesB || d->samplesB > maxSamples || d->tileShift < 3u || d->tileShift > kNoiseBlockShift ||
        (d->flags & ~(uint32_t)PTX_NOISE_WRITE_SUM) || d->reserved[0] || d->reserved[1])
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "%s: need samplesA and samplesB in 1 .. 2^24 (%u, %u), tileShift in 3 .. 6 (%u), no unknown flag (0x%x) and "
                    "reserved 0 (%u, %u)", who, d->samplesA, d->samplesB, d->tileShift, d->flags, d->reserved[0], d->reserved[1]);
    if (!finiteFloat(d->exposure) || !finiteFloat(d->threshold) || !(d->exposure > 0.0f) || d->threshold < 0.0f)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "%s: need a finite exposure > 0 (%g) and a finite threshold >= 0 (%g)", who, (double)d->exposure,
                    (double)d->threshold);
    if (const int rc = outputRefusal(r, who, NEEDS_FRAME | NEEDS_ONE_SHARD))
        return rc;
    OutputState::NoiseState &s = r->output.noise;
    if (!s.half[0].p || !s.half[1].p)
        return fail(r, PTX_ERROR_NOT_READY, "%s: no halves (call ptx_noise_halves)", who);
    HIP_TRY(r, hipSetDevice(r->device));
    const uint32_t W = r->frame.width, H = r->frame.height, sh = d->tileShift;
    const uint32_t tilesX = (W + (1u << sh) - 1u) >> sh, tilesY = (H + (1u << sh) - 1u) >> sh;
    const dim3 grid((W + kNoiseBlockSide - 1u) / kNoiseBlockSide, (H + kNoiseBlockSide - 1u) / kNoiseBlockSide);
    const size_t tiles = (size_t)tilesX * tilesY, groups = (size_t)grid.x * grid.y;
    HIP_TRY(r, s.result.alloc(1));
    HIP_TRY(r, s.tiles.alloc(tiles));
    HIP_TRY(r, s.tileErrors.alloc(tiles));
    HIP_TRY(r, s.records.alloc(groups * kNoiseRecordWords));
    NoiseArgs a;
    a.halfA = s.half[0].p;
    a.halfB = s.half[1].p;
    a.sum = r->frame.image.p; // the internal image, whatever is bound
    a.tiles = s.tiles.p;
    a.tileErrors = s.tileErrors.p;
    a.records = s.records.p;
    a.width = W; a.height = H; a.tileShift = sh; a.tilesX = tilesX; a.tilesY = tilesY;
    // step 2: rcp_ is the correctly rounded reciprocal on these arguments (1 .. 2^25), and so is the host's 1 / x
    a.sa = d->exposure * (1.0f / (float)d->samplesA);
    a.sb = d->exposure * (1.0f / (float)d->samplesB);
    a.st = d->exposure * (1.0f / (float)(d->samplesA + d->samplesB));
    a.threshold = d->threshold;
    if (d->flags & PTX_NOISE_WRITE_SUM)
        k_noise_tiles<true><<<grid, kNoiseBlock, 0, r->stream>>>(a);
    else
        k_noise_tiles<false><<<grid, kNoiseBlock, 0, r->stream>>>(a);
    NoiseResolveArgs v;
    v.records = s.records.p;
    v.recordCount = (uint32_t)groups;
    v.result = s.result.p;
    v.tilesX = tilesX;
    v.tilesY = tilesY;
    v.calls = s.calls + 1u;
    k_noise_resolve<<<1, kNoiseResolveBlock, 0, r->stream>>>(v);
    HIP_TRY(r, hipGetLastError());
    s.calls += 1u;
    s.tilesX = tilesX;
    s.tilesY = tilesY;
    s.tileShift = sh;
    return PTX_OK;
}

static int readNoise(PtxRenderer *r, PtxNoiseResult *out, float *tileErrors, size_t bytes)
{
    const char *who = "ptx_read_noise";
    if (!r || !out)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "%s: null argument", who);
    const OutputState::NoiseState &s = r->output.noise;
    if (!s.calls)
        return fail(r, PTX_ERROR_NOT_READY, "%s: call ptx_noise_meter first", who);
    const size_t want = (size_t)s.tilesX * s.tilesY * sizeof(float);
    if (tileErrors && bytes != want)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "%s: the tile map of %u x %u tiles is %zu bytes", who, s.tilesX, s.tilesY, want);
    HIP_TRY(r, hipSetDevice(r->device));
    if (tileErrors)
        HIP_TRY(r, hipMemcpyAsync(tileErrors, s.tileErrors.p, want, hipMemcpyDeviceToHost, r->stream));
    return readBack(r, out, s.result.p, sizeof(PtxNoiseResult));
}

// ---- adaptive sampling (docs/NEXT_ROWS.md section 27; semantics: include/ptx.h ptx_adaptive_plan; kernels: pt_adaptive.hpp) ----------

// ptx_adaptive_plan: one launch of one workgroup and the read-back of its result.  Every refusal comes before the first allocation,
// copy or launch.
static int adaptivePlan(PtxRenderer *r, const PtxAdaptiveDesc *d, PtxAdaptivePlan *out)
{
    const char *who = "ptx_adaptive_plan";
    if (!r || !d || !out)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "%s: null argument", who);
    const uint32_t maxFrames = 1u << 24;
    if (d->tileShift < 3u || d->tileShift > kNoiseBlockShift || d->source > PTX_ADAPTIVE_FROM_MASK || d->flags || d->reserved[0] || d->reserved[1] || d->dilate > 2u ||
        d->framesA > maxFrames || d->framesB > maxFrames)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "%s: need tileShift in 3 .. 6 (%u), a source of 0 or 1 (%u), no flag (0x%x), reserved 0 (%u, %u), dilate in 0 .. 2 (%u) "
                    "and frame counts of at most 2^24 (%u, %u)", who, d->tileShift, d->source, d->flags, d->reserved[0], d->reserved[1], d->dilate, d->framesA, d->framesB);
    if (d->source == PTX_ADAPTIVE_FROM_MASK && !d->mask)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "%s: PTX_ADAPTIVE_FROM_MASK needs a mask", who);
    if (const int rc = outputRefusal(r, who, NEEDS_FRAME | NEEDS_ONE_SHARD))
        return rc;
    const OutputState::NoiseState &ns = r->output.noise;
    if (d->source == PTX_ADAPTIVE_FROM_NOISE && (!ns.calls || ns.tileShift != d->tileShift))
        return fail(r, PTX_ERROR_NOT_READY, "%s: PTX_ADAPTIVE_FROM_NOISE needs an accepted meter call of tileShift %u (the last one: %u)", who, d->tileShift, ns.tileShift);
    OutputState::AdaptiveState &s = r->output.adaptive;
    if (s.tileShift && s.tileShift != d->tileShift && (s.counted || (s.planned && (d->framesA | d->framesB))))
        return fail(r, PTX_ERROR_NOT_READY, "%s: the counts are of tileShift %u, not %u, and are not all zero", who, s.tileShift, d->tileShift);
    HIP_TRY(r, hipSetDevice(r->device));
    const uint32_t W = r->frame.width, H = r->frame.height, sh = d->tileShift;
    const uint32_t tilesX = (W + (1u << sh) - 1u) >> sh, tilesY = (H + (1u << sh) - 1u) >> sh;
    const size_t tiles = (size_t)tilesX * tilesY;
    if (s.tileShift != sh) // the first accepted call, or all counts zero and nothing to commit: the counts are made (anew) and zeroed
    {
        // no counts and no plan until all of it stands: an allocation that fails below leaves the handle without either
        s.tileShift = s.generation = 0u;
        s.planned = s.counted = false;
        s.plan = {};
        HIP_TRY(r, s.counts.alloc(2u * tiles));
        HIP_TRY(r, s.list.alloc(tiles));
        HIP_TRY(r, s.active.alloc(tiles));
        HIP_TRY(r, s.seed.alloc(tiles));
        HIP_TRY(r, s.result.alloc(1));
        HIP_TRY(r, hipMemsetAsync(s.counts.p, 0, 2u * tiles * sizeof(uint32_t), r->stream));
        s.tileShift = sh;
        s.plan.tilesX = tilesX;
        s.plan.tilesY = tilesY;
    }
    if (d->source == PTX_ADAPTIVE_FROM_MASK)
    {
        HIP_TRY(r, s.mask.alloc(tiles));
        HIP_TRY(r, hipMemcpyAsync(s.mask.p, d->mask, tiles, hipMemcpyHostToDevice, r->stream));
    }
    AdaptiveArgs a;
    a.countA = s.counts.p;
    a.countB = s.counts.p + tiles;
    a.active = s.active.p;
    a.seed = s.seed.p;
    a.records = d->source == PTX_ADAPTIVE_FROM_NOISE ? ns.tiles.p : nullptr;
    a.mask = d->source == PTX_ADAPTIVE_FROM_MASK ? s.mask.p : nullptr;
    a.list = s.list.p;
    a.plan = s.result.p;
    a.width = W; a.height = H; a.tileShift = sh; a.tilesX = tilesX; a.tilesY = tilesY;
    a.hadPlan = s.planned ? 1u : 0u;
    a.framesA = d->framesA; a.framesB = d->framesB; a.dilate = d->dilate;
    a.generation = s.generation + 1u;
    k_adaptive_plan<<<1, kAdaptiveBlock, 0, r->stream>>>(a);
    HIP_TRY(r, hipGetLastError());
    if ((d->framesA | d->framesB) && (!s.planned || s.plan.activeTiles))
        s.counted = true;
    s.generation += 1u;
    s.planned = true;
    r->launch.hint.forget(); // learnt on another set of tiles
    if (const int rc = readBack(r, &s.plan, s.result.p, sizeof(PtxAdaptivePlan)))
    {
        s.planned = false; // the list's length is unknown: renders cover the frame
        return rc;
    }
    *out = s.plan;
    return PTX_OK;
}

static int adaptiveClear(PtxRenderer *r)
{
    if (!r)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "ptx_adaptive_clear: null handle");
    OutputState::AdaptiveState &s = r->output.adaptive;
    if (s.planned)
        r->launch.hint.forget();
    s.planned = false;
    s.plan.activeTiles = s.plan.activePixels = s.plan.seedTiles = 0u;
    return PTX_OK;
}

static int readAdaptive(PtxRenderer *r, PtxAdaptivePlan *out, uint32_t *tiles, size_t tileBytes, uint32_t *counts, size_t countBytes)
{
    const char *who = "ptx_read_adaptive";
    if (!r || !out)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "%s: null argument", who);
    const OutputState::AdaptiveState &s = r->output.adaptive;
    if (!s.tileShift)
        return fail(r, PTX_ERROR_NOT_READY, "%s: call ptx_adaptive_plan first", who);
    const size_t wantTiles = (size_t)s.plan.activeTiles * sizeof(uint32_t), wantCounts = 2u * (size_t)s.numTiles() * sizeof(uint32_t);
    if ((tiles && tileBytes != wantTiles) || (counts && countBytes != wantCounts))
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "%s: the list of %u tiles is %zu bytes and the counts of %u x %u tiles are %zu", who, s.plan.activeTiles, wantTiles,
                    s.plan.tilesX, s.plan.tilesY, wantCounts);
    HIP_TRY(r, hipSetDevice(r->device));
    if (tiles && wantTiles)
        HIP_TRY(r, hipMemcpyAsync(tiles, s.list.p, wantTiles, hipMemcpyDeviceToHost, r->stream));
    if (counts)
        HIP_TRY(r, hipMemcpyAsync(counts, s.counts.p, wantCounts, hipMemcpyDeviceToHost, r->stream));
    HIP_TRY(r, hipStreamSynchronize(r->stream));
    HIP_TRY(r, hipGetLastError());
    *out = s.plan;
    return PTX_OK;
}

// ptx_noise_meter_adaptive: noiseMeter with the scale factors per tile (k_noise_tiles_adaptive) and the same second launch
static int noiseMeterAdaptive(PtxRenderer *r, const PtxAdaptiveMeterDesc *d)
{
    const char *who = "ptx_noise_meter_adaptive";
    if (!r || !d)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "%s: null argument", who);
    const uint32_t maxFrames = 1u << 24;
    if (d->pendingA > maxFrames || d->pendingB > maxFrames || !d->normalizeTo || d->normalizeTo > (1u << 25) || d->tileShift < 3u || d->tileShift > kNoiseBlockShift ||
        (d->flags & ~(uint32_t)PTX_NOISE_WRITE_SUM) || d->reserved[0] || d->reserved[1])
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "%s: need pendingA and pendingB of at most 2^24 (%u, %u), normalizeTo in 1 .. 2^25 (%u), tileShift in 3 .. 6 (%u), no "
                    "unknown flag (0x%x) and reserved 0 (%u, %u)", who, d->pendingA, d->pendingB, d->normalizeTo, d->tileShift, d->flags, d->reserved[0], d->reserved[1]);
    if (!finiteFloat(d->exposure) || !finiteFloat(d->threshold) || !(d->exposure > 0.0f) || d->threshold < 0.0f)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "%s: need a finite exposure > 0 (%g) and a finite threshold >= 0 (%g)", who, (double)d->exposure,
                    (double)d->threshold);
    if (const int rc = outputRefusal(r, who, NEEDS_FRAME | NEEDS_ONE_SHARD))
        return rc;
    OutputState::NoiseState &s = r->output.noise;
    if (!s.half[0].p || !s.half[1].p)
        return fail(r, PTX_ERROR_NOT_READY, "%s: no halves (call ptx_noise_halves)", who);
    const OutputState::AdaptiveState &ad = r->output.adaptive;
    if (!ad.tileShift)
        return fail(r, PTX_ERROR_NOT_READY, "%s: no counts (call ptx_adaptive_plan first)", who);
    if (ad.tileShift != d->tileShift)
        return fail(r, PTX_ERROR_NOT_READY, "%s: the counts are of tileShift %u, not %u", who, ad.tileShift, d->tileShift);
    HIP_TRY(r, hipSetDevice(r->device));
    const uint32_t W = r->frame.width, H = r->frame.height, sh = d->tileShift;
    const uint32_t tilesX = ad.plan.tilesX, tilesY = ad.plan.tilesY;
    const dim3 grid((W + kNoiseBlockSide - 1u) / kNoiseBlockSide, (H + kNoiseBlockSide - 1u) / kNoiseBlockSide);
    const size_t tiles = (size_t)tilesX * tilesY, groups = (size_t)grid.x * grid.y;
    HIP_TRY(r, s.result.alloc(1));
    HIP_TRY(r, s.tiles.alloc(tiles));
    HIP_TRY(r, s.tileErrors.alloc(tiles));
    HIP_TRY(r, s.records.alloc(groups * kNoiseRecordWords));
    AdaptiveNoiseArgs a;
    a.noise.halfA = s.half[0].p;
    a.noise.halfB = s.half[1].p;
    a.noise.sum = r->frame.image.p;
    a.noise.tiles = s.tiles.p;
    a.noise.tileErrors = s.tileErrors.p;
    a.noise.records = s.records.p;
    a.noise.width = W; a.noise.height = H; a.noise.tileShift = sh; a.noise.tilesX = tilesX; a.noise.tilesY = tilesY;
    a.noise.sa = a.noise.sb = a.noise.st = 0.0f;
    a.noise.threshold = d->threshold;
    a.countA = ad.counts.p;
    a.countB = ad.counts.p + tiles;
    a.active = ad.planned ? ad.active.p : nullptr;
    a.pendingA = d->pendingA; a.pendingB = d->pendingB; a.normalizeTo = d->normalizeTo;
    a.exposure = d->exposure;
    if (d->flags & PTX_NOISE_WRITE_SUM)
        k_noise_tiles_adaptive<true><<<grid, kNoiseBlock, 0, r->stream>>>(a);
    else
        k_noise_tiles_adaptive<false><<<grid, kNoiseBlock, 0, r->stream>>>(a);
    NoiseResolveArgs v;
    v.records = s.records.p;
    v.recordCount = (uint32_t)groups;
    v.result = s.result.p;
    v.tilesX = tilesX;
    v.tilesY = tilesY;
    v.calls = s.calls + 1u;
    k_noise_resolve<<<1, kNoiseResolveBlock, 0, r->stream>>>(v);
    HIP_TRY(r, hipGetLastError());
    s.calls += 1u;
    s.tilesX = tilesX;
    s.tilesY = tilesY;
    s.tileShift = sh;
    return PTX_OK;
}

// What ptx_resize does to the output stage: the output is not ready, G and the grid of ptx_local_exposure go with the extent they were
// made for, as do the halves of ptx_noise_halves and the count of ptx_noise_meter calls, and the meter starts over, its exposure having
// been metered on an image of the old extent.  The present image, the LUT and the kept grade desc stay: they belong to the window and
// the display.
static int outputResized(PtxRenderer *r)
{
    OutputState &o = r->output;
    o.invalidate();
    o.localGain.release();
    o.localGrid.release();
    o.localReady = false;
    dropNoiseHalves(r);
    dropAdaptive(r);
    o.noise.calls = 0u;
    o.noise.tilesX = o.noise.tilesY = o.noise.tileShift = 0u;
    return meterReset(r);
}
