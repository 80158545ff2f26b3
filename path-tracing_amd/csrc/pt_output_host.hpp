// pt_output_host.hpp -- the output stage (ptx_postprocess, ptx_read_output: row N4) and the screen path (ptx_present, ptx_read_present:
// row D15; docs/NEXT_ROWS.md section 12).  Kernels: pt_post.hpp, pt_present.hpp; state: OutputState, the member `output` of the handle.
// Included by pt_runtime.hpp ahead of pt_chain_host.hpp, whose ptx_postprocess_denoised runs postprocessImage on the denoised image.
#pragma once

// Renderer::RecordPostProcessCommands + RecordSaveOutputCommands (Renderer.cpp:928-1085, :1204-1246)
// the chain on `source` (width x height running sums of uniform->TotalSamples samples): the accumulation image, or the denoised mean
static int postprocessImage(PtxRenderer *r, const float4 *source, const PtxPostProcessingUniformData *uniform, uint32_t toneMappingMode)
{
    HIP_TRY(r, hipSetDevice(r->device));
    const uint32_t W = r->frame.width, H = r->frame.height, n = W * H;
    uint32_t levels = 1;
    for (uint32_t m = W > H ? W : H; m > 1; m >>= 1)
        levels++;
    // mips 0 .. maxMipLevel-1 take part, maxMipLevel = min(levels - 3, MaxBloomMipmapLevel) (Renderer.cpp:955-956)
    uint32_t used = levels >= 5 ? (levels - 3 < 12 ? levels - 3 : 12) : 1;
    BloomLevel L[13];
    size_t total = 0;
    for (uint32_t l = 0; l < used; l++)
    {
        L[l].w = (W >> l) ? (W >> l) : 1;
        L[l].h = (H >> l) ? (H >> l) : 1;
        total += (size_t)L[l].w * L[l].h * 3;
    }
    HIP_TRY(r, r->output.postRgb.alloc((size_t)n * 3));
    HIP_TRY(r, r->output.bloomRgb.alloc(total));
    HIP_TRY(r, r->output.outLinear.alloc(n));
    size_t off = 0;
    for (uint32_t l = 0; l < used; l++)
    {
        L[l].rgb = r->output.bloomRgb.p + off;
        off += (size_t)L[l].w * L[l].h * 3;
    }
    k_postprocess<<<gridFor(n), kBlock, 0, r->stream>>>(source, n, *uniform, r->output.postRgb.p, L[0].rgb);
    for (uint32_t i = 0; i + 1 < used; i++)
        k_bloom_downsample<<<gridFor((size_t)L[i + 1].w * L[i + 1].h), kBlock, 0, r->stream>>>(L[i], L[i + 1]);
    for (uint32_t i = used - 1; i > 0; i--)
        k_bloom_upsample<<<gridFor((size_t)L[i - 1].w * L[i - 1].h), kBlock, 0, r->stream>>>(L[i], L[i - 1]);
    k_compose_tonemap<<<gridFor(n), kBlock, 0, r->stream>>>(r->output.postRgb.p, L[0].rgb, n, *uniform, toneMappingMode, r->output.outLinear.p);
    HIP_TRY(r, hipGetLastError());
    r->output.postUniform = *uniform;
    r->output.ready = true;
    return PTX_OK;
}

static int postprocess(PtxRenderer *r, const PtxPostProcessingUniformData *uniform, uint32_t toneMappingMode)
{
    if (!r || !uniform || toneMappingMode > PTX_TONE_MAPPING_HDR)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "ptx_postprocess: bad argument");
    if (!imagePtr(r))
        return fail(r, PTX_ERROR_NOT_READY, "ptx_postprocess: no accumulation image (call ptx_resize)");
    if (r->frame.boundShard)
        return frameIsElsewhere(r, "ptx_postprocess");
    return postprocessImage(r, imagePtr(r), uniform, toneMappingMode);
}

// OutputSaver: blit of the tone-mapped image into its output image + readback (OutputSaver.cpp:64-86, :120-199)
static int readOutput(PtxRenderer *r, uint32_t outputFormat, void *host, size_t bytes)
{
    if (!r || !host || outputFormat > PTX_OUTPUT_RGBA32F)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "ptx_read_output: bad argument");
    if (!r->output.ready)
        return fail(r, PTX_ERROR_NOT_READY, "ptx_read_output: call ptx_postprocess first");
    const uint32_t n = r->frame.width * r->frame.height;
    const size_t want = (size_t)n * (outputFormat == PTX_OUTPUT_RGBA32F ? 16 : 4);
    if (bytes != want)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "ptx_read_output: buffer must be %zu bytes", want);
    HIP_TRY(r, hipSetDevice(r->device));
    if (outputFormat == PTX_OUTPUT_RGBA32F)
        HIP_TRY(r, hipMemcpyAsync(host, r->output.outLinear.p, bytes, hipMemcpyDeviceToHost, r->stream));
    else
    {
        HIP_TRY(r, r->output.outSrgb8.alloc(n));
        k_encode_srgb8<<<gridFor(n), kBlock, 0, r->stream>>>(r->output.outLinear.p, n, r->output.outSrgb8.p);
        HIP_TRY(r, hipMemcpyAsync(host, r->output.outSrgb8.p, bytes, hipMemcpyDeviceToHost, r->stream));
    }
    HIP_TRY(r, hipStreamSynchronize(r->stream));
    HIP_TRY(r, hipGetLastError());
    return PTX_OK;
}

// The screen path: RecordPostProcessCommands' final blit + RecordUICommands (Renderer.cpp:1075-1203) in one launch of k_present
static int present(PtxRenderer *r, const PtxPresentDesc *d)
{
    if (!r || !d)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "ptx_present: null argument");
    if (!d->width || !d->height || d->width > 16384u || d->height > 16384u)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "ptx_present: bad screen extent %ux%u (1 .. 16384 each)", d->width, d->height);
    if (d->format > PTX_PRESENT_R16G16B16A16_SFLOAT || d->toneMappingMode > PTX_TONE_MAPPING_HDR || (d->flags & ~(uint32_t)PTX_PRESENT_UI_ON_DEVICE) || d->reserved)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "ptx_present: unknown format %u, mode %u or flags 0x%x, or reserved != 0", d->format, d->toneMappingMode, d->flags);
    const bool hdr = d->toneMappingMode == PTX_TONE_MAPPING_HDR;
    if ((hdr && d->format <= PTX_PRESENT_B8G8R8A8_SRGB) || (!hdr && d->format == PTX_PRESENT_A2B10G10R10_UNORM))
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "ptx_present: an 8-bit sRGB surface is SDR and A2B10G10R10 is HDR10 (Swapchain.cpp:317-340)");
    if (!r->output.ready)
        return fail(r, PTX_ERROR_NOT_READY, "ptx_present: call ptx_postprocess first");
    if (r->frame.boundShard)
        return frameIsElsewhere(r, "ptx_present");
    HIP_TRY(r, hipSetDevice(r->device));
    const uint32_t n = d->width * d->height;
    const size_t words = (size_t)n * (d->format == PTX_PRESENT_R16G16B16A16_SFLOAT ? 2 : 1);
    if (words > r->output.presentImage.n || !r->output.presentImage.p) // a failed allocation keeps the previous image
    {
        DevBuf<uint32_t> grown;
        HIP_TRY(r, grown.alloc(words));
        r->output.presentImage.swap(grown);
    }
    PresentArgs a;
    a.post = r->output.postRgb.p;
    a.bloom0 = r->output.bloomRgb.p; // level 0 of the chain
    a.ui = static_cast<const uint32_t *>(d->ui);
    a.out = r->output.presentImage.p;
    a.u = r->output.postUniform;
    a.W = r->frame.width; a.H = r->frame.height; a.SW = d->width; a.SH = d->height;
    if (d->ui && !(d->flags & PTX_PRESENT_UI_ON_DEVICE))
    {
        HIP_TRY(r, r->output.presentUi.alloc(n));
        HIP_TRY(r, hipMemcpyAsync(r->output.presentUi.p, d->ui, (size_t)n * 4, hipMemcpyHostToDevice, r->stream));
        a.ui = r->output.presentUi.p;
    }
    const uint32_t grid = (n + kPresentBlock - 1) / kPresentBlock;
    switch (d->format)
    {
    case PTX_PRESENT_R8G8B8A8_SRGB: k_present<PTX_PRESENT_R8G8B8A8_SRGB, false><<<grid, kPresentBlock, 0, r->stream>>>(a); break;
    case PTX_PRESENT_B8G8R8A8_SRGB: k_present<PTX_PRESENT_B8G8R8A8_SRGB, false><<<grid, kPresentBlock, 0, r->stream>>>(a); break;
    case PTX_PRESENT_A2B10G10R10_UNORM: k_present<PTX_PRESENT_A2B10G10R10_UNORM, true><<<grid, kPresentBlock, 0, r->stream>>>(a); break;
    default:
        if (hdr)
            k_present<PTX_PRESENT_R16G16B16A16_SFLOAT, true><<<grid, kPresentBlock, 0, r->stream>>>(a);
        else
            k_present<PTX_PRESENT_R16G16B16A16_SFLOAT, false><<<grid, kPresentBlock, 0, r->stream>>>(a);
    }
    HIP_TRY(r, hipGetLastError());
    r->output.presentWidth = d->width;
    r->output.presentHeight = d->height;
    r->output.presentFormat = d->format;
    r->output.presentBytes = words * 4;
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
    HIP_TRY(r, hipMemcpyAsync(host, r->output.presentImage.p, bytes, hipMemcpyDeviceToHost, r->stream));
    HIP_TRY(r, hipStreamSynchronize(r->stream));
    HIP_TRY(r, hipGetLastError());
    return PTX_OK;
}
