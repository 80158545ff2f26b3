// pt_test_host.hpp -- the entry points that exist for the tests: ptx_test_eval, ptx_test_texture, ptx_test_debug_eval (device
// functions on arrays of inputs) and ptx_trace_rays (the traversal kernels on the caller's rays).  Included by pt_runtime.hpp last;
// the state is TestState: the staging buffers and the two events of ptx_trace_rays' kernel span.
#pragma once

static int testDebugEval(PtxRenderer *r, uint32_t which, const float *in, float *out, uint32_t n)
{
    if (!r || which > 1u || !in || !out)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "ptx_test_debug_eval: bad argument");
    if (!n)
        return PTX_OK;
    HIP_TRY(r, hipSetDevice(r->device));
    const size_t ni = (size_t)n * (which == 0u ? 18u : 1u), no = (size_t)n * 3u;
    HIP_TRY(r, r->test.testIn.alloc(ni));
    HIP_TRY(r, r->test.testOut.alloc(no));
    HIP_TRY(r, hipMemcpyAsync(r->test.testIn.p, in, ni * 4, hipMemcpyHostToDevice, r->stream));
    k_test_debug_eval<<<(n + 63) / 64, 64, 0, r->stream>>>(which, r->test.testIn.p, r->test.testOut.p, n);
    HIP_TRY(r, hipMemcpyAsync(out, r->test.testOut.p, no * 4, hipMemcpyDeviceToHost, r->stream));
    HIP_TRY(r, hipStreamSynchronize(r->stream));
    HIP_TRY(r, hipGetLastError());
    return PTX_OK;
}

static int testEval(PtxRenderer *r, uint32_t fn, const float *in, float *out, uint32_t n)
{
    if (!r || fn >= PTX_FN_COUNT || !in || !out)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "ptx_test_eval: bad argument");
    if (!n)
        return PTX_OK;
    HIP_TRY(r, hipSetDevice(r->device));
    const size_t ni = (size_t)n * h_inStride[fn], no = (size_t)n * h_outStride[fn];
    HIP_TRY(r, r->test.testIn.alloc(ni));
    HIP_TRY(r, r->test.testOut.alloc(no));
    if (fn == PTX_FN_SAMPLE_LIGHT)
        HIP_TRY(r, r->test.testUbo.alloc(n));
    HIP_TRY(r, hipMemcpyAsync(r->test.testIn.p, in, ni * 4, hipMemcpyHostToDevice, r->stream));
    HIP_TRY(r, hipMemsetAsync(r->test.testOut.p, 0, no * 4, r->stream));
    k_test_eval<<<(n + 63) / 64, 64, 0, r->stream>>>(fn, r->test.testIn.p, r->test.testOut.p, n, r->test.testUbo.p);
    HIP_TRY(r, hipMemcpyAsync(out, r->test.testOut.p, no * 4, hipMemcpyDeviceToHost, r->stream));
    HIP_TRY(r, hipStreamSynchronize(r->stream));
    HIP_TRY(r, hipGetLastError());
    return PTX_OK;
}

static int testTexture(PtxRenderer *r, const float *in, float *out, uint32_t n, int implicitLod)
{
    if (!r || !in || !out)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "ptx_test_texture: null argument");
    if (!r->link.ready)
        return fail(r, PTX_ERROR_NOT_READY, "ptx_test_texture: no scene uploaded");
    if (!n)
        return PTX_OK;
    HIP_TRY(r, hipSetDevice(r->device));
    HIP_TRY(r, r->test.testIn.alloc((size_t)n * 7));
    HIP_TRY(r, r->test.testOut.alloc((size_t)n * 4));
    HIP_TRY(r, hipMemcpyAsync(r->test.testIn.p, in, (size_t)n * 28, hipMemcpyHostToDevice, r->stream));
    TextureView tv;
    tv.textures = r->scene.renderTextures.p; tv.textureCount = r->scene.textureCount; tv.texels8 = nullptr; tv.texelsF = r->scene.renderTexels.p;
    tv.srgbLut = nullptr;
    k_test_texture<<<(n + 63) / 64, 64, 0, r->stream>>>(tv, r->test.testIn.p, r->test.testOut.p, n, implicitLod);
    HIP_TRY(r, hipMemcpyAsync(out, r->test.testOut.p, (size_t)n * 16, hipMemcpyDeviceToHost, r->stream));
    HIP_TRY(r, hipStreamSynchronize(r->stream));
    HIP_TRY(r, hipGetLastError());
    return PTX_OK;
}

static int traceRays(PtxRenderer *r, const float *rays, uint32_t n, int anyHit, float *hits, uint32_t *ids)
{
    if (!r || !rays || !hits || !ids)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "ptx_trace_rays: null argument");
    if (!sceneUsable(r))
        return fail(r, PTX_ERROR_NOT_READY, "ptx_trace_rays: no acceleration structure (of a shared scene: the owner's is being replaced)");
    if (!n)
        return PTX_OK;
    HIP_TRY(r, hipSetDevice(r->device));
    DevBuf<float4> dRays, dHits;
    DevBuf<uint2> dIds;
    DevBuf<uint32_t> dOverflow; // the call's own count: a render whose counters are still to be collected keeps its C_OVERFLOW
    HIP_TRY(r, dRays.alloc((size_t)n * 2));
    HIP_TRY(r, dHits.alloc(n));
    HIP_TRY(r, dIds.alloc(n));
    HIP_TRY(r, dOverflow.alloc(1));
    if (const int rcCommit = waitForCommits(r))
        return rcCommit;
    const TraceScene sc = makeTraceScene(r);
    const hipEvent_t evT0 = r->test.evT0.get(), evT1 = r->test.evT1.get();
    hipError_t e = hipMemcpyAsync(dRays.p, rays, (size_t)n * 32, hipMemcpyHostToDevice, r->stream);
    if (e == hipSuccess)
    {
        (void)hipEventRecord(evT0, r->stream);
        (void)hipMemsetAsync(&r->launch.counters.p[C_CHUNK], 0, sizeof(uint32_t), r->stream);
        (void)hipMemsetAsync(dOverflow.p, 0, sizeof(uint32_t), r->stream);
        withFlag(sceneOf(r)->scene.anyNonOpaque, [&](auto ALPHA) {
            k_trace_rays<decltype(ALPHA)::value><<<gridFor(n), kBlock, 0, r->stream>>>(sc, dRays.p, n, anyHit, dHits.p, dIds.p, &r->launch.counters.p[C_CHUNK], r->launch.spill.p, dOverflow.p);
        });
        (void)hipEventRecord(evT1, r->stream);
        e = hipMemcpyAsync(hits, dHits.p, (size_t)n * 16, hipMemcpyDeviceToHost, r->stream);
    }
    if (e == hipSuccess)
        e = hipMemcpyAsync(ids, dIds.p, (size_t)n * 8, hipMemcpyDeviceToHost, r->stream);
    uint32_t overflowed = 0;
    if (e == hipSuccess)
        e = hipMemcpyAsync(&overflowed, dOverflow.p, sizeof(uint32_t), hipMemcpyDeviceToHost, r->stream);
    if (e == hipSuccess)
        e = hipStreamSynchronize(r->stream);
    if (e == hipSuccess)
        e = hipGetLastError();
    float ms = 0.0f;
    (void)hipEventElapsedTime(&ms, evT0, evT1);
    r->stats.lastTraceMs = ms;
    dRays.release(); dHits.release(); dIds.release(); dOverflow.release();
    if (e != hipSuccess)
        return fail(r, PTX_ERROR_DEVICE, "ptx_trace_rays: %s", hipGetErrorString(e));
    if (overflowed)
        return fail(r, PTX_ERROR_DEVICE, "ptx_trace_rays: traversal stack overflow (tree deeper than %d levels)", kLdsStack + kGlobalSpill);
    return PTX_OK;
}
