// ptx_capi.hip -- the C-ABI of include/ptx.h (the one translation unit of libptx_hip.so).  Every entry point cites the
// Renderer member it replaces in include/ptx.h; here each is ONE line (ptx_set_backend, ptx_synchronize and the trivial getters
// apart) that calls the implementation in pt_runtime.hpp (ptx_create, ptx_destroy) or one of the host files it includes
// (pt_scene_host.hpp, pt_bvh_host.hpp, pt_animation_host.hpp, pt_render_host.hpp, pt_frame_host.hpp, pt_output_host.hpp,
// pt_chain_host.hpp, pt_test_host.hpp);
// device side: pt_wavefront.hpp / pt_bvh.hpp / pt_bvh_build.hpp / pt_device.hpp.  No exceptions cross this boundary: status codes + ptx_last_error.
#include "pt_runtime.hpp"

extern "C" {

uint32_t ptx_abi_version(void)
{
    return PTX_ABI_VERSION;
}

int ptx_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess)
        return 0;
    return n;
}

int ptx_create(const PtxDeviceDesc *desc, PtxRenderer **out)
{
    return createRenderer(desc, out);
}

void ptx_destroy(PtxRenderer *r)
{
    destroyRenderer(r);
}

const char *ptx_last_error(const PtxRenderer *r)
{
    return r ? r->error.c_str() : "null renderer";
}

int ptx_set_backend(PtxRenderer *r, uint32_t backend)
{
    if (!r || backend > PTX_BACKEND_MEGAKERNEL)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "ptx_set_backend: bad backend %u", backend);
    if (r->backend != backend)
        r->launch.hint.forget(); // the learnt bounce schedule is the wavefront backend's
    r->backend = backend;
    return PTX_OK;
}

int ptx_share_scene(PtxRenderer *r, PtxRenderer *owner)
{
    return shareScene(r, owner);
}

int ptx_scene_upload(PtxRenderer *r, const PtxSceneDesc *s)
{
    return sceneUpload(r, s);
}

int ptx_scene_upload_streamed(PtxRenderer *r, const PtxSceneDesc *s, const uint32_t *standIn)
{
    return sceneUpload(r, s, true, standIn);
}

int ptx_texture_upload(PtxRenderer *r, uint32_t index, const PtxTextureDesc *desc)
{
    return textureUpload(r, index, desc);
}

int ptx_textures_commit(PtxRenderer *r, uint32_t *committed)
{
    return texturesCommit(r, committed);
}

int ptx_texture_residency(PtxRenderer *r, uint32_t *resident, uint32_t *pending)
{
    return textureResidency(r, resident, pending);
}

uint32_t ptx_textures_rejected(PtxRenderer *r, uint32_t *indices, uint32_t capacity)
{
    return texturesRejected(r, indices, capacity);
}

int ptx_build_accel(PtxRenderer *r)
{
    return buildBestTree(r);
}

int ptx_update_animation(PtxRenderer *r, const PtxTransform *instanceTransforms, uint32_t instanceCount, const PtxTransform *boneTransforms, uint32_t boneCount, uint32_t accelUpdate)
{
    return updateAnimation(r, instanceTransforms, instanceCount, boneTransforms, boneCount, accelUpdate);
}

int ptx_resize(PtxRenderer *r, uint32_t width, uint32_t height)
{
    return resizeFrame(r, width, height);
}

int ptx_set_tile_shard(PtxRenderer *r, const PtxTileShard *s)
{
    return setTileShard(r, s);
}

int ptx_reset_accumulation(PtxRenderer *r)
{
    return resetAccumulation(r);
}

int ptx_render(PtxRenderer *r, const PtxRaygenUniformData *uniform, const PtxLightsUbo *lights)
{
    return renderImpl(r, uniform, lights, uniform ? uniform->TotalSamples : 0, 1);
}

int ptx_render_frames(PtxRenderer *r, const PtxRaygenUniformData *uniform, const PtxLightsUbo *lights, uint32_t firstFrame, uint32_t frames)
{
    if (!uniform)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "ptx_render_frames: null uniform");
    PtxRaygenUniformData u = *uniform;
    u.SampleCount = 1; // canonical schedule: one sample per launch, RNG frame = launch index
    u.TotalSamples = firstFrame;
    return renderImpl(r, &u, lights, firstFrame, frames);
}

int ptx_render_debug(PtxRenderer *r, const PtxRaygenUniformData *uniform, const PtxLightsUbo *lights, const PtxDebugViewDesc *view)
{
    return renderDebug(r, uniform, lights, view);
}

int ptx_test_debug_eval(PtxRenderer *r, uint32_t which, const float *in, float *out, uint32_t n)
{
    return testDebugEval(r, which, in, out, n);
}

int ptx_synchronize(PtxRenderer *r)
{
    if (!r)
        return PTX_ERROR_INVALID_ARGUMENT;
    HIP_TRY(r, hipStreamSynchronize(r->stream));
    return collectRender(r); // errors of an asynchronous launch surface here
}

int ptx_readback(PtxRenderer *r, float *rgba, size_t bytes)
{
    return readback(r, rgba, bytes);
}

int ptx_readback_begin(PtxRenderer *r, float *pinnedHost, size_t bytes)
{
    return readbackBegin(r, pinnedHost, bytes);
}

int ptx_readback_end(PtxRenderer *r)
{
    return readbackEnd(r);
}

void *ptx_device_accum_ptr(PtxRenderer *r)
{
    return r ? imagePtr(r) : nullptr;
}

size_t ptx_accum_bytes(const PtxRenderer *r)
{
    return r ? r->frame.bytes() : 0;
}

size_t ptx_shard_bytes(const PtxRenderer *r, uint32_t rank)
{
    return shardBytes(r, rank);
}

int ptx_pack_shard(PtxRenderer *r, void *devDst)
{
    return packShard(r, devDst);
}

int ptx_unpack_shard(PtxRenderer *r, uint32_t rank, const void *devSrc)
{
    return unpackShard(r, rank, devSrc);
}

int ptx_unpack_shard_host(PtxRenderer *r, uint32_t rank, const void *devSrc, float *pinnedHost, size_t bytes)
{
    if (!pinnedHost)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "ptx_unpack_shard_host: null host buffer");
    return unpackShard(r, rank, devSrc, pinnedHost, bytes);
}

int ptx_unpack_shards(PtxRenderer *r, const void *devSrc, size_t strideBytes, int toDeviceImage, float *pinnedHost, size_t bytes)
{
    return unpackShards(r, devSrc, strideBytes, toDeviceImage, pinnedHost, bytes);
}

int ptx_bind_shard_accumulation(PtxRenderer *r, void *devShard, size_t bytes)
{
    return bindShardAccumulation(r, devShard, bytes);
}

int ptx_postprocess(PtxRenderer *r, const PtxPostProcessingUniformData *uniform, uint32_t toneMappingMode)
{
    return postprocessSource(r, "ptx_postprocess", uniform, toneMappingMode, PTX_METER_SUM);
}

int ptx_read_output(PtxRenderer *r, uint32_t outputFormat, void *host, size_t bytes)
{
    return readOutput(r, outputFormat, host, bytes);
}

int ptx_present(PtxRenderer *r, const PtxPresentDesc *desc)
{
    return presentFrame(r, desc, "ptx_present", false);
}

int ptx_read_present(PtxRenderer *r, void *host, size_t bytes)
{
    return readPresent(r, host, bytes);
}

void *ptx_device_present_ptr(PtxRenderer *r)
{
    return r && r->output.presentBytes ? r->output.presentImage.p : nullptr;
}

size_t ptx_present_bytes(const PtxRenderer *r)
{
    return r ? r->output.presentBytes : 0;
}

int ptx_render_guides(PtxRenderer *r, const PtxRaygenUniformData *uniform)
{
    return renderGuides(r, uniform);
}

int ptx_read_guide(PtxRenderer *r, uint32_t which, void *host, size_t bytes)
{
    return readGuide(r, which, host, bytes);
}

void *ptx_device_guide_ptr(PtxRenderer *r, uint32_t which)
{
    return r && r->chain.status.guidesReady && which < PTX_GUIDE_COUNT ? r->chain.guidePtr(which, r->frame.pixels()) : nullptr;
}

int ptx_denoise(PtxRenderer *r, const PtxDenoiseDesc *desc)
{
    return denoise(r, desc);
}

int ptx_read_denoised(PtxRenderer *r, void *host, size_t bytes)
{
    return readDenoised(r, host, bytes);
}

void *ptx_device_denoised_ptr(PtxRenderer *r)
{
    return r ? r->chain.denoised() : nullptr;
}

int ptx_postprocess_denoised(PtxRenderer *r, const PtxPostProcessingUniformData *uniform, uint32_t toneMappingMode)
{
    return postprocessSource(r, "ptx_postprocess_denoised", uniform, toneMappingMode, PTX_METER_DENOISED);
}

int ptx_temporal_accumulate(PtxRenderer *r, const PtxTemporalDesc *desc)
{
    return temporalAccumulate(r, desc);
}

int ptx_read_temporal(PtxRenderer *r, void *host, size_t bytes)
{
    return readTemporal(r, host, bytes);
}

void *ptx_device_temporal_ptr(PtxRenderer *r)
{
    return r && r->chain.status.temporalReady ? r->chain.temporalImage.p : nullptr;
}

int ptx_denoise_temporal(PtxRenderer *r, const PtxDenoiseDesc *desc)
{
    return denoiseTemporal(r, desc);
}

int ptx_temporal_accumulate_moments(PtxRenderer *r, const PtxTemporalDesc *desc)
{
    return temporalAccumulate(r, desc, true, "ptx_temporal_accumulate_moments");
}

int ptx_track_motion(PtxRenderer *r, int enable)
{
    return trackMotion(r, enable);
}

int ptx_render_guides_motion(PtxRenderer *r, const PtxRaygenUniformData *uniform)
{
    return renderGuides(r, uniform, true, "ptx_render_guides_motion");
}

int ptx_read_motion(PtxRenderer *r, uint32_t which, void *host, size_t bytes)
{
    return readMotion(r, which, host, bytes);
}

void *ptx_device_motion_ptr(PtxRenderer *r, uint32_t which)
{
    return r && r->chain.status.motionReady && which < PTX_MOTION_COUNT ? r->chain.motionPtr(which, r->frame.pixels()) : nullptr;
}

int ptx_render_guides_specular(PtxRenderer *r, const PtxRaygenUniformData *uniform, const PtxSpecularGuidesDesc *desc)
{
    return renderGuidesSpecular(r, uniform, desc);
}

int ptx_read_specular_guide(PtxRenderer *r, uint32_t which, void *host, size_t bytes)
{
    return readSpecularGuide(r, which, host, bytes);
}

void *ptx_device_specular_guide_ptr(PtxRenderer *r, uint32_t which)
{
    return r && r->chain.status.specularReady && which < PTX_SPECULAR_COUNT ? r->chain.specularPtr(which, r->frame.pixels()) : nullptr;
}

int ptx_temporal_accumulate_motion(PtxRenderer *r, const PtxTemporalDesc *desc, uint32_t withMoments)
{
    return temporalAccumulateMotion(r, desc, withMoments);
}

int ptx_temporal_accumulate_responsive(PtxRenderer *r, const PtxTemporalDesc *desc, const PtxResponsiveDesc *responsive)
{
    return temporalAccumulateResponsive(r, desc, responsive);
}

int ptx_read_fast_history(PtxRenderer *r, void *host, size_t bytes)
{
    return readFastHistory(r, host, bytes);
}

void *ptx_device_fast_history_ptr(PtxRenderer *r)
{
    return r && r->chain.status.fastCurrent() ? r->chain.fastHistory[r->chain.status.historyIn].p : nullptr;
}

int ptx_despike(PtxRenderer *r, const PtxDespikeDesc *desc)
{
    return despike(r, desc);
}

int ptx_read_despiked(PtxRenderer *r, void *host, size_t bytes)
{
    return readDespiked(r, host, bytes);
}

void *ptx_device_despiked_ptr(PtxRenderer *r)
{
    return r ? r->chain.despiked() : nullptr;
}

int ptx_chain_use_despiked(PtxRenderer *r, int enable)
{
    return chainUseDespiked(r, enable);
}

int ptx_postprocess_despiked(PtxRenderer *r, const PtxPostProcessingUniformData *uniform, uint32_t toneMappingMode)
{
    return postprocessSource(r, "ptx_postprocess_despiked", uniform, toneMappingMode, PTX_METER_DESPIKED);
}

int ptx_meter(PtxRenderer *r, const PtxMeterDesc *desc)
{
    return meter(r, desc);
}

int ptx_read_meter(PtxRenderer *r, PtxMeterResult *out, uint32_t *bins256)
{
    return readMeter(r, out, bins256);
}

void *ptx_device_meter_ptr(PtxRenderer *r)
{
    return r && r->output.meterState.p ? &r->output.meterState.p->result : nullptr;
}

int ptx_meter_reset(PtxRenderer *r)
{
    return meterReset(r);
}

int ptx_postprocess_metered(PtxRenderer *r, const PtxPostProcessingUniformData *u, uint32_t toneMappingMode, uint32_t source)
{
    return postprocessSource(r, "ptx_postprocess_metered", u, toneMappingMode, source, true);
}

int ptx_grade(PtxRenderer *r, const PtxGradeDesc *d, uint32_t toneMappingMode)
{
    return grade(r, d, toneMappingMode);
}

int ptx_grade_lut(PtxRenderer *r, uint32_t size, const float *rgb)
{
    return setGradeLut(r, size, rgb);
}

int ptx_present_graded(PtxRenderer *r, const PtxPresentDesc *desc)
{
    return presentFrame(r, desc, "ptx_present_graded", true);
}

int ptx_local_exposure(PtxRenderer *r, const PtxLocalExposureDesc *desc)
{
    return localExposure(r, desc);
}

int ptx_read_local_exposure(PtxRenderer *r, void *host, size_t bytes)
{
    return readLocalExposure(r, host, bytes);
}

void *ptx_device_local_exposure_ptr(PtxRenderer *r)
{
    return r && r->output.localReady ? r->output.localGain.p : nullptr;
}

int ptx_postprocess_local(PtxRenderer *r, const PtxPostProcessingUniformData *u, uint32_t toneMappingMode, uint32_t source, uint32_t metered)
{
    return postprocessLocal(r, u, toneMappingMode, source, metered);
}

int ptx_present_upscaled(PtxRenderer *r, const PtxPresentDesc *desc, const PtxUpscaleDesc *up)
{
    return presentFrame(r, desc, "ptx_present_upscaled", false, true, up);
}

int ptx_noise_halves(PtxRenderer *r, uint32_t enable)
{
    return noiseHalves(r, enable);
}

void *ptx_device_noise_half_ptr(PtxRenderer *r, uint32_t which)
{
    return r && which < 2u ? r->output.noise.half[which].p : nullptr;
}

int ptx_noise_meter(PtxRenderer *r, const PtxNoiseDesc *desc)
{
    return noiseMeter(r, desc);
}

int ptx_read_noise(PtxRenderer *r, PtxNoiseResult *out, float *tileErrors, size_t bytes)
{
    return readNoise(r, out, tileErrors, bytes);
}

int ptx_adaptive_plan(PtxRenderer *r, const PtxAdaptiveDesc *desc, PtxAdaptivePlan *out)
{
    return adaptivePlan(r, desc, out);
}

int ptx_read_adaptive(PtxRenderer *r, PtxAdaptivePlan *out, uint32_t *tiles, size_t tileBytes, uint32_t *counts, size_t countBytes)
{
    return readAdaptive(r, out, tiles, tileBytes, counts, countBytes);
}

int ptx_adaptive_clear(PtxRenderer *r)
{
    return adaptiveClear(r);
}

int ptx_noise_meter_adaptive(PtxRenderer *r, const PtxAdaptiveMeterDesc *desc)
{
    return noiseMeterAdaptive(r, desc);
}

int ptx_read_moments(PtxRenderer *r, void *host, size_t bytes)
{
    return readMoments(r, host, bytes);
}

int ptx_denoise_variance(PtxRenderer *r, const PtxDenoiseDesc *desc)
{
    return denoiseVariance(r, desc);
}

int ptx_read_variance(PtxRenderer *r, void *host, size_t bytes)
{
    return readVariance(r, host, bytes);
}

int ptx_write_accumulation(PtxRenderer *r, const float *rgba, size_t bytes)
{
    return writeAccumulation(r, rgba, bytes);
}

int ptx_get_stats(PtxRenderer *r, PtxStats *stats)
{
    return getStats(r, stats);
}

int ptx_test_input_stride(uint32_t fn)
{
    return fn < PTX_FN_COUNT ? h_inStride[fn] : -1;
}

int ptx_test_output_stride(uint32_t fn)
{
    return fn < PTX_FN_COUNT ? h_outStride[fn] : -1;
}

int ptx_test_eval(PtxRenderer *r, uint32_t fn, const float *in, float *out, uint32_t n)
{
    return testEval(r, fn, in, out, n);
}

int ptx_test_texture(PtxRenderer *r, const float *in, float *out, uint32_t n, int implicitLod)
{
    return testTexture(r, in, out, n, implicitLod);
}

int ptx_trace_rays(PtxRenderer *r, const float *rays, uint32_t n, int anyHit, float *hits, uint32_t *ids)
{
    return traceRays(r, rays, n, anyHit, hits, ids);
}

int ptx_bind_accumulation(PtxRenderer *r, void *devPtr, size_t bytes)
{
    return bindAccumulation(r, devPtr, bytes);
}

} // extern "C"
