#include "RendererHip.h"

#include "CubeLut.h"

namespace PathTracing
{

namespace
{
float PostProcessExposure(); // PostProcessSettings::Exposure, below
PtxRenderer *s_Renderer = nullptr;
std::shared_ptr<Scene> s_Scene; // SceneData::Handle (Renderer.h:187)
RendererHip::PathTracingSettings s_PathTracingSettings;
uint32_t s_SamplesPerFrame = 1;
uint32_t s_TotalSamples = 0;
uint32_t s_Width = 0, s_Height = 0;
bool s_DebugPipeline = false; // s_ActiveRaytracingPipeline == the debug pipeline (Renderer.cpp:579-610)
PtxDebugViewDesc s_DebugView = { PTX_DEBUG_MODE_COLOR, 0u, 0u, 0u };
bool s_AccumulationRestarted = true; // since the last temporal accumulation: the sum holds samples of a frame the history has not seen
bool s_MotionVectors = false; // denoiser, temporal accumulation and TemporalSettings.MotionVectors are all on (UpdateMotionVectors)
// noise metering (ptx.h "Noise metering"): the render calls alternate between the two halves
RendererHip::NoiseSettings s_NoiseSettings;
uint32_t s_NoiseSamples[2] = { 0, 0 }; // samples summed in half 0 / half 1
uint32_t s_NoiseCalls = 0;             // render calls since the accumulation restarted: its parity names the next half
PtxNoiseResult s_NoiseResult = {};     // of the last metered check, once read
bool s_NoisePending = false;           // a ptx_noise_meter has been enqueued since s_NoiseResult was read

// adaptive sampling (ptx.h "Adaptive sampling"): the checks plan the render calls that follow
RendererHip::AdaptiveSettings s_AdaptiveSettings;
uint32_t s_AdaptivePending[2] = { 0, 0 }; // samples rendered into half 0 / half 1 since the last ptx_adaptive_plan
bool s_AdaptiveCounts = false;            // the handle holds counts: a ptx_adaptive_plan has been accepted since Init or OnResize

bool NoiseIsOn()
{
    return s_NoiseSettings.Enabled && !s_DebugPipeline;
}

bool AdaptiveIsOn()
{
    return s_AdaptiveSettings.Enabled && s_NoiseSettings.Enabled;
}

int BindNoiseHalf(uint32_t which)
{
    return ptx_bind_accumulation(s_Renderer, ptx_device_noise_half_ptr(s_Renderer, which), ptx_accum_bytes(s_Renderer));
}

// the check of Render, and with PTX_NOISE_WRITE_SUM what SaveOutput, Present and ReadAccumulationImage do first
int MeterNoise(uint32_t flags)
{
    if (AdaptiveIsOn() && s_AdaptiveCounts) // every tile by its own counts; the sum scaled to the samples of all render calls
    {
        const PtxAdaptiveMeterDesc adaptive = { s_AdaptivePending[0], s_AdaptivePending[1], s_NoiseSamples[0] + s_NoiseSamples[1], PostProcessExposure(),
                                                s_NoiseSettings.Threshold, s_NoiseSettings.TileShift, flags, { 0u, 0u } };
        const int rc = ptx_noise_meter_adaptive(s_Renderer, &adaptive);
        if (rc == PTX_OK)
            s_NoisePending = true;
        return rc;
    }
    const PtxNoiseDesc desc = { s_NoiseSamples[0], s_NoiseSamples[1], PostProcessExposure(), s_NoiseSettings.Threshold, s_NoiseSettings.TileShift, flags, { 0u, 0u } };
    const int rc = ptx_noise_meter(s_Renderer, &desc);
    if (rc == PTX_OK)
        s_NoisePending = true;
    return rc;
}

// behind the check of Render: the samples since the last plan are committed and the tiles the check left open are planned
int PlanAdaptive()
{
    const PtxAdaptiveDesc desc = { s_NoiseSettings.TileShift, PTX_ADAPTIVE_FROM_NOISE, nullptr, s_AdaptiveSettings.Dilate, s_AdaptivePending[0], s_AdaptivePending[1], 0u,
                                   { 0u, 0u } };
    PtxAdaptivePlan plan;
    const int rc = ptx_adaptive_plan(s_Renderer, &desc, &plan);
    if (rc == PTX_OK)
    {
        s_AdaptivePending[0] = s_AdaptivePending[1] = 0;
        s_AdaptiveCounts = true;
    }
    return rc;
}
}

void RendererHip::Check(int status)
{
    if (status != PTX_OK)
        throw error(std::string("RendererHip: ") + (s_Renderer ? ptx_last_error(s_Renderer) : "no renderer"));
}

void RendererHip::Init(int deviceIndex, void *stream)
{
    PtxDeviceDesc desc = { deviceIndex, PTX_BACKEND_WAVEFRONT, stream, 0u, 0u };
    if (ptx_abi_version() != PTX_ABI_VERSION)
        throw error("RendererHip: libptx_hip.so was built against another ptx.h (ABI " + std::to_string(ptx_abi_version()) + ", expected " +
                    std::to_string(PTX_ABI_VERSION) + ")");
    if (ptx_create(&desc, &s_Renderer) != PTX_OK)
        throw error("RendererHip: ptx_create failed (no HIP device?)");
}

void RendererHip::Shutdown()
{
    ptx_destroy(s_Renderer);
    s_Renderer = nullptr;
    s_Scene.reset();
}

// Renderer.cpp:238-439
void RendererHip::UpdateSceneData(const std::shared_ptr<Scene> &scene, bool updated)
{
    if (s_Scene == scene)
    {
        if (updated)
            ResetAccumulationImage();
        return;
    }
    s_Scene = scene;
    const PtxSceneDesc desc = scene->GetDesc();
    Check(ptx_scene_upload(s_Renderer, &desc));
    Check(ptx_build_accel(s_Renderer));
    if (s_MotionVectors) // the upload turned tracking off
        Check(ptx_track_motion(s_Renderer, 1));
    ResetAccumulationImage();
}

void RendererHip::OnResize(uint32_t width, uint32_t height)
{
    s_Width = width;
    s_Height = height;
    Check(ptx_resize(s_Renderer, width, height));
    s_AdaptiveCounts = false; // ptx_resize drops them
    ResetAccumulationImage();
}

void RendererHip::SetSettings(const PathTracingSettings &settings)
{
    s_PathTracingSettings = settings;
    ResetAccumulationImage();
}

void RendererHip::SetSamplesPerFrame(uint32_t samples)
{
    s_SamplesPerFrame = samples ? samples : 1;
}

void RendererHip::SetTileShard(uint32_t rank, uint32_t worldSize, uint32_t tileSize)
{
    const PtxTileShard shard = { rank, worldSize, tileSize };
    Check(ptx_set_tile_shard(s_Renderer, &shard));
    if (s_AdaptiveCounts) // a change of the shard drops plan and counts: ask, and start over
    {
        PtxAdaptivePlan plan;
        s_AdaptiveCounts = ptx_read_adaptive(s_Renderer, &plan, nullptr, 0, nullptr, 0) == PTX_OK;
        ResetAccumulationImage();
    }
}

// Renderer.cpp:801-808
void RendererHip::ResetAccumulationImage()
{
    s_TotalSamples = 0;
    s_AccumulationRestarted = true;
    s_NoiseSamples[0] = s_NoiseSamples[1] = 0;
    s_NoiseCalls = 0;
    s_AdaptivePending[0] = s_AdaptivePending[1] = 0;
    if (s_Renderer && s_Width && s_NoiseSettings.Enabled) // makes the halves, or zeroes them again; the sum is formed from them when it is needed
    {
        Check(ptx_noise_halves(s_Renderer, 1u)); // (the counts of an adaptive render are zeroed with them)
        if (s_AdaptiveCounts)
            Check(ptx_adaptive_clear(s_Renderer));
        return;
    }
    if (s_Renderer && s_Width)
        Check(ptx_reset_accumulation(s_Renderer));
}

// the raygen uniform of the active camera (Renderer.cpp:1686-1696)
static PtxRaygenUniformData FillRaygenUniform()
{
    Camera &camera = s_Scene->GetActiveCamera();
    camera.OnResize(s_Width, s_Height);
    PtxRaygenUniformData rgenData;
    ToColumnMajor(camera.GetInvViewMatrix(), rgenData.ViewInverse);
    ToColumnMajor(camera.GetInvProjectionMatrix(), rgenData.ProjInverse);
    rgenData.BounceCount = s_PathTracingSettings.BounceCount;
    rgenData.LensRadius = s_PathTracingSettings.LensRadius;
    rgenData.FocalDistance = s_PathTracingSettings.FocalDistance;
    rgenData.SampleCount = s_SamplesPerFrame;
    rgenData.TotalSamples = s_TotalSamples;
    return rgenData;
}

// Renderer.cpp:1686-1726
void RendererHip::Render()
{
    const PtxRaygenUniformData rgenData = FillRaygenUniform();
    s_TotalSamples += s_SamplesPerFrame;
    const PtxLightsUbo lights = s_Scene->GetLightsUbo();
    if (s_DebugPipeline) // the debug raygen stores its one sample: nothing accumulates
    {
        s_TotalSamples = 0;
        if (s_NoiseSettings.Enabled) // ... and it stores it into the internal image
            Check(ptx_bind_accumulation(s_Renderer, nullptr, 0));
        Check(ptx_render_debug(s_Renderer, &rgenData, &lights, &s_DebugView));
        return;
    }
    if (!s_NoiseSettings.Enabled)
    {
        Check(ptx_render(s_Renderer, &rgenData, &lights));
        return;
    }
    // noise metering: this call's samples go to the half its parity names, and every CheckEvery calls the halves are compared
    const uint32_t which = s_NoiseCalls & 1u;
    Check(BindNoiseHalf(which));
    Check(ptx_render(s_Renderer, &rgenData, &lights));
    s_NoiseSamples[which] += s_SamplesPerFrame;
    s_NoiseCalls++;
    uint32_t every = s_NoiseSettings.CheckEvery ? s_NoiseSettings.CheckEvery : 1u;
    if (AdaptiveIsOn())
    {
        s_AdaptivePending[which] += s_SamplesPerFrame;
        every += every & 1u; // both halves receive the same samples under one plan
    }
    if (s_NoiseCalls % every == 0u && s_NoiseSamples[1] && s_NoiseSamples[0] + s_NoiseSamples[1] >= s_NoiseSettings.MinSamples)
    {
        Check(MeterNoise(0u));
        if (AdaptiveIsOn())
            Check(PlanAdaptive());
    }
}

// With the NoiseSettings on the running sum is A + B: ptx_noise_meter forms it in the internal image (PTX_NOISE_WRITE_SUM), which is then
// bound for the calls that read the sum.  Before the second render call there is no B to meter: half 0 is the sum and stays bound.
static int BindNoiseSum()
{
    if (!NoiseIsOn())
        return PTX_OK;
    if (!s_NoiseSamples[1])
        return BindNoiseHalf(0u);
    if (const int rc = MeterNoise(PTX_NOISE_WRITE_SUM))
        return rc;
    return ptx_bind_accumulation(s_Renderer, nullptr, 0);
}

// ... and afterwards the half of the next render call is bound again
static int RebindNoiseHalf()
{
    return NoiseIsOn() ? BindNoiseHalf(s_NoiseCalls & 1u) : (int)PTX_OK;
}

void RendererHip::SetSettings(const NoiseSettings &settings)
{
    const bool change = settings.Enabled != s_NoiseSettings.Enabled;
    // the counts of an adaptive render are per tile of the old size: the accumulation starts over with the new one
    const bool retile = !change && settings.Enabled && settings.TileShift != s_NoiseSettings.TileShift && s_AdaptiveCounts;
    s_NoiseSettings = settings;
    if (retile)
    {
        ResetAccumulationImage(); // zeroes the counts and clears the plan: the first plan of the new tile size makes them anew
        s_AdaptiveCounts = false; // ... and until then the checks are ptx_noise_meter's
    }
    if (!change)
        return;
    if (!settings.Enabled && s_Renderer) // the binding returns to the internal image
    {
        Check(ptx_noise_halves(s_Renderer, 0u));
        s_AdaptiveCounts = false; // they go with the halves
    }
    s_NoiseResult = {};
    s_NoisePending = false;
    ResetAccumulationImage(); // the samples so far are in the other kind of image
}

void RendererHip::SetSettings(const AdaptiveSettings &settings)
{
    const bool change = settings.Enabled != s_AdaptiveSettings.Enabled;
    s_AdaptiveSettings = settings;
    if (!change)
        return;
    if (s_Renderer && s_AdaptiveCounts) // render calls cover the frame again
        Check(ptx_adaptive_clear(s_Renderer));
    if (s_NoiseSettings.Enabled)
        ResetAccumulationImage(); // the tiles start over with equal counts
}

PtxNoiseResult RendererHip::GetNoise()
{
    if (s_NoisePending)
    {
        Check(ptx_read_noise(s_Renderer, &s_NoiseResult, nullptr, 0));
        s_NoisePending = false;
    }
    return s_NoiseResult;
}

bool RendererHip::IsConverged()
{
    if (!NoiseIsOn())
        return false;
    const PtxNoiseResult res = GetNoise();
    return res.valid && res.converged == res.tilesX * res.tilesY && s_NoiseSamples[0] + s_NoiseSamples[1] >= s_NoiseSettings.MinSamples;
}

// Renderer.cpp:579-610 / :769-772
void RendererHip::SetDebugRaytracingPipeline(uint32_t renderMode, uint32_t raygenFlags, uint32_t hitGroupFlags)
{
    s_DebugPipeline = true;
    s_DebugView = { renderMode, raygenFlags, hitGroupFlags, 0u };
}

void RendererHip::SetPathTracingPipeline()
{
    if (!s_DebugPipeline)
        return;
    s_DebugPipeline = false;
    ResetAccumulationImage(); // the image holds a debug frame, not a running sum
}

// Renderer.cpp:1697-1711: a debug frame is post-processed as one sample
uint32_t RendererHip::GetTotalSamples()
{
    return s_DebugPipeline ? 1u : s_TotalSamples;
}

static RendererHip::PostProcessSettings s_PostProcessSettings;

namespace
{
float PostProcessExposure()
{
    return s_PostProcessSettings.Exposure;
}
}

void RendererHip::SetPostProcessSettings(const PostProcessSettings &settings)
{
    s_PostProcessSettings = settings;
}

static RendererHip::DenoiserSettings s_DenoiserSettings;

static RendererHip::TemporalSettings s_TemporalSettings;

// Motion guides are used when all three are on; the scene's pose tracking follows (ptx_track_motion), and a host that never asks
// for them makes no call it did not make before.
static int UpdateMotionVectors()
{
    const bool want = s_DenoiserSettings.Enabled && s_TemporalSettings.Enabled && s_TemporalSettings.MotionVectors;
    const bool change = want != s_MotionVectors && s_Renderer && s_Scene;
    s_MotionVectors = want;
    return change ? ptx_track_motion(s_Renderer, want ? 1 : 0) : (int)PTX_OK;
}

void RendererHip::SetSettings(const DenoiserSettings &settings)
{
    s_DenoiserSettings = settings;
    Check(UpdateMotionVectors());
}

void RendererHip::SetSettings(const TemporalSettings &settings)
{
    s_TemporalSettings = settings;
    Check(UpdateMotionVectors());
}

static RendererHip::VarianceSettings s_VarianceSettings;

void RendererHip::SetSettings(const VarianceSettings &settings)
{
    s_VarianceSettings = settings;
}

static RendererHip::FireflySettings s_FireflySettings;

void RendererHip::SetSettings(const FireflySettings &settings)
{
    const bool wasOn = s_FireflySettings.Enabled;
    s_FireflySettings = settings;
    if (wasOn && !settings.Enabled && s_Renderer) // the chain reads the sum again
        Check(ptx_chain_use_despiked(s_Renderer, 0));
}

static RendererHip::ExposureSettings s_ExposureSettings;
static float s_TimeStep = 0.0f; // OnUpdate: the seconds since the last metered frame, used up by the ptx_meter that adapts over them

void RendererHip::SetSettings(const ExposureSettings &settings)
{
    s_ExposureSettings = settings;
}

void RendererHip::OnUpdate(float timeStep)
{
    s_TimeStep += timeStep;
}

static RendererHip::LocalExposureSettings s_LocalExposureSettings;

void RendererHip::SetSettings(const LocalExposureSettings &settings)
{
    s_LocalExposureSettings = settings;
}

// The output stage on the sum, on the despiked image or on the denoised one (PTX_METER_*).  With the ExposureSettings on (ptx.h,
// "Exposure metering") that image is metered first, with the frame's time step, and the metered call multiplies the exposure in;
// with the LocalExposureSettings on as well, ptx_local_exposure follows the meter and ptx_postprocess_local takes the metered call's place.
static int OutputStage(const PtxPostProcessingUniformData &u, uint32_t mode, uint32_t source)
{
    if (!s_ExposureSettings.Enabled || s_DebugPipeline)
        return source == PTX_METER_SUM        ? ptx_postprocess(s_Renderer, &u, mode)
               : source == PTX_METER_DESPIKED ? ptx_postprocess_despiked(s_Renderer, &u, mode)
                                              : ptx_postprocess_denoised(s_Renderer, &u, mode);
    const RendererHip::ExposureSettings &e = s_ExposureSettings;
    const PtxMeterDesc meter = { source, e.Mode, u.TotalSamples, { 0u, 0u, 0u, 0u }, e.LowPermille, e.HighPermille, e.KeyLog2, e.Compensation, e.MinLog2Exposure,
                                 e.MaxLog2Exposure, e.SpeedUp, e.SpeedDown, s_TimeStep, 0u, 0u };
    if (const int rc = ptx_meter(s_Renderer, &meter))
        return rc;
    s_TimeStep = 0.0f; // a second SaveOutput or Present of the same frame meters with deltaSeconds = 0, which leaves the exposure where it is
    if (s_LocalExposureSettings.Enabled) // behind the meter (ptx.h, "Local exposure"): the pivot is a display luminance, so the metered exposure comes off it
    {
        const RendererHip::LocalExposureSettings &l = s_LocalExposureSettings;
        const PtxLocalExposureDesc local = { source, u.TotalSamples, l.CellShift, l.PivotLog2, l.HighlightContrast, l.ShadowContrast, l.MaxStops,
                                             PTX_LOCAL_EXPOSURE_PIVOT_METERED, 0u };
        if (const int rc = ptx_local_exposure(s_Renderer, &local))
            return rc;
        return ptx_postprocess_local(s_Renderer, &u, mode, source, 1u);
    }
    return ptx_postprocess_metered(s_Renderer, &u, mode, source);
}

// The post-processing chain on the current frame: on the running sum, or -- with the denoiser enabled and the path-tracing pipeline
// bound -- guides, filter, and the chain on the denoised mean (ptx.h, "Denoiser"); with the temporal accumulation enabled as well
// the filter runs on its result (ptx.h, "Temporal accumulation"), and with the variance settings enabled on top the moments are
// accumulated beside it and the variance-guided filter takes the fixed-sigma one's place (ptx.h, "Variance-guided denoising").
static int PostProcessFrame(const PtxPostProcessingUniformData &u, uint32_t mode)
{
    // firefly suppression (ptx.h, "Firefly suppression") ahead of whatever follows: the despiked image stands where the sum did
    const bool despike = s_FireflySettings.Enabled && !s_DebugPipeline;
    if (despike)
    {
        const PtxDespikeDesc firefly = { s_FireflySettings.Radius, s_FireflySettings.Rank, s_FireflySettings.MinTaps, s_FireflySettings.Gain, 0u, 0u };
        if (const int rc = ptx_despike(s_Renderer, &firefly))
            return rc;
    }
    if (!s_DenoiserSettings.Enabled || s_DebugPipeline)
        return OutputStage(u, mode, despike ? PTX_METER_DESPIKED : PTX_METER_SUM);
    if (despike)
        if (const int rc = ptx_chain_use_despiked(s_Renderer, 1))
            return rc;
    const PtxRaygenUniformData rgenData = FillRaygenUniform();
    const bool motion = s_MotionVectors && s_TemporalSettings.Enabled;
    const PtxSpecularGuidesDesc specular = { s_DenoiserSettings.SpecularBounces, s_DenoiserSettings.SpecularRoughnessMax, 0u, 0u };
    if (const int rc = motion                                 ? ptx_render_guides_motion(s_Renderer, &rgenData)
                       : s_DenoiserSettings.SpecularBounces ? ptx_render_guides_specular(s_Renderer, &rgenData, &specular)
                                                            : ptx_render_guides(s_Renderer, &rgenData))
        return rc;
    const PtxDenoiseDesc desc = { u.TotalSamples, s_DenoiserSettings.Iterations, s_DenoiserSettings.SigmaColor, s_DenoiserSettings.SigmaNormal,
                                  s_DenoiserSettings.SigmaPosition, 0u, 0u };
    if (s_TemporalSettings.Enabled)
    {
        // a sum that continued from the previous frame already holds every sample of the history: start a new one from it
        PtxTemporalDesc temporal = { {}, {}, u.TotalSamples, s_TemporalSettings.MaxHistory, s_TemporalSettings.NormalThreshold,
                                     s_TemporalSettings.PositionThreshold, s_AccumulationRestarted ? 0u : (uint32_t)PTX_TEMPORAL_RESET, 0u };
        const Camera &camera = s_Scene->GetActiveCamera(); // FillRaygenUniform brought it to the extent
        ToColumnMajor(camera.GetViewMatrix(), temporal.View);
        ToColumnMajor(camera.GetProjectionMatrix(), temporal.Proj);
        const PtxResponsiveDesc responsive = { s_TemporalSettings.FastHistory, s_TemporalSettings.ClampSigma,
                                               (motion ? (uint32_t)PTX_RESPONSIVE_MOTION : 0u) | (s_VarianceSettings.Enabled ? (uint32_t)PTX_RESPONSIVE_MOMENTS : 0u), 0u };
        if (const int rc = s_TemporalSettings.Responsive ? ptx_temporal_accumulate_responsive(s_Renderer, &temporal, &responsive)
                           : motion                     ? ptx_temporal_accumulate_motion(s_Renderer, &temporal, s_VarianceSettings.Enabled ? 1u : 0u)
                           : s_VarianceSettings.Enabled ? ptx_temporal_accumulate_moments(s_Renderer, &temporal)
                                                        : ptx_temporal_accumulate(s_Renderer, &temporal))
            return rc;
        s_AccumulationRestarted = false;
        if (s_VarianceSettings.Enabled)
        {
            const PtxDenoiseDesc variance = { 1u, s_VarianceSettings.Iterations, s_VarianceSettings.SigmaLuminance, s_DenoiserSettings.SigmaNormal,
                                              s_DenoiserSettings.SigmaPosition, 0u, 0u };
            if (const int rc = ptx_denoise_variance(s_Renderer, &variance))
                return rc;
        }
        else if (const int rc = ptx_denoise_temporal(s_Renderer, &desc))
            return rc;
        return OutputStage(u, mode, PTX_METER_DENOISED);
    }
    if (const int rc = ptx_denoise(s_Renderer, &desc))
        return rc;
    return OutputStage(u, mode, PTX_METER_DENOISED);
}

static RendererHip::GradeSettings s_GradeSettings;
static PtxGradeDesc s_GradeDesc;

void RendererHip::SetSettings(const GradeSettings &settings)
{
    PtxGradeDesc d = {};
    WhiteBalanceMatrix(settings.TemperatureKelvin, d.colourMatrix);
    for (int k = 0; k < 3; k++)
    {
        d.slope[k] = settings.Slope[k];
        d.offset[k] = settings.Offset[k];
        d.power[k] = settings.Power[k];
    }
    d.saturation = settings.Saturation;
    d.curve = settings.Curve;
    d.whitePoint = settings.WhitePoint;
    if (settings.Enabled && !settings.LutFile.empty())
    {
        if (settings.LutFile != s_GradeSettings.LutFile || !s_GradeSettings.Enabled)
        {
            const CubeLut lut = ReadCubeLut(settings.LutFile);
            Check(ptx_grade_lut(s_Renderer, lut.Size, lut.Rgb.data()));
        }
        d.flags = (uint32_t)PTX_GRADE_USE_LUT | (settings.LutSrgbDomain ? (uint32_t)PTX_GRADE_LUT_SRGB_DOMAIN : 0u);
    }
    else if (s_GradeSettings.Enabled && !s_GradeSettings.LutFile.empty())
        Check(ptx_grade_lut(s_Renderer, 0u, nullptr));
    s_GradeSettings = settings;
    s_GradeDesc = d;
}

static bool GradeIsOn()
{
    return s_GradeSettings.Enabled && !s_DebugPipeline;
}

void RendererHip::SaveOutput(const OutputInfo &info)
{
    if (info.Extent.width != s_Width || info.Extent.height != s_Height)
        throw error("SaveOutput: the output extent must equal the render extent");
    const PtxPostProcessingUniformData u = { GetTotalSamples(), s_PostProcessSettings.Exposure, s_PostProcessSettings.BloomThreshold,
                                             s_PostProcessSettings.BloomIntensity };
    const uint32_t mode = s_PostProcessSettings.Hdr ? PTX_TONE_MAPPING_HDR : PTX_TONE_MAPPING_SDR;
    Check(BindNoiseSum());
    Check(PostProcessFrame(u, mode));
    if (GradeIsOn())
        Check(ptx_grade(s_Renderer, &s_GradeDesc, mode));
    Check(RebindNoiseHalf());
    const uint32_t format = OutputSaver::SelectImageFormat(info.Format);
    std::vector<std::byte> bytes(static_cast<size_t>(s_Width) * s_Height * (format == PTX_OUTPUT_RGBA32F ? 16 : 4));
    Check(ptx_read_output(s_Renderer, format, bytes.data(), bytes.size()));
    if (!OutputSaver::WriteImage(info, bytes))
        throw error("SaveOutput: cannot write " + info.Path.string());
}

static RendererHip::UpscaleSettings s_UpscaleSettings;

void RendererHip::SetSettings(const UpscaleSettings &settings)
{
    s_UpscaleSettings = settings;
}

static bool s_SurfaceIsHdr = false; // Swapchain::IsHdr()

void RendererHip::UpdateHdr(bool isHdr)
{
    s_SurfaceIsHdr = isHdr;
}

// Renderer.cpp:928-1203 after the path-tracing pass
void RendererHip::Present(uint32_t width, uint32_t height, const uint8_t *ui)
{
    const PtxPostProcessingUniformData u = { GetTotalSamples(), s_PostProcessSettings.Exposure, s_PostProcessSettings.BloomThreshold,
                                             s_PostProcessSettings.BloomIntensity };
    const uint32_t mode = s_SurfaceIsHdr ? PTX_TONE_MAPPING_HDR : PTX_TONE_MAPPING_SDR; // Renderer.cpp:737-742
    Check(BindNoiseSum());
    Check(PostProcessFrame(u, mode));
    if (GradeIsOn())
        Check(ptx_grade(s_Renderer, &s_GradeDesc, mode));
    Check(RebindNoiseHalf());
    const PtxPresentDesc desc = { width, height, s_SurfaceIsHdr ? (uint32_t)PTX_PRESENT_A2B10G10R10_UNORM : (uint32_t)PTX_PRESENT_R8G8B8A8_SRGB, mode, ui, 0u, 0u };
    if (s_UpscaleSettings.Enabled && width >= s_Width && height >= s_Height) // ptx.h, "Enlarging screen path": a smaller window stays with the blit
    {
        const PtxUpscaleDesc up = { PTX_UPSCALE_CATMULL_ROM, s_UpscaleSettings.Sharpness, GradeIsOn() ? (uint32_t)PTX_UPSCALE_GRADED : 0u, 0u };
        Check(ptx_present_upscaled(s_Renderer, &desc, &up));
        return;
    }
    Check(GradeIsOn() ? ptx_present_graded(s_Renderer, &desc) : ptx_present(s_Renderer, &desc));
}

std::vector<std::byte> RendererHip::ReadPresent()
{
    std::vector<std::byte> bytes(ptx_present_bytes(s_Renderer));
    Check(ptx_read_present(s_Renderer, bytes.data(), bytes.size()));
    return bytes;
}

std::vector<float> RendererHip::ReadAccumulationImage()
{
    std::vector<float> image(static_cast<size_t>(s_Width) * s_Height * 4);
    Check(BindNoiseSum());
    Check(ptx_readback(s_Renderer, image.data(), image.size() * sizeof(float)));
    Check(RebindNoiseHalf());
    return image;
}

PtxRenderer *RendererHip::GetHandle()
{
    return s_Renderer;
}

}
