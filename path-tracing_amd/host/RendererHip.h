// RendererHip.h -- adapter with the reference's `Renderer` method names
// (Path-Tracing/Renderer/Renderer.h:42-85) on top of the C-ABI in include/ptx.h, so
// host code written against the static Renderer class keeps its call sequence:
//   Init -> UpdateSceneData -> OnResize -> [SetSettings] -> Render ... -> Shutdown.
// The path-tracing pass, the output stage (post-processing chain + OutputSaver, row N4), the optional denoiser in front of it and the screen path (row D15:
// scaling blit, tone mapping, UI composition, HDR10 encode, store in the swapchain's format) are implemented; the UI image
// itself (ImGui), the window and the swapchain stay with the host.
#pragma once

#include <memory>
#include <string>
#include <vector>

#include "OutputSaver.h"
#include "Scene.h"

namespace PathTracing
{

class RendererHip
{
public:
    // Renderer::PathTracingSettings (Renderer.h:61-66)
    struct PathTracingSettings
    {
        uint32_t BounceCount = 4;
        float LensRadius = 0.0f;
        float FocalDistance = 10.0f;
    };

    static void Init(int deviceIndex = 0, void *stream = nullptr);
    static void Shutdown();

    static void UpdateSceneData(const std::shared_ptr<Scene> &scene, bool updated);
    static void OnResize(uint32_t width, uint32_t height);
    static void SetSettings(const PathTracingSettings &settings);
    static void SetSamplesPerFrame(uint32_t samples); // s_RefreshRate.SamplesPerFrame (Renderer.cpp:1615-1657)
    static void SetTileShard(uint32_t rank, uint32_t worldSize, uint32_t tileSize);

    // Renderer::Render (Renderer.cpp:1659-1809): uniform fill + one path-tracing launch.
    static void Render();
    static void ResetAccumulationImage();
    // Renderer::SetDebugRaytracingPipeline (Renderer.cpp:579-610, :769-772): from now on Render() draws the debug view
    // (ptx_render_debug: PTX_DEBUG_MODE_*, PTX_DEBUG_RAYGEN_*, PTX_DEBUG_HIT_*), GetTotalSamples() is 1 and SaveOutput
    // post-processes the frame as one sample (Renderer.cpp:1697-1711).  SetPathTracingPipeline switches back and resets the accumulation.
    static void SetDebugRaytracingPipeline(uint32_t renderMode, uint32_t raygenFlags = 0, uint32_t hitGroupFlags = 0);
    static void SetPathTracingPipeline();

    // Renderer::PostProcessSettings (Renderer.h:68-75) / RenderSettings::Output
    struct PostProcessSettings
    {
        float Exposure = 1.0f;
        float BloomThreshold = 1.0f;
        float BloomIntensity = 1.0f;
        bool Hdr = false; // ToneMappingModeHDR
    };
    static void SetPostProcessSettings(const PostProcessSettings &settings);
    // The denoiser (ptx.h "Denoiser"; the reference has none).  Enabled: SaveOutput and Present run ptx_render_guides -> ptx_denoise
    // -> ptx_postprocess_denoised on the current running sum instead of ptx_postprocess; a debug-view frame is shown as it is.
    // Disabled (the default): both do exactly what they did without it.  The defaults are the measured ones of
    // docs/NEXT_ROWS.md section 13.
    // SpecularBounces (ptx.h "Specular-chain guides", docs/NEXT_ROWS.md section 18): 0 (the default) calls exactly what it called
    // before; above 0 ptx_render_guides_specular(SpecularBounces, SpecularRoughnessMax) takes ptx_render_guides' place, so that the
    // filter and the temporal stage see what mirrors and glass show.  The pass has no motion variant: with TemporalSettings'
    // MotionVectors in use the motion pass runs instead.
    struct DenoiserSettings
    {
        bool Enabled = false;
        uint32_t Iterations = 3;
        float SigmaColor = 1.5f;
        float SigmaNormal = 0.3f;
        float SigmaPosition = 0.03f;
        uint32_t SpecularBounces = 0;
        float SpecularRoughnessMax = 0.2f;
    };
    static void SetSettings(const DenoiserSettings &settings);
    // Temporal accumulation (ptx.h "Temporal accumulation").  Enabled together with the denoiser: SaveOutput and Present run
    // ptx_render_guides -> ptx_temporal_accumulate -> ptx_denoise_temporal -> ptx_postprocess_denoised, with the forward matrices of
    // the active camera; a frame whose accumulation continued from the previous one (nothing moved: the sum already holds every
    // sample) passes PTX_TEMPORAL_RESET.  Disabled (the default), or without the denoiser: everything does exactly what it did
    // without it.  The thresholds are the filter's sigmas; nobody has tuned them (docs/NEXT_ROWS.md section 14).
    // MotionVectors (ptx.h "Motion guides", docs/NEXT_ROWS.md section 17), together with the denoiser and Enabled: UpdateSceneData
    // turns ptx_track_motion on, and SaveOutput and Present call ptx_render_guides_motion and ptx_temporal_accumulate_motion (with
    // the VarianceSettings its moments form) in the plain pair's place, so that animated geometry keeps its history.  Off (the
    // default): nothing changes.  RendererHip itself never moves a pose: the switch pays off for a host that calls
    // ptx_update_animation on GetHandle() between frames (examples/motion_frame.cpp); without that every frame finds the previous
    // pose equal to the current one, at the motion variants' cost.
    // Responsive (ptx.h "Responsive temporal history", docs/NEXT_ROWS.md section 19), together with the denoiser and Enabled: the
    // accumulate call, whichever of the four the other switches choose, is made through ptx_temporal_accumulate_responsive with
    // FastHistory and ClampSigma, so that a change of lighting shows within a few frames.  Off (the default): SaveOutput and Present
    // enqueue exactly what they did without it.  The defaults are the measured ones of section 19.  A frame whose accumulation
    // continued from the previous one passes PTX_TEMPORAL_RESET as always, and on such a frame the responsive call is the base call:
    // the switch pays off while something moves and every frame's sum starts anew.
    struct TemporalSettings
    {
        bool Enabled = false;
        float MaxHistory = 32.0f;
        float NormalThreshold = 0.3f;
        float PositionThreshold = 0.03f;
        bool MotionVectors = false;
        bool Responsive = false;
        float FastHistory = 2.0f;
        float ClampSigma = 1.0f;
    };
    static void SetSettings(const TemporalSettings &settings);
    // Firefly suppression (ptx.h "Firefly suppression", docs/NEXT_ROWS.md section 20): a rank clamp of every pixel's luminance ahead of
    // everything SaveOutput and Present do with the sum.  Enabled without the denoiser: ptx_despike -> ptx_postprocess_despiked in
    // ptx_postprocess' place.  Enabled with the denoiser (and whatever temporal and variance settings): ptx_despike, then
    // ptx_chain_use_despiked, then the chain as configured, whose accumulate call or ptx_denoise reads the despiked image where it
    // read the sum.  Disabled (the default): SaveOutput and Present enqueue exactly what they did; disabling it turns the switch off
    // again.  A debug-view frame is shown as it is.  The defaults are the measured ones of section 20.
    struct FireflySettings
    {
        bool Enabled = false;
        uint32_t Radius = 2;
        uint32_t Rank = 4;
        float Gain = 1.0f;
        uint32_t MinTaps = 8;
    };
    static void SetSettings(const FireflySettings &settings);
    // Exposure metering (ptx.h "Exposure metering", docs/NEXT_ROWS.md section 21).  Enabled: SaveOutput and Present meter the image
    // they are about to post-process -- the sum, the despiked image or the denoised one, as the FireflySettings and the denoiser's
    // settings decide -- with ptx_meter over the time OnUpdate has counted since the last metered frame, and ptx_postprocess_metered takes the output call's
    // place: PostProcessSettings::Exposure times the metered exposure.  Disabled (the default): SaveOutput and Present enqueue exactly
    // what they did.  A debug-view frame is shown as it is.  PTX_METER_REGION is not offered here.  The defaults are METER_DEFAULTS of
    // the Python package.
    struct ExposureSettings
    {
        bool Enabled = false;
        uint32_t Mode = 0; // PTX_METER_AVERAGE
        float KeyLog2 = -2.473931f; // log2(0.18)
        float Compensation = 0.0f;
        float MinLog2Exposure = -8.0f;
        float MaxLog2Exposure = 8.0f;
        float SpeedUp = 1.0f;
        float SpeedDown = 3.0f;
        uint32_t LowPermille = 100;
        uint32_t HighPermille = 50;
    };
    static void SetSettings(const ExposureSettings &settings);
    // Renderer::OnUpdate (Renderer.cpp:1615-1657): the seconds since the previous frame.  They add up until a SaveOutput or Present
    // meters a frame, which adapts over them and uses them up: a second output call of the same frame, or every frame of a host that
    // never calls OnUpdate again, meters with deltaSeconds = 0 and leaves the exposure where it is.
    static void OnUpdate(float timeStep);
    // Local exposure (ptx.h "Local exposure", docs/NEXT_ROWS.md section 23).  Enabled together with the ExposureSettings: behind the
    // ptx_meter of the frame SaveOutput and Present call ptx_local_exposure on the same image with PTX_LOCAL_EXPOSURE_PIVOT_METERED, and
    // ptx_postprocess_local (metered = 1) takes ptx_postprocess_metered's place.  Disabled (the default), or without the
    // ExposureSettings: SaveOutput and Present enqueue exactly what they did.  The defaults are LOCAL_EXPOSURE_DEFAULTS of the Python
    // package; nobody has tuned them.
    struct LocalExposureSettings
    {
        bool Enabled = false;
        uint32_t CellShift = 5;
        float PivotLog2 = -2.473931f; // log2(0.18)
        float HighlightContrast = 0.6f;
        float ShadowContrast = 0.8f;
        float MaxStops = 4.0f;
    };
    static void SetSettings(const LocalExposureSettings &settings);
    // Display transform (ptx.h "Display transform", docs/NEXT_ROWS.md section 22).  Enabled: ptx_grade follows whichever post-process
    // call SaveOutput and Present make -- with the same tone-mapping mode, so ptx_read_output returns the graded image -- and Present
    // calls ptx_present_graded in ptx_present's place.  Disabled (the default): both enqueue exactly what they did, and nothing is
    // allocated.  TemperatureKelvin != 0 sets the colour matrix to WhiteBalanceMatrix(TemperatureKelvin) (CubeLut.h); LutFile, where not
    // empty, is read as a .cube file (ReadCubeLut) and handed to ptx_grade_lut by SetSettings, which throws on a file it cannot take.
    // A debug-view frame is shown as it is.  The defaults are GRADE_DEFAULTS of the Python package.
    struct GradeSettings
    {
        bool Enabled = false;
        uint32_t Curve = 0; // PTX_CURVE_REFERENCE
        float WhitePoint = 4.0f;
        float TemperatureKelvin = 0.0f;
        float Slope[3] = { 1.0f, 1.0f, 1.0f };
        float Offset[3] = { 0.0f, 0.0f, 0.0f };
        float Power[3] = { 1.0f, 1.0f, 1.0f };
        float Saturation = 1.0f;
        std::string LutFile;
        bool LutSrgbDomain = false;
    };
    static void SetSettings(const GradeSettings &settings);
    // Enlarging screen path (ptx.h "Enlarging screen path", docs/NEXT_ROWS.md section 25), for a host that renders below the window's
    // extent.  Enabled, and the extent given to Present at least the render extent on both axes: Present calls ptx_present_upscaled --
    // a clamped Catmull-Rom enlargement and a clamped unsharp mask of strength Sharpness (0 ... 2) where ptx_present has the linear
    // blit -- with PTX_UPSCALE_GRADED when the GradeSettings are on.  Disabled (the default), or for a smaller window: Present enqueues
    // exactly what it did.  SaveOutput is not concerned: it writes the render extent.  The default is UPSCALE_DEFAULTS of the Python
    // package; nobody has tuned it.
    struct UpscaleSettings
    {
        bool Enabled = false;
        float Sharpness = 0.5f;
    };
    static void SetSettings(const UpscaleSettings &settings);
    // Noise metering (ptx.h "Noise metering", docs/NEXT_ROWS.md section 26), for an offline render that should stop on a noise
    // threshold and not on a sample count.  Enabled: Render() binds one of the two halves of ptx_noise_halves -- half 0 on its even
    // calls since the accumulation restarted, half 1 on its odd ones -- before ptx_render and keeps both sample counts; every
    // CheckEvery calls, once MinSamples samples are in, it enqueues ptx_noise_meter on PostProcessSettings::Exposure.  GetNoise() reads
    // the last check's result (it synchronises when one is outstanding) and IsConverged() is true when every tile of it is converged.
    // SaveOutput, Present and ReadAccumulationImage first meter with PTX_NOISE_WRITE_SUM, bind the internal image, which then holds
    // A + B, for their calls and bind the next half again; before the second render call half 0 is the sum.  ResetAccumulationImage
    // zeroes both halves and the counts.  A debug-view frame is shown as it is.  Disabled (the default): Render, SaveOutput and
    // Present enqueue exactly what they did, and nothing is allocated.  The defaults are NOISE_DEFAULTS of the Python package; nobody
    // has tuned the threshold.
    struct NoiseSettings
    {
        bool Enabled = false;
        float Threshold = 0.02f;
        uint32_t TileShift = 4;
        uint32_t CheckEvery = 8;
        uint32_t MinSamples = 16;
    };
    static void SetSettings(const NoiseSettings &settings);
    static bool IsConverged();
    static PtxNoiseResult GetNoise();
    // Adaptive sampling (ptx.h "Adaptive sampling", docs/NEXT_ROWS.md section 27).  It has effect only together with
    // NoiseSettings::Enabled.  Enabled: at every check Render() enqueues ptx_noise_meter_adaptive with the samples rendered since the
    // last check as the pending counts (ptx_noise_meter at the first check after Init or OnResize, when the handle holds no counts yet
    // and every tile has received every sample) and then ptx_adaptive_plan(PTX_ADAPTIVE_FROM_NOISE, Dilate) with the same counts as
    // framesA and framesB; the render calls that follow cover the tiles that check left open, and their margin.  The two halves must
    // receive equal samples under one plan, so CheckEvery is rounded up to an even number.  IsConverged() is unchanged: every tile of
    // the last check is converged -- not "no tile is active", because the margin keeps converged tiles active.  SaveOutput, Present
    // and ReadAccumulationImage meter with PTX_NOISE_WRITE_SUM and normalizeTo = the samples of all render calls so far, so that every
    // tile shows its own mean.  ResetAccumulationImage clears the plan and zeroes the counts, and so does a change of
    // NoiseSettings::TileShift, whose tiles the counts are.  GetTotalSamples() counts render calls'
    // samples; ptx_get_stats' pathSamples says what a call traced.  Sharded frames are refused.  Disabled (the default): every call
    // enqueues exactly what it did.  The default is ADAPTIVE_DEFAULTS of the Python package; nobody has tuned it.
    struct AdaptiveSettings
    {
        bool Enabled = false;
        uint32_t Dilate = 1;
    };
    static void SetSettings(const AdaptiveSettings &settings);
    // Variance-guided denoising (ptx.h "Variance-guided denoising").  Enabled together with the denoiser and the temporal
    // accumulation: SaveOutput and Present run ptx_render_guides -> ptx_temporal_accumulate_moments -> ptx_denoise_variance ->
    // ptx_postprocess_denoised; the normal and position sigmas are the DenoiserSettings'.  Disabled (the default), or without either
    // of the two: everything does exactly what it did without it.  The defaults are the measured ones of docs/NEXT_ROWS.md section 16.
    struct VarianceSettings
    {
        bool Enabled = false;
        float SigmaLuminance = 0.75f;
        uint32_t Iterations = 3;
    };
    static void SetSettings(const VarianceSettings &settings);
    // RecordPostProcessCommands + RecordSaveOutputCommands on the current running sum, then OutputSaver::WriteImage
    static void SaveOutput(const OutputInfo &info);

    // Renderer::UpdateHdr (the swapchain was recreated, Application.cpp:281-286): Swapchain::IsHdr() of the surface Present draws
    // to.  true: the HDR tone-mapping mode and A2B10G10R10_UNORM (HDR10, Swapchain.cpp:317-340); false: SDR and R8G8B8A8_SRGB.
    static void UpdateHdr(bool isHdr);
    // The rest of a frame after the path-tracing pass (RecordPostProcessCommands with its final blit + RecordUICommands,
    // Renderer.cpp:928-1203): post-processes the current running sum with the PostProcessSettings and presents it at the
    // swapchain's extent under the UI image (RGBA8 UNORM, width * height * 4 bytes, nullptr: none).  Asynchronous: `ui` must
    // stay unchanged until ReadPresent or the next read-back.
    static void Present(uint32_t width, uint32_t height, const uint8_t *ui = nullptr);
    // the presented image: width * height * 4 bytes, R G B A per pixel or one packed A2B10G10R10 word
    static std::vector<std::byte> ReadPresent();

    static uint32_t GetTotalSamples();
    static std::vector<float> ReadAccumulationImage(); // RGBA32F running sum
    static PtxRenderer *GetHandle();

private:
    static void Check(int status);
};

}
