// motion_frame.cpp -- two frames of an animated scene through RendererHip with TemporalSettings::MotionVectors on (ptx.h "Motion
// guides", docs/NEXT_ROWS.md section 17), dumped raw so that a test can hold them against the same ptx_* calls made by hand
// (tests/test_motion.py).  RendererHip has no animation path of its own: the pose is moved with ptx_update_animation on its handle,
// as a host with animated scenes does today.
//
//   g++ -std=c++20 -O2 examples/motion_frame.cpp path-tracing_amd/host/{Scene,Camera,ExampleScenes,OutputSaver,TextureImporter,JpegDecoder,SceneImporter,SceneDescription,FbxReader,ObjReader,RendererHip}.cpp \
//       -Ipath-tracing_amd/host -Lpath-tracing_amd -lptx_hip -Wl,-rpath,'$ORIGIN/../path-tracing_amd' -o examples/motion_frame
//   examples/motion_frame animated_test 67 45 2 4 0.37 0 frames.bin     (scene, extent, spp, depth, time step, variance 0 / 1, file)
//   examples/motion_frame animated_test 67 45 2 4 0.37 0 frames.bin 1   (... with TemporalSettings::Responsive on: section 19,
//                                                                        tests/test_responsive.py)
//   examples/motion_frame animated_test 67 45 2 4 0.37 0 frames.bin 0 1 (... with FireflySettings on: section 20, tests/test_fireflies.py)
//   examples/motion_frame animated_test 67 45 2 4 0.37 0 frames.bin 0 1 0   (... and without the denoiser: the plain output path)
//   examples/motion_frame animated_test 67 45 2 4 0.37 0 frames.bin 0 0 0 1 (... with ExposureSettings on: section 21, tests/test_metering.py;
//                                                                            every frame is announced with OnUpdate(timeStep)
//                                                                            and, without the denoiser, saved twice)
//   examples/motion_frame animated_test 67 45 2 4 0.37 0 frames.bin 0 0 1 1 (... with the denoiser: the denoised image is metered)
//   examples/motion_frame animated_test 67 45 2 4 0.37 0 frames.bin 0 0 0 2 (... with ExposureSettings and LocalExposureSettings on: section 23,
//                                                                            tests/test_local_exposure.py; the exposure argument is 2)
//   examples/motion_frame animated_test 67 45 2 4 0.37 0 frames.bin 0 0 0 0 1 [look.cube] (... with GradeSettings on: section 22,
//                                                                            tests/test_grade.py: Hable's curve, 4500 K, a CDL grade,
//                                                                            the LUT where a file is named; every frame is also
//                                                                            presented at 100 x 37 and that image appended)
//   examples/motion_frame animated_test 67 45 2 4 0.37 0 frames.bin 0 0 0 0 1 - 1 (... with UpscaleSettings on as well: section 25,
//                                                                            tests/test_upscale.py; "-" names no LUT, and every frame is
//                                                                            presented at 100 x 68, where the adapter enlarges)
//   examples/motion_frame animated_test 67 45 16 4 0.37 0 frames.bin 0 0 0 0 0 - 0 1 (... with NoiseSettings on: section 26,
//                                                                            tests/test_noise_meter.py; CheckEvery 4, MinSamples 4; with the
//                                                                            argument given, 0 or 1, a trailer follows the presented images)
//
// The file holds, per frame, the running sum, T (ptx_read_temporal) and the output image (ptx_read_output, RGBA32F): 2 x 3 x width x
// height x 16 bytes.  With the grade argument given -- 0 or 1 -- the two presented images follow, 2 x 100 x 37 x 4 bytes (R8G8B8A8), or
// 2 x 100 x 68 x 4 with the upscale argument at 1.  The trailer of the noise argument: per frame the PtxNoiseResult GetNoise() returned after
// the frame's render calls and IsConverged() as a uint32, then one uint32 that says whether the handle holds halves at the end.  The trailer
// of the adaptive argument (AdaptiveSettings, section 27, tests/test_adaptive.py; 0: off, d + 1: on with Dilate d and a noise threshold
// of 0.05, at which the plans of the test's small frame are partial) follows it: per frame the PtxAdaptivePlan in force after the frame's
// render calls.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "ExampleScenes.h"
#include "RendererHip.h"

using namespace PathTracing;

static void Check(int status, const char *what)
{
    if (status != PTX_OK)
        throw error(std::string(what) + ": " + ptx_last_error(RendererHip::GetHandle()));
}

int main(int argc, char **argv)
{
    if (argc < 9 || argc > 18)
    {
        std::fprintf(stderr, "usage: motion_frame scene width height spp depth timeStep variance(0|1) out.bin [responsive(0|1) [despike(0|1) [denoiser(0|1) [exposure(0|1|2: with local exposure) "
                             "[grade(0|1) [lut.cube|- [upscale(0|1) [noise(0|1) [adaptive(0: off, d + 1: on with Dilate d)]]]]]]]]]\n");
        return 1;
    }
    const std::string name = argv[1];
    const uint32_t width = std::atoi(argv[2]), height = std::atoi(argv[3]), spp = std::atoi(argv[4]), bounces = std::atoi(argv[5]);
    const float timeStep = static_cast<float>(std::atof(argv[6]));
    const bool useVariance = std::atoi(argv[7]) != 0, useResponsive = argc >= 10 && std::atoi(argv[9]) != 0;
    const bool useDespike = argc >= 11 && std::atoi(argv[10]) != 0;
    const bool useDenoiser = argc < 12 || std::atoi(argv[11]) != 0; // 0: the plain output path, T is left as zeros
    const bool useExposure = argc >= 13 && std::atoi(argv[12]) != 0;
    const bool useLocalExposure = argc >= 13 && std::atoi(argv[12]) == 2; // behind the meter
    const bool presentToo = argc >= 14, useGrade = presentToo && std::atoi(argv[13]) != 0;
    const bool useLut = argc >= 15 && std::strcmp(argv[14], "-") != 0;
    const bool useUpscale = argc >= 16 && std::atoi(argv[15]) != 0;
    const bool noiseTrailer = argc >= 17, useNoise = noiseTrailer && std::atoi(argv[16]) != 0;
    const bool adaptiveTrailer = argc >= 18, useAdaptive = adaptiveTrailer && std::atoi(argv[17]) != 0;
    const uint32_t adaptiveDilate = useAdaptive ? static_cast<uint32_t>(std::atoi(argv[17])) - 1u : 0u;
    const uint32_t screenWidth = 100, screenHeight = useUpscale ? 68 : 37; // below the render extent on one axis, or above it on both
    setenv("GPU_MAX_HW_QUEUES", "16", 0);
    try
    {
        std::shared_ptr<Scene> scene = ExampleScenes::CreateScene(name, 0.25f, 0, 0u);
        RendererHip::Init(0);
        // the settings first: the upload below turns the scene's tracking off, and UpdateSceneData has to turn it on again
        RendererHip::DenoiserSettings denoiser;
        denoiser.Enabled = useDenoiser;
        RendererHip::TemporalSettings temporal;
        temporal.Enabled = temporal.MotionVectors = useDenoiser;
        temporal.Responsive = useResponsive;
        RendererHip::VarianceSettings variance;
        variance.Enabled = useVariance;
        RendererHip::SetSettings(denoiser);
        RendererHip::SetSettings(temporal);
        RendererHip::SetSettings(variance);
        RendererHip::FireflySettings firefly;
        firefly.Enabled = useDespike;
        RendererHip::SetSettings(firefly);
        RendererHip::ExposureSettings exposure;
        exposure.Enabled = useExposure;
        RendererHip::SetSettings(exposure);
        RendererHip::LocalExposureSettings localExposure;
        localExposure.Enabled = useLocalExposure;
        RendererHip::SetSettings(localExposure);
        RendererHip::GradeSettings grade; // the values tests/test_grade.py repeats by hand
        grade.Enabled = useGrade;
        grade.Curve = PTX_CURVE_HABLE;
        grade.TemperatureKelvin = 4500.0f;
        grade.Slope[0] = 1.1f; grade.Offset[1] = 0.01f; grade.Power[2] = 0.9f;
        grade.Saturation = 1.2f;
        if (useLut)
            grade.LutFile = argv[14];
        RendererHip::SetSettings(grade);
        RendererHip::UpscaleSettings upscale; // the default sharpness
        upscale.Enabled = useUpscale;
        RendererHip::SetSettings(upscale);
        RendererHip::NoiseSettings noise; // the values tests/test_noise_meter.py repeats by hand
        noise.Enabled = useNoise;
        noise.CheckEvery = 4;
        noise.MinSamples = 4;
        if (useAdaptive)
            noise.Threshold = 0.05f; // where some tiles of animated_test at 67 x 45 pass at the first check and some never do: partial plans
        RendererHip::SetSettings(noise);
        RendererHip::AdaptiveSettings adaptive; // the margin and the threshold above are what tests/test_adaptive.py repeats by hand
        adaptive.Enabled = useAdaptive;
        if (useAdaptive)
            adaptive.Dilate = adaptiveDilate;
        RendererHip::SetSettings(adaptive);
        scene->Update(0.0f);
        RendererHip::UpdateSceneData(scene, true);
        RendererHip::OnResize(width, height);
        RendererHip::PathTracingSettings settings;
        settings.BounceCount = bounces;
        RendererHip::SetSettings(settings);
        const size_t bytes = static_cast<size_t>(width) * height * 16;
        const size_t screenBytes = static_cast<size_t>(screenWidth) * screenHeight * 4;
        const size_t trailerAt = 6 * bytes + (presentToo ? 2 * screenBytes : 0), perFrame = sizeof(PtxNoiseResult) + 4;
        const size_t adaptiveAt = trailerAt + (noiseTrailer ? 2 * perFrame + 4 : 0);
        std::vector<char> file(adaptiveAt + (adaptiveTrailer ? 2 * sizeof(PtxAdaptivePlan) : 0));
        const std::string scratch = std::string(argv[8]) + ".png";
        for (int frame = 0; frame < 2; frame++)
        {
            // every frame is posed explicitly, the first one as Scene::Update(0) left it (the uploaded description is the bind pose)
            {
                if (frame)
                    scene->Update(timeStep);
                const auto instances = scene->GetModelInstances();
                const auto bones = scene->GetBoneTransforms();
                std::vector<PtxTransform> it(instances.size());
                for (size_t i = 0; i < instances.size(); i++)
                    std::memcpy(it[i].m, &instances[i].Transform.m[0][0], sizeof(float) * 12);
                Check(ptx_update_animation(RendererHip::GetHandle(), it.data(), static_cast<uint32_t>(it.size()), bones.empty() ? nullptr : bones.data(),
                                           static_cast<uint32_t>(bones.size()), PTX_ACCEL_REFIT), "ptx_update_animation");
                RendererHip::UpdateSceneData(scene, true); // the same scene, moved: the accumulation restarts, the history stays
            }
            if (useExposure)
                RendererHip::OnUpdate(timeStep);
            for (uint32_t i = 0; i < spp; i++)
                RendererHip::Render();
            if (noiseTrailer)
            {
                const PtxNoiseResult res = RendererHip::GetNoise();
                const uint32_t converged = RendererHip::IsConverged() ? 1u : 0u;
                std::memcpy(&file[trailerAt + frame * perFrame], &res, sizeof(res));
                std::memcpy(&file[trailerAt + frame * perFrame + sizeof(res)], &converged, 4);
            }
            if (adaptiveTrailer) // zeros where the handle holds no counts
            {
                PtxAdaptivePlan plan = {};
                (void)ptx_read_adaptive(RendererHip::GetHandle(), &plan, nullptr, 0, nullptr, 0);
                std::memcpy(&file[adaptiveAt + frame * sizeof(plan)], &plan, sizeof(plan));
            }
            const std::vector<float> sum = RendererHip::ReadAccumulationImage();
            std::memcpy(&file[(3 * frame) * bytes], sum.data(), bytes);
            RendererHip::SaveOutput({ scratch, { width, height }, 0, OutputFormat::Png });
            if (useExposure && !useDenoiser) // a second output call of the same frame: the time step is used up, the exposure stays
                RendererHip::SaveOutput({ scratch, { width, height }, 0, OutputFormat::Png });
            if (useDenoiser)
                Check(ptx_read_temporal(RendererHip::GetHandle(), &file[(3 * frame + 1) * bytes], bytes), "ptx_read_temporal");
            Check(ptx_read_output(RendererHip::GetHandle(), PTX_OUTPUT_RGBA32F, &file[(3 * frame + 2) * bytes], bytes), "ptx_read_output");
            if (presentToo)
            {
                RendererHip::Present(screenWidth, screenHeight, nullptr);
                const std::vector<std::byte> screen = RendererHip::ReadPresent();
                if (screen.size() != screenBytes)
                    throw error("the presented image has another size");
                std::memcpy(&file[6 * bytes + frame * screenBytes], screen.data(), screenBytes);
            }
        }
        if (noiseTrailer)
        {
            const uint32_t halves = ptx_device_noise_half_ptr(RendererHip::GetHandle(), 0u) ? 1u : 0u;
            std::memcpy(&file[trailerAt + 2 * perFrame], &halves, 4);
        }
        FILE *f = std::fopen(argv[8], "wb");
        if (!f || std::fwrite(file.data(), 1, file.size(), f) != file.size())
            throw error(std::string("cannot write ") + argv[8]);
        std::fclose(f);
        std::printf("scene %s %ux%u %u spp depth %u, two frames %g apart -> %s\n", name.c_str(), width, height, spp, bounces, (double)timeStep, argv[8]);
        RendererHip::Shutdown();
    }
    catch (const std::exception &e)
    {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
