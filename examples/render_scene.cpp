// render_scene.cpp -- the backend driven from C++ exactly as the reference drives its Renderer
// (Application::Run, Application.cpp:328-351): scene->Update -> UpdateSceneData -> Render ... and
// then the equivalent of its offline "Render" dialog (UserInterface.cpp:1076-1090): accumulate N
// samples, run the post-process chain (postprocess.comp -> bloom -> composition.comp -> toneMapping.comp) and
// hand the output image to the OutputSaver (PNG / TGA / HDR by file extension).
//
//   g++ -std=c++20 -O2 examples/render_scene.cpp path-tracing_amd/host/{Scene,Camera,ExampleScenes,OutputSaver,TextureImporter,JpegDecoder,SceneImporter,SceneDescription,FbxReader,ObjReader,RendererHip}.cpp \
//       -Ipath-tracing_amd/host -Lpath-tracing_amd -lptx_hip -Wl,-rpath,'$ORIGIN/../path-tracing_amd' -o examples/render_scene
//   examples/render_scene default 640 360 16 4 out.png
//   examples/render_scene default 640 360 1 4 normals.png --debug-mode 2    (the debug view instead: PTX_DEBUG_MODE_*)
//   examples/render_scene default 640 360 16 4 screen.png --present 1280x720          (the screen path: the frame as an SDR window of that size shows it)
//   examples/render_scene default 640 360 16 4 screen.a2b10g10r10 --present 1280x720 --hdr10   (... an HDR10 one: the raw packed words)
//   examples/render_scene default 640 360 16 4 screen.png --present 1280x720 --upscale 0.5   (... enlarged by the clamped Catmull-Rom filter and sharpened, not by the linear blit)
//   examples/render_scene default 640 360 4 4 denoised.png --denoise 3       (guides + the a-trous filter, 3 iterations, in front of the output stage)
//   examples/render_scene default 640 360 4 4 denoised.png --denoise-variance 3   (guides + temporal moments + the variance-guided filter)
//   examples/render_scene default 640 360 4 4 denoised.png --denoise 3 --specular-guides 4   (... whose guides follow mirrors and glass)
//   examples/render_scene default 640 360 4 4 denoised.png --denoise-variance 3 --responsive   (... whose history follows a change of lighting)
//   examples/render_scene default 640 360 1 4 despiked.png --despike        (firefly suppression: a rank clamp of every pixel's luminance; with --denoise ahead of the chain)
//   examples/render_scene default 640 360 16 4 metered.png --auto-exposure  (exposure metering: a luminance histogram sets the output stage's exposure)
//   examples/render_scene atrium_like 640 360 16 4 local.png --local-exposure  (local exposure behind the meter: highlights and shadows move towards middle grey)
//   examples/render_scene default 640 360 16 4 graded.png --curve aces --temperature 4500 --lut look.cube   (display transform: tone curve reference | reinhard | hable | aces,
//                                                                            white balance for a light of that many kelvin, a .cube 3-D LUT)
//   examples/render_scene default 640 360 4096 4 out.png --noise-threshold 0.02 --adaptive   (... and adaptive sampling: each check plans the tiles the next render calls cover)
//   examples/render_scene default 640 360 4096 4 out.png --noise-threshold 0.02   (noise metering: the sample count is the maximum; the render stops at the
//                                                                            first check where every tile's error is at or below the threshold)
//   examples/render_scene file:scene.gltf 640 360 16 4 out.png --native-bc   (.dds textures uploaded as blocks and decoded on the device)
#include <cmath>
#include <cstdio>
#include <filesystem>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../include/ptx_host.h"
#include "ExampleScenes.h"
#include "RendererHip.h"

using namespace PathTracing;

int main(int argc, char **argv)
{
    int debugMode = -1; // --debug-mode N anywhere on the line: one frame of the debug view instead of the path tracer
    for (int i = 1; i + 1 < argc; i++)
        if (std::string(argv[i]) == "--debug-mode")
        {
            debugMode = std::atoi(argv[i + 1]);
            for (int k = i; k + 2 < argc; k++)
                argv[k] = argv[k + 2];
            argc -= 2;
            break;
        }
    uint32_t presentWidth = 0, presentHeight = 0; // --present WxH [--hdr10]: the file holds what a window of that extent shows
    bool hdr10 = false;
    for (int i = 1; i < argc; i++)
        if (std::string(argv[i]) == "--hdr10")
        {
            hdr10 = true;
            for (int k = i; k + 1 < argc; k++)
                argv[k] = argv[k + 1];
            argc -= 1;
            break;
        }
    for (int i = 1; i + 1 < argc; i++)
        if (std::string(argv[i]) == "--present")
        {
            if (std::sscanf(argv[i + 1], "%ux%u", &presentWidth, &presentHeight) != 2 || !presentWidth || !presentHeight)
            {
                std::fprintf(stderr, "error: --present takes WxH\n");
                return 1;
            }
            for (int k = i; k + 2 < argc; k++)
                argv[k] = argv[k + 2];
            argc -= 2;
            break;
        }
    RendererHip::DenoiserSettings denoiser; // --denoise [iterations]: the filter between the path-tracing pass and the output stage
    for (int i = 1; i < argc; i++)
        if (std::string(argv[i]) == "--denoise")
        {
            denoiser.Enabled = true;
            // the iteration count is optional: one digit 1 .. 6 right behind the switch
            const bool counted = i + 1 < argc && std::strlen(argv[i + 1]) == 1 && argv[i + 1][0] >= '1' && argv[i + 1][0] <= '6';
            if (counted)
                denoiser.Iterations = static_cast<uint32_t>(argv[i + 1][0] - '0');
            const int drop = counted ? 2 : 1;
            for (int k = i; k + drop < argc; k++)
                argv[k] = argv[k + drop];
            argc -= drop;
            break;
        }
    // --denoise-variance [iterations]: the denoiser, the temporal accumulation and, in the fixed-sigma filter's place, the variance-guided one
    RendererHip::TemporalSettings temporal;
    RendererHip::VarianceSettings variance;
    for (int i = 1; i < argc; i++)
        if (std::string(argv[i]) == "--denoise-variance")
        {
            denoiser.Enabled = temporal.Enabled = variance.Enabled = true;
            const bool counted = i + 1 < argc && std::strlen(argv[i + 1]) == 1 && argv[i + 1][0] >= '1' && argv[i + 1][0] <= '6';
            if (counted)
                variance.Iterations = static_cast<uint32_t>(argv[i + 1][0] - '0');
            const int drop = counted ? 2 : 1;
            for (int k = i; k + drop < argc; k++)
                argv[k] = argv[k + drop];
            argc -= drop;
            break;
        }
    // --specular-guides [bounces]: with a denoiser, the guide pass follows mirrors and glass (1 .. 8 continuation rays, 1 without a count)
    for (int i = 1; i < argc; i++)
        if (std::string(argv[i]) == "--specular-guides")
        {
            const bool counted = i + 1 < argc && std::strlen(argv[i + 1]) == 1 && argv[i + 1][0] >= '1' && argv[i + 1][0] <= '8';
            denoiser.SpecularBounces = counted ? static_cast<uint32_t>(argv[i + 1][0] - '0') : 1u;
            const int drop = counted ? 2 : 1;
            for (int k = i; k + drop < argc; k++)
                argv[k] = argv[k + drop];
            argc -= drop;
            break;
        }
    // --responsive: with a temporal accumulation, the accumulate call keeps a fast history and clamps the long one into its box
    for (int i = 1; i < argc; i++)
        if (std::string(argv[i]) == "--responsive")
        {
            temporal.Responsive = true;
            for (int k = i; k + 1 < argc; k++)
                argv[k] = argv[k + 1];
            argc -= 1;
            break;
        }
    RendererHip::FireflySettings firefly; // --despike: firefly suppression ahead of the output stage, or of the chain where one is configured
    for (int i = 1; i < argc; i++)
        if (std::string(argv[i]) == "--despike")
        {
            firefly.Enabled = true;
            for (int k = i; k + 1 < argc; k++)
                argv[k] = argv[k + 1];
            argc -= 1;
            break;
        }
    RendererHip::ExposureSettings exposure; // --auto-exposure: the image about to be post-processed is metered and sets its own exposure
    for (int i = 1; i < argc; i++)
        if (std::string(argv[i]) == "--auto-exposure")
        {
            exposure.Enabled = true;
            for (int k = i; k + 1 < argc; k++)
                argv[k] = argv[k + 1];
            argc -= 1;
            break;
        }
    // --curve NAME, --lut FILE, --temperature K: the display transform; any of the three turns it on
    RendererHip::GradeSettings grade;
    for (const char *option : { "--curve", "--lut", "--temperature" })
        for (int i = 1; i < argc; i++)
            if (std::string(argv[i]) == option)
            {
                if (i + 1 >= argc)
                {
                    std::fprintf(stderr, "error: %s takes a value\n", option);
                    return 1;
                }
                const std::string value = argv[i + 1];
                grade.Enabled = true;
                if (option[2] == 'c')
                {
                    const char *names[] = { "reference", "reinhard", "hable", "aces" };
                    uint32_t curve = 0;
                    while (curve < 4u && value != names[curve])
                        curve++;
                    if (curve == 4u)
                    {
                        std::fprintf(stderr, "error: --curve takes reference, reinhard, hable or aces\n");
                        return 1;
                    }
                    grade.Curve = curve;
                }
                else if (option[2] == 'l')
                    grade.LutFile = value;
                else
                    grade.TemperatureKelvin = static_cast<float>(std::atof(value.c_str()));
                for (int k = i; k + 2 < argc; k++)
                    argv[k] = argv[k + 2];
                argc -= 2;
                break;
            }
    RendererHip::LocalExposureSettings localExposure; // --local-exposure: behind the meter, a bilateral grid compresses the scene's contrast (implies --auto-exposure)
    for (int i = 1; i < argc; i++)
        if (std::string(argv[i]) == "--local-exposure")
        {
            localExposure.Enabled = true;
            exposure.Enabled = true;
            for (int k = i; k + 1 < argc; k++)
                argv[k] = argv[k + 1];
            argc -= 1;
            break;
        }
    RendererHip::UpscaleSettings upscale; // --upscale [sharpness]: with --present WxH at or above the render extent, the clamped bicubic enlargement and unsharp mask
    for (int i = 1; i < argc; i++)
        if (std::string(argv[i]) == "--upscale")
        {
            upscale.Enabled = true;
            char *end = nullptr;
            const float sharpness = i + 1 < argc ? std::strtof(argv[i + 1], &end) : 0.0f;
            const bool given = i + 1 < argc && end != argv[i + 1] && *end == '\0' && argv[i + 1][0] != '-';
            if (given)
                upscale.Sharpness = sharpness;
            const int drop = given ? 2 : 1;
            for (int k = i; k + drop < argc; k++)
                argv[k] = argv[k + drop];
            argc -= drop;
            break;
        }
    RendererHip::NoiseSettings noise; // --noise-threshold T: the two half-sums are compared every CheckEvery samples, and the render stops when every tile is converged
    for (int i = 1; i + 1 < argc; i++)
        if (std::string(argv[i]) == "--noise-threshold")
        {
            char *end = nullptr;
            noise.Threshold = std::strtof(argv[i + 1], &end);
            if (end == argv[i + 1] || *end != '\0' || !(noise.Threshold >= 0.0f) || !std::isfinite(noise.Threshold))
            {
                std::fprintf(stderr, "--noise-threshold takes a finite number >= 0\n");
                return 1;
            }
            noise.Enabled = true;
            for (int k = i; k + 2 < argc; k++)
                argv[k] = argv[k + 2];
            argc -= 2;
            break;
        }
    RendererHip::AdaptiveSettings adaptive; // --adaptive: beside --noise-threshold, every check plans the tiles the render calls that follow cover
    for (int i = 1; i < argc; i++)
        if (std::string(argv[i]) == "--adaptive")
        {
            adaptive.Enabled = true;
            for (int k = i; k + 1 < argc; k++)
                argv[k] = argv[k + 1];
            argc -= 1;
            break;
        }
    if (adaptive.Enabled && !noise.Enabled)
    {
        std::fprintf(stderr, "--adaptive needs --noise-threshold T\n");
        return 1;
    }
    bool nativeBc = false; // --native-bc: the .dds textures of an imported scene are uploaded as BC1 / BC3 / BC5 blocks
    for (int i = 1; i < argc; i++)
        if (std::string(argv[i]) == "--native-bc")
        {
            nativeBc = true;
            for (int k = i; k + 1 < argc; k++)
                argv[k] = argv[k + 1];
            argc -= 1;
            break;
        }
    const std::string name = argc > 1 ? argv[1] : "default";
    const uint32_t width = argc > 2 ? std::atoi(argv[2]) : 640, height = argc > 3 ? std::atoi(argv[3]) : 360;
    const uint32_t spp = argc > 4 ? std::atoi(argv[4]) : 16, bounces = argc > 5 ? std::atoi(argv[5]) : 4;
    const char *out = argc > 6 ? argv[6] : "render.png";
    // the host's job, before the process first uses HIP (INTEGRATION.md "Frames in flight"): one hardware queue per stream
    setenv("GPU_MAX_HW_QUEUES", "16", 0);
    try
    {
        std::shared_ptr<Scene> scene = ExampleScenes::CreateScene(name, 0.25f, 0, nativeBc ? static_cast<uint32_t>(PTH_SCENE_NATIVE_BC) : 0u);
        RendererHip::Init(0);
        scene->Update(0.0f);
        RendererHip::UpdateSceneData(scene, true);
        RendererHip::OnResize(width, height);
        RendererHip::PathTracingSettings settings;
        settings.BounceCount = bounces;
        RendererHip::SetSettings(settings);
        RendererHip::SetSettings(denoiser);
        RendererHip::SetSettings(temporal);
        RendererHip::SetSettings(variance);
        RendererHip::SetSettings(firefly);
        RendererHip::SetSettings(exposure);
        RendererHip::SetSettings(localExposure);
        RendererHip::SetSettings(grade);
        RendererHip::SetSettings(upscale);
        RendererHip::SetSettings(noise);
        RendererHip::SetSettings(adaptive);
        if (debugMode >= 0)
            RendererHip::SetDebugRaytracingPipeline(static_cast<uint32_t>(debugMode));
        // RendererHip's own rule: at least 1, and with adaptive sampling rounded up to an even number
        uint32_t checkEvery = noise.CheckEvery ? noise.CheckEvery : 1u;
        if (adaptive.Enabled)
            checkEvery += checkEvery & 1u;
        uint32_t used = 0;
        uint64_t pathSamples = 0; // --adaptive: what the render calls traced (ptx_get_stats waits for each: the price of the report)
        for (uint32_t i = 0; i < (debugMode >= 0 ? 1u : spp); i++) // one sample per frame, like a Profile/Debug build (Config.h:34-36)
        {
            RendererHip::Render();
            used++;
            if (adaptive.Enabled && debugMode < 0)
            {
                PtxStats stats;
                if (ptx_get_stats(RendererHip::GetHandle(), &stats) != PTX_OK)
                    throw error(std::string("ptx_get_stats: ") + ptx_last_error(RendererHip::GetHandle()));
                pathSamples += stats.pathSamples;
            }
            // the third stop condition beside MaxSampleCount and MaxTime (Renderer.cpp:1701-1704): asked only after a check, so that
            // the other render calls stay asynchronous
            if (noise.Enabled && debugMode < 0 && used % checkEvery == 0u && RendererHip::IsConverged())
                break;
        }
        if (noise.Enabled && debugMode < 0)
        {
            const PtxNoiseResult res = RendererHip::GetNoise();
            std::printf("noise threshold %g: %u of at most %u samples used, %s; last check: mean error %.6g, max %.6g, %u of %u tiles converged\n", (double)noise.Threshold,
                        used, spp, RendererHip::IsConverged() ? "converged" : "not converged", (double)res.meanError, (double)res.maxError, res.converged,
                        res.tilesX * res.tilesY);
            if (adaptive.Enabled)
                std::printf("adaptive sampling: %.3f samples per pixel on average (%llu path samples over %u pixels), stopped at sample %u\n",
                            (double)pathSamples / ((double)width * height), (unsigned long long)pathSamples, width * height, used);
        }
        const std::vector<float> acc = RendererHip::ReadAccumulationImage();
        const float inv = 1.0f / static_cast<float>(RendererHip::GetTotalSamples());
        double sum = 0.0;
        for (size_t p = 0; p < static_cast<size_t>(width) * height; p++)
            for (int c = 0; c < 3; c++)
                sum += acc[p * 4 + c] * inv;
        // post-process chain + OutputSaver: the format follows the file extension like UserInterface.cpp:1060-1074
        const std::string ext = std::filesystem::path(out).extension().string();
        const OutputFormat format = ext == ".hdr" ? OutputFormat::Hdr : ext == ".tga" ? OutputFormat::Tga : OutputFormat::Png;
        if (presentWidth)
        {
            // no ImGui here: the UI image is a title bar, opaque on the left and absent on the right
            std::vector<uint8_t> ui(static_cast<size_t>(presentWidth) * presentHeight * 4, 0);
            for (uint32_t y = 0; y < (presentHeight < 16 ? presentHeight : 16u); y++)
                for (uint32_t x = 0; x < presentWidth / 2; x++)
                {
                    uint8_t *t = &ui[(static_cast<size_t>(y) * presentWidth + x) * 4];
                    t[0] = 40; t[1] = 44; t[2] = 52; t[3] = 255;
                }
            RendererHip::UpdateHdr(hdr10);
            RendererHip::Present(presentWidth, presentHeight, ui.data());
            const std::vector<std::byte> screen = RendererHip::ReadPresent();
            if (hdr10)
            {
                FILE *f = std::fopen(out, "wb");
                if (!f || std::fwrite(screen.data(), 1, screen.size(), f) != screen.size())
                    throw error(std::string("cannot write ") + out);
                std::fclose(f);
                uint32_t word = 0;
                std::memcpy(&word, &screen[(static_cast<size_t>(presentHeight / 2) * presentWidth + presentWidth / 2) * 4], 4);
                std::printf("HDR10 centre pixel: R %u G %u B %u (10-bit ST 2084 codes, BT.2020)\n", word & 1023u, (word >> 10) & 1023u, (word >> 20) & 1023u);
            }
            else if (!OutputSaver::WriteImage({ out, { presentWidth, presentHeight }, 0, OutputFormat::Png }, screen))
                throw error(std::string("cannot write ") + out);
        }
        else
            RendererHip::SaveOutput({ out, { width, height }, 0, format });
        std::printf("scene %s %ux%u %u spp depth %u: mean radiance %.9g -> %s\n", name.c_str(), width, height, debugMode >= 0 ? spp : used, bounces,
                    sum / (3.0 * width * height), out);
        RendererHip::Shutdown();
    }
    catch (const std::exception &e)
    {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
