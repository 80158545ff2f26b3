"""path-tracing_amd -- Python plumbing over the C-ABIs of the MI355X path-tracing backend.

This package holds NO rendering logic: it only loads
  * libptx_hip.so   (include/ptx.h)       HIP kernels + renderer   -- the product
  * libptx_host.so  (include/ptx_host.h)  C++ mirror of the reference's Scene/SceneBuilder/
                                          Camera/ExampleScenes (CPU only)
through ctypes, mirroring the call sequence of the reference's Renderer
(Path-Tracing/Renderer/Renderer.h:42-85): create -> scene_upload -> build_accel -> resize ->
render ... -> readback.

The directory name contains a hyphen, so import it with `load_package()` from
`__graft_entry__` / `tests/conftest.py` (importlib by path) under the module name
`path_tracing_amd`.

There is deliberately no CPU fallback: `Renderer()` raises if the HIP library is missing or no
GPU is visible.  The CPU oracle lives in /oracle and is test infrastructure only.
"""
from __future__ import annotations

import atexit
import ctypes as C
import glob
import os
import subprocess
import sys
import weakref

import numpy as np

# The runtime maps all HIP streams of the process onto GPU_MAX_HW_QUEUES hardware queues (default 4); frames in flight need
# one per stream to overlap (csrc/pt_runtime.hpp, hardwareQueuesGranted).  It is read at the first HIP call, so it has to
# be in the environment before torch initialises the device -- and it is the host's to set, which for Python callers is
# this package at import time (no thread of ours exists yet); the C library only reports what it finds.
os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
REPO_DIR = os.path.dirname(PKG_DIR)
HIP_LIB = os.environ.get("PTX_HIP_LIB") or os.path.join(PKG_DIR, "libptx_hip.so")  # PTX_HIP_LIB: an experimental build of the same ABI
HOST_LIB = os.environ.get("PTX_HOST_LIB") or os.path.join(PKG_DIR, "libptx_host.so")  # PTX_HOST_LIB: e.g. a sanitizer build

HIPCC_FLAGS = [
    "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared",
    "-ffp-contract=off", "-fno-fast-math",  # arithmetic conventions of csrc/pt_device.hpp
    "-fvisibility=hidden", "-Wall", "-Wno-unused-function",
    # No SLP vectorisation: under plain -O3 the compiler packs adjacent scalar f32 multiplies and adds into v_pk_mul_f32 /
    # v_pk_add_f32, whose operands must sit in aligned register PAIRS -- the shading kernels then spend a tenth of their VALU
    # instructions on v_mov shuffling (731 -> 391 in k_shade<false>) and every kernel pays in registers: k_trace_closest 64 -> 54
    # VGPRs, k_shade<false> 168 with 15 spilled -> 168 with none, k_shade<true> 238 -> 221, k_generate 57 -> 51 (8 waves).  Same
    # IEEE operations, same bits.  Measured (1 MI355X, 1080p, 8 spp, two runs each in one call): chess_like 2,139 / 2,158 ->
    # 2,265 / 2,290 Msamples/s, street_like 1,135 / 1,145 -> 1,176 / 1,174, temple_like 822 / 827 -> 843 / 846, atrium_like flat.
    "-fno-slp-vectorize",
]
HOST_FLAGS = ["-std=c++20", "-O2", "-fPIC", "-shared", "-Wall", "-Wextra", "-fvisibility=hidden"]

# every symbol include/ptx.h and include/ptx_host.h declare
PTX_SYMBOLS = [
    "ptx_create", "ptx_destroy", "ptx_last_error", "ptx_device_count", "ptx_abi_version", "ptx_scene_upload", "ptx_build_accel", "ptx_share_scene",
    "ptx_resize", "ptx_set_tile_shard", "ptx_set_backend", "ptx_reset_accumulation", "ptx_render",
    "ptx_render_frames", "ptx_synchronize", "ptx_readback", "ptx_readback_begin", "ptx_readback_end", "ptx_device_accum_ptr", "ptx_accum_bytes",
    "ptx_shard_bytes", "ptx_pack_shard", "ptx_unpack_shard", "ptx_unpack_shard_host", "ptx_unpack_shards", "ptx_bind_shard_accumulation", "ptx_get_stats", "ptx_bind_accumulation",
    "ptx_trace_rays", "ptx_test_input_stride", "ptx_test_output_stride", "ptx_test_eval", "ptx_test_texture",
    "ptx_postprocess", "ptx_read_output", "ptx_write_accumulation", "ptx_update_animation",
    "ptx_scene_upload_streamed", "ptx_texture_upload", "ptx_textures_commit", "ptx_texture_residency", "ptx_textures_rejected",
    "ptx_render_debug", "ptx_test_debug_eval",
    "ptx_present", "ptx_read_present", "ptx_device_present_ptr", "ptx_present_bytes",
    "ptx_render_guides", "ptx_read_guide", "ptx_device_guide_ptr", "ptx_denoise", "ptx_read_denoised", "ptx_device_denoised_ptr",
    "ptx_postprocess_denoised",
    "ptx_temporal_accumulate", "ptx_read_temporal", "ptx_device_temporal_ptr", "ptx_denoise_temporal",
    "ptx_temporal_accumulate_moments", "ptx_read_moments", "ptx_denoise_variance", "ptx_read_variance",
    "ptx_track_motion", "ptx_render_guides_motion", "ptx_read_motion", "ptx_device_motion_ptr", "ptx_temporal_accumulate_motion",
    "ptx_render_guides_specular", "ptx_read_specular_guide", "ptx_device_specular_guide_ptr",
    "ptx_temporal_accumulate_responsive", "ptx_read_fast_history", "ptx_device_fast_history_ptr",
    "ptx_despike", "ptx_read_despiked", "ptx_device_despiked_ptr", "ptx_chain_use_despiked", "ptx_postprocess_despiked",
    "ptx_meter", "ptx_read_meter", "ptx_device_meter_ptr", "ptx_meter_reset", "ptx_postprocess_metered",
    "ptx_grade", "ptx_grade_lut", "ptx_present_graded",
    "ptx_local_exposure", "ptx_read_local_exposure", "ptx_device_local_exposure_ptr", "ptx_postprocess_local",
    "ptx_present_upscaled",
    "ptx_noise_halves", "ptx_device_noise_half_ptr", "ptx_noise_meter", "ptx_read_noise",
    "ptx_adaptive_plan", "ptx_read_adaptive", "ptx_adaptive_clear", "ptx_noise_meter_adaptive",
]
PTH_SYMBOLS = [
    "pth_scene_names", "pth_scene_create", "pth_scene_create_ex", "pth_scene_destroy", "pth_last_error", "pth_scene_desc",
    "pth_scene_lights", "pth_scene_triangle_count", "pth_scene_raygen_uniform", "pth_scene_camera_matrices", "pth_scene_set_active_camera",
    "pth_scene_set_camera_pose", "pth_scene_update", "pth_scene_bone_count", "pth_scene_animation_state", "pth_decode_image", "pth_decode_image_levels", "pth_write_image", "pth_save_checkpoint", "pth_load_checkpoint",
    "pth_read_cube", "pth_white_balance_matrix",
]

SCENE_NATIVE_BC = 1  # PTH_SCENE_NATIVE_BC

BACKEND_WAVEFRONT = 0
BACKEND_MEGAKERNEL = 1


# ---------------------------------------------------------------------------------------
# ctypes images of the PODs in include/ptx.h
# ---------------------------------------------------------------------------------------
class SceneDesc(C.Structure):
    _fields_ = [
        ("vertices", C.c_void_p), ("vertexCount", C.c_uint64),
        ("indices", C.c_void_p), ("indexCount", C.c_uint64),
        ("transforms", C.c_void_p), ("transformCount", C.c_uint32),
        ("geometries", C.c_void_p), ("geometryCount", C.c_uint32),
        ("metallicRoughnessMaterials", C.c_void_p), ("metallicRoughnessMaterialCount", C.c_uint32),
        ("specularGlossinessMaterials", C.c_void_p), ("specularGlossinessMaterialCount", C.c_uint32),
        ("phongMaterials", C.c_void_p), ("phongMaterialCount", C.c_uint32),
        ("meshes", C.c_void_p), ("meshCount", C.c_uint32),
        ("models", C.c_void_p), ("modelCount", C.c_uint32),
        ("instances", C.c_void_p), ("instanceCount", C.c_uint32),
        ("skyboxKind", C.c_uint32), ("dxNormalTextures", C.c_uint32),
        ("textures", C.c_void_p), ("textureCount", C.c_uint32), ("forceFullTextureSize", C.c_uint32),
        ("skybox", C.c_void_p),
        ("animatedVertices", C.c_void_p), ("animatedVertexCount", C.c_uint64),
        ("animatedIndices", C.c_void_p), ("animatedIndexCount", C.c_uint64),
        ("textureMemoryBudget", C.c_uint64),
    ]


class TextureDesc(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("format", C.c_uint32), ("levels", C.c_uint32), ("data", C.c_void_p)]


TEXTURE_RGBA8_UNORM, TEXTURE_RGBA8_SRGB, TEXTURE_RGBA32F = 0, 1, 2
# block-compressed scene textures, uploaded as blocks (include/ptx.h, PtxTextureFormat; docs/NEXT_ROWS.md section 15)
TEXTURE_BC1_UNORM, TEXTURE_BC1_SRGB, TEXTURE_BC3_SRGB, TEXTURE_BC5_UNORM = 3, 4, 5, 6
PLACEHOLDER_TEXTURE_INDEX = 8  # PTX_PLACEHOLDER_TEXTURE_INDEX


class RaygenUniformData(C.Structure):
    _fields_ = [
        ("ViewInverse", C.c_float * 16), ("ProjInverse", C.c_float * 16), ("BounceCount", C.c_uint32),
        ("LensRadius", C.c_float), ("FocalDistance", C.c_float), ("SampleCount", C.c_uint32),
        ("TotalSamples", C.c_uint32),
    ]


class DirectionalLight(C.Structure):
    _fields_ = [("Color", C.c_float * 3), ("pad0", C.c_float), ("Direction", C.c_float * 3), ("pad1", C.c_float)]


class PointLight(C.Structure):
    _fields_ = [
        ("Color", C.c_float * 3), ("pad0", C.c_float), ("Position", C.c_float * 3), ("pad1", C.c_float),
        ("AttenuationConstant", C.c_float), ("AttenuationLinear", C.c_float), ("AttenuationQuadratic", C.c_float),
        ("pad2", C.c_float),
    ]


class LightsUbo(C.Structure):
    _fields_ = [("LightCount", C.c_uint32), ("pad", C.c_uint32 * 3), ("Directional", DirectionalLight),
                ("Lights", PointLight * 64)]


class PostProcessingUniformData(C.Structure):
    _fields_ = [("TotalSamples", C.c_uint32), ("Exposure", C.c_float), ("BloomThreshold", C.c_float), ("BloomIntensity", C.c_float)]


class DebugViewDesc(C.Structure):
    _fields_ = [("renderMode", C.c_uint32), ("raygenFlags", C.c_uint32), ("hitGroupFlags", C.c_uint32), ("reserved", C.c_uint32)]


# PTX_DEBUG_MODE_* / PTX_DEBUG_RAYGEN_* / PTX_DEBUG_HIT_* of include/ptx.h
(DEBUG_MODE_COLOR, DEBUG_MODE_WORLD_POSITION, DEBUG_MODE_NORMAL, DEBUG_MODE_TEXTURE_COORDS, DEBUG_MODE_MIPS, DEBUG_MODE_GEOMETRY,
 DEBUG_MODE_PRIMITIVE, DEBUG_MODE_INSTANCE) = range(8)
DEBUG_RAYGEN_FORCE_OPAQUE, DEBUG_RAYGEN_CULL_BACK_FACES = 1, 2
DEBUG_HIT_DISABLE_COLOR_TEXTURE, DEBUG_HIT_DISABLE_NORMAL_TEXTURE, DEBUG_HIT_DISABLE_MIP_MAPS, DEBUG_HIT_DISABLE_SHADOWS = 1, 2, 4, 8
DEBUG_EVAL_LIGHT_CONTRIBUTION, DEBUG_EVAL_RANDOM_COLOR = 0, 1  # `which` of ptx_test_debug_eval



class PresentDesc(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("format", C.c_uint32), ("toneMappingMode", C.c_uint32),
                ("ui", C.c_void_p), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


# PTX_PRESENT_* of include/ptx.h: the swapchain's format, and the flag bit
PRESENT_R8G8B8A8_SRGB, PRESENT_B8G8R8A8_SRGB, PRESENT_A2B10G10R10_UNORM, PRESENT_R16G16B16A16_SFLOAT = range(4)
PRESENT_UI_ON_DEVICE = 1


class DenoiseDesc(C.Structure):
    _fields_ = [("totalSamples", C.c_uint32), ("iterations", C.c_uint32), ("sigmaColor", C.c_float), ("sigmaNormal", C.c_float),
                ("sigmaPosition", C.c_float), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


GUIDE_NORMAL, GUIDE_POSITION, GUIDE_ALBEDO = range(3)  # PTX_GUIDE_* of include/ptx.h
MOTION_POSITION, MOTION_NORMAL = range(2)  # PTX_MOTION_* of include/ptx.h
# The defaults of Renderer.denoise, chosen on 4-spp frames of three scenes against 512 spp (docs/NEXT_ROWS.md section 13)
DENOISE_DEFAULTS = dict(iterations=3, sigma_color=1.5, sigma_normal=0.3, sigma_position=0.03)



class TemporalDesc(C.Structure):
    _fields_ = [("View", C.c_float * 16), ("Proj", C.c_float * 16), ("totalSamples", C.c_uint32), ("maxHistory", C.c_float),
                ("normalThreshold", C.c_float), ("positionThreshold", C.c_float), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


TEMPORAL_RESET = 1  # PTX_TEMPORAL_RESET
# The defaults of Renderer.temporal_accumulate: the thresholds are the filter's sigmas and nobody has tuned them; the defaults of the
# filter behind it come first in the sweep of tools/temporal_quality.py (docs/NEXT_ROWS.md section 14)
TEMPORAL_DEFAULTS = dict(max_history=32.0, normal_threshold=0.3, position_threshold=0.03)
TEMPORAL_DENOISE_DEFAULTS = dict(iterations=2, sigma_color=0.5, sigma_normal=0.3, sigma_position=0.03)
# The defaults of Renderer.denoise_variance: the best geometric mean over two scenes at 8 frames of history in the sweep of
# tools/temporal_quality.py (docs/NEXT_ROWS.md section 16); sigma_luminance is in standard deviations of the pixel's luminance
VARIANCE_DENOISE_DEFAULTS = dict(iterations=3, sigma_luminance=0.75, sigma_normal=0.3, sigma_position=0.03)


class SpecularGuidesDesc(C.Structure):
    _fields_ = [("maxBounces", C.c_uint32), ("roughnessMax", C.c_float), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


SPECULAR_SURFACE = 0  # PTX_SPECULAR_SURFACE of include/ptx.h
SPECULAR_CLASS_SURFACE, SPECULAR_CLASS_CAPPED, SPECULAR_CLASS_ESCAPED = range(3)  # the class in SURFACE.w = bounces + 16 * class
# The defaults of Renderer.render_guides_specular: first in the sweep of tools/specular_guides_quality.py (docs/NEXT_ROWS.md section 18)
SPECULAR_GUIDES_DEFAULTS = dict(max_bounces=1, roughness_max=0.2)


class ResponsiveDesc(C.Structure):
    _fields_ = [("fastHistory", C.c_float), ("clampSigma", C.c_float), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


RESPONSIVE_MOMENTS, RESPONSIVE_MOTION = 1, 2  # PTX_RESPONSIVE_* of include/ptx.h
# The defaults of Renderer.temporal_accumulate_responsive: first in the sweep of tools/temporal_quality.py --responsive
# (docs/NEXT_ROWS.md section 19)
RESPONSIVE_DEFAULTS = dict(fast_history=2.0, clamp_sigma=1.0)


class DespikeDesc(C.Structure):
    _fields_ = [("radius", C.c_uint32), ("rank", C.c_uint32), ("minTaps", C.c_uint32), ("gain", C.c_float), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


# The defaults of Renderer.despike: first in the sweep of tools/firefly_quality.py (docs/NEXT_ROWS.md section 20)
DESPIKE_DEFAULTS = dict(radius=2, rank=4, gain=1.0, min_taps=8)


class MeterDesc(C.Structure):
    _fields_ = [("source", C.c_uint32), ("mode", C.c_uint32), ("totalSamples", C.c_uint32), ("region", C.c_uint32 * 4), ("lowPermille", C.c_uint32),
                ("highPermille", C.c_uint32), ("keyLog2", C.c_float), ("compensation", C.c_float), ("minLog2Exposure", C.c_float),
                ("maxLog2Exposure", C.c_float), ("speedUp", C.c_float), ("speedDown", C.c_float), ("deltaSeconds", C.c_float), ("flags", C.c_uint32),
                ("reserved", C.c_uint32)]


class MeterResult(C.Structure):
    _fields_ = [("exposure", C.c_float), ("log2Exposure", C.c_float), ("avgLog2", C.c_float), ("targetLog2", C.c_float), ("counted", C.c_uint32),
                ("kept", C.c_uint32), ("black", C.c_uint32), ("rejected", C.c_uint32), ("under", C.c_uint32), ("over", C.c_uint32), ("valid", C.c_uint32),
                ("calls", C.c_uint32)]


METER_SUM, METER_DESPIKED, METER_DENOISED = 0, 1, 2  # PTX_METER_* of include/ptx.h: the image ...
METER_AVERAGE, METER_CENTRE, METER_REGION = 0, 1, 2  # ... and the weighting
# The defaults of Renderer.meter and of RendererHip::ExposureSettings (docs/NEXT_ROWS.md section 21): middle grey, a tenth cut off at
# the dark end and a twentieth at the bright one, +-8 stops, three times faster towards a brighter image than towards a darker one
METER_DEFAULTS = dict(mode=METER_AVERAGE, key_log2=-2.473931, compensation=0.0, min_log2_exposure=-8.0, max_log2_exposure=8.0, speed_up=1.0,
                      speed_down=3.0, low_permille=100, high_permille=50)


class GradeDesc(C.Structure):
    _fields_ = [("colourMatrix", C.c_float * 9), ("slope", C.c_float * 3), ("offset", C.c_float * 3), ("power", C.c_float * 3), ("saturation", C.c_float),
                ("curve", C.c_uint32), ("whitePoint", C.c_float), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


CURVE_REFERENCE, CURVE_REINHARD, CURVE_HABLE, CURVE_ACES_FIT = range(4)  # PTX_CURVE_* of include/ptx.h
CURVE_NAMES = {"reference": CURVE_REFERENCE, "reinhard": CURVE_REINHARD, "hable": CURVE_HABLE, "aces": CURVE_ACES_FIT}  # render_scene --curve
GRADE_USE_LUT, GRADE_LUT_SRGB_DOMAIN = 1, 2  # PTX_GRADE_*: the flag bits
GRADE_LUT_MIN_SIZE, GRADE_LUT_MAX_SIZE = 2, 65
# The defaults of Renderer.grade and of RendererHip::GradeSettings (docs/NEXT_ROWS.md section 22): the identity grade, under which
# ptx_grade gives ptx_postprocess's bits; the white point is read by CURVE_REINHARD only
GRADE_DEFAULTS = dict(colour_matrix=(1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0), slope=(1.0, 1.0, 1.0), offset=(0.0, 0.0, 0.0), power=(1.0, 1.0, 1.0),
                      saturation=1.0, curve=CURVE_REFERENCE, white_point=4.0)


class LocalExposureDesc(C.Structure):
    _fields_ = [("source", C.c_uint32), ("totalSamples", C.c_uint32), ("cellShift", C.c_uint32), ("pivotLog2", C.c_float), ("highlightContrast", C.c_float),
                ("shadowContrast", C.c_float), ("maxStops", C.c_float), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


LOCAL_EXPOSURE_PIVOT_METERED = 1  # PTX_LOCAL_EXPOSURE_PIVOT_METERED
# The defaults of Renderer.local_exposure and of RendererHip::LocalExposureSettings (docs/NEXT_ROWS.md section 23): cells of 32 x 32
# pixels, middle grey, highlights compressed to 0.6 of their distance from it and shadows to 0.8, at most four stops either way.
# Nobody has tuned them: they are a starting point that shows the effect, not the result of a sweep.
LOCAL_EXPOSURE_DEFAULTS = dict(cell_shift=5, pivot_log2=-2.473931, highlight_contrast=0.6, shadow_contrast=0.8, max_stops=4.0)


class UpscaleDesc(C.Structure):
    _fields_ = [("filter", C.c_uint32), ("sharpness", C.c_float), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


UPSCALE_CATMULL_ROM = 0  # PTX_UPSCALE_CATMULL_ROM
UPSCALE_GRADED = 1  # PTX_UPSCALE_GRADED
# The default of Renderer.present_upscaled and of RendererHip::UpscaleSettings (docs/NEXT_ROWS.md section 25).  Nobody has tuned it.
UPSCALE_DEFAULTS = dict(sharpness=0.5)


class NoiseDesc(C.Structure):
    _fields_ = [("samplesA", C.c_uint32), ("samplesB", C.c_uint32), ("exposure", C.c_float), ("threshold", C.c_float), ("tileShift", C.c_uint32),
                ("flags", C.c_uint32), ("reserved", C.c_uint32 * 2)]


class NoiseResult(C.Structure):
    _fields_ = [("meanError", C.c_float), ("maxError", C.c_float), ("tilesX", C.c_uint32), ("tilesY", C.c_uint32), ("converged", C.c_uint32),
                ("counted", C.c_uint32), ("black", C.c_uint32), ("rejected", C.c_uint32), ("valid", C.c_uint32), ("calls", C.c_uint32)]


NOISE_WRITE_SUM = 1  # PTX_NOISE_WRITE_SUM
# The defaults of Renderer.noise_meter and of RendererHip::NoiseSettings (docs/NEXT_ROWS.md section 26): tiles of 16 x 16 pixels, a check
# every eight render calls, none before 16 samples.  Nobody has tuned the threshold: it is a starting point, not the result of a sweep.
NOISE_DEFAULTS = dict(threshold=0.02, tile_shift=4, check_every=8, min_samples=16)


class AdaptiveDesc(C.Structure):
    _fields_ = [("tileShift", C.c_uint32), ("source", C.c_uint32), ("mask", C.c_void_p), ("dilate", C.c_uint32), ("framesA", C.c_uint32),
                ("framesB", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32 * 2)]


class AdaptivePlan(C.Structure):
    _fields_ = [("tilesX", C.c_uint32), ("tilesY", C.c_uint32), ("activeTiles", C.c_uint32), ("activePixels", C.c_uint32), ("seedTiles", C.c_uint32),
                ("generation", C.c_uint32)]


class AdaptiveMeterDesc(C.Structure):
    _fields_ = [("pendingA", C.c_uint32), ("pendingB", C.c_uint32), ("normalizeTo", C.c_uint32), ("exposure", C.c_float), ("threshold", C.c_float),
                ("tileShift", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32 * 2)]


ADAPTIVE_FROM_NOISE, ADAPTIVE_FROM_MASK = 0, 1  # PTX_ADAPTIVE_FROM_* of include/ptx.h
# The default margin of Renderer.adaptive_plan and of RendererHip::AdaptiveSettings (docs/NEXT_ROWS.md section 27): one tile.  Not tuned.
ADAPTIVE_DEFAULTS = dict(dilate=1)

TONE_MAPPING_SDR, TONE_MAPPING_HDR = 0, 1
ACCEL_REFIT, ACCEL_REBUILD = 0, 1
OUTPUT_RGBA8_SRGB, OUTPUT_RGBA32F = 0, 1
ABI_VERSION = 5  # PTX_ABI_VERSION of include/ptx.h


DEVICE_SINGLE_STREAM = 1  # PTX_DEVICE_SINGLE_STREAM


class DeviceDesc(C.Structure):
    _fields_ = [("deviceIndex", C.c_int32), ("backend", C.c_uint32), ("stream", C.c_void_p), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


class TileShard(C.Structure):
    _fields_ = [("rank", C.c_uint32), ("worldSize", C.c_uint32), ("tileSize", C.c_uint32)]


class Stats(C.Structure):
    _fields_ = [
        ("pathSamples", C.c_uint64), ("segments", C.c_uint64), ("shadowRays", C.c_uint64), ("retries", C.c_uint64),
        ("triangles", C.c_uint64), ("bvhNodes", C.c_uint64), ("lastRenderMs", C.c_double), ("lastTraceMs", C.c_double),
        ("lastBuildMs", C.c_double), ("traceLaunches", C.c_uint64), ("lastShadeMs", C.c_double), ("lastShadowMs", C.c_double), ("lastTailMs", C.c_double),
        ("tracedRays", C.c_uint64), ("hardwareQueues", C.c_uint64), ("treeTriangles", C.c_uint64), ("treeReferences", C.c_uint64),
    ]


assert C.sizeof(RaygenUniformData) == 148 and C.sizeof(LightsUbo) == 3120 and C.sizeof(PointLight) == 48

FN = {
    "GGXDistribution": 0, "Lambda": 1, "GGXSmith": 2, "DielectricFresnel": 3, "SchlickFresnel": 4,
    "EvaluateReflection": 5, "EvaluateRefraction": 6, "SampleGGX": 7, "sampleLobePdfs": 8, "evaluateBSDF": 9,
    "sampleBSDF": 10, "rng": 11, "sampleUniformDiskConcentric": 12, "sampleCosineHemisphere": 13,
    "computeTangentSpace": 14, "offsetRayOriginSelfIntersection": 15, "constructPrimaryRay": 16, "sincos": 17,
    "pow": 18, "sampleLight": 19, "offsetRayOriginShadowTerminator": 20, "constructPrimaryRayLens": 21,
    "computeDpnDuv": 22, "computeDpDxy": 23, "computeDerivatives": 24, "computeReflectedDifferentialRays": 25,
    "computeRefractedDifferentialRays": 26, "computeLod": 27, "missSkyboxTexCoords": 28, "hdrToLdr": 29, "atanAsin": 30,
    "postprocessPixel": 31, "compositionPixel": 32, "toneMapPixel": 33, "sampleMaterial": 34,
    "divide": 35, "sqrt": 36, "rsq": 37,
}


# ---------------------------------------------------------------------------------------
# build (used by __graft_entry__.build)
# ---------------------------------------------------------------------------------------
def _newer(target, sources):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(s) > t for s in sources)


HIP_TRANSLATION_UNIT = "ptx_capi.hip"  # the one translation unit of libptx_hip.so; it includes every header of csrc/


def hip_sources():
    """Every source file of the HIP library, the translation unit first (build dependencies, source digests of the profiles)."""
    csrc = os.path.join(PKG_DIR, "csrc")
    return [os.path.join(csrc, HIP_TRANSLATION_UNIT)] + sorted(glob.glob(os.path.join(csrc, "*.hpp")))


def build(force: bool = False, verbose: bool = True) -> None:
    """Compile the HIP extension for gfx950 and the C++ host mirror, in-tree."""
    csrc = os.path.join(PKG_DIR, "csrc")
    hip_src = [os.path.join(csrc, HIP_TRANSLATION_UNIT)] + hip_sources()[1:] + [os.path.join(REPO_DIR, "include", "ptx.h")]
    if force or _newer(HIP_LIB, hip_src):
        hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
        cmd = [hipcc] + HIPCC_FLAGS + ["-o", HIP_LIB, hip_src[0]]
        if verbose:
            print("[build]", " ".join(cmd), flush=True)
        subprocess.check_call(cmd)
    host = os.path.join(PKG_DIR, "host")
    host_src = [os.path.join(host, f) for f in ("Scene.cpp", "Camera.cpp", "ExampleScenes.cpp", "OutputSaver.cpp", "TextureImporter.cpp", "JpegDecoder.cpp", "SceneImporter.cpp", "SceneDescription.cpp", "FbxReader.cpp", "ObjReader.cpp", "host_capi.cpp")]
    # every header and source of host/ (a stale library after an edit to a header that is not listed is a silent wrong test)
    host_dep = sorted(glob.glob(os.path.join(host, "*.h")) + glob.glob(os.path.join(host, "*.cpp"))) + [
        os.path.join(REPO_DIR, "include", "ptx_host.h"), os.path.join(REPO_DIR, "include", "ptx.h")]
    if force or _newer(HOST_LIB, host_dep):
        cmd = ["g++"] + HOST_FLAGS + ["-o", HOST_LIB] + host_src
        if verbose:
            print("[build]", " ".join(cmd), flush=True)
        subprocess.check_call(cmd)


# ---------------------------------------------------------------------------------------
# library loading
# ---------------------------------------------------------------------------------------
_hip = None
_host = None


def load_host() -> C.CDLL:
    global _host
    if _host is None:
        if not os.path.exists(HOST_LIB):
            raise RuntimeError(f"{HOST_LIB} missing: run __graft_entry__.build()")
        lib = C.CDLL(HOST_LIB)
        lib.pth_scene_names.restype = C.c_char_p
        lib.pth_last_error.restype = C.c_char_p
        lib.pth_scene_create.restype = C.c_void_p
        lib.pth_scene_create.argtypes = [C.c_char_p, C.c_float, C.c_uint32]
        lib.pth_scene_create_ex.restype = C.c_void_p
        lib.pth_scene_create_ex.argtypes = [C.c_char_p, C.c_float, C.c_uint32, C.c_uint32]
        lib.pth_scene_destroy.argtypes = [C.c_void_p]
        lib.pth_scene_desc.argtypes = [C.c_void_p, C.POINTER(SceneDesc)]
        lib.pth_scene_lights.argtypes = [C.c_void_p, C.POINTER(LightsUbo)]
        lib.pth_scene_triangle_count.restype = C.c_uint64
        lib.pth_scene_triangle_count.argtypes = [C.c_void_p]
        lib.pth_scene_raygen_uniform.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_float, C.c_float,
                                                 C.c_uint32, C.c_uint32, C.POINTER(RaygenUniformData)]
        lib.pth_scene_camera_matrices.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_float), C.POINTER(C.c_float)]
        lib.pth_scene_set_active_camera.argtypes = [C.c_void_p, C.c_int32]
        lib.pth_scene_set_camera_pose.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float)]
        lib.pth_scene_update.argtypes = [C.c_void_p, C.c_float]
        lib.pth_scene_bone_count.argtypes = [C.c_void_p]
        lib.pth_scene_bone_count.restype = C.c_uint32
        lib.pth_scene_animation_state.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]
        lib.pth_decode_image.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(C.c_uint32), C.c_void_p, C.c_size_t]
        lib.pth_decode_image_levels.argtypes = [C.c_char_p, C.c_size_t]
        lib.pth_decode_image_levels.restype = C.c_uint32
        lib.pth_write_image.argtypes = [C.c_char_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t]
        lib.pth_save_checkpoint.argtypes = [C.c_char_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
        lib.pth_load_checkpoint.argtypes = [C.c_char_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_void_p, C.c_size_t]
        lib.pth_read_cube.argtypes = [C.c_char_p, C.POINTER(C.c_uint32), C.c_void_p, C.c_size_t]
        lib.pth_white_balance_matrix.argtypes = [C.c_double, C.POINTER(C.c_float)]
        _host = lib
    return _host


def load_hip() -> C.CDLL:
    """Load the HIP renderer.  If torch is in use, import it BEFORE calling this so both share
    one HIP runtime (the soname libamdhip64.so.7 is resolved to the copy already loaded)."""
    global _hip
    if _hip is None:
        if "torch" not in sys.modules:
            # torch brings its own libamdhip64; loaded after this library the process would hold two HIP runtimes, and the
            # one this library is bound to then finds no device (seen as ptx_create -> PTX_ERROR_NO_DEVICE when
            # __graft_entry__.build() and smoke() ran in one process)
            try:
                import torch  # noqa: F401
            except ImportError:
                pass
        if not os.path.exists(HIP_LIB):
            raise RuntimeError(f"{HIP_LIB} missing: the HIP extension is not built (run __graft_entry__.build())")
        lib = C.CDLL(HIP_LIB)
        have = None
        if hasattr(lib, "ptx_abi_version"):
            lib.ptx_abi_version.restype = C.c_uint32
            have = lib.ptx_abi_version()
        if have != ABI_VERSION and not os.environ.get("PTX_ABI_UNCHECKED"):  # PTX_ABI_UNCHECKED: A/B runs against an older experimental build
            raise RuntimeError(f"{HIP_LIB} has ABI {have}, this package was written against {ABI_VERSION} (include/ptx.h): rebuild")
        P = C.c_void_p
        lib.ptx_create.argtypes = [C.POINTER(DeviceDesc), C.POINTER(P)]
        lib.ptx_destroy.argtypes = [P]
        lib.ptx_destroy.restype = None
        lib.ptx_last_error.argtypes = [P]
        lib.ptx_last_error.restype = C.c_char_p
        lib.ptx_scene_upload.argtypes = [P, C.POINTER(SceneDesc)]
        lib.ptx_build_accel.argtypes = [P]
        lib.ptx_share_scene.argtypes = [P, P]
        lib.ptx_resize.argtypes = [P, C.c_uint32, C.c_uint32]
        lib.ptx_set_tile_shard.argtypes = [P, C.POINTER(TileShard)]
        lib.ptx_set_backend.argtypes = [P, C.c_uint32]
        lib.ptx_reset_accumulation.argtypes = [P]
        lib.ptx_render.argtypes = [P, C.POINTER(RaygenUniformData), C.POINTER(LightsUbo)]
        lib.ptx_render_frames.argtypes = [P, C.POINTER(RaygenUniformData), C.POINTER(LightsUbo), C.c_uint32, C.c_uint32]
        lib.ptx_synchronize.argtypes = [P]
        lib.ptx_readback.argtypes = [P, P, C.c_size_t]
        lib.ptx_readback_begin.argtypes = [P, P, C.c_size_t]
        lib.ptx_readback_end.argtypes = [P]
        lib.ptx_device_accum_ptr.argtypes = [P]
        lib.ptx_device_accum_ptr.restype = P
        lib.ptx_accum_bytes.argtypes = [P]
        lib.ptx_accum_bytes.restype = C.c_size_t
        lib.ptx_shard_bytes.argtypes = [P, C.c_uint32]
        lib.ptx_shard_bytes.restype = C.c_size_t
        lib.ptx_pack_shard.argtypes = [P, P]
        lib.ptx_unpack_shard.argtypes = [P, C.c_uint32, P]
        lib.ptx_unpack_shard_host.argtypes = [P, C.c_uint32, P, P, C.c_size_t]
        lib.ptx_unpack_shards.argtypes = [P, P, C.c_size_t, C.c_int, P, C.c_size_t]
        lib.ptx_bind_shard_accumulation.argtypes = [P, P, C.c_size_t]
        lib.ptx_get_stats.argtypes = [P, C.POINTER(Stats)]
        lib.ptx_postprocess.argtypes = [P, C.POINTER(PostProcessingUniformData), C.c_uint32]
        lib.ptx_read_output.argtypes = [P, C.c_uint32, P, C.c_size_t]
        lib.ptx_write_accumulation.argtypes = [P, P, C.c_size_t]
        lib.ptx_update_animation.argtypes = [P, P, C.c_uint32, P, C.c_uint32, C.c_uint32]
        lib.ptx_bind_accumulation.argtypes = [P, P, C.c_size_t]
        lib.ptx_trace_rays.argtypes = [P, P, C.c_uint32, C.c_int, P, P]
        lib.ptx_test_input_stride.argtypes = [C.c_uint32]
        lib.ptx_test_output_stride.argtypes = [C.c_uint32]
        lib.ptx_test_eval.argtypes = [P, C.c_uint32, P, P, C.c_uint32]
        lib.ptx_test_texture.argtypes = [P, P, P, C.c_uint32, C.c_int]
        lib.ptx_scene_upload_streamed.argtypes = [P, C.POINTER(SceneDesc), P]
        lib.ptx_texture_upload.argtypes = [P, C.c_uint32, C.POINTER(TextureDesc)]
        lib.ptx_textures_commit.argtypes = [P, C.POINTER(C.c_uint32)]
        lib.ptx_texture_residency.argtypes = [P, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        lib.ptx_textures_rejected.argtypes = [P, P, C.c_uint32]
        lib.ptx_textures_rejected.restype = C.c_uint32
        lib.ptx_render_debug.argtypes = [P, C.POINTER(RaygenUniformData), C.POINTER(LightsUbo), C.POINTER(DebugViewDesc)]
        lib.ptx_test_debug_eval.argtypes = [P, C.c_uint32, P, P, C.c_uint32]
        lib.ptx_present.argtypes = [P, C.POINTER(PresentDesc)]
        lib.ptx_read_present.argtypes = [P, P, C.c_size_t]
        lib.ptx_device_present_ptr.argtypes = [P]
        lib.ptx_device_present_ptr.restype = P
        lib.ptx_present_bytes.argtypes = [P]
        lib.ptx_present_bytes.restype = C.c_size_t
        lib.ptx_render_guides.argtypes = [P, C.POINTER(RaygenUniformData)]
        lib.ptx_read_guide.argtypes = [P, C.c_uint32, P, C.c_size_t]
        lib.ptx_device_guide_ptr.argtypes = [P, C.c_uint32]
        lib.ptx_device_guide_ptr.restype = P
        lib.ptx_denoise.argtypes = [P, C.POINTER(DenoiseDesc)]
        lib.ptx_read_denoised.argtypes = [P, P, C.c_size_t]
        lib.ptx_device_denoised_ptr.argtypes = [P]
        lib.ptx_device_denoised_ptr.restype = P
        lib.ptx_postprocess_denoised.argtypes = [P, C.POINTER(PostProcessingUniformData), C.c_uint32]
        lib.ptx_temporal_accumulate.argtypes = [P, C.POINTER(TemporalDesc)]
        lib.ptx_read_temporal.argtypes = [P, P, C.c_size_t]
        lib.ptx_device_temporal_ptr.argtypes = [P]
        lib.ptx_device_temporal_ptr.restype = P
        lib.ptx_denoise_temporal.argtypes = [P, C.POINTER(DenoiseDesc)]
        lib.ptx_temporal_accumulate_moments.argtypes = [P, C.POINTER(TemporalDesc)]
        lib.ptx_read_moments.argtypes = [P, P, C.c_size_t]
        lib.ptx_denoise_variance.argtypes = [P, C.POINTER(DenoiseDesc)]
        lib.ptx_read_variance.argtypes = [P, P, C.c_size_t]
        lib.ptx_track_motion.argtypes = [P, C.c_int]
        lib.ptx_render_guides_motion.argtypes = [P, C.POINTER(RaygenUniformData)]
        lib.ptx_read_motion.argtypes = [P, C.c_uint32, P, C.c_size_t]
        lib.ptx_device_motion_ptr.argtypes = [P, C.c_uint32]
        lib.ptx_device_motion_ptr.restype = P
        lib.ptx_temporal_accumulate_motion.argtypes = [P, C.POINTER(TemporalDesc), C.c_uint32]
        lib.ptx_render_guides_specular.argtypes = [P, C.POINTER(RaygenUniformData), C.POINTER(SpecularGuidesDesc)]
        lib.ptx_read_specular_guide.argtypes = [P, C.c_uint32, P, C.c_size_t]
        lib.ptx_device_specular_guide_ptr.argtypes = [P, C.c_uint32]
        lib.ptx_device_specular_guide_ptr.restype = P
        lib.ptx_temporal_accumulate_responsive.argtypes = [P, C.POINTER(TemporalDesc), C.POINTER(ResponsiveDesc)]
        lib.ptx_read_fast_history.argtypes = [P, P, C.c_size_t]
        lib.ptx_device_fast_history_ptr.argtypes = [P]
        lib.ptx_device_fast_history_ptr.restype = P
        lib.ptx_despike.argtypes = [P, C.POINTER(DespikeDesc)]
        lib.ptx_read_despiked.argtypes = [P, P, C.c_size_t]
        lib.ptx_device_despiked_ptr.argtypes = [P]
        lib.ptx_device_despiked_ptr.restype = P
        lib.ptx_chain_use_despiked.argtypes = [P, C.c_int]
        lib.ptx_postprocess_despiked.argtypes = [P, C.POINTER(PostProcessingUniformData), C.c_uint32]
        lib.ptx_meter.argtypes = [P, C.POINTER(MeterDesc)]
        lib.ptx_read_meter.argtypes = [P, C.POINTER(MeterResult), P]
        lib.ptx_device_meter_ptr.argtypes = [P]
        lib.ptx_device_meter_ptr.restype = P
        lib.ptx_meter_reset.argtypes = [P]
        lib.ptx_postprocess_metered.argtypes = [P, C.POINTER(PostProcessingUniformData), C.c_uint32, C.c_uint32]
        lib.ptx_grade.argtypes = [P, C.POINTER(GradeDesc), C.c_uint32]
        lib.ptx_grade_lut.argtypes = [P, C.c_uint32, P]
        lib.ptx_present_graded.argtypes = [P, C.POINTER(PresentDesc)]
        lib.ptx_local_exposure.argtypes = [P, C.POINTER(LocalExposureDesc)]
        lib.ptx_present_upscaled.argtypes = [P, C.POINTER(PresentDesc), C.POINTER(UpscaleDesc)]
        lib.ptx_read_local_exposure.argtypes = [P, P, C.c_size_t]
        lib.ptx_device_local_exposure_ptr.argtypes = [P]
        lib.ptx_device_local_exposure_ptr.restype = P
        lib.ptx_postprocess_local.argtypes = [P, C.POINTER(PostProcessingUniformData), C.c_uint32, C.c_uint32, C.c_uint32]
        lib.ptx_noise_halves.argtypes = [P, C.c_uint32]
        lib.ptx_device_noise_half_ptr.argtypes = [P, C.c_uint32]
        lib.ptx_device_noise_half_ptr.restype = P
        lib.ptx_noise_meter.argtypes = [P, C.POINTER(NoiseDesc)]
        lib.ptx_read_noise.argtypes = [P, C.POINTER(NoiseResult), P, C.c_size_t]
        lib.ptx_adaptive_plan.argtypes = [P, C.POINTER(AdaptiveDesc), C.POINTER(AdaptivePlan)]
        lib.ptx_read_adaptive.argtypes = [P, C.POINTER(AdaptivePlan), P, C.c_size_t, P, C.c_size_t]
        lib.ptx_adaptive_clear.argtypes = [P]
        lib.ptx_noise_meter_adaptive.argtypes = [P, C.POINTER(AdaptiveMeterDesc)]
        _hip = lib
    return _hip


class PtxError(RuntimeError):
    pass


# ---------------------------------------------------------------------------------------
# thin object wrappers
# ---------------------------------------------------------------------------------------
class Scene:
    """A host-side scene (PathTracing::Scene built by ExampleScenes::CreateScene)."""

    def __init__(self, name: str = "default", detail: float = 1.0, seed: int = 0, native_bc: bool = False):
        """native_bc: the .dds textures of an imported scene keep their BC1 / BC3 / BC5 blocks (PTH_SCENE_NATIVE_BC)."""
        self.lib = load_host()
        self.name = name
        if native_bc:
            self.handle = self.lib.pth_scene_create_ex(name.encode(), float(detail), int(seed), SCENE_NATIVE_BC)
        else:
            self.handle = self.lib.pth_scene_create(name.encode(), float(detail), int(seed))
        if not self.handle:
            raise PtxError(self.lib.pth_last_error().decode())

    def close(self):
        if getattr(self, "handle", None):
            self.lib.pth_scene_destroy(self.handle)
            self.handle = None

    __del__ = close

    @property
    def desc(self) -> SceneDesc:
        d = SceneDesc()
        if self.lib.pth_scene_desc(self.handle, C.byref(d)):
            raise PtxError("pth_scene_desc failed")
        return d

    @property
    def lights(self) -> LightsUbo:
        l = LightsUbo()
        self.lib.pth_scene_lights(self.handle, C.byref(l))
        return l

    @property
    def triangle_count(self) -> int:
        return int(self.lib.pth_scene_triangle_count(self.handle))

    def uniform(self, width, height, bounces=4, sample_count=1, total_samples=0, lens_radius=0.0,
                focal_distance=10.0) -> RaygenUniformData:
        u = RaygenUniformData()
        rc = self.lib.pth_scene_raygen_uniform(self.handle, width, height, bounces, lens_radius, focal_distance,
                                               sample_count, total_samples, C.byref(u))
        if rc:
            raise PtxError("pth_scene_raygen_uniform failed")
        return u

    def camera_matrices(self, width, height):
        """(View, Proj): the forward matrices of the active camera at this extent, 16 float32 each, column-major -- the inverses of
        uniform()'s ViewInverse and ProjInverse, as TemporalDesc takes them."""
        view, proj = np.zeros(16, np.float32), np.zeros(16, np.float32)
        FP = C.POINTER(C.c_float)
        if self.lib.pth_scene_camera_matrices(self.handle, width, height, view.ctypes.data_as(FP), proj.ctypes.data_as(FP)):
            raise PtxError("pth_scene_camera_matrices failed")
        return view, proj

    def update(self, time_step: float) -> bool:
        """Scene::Update(timeStep): True if something the renderer consumes has moved."""
        rc = self.lib.pth_scene_update(self.handle, float(time_step))
        if rc < 0:
            raise PtxError("pth_scene_update failed")
        return bool(rc)

    def animation_state(self):
        """(instance transforms n x 12, bone matrices m x 12) as Scene::Update left them."""
        n, m = self.desc.instanceCount, self.lib.pth_scene_bone_count(self.handle)
        it, bn = np.zeros((n, 12), np.float32), np.zeros((m, 12), np.float32)
        if self.lib.pth_scene_animation_state(self.handle, it.ctypes.data, n, bn.ctypes.data if m else None, m):
            raise PtxError("pth_scene_animation_state failed")
        return it, bn

    def set_active_camera(self, camera_id: int):
        if self.lib.pth_scene_set_active_camera(self.handle, camera_id):
            raise PtxError("bad camera id")

    def set_camera_pose(self, position, direction):
        p = (C.c_float * 3)(*position)
        d = (C.c_float * 3)(*direction)
        self.lib.pth_scene_set_camera_pose(self.handle, p, d)


_live_renderers: "weakref.WeakSet[Renderer]" = weakref.WeakSet()


@atexit.register
def _close_renderers():
    # A renderer still alive at interpreter exit would be destroyed by __del__ during module teardown, possibly after
    # the HIP runtime's own exit handlers have run (seen as "double free or corruption" at exit): destroy them first.
    for r in list(_live_renderers):
        r.close()


class Renderer:
    """include/ptx.h as an object.  Raises PtxError (with ptx_last_error) on any failure."""

    def __init__(self, device: int = 0, backend: int = BACKEND_WAVEFRONT, stream: int | None = None, single_stream: bool = False):
        self.lib = load_hip()
        self.handle = C.c_void_p()
        desc = DeviceDesc(device, backend, stream, DEVICE_SINGLE_STREAM if single_stream else 0, 0)
        rc = self.lib.ptx_create(C.byref(desc), C.byref(self.handle))
        if rc:
            self.handle = None
            raise PtxError(f"ptx_create failed with status {rc} (no HIP device? there is no CPU fallback)")
        self.width = self.height = 0
        _live_renderers.add(self)

    def close(self):
        if getattr(self, "handle", None):
            self.lib.ptx_destroy(self.handle)
            self.handle = None

    __del__ = close

    def _check(self, rc):
        if rc:
            raise PtxError(f"status {rc}: {self.lib.ptx_last_error(self.handle).decode()}")

    def upload(self, scene: Scene | SceneDesc):
        d = scene.desc if isinstance(scene, Scene) else scene
        self._check(self.lib.ptx_scene_upload(self.handle, C.byref(d)))
        self._check(self.lib.ptx_build_accel(self.handle))

    def upload_streamed(self, scene: Scene | SceneDesc, stand_in=None, build: bool = True):
        """ptx_scene_upload_streamed (+ ptx_build_accel): the scene textures whose `data` is NULL are pending and sample as the
        fixed 1 x 1 texture stand_in[i] (an index below 9; None: the placeholder for all) until upload_texture and
        commit_textures bring them in."""
        d = scene.desc if isinstance(scene, Scene) else scene
        si = None if stand_in is None else np.ascontiguousarray(stand_in, np.uint32)
        if si is not None and si.size != d.textureCount:
            raise PtxError(f"stand_in has {si.size} entries for {d.textureCount} textures")
        self._check(self.lib.ptx_scene_upload_streamed(self.handle, C.byref(d), si.ctypes.data if si is not None and si.size else None))
        if build:
            self._check(self.lib.ptx_build_accel(self.handle))

    def upload_texture(self, index: int, desc, fmt: int | None = None, levels: int = 1):
        """ptx_texture_upload: `desc` is a TextureDesc, or an H x W x 4 array (uint8 with `fmt` UNORM / sRGB, float32 for RGBA32F)
        holding level 0.  The texels are staged before the call returns."""
        if not isinstance(desc, TextureDesc):
            a = np.ascontiguousarray(desc)
            if a.ndim != 3 or a.shape[2] != 4 or a.dtype not in (np.uint8, np.float32):
                raise PtxError("upload_texture: need an H x W x 4 array of uint8 or float32")
            if fmt is None:
                fmt = TEXTURE_RGBA32F if a.dtype == np.float32 else TEXTURE_RGBA8_SRGB
            desc = TextureDesc(a.shape[1], a.shape[0], fmt, levels, a.ctypes.data)
        self._check(self.lib.ptx_texture_upload(self.handle, index, C.byref(desc)))

    def commit_textures(self) -> int:
        """ptx_textures_commit: the textures uploaded so far are what the frames enqueued from now on sample; returns their count."""
        n = C.c_uint32()
        self._check(self.lib.ptx_textures_commit(self.handle, C.byref(n)))
        return int(n.value)

    def texture_residency(self):
        """ptx_texture_residency: (resident, pending) over the scene's textures."""
        a, b = C.c_uint32(), C.c_uint32()
        self._check(self.lib.ptx_texture_residency(self.handle, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def textures_rejected(self):
        """ptx_textures_rejected: the scene texture indices of the block-compressed files the last upload could not take by the
        upload rules (they sample the white texel); empty for a scene without block-compressed textures."""
        n = int(self.lib.ptx_textures_rejected(self.handle, None, 0))
        idx = np.zeros(max(n, 1), np.uint32)
        n = min(n, int(self.lib.ptx_textures_rejected(self.handle, idx.ctypes.data, n)))
        return [int(i) for i in idx[:n]]

    def share_scene(self, owner: "Renderer"):
        """Render `owner`'s scene and tree instead of holding copies (ptx_share_scene): frames in flight share one scene."""
        self._check(self.lib.ptx_share_scene(self.handle, owner.handle))

    def resize(self, width: int, height: int):
        self._check(self.lib.ptx_resize(self.handle, width, height))
        self.width, self.height = width, height

    def set_tile_shard(self, rank: int, world: int, tile: int = 32):
        s = TileShard(rank, world, tile)
        self._check(self.lib.ptx_set_tile_shard(self.handle, C.byref(s)))

    def set_backend(self, backend: int):
        self._check(self.lib.ptx_set_backend(self.handle, backend))

    def reset(self):
        self._check(self.lib.ptx_reset_accumulation(self.handle))

    def render(self, uniform: RaygenUniformData, lights: LightsUbo):
        self._check(self.lib.ptx_render(self.handle, C.byref(uniform), C.byref(lights)))

    def render_debug(self, uniform: RaygenUniformData, lights: LightsUbo, mode: int, raygen_flags: int = 0, hit_flags: int = 0):
        """ptx_render_debug: one frame of the debug view (DEBUG_MODE_*, DEBUG_RAYGEN_*, DEBUG_HIT_*) STORED into the owned pixels."""
        view = DebugViewDesc(mode, raygen_flags, hit_flags, 0)
        self._check(self.lib.ptx_render_debug(self.handle, C.byref(uniform), C.byref(lights), C.byref(view)))

    def render_frames(self, uniform: RaygenUniformData, lights: LightsUbo, first_frame: int, frames: int):
        self._check(self.lib.ptx_render_frames(self.handle, C.byref(uniform), C.byref(lights), first_frame, frames))

    def synchronize(self):
        self._check(self.lib.ptx_synchronize(self.handle))

    def readback(self) -> np.ndarray:
        img = np.empty((self.height, self.width, 4), dtype=np.float32)
        self._check(self.lib.ptx_readback(self.handle, img.ctypes.data, img.nbytes))
        return img

    def readback_begin(self, pinned_ptr: int, nbytes: int):
        """ptx_readback_begin into page-locked host memory (e.g. a torch tensor with pin_memory=True)."""
        self._check(self.lib.ptx_readback_begin(self.handle, pinned_ptr, nbytes))

    def readback_end(self):
        self._check(self.lib.ptx_readback_end(self.handle))

    def update_animation(self, instance_transforms=None, bones=None, rebuild: bool = False):
        """ptx_update_animation: n x 12 instance transforms and / or m x 12 bone matrices, then refit (or rebuild)."""
        it = None if instance_transforms is None else np.ascontiguousarray(instance_transforms, np.float32).reshape(-1, 12)
        bn = None if bones is None else np.ascontiguousarray(bones, np.float32).reshape(-1, 12)
        self._check(self.lib.ptx_update_animation(self.handle, it.ctypes.data if it is not None else None, 0 if it is None else it.shape[0],
                                                  bn.ctypes.data if bn is not None else None, 0 if bn is None else bn.shape[0],
                                                  ACCEL_REBUILD if rebuild else ACCEL_REFIT))

    def write_accumulation(self, img: np.ndarray):
        img = np.ascontiguousarray(img, dtype=np.float32)
        self._check(self.lib.ptx_write_accumulation(self.handle, img.ctypes.data, img.nbytes))

    def postprocess(self, total_samples: int, exposure: float = 1.0, bloom_threshold: float = 1.0, bloom_intensity: float = 1.0,
                    tone_mapping: int = TONE_MAPPING_SDR):
        u = PostProcessingUniformData(total_samples, exposure, bloom_threshold, bloom_intensity)
        self._check(self.lib.ptx_postprocess(self.handle, C.byref(u), tone_mapping))

    def read_output(self, fmt: int = OUTPUT_RGBA8_SRGB) -> np.ndarray:
        out = np.empty((self.height, self.width, 4), dtype=np.float32 if fmt == OUTPUT_RGBA32F else np.uint8)
        self._check(self.lib.ptx_read_output(self.handle, fmt, out.ctypes.data, out.nbytes))
        return out

    def present(self, width: int, height: int, fmt: int = PRESENT_R8G8B8A8_SRGB, tone_mapping: int = TONE_MAPPING_SDR, ui=None, _call=None):
        """ptx_present: the last postprocess()' frame at the screen extent width x height in the swapchain format `fmt`, under
        the UI image `ui`: None, an H x W x 4 uint8 array (RGBA8 UNORM), or a torch tensor of that shape on the renderer's device,
        which is read in place."""
        flags, ptr = 0, None
        if ui is not None and hasattr(ui, "data_ptr"):
            if not ui.is_cuda:
                ui = ui.numpy()
            else:
                import torch
                if ui.dtype != torch.uint8 or tuple(ui.shape) != (height, width, 4) or not ui.is_contiguous():
                    raise ValueError("ui must be a contiguous height x width x 4 uint8 tensor")
                flags, ptr = PRESENT_UI_ON_DEVICE, ui.data_ptr()
        if ui is not None and not flags:
            ui = np.ascontiguousarray(ui, dtype=np.uint8)
            if ui.shape != (height, width, 4):
                raise ValueError("ui must be height x width x 4 uint8")
            ptr = ui.ctypes.data
        self._present_ui = ui  # the copy is asynchronous: keep the image alive
        d = PresentDesc(width, height, fmt, tone_mapping, ptr, flags, 0)
        self._check((_call or self.lib.ptx_present)(self.handle, C.byref(d)))
        self._present = (width, height, fmt)

    def present_graded(self, width: int, height: int, fmt: int = PRESENT_R8G8B8A8_SRGB, tone_mapping: int = TONE_MAPPING_SDR, ui=None):
        """ptx_present_graded: present() with the desc of the last grade() applied between the scaling blit and the UI."""
        self.present(width, height, fmt, tone_mapping, ui, _call=self.lib.ptx_present_graded)

    def present_upscaled(self, width: int, height: int, fmt: int = PRESENT_R8G8B8A8_SRGB, tone_mapping: int = TONE_MAPPING_SDR, ui=None,
                         sharpness: float = UPSCALE_DEFAULTS["sharpness"], graded: bool = False):
        """ptx_present_upscaled: present() for a screen extent of at least the render extent, with a clamped Catmull-Rom enlargement in
        the place of the linear blit and a clamped unsharp mask of strength `sharpness` (0 ... 2; 0 skips it) behind it; `graded`: with
        the desc of the last grade() where the tone mapping stands, as present_graded() has it."""
        up = UpscaleDesc(UPSCALE_CATMULL_ROM, sharpness, UPSCALE_GRADED if graded else 0, 0)
        self.present(width, height, fmt, tone_mapping, ui, _call=lambda handle, desc: self.lib.ptx_present_upscaled(handle, desc, C.byref(up)))

    def grade(self, tone_mapping: int = TONE_MAPPING_SDR, colour_matrix=GRADE_DEFAULTS["colour_matrix"], slope=GRADE_DEFAULTS["slope"],
              offset=GRADE_DEFAULTS["offset"], power=GRADE_DEFAULTS["power"], saturation: float = GRADE_DEFAULTS["saturation"],
              curve: int = GRADE_DEFAULTS["curve"], white_point: float = GRADE_DEFAULTS["white_point"], use_lut: bool = False, lut_srgb_domain: bool = False):
        """ptx_grade: the display transform -- colour matrix (row-major, 9 values), ASC CDL slope / offset / power and saturation, the
        tone curve CURVE_* and, with use_lut, the LUT of set_lut() -- on what the last postprocess*() left, into the image
        read_output() reads.  The desc is kept for present_graded().  Asynchronous."""
        d = GradeDesc((C.c_float * 9)(*np.asarray(colour_matrix, np.float32).reshape(9)), (C.c_float * 3)(*slope), (C.c_float * 3)(*offset),
                      (C.c_float * 3)(*power), saturation, curve, white_point, (GRADE_USE_LUT if use_lut else 0) | (GRADE_LUT_SRGB_DOMAIN if lut_srgb_domain else 0), 0)
        self._check(self.lib.ptx_grade(self.handle, C.byref(d), tone_mapping))

    def set_lut(self, lut):
        """ptx_grade_lut: an N x N x N x 3 float32 array indexed [blue, green, red] (red fastest: a .cube file's order, read_cube()'s
        result), 2 <= N <= 65; None clears it."""
        if lut is None:
            self._check(self.lib.ptx_grade_lut(self.handle, 0, None))
            return
        lut = np.ascontiguousarray(lut, dtype=np.float32)
        n = lut.shape[0]
        if lut.shape != (n, n, n, 3):
            raise ValueError("lut must be N x N x N x 3")
        self._check(self.lib.ptx_grade_lut(self.handle, n, lut.ctypes.data))

    def read_present(self) -> np.ndarray:
        """The image of the last present(): H x W x 4 uint8 (bytes in the format's order), H x W uint32 for A2B10G10R10,
        H x W x 4 float16 for R16G16B16A16."""
        if not getattr(self, "_present", None):
            raise PtxError("status 1: ptx_read_present: nothing presented yet (call ptx_present)")
        w, h, fmt = self._present
        if fmt == PRESENT_A2B10G10R10_UNORM:
            out = np.empty((h, w), np.uint32)
        else:
            out = np.empty((h, w, 4), np.float16 if fmt == PRESENT_R16G16B16A16_SFLOAT else np.uint8)
        self._check(self.lib.ptx_read_present(self.handle, out.ctypes.data, out.nbytes))
        return out

    def present_ptr(self) -> int:
        return int(self.lib.ptx_device_present_ptr(self.handle) or 0)

    def present_bytes(self) -> int:
        return int(self.lib.ptx_present_bytes(self.handle))

    def _read_image(self, read, *which) -> np.ndarray:
        """One RGBA32F image of the render extent through a ptx_read_* entry point (`which`: the image's index, where it takes one)."""
        img = np.empty((self.height, self.width, 4), dtype=np.float32)
        self._check(read(self.handle, *which, img.ctypes.data, img.nbytes))
        return img

    def render_guides(self, uniform: RaygenUniformData):
        """ptx_render_guides: the first hit's normal, position and base colour of every owned pixel, kept for denoise()."""
        self._check(self.lib.ptx_render_guides(self.handle, C.byref(uniform)))

    def read_guide(self, which: int) -> np.ndarray:
        """One guide image (GUIDE_NORMAL / GUIDE_POSITION / GUIDE_ALBEDO), H x W x 4 float32."""
        return self._read_image(self.lib.ptx_read_guide, which)

    def guide_ptr(self, which: int) -> int:
        return int(self.lib.ptx_device_guide_ptr(self.handle, which) or 0)

    def denoise(self, total_samples: int, iterations: int = DENOISE_DEFAULTS["iterations"], sigma_color: float = DENOISE_DEFAULTS["sigma_color"],
                sigma_normal: float = DENOISE_DEFAULTS["sigma_normal"], sigma_position: float = DENOISE_DEFAULTS["sigma_position"]):
        """ptx_denoise: the edge-avoiding a-trous filter over the mean of the accumulation image, guided by render_guides()."""
        d = DenoiseDesc(total_samples, iterations, sigma_color, sigma_normal, sigma_position, 0, 0)
        self._check(self.lib.ptx_denoise(self.handle, C.byref(d)))

    def read_denoised(self) -> np.ndarray:
        """The denoised MEAN of the last denoise(), H x W x 4 float32, alpha 1."""
        return self._read_image(self.lib.ptx_read_denoised)

    def denoised_ptr(self) -> int:
        return int(self.lib.ptx_device_denoised_ptr(self.handle) or 0)

    def postprocess_denoised(self, total_samples: int = 1, exposure: float = 1.0, bloom_threshold: float = 1.0, bloom_intensity: float = 1.0,
                             tone_mapping: int = TONE_MAPPING_SDR):
        """ptx_postprocess_denoised: postprocess() on the denoised image; it holds the mean, so total_samples is taken as 1."""
        u = PostProcessingUniformData(total_samples, exposure, bloom_threshold, bloom_intensity)
        self._check(self.lib.ptx_postprocess_denoised(self.handle, C.byref(u), tone_mapping))

    def temporal_accumulate(self, total_samples: int, view, proj, max_history: float = TEMPORAL_DEFAULTS["max_history"],
                            normal_threshold: float = TEMPORAL_DEFAULTS["normal_threshold"],
                            position_threshold: float = TEMPORAL_DEFAULTS["position_threshold"], flags: int = 0):
        """ptx_temporal_accumulate: blend the demodulated mean of the accumulation image with the history of the previous calls,
        reprojected through the position guide.  view, proj: the forward matrices of the camera render_guides() was given
        (Scene.camera_matrices)."""
        d = self._temporal_desc(total_samples, view, proj, max_history, normal_threshold, position_threshold, flags)
        self._check(self.lib.ptx_temporal_accumulate(self.handle, C.byref(d)))

    @staticmethod
    def _temporal_desc(total_samples, view, proj, max_history, normal_threshold, position_threshold, flags):
        d = TemporalDesc()
        d.View[:] = [float(v) for v in np.asarray(view, np.float32).reshape(16)]
        d.Proj[:] = [float(v) for v in np.asarray(proj, np.float32).reshape(16)]
        d.totalSamples, d.maxHistory, d.normalThreshold, d.positionThreshold, d.flags = total_samples, max_history, normal_threshold, position_threshold, flags
        return d

    def read_temporal(self) -> np.ndarray:
        """T of the last temporal_accumulate(): the accumulated MEAN, H x W x 4 float32, alpha = the history length (0: not valid)."""
        return self._read_image(self.lib.ptx_read_temporal)

    def temporal_ptr(self) -> int:
        return int(self.lib.ptx_device_temporal_ptr(self.handle) or 0)

    def denoise_temporal(self, iterations: int = TEMPORAL_DENOISE_DEFAULTS["iterations"], sigma_color: float = TEMPORAL_DENOISE_DEFAULTS["sigma_color"],
                         sigma_normal: float = TEMPORAL_DENOISE_DEFAULTS["sigma_normal"], sigma_position: float = TEMPORAL_DENOISE_DEFAULTS["sigma_position"]):
        """ptx_denoise_temporal: denoise() on T, which holds the mean; the result is read with read_denoised()."""
        d = DenoiseDesc(1, iterations, sigma_color, sigma_normal, sigma_position, 0, 0)
        self._check(self.lib.ptx_denoise_temporal(self.handle, C.byref(d)))

    def temporal_accumulate_moments(self, total_samples: int, view, proj, max_history: float = TEMPORAL_DEFAULTS["max_history"],
                                    normal_threshold: float = TEMPORAL_DEFAULTS["normal_threshold"],
                                    position_threshold: float = TEMPORAL_DEFAULTS["position_threshold"], flags: int = 0):
        """ptx_temporal_accumulate_moments: temporal_accumulate() that also accumulates the first two luminance moments, which
        denoise_variance() needs."""
        d = self._temporal_desc(total_samples, view, proj, max_history, normal_threshold, position_threshold, flags)
        self._check(self.lib.ptx_temporal_accumulate_moments(self.handle, C.byref(d)))

    def read_moments(self) -> np.ndarray:
        """The moment history of the last temporal_accumulate_moments(): H x W x 4 float32, (mu1, mu2, L_M, 0); L_M = 0: unknown."""
        return self._read_image(self.lib.ptx_read_moments)

    def denoise_variance(self, iterations: int = VARIANCE_DENOISE_DEFAULTS["iterations"], sigma_luminance: float = VARIANCE_DENOISE_DEFAULTS["sigma_luminance"],
                         sigma_normal: float = VARIANCE_DENOISE_DEFAULTS["sigma_normal"], sigma_position: float = VARIANCE_DENOISE_DEFAULTS["sigma_position"]):
        """ptx_denoise_variance: the filter on T with the colour weight in units of the pixel's own standard deviation, estimated from
        the moments; the result is read with read_denoised(), V_0 with read_variance()."""
        d = DenoiseDesc(1, iterations, sigma_luminance, sigma_normal, sigma_position, 0, 0)
        self._check(self.lib.ptx_denoise_variance(self.handle, C.byref(d)))

    def read_variance(self) -> np.ndarray:
        """V_0 of the last denoise_variance(): H x W float32, 0 on pixels that are not valid."""
        img = np.empty((self.height, self.width), dtype=np.float32)
        self._check(self.lib.ptx_read_variance(self.handle, img.ctypes.data, img.nbytes))
        return img

    def track_motion(self, enable: bool = True):
        """ptx_track_motion: update_animation() keeps the pose it replaces, for render_guides_motion().  Owner only."""
        self._check(self.lib.ptx_track_motion(self.handle, 1 if enable else 0))

    def render_guides_motion(self, uniform: RaygenUniformData):
        """ptx_render_guides_motion: render_guides() plus where every hit was, and which way its normal pointed, in the pose the
        temporal history was made from."""
        self._check(self.lib.ptx_render_guides_motion(self.handle, C.byref(uniform)))

    def read_motion(self, which: int) -> np.ndarray:
        """One motion image (MOTION_POSITION / MOTION_NORMAL), H x W x 4 float32; w = 1: known, 0: unknown (xyz = the guide) or a miss."""
        return self._read_image(self.lib.ptx_read_motion, which)

    def motion_ptr(self, which: int) -> int:
        return int(self.lib.ptx_device_motion_ptr(self.handle, which) or 0)

    def temporal_accumulate_motion(self, total_samples: int, view, proj, max_history: float = TEMPORAL_DEFAULTS["max_history"],
                                   normal_threshold: float = TEMPORAL_DEFAULTS["normal_threshold"],
                                   position_threshold: float = TEMPORAL_DEFAULTS["position_threshold"], flags: int = 0, moments: bool = False):
        """ptx_temporal_accumulate_motion: temporal_accumulate() (moments: temporal_accumulate_moments()) that looks the history up
        through the motion guides of render_guides_motion(), so that animated geometry keeps it."""
        d = self._temporal_desc(total_samples, view, proj, max_history, normal_threshold, position_threshold, flags)
        self._check(self.lib.ptx_temporal_accumulate_motion(self.handle, C.byref(d), int(moments)))

    def render_guides_specular(self, uniform: RaygenUniformData, max_bounces: int = None, roughness_max: float = None):
        """ptx_render_guides_specular: render_guides() that follows mirrors and glass (Roughness <= roughness_max) for up to
        max_bounces continuation rays and stores the guides of the surface the chain ends on; max_bounces 0 is render_guides()."""
        d = SpecularGuidesDesc(SPECULAR_GUIDES_DEFAULTS["max_bounces"] if max_bounces is None else max_bounces,
                               SPECULAR_GUIDES_DEFAULTS["roughness_max"] if roughness_max is None else roughness_max, 0, 0)
        self._check(self.lib.ptx_render_guides_specular(self.handle, C.byref(uniform), C.byref(d)))

    def read_specular_guide(self, which: int = 0) -> np.ndarray:
        """The fourth image of render_guides_specular() (SPECULAR_SURFACE), H x W x 4 float32: the first hit's position, and
        w = bounces + 16 * class (0: ended on a surface that is not followed, 1: stopped at max_bounces, 2: escaped)."""
        return self._read_image(self.lib.ptx_read_specular_guide, which)

    def specular_guide_ptr(self, which: int = 0) -> int:
        return int(self.lib.ptx_device_specular_guide_ptr(self.handle, which) or 0)

    def temporal_accumulate_responsive(self, total_samples: int, view, proj, max_history: float = TEMPORAL_DEFAULTS["max_history"],
                                       normal_threshold: float = TEMPORAL_DEFAULTS["normal_threshold"],
                                       position_threshold: float = TEMPORAL_DEFAULTS["position_threshold"], flags: int = 0,
                                       fast_history: float = RESPONSIVE_DEFAULTS["fast_history"], clamp_sigma: float = RESPONSIVE_DEFAULTS["clamp_sigma"],
                                       responsive_flags: int = 0):
        """ptx_temporal_accumulate_responsive: the accumulate call responsive_flags names (0: temporal_accumulate, RESPONSIVE_MOMENTS:
        temporal_accumulate_moments, RESPONSIVE_MOTION: temporal_accumulate_motion) carrying a fast history of at most fast_history
        frames, followed by a clamp of the long history into mean +- clamp_sigma standard deviations of the fast one's 5 x 5
        neighbourhood; a clamped pixel's history length drops to the fast one's, so a change of lighting shows within a few frames."""
        d = self._temporal_desc(total_samples, view, proj, max_history, normal_threshold, position_threshold, flags)
        rd = ResponsiveDesc(fast_history, clamp_sigma, responsive_flags, 0)
        self._check(self.lib.ptx_temporal_accumulate_responsive(self.handle, C.byref(d), C.byref(rd)))

    def read_fast_history(self) -> np.ndarray:
        """The fast history of the last temporal_accumulate_responsive(): H x W x 4 float32, (F.rgb demodulated, L_F); L_F = 0: unknown."""
        return self._read_image(self.lib.ptx_read_fast_history)

    def fast_history_ptr(self) -> int:
        return int(self.lib.ptx_device_fast_history_ptr(self.handle) or 0)

    def despike(self, radius: int = DESPIKE_DEFAULTS["radius"], rank: int = DESPIKE_DEFAULTS["rank"], gain: float = DESPIKE_DEFAULTS["gain"],
                min_taps: int = DESPIKE_DEFAULTS["min_taps"]):
        """ptx_despike: firefly suppression.  Every pixel's luminance is capped at `gain` times the `rank`-th largest luminance among
        the counting neighbours of its (2 radius + 1)^2 window, where there are at least min_taps of them; the result is an image in
        the accumulation's scale that the renderer keeps.  No scene and no guides needed."""
        d = DespikeDesc(radius, rank, min_taps, gain, 0, 0)
        self._check(self.lib.ptx_despike(self.handle, C.byref(d)))

    def read_despiked(self) -> np.ndarray:
        """The image of the last despike(): H x W x 4 float32, a running sum like readback()'s."""
        return self._read_image(self.lib.ptx_read_despiked)

    def despiked_ptr(self) -> int:
        return int(self.lib.ptx_device_despiked_ptr(self.handle) or 0)

    def chain_use_despiked(self, enable: bool = True):
        """ptx_chain_use_despiked: while on, the accumulate calls and denoise() read despike()'s image where they read the sum."""
        self._check(self.lib.ptx_chain_use_despiked(self.handle, 1 if enable else 0))

    def postprocess_despiked(self, total_samples: int, exposure: float = 1.0, bloom_threshold: float = 1.0, bloom_intensity: float = 1.0,
                             tone_mapping: int = TONE_MAPPING_SDR):
        """ptx_postprocess_despiked: postprocess() on despike()'s image, which is in the sum's scale: total_samples is the caller's."""
        u = PostProcessingUniformData(total_samples, exposure, bloom_threshold, bloom_intensity)
        self._check(self.lib.ptx_postprocess_despiked(self.handle, C.byref(u), tone_mapping))

    def meter(self, total_samples: int, delta_seconds: float = 0.0, source: int = METER_SUM, mode: int = METER_DEFAULTS["mode"], region=(0, 0, 0, 0),
              low_permille: int = METER_DEFAULTS["low_permille"], high_permille: int = METER_DEFAULTS["high_permille"],
              key_log2: float = METER_DEFAULTS["key_log2"], compensation: float = METER_DEFAULTS["compensation"],
              min_log2_exposure: float = METER_DEFAULTS["min_log2_exposure"], max_log2_exposure: float = METER_DEFAULTS["max_log2_exposure"],
              speed_up: float = METER_DEFAULTS["speed_up"], speed_down: float = METER_DEFAULTS["speed_down"]):
        """ptx_meter: a weighted luminance histogram of `source` (METER_SUM, METER_DESPIKED, METER_DENOISED: the image the output call
        of that name reads, with its total_samples convention) moves the exposure kept on the device towards
        2^(key_log2 - mean log2 luminance + compensation), at speed_up or speed_down per second over delta_seconds; the first call
        after a reset jumps.  region = (x0, x1, y0, y1) counts in METER_REGION only.  Asynchronous."""
        d = MeterDesc(source, mode, total_samples, (C.c_uint32 * 4)(*region), low_permille, high_permille, key_log2, compensation, min_log2_exposure,
                      max_log2_exposure, speed_up, speed_down, delta_seconds, 0, 0)
        self._check(self.lib.ptx_meter(self.handle, C.byref(d)))

    def read_meter(self, bins: bool = False):
        """ptx_read_meter: the MeterResult of the last meter(), with bins=True also the 256 bins (uint32); synchronises."""
        out = MeterResult()
        hist = np.empty(256, np.uint32) if bins else None
        self._check(self.lib.ptx_read_meter(self.handle, C.byref(out), hist.ctypes.data if bins else None))
        return (out, hist) if bins else out

    def meter_ptr(self) -> int:
        return int(self.lib.ptx_device_meter_ptr(self.handle) or 0)

    def meter_reset(self):
        """ptx_meter_reset: exposure 1 again, and the next meter() jumps to its target."""
        self._check(self.lib.ptx_meter_reset(self.handle))

    def postprocess_metered(self, total_samples: int, exposure: float = 1.0, bloom_threshold: float = 1.0, bloom_intensity: float = 1.0,
                            tone_mapping: int = TONE_MAPPING_SDR, source: int = METER_SUM):
        """ptx_postprocess_metered: postprocess(), postprocess_despiked() or postprocess_denoised() by `source`, with `exposure`
        multiplied by the metered exposure on the device."""
        u = PostProcessingUniformData(total_samples, exposure, bloom_threshold, bloom_intensity)
        self._check(self.lib.ptx_postprocess_metered(self.handle, C.byref(u), tone_mapping, source))

    def local_exposure(self, total_samples: int, source: int = METER_SUM, cell_shift: int = LOCAL_EXPOSURE_DEFAULTS["cell_shift"],
                       pivot_log2: float = LOCAL_EXPOSURE_DEFAULTS["pivot_log2"], highlight_contrast: float = LOCAL_EXPOSURE_DEFAULTS["highlight_contrast"],
                       shadow_contrast: float = LOCAL_EXPOSURE_DEFAULTS["shadow_contrast"], max_stops: float = LOCAL_EXPOSURE_DEFAULTS["max_stops"],
                       pivot_metered: bool = False):
        """ptx_local_exposure: the per-pixel gain G of `source` (METER_SUM, METER_DESPIKED, METER_DENOISED, with meter()'s total_samples
        convention): the base layer of the log2 luminance, taken from a bilateral grid of 2^cell_shift-pixel cells and 32 octave slices,
        is moved towards pivot_log2 by the factor highlight_contrast above it and shadow_contrast below, by at most max_stops.
        pivot_metered: the pivot is a display luminance, the metered exposure's log2 is taken off it on the device.  Asynchronous."""
        d = LocalExposureDesc(source, total_samples, cell_shift, pivot_log2, highlight_contrast, shadow_contrast, max_stops,
                              LOCAL_EXPOSURE_PIVOT_METERED if pivot_metered else 0, 0)
        self._check(self.lib.ptx_local_exposure(self.handle, C.byref(d)))

    def read_local_exposure(self) -> np.ndarray:
        """ptx_read_local_exposure: G of the last local_exposure(), H x W float32; synchronises."""
        img = np.empty((self.height, self.width), dtype=np.float32)
        self._check(self.lib.ptx_read_local_exposure(self.handle, img.ctypes.data, img.nbytes))
        return img

    def local_exposure_ptr(self) -> int:
        return int(self.lib.ptx_device_local_exposure_ptr(self.handle) or 0)

    def postprocess_local(self, total_samples: int, exposure: float = 1.0, bloom_threshold: float = 1.0, bloom_intensity: float = 1.0,
                          tone_mapping: int = TONE_MAPPING_SDR, source: int = METER_SUM, metered: bool = False):
        """ptx_postprocess_local: postprocess(), postprocess_despiked() or postprocess_denoised() by `source`, with `exposure` multiplied
        by the metered exposure (metered=True) or by 1, and then per pixel by G of local_exposure(), on the device."""
        u = PostProcessingUniformData(total_samples, exposure, bloom_threshold, bloom_intensity)
        self._check(self.lib.ptx_postprocess_local(self.handle, C.byref(u), tone_mapping, source, 1 if metered else 0))

    def stats(self) -> Stats:
        s = Stats()
        self._check(self.lib.ptx_get_stats(self.handle, C.byref(s)))
        return s

    def noise_halves(self, enable: bool = True):
        """ptx_noise_halves: make and zero the two half-images of the render extent (enable) or release them; bind one with
        bind_accumulation(noise_half_ptr(which), accum_bytes) and render into it."""
        self._check(self.lib.ptx_noise_halves(self.handle, 1 if enable else 0))

    def noise_half_ptr(self, which: int) -> int:
        return int(self.lib.ptx_device_noise_half_ptr(self.handle, which) or 0)

    def noise_meter(self, samples_a: int, samples_b: int, exposure: float = 1.0, threshold: float = NOISE_DEFAULTS["threshold"],
                    tile_shift: int = NOISE_DEFAULTS["tile_shift"], write_sum: bool = False):
        """ptx_noise_meter: the per-tile error of the two halves (samples_a in half 0, samples_b in half 1) on mean * exposure; with
        write_sum the internal accumulation image becomes A + B.  Asynchronous."""
        d = NoiseDesc(samples_a, samples_b, exposure, threshold, tile_shift, NOISE_WRITE_SUM if write_sum else 0, (C.c_uint32 * 2)(0, 0))
        self._check(self.lib.ptx_noise_meter(self.handle, C.byref(d)))

    def read_noise(self, tile_errors: bool = False):
        """ptx_read_noise: the NoiseResult of the last noise_meter(), with tile_errors=True also the tilesY x tilesX map of E_t
        (float32); synchronises."""
        out = NoiseResult()
        self._check(self.lib.ptx_read_noise(self.handle, C.byref(out), None, 0))
        if not tile_errors:
            return out
        tiles = np.empty((out.tilesY, out.tilesX), dtype=np.float32)
        self._check(self.lib.ptx_read_noise(self.handle, C.byref(out), tiles.ctypes.data, tiles.nbytes))
        return out, tiles

    def adaptive_plan(self, tile_shift: int = NOISE_DEFAULTS["tile_shift"], mask=None, dilate: int = ADAPTIVE_DEFAULTS["dilate"], frames_a: int = 0,
                      frames_b: int = 0) -> AdaptivePlan:
        """ptx_adaptive_plan: commit frames_a / frames_b (rendered into half 0 / 1 under the plan being replaced) to the counts, then plan
        the next render calls: the tiles within `dilate` of a seed -- a tile the last meter call left open or, with `mask` (tilesY x tilesX,
        non-zero = seed), the host's own.  Synchronises."""
        d = AdaptiveDesc(tile_shift, ADAPTIVE_FROM_NOISE, None, dilate, frames_a, frames_b, 0, (C.c_uint32 * 2)(0, 0))
        if mask is not None:
            m = np.asarray(mask)
            m = np.ascontiguousarray(m if m.dtype == np.uint8 else m != 0, dtype=np.uint8)  # bytes go to the device as they are
            side = 1 << tile_shift
            tiles = ((getattr(self, "width", 0) + side - 1) // side) * ((getattr(self, "height", 0) + side - 1) // side)
            if 3 <= tile_shift <= 6 and m.size != tiles:  # the library copies tilesX * tilesY bytes: never from a smaller array
                raise PtxError(f"adaptive_plan: the mask has {m.size} entries, the frame has {tiles} tiles of {side} pixels")
            d.source, d.mask = ADAPTIVE_FROM_MASK, m.ctypes.data
        out = AdaptivePlan()
        self._check(self.lib.ptx_adaptive_plan(self.handle, C.byref(d), C.byref(out)))
        return out

    def read_adaptive(self):
        """ptx_read_adaptive: (AdaptivePlan, the active tile ids in ascending order, the counts as a 2 x tilesY x tilesX uint32 array:
        frames per tile in half 0 and in half 1); synchronises."""
        out = AdaptivePlan()
        self._check(self.lib.ptx_read_adaptive(self.handle, C.byref(out), None, 0, None, 0))
        tiles = np.empty(out.activeTiles, dtype=np.uint32)
        counts = np.empty((2, out.tilesY, out.tilesX), dtype=np.uint32)
        self._check(self.lib.ptx_read_adaptive(self.handle, C.byref(out), tiles.ctypes.data, tiles.nbytes, counts.ctypes.data, counts.nbytes))
        return out, tiles, counts

    def adaptive_clear(self):
        """ptx_adaptive_clear: render calls cover the frame again; the counts stay."""
        self._check(self.lib.ptx_adaptive_clear(self.handle))

    def noise_meter_adaptive(self, pending_a: int, pending_b: int, normalize_to: int, exposure: float = 1.0, threshold: float = NOISE_DEFAULTS["threshold"],
                             tile_shift: int = NOISE_DEFAULTS["tile_shift"], write_sum: bool = False):
        """ptx_noise_meter_adaptive: noise_meter() with every tile's own sample counts (the committed ones plus pending_a / pending_b on
        the tiles of the plan in force); with write_sum the internal image holds every tile's sum scaled to normalize_to samples."""
        d = AdaptiveMeterDesc(pending_a, pending_b, normalize_to, exposure, threshold, tile_shift, NOISE_WRITE_SUM if write_sum else 0, (C.c_uint32 * 2)(0, 0))
        self._check(self.lib.ptx_noise_meter_adaptive(self.handle, C.byref(d)))

    def accum_ptr(self) -> int:
        return int(self.lib.ptx_device_accum_ptr(self.handle) or 0)

    def bind_accumulation(self, dev_ptr: int, nbytes: int):
        self._check(self.lib.ptx_bind_accumulation(self.handle, dev_ptr, nbytes))

    def shard_bytes(self, rank: int) -> int:
        return int(self.lib.ptx_shard_bytes(self.handle, rank))

    def pack_shard(self, dev_dst: int):
        self._check(self.lib.ptx_pack_shard(self.handle, dev_dst))

    def unpack_shard(self, rank: int, dev_src: int, pinned_host: int = 0, nbytes: int = 0):
        """ptx_unpack_shard; with `pinned_host` (address of a page-locked width*height*16-byte buffer) ptx_unpack_shard_host: the
        shard's pixels also go straight to the host's frame (complete after every rank's shard and readback_end())."""
        if pinned_host:
            self._check(self.lib.ptx_unpack_shard_host(self.handle, rank, dev_src, pinned_host, nbytes))
        else:
            self._check(self.lib.ptx_unpack_shard(self.handle, rank, dev_src))

    def unpack_shards(self, dev_src: int, stride_bytes: int, to_device_image: bool = True, pinned_host: int = 0, nbytes: int = 0):
        """ptx_unpack_shards: the whole gathered frame (every rank's shard, `stride_bytes` apart in `dev_src`) in one launch, to
        the device image and / or the host's page-locked frame (complete after readback_end())."""
        self._check(self.lib.ptx_unpack_shards(self.handle, dev_src, stride_bytes, 1 if to_device_image else 0, pinned_host or None, nbytes))

    def bind_shard_accumulation(self, dev_shard: int, nbytes: int = 0):
        """ptx_bind_shard_accumulation: accumulate this rank's samples in the dense tile-major shard buffer (0 unbinds)."""
        self._check(self.lib.ptx_bind_shard_accumulation(self.handle, dev_shard or None, nbytes))

    def trace_rays(self, rays: np.ndarray, any_hit: bool = False):
        rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 8)
        n = rays.shape[0]
        hits = np.zeros((n, 4), np.float32)
        ids = np.zeros((n, 2), np.uint32)
        self._check(self.lib.ptx_trace_rays(self.handle, rays.ctypes.data, n, int(any_hit), hits.ctypes.data,
                                            ids.ctypes.data))
        return hits, ids

    def test_texture(self, inputs: np.ndarray, implicit_lod: bool = False) -> np.ndarray:
        inputs = np.ascontiguousarray(inputs).view(np.uint32).reshape(-1, 7)
        out = np.zeros((inputs.shape[0], 4), np.uint32)
        self._check(self.lib.ptx_test_texture(self.handle, inputs.ctypes.data, out.ctypes.data, inputs.shape[0], int(implicit_lod)))
        return out

    def test_eval(self, fn: int, inputs: np.ndarray) -> np.ndarray:
        nin, nout = self.lib.ptx_test_input_stride(fn), self.lib.ptx_test_output_stride(fn)
        inputs = np.ascontiguousarray(inputs).view(np.uint32).reshape(-1, nin)
        out = np.zeros((inputs.shape[0], nout), np.uint32)
        self._check(self.lib.ptx_test_eval(self.handle, fn, inputs.ctypes.data, out.ctypes.data, inputs.shape[0]))
        return out

    def test_debug_eval(self, which: int, inputs: np.ndarray) -> np.ndarray:
        """ptx_test_debug_eval: DEBUG_EVAL_LIGHT_CONTRIBUTION (rows of 18 floats) or DEBUG_EVAL_RANDOM_COLOR (uint32 ids) -> rgb bits."""
        inputs = np.ascontiguousarray(inputs).view(np.uint32).reshape(-1, 18 if which == DEBUG_EVAL_LIGHT_CONTRIBUTION else 1)
        out = np.zeros((inputs.shape[0], 3), np.uint32)
        self._check(self.lib.ptx_test_debug_eval(self.handle, which, inputs.ctypes.data, out.ctypes.data, inputs.shape[0]))
        return out


OUTPUT_PNG, OUTPUT_JPG, OUTPUT_TGA, OUTPUT_HDR = 0, 1, 2, 3


def decode_image(data: bytes):
    """TextureImporter::Decode: returns (H x W x 4 array, uint8 or float32; channels in the file)."""
    lib = load_host()
    info = (C.c_uint32 * 4)()
    if lib.pth_decode_image(data, len(data), info, None, 0):
        raise PtxError(lib.pth_last_error().decode())
    img = np.empty((info[1], info[0], 4), np.float32 if info[3] else np.uint8)
    if lib.pth_decode_image(data, len(data), info, img.ctypes.data, img.nbytes):
        raise PtxError(lib.pth_last_error().decode())
    return img, int(info[2])


def decode_image_levels(data: bytes):
    """The file's whole mip chain (DDS): list of H_l x W_l x 4 arrays, level 0 first."""
    lib = load_host()
    info = (C.c_uint32 * 4)()
    levels = lib.pth_decode_image_levels(data, len(data))
    if not levels or lib.pth_decode_image(data, len(data), info, None, 0):
        raise PtxError(lib.pth_last_error().decode())
    dims = [(max(info[1] >> l, 1), max(info[0] >> l, 1)) for l in range(levels)]
    flat = np.empty(sum(h * w for h, w in dims) * 4, np.float32 if info[3] else np.uint8)
    if lib.pth_decode_image(data, len(data), info, flat.ctypes.data, flat.nbytes):
        raise PtxError(lib.pth_last_error().decode())
    out, at = [], 0
    for h, w in dims:
        out.append(flat[at:at + h * w * 4].reshape(h, w, 4))
        at += h * w * 4
    return out


def read_cube(path: str) -> np.ndarray:
    """host/CubeLut.h ReadCubeLut: a .cube 3-D LUT file as an N x N x N x 3 float32 array indexed [blue, green, red], what
    Renderer.set_lut takes.  A malformed, truncated or oversized file raises PtxError."""
    lib = load_host()
    size = C.c_uint32(0)
    if lib.pth_read_cube(str(path).encode(), C.byref(size), None, 0):
        raise PtxError(lib.pth_last_error().decode())
    n = size.value
    lut = np.empty((n, n, n, 3), np.float32)
    if lib.pth_read_cube(str(path).encode(), C.byref(size), lut.ctypes.data, lut.size):
        raise PtxError(lib.pth_last_error().decode())
    return lut


def white_balance_matrix(kelvin: float) -> np.ndarray:
    """host/CubeLut.h WhiteBalanceMatrix: the 3 x 3 colour matrix (float32, row-major, linear sRGB) that turns the light of a
    `kelvin` black body into white; 0 is the identity."""
    m = np.empty(9, np.float32)
    lib = load_host()
    if lib.pth_white_balance_matrix(float(kelvin), m.ctypes.data_as(C.POINTER(C.c_float))):
        raise PtxError(lib.pth_last_error().decode())
    return m.reshape(3, 3)


def write_image(path: str, img: np.ndarray, fmt: int = OUTPUT_PNG):
    """OutputSaver::WriteImage: H x W x 4 uint8 (Png / Tga) or float32 (Hdr)."""
    img = np.ascontiguousarray(img)
    if load_host().pth_write_image(str(path).encode(), fmt, img.shape[1], img.shape[0], img.ctypes.data, img.nbytes):
        raise PtxError(f"pth_write_image({path}) failed")


def save_checkpoint(path: str, accum: np.ndarray, total_samples: int):
    accum = np.ascontiguousarray(accum, dtype=np.float32)
    if load_host().pth_save_checkpoint(str(path).encode(), accum.shape[1], accum.shape[0], total_samples, accum.ctypes.data):
        raise PtxError(f"pth_save_checkpoint({path}) failed")


def load_checkpoint(path: str):
    lib = load_host()
    w, h, n = C.c_uint32(), C.c_uint32(), C.c_uint32()
    if lib.pth_load_checkpoint(str(path).encode(), C.byref(w), C.byref(h), C.byref(n), None, 0):
        raise PtxError(f"pth_load_checkpoint({path}) failed")
    img = np.empty((h.value, w.value, 4), np.float32)
    if lib.pth_load_checkpoint(str(path).encode(), C.byref(w), C.byref(h), C.byref(n), img.ctypes.data, img.nbytes):
        raise PtxError(f"pth_load_checkpoint({path}) failed")
    return img, n.value


def owned_tiles(width: int, height: int, rank: int, world: int, tile: int = 32):
    """Tile ids (row-major) a rank owns under the round-robin pixel-tile shard."""
    tiles_x = (width + tile - 1) // tile
    tiles_y = (height + tile - 1) // tile
    return list(range(rank, tiles_x * tiles_y, world))


def shard_mask(width: int, height: int, rank: int, world: int, tile: int = 32) -> np.ndarray:
    """Boolean H x W mask of the pixels a rank owns."""
    tiles_x = (width + tile - 1) // tile
    ys, xs = np.mgrid[0:height, 0:width]
    tid = (ys // tile) * tiles_x + (xs // tile)
    return (tid % world) == rank
