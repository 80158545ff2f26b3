/*
 * ptx.h -- C-ABI of the MI355X wavefront path-tracing backend.
 *
 * This is the drop-in boundary for ONE hot path of piotrprzybyszdev/Path-Tracing:
 * the vkCmdTraceRaysKHR(W,H,1) pass recorded by Renderer::RecordPathTracingCommands
 * (Path-Tracing/Renderer/Renderer.cpp:892-926) and the scene upload that feeds it
 * (Renderer::UpdateSceneData, Renderer.cpp:238-439).  The reference has no FFI; the
 * seam is the static C++ class `Renderer` (Renderer/Renderer.h:39-85).  Every entry
 * point below names the reference call it stands in for.
 *
 * Rules of the ABI: plain pointers and sizes, no C++ types, no exceptions; every
 * function returns a PtxStatus (0 = OK) and ptx_last_error() gives the message
 * (the reference throws PathTracing::error, Core/Core.h:117-122).  A handle is NOT
 * thread-safe; one host thread per handle, one handle per GPU.
 *
 * All structs in the "data contract" block are byte-compatible with the reference's
 * host/device shared headers (Path-Tracing/Shaders/ShaderTypes.incl and
 * ShaderRendererTypes.incl); sizes are checked by PTX_STATIC_ASSERTs (the
 * equivalent of the reference's PaddingTest.cpp).
 */
#ifndef PTX_H
#define PTX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#define PTX_STATIC_ASSERT(c, m) static_assert(c, m)
#else
#define PTX_STATIC_ASSERT(c, m) _Static_assert(c, m)
#endif

#if defined(_WIN32)
#define PTX_API
#else
#define PTX_API __attribute__((visibility("default")))
#endif

/* Bumped whenever a struct of this header changes size or layout or an entry point changes meaning; ptx_abi_version()
 * returns the value the loaded library was built with.  3: PtxSceneDesc.textureMemoryBudget (round 2),
 * PtxStats.hardwareQueues (round 3).  4: PtxStats.treeTriangles / treeReferences (round 4).  5: every `/` of the shader path
 * became a * rcp(b) (round 5: ptx_test_eval and rendered images changed meaning in the last bits) and ptx_unpack_shard_host was
 * added; ptx_unpack_shards, ptx_bind_shard_accumulation; repeat addressing of the sampler takes the exact floor(x) mod n for extents
 * that are not powers of two; normalize() / inversesqrt() go through the specified rsq (PTX_FN_RSQ) instead of rcp(sqrt());
 * PtxDeviceDesc.flags (round 6). */
#define PTX_ABI_VERSION 5u

/* ------------------------------------------------------------------------- */
/* Data contract                                                             */
/* ------------------------------------------------------------------------- */

/* ShaderTypes.incl:18-33 */
enum {
    PTX_DEFAULT_COLOR_TEXTURE_INDEX = 0,
    PTX_DEFAULT_NORMAL_TEXTURE_INDEX = 1,
    PTX_DEFAULT_ROUGHNESS_TEXTURE_INDEX = 2,
    PTX_DEFAULT_METALLIC_TEXTURE_INDEX = 3,
    PTX_DEFAULT_EMISSIVE_TEXTURE_INDEX = 4,
    PTX_DEFAULT_SPECULAR_TEXTURE_INDEX = 5,
    PTX_DEFAULT_GLOSSINESS_TEXTURE_INDEX = 6,
    PTX_DEFAULT_SHININESS_TEXTURE_INDEX = 7,
    PTX_PLACEHOLDER_TEXTURE_INDEX = 8,
    PTX_SCENE_TEXTURE_OFFSET = 9,
    PTX_MAX_TEXTURE_COUNT = 1024,
    PTX_MAX_LIGHT_COUNT = 64
};

/* ShaderTypes.incl:143-145 */
enum {
    PTX_MATERIAL_TYPE_METALLIC_ROUGHNESS = 0,
    PTX_MATERIAL_TYPE_SPECULAR_GLOSSINESS = 1,
    PTX_MATERIAL_TYPE_PHONG = 2
};

/* ShaderTypes.incl:41-48 -- 14 floats, unpadded, read by GLSL as vec2[7] (common.glsl:27-46) */
typedef struct PtxVertex {
    float Position[3];
    float TexCoords[2];
    float Normal[3];
    float Tangent[3];
    float Bitangent[3];
} PtxVertex;
PTX_STATIC_ASSERT(sizeof(PtxVertex) == 56, "Vertex is 56 B");

/* ShaderTypes.incl:61-80 */
typedef struct PtxMetallicRoughnessMaterial {
    float EmissiveColor[3];
    float EmissiveIntensity;
    float Color[4];
    float Roughness;
    float Metalness;
    float Ior;
    float Transmission;
    float AttenuationColor[3];
    float AttenuationDistance;
    float pad0, pad1, pad2;
    uint32_t EmissiveIdx;
    uint32_t ColorIdx;
    uint32_t NormalIdx;
    uint32_t RoughnessIdx;
    uint32_t MetallicIdx;
} PtxMetallicRoughnessMaterial;
PTX_STATIC_ASSERT(sizeof(PtxMetallicRoughnessMaterial) == 96, "MR material is 96 B");

/* ShaderTypes.incl:82-99 */
typedef struct PtxSpecularGlossinessMaterial {
    float EmissiveColor[3];
    float EmissiveIntensity;
    float Color[4];
    float Specular[3];
    float Glossiness;
    float AttenuationColor[3];
    float AttenuationDistance;
    float Ior;
    float Transmission;
    uint32_t EmissiveIdx;
    uint32_t ColorIdx;
    uint32_t NormalIdx;
    uint32_t SpecularIdx;
    uint32_t GlossinessIdx;
    float pad0;
} PtxSpecularGlossinessMaterial;
PTX_STATIC_ASSERT(sizeof(PtxSpecularGlossinessMaterial) == 96, "SG material is 96 B");

/* ShaderTypes.incl:101-118 */
typedef struct PtxPhongMaterial {
    float EmissiveColor[3];
    float EmissiveIntensity;
    float Color[4];
    float Specular[3];
    float Shininess;
    float AttenuationColor[3];
    float AttenuationDistance;
    float Ior;
    float Transmission;
    uint32_t EmissiveIdx;
    uint32_t ColorIdx;
    uint32_t NormalIdx;
    uint32_t SpecularIdx;
    uint32_t ShininessIdx;
    float pad0;
} PtxPhongMaterial;
PTX_STATIC_ASSERT(sizeof(PtxPhongMaterial) == 96, "Phong material is 96 B");

/* ShaderTypes.incl:120-126 */
typedef struct PtxDirectionalLight {
    float Color[3];
    float pad0;
    float Direction[3];
    float pad1;
} PtxDirectionalLight;
PTX_STATIC_ASSERT(sizeof(PtxDirectionalLight) == 32, "DirectionalLight is 32 B");

/* ShaderTypes.incl:128-138 */
typedef struct PtxPointLight {
    float Color[3];
    float pad0;
    float Position[3];
    float pad1;
    float AttenuationConstant;
    float AttenuationLinear;
    float AttenuationQuadratic;
    float pad2;
} PtxPointLight;
PTX_STATIC_ASSERT(sizeof(PtxPointLight) == 48, "PointLight is 48 B");

/* closestHit.rchit:32-36 with the offsets of Renderer.h:152-156:
 * uint count @0, DirectionalLight @16, PointLight[64] @48. */
typedef struct PtxLightsUbo {
    uint32_t LightCount;
    uint32_t pad[3];
    PtxDirectionalLight Directional;
    PtxPointLight Lights[PTX_MAX_LIGHT_COUNT];
} PtxLightsUbo;
PTX_STATIC_ASSERT(sizeof(PtxLightsUbo) == 48 + 64 * 48, "lights UBO is 3120 B");

/* ShaderRendererTypes.incl:26-34 (Camera = ShaderTypes.incl:35-39).  Matrices are
 * glm column-major: element [col*4 + row]. */
typedef struct PtxRaygenUniformData {
    float ViewInverse[16];
    float ProjInverse[16];
    uint32_t BounceCount;
    float LensRadius;
    float FocalDistance;
    uint32_t SampleCount;  /* samples added by this launch                      */
    uint32_t TotalSamples; /* samples accumulated BEFORE this launch = RNG frame */
} PtxRaygenUniformData;
PTX_STATIC_ASSERT(sizeof(PtxRaygenUniformData) == 148, "RaygenUniformData is 148 B");

/* Scene.h:63-71 */
typedef struct PtxGeometry {
    uint32_t VertexOffset;
    uint32_t VertexLength;
    uint32_t IndexOffset;
    uint32_t IndexLength;
    uint8_t IsOpaque;
    uint8_t IsAnimated;
    uint8_t pad[2];
} PtxGeometry;
PTX_STATIC_ASSERT(sizeof(PtxGeometry) == 20, "Geometry is 20 B");

/* ShaderRendererTypes.incl:42-47 (SBTBuffer); one per mesh, in model-then-mesh order
 * (Renderer.cpp:378-399).  Record index = Model.MeshOffset + geometry index inside
 * the model's BLAS (AccelerationStructure.cpp:270-274). */
typedef struct PtxMeshRecord {
    uint32_t GeometryIndex;
    uint32_t MaterialId; /* (index << 8) | type, ShaderTypes.incl:155-168 */
    uint32_t TransformIndex;
} PtxMeshRecord;
PTX_STATIC_ASSERT(sizeof(PtxMeshRecord) == 12, "SBTBuffer is 12 B");

/* glm::mat3x4 as used for Scene::GetTransforms() and VkTransformMatrixKHR
 * (closestHit.rchit:12-14): 3 rows of the affine matrix, 4 floats each. */
typedef struct PtxTransform {
    float m[12];
} PtxTransform;
PTX_STATIC_ASSERT(sizeof(PtxTransform) == 48, "mat3x4 is 48 B");

/* Scene.h:96-100 flattened: the meshes of model i are records
 * [MeshOffset, MeshOffset + MeshCount). */
typedef struct PtxModel {
    uint32_t MeshOffset;
    uint32_t MeshCount;
} PtxModel;

/* Scene.h:102-107; Transform = first 3 rows of the instance's affine matrix
 * (AccelerationStructure.cpp:271). */
typedef struct PtxModelInstance {
    uint32_t ModelIndex;
    PtxTransform Transform;
} PtxModelInstance;

/* Scene textures (row N1).  Texture i of the scene has shader index PTX_SCENE_TEXTURE_OFFSET + i
 * (Scene.cpp:125-141).  8-bit data is RGBA8; the image format follows the texture TYPE as in
 * TextureUploader::GetImageFormat (TextureUploader.cpp:571-594): sRGB for Color / Specular /
 * Emissive / Skybox, UNORM otherwise.  The full mip chain (floor(log2(max(w,h))) + 1 levels,
 * Image.cpp:14-17) is generated level by level with a linear 2:1 blit (Image.cpp:264-300). */
typedef enum PtxTextureFormat {
    PTX_TEXTURE_RGBA8_UNORM = 0,
    PTX_TEXTURE_RGBA8_SRGB = 1,
    PTX_TEXTURE_RGBA32F = 2,
    /* Block-compressed scene textures, uploaded as blocks and decoded on the device (docs/NEXT_ROWS.md section 15).  The format
     * follows TextureUploader::GetImageFormat in full (TextureUploader.cpp:586-591): BC3 is always sRGB, BC5 always UNORM, BC1 is
     * sRGB or UNORM by the texture type.  Skybox images in these formats are refused.
     *
     * Layout of PtxTextureDesc.data: `levels` levels back to back, level 0 first (the order of a DDS file).  Level l has the
     * extent w_l x h_l = max(w >> l, 1) x max(h >> l, 1) and is ceil(w_l / 4) * ceil(h_l / 4) blocks, row-major (block (bx, by)
     * covers the texels 4 bx .. 4 bx + 3, 4 by .. 4 by + 3; texels of a partial block beyond the extent do not exist).  A block is
     * 8 bytes for BC1 and 16 bytes for BC3 / BC5, little-endian.  Texel (x, y) of a block has the number i = 4 (y & 3) + (x & 3).
     *
     * Colour block (8 bytes; all of BC1, bytes 8 .. 15 of BC3): c0 = bytes 0-1 and c1 = bytes 2-3 as 16-bit RGB565 (R in bits
     * 11-15, G in 5-10, B in 0-4), then 32 bits of codes, 2 bits per texel, texel i in bits 2i, 2i + 1 of the dword of bytes 4-7.
     * An end point expands to 8 bits by bit replication: R8 = R5 << 3 | R5 >> 2, G8 = G6 << 2 | G6 >> 4, B8 = B5 << 3 | B5 >> 2.
     * Per channel, with p0 / p1 the expanded end points and integer arithmetic with floor division:
     *   four-colour mode:  code 0: p0, 1: p1, 2: (2 p0 + p1) / 3, 3: (p0 + 2 p1) / 3; alpha 255
     *   three-colour mode: code 0: p0, 1: p1, 2: (p0 + p1) / 2, alpha 255;  code 3: R = G = B = 0 and alpha 0
     * BC1 is the RGBA variant: four-colour mode iff c0 > c1 (compared as 16-bit integers), three-colour mode otherwise.  The colour
     * block of BC3 is always in four-colour mode and its alpha comes from the alpha block.
     * Alpha block (8 bytes, the "BC4" block; bytes 0 .. 7 of BC3, both halves of BC5): a0 = byte 0, a1 = byte 1, then 48 bits of
     * codes, 3 bits per texel, texel i in bits 3i .. 3i + 2 of the little-endian integer of bytes 2-7.  Integer, floor division:
     *   a0 > a1:  code 0: a0, 1: a1, c = 2 .. 7: ((8 - c) a0 + (c - 1) a1) / 7
     *   a0 <= a1: code 0: a0, 1: a1, c = 2 .. 5: ((6 - c) a0 + (c - 1) a1) / 5, 6: 0, 7: 255
     * BC3: RGB from the colour block, A from the alpha block.  BC5: R from bytes 0-7, G from bytes 8-15, B = 0, A = 255.
     * The 8-bit RGBA result becomes four floats exactly as an RGBA8 texel of PTX_TEXTURE_RGBA8_SRGB (the _SRGB formats) or
     * PTX_TEXTURE_RGBA8_UNORM (the _UNORM formats) does: the same blocks decoded by the caller and uploaded as RGBA8 sample the
     * same bits.
     *
     * Upload rules (TextureUploader::UploadTexture for a format that cannot be blitted, TextureUploader.cpp:401-503).  The budget
     * prices a texture in block bytes: the largest square extent whose full chain, sum over its levels of
     * ceil(w_l / 4) ceil(h_l / 4) block bytes, fits textureMemoryBudget / textureCount (BC1 keeps 8x, BC3 / BC5 4x the texels of
     * RGBA8).  Scale and budgeted extent w' x h' as for the other formats.  At scale 1: a full chain is used as it is; levels <= 1
     * gives a ONE-level image at the full extent (no levels are generated); any other count is REJECTED.  At scale > 1: levels <= 1
     * is rejected; otherwise with skip = levels - fullLevels(w', h'), the image is the file's levels from `skip` on iff skip >= 0
     * and file level `skip` has exactly the extent w' x h', and rejected otherwise.  A rejected texture (the reference's
     * m_RejectedCount) does not fail the upload: it is replaced by the 1 x 1 one-level opaque-white RGBA8 texel and reported by
     * ptx_textures_rejected. */
    PTX_TEXTURE_BC1_UNORM = 3,
    PTX_TEXTURE_BC1_SRGB = 4,
    PTX_TEXTURE_BC3_SRGB = 5,
    PTX_TEXTURE_BC5_UNORM = 6
} PtxTextureFormat;

/* ShaderTypes.incl:50-59 (scalar block layout), the input of skinning.comp */
typedef struct PtxAnimatedVertex {
    float Position[3];
    float TexCoords[2];
    float Normal[3];
    float Tangent[3];
    float Bitangent[3];
    uint32_t BoneIndices[4]; /* MaxBonesPerVertex */
    float BoneWeights[4];
} PtxAnimatedVertex;

typedef struct PtxTextureDesc {
    uint32_t width, height;
    uint32_t format;   /* PtxTextureFormat */
    uint32_t levels;   /* TextureInfo::Levels: mip levels in `data` (0 or 1: level 0 only).  A full chain (floor(log2(max(w, h))) + 1
                        * levels) is uploaded as it is; from any other count only level 0 is used and the chain is generated by
                        * linear blits (TextureUploader.cpp:440-456).  Skybox images: level 0 only */
    const void *data;  /* level 0 first, then max(w >> l, 1) x max(h >> l, 1) texels per level, row-major, tightly packed */
} PtxTextureDesc;

enum {
    PTX_SKYBOX_CLEAR_COLOR = 0, /* miss.rmiss:37: constant (0.08, 0.09, 0.10) */
    PTX_SKYBOX_2D = 1,          /* MissFlagsSkybox2D: miss.rmiss:18-30, skybox[0] is the equirectangular image */
    PTX_SKYBOX_CUBE = 2         /* MissFlagsSkyboxCube: miss.rmiss:31-34, skybox[0..5] = +X -X +Y -Y +Z -Z
                                 * (the layer order of TextureUploader.cpp:234-235: Front Back Up Down Left Right) */
};

/* What Renderer::UpdateSceneData pulls through the Scene getters
 * (Scene.h:182-207).  The caller keeps ownership; ptx_scene_upload copies. */
typedef struct PtxSceneDesc {
    const PtxVertex *vertices;
    uint64_t vertexCount;
    const uint32_t *indices; /* relative to the geometry's VertexOffset */
    uint64_t indexCount;
    const PtxTransform *transforms; /* [0] = identity (Scene.h:306,312) */
    uint32_t transformCount;
    const PtxGeometry *geometries;
    uint32_t geometryCount;
    const PtxMetallicRoughnessMaterial *metallicRoughnessMaterials;
    uint32_t metallicRoughnessMaterialCount;
    const PtxSpecularGlossinessMaterial *specularGlossinessMaterials;
    uint32_t specularGlossinessMaterialCount;
    const PtxPhongMaterial *phongMaterials;
    uint32_t phongMaterialCount;
    const PtxMeshRecord *meshes;
    uint32_t meshCount;
    const PtxModel *models;
    uint32_t modelCount;
    const PtxModelInstance *instances;
    uint32_t instanceCount;
    uint32_t skyboxKind;       /* PTX_SKYBOX_*; PathTracingPipelineConfig.MissFlags */
    uint32_t dxNormalTextures; /* HitFlagsDxNormalTextures, ShaderRendererTypes.incl:96-99 */
    const PtxTextureDesc *textures; /* Scene::GetTextures(); may be NULL: indices >= 9 then sample the white placeholder */
    uint32_t textureCount;
    uint32_t forceFullTextureSize; /* Scene::GetForceFullTextureSize(): TextureUploader::DetermineMaxTextureSizes never halves
                                    * (TextureUploader.cpp:551-569): every texture keeps its size up to 4096 x 4096 */
    const PtxTextureDesc *skybox; /* Scene::GetSkybox(): 1 (2D) or 6 (cube, equal square faces) images, one level each
                                   * (TextureUploader.cpp:203-262); ignored for PTX_SKYBOX_CLEAR_COLOR */
    /* Scene::GetAnimatedVertices() / GetAnimatedIndices(): geometries with IsAnimated index THESE arrays
     * (Renderer.cpp:262-265, :280-312).  Every instanced animated mesh gets its own skinned copy, in bind pose
     * until the first ptx_update_animation. */
    const PtxAnimatedVertex *animatedVertices;
    uint64_t animatedVertexCount;
    const uint32_t *animatedIndices;
    uint64_t animatedIndexCount;
    /* Config MaxTextureMemoryBudgetAbsolute / ...VramPercent (Config.h:63-64,162-163; TextureUploader.cpp:29-37): bytes the scene
     * textures may take together.  Each gets budget / textureCount; a larger one is scaled down by an integer factor on upload
     * (TextureUploader.cpp:409-415,479-501).  0 = the reference's default, min(80 % of the device memory, 1 GiB);
     * ~0 = no limit.  Ignored with forceFullTextureSize.
     * The budget prices the texels in the IMAGE format, as the reference does (4 B per texel for the 8-bit formats); what this
     * library keeps resident is every level decoded to four floats (16 B per texel) plus, for the colour textures of non-opaque
     * geometry, one more float4 per base-level texel (the alpha footprints of the any-hit stages): about 4x the budgeted bytes
     * for 8-bit textures, and about 5x at the peak of the upload, while the encoded pools and the decoded pool coexist.  A host
     * that passes its whole VRAM share here leaves too little for that; the default (at most 1 GiB) does not come near it. */
    uint64_t textureMemoryBudget;
} PtxSceneDesc;

/* ------------------------------------------------------------------------- */
/* Renderer                                                                  */
/* ------------------------------------------------------------------------- */

typedef enum PtxStatus {
    PTX_OK = 0,
    PTX_ERROR_INVALID_ARGUMENT = 1,
    PTX_ERROR_NO_DEVICE = 2,
    PTX_ERROR_OUT_OF_MEMORY = 3,
    PTX_ERROR_DEVICE = 4,
    PTX_ERROR_NOT_READY = 5
} PtxStatus;

typedef enum PtxBackend {
    PTX_BACKEND_WAVEFRONT = 0,  /* queue-per-stage kernels (production path)            */
    PTX_BACKEND_MEGAKERNEL = 1  /* one thread per pixel running raygen.rgen's loop 1:1  */
} PtxBackend;

enum {
    /* ONE stream per handle: the shadow and tail kernels of a frame ride on its main stream instead of an auxiliary one -- no overlap
     * inside a frame, but a frame in flight then takes one hardware queue, not two, and twice as many frames fit the queues.  Pays
     * for THIN frames (a rank's tile shard of an N-GPU job: 16 single-stream frames in flight against 8 two-stream ones, a 1 / 8
     * shard step of chess_like 1.05 -> 0.95 ms, the heavier stand-ins -1 ... -4 %); a whole frame on one GPU does better with two
     * streams (profiles/r06_single_stream*.txt). */
    PTX_DEVICE_SINGLE_STREAM = 1u
};

typedef struct PtxDeviceDesc {
    int32_t deviceIndex;  /* HIP device ordinal                                        */
    uint32_t backend;     /* PtxBackend                                                */
    void *stream;         /* hipStream_t to launch on, or NULL for an internal stream  */
    uint32_t flags;       /* PTX_DEVICE_*                                              */
    uint32_t reserved;    /* 0                                                         */
} PtxDeviceDesc;

/* Pixel-tile shard of a frame: the image is cut into tileSize x tileSize
 * tiles, numbered row-major; this renderer owns tiles with (tile % worldSize) == rank.
 * rank 0 / worldSize 1 = whole frame. */
typedef struct PtxTileShard {
    uint32_t rank;
    uint32_t worldSize;
    uint32_t tileSize;
} PtxTileShard;

/* Counters of the last ptx_render() (all deterministic given the RNG schedule). */
typedef struct PtxStats {
    uint64_t pathSamples;    /* pixel-samples completed (incl. NaN/Inf retries)     */
    uint64_t segments;       /* closest-hit queries traced                          */
    uint64_t shadowRays;     /* occlusion queries traced                            */
    uint64_t retries;        /* NaN/Inf sample restarts (raygen.rgen:99-112)        */
    uint64_t triangles;      /* flattened world-space triangles in the LBVH         */
    uint64_t bvhNodes;       /* nodes of the 4-wide tree (reachable from the root)  */
    double lastRenderMs;     /* device time of the last ptx_render (HIP events)     */
    double lastTraceMs;      /* ... spent in k_trace_closest (HIP events on the stream) */
    double lastBuildMs;      /* device time of the last ptx_build_accel (every candidate tree it built) */
    uint64_t traceLaunches;  /* number of traversal kernel launches in last render  */
    double lastShadeMs;      /* ... spent in k_shade                                */
    double lastShadowMs;     /* ... spent in k_trace_shadow                         */
    double lastTailMs;       /* ... spent in k_tail (fused late bounces)            */
    uint64_t tracedRays;     /* closest-hit queries carried by the k_trace_closest launches timed in lastTraceMs
                                (segments also counts the ones k_tail traces itself) */
    uint64_t hardwareQueues; /* hardware queues the environment grants the process's HIP streams (GPU_MAX_HW_QUEUES when
                                the handle was created, 4 = the runtime's default when unset): below two per handle the
                                frames in flight run one after the other */
    uint64_t treeTriangles;  /* triangles in the tree: `triangles` minus the zero-area ones, which no ray can hit (a full
                                build leaves them out; bvhNodes is no measure of this -- the collapse into 4-wide nodes is
                                driven by the boxes' areas, so fewer triangles can make more nodes) */
    uint64_t treeReferences; /* leaves of the tree: treeTriangles plus the extra references of triangles that were split before
                                the build (a large triangle may hang from several leaves, each with a tighter box) */
} PtxStats;

typedef struct PtxRenderer PtxRenderer;

/* Renderer::Init / Renderer::Shutdown (Renderer.cpp:77-218).  One handle = one frame in flight (the reference's per-frame
 * rendering resources, Renderer.cpp:1454-1460): two HIP streams each while the streams of every live handle fit the hardware
 * queues of the process, one otherwise.  The HIP runtime maps a process's streams onto GPU_MAX_HW_QUEUES hardware queues (4 by
 * default), and streams that share a queue run one after the other: a host that keeps several handles exports
 * GPU_MAX_HW_QUEUES=16 before its first HIP call.  The library does not touch the environment; it reports what
 * it finds (PtxStats::hardwareQueues), every launch takes the schedule that fits it (PTX_STREAM_PLAN=0: always two streams), and
 * the first handle whose streams no longer fit leaves a note that names its schedule in ptx_last_error although ptx_create
 * returned PTX_OK.  Images and statistics do not depend on the schedule. */
PTX_API int ptx_create(const PtxDeviceDesc *desc, PtxRenderer **out);
PTX_API void ptx_destroy(PtxRenderer *r);
PTX_API const char *ptx_last_error(const PtxRenderer *r);
PTX_API int ptx_device_count(void);
/* PTX_ABI_VERSION of the library that was loaded: the structs of this header carry no size fields, so a binding compares
 * this with the header it was written against before the first call (the Python package and RendererHip do). */
PTX_API uint32_t ptx_abi_version(void);

/* Renderer::UpdateSceneData (Renderer.cpp:238-439): copy the scene to HBM.  A description that is refused with
 * PTX_ERROR_INVALID_ARGUMENT, for whatever reason, leaves the handle as it was: its own scene, or the one it borrows. */
PTX_API int ptx_scene_upload(PtxRenderer *r, const PtxSceneDesc *scene);
/* The same upload without waiting for the textures (Renderer.cpp:419-438: every scene texture is first mapped to a stand-in, then
 * TextureUploader::UploadTextures fills them in).  A scene texture with data == NULL is PENDING instead of reading as zeros: its
 * width / height / format / levels are binding -- the plan places it exactly as if the texels were there, budget rule included --
 * and until it is committed it samples as the fixed 1 x 1 texture standIn[i], one of the nine indices below
 * PTX_SCENE_TEXTURE_OFFSET (the caller passes what Renderer.cpp:426-428 computes: the placeholder for Color, the type's default
 * otherwise); standIn == NULL: the placeholder for all.  Textures that carry data are uploaded at once, and so are the skybox
 * images (UploadSkyboxBlocking, Renderer.cpp:408-411).  A scene with a pending texture renders with the sampling kernels from
 * the start; that never changes afterwards.  Refusals (a stand-in index above 8 among them) leave the handle as it was. */
PTX_API int ptx_scene_upload_streamed(PtxRenderer *r, const PtxSceneDesc *scene, const uint32_t *standIn);
/* TextureUploader's submit step for one texture (TextureUploader.cpp:312-360).  `index` is the scene texture's index (0-based,
 * not the shader index); `desc` repeats the width / height / format / levels declared at upload and carries `data`.  The texels
 * are copied into page-locked staging of the library before the call returns; the copy to the device, the scaled-down path,
 * the mip chain, the decode into the pool the render kernels sample and, for a colour texture of non-opaque geometry, its alpha
 * footprints are enqueued on an upload stream of their own (created by the first call; it takes a hardware queue,
 * INTEGRATION.md).  The call does not wait for frames in flight and changes nothing a frame sees; it waits only when both
 * staging slots still hold an upload in flight (the reference's free-buffer semaphore).  PTX_ERROR_INVALID_ARGUMENT: index out
 * of range, a descriptor that differs from the declared one, NULL data, a texture that is not pending, a scene that was not
 * uploaded by ptx_scene_upload_streamed, a handle that borrows its scene (uploads are the owner's calls).  Replacing a resident
 * texture is not supported. */
PTX_API int ptx_texture_upload(PtxRenderer *r, uint32_t index, const PtxTextureDesc *desc);
/* Renderer::UpdateTexture (Renderer.cpp:441-471) for every texture uploaded since the last commit: from the ptx_render* /
 * ptx_trace_rays / ptx_test_texture calls that follow, on this handle and on its borrowers, these textures sample as a blocking
 * ptx_scene_upload of the same description would have made them; nothing enqueued earlier changes.  Which of the two a frame
 * sees is fixed by the order of the calls, never by timing.  The render stream waits for the upload stream on the device (an
 * event); the host waits only for the borrowers' frames in flight, as ptx_build_accel does.  With a tree built, the any-hit
 * records of its triangles are rewritten (an alpha texture's extent and footprints are part of them); before ptx_build_accel the
 * commit only switches the tables and the build picks them up.  *committed (may be NULL): textures switched by this call; nothing
 * to commit is PTX_OK with 0.  The accumulation is not reset: as in the reference, that is the caller's decision. */
PTX_API int ptx_textures_commit(PtxRenderer *r, uint32_t *committed);
/* Counts over the scene's textures (of the owner's scene on a borrower): resident = uploaded with the scene or committed,
 * pending = everything else.  After a plain ptx_scene_upload every texture is resident. */
PTX_API int ptx_texture_residency(PtxRenderer *r, uint32_t *resident, uint32_t *pending);
/* TextureUploader's m_RejectedCount: the block-compressed scene textures the last ptx_scene_upload / ptx_scene_upload_streamed
 * on this handle (on the owner, for a borrower) could not take by the upload rules of PtxTextureFormat and replaced by the white
 * texel.  Returns their count and writes the first min(count, capacity) scene texture indices, ascending, into `indices` (may be
 * NULL with capacity 0).  0 for a scene without block-compressed textures, without a scene, and for a NULL handle.  In a
 * streamed upload a rejected texture is resident at once, never pending, and ptx_texture_upload for it is refused with
 * PTX_ERROR_INVALID_ARGUMENT. */
PTX_API uint32_t ptx_textures_rejected(PtxRenderer *r, uint32_t *indices, uint32_t capacity);
/* AccelerationStructure::Build (AccelerationStructure.cpp:26-46; BLAS :64-247, TLAS
 * :250-301), replaced by a software LBVH over the flattened world-space triangles.
 * The reference asks its driver for ePreferFastTrace (AccelerationStructure.cpp:319-324); this build spends time the same way:
 * seven candidate trees (clustering radius, merge metric, Morton cells), each re-optimised by two passes of parallel reinsertion
 * and collapsed to 4-wide nodes by a cost-driven rule, are priced on a sample of path-like rays (node visits + triangle tests), and
 * the cheapest is built once more with 32 reinsertion passes.  Results never depend on the tree; its quality moves frame times by
 * several per cent, and no one setting is best for every scene.  PtxStats::lastBuildMs is the time of all of it (2 M triangles:
 * ~0.8 s, 4 M: ~1.7 s; PTX_REINSERT=0 in the environment: 0.14 / 0.27 s).  PTX_PLOC_RADIUS / PTX_PLOC_SHAPE build one tree with
 * those parameters instead; the per-frame rebuilds of ptx_update_animation use the parameters chosen here with two reinsertion
 * passes. */
PTX_API int ptx_build_accel(PtxRenderer *r);
/* Frames in flight share ONE scene: the reference keeps GetInFlightCount() sets of per-frame rendering resources
 * (Renderer.cpp:1454-1460) over one set of scene buffers and one acceleration structure (s_StaticSceneData / s_SceneData,
 * Renderer.cpp:238-439).  `r` from now on renders the scene and the tree of `owner` (same device, uploaded and built)
 * instead of holding copies; its own scene, if any, is released.  Lights, camera, image, path state stay per renderer.
 * The borrowing ends with ptx_scene_upload on `r`, or when either renderer is destroyed (a borrower whose owner is gone
 * reports PTX_ERROR_NOT_READY).  ptx_build_accel / ptx_update_animation are the owner's calls; they, and a new
 * ptx_scene_upload on the owner, first wait for the borrowers' frames in flight.  Not thread-safe across the two
 * renderers, like the rest of the interface (the reference's Renderer is driven from one thread). */
PTX_API int ptx_share_scene(PtxRenderer *r, PtxRenderer *owner);

/* Renderer::OnResize / CreateSceneRenderingResources: (re)allocate the RGBA32F
 * accumulation image (Renderer.cpp:1284-1287) and the wavefront path state. */
PTX_API int ptx_resize(PtxRenderer *r, uint32_t width, uint32_t height);
PTX_API int ptx_set_tile_shard(PtxRenderer *r, const PtxTileShard *shard);
PTX_API int ptx_set_backend(PtxRenderer *r, uint32_t backend);

/* Renderer::ResetAccumulationImage (Renderer.cpp:801-808, clear at :1734-1748). */
PTX_API int ptx_reset_accumulation(PtxRenderer *r);

/* Renderer::Render's uniform fill + RecordPathTracingCommands (Renderer.cpp:1686-1726,
 * 892-926): adds uniform->SampleCount samples per owned pixel, RNG frame =
 * uniform->TotalSamples, into the accumulation image.  Asynchronous on the stream. */
PTX_API int ptx_render(PtxRenderer *r, const PtxRaygenUniformData *uniform, const PtxLightsUbo *lights);
/* Convenience for the canonical schedule: `frames` launches with
 * SampleCount = 1 and TotalSamples = firstFrame .. firstFrame+frames-1, issued as ONE
 * wavefront batch; the result is bit-identical to `frames` ptx_render calls. */
PTX_API int ptx_render_frames(PtxRenderer *r, const PtxRaygenUniformData *uniform, const PtxLightsUbo *lights,
                              uint32_t firstFrame, uint32_t frames);

PTX_API int ptx_synchronize(PtxRenderer *r);
/* imageLoad of the accumulation image: device -> host, W*H*4 floats (running SUM). */
PTX_API int ptx_readback(PtxRenderer *r, float *rgba, size_t bytes);
/* The same read-back, overlapped with whatever is launched next: _begin snapshots the image on the render stream and
 * starts the copy into `pinnedHost` (page-locked memory, width*height*16 bytes) on the renderer's auxiliary stream -- a
 * one-workgroup copy kernel when the device can address the buffer (hipHostMalloc / hipHostRegister memory; gentle on the
 * PCIe link the other frames' dispatches share), the runtime's copy otherwise; _end waits for it.
 * A second _begin before _end queues behind the first.  (OutputSaver reads its output back a frame late in the same
 * way, OutputSaver.cpp:120-199.) */
PTX_API int ptx_readback_begin(PtxRenderer *r, float *pinnedHost, size_t bytes);
PTX_API int ptx_readback_end(PtxRenderer *r);
/* Device pointer of the accumulation image (for the RCCL gather) and its size. */
PTX_API void *ptx_device_accum_ptr(PtxRenderer *r);
PTX_API size_t ptx_accum_bytes(const PtxRenderer *r);
/* Pack / unpack this shard's tiles to/from a dense tile-major buffer of
 * ptx_shard_bytes() bytes (the message of the single gather). */
PTX_API size_t ptx_shard_bytes(const PtxRenderer *r, uint32_t rank);
PTX_API int ptx_pack_shard(PtxRenderer *r, void *devDst);
PTX_API int ptx_unpack_shard(PtxRenderer *r, uint32_t rank, const void *devSrc);
/* The same, and the shard's pixels also go straight into `pinnedHost` (page-locked, device-addressable, width*height*16 bytes):
 * the rank that owns the gathered frame hands it to the host while it unpacks it -- no snapshot and no second pass over the image,
 * which is what bounds a step once the ranks render faster than the PCIe link reads back.  Asynchronous on
 * the render stream; the buffer is complete once every rank's shard has been unpacked into it and ptx_readback_end() has returned
 * (it waits for the last such call). */
PTX_API int ptx_unpack_shard_host(PtxRenderer *r, uint32_t rank, const void *devSrc, float *pinnedHost, size_t bytes);
/* The whole gathered frame in ONE launch: `devSrc` holds the shards of ranks 0 .. worldSize-1 (ptx_pack_shard's layout each),
 * `strideBytes` apart (a multiple of 16, at least the largest ptx_shard_bytes) -- the receive buffer of the gather as it is.
 * Targets: this renderer's device image (toDeviceImage != 0), the host's page-locked frame (pinnedHost != NULL, width*height*16
 * bytes; complete after ptx_readback_end), or both.  A rank that only hands the frame to the host -- OutputSaver's role
 * (OutputSaver.cpp:120-199) -- passes toDeviceImage = 0 and never rewrites its device image.  One thread per pixel in row-major
 * order: the stores are one contiguous stream over the frame.  Because the RNG is a pure function of (pixel, width, frame)
 * (common.glsl:143-147) ANY rank may own any frame: a job rotates the owner over the ranks with its frames in flight
 * (bench.py), so that no rank carries the read-back of every step. */
PTX_API int ptx_unpack_shards(PtxRenderer *r, const void *devSrc, size_t strideBytes, int toDeviceImage, float *pinnedHost, size_t bytes);
/* Accumulate the samples of this renderer's tile shard IN `devShard` (at least ptx_shard_bytes(r, own rank) bytes of device memory,
 * e.g. the send buffer of the gather) in ptx_pack_shard's layout, instead of in the row-major accumulation image:
 * raygen.rgen:115-117's imageLoad / imageStore go to entry = slot inside the frame.  ptx_reset_accumulation clears it,
 * ptx_pack_shard becomes a no-op (or a device copy if asked for another buffer); the calls that need the row-major frame
 * (ptx_readback*, ptx_postprocess, ptx_write_accumulation) return PTX_ERROR_NOT_READY until NULL is bound again.  ptx_resize and a
 * ptx_set_tile_shard that changes the shard unbind it. */
PTX_API int ptx_bind_shard_accumulation(PtxRenderer *r, void *devShard, size_t bytes);

PTX_API int ptx_get_stats(PtxRenderer *r, PtxStats *stats);

/* ------------------------------------------------------------------------- */
/* Animation (row N3)                                                        */
/* ------------------------------------------------------------------------- */

typedef enum PtxAccelUpdate {
    PTX_ACCEL_REFIT = 0,   /* keep the tree topology of the last full build: new triangle positions, boxes refitted bottom-up
                            * (the reference's BLAS update + TLAS rebuild, AccelerationStructure.cpp:48-57) */
    PTX_ACCEL_REBUILD = 1  /* full LBVH build */
} PtxAccelUpdate;

/* What Renderer::Render does when Scene::Update reported a change (Renderer.cpp:1750-1754, :854-890):
 * new ModelInstance transforms (instanceCount must match the uploaded scene; NULL = unchanged), new bone
 * matrices for skinning.comp (Scene::GetBoneTransforms(): boneCount x mat3x4; NULL = unchanged), the skinning
 * pass over every animated mesh, then the acceleration-structure update.  Results never depend on the tree:
 * a refit and a rebuild render identical images. */
PTX_API int ptx_update_animation(PtxRenderer *r, const PtxTransform *instanceTransforms, uint32_t instanceCount,
                                 const PtxTransform *boneTransforms, uint32_t boneCount, uint32_t accelUpdate);

/* ------------------------------------------------------------------------- */
/* Output stage (row N4): what turns the running sum into a displayable image */
/* ------------------------------------------------------------------------- */

/* ShaderRendererTypes.incl:81-87 (uniform of postprocess.comp / composition.comp) */
typedef struct PtxPostProcessingUniformData {
    uint32_t TotalSamples;
    float Exposure;
    float BloomThreshold;
    float BloomIntensity;
} PtxPostProcessingUniformData;

typedef enum PtxToneMappingMode {
    PTX_TONE_MAPPING_SDR = 0, /* ToneMappingModeSDR: 1 - exp(-c), toneMapping.comp:22 */
    PTX_TONE_MAPPING_HDR = 1  /* ToneMappingModeHDR: pass through                      */
} PtxToneMappingMode;

typedef enum PtxOutputFormat {
    PTX_OUTPUT_RGBA8_SRGB = 0, /* OutputSaver::SelectImageFormat: Png / Jpg / Tga / Mp4 -> eR8G8B8A8Srgb */
    PTX_OUTPUT_RGBA32F = 1     /* Hdr -> eR32G32B32A32Sfloat                                            */
} PtxOutputFormat;

/* Renderer::RecordPostProcessCommands (Renderer.cpp:928-1085) followed by RecordSaveOutputCommands
 * (:1204-1246) on the accumulation image: postprocess.comp (sum / TotalSamples * Exposure, NaN / Inf
 * markers, bloom prefilter) -> bloomDownsample.comp / bloomUpsample.comp over min(levels - 3, 12) mips
 * -> composition.comp -> toneMapping.comp.  Every intermediate image of the reference is rgba16f and so
 * is every intermediate value here.  Images whose larger side is below 16 pixels skip the bloom chain.
 * The result stays on the device until ptx_read_output. */
PTX_API int ptx_postprocess(PtxRenderer *r, const PtxPostProcessingUniformData *uniform, uint32_t toneMappingMode);
/* OutputSaver's blit of the tone-mapped image into its sRGB8 / RGBA32F output image + readback
 * (OutputSaver.cpp:64-86, :120-199): W*H*4 bytes or W*H*16 bytes, row-major, top row first. */
PTX_API int ptx_read_output(PtxRenderer *r, uint32_t outputFormat, void *host, size_t bytes);
/* Restores the accumulation image from a host copy of the running sum (checkpoint / resume). */
PTX_API int ptx_write_accumulation(PtxRenderer *r, const float *rgba, size_t bytes);

/* Use caller-owned device memory (width*height*16 bytes, e.g. a torch tensor that takes
 * part in the RCCL gather) as the accumulation image; NULL returns to the internal one. */
PTX_API int ptx_bind_accumulation(PtxRenderer *r, void *devPtr, size_t bytes);

/* traceRayEXT stand-in on explicit rays, 8 floats each (ox,oy,oz,tmin, dx,dy,dz,tmax):
 * closest hit (anyHit = 0, gl_RayFlagsNoneEXT, raygen.rgen:68) or occlusion (anyHit = 1,
 * TerminateOnFirstHit, raygen.rgen:31).  hits: 4 floats per ray (t, u, v, hit ? 1 : 0);
 * ids: 2 uints per ray ((instance,mesh) pair index, primitive index; 0xffffffff = miss).
 * A ray whose walk needs more traversal-stack entries than the stack holds fails the call
 * with PTX_ERROR_DEVICE (as ptx_render does) instead of returning its hit.
 * Diagnostic modes (closest hit, one thread per ray, no overflow check; hits as above):
 *   anyHit = 2: ids = (node visits, triangle tests)
 *   anyHit = 3: ids = (deepest traversal-stack position, node visits); the position counts
 *               on past the stack's capacity, so a value above it means the walk overflowed. */
PTX_API int ptx_trace_rays(PtxRenderer *r, const float *rays, uint32_t n, int anyHit, float *hits, uint32_t *ids);

/* ------------------------------------------------------------------------- */
/* Function-level entry (mirrors Path-Tracing-Tests/TestRenderer.cpp:79-105:   */
/* run one production shading function over n packed inputs on the device).    */
/* ------------------------------------------------------------------------- */
typedef enum PtxTestFunction {
    /* ShadingTestShaderTypes.incl:19-27 */
    PTX_FN_GGX_DISTRIBUTION = 0,    /* in: H.xyz, alpha            out: result                  */
    PTX_FN_LAMBDA = 1,              /* in: V.xyz, alpha            out: result                  */
    PTX_FN_GGX_SMITH = 2,           /* in: V.xyz, alpha            out: result                  */
    PTX_FN_DIELECTRIC_FRESNEL = 3,  /* in: VdotH, eta              out: result                  */
    PTX_FN_SCHLICK_FRESNEL = 4,     /* in: VdotH                   out: result                  */
    PTX_FN_EVALUATE_REFLECTION = 5, /* in: V, L, F, alpha (10)     out: result.xyz, pdf         */
    PTX_FN_EVALUATE_REFRACTION = 6, /* in: V, L, F, alpha, eta(11) out: result.xyz, pdf         */
    PTX_FN_SAMPLE_GGX = 7,          /* in: u.xy, V.xyz, alpha      out: result.xyz              */
    /* BsdfTestShaderTypes.incl:13 */
    PTX_FN_SAMPLE_LOBE_PDFS = 8,    /* in: metalness, transmission, F   out: 4 lobe weights     */
    /* additional coverage of bsdf.glsl / common.glsl / sampling.glsl / ray.glsl */
    PTX_FN_EVALUATE_BSDF = 9,       /* in: material(8) V L (14)    out: bsdf.xyz, pdf           */
    PTX_FN_SAMPLE_BSDF = 10,        /* in: material(8) V rng (12)  out: dir.xyz pdf color.xyz rng (8) */
    PTX_FN_RNG = 11,                /* in: px py w frame (as u32)  out: state0, 4 draws (5)     */
    PTX_FN_DISK = 12,               /* in: u.xy                    out: d.xy                    */
    PTX_FN_COS_HEMISPHERE = 13,     /* in: u.xy                    out: d.xyz                   */
    PTX_FN_TANGENT_SPACE = 14,      /* in: n.xyz                   out: 9 (columns T,B,N)       */
    PTX_FN_OFFSET_SELF_INTERSECTION = 15, /* in: origin.xyz normal.xyz  out: p.xyz              */
    PTX_FN_PRIMARY_RAY = 16,        /* in: px py w h u.xy + 32 matrix floats (38)  out: o d rx.o rx.d ry.o ry.d (18) */
    PTX_FN_SINCOS = 17,             /* in: x                       out: sin, cos                */
    PTX_FN_POW = 18,                /* in: x, y                    out: pow(x, y)               */
    PTX_FN_SAMPLE_LIGHT = 19,       /* in: u.xyz pos.xyz count(u32) dirColor dirDir 2x(color pos att) (31)
                                       out: dir.xyz dist color.xyz atten pdf (9)                 */
    PTX_FN_SHADOW_TERMINATOR = 20,  /* in: P, (P,N)x3, bary.xyz, isRefracted (25)  out: origin.xyz */
    PTX_FN_PRIMARY_RAY_LENS = 21,   /* in: px py w h u.xy u2.xy lensRadius focalDistance + 32 (42) out: as 16 (18) */
    /* tracing.glsl (ray differentials -> texture footprint) */
    PTX_FN_DPN_DUV = 22,            /* in: (P,N,uv)x3 (24), vertex T,B (6) = 30   out: dpdu dpdv dndu dndv (12)  */
    PTX_FN_DP_DXY = 23,             /* in: p o d rxO rxD ryO ryD n (24)           out: dpdx dpdy (6)             */
    PTX_FN_DERIVATIVES = 24,        /* in: dpdx dpdy dpdu dpdv (12)               out: dudx dvdx dudy dvdy (4)   */
    PTX_FN_REFLECTED_DIFFERENTIALS = 25, /* in: deriv(4) n p wo wi dndu dndv rxO rxD ryO ryD (34)  out: rxO rxD ryO ryD (12) */
    PTX_FN_REFRACTED_DIFFERENTIALS = 26, /* in: same + eta (35)                   out: rxO rxD ryO ryD (12)      */
    PTX_FN_COMPUTE_LOD = 27,        /* in: derivatives (4)                        out: lod                       */
    PTX_FN_SKYBOX_TEXCOORDS = 28,   /* in: ray direction (3)                      out: uv (2)   miss.rmiss:20-25 */
    PTX_FN_HDR_TO_LDR = 29,         /* in: rgb (3)                                out: rgb (3)  common.glsl:17-20 */
    PTX_FN_ATAN_ASIN = 30,          /* in: y x (2)                                out: atan(y,x) asin(y) kernels */
    PTX_FN_POSTPROCESS_PIXEL = 31,  /* in: acc.rgb TotalSamples(bits) Exposure BloomThreshold (6) out: color bloom (6) postprocess.comp:22-37 */
    PTX_FN_COMPOSITION_PIXEL = 32,  /* in: post.rgb bloom.rgb BloomIntensity (7)    out: rgb (3)  composition.comp:23 */
    PTX_FN_TONEMAP_PIXEL = 33,      /* in: rgb (3)                                  out: rgb (3)  toneMapping.comp:20-22, SDR */
    PTX_FN_SAMPLE_MATERIAL = 34,    /* material.glsl:62-171 on explicit texels.  in (47): type, isHitFromInside, flipNormalY (u32 bits), the 96-byte
                                       material record of that type (24 dwords; its texture indices are ignored), the five textureGrad
                                       results in slot order (emissive, colour, normal, 4th, 5th; rgba each)
                                       out (17): EmissiveColor Color Normal Roughness Metalness Transmission Eta AttenuationColor AttenuationDistance */
    PTX_FN_DIVIDE = 35,             /* in: a, b (2)   out: rcp(b), a / b (2) -- the specified division every `/` of the shader path goes
                                       through: a * rcp(b), rcp correctly rounded on [2^-126, 2^126], +-inf below, +-0 above */
    PTX_FN_SQRT = 36,               /* in: x          out: sqrt(x), correctly rounded                                          */
    PTX_FN_RSQ = 37,                /* in: x          out: rsq(x) -- the specified reciprocal square root of normalize() and inversesqrt():
                                       RN(1 / sqrt(x)) for positive normal x, +-inf for +-0 / denormals, +0 for +inf, NaN otherwise  */
    PTX_FN_COUNT = 38
} PtxTestFunction;

/* Material block used by PTX_FN_EVALUATE_BSDF / PTX_FN_SAMPLE_BSDF:
 * color.rgb, roughness, metalness, transmission, eta (7 floats + 1 pad). */

/* textureGrad (implicitLod = 0; material.glsl:72-76) or texture() at LOD 0 (implicitLod = 1, the
 * any-hit shaders: anyhit.rahit:48) of the uploaded scene's textures.  in: 7 floats per sample
 * (texture index as uint bits, u, v, dudx, dvdx, dudy, dvdy); out: rgba. */
PTX_API int ptx_test_texture(PtxRenderer *r, const float *in, float *out, uint32_t n, int implicitLod);

/* ------------------------------------------------------------------------- */
/* Debug view (row D16): the debug ray-tracing pipeline, Shaders/Debug and   */
/* Renderer::SetDebugRaytracingPipeline (Renderer.cpp:579-610, 769-772)      */
/* ------------------------------------------------------------------------- */

/* DebugShaderTypes.incl:18-26 (s_RenderMode) */
enum {
    PTX_DEBUG_MODE_COLOR = 0,          /* rasteriser-style direct light with shadow rays, debugClosestHit.rchit:204-243 */
    PTX_DEBUG_MODE_WORLD_POSITION = 1,
    PTX_DEBUG_MODE_NORMAL = 2,         /* the shading normal, normal map applied */
    PTX_DEBUG_MODE_TEXTURE_COORDS = 3,
    PTX_DEBUG_MODE_MIPS = 4,           /* 0.1 * computeLod(derivatives) + 1 */
    PTX_DEBUG_MODE_GEOMETRY = 5,       /* getRandomColor(gl_GeometryIndexEXT): the mesh's index inside its model */
    PTX_DEBUG_MODE_PRIMITIVE = 6,      /* getRandomColor(gl_PrimitiveID) */
    PTX_DEBUG_MODE_INSTANCE = 7        /* getRandomColor(gl_InstanceID): the index of the PtxModelInstance */
};
/* DebugShaderTypes.incl:28-31 (s_RaygenFlags) */
enum {
    PTX_DEBUG_RAYGEN_FORCE_OPAQUE = 1u,    /* gl_RayFlagsOpaqueEXT on the primary ray: no any-hit stage, no decal */
    PTX_DEBUG_RAYGEN_CULL_BACK_FACES = 2u  /* gl_RayFlagsCullBackFacingTrianglesEXT on the primary ray; facing is decided in the
                                            * space of the model's acceleration structure: a mirrored instance keeps its winding */
};
/* DebugShaderTypes.incl:33-39 (s_HitGroupFlags).  HitGroupFlagsDxNormalTextures is not the caller's: it follows
 * PtxSceneDesc.dxNormalTextures of the uploaded scene, as Renderer.cpp:699-708 sets it. */
enum {
    PTX_DEBUG_HIT_DISABLE_COLOR_TEXTURE = 1u,  /* the colour slot reads PTX_DEFAULT_COLOR_TEXTURE_INDEX (material.glsl:69-70) */
    PTX_DEBUG_HIT_DISABLE_NORMAL_TEXTURE = 2u, /* the normal slot reads PTX_DEFAULT_NORMAL_TEXTURE_INDEX */
    PTX_DEBUG_HIT_DISABLE_MIP_MAPS = 4u,       /* derivatives = vec4(0) */
    PTX_DEBUG_HIT_DISABLE_SHADOWS = 8u         /* every light is added without its shadow ray */
};
typedef struct PtxDebugViewDesc {
    uint32_t renderMode;    /* PTX_DEBUG_MODE_* */
    uint32_t raygenFlags;   /* PTX_DEBUG_RAYGEN_* */
    uint32_t hitGroupFlags; /* PTX_DEBUG_HIT_* */
    uint32_t reserved;      /* 0 */
} PtxDebugViewDesc;

/* RecordPathTracingCommands with the debug pipeline bound (debugRaygen.rgen:22-40): one primary ray through the centre of every
 * owned pixel of the current tile shard, no RNG and no lens (LensRadius, FocalDistance, BounceCount, SampleCount and TotalSamples
 * of the uniform are ignored), and the result is STORED, not added: image[pixel] = payload.Color, alpha included; no other pixel
 * is touched.  Asynchronous on the render stream, like ptx_render; works on a borrower of a shared scene and on a scene with
 * pending streamed textures (they sample their stand-ins).  PTX_ERROR_INVALID_ARGUMENT: a mode above 7, unknown flag bits,
 * reserved != 0, LightCount above PTX_MAX_LIGHT_COUNT; PTX_ERROR_NOT_READY: no scene, tree or image, or a shard accumulation buffer
 * is bound.  ptx_get_stats afterwards: pathSamples = owned pixels, segments = primary rays, shadowRays = occlusion queries
 * (1 + LightCount per hit pixel, 0 with shadows disabled), retries = 0, lastRenderMs; the other timing fields 0. */
PTX_API int ptx_render_debug(PtxRenderer *r, const PtxRaygenUniformData *uniform, const PtxLightsUbo *lights, const PtxDebugViewDesc *view);
/* Function-level entry for the two pieces of arithmetic only this stage has.  which = 0: DDDcomputeLightContribution
 * (debugClosestHit.rchit:71-141), in: lightDir lightColor attenuation V N color roughness metalness (18 floats), out: rgb;
 * which = 1: getRandomColor (:143-162), in: x (u32 bits), out: rgb. */
PTX_API int ptx_test_debug_eval(PtxRenderer *r, uint32_t which, const float *in, float *out, uint32_t n);

/* ------------------------------------------------------------------------- */
/* Screen path (row D15): what turns the post-processed frame into the image   */
/* the window shows -- the final blit of Renderer::RecordPostProcessCommands   */
/* (Renderer.cpp:1075-1085), RecordUICommands (:1089-1203: toneMapping.comp    */
/* and uiComposition.comp on the screen image, blit to the swapchain image),   */
/* Renderer::UpdateHdr / Swapchain::IsHdr (Swapchain.cpp:317-340)              */
/* ------------------------------------------------------------------------- */

/* the swapchain's format */
enum { PTX_PRESENT_R8G8B8A8_SRGB = 0, PTX_PRESENT_B8G8R8A8_SRGB = 1,
       PTX_PRESENT_A2B10G10R10_UNORM = 2,   /* HDR10 */
       PTX_PRESENT_R16G16B16A16_SFLOAT = 3  /* the screen image itself, 4 x binary16 per pixel */ };
enum { PTX_PRESENT_UI_ON_DEVICE = 1u };     /* PtxPresentDesc.ui is device memory and is read in place */
typedef struct PtxPresentDesc {
    uint32_t width, height;     /* screen extent, 1 .. 16384 each */
    uint32_t format;            /* PTX_PRESENT_* */
    uint32_t toneMappingMode;   /* PtxToneMappingMode; HDR = the surface is HDR10 */
    const void *ui;             /* RGBA8 UNORM, width*height*4 bytes, row-major; NULL = alpha 0 everywhere */
    uint32_t flags;             /* PTX_PRESENT_* flag bits */
    uint32_t reserved;          /* 0 */
} PtxPresentDesc;

/* One frame of the screen path, on the images the last ptx_postprocess left behind (whatever tone-mapping mode that call was
 * given; its uniform supplies BloomIntensity).  Per screen pixel: the composed colour (composition.comp, not tone-mapped) is
 * scaled from the render extent to the screen extent by a linear blit with clamp to edge -- the Vulkan specification's filter, not
 * a bit-match of a GPU's; an axis whose two extents are equal is not filtered, so a frame shown at its own size is the same bits
 * as ptx_read_output's -- then tone-mapped (toneMapping.comp), then uiComposition.comp:49-63: where the UI's alpha is non-zero,
 * srgb_to_linear(ui.rgb) * 0.99 + colour * 0.01; in HDR mode linear_to_hdr10(colour, 203) (BT.709 -> BT.2020, ST 2084); alpha 1.
 * Every store of the reference into its rgba16f screen image is a rounding to binary16 here.  The result is stored in `format`:
 * the sRGB formats encode as ptx_read_output(PTX_OUTPUT_RGBA8_SRGB) does, bytes R G B A or B G R A; A2B10G10R10 packs
 * floor(clamp(c, 0, 1) * 1023 + 0.5) as R | G << 10 | B << 20 | 3 << 30; R16G16B16A16 is the four binary16 bit patterns.
 * The UI image is the caller's (ImGui stays outside) and is not scaled.  Asynchronous on the render stream: a host `ui` is copied on
 * that stream into a buffer the renderer keeps and must stay unchanged until the stream has passed the call (ptx_synchronize,
 * ptx_read_present).  Neither the accumulation image nor ptx_read_output's image is touched.
 * PTX_ERROR_NOT_READY: no ptx_postprocess since the last ptx_resize, or a shard accumulation buffer is bound.
 * PTX_ERROR_INVALID_ARGUMENT: a zero or too large extent, an unknown format, mode or flag bit, reserved != 0, an 8-bit sRGB format
 * with the HDR mode or A2B10G10R10 with the SDR mode (the reference never pairs either).  A refused call leaves the previous
 * present image intact; ptx_resize keeps it too. */
PTX_API int ptx_present(PtxRenderer *r, const PtxPresentDesc *desc);
/* The image of the last ptx_present, row-major, top row first: width*height*4 bytes, *8 for R16G16B16A16.  Synchronous, like
 * ptx_read_output.  PTX_ERROR_INVALID_ARGUMENT: a buffer of another size, or nothing presented yet. */
PTX_API int ptx_read_present(PtxRenderer *r, void *host, size_t bytes);
/* ... or its device address and size, for a host that shares the buffer with its window system (NULL / 0 before any present;
 * a present with a larger image may move it). */
PTX_API void *ptx_device_present_ptr(PtxRenderer *r);
PTX_API size_t ptx_present_bytes(const PtxRenderer *r);

/* ------------------------------------------------------------------------- */
/* Denoiser (docs/NEXT_ROWS.md section 13).  The reference has none: it relies */
/* on accumulation.  This is the stated exception of DESIGN.md section 9, the  */
/* piece that makes a frame of 1 - 8 samples per pixel presentable.            */
/* ------------------------------------------------------------------------- */

enum {
    PTX_GUIDE_NORMAL = 0,   /* hit: the value of PTX_DEBUG_MODE_NORMAL, w = 1;                        miss: (0, 0, 0, 0) */
    PTX_GUIDE_POSITION = 1, /* hit: the value of PTX_DEBUG_MODE_WORLD_POSITION, w = the hit distance; miss: (0, 0, 0, 0) */
    PTX_GUIDE_ALBEDO = 2,   /* hit: material.Color after the decal mix, w = 1;                        miss: (1, 1, 1, 1) */
    PTX_GUIDE_COUNT = 3
};

/* The guide pass: one primary ray through the centre of every owned pixel of the current tile shard -- ptx_render_debug's ray
 * (no RNG, no lens, no culling, no flags; tmin 1e-5, tmax 1e4; the any-hit stage with its decal) -- and the first hit's shading
 * normal, world position + hit distance and base colour STORED into three RGBA32F images of the render extent that the renderer
 * keeps.  Asynchronous on the render stream; works on a borrower and on a scene with pending streamed textures (they sample
 * their stand-ins).  The accumulation image is not touched.  PTX_ERROR_NOT_READY: no scene, tree or image, or a shard
 * accumulation buffer is bound.  A traversal-stack overflow fails the stream, as in ptx_render.  ptx_get_stats afterwards:
 * pathSamples = owned pixels, segments = primary rays, shadowRays = retries = 0.  ptx_resize drops the guides. */
PTX_API int ptx_render_guides(PtxRenderer *r, const PtxRaygenUniformData *uniform);
/* One guide image, device -> host, width*height*16 bytes.  Synchronous, like ptx_read_output.  PTX_ERROR_INVALID_ARGUMENT: an
 * unknown guide or a buffer of another size; PTX_ERROR_NOT_READY: no ptx_render_guides since the last ptx_resize. */
PTX_API int ptx_read_guide(PtxRenderer *r, uint32_t which, void *host, size_t bytes);
/* ... or its device address (width*height*16 bytes; NULL without guides). */
PTX_API void *ptx_device_guide_ptr(PtxRenderer *r, uint32_t which);

typedef struct PtxDenoiseDesc {
    uint32_t totalSamples;  /* samples in the accumulation image: the filter works on the mean, sum / totalSamples */
    uint32_t iterations;    /* 1 .. 6: iteration i (from 0) spreads its 5 x 5 taps 2^i pixels apart */
    float sigmaColor;       /* >= 0; 0: no colour term.  Halved with every iteration */
    float sigmaNormal;      /* > 0 */
    float sigmaPosition;    /* > 0, relative to the centre pixel's hit distance */
    uint32_t flags;         /* 0 */
    uint32_t reserved;      /* 0 */
} PtxDenoiseDesc;

/* The edge-avoiding a-trous filter.  Input: the accumulation image S and the three guides; output: a renderer-owned RGBA32F
 * image D of the MEAN, alpha 1; neither input is written.  With h = (1/16, 1/4, 3/8, 1/4, 1/16), m(p) = S(p).rgb / totalSamples
 * and a_p = max(albedo_p, 0.01) per channel, a pixel p is VALID when it was hit, m(p), n_p and t_p are finite and t_p > 0.
 * c_0(p) = m(p) / a_p on valid pixels and m(p) elsewhere; for i = 0 .. iterations-1 and s = 2^i, on a valid p
 *     c_{i+1}(p) = sum_q w_q c_i(q) / sum_q w_q       over q = p + s (dx, dy), dx, dy in -2 .. 2,
 * the centre with w = h[2] h[2] by rule, any other tap only if q is inside the image and valid, c_i(q) is finite and e >= 0, with
 *     w = h[dx+2] h[dy+2] exp(-e),
 *     e = |c_i(p) - c_i(q)|^2 / (sigmaColor 2^-i)^2 + |n_p - n_q|^2 / sigmaNormal^2 + (dot(n_p, x_q - x_p) / (sigmaPosition t_p))^2
 * (the colour term only with sigmaColor > 0); on any other p, c_{i+1}(p) = c_i(p).  D(p).rgb = c_N(p) a_p on valid pixels and
 * m(p) elsewhere: a NaN or Inf pixel keeps its class and still gets postprocess.comp's marker.  float32 throughout.  One launch
 * per iteration, asynchronous on the render stream.
 * PTX_ERROR_INVALID_ARGUMENT: iterations outside 1 .. 6, totalSamples 0, a sigma that is negative or not finite, sigmaNormal or
 * sigmaPosition 0, unknown flags, reserved != 0.  PTX_ERROR_NOT_READY: no image, no ptx_render_guides since the last ptx_resize, a
 * shard accumulation buffer is bound, or a tile shard with worldSize > 1 (the taps cross tiles; denoising a gathered frame is
 * out of scope).  A refused call leaves the previous D intact; ptx_resize drops it. */
PTX_API int ptx_denoise(PtxRenderer *r, const PtxDenoiseDesc *desc);
/* D, device -> host, width*height*16 bytes; synchronous.  PTX_ERROR_NOT_READY: no ptx_denoise since the last ptx_resize. */
PTX_API int ptx_read_denoised(PtxRenderer *r, void *host, size_t bytes);
/* ... or its device address (NULL without one; the next ptx_denoise may move it). */
PTX_API void *ptx_device_denoised_ptr(PtxRenderer *r);
/* ptx_postprocess's chain with D as the source and TotalSamples taken as 1 (the uniform's own value is ignored): the same
 * kernels on another pointer.  ptx_read_output and ptx_present follow unchanged.  PTX_ERROR_NOT_READY: no ptx_denoise since the
 * last ptx_resize. */
PTX_API int ptx_postprocess_denoised(PtxRenderer *r, const PtxPostProcessingUniformData *uniform, uint32_t toneMappingMode);

/* ------------------------------------------------------------------------- */
/* Temporal accumulation (docs/NEXT_ROWS.md section 14): the history of the   */
/* previous frames, reprojected through the position guide, ahead of the       */
/* filter.  Like the denoiser it has no counterpart in the reference.          */
/* ------------------------------------------------------------------------- */

enum { PTX_TEMPORAL_RESET = 1 }; /* PtxTemporalDesc.flags: ignore the history, start a new one */

typedef struct PtxTemporalDesc {
    float View[16], Proj[16];   /* FORWARD matrices of the camera the current guides were rendered with, column-major like ViewInverse */
    uint32_t totalSamples;      /* samples in the accumulation image */
    float maxHistory;           /* >= 1, finite: cap of the history length L; the blend weight is 1 / L */
    float normalThreshold;      /* > 0 */
    float positionThreshold;    /* > 0, relative to the pixel's hit distance */
    uint32_t flags;             /* PTX_TEMPORAL_RESET = 1: ignore the history */
    uint32_t reserved;          /* 0 */
} PtxTemporalDesc;

/* Temporal accumulation.  Input: the accumulation image S, the three guides and the history the previous accepted call on this
 * handle left; output: a renderer-owned RGBA32F image T of the MEAN with the history length in alpha, and the next call's history.
 * Neither S nor the guides are written.  View and Proj are the forward matrices (world -> view, view -> clip with w = view depth,
 * x and y in -1 .. 1 over the image) whose inverses the uniform of ptx_render_guides carried: keeping them consistent with the
 * guides is the CALLER's duty, nothing here inverts a matrix or can check it.
 *
 * With the denoiser's definitions -- m(p) = S(p).rgb / totalSamples, a_p = max(albedo_p, 0.01) per channel, p VALID when it was
 * hit, m(p), n_p and t_p are finite and t_p > 0 -- the demodulated colour is c(p) = m(p) / a_p.  The history is, per pixel q, the
 * demodulated colour H(q), the length L'(q) (0 on a pixel that was not valid), the normal N'(q) and the position X'(q), and that
 * call's View' and Proj'.  For a valid p, with a history and without PTX_TEMPORAL_RESET:
 *   1. Project.  view = View' (x_p, 1), clip = Proj' view (column-major: out_i = M[i] x + M[4+i] y + M[8+i] z + M[12+i] w).
 *      If clip.w <= 0, or u or v below is not finite, there is no history.  Otherwise, for a W x H image,
 *          u = (clip.x / clip.w * 0.5 + 0.5) W - 0.5,   v = (clip.y / clip.w * 0.5 + 0.5) H - 0.5
 *      (the inverse of the primary ray's pixel-centre convention).
 *      SAME-CAMERA RULE: if View' and Proj' equal this call's View and Proj bit for bit, nothing is projected and the history is
 *      read at p itself, one tap of weight 1: a still camera does not blur its history by rounding (ptx_present's unfiltered
 *      axis is the precedent).
 *   2. Gather.  The taps are the four texels around (u, v): x0 = floor(u), y0 = floor(v), fx = u - x0, fy = v - y0, the texel
 *      (x0 + i, y0 + j) with the bilinear weight (i ? fx : 1 - fx) (j ? fy : 1 - fy).  A tap q COUNTS only if q is inside the
 *      image, L'(q) > 0, H(q) is finite, |n_p - N'(q)|^2 <= normalThreshold^2 and
 *      |dot(n_p, X'(q) - x_p)| <= positionThreshold t_p (the plane distance, the filter's own position term).
 *      The history is FOUND iff the weights of the taps that count sum to >= 1/64 (a rule, like the albedo floor: it bounds how
 *      much the renormalisation amplifies rounding).
 *   3. Blend.  c_h = sum w H(q) / sum w, L_h = sum w L'(q) / sum w over the taps that count, L = min(L_h + 1, maxHistory),
 *      c_acc = c_h + (c(p) - c_h) / L.
 * Without a history, with PTX_TEMPORAL_RESET or where none is found: c_acc = c(p), L = 1.
 * T(p) = (c_acc a_p, L) on valid pixels and (m(p), 0) elsewhere: a miss, NaN or Inf pixel keeps its class and takes part in no
 * other pixel.  float32 throughout.  The call stores c_acc, L, n_p, (x_p, t_p), View and Proj as the next call's history (L = 0
 * on pixels that are not valid).
 *
 * One launch, asynchronous on the render stream; works on a borrower.  Moving geometry is handled conservatively: its previous
 * position fails the plane test and the pixel restarts; there are no per-object motion vectors.  The history is three RGBA32F
 * images kept twice (a thread reads q while its neighbour writes it), with T 112 bytes per pixel.
 * PTX_ERROR_INVALID_ARGUMENT: totalSamples 0, maxHistory < 1 or not finite, a threshold <= 0 or not finite, unknown flags,
 * reserved != 0.  PTX_ERROR_NOT_READY: no image, no ptx_render_guides since the last ptx_resize, a shard accumulation buffer is
 * bound, or a tile shard with worldSize > 1.  A refused call leaves T and the history intact; ptx_resize drops both. */
PTX_API int ptx_temporal_accumulate(PtxRenderer *r, const PtxTemporalDesc *desc);
/* T, device -> host, width*height*16 bytes; synchronous.  PTX_ERROR_INVALID_ARGUMENT: a buffer of another size;
 * PTX_ERROR_NOT_READY: no ptx_temporal_accumulate since the last ptx_resize. */
PTX_API int ptx_read_temporal(PtxRenderer *r, void *host, size_t bytes);
/* ... or its device address (NULL without one). */
PTX_API void *ptx_device_temporal_ptr(PtxRenderer *r);
/* ptx_denoise with T.rgb as the source and totalSamples taken as 1 (the desc's own value is ignored): the same kernels on another
 * pointer, as ptx_postprocess_denoised relates to ptx_postprocess.  The result lands where ptx_denoise's does: ptx_read_denoised,
 * ptx_postprocess_denoised and ptx_present follow unchanged.  Refusals as ptx_denoise's, and PTX_ERROR_NOT_READY: no
 * ptx_temporal_accumulate since the last ptx_resize. */
PTX_API int ptx_denoise_temporal(PtxRenderer *r, const PtxDenoiseDesc *desc);

/* ------------------------------------------------------------------------- */
/* Variance-guided denoising (docs/NEXT_ROWS.md section 16): the first two     */
/* luminance moments accumulated beside the colour history, a per-pixel        */
/* variance from them, and a filter whose colour weight is measured in it.     */
/* ------------------------------------------------------------------------- */

/* ptx_temporal_accumulate, and beside it the MOMENT HISTORY.  T, the colour history and the refusals are the plain call's, bit for
 * bit.  In addition, per valid pixel p with this frame's demodulated mean c = c(p):
 *     l = (0.2126 c.x + 0.7152 c.y) + 0.0722 c.z,   mu = (l, l l).
 * The moment history M' = (mu1', mu2', L_M') of the previous moments call is gathered at the same texels with the same bilinear
 * weights as the colour.  A tap q counts for the moments iff it counted for the colour, L_M'(q) > 0 and both of its moments are
 * finite.  With sum w_M >= 1/64 over those taps:
 *     M_h = sum w mu'(q) / sum w_M,   L_M = min(sum w L_M'(q) / sum w_M + 1, maxHistory),   M = M_h + (mu - M_h) / L_M;
 * otherwise M = mu and L_M = 1 -- also without a history and with PTX_TEMPORAL_RESET.  If either component of M is not finite,
 * (0, 0, 0, 0) is stored: the pixel's moments are UNKNOWN (L_M = 0) and no later tap takes them.  A pixel that is not valid stores
 * zeros.  float32 throughout.
 * The moment history is one more RGBA32F image, (mu1, mu2, L_M, 0), kept twice, ping-ponging with the colour history: 32 more bytes
 * per pixel.  A plain ptx_temporal_accumulate DROPS the moment history: the next moments call restarts M (M = mu, L_M = 1) on the
 * colour history as it stands.  ptx_resize drops everything; a refused call leaves everything intact.  One launch, asynchronous on
 * the render stream; a caller that never makes this call allocates nothing for it. */
PTX_API int ptx_temporal_accumulate_moments(PtxRenderer *r, const PtxTemporalDesc *desc);
/* The moment history of the last moments call, device -> host, width*height*16 bytes: (mu1, mu2, L_M, 0) per pixel; synchronous.
 * PTX_ERROR_INVALID_ARGUMENT: a buffer of another size; PTX_ERROR_NOT_READY: the last accepted accumulate call since ptx_resize was
 * not ptx_temporal_accumulate_moments. */
PTX_API int ptx_read_moments(PtxRenderer *r, void *host, size_t bytes);

/* The variance-guided filter.  Input: T, the moment history and the three guides; output: D where ptx_denoise leaves it (alpha 1),
 * so ptx_read_denoised, ptx_postprocess_denoised and ptx_present follow unchanged, and V_0 for ptx_read_variance.  No input is
 * written.  The desc is read as: iterations 1 .. 6; sigmaColor as sigmaLuminance, > 0 here; sigmaNormal, sigmaPosition > 0;
 * totalSamples ignored (T is a mean); flags 0, reserved 0.  Validity, a_p and h are the denoiser's with m(p) = T(p).rgb;
 * lum(c) = (0.2126 c.x + 0.7152 c.y) + 0.0722 c.z; c_0(p) = m(p) / a_p on valid pixels and m(p) elsewhere.
 *
 * 1. ESTIMATE (the first launch).  V_0(p) = 0 on a pixel that is not valid.  On a valid p with the moments (mu1, mu2, L_M):
 *    where L_M(p) >= 4, v = mu2 - mu1 mu1.  Otherwise a 7 x 7 window around p: a tap q counts iff it is inside the image, valid and
 *    L_M(q) > 0, with
 *        w = exp(-(|n_p - n_q|^2 / sigmaNormal^2 + (dot(n_p, x_q - x_p) / (sigmaPosition t_p))^2)),
 *    the centre with w = 1 iff its moments are known (L_M(p) > 0);
 *        m1 = sum w mu1(q) / sum w,  m2 = sum w mu2(q) / sum w,  v = m2 - m1 m1;   sum w = 0 gives v = 0.
 *    V_0 = v where v is finite and > 0, else 0.  There is no boost for a short history.
 * 2. FILTER.  For i = 0 .. iterations-1 and s = 2^i, on a valid p:
 *    PREFILTER: vt(p) = the 3 x 3 mean of V_i around p (not dilated) with the weights 1/4 (centre), 1/8 (edges), 1/16 (corners) over
 *    the taps inside the image and valid, divided by the sum of the weights that count.
 *    TAPS: the denoiser's -- q = p + s (dx, dy), dx, dy in -2 .. 2, the centre with w = h[2] h[2] by rule, any other tap only if q is
 *    inside the image and valid, c_i(q) is finite and e >= 0 -- with the colour term replaced:
 *        d = |lum(c_i(p)) - lum(c_i(q))|;  e_l = 0 if d = 0;  the tap does NOT count if d > 0 and vt(p) = 0;  otherwise
 *        e_l = d^2 / (sigmaLuminance^2 vt(p)),
 *        e = e_l + |n_p - n_q|^2 / sigmaNormal^2 + (dot(n_p, x_q - x_p) / (sigmaPosition t_p))^2,   w = h[dx+2] h[dy+2] exp(-e),
 *        c_{i+1}(p) = sum w c_i(q) / sum w,   V_{i+1}(p) = sum w^2 V_i(q) / (sum w)^2.
 *    sigmaLuminance is NOT halved per iteration: the variance shrinks by itself.  On any other p, c_{i+1}(p) = c_i(p).
 *    D(p).rgb = c_N(p) a_p on valid pixels and m(p) elsewhere, as in ptx_denoise.
 * The formulas hold no epsilon and no square root: a sum scaled by 2^k gives D scaled by 2^k.  float32 throughout; 1 + iterations
 * launches, asynchronous on the render stream; V_0 is one float per pixel the renderer keeps.
 * PTX_ERROR_INVALID_ARGUMENT: iterations outside 1 .. 6, a sigma that is <= 0 or not finite, unknown flags, reserved != 0.
 * PTX_ERROR_NOT_READY: whatever ptx_denoise_temporal answers so, and unless the last accepted accumulate call since ptx_resize
 * was ptx_temporal_accumulate_moments.  A refused call leaves D, V_0, T and both histories intact. */
PTX_API int ptx_denoise_variance(PtxRenderer *r, const PtxDenoiseDesc *desc);
/* V_0 of the last ptx_denoise_variance, device -> host, width*height*4 bytes: one float per pixel; synchronous.
 * PTX_ERROR_INVALID_ARGUMENT: a buffer of another size; PTX_ERROR_NOT_READY: no ptx_denoise_variance since the last ptx_resize. */
PTX_API int ptx_read_variance(PtxRenderer *r, void *host, size_t bytes);

/* ------------------------------------------------------------------------- */
/* Motion guides (docs/NEXT_ROWS.md section 17): where every first hit was in  */
/* the pose the temporal history was made from, so that animated geometry      */
/* keeps its history.  An addition: a host that never calls ptx_track_motion   */
/* pays nothing, and every call above computes what it computed before.        */
/* ------------------------------------------------------------------------- */

enum {
    PTX_MOTION_POSITION = 0, /* X_prev: (Position_prev, 1) known, (x_p, 0) unknown, (0, 0, 0, 0) miss */
    PTX_MOTION_NORMAL = 1,   /* N_prev: (Normal_prev, 1) known,   (n_p, 0) unknown, (0, 0, 0, 0) miss */
    PTX_MOTION_COUNT = 2
};

/* POSE BOOKKEEPING, kept with the scene, so the borrowers of a shared scene see it.  The POSE SERIAL S counts the accepted
 * ptx_update_animation calls, tracking or not.  Every guide pass (ptx_render_guides, ptx_render_guides_motion) records the serial
 * it rendered at; every accepted accumulate call (plain, moments or motion) tags its history with the serial of the guides it
 * consumed.  While tracking is on, ptx_update_animation first SNAPSHOTS the pose it is about to replace: the device pair-transform
 * table and the skinned part of the vertex buffer (whole PtxVertex records), device to device on the render stream ahead of its
 * uploads and the skinning; the snapshot is valid for serial S - 1.  The buffers come with the first such update (the table plus
 * 56 bytes per skinned vertex); turning tracking off releases them; with tracking off the update enqueues exactly what it always
 * did.  ptx_scene_upload and its streamed form reset everything: tracking off, no snapshot, and a serial no earlier history
 * leads back to.
 * Owner only: PTX_ERROR_INVALID_ARGUMENT on a renderer that borrows its scene (like ptx_update_animation), PTX_ERROR_NOT_READY
 * without a scene. */
PTX_API int ptx_track_motion(PtxRenderer *r, int enable);

/* ptx_render_guides plus two more RGBA32F images from the same single traversal.  The three guides it stores are those of
 * ptx_render_guides bit for bit.  Let h be the pose serial of this renderer's current temporal history and S the scene's:
 *     h == S                                  the previous pose is the current one;
 *     h == S - 1 and the snapshot is valid    the previous pose is the snapshot;
 *     anything else (no history, several updates since, tracking enabled after the update)   the motion is UNKNOWN.
 * At a pixel whose primary ray hit (pair, prim) with the barycentrics b = (1 - u - v, u, v), with a known previous pose:
 *   1. the triangle's three vertices of the previous pose are vertices[pair.vertexOffset + indices[pair.indexOffset + 3 prim + k]],
 *      k = 0, 1, 2 -- a vertex from the snapshot when its index lies in the skinned block, from the vertex buffer otherwise;
 *   2. Position, Normal, Tangent and Bitangent are interpolated as (a b.x + b b.y) + c b.z;
 *   3. the previous pose's pair transform is applied as the guide pass applies the current one: the position by the 3 x 4 matrix,
 *      tangent and bitangent by its linear part and normalised, the normal by the inverse transpose and normalised;
 *   4. X_prev = (Position_prev, 1) and N_prev = (normalize(Normal_prev + TBN_prev material.Normal), 1), where material.Normal is
 *      the tangent-space normal the guide pass sampled at this hit (of the CURRENT frame; it is not sampled again).
 * Unknown motion stores (x_p, 0) and (n_p, 0), the position and normal guides with w = 0; a miss stores zeros.  Where neither the
 * pair's transform nor the triangle's vertices changed, X_prev.xyz and N_prev.xyz equal the guides bit for bit (the same
 * operations on the same operands).  The previous pose is found through (pair, prim), never through the triangle's place in the
 * tree: the result does not depend on PTX_ACCEL_REFIT versus PTX_ACCEL_REBUILD.
 * Refusals as ptx_render_guides', and PTX_ERROR_NOT_READY while the scene's owner does not track motion.  Works on a borrower and
 * with pending streamed textures.  ptx_resize drops the motion images; a later plain ptx_render_guides makes them stale.  Known
 * limits: two updates between temporal frames make the motion unknown; first hit only; a moving light lags unless the
 * accumulate call is ptx_temporal_accumulate_responsive (docs/NEXT_ROWS.md section 19); several
 * borrowers at different histories share the one snapshot, which the serial rule keeps correct, not optimal. */
PTX_API int ptx_render_guides_motion(PtxRenderer *r, const PtxRaygenUniformData *uniform);
/* One motion image, device -> host, width*height*16 bytes; synchronous.  PTX_ERROR_INVALID_ARGUMENT: an unknown image or a buffer
 * of another size; PTX_ERROR_NOT_READY: the last guide pass since ptx_resize was not ptx_render_guides_motion. */
PTX_API int ptx_read_motion(PtxRenderer *r, uint32_t which, void *host, size_t bytes);
/* ... or its device address (NULL without one). */
PTX_API void *ptx_device_motion_ptr(PtxRenderer *r, uint32_t which);

/* ptx_temporal_accumulate (withMoments = 0) or ptx_temporal_accumulate_moments (withMoments = 1) with steps 1 and 2 of
 * ptx_temporal_accumulate run on (x~, n~) = (X_prev.xyz, N_prev.xyz) of the last ptx_render_guides_motion in place of (x_p, n_p):
 * x~ is projected, and a tap q counts only if |n~ - N'(q)|^2 <= normalThreshold^2 and |dot(n~, X'(q) - x~)| <= positionThreshold t_p
 * (the other conditions as they were).  SAME-CAMERA RULE: one tap of weight 1 at p itself requires equal matrices AND x~ bit-equal to
 * x_p; under equal matrices a pixel whose x~ differs is projected through them like any other.  A pixel whose motion is unknown
 * takes no history: c_acc = c(p), L = 1 (and M = mu, L_M = 1).  Everything else is the plain call's: the blend, what is stored for
 * the next call (the CURRENT n_p and (x_p, t_p)), the moments' taps, the treatment of pixels that are not valid, the refusals.
 * Consequence: after a ptx_render_guides_motion with no update since the history's pose, the call is the plain one bit for bit.
 * PTX_ERROR_INVALID_ARGUMENT: withMoments above 1.  PTX_ERROR_NOT_READY: the motion guides are stale -- a plain ptx_render_guides
 * came after them, or an accumulate call moved the history to another pose.  ptx_denoise_temporal, ptx_denoise_variance and the
 * output stage follow unchanged. */
PTX_API int ptx_temporal_accumulate_motion(PtxRenderer *r, const PtxTemporalDesc *desc, uint32_t withMoments);

/* ------------------------------------------------------------------------- */
/* Specular-chain guides (docs/NEXT_ROWS.md section 18): the guide pass that   */
/* follows mirrors and glass to the first surface that is neither, so that the */
/* filters and the temporal stage see what a mirror shows, not the mirror.  An */
/* addition: every call above computes what it computed before.                */
/* ------------------------------------------------------------------------- */

typedef struct PtxSpecularGuidesDesc {
    uint32_t maxBounces;   /* 0 ... 8 continuation rays per pixel; 0 = the plain pass */
    float    roughnessMax; /* a surface is followed only if material.Roughness <= roughnessMax; >= 0, finite */
    uint32_t flags;        /* 0 */
    uint32_t reserved;     /* 0 */
} PtxSpecularGuidesDesc;

enum {
    PTX_SPECULAR_SURFACE = 0, /* (first-hit Position, float(bounces) + 16 class); primary miss: (0, 0, 0, 0) */
    PTX_SPECULAR_COUNT = 1
};

/* ptx_render_guides that follows near-delta surfaces.  Writes PTX_GUIDE_NORMAL, PTX_GUIDE_POSITION, PTX_GUIDE_ALBEDO and
 * PTX_SPECULAR_SURFACE for the owned pixels of the current tile shard, in one launch.
 * PRIMARY RAY AND FIRST HIT are ptx_render_guides': the ray through (0.5, 0.5) of the pixel with its two offset rays (which start at
 * the primary's origin), traced over 1e-5 ... 1e4 with the any-hit stage where the scene has non-opaque geometry, an ignored
 * candidate in front of the hit tinting its colour (the decal mix).
 * THE CHAIN.  Let d be the current ray's direction, T = 0, M = the identity, tint = (1, 1, 1), bounces = 0.  At the current hit, at
 * distance t:
 *   1. The vertex is interpolated and transformed, the texture footprint taken from the offset rays and the material sampled: at
 *      the first hit with the expressions of ptx_render_guides, at later hits with those of the path tracer's closest-hit stage.
 *      isHitFromInside = dot(geometricNormal, d) > 0; the material is sampled with it, so that Eta is the path tracer's (Ior from
 *      inside, 1 / Ior from outside); the decal mix follows as above.
 *   2. N = normalize(vertex.Normal + TBN material.Normal).  N_guide takes the vertex frame as interpolated (nothing flipped, as
 *      ptx_render_guides); N_cont takes the frame with Normal, Tangent and Bitangent negated where the hit is from inside, and is
 *      the only one the continuation uses.
 *   3. The chain STOPS here if bounces == maxBounces, or material.Roughness > roughnessMax, or neither class of 4 applies.
 *   4. Otherwise it continues along the zero-roughness limit of the BSDF sample (the half vector is the shading normal):
 *        MIRROR, Metalness >= 0.5: d' = normalize(reflect(d, N_cont)); the origin is the closest-hit stage's shadow-terminator
 *          offset for a reflected ray; tint *= material.Color; M = M (I - 2 N_cont N_cont^T).
 *        GLASS, else Transmission >= 0.5: r = refract(d, N_cont, material.Eta).  r = 0 (total internal reflection): as MIRROR, but
 *          tint stays.  Otherwise d' = normalize(r), the origin is the closest-hit stage's self-intersection offset along
 *          -geometricNormal (flipped where the hit is from inside), tint *= material.Color, M stays.
 *      The offset rays follow as the closest-hit stage propagates them (reflected or refracted differentials, vertex.Normal flipped
 *      where from inside).  T += t, bounces += 1, and d' is traced like the primary ray (interval, any-hit stage, decal).  A miss
 *      ends the chain as ESCAPED.
 * STORED, with T including the last segment, ro and rd0 the primary ray's origin and direction (t is the ray parameter of the
 * traced direction: later directions are normalised, rd0 is the primary ray's as it is, unit to float32 rounding):
 *                   chain ends on a surface                         escaped (miss after >= 1 bounce)   primary miss
 *     NORMAL        (M N_guide, 1)                                  (0, 0, 0, 0)                       (0, 0, 0, 0)
 *     POSITION      (ro + normalize(rd0) T, T)                      (0, 0, 0, 0)                       (0, 0, 0, 0)
 *     ALBEDO        (tint material.Color, 1)                        (1, 1, 1, 1)                       (1, 1, 1, 1)
 *     SURFACE       (first-hit Position, bounces + 16 class)        the same with class 2              (0, 0, 0, 0)
 *   class 0: ended on a surface that is not followed; 1: stopped at maxBounces; 2: escaped.  For a planar mirror the stored position
 *   is the mirror image of the reflected surface point, a fixed world point: it reprojects into the previous camera, and the
 *   unfolded normal M N passes the plane tests of the filters and of ptx_temporal_accumulate.  An escaped pixel is "not hit" to every
 *   consumer and passes through unfiltered, as sky does.
 * BIT-EXACTNESS.  A pixel with bounces == 0 holds exactly the bits ptx_render_guides stores in all three guides, whatever the desc
 * says -- (N_guide, 1), (vertex.Position, t) and (material.Color, 1), never M N or ro + rd T; maxBounces == 0 reproduces
 * ptx_render_guides entirely.
 * CONTRACT: ptx_render_guides'.  Asynchronous on the render stream; works on a borrower and with pending streamed textures; uploads
 * the empty light block; a traversal-stack overflow fails the stream through the counter block; the accumulation is untouched.
 * ptx_get_stats: pathSamples = owned pixels, segments = rays traced (primary + continuation), shadowRays = retries = 0.  To the
 * chain the call is a plain guide pass: the motion images go stale.  ptx_resize drops the fourth image with the guides.
 * A later ptx_render_guides or ptx_render_guides_motion rewrites the three guides and leaves the fourth image as it was: it then
 * belongs to older guides and stays readable until the next ptx_resize.
 * PTX_ERROR_NOT_READY: as ptx_render_guides.  PTX_ERROR_INVALID_ARGUMENT: a NULL argument, maxBounces > 8, roughnessMax negative or
 * not finite, flags or reserved not 0.  A refused call leaves all four images and the chain's state intact.
 * Known limits: refraction does not unfold the normal and the virtual point is exact for planar mirrors only (curved mirrors and
 * glass are an approximation the plane test may reject: the pixel restarts); Fresnel reflection on glass is not followed; there is
 * no motion variant; surfaces rougher than roughnessMax stay first-hit. */
PTX_API int ptx_render_guides_specular(PtxRenderer *r, const PtxRaygenUniformData *uniform, const PtxSpecularGuidesDesc *desc);
/* The fourth image, device -> host, width*height*16 bytes; synchronous.  PTX_ERROR_INVALID_ARGUMENT: an unknown image or a buffer of
 * another size; PTX_ERROR_NOT_READY: no ptx_render_guides_specular since the last ptx_resize. */
PTX_API int ptx_read_specular_guide(PtxRenderer *r, uint32_t which, void *host, size_t bytes);
/* ... or its device address (NULL without one). */
PTX_API void *ptx_device_specular_guide_ptr(PtxRenderer *r, uint32_t which);

/* ------------------------------------------------------------------------- */
/* Responsive temporal history (docs/NEXT_ROWS.md section 19): a second, short */
/* history beside the long one follows a change of lighting within a few       */
/* frames; the long history is clamped into the box the short one spans around */
/* the pixel and shortened where the clamp bit.  An addition: every call above */
/* computes what it computed before, and a host that never makes this call     */
/* allocates nothing for it.                                                   */
/* ------------------------------------------------------------------------- */

enum { PTX_RESPONSIVE_MOMENTS = 1, PTX_RESPONSIVE_MOTION = 2 };   /* PtxResponsiveDesc.flags */

typedef struct PtxResponsiveDesc {
    float fastHistory;   /* >= 1, finite, <= the temporal desc's maxHistory: cap of the fast history's length L_F */
    float clampSigma;    /* > 0, finite: half-width of the clamp box in standard deviations */
    uint32_t flags;      /* which accumulate call this one extends */
    uint32_t reserved;   /* 0 */
} PtxResponsiveDesc;

/* Two launches on the render stream: pass A accumulates, pass B clamps.
 *
 * PASS A is the BASE CALL chosen by responsive->flags, bit for bit in T, the colour history, the moment history and every tap
 * decision:
 *     0                                                ptx_temporal_accumulate
 *     PTX_RESPONSIVE_MOMENTS                           ptx_temporal_accumulate_moments
 *     PTX_RESPONSIVE_MOTION                            ptx_temporal_accumulate_motion(.., 0)
 *     PTX_RESPONSIVE_MOTION | PTX_RESPONSIVE_MOMENTS   ptx_temporal_accumulate_motion(.., 1)
 * Beside the colour history it carries the FAST HISTORY F' = (F.rgb, L_F) of the previous responsive call along the same taps with
 * the same bilinear weights, as the moments are carried.  With c = c(p), this frame's demodulated mean: a tap q counts for F iff it
 * counted for the colour, L_F'(q) > 0 and F'(q).rgb is finite.  With sum w_F >= 1/64 over those taps:
 *     F_h = sum w F'(q) / sum w_F,   L_F = min(sum w L_F'(q) / sum w_F + 1, fastHistory),   F = F_h + (c - F_h) / L_F
 * (the colour's own operations in the colour's own order); otherwise F = c and L_F = 1 -- also without a history, with
 * PTX_TEMPORAL_RESET and on a pixel whose motion is unknown.  If F is not finite, (0, 0, 0, 0) is stored: F is UNKNOWN (L_F = 0) and
 * no later tap takes it.  A pixel that is not valid stores zeros.  F is one more RGBA32F image, (F.rgb demodulated, L_F), kept twice,
 * ping-ponging with the colour history: 32 more bytes per pixel, allocated by the first responsive call.  An accumulate call that is
 * not responsive DROPS the fast history, as a plain call drops the moments: the next responsive call restarts F (F = c, L_F = 1) on
 * the colour history as it stands.
 *
 * PASS B acts on a valid pixel p only if pass A found a history for it (L > 1), L_F(p) > 0 and c_acc(p) is finite; everywhere else
 * it is the identity.  The window is the 5 x 5 texels around p (not dilated) of THIS call's F; a tap q counts iff it is inside the
 * image and L_F(q) > 0, so the centre always counts and n >= 1.  There is no normal or position term: a window that straddles an
 * edge only widens the box.  Per channel, in two passes over the window, row by row from (-2, -2) to (2, 2):
 *     mu = sum F(q) / n,   var = sum (F(q) - mu)^2 / n,   sigma = sqrt(var),
 *     lo = mu - clampSigma sigma,   hi = mu + clampSigma sigma,   c' = min(max(c_acc, lo), hi),
 * min and max taken as comparisons (c' = lo where c_acc < lo, hi where c_acc > hi, else c_acc: a bound that is not a number leaves
 * c_acc as it is).  The pixel is CLAMPED iff c_acc < lo or c_acc > hi in some channel.  On a clamped pixel L_out = min(L, L_F(p)),
 * and with PTX_RESPONSIVE_MOMENTS and L_M(p) > 0, L_M becomes min(L_M, L_F(p)); the moments themselves are kept.  Elsewhere
 * L_out = L.  Pass B rewrites T(p) = (c' a_p, L_out), the pixel's own entry (c', L_out) of the colour history pass A just wrote, and
 * L_M of its own entry of the moment history; it touches nothing of any other pixel, so both passes work on the same ping-pong copy.
 * float32 throughout; n is a float; a division is the project's a * rcp(b); the square root is sqrt_ of csrc/pt_device.hpp, the
 * correctly rounded IEEE square root PTX_FN_SQRT exposes.
 *
 * Consequences: (a) a first call, a PTX_TEMPORAL_RESET call and a maxHistory 1 call are the base call bit for bit (no pixel has
 * L > 1); (b) with fastHistory == maxHistory, from a common start and while nothing is clamped, F equals the colour history bit for
 * bit; (c) where F is constant over the window (sigma = 0), c' = F(p).
 *
 * PTX_ERROR_INVALID_ARGUMENT: a NULL argument, fastHistory below 1, not finite or above desc->maxHistory, clampSigma <= 0 or not
 * finite, unknown flags, reserved != 0, and whatever the base call answers so.  PTX_ERROR_NOT_READY: whatever the base call answers
 * so, stale motion guides under PTX_RESPONSIVE_MOTION included.  A refused call leaves T, all three histories and D intact;
 * ptx_resize drops everything.  Works on a borrower; ptx_denoise_temporal, ptx_denoise_variance and the output stage follow
 * unchanged. */
PTX_API int ptx_temporal_accumulate_responsive(PtxRenderer *r, const PtxTemporalDesc *desc, const PtxResponsiveDesc *responsive);
/* The fast history of the last responsive call, device -> host, width*height*16 bytes: (F.rgb demodulated, L_F) per pixel;
 * synchronous.  PTX_ERROR_INVALID_ARGUMENT: a buffer of another size; PTX_ERROR_NOT_READY: the last accepted accumulate call since
 * ptx_resize was not ptx_temporal_accumulate_responsive. */
PTX_API int ptx_read_fast_history(PtxRenderer *r, void *host, size_t bytes);   /* (F.rgb demodulated, L_F), width*height*16 */
/* ... or its device address (NULL without one). */
PTX_API void *ptx_device_fast_history_ptr(PtxRenderer *r);

/* ------------------------------------------------------------------------- */
/* Firefly suppression (docs/NEXT_ROWS.md section 20): a rank clamp ahead of   */
/* the chain and the output stage.  Every pixel's luminance is capped at gain  */
/* times the rank-th largest luminance among its neighbours; only comparisons  */
/* decide who is clamped, so the result does not depend on the image's scale.  */
/* An addition: every call above computes what it computed before, and a host  */
/* that never calls these functions allocates nothing for them.                */
/* ------------------------------------------------------------------------- */

typedef struct PtxDespikeDesc {
    uint32_t radius;   /* 1 or 2: the window is (2 radius + 1)^2 without its centre */
    uint32_t rank;     /* 1 ... 4: which of the neighbours' luminances, counted from the largest, is the bound */
    uint32_t minTaps;  /* rank ... (2 radius + 1)^2 - 1: a pixel with fewer counting neighbours is left alone */
    float    gain;     /* >= 1, finite: the bound is gain times that luminance */
    uint32_t flags;    /* 0 */
    uint32_t reserved; /* 0 */
} PtxDespikeDesc;

/* S is the accumulation image (ptx_device_accum_ptr, a bound image included).  C is a renderer-owned RGBA32F image of the render
 * extent IN THE SUM'S SCALE, so that C can stand wherever S does; S is never written.  All arithmetic is float32 with the operations
 * in the order written (no contraction).
 *   1. Y(p) = (0.2126f S(p).r + 0.7152f S(p).g) + 0.0722f S(p).b.
 *   2. A pixel COUNTS iff Y(p) is finite (a NaN or Inf channel makes Y non-finite).
 *   3. The window of p is the (2 radius + 1)^2 texels around p without p itself.
 *   4. A tap q counts iff it is inside the image and the pixel there counts.
 *   5. n is the number of counting taps.
 *   6. h is the rank-th largest Y among the counting taps, equal values counted separately.
 *   7. b = gain h where that product is greater than zero, and b = +0 otherwise (a negative product and -0 alike).
 *   8. p is CLAMPED iff all four hold: p counts; n >= minTaps; Y(p) >= 2^-126 (a normal number, so that the specified reciprocal
 *      is finite); Y(p) > b.
 *   9. If p is clamped, s = b rcp(Y(p)) -- the project's division: rcp is the correctly rounded reciprocal on [2^-126, 2^126] and
 *      +-0 above -- C(p).rgb = S(p).rgb s, channel by channel, and C(p).a = S(p).a.
 *  10. Otherwise C(p) = S(p) bit for bit.  A pixel that is not finite keeps its class, so the output stage's markers still appear.
 * Consequences: (a) a constant image comes back bit for bit; (b) multiplying S by a power of two multiplies C by it, bit for bit
 * (short of overflow and of denormals); (c) a pixel whose counting neighbours are all black becomes zeros; (d) with rank 1 two adjacent equal
 * spikes protect each other, with rank 2 both are clamped.
 * One launch, asynchronous on the render stream; needs no scene and no guides; works on a borrower.  C is of the sum as it stood
 * when the call was enqueued: a later ptx_render does not refresh it, that is the host's job, as with the guides.  C is allocated by
 * the first call (16 bytes per pixel).
 * PTX_ERROR_INVALID_ARGUMENT: a NULL argument, radius other than 1 or 2, rank outside 1 ... 4, minTaps < rank,
 * minTaps > (2 radius + 1)^2 - 1, gain < 1 or not finite, flags != 0, reserved != 0.  PTX_ERROR_NOT_READY: no image (ptx_resize), a
 * shard accumulation buffer bound, a tile shard with worldSize > 1 (the taps cross tiles).  A refused call leaves the previous C
 * intact; ptx_resize drops C.
 * Known limits: a one-pixel emitter or sun is clamped like a firefly; energy is lost by design; there is no guide term. */
PTX_API int ptx_despike(PtxRenderer *r, const PtxDespikeDesc *desc);
/* C, device -> host, width*height*16 bytes; synchronous.  PTX_ERROR_INVALID_ARGUMENT: a NULL argument or a buffer of another size;
 * PTX_ERROR_NOT_READY: no ptx_despike since the last ptx_resize. */
PTX_API int ptx_read_despiked(PtxRenderer *r, void *host, size_t bytes);
/* ... or its device address (NULL without one). */
PTX_API void *ptx_device_despiked_ptr(PtxRenderer *r);
/* A sticky switch, like ptx_track_motion: off by default, kept across ptx_resize.  While on, ptx_temporal_accumulate, its moments,
 * motion and responsive forms and ptx_denoise read C where they read S, and nothing else changes; their refusals gain one last
 * reason, behind every other: PTX_ERROR_NOT_READY while no C exists since the last ptx_resize, with T, the histories and D intact.
 * While off those calls are what they were.  PTX_ERROR_INVALID_ARGUMENT: a NULL handle. */
PTX_API int ptx_chain_use_despiked(PtxRenderer *r, int enable);
/* ptx_postprocess's chain on C with the caller's TotalSamples (C is in the sum's scale); ptx_read_output and ptx_present follow
 * unchanged.  PTX_ERROR_INVALID_ARGUMENT as ptx_postprocess; PTX_ERROR_NOT_READY: no ptx_despike since the last ptx_resize. */
PTX_API int ptx_postprocess_despiked(PtxRenderer *r, const PtxPostProcessingUniformData *uniform, uint32_t toneMappingMode);

/* ------------------------------------------------------------------------- */
/* Exposure metering (docs/NEXT_ROWS.md section 21): a luminance histogram of  */
/* the image the output stage is about to read sets that stage's exposure, on  */
/* the device.  An addition: every call above computes what it computed        */
/* before, and a host that never calls ptx_meter allocates nothing for it.     */
/* ------------------------------------------------------------------------- */

enum {
    PTX_METER_SUM = 0,      /* the accumulation image, as ptx_postprocess reads it: totalSamples is the caller's */
    PTX_METER_DESPIKED = 1, /* C of ptx_despike, as ptx_postprocess_despiked reads it: in the sum's scale, totalSamples is the caller's */
    PTX_METER_DENOISED = 2  /* D of the filters, as ptx_postprocess_denoised reads it: D holds the mean, so 1 stands for totalSamples */
};
enum {
    PTX_METER_AVERAGE = 0,
    PTX_METER_CENTRE = 1,
    PTX_METER_REGION = 2
};

typedef struct PtxMeterDesc {
    uint32_t source;          /* PTX_METER_SUM / _DESPIKED / _DENOISED */
    uint32_t mode;            /* PTX_METER_AVERAGE / _CENTRE / _REGION */
    uint32_t totalSamples;    /* > 0; what PtxPostProcessingUniformData::TotalSamples will be (PTX_METER_DENOISED: checked, then 1 is used) */
    uint32_t region[4];       /* x0, x1, y0, y1: [x0, x1) x [y0, y1), read in PTX_METER_REGION only */
    uint32_t lowPermille;     /* the share of the counted weight cut off at the dark end ... */
    uint32_t highPermille;    /* ... and at the bright end; lowPermille + highPermille < 1000 */
    float    keyLog2;         /* log2 of the luminance the kept mean is brought to (log2(0.18): middle grey) */
    float    compensation;    /* stops added on top */
    float    minLog2Exposure; /* the target is clamped to [minLog2Exposure, maxLog2Exposure] */
    float    maxLog2Exposure;
    float    speedUp;         /* 1 / seconds, >= 0: the rate while the exposure rises ... */
    float    speedDown;       /* ... and while it falls */
    float    deltaSeconds;    /* >= 0: the time since the previous ptx_meter */
    uint32_t flags;           /* 0 */
    uint32_t reserved;        /* 0 */
} PtxMeterDesc;

typedef struct PtxMeterResult {
    float    exposure;     /* the factor ptx_postprocess_metered multiplies PtxPostProcessingUniformData::Exposure by; 1 after a reset */
    float    log2Exposure; /* its logarithm, the adapted state; 0 after a reset */
    float    avgLog2;      /* the mean log2 luminance of the kept weight (step 6) of the last valid call */
    float    targetLog2;   /* where the last valid call was heading (step 7) */
    uint32_t counted;      /* N: the weight in the 256 bins */
    uint32_t kept;         /* K: what the trim left of it */
    uint32_t black;        /* the weight of the black class ... */
    uint32_t rejected;     /* ... and of the rejected one */
    uint32_t under;        /* the part of bin 0 that lies below 2^-16 */
    uint32_t over;         /* the part of bin 255 that lies at or above 2^16 */
    uint32_t valid;        /* 1: the last call had K > 0 and moved the exposure; 0: it left it alone */
    uint32_t calls;        /* accepted ptx_meter calls since the last reset */
} PtxMeterResult;

/* ptx_meter.  W x H is the render extent, p = (x, y) a pixel.  Unless stated otherwise the arithmetic is float32 up to the histogram
 * (steps 1 - 4) and float64 behind it (steps 5 - 8), IEEE operations in the order written with no contraction; rcp, exp2 and the
 * division f3 / float are the project's own specified kernels.
 *   1. LUMINANCE.  c(p) = source(p).rgb / (float)totalSamples: one rcp of (float)totalSamples and three multiplies, exactly as the
 *      output stage forms the value it multiplies by Exposure.  Y(p) = (0.2126f c.r + 0.7152f c.g) + 0.0722f c.b.
 *   2. CLASSES.  Every pixel of weight above zero falls into exactly one of three: REJECTED iff Y is not finite (the output stage's
 *      NaN / Inf marker pixels); BLACK iff Y <= 0 or Y < 2^-126 (zero of either sign, negatives, denormals); COUNTED otherwise.
 *   3. BIN.  Comparisons and shifts only, no logarithm per pixel: k = bits(Y) >> 20 (the eight exponent bits and the top three
 *      mantissa bits: eight sub-bins per octave), i = k - 888.  i < 0 goes to bin 0 and counts in `under`; i > 255 goes to bin 255 and
 *      counts in `over`.  The 256 bins span [2^-16, 2^16); Y = 1 lands in bin 128.
 *   4. WEIGHT.  w(p) is an integer.  PTX_METER_AVERAGE: w = 1.  PTX_METER_CENTRE: w = wx wy with
 *      wx = 1 + [W <= 4x + 2 <= 3W] + [3W <= 8x + 4 <= 5W] and wy the same expression in y and H: 1 ... 9, integers only.
 *      PTX_METER_REGION: w = 1 inside region = [x0, x1) x [y0, y1) and 0 outside; a pixel of weight 0 belongs to no class.
 *      Bins and class counters are sums of weights in uint32.  A call whose largest possible total -- W H, 9 W H, or the region's
 *      area -- reaches 2^32 is refused.
 *   5. TRIM.  n_i is bin i, N = SUM n_i.  lo = floor(N lowPermille / 1000), hi = floor(N highPermille / 1000) in 64-bit integers.
 *      P_i is the exclusive prefix sum of n.  kept_i = max(0, min(P_i + n_i, N - hi) - max(P_i, lo)).  K = SUM kept_i (= N - lo - hi).
 *      If K = 0: valid = 0, and the four floats of the result keep their previous values; steps 6 - 8 do not run.
 *   6. MEAN.  A = SUM kept_i (i >> 3) and B_j = SUM over i & 7 = j of kept_i, exact in uint64.  T_j is the double nearest to
 *      log2(1 + (2j + 1) / 16), the centre of sub-bin j:
 *        T_0 = 0x1.663f6fac91316p-4   T_1 = 0x1.fbc16b902680ap-3   T_2 = 0x1.91bba891f1709p-2   T_3 = 0x1.0c10500d63aa6p-1
 *        T_4 = 0x1.49a784bcd1b8bp-1   T_5 = 0x1.82809d5be7073p-1   T_6 = 0x1.b74948f5532dap-1   T_7 = 0x1.e88c6b3626a73p-1
 *      avg = ((double)A + ((...((double)B_0 T_0 + (double)B_1 T_1) + ...) + (double)B_7 T_7)) / (double)K - 16.
 *      avgLog2 = (float)avg.
 *   7. TARGET.  target = clamp(((double)keyLog2 - avg) + (double)compensation, minLog2Exposure, maxLog2Exposure), the clamp being
 *      min(max(x, lo), hi).  targetLog2 = (float)target.
 *   8. ADAPTATION.  cur is a double of the device state.  On the first valid call after creation, after ptx_resize or after
 *      ptx_meter_reset: cur = target.  Otherwise rate = speedUp if target > cur, else speedDown;
 *      a = 1 - exp2(max(((-(double)deltaSeconds) (double)rate) 1.4426950408889634, -300)); cur = cur + (target - cur) a, and
 *      cur = target where a = 1 (the rounded sum cur + (target - cur) can miss target by an ulp).
 *      log2Exposure = (float)cur.  exposure = (float)exp2(clamp(cur, -300, 300)).
 *   9. STATE.  The result, the 256 bins and cur live in device memory, allocated by the first accepted call.  ptx_meter is
 *      asynchronous on the render stream and never synchronises: two launches, the second a single workgroup.
 * Consequences: (a) the exposure is quantised to sub-bin centres: a constant image is off by at most 1.0625 = 6.25 %, the width of
 * the widest sub-bin over its centre, and nothing else in the stage is approximate; (b) deltaSeconds = 0 leaves cur where it is;
 * (c) a deltaSeconds large enough for a = 1 (deltaSeconds rate >= 38) lands on the target exactly.
 * PTX_ERROR_INVALID_ARGUMENT: a NULL argument, an unknown source or mode, totalSamples = 0, lowPermille + highPermille >= 1000, a
 * float field that is not finite, minLog2Exposure > maxLog2Exposure, a negative speed or deltaSeconds, flags != 0, reserved != 0.
 * PTX_ERROR_NOT_READY: no image (ptx_resize), a shard accumulation buffer bound, a tile shard with worldSize > 1.  Then, against the
 * extent, PTX_ERROR_INVALID_ARGUMENT: in PTX_METER_REGION x0 >= x1, y0 >= y1, x1 > W or y1 > H; the bound of step 4.  Last,
 * PTX_ERROR_NOT_READY: a source that does not exist since the last ptx_resize (no C, no D).  A refused call leaves the state and the
 * bins intact; ptx_resize resets the state.
 * Known limits: the quantisation of (a); the range is fixed at 32 octaves; sharded frames are refused (a host can still sum bins256
 * across ranks itself); there is no perceptual model: no scotopic shift, and no local adaptation in the meter itself (that is
 * ptx_local_exposure's part, below). */
PTX_API int ptx_meter(PtxRenderer *r, const PtxMeterDesc *desc);
/* The result and, where bins256 is not NULL, the 256 bins of the last ptx_meter, device -> host; synchronous, as ptx_read_output is.
 * PTX_ERROR_INVALID_ARGUMENT: a NULL handle or result; PTX_ERROR_NOT_READY: no accepted ptx_meter on this handle yet. */
PTX_API int ptx_read_meter(PtxRenderer *r, PtxMeterResult *out, uint32_t *bins256 /* may be NULL */);
/* ... or the PtxMeterResult's device address (NULL before the first accepted ptx_meter); it stays where it is until ptx_destroy. */
PTX_API void *ptx_device_meter_ptr(PtxRenderer *r);
/* The state becomes what ptx_resize leaves: exposure 1, log2Exposure 0, everything else zero, and the next valid ptx_meter jumps to
 * its target instead of adapting.  Asynchronous on the render stream; PTX_OK and nothing to do before the first ptx_meter.
 * PTX_ERROR_INVALID_ARGUMENT: a NULL handle. */
PTX_API int ptx_meter_reset(PtxRenderer *r);
/* The output stage on `source` (PTX_METER_*: ptx_postprocess, ptx_postprocess_despiked or ptx_postprocess_denoised, with that call's
 * TotalSamples convention) with Exposure = uniform->Exposure * exposure, the float product, `exposure` being read from the device
 * state inside the first kernel: no synchronisation, no read-back.  Everything behind that kernel is the existing chain, and
 * ptx_read_output and ptx_present follow unchanged.  With a reset state exposure is 1 and the call gives the plain call's bits.
 * PTX_ERROR_INVALID_ARGUMENT: a NULL argument, an unknown mode or source; PTX_ERROR_NOT_READY: as the plain call of that source,
 * or no accepted ptx_meter on this handle yet. */
PTX_API int ptx_postprocess_metered(PtxRenderer *r, const PtxPostProcessingUniformData *u, uint32_t toneMappingMode, uint32_t source);

/* ------------------------------------------------------------------------- */
/* Display transform (docs/NEXT_ROWS.md section 22): a colour matrix, an ASC   */
/* CDL grade, a choice of tone curves and a 3-D LUT in the place of the output */
/* stage's last step.  An addition: every call above computes what it computed */
/* before, and a host that never calls these allocates nothing for them.       */
/* ------------------------------------------------------------------------- */

enum {
    PTX_CURVE_REFERENCE = 0, /* toneMapping.comp's 1 - exp(-c) */
    PTX_CURVE_REINHARD = 1,  /* extended Reinhard with a white point */
    PTX_CURVE_HABLE = 2,     /* Hable's filmic curve, exposure bias 2, white 11.2 */
    PTX_CURVE_ACES_FIT = 3   /* Hill's fit of the ACES RRT + ODT */
};
enum {
    PTX_GRADE_USE_LUT = 1u,        /* step 4 runs, on the LUT of ptx_grade_lut */
    PTX_GRADE_LUT_SRGB_DOMAIN = 2u /* the LUT is indexed by, and holds, sRGB-encoded values; needs PTX_GRADE_USE_LUT */
};

/* The constants of step 3, written once: the curves of csrc/pt_grade.hpp read these macros. */
#define PTX_HABLE_A 0.15f
#define PTX_HABLE_B 0.50f
#define PTX_HABLE_C 0.10f
#define PTX_HABLE_D 0.20f
#define PTX_HABLE_E 0.02f
#define PTX_HABLE_F 0.30f
#define PTX_HABLE_EXPOSURE_BIAS 2.0f
#define PTX_HABLE_WHITE 11.2f
#define PTX_ACES_IN { 0.59719f, 0.35458f, 0.04823f, 0.07600f, 0.90834f, 0.01566f, 0.02840f, 0.13383f, 0.83777f }       /* rows */
#define PTX_ACES_OUT { 1.60475f, -0.53108f, -0.07367f, -0.10208f, 1.10813f, -0.00605f, -0.00327f, -0.07276f, 1.07602f } /* rows */
#define PTX_ACES_A 0.0245786f
#define PTX_ACES_B 0.000090537f
#define PTX_ACES_C 0.983729f
#define PTX_ACES_D 0.4329510f
#define PTX_ACES_E 0.238081f
#define PTX_GRADE_LUT_MIN_SIZE 2u
#define PTX_GRADE_LUT_MAX_SIZE 65u

typedef struct PtxGradeDesc {
    float    colourMatrix[9];   /* row-major, applied to scene-linear RGB */
    float    slope[3], offset[3], power[3];   /* ASC CDL */
    float    saturation;
    uint32_t curve;             /* PTX_CURVE_REFERENCE | _REINHARD | _HABLE | _ACES_FIT */
    float    whitePoint;        /* PTX_CURVE_REINHARD only */
    uint32_t flags;             /* PTX_GRADE_USE_LUT, PTX_GRADE_LUT_SRGB_DOMAIN */
    uint32_t reserved;
} PtxGradeDesc;

/* ptx_grade: the display transform on what the last accepted ptx_postprocess / _denoised / _despiked / _metered left behind -- the
 * post-process image, bloom level 0 and that call's uniform, as ptx_present reads them -- into the image ptx_read_output reads, which
 * it overwrites: ptx_read_output follows unchanged in both formats.  Per pixel, all arithmetic float32 in the order written with no
 * contraction; every `/` is the specified division a * rcp(b), pow and exp the project's fixed kernels,
 * luminance (0.2126f r + 0.7152f g) + 0.0722f b, f16Round the rounding to binary16 of every store into an rgba16f image.
 *   0. COMPOSITION.  c = f16Round(bloom0 * (BloomIntensity * 0.1f) + post * 1.0f): composition.comp's store, the first half of
 *      ptx_postprocess's last kernel.  In ptx_present_graded c is the value after the scaling blit's f16Round (step 2 there).
 *   1. MATRIX.  m = colourMatrix.  c'_i = (m[3i] c.x + m[3i+1] c.y) + m[3i+2] c.z for i = 0, 1, 2; c = c'.
 *   2. CDL, v = c, per channel k:
 *      2a. SLOPE, OFFSET.  v_k = max(v_k slope_k + offset_k, 0), max(a, b) being a < b ? b : a (a NaN passes through).
 *      2b. POWER.          v_k = pow(v_k, power_k).
 *      2c. SATURATION.     Y = luminance(v); v_k = Y + (v_k - Y) saturation.
 *   3. CURVE, in PTX_TONE_MAPPING_SDR only (PTX_TONE_MAPPING_HDR skips steps 3 and 4, as the reference skips its own curve), per channel:
 *      PTX_CURVE_REFERENCE  v = 1 - exp(-v), ptx_postprocess's curve.
 *      PTX_CURVE_REINHARD   v = (v (1 + v / (w w))) / (1 + v), w = whitePoint.
 *      PTX_CURVE_HABLE      v = f(2 v) / f(11.2), f(x) = (x (A x + C B) + D E) / (x (A x + B) + D F) - E / F, A ... F = PTX_HABLE_A ... _F;
 *                           C B, D E, D F, E / F and f(11.2) are float32 values formed in that order.
 *      PTX_CURVE_ACES_FIT   t_i = (a[3i] v.x + a[3i+1] v.y) + a[3i+2] v.z with a = PTX_ACES_IN; per channel
 *                           t = (t (t + PTX_ACES_A) - PTX_ACES_B) / (t (PTX_ACES_C t + PTX_ACES_D) + PTX_ACES_E);
 *                           v_i = (o[3i] t.x + o[3i+1] t.y) + o[3i+2] t.z with o = PTX_ACES_OUT; v = min(max(v, 0), 1).
 *   4. LUT, with PTX_GRADE_USE_LUT; N and the table are ptx_grade_lut's, entry (r, g, b) at 3 ((b N + g) N + r):
 *      x_k = min(max(v_k, 0), 1) (a NaN passes through, and reads as 0 in the next line); with PTX_GRADE_LUT_SRGB_DOMAIN
 *      x_k = linearToSrgb(x_k) = x <= 0.0031308f ? 12.92f x : 1.055f pow(x, 1 / 2.4f) - 0.055f first.
 *      s_k = x_k (float)(N - 1); i_k = min((int)floor(s_k), N - 2), and 0 where s_k is a NaN; f_k = s_k - (float)i_k.
 *      Tetrahedral interpolation between V000 = LUT[i_r, i_g, i_b] and V111 = LUT[i_r + 1, i_g + 1, i_b + 1].  The order of the
 *      fractions is decided by >= comparisons in this order:
 *        f_r >= f_g:  f_g >= f_b -> rgb;  else f_r >= f_b -> rbg;  else brg.
 *        otherwise:   f_b >= f_g -> bgr;  else f_b >= f_r -> gbr;  else grb.
 *      An order "pqs" names f_hi = f_p, f_mid = f_q, f_lo = f_s; V_a is V000 stepped by one along p, V_b along p and q.
 *      out = ((V000 (1 - f_hi) + V_a (f_hi - f_mid)) + V_b (f_mid - f_lo)) + V111 f_lo, per channel of the entries.
 *      With PTX_GRADE_LUT_SRGB_DOMAIN out_k = srgbToLinear(out_k) = x <= 0.04045f ? x / 12.92f : pow((x + 0.055f) / 1.055f, 2.4f),
 *      these two divisions being IEEE quotients.  v = out.
 *   5. STORE.  f16Round(v), alpha 1.
 * SKIP RULE.  A step whose parameters are the identity bit for bit does not run, so it rounds nothing and clamps nothing: step 1 for the
 * identity matrix (1, 0, 0, 0, 1, 0, 0, 0, 1), step 2a for slope (1, 1, 1) and offset (+0, +0, +0) -- the max with 0 included --, step
 * 2b for power (1, 1, 1), step 2c for saturation 1.  The host decides; the kernel gets wave-uniform switches.  An identity desc with
 * PTX_CURVE_REFERENCE and no LUT therefore gives ptx_postprocess's bits, and ptx_present_graded then gives ptx_present's.
 * The renderer keeps the accepted desc (not the mode); ptx_resize keeps it, and the LUT.  Asynchronous on the render stream; works
 * on a borrower; touches neither the sum nor any image of the chain.
 * Refusals, in this order; a refused call leaves the output image, the kept desc and the LUT intact.  PTX_ERROR_INVALID_ARGUMENT: a
 * NULL argument; an unknown curve, mode or flag bit; reserved != 0; a float field that is not finite; a negative slope, power or
 * saturation; whitePoint <= 0 with PTX_CURVE_REINHARD; PTX_GRADE_LUT_SRGB_DOMAIN without PTX_GRADE_USE_LUT.  PTX_ERROR_NOT_READY: nothing
 * post-processed since the last ptx_resize; a shard accumulation buffer bound, or a tile shard with worldSize > 1; PTX_GRADE_USE_LUT
 * with no LUT set.
 * Known limits: the curves are fixed-parameter fits, no AgX and no full ACES RRT; the LUT has no 1-D shaper in front, so a linear-domain
 * LUT spends its lattice on the highlights (PTX_GRADE_LUT_SRGB_DOMAIN is the remedy); the 8-bit encodes are not dithered; the grade is
 * global, there is no local tone mapping; sharded frames are refused. */
PTX_API int ptx_grade(PtxRenderer *r, const PtxGradeDesc *d, uint32_t toneMappingMode);
/* The LUT of step 4: size^3 RGB entries of float32, red fastest, copied into a device buffer owned by the handle (synchronous, as
 * ptx_write_accumulation is); rgb = NULL clears it and frees the buffer, whatever `size` is.  The LUT belongs to the display, not to
 * the render extent: ptx_resize keeps it.  PTX_ERROR_INVALID_ARGUMENT: a NULL handle; size outside PTX_GRADE_LUT_MIN_SIZE ...
 * PTX_GRADE_LUT_MAX_SIZE (2 ... 65) with rgb != NULL.  The values are not inspected. */
PTX_API int ptx_grade_lut(PtxRenderer *r, uint32_t size, const float *rgb /* size^3 * 3, red fastest; NULL clears */);
/* ptx_present with the kept desc of the last accepted ptx_grade applied, steps 1 - 5 above with desc->toneMappingMode, in the place
 * of the tone mapping between the scaling blit and the UI composition (step 3 of the screen path).  A function of its own and not a
 * flag of ptx_present, whose unknown flag bits stay refused.  Arguments, result and refusals are ptx_present's; in addition
 * PTX_ERROR_NOT_READY: a tile shard with worldSize > 1; no accepted ptx_grade on this handle yet; the kept desc has PTX_GRADE_USE_LUT
 * and the LUT has been cleared. */
PTX_API int ptx_present_graded(PtxRenderer *r, const PtxPresentDesc *desc);

/* ------------------------------------------------------------------------- */
/* Local exposure (docs/NEXT_ROWS.md section 23): a bilateral grid over the    */
/* log of the luminance gives every pixel a gain that compresses the scene's   */
/* contrast and leaves local detail alone.  An addition: every call above      */
/* computes what it computed before, and a host that never calls these         */
/* allocates nothing for them.                                                 */
/* ------------------------------------------------------------------------- */

enum {
    PTX_LOCAL_EXPOSURE_PIVOT_METERED = 1u /* the pivot is a display luminance: the meter state's cur is subtracted from pivotLog2 on the device */
};

typedef struct PtxLocalExposureDesc {
    uint32_t source;            /* PTX_METER_SUM / _DESPIKED / _DENOISED, with ptx_meter's totalSamples convention */
    uint32_t totalSamples;      /* > 0 */
    uint32_t cellShift;         /* 3 ... 6: a grid cell is 2^cellShift x 2^cellShift pixels */
    float    pivotLog2;         /* log2 of the display luminance the base is compressed towards (log2(0.18)) */
    float    highlightContrast; /* 0 ... 2, finite: slope of the base above the pivot; 1 = untouched */
    float    shadowContrast;    /* 0 ... 2, finite: ... below it */
    float    maxStops;          /* >= 0, finite: |log2 gain| is clamped to it */
    uint32_t flags;             /* PTX_LOCAL_EXPOSURE_PIVOT_METERED or 0 */
    uint32_t reserved;          /* 0 */
} PtxLocalExposureDesc;

/* ptx_local_exposure computes G, an R32F image of the render extent W x H.  p = (x, y) is a pixel, s = cellShift.  Everything is
 * integer up to one float64 division; the float64 operations are IEEE operations in the order written with no contraction, and exp2 is
 * the project's specified kernel, so a reference in integers and doubles reproduces G bit for bit.
 *   1. LUMINANCE AND CLASSES.  Exactly ptx_meter's steps 1 and 2: c(p) = source(p).rgb / (float)totalSamples (one rcp, three
 *      multiplies; PTX_METER_DENOISED: 1 stands for totalSamples), Y(p) = (0.2126f c.r + 0.7152f c.g) + 0.0722f c.b; REJECTED iff Y is
 *      not finite, BLACK iff Y <= 0 or Y < 2^-126, COUNTED otherwise.
 *   2. FIXED-POINT LOG.  For a counted pixel l = clamp((int)(bits(Y) >> 15) - 888 * 32, 0, 8191): the eight exponent bits and the top
 *      eight mantissa bits, 256 steps per octave over [2^-16, 2^16).  l / 256 - 16 is the piecewise-linear log2 e + m of
 *      Y = (1 + m) 2^e, which lies at most 0.0861 below log2 Y and is smooth within an octave, with m cut to eight bits: less than
 *      1 / 256 further below.
 *   3. SPLAT.  The grid has nx = ceil(W / 2^s) by ny = ceil(H / 2^s) cells and 32 slices.  Every counted pixel adds l to
 *      sum[cy][cx][z] and 1 to cnt[cy][cx][z] with cx = x >> s, cy = y >> s, z = l >> 8.  Both arrays are uint32.
 *   4. BLUR.  One 1-2-1 pass along each of x, y and z over both arrays, clamp to edge: the edge cell stands in for the missing
 *      neighbour, so the weights of the three passes always sum to 64.  Integer arithmetic, nothing is divided.  A cell holds at most
 *      4096 pixels, so a blurred sum is at most 4096 * 8191 * 64 = 2,147,221,504 < 2^32.
 *   5. SLICE, for a counted pixel.  Along x: u = 2x + 1 - 2^s.  If u < 0 both taps are cell 0 and fx = 0; otherwise cx0 = u >> (s + 1),
 *      fx = u & (2^(s+1) - 1), cx1 = min(cx0 + 1, nx - 1); the weights are wx0 = 2^(s+1) - fx and wx1 = fx.  y is the same with ny.
 *      Along z: v = 2l + 1 - 256; if v < 0 both taps are slice 0 and fz = 0; otherwise z0 = v >> 9, fz = v & 511, z1 = min(z0 + 1, 31);
 *      weights 512 - fz and fz.  N = SUM wx wy wz sum and D = SUM wx wy wz cnt over the eight taps of the blurred arrays, in uint64
 *      (at most 2^54).  The pixel's own cell and slice carry a positive weight, so D > 0.  B = (double)N / (double)D / 256 - 16.
 *   6. GAIN.  pv = (double)pivotLog2; with PTX_LOCAL_EXPOSURE_PIVOT_METERED pv = pv - cur, cur being the double of the meter's device
 *      state (ptx_meter step 8), read on the device: no synchronisation.  d = B - pv; c = d > 0 ? highlightContrast : shadowContrast;
 *      g = clamp(((double)c - 1) d, -maxStops, maxStops), the clamp being min(max(x, lo), hi), and then clamp(g, -300, 300), the domain
 *      of exp2.  G(p) = (float)exp2(g).  A BLACK or REJECTED pixel gets G(p) = 1.
 *   7. OUTPUT.  ptx_postprocess_local is the output call of `source` with one change: its first kernel uses, per pixel,
 *      Exposure_p = (u->Exposure * m) * G(p), float products in that order; m is the metered exposure read on the device when
 *      `metered` is 1 and exactly 1.0f when it is 0.  Everything behind that kernel is the existing chain: bloom, composition,
 *      ptx_read_output, ptx_grade, ptx_present.
 * Consequences: (a) both contrasts at 1 give G = 1 everywhere, and with metered = 0 ptx_postprocess_local then gives the plain call's
 * bits; (b) on a constant counted image B = l / 256 - 16 exactly, so G is one known value everywhere; (c) multiplying the source by a
 * power of two shifts B by that many stops exactly, short of the range's ends; (d) two plateaus at least three octaves apart share no
 * slice after the blur and the slice, so each gets its own constant gain right up to the edge: no halo; (e) the approximate log
 * moves the gain by at most |c - 1| * (0.0861 + 1 / 256) stops against the exact one, smoothly: 0.0861 for the piecewise-linear
 * log, 1 / 256 for its eight bits.
 * Asynchronous on the render stream: three launches, no global atomics, nothing to zero between calls.  Works on a borrower; touches
 * neither the sum nor any image of the chain.
 * Refusals, in this order; a refused call leaves G intact.  PTX_ERROR_INVALID_ARGUMENT: a NULL argument, an unknown source,
 * totalSamples = 0, cellShift outside 3 ... 6, an unknown flag bit, reserved != 0; a float field that is not finite, a contrast outside
 * 0 ... 2, maxStops < 0.  PTX_ERROR_NOT_READY: no image (ptx_resize), a shard accumulation buffer bound, a tile shard with
 * worldSize > 1; a source that does not exist since the last ptx_resize (no C, no D); PTX_LOCAL_EXPOSURE_PIVOT_METERED without an
 * accepted ptx_meter on this handle.  ptx_resize drops G and the grid.
 * Known limits: there is no detail-strength control (the approximate log would print its sawtooth into the image); the pass count is
 * fixed at one; the range is fixed at 32 octaves; sharded frames are refused. */
PTX_API int ptx_local_exposure(PtxRenderer *r, const PtxLocalExposureDesc *desc);
/* G of the last accepted ptx_local_exposure, device -> host: width * height * 4 bytes, row-major; synchronous, as ptx_read_output is.
 * PTX_ERROR_INVALID_ARGUMENT: a NULL argument, another size; PTX_ERROR_NOT_READY: no accepted ptx_local_exposure since the last
 * ptx_resize. */
PTX_API int ptx_read_local_exposure(PtxRenderer *r, void *host, size_t bytes);
/* ... or its device address (NULL without one); it stays where it is until the next ptx_resize. */
PTX_API void *ptx_device_local_exposure_ptr(PtxRenderer *r);
/* Step 7.  PTX_ERROR_INVALID_ARGUMENT: a NULL argument, an unknown mode or source, metered > 1; PTX_ERROR_NOT_READY: as the plain call
 * of that source; metered = 1 without an accepted ptx_meter; no accepted ptx_local_exposure since the last ptx_resize; a tile shard
 * with worldSize > 1. */
PTX_API int ptx_postprocess_local(PtxRenderer *r, const PtxPostProcessingUniformData *u, uint32_t toneMappingMode,
                                  uint32_t source, uint32_t metered /* 0 or 1 */);

/* ------------------------------------------------------------------------- */
/* Enlarging screen path (docs/NEXT_ROWS.md section 25): a host that renders   */
/* below the window's extent gets a clamped bicubic enlargement and a clamped  */
/* unsharp mask where ptx_present has the reference's linear blit.  An         */
/* addition: every call above computes what it computed before, and a host     */
/* that never calls this allocates nothing for it.                             */
/* ------------------------------------------------------------------------- */

enum { PTX_UPSCALE_CATMULL_ROM = 0 };
enum { PTX_UPSCALE_GRADED = 1u };   /* the kept desc of the last accepted ptx_grade stands where the tone mapping stands */
typedef struct PtxUpscaleDesc {
    uint32_t filter;    /* PTX_UPSCALE_CATMULL_ROM */
    float    sharpness; /* 0 ... 2, finite; +0 skips step 5 */
    uint32_t flags;     /* PTX_UPSCALE_GRADED or 0 */
    uint32_t reserved;  /* 0 */
} PtxUpscaleDesc;

/* ptx_present_upscaled writes the image ptx_present writes -- ptx_read_present, ptx_device_present_ptr, ptx_present_bytes and ptx_resize
 * behave as after ptx_present -- from the same inputs: the post-process image, bloom level 0 and the uniform of the last accepted output
 * call.  It only enlarges: the screen extent SW x SH is at least the render extent W x H on both axes (a smaller window is
 * ptx_present's).  Per screen pixel (sx, sy) and colour channel, all arithmetic float32 in the order written with no contraction; every
 * `/` is the specified division a * rcp(b); f16Round is the rounding to binary16 of every store into an rgba16f image; min and max
 * are spelled out as selections, so what a NaN or an infinity does is part of the text.
 *   1. COMPOSED TEXEL.  T(x, y) = f16Round(bloom0 * (BloomIntensity * 0.1f) + post * 1.0f) at render pixel (x, y): step 1 of the screen
 *      path, composition.comp's store, unchanged.
 *   2. AXIS SET-UP, for x (y is the same with sy, H, SH):  x = ((float)sx + 0.5f) * ((float)W / (float)SW) - 0.5f; x0 = floor(x);
 *      t = x - x0.  Taps i_k = (uint32_t)min(max(x0 + (float)k, 0), (float)(W - 1)) for k = -1, 0, 1, 2 (clamp to edge).  Weights
 *        w0 = ((-0.5f t + 1.0f) t - 0.5f) t        w1 = ((1.5f t - 2.5f) t) t + 1.0f
 *        w2 = ((-1.5f t + 2.0f) t + 0.5f) t        w3 = ((0.5f t - 0.5f) t) t
 *      (Catmull-Rom).  An axis whose two extents are equal is NOT filtered: one texel, no arithmetic -- ptx_present's rule, for
 *      ptx_present's reason (W * rcp(W) is not 1 for every W).
 *   3. ROW PASS, on each of the source rows j_k the y taps name:
 *        a = ((T(i_-1, j) w0 + T(i_0, j) w1) + T(i_1, j) w2) + T(i_2, j) w3;
 *        lo = T(i_1, j) < T(i_0, j) ? T(i_1, j) : T(i_0, j);   hi = T(i_0, j) < T(i_1, j) ? T(i_1, j) : T(i_0, j);
 *        a = a >= lo ? a : lo;  then  a = a <= hi ? a : hi      (a NaN becomes lo).
 *      R(j) = a, not rounded.  On an unfiltered x axis R(j) = T(sx, j).
 *   4. COLUMN PASS.  The same expression and the same two selections over R(j_-1) ... R(j_2) with the y weights, lo and hi from R(j_0)
 *      and R(j_1) as above from T(i_0) and T(i_1); on an unfiltered y axis the value is R(sy).  S = f16Round(that value): the screen
 *      image after the enlargement.  The clamp is per axis on purpose: one clamp against the 2 x 2 central texels jumps where floor()
 *      flips, per axis S is continuous in t.  S lies within the range of the four central texels (an anti-ringing clamp: a 5000-valued
 *      marker pixel or an emitter does not ring), and a constant image comes through exactly.
 *   5. SHARPEN, skipped when sharpness is +0.0f bit for bit (the host decides; the kernel gets a wave-uniform switch).  c = S(sx, sy);
 *      N = S(sx, sy - 1), Sd = S(sx, sy + 1), Wt = S(sx - 1, sy), E = S(sx + 1, sy), coordinates clamped to the screen's edge.
 *        m = ((N + Sd) + (Wt + E)) * 0.25f;   v = c + (c - m) * sharpness;
 *        lo = c, hi = c, then for q = N, Sd, Wt, E in that order:  lo = q < lo ? q : lo;  hi = hi < q ? q : hi;
 *        v = v >= lo ? v : lo;  then  v = v <= hi ? v : hi;   S' = f16Round(v).
 *      A channel whose c is not finite passes through: S' = c.  The mask steepens edges and cannot leave the five-tap range, so it
 *      adds no halo, and a local extremum stays as it is.
 *   6. TONE OR GRADE, UI, HDR10, STORE.  ptx_present's steps from the tone mapping on, on S' (S without step 5): toneMapping.comp with
 *      desc->toneMappingMode, or under PTX_UPSCALE_GRADED steps 1 - 5 of ptx_grade with the kept desc, as in ptx_present_graded; then
 *      uiComposition.comp, the HDR10 encode, the store in desc->format.  The UI image is not scaled.
 * SKIP RULE.  With SW = W, SH = H and sharpness +0 the call enqueues exactly what ptx_present (ptx_present_graded) enqueues.
 * Asynchronous on the render stream, one launch; works on a borrower; touches neither the sum nor ptx_read_output's image.
 * Refusals, in this order; a refused call leaves the present image intact.  (1) PTX_ERROR_INVALID_ARGUMENT: everything ptx_present
 * refuses about desc, in its order.  (2) PTX_ERROR_INVALID_ARGUMENT: a NULL up; filter != PTX_UPSCALE_CATMULL_ROM; an unknown flag
 * bit; reserved != 0; a sharpness that is not finite, < 0 or > 2.  (3) PTX_ERROR_NOT_READY: ptx_present's refusals, and under
 * PTX_UPSCALE_GRADED ptx_present_graded's.  (4) PTX_ERROR_INVALID_ARGUMENT: desc->width < W or desc->height < H.
 * Known limits: one filter; the UI is not scaled; no temporal super-resolution and no jittered history; the default sharpness of the
 * layers above (0.5) has not been tuned by anybody; sharded frames are refused under PTX_UPSCALE_GRADED as everywhere behind ptx_grade. */
PTX_API int ptx_present_upscaled(PtxRenderer *r, const PtxPresentDesc *desc, const PtxUpscaleDesc *up);

/* ------------------------------------------------------------------------- */
/* Noise metering (docs/NEXT_ROWS.md section 26): two half-sums of an offline  */
/* render give an error estimate per tile, on the device and in the units of   */
/* the displayed mean, so that a render stops on a noise threshold and not on  */
/* a sample count.  An addition: every call above computes what it computed    */
/* before, and a host that never calls these allocates nothing for them.       */
/* ------------------------------------------------------------------------- */

enum { PTX_NOISE_WRITE_SUM = 1u }; /* step 1 stores S = A + B to the internal accumulation image */

typedef struct PtxNoiseDesc {
    uint32_t samplesA, samplesB; /* samples summed in half 0 / half 1, each 1 .. 2^24 */
    float    exposure;           /* the output stage's Exposure: the error is measured on mean * exposure */
    float    threshold;          /* a tile is converged iff its error <= threshold */
    uint32_t tileShift;          /* tiles of 2^tileShift pixels a side, 3 .. 6 */
    uint32_t flags;              /* PTX_NOISE_WRITE_SUM */
    uint32_t reserved[2];
} PtxNoiseDesc;

typedef struct PtxNoiseResult {
    float    meanError, maxError;
    uint32_t tilesX, tilesY, converged;   /* tiles whose error <= threshold */
    uint32_t counted, black, rejected;    /* pixels */
    uint32_t valid, calls;
} PtxNoiseResult;

/* The two halves.  enable = 1 makes and zeroes two width * height * 16-byte images owned by the handle (asynchronous on the render
 * stream; where they exist already they are zeroed again); enable = 0 releases them and returns the binding to the internal image if
 * one of them was bound.  They belong to the extent: ptx_resize drops them, as it already unbinds.  The host binds them with the
 * existing ptx_bind_accumulation(r, ptx_device_noise_half_ptr(r, which), ptx_accum_bytes(r)): ptx_render, ptx_render_frames (a block of
 * frames into whichever half is bound), ptx_reset_accumulation, ptx_write_accumulation and ptx_readback then act on the bound half as
 * they do on any bound buffer, unchanged.  The accumulation image is a kernel argument of the launch that adds a frame's samples, on
 * the handle's stream, and the random numbers are a function of pixel, width and frame alone: a host that binds half 0 before its even
 * render calls and half 1 before its odd ones gets two independent sums, each bit for bit what a handle of its own would have
 * accumulated from those frames, with no kernel touched.
 * PTX_ERROR_INVALID_ARGUMENT: a NULL handle, enable > 1.  PTX_ERROR_NOT_READY: enable = 1 before ptx_resize. */
PTX_API int ptx_noise_halves(PtxRenderer *r, uint32_t enable);
/* The device address of half `which` (0 / 1); NULL when there are none, for a NULL handle and for which > 1. */
PTX_API void *ptx_device_noise_half_ptr(PtxRenderer *r, uint32_t which);
/* ptx_noise_meter.  W x H is the render extent, p = (x, y) a pixel, A(p) the float4 of half 0 and B(p) that of half 1.  All arithmetic
 * is float32 in the order written with no contraction; rcp, sqrt and the division a / b = a * rcp(b) are the project's specified
 * kernels, rcp being the correctly rounded 1 / x on every argument met here; fmin(a, b) = b < a ? b : a.  The
 * integers are exact and the two float64 divisions are IEEE.
 *   1. SUM.  S = A + B, component by component, alpha included.  With PTX_NOISE_WRITE_SUM, S is stored to the handle's internal
 *      accumulation image, the image ptx_bind_accumulation(NULL) selects.  The binding is not changed.  This is what the output stage
 *      and the chain read afterwards, so no existing call needs to know about halves.
 *   2. SCALE FACTORS.  sa = exposure * rcp((float)samplesA), sb likewise from samplesB, st = exposure * rcp((float)(samplesA + samplesB)).
 *   3. SCALED VALUES.  a = A.rgb * sa, b = B.rgb * sb, c = S.rgb * st.  D = (|a.r - b.r| + |a.g - b.g|) + |a.b - b.b|.
 *      m = (c.r + c.g) + c.b.
 *   4. CLASSES.  REJECTED iff any of the six input colour values, D or m is not finite.  BLACK iff not rejected and not (m >= 2^-20):
 *      zeros, negatives and everything near the denormals.  COUNTED = not rejected; black pixels count with error 0.
 *   5. PER-PIXEL ERROR.  For a counted pixel that is not black e = fmin(0.5f * (D / sqrt(m)), 255.0f) and q = (uint32_t)(e * 65536.0f),
 *      truncated, so q < 2^24.  Black pixels have q = 0.  e is the per-pixel term of Dammertz, Hanika, Keller and Lensch, "A hierarchical
 *      automatic stopping condition for Monte Carlo global illumination" (2010): |I - A| / sqrt(I) with A the image of half the samples.
 *      With equal halves it estimates the standard error of the pixel's mean over the square root of its value.
 *   6. PER TILE.  A tile is the pixels with x >> tileShift and y >> tileShift equal; ragged tiles lie at the right and bottom edges;
 *      tilesX = ceil(W / 2^tileShift), tilesY likewise.  Q_t = SUM q in uint64, n_t = the counted pixels of the tile.
 *      E_t = n_t ? (float)((double)Q_t / ((double)n_t * 65536.0)) : 0.  The tile is converged iff E_t <= threshold.
 *   7. RESULT.  maxError = max E_t.  meanError = (float)((double)SUM Q_t / ((double)SUM n_t * 65536.0)).  counted = SUM n_t, black and
 *      rejected the pixels of those classes (black ones are in counted too), converged the number of converged tiles.  valid = 0 with
 *      both errors 0 when SUM n_t = 0, and 1 otherwise.  calls counts accepted calls since creation or ptx_resize.  All sums are
 *      integers, so there is no order for the result to depend on.
 * Asynchronous on the render stream, two launches, the second a single workgroup; it never synchronises, has no global atomics and
 * nothing to zero between calls.  It needs no scene and so works on a borrower of a shared one.  The result, the tile map and the
 * other state are allocated by the first accepted call.
 * Refusals, in this order; a refused call leaves the state, the tile map and the internal image intact.  PTX_ERROR_INVALID_ARGUMENT:
 * a NULL argument; a sample count of 0 or above 2^24; tileShift outside 3 ... 6; unknown flag bits; reserved != 0; an exposure or
 * threshold that is not finite; exposure <= 0; threshold < 0.  PTX_ERROR_NOT_READY: no image (ptx_resize); a shard accumulation buffer
 * bound; a tile shard with worldSize > 1; no halves.
 * Known limits: S = A + B is not the bits of one sum accumulated in frame order; unequal halves bias e; the criterion is per tile, with
 * no hierarchy; sharded frames are refused; this call does no adaptive sampling itself: ptx_adaptive_plan (below) steers a render by its
 * tile records. */
PTX_API int ptx_noise_meter(PtxRenderer *r, const PtxNoiseDesc *desc);
/* The result of the last accepted ptx_noise_meter and, where tileErrors is not NULL, its tile map: tilesX * tilesY floats E_t,
 * row-major, `bytes` being exactly their size (with tileErrors NULL `bytes` is not read).  Synchronous, as ptx_read_output is.
 * PTX_ERROR_INVALID_ARGUMENT: a NULL handle or result.  PTX_ERROR_NOT_READY: no accepted ptx_noise_meter since creation or the last
 * ptx_resize.  PTX_ERROR_INVALID_ARGUMENT: a `bytes` that does not match. */
PTX_API int ptx_read_noise(PtxRenderer *r, PtxNoiseResult *out, float *tileErrors /* may be NULL */, size_t bytes);

/* ------------------------------------------------------------------------- */
/* Adaptive sampling (docs/NEXT_ROWS.md section 27): the noise meter's tile    */
/* records, or a mask of the host's, become the list of tiles the next render  */
/* calls cover, and the frames every tile has received are counted per half.   */
/* An addition: every call above computes what it computed before, and a host  */
/* that never calls these allocates nothing for them.                          */
/* ------------------------------------------------------------------------- */

enum { PTX_ADAPTIVE_FROM_NOISE = 0u, PTX_ADAPTIVE_FROM_MASK = 1u }; /* PtxAdaptiveDesc::source */

typedef struct PtxAdaptiveDesc {
    uint32_t       tileShift;        /* tiles of 2^tileShift pixels a side, 3 .. 6 */
    uint32_t       source;           /* PTX_ADAPTIVE_FROM_NOISE / PTX_ADAPTIVE_FROM_MASK */
    const uint8_t *mask;             /* FROM_MASK: tilesX * tilesY bytes of the host's, row-major, copied in; else not read */
    uint32_t       dilate;           /* 0 .. 2: the margin around the seeds, in tiles */
    uint32_t       framesA, framesB; /* frames rendered into half 0 / half 1 under the plan being replaced, each 0 .. 2^24 */
    uint32_t       flags;            /* none defined: 0 */
    uint32_t       reserved[2];
} PtxAdaptiveDesc;

typedef struct PtxAdaptivePlan {
    uint32_t tilesX, tilesY;
    uint32_t activeTiles, activePixels; /* the list's length, and the pixels inside the image of its tiles */
    uint32_t seedTiles;
    uint32_t generation;                /* accepted ptx_adaptive_plan calls since the counts were made */
} PtxAdaptivePlan;

typedef struct PtxAdaptiveMeterDesc {
    uint32_t pendingA, pendingB; /* frames rendered into half 0 / half 1 under the plan in force, not committed yet, each 0 .. 2^24 */
    uint32_t normalizeTo;        /* PTX_NOISE_WRITE_SUM stores every tile's sum scaled to this many samples, 1 .. 2^25 */
    float    exposure;           /* as PtxNoiseDesc's */
    float    threshold;
    uint32_t tileShift;          /* the counts' own */
    uint32_t flags;              /* PTX_NOISE_WRITE_SUM */
    uint32_t reserved[2];
} PtxAdaptiveMeterDesc;

/* ptx_adaptive_plan.  W x H is the render extent; tiles are ptx_noise_meter's (step 6): tile t = ty * tilesX + tx holds the pixels with
 * x >> tileShift = tx and y >> tileShift = ty, tilesX = ceil(W / 2^tileShift), tilesY likewise, ragged tiles at the right and bottom
 * edges.  The handle keeps two counts per tile, countA[t] and countB[t] (uint32): the frames the tile has received in half 0 and in
 * half 1.  They are made and zeroed by the first accepted call, zeroed again by ptx_noise_halves(1), and dropped with the plan by
 * ptx_resize, by a ptx_set_tile_shard that changes the shard and by ptx_noise_halves(0).  One launch of one workgroup on the render
 * stream, integers only:
 *   1. COMMIT.  For every tile t active in the plan being replaced, countA[t] += framesA and countB[t] += framesB: the frames the
 *      host rendered into half 0 and half 1 under that plan.  With no plan in force every tile counts as active: this is how uniform
 *      warm-up frames enter the counts.
 *   2. SEED AND DILATE.  PTX_ADAPTIVE_FROM_NOISE: t is a seed iff the tile record of the last accepted ptx_noise_meter or
 *      ptx_noise_meter_adaptive marks it not converged.  PTX_ADAPTIVE_FROM_MASK: t is a seed iff mask[t] != 0.  A tile is active iff
 *      some seed lies within Chebyshev distance `dilate` of it: max(|tx - sx|, |ty - sy|) <= dilate, in tiles.  The margin keeps a
 *      seam from forming between a frozen tile and a neighbour that is still refined.
 *   3. COMPACT.  The ids of the active tiles are written to a device list in ascending order, by a scan; the order is part of the
 *      contract and no atomic's arrival order can show in it.  activeTiles is its length, activePixels the pixels of its tiles that
 *      lie inside the image (a ragged tile counts less), seedTiles the number of seeds.
 * The list is unique and sorted by construction and no call takes a list from the host, so two slots never own one pixel.
 * While a plan is in force ptx_render and ptx_render_frames cover the listed tiles only, in tiles of 2^tileShift pixels: a pixel of
 * an active tile receives, bit for bit, what the unplanned call would have added to it (the random numbers are a function of pixel,
 * width and frame alone), every other pixel keeps its bits, and PtxStats::pathSamples is activePixels * frames * SampleCount plus
 * retries.  An empty plan (activeTiles = 0) renders and accumulates nothing.  ptx_render_guides and its kin, ptx_render_debug, the
 * shard calls and the output stage keep the whole frame.  ptx_bind_shard_accumulation with a buffer drops the plan, as
 * ptx_adaptive_clear does.
 * SYNCHRONOUS: the call ends with a read-back of *out, as ptx_read_noise does, because the host sizes the next launches by
 * activeTiles.  It needs no scene and so works on a borrower of a shared one.
 * Refusals, in this order, all before the first launch; a refused call leaves the plan, the counts and the list intact.
 * (1) PTX_ERROR_INVALID_ARGUMENT: a NULL handle, desc or out; tileShift outside 3 ... 6; a source other than the two; a flag bit;
 * reserved != 0; dilate > 2; framesA or framesB above 2^24; a NULL mask under PTX_ADAPTIVE_FROM_MASK.  (2) PTX_ERROR_NOT_READY: no
 * image (ptx_resize); a shard accumulation buffer bound; a tile shard with worldSize > 1.  (3) PTX_ERROR_NOT_READY: under
 * PTX_ADAPTIVE_FROM_NOISE no accepted meter call, or one of another tileShift.  (4) PTX_ERROR_NOT_READY: a tileShift that differs
 * from the counts' own while a count may be non-zero, or while a plan is in force and framesA or framesB is not 0 (with all counts
 * zero and nothing to commit the counts are made anew for the new tileShift).
 * Known limits: one workgroup builds the plan; the learnt bounce schedule is keyed on the slot count and so starts anew with every
 * plan; sharded frames are refused; counts are per tile, not per pixel. */
PTX_API int ptx_adaptive_plan(PtxRenderer *r, const PtxAdaptiveDesc *desc, PtxAdaptivePlan *out);
/* The plan in force, its list (activeTiles uint32 ids, ascending) and the counts (countA[0 .. numTiles), then countB[0 .. numTiles)).
 * `tiles` and `counts` may each be NULL, and then its byte count is not read; otherwise tileBytes is exactly activeTiles * 4 and
 * countBytes exactly 2 * tilesX * tilesY * 4.  With no plan in force (ptx_adaptive_clear) activeTiles, activePixels and seedTiles are
 * 0 and the list is empty.  Synchronous.  PTX_ERROR_INVALID_ARGUMENT: a NULL handle or out.  PTX_ERROR_NOT_READY: no counts (no
 * accepted ptx_adaptive_plan since they were last dropped).  PTX_ERROR_INVALID_ARGUMENT: a byte count that does not match. */
PTX_API int ptx_read_adaptive(PtxRenderer *r, PtxAdaptivePlan *out, uint32_t *tiles, size_t tileBytes, uint32_t *counts, size_t countBytes);
/* Drops the plan: render calls cover the frame again.  The counts stay.  PTX_ERROR_INVALID_ARGUMENT: a NULL handle. */
PTX_API int ptx_adaptive_clear(PtxRenderer *r);
/* ptx_noise_meter_adaptive: ptx_noise_meter on halves whose tiles have received different numbers of frames.  It shares
 * ptx_noise_meter's kernel bodies, writes the same state, and ptx_read_noise reads it.  It differs from ptx_noise_meter's steps so:
 *   COUNTS PER TILE.  NA_t = countA[t] + (active(t) ? pendingA : 0), NB_t likewise from countB and pendingB, N_t = NA_t + NB_t.
 *      active(t): t is in the plan in force; with no plan in force every tile is active.
 *   STEP 2 PER TILE.  sa_t = exposure * rcp((float)NA_t), sb_t = exposure * rcp((float)NB_t), st_t = exposure * rcp((float)N_t),
 *      and steps 3 - 5 of a pixel use its tile's factors.
 *   STEPS 3 - 7 are unchanged, with one exception: a tile with NA_t == 0 or NB_t == 0 has all its pixels REJECTED and is not
 *      converged, whatever E_t = 0 would say.  An unsampled tile never freezes.
 *   STEP 1 under PTX_NOISE_WRITE_SUM stores S where N_t == normalizeTo or N_t == 0, and S * k_t elsewhere,
 *      k_t = (float)normalizeTo * rcp((float)N_t), applied per component, alpha included.  ptx_postprocess with TotalSamples =
 *      normalizeTo then shows every tile's own mean; the output stage and the chain know nothing of halves or of counts.  The host
 *      passes the largest N_t: the frames of its render calls so far.
 * Asynchronous, two launches, as ptx_noise_meter.  Refusals, in this order; a refused call leaves the state, the tile map and the
 * internal image intact.  PTX_ERROR_INVALID_ARGUMENT: a NULL argument; pendingA or pendingB above 2^24; normalizeTo outside
 * 1 ... 2^25; tileShift outside 3 ... 6; unknown flag bits; reserved != 0; an exposure or threshold that is not finite; exposure <= 0;
 * threshold < 0.  PTX_ERROR_NOT_READY: ptx_noise_meter's, in its order; then no counts (call ptx_adaptive_plan first); then a
 * tileShift that differs from the counts' own. */
PTX_API int ptx_noise_meter_adaptive(PtxRenderer *r, const PtxAdaptiveMeterDesc *desc);

PTX_API int ptx_test_input_stride(uint32_t fn);
PTX_API int ptx_test_output_stride(uint32_t fn);
PTX_API int ptx_test_eval(PtxRenderer *r, uint32_t fn, const float *in, float *out, uint32_t n);

#ifdef __cplusplus
}
#endif
#endif /* PTX_H */
