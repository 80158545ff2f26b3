// pt_runtime.hpp -- host side of the HIP library: the renderer object behind a PtxRenderer handle (its state one struct per stage),
// the environment switches, createRenderer / destroyRenderer, the grid helpers, makeParams and the scene views, ptx_update_animation,
// ptx_get_stats and the ptx_test_* / ptx_trace_rays entry points.  The stages are host files of their own, included below in the
// order they build on one another: scene upload (pt_scene_host.hpp), the tree build (pt_bvh_host.hpp; kernels: pt_bvh_build.hpp),
// the render launches with the bounce schedule of the wavefront backend (pt_render_host.hpp), the frame's hand-over -- accumulation
// image, tile shards, read-back -- (pt_frame_host.hpp), the output stage and the screen path (pt_output_host.hpp), the interactive
// chain -- guide pass, temporal accumulation, the filters -- (pt_chain_host.hpp; its bookkeeping: pt_chain_state.hpp).  Their
// functions take a valid or null handle; include/ptx.h's entry points (ptx_capi.hip) are one-line wrappers around them.
// No CPU fallback exists: without a HIP device createRenderer fails.
#pragma once

#include <algorithm>
#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "pt_aux_kernels.hpp"
#include "pt_bc.hpp"
#include "pt_bvh_build.hpp"
#include "pt_chain_state.hpp"
#include "pt_debug_view.hpp"
#include "pt_denoise.hpp"
#include "pt_post.hpp"
#include "pt_present.hpp"
#include "pt_shard_layout.hpp"
#include "pt_stream_plan.hpp"
#include "pt_temporal.hpp"
#include "pt_variance.hpp"
#include "pt_responsive.hpp"

// =====================================================================================
// Host side: the renderer object behind the C-ABI
// =====================================================================================

// Owning device allocation: freed when it goes out of scope, so error returns (HIP_TRY) and ptx_destroy
// release everything without a list of names to keep in step.
template <typename T> struct DevBuf
{
    T *p = nullptr;
    size_t n = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept { swap(o); }
    DevBuf &operator=(DevBuf &&o) noexcept { release(); swap(o); return *this; }
    ~DevBuf() { release(); }
    hipError_t alloc(size_t count)
    {
        if (count <= n && p)
            return hipSuccess;
        release();
        const hipError_t e = hipMalloc(reinterpret_cast<void **>(&p), (count ? count : 1) * sizeof(T));
        if (e == hipSuccess)
            n = count;
        else
            p = nullptr;
        return e;
    }
    void release()
    {
        if (p)
            (void)hipFree(p);
        p = nullptr;
        n = 0;
    }
    void swap(DevBuf &o)
    {
        std::swap(p, o.p);
        std::swap(n, o.n);
    }
};

// How ptx_build_accel builds the tree (the software stand-in for VkBuildAccelerationStructureFlags: the reference asks its driver
// for ePreferFastTrace, AccelerationStructure.cpp:319-324).  buildBestTree tries a few settings and keeps the cheapest tree.
struct TreeParams
{
    uint32_t plocRadius = kPlocRadius; // PLOC: clusters look for their merge partner this many positions to either side
    float plocShape = kPlocShape;      // PLOC: weight of the compactness term in the merge metric
    bool mortonCubic = false;          // Morton curve with cubic cells (one scale for the three axes)
    uint32_t collapse = 1;             // 4-wide collapse: 0 greedy by surface area (round 1), 1 cost-driven (k_collapse_cost)
    uint32_t reinsertPasses = 2;       // passes of parallel reinsertion over the binary tree before the collapse (k_reinsert_*): every
                                       // candidate tree gets these; a build that keeps its state for refits (animation) at most these
    uint32_t reinsertFinal = 32;       // ... and the candidate that wins is built once more with this many (15 ms per pass at 2 M triangles)
    float splitBudget = 0.0f;          // pre-splitting: extra leaf references as a fraction of the triangle count (0: none)
    uint32_t layout = 0;               // node order: 0 breadth-first levels, 1 depth-first (every subtree one contiguous range; measured flat)
};

// The environment switches of the library (INTEGRATION.md lists them): experiment and test knobs, read ONCE per handle when it
// is created -- no entry point calls getenv afterwards, and a handle keeps the values it was created with.
struct EnvSwitches
{
    // Who runs where (round 6; docs/EXPERIMENTS.md): the handle's streams are created with a CU mask (hipExtStreamCreateWithCUMask)
    //   0 none (any CU)   1 one XCD per handle (handle h -> XCD h % 8)   2 two groups of four XCDs (h % 2)
    //   3 main stream (closest + shade) on XCDs 0-5, auxiliary stream (shadow, tail) on XCDs 6-7   4 two XCDs per handle (h % 4)
    //   5 main stream on XCD h % 8, auxiliary stream on XCD (h + 4) % 8
    // With a mask the library creates the main stream itself even if the host passed one (the host's stream cannot be masked).
    uint32_t cuPartition = 0;
    bool singleStream = false; // PTX_SINGLE_STREAM=1: every handle as if created with PTX_DEVICE_SINGLE_STREAM
    bool verbose = false;        // PTX_VERBOSE: progress and statistics on stderr
    bool karrasBuilder = false;  // PTX_BUILDER=lbvh: Karras topology instead of PLOC
    bool plocFixed = false;      // PTX_PLOC_RADIUS / PTX_PLOC_SHAPE given: ONE tree with these parameters, no candidates
    uint32_t plocRadius = 0;     // PTX_PLOC_RADIUS
    float plocShape = 0.0f;      // PTX_PLOC_SHAPE
    int reinsertPasses = -1;     // PTX_REINSERT=N: N reinsertion passes for the winning tree, min(N, 2) for every candidate (-1: not given)
    float splitBudget = -1.0f;   // PTX_SPLIT_BUDGET: extra leaf references as a fraction of the triangle count (< 0: not given)
    int layout = -1;             // PTX_NODE_LAYOUT=0 / 1: breadth-first / depth-first node order (-1: not given)
    int collapse = -1;           // PTX_COLLAPSE=0 / 1: greedy / cost-driven 4-wide collapse (-1: not given; does not fix the other parameters)
    int shadeSort = -1;          // PTX_SHADE_SORT=0 / 1 overrides the scene's choice (-1: not given)
    long tailThreshold = -1;     // PTX_TAIL_THRESHOLD: live paths at or below which k_tail takes over (-1: the default)
    uint32_t framesPerWave = 8;  // PTX_FRAMES_PER_WAVE: samples of one pixel in neighbouring lanes, at most this many
    uint32_t raysPerThread = 0;  // PTX_RAYS_PER_THREAD (process-wide: the last handle created sets it)
    long residentCap = -1;       // PTX_RESIDENT_CAP=0: persistent grids are not capped at the resident block count
    uint32_t copyGroups = 0;     // PTX_COPY_GROUPS: workgroups of the read-back copy kernel (0: one, or 2 per rank of a tile shard, at most 16)
    bool snapshotMemcpy = false; // PTX_SNAPSHOT_MEMCPY=1: the read-back's device-side snapshot by hipMemcpyAsync (rounds 1-4) instead of a kernel
    bool fenceRefit = false;     // PTX_FENCE_REFIT=1: the round-4 bottom-up kernels (fence and atomic per node) instead of the level lists
    bool pairLeaves = true;      // PTX_PAIR_LEAVES=0: single-triangle leaves only (pt_bvh_build.hpp, "pair leaves")
    bool firstBounce = true;     // PTX_FIRST_BOUNCE=0: k_generate hands the primary rays over through memory (rounds 1-6) instead of the first
                                 // bounce's kernels computing them (pt_wavefront.hpp, FirstClosestIO)
    bool streamLevelwise = false; // PTX_STREAM_LEVELWISE=1: ptx_texture_upload builds every chain level by level (k_blit_level) instead of k_stream_chain
    bool streamPlan = true;      // PTX_STREAM_PLAN=0: two streams per handle whatever the queues granted (rounds 1-9) instead of the plan of
                                 // pt_stream_plan.hpp
    bool bcRowMapping = false;   // PTX_BC_MAPPING=rows: k_decode_bc with one thread per block row and four stores (measured, not kept) instead of one per texel
    bool copyRuntime = false;    // PTX_COPY_RUNTIME=1: the read-back's copy to the host by hipMemcpyAsync instead of a kernel (measured, not kept)
    static EnvSwitches read()
    {
        EnvSwitches e;
        e.verbose = getenv("PTX_VERBOSE") != nullptr;
        e.streamLevelwise = getenv("PTX_STREAM_LEVELWISE") != nullptr && std::strcmp(getenv("PTX_STREAM_LEVELWISE"), "0") != 0;
        if (const char *v = getenv("PTX_PAIR_LEAVES"))
            e.pairLeaves = std::strcmp(v, "0") != 0;
        if (const char *v = getenv("PTX_FIRST_BOUNCE"))
            e.firstBounce = std::strcmp(v, "0") != 0;
        if (const char *v = getenv("PTX_STREAM_PLAN"))
            e.streamPlan = std::strcmp(v, "0") != 0;
        e.bcRowMapping = getenv("PTX_BC_MAPPING") != nullptr && std::strcmp(getenv("PTX_BC_MAPPING"), "rows") == 0;
        e.copyRuntime = getenv("PTX_COPY_RUNTIME") != nullptr && std::strcmp(getenv("PTX_COPY_RUNTIME"), "0") != 0;
        if (const char *v = getenv("PTX_COPY_GROUPS"))
            e.copyGroups = (uint32_t)strtoul(v, nullptr, 10);
        e.snapshotMemcpy = getenv("PTX_SNAPSHOT_MEMCPY") != nullptr && std::strcmp(getenv("PTX_SNAPSHOT_MEMCPY"), "0") != 0;
        e.fenceRefit = getenv("PTX_FENCE_REFIT") != nullptr && std::strcmp(getenv("PTX_FENCE_REFIT"), "0") != 0;
        if (const char *v = getenv("PTX_BUILDER"))
            e.karrasBuilder = std::strcmp(v, "lbvh") == 0;
        if (const char *v = getenv("PTX_PLOC_SHAPE"))
        {
            e.plocFixed = true;
            e.plocShape = (float)atof(v);
        }
        if (const char *v = getenv("PTX_PLOC_RADIUS"))
        {
            e.plocFixed = true;
            e.plocRadius = std::max(1u, (uint32_t)strtoul(v, nullptr, 10));
        }
        if (const char *v = getenv("PTX_REINSERT"))
            e.reinsertPasses = atoi(v);
        if (const char *v = getenv("PTX_SPLIT_BUDGET"))
            e.splitBudget = (float)atof(v);
        if (const char *v = getenv("PTX_NODE_LAYOUT"))
            e.layout = atoi(v) ? 1 : 0;
        if (const char *v = getenv("PTX_COLLAPSE"))
            e.collapse = atoi(v) ? 1 : 0;
        if (const char *v = getenv("PTX_SHADE_SORT"))
            e.shadeSort = atoi(v) ? 1 : 0;
        if (const char *v = getenv("PTX_TAIL_THRESHOLD"))
            e.tailThreshold = (long)strtoul(v, nullptr, 10);
        if (const char *v = getenv("PTX_FRAMES_PER_WAVE"))
            e.framesPerWave = (uint32_t)atoi(v);
        if (const char *v = getenv("PTX_RAYS_PER_THREAD"))
            e.raysPerThread = std::max(1u, (uint32_t)strtoul(v, nullptr, 10));
        if (const char *v = getenv("PTX_RESIDENT_CAP"))
            e.residentCap = (long)strtoul(v, nullptr, 10);
        e.singleStream = getenv("PTX_SINGLE_STREAM") != nullptr && std::strcmp(getenv("PTX_SINGLE_STREAM"), "0") != 0;
        if (const char *v = getenv("PTX_CU_PARTITION"))
            e.cuPartition = (uint32_t)strtoul(v, nullptr, 10);
        return e;
    }
};

// What ptx_scene_upload produces (pt_scene_host.hpp): HBM copies of the Scene getters, the decoded textures, the any-hit tables,
// the host's side of the animation.  One member of the handle, so that ptx_share_scene drops a borrower's copy by assignment.
struct SceneData
{
    DevBuf<PtxVertex> vertices;
    DevBuf<uint32_t> indices;
    DevBuf<PtxMetallicRoughnessMaterial> mr;
    DevBuf<PtxSpecularGlossinessMaterial> sg;
    DevBuf<PtxPhongMaterial> phong;
    DevBuf<DevPair> pairs;
    DevBuf<uint32_t> pairFirst;
    DevBuf<DebugPair> debugPairs; // per pair: instance, geometry index inside the model, mirrored (the debug view's ids and face culling)
    DevBuf<DevTexture> renderTextures; // what the render kernels sample: every texel decoded to four floats, one pool
    DevBuf<float4> renderTexels;
    // what the any-hit stages read (scenes with non-opaque geometry; pt_bvh.hpp, hitAlpha)
    DevBuf<AlphaTex> alphaTex;     // per colour texture
    DevBuf<uint32_t> alphaTexOf;   // scene texture -> entry of alphaTex
    DevBuf<float4> alphaQuads;     // 2 x 2 alpha footprints of their base levels
    uint32_t textureCount = 0;
    uint32_t skyKind = PTX_SKYBOX_CLEAR_COLOR; // its images follow the scene textures in `renderTextures`
    bool samplerNeeded = false; // some uploaded texture is not a 1x1 white placeholder
    std::vector<uint32_t> rejectedTextures; // block-compressed files the upload rules could not take (ptx_textures_rejected)
    // animation (row N3)
    std::vector<DevPair> hostPairs;            // to recompose pair transforms when instances move
    std::vector<uint32_t> pairInstance;        // pair -> instance
    std::vector<PtxTransform> pairMeshTransform; // pair -> baked mesh transform
    std::vector<DebugPair> hostDebugPairs;     // to refresh the mirrored flags when instances move
    uint32_t instanceCount = 0, skinnedCount = 0, boneCount = 0;
    uint64_t staticVertexCount = 0;
    DevBuf<PtxAnimatedVertex> animatedVertices;
    DevBuf<uint32_t> skinSource;
    DevBuf<PtxTransform> bones;
    bool anyNonOpaque = false;  // some instanced geometry lacks the opaque flag: any-hit stages run
    bool mixedMaterialTypes = false; // the instanced meshes use more than one material type (ShaderTypes.incl:143-145): k_shade sorts its queue
    bool mixedTextured = false;      // ... or materials with and without scene textures: the sampler runs for waves of textured hits only
    uint32_t pairCount = 0, triCount = 0, dxNormalTextures = 0;
    // pose bookkeeping of the motion guides (docs/NEXT_ROWS.md section 17): here, so that the borrowers of a shared scene see it
    struct PoseTracking
    {
        uint64_t serial = 0;        // accepted ptx_update_animation calls; an upload moves it past every history made before it
        bool enabled = false;       // ptx_track_motion
        bool snapshotValid = false; // prevPairs / prevSkinned hold the pose of serial - 1
        DevBuf<DevPair> prevPairs;        // the DevPair table ...
        DevBuf<PtxVertex> prevSkinned;    // ... and vertices[staticVertexCount ...] of the pose the last update replaced
        void release()
        {
            snapshotValid = false;
            prevPairs.release();
            prevSkinned.release();
        }
    } pose;
    // ptx_scene_upload_streamed: the plan, the texture states and the upload stream (pt_scene_host.hpp); null after a plain upload.
    // The last member: it goes first, and its destructor waits for the uploads that still write into the buffers above.
    std::shared_ptr<struct TextureStreaming> streaming;
};

// Per-slot state of the paths in flight (the Wavefront of pt_path_state.hpp, owned).
struct PathState
{
    DevBuf<float4> rayO, rayD, thr, rad, hit, shD, shC, slotRad;
    DevBuf<uint32_t> hitPair, queue0, queue1, shadowQueue, restartQueue;
    DevBuf<uint8_t> shadowResult;
    DevBuf<float4> diffs; // three planes of ray differentials, only for scenes with textures (kernel mode >= 1)
    DevBuf<float4> decal; DevBuf<float> decalT; // nearest ignored any-hit candidate and its distance, only for non-opaque geometry (mode 2)
    // Room for `slots` paths of a scene in kernel mode `mode`: grow-only; differentials and decals a scene needs later come at the
    // largest size asked for.
    hipError_t ensure(int mode, size_t slots)
    {
        const size_t want = std::max(slots, slotRad.n);
        hipError_t e = hipSuccess;
        const auto grow = [&](auto &buf, size_t n) { if (e == hipSuccess) e = buf.alloc(n); };
        if (mode >= 1)
            grow(diffs, 3 * want);
        if (mode == 2)
        {
            grow(decal, want); grow(decalT, want);
        }
        grow(slotRad, want);
        grow(rayO, want); grow(rayD, want); grow(thr, want); grow(rad, want);
        grow(hit, want); grow(shD, want); grow(shC, want);
        grow(hitPair, want);
        grow(queue0, want); grow(queue1, want); grow(shadowQueue, want); grow(shadowResult, want);
        grow(restartQueue, want);
        return e;
    }
    Wavefront view(int mode, uint32_t *counters, uint32_t *spill) const
    {
        Wavefront wf;
        wf.rayO = rayO.p; wf.rayD = rayD.p; wf.thr = thr.p; wf.rad = rad.p;
        wf.hit = hit.p; wf.hitPair = hitPair.p;
        wf.shD = shD.p; wf.shC = shC.p; wf.slotRad = slotRad.p;
        wf.queue[0] = queue0.p; wf.queue[1] = queue1.p; wf.shadowQueue = shadowQueue.p; wf.shadowResult = shadowResult.p;
        wf.restartQueue = restartQueue.p;
        for (int k = 0; k < 3; k++)
            wf.diff[k] = mode >= 1 ? diffs.p + (size_t)k * (diffs.n / 3) : nullptr; // the three planes lie one stride apart
        wf.decal = mode == 2 ? decal.p : nullptr;
        wf.decalT = mode == 2 ? decalT.p : nullptr;
        wf.counters = counters;
        wf.spill = spill;
        return wf;
    }
};

// What the last launch left for ptx_get_stats / the next launch to pick up once the device is done (collectRender).
struct PendingLaunch
{
    enum Kind { kNone, kWavefront, kDebugView } kind = kNone; // kDebugView: a ptx_render_debug, whose counters are the kernel's own
    uint32_t bounces = 0, tailBelow = 0, slots = 0; // slots: 0 for a launch that is not canonical, it teaches no hint
    uint32_t deadSlots = 0; // slots of ragged edge tiles outside the image: in the first queue, not rays
    uint64_t epoch = 0;     // sceneEpoch of the scene it rendered
    bool verbose = false;
};

// The bounce schedule learnt from the last canonical launch: sizes the grids of the next one of the same shape on the same scene.
struct BounceStep { uint32_t bounce, est; int tail; }; // one bounce of a hinted round (hintedSchedule, enqueueBounce)
struct ScheduleHint
{
    std::vector<uint32_t> active; // queue length per bounce
    std::vector<BounceStep> steps; // the round laid out for the launch that uses the hint
    uint32_t slots = 0, bounces = 0;
    uint64_t epoch = 0; // sceneEpoch of the scene the hint was learnt on
    bool matches(uint32_t s, uint32_t b, uint64_t e) const { return slots == s && bounces == b && epoch == e && !active.empty(); }
    void forget() { slots = 0u; } // (no launch has 0 slots: the next one is driven from the host and learns again)
};

// The frame between "the samples are accumulated" and "the host has them" (pt_frame_host.hpp): extent and tile shard, the
// accumulation image and what may stand in for it, and the pipelined copy to the host.  The stream and the events are released by
// destroyRenderer, not by a destructor.
struct FrameState
{
    uint32_t width = 0, height = 0;
    PtxTileShard shard = { 0, 1, 32 };
    DevBuf<float4> image;
    float4 *boundImage = nullptr; // external accumulation buffer, if bound
    float4 *boundShard = nullptr; // ... or the dense tile-major shard buffer the samples are accumulated in (ptx_bind_shard_accumulation)
    size_t boundShardBytes = 0;
    // device alias of the page-locked host frame last used by a read-back / unpack (hipHostGetDevicePointer once per buffer)
    const void *hostAliasOf = nullptr;
    size_t hostAliasBytes = 0;
    float4 *hostAlias = nullptr;
    // pipelined read-back (ptx_readback_begin / _end): snapshot of the image, copied out on its own stream
    DevBuf<float4> staging;
    hipStream_t copyStream = nullptr;
    hipEvent_t evSnapshot = nullptr, evCopied = nullptr;
    bool copyInFlight = false;

    size_t pixels() const { return (size_t)width * height; }
    size_t bytes() const { return pixels() * sizeof(float4); } // of the row-major frame
    float4 *accum() const { return boundImage ? boundImage : image.p; }
    // where k_accumulate adds the samples: the row-major frame, or this rank's dense tile-major shard
    float4 *target() const { return boundShard ? boundShard : accum(); }
    ShardLayout layout(uint32_t rank) const { return shardLayout(width, height, rank, shard.worldSize, shard.tileSize); }
    void unbindShard() // the bound buffer was laid out for another shard or extent
    {
        boundShard = nullptr;
        boundShardBytes = 0;
    }
    void unbind() // a new extent: the caller's buffers have the old size, and a host frame of the new size is another registration
    {
        boundImage = nullptr;
        unbindShard();
        hostAlias = nullptr;
    }
};

// The output stage (row N4) and the screen path (row D15), pt_output_host.hpp.
struct OutputState
{
    DevBuf<float> postRgb, bloomRgb; // rgba16f-valued post-process image and bloom mip chain (3 floats per texel)
    DevBuf<float4> outLinear;        // tone-mapped image (OutputSaver's m_LinearImage)
    DevBuf<uint32_t> outSrgb8;
    bool ready = false;              // a ptx_postprocess since the last ptx_resize / ptx_render_debug
    PtxPostProcessingUniformData postUniform = {}; // of the last ptx_postprocess (composition.comp's BloomIntensity)
    // the swapchain image of the last ptx_present and the caller's UI image
    DevBuf<uint32_t> presentImage, presentUi;
    uint32_t presentWidth = 0, presentHeight = 0, presentFormat = 0;
    size_t presentBytes = 0; // 0: nothing presented yet
    void invalidate() { ready = false; } // the present image stays: it belongs to the window, not to the render extent
};

// The interactive chain behind ptx_render (pt_chain_host.hpp): the images of the guide pass, the temporal accumulation and the
// filters, all of the render extent and allocated by the first call that needs them, and the bookkeeping over them.
struct ChainState
{
    DevBuf<float4> guides;                            // the PTX_GUIDE_COUNT images of the last guide pass
    DevBuf<float4> motion;                            // the PTX_MOTION_COUNT images of the last ptx_render_guides_motion
    DevBuf<float4> specular;                          // the PTX_SPECULAR_COUNT images of the last ptx_render_guides_specular
    DevBuf<float4> denoisePing[2];                    // the filters' iterations alternate between them: D is [status.denoisedIn]
    DevBuf<float4> temporalImage, temporalHistory[2]; // T, and the two copies of the three history images the calls alternate between
    DevBuf<float4> momentHistory[2];                  // the moment history ping-pongs with temporalHistory
    DevBuf<float4> fastHistory[2];                    // ... and so does the fast history of ptx_temporal_accumulate_responsive
    DevBuf<float> varianceImage;                      // V_0 of the last ptx_denoise_variance
    float temporalView[16] = {}, temporalProj[16] = {}; // the matrices the last accepted accumulate call was given
    ChainStatus status;

    float4 *guidePtr(uint32_t which, size_t pixels) const { return guides.p + which * pixels; }
    float4 *motionPtr(uint32_t which, size_t pixels) const { return motion.p + which * pixels; }
    float4 *specularPtr(uint32_t which, size_t pixels) const { return specular.p + which * pixels; }
    float4 *denoised() const { return status.denoisedIn >= 0 ? denoisePing[status.denoisedIn].p : nullptr; }
    void invalidate() { status.resize(); } // the images stay allocated: the next calls of the new extent grow them if they must
};

struct PtxRenderer
{
    EnvSwitches env;
    int device = 0;
    uint32_t backend = PTX_BACKEND_WAVEFRONT;
    hipStream_t stream = nullptr;
    bool ownStream = false;
    bool counted = false; // in g_liveHandles
    std::string error;

    SceneData scene;
    DevBuf<PtxLightsUbo> lights;
    DevBuf<LaunchParams> launchParams; // device copy of the current launch's parameters, written with the lights (k_upload_lights)
    DevBuf<AlphaTri> alphaTris;    // what the any-hit stages read per triangle slot, written behind k_emit
    struct BuildState // what a refit reuses from the last full build: sorted order and the binary topology
    {
        DevBuf<Tri> triTmp;
        DevBuf<float4> boxLo, boxHi, nodeLo, nodeHi;
        DevBuf<uint32_t> sceneBounds, vals0, vals1, hist, histSums, flags;
        DevBuf<uint8_t> inert; // per flattened triangle: left out of the tree (zero area) by the last full build
        // leaf references of a build that splits triangles (k_split_*): boxes, triangle and zero-area flag per reference
        DevBuf<float4> refLo, refHi;
        DevBuf<uint32_t> refTri;
        DevBuf<uint8_t> refInert;
        // ... or that pairs them (k_pair_*): refTri names a reference's first triangle, refPair says whether the next one is in it
        // too, slotOf is the first triangle slot of the reference at each sorted position
        DevBuf<uint8_t> refPair;
        DevBuf<uint32_t> slotOf;
        bool pairRefs = false;
        uint32_t refCount = 0; // references of the last full build (= triangles unless it split or paired some)
        uint32_t treeTris = 0; // triangles in the tree = the first treeTris entries of the sorted order
        DevBuf<uint64_t> keys0, keys1;
        DevBuf<int2> children;
        DevBuf<int> parentOfNode, parentOfLeaf;
        DevBuf<BvhNode> rawNodes; // k_emit's output, one slot per binary node; k_relayout_level compacts it into `nodes`
        DevBuf<float4> collapseCost; // k_collapse_cost: T(x, 1..4) per binary node
        DevBuf<uint8_t> collapseDecide;
        DevBuf<uint32_t> oldOf;   // [0] onwards: emitted index of every node of the compact array; the last entry is the level counter
        // level lists of the binary topology (pt_bvh_build.hpp, round 5): the nodes sorted by depth, for the bottom-up passes
        DevBuf<uint32_t> lvDepth0, lvDepth1, lvVals0, lvVals1, lvStartDev;
        DevBuf<int> lvAnc0, lvAnc1;
        const uint32_t *levelOrder = nullptr; // lvVals0 or lvVals1
        std::vector<uint32_t> levelStart;     // [d] first position of depth d in levelOrder, [maxDepth + 1] = nodes
        bool levelsValid = false;
        bool valid = false;
    } build;
    bool usePloc = true;        // PLOC topology instead of Karras (PTX_BUILDER=lbvh switches back)
    TreeParams tree;            // of the tree in use; the per-frame rebuilds of an animation build with them again
    bool reinsertBroken = false; // a reinsertion pass once left something that was not a tree (k_tree_check): off for this handle
    uint32_t residentClosest[2] = { 0, 0 }, residentShadow[2] = { 0, 0 }; // blocks the chip holds at once, per [ALPHA] variant
    uint32_t treeTris = 0; // scene.triCount minus the zero-area triangles, which are not in the tree
    bool sceneReady = false, accelReady = false;
    // ptx_share_scene: this renderer renders the scene and tree of `sceneOwner` instead of holding copies (frames in flight
    // share one scene, as the reference's per-frame resources do); the owner knows who borrows from it
    PtxRenderer *sceneOwner = nullptr;
    std::vector<PtxRenderer *> sceneSharers;

    // accel
    DevBuf<BvhNode> nodes;
    DevBuf<Tri> tris;
    DevBuf<ShadeTri> shadeTris; // deindexed vertices per triangle slot (leaf order), written by k_emit

    FrameState frame;
    OutputState output;
    ChainState chain;

    // wavefront state
    PathState paths;
    DevBuf<uint32_t> counters, spill; // the counter block (enum Counter) and the traversal-stack overflow region of the main stream
    uint32_t *hostCounters = nullptr; // pinned

    DevBuf<float> testIn, testOut;
    DevBuf<PtxLightsUbo> testUbo;

    hipEvent_t evA = nullptr, evB = nullptr, evT0 = nullptr, evT1 = nullptr; // render / build span; ptx_trace_rays kernel span

    // bounce schedule of the wavefront backend (pt_render_host.hpp): closest + shade on `stream`, shadow + tail on `auxStream` or,
    // where the launch's plan says so (pt_stream_plan.hpp, planFor), on `stream` too.  auxStream is made by the first launch whose
    // plan wants it and stays.
    hipStream_t auxStream = nullptr;
    bool auxIsMain = false; // single-stream handle: auxStream is `stream` itself
    StreamPlan plan = { false, false, 1u }; // of the last launch or read-back (what a change is logged against)
    bool planSeen = false;
    bool singleStream = false; // PtxDeviceDesc.flags & PTX_DEVICE_SINGLE_STREAM
    uint32_t handleSeq = 0, mainXcds = 0xffu, auxXcds = 0xffu; // PTX_CU_PARTITION: the XCDs this handle's streams may use
    DevBuf<uint32_t> spillAux; // traversal-stack overflow region of the kernels on auxStream
    struct BounceEvents
    {
        hipEvent_t t0 = nullptr, t1 = nullptr, t2 = nullptr; // stream: before closest, after closest, after shade
        hipEvent_t x0 = nullptr, x1 = nullptr, x2 = nullptr; // auxStream: before shadow, after shadow, after tail
    };
    std::vector<BounceEvents> bounceEvents; // [min(BounceCount, kMaxTimedBounces)], reused cyclically beyond
    PendingLaunch pending;
    ScheduleHint hint;
    uint64_t sceneEpoch = 1; // bumped by every upload and full build of THIS handle's scene (a refit keeps it: the poses of
                             // an animation differ little from frame to frame)
    PtxStats stats = {};
};

static int fail(PtxRenderer *r, int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if (r)
        r->error = buf;
    return code;
}

#define HIP_TRY(r, expr)                                                                                                   \
    do                                                                                                                     \
    {                                                                                                                      \
        const hipError_t e_ = (expr);                                                                                      \
        if (e_ != hipSuccess)                                                                                              \
            return fail(r, e_ == hipErrorOutOfMemory ? PTX_ERROR_OUT_OF_MEMORY : PTX_ERROR_DEVICE, "%s: %s", #expr,       \
                        hipGetErrorString(e_));                                                                            \
    } while (0)

// the renderer whose scene buffers, tree and scene flags `r` renders with
static const PtxRenderer *sceneOf(const PtxRenderer *r)
{
    return r->sceneOwner ? r->sceneOwner : r;
}

// May `r` trace and shade right now?  A borrower is only as ready as its owner: between the owner's ptx_scene_upload and
// its ptx_build_accel the owner's tree describes the OLD triangles while pairs, vertices and textures are the new ones.
static bool sceneUsable(const PtxRenderer *r)
{
    return r->accelReady && (!r->sceneOwner || (r->sceneOwner->sceneReady && r->sceneOwner->accelReady));
}

static void detachSharedScene(PtxRenderer *r)
{
    if (!r->sceneOwner)
        return;
    std::vector<PtxRenderer *> &v = r->sceneOwner->sceneSharers;
    for (size_t i = 0; i < v.size(); i++)
        if (v[i] == r)
        {
            v.erase(v.begin() + (long)i);
            break;
        }
    r->sceneOwner = nullptr;
    r->accelReady = false; // ptx_share_scene released the borrower's own scene: it needs ptx_scene_upload + ptx_build_accel again
}

// Before the owner of a shared scene changes it (upload, rebuild, animation step): the borrowers' frames in flight end.
static void quiesceSharers(PtxRenderer *r)
{
    for (PtxRenderer *sh : r->sceneSharers)
    {
        if (sh->stream)
            (void)hipStreamSynchronize(sh->stream);
        if (sh->auxStream)
            (void)hipStreamSynchronize(sh->auxStream);
    }
}

static float4 *imagePtr(const PtxRenderer *r) { return r->frame.accum(); }
static float4 *accumTarget(const PtxRenderer *r) { return r->frame.target(); }
static int frameIsElsewhere(PtxRenderer *r, const char *who)
{
    return fail(r, PTX_ERROR_NOT_READY, "%s: the accumulation of this renderer lives in a shard buffer (ptx_bind_shard_accumulation); the frame "
                                         "is composed by ptx_unpack_shards on the rank that gathers it", who);
}

static uint32_t gridFor(size_t n, uint32_t block = kBlock, uint32_t cap = 256 * 8)
{
    size_t g = (n + block - 1) / block;
    if (g < 1)
        g = 1;
    if (g > cap)
        g = cap;
    return static_cast<uint32_t>(g);
}

// Grid of a persistent traversal kernel.  A launch never finishes before its longest ray (hundreds of dependent node
// fetches), which is many times an average ray: giving every thread several rays of a SMALL launch costs nothing, and
// leaves compute units free for the kernel running beside it on the other stream.
// Rays per thread: PTX_RAYS_PER_THREAD fixes it; otherwise 4 while the process holds fewer than four renderers -- a frame alone
// on the machine wants every launch spread over all of it (one frame in flight: 9.6 ms per frame with 4, 10.6 with 8 / 12) -- and,
// with four or more (frames in flight share the machine), 8, or 12 for a launch below 3 M rays: a SMALL launch then does better
// with fewer, longer-lived waves -- a wave that works through eight chunks drains its stragglers once, not once per two chunks,
// and holds a quarter of the wave slots meanwhile.  Measured with eight frames in flight on 16 hardware queues, 4 / 6 / 8 / 12 rays
// per thread: a rank's tile shard of 8 (2.07 M slots) 1.158 / 1.100 / 1.085 / 1.074 ms per step, of 4: 1.912 / 1.903 / 1.886 /
// 1.846, of 2: 3.442 / 3.431 / 3.401 / 3.355; the whole frame, read-back included, three interleaved runs of 4 / this rule / 8:
// chess_like 2,439 / 2,437 / 2,444 Msamples/s, atrium_like 816 / 812 / 820; 16 and 32 lose on both.
static uint32_t g_raysPerThread = 0;
static std::atomic<uint32_t> g_liveHandles{0};
static uint32_t raysPerThreadFor(size_t n)
{
    if (g_raysPerThread)
        return g_raysPerThread;
    return g_liveHandles.load(std::memory_order_relaxed) < 4u ? 4u : (n < 3000000u ? 12u : 8u);
}
// A persistent kernel must not launch more blocks than the chip holds at once: with the static chunk schedule the chunks
// of a block that is not resident yet wait until a resident block has drained the whole queue, and then run on a mostly
// empty chip.  residentBlocks = occupancy (blocks per CU, from the kernel's VGPR / LDS use) x compute units.
static uint32_t g_residentCap = 1; // PTX_RESIDENT_CAP=0: the old fixed cap of 2048 blocks
static uint32_t traceGridFor(size_t n, uint32_t residentBlocks = 0)
{
    const uint32_t per = raysPerThreadFor(n);
    const uint32_t g = gridFor((n + per - 1) / per);
    return g_residentCap && residentBlocks && g > residentBlocks ? residentBlocks : g;
}

template <typename K>
static uint32_t residentBlocksOf(K kernel, int device)
{
    int perCu = 0, cus = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&perCu, kernel, kBlock, 0) != hipSuccess || perCu < 1)
        return 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus < 1)
        return 0;
    return (uint32_t)perCu * (uint32_t)cus;
}

// The parameters of a launch over `rank`'s shard of the handle's frame (the geometry: pt_shard_layout.hpp).  Another rank's than the
// handle's own is what the unpack kernel of a gathered frame reads.
static LaunchParams makeParams(const PtxRenderer *r, const PtxRaygenUniformData *u, uint32_t firstFrame, uint32_t frames, uint32_t rank)
{
    LaunchParams p;
    std::memset(&p, 0, sizeof(p));
    if (u)
        p.u = *u;
    const ShardLayout s = r->frame.layout(rank);
    p.width = r->frame.width;
    p.height = r->frame.height;
    p.rank = rank;
    p.worldSize = r->frame.shard.worldSize;
    p.tileSize = r->frame.shard.tileSize;
    p.tilesX = s.tilesX;
    p.numTiles = s.numTiles;
    p.ownedTiles = s.ownedTiles;
    p.slotsPerFrame = s.slotsPerFrame;
    p.ownedPixels = s.ownedPixels;
    p.frames = frames;
    p.firstFrame = firstFrame;
    p.numSlots = p.slotsPerFrame * frames;
    const uint32_t maxPerWave = r->env.framesPerWave;
    p.framesPerWave = 1;
    while (p.framesPerWave < maxPerWave && p.framesPerWave < 8u && frames % (p.framesPerWave * 2u) == 0u)
        p.framesPerWave *= 2u;
    return p;
}
static LaunchParams makeParams(const PtxRenderer *r, const PtxRaygenUniformData *u, uint32_t firstFrame, uint32_t frames)
{
    return makeParams(r, u, firstFrame, frames, r->frame.shard.rank);
}

// Every frame in flight owns two HIP streams (main + auxiliary), and the runtime multiplexes all streams of a process
// onto GPU_MAX_HW_QUEUES hardware queues -- 4 unless the environment says otherwise.  Streams that share a queue run
// one after the other, which is exactly what frames in flight are meant to avoid: measured on chess_like with 2 / 4 /
// 8 / 16 queues, whole frame (3 in flight) 10.7 / 8.50 / 8.17 / 8.16 ms per step, one rank's shard of 8 (12 in flight)
// - / 1.73 / 1.68 / 1.54.  The variable is read when the runtime initialises (the first HIP call of the process) and is
// the HOST's to set (the Python package and bench.py set it at import): a library that edits its host's
// environment at load time races with getenv in the host's other threads and cannot know whether HIP is up already.  What
// the library does instead is REPORT and ADAPT: PtxStats::hardwareQueues says how many queues the environment grants, the
// handle whose streams no longer fit says so once (ptx_last_error after a successful ptx_create, stderr under PTX_VERBOSE),
// and every launch takes the schedule that fits what is granted (planFor, pt_stream_plan.hpp): while the two streams of every
// live handle have a queue each, the two-stream schedule measured above; once they do not, the frame's auxiliary kernels and
// its read-back ride the main stream -- a stream that waits for another stream's event, or runs a one-workgroup copy for
// milliseconds, holds a queue that another frame's stream shares (docs/EXPERIMENTS.md, "Stream plan").
static uint32_t hardwareQueuesGranted()
{
    const char *e = getenv("GPU_MAX_HW_QUEUES");
    const unsigned long v = e ? strtoul(e, nullptr, 10) : 0ul;
    return v ? (uint32_t)v : 4u; // the runtime's default
}
static std::atomic<bool> g_queueWarningGiven{false};

// The plan of the launch (or read-back) being enqueued now: handles come and go, so it is evaluated every time.  A change is logged
// under PTX_VERBOSE; nothing else happens on one -- the streams a plan no longer uses stay.
static StreamPlan planFor(PtxRenderer *r)
{
    const StreamPlan now = streamPlanFor({ (uint32_t)r->stats.hardwareQueues, g_liveHandles.load(std::memory_order_relaxed),
                                           r->env.singleStream || r->singleStream, r->env.streamPlan });
    if (r->env.verbose && (!r->planSeen || now != r->plan))
        fprintf(stderr, "[ptx] handle %u: stream plan %s: %s (%u live handles, %u hardware queues)\n", r->handleSeq, r->planSeen ? "changes to" : "is",
                streamPlanName(now), g_liveHandles.load(std::memory_order_relaxed), (uint32_t)r->stats.hardwareQueues);
    r->plan = now;
    r->planSeen = true;
    return now;
}

static void destroyRenderer(PtxRenderer *r);

// CU masks of PTX_CU_PARTITION.  Bit i of the mask is compute unit i in the driver's numbering, which deals the CUs of a
// multi-XCD device round-robin over the XCDs (bit i -> XCD i % 8, the amdgpu driver's mqd_symmetrically_map_cu_mask walks the mask
// with a stride of the XCD count): XCD x = bits x, x + 8, x + 16 ...
static std::atomic<uint32_t> g_handleSeq{0};
static void xcdMask(uint32_t xcdBits, uint32_t cus, std::vector<uint32_t> &mask)
{
    mask.assign((cus + 31) / 32, 0u);
    for (uint32_t i = 0; i < cus; i++)
        if (xcdBits & (1u << (i % 8u)))
            mask[i / 32] |= 1u << (i % 32);
}
// the XCDs of the handle's main / auxiliary stream under partition `mode`; 0xff = no mask
static void partitionOf(uint32_t mode, uint32_t h, uint32_t &mainXcds, uint32_t &auxXcds)
{
    mainXcds = auxXcds = 0xffu;
    switch (mode)
    {
    case 1: mainXcds = auxXcds = 1u << (h % 8u); break;
    case 2: mainXcds = auxXcds = (h % 2u) ? 0xf0u : 0x0fu; break;
    case 3: mainXcds = 0x3fu; auxXcds = 0xc0u; break;
    case 4: mainXcds = auxXcds = 0x3u << (2u * (h % 4u)); break;
    case 5: mainXcds = 1u << (h % 8u); auxXcds = 1u << ((h + 4u) % 8u); break;
    case 6: mainXcds = auxXcds = 0x1ffu; break; // control: hipExtStreamCreateWithCUMask with EVERY CU enabled
    case 7: mainXcds = auxXcds = 0x2ffu; break; // control: the library's own plain streams instead of the host's
    default: break;
    }
}
static hipError_t createStreamOn(hipStream_t *s, uint32_t xcds, int device)
{
    int cus = 0;
    if (xcds == 0xffu || xcds == 0x2ffu || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus < 8)
        return hipStreamCreateWithFlags(s, hipStreamNonBlocking);
    std::vector<uint32_t> mask;
    xcdMask(xcds & 0xffu, (uint32_t)cus, mask);
    return hipExtStreamCreateWithCUMask(s, (uint32_t)mask.size(), mask.data());
}

static int createRenderer(const PtxDeviceDesc *desc, PtxRenderer **out)
{
    if (!out)
        return PTX_ERROR_INVALID_ARGUMENT;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
        return PTX_ERROR_NO_DEVICE; // no CPU fallback: the product path needs a HIP device
    PtxRenderer *r = new PtxRenderer;
    r->device = desc ? desc->deviceIndex : 0;
    r->backend = desc ? desc->backend : PTX_BACKEND_WAVEFRONT;
    r->singleStream = desc && (desc->flags & PTX_DEVICE_SINGLE_STREAM) != 0u;
    if (r->device < 0 || r->device >= n || hipSetDevice(r->device) != hipSuccess)
    {
        delete r;
        return PTX_ERROR_NO_DEVICE;
    }
    r->env = EnvSwitches::read(); // the only place the library reads its switches
    r->handleSeq = g_handleSeq++;
    partitionOf(r->env.cuPartition, r->handleSeq, r->mainXcds, r->auxXcds);
    if (desc && desc->stream && r->mainXcds == 0xffu)
        r->stream = static_cast<hipStream_t>(desc->stream);
    else
    {
        if (createStreamOn(&r->stream, r->mainXcds, r->device) != hipSuccess)
        {
            delete r;
            return PTX_ERROR_DEVICE;
        }
        r->ownStream = true;
    }
    r->usePloc = !r->env.karrasBuilder;
    if (r->env.collapse >= 0)
        r->tree.collapse = (uint32_t)r->env.collapse;
    if (r->env.layout >= 0)
        r->tree.layout = (uint32_t)r->env.layout;
    if (r->env.splitBudget >= 0.0f)
        r->tree.splitBudget = r->env.splitBudget;
    if (r->env.reinsertPasses >= 0)
    {
        r->tree.reinsertFinal = (uint32_t)r->env.reinsertPasses;
        r->tree.reinsertPasses = std::min(r->tree.reinsertPasses, r->tree.reinsertFinal);
    }
    if (r->env.plocFixed)
    {
        r->tree.plocShape = r->env.plocShape;
        if (r->env.plocRadius)
            r->tree.plocRadius = r->env.plocRadius;
    }
    if (r->env.raysPerThread)
        g_raysPerThread = r->env.raysPerThread;
    if (r->env.residentCap >= 0)
        g_residentCap = (uint32_t)r->env.residentCap;
    // (a masked stream holds fewer blocks at once: the persistent grids are sized to the XCDs the stream may use)
    const uint32_t mainShare = (uint32_t)__builtin_popcount(r->mainXcds & 0xffu), auxShare = (uint32_t)__builtin_popcount(r->auxXcds & 0xffu);
    r->residentClosest[0] = residentBlocksOf(k_trace_closest<false>, r->device) * mainShare / 8u;
    r->residentClosest[1] = residentBlocksOf(k_trace_closest<true>, r->device) * mainShare / 8u;
    r->residentShadow[0] = residentBlocksOf(k_trace_shadow<false>, r->device) * auxShare / 8u;
    r->residentShadow[1] = residentBlocksOf(k_trace_shadow<true>, r->device) * auxShare / 8u;
    if (r->env.verbose)
        fprintf(stderr, "[ptx] resident blocks: closest %u / %u, shadow %u / %u\n", r->residentClosest[0], r->residentClosest[1], r->residentShadow[0],
                r->residentShadow[1]);
    (void)hipEventCreate(&r->evA);
    (void)hipEventCreate(&r->evB);
    (void)hipEventCreate(&r->evT0);
    (void)hipEventCreate(&r->evT1);
    (void)hipHostMalloc(reinterpret_cast<void **>(&r->hostCounters), C_COUNT * sizeof(uint32_t), hipHostMallocDefault);
    if (r->counters.alloc(C_COUNT) != hipSuccess || r->lights.alloc(1) != hipSuccess || r->launchParams.alloc(1) != hipSuccess || !r->hostCounters ||
        r->spill.alloc((size_t)kGlobalSpill * kMaxPersistentThreads) != hipSuccess)
    {
        destroyRenderer(r);
        return PTX_ERROR_OUT_OF_MEMORY;
    }
    r->stats.hardwareQueues = hardwareQueuesGranted();
    r->counted = true;
    const uint32_t live = ++g_liveHandles;
    const uint32_t streamsPerHandle = (r->singleStream || r->env.singleStream) ? 1u : 2u;
    if (streamsPerHandle * live > r->stats.hardwareQueues && live > 1 && !g_queueWarningGiven.exchange(true))
    {
        // not an error: the handle works, and the note says which schedule its launches take from here on (planFor)
        const StreamPlan plan = streamPlanFor({ (uint32_t)r->stats.hardwareQueues, live, streamsPerHandle == 1u, r->env.streamPlan });
        fail(r, PTX_OK, "%u handles (%u stream(s) each) share %u hardware queues; stream plan: %s; export GPU_MAX_HW_QUEUES=16 "
                        "(24 for a process that also gathers) before the process first uses HIP to give every stream a queue", live, streamsPerHandle,
             (uint32_t)r->stats.hardwareQueues, streamPlanName(plan));
        if (r->env.verbose)
            fprintf(stderr, "[ptx] %s\n", r->error.c_str());
    }
    *out = r;
    return PTX_OK;
}

static void destroyRenderer(PtxRenderer *r)
{
    if (!r)
        return;
    (void)hipSetDevice(r->device);
    if (r->counted)
        --g_liveHandles;
    if (r->stream)
        (void)hipStreamSynchronize(r->stream);
    detachSharedScene(r);
    quiesceSharers(r);
    for (PtxRenderer *sh : r->sceneSharers) // borrowers of this scene: their frames have ended, and now they have no scene
    {
        sh->sceneOwner = nullptr;
        sh->accelReady = false;
    }
    r->sceneSharers.clear();
    // every DevBuf member (scene, tree, build state, wavefront state, animation, output stage) frees itself in `delete r`
    if (r->auxStream && !r->auxIsMain) { (void)hipStreamSynchronize(r->auxStream); (void)hipStreamDestroy(r->auxStream); }
    for (PtxRenderer::BounceEvents &e : r->bounceEvents)
        for (hipEvent_t ev : { e.t0, e.t1, e.t2, e.x0, e.x1, e.x2 })
            if (ev)
                (void)hipEventDestroy(ev);
    if (r->frame.copyStream) { (void)hipStreamSynchronize(r->frame.copyStream); (void)hipStreamDestroy(r->frame.copyStream); }
    if (r->frame.evSnapshot) (void)hipEventDestroy(r->frame.evSnapshot);
    if (r->frame.evCopied) (void)hipEventDestroy(r->frame.evCopied);
    if (r->hostCounters)
        (void)hipHostFree(r->hostCounters);
    if (r->evA) (void)hipEventDestroy(r->evA);
    if (r->evB) (void)hipEventDestroy(r->evB);
    if (r->evT0) (void)hipEventDestroy(r->evT0);
    if (r->evT1) (void)hipEventDestroy(r->evT1);
    if (r->ownStream && r->stream)
        (void)hipStreamDestroy(r->stream);
    delete r;
}

// Kernel variant of the uploaded scene: 0 = opaque geometry with the fixed 1x1 textures only, 1 = ray
// differentials + software sampler, 2 = 1 + the any-hit stages (alpha test, decals).
static int kernelMode(const PtxRenderer *r)
{
    const PtxRenderer *s = sceneOf(r);
    return s->scene.anyNonOpaque ? 2 : (s->scene.samplerNeeded ? 1 : 0);
}

static SceneView makeSceneView(const PtxRenderer *r)
{
    const PtxRenderer *s = sceneOf(r);
    SceneView sv;
    sv.shadeTris = s->shadeTris.p;
    sv.vertices = s->scene.vertices.p; sv.indices = s->scene.indices.p; sv.mr = s->scene.mr.p; sv.sg = s->scene.sg.p; sv.phong = s->scene.phong.p;
    sv.pairs = s->scene.pairs.p; sv.dxNormalTextures = s->scene.dxNormalTextures;
    sv.lights = r->lights.p; // the lights come with every launch: each frame in flight has its own
    sv.tex.textures = s->scene.renderTextures.p; sv.tex.textureCount = s->scene.textureCount; sv.tex.texels8 = nullptr; sv.tex.texelsF = s->scene.renderTexels.p;
    sv.tex.srgbLut = nullptr;
    sv.skyKind = s->scene.skyKind;
    return sv;
}

static TraceScene makeTraceScene(const PtxRenderer *r)
{
    const PtxRenderer *s = sceneOf(r);
    TraceScene sc;
    sc.nodes = s->nodes.p; sc.tris = s->tris.p; sc.triCount = s->treeTris;
    sc.alphaTris = s->alphaTris.p; sc.alphaQuads = s->scene.alphaQuads.p;
    return sc;
}

// Does the linear part of a mat3x4 have a negative determinant (an instance that mirrors its model)?
static bool transformMirrors(const float *m)
{
    const double det = (double)m[0] * ((double)m[5] * m[10] - (double)m[6] * m[9]) - (double)m[1] * ((double)m[4] * m[10] - (double)m[6] * m[8]) +
                       (double)m[2] * ((double)m[4] * m[9] - (double)m[5] * m[8]);
    return det < 0.0;
}

#include "pt_scene_host.hpp" // ptx_share_scene and ptx_scene_upload: shareScene, sceneUpload and its stages

#include "pt_bvh_host.hpp" // the tree build: buildAccel, buildBestTree

// ptx_track_motion: whether ptx_update_animation keeps the pose it replaces (snapshotPose).  Owner only, like the update itself.
static int trackMotion(PtxRenderer *r, int enable)
{
    if (!r)
        return PTX_ERROR_INVALID_ARGUMENT;
    if (r->sceneOwner)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "ptx_track_motion: this renderer shares another renderer's scene (ptx_share_scene)");
    if (!r->sceneReady)
        return fail(r, PTX_ERROR_NOT_READY, "ptx_track_motion: no scene uploaded");
    SceneData::PoseTracking &pose = r->scene.pose;
    if (!enable && pose.enabled)
    {
        // a guide pass in flight may still read the snapshot
        HIP_TRY(r, hipSetDevice(r->device));
        quiesceSharers(r);
        HIP_TRY(r, hipStreamSynchronize(r->stream));
        pose.release();
    }
    pose.enabled = enable != 0;
    return PTX_OK;
}

// The first step of ptx_update_animation behind its checks: with tracking on the pose about to be replaced is kept -- the DevPair
// table and the skinned part of the vertex buffer, device to device on the render stream ahead of the uploads and k_skin.  With
// tracking off nothing is enqueued.  The snapshot counts, and the pose serial moves on, only once the update has succeeded
// (updateAnimation): a failed one leaves no snapshot, and the serial where it was.
static int snapshotPose(PtxRenderer *r)
{
    SceneData &sc = r->scene;
    sc.pose.snapshotValid = false;
    if (sc.pose.enabled)
    {
        HIP_TRY(r, sc.pose.prevPairs.alloc(sc.pairCount));
        HIP_TRY(r, sc.pose.prevSkinned.alloc(sc.skinnedCount));
        if (sc.pairCount)
            HIP_TRY(r, hipMemcpyAsync(sc.pose.prevPairs.p, sc.pairs.p, (size_t)sc.pairCount * sizeof(DevPair), hipMemcpyDeviceToDevice, r->stream));
        if (sc.skinnedCount)
            HIP_TRY(r, hipMemcpyAsync(sc.pose.prevSkinned.p, sc.vertices.p + sc.staticVertexCount, (size_t)sc.skinnedCount * sizeof(PtxVertex),
                                      hipMemcpyDeviceToDevice, r->stream));
    }
    return PTX_OK;
}

static int applyAnimation(PtxRenderer *r, const PtxTransform *instanceTransforms, const PtxTransform *boneTransforms, uint32_t boneCount, uint32_t accelUpdate);

// Renderer.cpp:1750-1754 (+ RecordSkinningCommands :854-890, AccelerationStructure::Update :48-57)
static int updateAnimation(PtxRenderer *r, const PtxTransform *instanceTransforms, uint32_t instanceCount, const PtxTransform *boneTransforms, uint32_t boneCount, uint32_t accelUpdate)
{
    if (!r || accelUpdate > PTX_ACCEL_REBUILD)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "ptx_update_animation: bad argument");
    if (r->sceneOwner)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "ptx_update_animation: this renderer shares another renderer's scene (ptx_share_scene)");
    if (!r->sceneReady)
        return fail(r, PTX_ERROR_NOT_READY, "ptx_update_animation: no scene uploaded");
    quiesceSharers(r);
    if (instanceTransforms && instanceCount != r->scene.instanceCount)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "ptx_update_animation: %u instance transforms for a scene of %u instances", instanceCount,
                    r->scene.instanceCount);
    HIP_TRY(r, hipSetDevice(r->device));
    if (const int rc = snapshotPose(r))
        return rc;
    const int rc = applyAnimation(r, instanceTransforms, boneTransforms, boneCount, accelUpdate);
    if (rc == PTX_OK) // accepted: the serial moves on, and what snapshotPose kept is the pose of the serial before
    {
        r->scene.pose.serial++;
        r->scene.pose.snapshotValid = r->scene.pose.enabled;
    }
    return rc;
}

// the update itself, behind ptx_update_animation's checks and the snapshot
static int applyAnimation(PtxRenderer *r, const PtxTransform *instanceTransforms, const PtxTransform *boneTransforms, uint32_t boneCount, uint32_t accelUpdate)
{
    if (instanceTransforms)
    {
        for (size_t p = 0; p < r->scene.hostPairs.size(); p++)
        {
            DevPair &pr = r->scene.hostPairs[p];
            composeTransform(instanceTransforms[r->scene.pairInstance[p]].m, r->scene.pairMeshTransform[p].m, pr.M);
            inverseLinear(pr.M, pr.Rinv);
            r->scene.hostDebugPairs[p].flags = transformMirrors(instanceTransforms[r->scene.pairInstance[p]].m) ? kDebugPairMirrored : 0u;
        }
        if (!r->scene.hostPairs.empty())
        {
            HIP_TRY(r, hipMemcpyAsync(r->scene.pairs.p, r->scene.hostPairs.data(), r->scene.hostPairs.size() * sizeof(DevPair), hipMemcpyHostToDevice, r->stream));
            HIP_TRY(r, hipMemcpyAsync(r->scene.debugPairs.p, r->scene.hostDebugPairs.data(), r->scene.hostDebugPairs.size() * sizeof(DebugPair), hipMemcpyHostToDevice, r->stream));
        }
    }
    if (boneTransforms && r->scene.skinnedCount)
    {
        if (boneCount > r->scene.bones.n)
            HIP_TRY(r, r->scene.bones.alloc(boneCount));
        r->scene.boneCount = boneCount;
        if (boneCount)
            HIP_TRY(r, hipMemcpyAsync(r->scene.bones.p, boneTransforms, (size_t)boneCount * sizeof(PtxTransform), hipMemcpyHostToDevice, r->stream));
        k_skin<<<(r->scene.skinnedCount + 255) / 256, 256, 0, r->stream>>>(r->scene.animatedVertices.p, r->scene.skinSource.p, r->scene.skinnedCount, r->scene.bones.p, boneCount,
                                                                  r->scene.vertices.p + r->scene.staticVertexCount);
    }
    HIP_TRY(r, hipStreamSynchronize(r->stream)); // the caller's arrays may go away
    const bool refit = accelUpdate == PTX_ACCEL_REFIT && r->build.valid && r->accelReady;
    return buildAccel(r, refit, true);
}

#include "pt_render_host.hpp" // ptx_render, ptx_render_debug: renderImpl and its stages, collectRender, renderDebug
#include "pt_frame_host.hpp" // accumulation image and its bindings, tile shards, read-back: resizeFrame ... unpackShards
#include "pt_output_host.hpp" // ptx_postprocess, ptx_read_output, ptx_present, ptx_read_present
#include "pt_chain_host.hpp" // the guide pass, the temporal accumulation, the three filters and their read-backs

static int testDebugEval(PtxRenderer *r, uint32_t which, const float *in, float *out, uint32_t n)
{
    if (!r || which > 1u || !in || !out)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "ptx_test_debug_eval: bad argument");
    if (!n)
        return PTX_OK;
    HIP_TRY(r, hipSetDevice(r->device));
    const size_t ni = (size_t)n * (which == 0u ? 18u : 1u), no = (size_t)n * 3u;
    HIP_TRY(r, r->testIn.alloc(ni));
    HIP_TRY(r, r->testOut.alloc(no));
    HIP_TRY(r, hipMemcpyAsync(r->testIn.p, in, ni * 4, hipMemcpyHostToDevice, r->stream));
    k_test_debug_eval<<<(n + 63) / 64, 64, 0, r->stream>>>(which, r->testIn.p, r->testOut.p, n);
    HIP_TRY(r, hipMemcpyAsync(out, r->testOut.p, no * 4, hipMemcpyDeviceToHost, r->stream));
    HIP_TRY(r, hipStreamSynchronize(r->stream));
    HIP_TRY(r, hipGetLastError());
    return PTX_OK;
}

static int getStats(PtxRenderer *r, PtxStats *stats)
{
    if (!r || !stats)
        return PTX_ERROR_INVALID_ARGUMENT;
    HIP_TRY(r, hipStreamSynchronize(r->stream));
    {
        const int rcc = collectRender(r);
        if (rcc != PTX_OK)
            return rcc;
    }
    float ms = 0.0f;
    if (hipEventElapsedTime(&ms, r->evA, r->evB) == hipSuccess)
        r->stats.lastRenderMs = ms;
    *stats = r->stats;
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
    HIP_TRY(r, r->testIn.alloc(ni));
    HIP_TRY(r, r->testOut.alloc(no));
    if (fn == PTX_FN_SAMPLE_LIGHT)
        HIP_TRY(r, r->testUbo.alloc(n));
    HIP_TRY(r, hipMemcpyAsync(r->testIn.p, in, ni * 4, hipMemcpyHostToDevice, r->stream));
    HIP_TRY(r, hipMemsetAsync(r->testOut.p, 0, no * 4, r->stream));
    k_test_eval<<<(n + 63) / 64, 64, 0, r->stream>>>(fn, r->testIn.p, r->testOut.p, n, r->testUbo.p);
    HIP_TRY(r, hipMemcpyAsync(out, r->testOut.p, no * 4, hipMemcpyDeviceToHost, r->stream));
    HIP_TRY(r, hipStreamSynchronize(r->stream));
    HIP_TRY(r, hipGetLastError());
    return PTX_OK;
}

static int testTexture(PtxRenderer *r, const float *in, float *out, uint32_t n, int implicitLod)
{
    if (!r || !in || !out)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "ptx_test_texture: null argument");
    if (!r->sceneReady)
        return fail(r, PTX_ERROR_NOT_READY, "ptx_test_texture: no scene uploaded");
    if (!n)
        return PTX_OK;
    HIP_TRY(r, hipSetDevice(r->device));
    HIP_TRY(r, r->testIn.alloc((size_t)n * 7));
    HIP_TRY(r, r->testOut.alloc((size_t)n * 4));
    HIP_TRY(r, hipMemcpyAsync(r->testIn.p, in, (size_t)n * 28, hipMemcpyHostToDevice, r->stream));
    TextureView tv;
    tv.textures = r->scene.renderTextures.p; tv.textureCount = r->scene.textureCount; tv.texels8 = nullptr; tv.texelsF = r->scene.renderTexels.p;
    tv.srgbLut = nullptr;
    k_test_texture<<<(n + 63) / 64, 64, 0, r->stream>>>(tv, r->testIn.p, r->testOut.p, n, implicitLod);
    HIP_TRY(r, hipMemcpyAsync(out, r->testOut.p, (size_t)n * 16, hipMemcpyDeviceToHost, r->stream));
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
    TraceScene sc;
    sc = makeTraceScene(r);
    hipError_t e = hipMemcpyAsync(dRays.p, rays, (size_t)n * 32, hipMemcpyHostToDevice, r->stream);
    if (e == hipSuccess)
    {
        (void)hipEventRecord(r->evT0, r->stream);
        (void)hipMemsetAsync(&r->counters.p[C_CHUNK], 0, sizeof(uint32_t), r->stream);
        (void)hipMemsetAsync(dOverflow.p, 0, sizeof(uint32_t), r->stream);
        withFlag(sceneOf(r)->scene.anyNonOpaque, [&](auto ALPHA) {
            k_trace_rays<decltype(ALPHA)::value><<<gridFor(n), kBlock, 0, r->stream>>>(sc, dRays.p, n, anyHit, dHits.p, dIds.p, &r->counters.p[C_CHUNK], r->spill.p, dOverflow.p);
        });
        (void)hipEventRecord(r->evT1, r->stream);
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
    (void)hipEventElapsedTime(&ms, r->evT0, r->evT1);
    r->stats.lastTraceMs = ms;
    dRays.release(); dHits.release(); dIds.release(); dOverflow.release();
    if (e != hipSuccess)
        return fail(r, PTX_ERROR_DEVICE, "ptx_trace_rays: %s", hipGetErrorString(e));
    if (overflowed)
        return fail(r, PTX_ERROR_DEVICE, "ptx_trace_rays: traversal stack overflow (tree deeper than %d levels)", kLdsStack + kGlobalSpill);
    return PTX_OK;
}
