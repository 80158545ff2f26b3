// pt_runtime.hpp -- host side of the HIP library: the renderer object behind a PtxRenderer handle -- its state one struct per stage,
// every resource a member that releases itself (device memory: DevBuf; events, streams, page-locked memory: Owned, pt_owned.hpp) --,
// createRenderer / destroyRenderer, the scene-sharing helpers, the grid helpers, makeParams, the stream plan and the CU masks, and the
// scene views.  What a handle is created with comes from pt_env.hpp (TreeParams, EnvSwitches).  The stages are host files of their
// own, included at the end in the order they build on one another: scene upload (pt_scene_host.hpp), the tree build (pt_bvh_host.hpp;
// kernels: pt_bvh_build.hpp), animation updates (pt_animation_host.hpp), the render launches with the bounce schedule of the wavefront
// backend and ptx_get_stats (pt_render_host.hpp), the frame's hand-over -- accumulation image, tile shards, read-back --
// (pt_frame_host.hpp), the output stage and the screen path (pt_output_host.hpp), the interactive chain -- guide pass, temporal
// accumulation, the filters -- (pt_chain_host.hpp; its bookkeeping: pt_chain_state.hpp), the ptx_test_* / ptx_trace_rays entry
// points (pt_test_host.hpp).  Their functions take a valid or null handle; include/ptx.h's entry points (ptx_capi.hip) are one-line
// wrappers around them.  No CPU fallback exists: without a HIP device createRenderer fails.
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
#include "pt_env.hpp"
#include "pt_owned.hpp"
#include "pt_post.hpp"
#include "pt_present.hpp"
#include "pt_shard_layout.hpp"
#include "pt_stream_plan.hpp"
#include "pt_temporal.hpp"
#include "pt_variance.hpp"
#include "pt_responsive.hpp"
#include "pt_despike.hpp"
#include "pt_meter.hpp"
#include "pt_grade.hpp"
#include "pt_local_exposure.hpp"
#include "pt_upscale.hpp"
#include "pt_noise.hpp"
#include "pt_adaptive.hpp"

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

// ... and the same for what is not device memory (pt_owned.hpp): a member that is created late, or not at all, and released by going
// out of scope.  A stream may also be borrowed: the host's, or the main stream standing in as the auxiliary one.
using OwnedEvent = Owned<hipEvent_t, hipEventDestroy>;
using OwnedStream = Owned<hipStream_t, hipStreamDestroy>;
template <typename T> using OwnedPinned = Owned<T *, hipHostFree>; // page-locked host memory (hipHostMalloc)
static hipError_t createEvent(OwnedEvent &ev, unsigned flags = 0u) // flags: hipEventCreateWithFlags'
{
    hipEvent_t e = nullptr;
    const hipError_t rc = flags ? hipEventCreateWithFlags(&e, flags) : hipEventCreate(&e);
    if (rc == hipSuccess)
        ev.adopt(e);
    return rc;
}

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
    uint64_t epoch = 0;     // SceneLink::epoch of the scene it rendered
    bool verbose = false;
};

// The bounce schedule learnt from the last canonical launch: sizes the grids of the next one of the same shape on the same scene.
struct BounceStep { uint32_t bounce, est; int tail; }; // one bounce of a hinted round (hintedSchedule, enqueueBounce)
struct ScheduleHint
{
    std::vector<uint32_t> active; // queue length per bounce
    std::vector<BounceStep> steps; // the round laid out for the launch that uses the hint
    uint32_t slots = 0, bounces = 0;
    uint64_t epoch = 0; // SceneLink::epoch of the scene the hint was learnt on
    bool matches(uint32_t s, uint32_t b, uint64_t e) const { return slots == s && bounces == b && epoch == e && !active.empty(); }
    void forget() { slots = 0u; } // (no launch has 0 slots: the next one is driven from the host and learns again)
};

// The frame between "the samples are accumulated" and "the host has them" (pt_frame_host.hpp): extent and tile shard, the
// accumulation image and what may stand in for it, and the pipelined copy to the host.
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
    OwnedStream copyStream; // made by the first read-back whose plan copies on neither the main nor the auxiliary stream
    OwnedEvent evSnapshot, evCopied;
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
    // exposure metering (ptx_meter, docs/NEXT_ROWS.md section 21): both allocated by the first accepted ptx_meter
    DevBuf<MeterState> meterState;  // result, bins and the adapted exposure
    DevBuf<uint32_t> meterSlabs;    // kMeterGridCap slabs of kMeterSlabWords words, rewritten whole by every call
    // display transform (ptx_grade, docs/NEXT_ROWS.md section 22): the LUT is allocated by ptx_grade_lut, nothing else is device memory
    DevBuf<float> gradeLut;         // gradeLutSize^3 x 3 floats, red fastest; belongs to the display and outlives ptx_resize ...
    uint32_t gradeLutSize = 0;
    PtxGradeDesc gradeDesc = {};    // ... as does the desc of the last accepted ptx_grade, which ptx_present_graded applies
    bool gradeSet = false;
    // local exposure (ptx_local_exposure, docs/NEXT_ROWS.md section 23): both allocated by the first accepted ptx_local_exposure and
    // released by ptx_resize (outputResized), whose extent they were made for
    DevBuf<float> localGain;        // G, one float per pixel
    DevBuf<uint2> localGrid;        // the splatted grid and the blurred one behind it: 2 x ny x nx x 32 entries of (sum, count)
    bool localReady = false;        // an accepted ptx_local_exposure since the last ptx_resize
    // noise metering (ptx_noise_halves, ptx_noise_meter, docs/NEXT_ROWS.md section 26): the halves are made by ptx_noise_halves(1), the
    // rest by the first accepted ptx_noise_meter; ptx_resize (outputResized) releases the halves, whose extent they were made for
    struct NoiseState
    {
        DevBuf<float4> half[2];         // A and B: two accumulation images the host binds with ptx_bind_accumulation
        DevBuf<PtxNoiseResult> result;  // written whole by every call's second kernel
        DevBuf<NoiseTile> tiles;        // (Q_t, n_t, converged) per tile ...
        DevBuf<float> tileErrors;       // ... and E_t, the map ptx_read_noise copies out
        DevBuf<uint32_t> records;       // kNoiseRecordWords words per workgroup of k_noise_tiles
        uint32_t tilesX = 0, tilesY = 0, tileShift = 0; // of the last accepted call
        uint32_t calls = 0;             // accepted calls since creation or ptx_resize
    } noise;
    // adaptive sampling (ptx_adaptive_plan, ptx_noise_meter_adaptive, docs/NEXT_ROWS.md section 27): everything is made by the first
    // accepted ptx_adaptive_plan and released by ptx_resize, a change of the tile shard and ptx_noise_halves(0) (dropAdaptive)
    struct AdaptiveState
    {
        DevBuf<uint32_t> counts;        // countA[numTiles], then countB[numTiles]: frames per tile and half
        DevBuf<uint32_t> list;          // the active tile ids of the plan in force, ascending: what slotPixel reads
        DevBuf<uint8_t> active, seed;   // a flag per tile: in the plan in force / a seed of the last call
        DevBuf<uint8_t> mask;           // the device copy of a PTX_ADAPTIVE_FROM_MASK call's mask
        DevBuf<PtxAdaptivePlan> result; // written whole by every call
        PtxAdaptivePlan plan = {};      // the host's copy of it
        uint32_t tileShift = 0;         // of the counts; 0: there are none
        uint32_t generation = 0;        // accepted ptx_adaptive_plan calls since the counts were made
        bool planned = false;           // a plan is in force: renderImpl covers `list`
        bool counted = false;           // some count may be non-zero
        uint32_t numTiles() const { return plan.tilesX * plan.tilesY; }
    } adaptive;
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
    DevBuf<float4> despikedImage;                     // C of the last ptx_despike, in the sum's scale
    float temporalView[16] = {}, temporalProj[16] = {}; // the matrices the last accepted accumulate call was given
    ChainStatus status;

    float4 *guidePtr(uint32_t which, size_t pixels) const { return guides.p + which * pixels; }
    float4 *motionPtr(uint32_t which, size_t pixels) const { return motion.p + which * pixels; }
    float4 *specularPtr(uint32_t which, size_t pixels) const { return specular.p + which * pixels; }
    float4 *denoised() const { return status.denoisedIn >= 0 ? denoisePing[status.denoisedIn].p : nullptr; }
    float4 *despiked() const { return status.despikedReady ? despikedImage.p : nullptr; }
    void invalidate() { status.resize(); } // the images stay allocated: the next calls of the new extent grow them if they must
};

// What a refit reuses from the last full build (pt_bvh_host.hpp): sorted order and the binary topology.
struct BuildState
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
    DevBuf<BvhNode> rawNodes; // k_emit's output, one slot per binary node; k_relayout_level compacts it into the tree's `nodes`
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
};

// The tree and how it is built (pt_bvh_host.hpp).  A Tree is the buffers the traversal and shading kernels read and the numbers
// that describe them: they move together -- buildBestTree swaps whole trees, ptx_share_scene drops a borrower's by assignment.
struct AccelState
{
    struct Tree
    {
        DevBuf<BvhNode> nodes;
        DevBuf<Tri> tris;
        DevBuf<ShadeTri> shadeTris; // deindexed vertices per triangle slot (leaf order), written by k_emit
        DevBuf<AlphaTri> alphaTris; // what the any-hit stages read per triangle slot, written behind k_emit
        uint32_t slots = 0;         // triangle slots in the tree: scene.triCount minus the zero-area triangles, plus the copies of a split
        uint64_t nodeCount = 0, references = 0; // PtxStats::bvhNodes / treeReferences of this tree
        void swap(Tree &o) { std::swap(*this, o); } // (by moves: a buffer added above is swapped too)
    } tree;
    BuildState build;
    TreeParams params;           // of the tree in use; the per-frame rebuilds of an animation build with them again
    bool usePloc = true;         // PLOC topology instead of Karras (PTX_BUILDER=lbvh switches back)
    bool reinsertBroken = false; // a reinsertion pass once left something that was not a tree (k_tree_check): off for this handle
    bool ready = false;          // a tree over the uploaded scene (a borrower: ptx_share_scene has been called)
    uint32_t residentClosest[2] = { 0, 0 }, residentShadow[2] = { 0, 0 }; // blocks the chip holds at once, per [ALPHA] variant
};

// Whose scene this renderer renders.  ptx_share_scene: it renders the scene and tree of `owner` instead of holding copies (frames in
// flight share one scene, as the reference's per-frame resources do); the owner knows who borrows from it.  Not in SceneData, which
// a borrower drops by assignment.
struct SceneLink
{
    bool ready = false; // a scene has been uploaded to THIS handle
    uint64_t epoch = 1; // bumped by every upload and full build of THIS handle's scene (a refit keeps it: the poses of
                        // an animation differ little from frame to frame)
    PtxRenderer *owner = nullptr;
    std::vector<PtxRenderer *> sharers;
};

// The streams of the handle and the plan of its launches.  Bounce schedule of the wavefront backend (pt_render_host.hpp): closest +
// shade on `main`, shadow + tail on `aux` or, where the launch's plan says so (pt_stream_plan.hpp, planFor), on `main` too.  aux is
// made by the first launch whose plan wants it and stays.
struct StreamSet
{
    OwnedStream main; // the library's own, or the host's of PtxDeviceDesc::stream borrowed; PtxRenderer::stream is the plain view of it
    OwnedStream aux;  // the library's own, or on a single-stream handle `main` borrowed
    bool singleStream = false; // PtxDeviceDesc.flags & PTX_DEVICE_SINGLE_STREAM
    uint32_t handleSeq = 0, mainXcds = 0xffu, auxXcds = 0xffu; // PTX_CU_PARTITION: the XCDs this handle's streams may use
    StreamPlan plan = { false, false, 1u }; // of the last launch or read-back (what a change is logged against)
    bool planSeen = false;
    bool auxIsMain() const { return aux && aux.get() == main.get(); }
};

// What a render launch needs beside the path state, and what it leaves behind (pt_render_host.hpp).
struct BounceEvents
{
    OwnedEvent t0, t1, t2; // main stream: before closest, after closest, after shade
    OwnedEvent x0, x1, x2; // auxiliary stream: before shadow, after shadow, after tail
};
struct LaunchState
{
    DevBuf<PtxLightsUbo> lights;
    DevBuf<LaunchParams> launchParams; // device copy of the current launch's parameters, written with the lights (k_upload_lights)
    DevBuf<uint32_t> counters, spill;  // the counter block (enum Counter) and the traversal-stack overflow region of the main stream
    DevBuf<uint32_t> spillAux;         // traversal-stack overflow region of the kernels on the auxiliary stream
    OwnedPinned<uint32_t> hostCounters;     // the host's copy of the counter block
    OwnedEvent evA, evB;                    // render / build span
    std::vector<BounceEvents> bounceEvents; // [min(BounceCount, kMaxTimedBounces)], reused cyclically beyond
    PendingLaunch pending;
    ScheduleHint hint;
};

// Staging of the ptx_test_* entry points and the kernel span of ptx_trace_rays (pt_test_host.hpp).
struct TestState
{
    DevBuf<float> testIn, testOut;
    DevBuf<PtxLightsUbo> testUbo;
    OwnedEvent evT0, evT1;
};

struct PtxRenderer
{
    EnvSwitches env;
    int device = 0;
    uint32_t backend = PTX_BACKEND_WAVEFRONT;
    bool counted = false; // in g_liveHandles
    std::string error;
    PtxStats stats = {};

    StreamSet streams; // (the first stage member: streams go last, after everything that was ever enqueued on them)
    hipStream_t stream = nullptr; // streams.main.get()
    SceneLink link;
    SceneData scene;
    AccelState accel;
    PathState paths;
    LaunchState launch;
    FrameState frame;
    OutputState output;
    ChainState chain;
    TestState test;
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
    return r->link.owner ? r->link.owner : r;
}

// May `r` trace and shade right now?  A borrower is only as ready as its owner: between the owner's ptx_scene_upload and
// its ptx_build_accel the owner's tree describes the OLD triangles while pairs, vertices and textures are the new ones.
static bool sceneUsable(const PtxRenderer *r)
{
    return r->accel.ready && (!r->link.owner || (r->link.owner->link.ready && r->link.owner->accel.ready));
}

static void detachSharedScene(PtxRenderer *r)
{
    if (!r->link.owner)
        return;
    std::vector<PtxRenderer *> &v = r->link.owner->link.sharers;
    for (size_t i = 0; i < v.size(); i++)
        if (v[i] == r)
        {
            v.erase(v.begin() + (long)i);
            break;
        }
    r->link.owner = nullptr;
    r->accel.ready = false; // ptx_share_scene released the borrower's own scene: it needs ptx_scene_upload + ptx_build_accel again
}

// Before the owner of a shared scene changes it (upload, rebuild, animation step): the borrowers' frames in flight end.
static void quiesceSharers(PtxRenderer *r)
{
    for (PtxRenderer *sh : r->link.sharers)
        for (hipStream_t st : { sh->stream, sh->streams.aux.get() })
            if (st)
                (void)hipStreamSynchronize(st);
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
                                           r->env.singleStream || r->streams.singleStream, r->env.streamPlan });
    if (r->env.verbose && (!r->streams.planSeen || now != r->streams.plan))
        fprintf(stderr, "[ptx] handle %u: stream plan %s: %s (%u live handles, %u hardware queues)\n", r->streams.handleSeq, r->streams.planSeen ? "changes to" : "is",
                streamPlanName(now), g_liveHandles.load(std::memory_order_relaxed), (uint32_t)r->stats.hardwareQueues);
    r->streams.plan = now;
    r->streams.planSeen = true;
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
static hipError_t createStreamOn(OwnedStream &out, uint32_t xcds, int device)
{
    int cus = 0;
    hipStream_t s = nullptr;
    std::vector<uint32_t> mask;
    const bool plain = xcds == 0xffu || xcds == 0x2ffu || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus < 8;
    if (!plain)
        xcdMask(xcds & 0xffu, (uint32_t)cus, mask);
    const hipError_t rc = plain ? hipStreamCreateWithFlags(&s, hipStreamNonBlocking) : hipExtStreamCreateWithCUMask(&s, (uint32_t)mask.size(), mask.data());
    if (rc == hipSuccess)
        out.adopt(s);
    return rc;
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
    r->streams.singleStream = desc && (desc->flags & PTX_DEVICE_SINGLE_STREAM) != 0u;
    if (r->device < 0 || r->device >= n || hipSetDevice(r->device) != hipSuccess)
    {
        delete r;
        return PTX_ERROR_NO_DEVICE;
    }
    r->env = EnvSwitches::read(); // the only place the library reads its switches
    r->streams.handleSeq = g_handleSeq++;
    partitionOf(r->env.cuPartition, r->streams.handleSeq, r->streams.mainXcds, r->streams.auxXcds);
    if (desc && desc->stream && r->streams.mainXcds == 0xffu)
        r->streams.main.borrow(static_cast<hipStream_t>(desc->stream));
    else if (createStreamOn(r->streams.main, r->streams.mainXcds, r->device) != hipSuccess)
    {
        delete r;
        return PTX_ERROR_DEVICE;
    }
    r->stream = r->streams.main.get();
    r->accel.usePloc = !r->env.karrasBuilder;
    if (r->env.collapse >= 0)
        r->accel.params.collapse = (uint32_t)r->env.collapse;
    if (r->env.layout >= 0)
        r->accel.params.layout = (uint32_t)r->env.layout;
    if (r->env.splitBudget >= 0.0f)
        r->accel.params.splitBudget = r->env.splitBudget;
    if (r->env.reinsertPasses >= 0)
    {
        r->accel.params.reinsertFinal = (uint32_t)r->env.reinsertPasses;
        r->accel.params.reinsertPasses = std::min(r->accel.params.reinsertPasses, r->accel.params.reinsertFinal);
    }
    if (r->env.plocFixed)
    {
        r->accel.params.plocShape = r->env.plocShape;
        if (r->env.plocRadius)
            r->accel.params.plocRadius = r->env.plocRadius;
    }
    if (r->env.raysPerThread)
        g_raysPerThread = r->env.raysPerThread;
    if (r->env.residentCap >= 0)
        g_residentCap = (uint32_t)r->env.residentCap;
    // (a masked stream holds fewer blocks at once: the persistent grids are sized to the XCDs the stream may use)
    const uint32_t mainShare = (uint32_t)__builtin_popcount(r->streams.mainXcds & 0xffu), auxShare = (uint32_t)__builtin_popcount(r->streams.auxXcds & 0xffu);
    r->accel.residentClosest[0] = residentBlocksOf(k_trace_closest<false>, r->device) * mainShare / 8u;
    r->accel.residentClosest[1] = residentBlocksOf(k_trace_closest<true>, r->device) * mainShare / 8u;
    r->accel.residentShadow[0] = residentBlocksOf(k_trace_shadow<false>, r->device) * auxShare / 8u;
    r->accel.residentShadow[1] = residentBlocksOf(k_trace_shadow<true>, r->device) * auxShare / 8u;
    if (r->env.verbose)
        fprintf(stderr, "[ptx] resident blocks: closest %u / %u, shadow %u / %u\n", r->accel.residentClosest[0], r->accel.residentClosest[1], r->accel.residentShadow[0],
                r->accel.residentShadow[1]);
    LaunchState &L = r->launch;
    uint32_t *pinned = nullptr; // (an event that cannot be made leaves no counter block, and the handle fails like an allocation)
    if (createEvent(L.evA) == hipSuccess && createEvent(L.evB) == hipSuccess && createEvent(r->test.evT0) == hipSuccess && createEvent(r->test.evT1) == hipSuccess &&
        hipHostMalloc(reinterpret_cast<void **>(&pinned), C_COUNT * sizeof(uint32_t), hipHostMallocDefault) == hipSuccess)
        L.hostCounters.adopt(pinned);
    if (L.counters.alloc(C_COUNT) != hipSuccess || L.lights.alloc(1) != hipSuccess || L.launchParams.alloc(1) != hipSuccess || !L.hostCounters ||
        L.spill.alloc((size_t)kGlobalSpill * kMaxPersistentThreads) != hipSuccess)
    {
        destroyRenderer(r);
        return PTX_ERROR_OUT_OF_MEMORY;
    }
    r->stats.hardwareQueues = hardwareQueuesGranted();
    r->counted = true;
    const uint32_t live = ++g_liveHandles;
    const uint32_t streamsPerHandle = (r->streams.singleStream || r->env.singleStream) ? 1u : 2u;
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
    for (hipStream_t st : { r->stream, r->streams.aux.get(), r->frame.copyStream.get() }) // idle before anything is freed
        if (st)
            (void)hipStreamSynchronize(st);
    detachSharedScene(r);
    quiesceSharers(r);
    for (PtxRenderer *sh : r->link.sharers) // borrowers of this scene: their frames have ended, and now they have no scene
    {
        sh->link.owner = nullptr;
        sh->accel.ready = false;
    }
    r->link.sharers.clear();
    // every member (scene, tree, build state, wavefront state, events, streams ...) releases itself in `delete r`, the streams last
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
    sv.shadeTris = s->accel.tree.shadeTris.p;
    sv.vertices = s->scene.vertices.p; sv.indices = s->scene.indices.p; sv.mr = s->scene.mr.p; sv.sg = s->scene.sg.p; sv.phong = s->scene.phong.p;
    sv.pairs = s->scene.pairs.p; sv.dxNormalTextures = s->scene.dxNormalTextures;
    sv.lights = r->launch.lights.p; // the lights come with every launch: each frame in flight has its own
    sv.tex.textures = s->scene.renderTextures.p; sv.tex.textureCount = s->scene.textureCount; sv.tex.texels8 = nullptr; sv.tex.texelsF = s->scene.renderTexels.p;
    sv.tex.srgbLut = nullptr;
    sv.skyKind = s->scene.skyKind;
    return sv;
}

static TraceScene makeTraceScene(const PtxRenderer *r)
{
    const PtxRenderer *s = sceneOf(r);
    TraceScene sc;
    sc.nodes = s->accel.tree.nodes.p; sc.tris = s->accel.tree.tris.p; sc.triCount = s->accel.tree.slots;
    sc.alphaTris = s->accel.tree.alphaTris.p; sc.alphaQuads = s->scene.alphaQuads.p;
    return sc;
}

static bool transformMirrors(const float *m); // (pt_animation_host.hpp; the upload asks it about every instance too)

#include "pt_scene_host.hpp" // ptx_share_scene and ptx_scene_upload: shareScene, sceneUpload and its stages
#include "pt_bvh_host.hpp" // the tree build: buildAccel, buildBestTree
#include "pt_animation_host.hpp" // ptx_track_motion, ptx_update_animation: trackMotion, snapshotPose, updateAnimation
#include "pt_render_host.hpp" // ptx_render, ptx_render_debug, ptx_get_stats: renderImpl and its stages, collectRender, getStats, renderDebug
#include "pt_output_host.hpp" // the output calls, the meter, the grade, the local exposure, the screen path and their read-backs
#include "pt_frame_host.hpp" // accumulation image and its bindings, tile shards, read-back: resizeFrame ... unpackShards
#include "pt_chain_host.hpp" // the guide pass, the temporal accumulation, the three filters and their read-backs
#include "pt_test_host.hpp" // ptx_test_eval, ptx_test_texture, ptx_test_debug_eval, ptx_trace_rays
