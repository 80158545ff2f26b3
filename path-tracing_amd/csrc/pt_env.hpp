// pt_env.hpp -- what a handle is created with before it touches the device: the parameters of the tree build (TreeParams) and the
// environment switches of the library (EnvSwitches; INTEGRATION.md lists them).  No HIP in here.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>

// PLOC's search radius and shape weight in builds that skip the comparison of candidates (the measurements: pt_bvh_build.hpp, "PLOC")
constexpr int kPlocRadius = 16;
constexpr float kPlocShape = 0.0f;

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
        // the four ways a switch is "on"; the variables are not all of one class, and each keeps the one it has
        const auto given = [](const char *name) { return getenv(name) != nullptr; }; // set at all, even to 0
        const auto on = [](const char *name) { const char *v = getenv(name); return v && std::strcmp(v, "0") != 0; };     // set and not the string 0
        const auto notOff = [](const char *name) { const char *v = getenv(name); return !v || std::strcmp(v, "0") != 0; }; // on unless set to the string 0
        const auto is = [](const char *name, const char *word) { const char *v = getenv(name); return v && std::strcmp(v, word) == 0; };
        EnvSwitches e;
        e.verbose = given("PTX_VERBOSE");
        e.streamLevelwise = on("PTX_STREAM_LEVELWISE");
        e.copyRuntime = on("PTX_COPY_RUNTIME");
        e.snapshotMemcpy = on("PTX_SNAPSHOT_MEMCPY");
        e.fenceRefit = on("PTX_FENCE_REFIT");
        e.singleStream = on("PTX_SINGLE_STREAM");
        e.pairLeaves = notOff("PTX_PAIR_LEAVES");
        e.firstBounce = notOff("PTX_FIRST_BOUNCE");
        e.streamPlan = notOff("PTX_STREAM_PLAN");
        e.bcRowMapping = is("PTX_BC_MAPPING", "rows");
        e.karrasBuilder = is("PTX_BUILDER", "lbvh");
        e.plocFixed = given("PTX_PLOC_SHAPE") || given("PTX_PLOC_RADIUS");
        if (const char *v = getenv("PTX_PLOC_SHAPE")) e.plocShape = (float)atof(v);
        if (const char *v = getenv("PTX_PLOC_RADIUS")) e.plocRadius = std::max(1u, (uint32_t)strtoul(v, nullptr, 10));
        if (const char *v = getenv("PTX_COPY_GROUPS")) e.copyGroups = (uint32_t)strtoul(v, nullptr, 10);
        if (const char *v = getenv("PTX_REINSERT")) e.reinsertPasses = atoi(v);
        if (const char *v = getenv("PTX_SPLIT_BUDGET")) e.splitBudget = (float)atof(v);
        if (const char *v = getenv("PTX_NODE_LAYOUT")) e.layout = atoi(v) ? 1 : 0;
        if (const char *v = getenv("PTX_COLLAPSE")) e.collapse = atoi(v) ? 1 : 0;
        if (const char *v = getenv("PTX_SHADE_SORT")) e.shadeSort = atoi(v) ? 1 : 0;
        if (const char *v = getenv("PTX_TAIL_THRESHOLD")) e.tailThreshold = (long)strtoul(v, nullptr, 10);
        if (const char *v = getenv("PTX_FRAMES_PER_WAVE")) e.framesPerWave = (uint32_t)atoi(v);
        if (const char *v = getenv("PTX_RAYS_PER_THREAD")) e.raysPerThread = std::max(1u, (uint32_t)strtoul(v, nullptr, 10));
        if (const char *v = getenv("PTX_RESIDENT_CAP")) e.residentCap = (long)strtoul(v, nullptr, 10);
        if (const char *v = getenv("PTX_CU_PARTITION")) e.cuPartition = (uint32_t)strtoul(v, nullptr, 10);
        return e;
    }
};
