// pt_render_host.hpp -- ptx_render / ptx_render_frames / ptx_render_debug: the bounce schedule of the wavefront backend as named
// stages, the megakernel and zero-bounce launches beside it, what a launch leaves for the next one (collectRender) and for
// ptx_get_stats (getStats).  Included by pt_runtime.hpp after pt_animation_host.hpp; the state is two members of the handle:
// PathState (the per-slot buffers: the list, their growth and the kernels' view of them are that one struct) and LaunchState (lights
// and launch parameters, counter block and its page-locked copy, spill regions, the span and bounce events -- each event an owner
// that releases itself --, PendingLaunch, ScheduleHint); the streams are StreamSet's.
#pragma once

#include <type_traits>

// The kernel variant is a template argument, the scene's mode a run-time value: f(std::integral_constant<int, MODE>) for
// kernelMode()'s 0 / 1 / 2, f(std::true_type / std::false_type) for a flag (ALPHA, textured, face culling).
template <typename F> static void withMode(int mode, F &&f)
{
    if (mode == 2) f(std::integral_constant<int, 2>());
    else if (mode == 1) f(std::integral_constant<int, 1>());
    else f(std::integral_constant<int, 0>());
}
template <typename F> static void withFlag(bool flag, F &&f)
{
    if (flag) f(std::true_type());
    else f(std::false_type());
}

// 3,120 + 204 bytes as kernel arguments: no staging buffer to keep alive.  The launch parameters go with the lights: the first
// bounce's traversal kernel reads them through `dstParams` (FirstClosestIO).  Every frame in flight has its own renderer and
// writes its copy once per launch on its main stream, ahead of the only kernel that reads it: stream order is all it needs.
__global__ void k_upload_lights(PtxLightsUbo lights, LaunchParams params, PtxLightsUbo *dst, LaunchParams *dstParams)
{
    static_assert(sizeof(PtxLightsUbo) % 4 == 0 && sizeof(LaunchParams) % 4 == 0, "copied word by word");
    const uint32_t *src = reinterpret_cast<const uint32_t *>(&lights);
    uint32_t *d = reinterpret_cast<uint32_t *>(dst);
    for (uint32_t i = threadIdx.x; i < sizeof(PtxLightsUbo) / 4; i += blockDim.x)
        d[i] = src[i];
    const uint32_t *srcP = reinterpret_cast<const uint32_t *>(&params);
    uint32_t *dP = reinterpret_cast<uint32_t *>(dstParams);
    for (uint32_t i = threadIdx.x; i < sizeof(LaunchParams) / 4; i += blockDim.x)
        dP[i] = srcP[i];
}

// What a wavefront launch needs beside the path state.  The auxiliary stream is made by the first launch whose plan puts work on it
// (a handle whose streams never fit the queues never makes one) and stays; nothing here runs again in the steady state.
static int ensureRenderResources(PtxRenderer *r, uint32_t bounces, const StreamPlan &plan)
{
    if (!r->streams.aux)
    {
        // PTX_DEVICE_SINGLE_STREAM (or PTX_SINGLE_STREAM=1 in the environment): the shadow and tail kernels ride on the main stream
        // too -- no overlap inside a frame, one hardware queue per frame in flight instead of two (twice the frames on the same
        // queues; what a rank's thin tile shard of an N-GPU job wants, include/ptx.h)
        if (r->env.singleStream || r->streams.singleStream)
            r->streams.aux.borrow(r->stream);
        else if (!plan.auxOnMain)
            HIP_TRY(r, createStreamOn(r->streams.aux, r->streams.auxXcds, r->device));
    }
    if (!r->launch.spillAux.p)
        HIP_TRY(r, r->launch.spillAux.alloc((size_t)kGlobalSpill * kMaxPersistentThreads));
    const size_t want = bounces < (uint32_t)kMaxTimedBounces ? bounces : (uint32_t)kMaxTimedBounces;
    while (r->launch.bounceEvents.size() < want)
    {
        BounceEvents e; // pushed only when all six exist: a partial one releases itself
        for (OwnedEvent *ev : { &e.t0, &e.t1, &e.t2, &e.x0, &e.x1, &e.x2 })
            HIP_TRY(r, createEvent(*ev));
        r->launch.bounceEvents.push_back(std::move(e));
    }
    return PTX_OK;
}

// What the kernels of one launch share.
struct RenderPlan
{
    LaunchParams p;
    SceneView sv;
    TraceScene sc;
    int mode;           // kernelMode()
    uint32_t bounces;   // BounceCount
    uint32_t tailBelow; // queues of at most this many paths are finished by k_tail
    uint32_t sortShade; // material-sorted shade queue (scenes that mix material types; PTX_SHADE_SORT=0 / 1 overrides)
    Wavefront wf, wfAux;
    // of this launch's StreamPlan: the stream of the shadow, k_apply_shadow and tail kernels (the auxiliary stream or the main one),
    // and whether the two streams order themselves by events (no: everything is on one stream, whose order is all it needs)
    hipStream_t aux;
    bool crossWaits;
};

// The two failures a counter block reports, from the host's copy of it.
static int counterErrors(PtxRenderer *r)
{
    const uint32_t *h = r->launch.hostCounters.get();
    if (h[C_OVERFLOW])
        return fail(r, PTX_ERROR_DEVICE, "ptx_render: traversal stack overflow (tree deeper than %d levels)", kLdsStack + kGlobalSpill);
    if (h[C_OVERFLOW + 1])
        return fail(r, PTX_ERROR_DEVICE, "ptx_render: %u paths never produced a finite sample in %u attempts", h[C_OVERFLOW + 1], kMaxSampleRetries);
    return PTX_OK;
}

// The counter block as the main stream has left it: the host waits for the device here.  (Inside a wavefront launch only the
// first message can fire: C_OVERFLOW + 1 is k_megakernel's and k_finish_restarts', which have not run yet.)
static int fetchCounters(PtxRenderer *r)
{
    HIP_TRY(r, hipMemcpyAsync(r->launch.hostCounters.get(), r->launch.counters.p, C_COUNT * sizeof(uint32_t), hipMemcpyDeviceToHost, r->stream));
    HIP_TRY(r, hipStreamSynchronize(r->stream));
    return counterErrors(r);
}

static void launchAccumulate(PtxRenderer *r, const LaunchParams &p)
{
    k_accumulate<<<gridFor((size_t)p.slotsPerFrame * p.framesPerWave), kBlock, 0, r->stream>>>(p, r->paths.slotRad.p, accumTarget(r), nullptr, r->frame.boundShard ? 1u : 0u);
}

// k_tail on the stream of the auxiliary work, a thread per path of `queue` for up to `paths` of them (grid-stride; the spill region holds kMaxPersistentThreads)
static void launchTail(PtxRenderer *r, const RenderPlan &pl, int queue, uint32_t paths, BounceCtl ctl)
{
    const dim3 grid(gridFor(paths, kBlock, kMaxPersistentThreads / kBlock));
    withMode(pl.mode, [&](auto M) { k_tail<decltype(M)::value><<<grid, kBlock, 0, pl.aux>>>(pl.p, pl.sv, pl.sc, pl.wfAux, queue, ctl); });
}

// One BOUNCE of the wavefront over queue `qin` (length in the counter block, at most `est`), enqueued without waiting
// for the device: every kernel reads its queue length from the counter block (BounceCtl).
//
//   stream     P(b)  closest(b)  [wait aux(b-1)]  shade(b)                      P(b+1) closest(b+1) ...
//   auxStream                                     [wait shade(b)] shadow(b) [tail(b)]
//
// ... where the launch's plan gives the auxiliary work its own stream.  Where it rides the main stream (pl.aux == r->stream: the
// handle's two streams do not fit the hardware queues, or it asked for one), the same kernels in the same order on one stream,
//
//   stream     P(b)  closest(b)  shade(b)  shadow(b)  apply(b)  [tail(b)]  P(b+1) closest(b+1) ...
//
// and no event is waited for: a wait for another stream holds the hardware queue of the waiting stream, and with it every other
// frame whose stream shares that queue.  The events are still recorded: they time the kernels (collectRender).
//
// `fresh`: b is bounce 1 of the round renderWavefront starts, whose queue is every slot of the launch.  closest(1) and shade(1)
// are then the <FirstBounce, ..> variants, which compute the primary ray of a slot from the launch parameters -- no k_generate in front:
//
//   stream     upload(lights, params)  P(1)  closest<FirstBounce>(1)  shade<FirstBounce>(1)  P(2) closest(2) ...
//
// (PTX_FIRST_BOUNCE=0: k_generate, then the general kernels over the identity queue it wrote.)  The rounds k_restart starts
// (runSampleRounds) are never fresh: their queue is the restart queue and their rays carry the RNG state on.
//
// shadow(b) only adds into rad[slot], which shade(b + 1) reads -- not closest(b + 1) -- so it runs beside the next
// traversal; k_tail, where the schedule has one, follows it in stream order (the NEE adds it continues from have
// landed): the last shadow query before the tail needs no event of its own.
// shadow(b) also READS rayO[slot]: the shadow ray leaves the point the continuation ray leaves, and the record holds it once.
// closest(b + 1) beside it only reads it too; shade(b + 1) overwrites it, so its wait for aux(b) protects rayO as well as rad.
// tail: 0 = none, 1 = k_tail takes the queue shade(b) filled if it holds at most pl.tailBelow paths, 2 = takes it whatever
// its length (nothing is enqueued behind this bounce).
static int enqueueBounce(PtxRenderer *r, const RenderPlan &pl, uint32_t b, int qin, uint32_t est, int tail, bool fresh)
{
    hipStream_t S = r->stream, X = pl.aux;
    BounceEvents &ev = r->launch.bounceEvents[(b - 1) % r->launch.bounceEvents.size()];
    const BounceCtl ctl = { b, 0u };
    const int qout = qin ^ 1, parity = (int)(b & 1u);
    k_prologue<<<1, 1, 0, S>>>(pl.wf, qin, ctl);
    HIP_TRY(r, hipEventRecord(ev.t0.get(), S));
    withFlag(pl.mode == 2, [&](auto ALPHA) {
        const dim3 grid(traceGridFor(est, r->accel.residentClosest[decltype(ALPHA)::value])); // (the FIRST variants hold the same occupancy)
        if (fresh)
            k_trace_closest<FirstBounce, decltype(ALPHA)::value><<<grid, kBlock, 0, S>>>(pl.sc, pl.wf, r->launch.launchParams.p, pl.p.numSlots);
        else
            k_trace_closest<decltype(ALPHA)::value><<<grid, kBlock, 0, S>>>(pl.sc, pl.wf, qin, ctl);
    });
    HIP_TRY(r, hipEventRecord(ev.t1.get(), S));
    if (b > 1 && pl.crossWaits) // shade reads rad[slot] and overwrites rayO[slot]: the previous bounce's shadow adds must have landed, its rays been read
        HIP_TRY(r, hipStreamWaitEvent(S, r->launch.bounceEvents[(b - 2) % r->launch.bounceEvents.size()].x2.get(), 0));
    const uint32_t shadeGrid = gridFor((est + kShadeItems - 1) / kShadeItems);
    withFlag(pl.mode >= 1, [&](auto TEXTURED) {
        constexpr bool TEX = decltype(TEXTURED)::value;
        if (pl.sortShade && fresh)
            k_shade_sorted<FirstBounce, TEX><<<shadeGrid, kBlock, 0, S>>>(pl.p, pl.sv, pl.wf, qin, ctl);
        else if (pl.sortShade)
            k_shade_sorted<TEX><<<shadeGrid, kBlock, 0, S>>>(pl.p, pl.sv, pl.wf, qin, ctl);
        else if (fresh)
            k_shade<FirstBounce, TEX><<<shadeGrid, kBlock, 0, S>>>(pl.p, pl.sv, pl.wf, qin, ctl);
        else
            k_shade<TEX><<<shadeGrid, kBlock, 0, S>>>(pl.p, pl.sv, pl.wf, qin, ctl);
    });
    HIP_TRY(r, hipEventRecord(ev.t2.get(), S));
    if (pl.crossWaits)
        HIP_TRY(r, hipStreamWaitEvent(X, ev.t2.get(), 0));
    HIP_TRY(r, hipEventRecord(ev.x0.get(), X));
    withFlag(pl.mode == 2, [&](auto ALPHA) {
        k_trace_shadow<decltype(ALPHA)::value><<<traceGridFor(est, r->accel.residentShadow[decltype(ALPHA)::value]), kBlock, 0, X>>>(pl.p, pl.sc, pl.wfAux, qout, parity);
    });
    k_apply_shadow<<<gridFor(est, kBlock, 4096u), kBlock, 0, X>>>(pl.p, pl.wfAux, parity);
    HIP_TRY(r, hipEventRecord(ev.x1.get(), X));
    if (tail)
    {
        // A hinted schedule (tail == 2) hands the tail whatever is left, and the hint is last frame's: a view that keeps four
        // times the paths alive still finds a thread per path (blocks beyond the queue return at once), anything beyond that
        // strides.
        const uint32_t room = tail == 2 ? 4u * pl.tailBelow : pl.tailBelow;
        launchTail(r, pl, qout, est < room ? est : room, { b, tail == 2 ? kTailAnyLength : pl.tailBelow });
    }
    HIP_TRY(r, hipEventRecord(ev.x2.get(), X));
    return PTX_OK;
}

// The round a hint enqueues at once: the bounces that ran as wavefront kernels last time, each with the estimate that sizes its
// grids, and k_tail (tail == 2) behind the bounce whose output it took over last time (or that left nothing).
static void hintedSchedule(const uint32_t *hint, uint32_t bounces, uint32_t tailBelow, uint32_t upperBound, std::vector<BounceStep> &steps)
{
    uint32_t last = bounces;
    if (tailBelow)
        for (uint32_t b = 1; b < bounces && b < (uint32_t)kMaxTimedBounces; b++)
            if (hint[b + 1] <= tailBelow) { last = b; break; } // k_tail took the queue of bounce b (or nothing was left of it)
    steps.clear(); // (keeps its storage: no allocation per launch)
    for (uint32_t b = 1; b <= last; b++)
    {
        uint32_t est = upperBound; // exact for the first bounce; later ones shrink
        if (b > 1 && b <= (uint32_t)kMaxTimedBounces)
            est = (uint32_t)std::min<uint64_t>((uint64_t)hint[b] + hint[b] / 4 + 4096, upperBound);
        steps.push_back({ b, est, (b == last && last < bounces) ? 2 : 0 });
    }
}

// One ROUND: the slots listed in queue 0 (ACTIVE0 set by the caller, at most `upperBound`) start at bounce 0 of a sample
// and are advanced BounceCount times, or until the queue is short enough for k_tail to finish them in one launch.
//
// With a hint (queue lengths of the previous canonical launch of this shape) the whole round is enqueued at once: the
// bounces that ran as wavefront kernels last time, then k_tail for whatever is left -- results do not depend on who
// finishes a path, only the time does, and collectRender drops a hint that turned out wrong.  No kernel is launched just
// to find its queue empty, and the host does not wait for the device.
// Without one (first launch of a shape, rounds of a multi-sample launch) the round is driven bounce by bounce: the host
// reads the counter block after every shade kernel and decides -- which is also how the hint is learned.
static int enqueueRound(PtxRenderer *r, const RenderPlan &pl, uint32_t upperBound, const uint32_t *hint, bool fresh)
{
    uint32_t last = 0; // the last bounce enqueued
    int qin = 0;
    if (hint)
    {
        hintedSchedule(hint, pl.bounces, pl.tailBelow, upperBound, r->launch.hint.steps);
        for (const BounceStep &s : r->launch.hint.steps)
        {
            if (const int rc = enqueueBounce(r, pl, s.bounce, qin, s.est, s.tail, fresh && s.bounce == 1u))
                return rc;
            last = s.bounce;
            qin ^= 1;
        }
    }
    else
    {
        uint32_t est = upperBound;
        for (uint32_t b = 1; b <= pl.bounces; b++)
        {
            if (const int rc = enqueueBounce(r, pl, b, qin, est, 0, fresh && b == 1u))
                return rc;
            last = b;
            qin ^= 1;
            if (const int rc = fetchCounters(r))
                return rc;
            est = r->launch.hostCounters.get()[qin ? C_ACTIVE1 : C_ACTIVE0];
            if (est == 0u)
                break;
            if (b < pl.bounces && est <= pl.tailBelow)
            {
                // the queue is short: k_tail finishes it, behind the shadow kernel of this bounce on its stream
                launchTail(r, pl, qin, est, { b, kTailAnyLength });
                // re-recorded behind the tail: what the stream waits for below
                HIP_TRY(r, hipEventRecord(r->launch.bounceEvents[(b - 1) % r->launch.bounceEvents.size()].x2.get(), pl.aux));
                break;
            }
        }
    }
    if (last && pl.crossWaits)
        HIP_TRY(r, hipStreamWaitEvent(r->stream, r->launch.bounceEvents[(last - 1) % r->launch.bounceEvents.size()].x2.get(), 0));
    HIP_TRY(r, hipGetLastError());
    return PTX_OK;
}

// Statistics and errors of the last wavefront or debug-view launch, once the device is done with it (blocks until then).
static int collectRender(PtxRenderer *r)
{
    if (r->launch.pending.kind == PendingLaunch::kNone)
        return PTX_OK;
    const PendingLaunch pd = r->launch.pending;
    r->launch.pending = PendingLaunch();
    HIP_TRY(r, hipEventSynchronize(r->launch.evB.get()));
    if (const int rc = counterErrors(r))
        return rc;
    const uint32_t *h = r->launch.hostCounters.get();
    r->stats.shadowRays = h[C_HITS];
    r->stats.pathSamples = h[C_SAMPLES];
    if (pd.kind == PendingLaunch::kDebugView) // its counters are the kernel's own, no bounce schedule
    {
        r->stats.segments = h[C_SEGMENTS];
        return PTX_OK;
    }
    unsigned long long waveSegments = 0;
    std::memcpy(&waveSegments, &h[C_WAVE_SEGMENTS], sizeof(waveSegments));
    waveSegments -= pd.deadSlots; // k_prologue counted the whole first queue
    r->stats.segments = waveSegments + h[C_SEGMENTS];
    r->stats.tracedRays = waveSegments;
    r->stats.retries = h[C_RETRIES];
    // kernel times of the bounces that ran (the others returned at once), from the events around every launch
    const uint32_t timed = pd.bounces < (uint32_t)kMaxTimedBounces ? pd.bounces : (uint32_t)kMaxTimedBounces;
    const uint32_t tailPaths = h[C_TAIL_PATHS], tailBounce = h[C_TAIL_PATHS + 1]; // k_tail took the queue shade(tailBounce) filled
    for (uint32_t b = 1; b <= timed; b++)
    {
        const BounceEvents &ev = r->launch.bounceEvents[b - 1];
        const uint32_t active = h[C_BOUNCE_ACTIVE + b];
        const bool ran = active != 0u && !(tailPaths && b > tailBounce);
        if (!ran)
            continue;
        float closestMs = 0.0f, shadeMs = 0.0f, shadowMs = 0.0f, tailMs = 0.0f;
        (void)hipEventElapsedTime(&closestMs, ev.t0.get(), ev.t1.get());
        (void)hipEventElapsedTime(&shadeMs, ev.t1.get(), ev.t2.get());
        (void)hipEventElapsedTime(&shadowMs, ev.x0.get(), ev.x1.get());
        r->stats.lastTraceMs += closestMs;
        r->stats.lastShadeMs += shadeMs;
        r->stats.lastShadowMs += shadowMs;
        r->stats.traceLaunches += 2;
        if (tailPaths && tailBounce == b)
        {
            (void)hipEventElapsedTime(&tailMs, ev.x1.get(), ev.x2.get());
            r->stats.lastTailMs += tailMs;
        }
        if (pd.verbose)
        {
            fprintf(stderr, "[ptx] bounce %u: %u rays closest %.3f ms (%.2f Grays/s) | shade (incl. wait for the previous shadow kernel) %.3f ms | shadow %.3f ms\n",
                    b, active, closestMs, active / closestMs / 1e6, shadeMs, shadowMs);
            if (tailMs > 0.0f)
                fprintf(stderr, "[ptx] tail: %u paths, %u segments, %.3f ms\n", tailPaths, h[C_SEGMENTS], tailMs);
        }
    }
    if (pd.verbose && h[C_RETRIES])
        fprintf(stderr, "[ptx] %u NaN / Inf sample restarts\n", h[C_RETRIES]);
    // grid / schedule hints for the next launch of this shape.  The queue k_tail took over is part of them (a truncated
    // schedule has no prologue behind its last bounce to record it); a tail that had to take more than its threshold
    // means the hints were off: forget them, the next launch runs the full schedule and learns again.
    r->launch.hint.active.assign(h + C_BOUNCE_ACTIVE, h + C_BOUNCE_ACTIVE + kMaxTimedBounces + 1);
    if (tailPaths && tailBounce + 1 <= (uint32_t)kMaxTimedBounces)
        r->launch.hint.active[tailBounce + 1] = tailPaths;
    r->launch.hint.slots = pd.slots; r->launch.hint.bounces = pd.bounces; r->launch.hint.epoch = pd.epoch;
    if (tailPaths > pd.tailBelow)
        r->launch.hint.forget();
    return PTX_OK;
}

// ptx_get_stats: waits for the main stream, collects the last launch, and reads the render / build span off its two events.
static int getStats(PtxRenderer *r, PtxStats *stats)
{
    if (!r || !stats)
        return PTX_ERROR_INVALID_ARGUMENT;
    HIP_TRY(r, hipStreamSynchronize(r->stream));
    if (const int rc = collectRender(r))
        return rc;
    float ms = 0.0f;
    if (hipEventElapsedTime(&ms, r->launch.evA.get(), r->launch.evB.get()) == hipSuccess)
        r->stats.lastRenderMs = ms;
    *stats = r->stats;
    return PTX_OK;
}

// What ptx_render and ptx_render_debug open with: the previous launch is collected (the counter block is reused below), texture
// commits land, the per-slot buffers hold `slots` paths (0: none needed), the stream gets the lights, zeroed counters and evA.
static int beginLaunch(PtxRenderer *r, const PtxLightsUbo *lights, const LaunchParams &p, uint64_t slots)
{
    HIP_TRY(r, hipSetDevice(r->device));
    if (const int rc = collectRender(r))
        return rc;
    if (const int rc = waitForCommits(r))
        return rc;
    if (slots > 0x7fffffffull)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "ptx_render: too many path slots in one batch");
    if (slots)
        HIP_TRY(r, r->paths.ensure(kernelMode(r), (size_t)slots));
    k_upload_lights<<<1, 256, 0, r->stream>>>(*lights, p, r->launch.lights.p, r->launch.launchParams.p);
    HIP_TRY(r, hipMemsetAsync(r->launch.counters.p, 0, C_COUNT * sizeof(uint32_t), r->stream));
    r->stats.pathSamples = r->stats.segments = r->stats.shadowRays = r->stats.retries = r->stats.tracedRays = 0;
    r->stats.traceLaunches = 0;
    r->stats.lastTraceMs = r->stats.lastShadeMs = r->stats.lastShadowMs = r->stats.lastTailMs = 0.0;
    HIP_TRY(r, hipEventRecord(r->launch.evA.get(), r->stream));
    return PTX_OK;
}

// ... and close with: the counter block on its way to the host behind the launch, evB, and the record collectRender picks up.
static int endLaunch(PtxRenderer *r, const PendingLaunch &pd)
{
    HIP_TRY(r, hipMemcpyAsync(r->launch.hostCounters.get(), r->launch.counters.p, C_COUNT * sizeof(uint32_t), hipMemcpyDeviceToHost, r->stream));
    HIP_TRY(r, hipEventRecord(r->launch.evB.get(), r->stream));
    HIP_TRY(r, hipGetLastError());
    r->launch.pending = pd;
    return PTX_OK;
}

// raygen.rgen:62: the bounce loop never runs, every sample ends with radiance 0 -- nothing is generated, traced or
// shaded (the wavefront kernels test the bounce limit only AFTER a bounce); the image still gets its alpha
static int renderZeroBounces(PtxRenderer *r, const LaunchParams &p, uint32_t sampleCount)
{
    HIP_TRY(r, hipMemsetAsync(r->paths.slotRad.p, 0, (size_t)p.numSlots * sizeof(float4), r->stream));
    launchAccumulate(r, p);
    HIP_TRY(r, hipEventRecord(r->launch.evB.get(), r->stream));
    HIP_TRY(r, hipGetLastError());
    r->stats.pathSamples = (uint64_t)p.ownedPixels * p.frames * sampleCount;
    return PTX_OK;
}

// One kernel runs every path to its end; the host waits for it, so nothing is left pending.
static int renderMegakernel(PtxRenderer *r, const RenderPlan &pl)
{
    const dim3 grid((pl.p.numSlots + kBlock - 1) / kBlock);
    withMode(pl.mode, [&](auto M) { k_megakernel<decltype(M)::value><<<grid, kBlock, 0, r->stream>>>(pl.p, pl.sv, pl.sc, r->paths.slotRad.p, r->launch.counters.p); });
    launchAccumulate(r, pl.p);
    HIP_TRY(r, hipMemcpyAsync(r->launch.hostCounters.get(), r->launch.counters.p, C_COUNT * sizeof(uint32_t), hipMemcpyDeviceToHost, r->stream));
    HIP_TRY(r, hipEventRecord(r->launch.evB.get(), r->stream));
    HIP_TRY(r, hipStreamSynchronize(r->stream));
    HIP_TRY(r, hipGetLastError());
    if (r->launch.hostCounters.get()[C_OVERFLOW])
        return fail(r, PTX_ERROR_DEVICE, "ptx_render: traversal stack overflow in the megakernel (depth > %d)", kLdsStackMega);
    if (const int rc = counterErrors(r))
        return rc;
    r->stats.segments = r->launch.hostCounters.get()[C_SEGMENTS];
    r->stats.shadowRays = r->launch.hostCounters.get()[C_HITS];
    r->stats.pathSamples = r->launch.hostCounters.get()[C_SAMPLES];
    r->stats.retries = r->launch.hostCounters.get()[C_RETRIES];
    return PTX_OK;
}

// Canonical launch (one sample per slot): the rare NaN / Inf restarts are finished on the device.
static void finishCanonical(PtxRenderer *r, const RenderPlan &pl)
{
    withMode(pl.mode, [&](auto M) { k_finish_restarts<decltype(M)::value><<<dim3(64), kBlock, 0, r->stream>>>(pl.p, pl.sv, pl.sc, pl.wf); });
}

// multi-sample launch: every slot comes back through the restart queue once per extra sample (and per NaN / Inf
// restart, raygen.rgen:99-112), one round each; a path that never yields a finite sample would go round for ever
// (it hangs the GPU in the reference): give up instead
static int runSampleRounds(PtxRenderer *r, const RenderPlan &pl, uint32_t sampleCount)
{
    const uint64_t maxRounds = (uint64_t)sampleCount * 64 + 64;
    for (uint64_t round = 1;; round++)
    {
        if (const int rc = fetchCounters(r))
            return rc;
        const uint32_t restarts = r->launch.hostCounters.get()[C_RESTART];
        if (!restarts)
            return PTX_OK;
        if (round > maxRounds)
            return fail(r, PTX_ERROR_DEVICE, "ptx_render: %u paths still active after %llu rounds", restarts, (unsigned long long)maxRounds);
        k_restart<<<gridFor(restarts), kBlock, 0, r->stream>>>(pl.p, pl.wf, restarts); // next primary ray of every re-queued slot
        HIP_TRY(r, hipMemcpyAsync(pl.wf.queue[0], pl.wf.restartQueue, (size_t)restarts * sizeof(uint32_t), hipMemcpyDeviceToDevice, r->stream));
        HIP_TRY(r, hipMemsetAsync(&r->launch.counters.p[C_RESTART], 0, sizeof(uint32_t), r->stream));
        HIP_TRY(r, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(&r->launch.counters.p[C_ACTIVE0]), (int)restarts, 1, r->stream));
        if (const int rc = enqueueRound(r, pl, restarts, nullptr, false))
            return rc;
    }
}

// ---- wavefront.  The whole launch is enqueued without waiting for the device (enqueueRound): the kernels take their
// queue lengths from the counter block, k_tail decides for itself when to take a queue over, and the rare NaN / Inf
// restarts of a canonical launch are finished on the device too (k_finish_restarts).  The host reads ONE counter
// block per launch, after the fact (collectRender: statistics, errors, grid hints).  A step of the benchmark used
// to carry 26 host round trips (0.33 ms of idle GPU per 10 ms step, 6 % of a 1/8 tile shard's step).
//
// Measured and dropped along the way: sub-batches of one call as interleaved state machines
// (PTX_BATCHES: 1 -> 1204, 2 -> 1017, 3 -> 1006, 4 -> 733 Msamples/s -- they pass through their throughput- and
// latency-bound phases in lockstep), staggered sub-batches (the tail kernel starves beside full-size kernels), ONE
// traversal launch per bounce carrying closest(b + 1) and shadow(b) (11.4 vs 11.1 ms), a one-entry software pipeline
// in k_shade (3.50 vs 3.44 ms).
static int renderWavefront(PtxRenderer *r, RenderPlan &pl, uint32_t sampleCount)
{
    const LaunchParams &p = pl.p;
    // per launch: the handles of the process come and go (pt_stream_plan.hpp).  A handle that ASKED for one stream is enqueued exactly
    // as before, its (same-stream) waits included: only the plan's own one-stream launches leave them out.
    const StreamPlan plan = planFor(r);
    if (const int rc = ensureRenderResources(r, pl.bounces, plan))
        return rc;
    pl.aux = plan.auxOnMain ? r->stream : r->streams.aux.get();
    pl.crossWaits = !plan.auxOnMain || r->streams.auxIsMain();
    pl.sortShade = r->env.shadeSort >= 0 ? (uint32_t)r->env.shadeSort : (sceneOf(r)->scene.mixedMaterialTypes || sceneOf(r)->scene.mixedTextured) ? 1u : 0u;
    // measured with 16 hardware queues (chess_like, ms per step at 25 / 50 / 75 / 100 / 200 / 400 K live paths): whole frame 8.04 / 7.82 /
    // 7.85 / 7.80 / 8.14 / 8.13, a rank's tile shard of 8: 1.44 / 1.44 / 1.39 / 1.39 / 1.54 / 1.55, of 4: 2.29 / 2.24 / 2.24 / 2.33 / 2.34 /
    // 2.77, of 2: 3.93 / 3.89 / 3.91 / 3.98 / 4.06 / 4.41; the other scenes are flat from 50 K to 200 K
    pl.tailBelow = r->env.tailThreshold >= 0 ? (uint32_t)r->env.tailThreshold : 75000u;
    pl.wf = r->paths.view(pl.mode, r->launch.counters.p, r->launch.spill.p);
    pl.wfAux = r->paths.view(pl.mode, r->launch.counters.p, r->launch.spillAux.p);
    const bool canonical = sampleCount == 1;
    const uint64_t epoch = sceneOf(r)->link.epoch;
    // the learnt schedule belongs to (shape of the launch, scene it was learnt on); a camera or light change inside one scene
    // keeps it -- a hint that is off costs time, never results, and the tail's grid leaves room for that (enqueueBounce)
    const uint32_t *hint = canonical && r->launch.hint.matches(p.numSlots, pl.bounces, epoch) ? r->launch.hint.active.data() : nullptr;
    // the primary rays: computed by the first bounce's kernels, or handed over through memory by k_generate (PTX_FIRST_BOUNCE=0)
    const bool fresh = r->env.firstBounce;
    if (!fresh)
        k_generate<<<gridFor(p.numSlots), kBlock, 0, r->stream>>>(p, pl.wf);
    HIP_TRY(r, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(&r->launch.counters.p[C_ACTIVE0]), (int)p.numSlots, 1, r->stream));
    if (const int rc = enqueueRound(r, pl, p.numSlots, hint, fresh))
        return rc;
    if (canonical)
        finishCanonical(r, pl);
    else if (const int rc = runSampleRounds(r, pl, sampleCount))
        return rc;
    launchAccumulate(r, p);
    // (kind, bounces, tailBelow, slots -- a multi-sample launch teaches no hint --, deadSlots, epoch, verbose)
    return endLaunch(r, { PendingLaunch::kWavefront, pl.bounces, pl.tailBelow, canonical ? p.numSlots : 0u, p.numSlots - p.ownedPixels * p.frames, epoch, r->env.verbose });
}

// The launch covers the tiles of the adaptive plan in force (ptx_adaptive_plan, pt_output_host.hpp), in the plan's own tile size:
// slotPixel takes slot k's tile from the list.  Only renderImpl does this; every other launch keeps the frame.
static void coverPlan(LaunchParams &p, const OutputState::AdaptiveState &s)
{
    p.tileSize = 1u << s.tileShift;
    p.tilesX = s.plan.tilesX;
    p.numTiles = s.plan.tilesX * s.plan.tilesY;
    p.rank = 0u;
    p.worldSize = 1u;
    p.ownedTiles = s.plan.activeTiles;
    p.slotsPerFrame = s.plan.activeTiles * p.tileSize * p.tileSize;
    p.ownedPixels = s.plan.activePixels;
    p.numSlots = p.slotsPerFrame * p.frames;
    p.tileList = s.list.p;
}

static int renderImpl(PtxRenderer *r, const PtxRaygenUniformData *uniform, const PtxLightsUbo *lights, uint32_t firstFrame, uint32_t frames)
{
    if (!r || !uniform || !lights)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "ptx_render: null argument");
    if (!sceneUsable(r) || !imagePtr(r))
        return fail(r, PTX_ERROR_NOT_READY, "ptx_render: need ptx_scene_upload (or ptx_share_scene), ptx_build_accel and ptx_resize first");
    if (uniform->SampleCount == 0 || uniform->SampleCount > kMaxSampleCount || uniform->BounceCount > kMaxBounceCount || frames == 0)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "ptx_render: SampleCount must be in [1, 65535], BounceCount <= 65535");
    if (lights->LightCount > PTX_MAX_LIGHT_COUNT)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "ptx_render: LightCount %u exceeds MaxLightCount", lights->LightCount);
    RenderPlan pl;
    pl.p = makeParams(r, uniform, firstFrame, frames);
    if (r->output.adaptive.planned) // an adaptive plan is in force: its tiles, as the one shard of the frame
        coverPlan(pl.p, r->output.adaptive);
    if (const int rc = beginLaunch(r, lights, pl.p, (uint64_t)pl.p.slotsPerFrame * frames))
        return rc;
    if (pl.p.numSlots == 0)
    {
        HIP_TRY(r, hipEventRecord(r->launch.evB.get(), r->stream));
        return PTX_OK;
    }
    pl.sv = makeSceneView(r); pl.sc = makeTraceScene(r);
    pl.mode = kernelMode(r); pl.bounces = uniform->BounceCount;
    if (r->backend == PTX_BACKEND_MEGAKERNEL)
        return renderMegakernel(r, pl);
    if (pl.bounces == 0)
        return renderZeroBounces(r, pl.p, uniform->SampleCount);
    return renderWavefront(r, pl, uniform->SampleCount);
}

// ptx_render_debug: RecordPathTracingCommands with the debug pipeline bound (pt_debug_view.hpp).  One launch, enqueued like
// a wavefront launch: the counter block comes back with collectRender.
static int renderDebug(PtxRenderer *r, const PtxRaygenUniformData *uniform, const PtxLightsUbo *lights, const PtxDebugViewDesc *view)
{
    if (!r || !uniform || !lights || !view)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "ptx_render_debug: null argument");
    if (view->renderMode > PTX_DEBUG_MODE_INSTANCE || (view->raygenFlags & ~(PTX_DEBUG_RAYGEN_FORCE_OPAQUE | PTX_DEBUG_RAYGEN_CULL_BACK_FACES)) != 0u ||
        (view->hitGroupFlags & ~(PTX_DEBUG_HIT_DISABLE_COLOR_TEXTURE | PTX_DEBUG_HIT_DISABLE_NORMAL_TEXTURE | PTX_DEBUG_HIT_DISABLE_MIP_MAPS | PTX_DEBUG_HIT_DISABLE_SHADOWS)) != 0u ||
        view->reserved != 0u)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "ptx_render_debug: render mode %u, raygen flags 0x%x, hit group flags 0x%x, reserved %u", view->renderMode,
                    view->raygenFlags, view->hitGroupFlags, view->reserved);
    if (!sceneUsable(r) || !imagePtr(r))
        return fail(r, PTX_ERROR_NOT_READY, "ptx_render_debug: need ptx_scene_upload (or ptx_share_scene), ptx_build_accel and ptx_resize first");
    if (r->frame.boundShard)
        return frameIsElsewhere(r, "ptx_render_debug");
    if (lights->LightCount > PTX_MAX_LIGHT_COUNT)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "ptx_render_debug: LightCount %u exceeds MaxLightCount", lights->LightCount);
    const LaunchParams p = makeParams(r, uniform, 0, 1);
    if (const int rc = beginLaunch(r, lights, p, 0))
        return rc;
    if (p.slotsPerFrame)
    {
        const SceneView sv = makeSceneView(r);
        const TraceScene sc = makeTraceScene(r);
        const DebugPair *pairIds = sceneOf(r)->scene.debugPairs.p;
        DebugView dv;
        dv.renderMode = view->renderMode; dv.raygenFlags = view->raygenFlags; dv.hitGroupFlags = view->hitGroupFlags;
        // at most kMaxPersistentThreads threads: the global part of the traversal stack is sized for that many
        const dim3 grid(gridFor(p.slotsPerFrame, kBlock, kMaxPersistentThreads / kBlock));
        withMode(kernelMode(r), [&](auto M) {
            withFlag((view->raygenFlags & PTX_DEBUG_RAYGEN_CULL_BACK_FACES) != 0u, [&](auto CULL) {
                k_debug_view<decltype(M)::value, decltype(CULL)::value><<<grid, kBlock, 0, r->stream>>>(p, sv, sc, pairIds, dv, imagePtr(r), r->launch.counters.p, r->launch.spill.p);
            });
        });
    }
    if (const int rc = endLaunch(r, { PendingLaunch::kDebugView }))
        return rc;
    r->output.invalidate();
    return PTX_OK;
}
