// pt_frame_host.hpp -- the frame's hand-over, from "the samples are in the accumulation image" to "the host has them": ptx_resize,
// ptx_set_tile_shard, ptx_reset_accumulation, the two bindings of the accumulation image, the blocking and the pipelined read-back,
// and the tile-shard message of a multi-GPU frame (pack, unpack, gather).  Kernels: pt_wavefront.hpp (k_copy_out, k_pack_shard,
// k_unpack_shard, k_gather_frame); shard geometry: pt_shard_layout.hpp; state: FrameState, the member `frame` of the handle.
// Included by pt_runtime.hpp after pt_render_host.hpp (collectRender) and pt_output_host.hpp (outputResized); every function takes a valid or null handle and returns a
// PTX_* code.
#pragma once

static int resetAccumulation(PtxRenderer *r)
{
    if (!r || !r->frame.accum())
        return fail(r, PTX_ERROR_NOT_READY, "ptx_reset_accumulation: no accumulation image (call ptx_resize)");
    const FrameState &f = r->frame;
    HIP_TRY(r, hipMemsetAsync(f.target(), 0, f.boundShard ? f.boundShardBytes : f.bytes(), r->stream));
    return PTX_OK;
}

static int resizeFrame(PtxRenderer *r, uint32_t width, uint32_t height)
{
    if (!r || !width || !height || (uint64_t)width * height > 0x7fffffffull)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "ptx_resize: bad extent %ux%u", width, height);
    HIP_TRY(r, hipSetDevice(r->device));
    r->frame.width = width;
    r->frame.height = height;
    r->frame.unbind();
    r->chain.invalidate(); // guides, D, T, the histories, V_0 and the motion guides belong to the extent they were made for
    if (const int rc = outputResized(r)) // ... and so does what the output stage keeps per extent
        return rc;
    HIP_TRY(r, r->frame.image.alloc(r->frame.pixels()));
    return resetAccumulation(r);
}

static int setTileShard(PtxRenderer *r, const PtxTileShard *s)
{
    if (!r || !s || !s->worldSize || s->rank >= s->worldSize || !s->tileSize || (s->tileSize % 8) != 0 || s->tileSize > 1024)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "ptx_set_tile_shard: need rank < worldSize and tileSize a multiple of 8");
    const PtxTileShard &now = r->frame.shard;
    if (now.rank != s->rank || now.worldSize != s->worldSize || now.tileSize != s->tileSize)
    {
        r->frame.unbindShard();
        dropAdaptive(r); // an adaptive plan and its counts belong to the unsharded frame
    }
    r->frame.shard = *s;
    return PTX_OK;
}

static int bindAccumulation(PtxRenderer *r, void *devPtr, size_t bytes)
{
    if (!r || !r->frame.width)
        return fail(r, PTX_ERROR_NOT_READY, "ptx_bind_accumulation: call ptx_resize first");
    if (devPtr && bytes != r->frame.bytes())
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "ptx_bind_accumulation: buffer must be width*height*16 bytes");
    r->frame.boundImage = static_cast<float4 *>(devPtr);
    return PTX_OK;
}

static size_t shardBytes(const PtxRenderer *r, uint32_t rank)
{
    if (!r || !r->frame.width || rank >= r->frame.shard.worldSize)
        return 0;
    return (size_t)r->frame.layout(rank).slotsPerFrame * sizeof(float4);
}

// ptx_bind_shard_accumulation: the samples of a tile-sharded renderer are accumulated IN the dense tile-major buffer that is the
// message of the gather (k_accumulate's shard-major target) -- no ptx_pack_shard pass, no row-major frame on a rank that is not
// the frame's owner.  The buffer must hold this rank's shard (ptx_shard_bytes); entries of ragged tiles outside the image stay 0.
static int bindShardAccumulation(PtxRenderer *r, void *devShard, size_t bytes)
{
    if (!r || !r->frame.width)
        return fail(r, PTX_ERROR_NOT_READY, "ptx_bind_shard_accumulation: call ptx_resize and ptx_set_tile_shard first");
    const size_t need = shardBytes(r, r->frame.shard.rank);
    if (devShard && bytes < need)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "ptx_bind_shard_accumulation: the buffer must hold ptx_shard_bytes() = %zu bytes", need);
    r->frame.boundShard = static_cast<float4 *>(devShard);
    r->frame.boundShardBytes = devShard ? need : 0;
    if (devShard) // the shard buffer is laid out by the shard's own tiles: an adaptive plan ends here
        (void)adaptiveClear(r);
    return PTX_OK;
}

static int writeAccumulation(PtxRenderer *r, const float *rgba, size_t bytes)
{
    if (!r || !rgba || !r->frame.accum() || bytes != r->frame.bytes())
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "ptx_write_accumulation: buffer must be width*height*16 bytes");
    if (r->frame.boundShard)
        return frameIsElsewhere(r, "ptx_write_accumulation");
    HIP_TRY(r, hipMemcpyAsync(r->frame.accum(), rgba, bytes, hipMemcpyHostToDevice, r->stream));
    HIP_TRY(r, hipStreamSynchronize(r->stream));
    return PTX_OK;
}

static int readback(PtxRenderer *r, float *rgba, size_t bytes)
{
    if (!r || !rgba || !r->frame.accum() || bytes != r->frame.bytes())
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "ptx_readback: buffer must be width*height*16 bytes");
    if (r->frame.boundShard)
        return frameIsElsewhere(r, "ptx_readback");
    HIP_TRY(r, hipMemcpyAsync(rgba, r->frame.accum(), bytes, hipMemcpyDeviceToHost, r->stream));
    HIP_TRY(r, hipStreamSynchronize(r->stream));
    return collectRender(r); // an error of the launch that produced the image surfaces with it
}

// Device alias of a page-locked host frame (hipHostMalloc / hipHostRegister memory), looked up once per (pointer, size): the
// owner of a gathered frame passes the same few buffers step after step.  nullptr: the device cannot address the buffer.
static float4 *hostFrameAlias(PtxRenderer *r, const void *pinnedHost, size_t bytes)
{
    FrameState &f = r->frame;
    if (f.hostAlias && f.hostAliasOf == pinnedHost && f.hostAliasBytes == bytes)
        return f.hostAlias;
    void *dp = nullptr;
    if (hipHostGetDevicePointer(&dp, const_cast<void *>(pinnedHost), 0) != hipSuccess || !dp)
    {
        (void)hipGetLastError();
        return nullptr;
    }
    f.hostAliasOf = pinnedHost;
    f.hostAliasBytes = bytes;
    f.hostAlias = static_cast<float4 *>(dp);
    return f.hostAlias;
}

// The two events of the copies to the host, made on first use.  evCopied is what ptx_readback_end waits on, and the copy may be a
// kernel storing to host memory: the event must release those stores to the system scope, also for page-locked memory that is
// not host-coherent.
static int ensureCopyEvents(PtxRenderer *r)
{
    if (!r->frame.evCopied) // (the second of the two: a call that failed between them makes it again)
    {
        HIP_TRY(r, createEvent(r->frame.evSnapshot, hipEventDisableTiming));
        HIP_TRY(r, createEvent(r->frame.evCopied, hipEventDisableTiming | hipEventReleaseToSystem));
    }
    return PTX_OK;
}

// The host's frame as a target of an unpack kernel's stores: the size of the frame, page-locked memory the device can address
// (`alias`), and the events are there.  `who` names the entry point and `its` the buffer in its messages ("" / "host ").
static int hostTarget(PtxRenderer *r, const void *pinnedHost, size_t bytes, const char *who, const char *its, float4 **alias)
{
    if (bytes != r->frame.bytes())
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "%s: %s%sbuffer must be width*height*16 bytes", who, *its ? "the " : "", its);
    HIP_TRY(r, hipSetDevice(r->device));
    *alias = hostFrameAlias(r, pinnedHost, bytes);
    if (!*alias)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "%s: the %sbuffer is not page-locked memory the device can address", who, its);
    return ensureCopyEvents(r);
}

// Stores to the host's frame have been enqueued on `stream`: ptx_readback_end waits for the LAST such record, and the stores of
// everything enqueued before it are released with it.
static int markHostStoresPending(PtxRenderer *r, hipStream_t stream)
{
    HIP_TRY(r, hipEventRecord(r->frame.evCopied.get(), stream));
    r->frame.copyInFlight = true;
    return PTX_OK;
}

// How many workgroups write over the link to the host.  A FEW: what the link carries in a burst, the command processor's own
// traffic over it -- the completion signals and packet fetches of every other frame in flight -- waits behind.  PTX_COPY_GROUPS
// overrides each of the three.
enum HostCopy { kCopyReadback, kCopyUnpackShard, kCopyGather };
static uint32_t hostCopyGroups(const PtxRenderer *r, HostCopy kind, uint32_t planGroups = 1u)
{
    if (r->env.copyGroups)
        return r->env.copyGroups;
    switch (kind)
    {
    case kCopyReadback:
        // The snapshot leaves through ONE workgroup writing to the page-locked buffer (posted writes over PCIe, 33 MB in a few ms)
        // rather than through hipMemcpyAsync: a DMA burst at the link's full rate delays the completion signals and packet fetches
        // of every other frame in flight for its 1.2 ms -- measured on chess_like with 8 frames in flight: no read-back 2,600
        // Msamples/s, hipMemcpyAsync (SDMA) 2,416 / 2,422, copy kernel with 256 / 64 / 8 / 4 / 2 / 1 workgroups 2,359 / 2,395 / 2,445
        // / 2,441 / 2,465 / 2,483-2,494.
        // ... for a whole frame on one GPU.  Rank 0 of an N-GPU job renders 1 / N of the frame per step and still reads ALL of it
        // back: there the link, not the rendering, sets the pace, and one workgroup's 8 GB/s (4.1 ms per 1080p image) made a 1 / 8
        // step of chess_like 2.2 ms instead of 0.96 (tools/experiments/gather_cost.sh) -- more workgroups with more ranks.
        // ... and all of that where the copy's stream has a hardware queue to itself.  Where it shares one with other frames' streams
        // (`planGroups` of the call's StreamPlan), a copy that trickles for 4-5 ms holds THEIR kernels back for as long: it leaves
        // through as many workgroups as move it in well under a millisecond.
        return std::max(planGroups, r->frame.shard.worldSize > 1 ? std::min(16u, 2u * r->frame.shard.worldSize) : 1u);
    case kCopyUnpackShard:
        // 4 per shard -- 2 / 4 / 8 / 16 / 64 / 2,048 workgroups: 1.45 / 1.38 / 1.42 / 1.47 / 1.50 / 1.51 ms per 1 / 8 step of
        // chess_like (profiles/r05_unpack_groups.txt)
        return 4u;
    default:
        // the whole gathered frame in one launch (profiles/r05_unpack_groups.txt); a device-only gather runs at the memory's rate
        return 16u;
    }
}

// Read-back that overlaps the next launches: a device-to-device snapshot of the image on the render stream (33 MB at
// 1080p: ~20 us), then the PCIe copy on a second stream while the render stream goes on.  The reference reads its
// output back the same way, a frame late (OutputSaver.cpp:120-199).
static int readbackBegin(PtxRenderer *r, float *pinnedHost, size_t bytes)
{
    if (!r || !pinnedHost || !r->frame.accum() || bytes != r->frame.bytes())
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "ptx_readback_begin: buffer must be width*height*16 bytes");
    FrameState &f = r->frame;
    if (f.boundShard)
        return frameIsElsewhere(r, "ptx_readback_begin");
    HIP_TRY(r, hipSetDevice(r->device));
    if (const int rc = ensureCopyEvents(r))
        return rc;
    // The copy to the host rides on the renderer's auxiliary stream -- idle once the frame's shadow and tail kernels are done,
    // and not needed again before this renderer's next frame -- instead of a third stream per frame in flight: the streams of a
    // process share GPU_MAX_HW_QUEUES hardware queues, and streams on one queue run one after the other.  Where the call's plan
    // keeps the handle to ONE stream (pt_stream_plan.hpp: its two do not fit the queues), the copy follows the snapshot on the main
    // stream: a second stream's wait for the snapshot would hold whichever queue that stream shares until this frame is done.
    const StreamPlan plan = planFor(r);
    if (!plan.copyOnMain && !r->streams.aux && !f.copyStream)
        HIP_TRY(r, createStreamOn(f.copyStream, 0xffu, r->device)); // (no mask: a plain non-blocking stream)
    const hipStream_t copyOn = plan.copyOnMain ? r->stream : r->streams.aux.get() ? r->streams.aux.get() : f.copyStream.get();
    HIP_TRY(r, f.staging.alloc(f.pixels()));
    if (f.copyInFlight) // the previous copy still reads the staging image
        HIP_TRY(r, hipStreamWaitEvent(r->stream, f.evCopied.get(), 0));
    // the snapshot by a copy KERNEL (33 MB at the memory's rate: ~20 us), not hipMemcpyAsync: the runtime's device-to-device copy
    // took 0.5 ms per 1080p image and the copies of the frames in flight queue behind one another -- a floor of 0.5 ms per step
    // under every renderer that reads back, half the step of a 1 / 8 tile shard (tools/experiments/gather_cost.sh, round 5)
    if (r->env.snapshotMemcpy)
        HIP_TRY(r, hipMemcpyAsync(f.staging.p, f.accum(), bytes, hipMemcpyDeviceToDevice, r->stream));
    else
    {
        k_copy_out<<<1024, kBlock, 0, r->stream>>>(f.accum(), f.staging.p, (uint32_t)(bytes / sizeof(float4)));
        HIP_TRY(r, hipGetLastError()); // (a failed launch would hand the host a stale staging image)
    }
    if (!plan.copyOnMain || r->streams.auxIsMain()) // (a handle that asked for one stream: enqueued exactly as before)
    {
        HIP_TRY(r, hipEventRecord(f.evSnapshot.get(), r->stream));
        HIP_TRY(r, hipStreamWaitEvent(copyOn, f.evSnapshot.get(), 0));
    }
    // Host memory the device cannot address (not page-locked) takes the runtime's copy.
    float4 *const hostOnDevice = r->env.copyRuntime ? nullptr : hostFrameAlias(r, pinnedHost, bytes);
    if (hostOnDevice)
    {
        k_copy_out<<<hostCopyGroups(r, kCopyReadback, plan.copyGroups), kBlock, 0, copyOn>>>(f.staging.p, hostOnDevice, (uint32_t)(bytes / sizeof(float4)));
        HIP_TRY(r, hipGetLastError());
    }
    else
        HIP_TRY(r, hipMemcpyAsync(pinnedHost, f.staging.p, bytes, hipMemcpyDeviceToHost, copyOn));
    return markHostStoresPending(r, copyOn);
}

static int readbackEnd(PtxRenderer *r)
{
    if (!r)
        return PTX_ERROR_INVALID_ARGUMENT;
    if (r->frame.copyInFlight)
    {
        HIP_TRY(r, hipEventSynchronize(r->frame.evCopied.get()));
        r->frame.copyInFlight = false;
    }
    return PTX_OK;
}

static int packShard(PtxRenderer *r, void *devDst)
{
    if (!r || !devDst || !r->frame.accum())
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "ptx_pack_shard: null argument");
    const FrameState &f = r->frame;
    const LaunchParams p = makeParams(r, nullptr, 0, 1);
    if (f.boundShard) // the accumulation already IS the packed shard (ptx_bind_shard_accumulation)
    {
        if (devDst != f.boundShard && p.slotsPerFrame)
            HIP_TRY(r, hipMemcpyAsync(devDst, f.boundShard, (size_t)p.slotsPerFrame * sizeof(float4), hipMemcpyDeviceToDevice, r->stream));
        return PTX_OK;
    }
    if (p.slotsPerFrame)
        k_pack_shard<<<gridFor(p.slotsPerFrame), kBlock, 0, r->stream>>>(p, f.accum(), static_cast<float4 *>(devDst));
    HIP_TRY(r, hipGetLastError());
    return PTX_OK;
}

// ptx_unpack_shard / ptx_unpack_shard_host (pinnedHost != nullptr): the shard of `rank` into the device image and the host's frame
static int unpackShard(PtxRenderer *r, uint32_t rank, const void *devSrc, float *pinnedHost = nullptr, size_t hostBytes = 0)
{
    if (!r || !devSrc || !r->frame.accum() || rank >= r->frame.shard.worldSize)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "ptx_unpack_shard: bad argument");
    float4 *hostOnDevice = nullptr;
    if (pinnedHost)
        if (const int rc = hostTarget(r, pinnedHost, hostBytes, "ptx_unpack_shard_host", "", &hostOnDevice))
            return rc;
    const LaunchParams p = makeParams(r, nullptr, 0, 1, rank);
    if (p.slotsPerFrame)
    {
        uint32_t grid = gridFor(p.slotsPerFrame);
        if (hostOnDevice)
            grid = std::min(grid, hostCopyGroups(r, kCopyUnpackShard));
        k_unpack_shard<<<grid, kBlock, 0, r->stream>>>(p, static_cast<const float4 *>(devSrc), r->frame.accum(), hostOnDevice);
    }
    HIP_TRY(r, hipGetLastError());
    return hostOnDevice ? markHostStoresPending(r, r->stream) : PTX_OK;
}

// The whole gathered frame in ONE launch (k_gather_frame): `devSrc` holds the shards of ranks 0 .. worldSize-1, `strideBytes`
// apart, each in ptx_pack_shard's layout.  Targets: the device image (toDeviceImage), the host's page-locked frame, or both --
// a rank that only hands the frame to the host (OutputSaver's role, OutputSaver.cpp:120-199) never rewrites its device image.
static int unpackShards(PtxRenderer *r, const void *devSrc, size_t strideBytes, int toDeviceImage, float *pinnedHost, size_t hostBytes)
{
    if (!r || !devSrc || !r->frame.width || (!toDeviceImage && !pinnedHost))
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "ptx_unpack_shards: need the gathered shards and at least one target");
    const FrameState &f = r->frame;
    if (toDeviceImage && !f.accum())
        return fail(r, PTX_ERROR_NOT_READY, "ptx_unpack_shards: no accumulation image (call ptx_resize)");
    // the largest shard is rank 0's: it owns ceil(numTiles / worldSize) tiles, and rank k owns ceil((numTiles - k) / worldSize)
    const ShardLayout s = f.layout(0);
    const size_t largest = (size_t)s.slotsPerFrame * sizeof(float4);
    if (strideBytes < largest || strideBytes % sizeof(float4) != 0 || strideBytes / sizeof(float4) > 0xffffffffull)
        return fail(r, PTX_ERROR_INVALID_ARGUMENT, "ptx_unpack_shards: the stride must be a multiple of 16 bytes and at least the largest shard (%zu bytes)", largest);
    HIP_TRY(r, hipSetDevice(r->device));
    float4 *hostOnDevice = nullptr;
    if (pinnedHost)
        if (const int rc = hostTarget(r, pinnedHost, hostBytes, "ptx_unpack_shards", "host ", &hostOnDevice))
            return rc;
    GatherParams g;
    g.width = f.width;
    g.height = f.height;
    g.tileSize = f.shard.tileSize;
    g.tilesX = s.tilesX;
    g.worldSize = f.shard.worldSize;
    g.strideSlots = (uint32_t)(strideBytes / sizeof(float4));
    uint32_t grid = gridFor(f.pixels());
    if (hostOnDevice)
        grid = std::min(grid, hostCopyGroups(r, kCopyGather));
    k_gather_frame<<<grid, kBlock, 0, r->stream>>>(g, static_cast<const float4 *>(devSrc), toDeviceImage ? f.accum() : nullptr, hostOnDevice);
    HIP_TRY(r, hipGetLastError());
    return hostOnDevice ? markHostStoresPending(r, r->stream) : PTX_OK;
}
