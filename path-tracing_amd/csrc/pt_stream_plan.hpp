// pt_stream_plan.hpp -- which streams the kernels of ONE launch go to, as a pure function of what the process has: the hardware
// queues it is granted, the handles alive in it, and what the handle asked for.  No HIP in here (tests/test_stream_plan.py compiles
// it alone); pt_render_host.hpp and pt_frame_host.hpp evaluate it per launch, because handles come and go.
//
// Why: the runtime maps every stream of the process onto the granted queues, and the packets of one queue run one after the other.
// A stream that waits for another stream's event holds its queue for as long as it waits, and so does a kernel that runs for
// milliseconds on one workgroup.  Both are free while every stream has a queue to itself -- the two-stream schedule (shadow and tail
// kernels beside the next bounce's traversal, the read-back trickling out through one workgroup) was tuned there -- and both are
// convoys once streams of DIFFERENT frames share a queue: a frame then stands behind another frame's wait or copy.  So:
//
//   everything fits (two streams per live handle <= queues)   auxiliary work on its own stream, read-back on it through one workgroup
//   it does not                                                auxiliary work and read-back ride the main stream: no cross-stream
//                                                              event, and the copy to the host is short (kScarceCopyGroups workgroups)
//   the handle asked for one stream                            as before: one stream, the copy as it was
//   PTX_STREAM_PLAN=0                                          the schedule of the rounds before: two streams whatever the queues
#pragma once

#include <cstdint>

struct StreamPlanInput
{
    uint32_t queues;      // hardware queues the process is granted (hardwareQueuesGranted)
    uint32_t liveHandles; // handles of the process alive at this launch, this one included
    bool singleStream;    // PTX_DEVICE_SINGLE_STREAM / PTX_SINGLE_STREAM: the handle asked for one stream
    bool enabled;         // false: PTX_STREAM_PLAN=0
};

struct StreamPlan
{
    bool auxOnMain;      // shadow, k_apply_shadow and tail kernels: false = own auxiliary stream, true = the main stream
    bool copyOnMain;     // the read-back's copy to the host: false = the auxiliary stream, true = the main stream
    uint32_t copyGroups; // workgroups of that copy (a whole frame; a tile shard's rule may ask for more)
    bool twoStream() const { return !auxOnMain; }
};

static inline bool operator==(const StreamPlan &a, const StreamPlan &b)
{
    return a.auxOnMain == b.auxOnMain && a.copyOnMain == b.copyOnMain && a.copyGroups == b.copyGroups;
}
static inline bool operator!=(const StreamPlan &a, const StreamPlan &b) { return !(a == b); }

// Workgroups of the copy to the host where it shares a queue with other frames: 16 workgroups move a 1080p frame in 0.67 ms (one: 4.2-4.9 ms)
constexpr uint32_t kScarceCopyGroups = 16u;

static inline bool streamsFit(uint32_t queues, uint32_t liveHandles)
{
    return 2ull * liveHandles <= queues;
}

static inline StreamPlan streamPlanFor(const StreamPlanInput &in)
{
    if (!in.enabled) // the rounds before: the copy on the auxiliary stream, which is the main stream of a handle that asked for one
        return { in.singleStream, false, 1u };
    if (in.singleStream) // what the handle asked for is not the plan's to change: one stream, the copy it always had
        return { true, false, 1u };
    if (streamsFit(in.queues, in.liveHandles))
        return { false, false, 1u };
    return { true, true, kScarceCopyGroups };
}

static inline const char *streamPlanName(const StreamPlan &p)
{
    return !p.auxOnMain ? "two streams (auxiliary work beside the next bounce, read-back through one workgroup)"
           : p.copyGroups > 1u ? "one stream (the handle's two streams do not fit the queues: auxiliary work and a short read-back copy ride the main stream)"
                               : "one stream (asked for)";
}
