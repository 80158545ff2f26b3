// stream_plan_check.cpp -- the properties of csrc/pt_stream_plan.hpp over every input the library can hand it, as a program of its own
// (tests/test_stream_plan.py compiles it with the address and undefined-behaviour sanitizers and runs it; no HIP, no GPU).
#include <cstdio>
#include <vector>

#include "pt_stream_plan.hpp"

static int failures = 0;
#define CHECK(cond, ...)                                                                                                                   \
    do                                                                                                                                     \
    {                                                                                                                                      \
        if (!(cond))                                                                                                                       \
        {                                                                                                                                  \
            failures++;                                                                                                                    \
            std::printf("FAILED %s: ", #cond);                                                                                             \
            std::printf(__VA_ARGS__);                                                                                                      \
            std::printf("\n");                                                                                                             \
        }                                                                                                                                  \
    } while (0)

int main()
{
    unsigned twoStream = 0, oneStream = 0;
    for (int enabled = 0; enabled <= 1; enabled++)
        for (int single = 0; single <= 1; single++)
            for (uint32_t handles = 1; handles <= 20; handles++)
            {
                std::vector<StreamPlan> byQueues; // the plans of this (handles, flag) row, one per queue count: kept to compare neighbours
                for (uint32_t queues = 1; queues <= 32; queues++)
                {
                    const StreamPlan p = streamPlanFor({ queues, handles, single != 0, enabled != 0 });
                    byQueues.push_back(p);
                    const bool fits = 2u * handles <= queues;
                    CHECK(p.twoStream() == !p.auxOnMain, "q %u h %u", queues, handles);
                    CHECK(p.copyGroups >= 1u && p.copyGroups <= 16u, "q %u h %u: %u copy workgroups", queues, handles, p.copyGroups);
                    CHECK(streamPlanName(p) != nullptr && streamPlanName(p)[0] != 0, "q %u h %u: no name", queues, handles);
                    if (single) // never two streams for a handle that asked for one, whatever else holds
                    {
                        CHECK(!p.twoStream(), "q %u h %u enabled %d: two streams for a single-stream handle", queues, handles, enabled);
                        CHECK(p.copyGroups == 1u, "q %u h %u: a single-stream handle keeps its copy", queues, handles);
                        continue;
                    }
                    if (!enabled) // PTX_STREAM_PLAN=0: the schedule of the rounds before
                    {
                        CHECK(p.twoStream() && !p.copyOnMain && p.copyGroups == 1u, "q %u h %u: PTX_STREAM_PLAN=0 is not the old schedule", queues, handles);
                        continue;
                    }
                    if (fits) // two streams whenever everything fits, with the copy that was the optimum there
                        CHECK(p.twoStream() && !p.copyOnMain && p.copyGroups == 1u, "q %u h %u: fits, but not the two-stream schedule", queues, handles);
                    else
                    {
                        // ... and no stream of the handle may wait for another, nor a copy hold a shared queue for milliseconds
                        CHECK(p.auxOnMain && p.copyOnMain, "q %u h %u: does not fit, but work is left on a second stream", queues, handles);
                        CHECK(p.copyGroups >= 4u, "q %u h %u: a %u-workgroup copy on a shared queue", queues, handles, p.copyGroups);
                    }
                    (p.twoStream() ? twoStream : oneStream)++;
                }
                // monotone in the queue count: more queues never take the second stream away, nor bring the short copy back
                for (size_t q = 1; q < byQueues.size(); q++)
                {
                    CHECK(!(byQueues[q - 1].twoStream() && !byQueues[q].twoStream()), "h %u: two streams with %zu queues, one with %zu", handles, q, q + 1);
                    CHECK(byQueues[q].copyGroups <= byQueues[q - 1].copyGroups, "h %u: more copy workgroups with %zu queues than with %zu", handles, q + 1, q);
                }
                // ... and in the handle count the other way round: a row with more handles is never two-stream where this one is not
                for (uint32_t queues = 1; queues <= 32; queues++)
                    if (handles < 20u)
                        CHECK(!(streamPlanFor({ queues, handles + 1u, single != 0, enabled != 0 }).twoStream() && !byQueues[queues - 1].twoStream()),
                              "q %u: two streams with %u handles, one with %u", queues, handles + 1u, handles);
            }
    // the two cases the benchmark meets: one handle alone on 4 queues, eight on 4 and on 16
    CHECK(streamPlanFor({ 4, 1, false, true }).twoStream(), "one handle on 4 queues");
    CHECK(!streamPlanFor({ 4, 8, false, true }).twoStream(), "eight handles on 4 queues");
    CHECK(streamPlanFor({ 16, 8, false, true }).twoStream(), "eight handles on 16 queues");
    CHECK(streamPlanFor({ 4, 8, false, true }) != streamPlanFor({ 16, 8, false, true }), "operator!=");
    CHECK(twoStream > 0 && oneStream > 0, "both plans must occur (%u, %u)", twoStream, oneStream);
    std::printf("%s: %u two-stream and %u one-stream plans checked\n", failures ? "FAILED" : "ok", twoStream, oneStream);
    return failures ? 1 : 0;
}
