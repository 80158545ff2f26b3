// pt_chain_state.hpp -- the bookkeeping of the interactive chain (guide pass, temporal accumulation, the filters; semantics:
// include/ptx.h, docs/NEXT_ROWS.md sections 13-20): what is ready, which ping-pong copy is current, whether the moments are live and
// which pose a history leads back to, with every event that changes them as one member function.  No buffers, no matrices and no HIP
// in here (tests/test_chain_state.py compiles it alone); ChainState (pt_runtime.hpp) holds one beside the images, and
// pt_chain_host.hpp, pt_frame_host.hpp and pt_scene_host.hpp report the events.
#pragma once

#include <cstdint>

enum class PrevPoseSource { kUnknown, kCurrent, kSnapshot }; // the pose ptx_render_guides_motion takes for "previous"

struct ChainStatus
{
    static constexpr uint64_t kNoPose = ~0ull;
    bool guidesReady = false;   // a guide pass since the last ptx_resize
    int denoisedIn = -1;        // which of the two filter images holds D (-1: nothing denoised since the last ptx_resize)
    bool temporalReady = false; // T holds the result of an accumulate call
    int historyIn = -1;         // which copy of the history the last accepted accumulate call wrote (-1: none since the last ptx_resize)
    bool momentsLive = false;   // that call was a moments call: copy `historyIn` of the moment history is current
    bool fastLive = false;      // that call was a responsive call: copy `historyIn` of the fast history is current
    bool varianceReady = false; // V_0 of a ptx_denoise_variance
    bool motionReady = false;   // the motion images belong to the current guides
    bool specularReady = false; // a ptx_render_guides_specular since the last ptx_resize: the fourth image exists
    bool despikedReady = false; // a ptx_despike since the last ptx_resize: C exists
    bool useDespiked = false;   // ptx_chain_use_despiked: the calls that read the sum read C; sticky, ptx_resize keeps it
    // pose serials (SceneData::PoseTracking): the one the guides were rendered at, the one the history was made from, and the history
    // pose the motion images lead back to (kNoPose: there was no history)
    uint64_t guidesPose = kNoPose, temporalPose = kNoPose, motionFromPose = kNoPose;

    uint64_t historyPose() const { return historyIn >= 0 ? temporalPose : kNoPose; }
    // the motion images belong to the guides they were rendered with and lead back to the history as it stood then
    bool motionFresh() const { return motionReady && motionFromPose == historyPose(); }
    bool momentsCurrent() const { return temporalReady && momentsLive; }
    bool fastCurrent() const { return temporalReady && fastLive; }
    // `from`: the history's pose; `serial`: the scene's; a valid snapshot holds the pose of serial - 1
    static PrevPoseSource prevPoseSource(uint64_t from, uint64_t serial, bool snapshotValid)
    {
        if (from == serial)
            return PrevPoseSource::kCurrent;
        return snapshotValid && from != kNoPose && from + 1u == serial ? PrevPoseSource::kSnapshot : PrevPoseSource::kUnknown;
    }

    // ptx_resize: everything belongs to the extent it was made for (the serials stay: nothing is left that they describe)
    void resize()
    {
        guidesReady = temporalReady = momentsLive = fastLive = varianceReady = motionReady = specularReady = despikedReady = false;
        denoisedIn = historyIn = -1;
    }
    // ptx_scene_upload, its streamed form, ptx_share_scene: guides and history lead back to no pose of the new scene, the motion images are stale
    void sceneChanged()
    {
        guidesPose = temporalPose = kNoPose;
        motionReady = false;
    }
    // an accepted guide pass at the scene's `serial`; a plain one leaves the motion images behind the guides: stale
    void guidesRendered(uint64_t serial, bool motion)
    {
        motionFromPose = historyPose();
        guidesReady = true;
        guidesPose = serial;
        motionReady = motion;
    }
    // an accepted ptx_render_guides_specular, beside its guidesRendered(serial, false)
    void specularRendered() { specularReady = true; }
    // An accepted accumulate call.  The history ping-pongs (a thread reads q while its neighbour writes it) and the moment history with
    // it: `src` is read where there is a history and the call did not ask for PTX_TEMPORAL_RESET (useHistory), its moments where they are
    // live too (useMoments: without, they restart on the colour history as it stands); `dst` is written.  A plain call drops the moments.
    // The fast history of a responsive call (`fast`, docs/NEXT_ROWS.md section 19) ping-pongs and is dropped in the same way (useFast).
    struct Accumulate { int src, dst; bool useHistory, useMoments, useFast; };
    Accumulate accumulate(bool moments, bool reset, bool fast = false)
    {
        const bool useHistory = historyIn >= 0 && !reset;
        const Accumulate a = { historyIn, historyIn == 0 ? 1 : 0, useHistory, useHistory && momentsLive, useHistory && fastLive };
        historyIn = a.dst;
        momentsLive = moments;
        fastLive = fast;
        temporalReady = true;
        temporalPose = guidesPose; // the history now leads back to the pose its guides were rendered at
        return a;
    }
    // an accepted ptx_despike (docs/NEXT_ROWS.md section 20)
    void despiked() { despikedReady = true; }
    // the filters: iteration i writes filter image i & 1
    void filtered(uint32_t iterations) { denoisedIn = (int)((iterations - 1u) & 1u); }
    void varianceFiltered(uint32_t iterations) { filtered(iterations); varianceReady = true; }
};
