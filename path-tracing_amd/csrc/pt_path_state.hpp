// pt_path_state.hpp -- the per-slot state of the paths in flight: the records (struct Wavefront), how they are streamed, and ONE
// named load / store per record and per meaning of its spare word.  The kernels of pt_wavefront.hpp go through these and build
// no record by hand; the words themselves are pt_path_words.hpp's.
//
// Every record is 16 bytes (hitPair, decalT: 4; the result byte: 1), written by one kernel and read once by the next.  There is no
// record for the RNG state and bounce | smpl << 16 (the state word): they ride as bit patterns in the .w of records that travel
// anyway.  Pixel and frame are functions of the slot (slotFrame, slotPixel) and are stored nowhere.  Who writes and who reads what:
//
//   hand-over      writer -> reader                                    records
//   continuation   k_shade, k_restart, k_generate                      rayO  (origin, MaxRoughness)
//                    -> k_trace_closest, next k_shade, k_tail          rayD  (direction, state word -- or kDeadWord: k_generate, slot outside the image)
//                                                                      thr   (throughput, RNG state)
//                                                                      rad   (radiance of the launch so far; read only if state != 0)
//                                                                      diff  (ray differentials, three records; scenes with textures)
//   hit            k_trace_closest -> k_shade                          hit   (t, u, v, triangle slot in leaf order)
//                                                                      hitPair (pair, kMissPair or kDeadPair)
//                                                                      decal + decalT (nearest ignored any-hit candidate and its distance,
//                                                                            -1 = none; scenes with non-opaque geometry)
//   shadow query   k_shade -> k_trace_shadow, k_apply_shadow           rayO.xyz (the shadow ray leaves where the continuation ray does)
//                                                                      shD   (direction, packed shadow length)
//                                                                      shC   (contribution, state word)
//                                                                      rayO.w = RNG state, for a path that ENDED with the query pending
//                                                                            (it has no use for MaxRoughness and writes no rayD / thr)
//                                                                      shadowResult (the result byte, per queue entry)
//   restart        finishSample (k_shade, k_apply_shadow), k_tail      rad, and as single words thr.w = RNG state, carried on, and
//                    -> k_restart, k_finish_restarts                   rayD.w = state word of the next sample (bounce 0)
//   final          any -> k_accumulate                                 slotRad
//
// A reader skips what it has no use for -- rad at state 0, rayO on a miss, shC for an occluded light on a live path -- so the
// accessors are per record, not per hand-over, and each does exactly one access of the width and kind its name says.
#pragma once

#include "pt_device.hpp"
#include "pt_path_words.hpp"

using namespace ptd;

// Per-slot path state is written by one kernel and read once by the next: a stream.  Its loads and stores carry the
// non-temporal hint (global_load / global_store ... nt), so that the 4 MB of L2 an XCD has keep tree nodes and texels instead
// of records nobody reads twice.  Measured (1 MI355X, 1080p, 8 spp, two runs each in one call, plain -> nt): atrium_like
// 788 / 789 -> 811 / 823 Msamples/s, chess_like 2,248 / 2,229 -> 2,267 / 2,262, temple_like 898 / 883 -> 905 / 895, street_like
// flat; the hint on the loads alone or on the stores alone gives half of it; on the ShadeTri reads it costs 4 % (the samples
// of one pixel sit in neighbouring lanes and share them).
template <typename T> struct StreamWord { typedef T type; };
template <> struct StreamWord<float4> { typedef float type __attribute__((ext_vector_type(4))); };
template <> struct StreamWord<uint4> { typedef uint32_t type __attribute__((ext_vector_type(4))); };
template <typename T> struct StreamRef
{
    T *p;
    typedef typename StreamWord<T>::type W;
    PT_DEV operator T() const
    {
        const W w = __builtin_nontemporal_load(reinterpret_cast<const W *>(p));
        T v;
        __builtin_memcpy(&v, &w, sizeof(T));
        return v;
    }
    PT_DEV void operator=(const T &v) const
    {
        W w;
        __builtin_memcpy(&w, &v, sizeof(T));
        __builtin_nontemporal_store(w, reinterpret_cast<W *>(p));
    }
};
template <typename T> struct Stream // wf.rayO[slot] is the streamed access; wf.rayO.p[slot] is the plain one (single words)
{
    T *p;
    PT_DEV StreamRef<T> operator[](size_t i) const { return StreamRef<T>{p + i}; }
    __host__ __device__ Stream &operator=(T *q) { p = q; return *this; }
    __host__ __device__ explicit operator bool() const { return p != nullptr; }
};

struct Wavefront // device pointers of the per-slot state (SoA); the table above says what travels where
{
    Stream<float4> rayO;    // origin | MaxRoughness, or the RNG state of a path that ended with its shadow query pending
    Stream<float4> rayD;    // direction | state word, or kDeadWord
    Stream<float4> thr;     // throughput | RNG state
    Stream<float4> rad;     // radiance accumulated over the samples of this launch
    Stream<float4> hit;     // t, u, v | triangle slot
    Stream<uint32_t> hitPair;
    Stream<float4> shD;     // shadow direction | packed shadow length
    Stream<float4> shC;     // NEE contribution | state word
    Stream<float4> slotRad; // final radiance of the slot
    Stream<float4> decal;   // triangle slot, u, v, pair of the nearest ignored any-hit candidate; null unless the scene has non-opaque geometry
    Stream<float> decalT;   // its distance, or -1
    Stream<float4> diff[3]; // payload.RayDifferentials0..2; null unless the scene has textures
    uint32_t *queue[2];
    uint32_t *shadowQueue;
    uint8_t *shadowResult; // per shadow queue entry: packShadowResult
    uint32_t *restartQueue;
    uint32_t *counters; // see enum Counter
    uint32_t *spill;    // traversal stack overflow region [kGlobalSpill][kMaxPersistentThreads]
};

PT_DEV float4 record(f3 v, float w) { return make_float4(v.x, v.y, v.z, w); }
PT_DEV float4 record(f3 v, uint32_t w) { return make_float4(v.x, v.y, v.z, __uint_as_float(w)); }

// ---- continuation ----------------------------------------------------------------------------------------------------------------
PT_DEV void storeRayOrigin(const Wavefront &wf, uint32_t slot, f3 o, float maxRoughness) { wf.rayO[slot] = record(o, maxRoughness); }
// k_shade's store: the hit point, from which the continuation ray and the shadow ray leave.  A path that ends here with its shadow
// query pending keeps its RNG state in the word (k_apply_shadow may find the slot due a restart); a live one MaxRoughness.
PT_DEV void storeHitPoint(const Wavefront &wf, uint32_t slot, f3 position, bool pathEnded, float maxRoughness, uint32_t rng)
{
    wf.rayO[slot] = record(position, pathEnded ? __uint_as_float(rng) : maxRoughness);
}
PT_DEV void loadRayOrigin(const Wavefront &wf, uint32_t slot, f3 &o, float &maxRoughness)
{
    const float4 o4 = wf.rayO[slot];
    o = F3(o4.x, o4.y, o4.z);
    maxRoughness = o4.w;
}
PT_DEV uint32_t endedPathRng(const Wavefront &wf, uint32_t slot) { return __float_as_uint(wf.rayO.p[slot].w); } // one word

PT_DEV void storeRayDirection(const Wavefront &wf, uint32_t slot, f3 d, uint32_t state) { wf.rayD[slot] = record(d, state); }
PT_DEV void storeDeadSlot(const Wavefront &wf, uint32_t slot) { wf.rayD[slot] = record(F3s(0.0f), kDeadWord); }
PT_DEV void loadRayDirection(const Wavefront &wf, uint32_t slot, f3 &d, uint32_t &state) // state == kDeadWord: nothing else of the slot is valid
{
    const float4 d4 = wf.rayD[slot];
    d = F3(d4.x, d4.y, d4.z);
    state = __float_as_uint(d4.w);
}

PT_DEV void storeThroughput(const Wavefront &wf, uint32_t slot, f3 throughput, uint32_t rng) { wf.thr[slot] = record(throughput, rng); }
PT_DEV void loadThroughput(const Wavefront &wf, uint32_t slot, f3 &throughput, uint32_t &rng)
{
    const float4 t4 = wf.thr[slot];
    throughput = F3(t4.x, t4.y, t4.z);
    rng = __float_as_uint(t4.w);
}

PT_DEV void storeRadiance(const Wavefront &wf, uint32_t slot, f3 radiance) { wf.rad[slot] = record(radiance, 0.0f); }
PT_DEV f3 loadRadiance(const Wavefront &wf, uint32_t slot) // not at state 0: nothing has written it yet
{
    const float4 r4 = wf.rad[slot];
    return F3(r4.x, r4.y, r4.z);
}

// the payload packing of raygen.rgen:56-58 / closestHit.rchit:157-159
PT_DEV void storeDiff(const Wavefront &wf, uint32_t slot, const DiffRays &d)
{
    wf.diff[0][slot] = make_float4(d.rxOrigin.x, d.rxOrigin.y, d.rxOrigin.z, d.rxDirection.x);
    wf.diff[1][slot] = make_float4(d.rxDirection.y, d.rxDirection.z, d.ryOrigin.x, d.ryOrigin.y);
    wf.diff[2][slot] = make_float4(d.ryOrigin.z, d.ryDirection.x, d.ryDirection.y, d.ryDirection.z);
}
PT_DEV DiffRays loadDiff(const Wavefront &wf, uint32_t slot)
{
    const float4 a = wf.diff[0][slot], b = wf.diff[1][slot], c = wf.diff[2][slot];
    DiffRays d;
    d.rxOrigin = F3(a.x, a.y, a.z);
    d.rxDirection = F3(a.w, b.x, b.y);
    d.ryOrigin = F3(b.z, b.w, c.x);
    d.ryDirection = F3(c.y, c.z, c.w);
    return d;
}

// ---- hit ---------------------------------------------------------------------------------------------------------------------------
PT_DEV void storeHit(const Wavefront &wf, uint32_t slot, float t, float u, float v, uint32_t triSlot)
{
    wf.hit[slot] = make_float4(t, u, v, __uint_as_float(triSlot));
}
PT_DEV void loadHit(const Wavefront &wf, uint32_t slot, float &t, float &u, float &v, uint32_t &triSlot)
{
    const float4 h = wf.hit[slot];
    t = h.x; u = h.y; v = h.z;
    triSlot = __float_as_uint(h.w);
}
PT_DEV uint32_t hitTriSlot(const Wavefront &wf, uint32_t slot) { return __float_as_uint(wf.hit.p[slot].w); } // one word
PT_DEV void storeHitPair(const Wavefront &wf, uint32_t slot, uint32_t pair) { wf.hitPair[slot] = pair; }
PT_DEV uint32_t loadHitPair(const Wavefront &wf, uint32_t slot) { return wf.hitPair[slot]; }

// anyhit.rahit state of a ray (scenes with non-opaque geometry: wf.decalT is null otherwise and the caller asks)
PT_DEV void storeDecalDistance(const Wavefront &wf, uint32_t slot, float t) { wf.decalT[slot] = t; } // -1: a fresh ray, nothing ignored yet
PT_DEV float decalDistance(const Wavefront &wf, uint32_t slot) { return wf.decalT[slot]; }
PT_DEV uint32_t decalTriSlot(const Wavefront &wf, uint32_t slot) { return __float_as_uint(wf.decal.p[slot].x); } // one word
PT_DEV void storeDecal(const Wavefront &wf, uint32_t slot, uint32_t triSlot, float u, float v, float pairBits) // behind its distance
{
    wf.decal[slot] = make_float4(__uint_as_float(triSlot), u, v, pairBits);
}
PT_DEV Decal loadDecal(const Wavefront &wf, uint32_t slot) // the record itself only behind a distance
{
    Decal decal = noDecal();
    decal.dist = wf.decalT[slot];
    if (decal.dist != -1.0f)
    {
        const float4 dq = wf.decal[slot];
        decal.slot = __float_as_uint(dq.x);
        decal.u = dq.y;
        decal.v = dq.z;
        decal.pair = __float_as_uint(dq.w);
    }
    return decal;
}

// ---- shadow query ------------------------------------------------------------------------------------------------------------------
// What k_shade leaves beside the hit point (storeHitPoint): the ray, and what k_apply_shadow needs to add the light and to finish
// a path that ends here -- `state` beside the contribution, the flag in the length word.
PT_DEV void storeShadowQuery(const Wavefront &wf, uint32_t slot, f3 direction, float lightDistance, bool endsPath, f3 contribution, uint32_t state)
{
    wf.shD[slot] = record(direction, packShadowLength(lightDistance, endsPath));
    wf.shC[slot] = record(contribution, state);
}
PT_DEV void loadShadowRay(const Wavefront &wf, uint32_t slot, f3 &o, f3 &d, uint32_t &lengthWord) // shadowLength / shadowEndsPath of the word
{
    const float4 o4 = wf.rayO[slot], d4 = wf.shD[slot];
    o = F3(o4.x, o4.y, o4.z);
    d = F3(d4.x, d4.y, d4.z);
    lengthWord = __float_as_uint(d4.w);
}
PT_DEV void loadShadowContribution(const Wavefront &wf, uint32_t slot, f3 &contribution, uint32_t &state)
{
    const float4 c = wf.shC[slot];
    contribution = F3(c.x, c.y, c.z);
    state = __float_as_uint(c.w);
}

// ---- restart -----------------------------------------------------------------------------------------------------------------------
// What a slot in the restart queue hands to k_restart / k_finish_restarts beside rad[slot]: the RNG state, carried on, and the
// state word of its next sample, as single words where a live path has them (thr.w, rayD.w).  Rare in a canonical launch (a NaN).
PT_DEV void storeRestart(const Wavefront &wf, uint32_t slot, uint32_t rng, uint32_t state)
{
    wf.thr.p[slot].w = __uint_as_float(rng);
    wf.rayD.p[slot].w = __uint_as_float(state);
}
PT_DEV void loadRestart(const Wavefront &wf, uint32_t slot, uint32_t &rng, uint32_t &state)
{
    rng = __float_as_uint(wf.thr.p[slot].w);
    state = __float_as_uint(wf.rayD.p[slot].w);
}

// ---- final -------------------------------------------------------------------------------------------------------------------------
PT_DEV void storeFinal(const Wavefront &wf, uint32_t slot, f3 radiance) { wf.slotRad[slot] = record(radiance, 0.0f); }
