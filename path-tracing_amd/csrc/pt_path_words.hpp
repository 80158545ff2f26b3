// pt_path_words.hpp -- the words of the per-slot path state that are no plain float: what is packed into the spare .w of the
// records (pt_path_state.hpp says which record carries which word on which route) and the reserved patterns of the 32-bit ids.
// Pure functions on bit patterns with no HIP in them: the header compiles alone with the host compiler (tests/test_path_words.py)
// and is used as it stands by the device code.
#pragma once

#include <cstdint>

#if defined(__HIP__) || defined(__HIPCC__)
#define PT_WORD_FN __host__ __device__ __forceinline__ constexpr
#else
#define PT_WORD_FN inline constexpr
#endif

PT_WORD_FN uint32_t floatBits(float f) { return __builtin_bit_cast(uint32_t, f); }
PT_WORD_FN float bitsFloat(uint32_t w) { return __builtin_bit_cast(float, w); }

// ---- the state word: bounce | smpl << 16 (rayD.w of a live path, shC.w of one that ended with its shadow query pending) ----
// bounce = segments of the current sample behind the path, smpl = samples of this launch behind the slot.  0 = first bounce of
// the first sample: the one state at which rad[slot] holds nothing yet and is not read.
constexpr uint32_t kMaxSampleCount = 0xffffu, kMaxBounceCount = 0xffffu; // what ptx_render accepts (renderImpl): 16 bits each
PT_WORD_FN uint32_t packState(uint32_t bounce, uint32_t smpl) { return bounce | smpl << 16; }
PT_WORD_FN uint32_t stateBounce(uint32_t state) { return state & 0xffffu; }
PT_WORD_FN uint32_t stateSample(uint32_t state) { return state >> 16; }
PT_WORD_FN uint32_t withBounce(uint32_t state, uint32_t bounce) { return (state & 0xffff0000u) | bounce; }
// rayD.w of a slot outside the image (ragged edge tiles) under k_generate's schedule: the one pattern no live state word takes.
// A stored smpl is below SampleCount <= kMaxSampleCount, so the upper half of a live word is at most 0xfffe.  The sign bit alone
// would not do -- smpl >= 0x8000 sets it in a live word -- so the reader compares the whole pattern; as floats the words are
// denormals and NaNs, and no float comparison is made on them anywhere.
constexpr uint32_t kDeadWord = 0xffffffffu;

// ---- the shadow length: shD.w = the distance to the light, its sign bit = "the path ends after this bounce" ----
// The distance is a length or 100000, never negative; flag and length are set and tested on the bit pattern.
PT_WORD_FN uint32_t packShadowLength(float lightDistance, bool endsPath)
{
    return (floatBits(lightDistance) & 0x7fffffffu) | (endsPath ? 0x80000000u : 0u);
}
PT_WORD_FN float shadowLength(uint32_t w) { return bitsFloat(w & 0x7fffffffu); }
PT_WORD_FN bool shadowEndsPath(uint32_t w) { return (w >> 31) != 0u; }

// ---- the shadow result byte: one per shadow queue entry, k_trace_shadow -> k_apply_shadow.  0 = nothing to do for the entry ----
constexpr uint32_t kShadowLightVisible = 1u; // add the contribution k_shade prepared
constexpr uint32_t kShadowEndsPath = 2u;     // finish the sample: the path ended on this bounce
PT_WORD_FN uint8_t packShadowResult(bool occluded, bool endsPath)
{
    return (uint8_t)((occluded ? 0u : kShadowLightVisible) | (endsPath ? kShadowEndsPath : 0u));
}

// ---- reserved ids.  Three of them and kDeadWord are all-ones: four meanings in four value spaces, told apart by their names ----
constexpr uint32_t kMissPair = 0xffffffffu; // hitPair: the ray left the scene (Hit::pair of a miss, pt_bvh.hpp)
constexpr uint32_t kDeadPair = 0xfffffffeu; // hitPair of a slot outside the image: neither shaded nor sorted as a miss
constexpr uint32_t kNoPixel = 0xffffffffu;  // slotPixel: the slot of a ragged edge tile lies outside the image
constexpr uint32_t kPadSlot = 0xffffffffu;  // sorted shade queue: padding past the end of the queue.  Never a slot: 152 B of state
                                            // per slot bound the count far below
