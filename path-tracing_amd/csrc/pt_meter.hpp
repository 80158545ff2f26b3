// pt_meter.hpp -- exposure metering between the interactive chain and the output stage (docs/NEXT_ROWS.md section 21; semantics:
// include/ptx.h ptx_meter, steps 1 - 9): a weighted luminance histogram of the image the output stage is about to read, and from it
// the exposure that ptx_postprocess_metered multiplies in.  Three kernels, host side in pt_output_host.hpp:
//
//   k_meter_histogram<MODE>  one load per pixel (the compiler narrows the float4 to the 12 bytes used), grid-stride over a grid
//                            capped at kMeterGridCap workgroups.  Class and bin come from the bits of the luminance (two compares on
//                            the exponent field, one shift); the bins are summed with LDS integer atomics into one 1 KB histogram
//                            per workgroup, the four class counters in registers and then once per thread into LDS.  Every workgroup stores its 256 bins and 4 counters as one
//                            slab of kMeterSlabWords words with plain stores: nothing is zeroed between calls, there is no global
//                            atomic, and integer sums have no order to depend on.
//   k_meter_resolve          one workgroup of four slices of 256 threads: thread i of slice q sums bin i over every fourth slab from
//                            slab q on (one coalesced 1 KB row per slab, sixteen rows in flight per thread), the first four threads
//                            also a counter each; the slices meet in LDS; the first slice scans the 256 bins (Hillis-Steele, eight
//                            rounds), thread i keeps kept_i and adds it to K, A and B_(i & 7) with 64-bit LDS atomics; thread 0
//                            does the float64 of steps 6 - 8 and writes the state.  Why this shape and not 256 threads with one
//                            lane's loop: the measured variants of section 21.
//   k_meter_reset            the state ptx_resize and ptx_meter_reset leave: exposure 1, everything else zero.
//
// LDS: 1,040 B in the histogram, 4,240 B in the resolve; the atomics of a wave land on as many banks as its luminances differ in
// sub-bin, and 64 lanes on one bin (a constant image) are the worst case, measured in section 21.  All device memory is written with
// the compiler's ordinary vector stores.  -ffp-contract=off keeps every product and sum of steps 6 - 8 an operation of its own; the
// double division is the compiler's IEEE sequence (v_div_scale_f64, v_rcp_f64, v_fma_f64 ..., v_div_fmas_f64, v_div_fixup_f64).
#pragma once

#include "pt_variance.hpp"

constexpr int kMeterBlock = 256;
constexpr uint32_t kMeterGridCap = 1024;   // workgroups of k_meter_histogram, and so slabs k_meter_resolve sums
constexpr uint32_t kMeterSlabWords = 260;  // 256 bins, then black, rejected, under, over
constexpr uint32_t kMeterResolveSlices = 4; // k_meter_resolve: 256 threads per slice of the slabs
constexpr int kMeterResolveBlock = 256 * kMeterResolveSlices;
static_assert(kMeterSlabWords == 260, "k_meter_resolve reads counter t & 3");

// What lives in device memory (step 9): the result first, so that ptx_device_meter_ptr is its address
struct MeterState
{
    PtxMeterResult result;
    uint32_t bins[256];
    double cur;       // log2 of the exposure, the adapted state
    uint32_t started; // a valid call since the last reset: the next one adapts instead of jumping
    uint32_t pad;
};
static_assert(sizeof(PtxMeterResult) == 48 && offsetof(MeterState, bins) == 48 && offsetof(MeterState, cur) == 1072, "MeterState layout");

struct MeterArgs
{
    const float4 *source;
    uint32_t *slabs; // gridDim.x x kMeterSlabWords
    uint32_t n, width, height;
    float totalSamples;      // (float)totalSamples
    uint32_t x0, x1, y0, y1; // PTX_METER_REGION
};

// step 4, PTX_METER_CENTRE: 1 + [W <= 4x + 2 <= 3W] + [3W <= 8x + 4 <= 5W] (64-bit: 8x + 4 and 5W pass 2^32 on a very wide image)
PT_DEV uint32_t meterCentreWeight(uint32_t x, uint32_t W)
{
    const uint64_t x4 = 4ull * x + 2ull, x8 = 8ull * x + 4ull, w = W;
    return 1u + ((w <= x4 && x4 <= 3ull * w) ? 1u : 0u) + ((3ull * w <= x8 && x8 <= 5ull * w) ? 1u : 0u);
}

template <uint32_t MODE>
__global__ void __launch_bounds__(kMeterBlock) k_meter_histogram(MeterArgs a)
{
    __shared__ uint32_t hist[kMeterSlabWords];
    const uint32_t t = threadIdx.x;
    hist[t] = 0u;
    if (t < kMeterSlabWords - 256u)
        hist[256u + t] = 0u;
    __syncthreads();
    const float rs = rcp_(a.totalSamples); // operator/(f3, float): this reciprocal and three multiplies
    uint32_t black = 0u, rejected = 0u, under = 0u, over = 0u;
    for (uint32_t i = blockIdx.x * kMeterBlock + t; i < a.n; i += gridDim.x * kMeterBlock) // n < 2^31: the index cannot wrap
    {
        uint32_t w = 1u;
        if (MODE != PTX_METER_AVERAGE)
        {
            const uint32_t y = i / a.width, x = i - y * a.width;
            if (MODE == PTX_METER_CENTRE)
                w = meterCentreWeight(x, a.width) * meterCentreWeight(y, a.height);
            else if (x < a.x0 || x >= a.x1 || y < a.y0 || y >= a.y1)
                continue; // weight 0: in no class
        }
        const float4 s = a.source[i];
        const float Y = luminance_(F3(s.x * rs, s.y * rs, s.z * rs));
        const uint32_t bits = __float_as_uint(Y), e = bits >> 23; // sign and exponent field
        if ((e & 0xffu) == 0xffu)
            rejected += w; // NaN, +-Inf
        else if (e - 1u >= 254u)
            black += w; // the sign set, zero or a denormal: Y <= 0 or Y < 2^-126
        else
        {
            int k = (int)(bits >> 20) - 888;
            if (k < 0)
            {
                under += w;
                k = 0;
            }
            if (k > 255)
            {
                over += w;
                k = 255;
            }
            atomicAdd(&hist[k], w);
        }
    }
    if (black)
        atomicAdd(&hist[256], black);
    if (rejected)
        atomicAdd(&hist[257], rejected);
    if (under)
        atomicAdd(&hist[258], under);
    if (over)
        atomicAdd(&hist[259], over);
    __syncthreads();
    uint32_t *slab = a.slabs + (size_t)blockIdx.x * kMeterSlabWords;
    slab[t] = hist[t];
    if (t < kMeterSlabWords - 256u)
        slab[256u + t] = hist[256u + t];
}

struct MeterResolveArgs
{
    const uint32_t *slabs;
    uint32_t slabCount;
    MeterState *state;
    uint32_t lowPermille, highPermille;
    float keyLog2, compensation, minLog2Exposure, maxLog2Exposure, speedUp, speedDown, deltaSeconds;
};

// T_j of step 6: the doubles nearest to log2(1 + (2j + 1) / 16)
__device__ const double kMeterSubBinLog2[8] = { 0x1.663f6fac91316p-4, 0x1.fbc16b902680ap-3, 0x1.91bba891f1709p-2, 0x1.0c10500d63aa6p-1,
                                                0x1.49a784bcd1b8bp-1, 0x1.82809d5be7073p-1, 0x1.b74948f5532dap-1, 0x1.e88c6b3626a73p-1 };

PT_DEV double meterClamp(double x, double lo, double hi)
{
    const double m = x < lo ? lo : x; // max(x, lo)
    return hi < m ? hi : m;           // min(., hi)
}

__global__ void __launch_bounds__(kMeterResolveBlock) k_meter_resolve(MeterResolveArgs a)
{
    __shared__ uint32_t part[kMeterResolveSlices][kMeterSlabWords];
    __shared__ unsigned long long acc[10]; // K, A and B_0 ... B_7 of steps 5 and 6
    if (threadIdx.x < 10u)
        acc[threadIdx.x] = 0ull;
    const uint32_t t = threadIdx.x & 255u, q = threadIdx.x >> 8; // word t of every kMeterResolveSlices-th slab, from slab q on
    const bool counter = t < kMeterSlabWords - 256u;
    uint32_t sum = 0u, c = 0u;
    // Sixteen slabs' bin and counter words are loaded before the first is added (the loads of a plain loop were waited for within
    // four iterations).  Every thread loads a counter, t & 3, and only the first four keep it: a load behind a branch is waited
    // for at once.
    constexpr uint32_t kBatch = 16u;
    uint32_t s = q;
    for (; s + (kBatch - 1u) * kMeterResolveSlices < a.slabCount; s += kBatch * kMeterResolveSlices)
    {
        uint32_t v[kBatch], w[kBatch];
#pragma unroll
        for (uint32_t j = 0; j < kBatch; j++)
        {
            const uint32_t *slab = a.slabs + (size_t)(s + j * kMeterResolveSlices) * kMeterSlabWords;
            v[j] = slab[t];
            w[j] = slab[256u + (t & 3u)];
        }
#pragma unroll
        for (uint32_t j = 0; j < kBatch; j++)
        {
            sum += v[j];
            c += w[j];
        }
    }
    for (; s < a.slabCount; s += kMeterResolveSlices)
    {
        const uint32_t *slab = a.slabs + (size_t)s * kMeterSlabWords;
        sum += slab[t];
        c += slab[256u + (t & 3u)];
    }
    part[q][t] = sum;
    if (counter)
        part[q][256u + t] = c;
    __syncthreads();
    uint32_t *bins = part[0];
    MeterState &st = *a.state;
    if (q == 0u) // the first slice adds the others' columns to its own: a thread reads and writes column t only
    {
#pragma unroll
        for (uint32_t k = 1; k < kMeterResolveSlices; k++)
        {
            sum += part[k][t];
            c += part[k][256u + (counter ? t : 0u)];
        }
        bins[t] = sum;
        if (counter)
            bins[256u + t] = c;
        st.bins[t] = sum;
        part[1][t] = sum; // the scan's input: this thread's own column, which nobody else reads before the barrier
    }
    // step 5: inclusive prefix sums of the bins (Hillis-Steele between the second and third slice's columns, which are free now):
    // eight rounds, every thread of the workgroup at every barrier.  They fit 32 bits: N < 2^32 by the bound of step 4.
    uint32_t *from = part[1], *to = part[2];
    for (uint32_t d = 1u; d < 256u; d <<= 1)
    {
        __syncthreads();
        if (q == 0u)
            to[t] = from[t] + (t >= d ? from[t - d] : 0u);
        uint32_t *const swap = from;
        from = to;
        to = swap;
    }
    __syncthreads();
    const uint64_t N = from[255];
    if (q == 0u) // thread i keeps kept_i; the integer sums of steps 5 and 6 meet in LDS atomics, which have no order to depend on
    {
        const uint64_t lo = N * a.lowPermille / 1000ull, hi = N * a.highPermille / 1000ull, top = N - hi;
        const uint64_t n = sum, P = (uint64_t)from[t] - n, end = P + n < top ? P + n : top, begin = P > lo ? P : lo;
        const uint64_t kept = end > begin ? end - begin : 0ull;
        if (kept)
        {
            atomicAdd(&acc[0], (unsigned long long)kept);
            atomicAdd(&acc[1], (unsigned long long)(kept * (uint64_t)(t >> 3)));
            atomicAdd(&acc[2u + (t & 7u)], (unsigned long long)kept);
        }
    }
    __syncthreads();
    if (threadIdx.x != 0u)
        return;
    const uint64_t K = acc[0], A = acc[1];
    const unsigned long long *B = acc + 2;
    PtxMeterResult res = st.result;
    res.counted = (uint32_t)N;
    res.kept = (uint32_t)K;
    res.black = bins[256];
    res.rejected = bins[257];
    res.under = bins[258];
    res.over = bins[259];
    res.calls += 1u;
    res.valid = K ? 1u : 0u;
    if (K)
    {
        // step 6
        double frac = (double)B[0] * kMeterSubBinLog2[0] + (double)B[1] * kMeterSubBinLog2[1];
#pragma unroll
        for (int j = 2; j < 8; j++)
            frac = frac + (double)B[j] * kMeterSubBinLog2[j];
        const double avg = ((double)A + frac) / (double)K - 16.0;
        // step 7
        const double target = meterClamp(((double)a.keyLog2 - avg) + (double)a.compensation, (double)a.minLog2Exposure, (double)a.maxLog2Exposure);
        // step 8
        double cur = st.cur;
        if (!st.started)
            cur = target;
        else
        {
            const double rate = target > cur ? (double)a.speedUp : (double)a.speedDown;
            const double x = ((-(double)a.deltaSeconds) * rate) * 1.4426950408889634;
            const double blend = 1.0 - exp2_(x < -300.0 ? -300.0 : x);
            cur = blend == 1.0 ? target : cur + (target - cur) * blend;
        }
        st.cur = cur;
        st.started = 1u;
        res.avgLog2 = (float)avg;
        res.targetLog2 = (float)target;
        res.log2Exposure = (float)cur;
        res.exposure = (float)exp2_(meterClamp(cur, -300.0, 300.0));
    }
    st.result = res;
}

__global__ void __launch_bounds__(kMeterBlock) k_meter_reset(MeterState *state)
{
    const uint32_t t = threadIdx.x;
    state->bins[t] = 0u;
    if (t != 0u)
        return;
    PtxMeterResult res = {};
    res.exposure = 1.0f;
    state->result = res;
    state->cur = 0.0;
    state->started = 0u;
    state->pad = 0u;
}
