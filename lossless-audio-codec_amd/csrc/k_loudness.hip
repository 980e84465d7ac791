// k_loudness.hip -- CDNA4 (gfx950) kernels of the loudness job: the K-weighted energy per sub-block of what a
// stream decodes to, or of device-resident source PCM, after ITU-R BS.1770 (lacx.h).  The K-weighting is a recursive filter
// over the whole stream: a serial chain, cut into chunks of kLoudChunk frames by the linearity of the filter
// (loudness_core.h): the state behind a chunk that starts in state s is A s + f.
//   k_loud_states   one lane per chunk: both channels from zero state, the final states f[c]; validates a source
//   k_loud_carry    one wave per (item, channel): s[c + 1] = A s[c] + f[c], serially, s[c] in f[c]'s place
//   k_loud_energy   one lane per chunk: both channels again from s[c], two partial sums per channel
//   k_loud_rows     one lane per (row, channel): the partials of the sub-block added in chunk order
// Four launches on the job's stream.  Every record of the scratch is written by one lane with plain stores before a later
// launch reads it; there are no atomics on doubles and no reductions whose order the hardware chooses, and this
// translation unit is compiled with -ffp-contract=off (Makefile): a row is the bits loudness_core.h defines.
// The chain inside a chunk is serial FP64 -- eight dependent fma per frame and channel -- so the parallelism is chunks, and
// the workgroups are small (64 lanes) for occupancy on short jobs; nothing goes through LDS.  A lane walks its chunk in
// 16-byte loads per channel (stats_load_source): the lanes of a wave touch 64 different cache lines per load and come
// back to each line for its other seven quarters, so every fetched line is used whole, but through the vector L1 / L2 and
// not from one coalesced request (DESIGN §6b says what that costs).
// A translation unit of its own, like k_stats.hip: helpers shared with other kernels change their register allocation.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.h"
#include "loudness_core.h"

namespace lacx {

namespace {

constexpr uint32_t kLoudThreads = 64;

// (decode.hip) a pointer read from an item descriptor is generic to the compiler; these all point into global memory
template <typename T>
__device__ __forceinline__ T* global_ptr(T* p) {
    return (T*)(__attribute__((address_space(1))) T*)(uintptr_t)p;
}

// the item of global index x in the prefix sums off [nitems + 1] (x < off[nitems])
__device__ __forceinline__ uint32_t item_of(const unsigned long long* __restrict__ off, uint32_t nitems, unsigned long long x) {
    uint32_t lo = 0, hi = nitems;  // off[lo] <= x < off[hi]
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (off[mid] <= x) lo = mid;
        else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ LoudItem item_record(const LoudItem* __restrict__ items, uint32_t j) {
    LoudItem it = items[j];
    it.data0 = global_ptr(it.data0);
    it.data1 = global_ptr(it.data1);
    return it;
}

__global__ __launch_bounds__(kLoudThreads) void k_loud_states(LoudArgs a) {
    const unsigned long long g = (unsigned long long)blockIdx.x * kLoudThreads + threadIdx.x;
    if (g >= a.total_chunks) return;
    const uint32_t j = item_of(a.chunk_off, a.nitems, g);
    const LoudItem it = item_record(a.items, j);
    const uint32_t c = (uint32_t)(g - a.chunk_off[j]);
    unsigned long long key = kDigestClean;
    LoudState out[2];
    loud_chunk_states(a.filters[it.rate], it, c, out, key);
    LoudState* at = a.states + it.lane0 + (unsigned long long)c * it.channels;
    at[0] = out[0];
    if (it.channels == 2) at[1] = out[1];
    if (it.validate && key != kDigestClean) atomicMin(&a.bad[j], key);
}

// the value a double has in lane `from` (a constant), in every lane
__device__ __forceinline__ double lane_value(double v, uint32_t from) {
    const unsigned long long u = (unsigned long long)__double_as_longlong(v);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)u, (int)from);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(u >> 32), (int)from);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// loud_carry_lane (loudness_core.h) by one wave per (item, channel): the recurrence is serial, its memory traffic is not.
// The wave loads the f of 64 consecutive chunks in one request, every lane then takes the same 64 loud_carry_step in
// chunk order -- step i with lane i's f, read across the wave -- and lane i keeps the state in front of its step; one
// store per lane puts s[c] in f[c]'s place.  The wave waits for memory once per 64 chunks instead of once per chunk; the
// arithmetic and its order are loud_carry_lane's.  (Behind an item's last chunk the lanes hold zeros and the steps run on:
// nothing of them is stored.)
__global__ __launch_bounds__(64) void k_loud_carry(LoudArgs a) {
    const uint32_t j = blockIdx.x >> 1, ch = blockIdx.x & 1u, lane = threadIdx.x;  // (uniform) the wave's item and channel
    const LoudItem& it = a.items[j];
    if (ch >= it.channels) return;
    const LoudFilter k = a.filters[it.rate];
    const uint32_t chunks = it.chunks, channels = it.channels;
    LoudState* st = a.states + it.lane0 + ch;
    LoudState s{{0.0, 0.0, 0.0, 0.0}};
    for (uint32_t c0 = 0; c0 < chunks; c0 += 64u) {
        const bool have = chunks - c0 > lane;
        LoudState* at = st + (unsigned long long)(c0 + lane) * channels;
        LoudState f{{0.0, 0.0, 0.0, 0.0}};
        if (have) f = *at;
        LoudState mine = s;
#pragma unroll
        for (uint32_t i = 0; i < 64u; ++i) {
            if (lane == i) mine = s;
            const LoudState fi{{lane_value(f.s[0], i), lane_value(f.s[1], i), lane_value(f.s[2], i), lane_value(f.s[3], i)}};
            loud_carry_step(k, s, fi);
        }
        if (have) *at = mine;
    }
}

__global__ __launch_bounds__(kLoudThreads) void k_loud_energy(LoudArgs a) {
    const unsigned long long g = (unsigned long long)blockIdx.x * kLoudThreads + threadIdx.x;
    if (g >= a.total_chunks) return;
    const uint32_t j = item_of(a.chunk_off, a.nitems, g);
    const LoudItem it = item_record(a.items, j);
    const uint32_t c = (uint32_t)(g - a.chunk_off[j]);
    const unsigned long long at = it.lane0 + (unsigned long long)c * it.channels;
    LoudState start[2];
    start[0] = a.states[at];
    if (it.channels == 2) start[1] = a.states[at + 1];
    LoudPartial out[2];
    loud_chunk_energy(a.filters[it.rate], it, c, start, out);
    a.partials[at] = out[0];
    if (it.channels == 2) a.partials[at + 1] = out[1];
}

__global__ __launch_bounds__(kLoudThreads) void k_loud_rows(LoudArgs a) {
    const unsigned long long g = (unsigned long long)blockIdx.x * kLoudThreads + threadIdx.x;  // (row, channel)
    const unsigned long long row = g >> 1;
    const uint32_t ch = (uint32_t)(g & 1u);
    if (row >= a.total_rows) return;
    const uint32_t j = item_of(a.row_off, a.nitems, row);
    const LoudItem& it = a.items[j];
    a.rows[row].energy[ch] = ch < it.channels ? loud_row(a.partials + it.lane0, it.channels, ch, it.sub, (uint32_t)(row - a.row_off[j])) : 0.0;
}

}  // namespace

hipError_t launch_loudness(const LoudArgs& a, hipStream_t stream) {
    if (!a.nitems) return hipSuccess;
    const auto grid = [](unsigned long long lanes) { return dim3((uint32_t)((lanes + kLoudThreads - 1u) / kLoudThreads)); };
    if (a.total_chunks) {
        hipLaunchKernelGGL(k_loud_states, grid(a.total_chunks), dim3(kLoudThreads), 0, stream, a);
        hipLaunchKernelGGL(k_loud_carry, dim3(2u * a.nitems), dim3(64), 0, stream, a);
        hipLaunchKernelGGL(k_loud_energy, grid(a.total_chunks), dim3(kLoudThreads), 0, stream, a);
    }
    if (a.total_rows) hipLaunchKernelGGL(k_loud_rows, grid(2ull * a.total_rows), dim3(kLoudThreads), 0, stream, a);
    return hipGetLastError();
}

}  // namespace lacx
