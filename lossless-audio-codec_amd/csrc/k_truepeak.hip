// k_truepeak.hip -- CDNA4 (gfx950) kernel of the true-peak job: the maximum of the 4x oversampled signal of
// ITU-R BS.1770-4 Annex 2 per segment of 16384 frames of what a stream decodes to, or of device-resident source PCM, in
// exact integers (lacx.h, truepeak_core.h).  One launch.
// A workgroup of kTpThreads lanes takes one tile of kTpTileFrames outputs-frames n of one item, tile-aligned to the item's
// frame 0; a lane loads its unit of four frames (stats_load_source), the tile's first three lanes also the three units in
// front of the tile, and the tile is staged per channel in LDS: 12 + 1024 words, 8288 bytes for both channels (the code
// object asks for 14.5 KB: the compiler keeps thread-private arrays of the loads there too).  Behind the
// barrier a lane reads the 16 words x[n0 - 12 .. n0 + 3] per channel as four 16-byte reads -- lane t at byte 16 t + 16 q:
// the lanes of every 16-lane group of such a read cover sixteen consecutive 16-byte slots, one bank row, so the reads are
// free of bank conflicts, and so are the 16-byte stores of the staging -- and evaluates 4 frames x 4 phases x 12 taps per
// channel out of registers (tp_channel: 16-bit dot products, v_dot2c_i32_i16, six per output at depth 16, twelve at depth
// 24, chosen per item).
// The lane's keys and sample peaks are combined across the wave by shuffles, across the four waves through LDS, and lane 0
// issues at most one integer atomicMax per (row, channel) and quantity into the job's zeroed rows: 64-bit for the packed
// key, 32-bit for the sample peak.  A tile's outputs all belong to one row (tp_tile_row).  Integer maxima do not depend on
// the order in which they arrive: a row is the same bits in any batch.
// Measured (scripts/truepeak_bench.py, profiles/truepeak_bench.txt): 4.03 ms for 4.06 GB of 16-bit PCM, 1.34 ms for 1.02
// GB of 24-bit PCM: 1.0 and 0.76 TB/s, a quarter of what the memory delivers.  The multiply-adds are not what bounds it:
// with one 24-bit multiply and half a three-input add per tap instead of half a dot product -- about three times the arithmetic --
// the same kernel took 4.51 and 1.58 ms.  What does has not been measured.
// A translation unit of its own, like k_stats.hip: helpers shared with other kernels change their register allocation.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.h"
#include "truepeak_core.h"

namespace lacx {

namespace {

// (decode.hip) a pointer read from an item descriptor is generic to the compiler; these all point into global memory
template <typename T>
__device__ __forceinline__ T* global_ptr(T* p) {
    return (T*)(__attribute__((address_space(1))) T*)(uintptr_t)p;
}

struct alignas(16) Quad {
    int32_t v[4];
};

__global__ __launch_bounds__(kTpThreads) void k_truepeak(TpArgs a) {
    constexpr uint32_t kStage = kTpHistory + kTpTileFrames;  // words per channel; a multiple of 4
    __shared__ Quad stage[2][kStage / 4u];
    __shared__ TpLane wave_part[kTpThreads / 64u];
    const unsigned long long tile = blockIdx.x;
    uint32_t j = 0, hi = a.nitems;  // (uniform) tile_off[j] <= tile < tile_off[hi]
    while (hi - j > 1u) {
        const uint32_t mid = j + (hi - j) / 2u;
        if (a.tile_off[mid] <= tile) j = mid;
        else hi = mid;
    }
    TpItem it = a.items[j];
    it.data0 = global_ptr(it.data0);
    it.data1 = global_ptr(it.data1);
    const unsigned long long t = tile - a.tile_off[j];
    const unsigned long long tile_start = t * kTpTileFrames, n0 = tile_start + 4u * threadIdx.x;
    const bool stereo = it.channels == 2, deep = it.bit_depth == 24;

    // the lane's unit, and (lanes 0 .. 2) the units in front of the tile: zeros in front of frame 0 and behind the last frame
    unsigned long long key = kDigestClean, other = kDigestClean;
    Quad l, r;
    tp_load_unit(it, n0, key, l.v, r.v);
    stage[0][kTpHistory / 4u + threadIdx.x] = l;
    if (stereo) stage[1][kTpHistory / 4u + threadIdx.x] = r;
    if (threadIdx.x < kTpHistory / 4u) {
        Quad hl{{0, 0, 0, 0}}, hr{{0, 0, 0, 0}};
        if (t != 0u) tp_load_unit(it, tile_start - kTpHistory + 4u * threadIdx.x, other, hl.v, hr.v);
        stage[0][threadIdx.x] = hl;
        if (stereo) stage[1][threadIdx.x] = hr;
    }
    if (it.validate && key != kDigestClean) atomicMin(&a.bad[j], key);
    __syncthreads();

    // x[n0 - 12 .. n0 + 3] per channel, then the lane's 16 outputs per channel
    alignas(16) int32_t wl[16], wr[16] = {};
#pragma unroll
    for (uint32_t q = 0; q < 4u; ++q) {
        __builtin_memcpy(wl + 4u * q, &stage[0][threadIdx.x + q], 16);
        if (stereo) __builtin_memcpy(wr + 4u * q, &stage[1][threadIdx.x + q], 16);
    }
    const uint32_t row = tp_tile_row(tile_start, it.frames);
    const uint32_t pos0 = 4u * (uint32_t)(n0 - (unsigned long long)row * kTpRowFrames);
    TpLane mine = tp_lane(wl, wr, l.v, r.v, stereo, deep, pos0);

    // across the wave, across the waves, into the row
#pragma unroll
    for (uint32_t step = 32u; step; step >>= 1) {
        TpLane up;
        up.key[0] = __shfl_xor(mine.key[0], (int)step);
        up.key[1] = __shfl_xor(mine.key[1], (int)step);
        up.sample_peak[0] = (uint32_t)__shfl_xor((int)mine.sample_peak[0], (int)step);
        up.sample_peak[1] = (uint32_t)__shfl_xor((int)mine.sample_peak[1], (int)step);
        tp_merge(mine, up);
    }
    if ((threadIdx.x & 63u) == 0u) wave_part[threadIdx.x >> 6] = mine;
    __syncthreads();
    if (threadIdx.x == 0u) {
#pragma unroll
        for (uint32_t w = 1; w < kTpThreads / 64u; ++w) tp_merge(mine, wave_part[w]);
        TpAcc* at = a.rows + it.row0 + row;
        for (uint32_t c = 0; c < it.channels; ++c) {
            if (mine.key[c]) atomicMax(&at->key[c], mine.key[c]);
            if (mine.sample_peak[c]) atomicMax(&at->sample_peak[c], mine.sample_peak[c]);
        }
    }
}

}  // namespace

hipError_t launch_truepeak(const TpArgs& a, hipStream_t stream) {
    if (a.nitems && a.total_tiles) hipLaunchKernelGGL(k_truepeak, dim3((uint32_t)a.total_tiles), dim3(kTpThreads), 0, stream, a);
    return hipGetLastError();
}

}  // namespace lacx
