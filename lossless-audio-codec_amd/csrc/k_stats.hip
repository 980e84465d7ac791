// k_stats.hip -- CDNA4 (gfx950) kernel of the audio statistics: per BLOCK of what a stream decodes to, or per
// block_frames frames of device-resident source PCM, and per channel min, max, OR of the bits, full-scale and zero counts,
// sum and sum of squares; per block the leading / trailing all-zero frames and the frames whose channels differ.  A thread
// takes one unit of four frames and yields one partial record, or two where the unit straddles a block border
// (stats_core.h); the records of a block are combined into its device row.
// The device rows (StatsAcc, 96 bytes per global block; the layout is internal): every field is encoded so that its
// identity is all-zero bytes -- min and max as biased maxima, the lead / trail fields as distances that grow, the rest ORs
// and sums (stats_core.h) -- so the rows are zeroed like the block digests' raw words and no kernel initialises them.
// Every operation is an integer max / or / add: the result does not depend on the order in which the atomics arrive and
// is the same from run to run.
// A translation unit of its own, like k_blockdigest.hip: helpers shared with other kernels change their register allocation.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.h"
#include "stats_core.h"

namespace lacx {

namespace {

// (decode.hip) a pointer read from an item descriptor is generic to the compiler; these all point into global memory
template <typename T>
__device__ __forceinline__ T* global_ptr(T* p) {
    return (T*)(__attribute__((address_space(1))) T*)(uintptr_t)p;
}

__device__ __forceinline__ uint32_t shfl32(uint32_t v, int m) { return (uint32_t)__shfl_xor((int)v, m); }
__device__ __forceinline__ unsigned long long shfl64(unsigned long long v, int m) {
    return ((unsigned long long)shfl32((uint32_t)(v >> 32), m) << 32) | shfl32((uint32_t)v, m);
}
// the record of lane (this ^ m)
__device__ __forceinline__ StatsChan shfl_chan(const StatsChan& c, int m) {
    StatsChan o;
    o.min_enc = shfl32(c.min_enc, m), o.max_enc = shfl32(c.max_enc, m), o.or_bits = shfl32(c.or_bits, m);
    o.full_scale = shfl32(c.full_scale, m), o.zeros = shfl32(c.zeros, m), o.pad = 0;
    o.sum = shfl64(c.sum, m), o.sum_sq = shfl64(c.sum_sq, m);
    return o;
}

// a record into a block's row: only what differs from the identity costs an atomic
__device__ __forceinline__ void flush_chan(StatsChan* row, const StatsChan& c) {
    if (c.min_enc) atomicMax(&row->min_enc, c.min_enc);
    if (c.max_enc) atomicMax(&row->max_enc, c.max_enc);
    if (c.or_bits) atomicOr(&row->or_bits, c.or_bits);
    if (c.full_scale) atomicAdd(&row->full_scale, c.full_scale);
    if (c.zeros) atomicAdd(&row->zeros, c.zeros);
    if (c.sum) atomicAdd(&row->sum, c.sum);
    if (c.sum_sq) atomicAdd(&row->sum_sq, c.sum_sq);
}
__device__ __forceinline__ void flush(StatsAcc* row, const StatsAcc& a, bool stereo) {
    if (a.first_nz) atomicMax(&row->first_nz, a.first_nz);
    if (a.last_nz) atomicMax(&row->last_nz, a.last_nz);
    if (a.differing) atomicAdd(&row->differing, a.differing);
    flush_chan(&row->ch[0], a.ch[0]);
    if (stereo) flush_chan(&row->ch[1], a.ch[1]);
}

// Laid out as k_digest_blocks: thread u handles unit u of the concatenated unit ranges of all items; the item is found by
// one uniform binary search per workgroup and again per thread only in a workgroup that spans items.  rows: one StatsAcc
// per global block, zero on entry.  kSource: DigestSource records on a grid of `grid` frames, item j's blocks from
// block_off[j] on; else DecodeItem records whose samples k_ms_inverse left in place, item j's blocks from its block0 on,
// of which only those with index < present[j] and status 0 count.
//
// Fast path: a wave whose 64 units are full, lie in one block of one item and hold no straddler.  Six xor-shuffle levels
// leave the wave's record in every lane; lane 0 of every such wave leaves record and block in LDS, and thread 0 combines
// the records of consecutive waves of one block: a workgroup that lies wholly inside one block issues one set of global
// atomics, so a 16 384-frame block costs 16 sets.
// General path (block borders, partial last units, item borders, lost blocks): every lane issues its own atomics for its
// one record, or two.
template <bool kSource>
__global__ __launch_bounds__(kDigestThreads) void k_stats_blocks(uint32_t nitems, unsigned long long total_units,
                                                                 const unsigned long long* __restrict__ unit_off,
                                                                 const DecodeItem* __restrict__ items,
                                                                 const uint32_t* __restrict__ present,
                                                                 const DigestSource* __restrict__ src,
                                                                 const unsigned long long* __restrict__ block_off, uint32_t grid,
                                                                 StatsAcc* __restrict__ rows, unsigned long long* __restrict__ bad,
                                                                 const unsigned long long* __restrict__ frame_off,
                                                                 const uint32_t* __restrict__ status) {
    __shared__ StatsAcc wave_acc[kDigestThreads / 64u];
    __shared__ uint32_t wave_blk[kDigestThreads / 64u], wave_stereo[kDigestThreads / 64u];
    const unsigned long long first = (unsigned long long)blockIdx.x * kDigestThreads;
    uint32_t lo = 0, hi = nitems;  // unit_off[lo] <= first < unit_off[hi]
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (unit_off[mid] <= first) lo = mid;
        else hi = mid;
    }
    const unsigned long long u = first + threadIdx.x;
    const bool one_item = unit_off[lo + 1] >= first + kDigestThreads;  // (uniform) the whole workgroup lies in item lo
    const bool valid = u < total_units;
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t j = lo, g0 = 0;  // g0: the global block of the unit's first frame
    bool stereo = false;
    StatsUnit su{};
    if (valid) {
        if (!one_item) {  // this thread's item, among the later ones
            uint32_t h2 = nitems;  // unit_off[j] <= u < unit_off[h2]
            while (h2 - j > 1u) {
                const uint32_t mid = j + (h2 - j) / 2u;
                if (unit_off[mid] <= u) j = mid;
                else h2 = mid;
            }
        }
        const unsigned long long f0 = (unsigned long long)kDigestUnitFrames * (u - unit_off[j]);
        if constexpr (kSource) {
            const DigestSource& s = src[j];
            unsigned long long key = kDigestClean;
            stereo = s.channels == 2;
            su = stats_unit_source(f0, grid, s.channels, s.bit_depth, s.frames, global_ptr(s.data0), global_ptr(s.data1), s.layout, key);
            if (key != kDigestClean) atomicMin(&bad[j], key);
            g0 = (uint32_t)block_off[j] + su.b0;
        } else {
            const DecodeItem& it = items[j];
            stereo = it.channels == 2;
            su = stats_unit_decoded(f0, it.blocks, present[j], it.channels, it.bit_depth, it.frames, frame_off + it.block0, it.frame0,
                                    global_ptr(it.left), global_ptr(it.right), status + it.block0);
            g0 = it.block0 + su.b0;
        }
    }
    const bool full = valid && su.n0 == kDigestUnitFrames;  // (then the unit has no second piece)
    const bool fast = __ballot(full && g0 == (uint32_t)__builtin_amdgcn_readfirstlane((int)g0)) == ~0ull;  // (uniform per wave)
    if (fast) {
        if (su.use0) {  // (uniform: one block, hence one item and one channel count)
#pragma unroll
            for (int level = 0; level < 6; ++level) {
                const int m = 1 << level;
                su.p0.first_nz = stats_umax(su.p0.first_nz, shfl32(su.p0.first_nz, m));
                su.p0.last_nz = stats_umax(su.p0.last_nz, shfl32(su.p0.last_nz, m));
                su.p0.differing += shfl32(su.p0.differing, m);
                stats_chan_merge(su.p0.ch[0], shfl_chan(su.p0.ch[0], m));
                if (stereo) stats_chan_merge(su.p0.ch[1], shfl_chan(su.p0.ch[1], m));
            }
        }
    } else if (valid) {
        if (su.use0 && su.n0) flush(&rows[g0], su.p0, stereo);
        if (su.use1 && su.n1) flush(&rows[g0 + 1u], su.p1, stereo);
    }
    if (lane == 0u) {
        const bool has = fast && su.use0;
        wave_blk[threadIdx.x >> 6] = has ? g0 : ~0u;
        wave_stereo[threadIdx.x >> 6] = stereo ? 1u : 0u;
        if (has) wave_acc[threadIdx.x >> 6] = su.p0;
    }
    __syncthreads();
    if (threadIdx.x == 0u) {  // consecutive waves of one block: one set of atomics
        StatsAcc acc{};
        uint32_t blk = ~0u;
        bool st = false;
        for (uint32_t w = 0; w < kDigestThreads / 64u; ++w) {
            if (wave_blk[w] != blk) {
                if (blk != ~0u) flush(&rows[blk], acc, st);
                acc = StatsAcc{};
                blk = wave_blk[w];
                st = wave_stereo[w] != 0u;
            }
            if (blk != ~0u) stats_merge(acc, wave_acc[w], st);
        }
        if (blk != ~0u) flush(&rows[blk], acc, st);
    }
}

}  // namespace

hipError_t launch_stats_blocks(const StatsArgs& s, hipStream_t stream) {
    const DecodeArgs& a = s.dec;
    if (a.total_units)
        hipLaunchKernelGGL(k_stats_blocks<false>, dim3((uint32_t)((a.total_units + kDigestThreads - 1u) / kDigestThreads)),
                           dim3(kDigestThreads), 0, stream, a.nitems, a.total_units, a.unit_off, a.items, a.present, nullptr, nullptr, 0u,
                           s.rows, nullptr, a.frame_off, a.status);
    return hipGetLastError();
}

hipError_t launch_stats_pcm_blocks(const StatsPcmArgs& a, hipStream_t stream) {
    if (a.pcm.total_units)
        hipLaunchKernelGGL(k_stats_blocks<true>, dim3((uint32_t)((a.pcm.total_units + kDigestThreads - 1u) / kDigestThreads)),
                           dim3(kDigestThreads), 0, stream, a.pcm.nitems, a.pcm.total_units, a.pcm.unit_off, nullptr, nullptr, a.pcm.src,
                           a.block_off, a.grid, a.rows, a.pcm.bad, nullptr, nullptr);
    return hipGetLastError();
}

}  // namespace lacx
