// k_blockdigest.hip -- CDNA4 (gfx950) kernels of the block digests: one CRC-32 per BLOCK of what a stream
// decodes to, or per block_frames frames of device-resident source PCM, and the judge that compares a stream's with the
// values a manifest expects.  The arithmetic is k_digest.hip's (crc32_core.h): a thread digests the bytes of one unit of
// four frames, and every unit's value is moved to the end of its block and added into the block's result word; the init
// term and the final xor depend on the block's byte count alone.  A unit that straddles a block border contributes a piece
// to each of the two blocks (blockdigest_core.h).
// A translation unit of its own, like k_digest.hip: helpers shared with other kernels change their register allocation.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "blockdigest_core.h"
#include "kernels.h"

namespace lacx {

namespace {

// (decode.hip) a pointer read from an item descriptor is generic to the compiler; these all point into global memory
template <typename T>
__device__ __forceinline__ T* global_ptr(T* p) {
    return (T*)(__attribute__((address_space(1))) T*)(uintptr_t)p;
}

// Laid out as k_digest: thread u handles unit u of the concatenated unit ranges of all items; the item is found by one
// uniform binary search per workgroup and again per thread only in a workgroup that spans items.  raw: one word per
// global block, zero on entry.  kSource: DigestSource records on a grid of `grid` frames, item j's blocks from
// block_off[j] on; else DecodeItem records whose samples k_ms_inverse left in place, item j's blocks from its block0 on,
// of which only those with index < present[j] and status 0 count.
//
// Fast path: a wave whose 64 units are full, lie in one block of one item and hold no straddler.  The six-level lane tree
// of k_digest combines them, and the distance from the wave's end to the BLOCK's end is uniform: its factor comes from
// the five-level tree over 32 lanes.  Lane 0 of every such wave leaves value and block in LDS, and thread 0 adds up the
// values of consecutive waves of one block: a workgroup that lies wholly inside one block issues one atomicXor, so a
// 16 384-frame block costs 16.
// General path: every lane shifts its own piece, or two, and issues its own atomics.
// XOR commutes: the result does not depend on the order in which the atomics arrive.
template <bool kSource>
__global__ __launch_bounds__(kDigestThreads) void k_digest_blocks(uint32_t nitems, unsigned long long total_units,
                                                                  const unsigned long long* __restrict__ unit_off,
                                                                  const DecodeItem* __restrict__ items,
                                                                  const uint32_t* __restrict__ present,
                                                                  const DigestSource* __restrict__ src,
                                                                  const unsigned long long* __restrict__ block_off, uint32_t grid,
                                                                  uint32_t* __restrict__ raw, unsigned long long* __restrict__ bad,
                                                                  const unsigned long long* __restrict__ frame_off,
                                                                  const uint32_t* __restrict__ status) {
    __shared__ uint32_t wave_sum[kDigestThreads / 64u], wave_blk[kDigestThreads / 64u];
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
    uint32_t j = lo, align = 0, fmt = 0, g0 = 0;  // g0: the global block of the unit's first frame
    BlockUnit bu{};
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
            align = (uint32_t)s.channels * (s.bit_depth / 8u);
            fmt = crc_format(s.channels, s.bit_depth);
            bu = block_unit_source(f0, grid, s.channels, s.bit_depth, s.frames, global_ptr(s.data0), global_ptr(s.data1), s.layout, key);
            if (key != kDigestClean) atomicMin(&bad[j], key);
            g0 = (uint32_t)block_off[j] + bu.b0;
        } else {
            const DecodeItem& it = items[j];
            align = (uint32_t)it.channels * (it.bit_depth / 8u);
            fmt = crc_format(it.channels, it.bit_depth);
            bu = block_unit_decoded(f0, it.blocks, present[j], it.channels, it.bit_depth, it.frames, frame_off + it.block0, it.frame0,
                                    global_ptr(it.left), global_ptr(it.right), status + it.block0);
            g0 = it.block0 + bu.b0;
        }
    }
    const bool full = valid && bu.p0.bytes == kDigestUnitFrames * align;  // (then the unit has no second piece)
    const bool fast = __ballot(full && g0 == (uint32_t)__builtin_amdgcn_readfirstlane((int)g0)) == ~0ull;  // (uniform per wave)
    uint32_t wave_value = 0;
    if (fast) {
        if (bu.use0) {  // (uniform: one block)
            const uint32_t* tree = kCrcTables.tree[__builtin_amdgcn_readfirstlane((int)fmt)];
            uint32_t v = bu.p0.raw;
#pragma unroll
            for (uint32_t level = 0; level < 6u; ++level) {
                const uint32_t other = (uint32_t)__shfl_xor((int)v, 1 << level);
                const bool upper = ((lane >> level) & 1u) != 0u;  // the partner's units come first in the message
                v = crc_mul(upper ? other : v, tree[level]) ^ (upper ? v : other);
            }
            // bytes from the end of the wave's last unit to the block's end: the same in every lane
            const unsigned long long dist = bu.dist0 - (unsigned long long)(kDigestUnitFrames * align) * (63u - lane);
            const uint32_t d = crc_reduce(dist);
            uint32_t factor = ((d >> (lane & 31u)) & 1u) != 0u ? kCrcTables.pow8[lane & 31u] : kCrcOne;
#pragma unroll
            for (uint32_t level = 0; level < 5u; ++level) factor = crc_mul(factor, (uint32_t)__shfl_xor((int)factor, 1 << level));
            wave_value = crc_mul(v, factor);
        }
    } else if (valid) {
        if (bu.use0 && bu.p0.bytes) atomicXor(&raw[g0], crc_shift(bu.p0.raw, bu.dist0));
        if (bu.use1 && bu.p1.bytes) atomicXor(&raw[g0 + 1u], crc_shift(bu.p1.raw, bu.dist1));
    }
    if (lane == 0u) {
        const bool has = fast && bu.use0;
        wave_sum[threadIdx.x >> 6] = has ? wave_value : 0u;
        wave_blk[threadIdx.x >> 6] = has ? g0 : ~0u;
    }
    __syncthreads();
    if (threadIdx.x == 0u) {  // consecutive waves of one block: one atomic
        uint32_t acc = 0, blk = ~0u;
#pragma unroll
        for (uint32_t w = 0; w < kDigestThreads / 64u; ++w) {
            if (wave_blk[w] != blk) {
                if (blk != ~0u && acc) atomicXor(&raw[blk], acc);
                acc = 0;
                blk = wave_blk[w];
            }
            acc ^= wave_sum[w];
        }
        if (blk != ~0u && acc) atomicXor(&raw[blk], acc);
    }
}

// One thread per global block of a judged job (judge_block): behind k_digest_blocks on the same stream, in front of the
// salvage pass, which reads nothing but final status words.
__global__ __launch_bounds__(256) void k_digest_judge(uint32_t total_blocks, const uint32_t* __restrict__ blk_item,
                                                      const DecodeItem* __restrict__ items, const uint32_t* __restrict__ present,
                                                      const uint32_t* __restrict__ judged,
                                                      const unsigned long long* __restrict__ frame_off,
                                                      const uint32_t* __restrict__ raw, const uint32_t* __restrict__ expect,
                                                      uint32_t* __restrict__ status) {
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    if (g >= total_blocks) return;
    const uint32_t j = blk_item[g];
    const DecodeItem& it = items[j];
    judge_block(g, g - it.block0, present[j], judged[j] != 0u, (uint32_t)(frame_off[g + 1] - frame_off[g]),
                (uint32_t)it.channels * (it.bit_depth / 8u), raw, expect, status);
}

}  // namespace

hipError_t launch_digest_blocks(const DecodeArgs& a, hipStream_t stream) {
    if (a.total_units)
        hipLaunchKernelGGL(k_digest_blocks<false>, dim3((uint32_t)((a.total_units + kDigestThreads - 1u) / kDigestThreads)),
                           dim3(kDigestThreads), 0, stream, a.nitems, a.total_units, a.unit_off, a.items, a.present, nullptr, nullptr, 0u,
                           a.block_raw, nullptr, a.frame_off, a.status);
    if (a.block_expect && a.total_blocks)
        hipLaunchKernelGGL(k_digest_judge, dim3((a.total_blocks + 255u) / 256u), dim3(256), 0, stream, a.total_blocks, a.blk_item, a.items,
                           a.present, a.judged, a.frame_off, a.block_raw, a.block_expect, a.status);
    return hipGetLastError();
}

hipError_t launch_digest_pcm_blocks(const BlockPcmArgs& a, hipStream_t stream) {
    if (a.pcm.total_units)
        hipLaunchKernelGGL(k_digest_blocks<true>, dim3((uint32_t)((a.pcm.total_units + kDigestThreads - 1u) / kDigestThreads)),
                           dim3(kDigestThreads), 0, stream, a.pcm.nitems, a.pcm.total_units, a.pcm.unit_off, nullptr, nullptr, a.pcm.src,
                           a.block_off, a.grid, a.raw, a.pcm.bad, nullptr, nullptr);
    return hipGetLastError();
}

}  // namespace lacx
