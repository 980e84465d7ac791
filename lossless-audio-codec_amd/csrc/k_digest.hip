// k_digest.hip -- CDNA4 (gfx950) kernel of the decoder's digest form: the CRC-32 of what a stream decodes to,
// or of device-resident source PCM, made where the samples lie.  CRC-32 is linear over GF(2): the raw value of a message
// is the XOR of its pieces' raw values, each multiplied by x^(8 * bytes behind the piece) mod P (crc32_core.h).  A thread
// digests the bytes of one unit of four frames (digest_core.h); what is left is to move every unit's value to the end
// of its item and to add the values up, in any order, in the item's result word.  The init term and the final xor depend
// on the item's length alone and are the host's.
// Kept apart from decode.hip: helpers shared with its kernels change k_wav_pack's register allocation.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "digest_core.h"
#include "kernels.h"

namespace lacx {

namespace {

// (decode.hip) a pointer read from an item descriptor is generic to the compiler; these all point into global memory
template <typename T>
__device__ __forceinline__ T* global_ptr(T* p) {
    return (T*)(__attribute__((address_space(1))) T*)(uintptr_t)p;
}

// Laid out as k_verify: thread u handles unit u of the concatenated unit ranges of all items (unit_off: [nitems + 1]
// prefix sums of ceil(frames / 4)); the item is found by one uniform binary search per workgroup, on its first unit, and
// again per thread only in a workgroup that spans items.  kSource: the items are DigestSource records (device-resident
// PCM in its own layout, validated on the way: the lowest invalid sample's key per item by atomicMin), else DecodeItem
// records whose samples lie in the decoder's scratch.
//
// Fast path: a wave whose 64 units are all full units of one item.  A tree over the lanes combines them: at level k
// the value of 2^k units is multiplied by x^(8 * unit_bytes * 2^k) -- a constant of the sample format -- and the value of
// the 2^k units behind it is added; after six levels every lane holds the wave's value.  The distance from the wave's
// end to the item's end is uniform: its factor x^(8 * distance) is the product of the table entries of its set bits, made
// by a second tree over 32 lanes (five multiplies) instead of up to 32 in one lane.  In a workgroup that lies in one
// item the waves' shifted values -- all relative to the same end -- are added up in LDS and one lane issues one atomicXor;
// elsewhere one lane per wave does.
// General path: a wave that holds an item's partial last unit, or units of several items, or the end of the job.  Every
// lane shifts its own value by its own distance and issues its own atomicXor.
// XOR commutes: the result does not depend on the order in which the atomics arrive.
template <bool kSource>
__global__ __launch_bounds__(kDigestThreads) void k_digest(uint32_t nitems, unsigned long long total_units,
                                                           const unsigned long long* __restrict__ unit_off,
                                                           const DecodeItem* __restrict__ items,
                                                           const DigestSource* __restrict__ src, DigestWords* __restrict__ res,
                                                           unsigned long long* __restrict__ bad,
                                                           const unsigned long long* __restrict__ frame_off,
                                                           const uint8_t* __restrict__ ms_flag, uint32_t* __restrict__ status) {
    __shared__ uint32_t wave_sum[kDigestThreads / 64u];
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
    uint32_t j = lo, align = 0, fmt = 0;
    unsigned long long f0 = 0, frames = 0;
    DigestPiece piece{0u, 0u};
    if (valid) {
        if (!one_item) {  // this thread's item, among the later ones
            uint32_t h2 = nitems;  // unit_off[j] <= u < unit_off[h2]
            while (h2 - j > 1u) {
                const uint32_t mid = j + (h2 - j) / 2u;
                if (unit_off[mid] <= u) j = mid;
                else h2 = mid;
            }
        }
        f0 = (unsigned long long)kDigestUnitFrames * (u - unit_off[j]);
        if constexpr (kSource) {
            const DigestSource& s = src[j];
            unsigned long long key = kDigestClean;
            frames = s.frames;
            align = (uint32_t)s.channels * (s.bit_depth / 8u);
            fmt = crc_format(s.channels, s.bit_depth);
            piece = digest_unit_source(f0, s.channels, s.bit_depth, frames, global_ptr(s.data0), global_ptr(s.data1), s.layout, key);
            if (key != kDigestClean) atomicMin(&bad[j], key);
        } else {
            const DecodeItem& it = items[j];
            frames = it.frames;
            align = (uint32_t)it.channels * (it.bit_depth / 8u);
            fmt = crc_format(it.channels, it.bit_depth);
            piece = digest_unit_decoded(f0, it.blocks, it.channels, it.bit_depth, frames, frame_off + it.block0, it.frame0,
                                        global_ptr(it.left), global_ptr(it.right), ms_flag + it.block0, status + it.block0);
        }
    }
    const bool full = valid && piece.bytes == kDigestUnitFrames * align;
    const bool fast = __ballot(full && j == (uint32_t)__builtin_amdgcn_readfirstlane((int)j)) == ~0ull;  // (uniform per wave)
    uint32_t wave_value = 0;
    if (fast) {
        const uint32_t* tree = kCrcTables.tree[__builtin_amdgcn_readfirstlane((int)fmt)];
        uint32_t v = piece.raw;
#pragma unroll
        for (uint32_t level = 0; level < 6u; ++level) {
            const uint32_t other = (uint32_t)__shfl_xor((int)v, 1 << level);
            const bool upper = ((lane >> level) & 1u) != 0u;  // the partner's units come first in the message
            v = crc_mul(upper ? other : v, tree[level]) ^ (upper ? v : other);
        }
        // bytes from the end of the wave's last unit to the item's end: the same in every lane
        const unsigned long long dist = (frames - (f0 + kDigestUnitFrames * (64u - lane))) * align;
        const uint32_t d = crc_reduce(dist);
        uint32_t factor = ((d >> (lane & 31u)) & 1u) != 0u ? kCrcTables.pow8[lane & 31u] : kCrcOne;
#pragma unroll
        for (uint32_t level = 0; level < 5u; ++level) factor = crc_mul(factor, (uint32_t)__shfl_xor((int)factor, 1 << level));
        wave_value = crc_mul(v, factor);
        if (!one_item && lane == 0u) atomicXor(&res[j].raw, wave_value);
    } else if (valid) {
        atomicXor(&res[j].raw, crc_shift(piece.raw, (frames - f0) * align - piece.bytes));
    }
    if (one_item) {  // (uniform) every wave's fast-path value ends at item lo's end
        if (lane == 0u) wave_sum[threadIdx.x >> 6] = fast ? wave_value : 0u;
        __syncthreads();
        if (threadIdx.x == 0u) {
            uint32_t x = 0;
#pragma unroll
            for (uint32_t w = 0; w < kDigestThreads / 64u; ++w) x ^= wave_sum[w];
            if (x) atomicXor(&res[lo].raw, x);
        }
    }
}

}  // namespace

hipError_t launch_digest(const DecodeArgs& a, hipStream_t stream) {
    if (a.total_units)
        hipLaunchKernelGGL(k_digest<false>, dim3((uint32_t)((a.total_units + kDigestThreads - 1u) / kDigestThreads)), dim3(kDigestThreads),
                           0, stream, a.nitems, a.total_units, a.unit_off, a.items, nullptr, a.digest, nullptr, a.frame_off, a.ms_flag,
                           a.status);
    return hipGetLastError();
}

hipError_t launch_digest_pcm(const DigestPcmArgs& a, hipStream_t stream) {
    if (a.total_units)
        hipLaunchKernelGGL(k_digest<true>, dim3((uint32_t)((a.total_units + kDigestThreads - 1u) / kDigestThreads)), dim3(kDigestThreads),
                           0, stream, a.nitems, a.total_units, a.unit_off, nullptr, a.src, a.res, a.bad, nullptr, nullptr, nullptr);
    return hipGetLastError();
}

}  // namespace lacx
