// k_compare.hip -- CDNA4 (gfx950) kernels of the bit-compare job: how two streams relate -- the mismatches at
// every offset within a radius and, at the chosen offset, the rows of the null test a - b -- of what streams decode to or of
// device-resident source PCM, in exact integers (lacx.h, compare_core.h).  Two launches, the first only where a pair has a
// radius above 0.
// k_compare_search: a workgroup of kCmpThreads lanes takes one tile: up to kCmpTileFrames frames of one span of A's axis and
// 4 * lanes consecutive offsets (cmp_tile; the span by bisection over tile_off).  It stages A's frames and the B window those
// offsets reach in LDS once, as units of four frames (cmp_stage_unit: stats_load_source behind the source table, zeros
// outside a source; a tile all of whose words would be zero ends at once) stored as 16-byte words: one plane of words for
// mono and 16-bit stereo, two for 24-bit stereo, 40 KB for the largest tile.  Behind the barrier lane tid owns the four offsets of lane tid % lanes and walks the quads of frames
// of its stripe tid / lanes (cmp_search_lane): one 16-byte LDS read of A (the same address across a stripe: a broadcast) and
// two of B (consecutive 16-byte slots across lanes) feed 16 comparisons, each an xor, one or two compares and an add into
// one of four 32-bit counters.  The stripes' parts are added through LDS, and the tile ends with at most one 64-bit
// atomicAdd per offset into the job's zeroed counts.  Integer adds do not depend on the order in which they arrive.
// k_compare_rows: one workgroup per row of 16384 frames of a pair's domain at its chosen offset (the pair by bisection over
// row_off).  A thread takes every kCmpThreads-th unit of four of A's frames and the four frames of B they are paired with
// (two units where the offset is no multiple of 4), keeps a record per channel, the records are merged pairwise through LDS
// (cmp_row_merge: counts, minima, maxima and sums) and thread 0 writes the row: one writer, no atomics, no scratch.
// Measured (scripts/compare_bench.py, profiles/compare_bench.txt): 13.8e12 sample comparisons per second at radius
// 2939, 8.3e12 at radius 588, the round trip between the two kernels included.  Only this register-blocked search loop (four
// offsets a lane, four frames a step) was built and measured; one LDS read per pair -- three times the LDS bytes per
// comparison -- was judged from the code alone.
// A translation unit of its own, like k_accuraterip.hip.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "compare_core.h"
#include "kernels.h"

namespace lacx {

namespace {

struct alignas(16) CmpQuad {
    uint32_t v[4];
};

__global__ __launch_bounds__(kCmpThreads) void k_compare_search(CmpArgs a) {
    __shared__ CmpQuad stage_a[2][kCmpStageA / 4u];
    __shared__ CmpQuad stage_b[2][kCmpStageB / 4u];
    __shared__ uint32_t part[kCmpLaneOffsets][kCmpThreads];
    const unsigned long long tile = blockIdx.x;
    uint32_t j = 0, top = a.nspans;  // (uniform) tile_off[j] <= tile < tile_off[top]
    while (top - j > 1u) {
        const uint32_t mid = j + (top - j) / 2u;
        if (a.tile_off[mid] <= tile) j = mid;
        else top = mid;
    }
    const CmpSpan sp = a.spans[j];
    const CmpPair pr = a.pairs[sp.pair];
    const CmpSource sa = a.sources[pr.a];
    const CmpSource sb = a.sources[pr.b];
    const CmpTile y = cmp_tile(sp, pr, tile - a.tile_off[j]);
    if (cmp_tile_empty(y, sa.frames, sb.frames)) return;  // (uniform)
    const uint32_t planes = cmp_planes(sa);
    auto note = [&](uint32_t item, unsigned long long key) { atomicMin(&a.bad[item], key); };

    for (uint32_t u = threadIdx.x; u < y.units_a; u += kCmpThreads) {  // u < kCmpStageA / 4: cmp_tile
        CmpQuad q0, q1;
        cmp_stage_unit(sa, y.g0 + 4ll * (long long)u, planes, q0.v, q1.v, note);
        stage_a[0][u] = q0;
        if (planes == 2u) stage_a[1][u] = q1;
    }
    for (uint32_t u = threadIdx.x; u < y.units_b; u += kCmpThreads) {  // u < kCmpStageB / 4: units_a + lanes
        CmpQuad q0, q1;
        cmp_stage_unit(sb, y.b0 + 4ll * (long long)u, planes, q0.v, q1.v, note);
        stage_b[0][u] = q0;
        if (planes == 2u) stage_b[1][u] = q1;
    }
    __syncthreads();

    uint32_t cnt[kCmpLaneOffsets] = {0u, 0u, 0u, 0u};
    if (sa.bit_depth == 16) {  // (uniform)
        cmp_search_lane<true>(stage_a[0][0].v, stage_b[0][0].v, sp, y, threadIdx.x, cnt);
    } else {
        cmp_search_lane<false>(stage_a[0][0].v, stage_b[0][0].v, sp, y, threadIdx.x, cnt);
        if (planes == 2u) cmp_search_lane<false>(stage_a[1][0].v, stage_b[1][0].v, sp, y, threadIdx.x, cnt);
    }

    // the stripes' parts: threads tid, tid + lanes, tid + 2 lanes, ... hold the same offsets
    if (sp.lanes < kCmpThreads) {  // (uniform)
#pragma unroll
        for (uint32_t k = 0; k < kCmpLaneOffsets; ++k) part[k][threadIdx.x] = cnt[k];
        __syncthreads();
        if (threadIdx.x < sp.lanes) {
#pragma unroll
            for (uint32_t k = 0; k < kCmpLaneOffsets; ++k) {
                cnt[k] = 0u;
                for (uint32_t t = threadIdx.x; t < kCmpThreads; t += sp.lanes) cnt[k] += part[k][t];
            }
        }
    }
    if (threadIdx.x < sp.lanes) {
        const long long first = (long long)pr.centre - (long long)pr.radius;
#pragma unroll
        for (uint32_t k = 0; k < kCmpLaneOffsets; ++k) {
            const long long at = y.o0 + (long long)(kCmpLaneOffsets * threadIdx.x + k) - first;  // the offset's place among the pair's counts
            if (at >= 0 && at < (long long)cmp_width(pr) && cnt[k]) atomicAdd(&a.counts[pr.count0 + (unsigned long long)at], (unsigned long long)cnt[k]);
        }
    }
}

__global__ __launch_bounds__(kCmpThreads) void k_compare_rows(CmpArgs a) {
    __shared__ lacx_compare_channel_row acc[2][kCmpThreads];
    const unsigned long long row = blockIdx.x;
    uint32_t j = 0, top = a.npairs;  // (uniform) row_off[j] <= row < row_off[top]
    while (top - j > 1u) {
        const uint32_t mid = j + (top - j) / 2u;
        if (a.row_off[mid] <= row) j = mid;
        else top = mid;
    }
    const CmpPair pr = a.pairs[j];
    const unsigned long long r = row - a.row_off[j];  // < pr.nrows
    lacx_compare_channel_row mine[2];
    cmp_row_thread(a.sources, pr, r, threadIdx.x, mine, [&](uint32_t item, unsigned long long key) { atomicMin(&a.bad[item], key); });
    acc[0][threadIdx.x] = mine[0];
    acc[1][threadIdx.x] = mine[1];
    __syncthreads();
    for (uint32_t step = kCmpThreads / 2u; step >= 1u; step >>= 1) {
        if (threadIdx.x < step) {
            cmp_row_merge(acc[0][threadIdx.x], acc[0][threadIdx.x + step]);
            cmp_row_merge(acc[1][threadIdx.x], acc[1][threadIdx.x + step]);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        lacx_compare_row out;
        out.ch[0] = acc[0][0];
        out.ch[1] = acc[1][0];
        static_cast<lacx_compare_row*>(a.rows)[pr.row0 + r] = out;  // r < nrows <= the pair's capacity (compare_plan.h)
    }
}

}  // namespace

hipError_t launch_compare_search(const CmpArgs& a, hipStream_t stream) {
    if (a.nspans && a.total_tiles) hipLaunchKernelGGL(k_compare_search, dim3((uint32_t)a.total_tiles), dim3(kCmpThreads), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_compare_rows(const CmpArgs& a, hipStream_t stream) {
    if (a.npairs && a.total_rows) hipLaunchKernelGGL(k_compare_rows, dim3((uint32_t)a.total_rows), dim3(kCmpThreads), 0, stream, a);
    return hipGetLastError();
}

}  // namespace lacx
