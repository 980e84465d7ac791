// k_accuraterip.hip -- CDNA4 (gfx950) kernel of the rip-checksum job: the AccurateRip v1 / v2 track checksums
// and the 450th-sector sum of a disc of 16-bit stereo audio at every read offset within a radius, of what a disc's streams
// decode to or of device-resident source PCM, in exact integers (lacx.h, accuraterip_core.h).  One launch.
// A workgroup of kArThreads lanes takes one tile: up to kArTileMults multipliers of one span and `lanes` consecutive
// offsets (ar_tile; the span by bisection over tile_off).  It stages the count + lanes - 1 words the tile reads in LDS
// once, as units of four disc frames (ar_load_unit: stats_load_source behind the disc's source table, zeros outside the
// disc) stored as 16-byte words: 17.4 KB for the largest tile.  Behind the barrier lane tid owns offset tid % lanes and
// walks the multipliers of its stripe tid / lanes (ar_lane): at every step the lanes of a wave read consecutive LDS words
// (or, below 64 offsets, a few runs of consecutive words that overlap, which are broadcasts), so the reads are free of
// bank conflicts.  Each lane carries two 32-bit accumulators, the sums of the products' low and high halves.
// Where the workgroup holds several stripes (lanes < kArThreads) their parts are added by shuffles inside a wave and through
// LDS across waves, and the tile ends with at most one 32-bit atomicAdd per offset and kind (v1 / s450: the low halves; v2:
// low + high) into the job's zeroed sums.  Wrapping integer adds do not depend on the order in which they arrive: a sum is
// the same bits in any batch.
// At radius 0 a tile is 4096 frames read once and 16 multiplies per lane: one pass over the PCM.  At radius 2939 a tile is
// 4351 frames staged for 4096 x 256 multiplies: the staging is 0.4 % of the LDS reads.
// The pair: ar_add's (uint64)m * x is one v_mad_u64_u32 (4.8 cycles per wave and SIMD against 4.7 + 4.5 for v_mul_lo_u32 +
// v_mul_hi_u32, profiles/r02_opprobe_instruction_costs.txt; partial products of x's 16-bit fields need three multiplies
// since m has up to 28 bits), and the two halves go into the accumulators.  Where every lane owns an offset (radius >= 128)
// the multiplier and the trip count are wave-uniform: ar_lane takes eight pairs per turn, and the compiler makes 16 pairs of
// two turns -- 8 ds_read2_b32 at constant distances, 16 v_mad_u64_u32 with the multiplier in a scalar register, 16
// v_add3_u32 (two products' halves per add).  Measured (scripts/accuraterip_bench.py, profiles/accuraterip_bench.txt): see
// DESIGN 6b; the same loop one pair per turn (a read, its wait, three adds and a compare around every multiply) took 455 ms
// for the 2.99e12 pairs of the 48-song batch at radius 2939.
// A translation unit of its own, like k_truepeak.hip: helpers shared with other kernels change their register allocation.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "accuraterip_core.h"
#include "kernels.h"

namespace lacx {

namespace {

struct alignas(16) ArQuad {
    uint32_t v[4];
};

__global__ __launch_bounds__(kArThreads) void k_accuraterip(ArArgs a) {
    __shared__ ArQuad stage[kArStageWords / 4u];
    __shared__ uint32_t part[2][kArThreads];
    const unsigned long long tile = blockIdx.x;
    uint32_t j = 0, top = a.nspans;  // (uniform) tile_off[j] <= tile < tile_off[top]
    while (top - j > 1u) {
        const uint32_t mid = j + (top - j) / 2u;
        if (a.tile_off[mid] <= tile) j = mid;
        else top = mid;
    }
    const ArSpan sp = a.spans[j];
    const ArTile y = ar_tile(sp, tile - a.tile_off[j]);

    for (uint32_t u = threadIdx.x; u < y.units; u += kArThreads) {  // u < kArStageWords / 4: ar_tile
        ArQuad q;
        ar_load_unit(sp, a.sources, y.first + 4ll * (long long)u, q.v, [&](uint32_t item, unsigned long long key) { atomicMin(&a.bad[item], key); });
        stage[u] = q;
    }
    __syncthreads();

    uint32_t lo, hi;
    ar_lane(reinterpret_cast<const uint32_t*>(stage), sp, y, threadIdx.x, lo, hi);

    // the stripes' parts: lanes tid, tid + lanes, tid + 2 lanes, ... hold the same offset
    if (sp.lanes < 64u) {
        for (uint32_t step = 32u; step >= sp.lanes; step >>= 1) {
            lo += (uint32_t)__shfl_xor((int)lo, (int)step);
            hi += (uint32_t)__shfl_xor((int)hi, (int)step);
        }
    }
    if (sp.lanes < kArThreads) {  // (uniform)
        part[0][threadIdx.x] = lo;
        part[1][threadIdx.x] = hi;
        __syncthreads();
        if (threadIdx.x < sp.lanes) {
            const uint32_t stride = sp.lanes < 64u ? 64u : sp.lanes;  // below a wave of offsets every wave's first lanes hold its sum
            lo = hi = 0u;
            for (uint32_t k = threadIdx.x; k < kArThreads; k += stride) lo += part[0][k], hi += part[1][k];
        }
    }
    const uint32_t o = y.o0 + threadIdx.x;
    if (threadIdx.x < sp.lanes && o < ar_width(sp)) {
        if (lo) atomicAdd(&a.sums[sp.sum0 + o], lo);
        if (sp.keep_hi && lo + hi) atomicAdd(&a.sums[sp.sum0 + ar_width(sp) + o], lo + hi);
    }
}

}  // namespace

hipError_t launch_accuraterip(const ArArgs& a, hipStream_t stream) {
    if (a.nspans && a.total_tiles) hipLaunchKernelGGL(k_accuraterip, dim3((uint32_t)a.total_tiles), dim3(kArThreads), 0, stream, a);
    return hipGetLastError();
}

}  // namespace lacx
