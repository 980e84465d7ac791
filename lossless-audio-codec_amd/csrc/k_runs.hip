// k_runs.hip -- CDNA4 (gfx950) kernel of the run finder: the runs of consecutive frames of what a stream
// decodes to, or of device-resident source PCM, that satisfy a detector's predicate and reach its min_frames -- silence,
// clipping, stuck samples (lacx.h).  One pass over the PCM evaluates all of an item's detectors.
// A workgroup takes one tile of kRunsTileFrames frames of one item, a thread one unit of four frames (runs_core.h).  Per
// detector: the unit's summary, an inclusive scan of the summaries across the wave (six __shfl_up steps with
// runs_combine), the waves' totals combined through LDS, and with the length of the run that enters it every thread walks
// its four frames.  A run that ends inside the tile and does not start it is appended to the (item, detector) list
// through that list's counter: the counter counts every run, the store happens only below the capacity, and the host
// runs the kernel once more with exact capacities where a counter outgrew its list (api_decode.cpp).  The run that starts
// the tile and the run that ends it are the tile's row; the host stitches them (runs_rows.h).  A tile's row is written by
// plain stores of the one thread that knows each half, and every launch over the same PCM stores the same values.
// The list's arrival order depends on the atomics' order; the host sorts by start, so results are the same from run to run.
// A translation unit of its own, like k_stats.hip: helpers shared with other kernels change their register allocation.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.h"
#include "runs_core.h"

namespace lacx {

namespace {

// (decode.hip) a pointer read from an item descriptor is generic to the compiler; these all point into global memory
template <typename T>
__device__ __forceinline__ T* global_ptr(T* p) {
    return (T*)(__attribute__((address_space(1))) T*)(uintptr_t)p;
}

// kSource: DigestSource records, every frame counts; else DecodeItem records whose samples k_ms_inverse left in place, of
// whose blocks only those with index < present[j] and status 0 count.
template <bool kSource>
__global__ __launch_bounds__(kRunsThreads) void k_runs(uint32_t nitems, const unsigned long long* __restrict__ tile_off,
                                                       const RunsItem* __restrict__ ritems, const lacx_run_detector* __restrict__ dets,
                                                       RunsList* __restrict__ lists, RunsRow* __restrict__ rows, lacx_run* __restrict__ runs,
                                                       const DecodeItem* __restrict__ items, const uint32_t* __restrict__ present,
                                                       const DigestSource* __restrict__ src, unsigned long long* __restrict__ bad,
                                                       const unsigned long long* __restrict__ frame_off, const uint32_t* __restrict__ status) {
    __shared__ int32_t last_l[kRunsThreads], last_r[kRunsThreads];
    __shared__ uint32_t last_c[kRunsThreads];
    __shared__ uint32_t wave_tot[LACX_MAX_DETECTORS][kRunsThreads / 64u];
    const unsigned long long tile = blockIdx.x;
    uint32_t j = 0, hi = nitems;  // (uniform) tile_off[j] <= tile < tile_off[hi]
    while (hi - j > 1u) {
        const uint32_t mid = j + (hi - j) / 2u;
        if (tile_off[mid] <= tile) j = mid;
        else hi = mid;
    }
    const unsigned long long t = tile - tile_off[j];
    const unsigned long long tile_start = t * kRunsTileFrames, f0 = tile_start + kDigestUnitFrames * threadIdx.x;
    const RunsItem ri = ritems[j];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;

    // the unit's frames, and (thread 0 of a tile that is not the item's first) the unit in front of the tile
    unsigned long long frames;
    bool stereo;
    RunsUnit u{{0, 0, 0, 0}, {0, 0, 0, 0}, 0u}, before = u;
    if constexpr (kSource) {
        const DigestSource& s = src[j];
        frames = s.frames;
        stereo = s.channels == 2;
        unsigned long long key = kDigestClean, other = kDigestClean;
        if (f0 < frames) u = runs_unit_source(f0, s.channels, s.bit_depth, frames, global_ptr(s.data0), global_ptr(s.data1), s.layout, key);
        if (threadIdx.x == 0u && t != 0u)
            before = runs_unit_source(f0 - 4u, s.channels, s.bit_depth, frames, global_ptr(s.data0), global_ptr(s.data1), s.layout, other);
        if (key != kDigestClean) atomicMin(&bad[j], key);
    } else {
        const DecodeItem& it = items[j];
        frames = it.frames;
        stereo = it.channels == 2;
        if (f0 < frames)
            u = runs_unit_decoded(f0, it.blocks, present[j], it.channels, frames, frame_off + it.block0, it.frame0, global_ptr(it.left),
                                  global_ptr(it.right), status + it.block0);
        if (threadIdx.x == 0u && t != 0u)
            before = runs_unit_decoded(f0 - 4u, it.blocks, present[j], it.channels, frames, frame_off + it.block0, it.frame0, global_ptr(it.left),
                                       global_ptr(it.right), status + it.block0);
    }
    last_l[threadIdx.x] = u.l[3], last_r[threadIdx.x] = u.r[3], last_c[threadIdx.x] = u.counted >> 3;
    __syncthreads();
    const uint32_t from = threadIdx.x ? threadIdx.x - 1u : 0u;
    const int32_t pl = threadIdx.x ? last_l[from] : before.l[3], pr = threadIdx.x ? last_r[from] : before.r[3];
    const bool pc = (threadIdx.x ? last_c[from] : before.counted >> 3) != 0u;

    // per detector: the unit's mask and the summary of the wave's units in front of this one
    uint32_t mask[LACX_MAX_DETECTORS], excl[LACX_MAX_DETECTORS];
#pragma unroll
    for (uint32_t d = 0; d < LACX_MAX_DETECTORS; ++d) {
        mask[d] = 0u, excl[d] = kRunsIdentity;
        if (d < ri.ndet) {  // (uniform)
            mask[d] = runs_mask(dets[ri.det0 + d], u, pl, pr, pc, stereo);
            uint32_t incl = runs_summary(mask[d]);
#pragma unroll
            for (uint32_t step = 1; step < 64u; step <<= 1) {
                const uint32_t up = (uint32_t)__shfl_up((int)incl, step);
                if (lane >= step) incl = runs_combine(up, incl);
            }
            const uint32_t up = (uint32_t)__shfl_up((int)incl, 1u);
            excl[d] = lane ? up : kRunsIdentity;
            if (lane == 63u) wave_tot[d][wave] = incl;
        }
    }
    __syncthreads();
    const bool last_unit = threadIdx.x == kRunsThreads - 1u;
#pragma unroll
    for (uint32_t d = 0; d < LACX_MAX_DETECTORS; ++d) {
        if (d < ri.ndet) {
            uint32_t prefix = kRunsIdentity;  // the waves in front of this one
            for (uint32_t w = 0; w < wave; ++w) prefix = runs_combine(prefix, wave_tot[d][w]);
            const uint32_t enter = runs_combine(prefix, excl[d]) & ~kRunsAll;
            RunsList* list = &lists[ri.det0 + d];
            const unsigned long long off = list->off, cap = list->cap;
            const RunsWalk w = runs_walk(mask[d], enter, f0, tile_start, dets[ri.det0 + d].min_frames, [&](unsigned long long start, unsigned long long n) {
                const unsigned long long at = atomicAdd(&list->count, 1ull);
                if (at < cap) runs[off + at] = lacx_run{start, n};
            });
            RunsRow* row = &rows[ri.row0 + t * ri.ndet + d];
            if (w.lead) row->lead = (uint16_t)w.lead;
            if (last_unit) {
                row->trail = (uint16_t)w.exit;
                if (w.exit == kRunsTileFrames) row->lead = (uint16_t)w.exit;
            }
        }
    }
}

}  // namespace

hipError_t launch_runs(const RunsArgs& a, hipStream_t stream) {
    if (a.total_tiles)
        hipLaunchKernelGGL(k_runs<false>, dim3((uint32_t)a.total_tiles), dim3(kRunsThreads), 0, stream, a.nitems, a.tile_off, a.items, a.dets, a.lists,
                           a.rows, a.runs, a.dec.items, a.dec.present, nullptr, nullptr, a.dec.frame_off, a.dec.status);
    return hipGetLastError();
}

hipError_t launch_runs_pcm(const RunsArgs& a, hipStream_t stream) {
    if (a.total_tiles)
        hipLaunchKernelGGL(k_runs<true>, dim3((uint32_t)a.total_tiles), dim3(kRunsThreads), 0, stream, a.nitems, a.tile_off, a.items, a.dets, a.lists,
                           a.rows, a.runs, nullptr, nullptr, a.src, a.bad, nullptr, nullptr);
    return hipGetLastError();
}

}  // namespace lacx
