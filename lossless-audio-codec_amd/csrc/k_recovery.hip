// k_recovery.hip -- CDNA4 (gfx950) kernels of the recovery data: Reed-Solomon erasure coding over GF(2^8)
// on whole .lac files, many files as one job.  The per-thread code is recovery_core.h's, shared with the CPU twin.
//   k_gf_combine   out[t][o] = XOR_i M[t][o][i] * in[t][i] over a task table.  Making parity and repairing are the same
//                  kernel: the inputs are a group's data slices and the matrix its Cauchy rows, or the inputs are usable
//                  parity plus surviving data and the matrix the one the host solved.  A thread owns one word column of
//                  its task's slices: a wave reads and writes 256 consecutive bytes per slice, and the accumulators --
//                  8, 16 or 32 by the instantiation -- stay in registers.  No LDS, no table.
//   k_slice_crc    one CRC-32 per listed byte range, a wave per range.
// A translation unit of its own, like k_digest.hip.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.h"
#include "recovery_core.h"

namespace lacx {

namespace {

// The tasks [t0, t1) of one tier; the task of a workgroup is found by one uniform search, so everything that depends on
// the task alone -- the slices' offsets, the coefficients -- is scalar.
template <uint32_t kOuts>
__global__ __launch_bounds__(kGfThreads) void k_gf_combine(const GfTask* __restrict__ tasks, uint32_t t0, uint32_t t1,
                                                           const unsigned long long* __restrict__ refs, const uint8_t* __restrict__ mat,
                                                           uint8_t* arena) {
    const uint32_t ti = gf_task_of(tasks, t0, t1, blockIdx.x);
    const GfTask t = tasks[ti];
    const uint32_t col = (blockIdx.x - t.wg0) * kGfThreads + threadIdx.x;
    if (col >= t.words) return;
    gf_combine_column<kOuts>(t, refs, mat, arena, col);
}

__global__ __launch_bounds__(kCrcThreads) void k_slice_crc(const CrcRange* __restrict__ ranges, uint32_t nranges, const uint8_t* __restrict__ arena,
                                                           uint32_t* __restrict__ crc) {
    const uint32_t q = blockIdx.x * (kCrcThreads / 64u) + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (q >= nranges) return;  // (uniform per wave)
    const CrcRange r = ranges[q];
    uint32_t v = slice_crc_lane(arena, r, lane);
#pragma unroll
    for (int step = 1; step < 64; step <<= 1) v ^= (uint32_t)__shfl_xor((int)v, step);
    if (lane == 0u) crc[q] = crc_finish(v, r.len);
}

}  // namespace

hipError_t launch_recovery(const RecoveryArgs& a, hipStream_t stream) {
    const uint32_t* t0 = a.tier_t0;
    if (a.tier_wgs[0])
        hipLaunchKernelGGL(k_gf_combine<8>, dim3(a.tier_wgs[0]), dim3(kGfThreads), 0, stream, a.tasks, t0[0], t0[1], a.refs, a.mat, a.arena);
    if (a.tier_wgs[1])
        hipLaunchKernelGGL(k_gf_combine<16>, dim3(a.tier_wgs[1]), dim3(kGfThreads), 0, stream, a.tasks, t0[1], t0[2], a.refs, a.mat, a.arena);
    if (a.tier_wgs[2])
        hipLaunchKernelGGL(k_gf_combine<32>, dim3(a.tier_wgs[2]), dim3(kGfThreads), 0, stream, a.tasks, t0[2], t0[3], a.refs, a.mat, a.arena);
    if (a.nranges)
        hipLaunchKernelGGL(k_slice_crc, dim3((a.nranges + kCrcThreads / 64u - 1u) / (kCrcThreads / 64u)), dim3(kCrcThreads), 0, stream, a.ranges,
                           a.nranges, a.arena, a.crc);
    return hipGetLastError();
}

}  // namespace lacx
