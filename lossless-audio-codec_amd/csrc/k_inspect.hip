// k_inspect.hip -- CDNA4 (gfx950) kernels of the stream inspection (lacx.h): how a stream was coded and where
// its bits go, read out of the bytes by a parse-only walk (inspect_core.h).
// A channel block's header sits behind the previous channel's residuals, which carry no length, so even the second
// channel's header needs a walk of the whole first channel; but the Rice adaptation depends on residual magnitudes alone,
// so the walk needs no synthesis and no PCM.  Laid out as k_decode: ONE LANE PER BLOCK over the job's lane table, all
// blocks of every stream at once; a lane's indexed state is the 256-entry drift window of the stateful adaptation, one
// LDS column per lane (64 KiB per workgroup of one wave).
//   k_inspect         one lane per version-3 block -> one lacx_block_info, and with partition detail the entries
//   k_inspect_serial  the same for a version-2 stream (no compressed sizes): one lane walks it
// A lane writes the whole row itself (zeros first, the coefficients as they are read, the tally at the end of each
// channel block), so the rows need no initialisation; the partition entries are zeroed by launch_inspect.
// A translation unit of its own: nothing here is shared with decode.hip but headers, and k_decode's code is unchanged.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "inspect_core.h"
#include "kernels.h"

namespace lacx {

__global__ __launch_bounds__(kDecThreads) void k_inspect(uint32_t lanes, const uint32_t* __restrict__ lane_blk,
                                                         const uint32_t* __restrict__ blk_item,
                                                         const DecodeItem* __restrict__ items,
                                                         const uint8_t* __restrict__ payload,
                                                         const unsigned long long* __restrict__ byte_off,
                                                         const unsigned long long* __restrict__ frame_off,
                                                         lacx_block_info* __restrict__ rows, uint8_t* __restrict__ mode_k,
                                                         uint32_t* __restrict__ part_bits) {
    extern __shared__ __align__(16) unsigned char ins_raw[];
    DecMem dm = inspect_mem(ins_raw, blockDim.x);
    const int lane = (int)threadIdx.x;
    DecWave wave;
    const uint32_t g = blockIdx.x * kDecThreads + threadIdx.x;
    if (g >= lanes) return;
    const uint32_t blk = lane_blk[g];
    if (blk == ~0u) return;
    const DecodeItem& it = items[blk_item[blk]];
    inspect_block_lane(blk, it.channels, it.stereo_mode, payload, byte_off, frame_off, rows, mode_k, part_bits, dm, lane, wave);
}

__global__ __launch_bounds__(kDecThreads) void k_inspect_serial(uint32_t nv2, const uint32_t* __restrict__ v2_items,
                                                                const DecodeItem* __restrict__ items,
                                                                const uint8_t* __restrict__ payload,
                                                                const unsigned long long* __restrict__ frame_off,
                                                                lacx_block_info* __restrict__ rows, uint8_t* __restrict__ mode_k,
                                                                uint32_t* __restrict__ part_bits) {
    extern __shared__ __align__(16) unsigned char ins_raw[];
    DecMem dm = inspect_mem(ins_raw, kDecThreads);
    DecWave wave;
    const uint32_t g = blockIdx.x * kDecThreads + threadIdx.x;
    if (g >= nv2) return;
    const DecodeItem& it = items[v2_items[g]];
    const size_t slots = (size_t)it.block0 * 2u * kInspectPartSlots;
    inspect_serial_lane(it.blocks, it.channels, it.stereo_mode, payload + it.pay_off, it.pay_bits, frame_off + it.block0, rows + it.block0,
                        mode_k ? mode_k + slots : nullptr, part_bits ? part_bits + slots : nullptr, dm, (int)threadIdx.x, wave);
}

hipError_t launch_inspect(const InspectArgs& s, hipStream_t stream) {
    const DecodeArgs& a = s.dec;
    const size_t smem = kInspectBytesPerCol * kDecThreads;
    if (s.mode_k && a.total_blocks) {  // the entries beyond a channel block's partitions are written by nobody
        hipError_t e = hipMemsetAsync(s.mode_k, 0, (size_t)a.total_blocks * 2u * kInspectPartSlots, stream);
        if (e == hipSuccess) e = hipMemsetAsync(s.part_bits, 0, (size_t)a.total_blocks * 2u * kInspectPartSlots * 4u, stream);
        if (e != hipSuccess) return e;
    }
    if (a.lanes) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_inspect), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(k_inspect, dim3((a.lanes + kDecThreads - 1) / kDecThreads), dim3(kDecThreads), smem, stream, a.lanes, a.lane_blk,
                           a.blk_item, a.items, a.payload, a.byte_off, a.frame_off, s.rows, s.mode_k, s.part_bits);
    }
    if (a.nv2) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_inspect_serial), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(k_inspect_serial, dim3((a.nv2 + kDecThreads - 1) / kDecThreads), dim3(kDecThreads), smem, stream, a.nv2, a.v2_items,
                           a.items, a.payload, a.frame_off, s.rows, s.mode_k, s.part_bits);
    }
    return hipGetLastError();
}

}  // namespace lacx
