// k_import.hip -- the import pass: device-resident PCM in a tensor layout (planar int16, planar / interleaved float32)
// rewritten into a layout the front kernels read, validated on the way (import_core.h).  One launch covers every source of
// a job -- the sources of a batch, whatever their layouts -- and runs on the job's stream in front of k_ingest.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "import_core.h"
#include "kernels.h"

namespace lacx {

namespace {

// (see decode.hip: a pointer read from a descriptor is generic to the compiler; these all point into global memory)
template <typename T>
__device__ __forceinline__ T* global_ptr(T* p) {
    return (T*)(__attribute__((address_space(1))) T*)(uintptr_t)p;
}

__device__ __forceinline__ unsigned long long wave_min(unsigned long long v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const unsigned long long o = __shfl_xor(v, d, 64);
        v = o < v ? o : v;
    }
    return v;
}

}  // namespace

// Workgroup u handles unit u of the concatenated unit ranges of the items (unit_off: [nitems + 1] prefix sums of
// ceil(frames / kImportUnitFrames)), found by a uniform binary search; a unit lies in one item, so a wave's threads share
// their item and its layout.  Thread t of the unit handles the four frames from 4 t on (import_quad): consecutive lanes
// read and write consecutive 8 .. 32-byte pieces.  Validation: a wave in which every float is a sample -- the common case --
// issues no atomic at all; otherwise the wave's lowest keys are reduced with shuffles and lane 0 issues one 64-bit
// atomicMin per channel that has one.
__global__ __launch_bounds__(kImportThreads) void k_import(ImportJob job, ImportBad* __restrict__ bad) {
    unsigned long long unit = blockIdx.x;
    uint32_t j = 0;
    ImportItem it = job.single;
    if (job.table) {
        uint32_t hi = job.nitems;  // unit_off[j] <= unit < unit_off[hi]
        while (hi - j > 1u) {
            const uint32_t mid = j + (hi - j) / 2u;
            if (job.unit_off[mid] <= unit) j = mid;
            else hi = mid;
        }
        unit -= job.unit_off[j];
        it = job.table[j];
    }
    it.src0 = global_ptr(it.src0);
    it.src1 = global_ptr(it.src1);
    it.dst = global_ptr(it.dst);
    const unsigned long long f0 = unit * kImportUnitFrames + kImportQuad * threadIdx.x;
    unsigned long long key_l = kImportClean, key_r = kImportClean;
    if (f0 < it.frames) import_quad(it, f0, key_l, key_r);
    if (__ballot((key_l & key_r) != kImportClean) == 0ull) return;
    key_l = wave_min(key_l);
    key_r = wave_min(key_r);
    if ((threadIdx.x & 63u) == 0u) {
        if (key_l != kImportClean) atomicMin(&bad[j].key[0], key_l);
        if (key_r != kImportClean) atomicMin(&bad[j].key[1], key_r);
    }
}

hipError_t launch_import(const ImportJob& job, ImportBad* bad, hipStream_t stream) {
    if (job.total_units == 0 || job.total_units > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_import, dim3((uint32_t)job.total_units), dim3(kImportThreads), 0, stream, job, bad);
    return hipGetLastError();
}

}  // namespace lacx
