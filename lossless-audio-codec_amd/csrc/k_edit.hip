// k_edit.hip -- the edit pass of a transcode job: every output's staged planar int32 PCM through its channel operation and
// depth change into the layout the encoder's front kernels read, validated on the way (edit_core.h).  One launch covers
// every output of the job and runs on the decoder's stream behind the window job that filled the staging.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "edit_core.h"
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

// Laid out like k_import: workgroup u handles unit u of the concatenated unit ranges of the outputs (unit_off: [nitems + 1]
// prefix sums of ceil(frames / kEditUnitFrames)), found by a uniform binary search; a unit lies in one output, so a wave's
// threads share their output and its transforms.  Thread t of the unit handles the four frames from 4 t on (edit_quad):
// consecutive lanes read consecutive 16-byte pieces of each staging row and write consecutive 8 .. 24-byte pieces.
// Validation: a wave in which no frame breaks a rule -- the common case -- issues no atomic at all; otherwise the wave's
// lowest key is reduced with shuffles and lane 0 issues one 64-bit atomicMin.
__global__ __launch_bounds__(kEditThreads) void k_edit(EditJob job, EditBad* __restrict__ bad) {
    unsigned long long unit = blockIdx.x;
    uint32_t j = 0, hi = job.nitems;  // unit_off[j] <= unit < unit_off[hi]
    while (hi - j > 1u) {
        const uint32_t mid = j + (hi - j) / 2u;
        if (job.unit_off[mid] <= unit) j = mid;
        else hi = mid;
    }
    unit -= job.unit_off[j];
    EditItem it = job.table[j];
    it.left = global_ptr(it.left);
    it.right = global_ptr(it.right);
    it.dst = global_ptr(it.dst);
    const unsigned long long f0 = unit * kEditUnitFrames + kEditQuad * threadIdx.x;
    unsigned long long key = kEditClean;
    if (f0 < it.frames) edit_quad(it, f0, key);
    if (__ballot(key != kEditClean) == 0ull) return;
    key = wave_min(key);
    if ((threadIdx.x & 63u) == 0u) atomicMin(&bad[j].key, key);
}

hipError_t launch_edit(const EditJob& job, EditBad* bad, hipStream_t stream) {
    if (job.nitems == 0 || job.total_units == 0 || job.total_units > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_edit, dim3((uint32_t)job.total_units), dim3(kEditThreads), 0, stream, job, bad);
    return hipGetLastError();
}

}  // namespace lacx
