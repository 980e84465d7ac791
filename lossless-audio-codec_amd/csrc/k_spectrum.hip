// k_spectrum.hip -- CDNA4 (gfx950) kernel of the spectrum job: the banded power of the Hann-windowed STFT per
// row of 16384 frames of what a stream decodes to, or of device-resident source PCM (lacx.h, spectrum_core.h).  One launch.
// A workgroup of kSpThreads lanes takes one row of one item (binary search over row_off) and loops over the row's windows
// in order.  Per window: the lanes load the window's N / 4 units of four frames (stats_load_source: every layout, its
// bounds and validation keys), multiply by the window table and store z = w l + i w r into two LDS arrays of N doubles (re,
// im); log2 N radix-2 decimation-in-frequency stages of N / 2 butterflies follow, a barrier between stages, the twiddles
// read from the table in global memory (32 KB at N = 4096, so LDS holds only the points: 64 KB at N = 4096, two workgroups
// per CU; 4 KB at N = 256); then lane c * 64 + band separates its channel's bins out of Z_k and Z_{N-k} (bit-reversed
// places), sums them in bin order and adds the band's power to an accumulator it keeps in a register across the windows.
// Behind the last window the lane writes its accumulator into the row: plain stores, no atomics, no scratch.
// LDS layout: FP64 butterflies at power-of-two strides are the textbook bank-conflict case.  Chosen: split re / im arrays
// of doubles and an XOR swizzle (sp_at) instead of padding -- padding would push N = 4096 past 64 KB.  With 8-byte accesses
// a half-wave of 32 lanes is conflict-free where it covers 32 different doubles modulo 32, a 16-lane group of a store where
// it covers 16 different ones modulo 16.  Stages with h >= 32 read and write 32 consecutive points per half-wave: any
// bijection inside an aligned run of 32 keeps them conflict-free.  Stages with h < 32 take, out of 64 consecutive points,
// those with bit h clear (i) or set (j).  sp_at inverts the low four bits where bit 4 is set and flips bit 4 where bit 5 is
// set: for h < 16 the four runs of 16 then land on (0, S), (1, ~S), (1, S), (0, ~S) in (bit 4, low bits), S the points with
// bit h clear -- 32 different doubles; for h = 16 the two runs land on bit 4 = 0 and 1; and the two runs of a store's 16-lane
// group land on S and ~S.  The band sums' reads at fixed t are the even points of 64 consecutive ones for Z_k (the h = 1
// pattern) but up to 4-way conflicting for Z_{N-k}; they are N + 2 of the (log2 N + 1) N point reads of a window.  This is
// by the bank rule; a counter run of its own over 64 rows of stereo noise (profiles/spectrum_bench.txt) agrees with it:
// SQ_LDS_BANK_CONFLICT is 0.08 - 0.10 of SQ_LDS_IDX_ACTIVE at N = 256 .. 2048 and 0.20 at N = 4096, where a band holds 32 bins.
// Measured (scripts/spectrum_bench.py, profiles/spectrum_bench.txt): 14.4 ms at N = 2048 and 12.4 ms at N = 256 for 4.06 GB
// of 16-bit PCM (34 M and 320 M windows per second), 0.3 TB/s: a tenth of what the memory delivers.  What bounds it -- LDS
// traffic, the barrier per stage, the FP64 arithmetic -- has not been measured.
// A translation unit of its own, like k_truepeak.hip, compiled with -ffp-contract=off (Makefile): spectrum_core.h fixes
// every operation.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.h"
#include "spectrum_core.h"

namespace lacx {

namespace {

// (decode.hip) a pointer read from an item descriptor is generic to the compiler; these all point into global memory
template <typename T>
__device__ __forceinline__ T* global_ptr(T* p) {
    return (T*)(__attribute__((address_space(1))) T*)(uintptr_t)p;
}

template <uint32_t kLogN>
__global__ __launch_bounds__(kSpThreads) void k_spectrum(SpArgs a) {
    constexpr uint32_t kN = 1u << kLogN;
    __shared__ double re[kN], im[kN];
    const unsigned long long row = blockIdx.x;
    uint32_t j = 0, hi = a.nitems;  // (uniform) row_off[j] <= row < row_off[hi]
    while (hi - j > 1u) {
        const uint32_t mid = j + (hi - j) / 2u;
        if (a.row_off[mid] <= row) j = mid;
        else hi = mid;
    }
    SpItem it = a.items[j];
    it.data0 = global_ptr(it.data0);
    it.data1 = global_ptr(it.data1);
    const double* __restrict__ window = global_ptr(a.window);
    const double* __restrict__ twiddle = global_ptr(a.twiddle);
    const uint32_t r = (uint32_t)(row - a.row_off[j]);
    unsigned long long first, end;
    sp_row_windows(it, kLogN, r, first, end);
    const uint32_t c = threadIdx.x / kSpBands, band = threadIdx.x % kSpBands;  // the lane's accumulator (lanes 0 .. 127)

    unsigned long long key = kDigestClean;
    double acc = 0.0;
    for (unsigned long long k = first; k < end; ++k) {
        for (uint32_t u = threadIdx.x; u < kN / 4u; u += kSpThreads) sp_load_unit(it, kLogN, k, u, window, key, re, im);
        __syncthreads();
#pragma unroll 1
        for (uint32_t h = kN / 2u; h; h >>= 1) {
            for (uint32_t b = threadIdx.x; b < kN / 2u; b += kSpThreads) sp_butterfly(kLogN, h, b, twiddle, re, im);
            __syncthreads();
        }
        if (c < it.channels) acc = acc + sp_band_power(kLogN, c, band, re, im);
        __syncthreads();  // the next window's stores
    }
    if (it.validate && key != kDigestClean) atomicMin(&a.bad[j], key);
    if (c < it.channels) a.rows[it.row0 + r].power[c][band] = acc;
}

}  // namespace

hipError_t launch_spectrum(const SpArgs& a, hipStream_t stream) {
    if (!a.nitems || !a.total_rows) return hipGetLastError();
    const dim3 grid((uint32_t)a.total_rows), block(kSpThreads);
    switch (a.logn) {
    case 8: hipLaunchKernelGGL(k_spectrum<8>, grid, block, 0, stream, a); break;
    case 9: hipLaunchKernelGGL(k_spectrum<9>, grid, block, 0, stream, a); break;
    case 10: hipLaunchKernelGGL(k_spectrum<10>, grid, block, 0, stream, a); break;
    case 11: hipLaunchKernelGGL(k_spectrum<11>, grid, block, 0, stream, a); break;
    case 12: hipLaunchKernelGGL(k_spectrum<12>, grid, block, 0, stream, a); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace lacx
