// k_x87_hooks.hip -- test entry points of liblacx_hooks.so only (never linked into liblacx.so): the software x87 model
// of x87.h operation by operation on the device, and the product's k_levinson over caller-made autocorrelation tables.
//
//   lacx_hook_x87_ops          one thread per element: xf_add, xf_sub, xf_mul, xf_div, xf_from_i64 as raw (m, e, s), xf_lt
//                              and xf_to_q15(a) as ints.  The kernel here is compiled apart from k_levinson: what it shows
//                              is the device compile of x87.h, not the kernel that uses it.
//   lacx_hook_levinson_tables  k_levinson as launch_analysis launches it (k_analyze.hip: grid, block size, sizeof(LevMem)
//                              dynamic LDS), on a one-stream BatchRef or on a stream table, over tables [blocks][16][13]
//                              and need_probe words of the caller; the LpcSet array goes up as the caller filled it (a
//                              sentinel) and comes back with whatever the kernel wrote.
#include <hip/hip_runtime.h>

#include <vector>

#include "encoder_impl.h"
#include "kernels_internal.h"
#include "x87.h"

namespace lacx {

constexpr int kX87OpsThreads = 256;
constexpr int kX87Results = 5;  // add, sub, mul, div, from_i64

__global__ __launch_bounds__(kX87OpsThreads) void k_x87_ops(uint32_t n, const uint64_t* __restrict__ in_m,
                                                            const int32_t* __restrict__ in_e,
                                                            const uint32_t* __restrict__ in_s,
                                                            const int64_t* __restrict__ in_i, uint64_t* __restrict__ out_m,
                                                            int32_t* __restrict__ out_e, uint32_t* __restrict__ out_s,
                                                            int32_t* __restrict__ out_i) {
    const uint32_t i = blockIdx.x * (uint32_t)kX87OpsThreads + threadIdx.x;
    if (i >= n) return;
    const xf80 a{in_m[i], in_e[i], in_s[i]};
    const xf80 b{in_m[(size_t)n + i], in_e[(size_t)n + i], in_s[(size_t)n + i]};
    const xf80 r[kX87Results] = {xf_add(a, b), xf_sub(a, b), xf_mul(a, b), xf_div(a, b), xf_from_i64(in_i[i])};
#pragma unroll
    for (int k = 0; k < kX87Results; ++k) {
        out_m[(size_t)k * n + i] = r[k].m;
        out_e[(size_t)k * n + i] = r[k].e;
        out_s[(size_t)k * n + i] = r[k].s;
    }
    out_i[i] = xf_lt(a, b) ? 1 : 0;
    out_i[(size_t)n + i] = (int32_t)xf_to_q15(a);
}

}  // namespace lacx

namespace {

// device memory of one call
struct DevMem {
    std::vector<void*> ptrs;
    ~DevMem() {
        for (void* p : ptrs) (void)hipFree(p);
    }
    template <class T>
    hipError_t get(T** out, size_t count) {
        void* p = nullptr;
        const hipError_t e = hipMalloc(&p, count * sizeof(T));
        if (e == hipSuccess) ptrs.push_back(p);
        *out = static_cast<T*>(p);
        return e;
    }
};

int hook_device(lacx_encoder* e) {
    const int rc = ensure_device(e);
    if (rc) return rc;
    HIP_TRY(e, hipSetDevice(e->device), "hipSetDevice");
    return LACX_OK;
}

}  // namespace

extern "C" {

// One stream of lacx_hook_levinson_tables: ceil(frames / 16384) blocks, the last one short where frames says so.
struct lacx_hook_stream {
    uint64_t frames;      // >= 1
    int32_t channels;     // 1 or 2
    int32_t stereo_mode;  // 0 LR, 1 MS, 2 per-block
};

// in_m / in_e / in_s: [2][n] operands a then b (b != 0: xf_div requires it); in_i: [n].
// out_m / out_e / out_s: [5][n] add, sub, mul, div, from_i64; out_i: [2][n] lt, q15(a).
int lacx_hook_x87_ops(lacx_encoder* e, uint32_t n, const uint64_t* in_m, const int32_t* in_e, const uint32_t* in_s,
                      const int64_t* in_i, uint64_t* out_m, int32_t* out_e, uint32_t* out_s, int32_t* out_i) {
    if (!e || n == 0 || n > (1u << 24) || !in_m || !in_e || !in_s || !in_i || !out_m || !out_e || !out_s || !out_i)
        return LACX_E_INVALID;
    int rc = hook_device(e);
    if (rc) return rc;
    DevMem mem;
    uint64_t *d_im, *d_om;
    int32_t *d_ie, *d_oe, *d_oi;
    uint32_t *d_is, *d_os;
    int64_t* d_ii;
    const size_t N = n;
    HIP_TRY(e, mem.get(&d_im, 2 * N), "hipMalloc(x87 ops)");
    HIP_TRY(e, mem.get(&d_ie, 2 * N), "hipMalloc(x87 ops)");
    HIP_TRY(e, mem.get(&d_is, 2 * N), "hipMalloc(x87 ops)");
    HIP_TRY(e, mem.get(&d_ii, N), "hipMalloc(x87 ops)");
    HIP_TRY(e, mem.get(&d_om, kX87Results * N), "hipMalloc(x87 ops)");
    HIP_TRY(e, mem.get(&d_oe, kX87Results * N), "hipMalloc(x87 ops)");
    HIP_TRY(e, mem.get(&d_os, kX87Results * N), "hipMalloc(x87 ops)");
    HIP_TRY(e, mem.get(&d_oi, 2 * N), "hipMalloc(x87 ops)");
    hipStream_t st = e->stream[0];
    HIP_TRY(e, hipMemcpyAsync(d_im, in_m, 2 * N * sizeof(uint64_t), hipMemcpyHostToDevice, st), "H2D x87 operands");
    HIP_TRY(e, hipMemcpyAsync(d_ie, in_e, 2 * N * sizeof(int32_t), hipMemcpyHostToDevice, st), "H2D x87 operands");
    HIP_TRY(e, hipMemcpyAsync(d_is, in_s, 2 * N * sizeof(uint32_t), hipMemcpyHostToDevice, st), "H2D x87 operands");
    HIP_TRY(e, hipMemcpyAsync(d_ii, in_i, N * sizeof(int64_t), hipMemcpyHostToDevice, st), "H2D x87 operands");
    // results nobody wrote must not look like results
    HIP_TRY(e, hipMemsetAsync(d_om, 0xA5, kX87Results * N * sizeof(uint64_t), st), "memset x87 results");
    HIP_TRY(e, hipMemsetAsync(d_oe, 0xA5, kX87Results * N * sizeof(int32_t), st), "memset x87 results");
    HIP_TRY(e, hipMemsetAsync(d_os, 0xA5, kX87Results * N * sizeof(uint32_t), st), "memset x87 results");
    HIP_TRY(e, hipMemsetAsync(d_oi, 0xA5, 2 * N * sizeof(int32_t), st), "memset x87 results");
    hipLaunchKernelGGL(lacx::k_x87_ops, dim3((n + kX87OpsThreads - 1) / kX87OpsThreads), dim3(kX87OpsThreads), 0, st, n, d_im,
                       d_ie, d_is, d_ii, d_om, d_oe, d_os, d_oi);
    HIP_TRY(e, hipGetLastError(), "k_x87_ops");
    HIP_TRY(e, hipMemcpyAsync(out_m, d_om, kX87Results * N * sizeof(uint64_t), hipMemcpyDeviceToHost, st), "D2H x87 results");
    HIP_TRY(e, hipMemcpyAsync(out_e, d_oe, kX87Results * N * sizeof(int32_t), hipMemcpyDeviceToHost, st), "D2H x87 results");
    HIP_TRY(e, hipMemcpyAsync(out_s, d_os, kX87Results * N * sizeof(uint32_t), hipMemcpyDeviceToHost, st), "D2H x87 results");
    HIP_TRY(e, hipMemcpyAsync(out_i, d_oi, 2 * N * sizeof(int32_t), hipMemcpyDeviceToHost, st), "D2H x87 results");
    HIP_TRY(e, hipStreamSynchronize(st), "k_x87_ops");
    return LACX_OK;
}

// acorr: [total_blocks][16][13]; need_probe: [total_blocks]; lpcs: [total_blocks][16], in and out.  streams: the blocks
// of the launch set in order; as_table != 0 (or more than one stream): the kernel looks its stream up in a device table.
int lacx_hook_levinson_tables(lacx_encoder* e, const int64_t* acorr, const uint32_t* need_probe,
                              const lacx_hook_stream* streams, uint32_t nstreams, int as_table, uint32_t total_blocks,
                              void* lpcs) {
    if (!e || !acorr || !need_probe || !streams || !lpcs || nstreams == 0 || total_blocks == 0 || total_blocks > (1u << 16))
        return LACX_E_INVALID;
    std::vector<StreamDesc> table(nstreams);
    uint32_t first = 0;
    for (uint32_t i = 0; i < nstreams; ++i) {
        const lacx_hook_stream& s = streams[i];
        if (s.frames == 0 || s.frames > (uint64_t)(1u << 16) * kMaxBlock || (s.channels != 1 && s.channels != 2) ||
            s.stereo_mode < 0 || s.stereo_mode > 2)
            return fail(e, LACX_E_INVALID, "lacx_hook_levinson_tables: bad stream shape");
        StreamDesc sd{};
        sd.prm.frames = s.frames;
        sd.prm.num_blocks = (uint32_t)((s.frames + kMaxBlock - 1) / kMaxBlock);
        sd.prm.channels = s.channels;
        sd.prm.stereo_mode = s.stereo_mode;
        sd.prm.zero_run = 1;
        sd.prm.partitioning = 1;
        sd.first_block = first;
        sd.pad = i;
        first += sd.prm.num_blocks;
        table[i] = sd;
    }
    if (first != total_blocks) return fail(e, LACX_E_INVALID, "lacx_hook_levinson_tables: the streams' blocks are not total_blocks");
    int rc = hook_device(e);
    if (rc) return rc;
    HIP_TRY(e, ensure_kernel_attrs(), "kernel attributes");
    DevMem mem;
    const size_t slots = (size_t)total_blocks * kSlotsPerBlock;
    int64_t* d_acorr;
    uint32_t* d_need;
    LpcSet* d_lpcs;
    StreamDesc* d_table = nullptr;
    HIP_TRY(e, mem.get(&d_acorr, slots * 13), "hipMalloc(tables)");
    HIP_TRY(e, mem.get(&d_need, (size_t)total_blocks), "hipMalloc(need_probe)");
    HIP_TRY(e, mem.get(&d_lpcs, slots), "hipMalloc(lpc sets)");
    hipStream_t st = e->stream[0];
    BatchRef br{};
    br.nstreams = nstreams;
    br.total_blocks = total_blocks;
    if (nstreams > 1 || as_table) {
        HIP_TRY(e, mem.get(&d_table, (size_t)nstreams), "hipMalloc(stream table)");
        HIP_TRY(e, hipMemcpyAsync(d_table, table.data(), nstreams * sizeof(StreamDesc), hipMemcpyHostToDevice, st), "H2D stream table");
        br.table = d_table;
    } else {
        br.single = table[0];
    }
    HIP_TRY(e, hipMemcpyAsync(d_acorr, acorr, slots * 13 * sizeof(int64_t), hipMemcpyHostToDevice, st), "H2D tables");
    HIP_TRY(e, hipMemcpyAsync(d_need, need_probe, total_blocks * sizeof(uint32_t), hipMemcpyHostToDevice, st), "H2D need_probe");
    HIP_TRY(e, hipMemcpyAsync(d_lpcs, lpcs, slots * sizeof(LpcSet), hipMemcpyHostToDevice, st), "H2D lpc sets");
    // exactly launch_analysis's launch (k_analyze.hip, launch_front)
    hipLaunchKernelGGL(k_levinson, dim3((total_blocks * kSlotsPerBlock + kLevThreads - 1) / kLevThreads), dim3(kLevThreads),
                       sizeof(LevMem), st, br, d_acorr, d_need, d_lpcs);
    HIP_TRY(e, hipGetLastError(), "k_levinson");
    HIP_TRY(e, hipMemcpyAsync(lpcs, d_lpcs, slots * sizeof(LpcSet), hipMemcpyDeviceToHost, st), "D2H lpc sets");
    HIP_TRY(e, hipStreamSynchronize(st), "k_levinson");
    return LACX_OK;
}

}  // extern "C"
