// k_front_hooks.hip -- test entry point of liblacx_hooks.so only (never linked into liblacx.so): the product's k_ingest
// (and k_stereo) over caller-placed PCM, every word of what they write handed back.
//
//   lacx_hook_ingest_tables  k_ingest as launch_analysis launches it (k_analyze.hip, launch_front: grid blocks * 4,
//                            kIngestThreads, no dynamic LDS; k_stereo behind it where the estimate is not folded in), on a
//                            one-stream BatchRef or on a stream table, over PCM that already lies in device memory in one of
//                            the three source layouts.  sums, badidx, acorr, bplans and the two need masks are filled with a
//                            sentinel byte in front of every run and come back with whatever the kernels wrote; front_ctr is
//                            zeroed ONCE, in front of the first run, and comes back after every run: the kernels themselves
//                            must leave it zero.
#include <hip/hip_runtime.h>

#include <vector>

#include "encoder_impl.h"
#include "kernels_internal.h"

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

constexpr int kIngestSentinel = 0xA5;

}  // namespace

extern "C" {

// One stream of lacx_hook_ingest_tables: ceil(frames / 16384) blocks, the last one short where frames says so.  The PCM
// lies in device memory: planar int32 (data0 = left, data1 = right or null; 4-byte aligned), interleaved int16 (data0,
// 4-byte aligned) or packed interleaved int24 (data0, any byte), `frames` frames of it.
struct lacx_hook_ingest_stream {
    uint64_t frames;      // >= 1
    const void* data0;
    const void* data1;
    int32_t channels;     // 1 or 2
    int32_t stereo_mode;  // 0 LR, 1 MS, 2 per-block
    int32_t bit_depth;    // 0 (no validation), 16 or 24
    int32_t layout;       // PCM_PLANAR_I32 / PCM_INTERLEAVED_I16 / PCM_INTERLEAVED_I24
};

// streams: the blocks of the launch set in order; as_table != 0 (or more than one stream): the kernels look their stream
// up in a device table.  fold != 0: front_ctr is handed to k_ingest (the last workgroup of a block makes its estimate);
// 0: null, and k_stereo follows.  The kernels run `repeat` times on the same workspace.  Results, one set per run:
// sums [repeat][total_blocks][12], badidx [repeat][total_blocks][2], acorr [repeat][total_blocks][16][13],
// bplans [repeat][total_blocks] (BlockPlan), need_probe / need_full [repeat][total_blocks],
// front_ctr [repeat][total_blocks][2].
int lacx_hook_ingest_tables(lacx_encoder* e, const lacx_hook_ingest_stream* streams, uint32_t nstreams, int as_table,
                            int fold, uint32_t repeat, uint32_t total_blocks, unsigned long long* sums, uint32_t* badidx,
                            int64_t* acorr, void* bplans, uint32_t* need_probe, uint32_t* need_full, uint32_t* front_ctr) {
    if (!e || !streams || !sums || !badidx || !acorr || !bplans || !need_probe || !need_full || !front_ctr)
        return LACX_E_INVALID;
    if (nstreams == 0 || total_blocks == 0 || total_blocks > (1u << 16) || repeat == 0 || repeat > 16)
        return fail(e, LACX_E_INVALID, "lacx_hook_ingest_tables: bad stream, block or repeat count");
    std::vector<StreamDesc> table(nstreams);
    uint32_t first = 0;
    for (uint32_t i = 0; i < nstreams; ++i) {
        const lacx_hook_ingest_stream& s = streams[i];
        if (s.frames == 0 || s.frames > (uint64_t)(1u << 16) * kMaxBlock || (s.channels != 1 && s.channels != 2) ||
            s.stereo_mode < 0 || s.stereo_mode > 2)
            return fail(e, LACX_E_INVALID, "lacx_hook_ingest_tables: bad stream shape");
        if (s.bit_depth != 0 && s.bit_depth != 16 && s.bit_depth != 24)
            return fail(e, LACX_E_INVALID, "lacx_hook_ingest_tables: bit depth must be 0, 16 or 24");
        if (s.layout != PCM_PLANAR_I32 && s.layout != PCM_INTERLEAVED_I16 && s.layout != PCM_INTERLEAVED_I24)
            return fail(e, LACX_E_INVALID, "lacx_hook_ingest_tables: unknown layout");
        if (s.layout == PCM_INTERLEAVED_I16 && s.bit_depth == 24)
            return fail(e, LACX_E_INVALID, "lacx_hook_ingest_tables: 16-bit containers hold no 24-bit stream");
        const bool planar = s.layout == PCM_PLANAR_I32;
        if (!s.data0 || (planar && s.channels == 2 && !s.data1) || ((!planar || s.channels == 1) && s.data1))
            return fail(e, LACX_E_INVALID, "lacx_hook_ingest_tables: the arrays do not fit the layout and channel count");
        const uintptr_t a0 = reinterpret_cast<uintptr_t>(s.data0), a1 = reinterpret_cast<uintptr_t>(s.data1);
        if (s.layout != PCM_INTERLEAVED_I24 && ((a0 & 3u) || (a1 & 3u)))
            return fail(e, LACX_E_INVALID, "lacx_hook_ingest_tables: PCM arrays are not 4-byte aligned");
        StreamDesc sd{};
        sd.prm = make_params(ParamBase{}, s.frames, s.channels, s.stereo_mode, s.bit_depth, s.layout);
        sd.left = static_cast<const int32_t*>(s.data0);
        sd.right = static_cast<const int32_t*>(s.data1);
        sd.first_block = first;
        sd.pad = i;
        first += sd.prm.num_blocks;
        if (first > total_blocks) break;
        table[i] = sd;
    }
    if (first != total_blocks) return fail(e, LACX_E_INVALID, "lacx_hook_ingest_tables: the streams' blocks are not total_blocks");
    int rc = ensure_device(e);
    if (rc) return rc;
    HIP_TRY(e, hipSetDevice(e->device), "hipSetDevice");
    DevMem mem;
    const size_t nb = total_blocks;
    unsigned long long* d_sums;
    uint32_t *d_bad, *d_probe, *d_full, *d_ctr;
    int64_t* d_acorr;
    BlockPlan* d_bplans;
    StreamDesc* d_table = nullptr;
    HIP_TRY(e, mem.get(&d_sums, nb * 12), "hipMalloc(sums)");
    HIP_TRY(e, mem.get(&d_bad, nb * 2), "hipMalloc(badidx)");
    HIP_TRY(e, mem.get(&d_acorr, nb * kSlotsPerBlock * 13), "hipMalloc(acorr)");
    HIP_TRY(e, mem.get(&d_bplans, nb), "hipMalloc(block plans)");
    HIP_TRY(e, mem.get(&d_probe, nb), "hipMalloc(need_probe)");
    HIP_TRY(e, mem.get(&d_full, nb), "hipMalloc(need_full)");
    HIP_TRY(e, mem.get(&d_ctr, nb * 2), "hipMalloc(front counters)");
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
    HIP_TRY(e, hipMemsetAsync(d_ctr, 0, nb * 2 * sizeof(uint32_t), st), "memset front counters");
    uint32_t* fc = fold ? d_ctr : nullptr;
    const uint32_t cnt = total_blocks;
    for (uint32_t r = 0; r < repeat; ++r) {
        // words nobody wrote must not look like results
        HIP_TRY(e, hipMemsetAsync(d_sums, kIngestSentinel, nb * 12 * sizeof(unsigned long long), st), "memset ingest results");
        HIP_TRY(e, hipMemsetAsync(d_bad, kIngestSentinel, nb * 2 * sizeof(uint32_t), st), "memset ingest results");
        HIP_TRY(e, hipMemsetAsync(d_acorr, kIngestSentinel, nb * kSlotsPerBlock * 13 * sizeof(int64_t), st), "memset ingest results");
        HIP_TRY(e, hipMemsetAsync(d_bplans, kIngestSentinel, nb * sizeof(BlockPlan), st), "memset ingest results");
        HIP_TRY(e, hipMemsetAsync(d_probe, kIngestSentinel, nb * sizeof(uint32_t), st), "memset ingest results");
        HIP_TRY(e, hipMemsetAsync(d_full, kIngestSentinel, nb * sizeof(uint32_t), st), "memset ingest results");
        // exactly launch_analysis's launches (k_analyze.hip, launch_front)
        hipLaunchKernelGGL(k_ingest, dim3(cnt * 4u), dim3(kIngestThreads), 0, st, br, d_sums, d_bad, d_acorr, fc, d_bplans, d_probe,
                           d_full);
        HIP_TRY(e, hipGetLastError(), "k_ingest");
        if (!fc) {
            hipLaunchKernelGGL(k_stereo, dim3((cnt + 3) / 4), dim3(64), 0, st, br, d_sums, d_bad, d_bplans, d_probe, d_full);
            HIP_TRY(e, hipGetLastError(), "k_stereo");
        }
        HIP_TRY(e, hipMemcpyAsync(sums + r * nb * 12, d_sums, nb * 12 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st), "D2H sums");
        HIP_TRY(e, hipMemcpyAsync(badidx + r * nb * 2, d_bad, nb * 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, st), "D2H badidx");
        HIP_TRY(e, hipMemcpyAsync(acorr + r * nb * kSlotsPerBlock * 13, d_acorr, nb * kSlotsPerBlock * 13 * sizeof(int64_t), hipMemcpyDeviceToHost, st), "D2H acorr");
        HIP_TRY(e, hipMemcpyAsync(static_cast<BlockPlan*>(bplans) + r * nb, d_bplans, nb * sizeof(BlockPlan), hipMemcpyDeviceToHost, st), "D2H block plans");
        HIP_TRY(e, hipMemcpyAsync(need_probe + r * nb, d_probe, nb * sizeof(uint32_t), hipMemcpyDeviceToHost, st), "D2H need_probe");
        HIP_TRY(e, hipMemcpyAsync(need_full + r * nb, d_full, nb * sizeof(uint32_t), hipMemcpyDeviceToHost, st), "D2H need_full");
        HIP_TRY(e, hipMemcpyAsync(front_ctr + r * nb * 2, d_ctr, nb * 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, st), "D2H front counters");
    }
    HIP_TRY(e, hipStreamSynchronize(st), "k_ingest");
    return LACX_OK;
}

}  // extern "C"
