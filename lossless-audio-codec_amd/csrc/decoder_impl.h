// decoder_impl.h -- the decoder object behind lacx_decoder*, shared by the translation units of its entry points
// (api_decode.cpp: decode, verify, digest, salvage, manifests; api_recovery.cpp: recovery data; api_transcode.cpp).
#pragma once
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "accuraterip_plan.h"
#include "compare_plan.h"
#include "device_buf.h"
#include "lacx.h"

// The decoder object: device buffers, a stream and two events that live from call to call (grow-only), so that a decode
// costs its copies and its kernel, not six allocations (ref LAC::Decoder is an object too, src/codec/lac/decoder.hpp:10-24).
struct lacx_decoder {
    int device = -1;  // -1: whatever device is current at the first call
    bool ready = false;
    hipStream_t stream = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    lacx::Buf pay{{{false, 1, "hipMalloc(payload)"}}};             // (recovery data: the arena of a job)
    lacx::Buf stage{{{true, 1, "hipHostMalloc(payload stage)"}}};  // the window form's payload ranges, gathered for one H2D copy
                                                                    // (recovery data: the sidecars or files a call hands out)
    lacx::Buf pcm{{{false, 4, "hipMalloc(left)"}, {false, 4, "hipMalloc(right)"}}};  // both channels, whatever the streams' count
    lacx::Buf blocks{{{false, 4, "hipMalloc(status)"}, {false, 1, "hipMalloc(flags)"}, {true, 4, "hipHostMalloc(status)"}}};
    lacx::Buf image{{{false, 1, "hipMalloc(wav)"}, {true, 1, "hipHostMalloc(wav)"}}};  // WAV images (header + data + pad), host windows
    lacx::Buf tables{{{false, 1, "hipMalloc(batch tables)"}, {true, 1, "hipHostMalloc(batch tables)"}}};  // one upload (TableLayout)
    // a transcode job (api_transcode.cpp, edit_plan.h): the planar int32 staging the window job splices the segments into;
    // the destination k_edit writes and the encoder, the digest and the verification read; k_edit's tables
    lacx::Buf edit_stage{{{false, 4, "hipMalloc(edit staging)"}}};
    lacx::Buf edit_dst{{{false, 1, "hipMalloc(edit destination)"}}};
    lacx::Buf edit_tab{{{false, 1, "hipMalloc(edit tables)"}, {true, 1, "hipHostMalloc(edit tables)"}}};
    lacx::Buf runs_list{{{false, 16, "hipMalloc(run lists)"}}};  // a runs job's interior runs (lacx_run), runs_plan.h
    lacx::Buf loud{{{false, 16, "hipMalloc(loudness scratch)"}}};  // a loudness job's states, partial sums and rows, loudness_plan.h
    uint64_t runs_list_cap = 0;  // R of a runs job (0: kRunsListCap); LACX_RUNS_LIST_CAP at creation, tests force the second run with it
    uint8_t* d_pay() const { return static_cast<uint8_t*>(pay.part[0].p); }
    uint8_t* h_pay() const { return static_cast<uint8_t*>(stage.part[0].p); }
    int32_t* d_left() const { return static_cast<int32_t*>(pcm.part[0].p); }
    int32_t* d_right() const { return static_cast<int32_t*>(pcm.part[1].p); }
    uint32_t* d_status() const { return static_cast<uint32_t*>(blocks.part[0].p); }
    uint8_t* d_ms() const { return static_cast<uint8_t*>(blocks.part[1].p); }
    uint32_t* h_status() const { return static_cast<uint32_t*>(blocks.part[2].p); }
    uint8_t* d_wav() const { return static_cast<uint8_t*>(image.part[0].p); }
    uint8_t* h_wav() const { return static_cast<uint8_t*>(image.part[1].p); }  // behind lacx_decoder_decode_wav_view
    uint8_t* d_meta() const { return static_cast<uint8_t*>(tables.part[0].p); }
    uint8_t* h_meta() const { return static_cast<uint8_t*>(tables.part[1].p); }
    std::vector<std::string> item_err;  // the last batch call's message per item ("" = decoded)
    std::vector<std::vector<lacx_block_fault>> item_faults;  // the last salvage call's lost blocks per item
    std::vector<std::vector<lacx_block_digest>> item_rows;   // the last block digest call's rows per item
    std::vector<std::vector<lacx_block_stats>> item_stats;   // the last stats call's rows per item
    std::vector<lacx_run> runs_host;                             // ... as the device left them (k_runs's list buffer)
    std::vector<std::vector<std::vector<lacx_run>>> item_runs;  // the last runs call's lists per item and detector
    std::vector<lacx_loudness_row> loud_host;                    // the last loudness call's rows as the device left them
    std::vector<std::vector<lacx_loudness_row>> item_loud;       // ... per item
    std::vector<std::vector<lacx_truepeak_row>> item_peak;       // the last true-peak call's rows per item
    std::vector<std::vector<lacx_spectrum_row>> item_spec;       // the last spectrum call's rows per item
    // the last rip-checksum call: the plan's discs and tracks, the sums as the device left them, per disc whether it has any,
    // and its tracks as the ABI gives them
    lacx::ArLayout ar_at;
    std::vector<uint32_t> ar_sums;
    std::vector<uint8_t> ar_ok;
    std::vector<uint32_t> ar_slot;  // ... and its place among ar_at's discs
    std::vector<std::vector<lacx_ar_track>> ar_tracks;
    // the last compare call: the plan's pairs with their chosen offsets, the counts and the rows as the device left them, per
    // pair of the call whether it has an answer and its place among cmp_at's pairs
    lacx::CmpLayout cmp_at;
    std::vector<uint64_t> cmp_counts;
    std::vector<lacx_compare_row> cmp_rows;
    std::vector<uint8_t> cmp_ok;
    std::vector<uint32_t> cmp_slot;
    std::vector<std::vector<lacx_block_info>> item_info;     // the last inspection call's rows per item
    // ... and, where it asked for partition detail, the entries of all its blocks: [T][2][256] each, item i's blocks
    // from info_block0[i] on (~0u: the item has none)
    std::vector<uint8_t> info_mode_k;
    std::vector<uint32_t> info_part_bits;
    std::vector<uint32_t> info_block0;
    uint64_t info_guard = 0, info_guard_changed = 0;         // LACX_INSPECT_GUARD: the guard bytes behind its tables, and those the job changed
    std::vector<std::vector<uint32_t>> item_bad;             // the last recovery scan / repair call's damaged slices per item
    std::string err;
    // held by a transcode job for the whole call (the encoder has one too): its phases are calls of their own on this handle
    std::shared_ptr<std::mutex> call_mu = std::make_shared<std::mutex>();
};

namespace lacx_host {
// keeps msg for lacx_decode_last_error (per thread) and returns code
int decode_fail(int code, const std::string& msg);
// makes the decoder's device current, creating its stream and events at the first call; *prev_device: to put back, or -1
lacx::DevErr decoder_open(lacx_decoder* d, int* prev_device);
}  // namespace lacx_host
