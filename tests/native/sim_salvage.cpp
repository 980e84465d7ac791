// tests/native/sim_salvage.cpp -- TEST INFRASTRUCTURE: the decoder's salvage job (decode through errors) on the host.
//
// What lacx_decoder_salvage_wav_batch_view / lacx_decoder_salvage_batch_device run on the device, one lane and one thread
// after the other: the job planned by plan_decode(..., salvage) and its tables filled by plan_fill_tables
// (csrc/decode_plan.h, the code api_decode.cpp runs), the lane code of csrc/decode_core.h over the PRESENT blocks, then the
// two passes in stream order -- ms_inverse_tile over every block as k_ms_inverse's grid runs it, and salvage_wav_unit /
// salvage_blank_tile of csrc/salvage_core.h as k_salvage_wav / k_salvage_blank run them -- and salvage_report for the
// results and fault lists.  Every buffer is a heap allocation of its own of exactly the capacity the plan states: payload =
// the present blocks' bytes + the tail pad, scratch PCM = the items' frames each rounded up to 4, image = need.image; the
// device form's caller arrays are one allocation per item and channel of exactly `frames` samples (a mono item has no
// right array at all), so that a build with AddressSanitizer reports any access outside them.  Status words, flags,
// scratch and images start as 0xCD: a missing block's status word, flag and scratch were written by nobody (zero_status:
// the status words start as 0 instead, the one stale value that sends k_ms_inverse over such a block's unwritten scratch).
// It is not part of the product and is not a fallback.
//
// Built twice by tests/salvagetwin.py: a plain -O2 shared library for ctypes, and (-DSIM_SALVAGE_MAIN) a sanitized program
// that runs a file of cases and prints one digest line per case.
#define SIM_JOB_SIMULATOR
#include "sim_job.h"

using namespace lacx;
using namespace simjob;

namespace {

constexpr int kFill = 0xCD;

struct Job {
    SalvageIn src;
    DecodePlan plan;
    std::vector<int> code;
    std::vector<std::string> err;
    std::unique_ptr<Run> run;
    uint32_t over = 0;
    Job(const uint8_t* const* lacs, const uint64_t* sizes, uint32_t n, bool device) : src(lacs, sizes, n, device) {}
};

// plans and runs; false where the plan refuses the job as a whole
bool run(uint32_t n, bool device, int cols, bool never_lean, bool zero_status, Job& j) {
    const BatchIn* in = j.src.in.data();
    if (plan_decode(in, n, device ? DecodeForm::device : DecodeForm::wav, kWholeStreams, false, j.plan, j.code, j.err, true)) return false;
    j.run.reset(new Run(j.plan, in, (uint32_t)kDecodeTailPad, kFill, zero_status ? 0 : kFill));
    place_payload(j.plan, in, j.run->payload.p);
    if (j.plan.items.empty()) return true;
    Lane ln(cols, never_lean);
    run_lanes(j.run->a, ln);
    j.over = ln.wave.over;
    run_ms_inverse(j.run->a);
    if (!j.run->a.present) return false;
    run_salvage_pass(j.run->a);
    return true;
}

}  // namespace

extern "C" {

// n streams as one salvage job: the WAV form (device = 0) or the device form.  cols: 1 or 64 columns of lane memory;
// zero_status: see above.
// Per input i, rec[8 * i ..] = refused (1: the container, then nothing else is set) or 0, blocks, bad_blocks, frames,
// lost_frames, first_bad, flags, and `at`: the WAV form's image offset in `image` (need.image bytes are copied there;
// the 44 header bytes of every image and the padding between images still hold 0xCD), or the device form's offset of
// the item's frames in left / right (the caller's arrays back to back; a mono item's right stays as the caller passed
// it).  codes: per accepted item in input order, one word per block (0 decoded, else the fault code).  msg: the refused
// items' messages, '\n' between inputs.  Returns need.image (WAV form) or the frames written (device form), -1 where
// the job cannot be planned or an output is too small.
int64_t sim_salvage(const uint8_t* const* lacs, const uint64_t* sizes, uint32_t n, int device, int cols, int never_lean, int zero_status, uint64_t* rec,
                    uint32_t* codes, uint64_t codes_cap, uint8_t* image, uint64_t image_cap, int32_t* left, int32_t* right,
                    uint64_t pcm_cap, char* msg, uint32_t msg_cap, uint32_t* over) {
    if (cols != 1 && cols != 64) return -1;
    Job j(lacs, sizes, n, device != 0);
    if (!run(n, device != 0, cols, never_lean != 0, zero_status != 0, j)) return -1;
    std::string all;
    for (uint32_t i = 0; i < n; ++i) {
        rec[8 * i] = j.code[i] != LACX_OK;
        all += (i ? "\n" : "") + j.err[i];
    }
    std::snprintf(msg, msg_cap, "%s", all.c_str());
    uint64_t ncodes = 0, written = 0;
    bool fits = true;
    salvage_records(j.plan, j.src.in.data(), j.run->st.p, device != 0,
                    [&](const PlanItem& p, const lacx_salvage_result& r, const std::vector<lacx_block_fault>& faults, const uint64_t* q) {
        if (ncodes + r.blocks > codes_cap || (device && q[6] + r.frames > pcm_cap)) return fits = false;
        std::memset(codes + ncodes, 0, 4ull * r.blocks);
        for (const lacx_block_fault& f : faults) codes[ncodes + f.block] = f.code;
        ncodes += r.blocks;
        std::memcpy(rec + 8 * p.src + 1, q, 7 * sizeof(uint64_t));
        if (device) {
            std::memcpy(left + q[6], j.src.in[p.src].left, 4 * r.frames);
            if (j.src.in[p.src].right) std::memcpy(right + q[6], j.src.in[p.src].right, 4 * r.frames);
            written = q[6] + r.frames;
        }
        return true;
    });
    if (!fits) return -1;
    *over = j.over;
    if (device) return (int64_t)written;
    if (j.plan.need.image > image_cap) return -1;
    std::memcpy(image, j.run->image.p, j.plan.need.image);
    return (int64_t)j.plan.need.image;
}

// A case (little-endian, written by tests/salvagetwin.py): u32 n, u32 flags (1 device form, 2 64 columns, 4 never_lean, 8 zero_status),
// then per stream u64 size and the bytes.  One line: "<index> <over> <item>;<item>;..." with item = "-" (refused) or
// "<hash of what the caller gets: the image's data region and pad, or left then right> <flags> <code,code,...>".
int sim_salvage_digest(const uint8_t* blob, uint64_t size, uint32_t index, char* line, uint32_t cap) {
    if (size < 8) return -1;
    uint32_t n, flags;
    std::memcpy(&n, blob, 4), std::memcpy(&flags, blob + 4, 4);
    std::vector<std::unique_ptr<Heap<uint8_t>>> own;  // every stream an exact allocation of its own: the lenient walk is checked with it
    std::vector<const uint8_t*> lacs(n);
    std::vector<uint64_t> sizes(n);
    uint64_t at = 8;
    for (uint32_t i = 0; i < n; ++i) {
        if (size - at < 8) return -1;
        std::memcpy(&sizes[i], blob + at, 8);
        at += 8;
        if (size - at < sizes[i]) return -1;
        own.emplace_back(new Heap<uint8_t>(sizes[i]));
        std::memcpy(own.back()->p, blob + at, sizes[i]);
        lacs[i] = own.back()->p;
        at += sizes[i];
    }
    const bool device = flags & 1u;
    Job j(lacs.data(), sizes.data(), n, device);
    if (!run(n, device, (flags & 2u) ? 64 : 1, (flags & 4u) != 0, (flags & 8u) != 0, j)) return -1;
    std::vector<std::string> item(n, "-");
    salvage_records(j.plan, j.src.in.data(), j.run->st.p, device,
                    [&](const PlanItem& p, const lacx_salvage_result& r, const std::vector<lacx_block_fault>& faults, const uint64_t*) {
        char hex[24];
        std::snprintf(hex, sizeof(hex), "%016llx", (unsigned long long)salvage_hash(p, j.src.in[p.src], j.run->image.p, device, r.frames));
        std::vector<uint32_t> codes(r.blocks, 0);
        for (const lacx_block_fault& f : faults) codes[f.block] = f.code;
        std::string s = std::string(hex) + " " + std::to_string(r.flags) + " ";
        for (uint32_t b = 0; b < r.blocks; ++b) s += (b ? "," : "") + std::to_string(codes[b]);
        item[p.src] = s;
        return true;
    });
    std::string out = std::to_string(index) + " " + std::to_string(j.over) + " ";
    for (uint32_t i = 0; i < n; ++i) out += (i ? ";" : "") + item[i];
    if (out.size() + 1 > cap) return -1;
    std::memcpy(line, out.c_str(), out.size() + 1);
    return 0;
}

#ifndef SIM_SALVAGE_MAIN
// The plan of a salvage job and its filled tables as flat arrays (the plain build only), against made-up base addresses:
// buffer k of {payload, left, right, image, caller's left, caller's right} at (k + 1) << 40, the caller's of input i a
// further i << 32 on.  head[24]: m, total_blocks, total_frames, total_pay, total_units, pcm_total, image_total, lanes,
// version-2 items, the offsets of items / byte_off / frame_off / unit_off / blk_item / lane_blk / v2_items / present, the
// tables' size, the capacities payload / blocks / pcm_frames / image / stage / tables, kDecodeTailPad; item[12 * j]: src,
// present_blocks, flags, pay_bytes, head, pcm_at, image_at, image_size, frames, blocks, block0, pay_off; rc[n] and the
// messages, '\n' between them.  Returns the tables' bytes, or -1 / -2 (why in msg).
int64_t sim_salvage_plan(const uint8_t* const* lacs, const uint64_t* sizes, uint32_t n, int device, uint64_t* head, uint64_t* item,
                         int32_t* rc, char* msg, uint32_t msg_cap, uint8_t* tables, uint64_t tables_cap) {
    auto base = [](uint64_t k, uint64_t i) { return (uintptr_t)(((k + 1) << 40) + (i << 32)); };
    std::vector<BatchIn> in(n);
    for (uint32_t i = 0; i < n; ++i) {
        lacx_stream_info info{};
        uint32_t present = 0, flags = 0;
        const char* why = nullptr;
        (void)scan_stream(lacs[i], sizes[i], &info, &present, &flags, &why);
        in[i] = BatchIn{lacs[i], sizes[i], device ? (int32_t*)base(4, i) : nullptr, device ? (int32_t*)base(5, i) : nullptr, device ? info.frames : 0};
    }
    DecodePlan plan;
    std::vector<int> code;
    std::vector<std::string> err;
    std::string all;
    if (const char* whole = plan_decode(in.data(), n, device ? DecodeForm::device : DecodeForm::wav, kWholeStreams, false, plan, code, err, true)) {
        std::snprintf(msg, msg_cap, "%s", whole);
        return -1;
    }
    for (uint32_t i = 0; i < n; ++i) rc[i] = code[i], all += (i ? "\n" : "") + err[i];
    std::snprintf(msg, msg_cap, "%s", all.c_str());
    if (plan.need.tables > tables_cap) return -2;
    const TableLayout& at = plan.at;
    const uint64_t h[24] = {plan.items.size(), plan.total_blocks, plan.total_frames, plan.total_pay, plan.total_units, plan.pcm_total,
                            plan.image_total, plan.lane_blk.size(), plan.v2_items.size(), at.items, at.byte_off, at.frame_off, at.unit_off,
                            at.blk_item, at.lane_blk, at.v2_items, at.win, at.size, plan.need.payload, plan.need.blocks, plan.need.pcm_frames,
                            plan.need.image, plan.need.stage, kDecodeTailPad};
    std::memcpy(head, h, sizeof(h));
    for (size_t j = 0; j < plan.items.size(); ++j) {
        const PlanItem& p = plan.items[j];
        const uint64_t q[12] = {p.src, p.present_blocks, p.scan_flags, p.pay_bytes, p.head, p.pcm_at, p.image_at, p.image_size, p.item.frames,
                                p.item.blocks, p.item.block0, p.item.pay_off};
        std::memcpy(item + 12 * j, q, sizeof(q));
    }
    plan_fill_tables(plan, in.data(), PlanBases{(uint8_t*)base(0, 0), (int32_t*)base(1, 0), (int32_t*)base(2, 0), (uint8_t*)base(3, 0)}, tables);
    return (int64_t)plan.need.tables;
}
#endif

}  // extern "C"

#ifdef SIM_SALVAGE_MAIN
// sim_salvage_san CASES: every case of the file (per case: a 32-bit little-endian size, then the bytes, see
// sim_salvage_digest), one line each on stdout, "done <count>" at the end.
int main(int argc, char** argv) {
    if (argc != 2) return 2;
    std::vector<char> line(1 << 22);
    return for_each_case(argv[1], [&](const uint8_t* blob, uint32_t size, uint32_t i) {
        return !sim_salvage_digest(blob, size, i, line.data(), (uint32_t)line.size()) && std::puts(line.data()) >= 0;
    });
}
#endif
