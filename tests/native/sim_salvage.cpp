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
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "decode_core.h"
#include "decode_plan.h"
#include "salvage_core.h"

using namespace lacx;

namespace {

template <typename T>
struct Heap {  // exactly n elements, nothing behind them
    T* p;
    explicit Heap(size_t n, int fill = 0) : p(static_cast<T*>(std::malloc(n ? n * sizeof(T) : 1))) {
        if (n) std::memset(p, fill, n * sizeof(T));
    }
    ~Heap() { std::free(p); }
    Heap(const Heap&) = delete;
    Heap& operator=(const Heap&) = delete;
};

constexpr int kFill = 0xCD;

uint64_t fnv(const void* data, uint64_t bytes, uint64_t h) {
    const uint8_t* p = static_cast<const uint8_t*>(data);
    for (uint64_t i = 0; i < bytes; ++i) {
        h ^= p[i];
        h *= 0x100000001B3ull;
    }
    return h;
}

struct Job {
    std::vector<BatchIn> in;
    std::vector<std::unique_ptr<Heap<int32_t>>> own;  // device form: the caller's arrays
    DecodePlan plan;
    std::vector<int> code;
    std::vector<std::string> err;
    std::unique_ptr<Heap<uint8_t>> payload, tables, flag, image;
    std::unique_ptr<Heap<int32_t>> L, R;
    std::unique_ptr<Heap<uint32_t>> st;
    DecodeArgs a;
    uint32_t over = 0;
};

// plans and runs; false where the plan refuses the job as a whole
bool run(const uint8_t* const* lacs, const uint64_t* sizes, uint32_t n, bool device, int cols, bool never_lean, bool zero_status, Job& j) {
    j.in.resize(n);
    for (uint32_t i = 0; i < n; ++i) {
        lacx_stream_info info{};
        uint32_t present = 0, flags = 0;
        const char* why = nullptr;
        int32_t *l = nullptr, *r = nullptr;
        uint64_t frames = 0;
        if (device && scan_stream(lacs[i], sizes[i], &info, &present, &flags, &why) == LACX_OK) {
            frames = info.frames;  // what lacx_stream_scan tells the caller to allocate
            j.own.emplace_back(new Heap<int32_t>(frames, 0x5A));
            l = j.own.back()->p;
            if (info.channels == 2) {
                j.own.emplace_back(new Heap<int32_t>(frames, 0x5A));
                r = j.own.back()->p;
            }
        }
        j.in[i] = BatchIn{lacs[i], sizes[i], l, r, frames};
    }
    if (plan_decode(j.in.data(), n, device ? DecodeForm::device : DecodeForm::wav, kWholeStreams, false, j.plan, j.code, j.err, true)) return false;
    const DecodePlan& p = j.plan;
    j.payload.reset(new Heap<uint8_t>(p.need.payload));  // zeroed: the tail pad
    j.tables.reset(new Heap<uint8_t>(p.need.tables));
    j.flag.reset(new Heap<uint8_t>(p.need.blocks, kFill));
    j.image.reset(new Heap<uint8_t>(p.need.image, kFill));
    j.L.reset(new Heap<int32_t>(p.need.pcm_frames, kFill));
    j.R.reset(new Heap<int32_t>(p.need.pcm_frames, kFill));
    j.st.reset(new Heap<uint32_t>(p.need.blocks, zero_status ? 0 : kFill));
    plan_fill_tables(p, j.in.data(), PlanBases{j.payload->p, j.L->p, j.R->p, j.image->p}, j.tables->p);
    const DecodeArgs a = j.a = plan_args(p, j.tables->p, j.payload->p, j.st->p, j.flag->p);
    for (const PlanItem& it : p.items) std::memcpy(j.payload->p + it.item.pay_off, j.in[it.src].lac + it.head + it.pay_src, it.pay_bytes);
    if (p.items.empty()) return true;

    Heap<unsigned char> raw(kDecBytesPerCol * (size_t)cols, 0xA5);
    DecMem dm = dec_mem(raw.p, (uint32_t)cols);
    DecWave wave;
    wave.never_lean = never_lean;
    for (uint32_t g = 0; g < a.lanes; ++g) {  // k_decode
        const uint32_t blk = a.lane_blk[g];
        if (blk == ~0u) continue;
        const DecodeItem& it = a.items[a.blk_item[blk]];
        decode_block_lane(blk, it.channels, it.stereo_mode, a.payload, a.byte_off, a.frame_off, it.frame0, it.left, it.right, a.status,
                          a.ms_flag, dm, cols - 1, wave);
    }
    for (uint32_t g = 0; g < a.nv2; ++g) {  // k_decode_serial
        const DecodeItem& it = a.items[a.v2_items[g]];
        decode_serial_lane(it.blocks, it.channels, it.stereo_mode, a.payload + it.pay_off, it.pay_bits, a.frame_off + it.block0, it.frame0,
                           it.left, it.right, a.status + it.block0, a.ms_flag + it.block0, dm, cols - 1, wave);
    }
    j.over = wave.over;
    for (uint32_t blk = 0; blk < a.total_blocks; ++blk) {  // k_ms_inverse: grid (blocks, 16 tiles) x 256 threads
        if (a.status[blk]) continue;
        const DecodeItem& it = a.items[a.blk_item[blk]];
        const unsigned long long f0 = a.frame_off[blk];
        const uint32_t nfr = (uint32_t)(a.frame_off[blk + 1] - f0);
        for (uint32_t tile = 0; tile < (uint32_t)kMaxBlock / 1024u; ++tile)
            for (uint32_t tid = 0; tid < 256u; ++tid)
                ms_inverse_tile(blk, tile, it.channels, it.bit_depth, f0 - it.frame0, nfr, it.left, it.right, a.ms_flag, a.status, tid);
    }
    if (!a.present) return false;
    if (a.wav) {  // k_salvage_wav: thread u of the concatenated unit ranges
        uint32_t item = 0;
        for (unsigned long long u = 0; u < a.total_units; ++u) {
            while (a.unit_off[item + 1] <= u) ++item;
            const DecodeItem& it = a.items[item];
            salvage_wav_unit(4ull * (u - a.unit_off[item]), it.blocks, a.present[item], it.channels, it.bit_depth, it.frames,
                             a.frame_off + it.block0, it.frame0, it.left, it.right, a.status + it.block0, it.wav);
        }
    } else {  // k_salvage_blank: grid (blocks, 16 tiles) x 256 threads
        for (uint32_t blk = 0; blk < a.total_blocks; ++blk) {
            const uint32_t item = a.blk_item[blk];
            const DecodeItem& it = a.items[item];
            if (!salvage_lost(a.status + it.block0, blk - it.block0, a.present[item])) continue;
            const unsigned long long f0 = a.frame_off[blk];
            const uint32_t nfr = (uint32_t)(a.frame_off[blk + 1] - f0);
            for (uint32_t tile = 0; tile < (uint32_t)kMaxBlock / 1024u; ++tile)
                for (uint32_t tid = 0; tid < 256u; ++tid)
                    salvage_blank_tile(tile, f0 - it.frame0, nfr, it.left, it.channels == 2 ? it.right : nullptr, tid);
        }
    }
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
    Job j;
    if (!run(lacs, sizes, n, device != 0, cols, never_lean != 0, zero_status != 0, j)) return -1;
    std::string all;
    for (uint32_t i = 0; i < n; ++i) {
        rec[8 * i] = j.code[i] != LACX_OK;
        all += (i ? "\n" : "") + j.err[i];
    }
    std::snprintf(msg, msg_cap, "%s", all.c_str());
    uint64_t ncodes = 0, at = 0;
    for (const PlanItem& p : j.plan.items) {
        std::vector<lacx_block_fault> faults;
        const lacx_salvage_result r = salvage_report(p, j.in[p.src].lac, j.st->p, faults);
        if (ncodes + r.blocks > codes_cap) return -1;
        std::memset(codes + ncodes, 0, 4ull * r.blocks);
        for (const lacx_block_fault& f : faults) codes[ncodes + f.block] = f.code;
        ncodes += r.blocks;
        const uint64_t q[7] = {r.blocks, r.bad_blocks, r.frames, r.lost_frames, r.first_bad, r.flags, device ? at : p.image_at};
        std::memcpy(rec + 8 * p.src + 1, q, sizeof(q));
        if (device) {
            if (at + r.frames > pcm_cap) return -1;
            std::memcpy(left + at, j.in[p.src].left, 4 * r.frames);
            if (j.in[p.src].right) std::memcpy(right + at, j.in[p.src].right, 4 * r.frames);
            at += r.frames;
        }
    }
    *over = j.over;
    if (device) return (int64_t)at;
    if (j.plan.need.image > image_cap) return -1;
    std::memcpy(image, j.image->p, j.plan.need.image);
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
    Job j;
    const bool device = flags & 1u;
    if (!run(lacs.data(), sizes.data(), n, device, (flags & 2u) ? 64 : 1, (flags & 4u) != 0, (flags & 8u) != 0, j)) return -1;
    std::vector<std::string> item(n, "-");
    for (const PlanItem& p : j.plan.items) {
        std::vector<lacx_block_fault> faults;
        const lacx_salvage_result r = salvage_report(p, j.in[p.src].lac, j.st->p, faults);
        uint64_t h = 0xCBF29CE484222325ull;
        if (device) {
            h = fnv(j.in[p.src].left, 4 * r.frames, h);
            if (j.in[p.src].right) h = fnv(j.in[p.src].right, 4 * r.frames, h);
        } else {
            h = fnv(j.image->p + p.image_at + 44, p.image_size - 44, h);
        }
        char hex[24];
        std::snprintf(hex, sizeof(hex), "%016llx", (unsigned long long)h);
        std::vector<uint32_t> codes(r.blocks, 0);
        for (const lacx_block_fault& f : faults) codes[f.block] = f.code;
        std::string s = std::string(hex) + " " + std::to_string(r.flags) + " ";
        for (uint32_t b = 0; b < r.blocks; ++b) s += (b ? "," : "") + std::to_string(codes[b]);
        item[p.src] = s;
    }
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
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<char> line(1 << 22);
    unsigned long done = 0;
    for (uint8_t sz[4]; std::fread(sz, 1, 4, f) == 4; ++done) {
        const uint32_t size = sz[0] | (sz[1] << 8) | (sz[2] << 16) | ((uint32_t)sz[3] << 24);
        Heap<uint8_t> blob(size);
        if (std::fread(blob.p, 1, size, f) != size) return 3;
        if (sim_salvage_digest(blob.p, size, (uint32_t)done, line.data(), (uint32_t)line.size())) return 4;
        std::puts(line.data());
    }
    std::fclose(f);
    std::printf("done %lu\n", done);
    return 0;
}
#endif
