// tests/native/sim_decode.cpp -- TEST INFRASTRUCTURE: the decoder's lane code (csrc/decode_core.h) on the host.
//
// One "lane" per block of a version-3 stream (or one lane for a version-2 stream), then the mid/side pass over every
// block that decoded -- the work of k_decode / k_decode_serial / k_ms_inverse, one lane after the other.  What the lanes
// get is what the product gives them: the job is planned by plan_decode and its tables are filled by plan_fill_tables
// (csrc/decode_plan.h, the code api_decode.cpp runs), and every buffer is a heap allocation of its own of exactly the
// capacity the plan states, not the growth slack, so that a build with AddressSanitizer reports any access the bounds
// argument at BitIn does not cover:  payload = the items' bytes + the tail pad (zeroed), left / right = the items' frames,
// each rounded up to 4, lane memory = kDecBytesPerCol * cols.  It is not part of the product and is not a fallback.
//
// Built twice by tests/dectwin.py: a plain -O2 shared library for ctypes, and (-DSIM_DECODE_MAIN) a sanitized program that
// walks a corpus file through every switch setting and prints one digest line per stream, or a file of batch cases.
#define SIM_JOB_SIMULATOR
#include "sim_job.h"

using namespace lacx;
using namespace simjob;

namespace {

// a permutation of 0..n-1 from a seed (the order in which the gathered layout places the blocks)
void shuffle(std::vector<uint32_t>& v, uint32_t seed) {
    uint64_t s = 0x9E3779B97F4A7C15ull * (seed + 1u);
    for (size_t i = v.size(); i > 1; --i) {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        std::swap(v[i - 1], v[(size_t)((s >> 33) % i)]);
    }
}

constexpr uint32_t kSimDefaultPad = ~0u;

// a whole stream into host arrays, as a batch of one; false where the plan refuses it
bool plan_one(const uint8_t* lac, uint64_t size, int32_t* left, int32_t* right, BatchIn& in, DecodePlan& plan) {
    lacx_stream_info info;
    const char* why = nullptr;
    if (parse_stream(lac, size, &info, &why) != LACX_OK) return false;
    in = BatchIn{lac, size, left, right, info.frames};
    std::vector<int> code;
    std::vector<std::string> err;
    return !plan_decode(&in, 1, DecodeForm::host, kWholeStreams, false, plan, code, err) && code[0] == LACX_OK;
}

}  // namespace

// the bounds argument at BitIn: the derived worst overshoot of a trip must fit the pad the product appends
static_assert(kDecodeTailPad >= 25, "kDecodeTailPad is below the overshoot the comment at BitIn derives");

extern "C" {

uint32_t sim_tail_pad(void) { return (uint32_t)kDecodeTailPad; }

// FNV-1a over n samples, chained through `h` (start with 0): how the two builds' PCM is compared without moving it
uint64_t sim_hash(const int32_t* x, uint64_t n, uint64_t h) {
    if (h == 0) h = 0xCBF29CE484222325ull;
    for (uint64_t i = 0; i < n; ++i) {
        h ^= (uint32_t)x[i];
        h *= 0x100000001B3ull;
    }
    return h;
}

// A whole .lac that lacx_stream_parse accepts.  never_lean: the wave policy (DecWave); cols: 1 or 64 columns of lane
// memory, the lane being the last column; gather_seed: 0 = the payload where the plan puts it, else the blocks'
// payloads back to back in a shuffled order (what gather_ranges makes of a window batch: a block's successor in memory
// is not its successor in the stream), the one placement that is the twin's own; pad: the zero bytes behind the payload
// -- kSimDefaultPad (~0) = kDecodeTailPad, what the device path appends; any other value only to show that a shorter pad
// is reported.
// Out: status[blocks], ms[blocks], left[frames], right[frames] (stereo), *over = the furthest byte a load reached past
// the end of the block it was reading.  Returns 0, or -1 for a stream the plan cannot take.
int sim_decode(const uint8_t* lac, uint64_t size, int never_lean, int cols, uint32_t gather_seed, uint32_t pad,
               uint32_t* status, uint8_t* ms, int32_t* left, int32_t* right, uint32_t* over) {
    if (cols != 1 && cols != 64) return -1;
    if (pad == kSimDefaultPad) pad = (uint32_t)kDecodeTailPad;
    BatchIn in{};
    DecodePlan plan;
    if (!plan_one(lac, size, left, right, in, plan)) return -1;
    Run run(plan, &in, pad);
    Lane ln(cols, never_lean);
    const DecodeArgs& a = run.a;
    const DecodeItem& it = a.items[0];
    if (it.version == 3 && gather_seed) {
        std::vector<uint32_t> order(it.blocks);
        for (uint32_t b = 0; b < it.blocks; ++b) order[b] = b;
        shuffle(order, gather_seed);
        unsigned long long cur = 0;
        std::vector<unsigned long long> at(it.blocks);
        for (uint32_t b : order) {
            const unsigned long long bytes = a.byte_off[b + 1] - a.byte_off[b];
            at[b] = cur;
            std::memcpy(run.payload.p + cur, lac + plan.items[0].head + a.byte_off[b], bytes);
            cur += bytes;
        }
        for (uint32_t b = 0; b < it.blocks; ++b) {  // the block's own two-entry tables: its place in the buffer, its frames
            const unsigned long long bo[2] = {at[b], at[b] + (a.byte_off[b + 1] - a.byte_off[b])};
            const unsigned long long fo[2] = {a.frame_off[b], a.frame_off[b + 1]};
            decode_block_lane(0, it.channels, it.stereo_mode, a.payload, bo, fo, 0, it.left, it.right, a.status + b, a.ms_flag + b, ln.dm,
                              ln.lane, ln.wave);
        }
    } else {
        place_payload(plan, &in, run.payload.p);
        run_lanes(a, ln);
    }
    run_ms_inverse(a);
    std::memcpy(status, a.status, it.blocks * sizeof(uint32_t));
    std::memcpy(ms, a.ms_flag, it.blocks);
    std::memcpy(left, it.left, it.frames * sizeof(int32_t));
    if (it.channels == 2) std::memcpy(right, it.right, it.frames * sizeof(int32_t));
    *over = ln.wave.over;
    return 0;
}

// n streams as one job, planned as the product plans them: whole streams (start == null) or the windows
// [start[i], start[i] + frames[i]), host form; pad_waves: LACX_DECODE_BATCH_PAD.  The payload is laid out by the plan's
// pay_off / pay_src / pay_bytes.  The device-only post passes (wav_pack_unit, window_out_unit) are not run: what comes
// back is the scratch PCM of the blocks every item covers and, per input i, rec[8 * i ..] = the plan's refusal (1) or 0,
// pcm_at, decoded frames, WindowOut.start, WindowOut.frames, blk_first, blocks, block0.
// Out: status / ms [the streams' blocks, at most], left / right [the streams' frames, each rounded up to 4, at most].
int sim_decode_batch(const uint8_t* const* lacs, const uint64_t* sizes, uint32_t n, const uint64_t* start, const uint64_t* frames,
                     int pad_waves, int never_lean, int cols, uint64_t* rec, uint32_t* status, uint8_t* ms, int32_t* left,
                     int32_t* right, uint32_t* over) {
    if (cols != 1 && cols != 64) return -1;
    std::vector<BatchIn> in(n);
    for (uint32_t i = 0; i < n; ++i) {
        lacx_stream_info info{};
        const char* why = nullptr;
        (void)parse_stream(lacs[i], sizes[i], &info, &why);  // (a whole stream's arrays must match its frames; the plan parses again)
        in[i] = BatchIn{lacs[i], sizes[i], left, right, start ? frames[i] : info.frames, start ? start[i] : 0};
    }
    DecodePlan plan;
    std::vector<int> code;
    std::vector<std::string> err;
    if (plan_decode(in.data(), n, DecodeForm::host, start ? LACX_SAMPLE_I32 : kWholeStreams, pad_waves != 0, plan, code, err)) return -1;
    for (uint32_t i = 0; i < n; ++i) rec[8 * i] = code[i] != LACX_OK;
    Run run(plan, in.data(), (uint32_t)kDecodeTailPad);
    Lane ln(cols, never_lean);
    place_payload(plan, in.data(), run.payload.p);
    run_lanes(run.a, ln);
    run_ms_inverse(run.a);
    for (const PlanItem& p : plan.items) {
        const uint64_t r[7] = {p.pcm_at, p.item.frames, p.win.start, p.win.frames, p.blk_first, p.item.blocks, p.item.block0};
        std::memcpy(rec + 8 * p.src + 1, r, sizeof(r));
    }
    std::memcpy(status, run.st.p, plan.need.blocks * sizeof(uint32_t));
    std::memcpy(ms, run.flag.p, plan.need.blocks);
    std::memcpy(left, run.L.p, plan.need.pcm_frames * sizeof(int32_t));
    std::memcpy(right, run.R.p, plan.need.pcm_frames * sizeof(int32_t));
    *over = ln.wave.over;
    return 0;
}

// A batch case (little-endian, written by tests/dectwin.py): u32 n, u32 flags (1 pad_waves, 2 windows, 4 never_lean,
// 8 64 columns), then per stream u64 start, u64 frames, u64 size and the bytes.  One line:
//   "<index> <over> <item>;<item>;..."  item = "-" (refused) or "<hash of its decoded left, right> <status,status,...>"
int sim_batch_digest(const uint8_t* blob, uint64_t size, uint32_t index, char* line, uint32_t cap) {
    if (size < 8) return -1;
    uint32_t n, flags;
    std::memcpy(&n, blob, 4), std::memcpy(&flags, blob + 4, 4);
    std::vector<const uint8_t*> lacs(n);
    std::vector<uint64_t> start(n), frames(n), sizes(n);
    std::vector<Heap<uint8_t>*> own;  // every stream an exact allocation of its own: the plan's reads are checked with it
    uint64_t at = 8, blocks = 0, pcm = 0;
    for (uint32_t i = 0; i < n; ++i) {
        if (size - at < 24) return -1;
        std::memcpy(&start[i], blob + at, 8), std::memcpy(&frames[i], blob + at + 8, 8), std::memcpy(&sizes[i], blob + at + 16, 8);
        at += 24;
        if (size - at < sizes[i]) return -1;
        own.push_back(new Heap<uint8_t>(sizes[i]));
        std::memcpy(own.back()->p, blob + at, sizes[i]);
        lacs[i] = own.back()->p;
        at += sizes[i];
        lacx_stream_info info{};
        const char* why = nullptr;
        if (parse_stream(lacs[i], sizes[i], &info, &why) == LACX_OK) blocks += info.blocks, pcm += (info.frames + 3) & ~3ull;
    }
    std::vector<uint64_t> rec(8 * (size_t)n);
    std::vector<uint32_t> st(blocks + 1);
    std::vector<uint8_t> ms(blocks + 1);
    std::vector<int32_t> l(pcm + 1), r(pcm + 1);
    uint32_t over = 0;
    const bool win = flags & 2u;
    const int rc = sim_decode_batch(lacs.data(), sizes.data(), n, win ? start.data() : nullptr, win ? frames.data() : nullptr, flags & 1u,
                                    (flags >> 2) & 1u, (flags & 8u) ? 64 : 1, rec.data(), st.data(), ms.data(), l.data(), r.data(), &over);
    for (auto* h : own) delete h;
    if (rc) return -1;
    std::string out = std::to_string(index) + " " + std::to_string(over) + " ";
    for (uint32_t i = 0; i < n; ++i) {
        const uint64_t* q = &rec[8 * (size_t)i];
        if (i) out += ";";
        if (q[0]) {
            out += "-";
            continue;
        }
        char hex[24];
        std::snprintf(hex, sizeof(hex), "%016llx", (unsigned long long)sim_hash(&r[q[1]], q[2], sim_hash(&l[q[1]], q[2], 0)));
        out += hex;
        for (uint64_t b = 0; b < q[6]; ++b) out += (b ? "," : " ") + std::to_string(st[q[7] + b]);
    }
    if (out.size() + 1 > cap) return -1;
    std::memcpy(line, out.c_str(), out.size() + 1);
    return 0;
}

#ifndef SIM_DECODE_MAIN
// A plan and its filled tables as flat arrays (the plain build only): the same job description as sim_decode_batch, in any
// form (DecodeForm's number; sample_type -1 = whole streams), against made-up base addresses -- buffer k of {payload,
// left, right, image, caller's left, caller's right, source 0, source 1} at (k + 1) << 40, the caller's and the sources'
// of input i a further i << 32 on.  host_src_bytes != 0 (verify form, n = 1): the source is a WAV data chunk in host memory.
// head[32]: m, the totals, src_at, host_src_bytes, lanes, version-2 items, the layout, the capacities, the record sizes;
// item[12 * j]: src, blk_first, pay_src, pay_bytes, head, pcm_at, image_at, image_size, decoded frames, window start,
// window frames, blocks; rc[n] and the messages, '\n' between them.  Returns the tables' bytes, or -1 / -2 (why in msg).
int64_t sim_plan_dump(const uint8_t* const* lacs, const uint64_t* sizes, uint32_t n, const uint64_t* start, const uint64_t* frames,
                      int form, int sample_type, int pad_waves, uint64_t host_src_bytes, uint64_t* head, uint64_t* item, int32_t* rc,
                      char* msg, uint32_t msg_cap, uint8_t* tables, uint64_t tables_cap) {
    auto base = [](uint64_t k, uint64_t i) { return (uintptr_t)(((k + 1) << 40) + (i << 32)); };
    std::vector<BatchIn> in(n);
    for (uint32_t i = 0; i < n; ++i) {
        lacx_stream_info info{};
        const char* why = nullptr;
        (void)parse_stream(lacs[i], sizes[i], &info, &why);
        in[i] = BatchIn{lacs[i], sizes[i], (int32_t*)base(4, i), (int32_t*)base(5, i), start ? frames[i] : info.frames, start ? start[i] : 0};
        if (host_src_bytes) {
            in[i].pcm = lacx_pcm{nullptr, nullptr, info.bit_depth == 16 ? LACX_PCM_INTERLEAVED_I16 : LACX_PCM_INTERLEAVED_I24, info.channels};
            in[i].host_src = (const uint8_t*)base(6, i);
            in[i].host_src_bytes = host_src_bytes;
        } else {
            in[i].pcm = lacx_pcm{(const void*)base(6, i), (const void*)base(7, i), LACX_PCM_PLANAR_I32, info.channels};
        }
    }
    DecodePlan plan;
    std::vector<int> code;
    std::vector<std::string> err;
    std::string all;
    if (const char* whole = plan_decode(in.data(), n, (DecodeForm)form, sample_type, pad_waves != 0, plan, code, err)) {
        std::snprintf(msg, msg_cap, "%s", whole);
        return -1;
    }
    for (uint32_t i = 0; i < n; ++i) rc[i] = code[i], all += (i ? "\n" : "") + err[i];
    std::snprintf(msg, msg_cap, "%s", all.c_str());
    if (plan.need.tables > tables_cap) return -2;
    const TableLayout& at = plan.at;
    const uint64_t h[32] = {plan.items.size(), plan.total_blocks, plan.total_frames, plan.total_pay, plan.total_units, plan.pcm_total,
                            plan.image_total, plan.src_at, plan.host_src_bytes, plan.lane_blk.size(), plan.v2_items.size(), at.items,
                            at.byte_off, at.frame_off, at.unit_off, at.blk_item, at.lane_blk, at.v2_items, at.win, at.res, at.size,
                            plan.need.payload, plan.need.blocks, plan.need.pcm_frames, plan.need.image, plan.need.stage, plan.need.tables,
                            sizeof(DecodeItem), sizeof(WindowOut), sizeof(VerifySource), sizeof(VerifyWords), kDecodeTailPad};
    std::memcpy(head, h, sizeof(h));
    for (size_t j = 0; j < plan.items.size(); ++j) {
        const PlanItem& p = plan.items[j];
        const uint64_t q[12] = {p.src, p.blk_first, p.pay_src, p.pay_bytes, p.head, p.pcm_at, p.image_at, p.image_size, p.item.frames,
                                p.win.start, p.win.frames, p.item.blocks};
        std::memcpy(item + 12 * j, q, sizeof(q));
    }
    plan_fill_tables(plan, in.data(), PlanBases{(uint8_t*)base(0, 0), (int32_t*)base(1, 0), (int32_t*)base(2, 0), (uint8_t*)base(3, 0)}, tables);
    return (int64_t)plan.need.tables;
}
#endif

// One line per stream: what the first setting gave, and whether every other setting gave the same.
//   "<index> <over> <pcm hash of the blocks that decoded> <same: 1|0> <status,status,...>"
// settings: bit s set = run setting s, s = never_lean | (cols == 64) << 1 | gathered << 2.  0 = four of the eight, in
// which every switch takes both values and every pair of switches all four combinations: settings 0 3 5 6 for an even
// index, their complements 1 2 4 7 for an odd one (a corpus of tens of thousands then sees all eight, at half the time).
int sim_digest(const uint8_t* lac, uint64_t size, uint32_t index, uint32_t settings, uint32_t pad, char* line, uint32_t cap) {
    lacx_stream_info info;
    const char* why = nullptr;
    if (parse_stream(lac, size, &info, &why) != LACX_OK) return -1;
    const int channels = info.channels;
    const uint32_t nb = info.blocks;
    const uint64_t frames = info.frames;
    std::vector<uint32_t> fr(nb);  // the blocks' frames, from the plan's tables
    {
        BatchIn in{};
        DecodePlan plan;
        int32_t none = 0;
        if (!plan_one(lac, size, &none, &none, in, plan)) return -1;
        Run run(plan, &in, 0);
        for (uint32_t b = 0; b < nb; ++b) fr[b] = (uint32_t)(run.a.frame_off[b + 1] - run.a.frame_off[b]);
    }
    if (settings == 0) settings = (index & 1u) ? 0x96u : 0x69u;
    std::vector<uint32_t> st0, st(nb);
    std::vector<uint8_t> ms0, ms(nb);
    std::vector<int32_t> l0, r0, l(frames), r(channels == 2 ? frames : 0);
    uint32_t over = 0, same = 1;
    bool first = true;
    for (uint32_t s = 0; s < 8; ++s) {
        if (!((settings >> s) & 1u)) continue;
        uint32_t ov = 0;
        if (sim_decode(lac, size, s & 1, (s & 2) ? 64 : 1, (s & 4) ? index + 1u : 0u, pad, st.data(), ms.data(), l.data(),
                       r.data(), &ov))
            return -1;
        if (ov > over) over = ov;
        if (first) {
            st0 = st, ms0 = ms, l0 = l, r0 = r;
            first = false;
            continue;
        }
        if (st != st0) same = 0;
        uint64_t f0 = 0;
        for (uint32_t b = 0; b < nb; f0 += fr[b], ++b) {
            if (st0[b] || st[b]) continue;
            if (ms[b] != ms0[b] || std::memcmp(&l[f0], &l0[f0], 4ull * fr[b]) ||
                (channels == 2 && std::memcmp(&r[f0], &r0[f0], 4ull * fr[b])))
                same = 0;
        }
    }
    if (first) return -1;
    uint64_t h = 0, f0 = 0;
    for (uint32_t b = 0; b < nb; f0 += fr[b], ++b) {
        if (st0[b]) continue;
        h = sim_hash(&l0[f0], fr[b], h);
        if (channels == 2) h = sim_hash(&r0[f0], fr[b], h);
        h = sim_hash(reinterpret_cast<const int32_t*>(&fr[b]), 1, h ^ ms0[b]);
    }
    int n = std::snprintf(line, cap, "%u %u %016llx %u ", index, over, (unsigned long long)h, same);
    for (uint32_t b = 0; b < nb && n > 0 && (uint32_t)n + 12 < cap; ++b)
        n += std::snprintf(line + n, cap - (uint32_t)n, b ? ",%u" : "%u", st0[b]);
    return (n > 0 && (uint32_t)n + 12 < cap) ? 0 : -1;
}

}  // extern "C"

#ifdef SIM_DECODE_MAIN
// sim_decode_san CORPUS FIRST COUNT SETTINGS PAD (PAD 4294967295 = kDecodeTailPad): streams [FIRST, FIRST + COUNT) of a corpus file (per stream: a 32-bit
// little-endian size, then the bytes), one digest line each on stdout, "done <count>" at the end.
// sim_decode_san batch CASES: every batch case of the file (per case: a 32-bit little-endian size, then the bytes, see
// sim_batch_digest), one line each, "done <count>" at the end.
int main(int argc, char** argv) {
    const bool batch = argc == 3 && !std::strcmp(argv[1], "batch");
    if (argc != 6 && !batch) return 2;
    std::vector<char> line(1 << 20);
    if (batch)
        return for_each_case(argv[2], [&](const uint8_t* blob, uint32_t size, uint32_t i) {
            return !sim_batch_digest(blob, size, i, line.data(), (uint32_t)line.size()) && std::puts(line.data()) >= 0;
        });
    const unsigned long first = std::strtoul(argv[2], nullptr, 10), count = std::strtoul(argv[3], nullptr, 10);
    const uint32_t settings = (uint32_t)std::strtoul(argv[4], nullptr, 10), pad = (uint32_t)std::strtoul(argv[5], nullptr, 10);
    return for_each_case(argv[1], [&](const uint8_t* lac, uint32_t size, uint32_t i) {  // the stream itself exact too: the container walk is checked with it
        return !sim_digest(lac, size, i, settings, pad, line.data(), (uint32_t)line.size()) && std::puts(line.data()) >= 0;
    }, first, count);
}
#endif
