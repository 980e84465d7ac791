// tests/native/sim_truepeak.cpp -- TEST INFRASTRUCTURE: the true-peak job (csrc/truepeak_core.h, csrc/truepeak_plan.h,
// csrc/truepeak_rows.h) on the host, run the way k_truepeak of k_truepeak.hip runs it.
//
// Stream jobs: what lacx_decoder_truepeak_batch_device runs on the device, one lane after the other -- the job planned by
// plan_decode(..., digest form, truepeak) and its tables filled by plan_fill_tables (csrc/decode_plan.h, the code
// api_decode.cpp runs), the lane code over the blocks, ms_inverse_tile as k_ms_inverse's grid runs it, then k_truepeak: per
// tile the 256 lanes' units and the three units of history staged in an array of exactly the kernel's LDS size (filled
// with a byte pattern: every word must be written before it is read), every lane's 16-sample window read from it, the
// lanes' parts merged and the tile's part merged into its row.  The scratch PCM starts as a byte pattern too: a sample a
// lane must not read would change a row.  Source jobs: items of generated PCM in a layout, in allocations that END exactly
// at the source's last byte behind a base at the byte offset the case asks for; optionally one element replaced by a raw
// 32-bit word (an invalid sample).  The rows and totals are the product's (truepeak_rows.h).
// It is not part of the product and is not a fallback.
//
// Built twice by tests/peaktwin.py: a plain -O2 shared library for ctypes, and (-DSIM_TRUEPEAK_MAIN) a sanitized program
// that runs a file of cases and prints one line per case.
#define SIM_JOB_SIMULATOR
#include "sim_job.h"

#include "import_msg.h"
#include "truepeak_core.h"
#include "truepeak_rows.h"

using namespace lacx;
using namespace simjob;

namespace {

constexpr int kFill = 0xCD;

// launch_truepeak: every tile, every lane of each
void run_truepeak(const TpArgs& a) {
    if (!a.nitems) return;
    constexpr uint32_t kStage = kTpHistory + kTpTileFrames;
    for (unsigned long long tile = 0; tile < a.total_tiles; ++tile) {
        uint32_t j = 0;
        while (j + 1 < a.nitems && a.tile_off[j + 1] <= tile) ++j;
        const TpItem& it = a.items[j];
        const unsigned long long t = tile - a.tile_off[j], tile_start = t * kTpTileFrames;
        const bool stereo = it.channels == 2, deep = it.bit_depth == 24;
        Heap<int32_t> stage0(kStage, kFill), stage1(kStage, kFill);
        Heap<int32_t> own(8u * kTpThreads);  // every lane's unit as loaded: l[4], r[4]
        for (uint32_t tid = 0; tid < kTpThreads; ++tid) {
            unsigned long long key = kDigestClean, other = kDigestClean;
            int32_t* l = own.p + 8u * tid;
            int32_t* r = l + 4;
            tp_load_unit(it, tile_start + 4u * tid, key, l, r);
            std::memcpy(stage0.p + kTpHistory + 4u * tid, l, 16);
            if (stereo) std::memcpy(stage1.p + kTpHistory + 4u * tid, r, 16);
            if (tid < kTpHistory / 4u) {
                int32_t hl[4] = {0, 0, 0, 0}, hr[4] = {0, 0, 0, 0};
                if (t != 0u) tp_load_unit(it, tile_start - kTpHistory + 4u * tid, other, hl, hr);
                std::memcpy(stage0.p + 4u * tid, hl, 16);
                if (stereo) std::memcpy(stage1.p + 4u * tid, hr, 16);
            }
            if (it.validate && key < a.bad[j]) a.bad[j] = key;
        }
        const uint32_t row = tp_tile_row(tile_start, it.frames);
        TpLane all{{0, 0}, {0, 0}};
        for (uint32_t tid = 0; tid < kTpThreads; ++tid) {
            int32_t wl[16], wr[16] = {};
            std::memcpy(wl, stage0.p + 4u * tid, 64);
            if (stereo) std::memcpy(wr, stage1.p + 4u * tid, 64);
            const unsigned long long n0 = tile_start + 4u * tid;
            const uint32_t pos0 = 4u * (uint32_t)(n0 - (unsigned long long)row * kTpRowFrames);
            tp_merge(all, tp_lane(wl, wr, own.p + 8u * tid, own.p + 8u * tid + 4, stereo, deep, pos0));
        }
        TpAcc* at = a.rows + it.row0 + row;  // the atomics: maxima into the zeroed row
        for (uint32_t c = 0; c < it.channels; ++c) {
            if (all.key[c] > at->key[c]) at->key[c] = all.key[c];
            if (all.sample_peak[c] > at->sample_peak[c]) at->sample_peak[c] = all.sample_peak[c];
        }
    }
}

struct StreamJob {
    std::vector<BatchIn> in;
    DecodePlan plan;
    std::vector<int> code;
    std::vector<std::string> err;
    std::unique_ptr<Run> run;
};

bool run_streams(const uint8_t* const* lacs, const uint64_t* sizes, uint32_t n, StreamJob& j) {
    j.in.resize(n);
    for (uint32_t i = 0; i < n; ++i) j.in[i] = BatchIn{lacs[i], sizes[i], nullptr, nullptr, 0};
    if (plan_decode(j.in.data(), n, DecodeForm::digest, kWholeStreams, false, j.plan, j.code, j.err, false, false, false, false, kRunsListCap, false, true)) return false;
    if (j.plan.peak_at.size != j.plan.need.tables) return false;
    j.run.reset(new Run(j.plan, j.in.data(), (uint32_t)kDecodeTailPad, kFill, kFill));
    const DecodeArgs& a = j.run->a;
    place_payload(j.plan, j.in.data(), j.run->payload.p);
    if (j.plan.items.empty()) return true;
    if (a.digest || a.present || a.verify || a.window || a.wav) return false;  // launch_decode must end with k_ms_inverse in place
    Lane ln(1, 0);
    run_lanes(a, ln);
    run_ms_inverse(a);
    run_truepeak(plan_peak_args(j.plan, j.run->tables.p));
    return true;
}

// per planned item, as collect of api_decode.cpp: its first failing block's status, else its rows and totals
template <typename Fn>
void stream_results(const StreamJob& j, Fn fn) {
    const auto* acc = reinterpret_cast<const TpAcc*>(j.run->tables.p + j.plan.peak_at.rows);
    const auto* items = reinterpret_cast<const TpItem*>(j.run->tables.p + j.plan.peak_at.items);
    for (size_t k = 0; k < j.plan.items.size(); ++k) {
        const PlanItem& p = j.plan.items[k];
        uint32_t status = 0;
        for (uint32_t b = 0; b < p.item.blocks && !status; ++b) status = j.run->st.p[p.item.block0 + b];
        std::vector<lacx_truepeak_row> rows;
        if (!status) truepeak_rows_of(acc + items[k].row0, items[k].rows, rows);
        const lacx_truepeak t = status ? lacx_truepeak{}
                                       : truepeak_of_rows(TpSet{rows.data(), (uint32_t)rows.size(), p.info.channels, p.info.bit_depth, p.info.frames, p.info.sample_rate});
        if (!fn(p, status, rows, t)) return;
    }
}

std::string hex(uint64_t h) {
    char s[24];
    std::snprintf(s, sizeof(s), "%016llx", (unsigned long long)h);
    return s;
}

struct SourceSpec {
    uint32_t layout, channels, bit_depth, rate, offset;
    uint64_t frames;
    const int32_t* samples;  // [channels][frames]
    uint64_t bad_frame;
    uint32_t bad_channel, bad_word;
};

struct SourceJob {
    std::vector<std::unique_ptr<Exact>> own;
    std::vector<TpIn> in;
    TpLayout y;
    std::unique_ptr<Heap<uint8_t>> tables;
    std::vector<unsigned long long> bad;
};

void run_sources(const SourceSpec* spec, uint32_t n, SourceJob& j) {
    for (uint32_t k = 0; k < n; ++k) {
        const SourceSpec& s = spec[k];
        const uint32_t eb = elem_bytes(s.layout);
        const bool pl = planar(s.layout), f32 = s.layout == (uint32_t)PCM_PLANAR_F32 || s.layout == (uint32_t)PCM_INTERLEAVED_F32;
        const uint64_t bytes0 = pl ? s.frames * eb : s.frames * s.channels * eb;
        const bool two_rows = pl && s.channels == 2;
        j.own.emplace_back(new Exact(bytes0, s.offset % 16u));
        uint8_t* s0 = j.own.back()->data;
        uint8_t* s1 = nullptr;
        if (two_rows) {
            j.own.emplace_back(new Exact(bytes0, s.offset % 16u));
            s1 = j.own.back()->data;
        }
        for (uint64_t f = 0; f < s.frames; ++f)
            for (uint32_t c = 0; c < s.channels; ++c) {
                int32_t v = s.samples[c * s.frames + f];
                if (f32) {
                    const float x = (float)v / (float)(1 << (s.bit_depth - 1));
                    std::memcpy(&v, &x, 4);
                }
                if (f == s.bad_frame && c == s.bad_channel && eb == 4u) v = (int32_t)s.bad_word;
                put_elem(s0, s1, s.layout, s.channels, f, c, v);
            }
        j.in.push_back(TpIn{s0, s1, s.frames, s.layout, (uint8_t)s.channels, (uint8_t)s.bit_depth, true});
    }
    j.y = tp_layout(0, j.in.data(), n);
    j.tables.reset(new Heap<uint8_t>(j.y.size, kFill));
    j.bad.assign(n, kDigestClean);
    tp_fill(j.y, j.in.data(), n, j.tables->p);
    run_truepeak(tp_args(j.y, n, j.tables->p, j.bad.data()));
}

std::string bad_text(unsigned long long bad, int bit_depth) {  // as digest_pcm_run of api_decode.cpp words it
    ImportBad b{{kImportClean, kImportClean}};
    b.key[bad >> 63] = bad & ~(1ull << 63);
    int ch = 0;
    unsigned long long index = 0;
    std::string text;
    (void)import_bad_message(b, bit_depth, &ch, &index, text);
    return text;
}

}  // namespace

extern "C" {

// the table as truepeak_core.h has it: c[p][k], 48 integers
void sim_peak_table(int32_t* out) {
    for (uint32_t p = 0; p < kTpPhases; ++p)
        for (uint32_t k = 0; k < kTpTaps; ++k) out[kTpTaps * p + k] = tp_coef(p, k);
}

// n streams as one true-peak job.  Per input i, rec[3 * i] = the plan's code for it (0: it went to the device; then)
// rec[3 * i + 1] = its rows and rec[3 * i + 2] = the status of its first failing block (0: it decoded).  rows: per item that
// decoded, in input order, its rows; totals: lacx_truepeak[n] (zero for an item without a result).  msg: the refused items'
// messages, '\n' between inputs.  Returns the rows written, -1 where the job cannot be planned or rows_cap is too small.
int64_t sim_peak_streams(const uint8_t* const* lacs, const uint64_t* sizes, uint32_t n, uint64_t* rec, lacx_truepeak_row* rows, uint64_t rows_cap,
                         lacx_truepeak* totals, char* msg, uint32_t msg_cap) {
    StreamJob j;
    if (!run_streams(lacs, sizes, n, j)) return -1;
    std::string all;
    for (uint32_t i = 0; i < n; ++i) {
        rec[3 * i] = (uint64_t)j.code[i], rec[3 * i + 1] = rec[3 * i + 2] = 0;
        totals[i] = lacx_truepeak{};
        all += (i ? "\n" : "") + j.err[i];
    }
    std::snprintf(msg, msg_cap, "%s", all.c_str());
    std::vector<std::vector<lacx_truepeak_row>> per(n);
    uint64_t total = 0;
    stream_results(j, [&](const PlanItem& p, uint32_t status, const std::vector<lacx_truepeak_row>& r, const lacx_truepeak& t) {
        rec[3 * p.src + 1] = r.size(), rec[3 * p.src + 2] = status;
        per[p.src] = r;
        totals[p.src] = t;
        total += r.size();
        return true;
    });
    if (total > rows_cap) return -1;
    uint64_t at = 0;
    for (uint32_t i = 0; i < n; ++i)
        for (const lacx_truepeak_row& r : per[i]) rows[at++] = r;
    return (int64_t)at;
}

// A stream case (little-endian, written by tests/peaktwin.py): u32 n, then per stream u64 size and the bytes.  One line:
// "<index> <item>;<item>;..." with item = "!<code>" (refused by the plan), "x<status>" (a block failed) or
// "<rows> <hash of the rows> <hash of the totals>".
int sim_peak_line(const uint8_t* blob, uint64_t size, uint32_t index, char* line, uint32_t cap) {
    if (size < 4) return -1;
    uint32_t n;
    std::memcpy(&n, blob, 4);
    std::vector<std::unique_ptr<Heap<uint8_t>>> own;  // every stream an exact allocation of its own
    std::vector<const uint8_t*> lacs(n);
    std::vector<uint64_t> sizes(n);
    uint64_t at = 4;
    for (uint32_t i = 0; i < n; ++i) {
        if (size - at < 8) return -1;
        std::memcpy(&sizes[i], blob + at, 8);
        at += 8;
        if (size - at < sizes[i]) return -1;
        own.emplace_back(new Heap<uint8_t>(sizes[i]));
        std::memcpy(own.back()->p, blob + at, sizes[i]);
        at += sizes[i];
        lacs[i] = own.back()->p;
    }
    StreamJob j;
    if (!run_streams(lacs.data(), sizes.data(), n, j)) return -1;
    std::vector<std::string> item(n);
    for (uint32_t i = 0; i < n; ++i) item[i] = "!" + std::to_string(j.code[i]);
    stream_results(j, [&](const PlanItem& p, uint32_t status, const std::vector<lacx_truepeak_row>& r, const lacx_truepeak& t) {
        item[p.src] = status ? "x" + std::to_string(status)
                             : std::to_string(r.size()) + " " + hex(fnv(r.data(), r.size() * sizeof(lacx_truepeak_row), kFnvStart)) + " " + hex(fnv(&t, sizeof(t), kFnvStart));
        return true;
    });
    std::string out = std::to_string(index) + " ";
    for (uint32_t i = 0; i < n; ++i) out += (i ? ";" : "") + item[i];
    if (out.size() + 1 > cap) return -1;
    std::memcpy(line, out.c_str(), out.size() + 1);
    return 0;
}

// n items of generated PCM as one source job: item k has frames[k] frames whose sample (c, f) is samples[k][c * frames + f]
// (for a float layout the exact float of that sample at the depth), laid out as layout[k] in allocations that end with the
// source's last byte behind a base offset[k] bytes behind a 16-byte aligned address.  bad_frame[k] != all ones: element
// (bad_frame, bad_channel) of a 4-byte layout is the raw word bad_word instead.  keys[k]: the lowest invalid sample's key
// (all ones: none; the item then has no rows and a zeroed result), msg: the texts the product words them with, '\n' between
// items.  rows: the items' rows in order, counts[k] of them.  Returns the rows written, -1 where rows_cap is too small.
int64_t sim_peak_sources(uint32_t n, const uint32_t* layout, const uint32_t* channels, const uint32_t* bit_depth, const uint32_t* rate,
                         const uint32_t* offset, const uint64_t* frames, const int32_t* const* samples, const uint64_t* bad_frame,
                         const uint32_t* bad_channel, const uint32_t* bad_word, lacx_truepeak_row* rows, uint64_t rows_cap, uint32_t* counts,
                         lacx_truepeak* totals, uint64_t* keys, char* msg, uint32_t msg_cap) {
    std::vector<SourceSpec> spec(n);
    for (uint32_t k = 0; k < n; ++k)
        spec[k] = SourceSpec{layout[k], channels[k], bit_depth[k], rate[k], offset[k], frames[k], samples[k], bad_frame[k], bad_channel[k], bad_word[k]};
    SourceJob j;
    run_sources(spec.data(), n, j);
    const auto* items = reinterpret_cast<const TpItem*>(j.tables->p + j.y.items);
    const auto* acc = reinterpret_cast<const TpAcc*>(j.tables->p + j.y.rows);
    std::string text;
    uint64_t at = 0;
    for (uint32_t k = 0; k < n; ++k) {
        keys[k] = j.bad[k];
        counts[k] = 0;
        totals[k] = lacx_truepeak{};
        if (k) text += "\n";
        if (j.bad[k] != kDigestClean) {
            text += bad_text(j.bad[k], (int)bit_depth[k]);
            continue;
        }
        if (at + items[k].rows > rows_cap) return -1;
        std::vector<lacx_truepeak_row> mine;
        truepeak_rows_of(acc + items[k].row0, items[k].rows, mine);
        for (const lacx_truepeak_row& r : mine) rows[at++] = r;
        counts[k] = items[k].rows;
        totals[k] = truepeak_of_rows(TpSet{mine.data(), (uint32_t)mine.size(), (uint8_t)channels[k], (uint8_t)bit_depth[k], frames[k], rate[k]});
    }
    std::snprintf(msg, msg_cap, "%s", text.c_str());
    return (int64_t)at;
}

// truepeak_rows.h's totals through plain C (what lacx_truepeak_combine calls)
void sim_peak_combine(const lacx_truepeak_row* const* rows, const uint32_t* counts, const uint8_t* channels, const uint8_t* bit_depths,
                      const uint64_t* frames, const uint32_t* rates, uint32_t nsets, lacx_truepeak* out) {
    std::vector<TpSet> sets(nsets);
    for (uint32_t k = 0; k < nsets; ++k) sets[k] = TpSet{rows[k], counts[k], channels[k], bit_depths[k], frames[k], rates[k]};
    *out = truepeak_combine(sets.data(), nsets);
}

}  // extern "C"

#ifdef SIM_TRUEPEAK_MAIN
// sim_truepeak_san CASES: every case of the file (per case: a 32-bit little-endian size, a type byte, then the bytes).
// Type 0: a stream case (sim_peak_line).  Type 1: a source case of one item -- u32 layout, channels, bit_depth, rate, offset,
// u64 frames, u64 bad_frame, u32 bad_channel, bad_word, i32 samples[channels * frames] -- whose line is "<index> <key> <rows>
// <hash of the rows> <hash of the totals> <message>".  "done <count>" at the end.
int main(int argc, char** argv) {
    if (argc != 2) return 2;
    std::vector<char> line(1 << 20);
    return for_each_case(argv[1], [&](const uint8_t* blob, uint32_t size, uint32_t i) {
        if (size < 1) return false;
        if (blob[0] == 0) {
            if (sim_peak_line(blob + 1, size - 1, i, line.data(), (uint32_t)line.size())) return false;
        } else {
            Reader rd{blob + 1, blob + size};
            const uint32_t layout = rd.get<uint32_t>(), channels = rd.get<uint32_t>(), depth = rd.get<uint32_t>(), rate = rd.get<uint32_t>();
            const uint32_t offset = rd.get<uint32_t>();
            const uint64_t frames = rd.get<uint64_t>(), bad_frame = rd.get<uint64_t>();
            const uint32_t bad_channel = rd.get<uint32_t>(), bad_word = rd.get<uint32_t>();
            if (!rd.ok || frames == 0 || (uint64_t)(rd.end - rd.p) != 4ull * channels * frames) return false;
            Heap<int32_t> samples(channels * frames);
            std::memcpy(samples.p, rd.p, 4ull * channels * frames);
            const uint64_t cap = frames / kTpRowFrames + 1;
            std::vector<lacx_truepeak_row> rows(cap);
            const int32_t* sp = samples.p;
            lacx_truepeak t{};
            uint64_t key = 0;
            uint32_t count = 0;
            char msg[256];
            if (sim_peak_sources(1, &layout, &channels, &depth, &rate, &offset, &frames, &sp, &bad_frame, &bad_channel, &bad_word, rows.data(), cap, &count, &t,
                                 &key, msg, sizeof(msg)) < 0)
                return false;
            const std::string s = std::to_string(i) + " " + std::to_string(key) + " " + std::to_string(count) + " " +
                                  hex(fnv(rows.data(), (uint64_t)count * sizeof(lacx_truepeak_row), kFnvStart)) + " " + hex(fnv(&t, sizeof(t), kFnvStart)) + " " + msg;
            std::snprintf(line.data(), line.size(), "%s", s.c_str());
        }
        return std::puts(line.data()) >= 0;
    });
}
#endif
