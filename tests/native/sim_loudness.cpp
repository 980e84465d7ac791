// tests/native/sim_loudness.cpp -- TEST INFRASTRUCTURE: the loudness job (csrc/loudness_core.h, csrc/loudness_plan.h,
// csrc/loudness_rows.h) on the host, run the way the four kernels of k_loudness.hip run it.
//
// Stream jobs: what lacx_decoder_loudness_batch_device runs on the device, one lane after the other -- the job planned by
// plan_decode(..., digest form, loudness) and its tables filled by plan_fill_tables (csrc/decode_plan.h, the code
// api_decode.cpp runs), the lane code over the blocks, ms_inverse_tile as k_ms_inverse's grid runs it, then k_loud_states
// (one lane per chunk), k_loud_carry (one lane per item and channel), k_loud_energy and k_loud_rows (one lane per row and
// channel) over a scratch of exactly the plan's capacity, filled with a byte pattern: every record must be written before
// it is read.  Source jobs: items of generated PCM in a layout, in allocations that END exactly at the source's last byte
// behind a base at the byte offset the case asks for; optionally one element replaced by a raw 32-bit word (an invalid
// sample).  The totals are the product's (loudness_rows.h).
// Compiled with -ffp-contract=off like the kernels' translation unit: the rows are the bits the device must give.
// It is not part of the product and is not a fallback.
//
// Built twice by tests/loudtwin.py: a plain -O2 shared library for ctypes, and (-DSIM_LOUDNESS_MAIN) a sanitized program
// that runs a file of cases and prints one line per case.
#define SIM_JOB_SIMULATOR
#include "sim_job.h"

#include "import_msg.h"
#include "loudness_rows.h"

using namespace lacx;
using namespace simjob;

namespace {

constexpr int kFill = 0xCD;

uint32_t item_of(const unsigned long long* off, uint32_t nitems, unsigned long long x) {
    uint32_t j = 0;
    while (j + 1 < nitems && off[j + 1] <= x) ++j;
    return j;
}

// launch_loudness: the four kernels in stream order, every lane of each
void run_loudness(const LoudArgs& a) {
    if (!a.nitems) return;
    for (unsigned long long g = 0; g < a.total_chunks; ++g) {  // k_loud_states
        const uint32_t j = item_of(a.chunk_off, a.nitems, g);
        const LoudItem& it = a.items[j];
        const uint32_t c = (uint32_t)(g - a.chunk_off[j]);
        unsigned long long key = kDigestClean;
        LoudState out[2];
        loud_chunk_states(a.filters[it.rate], it, c, out, key);
        LoudState* at = a.states + it.lane0 + (unsigned long long)c * it.channels;
        at[0] = out[0];
        if (it.channels == 2) at[1] = out[1];
        if (it.validate && key < a.bad[j]) a.bad[j] = key;
    }
    for (uint32_t g = 0; a.total_chunks && g < 2u * a.nitems; ++g) {  // k_loud_carry
        const LoudItem& it = a.items[g >> 1];
        if ((g & 1u) < it.channels) loud_carry_lane(a.filters[it.rate], a.states + it.lane0, it.chunks, it.channels, g & 1u);
    }
    for (unsigned long long g = 0; g < a.total_chunks; ++g) {  // k_loud_energy
        const uint32_t j = item_of(a.chunk_off, a.nitems, g);
        const LoudItem& it = a.items[j];
        const uint32_t c = (uint32_t)(g - a.chunk_off[j]);
        const unsigned long long at = it.lane0 + (unsigned long long)c * it.channels;
        LoudState start[2];
        start[0] = a.states[at];
        if (it.channels == 2) start[1] = a.states[at + 1];
        LoudPartial out[2];
        loud_chunk_energy(a.filters[it.rate], it, c, start, out);
        a.partials[at] = out[0];
        if (it.channels == 2) a.partials[at + 1] = out[1];
    }
    for (unsigned long long g = 0; g < 2u * a.total_rows; ++g) {  // k_loud_rows
        const unsigned long long row = g >> 1;
        const uint32_t ch = (uint32_t)(g & 1u), j = item_of(a.row_off, a.nitems, row);
        const LoudItem& it = a.items[j];
        a.rows[row].energy[ch] = ch < it.channels ? loud_row(a.partials + it.lane0, it.channels, ch, it.sub, (uint32_t)(row - a.row_off[j])) : 0.0;
    }
}

struct StreamJob {
    std::vector<BatchIn> in;
    DecodePlan plan;
    std::vector<int> code;
    std::vector<std::string> err;
    std::unique_ptr<Run> run;
    std::unique_ptr<Heap<uint8_t>> scratch;
};

bool run_streams(const uint8_t* const* lacs, const uint64_t* sizes, uint32_t n, StreamJob& j) {
    j.in.resize(n);
    for (uint32_t i = 0; i < n; ++i) j.in[i] = BatchIn{lacs[i], sizes[i], nullptr, nullptr, 0};
    if (plan_decode(j.in.data(), n, DecodeForm::digest, kWholeStreams, false, j.plan, j.code, j.err, false, false, false, false, kRunsListCap, true)) return false;
    if (j.plan.loud_at.size != j.plan.need.tables || j.plan.need.loud_scratch != j.plan.loud_at.scratch) return false;
    j.run.reset(new Run(j.plan, j.in.data(), (uint32_t)kDecodeTailPad, kFill, kFill));
    j.scratch.reset(new Heap<uint8_t>(j.plan.need.loud_scratch, kFill));
    const DecodeArgs& a = j.run->a;
    place_payload(j.plan, j.in.data(), j.run->payload.p);
    if (j.plan.items.empty()) return true;
    if (a.digest || a.present || a.verify || a.window || a.wav) return false;  // launch_decode must end with k_ms_inverse in place
    Lane ln(1, 0);
    run_lanes(a, ln);
    run_ms_inverse(a);
    run_loudness(plan_loud_args(j.plan, j.run->tables.p, j.scratch->p));
    return true;
}

// per planned item, as collect of api_decode.cpp: its first failing block's status, else its rows and totals: fn(p, status, rows, count, totals)
template <typename Fn>
void stream_results(const StreamJob& j, Fn fn) {
    const auto* rows = reinterpret_cast<const lacx_loudness_row*>(j.scratch->p + j.plan.loud_at.rows);
    const auto* items = reinterpret_cast<const LoudItem*>(j.run->tables.p + j.plan.loud_at.items);
    for (size_t k = 0; k < j.plan.items.size(); ++k) {
        const PlanItem& p = j.plan.items[k];
        uint32_t status = 0;
        for (uint32_t b = 0; b < p.item.blocks && !status; ++b) status = j.run->st.p[p.item.block0 + b];
        const LoudItem& li = items[k];
        const lacx_loudness t = status ? lacx_loudness{} : loudness_of_rows(rows + li.row0, li.rows, p.info.channels, p.info.bit_depth, p.info.sample_rate);
        if (!fn(p, status, rows + li.row0, status ? 0u : li.rows, t)) return;
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

// items of generated PCM as one source job; key[j]: the lowest invalid sample's key
struct SourceJob {
    std::vector<std::unique_ptr<Exact>> own;
    std::vector<LoudIn> in;
    LoudLayout y;
    std::unique_ptr<Heap<uint8_t>> tables, scratch;
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
        j.in.push_back(LoudIn{s0, s1, s.frames, s.rate, s.layout, (uint8_t)s.channels, (uint8_t)s.bit_depth, true});
    }
    j.y = loud_layout(0, j.in.data(), n);
    j.tables.reset(new Heap<uint8_t>(j.y.size, kFill));
    j.scratch.reset(new Heap<uint8_t>(j.y.scratch, kFill));
    j.bad.assign(n, kDigestClean);
    loud_fill(j.y, j.in.data(), n, j.tables->p);
    run_loudness(loud_args(j.y, n, j.tables->p, j.scratch->p, j.bad.data()));
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

// the four rates' filters as loudness_plan.h makes them: 26 doubles each (sb, sna, hb, hna, A row by row)
void sim_loud_filters(double* out) {
    for (int k = 0; k < 4; ++k) {
        const LoudFilter f = loud_filter(kLoudRates[k]);
        static_assert(sizeof(LoudFilter) == 26 * sizeof(double), "sb sna hb hna A");
        std::memcpy(out + 26 * k, &f, sizeof(f));
    }
}

// n streams as one loudness job.  Per input i, rec[3 * i] = the plan's code for it (0: it went to the device; then)
// rec[3 * i + 1] = its rows and rec[3 * i + 2] = the status of its first failing block (0: it decoded).  rows: per item that
// decoded, in input order, its rows; totals: lacx_loudness[n] (zero for an item without a result).  msg: the refused items'
// messages, '\n' between inputs.  Returns the rows written, -1 where the job cannot be planned or rows_cap is too small.
int64_t sim_loud_streams(const uint8_t* const* lacs, const uint64_t* sizes, uint32_t n, uint64_t* rec, lacx_loudness_row* rows, uint64_t rows_cap,
                         lacx_loudness* totals, char* msg, uint32_t msg_cap) {
    StreamJob j;
    if (!run_streams(lacs, sizes, n, j)) return -1;
    std::string all;
    for (uint32_t i = 0; i < n; ++i) {
        rec[3 * i] = (uint64_t)j.code[i], rec[3 * i + 1] = rec[3 * i + 2] = 0;
        totals[i] = lacx_loudness{};
        all += (i ? "\n" : "") + j.err[i];
    }
    std::snprintf(msg, msg_cap, "%s", all.c_str());
    std::vector<std::vector<lacx_loudness_row>> per(n);
    bool fits = true;
    uint64_t total = 0;
    stream_results(j, [&](const PlanItem& p, uint32_t status, const lacx_loudness_row* r, uint32_t count, const lacx_loudness& t) {
        rec[3 * p.src + 1] = count, rec[3 * p.src + 2] = status;
        per[p.src].assign(r, r + count);
        totals[p.src] = t;
        total += count;
        return true;
    });
    if (total > rows_cap) fits = false;
    uint64_t at = 0;
    for (uint32_t i = 0; fits && i < n; ++i)
        for (const lacx_loudness_row& r : per[i]) rows[at++] = r;
    return fits ? (int64_t)at : -1;
}

// A stream case (little-endian, written by tests/loudtwin.py): u32 n, then per stream u64 size and the bytes.  One line:
// "<index> <item>;<item>;..." with item = "!<code>" (refused by the plan), "x<status>" (a block failed) or
// "<rows> <hash of the rows> <hash of the totals>".
int sim_loud_line(const uint8_t* blob, uint64_t size, uint32_t index, char* line, uint32_t cap) {
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
    stream_results(j, [&](const PlanItem& p, uint32_t status, const lacx_loudness_row* r, uint32_t count, const lacx_loudness& t) {
        item[p.src] = status ? "x" + std::to_string(status)
                             : std::to_string(count) + " " + hex(fnv(r, count * sizeof(lacx_loudness_row), kFnvStart)) + " " + hex(fnv(&t, sizeof(t), kFnvStart));
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
int64_t sim_loud_sources(uint32_t n, const uint32_t* layout, const uint32_t* channels, const uint32_t* bit_depth, const uint32_t* rate,
                         const uint32_t* offset, const uint64_t* frames, const int32_t* const* samples, const uint64_t* bad_frame,
                         const uint32_t* bad_channel, const uint32_t* bad_word, lacx_loudness_row* rows, uint64_t rows_cap, uint32_t* counts,
                         lacx_loudness* totals, uint64_t* keys, char* msg, uint32_t msg_cap) {
    std::vector<SourceSpec> spec(n);
    for (uint32_t k = 0; k < n; ++k)
        spec[k] = SourceSpec{layout[k], channels[k], bit_depth[k], rate[k], offset[k], frames[k], samples[k], bad_frame[k], bad_channel[k], bad_word[k]};
    SourceJob j;
    run_sources(spec.data(), n, j);
    const auto* items = reinterpret_cast<const LoudItem*>(j.tables->p + j.y.items);
    const auto* all = reinterpret_cast<const lacx_loudness_row*>(j.scratch->p + j.y.rows);
    std::string text;
    uint64_t at = 0;
    for (uint32_t k = 0; k < n; ++k) {
        keys[k] = j.bad[k];
        counts[k] = 0;
        totals[k] = lacx_loudness{};
        if (k) text += "\n";
        if (j.bad[k] != kDigestClean) {
            text += bad_text(j.bad[k], (int)bit_depth[k]);
            continue;
        }
        if (at + items[k].rows > rows_cap) return -1;
        for (uint32_t s = 0; s < items[k].rows; ++s) rows[at++] = all[items[k].row0 + s];
        counts[k] = items[k].rows;
        totals[k] = loudness_of_rows(all + items[k].row0, items[k].rows, (uint8_t)channels[k], (uint8_t)bit_depth[k], rate[k]);
    }
    std::snprintf(msg, msg_cap, "%s", text.c_str());
    return (int64_t)at;
}

// loudness_rows.h's totals through plain C (what lacx_loudness_combine calls)
void sim_loud_combine(const lacx_loudness_row* const* rows, const uint32_t* counts, const uint8_t* channels, const uint8_t* bit_depths,
                      const uint32_t* rates, uint32_t nsets, lacx_loudness* out) {
    std::vector<LoudSet> sets(nsets);
    for (uint32_t k = 0; k < nsets; ++k) sets[k] = LoudSet{rows[k], counts[k], channels[k], bit_depths[k], rates[k]};
    *out = loudness_combine(sets.data(), nsets);
}

}  // extern "C"

#ifdef SIM_LOUDNESS_MAIN
// sim_loudness_san CASES: every case of the file (per case: a 32-bit little-endian size, a type byte, then the bytes).
// Type 0: a stream case (sim_loud_line).  Type 1: a source case of one item -- u32 layout, channels, bit_depth, rate, offset,
// u64 frames, u64 bad_frame, u32 bad_channel, bad_word, i32 samples[channels * frames] -- whose line is "<index> <key> <rows>
// <hash of the rows> <hash of the totals> <message>".  "done <count>" at the end.
int main(int argc, char** argv) {
    if (argc != 2) return 2;
    std::vector<char> line(1 << 20);
    return for_each_case(argv[1], [&](const uint8_t* blob, uint32_t size, uint32_t i) {
        if (size < 1) return false;
        if (blob[0] == 0) {
            if (sim_loud_line(blob + 1, size - 1, i, line.data(), (uint32_t)line.size())) return false;
        } else {
            Reader rd{blob + 1, blob + size};
            const uint32_t layout = rd.get<uint32_t>(), channels = rd.get<uint32_t>(), depth = rd.get<uint32_t>(), rate = rd.get<uint32_t>();
            const uint32_t offset = rd.get<uint32_t>();
            const uint64_t frames = rd.get<uint64_t>(), bad_frame = rd.get<uint64_t>();
            const uint32_t bad_channel = rd.get<uint32_t>(), bad_word = rd.get<uint32_t>();
            if (!rd.ok || frames == 0 || (uint64_t)(rd.end - rd.p) != 4ull * channels * frames) return false;
            Heap<int32_t> samples(channels * frames);
            std::memcpy(samples.p, rd.p, 4ull * channels * frames);
            const uint64_t cap = frames / (rate / 10u) + 1;
            std::vector<lacx_loudness_row> rows(cap);
            const int32_t* sp = samples.p;
            lacx_loudness t{};
            uint64_t key = 0;
            uint32_t count = 0;
            char msg[256];
            if (sim_loud_sources(1, &layout, &channels, &depth, &rate, &offset, &frames, &sp, &bad_frame, &bad_channel, &bad_word, rows.data(), cap, &count,
                                 &t, &key, msg, sizeof(msg)) < 0)
                return false;
            const std::string s = std::to_string(i) + " " + std::to_string(key) + " " + std::to_string(count) + " " +
                                  hex(fnv(rows.data(), (uint64_t)count * sizeof(lacx_loudness_row), kFnvStart)) + " " + hex(fnv(&t, sizeof(t), kFnvStart)) + " " + msg;
            std::snprintf(line.data(), line.size(), "%s", s.c_str());
        }
        return std::puts(line.data()) >= 0;
    });
}
#endif
