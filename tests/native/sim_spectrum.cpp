// tests/native/sim_spectrum.cpp -- TEST INFRASTRUCTURE: the spectrum job (csrc/spectrum_core.h, csrc/spectrum_plan.h,
// csrc/spectrum_rows.h) on the host, run the way k_spectrum of k_spectrum.hip runs it.
//
// Stream jobs: what lacx_decoder_spectrum_batch_device runs on the device, one lane after the other -- the job planned by
// plan_decode(..., digest form, spectrum) and its tables filled by plan_fill_tables (csrc/decode_plan.h, the code
// api_decode.cpp runs), the lane code over the blocks, ms_inverse_tile as k_ms_inverse's grid runs it, then k_spectrum: per
// row its windows in order; per window the units loaded into two arrays of exactly the kernel's LDS size (filled with a
// byte pattern: every point must be written before it is read), the stages' butterflies one after the other, then the 128
// (channel, band) lanes' sums into their accumulators, and the row written once behind the last window.  The scratch PCM
// starts as a byte pattern too: a sample a lane must not read would change a row.  Source jobs: items of generated PCM in
// a layout, in allocations that END exactly at the source's last byte behind a base at the byte offset the case asks for;
// optionally one element replaced by a raw 32-bit word (an invalid sample).  The totals are the product's
// (spectrum_rows.h).  It is not part of the product and is not a fallback.
//
// Built twice by tests/spectwin.py, both with -ffp-contract=off as the kernel is: a plain -O2 shared library for ctypes, and
// (-DSIM_SPECTRUM_MAIN) a sanitized program that runs a file of cases and prints one line per case.
#define SIM_JOB_SIMULATOR
#include "sim_job.h"

#include "import_msg.h"
#include "spectrum_core.h"
#include "spectrum_rows.h"

using namespace lacx;
using namespace simjob;

namespace {

constexpr int kFill = 0xCD;

// launch_spectrum: every row, every window of each, every lane's part of each
void run_spectrum(const SpArgs& a) {
    if (!a.nitems) return;
    const uint32_t logn = a.logn, n = 1u << logn;
    for (unsigned long long row = 0; row < a.total_rows; ++row) {
        uint32_t j = 0;
        while (j + 1 < a.nitems && a.row_off[j + 1] <= row) ++j;
        const SpItem& it = a.items[j];
        const uint32_t r = (uint32_t)(row - a.row_off[j]);
        unsigned long long first, end;
        sp_row_windows(it, logn, r, first, end);
        double acc[2][kSpBands] = {};
        for (unsigned long long k = first; k < end; ++k) {
            Heap<double> re(n, kFill), im(n, kFill);
            for (uint32_t u = 0; u < n / 4u; ++u) {
                unsigned long long key = kDigestClean;
                sp_load_unit(it, logn, k, u, a.window, key, re.p, im.p);
                if (it.validate && key < a.bad[j]) a.bad[j] = key;
            }
            for (uint32_t h = n / 2u; h; h >>= 1)
                for (uint32_t b = 0; b < n / 2u; ++b) sp_butterfly(logn, h, b, a.twiddle, re.p, im.p);
            for (uint32_t c = 0; c < it.channels; ++c)
                for (uint32_t band = 0; band < kSpBands; ++band) acc[c][band] = acc[c][band] + sp_band_power(logn, c, band, re.p, im.p);
        }
        for (uint32_t c = 0; c < it.channels; ++c)
            for (uint32_t band = 0; band < kSpBands; ++band) a.rows[it.row0 + r].power[c][band] = acc[c][band];
    }
}

struct StreamJob {
    std::vector<BatchIn> in;
    DecodePlan plan;
    std::vector<int> code;
    std::vector<std::string> err;
    std::unique_ptr<Run> run;
};

bool run_streams(const uint8_t* const* lacs, const uint64_t* sizes, uint32_t n, uint32_t window, StreamJob& j) {
    j.in.resize(n);
    for (uint32_t i = 0; i < n; ++i) j.in[i] = BatchIn{lacs[i], sizes[i], nullptr, nullptr, 0};
    if (plan_decode(j.in.data(), n, DecodeForm::digest, kWholeStreams, false, j.plan, j.code, j.err, false, false, false, false, kRunsListCap, false, false, window))
        return false;
    if (j.plan.spec_at.size != j.plan.need.tables) return false;
    j.run.reset(new Run(j.plan, j.in.data(), (uint32_t)kDecodeTailPad, kFill, kFill));
    const DecodeArgs& a = j.run->a;
    place_payload(j.plan, j.in.data(), j.run->payload.p);
    if (j.plan.items.empty()) return true;
    if (a.digest || a.present || a.verify || a.window || a.wav) return false;  // launch_decode must end with k_ms_inverse in place
    Lane ln(1, 0);
    run_lanes(a, ln);
    run_ms_inverse(a);
    run_spectrum(plan_spec_args(j.plan, j.run->tables.p));
    return true;
}

// per planned item, as collect of api_decode.cpp: its first failing block's status, else its rows
template <typename Fn>
void stream_results(const StreamJob& j, Fn fn) {
    const auto* all = reinterpret_cast<const lacx_spectrum_row*>(j.run->tables.p + j.plan.spec_at.rows);
    const auto* items = reinterpret_cast<const SpItem*>(j.run->tables.p + j.plan.spec_at.items);
    for (size_t k = 0; k < j.plan.items.size(); ++k) {
        const PlanItem& p = j.plan.items[k];
        uint32_t status = 0;
        for (uint32_t b = 0; b < p.item.blocks && !status; ++b) status = j.run->st.p[p.item.block0 + b];
        std::vector<lacx_spectrum_row> rows;
        if (!status) rows.assign(all + items[k].row0, all + items[k].row0 + items[k].rows);
        if (!fn(p, status, rows)) return;
    }
}

std::string hex(uint64_t h) {
    char s[24];
    std::snprintf(s, sizeof(s), "%016llx", (unsigned long long)h);
    return s;
}

struct SourceSpec {
    uint32_t layout, channels, bit_depth, offset;
    uint64_t frames;
    const int32_t* samples;  // [channels][frames]
    uint64_t bad_frame;
    uint32_t bad_channel, bad_word;
};

struct SourceJob {
    std::vector<std::unique_ptr<Exact>> own;
    std::vector<SpIn> in;
    SpLayout y;
    std::unique_ptr<Heap<uint8_t>> tables;
    std::vector<unsigned long long> bad;
};

void run_sources(const SourceSpec* spec, uint32_t n, uint32_t logn, SourceJob& j) {
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
        j.in.push_back(SpIn{s0, s1, s.frames, s.layout, (uint8_t)s.channels, (uint8_t)s.bit_depth, true});
    }
    j.y = sp_layout(0, j.in.data(), n, logn);
    j.tables.reset(new Heap<uint8_t>(j.y.size, kFill));
    j.bad.assign(n, kDigestClean);
    sp_fill(j.y, j.in.data(), n, j.tables->p);
    run_spectrum(sp_args(j.y, n, j.tables->p, j.bad.data()));
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

// the tables as spectrum_plan.h makes them: window [N], twiddle [N / 2][2]; -1 for an unsupported window
int sim_spec_tables(uint32_t window, double* w, double* tw) {
    const uint32_t logn = sp_logn(window);
    if (!logn) return -1;
    SpLayout y = sp_layout(0, nullptr, 0, logn);
    Heap<uint8_t> tables(y.size, kFill);
    sp_fill(y, nullptr, 0, tables.p);
    std::memcpy(w, tables.p + y.window, 8u * window);
    std::memcpy(tw, tables.p + y.twiddle, 8u * window);
    return 0;
}

// sp_check over m items of the given frames: 0 where the job can run, else 1 with the reason in msg
int sim_spec_check(const uint64_t* frames, uint32_t m, uint32_t window, char* msg, uint32_t msg_cap) {
    std::vector<SpIn> in(m);
    for (uint32_t k = 0; k < m; ++k) in[k] = SpIn{nullptr, nullptr, frames[k], 0u, 1, 16, false};
    const char* why = sp_check(in.data(), m, sp_logn(window));
    std::snprintf(msg, msg_cap, "%s", why ? why : "");
    return why ? 1 : 0;
}

// n streams as one spectrum job.  Per input i, rec[3 * i] = the plan's code for it (0: it went to the device; then)
// rec[3 * i + 1] = its rows and rec[3 * i + 2] = the status of its first failing block (0: it decoded).  rows: per item that
// decoded, in input order, its rows.  msg: the refused items' messages, '\n' between inputs.  Returns the rows written, -1
// where the job cannot be planned or rows_cap is too small.
int64_t sim_spec_streams(const uint8_t* const* lacs, const uint64_t* sizes, uint32_t n, uint32_t window, uint64_t* rec, lacx_spectrum_row* rows,
                         uint64_t rows_cap, char* msg, uint32_t msg_cap) {
    StreamJob j;
    if (!run_streams(lacs, sizes, n, window, j)) return -1;
    std::string all;
    for (uint32_t i = 0; i < n; ++i) {
        rec[3 * i] = (uint64_t)j.code[i], rec[3 * i + 1] = rec[3 * i + 2] = 0;
        all += (i ? "\n" : "") + j.err[i];
    }
    std::snprintf(msg, msg_cap, "%s", all.c_str());
    std::vector<std::vector<lacx_spectrum_row>> per(n);
    uint64_t total = 0;
    stream_results(j, [&](const PlanItem& p, uint32_t status, const std::vector<lacx_spectrum_row>& r) {
        rec[3 * p.src + 1] = r.size(), rec[3 * p.src + 2] = status;
        per[p.src] = r;
        total += r.size();
        return true;
    });
    if (total > rows_cap) return -1;
    uint64_t at = 0;
    for (uint32_t i = 0; i < n; ++i)
        for (const lacx_spectrum_row& r : per[i]) rows[at++] = r;
    return (int64_t)at;
}

// A stream case (little-endian, written by tests/spectwin.py): u32 window, u32 n, then per stream u64 size and the bytes.
// One line: "<index> <item>;<item>;..." with item = "!<code>" (refused by the plan), "x<status>" (a block failed) or
// "<rows> <hash of the rows>".
int sim_spec_line(const uint8_t* blob, uint64_t size, uint32_t index, char* line, uint32_t cap) {
    if (size < 8) return -1;
    uint32_t window, n;
    std::memcpy(&window, blob, 4);
    std::memcpy(&n, blob + 4, 4);
    std::vector<std::unique_ptr<Heap<uint8_t>>> own;  // every stream an exact allocation of its own
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
        at += sizes[i];
        lacs[i] = own.back()->p;
    }
    StreamJob j;
    if (!run_streams(lacs.data(), sizes.data(), n, window, j)) return -1;
    std::vector<std::string> item(n);
    for (uint32_t i = 0; i < n; ++i) item[i] = "!" + std::to_string(j.code[i]);
    stream_results(j, [&](const PlanItem& p, uint32_t status, const std::vector<lacx_spectrum_row>& r) {
        item[p.src] = status ? "x" + std::to_string(status) : std::to_string(r.size()) + " " + hex(fnv(r.data(), r.size() * sizeof(lacx_spectrum_row), kFnvStart));
        return true;
    });
    std::string out = std::to_string(index) + " ";
    for (uint32_t i = 0; i < n; ++i) out += (i ? ";" : "") + item[i];
    if (out.size() + 1 > cap) return -1;
    std::memcpy(line, out.c_str(), out.size() + 1);
    return 0;
}

// n items of generated PCM as one source job at one window length: item k has frames[k] frames whose sample (c, f) is
// samples[k][c * frames + f] (for a float layout the exact float of that sample at the depth), laid out as layout[k] in
// allocations that end with the source's last byte behind a base offset[k] bytes behind a 16-byte aligned address.
// bad_frame[k] != all ones: element (bad_frame, bad_channel) of a 4-byte layout is the raw word bad_word instead.  keys[k]:
// the lowest invalid sample's key (all ones: none; the item then has no rows), msg: the texts the product words them
// with, '\n' between items.  rows: the items' rows in order, counts[k] of them.  Returns the rows written, -1 where rows_cap
// is too small or the window is unsupported.
int64_t sim_spec_sources(uint32_t n, uint32_t window, const uint32_t* layout, const uint32_t* channels, const uint32_t* bit_depth, const uint32_t* offset,
                         const uint64_t* frames, const int32_t* const* samples, const uint64_t* bad_frame, const uint32_t* bad_channel,
                         const uint32_t* bad_word, lacx_spectrum_row* rows, uint64_t rows_cap, uint32_t* counts, uint64_t* keys, char* msg, uint32_t msg_cap) {
    if (!sp_logn(window)) return -1;
    std::vector<SourceSpec> spec(n);
    for (uint32_t k = 0; k < n; ++k) spec[k] = SourceSpec{layout[k], channels[k], bit_depth[k], offset[k], frames[k], samples[k], bad_frame[k], bad_channel[k], bad_word[k]};
    SourceJob j;
    run_sources(spec.data(), n, sp_logn(window), j);
    const auto* items = reinterpret_cast<const SpItem*>(j.tables->p + j.y.items);
    const auto* all = reinterpret_cast<const lacx_spectrum_row*>(j.tables->p + j.y.rows);
    std::string text;
    uint64_t at = 0;
    for (uint32_t k = 0; k < n; ++k) {
        keys[k] = j.bad[k];
        counts[k] = 0;
        if (k) text += "\n";
        if (j.bad[k] != kDigestClean) {
            text += bad_text(j.bad[k], (int)bit_depth[k]);
            continue;
        }
        if (at + items[k].rows > rows_cap) return -1;
        for (uint32_t i = 0; i < items[k].rows; ++i) rows[at++] = all[items[k].row0 + i];
        counts[k] = items[k].rows;
    }
    std::snprintf(msg, msg_cap, "%s", text.c_str());
    return (int64_t)at;
}

// spectrum_rows.h's totals through plain C (what lacx_spectrum_combine calls)
void sim_spec_combine(const lacx_spectrum_row* rows, uint32_t count, uint8_t channels, uint8_t bit_depth, uint64_t frames, uint32_t rate, uint32_t window,
                      double floor_db, lacx_spectrum* out) {
    *out = spectrum_of_rows(SpSet{rows, count, channels, bit_depth, frames, rate, window, floor_db});
}

}  // extern "C"

#ifdef SIM_SPECTRUM_MAIN
// sim_spectrum_san CASES: every case of the file (per case: a 32-bit little-endian size, a type byte, then the bytes).
// Type 0: a stream case (sim_spec_line).  Type 1: a source case of one item -- u32 window, layout, channels, bit_depth,
// offset, u64 frames, u64 bad_frame, u32 bad_channel, bad_word, i32 samples[channels * frames] -- whose line is "<index> <key>
// <rows> <hash of the rows> <message>".  "done <count>" at the end.
int main(int argc, char** argv) {
    if (argc != 2) return 2;
    std::vector<char> line(1 << 20);
    return for_each_case(argv[1], [&](const uint8_t* blob, uint32_t size, uint32_t i) {
        if (size < 1) return false;
        if (blob[0] == 0) {
            if (sim_spec_line(blob + 1, size - 1, i, line.data(), (uint32_t)line.size())) return false;
        } else {
            Reader rd{blob + 1, blob + size};
            const uint32_t window = rd.get<uint32_t>(), layout = rd.get<uint32_t>(), channels = rd.get<uint32_t>(), depth = rd.get<uint32_t>();
            const uint32_t offset = rd.get<uint32_t>();
            const uint64_t frames = rd.get<uint64_t>(), bad_frame = rd.get<uint64_t>();
            const uint32_t bad_channel = rd.get<uint32_t>(), bad_word = rd.get<uint32_t>();
            if (!rd.ok || frames == 0 || (uint64_t)(rd.end - rd.p) != 4ull * channels * frames) return false;
            Heap<int32_t> samples(channels * frames);
            std::memcpy(samples.p, rd.p, 4ull * channels * frames);
            const uint64_t cap = frames / kSpRowFrames + 1;
            std::vector<lacx_spectrum_row> rows(cap);
            const int32_t* sp = samples.p;
            uint64_t key = 0;
            uint32_t count = 0;
            char msg[256];
            if (sim_spec_sources(1, window, &layout, &channels, &depth, &offset, &frames, &sp, &bad_frame, &bad_channel, &bad_word, rows.data(), cap, &count, &key,
                                 msg, sizeof(msg)) < 0)
                return false;
            const std::string s = std::to_string(i) + " " + std::to_string(key) + " " + std::to_string(count) + " " +
                                  hex(fnv(rows.data(), (uint64_t)count * sizeof(lacx_spectrum_row), kFnvStart)) + " " + msg;
            std::snprintf(line.data(), line.size(), "%s", s.c_str());
        }
        return std::puts(line.data()) >= 0;
    });
}
#endif
