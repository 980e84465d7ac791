// api_decode.cpp -- the decode entry points of the C ABI: container parsing and the device decoder's host side.
#include "crc32_core.h"
#include "decode_plan.h"
#include "decoder_impl.h"
#include "device_buf.h"
#include "encoder_impl.h"
#include "import_msg.h"
#include "inspect_plan.h"
#include "inspect_rows.h"
#include "loudness_rows.h"
#include "runs_rows.h"
#include "spectrum_rows.h"
#include "stats_rows.h"
#include "truepeak_rows.h"

// (the entry points are declared extern "C" in lacx.h)
// ---- decode -------------------------------------------------------------------------------------
namespace {
thread_local std::string g_decode_err;
}  // namespace
namespace lacx_host {
int decode_fail(int code, const std::string& msg) {
    g_decode_err = msg;
    return code;
}
}  // namespace lacx_host

const char* lacx_decode_last_error(void) { return g_decode_err.c_str(); }

int lacx_stream_parse(const uint8_t* lac, uint64_t size, lacx_stream_info* out) {  // the container walk: decode_plan.h
    const char* why = "";
    const int c = parse_stream(lac, size, out, &why);
    return c == LACX_OK ? c : decode_fail(c, why);
}

namespace {
void decoder_release(lacx_decoder* d) {
    if (d->ready) (void)hipSetDevice(d->device);
    if (d->e0) (void)hipEventDestroy(d->e0);
    if (d->e1) (void)hipEventDestroy(d->e1);
    if (d->stream) (void)hipStreamDestroy(d->stream);
    for (Buf* b : {&d->pay, &d->stage, &d->pcm, &d->blocks, &d->image, &d->tables, &d->edit_stage, &d->edit_dst, &d->edit_tab, &d->runs_list, &d->loud}) buf_free(*b);
    *d = lacx_decoder{};
}
// lacx_decode (no handle): one decoder per device for the life of the process (never freed: releasing device memory from
// a static or thread-local destructor would race the HIP runtime's own shutdown), calls on one device take turns
struct SharedDecoder {
    std::mutex mu;
    lacx_decoder dec;
};
constexpr int kMaxDecodeDevices = 64;
std::mutex g_shared_mu;
SharedDecoder* g_shared[kMaxDecodeDevices] = {};
}  // namespace

int lacx_decoder_create(int device, lacx_decoder** out) {
    if (!out) return LACX_E_INVALID;
    lacx_decoder* d = new lacx_decoder();
    d->device = device;
    if (const char* cap = std::getenv("LACX_RUNS_LIST_CAP")) d->runs_list_cap = std::strtoull(cap, nullptr, 10);
    *out = d;
    return LACX_OK;
}

void lacx_decoder_destroy(lacx_decoder* d) {
    if (!d) return;
    decoder_release(d);
    delete d;
}

namespace {
// The 44-byte canonical header of the decoded WAV (ref src/main.cpp:127-148, 248-262).
void wav_header(const lacx_stream_info& info, uint8_t* h) {
    const uint32_t align = (uint32_t)info.channels * (info.bit_depth / 8u);
    const uint64_t data = info.frames * align, pad = data & 1u;
    auto u16 = [&](int at, uint32_t v) { h[at] = (uint8_t)v, h[at + 1] = (uint8_t)(v >> 8); };
    auto u32 = [&](int at, uint32_t v) { u16(at, v & 0xFFFFu), u16(at + 2, v >> 16); };
    std::memcpy(h, "RIFF", 4);
    u32(4, (uint32_t)(36u + data + pad));  // below 2^32: parse_stream's RIFF limit
    std::memcpy(h + 8, "WAVEfmt ", 8);
    u32(16, 16);
    u16(20, 1);
    u16(22, info.channels);
    u32(24, info.sample_rate);
    u32(28, info.sample_rate * align);
    u16(32, align);
    u16(34, info.bit_depth);
    std::memcpy(h + 36, "data", 4);
    u32(40, (uint32_t)data);
}

const char* block_error(uint32_t st) {
    static const char* const kWhat[] = {"", "block header", "channel header", "residual", "padding", "sample overflow",
                                        "trailing bytes", "sample outside the bit depth", "not reached", "residual beyond 2^30"};
    return st < 10 ? kWhat[st] : st == LACX_BLOCK_MISSING ? "payload missing" : st == LACX_BLOCK_DIGEST ? "digest mismatch" : "?";
}

// A decode job: the items (BatchIn, DecodeForm, sample type: decode_plan.h) and where the call's answers go.
struct DecodeJob {
    const BatchIn* in;
    uint32_t n;
    DecodeForm form;
    int sample_type = kWholeStreams;
    hipStream_t stream = nullptr;        // the caller's: device form, verify form against device PCM
    lacx_span* out = nullptr;            // wav form: [n] each item's image in the decoder's pinned image buffer
    lacx_verify_result* vres = nullptr;  // verify form: [n]
    float* device_ms = nullptr;
    lacx_digest* dres = nullptr;         // digest form: [n]
    bool salvage = false;                // wav and device forms: decode through errors (DecodePlan::salvage)
    lacx_salvage_result* sres = nullptr; // salvage: [n]
    bool blocks = false;                 // salvage with block digests (DecodePlan::blocks); the items' manifests in BatchIn
    bool check = false;                  // ... as a question: a fault or a truncation fails the item with LACX_E_MISMATCH
    bool stats = false;                  // salvage in the blocks form with the statistics kernel (DecodePlan::stats)
    lacx_stats* stres = nullptr;         // stats: [n]
    bool runs = false;                   // salvage in the blocks form with the run finder (DecodePlan::runs); detectors in BatchIn
    lacx_runs_result* rres = nullptr;    // runs: [n]
    bool loudness = false;               // the digest form with the loudness kernels in k_digest's place (DecodePlan::loudness)
    lacx_loudness* lres = nullptr;       // loudness: [n]
    bool truepeak = false;               // the digest form with k_truepeak in k_digest's place (DecodePlan::truepeak)
    lacx_truepeak* pres = nullptr;       // true peak: [n]
    uint32_t spectrum = 0;               // the digest form with k_spectrum in k_digest's place (DecodePlan::spectrum): the window length
    double floor_db = 0.0;               // ... the totals' floor
    lacx_spectrum* xres = nullptr;       // spectrum: [n]
    const ArJobIn* ar = nullptr;         // the digest form with k_accuraterip in k_digest's place (DecodePlan::accuraterip): the discs
    std::vector<uint32_t>* ar_planned = nullptr;  // ... those that went to the device (DecodePlan::ar_disc); the rest in d->ar_at, d->ar_sums
    const CmpJobIn* cmp = nullptr;       // the digest form with k_compare_search / k_compare_rows in k_digest's place (DecodePlan::compare): the pairs
    std::vector<uint32_t>* cmp_planned = nullptr;  // ... those that went to the device (DecodePlan::cmp_pair); the rest in d->cmp_at, d->cmp_counts, d->cmp_rows
};
static_assert(sizeof(StatsAcc) == kStatsRowBytes, "the plan lays the accumulator rows out kStatsRowBytes apart");

// What the digest kernel left for an item (DigestWords::raw), as the caller's record: the init term and the final xor
// depend on the length alone, and the image's CRC-32 follows from its parts -- header, data, pad byte.
// (crc_known: data_crc32 is the data chunk's finished CRC-32 -- the combination of block digests -- not a raw word)
lacx_digest make_digest(uint32_t raw, uint64_t frames, uint32_t sample_rate, uint8_t channels, uint8_t bit_depth, bool crc_known = false) {
    lacx_digest g{};
    g.frames = frames;
    g.data_bytes = frames * channels * (bit_depth / 8u);
    g.sample_rate = sample_rate;
    g.channels = channels;
    g.bit_depth = bit_depth;
    g.data_crc32 = crc_known ? raw : crc_finish(raw, g.data_bytes);
    const uint64_t pad = g.data_bytes & 1u;
    g.wav_valid = 36u + g.data_bytes + pad < (1ull << 32) ? 1 : 0;
    if (g.wav_valid) {
        g.wav_crc32 = crc32_combine(crc32_wav_header(channels, bit_depth, sample_rate, g.data_bytes), g.data_crc32, g.data_bytes);
        if (pad) g.wav_crc32 = crc32_combine(g.wav_crc32, crc_finish(0u, 1), 1);  // (the raw value of a zero byte is 0)
    }
    return g;
}

// The digest of an item from its block rows: the data chunk's CRC-32 is their combination, known only when every block
// decoded; otherwise the format alone, both CRCs 0 and wav_valid 0.
lacx_digest digest_of_rows(const std::vector<lacx_block_digest>& rows, uint64_t frames, uint32_t sample_rate, uint8_t channels, uint8_t bit_depth) {
    const uint32_t align = (uint32_t)channels * (bit_depth / 8u);
    uint32_t all = 0;
    bool whole = !rows.empty();
    for (size_t b = 0; b < rows.size(); ++b) {
        whole = whole && rows[b].code == 0;
        all = b ? crc32_combine(all, rows[b].crc32, (unsigned long long)rows[b].frames * align) : rows[b].crc32;
    }
    lacx_digest g = make_digest(whole ? all : 0u, frames, sample_rate, channels, bit_depth, true);
    if (!whole) g.wav_crc32 = 0, g.wav_valid = 0;
    return g;
}

}  // namespace
// ---- the steps of a run (decode_batch_run) ----
namespace lacx_host {
DevErr decoder_open(lacx_decoder* d, int* prev_device) {  // *prev_device: to put back, or -1
    *prev_device = -1;
    if (!d->ready && d->device < 0)
        if (DevErr e = chk(hipGetDevice(&d->device), "hipGetDevice")) return e;
    int cur = -1;
    if (DevErr e = chk(hipGetDevice(&cur), "hipGetDevice")) return e;
    if (cur != d->device) {
        if (DevErr e = chk(hipSetDevice(d->device), "hipSetDevice")) return e;
        *prev_device = cur;
    }
    if (!d->ready) {
        if (DevErr e = chk(hipStreamCreateWithFlags(&d->stream, hipStreamNonBlocking), "hipStreamCreate")) return e;
        if (DevErr e = chk(hipEventCreate(&d->e0), "hipEventCreate")) return e;
        if (DevErr e = chk(hipEventCreate(&d->e1), "hipEventCreate")) return e;
        d->ready = true;
    }
    return DevErr{};
}
}  // namespace lacx_host
namespace {

// What k_runs left, once the stream is idle: the lists' counters and the rows lie in h_meta (the caller copied the tables'
// tail back, or does it here: `y.lists` to the tables' end).  Where a counter outgrew its list the lists are laid out
// once more with exactly the capacities the counters gave, `again` launches the kernel over the same PCM, and *rerun is
// set.  Then the stored entries of every list come back into d->runs_host, list by list.
template <typename Again>
DevErr runs_fetch(lacx_decoder* d, RunsLayout& y, hipStream_t st, Again again, bool* rerun) {
    uint8_t* h = d->h_meta();
    const size_t tail = y.size - y.lists;
    auto back = [&] {
        if (DevErr e = chk(hipMemcpyAsync(h + y.lists, d->d_meta() + y.lists, tail, hipMemcpyDeviceToHost, st), "D2H run rows")) return e;
        return chk(hipStreamSynchronize(st), "synchronize");
    };
    if (DevErr e = back()) return e;
    *rerun = runs_overflowed(y, h);
    if (*rerun) {
        runs_recap(y, h);
        if (DevErr e = buf_grow(d->runs_list, y.list_entries, 64)) return e;
        if (DevErr e = chk(hipMemcpyAsync(d->d_meta() + y.lists, h + y.lists, sizeof(RunsList) * (size_t)y.total_dets, hipMemcpyHostToDevice, st), "H2D run lists"))
            return e;
        if (DevErr e = chk(again(d->runs_list.as<lacx_run>()), "runs launch")) return e;
        if (DevErr e = back()) return e;
    }
    const auto* lists = reinterpret_cast<const RunsList*>(h + y.lists);
    d->runs_host.assign((size_t)y.list_entries, lacx_run{});
    for (uint64_t q = 0; q < y.total_dets; ++q) {
        const uint64_t stored = lists[q].count < lists[q].cap ? lists[q].count : lists[q].cap;
        if (stored)
            if (DevErr e = chk(hipMemcpyAsync(d->runs_host.data() + lists[q].off, d->runs_list.as<lacx_run>() + lists[q].off, sizeof(lacx_run) * (size_t)stored,
                                              hipMemcpyDeviceToHost, st),
                               "D2H runs"))
                return e;
    }
    return chk(hipStreamSynchronize(st), "synchronize");
}

// The plan's capacities, each buffer with its own slack: the image buffer and the PCM buffers grow to what is asked.
DevErr ensure_capacities(lacx_decoder* d, const DecodePlan& plan) {
    const auto& need = plan.need;
    const struct {
        Buf& buf;
        uint64_t need, slack;
    } want[] = {{d->pay, need.payload, (need.payload - kDecodeTailPad) / 8},
                {d->blocks, need.blocks, need.blocks / 8 + 16},
                {d->image, need.image, 0},
                {d->pcm, need.pcm_frames, 0},
                {d->tables, need.tables, need.tables / 8 + 256},
                {d->stage, need.stage, need.stage / 8 + 4096}};
    for (const auto& w : want)
        if (w.need)
            if (DevErr e = buf_grow(w.buf, w.need, w.slack)) return e;
    return DevErr{};
}

DevErr upload_tables(lacx_decoder* d, const DecodeJob& job, const DecodePlan& plan, hipStream_t st) {
    plan_fill_tables(plan, job.in, PlanBases{d->d_pay(), d->d_left(), d->d_right(), d->d_wav()}, d->h_meta());
    return chk(hipMemcpyAsync(d->d_meta(), d->h_meta(), plan.at.size, hipMemcpyHostToDevice, st), "H2D batch tables");
}

// dst[pay_off, pay_off + pay_bytes) = every item's payload range, the destination split into equal byte ranges over up to
// 8 threads (the calling thread takes the first): a window batch is many short ranges of different streams, which as
// one pageable copy each would cost 10-20 us apiece in the runtime.
void gather_ranges(uint8_t* dst, const DecodePlan& plan, const BatchIn* in) {
    const uint64_t total = plan.total_pay;
    const unsigned hw = std::thread::hardware_concurrency();
    const unsigned nt = total < (8u << 20) ? 1u : std::max(1u, std::min(8u, hw));
    auto part = [&](unsigned t) {
        const uint64_t lo = total * t / nt, hi = total * (t + 1) / nt;
        for (const PlanItem& p : plan.items) {
            const uint64_t off = p.item.pay_off, a = std::max(lo, off), b = std::min(hi, off + p.pay_bytes);
            if (a < b) std::memcpy(dst + a, in[p.src].lac + p.head + p.pay_src + (a - off), b - a);
        }
    };
    std::vector<std::thread> pool;
    unsigned t = 1;
    try {
        for (; t < nt; ++t) pool.emplace_back(part, t);
    } catch (...) {  // no thread to be had: the calling thread copies what is left
        for (unsigned u = t; u < nt; ++u) part(u);
    }
    part(0);
    for (auto& th : pool) th.join();
}

DevErr upload_payload(lacx_decoder* d, const DecodeJob& job, const DecodePlan& plan, hipStream_t st) {
    if (plan.window()) {  // the windows' ranges through the pinned stage: one copy
        gather_ranges(d->h_pay(), plan, job.in);
        if (DevErr e = chk(hipMemcpyAsync(d->d_pay(), d->h_pay(), plan.total_pay, hipMemcpyHostToDevice, st), "H2D payload")) return e;
    } else {
        for (const PlanItem& p : plan.items)
            if (p.pay_bytes)  // (a salvage item whose first block is cut has none)
                if (DevErr e = chk(hipMemcpyAsync(d->d_pay() + p.item.pay_off, job.in[p.src].lac + p.head, p.pay_bytes, hipMemcpyHostToDevice, st),
                                   "H2D payload"))
                    return e;
    }
    if (DevErr e = chk(hipMemsetAsync(d->d_pay() + plan.total_pay, 0, kDecodeTailPad, st), "memset")) return e;  // the bit reader's look-ahead
    if (!plan.host_src) return DevErr{};
    return chk(hipMemcpyAsync(d->d_pay() + plan.src_at, plan.host_src, plan.host_src_bytes, hipMemcpyHostToDevice, st), "H2D source");
}

// The kernels of a compare job whose tables (y, compare_plan.h) lie filled at d->d_meta() and d->h_meta(): where a pair has a
// radius the search, its counts back, the host's choice of the offsets and the pairs and row offsets to the device again --
// the second round trip -- then the rows.  y leaves with the choice.
DevErr compare_kernels(lacx_decoder* d, CmpLayout& y, unsigned long long* bad, hipStream_t st) {
    if (y.search) {
        if (DevErr e = chk(launch_compare_search(cmp_args(y, d->d_meta(), bad), st), "compare search launch")) return e;
        if (DevErr e = chk(hipMemcpyAsync(d->h_meta() + y.counts, d->d_meta() + y.counts, 8 * (size_t)y.total_counts, hipMemcpyDeviceToHost, st), "D2H compare counts"))
            return e;
        if (DevErr e = chk(hipStreamSynchronize(st), "synchronize")) return e;
        cmp_choose_all(y, reinterpret_cast<const unsigned long long*>(d->h_meta() + y.counts));
        cmp_fill_choice(y, d->h_meta());
        if (DevErr e = chk(hipMemcpyAsync(d->d_meta() + y.pairs, d->h_meta() + y.pairs, y.choice_bytes(), hipMemcpyHostToDevice, st), "H2D compare choice")) return e;
    }
    return chk(launch_compare_rows(cmp_args(y, d->d_meta(), bad), st), "compare rows launch");
}
// ... and its rows back (queued): 96 bytes per 16384 frames of a domain, inside the tables
DevErr compare_fetch(lacx_decoder* d, const CmpLayout& y, hipStream_t st) {
    if (!y.rows_cap) return DevErr{};
    return chk(hipMemcpyAsync(d->h_meta() + y.rows, d->d_meta() + y.rows, (size_t)kCmpRowBytes * (size_t)y.rows_cap, hipMemcpyDeviceToHost, st), "D2H compare rows");
}
// ... and what the item calls give, out of the host's copy of the tables
void compare_keep(lacx_decoder* d, const CmpLayout& y) {
    const auto* counts = reinterpret_cast<const uint64_t*>(d->h_meta() + y.counts);
    d->cmp_counts.assign(counts, counts + y.total_counts);
    const auto* rows = reinterpret_cast<const lacx_compare_row*>(d->h_meta() + y.rows);
    d->cmp_rows.assign(rows, rows + y.rows_cap);
}

// The kernels between the decoder's two events, then what every form reads back, and the wait for it.
DevErr launch_and_wait(lacx_decoder* d, const DecodeJob& job, const DecodePlan& plan, hipStream_t st, bool* runs_rerun) {
    const DecodeArgs a = plan_args(plan, d->d_meta(), d->d_pay(), d->d_status(), d->d_ms());
    const size_t res = plan.at.res, m = plan.items.size();
    if (DevErr e = chk(hipEventRecord(d->e0, st), "event record")) return e;
    if (DevErr e = chk(launch_decode(a, st), "decode launch")) return e;
    if (plan.stats)  // behind k_ms_inverse, every block's status final: the slot k_digest_blocks has in a digest job
        if (DevErr e = chk(launch_stats_blocks(plan_stats_args(plan, a, d->d_meta()), st), "stats launch")) return e;
    if (plan.runs)  // in the same slot
        if (DevErr e = chk(launch_runs(plan_runs_args(plan, a, d->d_meta(), d->runs_list.as<lacx_run>()), st), "runs launch")) return e;
    if (plan.loudness)  // behind k_ms_inverse: the slot k_digest has in a digest job
        if (DevErr e = chk(launch_loudness(plan_loud_args(plan, d->d_meta(), d->loud.as<uint8_t>()), st), "loudness launch")) return e;
    if (plan.truepeak)  // in the same slot
        if (DevErr e = chk(launch_truepeak(plan_peak_args(plan, d->d_meta()), st), "true peak launch")) return e;
    if (plan.spectrum)  // likewise
        if (DevErr e = chk(launch_spectrum(plan_spec_args(plan, d->d_meta()), st), "spectrum launch")) return e;
    if (plan.accuraterip)  // likewise
        if (DevErr e = chk(launch_accuraterip(plan_ar_args(plan, d->d_meta()), st), "rip checksum launch")) return e;
    if (plan.compare) {  // likewise, in two round trips where a pair has a radius
        d->cmp_at = plan.cmp_at;
        if (DevErr e = compare_kernels(d, d->cmp_at, nullptr, st)) return e;
    }
    if (DevErr e = chk(hipEventRecord(d->e1, st), "event record")) return e;
    if (plan.compare)
        if (DevErr e = compare_fetch(d, d->cmp_at, st)) return e;
    if (plan.accuraterip && plan.ar_at.total_sums)  // the sums: 12 bytes per track and offset, inside the tables
        if (DevErr e = chk(hipMemcpyAsync(d->h_meta() + plan.ar_at.sums, d->d_meta() + plan.ar_at.sums, 4 * (size_t)plan.ar_at.total_sums, hipMemcpyDeviceToHost, st),
                           "D2H rip checksums"))
            return e;
    if (plan.truepeak && plan.peak_at.total_rows)  // the rows: 32 bytes per 16384 frames, inside the tables
        if (DevErr e = chk(hipMemcpyAsync(d->h_meta() + plan.peak_at.rows, d->d_meta() + plan.peak_at.rows, sizeof(TpAcc) * (size_t)plan.peak_at.total_rows,
                                          hipMemcpyDeviceToHost, st),
                           "D2H true peak rows"))
            return e;
    if (plan.spectrum && plan.spec_at.total_rows)  // the rows: 1024 bytes per 16384 frames, inside the tables
        if (DevErr e = chk(hipMemcpyAsync(d->h_meta() + plan.spec_at.rows, d->d_meta() + plan.spec_at.rows, sizeof(lacx_spectrum_row) * (size_t)plan.spec_at.total_rows,
                                          hipMemcpyDeviceToHost, st),
                           "D2H spectrum rows"))
            return e;
    if (plan.loudness && plan.loud_at.total_rows) {  // the rows: 16 bytes per sub-block
        d->loud_host.resize((size_t)plan.loud_at.total_rows);
        if (DevErr e = chk(hipMemcpyAsync(d->loud_host.data(), d->loud.as<uint8_t>() + plan.loud_at.rows, sizeof(lacx_loudness_row) * d->loud_host.size(),
                                          hipMemcpyDeviceToHost, st),
                           "D2H loudness rows"))
            return e;
    }
    if (DevErr e = chk(hipMemcpyAsync(d->h_status(), d->d_status(), (size_t)plan.total_blocks * sizeof(uint32_t), hipMemcpyDeviceToHost, st), "D2H status"))
        return e;
    // the images of the items that decoded are valid whatever the others did: one copy for all
    if (plan.form == DecodeForm::wav)
        if (DevErr e = chk(hipMemcpyAsync(d->h_wav(), d->d_wav(), plan.image_total, hipMemcpyDeviceToHost, st), "D2H WAV images")) return e;
    // the verify form's whole answer: 32 bytes per item
    if (plan.form == DecodeForm::verify)
        if (DevErr e = chk(hipMemcpyAsync(d->h_meta() + res, d->d_meta() + res, sizeof(VerifyWords) * m, hipMemcpyDeviceToHost, st), "D2H verify results"))
            return e;
    // the digest form's whole answer: 8 bytes per item
    if (plan.form == DecodeForm::digest && !plan.loudness && !plan.truepeak && !plan.spectrum && !plan.accuraterip && !plan.compare)
        if (DevErr e = chk(hipMemcpyAsync(d->h_meta() + res, d->d_meta() + res, sizeof(DigestWords) * m, hipMemcpyDeviceToHost, st), "D2H digests"))
            return e;
    // block digests: 4 bytes per block beside the statuses
    if (plan.blocks && plan.total_blocks)
        if (DevErr e = chk(hipMemcpyAsync(d->h_meta() + plan.at.raw, d->d_meta() + plan.at.raw, 4 * (size_t)plan.total_blocks, hipMemcpyDeviceToHost, st),
                           "D2H block digests"))
            return e;
    // statistics: kStatsRowBytes per block beside the statuses
    if (plan.stats && plan.total_blocks)
        if (DevErr e = chk(hipMemcpyAsync(d->h_meta() + plan.at.stats, d->d_meta() + plan.at.stats, kStatsRowBytes * (size_t)plan.need.stats_rows,
                                          hipMemcpyDeviceToHost, st),
                           "D2H statistics"))
            return e;
    if (DevErr e = chk(hipStreamSynchronize(st), "synchronize")) return e;
    if (job.device_ms) (void)hipEventElapsedTime(job.device_ms, d->e0, d->e1);
    if (plan.runs) {
        RunsLayout y = plan.runs_at;
        y.list_entries = plan.need.runs_list;
        const RunsArgs r = plan_runs_args(plan, a, d->d_meta(), nullptr);
        return runs_fetch(d, y, st, [&](lacx_run* list) {
            RunsArgs again = r;
            again.runs = list;
            return launch_runs(again, st);
        }, runs_rerun);
    }
    return DevErr{};
}

// Per item: its first failing block, else what its form gives back.
DevErr collect(lacx_decoder* d, const DecodeJob& job, const DecodePlan& plan, hipStream_t st, std::vector<int>& code,
               std::vector<std::string>& err, bool runs_rerun) {
    const bool host = plan.form == DecodeForm::host;
    if (plan.accuraterip) {  // a disc's answer needs all of its items: the caller puts it together from these
        d->ar_at = plan.ar_at;
        const auto* sums = reinterpret_cast<const uint32_t*>(d->h_meta() + plan.ar_at.sums);
        d->ar_sums.assign(sums, sums + plan.ar_at.total_sums);
        if (job.ar_planned) *job.ar_planned = plan.ar_disc;
    }
    if (plan.compare) {  // a pair's answer needs both of its items: the caller puts it together from these
        compare_keep(d, d->cmp_at);
        if (job.cmp_planned) *job.cmp_planned = plan.cmp_pair;
    }
    for (size_t j = 0; j < plan.items.size(); ++j) {
        const PlanItem& p = plan.items[j];
        const BatchIn& x = job.in[p.src];
        const uint32_t i = p.src;
        if (plan.salvage) {  // every block's outcome, not the first: the status words and present_blocks are the whole report
            const lacx_salvage_result r = salvage_report(p, x.lac, d->h_status(), d->item_faults[i]);
            if (job.sres) job.sres[i] = r;
            if (plan.stats) {  // the rows: every block's frames and, where it decoded, its statistics; the totals from the rows
                const StatsAcc* acc = reinterpret_cast<const StatsAcc*>(d->h_meta() + plan.at.stats) + p.item.block0;
                std::vector<lacx_block_stats>& rows = d->item_stats[i];
                stats_rows_of_decoded(x.lac, p.info.version, p.item.blocks, p.info.channels, d->item_faults[i], acc, rows);
                if (job.stres) job.stres[i] = stats_combine(rows.data(), (uint32_t)rows.size(), p.info.channels, p.info.bit_depth, p.info.sample_rate);
            }
            if (plan.runs) {  // the lists: stitched from the rows, merged with what the kernel appended
                lacx_runs_result res = runs_item_result(plan.runs_at, d->h_meta(), d->runs_host.data(), j, p.item.frames, d->item_runs[i]);
                res.lost_frames = r.lost_frames, res.sample_rate = p.info.sample_rate, res.blocks = r.blocks, res.lost_blocks = r.bad_blocks;
                res.flags = runs_rerun ? LACX_RUNS_RERUN : 0u;
                res.channels = p.info.channels, res.bit_depth = p.info.bit_depth;
                if (job.rres) job.rres[i] = res;
            }
            if (plan.blocks) {  // the rows: every block's frames and, where it decoded, its finished CRC-32
                const uint32_t* raw = reinterpret_cast<const uint32_t*>(d->h_meta() + plan.at.raw) + p.item.block0;
                std::vector<lacx_block_digest>& rows = d->item_rows[i];
                rows_of_decoded(x.lac, p.info.version, p.item.blocks, p.info.channels, p.info.bit_depth, d->item_faults[i], raw, rows);
                if (job.dres) job.dres[i] = digest_of_rows(rows, p.info.frames, p.info.sample_rate, p.info.channels, p.info.bit_depth);
                if (job.check && (r.bad_blocks || (r.flags & LACX_SALVAGE_TRUNCATED))) {
                    code[i] = LACX_E_MISMATCH;
                    err[i] = "[check-error] block=" + std::to_string(r.first_bad) + " " +
                             block_error(r.bad_blocks ? d->item_faults[i][0].code : LACX_BLOCK_MISSING) + " bad_blocks=" + std::to_string(r.bad_blocks);
                }
            }
            if (plan.form == DecodeForm::wav) {
                uint8_t* img = d->h_wav() + p.image_at;
                wav_header(p.info, img);
                if (job.out) job.out[i] = lacx_span{img, p.image_size};
            }
            continue;
        }
        for (uint32_t b = 0; b < p.item.blocks; ++b) {
            const uint32_t sv = d->h_status()[p.item.block0 + b];
            if (sv) {  // the item's first failing block, like the reference's message (lac/decoder.cpp:24-32)
                code[i] = LACX_E_RUNTIME;
                err[i] = "[decode-error] block=" + std::to_string(p.blk_first + b) + " " + block_error(sv);
                break;
            }
        }
        if (code[i] != LACX_OK) continue;
        if (plan.loudness) {  // the item's rows, and the totals from the rows
            const LoudItem& li = reinterpret_cast<const LoudItem*>(d->h_meta() + plan.loud_at.items)[j];
            std::vector<lacx_loudness_row>& rows = d->item_loud[i];
            if (li.rows) rows.assign(d->loud_host.begin() + (size_t)li.row0, d->loud_host.begin() + (size_t)(li.row0 + li.rows));
            if (job.lres) job.lres[i] = loudness_of_rows(rows.data(), (uint32_t)rows.size(), p.info.channels, p.info.bit_depth, p.info.sample_rate);
        } else if (plan.truepeak) {  // likewise
            const TpItem& ti = reinterpret_cast<const TpItem*>(d->h_meta() + plan.peak_at.items)[j];
            std::vector<lacx_truepeak_row>& rows = d->item_peak[i];
            truepeak_rows_of(reinterpret_cast<const TpAcc*>(d->h_meta() + plan.peak_at.rows) + ti.row0, ti.rows, rows);
            if (job.pres) job.pres[i] = truepeak_of_rows(TpSet{rows.data(), (uint32_t)rows.size(), p.info.channels, p.info.bit_depth, p.info.frames, p.info.sample_rate});
        } else if (plan.spectrum) {  // likewise
            const SpItem& si = reinterpret_cast<const SpItem*>(d->h_meta() + plan.spec_at.items)[j];
            std::vector<lacx_spectrum_row>& rows = d->item_spec[i];
            const auto* all = reinterpret_cast<const lacx_spectrum_row*>(d->h_meta() + plan.spec_at.rows);
            rows.assign(all + si.row0, all + si.row0 + si.rows);
            if (job.xres) job.xres[i] = spectrum_of_rows(SpSet{rows.data(), (uint32_t)rows.size(), p.info.channels, p.info.bit_depth, p.info.frames, p.info.sample_rate, plan.spectrum, job.floor_db});
        } else if (plan.accuraterip) {  // (per disc, not per item)
        } else if (plan.compare) {      // (per pair, not per item)
        } else if (plan.form == DecodeForm::digest) {
            const DigestWords& w = reinterpret_cast<const DigestWords*>(d->h_meta() + plan.at.res)[j];
            if (job.dres) job.dres[i] = make_digest(w.raw, p.info.frames, p.info.sample_rate, p.info.channels, p.info.bit_depth);
        } else if (plan.form == DecodeForm::verify) {
            const VerifyWords& w = reinterpret_cast<const VerifyWords*>(d->h_meta() + plan.at.res)[j];
            if (w.count == 0) continue;
            lacx_verify_result r{};
            r.mismatches = w.count;
            r.frame = w.key >> 1;
            r.block = w.block;
            r.channel = (uint8_t)(w.key & 1u);
            r.decoded = w.decoded;
            r.source = w.source;
            if (job.vres) job.vres[i] = r;
            code[i] = LACX_E_MISMATCH;
            err[i] = "[verify-error] block=" + std::to_string(r.block) + " channel=" + (r.channel ? "right" : "left") +
                     " frame=" + std::to_string(r.frame) + " decoded=" + std::to_string(r.decoded) +
                     " source=" + std::to_string(r.source) + " mismatches=" + std::to_string(r.mismatches);
        } else if (plan.form == DecodeForm::wav) {
            uint8_t* img = d->h_wav() + p.image_at;
            wav_header(p.info, img);
            if (job.out) job.out[i] = lacx_span{img, p.image_size};
        } else if (host) {  // the two channels leave on two streams' worth of copy engine time: issue, then wait
            const uint64_t bytes = 4 * (plan.window() ? p.win.frames : p.item.frames);
            const uint8_t* stage = d->d_wav() + p.image_at;  // a window's samples: left, then right
            const void* left = plan.window() ? (const void*)stage : d->d_left() + p.pcm_at;
            const void* right = plan.window() ? (const void*)(stage + bytes) : d->d_right() + p.pcm_at;
            if (DevErr e = chk(hipMemcpyAsync(x.left, left, bytes, hipMemcpyDeviceToHost, st), "D2H left")) return e;
            if (p.item.channels == 2)
                if (DevErr e = chk(hipMemcpyAsync(x.right, right, bytes, hipMemcpyDeviceToHost, st), "D2H right")) return e;
        }
    }
    return host ? chk(hipStreamSynchronize(st), "synchronize") : DevErr{};
}

// The decoder: n streams as one decode (a single stream is n = 1), planned on the host (plan_decode: the per-item checks,
// the layout), then run as one device job.  Per item, code[i] and err[i] ("" = decoded): the message its decode gives.
// Returns LACX_OK, or LACX_E_DEVICE for a failure of the whole call (every item that passed its checks then carries it).
// The caller decides what the outcome becomes: the batch entry points keep it in d->item_err.
int decode_batch_run(lacx_decoder* d, const DecodeJob& job, std::vector<int>& code, std::vector<std::string>& err) {
    if (job.device_ms) *job.device_ms = 0.f;
    if (job.vres) std::memset(job.vres, 0, sizeof(lacx_verify_result) * job.n);
    if (job.dres) std::memset(job.dres, 0, sizeof(lacx_digest) * job.n);
    if (job.sres) std::memset(job.sres, 0, sizeof(lacx_salvage_result) * job.n);
    if (job.salvage) d->item_faults.assign(job.n, {});
    if (job.blocks) d->item_rows.assign(job.n, {});
    if (job.stres) std::memset(job.stres, 0, sizeof(lacx_stats) * job.n);
    if (job.stats) d->item_stats.assign(job.n, {});
    if (job.rres) std::memset(job.rres, 0, sizeof(lacx_runs_result) * job.n);
    if (job.runs) d->item_runs.assign(job.n, {});
    if (job.lres) std::memset(job.lres, 0, sizeof(lacx_loudness) * job.n);
    if (job.loudness) d->item_loud.assign(job.n, {});
    if (job.pres) std::memset(job.pres, 0, sizeof(lacx_truepeak) * job.n);
    if (job.truepeak) d->item_peak.assign(job.n, {});
    if (job.xres) std::memset(job.xres, 0, sizeof(lacx_spectrum) * job.n);
    if (job.spectrum) d->item_spec.assign(job.n, {});
    // LACX_DECODE_BATCH_PAD=1 (tuning knob, read per call): every item's blocks start a new wave
    const char* pad_env = std::getenv("LACX_DECODE_BATCH_PAD");
    DecodePlan plan;
    const char* whole = plan_decode_job(job.in, job.n, job.form, job.sample_type, pad_env && pad_env[0] == '1', plan, code, err, job.salvage, job.blocks, job.stats,
                                    job.runs, d->runs_list_cap ? d->runs_list_cap : kRunsListCap, job.loudness, job.truepeak, job.spectrum, job.ar, job.cmp);
    if (lacx_device_count() <= 0) whole = "no usable HIP device";
    int rc = whole ? decode_fail(LACX_E_DEVICE, whole) : LACX_OK;
    if (!whole && !plan.items.empty()) {
        int prev_device = -1;
        DevErr e = decoder_open(d, &prev_device);
        // (d->stream: created by decoder_open)
        hipStream_t st = job.form == DecodeForm::device || job.form == DecodeForm::digest || job.form == DecodeForm::blocks || (job.form == DecodeForm::verify && !plan.host_src) ? job.stream : d->stream;
        if (!e) e = ensure_capacities(d, plan);
        if (!e) e = upload_tables(d, job, plan, st);
        if (!e) e = upload_payload(d, job, plan, st);
        bool runs_rerun = false;
        if (!e && plan.runs) e = buf_grow(d->runs_list, plan.need.runs_list, plan.need.runs_list / 8 + 64);
        if (!e && plan.loudness) e = buf_grow(d->loud, (plan.need.loud_scratch + 15u) / 16u, plan.need.loud_scratch / 128u + 64);
        if (!e) e = launch_and_wait(d, job, plan, st, &runs_rerun);
        if (!e) e = collect(d, job, plan, st, code, err, runs_rerun);
        if (prev_device >= 0) (void)hipSetDevice(prev_device);
        if (e) rc = decode_fail(LACX_E_DEVICE, std::string(e.what) + ": " + hipGetErrorString(e.e));
    }
    if (rc != LACX_OK) {  // the whole call failed: no item decoded
        if (job.sres) std::memset(job.sres, 0, sizeof(lacx_salvage_result) * job.n);
        if (job.salvage) d->item_faults.assign(job.n, {});
        if (job.blocks) d->item_rows.assign(job.n, {});
        if (job.stats) d->item_stats.assign(job.n, {});
        if (job.stres) std::memset(job.stres, 0, sizeof(lacx_stats) * job.n);
        if (job.runs) d->item_runs.assign(job.n, {});
        if (job.rres) std::memset(job.rres, 0, sizeof(lacx_runs_result) * job.n);
        if (job.loudness) d->item_loud.assign(job.n, {});
        if (job.lres) std::memset(job.lres, 0, sizeof(lacx_loudness) * job.n);
        if (job.truepeak) d->item_peak.assign(job.n, {});
        if (job.pres) std::memset(job.pres, 0, sizeof(lacx_truepeak) * job.n);
        if (job.spectrum) d->item_spec.assign(job.n, {});
        if (job.xres) std::memset(job.xres, 0, sizeof(lacx_spectrum) * job.n);
        if (job.dres) std::memset(job.dres, 0, sizeof(lacx_digest) * job.n);
        for (uint32_t i = 0; i < job.n; ++i) {
            if (code[i] != LACX_OK) continue;
            code[i] = rc;
            err[i] = g_decode_err;
        }
    }
    for (uint32_t i = 0; job.out && i < job.n; ++i)
        if (code[i] != LACX_OK) job.out[i] = lacx_span{nullptr, 0};
    return rc;
}

// How a batch entry point ends: the per-item outcome into item_rc and d->item_err, and back the lowest failing item's
// code with "stream i: <message>" (or rc, the whole call's failure).
int batch_outcome(lacx_decoder* d, int rc, const std::vector<int>& code, std::vector<std::string>& err, int* item_rc) {
    if (item_rc) std::copy(code.begin(), code.end(), item_rc);
    d->item_err = std::move(err);
    if (rc != LACX_OK) return rc;
    for (size_t i = 0; i < code.size(); ++i)
        if (code[i] != LACX_OK) return decode_fail(code[i], "stream " + std::to_string(i) + ": " + d->item_err[i]);
    return LACX_OK;
}

// A copy of a view for the caller to free; null where the host is out of memory.
uint8_t* owned_copy(const uint8_t* data, uint64_t size) {
    uint8_t* buf = static_cast<uint8_t*>(std::malloc(size));
    if (buf) std::memcpy(buf, data, size);
    return buf;
}

// A batch entry point: runs the job and ends as batch_outcome says.
int run_batch(lacx_decoder* d, const DecodeJob& job, int* item_rc) {
    std::vector<int> code;
    std::vector<std::string> err;
    const int rc = decode_batch_run(d, job, code, err);
    return batch_outcome(d, rc, code, err, item_rc);
}

// A single stream as a batch of one: its own code and message.  d->item_err keeps the last batch call's.
int run_one(lacx_decoder* d, const BatchIn& in, DecodeJob job) {
    job.in = &in;
    job.n = 1;
    std::vector<int> code;
    std::vector<std::string> err;
    (void)decode_batch_run(d, job, code, err);
    return code[0] == LACX_OK ? LACX_OK : decode_fail(code[0], err[0]);
}
}  // namespace

int lacx_decoder_decode(lacx_decoder* d, const uint8_t* lac, uint64_t size, int32_t* left, int32_t* right, uint64_t frames,
                        float* device_ms) {
    if (!d) return decode_fail(LACX_E_INVALID, "null decoder");
    return run_one(d, BatchIn{lac, size, left, right, frames}, DecodeJob{nullptr, 1, DecodeForm::host, kWholeStreams, nullptr, nullptr, nullptr, device_ms});
}

int lacx_decoder_decode_wav_view(lacx_decoder* d, const uint8_t* lac, uint64_t size, const uint8_t** out, uint64_t* out_size,
                                 float* device_ms) {
    if (out) *out = nullptr;
    if (out_size) *out_size = 0;
    if (!d) return decode_fail(LACX_E_INVALID, "null decoder");
    if (!out || !out_size) return decode_fail(LACX_E_INVALID, "null argument");
    lacx_span img{nullptr, 0};
    const int rc = run_one(d, BatchIn{lac, size, nullptr, nullptr, 0}, DecodeJob{nullptr, 1, DecodeForm::wav, kWholeStreams, nullptr, &img, nullptr, device_ms});
    if (rc) return rc;
    *out = img.data;  // the start of d->h_wav: a batch of one
    *out_size = img.size;
    return LACX_OK;
}

int lacx_decoder_decode_wav(lacx_decoder* d, const uint8_t* lac, uint64_t size, uint8_t** out, uint64_t* out_size,
                            float* device_ms) {
    if (out) *out = nullptr;
    if (out_size) *out_size = 0;
    if (!out || !out_size) return decode_fail(LACX_E_INVALID, "null argument");
    const uint8_t* view = nullptr;
    uint64_t n = 0;
    const int rc = lacx_decoder_decode_wav_view(d, lac, size, &view, &n, device_ms);
    if (rc) return rc;
    uint8_t* buf = owned_copy(view, n);
    if (!buf) return decode_fail(LACX_E_RUNTIME, "out of host memory");
    *out = buf;
    *out_size = n;
    return LACX_OK;
}

int lacx_decoder_decode_wav_batch_view(lacx_decoder* d, const lacx_span* lacs, uint32_t n, lacx_span* out, int* item_rc,
                                       float* device_ms) {
    if (!d) return decode_fail(LACX_E_INVALID, "null decoder");
    if (!lacs || !out || n == 0) return decode_fail(LACX_E_INVALID, "null argument or empty batch");
    std::vector<BatchIn> in(n);
    for (uint32_t i = 0; i < n; ++i) in[i] = BatchIn{lacs[i].data, lacs[i].size, nullptr, nullptr, 0};
    return run_batch(d, DecodeJob{in.data(), n, DecodeForm::wav, kWholeStreams, nullptr, out, nullptr, device_ms}, item_rc);
}

int lacx_decoder_decode_wav_batch(lacx_decoder* d, const lacx_span* lacs, uint32_t n, lacx_span* out, int* item_rc,
                                  float* device_ms) {
    const int rc = lacx_decoder_decode_wav_batch_view(d, lacs, n, out, item_rc, device_ms);
    if (!out || !lacs || n == 0 || !d) return rc;
    for (uint32_t i = 0; i < n; ++i) {
        if (!out[i].data) continue;
        uint8_t* buf = owned_copy(out[i].data, out[i].size);
        if (!buf) {
            for (uint32_t k = 0; k < i; ++k) {
                std::free(const_cast<uint8_t*>(out[k].data));
                out[k] = lacx_span{nullptr, 0};
            }
            for (uint32_t k = i; k < n; ++k) out[k] = lacx_span{nullptr, 0};
            return decode_fail(LACX_E_RUNTIME, "out of host memory");
        }
        out[i].data = buf;
    }
    return rc;
}

int lacx_decoder_decode_batch_device(lacx_decoder* d, const lacx_decode_item* items, uint32_t n, void* stream, int* item_rc,
                                     float* device_ms) {
    if (!d) return decode_fail(LACX_E_INVALID, "null decoder");
    if (!items || n == 0) return decode_fail(LACX_E_INVALID, "null argument or empty batch");
    std::vector<BatchIn> in(n);
    for (uint32_t i = 0; i < n; ++i) in[i] = BatchIn{items[i].lac, items[i].size, items[i].left, items[i].right, items[i].frames};
    return run_batch(d, DecodeJob{in.data(), n, DecodeForm::device, kWholeStreams, static_cast<hipStream_t>(stream), nullptr, nullptr, device_ms}, item_rc);
}

int lacx_decoder_decode_window_batch_device(lacx_decoder* d, const lacx_window_item* items, uint32_t n, int sample_type,
                                            void* stream, int* item_rc, float* device_ms) {
    if (!d) return decode_fail(LACX_E_INVALID, "null decoder");
    if (!items || n == 0) return decode_fail(LACX_E_INVALID, "null argument or empty batch");
    if (sample_type != LACX_SAMPLE_I32 && sample_type != LACX_SAMPLE_F32) return decode_fail(LACX_E_INVALID, "unknown sample type");
    std::vector<BatchIn> in(n);
    for (uint32_t i = 0; i < n; ++i)
        in[i] = BatchIn{items[i].lac, items[i].size, static_cast<int32_t*>(items[i].left), static_cast<int32_t*>(items[i].right),
                        items[i].frames, items[i].start};
    return run_batch(d, DecodeJob{in.data(), n, DecodeForm::device, sample_type, static_cast<hipStream_t>(stream), nullptr, nullptr, device_ms}, item_rc);
}

int lacx_decoder_decode_window(lacx_decoder* d, const uint8_t* lac, uint64_t size, uint64_t start, uint64_t frames,
                               int sample_type, void* left, void* right, float* device_ms) {
    if (!d) return decode_fail(LACX_E_INVALID, "null decoder");
    if (sample_type != LACX_SAMPLE_I32 && sample_type != LACX_SAMPLE_F32) return decode_fail(LACX_E_INVALID, "unknown sample type");
    return run_one(d, BatchIn{lac, size, static_cast<int32_t*>(left), static_cast<int32_t*>(right), frames, start},
                   DecodeJob{nullptr, 1, DecodeForm::host, sample_type, nullptr, nullptr, nullptr, device_ms});
}

int lacx_decoder_verify_batch_device(lacx_decoder* d, const lacx_verify_item* items, uint32_t n, void* stream, int* item_rc,
                                     lacx_verify_result* results, float* device_ms) {
    if (!d) return decode_fail(LACX_E_INVALID, "null decoder");
    if (!items || n == 0) return decode_fail(LACX_E_INVALID, "null argument or empty batch");
    std::vector<BatchIn> in(n);
    for (uint32_t i = 0; i < n; ++i) {
        in[i] = BatchIn{items[i].lac, items[i].size, nullptr, nullptr, items[i].frames};
        in[i].pcm = items[i].pcm;
    }
    return run_batch(d, DecodeJob{in.data(), n, DecodeForm::verify, kWholeStreams, static_cast<hipStream_t>(stream), nullptr, results, device_ms}, item_rc);
}

// A WAV file image in host memory against a stream: the formats are compared on the host (a difference is an answer
// that needs no device), then the data chunk goes to the device as it is, 2 or 3 bytes per sample, and is compared
// there as an interleaved source -- a batch of one.  No PCM comes back.
int lacx_decoder_verify_wav(lacx_decoder* d, const uint8_t* lac, uint64_t size, const uint8_t* wav, uint64_t wav_size,
                            lacx_verify_result* result, float* device_ms) {
    if (device_ms) *device_ms = 0.f;
    if (result) std::memset(result, 0, sizeof(*result));
    if (!d) return decode_fail(LACX_E_INVALID, "null decoder");
    if (!wav) return decode_fail(LACX_E_INVALID, "null argument");
    lacx_stream_info info;
    const int prc = lacx_stream_parse(lac, size, &info);
    if (prc != LACX_OK) return prc;
    lacx_wav_info w;
    if (lacx_wav_parse(wav, wav_size, &w) != LACX_OK) return decode_fail(LACX_E_INVALID, "[verify-error] source is not a PCM WAV file the encoder reads");
    auto differs = [](const char* field, uint64_t a, uint64_t b) {
        return decode_fail(LACX_E_MISMATCH, std::string("[verify-error] ") + field + ": stream " + std::to_string(a) + ", source " + std::to_string(b));
    };
    if (w.channels != info.channels) return differs("channels", info.channels, w.channels);
    if (w.bit_depth != info.bit_depth) return differs("bit depth", info.bit_depth, w.bit_depth);
    if (w.sample_rate != info.sample_rate) return differs("sample rate", info.sample_rate, w.sample_rate);
    if (w.frames != info.frames) return differs("frames", info.frames, w.frames);
    BatchIn in{lac, size, nullptr, nullptr, w.frames};
    in.pcm = lacx_pcm{nullptr, nullptr, w.bit_depth == 16 ? LACX_PCM_INTERLEAVED_I16 : LACX_PCM_INTERLEAVED_I24, w.channels};
    in.host_src = wav + w.data_offset;
    in.host_src_bytes = w.frames * w.channels * (uint64_t)(w.bit_depth / 8);
    return run_one(d, in, DecodeJob{nullptr, 1, DecodeForm::verify, kWholeStreams, nullptr, nullptr, result, device_ms});
}

int lacx_decoder_digest_batch_device(lacx_decoder* d, const lacx_span* lacs, uint32_t n, void* stream, int* item_rc, lacx_digest* out,
                                     float* device_ms) {
    if (!d) return decode_fail(LACX_E_INVALID, "null decoder");
    if (!lacs || n == 0) return decode_fail(LACX_E_INVALID, "null argument or empty batch");
    std::vector<BatchIn> in(n);
    for (uint32_t i = 0; i < n; ++i) in[i] = BatchIn{lacs[i].data, lacs[i].size, nullptr, nullptr, 0};
    return run_batch(d, DecodeJob{in.data(), n, DecodeForm::digest, kWholeStreams, static_cast<hipStream_t>(stream), nullptr, nullptr, device_ms, out},
                     item_rc);
}

namespace {
// The source form's checks of an item, in the verify form's words where it has them.
const char* check_digest_source(const lacx_digest_source& x, std::string& text) {
    const lacx_pcm& p = x.pcm;
    const uintptr_t a0 = (uintptr_t)p.data0, a1 = (uintptr_t)p.data1;
    const bool tensor = p.layout == LACX_PCM_PLANAR_I16 || p.layout == LACX_PCM_PLANAR_F32 || p.layout == LACX_PCM_INTERLEAVED_F32;
    const bool planar = p.layout == LACX_PCM_PLANAR_I32 || p.layout == LACX_PCM_PLANAR_I16 || p.layout == LACX_PCM_PLANAR_F32;
    if (p.layout > LACX_PCM_INTERLEAVED_I24 && !tensor) return "unknown source layout";
    if (p.channels != 1 && p.channels != 2) return "unsupported channel count";
    if (!p.data0 || (planar && p.channels == 2 && !p.data1)) return "source arrays missing";
    if (x.frames == 0) return "source has no frames";
    if (x.frames >> 56) return "source frame count out of range";
    if (!rate_ok(x.sample_rate)) return (text = "unsupported sample rate: " + std::to_string(x.sample_rate)).c_str();
    if (x.bit_depth != 16 && x.bit_depth != 24) return (text = "unsupported bit depth: " + std::to_string((int)x.bit_depth)).c_str();
    if (((p.layout == LACX_PCM_INTERLEAVED_I16 || p.layout == LACX_PCM_PLANAR_I16) && x.bit_depth != 16) ||
        (p.layout == LACX_PCM_INTERLEAVED_I24 && x.bit_depth != 24))
        return "source layout does not match the stream's bit depth";
    if (p.layout == LACX_PCM_PLANAR_I16) {
        if ((a0 & 1u) || (planar && p.channels == 2 && (a1 & 1u))) return "source arrays are not 2-byte aligned";
    } else if ((p.layout != LACX_PCM_INTERLEAVED_I24 && (a0 & 3u)) || (planar && p.channels == 2 && (a1 & 3u))) {
        return "source arrays are not 4-byte aligned";
    }
    return nullptr;
}

// The source form: no stream, no decode -- the items' records and the prefix sums of their unit counts in the decoder's
// table buffers, k_digest over them on the caller's stream, and 16 bytes per item back (the result word and the lowest
// invalid sample's key).  Table layout: src [m] | unit_off [m + 1] | res [m] | bad [m].
// grid != 0: block digests on a regular grid of `grid` frames instead (k_digest_blocks); the tables then go on with
// | block_off [m + 1] | raw [blocks], and every item's rows are left in d->item_rows.
// stats (with a grid): the audio statistics on that grid instead (k_stats_blocks) -- in place of the raw words the
// accumulator rows | acc [blocks] (StatsAcc, 16-byte aligned, zeroed), the rows left in d->item_stats, the totals in sout.
// runs (without a grid): the run finder instead (k_runs) -- behind bad [m] the tables of runs_plan.h (16-byte aligned), the
// lists in the decoder's list buffer, every item's lists left in d->item_runs, the totals in runs->out.
// loud (without a grid): the loudness kernels instead (launch_loudness) -- behind bad [m] the tables of loudness_plan.h
// (16-byte aligned), the scratch in the decoder's own buffer, every item's rows left in d->item_loud, the totals in loud->out.
// peak (without a grid): k_truepeak instead -- behind bad [m] the tables of truepeak_plan.h (16-byte aligned, zeroed rows
// included), every item's rows left in d->item_peak, the totals in peak->out.
// spec (without a grid): k_spectrum instead -- behind bad [m] the tables of spectrum_plan.h (window, twiddles and zeroed rows
// included), every item's rows left in d->item_spec, the totals in spec->out.
struct LoudPcm {
    lacx_loudness* out;
};
struct PeakPcm {
    lacx_truepeak* out;
};
struct SpecPcm {
    lacx_spectrum* out;
    uint32_t window;  // a supported length
    double floor_db;
};
struct RunsPcm {
    std::vector<BatchIn> in;  // per item its detectors, or why they are refused (BatchIn::dets, ndet, dets_why)
    lacx_runs_result* out;
};
int digest_pcm_run(lacx_decoder* d, const lacx_digest_source* src, uint32_t n, hipStream_t st, lacx_digest* out, float* device_ms,
                   std::vector<int>& code, std::vector<std::string>& err, uint32_t grid = 0, bool stats = false, lacx_stats* sout = nullptr,
                   const RunsPcm* runs = nullptr, const LoudPcm* loud = nullptr, const PeakPcm* peak = nullptr,
                   const SpecPcm* spec = nullptr) {
    if (device_ms) *device_ms = 0.f;
    if (spec && spec->out) std::memset(spec->out, 0, sizeof(lacx_spectrum) * n);
    if (spec) d->item_spec.assign(n, {});
    if (peak && peak->out) std::memset(peak->out, 0, sizeof(lacx_truepeak) * n);
    if (peak) d->item_peak.assign(n, {});
    if (loud && loud->out) std::memset(loud->out, 0, sizeof(lacx_loudness) * n);
    if (loud) d->item_loud.assign(n, {});
    if (runs && runs->out) std::memset(runs->out, 0, sizeof(lacx_runs_result) * n);
    if (runs) d->item_runs.assign(n, {});
    if (out) std::memset(out, 0, sizeof(lacx_digest) * n);
    if (sout) std::memset(sout, 0, sizeof(lacx_stats) * n);
    code.assign(n, LACX_OK);
    err.assign(n, std::string());
    std::vector<uint32_t> went;  // the items that go to the device
    for (uint32_t i = 0; i < n; ++i) {
        std::string text;
        const char* why = check_digest_source(src[i], text);
        if (!why && runs) why = runs->in[i].dets_why;
        if (why) {
            code[i] = LACX_E_INVALID;
            err[i] = why;
        } else {
            went.push_back(i);
        }
    }
    int rc = lacx_device_count() <= 0 ? decode_fail(LACX_E_DEVICE, "no usable HIP device") : LACX_OK;
    const size_t m = went.size();
    if (grid && !stats) d->item_rows.assign(n, {});
    if (stats) d->item_stats.assign(n, {});
    unsigned long long nblocks = 0;
    for (size_t j = 0; grid && j < m; ++j) nblocks += (src[went[j]].frames + grid - 1u) / grid;
    if (rc == LACX_OK && nblocks >= (1ull << 31)) rc = decode_fail(LACX_E_DEVICE, "batch holds 2^31 blocks or more");
    if (rc == LACX_OK && m) {
        const size_t at_off = sizeof(DigestSource) * m, at_res = at_off + 8 * (m + 1), at_bad = at_res + sizeof(DigestWords) * m,
                     at_blk = at_bad + 8 * m, at_raw = stats ? plan_detail::up16(at_blk + 8 * (m + 1)) : at_blk + (grid ? 8 * (m + 1) : 0),
                     size0 = at_raw + (stats ? sizeof(StatsAcc) : 4) * (size_t)nblocks;
        std::vector<RunsIn> rin;
        for (size_t j = 0; runs && j < m; ++j) rin.push_back(RunsIn{runs->in[went[j]].dets, runs->in[went[j]].ndet, src[went[j]].frames});
        RunsLayout y = runs ? runs_layout(plan_detail::up16(at_blk), rin.data(), m) : RunsLayout{};
        std::vector<LoudIn> lin;
        for (size_t j = 0; loud && j < m; ++j) {
            const lacx_digest_source& x = src[went[j]];
            lin.push_back(LoudIn{x.pcm.data0, x.pcm.data1, x.frames, x.sample_rate, x.pcm.layout, (uint8_t)x.pcm.channels, x.bit_depth, true});
        }
        const LoudLayout ly = loud ? loud_layout(plan_detail::up16(at_blk), lin.data(), m) : LoudLayout{};
        std::vector<TpIn> tin;
        for (size_t j = 0; peak && j < m; ++j) {
            const lacx_digest_source& x = src[went[j]];
            tin.push_back(TpIn{x.pcm.data0, x.pcm.data1, x.frames, x.pcm.layout, (uint8_t)x.pcm.channels, x.bit_depth, true});
        }
        const TpLayout ty = peak ? tp_layout(plan_detail::up16(at_blk), tin.data(), m) : TpLayout{};
        std::vector<SpIn> xin;
        for (size_t j = 0; spec && j < m; ++j) {
            const lacx_digest_source& x = src[went[j]];
            xin.push_back(SpIn{x.pcm.data0, x.pcm.data1, x.frames, x.pcm.layout, (uint8_t)x.pcm.channels, x.bit_depth, true});
        }
        const SpLayout sy = spec ? sp_layout(plan_detail::up16(at_blk), xin.data(), m, sp_logn(spec->window)) : SpLayout{};
        const size_t size = spec ? sy.size : peak ? ty.size : loud ? ly.size : runs ? y.size : size0;
        int prev_device = -1;
        DevErr e = decoder_open(d, &prev_device);
        if (!e && loud)
            if (const char* why = loud_check(lin.data(), m)) rc = decode_fail(LACX_E_DEVICE, why);
        if (!e && loud && rc == LACX_OK) e = buf_grow(d->loud, (ly.scratch + 15u) / 16u, ly.scratch / 128u + 64);
        if (!e && peak)
            if (const char* why = tp_check(tin.data(), m)) rc = decode_fail(LACX_E_DEVICE, why);
        if (!e && spec)
            if (const char* why = sp_check(xin.data(), m, sy.logn)) rc = decode_fail(LACX_E_DEVICE, why);
        if (!e && y.total_tiles >= (1ull << 31)) rc = decode_fail(LACX_E_DEVICE, "batch holds 2^31 tiles or more");
        if (!e) e = buf_grow(d->tables, size, size / 8 + 256);
        if (!e && runs && rc == LACX_OK) {
            runs_fill(y, rin.data(), m, d->runs_list_cap ? d->runs_list_cap : kRunsListCap, d->h_meta());
            e = buf_grow(d->runs_list, y.list_entries, y.list_entries / 8 + 64);
        }
        bool runs_rerun = false;
        if (!e && rc == LACX_OK) {
            auto* hs = reinterpret_cast<DigestSource*>(d->h_meta());
            auto* unit_off = reinterpret_cast<unsigned long long*>(d->h_meta() + at_off);
            auto* block_off = reinterpret_cast<unsigned long long*>(d->h_meta() + at_blk);
            unit_off[0] = 0;
            if (grid) {
                block_off[0] = 0;
                for (size_t j = 0; j < m; ++j) block_off[j + 1] = block_off[j] + (src[went[j]].frames + grid - 1u) / grid;
                std::memset(d->h_meta() + at_raw, 0, size - at_raw);
            }
            for (size_t j = 0; j < m; ++j) {
                const lacx_digest_source& x = src[went[j]];
                hs[j] = DigestSource{x.pcm.data0, x.pcm.channels == 2 ? x.pcm.data1 : nullptr, x.frames, x.pcm.layout, (uint8_t)x.pcm.channels,
                                     x.bit_depth, {0, 0}};
                unit_off[j + 1] = unit_off[j] + (x.frames + 3u) / 4u;
                reinterpret_cast<DigestWords*>(d->h_meta() + at_res)[j] = DigestWords{0, 0};
                reinterpret_cast<unsigned long long*>(d->h_meta() + at_bad)[j] = kDigestClean;
            }
            if (loud) loud_fill(ly, lin.data(), m, d->h_meta());
            if (peak) tp_fill(ty, tin.data(), m, d->h_meta());
            if (spec) sp_fill(sy, xin.data(), m, d->h_meta());
            DigestPcmArgs a;
            a.nitems = (uint32_t)m;
            a.total_units = unit_off[m];
            a.unit_off = reinterpret_cast<const unsigned long long*>(d->d_meta() + at_off);
            a.src = reinterpret_cast<const DigestSource*>(d->d_meta());
            a.res = reinterpret_cast<DigestWords*>(d->d_meta() + at_res);
            a.bad = reinterpret_cast<unsigned long long*>(d->d_meta() + at_bad);
            e = chk(hipMemcpyAsync(d->d_meta(), d->h_meta(), size, hipMemcpyHostToDevice, st), "H2D digest tables");
            if (!e) e = chk(hipEventRecord(d->e0, st), "event record");
            BlockPcmArgs ba;
            ba.pcm = a;
            ba.grid = grid;
            ba.block_off = reinterpret_cast<const unsigned long long*>(d->d_meta() + at_blk);
            ba.raw = reinterpret_cast<uint32_t*>(d->d_meta() + at_raw);
            StatsPcmArgs sa;
            sa.pcm = a;
            sa.grid = grid;
            sa.block_off = ba.block_off;
            sa.rows = reinterpret_cast<StatsAcc*>(d->d_meta() + at_raw);
            RunsArgs ra;
            if (runs) {
                runs_args(y, m, d->d_meta(), d->runs_list.as<lacx_run>(), ra);
                ra.src = a.src;
                ra.bad = a.bad;
            }
            if (!e && loud) e = chk(launch_loudness(loud_args(ly, m, d->d_meta(), d->loud.as<uint8_t>(), a.bad), st), "loudness launch");
            if (!e && peak) e = chk(launch_truepeak(tp_args(ty, m, d->d_meta(), a.bad), st), "true peak launch");
            if (!e && spec) e = chk(launch_spectrum(sp_args(sy, m, d->d_meta(), a.bad), st), "spectrum launch");
            if (!e && !loud && !peak && !spec) e = runs ? chk(launch_runs_pcm(ra, st), "runs launch") : stats ? chk(launch_stats_pcm_blocks(sa, st), "stats launch") : chk(grid ? launch_digest_pcm_blocks(ba, st) : launch_digest_pcm(a, st), "digest launch");
            if (!e) e = chk(hipEventRecord(d->e1, st), "event record");
            if (!e) e = chk(hipMemcpyAsync(d->h_meta() + at_res, d->d_meta() + at_res, (runs || loud || peak || spec ? at_blk : size) - at_res, hipMemcpyDeviceToHost, st), "D2H digests");
            if (!e && spec && sy.total_rows)
                e = chk(hipMemcpyAsync(d->h_meta() + sy.rows, d->d_meta() + sy.rows, sizeof(lacx_spectrum_row) * (size_t)sy.total_rows, hipMemcpyDeviceToHost, st), "D2H spectrum rows");
            if (!e && peak && ty.total_rows)
                e = chk(hipMemcpyAsync(d->h_meta() + ty.rows, d->d_meta() + ty.rows, sizeof(TpAcc) * (size_t)ty.total_rows, hipMemcpyDeviceToHost, st), "D2H true peak rows");
            if (!e && loud && ly.total_rows) {
                d->loud_host.resize((size_t)ly.total_rows);
                e = chk(hipMemcpyAsync(d->loud_host.data(), d->loud.as<uint8_t>() + ly.rows, sizeof(lacx_loudness_row) * d->loud_host.size(), hipMemcpyDeviceToHost, st),
                        "D2H loudness rows");
            }
            if (!e) e = chk(hipStreamSynchronize(st), "synchronize");
            if (!e && device_ms) (void)hipEventElapsedTime(device_ms, d->e0, d->e1);
            if (!e && runs)
                e = runs_fetch(d, y, st, [&](lacx_run* list) {
                    ra.runs = list;
                    return launch_runs_pcm(ra, st);
                }, &runs_rerun);
        }
        if (prev_device >= 0) (void)hipSetDevice(prev_device);
        if (e) {
            rc = decode_fail(LACX_E_DEVICE, std::string(e.what) + ": " + hipGetErrorString(e.e));
        } else if (rc == LACX_OK) {
            for (size_t j = 0; j < m; ++j) {
                const uint32_t i = went[j];
                const lacx_digest_source& x = src[i];
                const unsigned long long key = reinterpret_cast<const unsigned long long*>(d->h_meta() + at_bad)[j];
                if (key != kDigestClean) {  // the encoder's words for it (import_msg.h): all of left first, then right
                    ImportBad b{{kImportClean, kImportClean}};
                    b.key[key >> 63] = key & ~(1ull << 63);
                    int ch = 0;
                    unsigned long long index = 0;
                    (void)import_bad_message(b, x.bit_depth, &ch, &index, err[i]);
                    code[i] = LACX_E_INVALID;
                    continue;
                }
                if (loud) {
                    const LoudItem& li = reinterpret_cast<const LoudItem*>(d->h_meta() + ly.items)[j];
                    std::vector<lacx_loudness_row>& rows = d->item_loud[i];
                    if (li.rows) rows.assign(d->loud_host.begin() + (size_t)li.row0, d->loud_host.begin() + (size_t)(li.row0 + li.rows));
                    if (loud->out) loud->out[i] = loudness_of_rows(rows.data(), (uint32_t)rows.size(), (uint8_t)x.pcm.channels, x.bit_depth, x.sample_rate);
                    continue;
                }
                if (peak) {
                    const TpItem& ti = reinterpret_cast<const TpItem*>(d->h_meta() + ty.items)[j];
                    std::vector<lacx_truepeak_row>& rows = d->item_peak[i];
                    truepeak_rows_of(reinterpret_cast<const TpAcc*>(d->h_meta() + ty.rows) + ti.row0, ti.rows, rows);
                    if (peak->out) peak->out[i] = truepeak_of_rows(TpSet{rows.data(), (uint32_t)rows.size(), (uint8_t)x.pcm.channels, x.bit_depth, x.frames, x.sample_rate});
                    continue;
                }
                if (spec) {
                    const SpItem& si = reinterpret_cast<const SpItem*>(d->h_meta() + sy.items)[j];
                    std::vector<lacx_spectrum_row>& rows = d->item_spec[i];
                    const auto* all = reinterpret_cast<const lacx_spectrum_row*>(d->h_meta() + sy.rows);
                    rows.assign(all + si.row0, all + si.row0 + si.rows);
                    if (spec->out) spec->out[i] = spectrum_of_rows(SpSet{rows.data(), (uint32_t)rows.size(), (uint8_t)x.pcm.channels, x.bit_depth, x.frames, x.sample_rate, spec->window, spec->floor_db});
                    continue;
                }
                if (runs) {
                    lacx_runs_result res = runs_item_result(y, d->h_meta(), d->runs_host.data(), j, x.frames, d->item_runs[i]);
                    res.sample_rate = x.sample_rate, res.blocks = (uint32_t)((x.frames + kMaxBlock - 1u) / kMaxBlock);
                    res.flags = runs_rerun ? LACX_RUNS_RERUN : 0u;
                    res.channels = (uint8_t)x.pcm.channels, res.bit_depth = x.bit_depth;
                    if (runs->out) runs->out[i] = res;
                    continue;
                }
                if (stats) {
                    const auto* block_off = reinterpret_cast<const unsigned long long*>(d->h_meta() + at_blk);
                    const StatsAcc* acc = reinterpret_cast<const StatsAcc*>(d->h_meta() + at_raw) + block_off[j];
                    std::vector<lacx_block_stats>& rows = d->item_stats[i];
                    stats_rows_of_source(x.frames, grid, (uint32_t)(block_off[j + 1] - block_off[j]), (uint32_t)x.pcm.channels, acc, rows);
                    if (sout) sout[i] = stats_combine(rows.data(), (uint32_t)rows.size(), (uint8_t)x.pcm.channels, x.bit_depth, x.sample_rate);
                    continue;
                }
                if (grid) {
                    const auto* block_off = reinterpret_cast<const unsigned long long*>(d->h_meta() + at_blk);
                    const uint32_t* braw = reinterpret_cast<const uint32_t*>(d->h_meta() + at_raw) + block_off[j];
                    std::vector<lacx_block_digest>& rows = d->item_rows[i];
                    rows_of_source(x.frames, grid, (uint32_t)(block_off[j + 1] - block_off[j]), (uint32_t)x.pcm.channels, x.bit_depth, braw, rows);
                    if (out) out[i] = digest_of_rows(rows, x.frames, x.sample_rate, (uint8_t)x.pcm.channels, x.bit_depth);
                    continue;
                }
                const uint32_t raw = reinterpret_cast<const DigestWords*>(d->h_meta() + at_res)[j].raw;
                if (out) out[i] = make_digest(raw, x.frames, x.sample_rate, (uint8_t)x.pcm.channels, x.bit_depth);
            }
        }
    }
    if (rc != LACX_OK) {  // the whole call failed: no item was digested
        if (grid && !stats) d->item_rows.assign(n, {});
        if (stats) d->item_stats.assign(n, {});
        if (sout) std::memset(sout, 0, sizeof(lacx_stats) * n);
        if (runs) d->item_runs.assign(n, {});
        if (runs && runs->out) std::memset(runs->out, 0, sizeof(lacx_runs_result) * n);
        if (loud) d->item_loud.assign(n, {});
        if (loud && loud->out) std::memset(loud->out, 0, sizeof(lacx_loudness) * n);
        if (peak) d->item_peak.assign(n, {});
        if (peak && peak->out) std::memset(peak->out, 0, sizeof(lacx_truepeak) * n);
        if (spec) d->item_spec.assign(n, {});
        if (spec && spec->out) std::memset(spec->out, 0, sizeof(lacx_spectrum) * n);
        for (uint32_t i = 0; i < n; ++i) {
            if (code[i] != LACX_OK) continue;
            code[i] = rc;
            err[i] = g_decode_err;
        }
    }
    return rc;
}
}  // namespace

int lacx_decoder_digest_pcm_batch_device(lacx_decoder* d, const lacx_digest_source* src, uint32_t n, void* stream, int* item_rc,
                                         lacx_digest* out, float* device_ms) {
    if (!d) return decode_fail(LACX_E_INVALID, "null decoder");
    if (!src || n == 0) return decode_fail(LACX_E_INVALID, "null argument or empty batch");
    std::vector<int> code;
    std::vector<std::string> err;
    const int rc = digest_pcm_run(d, src, n, static_cast<hipStream_t>(stream), out, device_ms, code, err);
    return batch_outcome(d, rc, code, err, item_rc);
}

// ---- salvage: decode through errors (lacx.h) ----
int lacx_stream_scan(const uint8_t* lac, uint64_t size, lacx_stream_info* info, uint32_t* present_blocks, uint32_t* flags) {
    const char* why = "";
    const int c = scan_stream(lac, size, info, present_blocks, flags, &why);
    return c == LACX_OK ? c : decode_fail(c, why);
}

namespace {
DecodeJob salvage_job(DecodeForm form, hipStream_t stream, lacx_span* out, lacx_salvage_result* results, float* device_ms) {
    DecodeJob job{nullptr, 0, form, kWholeStreams, stream, out, nullptr, device_ms};
    job.salvage = true;
    job.sres = results;
    return job;
}
}  // namespace

int lacx_decoder_salvage_wav_batch_view(lacx_decoder* d, const lacx_span* lacs, uint32_t n, lacx_span* out, int* item_rc,
                                        lacx_salvage_result* results, float* device_ms) {
    if (!d) return decode_fail(LACX_E_INVALID, "null decoder");
    if (!lacs || !out || n == 0) return decode_fail(LACX_E_INVALID, "null argument or empty batch");
    std::vector<BatchIn> in(n);
    for (uint32_t i = 0; i < n; ++i) in[i] = BatchIn{lacs[i].data, lacs[i].size, nullptr, nullptr, 0};
    DecodeJob job = salvage_job(DecodeForm::wav, nullptr, out, results, device_ms);
    job.in = in.data();
    job.n = n;
    return run_batch(d, job, item_rc);
}

int lacx_decoder_salvage_wav(lacx_decoder* d, const uint8_t* lac, uint64_t size, uint8_t** out, uint64_t* out_size,
                             lacx_salvage_result* result, float* device_ms) {
    if (out) *out = nullptr;
    if (out_size) *out_size = 0;
    if (result) std::memset(result, 0, sizeof(*result));
    if (!d) return decode_fail(LACX_E_INVALID, "null decoder");
    if (!out || !out_size) return decode_fail(LACX_E_INVALID, "null argument");
    lacx_span img{nullptr, 0};
    const int rc = run_one(d, BatchIn{lac, size, nullptr, nullptr, 0}, salvage_job(DecodeForm::wav, nullptr, &img, result, device_ms));
    if (rc) return rc;
    uint8_t* buf = owned_copy(img.data, img.size);
    if (!buf) return decode_fail(LACX_E_RUNTIME, "out of host memory");
    *out = buf;
    *out_size = img.size;
    return LACX_OK;
}

int lacx_decoder_salvage_batch_device(lacx_decoder* d, const lacx_decode_item* items, uint32_t n, void* stream, int* item_rc,
                                      lacx_salvage_result* results, float* device_ms) {
    if (!d) return decode_fail(LACX_E_INVALID, "null decoder");
    if (!items || n == 0) return decode_fail(LACX_E_INVALID, "null argument or empty batch");
    std::vector<BatchIn> in(n);
    for (uint32_t i = 0; i < n; ++i) in[i] = BatchIn{items[i].lac, items[i].size, items[i].left, items[i].right, items[i].frames};
    DecodeJob job = salvage_job(DecodeForm::device, static_cast<hipStream_t>(stream), nullptr, results, device_ms);
    job.in = in.data();
    job.n = n;
    return run_batch(d, job, item_rc);
}

// ---- block digests and manifests (lacx.h) ----
namespace {
// a salvage job with block digests: the blocks form (nothing is output), or a salvage form with manifests
int run_blocks(lacx_decoder* d, std::vector<BatchIn>& in, const lacx_span* manifests, DecodeJob job, int* item_rc) {
    for (size_t i = 0; manifests && i < in.size(); ++i) in[i].manifest = manifests[i].data, in[i].manifest_size = manifests[i].size;
    job.in = in.data();
    job.n = (uint32_t)in.size();
    job.blocks = true;
    return run_batch(d, job, item_rc);
}
}  // namespace

int lacx_decoder_digest_blocks_batch_device(lacx_decoder* d, const lacx_span* lacs, uint32_t n, void* stream, int* item_rc, lacx_digest* out,
                                            float* device_ms) {
    if (!d) return decode_fail(LACX_E_INVALID, "null decoder");
    if (!lacs || n == 0) return decode_fail(LACX_E_INVALID, "null argument or empty batch");
    std::vector<BatchIn> in(n);
    for (uint32_t i = 0; i < n; ++i) in[i] = BatchIn{lacs[i].data, lacs[i].size, nullptr, nullptr, 0};
    DecodeJob job = salvage_job(DecodeForm::blocks, static_cast<hipStream_t>(stream), nullptr, nullptr, device_ms);
    job.dres = out;
    return run_blocks(d, in, nullptr, job, item_rc);
}

int lacx_decoder_check_batch_device(lacx_decoder* d, const lacx_span* lacs, const lacx_span* manifests, uint32_t n, void* stream, int* item_rc,
                                    lacx_salvage_result* results, float* device_ms) {
    if (!d) return decode_fail(LACX_E_INVALID, "null decoder");
    if (!lacs || !manifests || n == 0) return decode_fail(LACX_E_INVALID, "null argument or empty batch");
    std::vector<BatchIn> in(n);
    for (uint32_t i = 0; i < n; ++i) in[i] = BatchIn{lacs[i].data, lacs[i].size, nullptr, nullptr, 0};
    DecodeJob job = salvage_job(DecodeForm::blocks, static_cast<hipStream_t>(stream), nullptr, results, device_ms);
    job.check = true;
    return run_blocks(d, in, manifests, job, item_rc);
}

int lacx_decoder_salvage_wav_batch_view_checked(lacx_decoder* d, const lacx_span* lacs, const lacx_span* manifests, uint32_t n, lacx_span* out,
                                                int* item_rc, lacx_salvage_result* results, float* device_ms) {
    if (!d) return decode_fail(LACX_E_INVALID, "null decoder");
    if (!lacs || !manifests || !out || n == 0) return decode_fail(LACX_E_INVALID, "null argument or empty batch");
    std::vector<BatchIn> in(n);
    for (uint32_t i = 0; i < n; ++i) in[i] = BatchIn{lacs[i].data, lacs[i].size, nullptr, nullptr, 0};
    return run_blocks(d, in, manifests, salvage_job(DecodeForm::wav, nullptr, out, results, device_ms), item_rc);
}

int lacx_decoder_salvage_batch_device_checked(lacx_decoder* d, const lacx_decode_item* items, const lacx_span* manifests, uint32_t n, void* stream,
                                              int* item_rc, lacx_salvage_result* results, float* device_ms) {
    if (!d) return decode_fail(LACX_E_INVALID, "null decoder");
    if (!items || !manifests || n == 0) return decode_fail(LACX_E_INVALID, "null argument or empty batch");
    std::vector<BatchIn> in(n);
    for (uint32_t i = 0; i < n; ++i) in[i] = BatchIn{items[i].lac, items[i].size, items[i].left, items[i].right, items[i].frames};
    return run_blocks(d, in, manifests, salvage_job(DecodeForm::device, static_cast<hipStream_t>(stream), nullptr, results, device_ms), item_rc);
}

int lacx_decoder_digest_pcm_blocks_batch_device(lacx_decoder* d, const lacx_digest_source* src, uint32_t n, uint32_t block_frames, void* stream,
                                                int* item_rc, lacx_digest* out, float* device_ms) {
    if (!d) return decode_fail(LACX_E_INVALID, "null decoder");
    if (!src || n == 0) return decode_fail(LACX_E_INVALID, "null argument or empty batch");
    if (block_frames != 0 && (block_frames < 256u || block_frames > (uint32_t)kMaxBlock)) return decode_fail(LACX_E_INVALID, "block_frames must be 0 or 256..16384");
    std::vector<int> code;
    std::vector<std::string> err;
    const int rc = digest_pcm_run(d, src, n, static_cast<hipStream_t>(stream), out, device_ms, code, err, block_frames ? block_frames : (uint32_t)kMaxBlock);
    return batch_outcome(d, rc, code, err, item_rc);
}

int lacx_decoder_item_block_digests(const lacx_decoder* d, uint32_t i, const lacx_block_digest** rows, uint32_t* count) {
    if (rows) *rows = nullptr;
    if (count) *count = 0;
    if (!d || !rows || !count) return decode_fail(LACX_E_INVALID, "null argument");
    if (i >= d->item_rows.size()) return decode_fail(LACX_E_INVALID, "no such item in the last block digest call");
    *rows = d->item_rows[i].data();
    *count = (uint32_t)d->item_rows[i].size();
    return LACX_OK;
}

// ---- audio statistics (lacx.h) ----
int lacx_decoder_stats_batch_device(lacx_decoder* d, const lacx_span* lacs, uint32_t n, void* stream, int* item_rc, lacx_stats* out,
                                    float* device_ms) {
    if (!d) return decode_fail(LACX_E_INVALID, "null decoder");
    if (!lacs || n == 0) return decode_fail(LACX_E_INVALID, "null argument or empty batch");
    std::vector<BatchIn> in(n);
    for (uint32_t i = 0; i < n; ++i) in[i] = BatchIn{lacs[i].data, lacs[i].size, nullptr, nullptr, 0};
    DecodeJob job = salvage_job(DecodeForm::blocks, static_cast<hipStream_t>(stream), nullptr, nullptr, device_ms);
    job.in = in.data();
    job.n = n;
    job.stats = true;
    job.stres = out;
    return run_batch(d, job, item_rc);
}

int lacx_decoder_stats_pcm_batch_device(lacx_decoder* d, const lacx_digest_source* src, uint32_t n, uint32_t block_frames, void* stream,
                                        int* item_rc, lacx_stats* out, float* device_ms) {
    if (!d) return decode_fail(LACX_E_INVALID, "null decoder");
    if (!src || n == 0) return decode_fail(LACX_E_INVALID, "null argument or empty batch");
    if (block_frames != 0 && (block_frames < 256u || block_frames > (uint32_t)kMaxBlock)) return decode_fail(LACX_E_INVALID, "block_frames must be 0 or 256..16384");
    std::vector<int> code;
    std::vector<std::string> err;
    const int rc = digest_pcm_run(d, src, n, static_cast<hipStream_t>(stream), nullptr, device_ms, code, err, block_frames ? block_frames : (uint32_t)kMaxBlock,
                                  true, out);
    return batch_outcome(d, rc, code, err, item_rc);
}

int lacx_decoder_item_block_stats(const lacx_decoder* d, uint32_t i, const lacx_block_stats** rows, uint32_t* count) {
    if (rows) *rows = nullptr;
    if (count) *count = 0;
    if (!d || !rows || !count) return decode_fail(LACX_E_INVALID, "null argument");
    if (i >= d->item_stats.size()) return decode_fail(LACX_E_INVALID, "no such item in the last stats call");
    *rows = d->item_stats[i].data();
    *count = (uint32_t)d->item_stats[i].size();
    return LACX_OK;
}

int lacx_stats_combine(const lacx_block_stats* rows, uint32_t count, uint8_t channels, uint8_t bit_depth, uint32_t sample_rate, lacx_stats* out) {
    if (out) std::memset(out, 0, sizeof(*out));
    if (!out || (!rows && count)) return decode_fail(LACX_E_INVALID, "null argument");
    if (channels != 1 && channels != 2) return decode_fail(LACX_E_INVALID, "unsupported channel count");
    if (bit_depth != 16 && bit_depth != 24) return decode_fail(LACX_E_INVALID, "unsupported bit depth: " + std::to_string((int)bit_depth));
    *out = stats_combine(rows, count, channels, bit_depth, sample_rate);
    return LACX_OK;
}

// ---- stream inspection (lacx.h) ----
namespace {
// An inspection job: planned by plan_inspect (a salvage job's items and tables, none of its decode), run as the decoder
// runs its jobs -- tables and payload up, k_inspect / k_inspect_serial between the two events, the rows back.
int inspect_run(lacx_decoder* d, const BatchIn* in, uint32_t n, bool partitions, hipStream_t st, lacx_stream_report* out, float* device_ms,
                std::vector<int>& code, std::vector<std::string>& err) {
    if (device_ms) *device_ms = 0.f;
    if (out) std::memset(out, 0, sizeof(lacx_stream_report) * n);
    auto clear = [&] {
        d->item_info.assign(n, {});
        d->info_mode_k.clear();
        d->info_part_bits.clear();
        d->info_block0.assign(n, ~0u);
    };
    clear();
    d->info_guard = d->info_guard_changed = 0;
    const char* pad_env = std::getenv("LACX_DECODE_BATCH_PAD");
    // LACX_INSPECT_GUARD=1 (diagnostic, read per call): the tables buffer is made larger than the plan asks by a guard --
    // 4096 bytes, and for a job without partition detail the bytes the partition entries of its blocks would take -- that
    // is filled with kGuardByte before the kernels run and read back behind them (lacx_decoder_inspect_guard)
    const char* guard_env = std::getenv("LACX_INSPECT_GUARD");
    constexpr int kGuardByte = 0xA5;
    InspectPlan plan;
    const char* whole = plan_inspect(in, n, partitions, pad_env && pad_env[0] == '1', plan, code, err);
    if (lacx_device_count() <= 0) whole = "no usable HIP device";
    int rc = whole ? decode_fail(LACX_E_DEVICE, whole) : LACX_OK;
    const DecodePlan& base = plan.base;
    if (!whole && !base.items.empty()) {
        DecodeJob job{in, n, DecodeForm::blocks};
        const size_t T = (size_t)base.total_blocks;
        const uint64_t guard = guard_env && guard_env[0] == '1'
                                   ? 4096u + (partitions ? 0u : (kInspectPartModeBytes + kInspectPartBitsBytes) * (uint64_t)T + 16u)
                                   : 0u;
        int prev_device = -1;
        DevErr e = decoder_open(d, &prev_device);
        if (!e && guard) e = buf_grow(d->tables, plan.need.tables + guard, 0);
        if (!e) e = ensure_capacities(d, base);
        if (!e) e = upload_tables(d, job, base, st);
        if (!e) e = upload_payload(d, job, base, st);
        if (!e && guard) e = chk(hipMemsetAsync(d->d_meta() + plan.need.tables, kGuardByte, guard, st), "memset");
        if (!e) e = chk(hipEventRecord(d->e0, st), "event record");
        if (!e) e = chk(launch_inspect(plan_inspect_args(plan, d->d_meta(), d->d_pay()), st), "inspect launch");
        if (!e) e = chk(hipEventRecord(d->e1, st), "event record");
        if (!e) e = chk(hipMemcpyAsync(d->h_meta() + plan.at_rows, d->d_meta() + plan.at_rows, plan.need.tables + guard - plan.at_rows, hipMemcpyDeviceToHost, st),
                        "D2H inspection rows");
        if (!e) e = chk(hipStreamSynchronize(st), "synchronize");
        if (!e && device_ms) (void)hipEventElapsedTime(device_ms, d->e0, d->e1);
        if (prev_device >= 0) (void)hipSetDevice(prev_device);
        if (!e && guard) {
            d->info_guard = guard;
            for (uint64_t k = 0; k < guard; ++k) d->info_guard_changed += d->h_meta()[plan.need.tables + k] != (uint8_t)kGuardByte;
        }
        if (e) {
            rc = decode_fail(LACX_E_DEVICE, std::string(e.what) + ": " + hipGetErrorString(e.e));
        } else if (d->info_guard_changed) {
            rc = decode_fail(LACX_E_DEVICE, "inspection wrote " + std::to_string(d->info_guard_changed) + " bytes behind its tables");
        } else {
            const lacx_block_info* dev = reinterpret_cast<const lacx_block_info*>(d->h_meta() + plan.at_rows);
            for (const PlanItem& p : base.items) {
                const uint32_t i = p.src;
                inspect_rows_of_item(in[i].lac, p.info.version, p.item.blocks, p.present_blocks, dev + p.item.block0, d->item_info[i]);
                if (out) out[i] = inspect_combine(d->item_info[i].data(), (uint32_t)d->item_info[i].size(), &p.info);
                if (partitions) d->info_block0[i] = p.item.block0;
            }
            if (partitions) {
                const uint8_t* mk = d->h_meta() + plan.at_mode_k;
                const uint32_t* pb = reinterpret_cast<const uint32_t*>(d->h_meta() + plan.at_part_bits);
                d->info_mode_k.assign(mk, mk + kInspectPartModeBytes * T);
                d->info_part_bits.assign(pb, pb + kInspectPartBitsBytes / 4 * T);
            }
        }
    }
    if (rc != LACX_OK) {  // the whole call failed: no item was inspected
        clear();
        if (out) std::memset(out, 0, sizeof(lacx_stream_report) * n);
        for (uint32_t i = 0; i < n; ++i) {
            if (code[i] != LACX_OK) continue;
            code[i] = rc;
            err[i] = g_decode_err;
        }
    }
    return rc;
}
}  // namespace

int lacx_decoder_inspect_batch_device(lacx_decoder* d, const lacx_span* lacs, uint32_t n, uint32_t flags, void* stream, int* item_rc,
                                      lacx_stream_report* out, float* device_ms) {
    if (!d) return decode_fail(LACX_E_INVALID, "null decoder");
    if (!lacs || n == 0) return decode_fail(LACX_E_INVALID, "null argument or empty batch");
    if (flags & ~LACX_INSPECT_PARTITIONS) return decode_fail(LACX_E_INVALID, "unknown inspection flag");
    std::vector<BatchIn> in(n);
    for (uint32_t i = 0; i < n; ++i) in[i] = BatchIn{lacs[i].data, lacs[i].size, nullptr, nullptr, 0};
    std::vector<int> code;
    std::vector<std::string> err;
    const int rc = inspect_run(d, in.data(), n, (flags & LACX_INSPECT_PARTITIONS) != 0, static_cast<hipStream_t>(stream), out, device_ms, code, err);
    return batch_outcome(d, rc, code, err, item_rc);
}

int lacx_decoder_item_block_info(const lacx_decoder* d, uint32_t i, const lacx_block_info** rows, uint32_t* count) {
    if (rows) *rows = nullptr;
    if (count) *count = 0;
    if (!d || !rows || !count) return decode_fail(LACX_E_INVALID, "null argument");
    if (i >= d->item_info.size()) return decode_fail(LACX_E_INVALID, "no such item in the last inspection call");
    *rows = d->item_info[i].data();
    *count = (uint32_t)d->item_info[i].size();
    return LACX_OK;
}

int lacx_decoder_item_partitions(const lacx_decoder* d, uint32_t i, uint32_t block, uint32_t channel, const uint8_t** mode_k,
                                 const uint32_t** part_bits, uint32_t* count) {
    if (mode_k) *mode_k = nullptr;
    if (part_bits) *part_bits = nullptr;
    if (count) *count = 0;
    if (!d || !mode_k || !part_bits || !count) return decode_fail(LACX_E_INVALID, "null argument");
    if (i >= d->item_info.size()) return decode_fail(LACX_E_INVALID, "no such item in the last inspection call");
    if (d->info_mode_k.empty() || d->info_block0[i] == ~0u) return decode_fail(LACX_E_INVALID, "the last inspection call kept no partition detail for this item");
    const std::vector<lacx_block_info>& rows = d->item_info[i];
    if (block >= rows.size() || channel >= 2u) return decode_fail(LACX_E_INVALID, "no such channel block in the item");
    const lacx_block_info& r = rows[block];
    if (r.code == LACX_BLOCK_MISSING || r.code != 0 || channel >= r.channels) return LACX_OK;  // nothing to report: count 0
    const size_t at = ((size_t)d->info_block0[i] + block) * 2u * kInspectPartSlots + (size_t)channel * kInspectPartSlots;
    const lacx_channel_info& c = r.ch[channel];
    *mode_k = d->info_mode_k.data() + at;
    *part_bits = d->info_part_bits.data() + at;
    *count = (uint32_t)c.mode_parts[0] + c.mode_parts[1] + c.mode_parts[2] + c.mode_parts[3];
    return LACX_OK;
}

int lacx_decoder_inspect_guard(const lacx_decoder* d, uint64_t* guarded, uint64_t* changed) {
    if (guarded) *guarded = 0;
    if (changed) *changed = 0;
    if (!d || !guarded || !changed) return decode_fail(LACX_E_INVALID, "null argument");
    *guarded = d->info_guard;
    *changed = d->info_guard_changed;
    return LACX_OK;
}

int lacx_inspect_combine(const lacx_block_info* rows, uint32_t count, const lacx_stream_info* info, lacx_stream_report* out) {
    if (out) std::memset(out, 0, sizeof(*out));
    if (!out || (!rows && count)) return decode_fail(LACX_E_INVALID, "null argument");
    *out = inspect_combine(rows, count, info);
    return LACX_OK;
}

// ---- runs (lacx.h) ----
namespace {
// every item's lacx_run_query resolved against the call's detectors (BatchIn::dets, ndet, dets_why)
void resolve_queries(const lacx_run_query* queries, const lacx_run_detector* dets, uint32_t ndets, std::vector<BatchIn>& in) {
    for (size_t i = 0; i < in.size(); ++i) {
        in[i].dets_why = check_detectors(queries[i], dets, ndets);
        if (!in[i].dets_why) in[i].dets = dets + queries[i].first_detector, in[i].ndet = queries[i].detectors;
    }
}
}  // namespace

int lacx_decoder_runs_batch_device(lacx_decoder* d, const lacx_span* lacs, const lacx_run_query* queries, uint32_t n, const lacx_run_detector* dets,
                                   uint32_t ndets, void* stream, int* item_rc, lacx_runs_result* out, float* device_ms) {
    if (!d) return decode_fail(LACX_E_INVALID, "null decoder");
    if (!lacs || !queries || n == 0) return decode_fail(LACX_E_INVALID, "null argument or empty batch");
    if (!dets || ndets == 0) return decode_fail(LACX_E_INVALID, "no detectors");
    std::vector<BatchIn> in(n);
    for (uint32_t i = 0; i < n; ++i) in[i] = BatchIn{lacs[i].data, lacs[i].size, nullptr, nullptr, 0};
    resolve_queries(queries, dets, ndets, in);
    DecodeJob job = salvage_job(DecodeForm::blocks, static_cast<hipStream_t>(stream), nullptr, nullptr, device_ms);
    job.in = in.data();
    job.n = n;
    job.runs = true;
    job.rres = out;
    return run_batch(d, job, item_rc);
}

int lacx_decoder_runs_pcm_batch_device(lacx_decoder* d, const lacx_digest_source* src, const lacx_run_query* queries, uint32_t n,
                                       const lacx_run_detector* dets, uint32_t ndets, void* stream, int* item_rc, lacx_runs_result* out,
                                       float* device_ms) {
    if (!d) return decode_fail(LACX_E_INVALID, "null decoder");
    if (!src || !queries || n == 0) return decode_fail(LACX_E_INVALID, "null argument or empty batch");
    if (!dets || ndets == 0) return decode_fail(LACX_E_INVALID, "no detectors");
    RunsPcm runs{std::vector<BatchIn>(n, BatchIn{nullptr, 0, nullptr, nullptr, 0}), out};
    resolve_queries(queries, dets, ndets, runs.in);
    std::vector<int> code;
    std::vector<std::string> err;
    const int rc = digest_pcm_run(d, src, n, static_cast<hipStream_t>(stream), nullptr, device_ms, code, err, 0, false, nullptr, &runs);
    return batch_outcome(d, rc, code, err, item_rc);
}

int lacx_decoder_item_runs(const lacx_decoder* d, uint32_t item, uint32_t detector, const lacx_run** runs, uint64_t* count) {
    if (runs) *runs = nullptr;
    if (count) *count = 0;
    if (!d || !runs || !count) return decode_fail(LACX_E_INVALID, "null argument");
    if (item >= d->item_runs.size()) return decode_fail(LACX_E_INVALID, "no such item in the last runs call");
    if (detector >= d->item_runs[item].size()) return decode_fail(LACX_E_INVALID, "no such detector of that item in the last runs call");
    *runs = d->item_runs[item][detector].data();
    *count = d->item_runs[item][detector].size();
    return LACX_OK;
}

// ---- loudness (lacx.h) ----
int lacx_decoder_loudness_batch_device(lacx_decoder* d, const lacx_span* lacs, uint32_t n, void* stream, int* item_rc, lacx_loudness* out,
                                       float* device_ms) {
    if (!d) return decode_fail(LACX_E_INVALID, "null decoder");
    if (!lacs || n == 0) return decode_fail(LACX_E_INVALID, "null argument or empty batch");
    std::vector<BatchIn> in(n);
    for (uint32_t i = 0; i < n; ++i) in[i] = BatchIn{lacs[i].data, lacs[i].size, nullptr, nullptr, 0};
    DecodeJob job{in.data(), n, DecodeForm::digest, kWholeStreams, static_cast<hipStream_t>(stream), nullptr, nullptr, device_ms};
    job.loudness = true;
    job.lres = out;
    return run_batch(d, job, item_rc);
}

int lacx_decoder_loudness_pcm_batch_device(lacx_decoder* d, const lacx_digest_source* src, uint32_t n, void* stream, int* item_rc,
                                           lacx_loudness* out, float* device_ms) {
    if (!d) return decode_fail(LACX_E_INVALID, "null decoder");
    if (!src || n == 0) return decode_fail(LACX_E_INVALID, "null argument or empty batch");
    const LoudPcm loud{out};
    std::vector<int> code;
    std::vector<std::string> err;
    const int rc = digest_pcm_run(d, src, n, static_cast<hipStream_t>(stream), nullptr, device_ms, code, err, 0, false, nullptr, nullptr, &loud);
    return batch_outcome(d, rc, code, err, item_rc);
}

int lacx_decoder_item_loudness_rows(const lacx_decoder* d, uint32_t i, const lacx_loudness_row** rows, uint32_t* count) {
    if (rows) *rows = nullptr;
    if (count) *count = 0;
    if (!d || !rows || !count) return decode_fail(LACX_E_INVALID, "null argument");
    if (i >= d->item_loud.size()) return decode_fail(LACX_E_INVALID, "no such item in the last loudness call");
    *rows = d->item_loud[i].data();
    *count = (uint32_t)d->item_loud[i].size();
    return LACX_OK;
}

int lacx_loudness_combine(const lacx_loudness_row* const* rows, const uint32_t* counts, const uint8_t* channels, const uint8_t* bit_depths,
                          const uint32_t* sample_rates, uint32_t nsets, lacx_loudness* out) {
    if (out) std::memset(out, 0, sizeof(*out));
    if (!out || !rows || !counts || !channels || !bit_depths || !sample_rates || nsets == 0) return decode_fail(LACX_E_INVALID, "null argument or no sets");
    std::vector<LoudSet> sets(nsets);
    for (uint32_t k = 0; k < nsets; ++k) {
        if (!rows[k] && counts[k]) return decode_fail(LACX_E_INVALID, "null argument");
        if (channels[k] != 1 && channels[k] != 2) return decode_fail(LACX_E_INVALID, "unsupported channel count");
        if (bit_depths[k] != 16 && bit_depths[k] != 24) return decode_fail(LACX_E_INVALID, "unsupported bit depth: " + std::to_string((int)bit_depths[k]));
        if (loud_rate_index(sample_rates[k]) < 0) return decode_fail(LACX_E_INVALID, "unsupported sample rate: " + std::to_string(sample_rates[k]));
        sets[k] = LoudSet{rows[k], counts[k], channels[k], bit_depths[k], sample_rates[k]};
    }
    *out = loudness_combine(sets.data(), nsets);
    return LACX_OK;
}

// ---- true peak (lacx.h) ----
int lacx_decoder_truepeak_batch_device(lacx_decoder* d, const lacx_span* lacs, uint32_t n, void* stream, int* item_rc, lacx_truepeak* out,
                                       float* device_ms) {
    if (!d) return decode_fail(LACX_E_INVALID, "null decoder");
    if (!lacs || n == 0) return decode_fail(LACX_E_INVALID, "null argument or empty batch");
    std::vector<BatchIn> in(n);
    for (uint32_t i = 0; i < n; ++i) in[i] = BatchIn{lacs[i].data, lacs[i].size, nullptr, nullptr, 0};
    DecodeJob job{in.data(), n, DecodeForm::digest, kWholeStreams, static_cast<hipStream_t>(stream), nullptr, nullptr, device_ms};
    job.truepeak = true;
    job.pres = out;
    return run_batch(d, job, item_rc);
}

int lacx_decoder_truepeak_pcm_batch_device(lacx_decoder* d, const lacx_digest_source* src, uint32_t n, void* stream, int* item_rc,
                                           lacx_truepeak* out, float* device_ms) {
    if (!d) return decode_fail(LACX_E_INVALID, "null decoder");
    if (!src || n == 0) return decode_fail(LACX_E_INVALID, "null argument or empty batch");
    const PeakPcm peak{out};
    std::vector<int> code;
    std::vector<std::string> err;
    const int rc = digest_pcm_run(d, src, n, static_cast<hipStream_t>(stream), nullptr, device_ms, code, err, 0, false, nullptr, nullptr, nullptr, &peak);
    return batch_outcome(d, rc, code, err, item_rc);
}

int lacx_decoder_item_truepeak_rows(const lacx_decoder* d, uint32_t i, const lacx_truepeak_row** rows, uint32_t* count) {
    if (rows) *rows = nullptr;
    if (count) *count = 0;
    if (!d || !rows || !count) return decode_fail(LACX_E_INVALID, "null argument");
    if (i >= d->item_peak.size()) return decode_fail(LACX_E_INVALID, "no such item in the last true peak call");
    *rows = d->item_peak[i].data();
    *count = (uint32_t)d->item_peak[i].size();
    return LACX_OK;
}

int lacx_truepeak_combine(const lacx_truepeak_row* const* rows, const uint32_t* counts, const uint8_t* channels, const uint8_t* bit_depths,
                          const uint64_t* frames, const uint32_t* sample_rates, uint32_t nsets, lacx_truepeak* out) {
    if (out) std::memset(out, 0, sizeof(*out));
    if (!out || !rows || !counts || !channels || !bit_depths || !frames || !sample_rates || nsets == 0) return decode_fail(LACX_E_INVALID, "null argument or no sets");
    std::vector<TpSet> sets(nsets);
    for (uint32_t k = 0; k < nsets; ++k) {
        if (!rows[k] && counts[k]) return decode_fail(LACX_E_INVALID, "null argument");
        if (channels[k] != 1 && channels[k] != 2) return decode_fail(LACX_E_INVALID, "unsupported channel count");
        if (bit_depths[k] != 16 && bit_depths[k] != 24) return decode_fail(LACX_E_INVALID, "unsupported bit depth: " + std::to_string((int)bit_depths[k]));
        if (loud_rate_index(sample_rates[k]) < 0) return decode_fail(LACX_E_INVALID, "unsupported sample rate: " + std::to_string(sample_rates[k]));
        if (tp_rows(frames[k]) != counts[k]) return decode_fail(LACX_E_INVALID, "row count does not match the frames");
        sets[k] = TpSet{rows[k], counts[k], channels[k], bit_depths[k], frames[k], sample_rates[k]};
    }
    *out = truepeak_combine(sets.data(), nsets);
    return LACX_OK;
}

// ---- spectrum (lacx.h) ----
int lacx_decoder_spectrum_batch_device(lacx_decoder* d, const lacx_span* lacs, uint32_t n, uint32_t window, double floor_db, void* stream, int* item_rc,
                                       lacx_spectrum* out, float* device_ms) {
    if (!d) return decode_fail(LACX_E_INVALID, "null decoder");
    if (!lacs || n == 0) return decode_fail(LACX_E_INVALID, "null argument or empty batch");
    if (!sp_logn(window)) return decode_fail(LACX_E_INVALID, "unsupported spectrum window: " + std::to_string(window));
    std::vector<BatchIn> in(n);
    for (uint32_t i = 0; i < n; ++i) in[i] = BatchIn{lacs[i].data, lacs[i].size, nullptr, nullptr, 0};
    DecodeJob job{in.data(), n, DecodeForm::digest, kWholeStreams, static_cast<hipStream_t>(stream), nullptr, nullptr, device_ms};
    job.spectrum = window;
    job.floor_db = floor_db;
    job.xres = out;
    return run_batch(d, job, item_rc);
}

int lacx_decoder_spectrum_pcm_batch_device(lacx_decoder* d, const lacx_digest_source* src, uint32_t n, uint32_t window, double floor_db, void* stream,
                                           int* item_rc, lacx_spectrum* out, float* device_ms) {
    if (!d) return decode_fail(LACX_E_INVALID, "null decoder");
    if (!src || n == 0) return decode_fail(LACX_E_INVALID, "null argument or empty batch");
    if (!sp_logn(window)) return decode_fail(LACX_E_INVALID, "unsupported spectrum window: " + std::to_string(window));
    const SpecPcm spec{out, window, floor_db};
    std::vector<int> code;
    std::vector<std::string> err;
    const int rc = digest_pcm_run(d, src, n, static_cast<hipStream_t>(stream), nullptr, device_ms, code, err, 0, false, nullptr, nullptr, nullptr, nullptr, &spec);
    return batch_outcome(d, rc, code, err, item_rc);
}

int lacx_decoder_item_spectrum_rows(const lacx_decoder* d, uint32_t i, const lacx_spectrum_row** rows, uint32_t* count) {
    if (rows) *rows = nullptr;
    if (count) *count = 0;
    if (!d || !rows || !count) return decode_fail(LACX_E_INVALID, "null argument");
    if (i >= d->item_spec.size()) return decode_fail(LACX_E_INVALID, "no such item in the last spectrum call");
    *rows = d->item_spec[i].data();
    *count = (uint32_t)d->item_spec[i].size();
    return LACX_OK;
}

int lacx_spectrum_combine(const lacx_spectrum_row* rows, uint32_t count, uint8_t channels, uint8_t bit_depth, uint64_t frames, uint32_t sample_rate,
                          uint32_t window, double floor_db, lacx_spectrum* out) {
    if (out) std::memset(out, 0, sizeof(*out));
    if (!out || (!rows && count)) return decode_fail(LACX_E_INVALID, "null argument");
    if (channels != 1 && channels != 2) return decode_fail(LACX_E_INVALID, "unsupported channel count");
    if (bit_depth != 16 && bit_depth != 24) return decode_fail(LACX_E_INVALID, "unsupported bit depth: " + std::to_string((int)bit_depth));
    if (loud_rate_index(sample_rate) < 0) return decode_fail(LACX_E_INVALID, "unsupported sample rate: " + std::to_string(sample_rate));
    if (!sp_logn(window)) return decode_fail(LACX_E_INVALID, "unsupported spectrum window: " + std::to_string(window));
    if (sp_rows(frames) != count) return decode_fail(LACX_E_INVALID, "row count does not match the frames");
    *out = spectrum_of_rows(SpSet{rows, count, channels, bit_depth, frames, sample_rate, window, floor_db});
    return LACX_OK;
}

// ---- rip checksums (lacx.h) ----
namespace {
// The discs of a call against its arrays: per disc its code and text ("" = it goes to the device) and its track lengths.
// frames / src_code / src_why: per source of the call its frames, or why it is refused.
struct ArCall {
    std::vector<int> code;
    std::vector<std::string> err;
    std::vector<std::vector<uint64_t>> tracks;
};
void ar_resolve(const lacx_ar_disc* discs, uint32_t ndiscs, uint32_t nsrc, const uint64_t* track_frames, uint32_t ntracks, const std::vector<uint64_t>& frames,
                const std::vector<int>& src_code, const std::vector<std::string>& src_why, ArCall& c) {
    c.code.assign(ndiscs, LACX_OK);
    c.err.assign(ndiscs, std::string());
    c.tracks.assign(ndiscs, {});
    for (uint32_t k = 0; k < ndiscs; ++k) {
        const lacx_ar_disc& x = discs[k];
        auto refuse = [&](int code, const std::string& why) { c.code[k] = code, c.err[k] = why; };
        if (x.sources == 0) { refuse(LACX_E_INVALID, "disc has no sources"); continue; }
        if (x.first_source > nsrc || x.sources > nsrc - x.first_source) { refuse(LACX_E_INVALID, "sources outside the call's array"); continue; }
        if (x.tracks && (!track_frames || x.first_track > ntracks || x.tracks > ntracks - x.first_track)) { refuse(LACX_E_INVALID, "tracks outside the call's array"); continue; }
        uint64_t total = 0;
        for (uint32_t i = 0; i < x.sources && c.code[k] == LACX_OK; ++i) {
            const uint32_t at = x.first_source + i;
            if (src_code[at] != LACX_OK) refuse(src_code[at], "source " + std::to_string(i) + ": " + src_why[at]);
            total += frames[at];
        }
        if (c.code[k] != LACX_OK) continue;
        if (x.tracks) c.tracks[k].assign(track_frames + x.first_track, track_frames + x.first_track + x.tracks);
        else c.tracks[k].assign(frames.begin() + x.first_source, frames.begin() + x.first_source + x.sources);
        const std::string why = ar_disc_why(x.sources, total, c.tracks[k].data(), (uint32_t)c.tracks[k].size(), x.flags, x.radius);
        if (!why.empty()) refuse(LACX_E_INVALID, why);
    }
}

void ar_reset(lacx_decoder* d, uint32_t ndiscs, lacx_ar_result* out, float* device_ms) {
    if (device_ms) *device_ms = 0.f;
    if (out) std::memset(out, 0, sizeof(lacx_ar_result) * ndiscs);
    d->ar_at = ArLayout{};
    d->ar_sums.clear();
    d->ar_ok.assign(ndiscs, 0);
    d->ar_slot.assign(ndiscs, 0);
    d->ar_tracks.assign(ndiscs, {});
}

// Disc k of the call went to the device as the plan's disc `slot` and all of its sources are good: its answer.
void ar_accept(lacx_decoder* d, uint32_t k, size_t slot, const lacx_ar_disc& x, const std::vector<uint64_t>& tracks, lacx_ar_result* out) {
    d->ar_ok[k] = 1;
    d->ar_slot[k] = (uint32_t)slot;
    ar_tracks(d->ar_at, slot, d->ar_sums.data(), d->ar_tracks[k]);
    if (out) out[k] = ar_result(d->ar_at, slot, x.lba0, tracks.data());
}

// How a rip-checksum call ends: as batch_outcome, per disc.
int ar_outcome(lacx_decoder* d, int rc, ArCall& c, int* disc_rc) {
    if (disc_rc) std::copy(c.code.begin(), c.code.end(), disc_rc);
    d->item_err = std::move(c.err);
    if (rc != LACX_OK) return rc;
    for (size_t k = 0; k < c.code.size(); ++k)
        if (c.code[k] != LACX_OK) return decode_fail(c.code[k], "disc " + std::to_string(k) + ": " + d->item_err[k]);
    return LACX_OK;
}
}  // namespace

int lacx_decoder_accuraterip_batch_device(lacx_decoder* d, const lacx_span* lacs, uint32_t nlacs, const uint64_t* track_frames, uint32_t ntracks,
                                          const lacx_ar_disc* discs, uint32_t ndiscs, void* stream, int* disc_rc, lacx_ar_result* out, float* device_ms) {
    if (!d) return decode_fail(LACX_E_INVALID, "null decoder");
    if (!lacs || nlacs == 0 || !discs || ndiscs == 0) return decode_fail(LACX_E_INVALID, "null argument or empty batch");
    ar_reset(d, ndiscs, out, device_ms);
    std::vector<uint64_t> frames(nlacs, 0);
    std::vector<int> src_code(nlacs, LACX_OK);
    std::vector<std::string> src_why(nlacs);
    for (uint32_t i = 0; i < nlacs; ++i) {
        lacx_stream_info f{};
        const char* why = nullptr;
        src_code[i] = parse_stream(lacs[i].data, lacs[i].size, &f, &why);
        if (src_code[i] != LACX_OK) {
            src_why[i] = why ? why : "";
        } else if (f.channels != 2 || f.bit_depth != 16 || f.sample_rate != 44100) {
            src_code[i] = LACX_E_INVALID;
            src_why[i] = "not CD audio (" + std::to_string((int)f.channels) + " channels, " + std::to_string((int)f.bit_depth) + " bit, " + std::to_string(f.sample_rate) + " Hz)";
        }
        frames[i] = f.frames;
    }
    ArCall c;
    ar_resolve(discs, ndiscs, nlacs, track_frames, ntracks, frames, src_code, src_why, c);
    std::vector<BatchIn> in;  // the accepted discs' sources, disc after disc
    std::vector<ArDiscIn> adiscs;
    std::vector<uint32_t> which;  // ... their indices in the call
    for (uint32_t k = 0; k < ndiscs; ++k) {
        if (c.code[k] != LACX_OK) continue;
        adiscs.push_back(ArDiscIn{(uint32_t)in.size(), discs[k].sources, c.tracks[k].data(), (uint32_t)c.tracks[k].size(), discs[k].flags, discs[k].radius, false});
        which.push_back(k);
        for (uint32_t i = 0; i < discs[k].sources; ++i) {
            const lacx_span& x = lacs[discs[k].first_source + i];
            in.push_back(BatchIn{x.data, x.size, nullptr, nullptr, 0});
        }
    }
    int rc = LACX_OK;
    if (!adiscs.empty()) {
        const ArJobIn arjob{adiscs.data(), (uint32_t)adiscs.size()};
        std::vector<uint32_t> planned;
        DecodeJob job{in.data(), (uint32_t)in.size(), DecodeForm::digest, kWholeStreams, static_cast<hipStream_t>(stream), nullptr, nullptr, device_ms};
        job.ar = &arjob;
        job.ar_planned = &planned;
        std::vector<int> code;
        std::vector<std::string> err;
        rc = decode_batch_run(d, job, code, err);
        for (size_t a = 0; a < adiscs.size(); ++a) {
            const uint32_t k = which[a];
            for (uint32_t i = 0; i < adiscs[a].nsrc && c.code[k] == LACX_OK; ++i)
                if (code[adiscs[a].src0 + i] != LACX_OK) c.code[k] = code[adiscs[a].src0 + i], c.err[k] = rc != LACX_OK ? err[adiscs[a].src0 + i] : "source " + std::to_string(i) + ": " + err[adiscs[a].src0 + i];
            if (c.code[k] != LACX_OK) continue;
            const auto slot = std::find(planned.begin(), planned.end(), (uint32_t)a);
            if (slot == planned.end()) c.code[k] = LACX_E_RUNTIME, c.err[k] = "disc was not planned";
            else ar_accept(d, k, (size_t)(slot - planned.begin()), discs[k], c.tracks[k], out);
        }
        if (rc != LACX_OK) ar_reset(d, ndiscs, out, nullptr);
    } else if (lacx_device_count() <= 0) {
        rc = decode_fail(LACX_E_DEVICE, "no usable HIP device");
    }
    return ar_outcome(d, rc, c, disc_rc);
}

int lacx_decoder_accuraterip_pcm_batch_device(lacx_decoder* d, const lacx_digest_source* src, uint32_t nsrc, const uint64_t* track_frames, uint32_t ntracks,
                                              const lacx_ar_disc* discs, uint32_t ndiscs, void* stream, int* disc_rc, lacx_ar_result* out, float* device_ms) {
    if (!d) return decode_fail(LACX_E_INVALID, "null decoder");
    if (!src || nsrc == 0 || !discs || ndiscs == 0) return decode_fail(LACX_E_INVALID, "null argument or empty batch");
    hipStream_t st = static_cast<hipStream_t>(stream);
    ar_reset(d, ndiscs, out, device_ms);
    std::vector<uint64_t> frames(nsrc, 0);
    std::vector<int> src_code(nsrc, LACX_OK);
    std::vector<std::string> src_why(nsrc);
    for (uint32_t i = 0; i < nsrc; ++i) {
        std::string text;
        if (const char* why = check_digest_source(src[i], text)) {
            src_code[i] = LACX_E_INVALID, src_why[i] = why;
        } else if (src[i].pcm.channels != 2 || src[i].bit_depth != 16 || src[i].sample_rate != 44100) {
            src_code[i] = LACX_E_INVALID;
            src_why[i] = "not CD audio (" + std::to_string(src[i].pcm.channels) + " channels, " + std::to_string((int)src[i].bit_depth) + " bit, " + std::to_string(src[i].sample_rate) + " Hz)";
        }
        frames[i] = src[i].frames;
    }
    ArCall c;
    ar_resolve(discs, ndiscs, nsrc, track_frames, ntracks, frames, src_code, src_why, c);
    std::vector<ArSrcIn> in;
    std::vector<ArDiscIn> adiscs;
    std::vector<uint32_t> which;
    for (uint32_t k = 0; k < ndiscs; ++k) {
        if (c.code[k] != LACX_OK) continue;
        adiscs.push_back(ArDiscIn{(uint32_t)in.size(), discs[k].sources, c.tracks[k].data(), (uint32_t)c.tracks[k].size(), discs[k].flags, discs[k].radius, true});
        which.push_back(k);
        for (uint32_t i = 0; i < discs[k].sources; ++i) {
            const lacx_digest_source& x = src[discs[k].first_source + i];
            in.push_back(ArSrcIn{x.pcm.data0, x.pcm.data1, x.frames, x.pcm.layout, (uint32_t)in.size()});
        }
    }
    int rc = lacx_device_count() <= 0 ? decode_fail(LACX_E_DEVICE, "no usable HIP device") : LACX_OK;
    if (rc == LACX_OK && !adiscs.empty()) {
        const size_t ns = in.size();
        if (const char* why = ar_check(in.data(), adiscs.data(), adiscs.size())) rc = decode_fail(LACX_E_DEVICE, why);
        if (rc == LACX_OK) {  // the tables: bad [ns] | the tables of accuraterip_plan.h (16-byte aligned)
            const ArLayout y = ar_layout(plan_detail::up16(8 * ns), in.data(), adiscs.data(), adiscs.size());
            int prev_device = -1;
            DevErr e = decoder_open(d, &prev_device);
            if (!e) e = buf_grow(d->tables, y.size, y.size / 8 + 256);
            if (!e) {
                for (size_t j = 0; j < ns; ++j) reinterpret_cast<unsigned long long*>(d->h_meta())[j] = kDigestClean;
                ar_fill(y, in.data(), adiscs.data(), adiscs.size(), d->h_meta());
                e = chk(hipMemcpyAsync(d->d_meta(), d->h_meta(), y.size, hipMemcpyHostToDevice, st), "H2D rip checksum tables");
            }
            if (!e) e = chk(hipEventRecord(d->e0, st), "event record");
            if (!e) e = chk(launch_accuraterip(ar_args(y, d->d_meta(), reinterpret_cast<unsigned long long*>(d->d_meta())), st), "rip checksum launch");
            if (!e) e = chk(hipEventRecord(d->e1, st), "event record");
            if (!e) e = chk(hipMemcpyAsync(d->h_meta(), d->d_meta(), 8 * ns, hipMemcpyDeviceToHost, st), "D2H validation keys");
            if (!e && y.total_sums) e = chk(hipMemcpyAsync(d->h_meta() + y.sums, d->d_meta() + y.sums, 4 * (size_t)y.total_sums, hipMemcpyDeviceToHost, st), "D2H rip checksums");
            if (!e) e = chk(hipStreamSynchronize(st), "synchronize");
            if (!e && device_ms) (void)hipEventElapsedTime(device_ms, d->e0, d->e1);
            if (prev_device >= 0) (void)hipSetDevice(prev_device);
            if (e) {
                rc = decode_fail(LACX_E_DEVICE, std::string(e.what) + ": " + hipGetErrorString(e.e));
            } else {
                d->ar_at = y;
                const auto* sums = reinterpret_cast<const uint32_t*>(d->h_meta() + y.sums);
                d->ar_sums.assign(sums, sums + y.total_sums);
                const auto* bad = reinterpret_cast<const unsigned long long*>(d->h_meta());
                for (size_t a = 0; a < adiscs.size(); ++a) {
                    const uint32_t k = which[a];
                    for (uint32_t i = 0; i < adiscs[a].nsrc && c.code[k] == LACX_OK; ++i) {
                        const unsigned long long key = bad[adiscs[a].src0 + i];
                        if (key == kDigestClean) continue;
                        ImportBad b{{kImportClean, kImportClean}};  // the encoder's words for it (import_msg.h)
                        b.key[key >> 63] = key & ~(1ull << 63);
                        int ch = 0;
                        unsigned long long index = 0;
                        std::string text;
                        (void)import_bad_message(b, 16, &ch, &index, text);
                        c.code[k] = LACX_E_INVALID, c.err[k] = "source " + std::to_string(i) + ": " + text;
                    }
                    if (c.code[k] == LACX_OK) ar_accept(d, k, a, discs[k], c.tracks[k], out);
                }
            }
        }
    }
    if (rc != LACX_OK) {  // the whole call failed: no disc has an answer
        ar_reset(d, ndiscs, out, nullptr);
        for (uint32_t k = 0; k < ndiscs; ++k)
            if (c.code[k] == LACX_OK) c.code[k] = rc, c.err[k] = g_decode_err;
    }
    return ar_outcome(d, rc, c, disc_rc);
}

int lacx_decoder_item_ar_tracks(const lacx_decoder* d, uint32_t disc, const lacx_ar_track** tracks, uint32_t* count) {
    if (tracks) *tracks = nullptr;
    if (count) *count = 0;
    if (!d || !tracks || !count) return decode_fail(LACX_E_INVALID, "null argument");
    if (disc >= d->ar_ok.size() || !d->ar_ok[disc]) return decode_fail(LACX_E_INVALID, "no such disc in the last rip checksum call");
    *tracks = d->ar_tracks[disc].data();
    *count = (uint32_t)d->ar_tracks[disc].size();
    return LACX_OK;
}

int lacx_decoder_item_ar_sums(const lacx_decoder* d, uint32_t disc, uint32_t track, const uint32_t** v1, const uint32_t** v2, const uint32_t** s450,
                              uint32_t* count) {
    if (v1) *v1 = nullptr;
    if (v2) *v2 = nullptr;
    if (s450) *s450 = nullptr;
    if (count) *count = 0;
    if (!d || !v1 || !v2 || !s450 || !count) return decode_fail(LACX_E_INVALID, "null argument");
    if (disc >= d->ar_ok.size() || !d->ar_ok[disc]) return decode_fail(LACX_E_INVALID, "no such disc in the last rip checksum call");
    const ArDiscAt& at = d->ar_at.discs[d->ar_slot[disc]];
    if (track >= at.ntracks) return decode_fail(LACX_E_INVALID, "no such track on the disc");
    const uint32_t width = 2u * at.radius + 1u;
    const uint32_t* row = d->ar_sums.data() + at.sum0 + 3ull * width * track;
    *v1 = row, *v2 = row + width, *s450 = row + 2u * width, *count = width;
    return LACX_OK;
}

int lacx_ar_ids(const uint64_t* track_frames, uint32_t ntracks, uint32_t flags, uint32_t lba0, lacx_ar_id* out) {
    if (out) *out = lacx_ar_id{0, 0, 0};
    if (!out || !track_frames) return decode_fail(LACX_E_INVALID, "null argument");
    if (ntracks == 0) return decode_fail(LACX_E_INVALID, "disc has no tracks");
    if (ntracks > 99) return decode_fail(LACX_E_INVALID, "more than 99 tracks");
    for (uint32_t t = 0; t < ntracks; ++t)
        if (track_frames[t] == 0) return decode_fail(LACX_E_INVALID, "track " + std::to_string(t) + " is empty");
    if (flags & ~(uint32_t)(LACX_AR_FIRST | LACX_AR_LAST)) return decode_fail(LACX_E_INVALID, "unknown flags");
    (void)ar_ids(track_frames, ntracks, flags, lba0, *out);
    return LACX_OK;
}

// ---- bit-compare (lacx.h) ----
namespace {
// The pairs of a call against its sources: per pair its code and text ("" = it goes to the device).  fmt / src_code / src_why:
// per source of the call its format, or why it is refused.
struct CmpCall {
    std::vector<int> code;
    std::vector<std::string> err;
};
void cmp_resolve(const lacx_compare_pair* pairs, uint32_t npairs, uint32_t nsrc, const std::vector<CmpFmt>& fmt, const std::vector<int>& src_code,
                 const std::vector<std::string>& src_why, CmpCall& c) {
    c.code.assign(npairs, LACX_OK);
    c.err.assign(npairs, std::string());
    for (uint32_t k = 0; k < npairs; ++k) {
        const lacx_compare_pair& x = pairs[k];
        if (x.a >= nsrc || x.b >= nsrc) {
            c.code[k] = LACX_E_INVALID, c.err[k] = "sources outside the call's array";
            continue;
        }
        for (uint32_t at : {x.a, x.b})
            if (c.code[k] == LACX_OK && src_code[at] != LACX_OK) c.code[k] = src_code[at], c.err[k] = "source " + std::to_string(at) + ": " + src_why[at];
        if (c.code[k] != LACX_OK) continue;
        const std::string why = cmp_pair_why(x, fmt.data(), nsrc);
        if (!why.empty()) c.code[k] = LACX_E_INVALID, c.err[k] = why;
    }
}

void cmp_reset(lacx_decoder* d, uint32_t npairs, lacx_compare* out, float* device_ms) {
    if (device_ms) *device_ms = 0.f;
    if (out) std::memset(out, 0, sizeof(lacx_compare) * npairs);
    d->cmp_at = CmpLayout{};
    d->cmp_counts.clear();
    d->cmp_rows.clear();
    d->cmp_ok.assign(npairs, 0);
    d->cmp_slot.assign(npairs, 0);
}

// Pair k of the call went to the device as the plan's pair `slot` and both of its sources are good: its answer.
void cmp_accept(lacx_decoder* d, uint32_t k, size_t slot, uint32_t sample_rate, lacx_compare* out) {
    d->cmp_ok[k] = 1;
    d->cmp_slot[k] = (uint32_t)slot;
    if (out) out[k] = cmp_result(d->cmp_at, slot, d->cmp_rows.data() + d->cmp_at.pair[slot].row0, sample_rate);
}

// How a compare call ends: as batch_outcome, per pair.
int cmp_outcome(lacx_decoder* d, int rc, CmpCall& c, int* pair_rc) {
    if (pair_rc) std::copy(c.code.begin(), c.code.end(), pair_rc);
    d->item_err = std::move(c.err);
    if (rc != LACX_OK) return rc;
    for (size_t k = 0; k < c.code.size(); ++k)
        if (c.code[k] != LACX_OK) return decode_fail(c.code[k], "pair " + std::to_string(k) + ": " + d->item_err[k]);
    return LACX_OK;
}

// The accepted pairs over the sources they name, each source once: used[i] = the source's place among them, or ~0u.
void cmp_gather(const lacx_compare_pair* pairs, uint32_t npairs, const CmpCall& c, uint32_t nsrc, std::vector<uint32_t>& used, std::vector<uint32_t>& order,
                std::vector<CmpPairIn>& apairs, std::vector<uint32_t>& which) {
    used.assign(nsrc, ~0u);
    for (uint32_t k = 0; k < npairs; ++k) {
        if (c.code[k] != LACX_OK) continue;
        for (uint32_t at : {pairs[k].a, pairs[k].b})
            if (used[at] == ~0u) used[at] = (uint32_t)order.size(), order.push_back(at);
        apairs.push_back(CmpPairIn{used[pairs[k].a], used[pairs[k].b], (long long)pairs[k].centre, pairs[k].radius});
        which.push_back(k);
    }
}
}  // namespace

int lacx_decoder_compare_batch_device(lacx_decoder* d, const lacx_span* lacs, uint32_t nlacs, const lacx_compare_pair* pairs, uint32_t npairs, void* stream,
                                      int* pair_rc, lacx_compare* out, float* device_ms) {
    if (!d) return decode_fail(LACX_E_INVALID, "null decoder");
    if (!lacs || nlacs == 0 || !pairs || npairs == 0) return decode_fail(LACX_E_INVALID, "null argument or empty batch");
    cmp_reset(d, npairs, out, device_ms);
    std::vector<CmpFmt> fmt(nlacs);
    std::vector<int> src_code(nlacs, LACX_OK);
    std::vector<std::string> src_why(nlacs);
    for (uint32_t i = 0; i < nlacs; ++i) {
        lacx_stream_info f{};
        const char* why = nullptr;
        src_code[i] = parse_stream(lacs[i].data, lacs[i].size, &f, &why);
        if (src_code[i] != LACX_OK) src_why[i] = why ? why : "";
        else if (f.frames == 0) src_code[i] = LACX_E_INVALID, src_why[i] = "source has no frames";
        fmt[i] = CmpFmt{f.frames, f.sample_rate, (uint8_t)f.channels, (uint8_t)f.bit_depth};
    }
    CmpCall c;
    cmp_resolve(pairs, npairs, nlacs, fmt, src_code, src_why, c);
    std::vector<uint32_t> used, order, which;
    std::vector<CmpPairIn> apairs;
    cmp_gather(pairs, npairs, c, nlacs, used, order, apairs, which);
    int rc = LACX_OK;
    if (!apairs.empty()) {
        std::vector<BatchIn> in;
        for (uint32_t at : order) in.push_back(BatchIn{lacs[at].data, lacs[at].size, nullptr, nullptr, 0});
        const CmpJobIn cjob{apairs.data(), (uint32_t)apairs.size()};
        std::vector<uint32_t> planned;
        DecodeJob job{in.data(), (uint32_t)in.size(), DecodeForm::digest, kWholeStreams, static_cast<hipStream_t>(stream), nullptr, nullptr, device_ms};
        job.cmp = &cjob;
        job.cmp_planned = &planned;
        std::vector<int> code;
        std::vector<std::string> err;
        rc = decode_batch_run(d, job, code, err);
        for (size_t a = 0; a < apairs.size(); ++a) {
            const uint32_t k = which[a];
            for (uint32_t at : {pairs[k].a, pairs[k].b})
                if (c.code[k] == LACX_OK && code[used[at]] != LACX_OK)
                    c.code[k] = code[used[at]], c.err[k] = rc != LACX_OK ? err[used[at]] : "source " + std::to_string(at) + ": " + err[used[at]];
            if (c.code[k] != LACX_OK) continue;
            const auto slot = std::find(planned.begin(), planned.end(), (uint32_t)a);
            if (slot == planned.end()) c.code[k] = LACX_E_RUNTIME, c.err[k] = "pair was not planned";
            else cmp_accept(d, k, (size_t)(slot - planned.begin()), fmt[pairs[k].a].sample_rate, out);
        }
        if (rc != LACX_OK) cmp_reset(d, npairs, out, nullptr);
    } else if (lacx_device_count() <= 0) {
        rc = decode_fail(LACX_E_DEVICE, "no usable HIP device");
    }
    return cmp_outcome(d, rc, c, pair_rc);
}

int lacx_decoder_compare_pcm_batch_device(lacx_decoder* d, const lacx_digest_source* src, uint32_t nsrc, const lacx_compare_pair* pairs, uint32_t npairs,
                                          void* stream, int* pair_rc, lacx_compare* out, float* device_ms) {
    if (!d) return decode_fail(LACX_E_INVALID, "null decoder");
    if (!src || nsrc == 0 || !pairs || npairs == 0) return decode_fail(LACX_E_INVALID, "null argument or empty batch");
    hipStream_t st = static_cast<hipStream_t>(stream);
    cmp_reset(d, npairs, out, device_ms);
    std::vector<CmpFmt> fmt(nsrc);
    std::vector<int> src_code(nsrc, LACX_OK);
    std::vector<std::string> src_why(nsrc);
    for (uint32_t i = 0; i < nsrc; ++i) {
        std::string text;
        if (const char* why = check_digest_source(src[i], text)) src_code[i] = LACX_E_INVALID, src_why[i] = why;
        fmt[i] = CmpFmt{src[i].frames, src[i].sample_rate, (uint8_t)src[i].pcm.channels, src[i].bit_depth};
    }
    CmpCall c;
    cmp_resolve(pairs, npairs, nsrc, fmt, src_code, src_why, c);
    std::vector<uint32_t> used, order, which;
    std::vector<CmpPairIn> apairs;
    cmp_gather(pairs, npairs, c, nsrc, used, order, apairs, which);
    std::vector<CmpSrcIn> in;
    for (uint32_t at : order) {
        const lacx_digest_source& x = src[at];
        in.push_back(CmpSrcIn{x.pcm.data0, x.pcm.data1, x.frames, x.pcm.layout, (uint32_t)in.size(), (uint8_t)x.pcm.channels, x.bit_depth, true});
    }
    int rc = lacx_device_count() <= 0 ? decode_fail(LACX_E_DEVICE, "no usable HIP device") : LACX_OK;
    if (rc == LACX_OK && !apairs.empty()) {
        const size_t ns = in.size();
        if (const char* why = cmp_check(in.data(), apairs.data(), apairs.size())) rc = decode_fail(LACX_E_DEVICE, why);
        if (rc == LACX_OK) {  // the tables: bad [ns] | the tables of compare_plan.h (16-byte aligned)
            d->cmp_at = cmp_layout(plan_detail::up16(8 * ns), in.data(), ns, apairs.data(), apairs.size());
            CmpLayout& y = d->cmp_at;
            int prev_device = -1;
            DevErr e = decoder_open(d, &prev_device);
            if (!e) e = buf_grow(d->tables, y.size, y.size / 8 + 256);
            if (!e) {
                for (size_t j = 0; j < ns; ++j) reinterpret_cast<unsigned long long*>(d->h_meta())[j] = kDigestClean;
                std::memset(d->h_meta() + 8 * ns, 0, y.base - 8 * ns);
                cmp_fill(y, in.data(), d->h_meta());
                e = chk(hipMemcpyAsync(d->d_meta(), d->h_meta(), y.rows, hipMemcpyHostToDevice, st), "H2D compare tables");
            }
            if (!e) e = chk(hipEventRecord(d->e0, st), "event record");
            if (!e) e = compare_kernels(d, y, reinterpret_cast<unsigned long long*>(d->d_meta()), st);
            if (!e) e = chk(hipEventRecord(d->e1, st), "event record");
            if (!e) e = chk(hipMemcpyAsync(d->h_meta(), d->d_meta(), 8 * ns, hipMemcpyDeviceToHost, st), "D2H validation keys");
            if (!e) e = compare_fetch(d, y, st);
            if (!e) e = chk(hipStreamSynchronize(st), "synchronize");
            if (!e && device_ms) (void)hipEventElapsedTime(device_ms, d->e0, d->e1);
            if (prev_device >= 0) (void)hipSetDevice(prev_device);
            if (e) {
                rc = decode_fail(LACX_E_DEVICE, std::string(e.what) + ": " + hipGetErrorString(e.e));
            } else {
                compare_keep(d, y);
                const auto* bad = reinterpret_cast<const unsigned long long*>(d->h_meta());
                for (size_t a = 0; a < apairs.size(); ++a) {
                    const uint32_t k = which[a];
                    for (uint32_t at : {pairs[k].a, pairs[k].b}) {
                        const unsigned long long key = bad[used[at]];
                        if (c.code[k] != LACX_OK || key == kDigestClean) continue;
                        ImportBad b{{kImportClean, kImportClean}};  // the encoder's words for it (import_msg.h)
                        b.key[key >> 63] = key & ~(1ull << 63);
                        int ch = 0;
                        unsigned long long index = 0;
                        std::string text;
                        (void)import_bad_message(b, src[at].bit_depth, &ch, &index, text);
                        c.code[k] = LACX_E_INVALID, c.err[k] = "source " + std::to_string(at) + ": " + text;
                    }
                    if (c.code[k] == LACX_OK) cmp_accept(d, k, a, fmt[pairs[k].a].sample_rate, out);
                }
            }
        }
    }
    if (rc != LACX_OK) {  // the whole call failed: no pair has an answer
        cmp_reset(d, npairs, out, nullptr);
        for (uint32_t k = 0; k < npairs; ++k)
            if (c.code[k] == LACX_OK) c.code[k] = rc, c.err[k] = g_decode_err;
    }
    return cmp_outcome(d, rc, c, pair_rc);
}

int lacx_decoder_item_compare_rows(const lacx_decoder* d, uint32_t pair, const lacx_compare_row** rows, uint32_t* count) {
    if (rows) *rows = nullptr;
    if (count) *count = 0;
    if (!d || !rows || !count) return decode_fail(LACX_E_INVALID, "null argument");
    if (pair >= d->cmp_ok.size() || !d->cmp_ok[pair]) return decode_fail(LACX_E_INVALID, "no such pair in the last compare call");
    const CmpPair& p = d->cmp_at.pair[d->cmp_slot[pair]];
    *rows = d->cmp_rows.data() + p.row0;
    *count = (uint32_t)p.nrows;
    return LACX_OK;
}

int lacx_decoder_item_compare_counts(const lacx_decoder* d, uint32_t pair, const uint64_t** counts, uint32_t* count) {
    if (counts) *counts = nullptr;
    if (count) *count = 0;
    if (!d || !counts || !count) return decode_fail(LACX_E_INVALID, "null argument");
    if (pair >= d->cmp_ok.size() || !d->cmp_ok[pair]) return decode_fail(LACX_E_INVALID, "no such pair in the last compare call");
    const CmpPair& p = d->cmp_at.pair[d->cmp_slot[pair]];
    if (p.radius == 0) return LACX_OK;  // not searched
    *counts = d->cmp_counts.data() + p.count0;
    *count = cmp_width(p);
    return LACX_OK;
}

int lacx_compare_combine(const lacx_compare_row* rows, uint32_t count, uint8_t channels, uint8_t bit_depth, uint32_t sample_rate, uint64_t frames_a,
                         uint64_t frames_b, int64_t offset, lacx_compare* out) {
    if (out) std::memset(out, 0, sizeof(*out));
    if (!out || (!rows && count)) return decode_fail(LACX_E_INVALID, "null argument");
    if (channels != 1 && channels != 2) return decode_fail(LACX_E_INVALID, "unsupported channel count");
    if (bit_depth != 16 && bit_depth != 24) return decode_fail(LACX_E_INVALID, "unsupported bit depth: " + std::to_string((int)bit_depth));
    if ((frames_a >> 32) || (frames_b >> 32) || offset <= -(1ll << 31) || offset >= (1ll << 31)) return decode_fail(LACX_E_INVALID, "frames or offset out of range");
    if (cmp_rows_at(frames_a, frames_b, offset) != count) return decode_fail(LACX_E_INVALID, "row count is not the domain's");
    *out = cmp_combine(rows, count, channels, bit_depth, sample_rate, frames_a, frames_b, offset);
    return LACX_OK;
}

int lacx_manifest_build(const lacx_digest* dg, const lacx_block_digest* rows, uint32_t count, uint8_t** out, uint64_t* size) {
    if (out) *out = nullptr;
    if (size) *size = 0;
    if (!dg || !rows || !out || !size || count == 0) return decode_fail(LACX_E_INVALID, "null argument or no rows");
    std::vector<uint8_t> m;
    std::string why;
    const int rc = manifest_build(*dg, rows, count, m, why);
    if (rc != LACX_OK) return decode_fail(rc, why);
    uint8_t* buf = static_cast<uint8_t*>(std::malloc(m.size()));
    if (!buf) return decode_fail(LACX_E_RUNTIME, "out of host memory");
    std::memcpy(buf, m.data(), m.size());
    *out = buf;
    *size = m.size();
    return LACX_OK;
}

int lacx_manifest_parse(const uint8_t* m, uint64_t size, lacx_manifest_info* info, lacx_block_digest* rows, uint32_t rows_cap) {
    std::string why;
    const int rc = manifest_parse(m, size, info, rows, rows_cap, why);
    return rc == LACX_OK ? rc : decode_fail(rc, why);
}

int lacx_decoder_item_faults(const lacx_decoder* d, uint32_t i, const lacx_block_fault** faults, uint32_t* count) {
    if (faults) *faults = nullptr;
    if (count) *count = 0;
    if (!d || !faults || !count) return decode_fail(LACX_E_INVALID, "null argument");
    if (i >= d->item_faults.size()) return decode_fail(LACX_E_INVALID, "no such item in the last salvage call");
    *faults = d->item_faults[i].data();
    *count = (uint32_t)d->item_faults[i].size();
    return LACX_OK;
}

const char* lacx_block_fault_text(uint32_t code) { return block_error(code); }

uint32_t lacx_crc32_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b) { return crc32_combine(crc_a, crc_b, len_b); }

const char* lacx_decoder_item_error(const lacx_decoder* d, uint32_t i) {
    if (!d || i >= d->item_err.size()) return "";
    return d->item_err[i].c_str();
}

int lacx_decode(int device, const uint8_t* lac, uint64_t size, int32_t* left, int32_t* right, uint64_t frames,
                float* device_ms) {
    int dev = device;
    if (dev < 0 && hipGetDevice(&dev) != hipSuccess) dev = -1;
    if (dev < 0 || dev >= kMaxDecodeDevices) {
        if (lacx_device_count() <= 0) {  // (parse errors come first, as before)
            lacx_stream_info info;
            const int prc = lacx_stream_parse(lac, size, &info);
            return prc ? prc : decode_fail(LACX_E_DEVICE, "no usable HIP device");
        }
        return decode_fail(LACX_E_DEVICE, "HIP device ordinal out of range");
    }
    SharedDecoder* sd = nullptr;
    {
        std::lock_guard<std::mutex> lock(g_shared_mu);
        if (!g_shared[dev]) {
            g_shared[dev] = new SharedDecoder();
            g_shared[dev]->dec.device = dev;
        }
        sd = g_shared[dev];
    }
    std::lock_guard<std::mutex> lock(sd->mu);
    lacx_decoder* d = &sd->dec;
    return lacx_decoder_decode(d, lac, size, left, right, frames, device_ms);
}
