// decode_plan.h -- the host-only half of the decoder's host side: the plan of a decode job (its streams parsed by container.h) --
// which blocks every item needs, where its payload, PCM and image lie in the job's buffers, the lane table, the layout
// of the tables the kernels read, and the capacities the run must provide.  Plain C++, no HIP: api_decode.cpp runs a
// plan on the device, tests/native/sim_decode.cpp runs the same plan on the host.
#pragma once
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "accuraterip_plan.h"
#include "compare_plan.h"
#include "container.h"
#include "lacx.h"
#include "lacx_types.h"
#include "loudness_plan.h"
#include "manifest.h"
#include "runs_plan.h"
#include "spectrum_plan.h"
#include "truepeak_plan.h"

namespace lacx {

// the decoded WAV image of a stream: 44-byte header, data, pad byte (below 2^32: parse_stream's RIFF limit)
inline uint64_t wav_image_bytes(const lacx_stream_info& f) {
    const uint64_t data = f.frames * (uint64_t)f.channels * (f.bit_depth / 8u);
    return 44u + data + (data & 1u);
}

// One item of a decode job: the stream, and for the device and host forms the caller's output arrays.  With a sample type
// (window job): frames [start, start + frames) of the stream, as that sample type.
struct BatchIn {
    const uint8_t* lac;
    uint64_t size;
    int32_t* left;
    int32_t* right;
    uint64_t frames;
    uint64_t start = 0;
    // verify form: the source PCM (device-resident), or -- lacx_decoder_verify_wav, a batch of one -- the WAV data chunk
    // in host memory, which the decoder uploads behind the payload and VerifySource::data0 then points at
    lacx_pcm pcm = {nullptr, nullptr, 0, 0};
    const uint8_t* host_src = nullptr;
    uint64_t host_src_bytes = 0;
    // a job with block digests: the item's manifest, or null -- nothing is expected of its blocks
    const uint8_t* manifest = nullptr;
    uint64_t manifest_size = 0;
    // a runs job: the item's detectors (its lacx_run_query resolved), or why they are refused (check_detectors)
    const lacx_run_detector* dets = nullptr;
    uint32_t ndet = 0;
    const char* dets_why = nullptr;
};

// Where the decoded items go.  wav: the images into the decoder's pinned image buffer (each item's 16-byte aligned, one
// D2H copy for all).  device: the caller's device arrays, in place, on the caller's stream.  host: the decoder's own PCM
// buffers, then, once the statuses are checked, the caller's host arrays of the items that decoded.  verify: the
// decoder's own PCM buffers, compared there with each item's source PCM (k_verify in place of the other post passes);
// what comes back is a result per item and, for an item that differs, LACX_E_MISMATCH.  digest: the decoder's own PCM
// buffers like verify, digested there (k_digest in place of the other post passes); what comes back is one result word
// per item (DigestWords).
// The device and host forms also come as window jobs (sample_type = LACX_SAMPLE_I32 / _F32 instead of kWholeStreams,
// DESIGN §6b): a version-3 item then covers just the blocks that overlap its window -- only their bytes are uploaded,
// they decode whole into the decoder's PCM buffers (scratch) and are all checked, and k_window_out writes the window's
// frames out; a version-2 item (no compressed sizes) decodes in full and is then windowed.  The host form's windows go
// through the decoder's image buffer, copied to the caller once the statuses are checked.
// The wav and device forms also come as salvage jobs (DecodePlan::salvage, lacx_decoder_salvage_*): the items are read
// by scan_stream, so a version-3 file may end early -- only its present blocks get a lane, only their bytes are payload --
// and the post pass is k_ms_inverse in place, then k_salvage_wav / k_salvage_blank over the final status words.
// A salvage job may carry block digests (DecodePlan::blocks, lacx_decoder_digest_blocks_* / _check_* / *_checked):
// k_digest_blocks behind k_ms_inverse leaves one raw word per global block, and where an item has a manifest
// (DecodePlan::judged) k_digest_judge compares them with the expected words and stores status 11 in front of the salvage
// pass.  blocks: the form of such a job that outputs nothing -- the decoder's own PCM buffers as verify and digest have
// them, and no salvage pass.
// The blocks form is also that of a stats job (DecodePlan::stats, lacx_decoder_stats_batch_device): the same salvage job
// with k_stats_blocks (stats_core.h) in place of k_digest_blocks -- no manifests, no judge, no raw words; one accumulator
// row of kStatsRowBytes per global block instead, zeroed with the tables.
// ... and of a runs job (DecodePlan::runs, lacx_decoder_runs_batch_device): the same salvage job with k_runs (runs_core.h)
// in that slot -- behind present [m] the tables of runs_plan.h (DecodePlan::runs_at), the lists in a buffer of their own.
// The digest form is also that of a loudness job (DecodePlan::loudness, lacx_decoder_loudness_batch_device): the same strict
// job with k_ms_inverse in place and then the four loudness kernels (loudness_core.h) in the slot k_digest has -- behind
// res [m] the tables of loudness_plan.h (DecodePlan::loud_at), whose items are the decoder's own PCM buffers as planar
// int32 sources; the scratch is a buffer of its own.
// ... and of a true-peak job (DecodePlan::truepeak, lacx_decoder_truepeak_batch_device): the same strict job with k_truepeak
// (truepeak_core.h) in that slot -- behind res [m] the tables of truepeak_plan.h (DecodePlan::peak_at), zeroed rows included.
// ... and of a spectrum job (DecodePlan::spectrum, lacx_decoder_spectrum_batch_device): likewise with k_spectrum
// (spectrum_core.h) -- behind res [m] the tables of spectrum_plan.h (DecodePlan::spec_at), window, twiddles and zeroed rows.
// ... and of a rip-checksum job (DecodePlan::accuraterip, lacx_decoder_accuraterip_batch_device): likewise with k_accuraterip
// (accuraterip_core.h) -- behind res [m] the tables of accuraterip_plan.h (DecodePlan::ar_at).  Its discs are runs of
// consecutive items (ArJobIn); a disc's items lie side by side in the decoder's PCM buffers, but the kernel reads them
// through the disc's source table, so nothing depends on that.
// ... and of a bit-compare job (DecodePlan::compare, lacx_decoder_compare_batch_device): likewise with k_compare_search and
// k_compare_rows (compare_core.h) -- behind res [m] the tables of compare_plan.h (DecodePlan::cmp_at).  Its sources are the
// planned items, each once however many pairs name it; the kernels read them through the source table.
enum class DecodeForm { wav, device, host, verify, digest, blocks };
constexpr int kWholeStreams = -1;
constexpr size_t kStatsRowBytes = 96;  // sizeof(StatsAcc), stats_core.h (k_stats.hip asserts it)

// The discs of a rip-checksum job: ArDiscIn::src0 / nsrc name items of the job's BatchIn array; every disc has passed
// ar_disc_why with its items' parsed frame counts (the caller parses them first: the track lengths may default to them).
struct ArJobIn {
    const ArDiscIn* discs;
    uint32_t ndiscs;
};

// The pairs of a bit-compare job: CmpPairIn::a / b name items of the job's BatchIn array; every pair has passed cmp_pair_why
// with its items' parsed formats.
struct CmpJobIn {
    const CmpPairIn* pairs;
    uint32_t npairs;
};

// One item that goes to the device (j counts these; the items that failed their checks are not among them).
struct PlanItem {
    uint32_t src;        // its index in the job's BatchIn array
    uint32_t blk_first;  // what it decodes: its blocks from blk_first on (item.blocks of them) ...
    uint64_t pay_src;    // ... and their pay_bytes payload bytes from pay_src on, counted from the end of the stream's
    uint64_t pay_bytes;  //     head (0 and the whole stream but for a window)
    uint64_t head;       // stream_head_bytes of the stream
    uint64_t pcm_at;     // own PCM buffers: the item's first frame there, a multiple of 4 (16-byte loads)
    uint64_t image_at, image_size;  // image buffer: the WAV image (16-byte aligned), or a host window's left, then right
    lacx_stream_info info;
    DecodeItem item;     // left / right / wav are null until plan_fill_tables
    WindowOut win;       // window job; left / right as above
    uint32_t present_blocks;  // the blocks whose bytes the file holds, a prefix: item.blocks but for a truncated salvage item
    uint32_t scan_flags;      // salvage job: LACX_SALVAGE_*
    bool judged;              // a job with block digests: the item has a manifest, its rows' CRCs are `expect`
    std::vector<uint32_t> expect;
};

// The tables the kernels read, one upload: items | byte_off [T + 1] | frame_off [T + 1] | unit_off [m + 1] | blk_item [T]
// | lane_blk | v2_items, then for a window job | win [m], for the verify form | ver [m] | res [m], for the digest form
// | res [m] at `win`, for a salvage job | present [m] (uint32) at `win` (byte offsets); with block digests behind that
// | judged [m] (uint32) | raw [T] (uint32, 16-byte aligned) and for a judged job | expect [T] (uint32); a stats job
// behind present [m] | stats [T] (kStatsRowBytes each, 16-byte aligned)
// (inspect_plan.h keeps items .. present [m] of a salvage job's layout and puts its rows behind them: a change of this
// order is a change there too, and plan_inspect refuses a layout it does not know)
struct TableLayout {
    size_t items, byte_off, frame_off, unit_off, blk_item, lane_blk, v2_items, win, res, size;
    size_t judged = 0, raw = 0, expect = 0;  // block digests only
    size_t stats = 0;                        // stats job only
    size_t runs = 0;                         // runs job only: RunsLayout::base
    size_t loud = 0;                         // loudness job only: LoudLayout::base
    size_t peak = 0;                         // true-peak job only: TpLayout::base
    size_t spec = 0;                         // spectrum job only: SpLayout::base
    size_t ar = 0;                           // rip-checksum job only: ArLayout::base
    size_t cmp = 0;                          // bit-compare job only: CmpLayout::base
};

struct DecodePlan {
    DecodeForm form = DecodeForm::host;
    int sample_type = kWholeStreams;
    bool salvage = false;  // wav and device forms of whole streams only, and the blocks form
    bool blocks = false;   // salvage job with block digests; judged: one item at least has a manifest
    bool judged = false;
    bool stats = false;    // salvage job in the blocks form with the statistics' accumulator rows (no block digests)
    bool runs = false;     // salvage job in the blocks form with the run finder's tables (no block digests, no statistics)
    uint64_t runs_list_cap = 0;
    RunsLayout runs_at{};  // ... inside the tables (byte offsets from the tables' first byte)
    bool loudness = false; // strict job in the digest form with the loudness kernels in k_digest's place
    LoudLayout loud_at{};  // ... inside the tables, and the scratch's layout
    bool truepeak = false; // strict job in the digest form with k_truepeak in k_digest's place
    TpLayout peak_at{};    // ... inside the tables
    uint32_t spectrum = 0; // strict job in the digest form with k_spectrum in k_digest's place: the window length, 0: none
    SpLayout spec_at{};    // ... inside the tables
    bool accuraterip = false;  // strict job in the digest form with k_accuraterip in k_digest's place
    ArLayout ar_at{};          // ... inside the tables
    // ... its discs that go to the device (every item of theirs does): src0 / nsrc name ar_src, whose entries name the
    // planned items j (ArSrcIn::item; addresses null until plan_fill_tables); ar_disc[k]: the disc's index in the job
    std::vector<ArDiscIn> ar_discs;
    std::vector<ArSrcIn> ar_src;
    std::vector<uint32_t> ar_disc;
    bool compare = false;      // strict job in the digest form with k_compare_search / k_compare_rows in k_digest's place
    CmpLayout cmp_at{};        // ... inside the tables
    // ... its sources (one per planned item j, ArSrcIn-like: item = j; addresses null until plan_fill_tables), its pairs that
    // go to the device (both items do; a / b name cmp_src) and cmp_pair[k]: the pair's index in the job
    std::vector<CmpSrcIn> cmp_src;
    std::vector<CmpPairIn> cmp_pairs;
    std::vector<uint32_t> cmp_pair;
    bool window() const { return sample_type != kWholeStreams; }
    bool own_pcm() const { return form != DecodeForm::device || window(); }  // into the decoder's PCM buffers
    bool post_units() const { return window() || form == DecodeForm::verify || form == DecodeForm::wav || form == DecodeForm::digest || blocks || stats || runs; }
    bool host_window() const { return form == DecodeForm::host && window(); }
    std::vector<PlanItem> items;
    // k_decode's lanes: lane g decodes global block lane_blk[g] (~0u: idle); version-3 blocks only, an item's in
    // consecutive lanes.  v2_items: the version-2 items, one lane each (k_decode_serial)
    std::vector<uint32_t> lane_blk, v2_items;
    uint64_t total_blocks = 0, total_frames = 0, total_pay = 0, total_units = 0, pcm_total = 0, image_total = 0;
    // the verify form of a WAV image in host memory (a batch of one): the data chunk lies behind the payload and its pad,
    // at the 16-byte aligned src_at (a device allocation's base is aligned further)
    const uint8_t* host_src = nullptr;
    uint64_t host_src_bytes = 0, src_at = 0;
    TableLayout at{};
    // What the run must provide (0: that buffer is not used).  payload: bytes, with kDecodeTailPad behind the last block
    // (and behind the host source, where there is one); blocks: status and flag entries; pcm_frames: samples of each
    // channel's buffer; image, stage (the pinned payload stage of a window job), tables: bytes.  stats_rows: the
    // accumulator rows of a stats job, which lie inside the tables at TableLayout::stats.  runs_list: the entries
    // (lacx_run) of a runs job's list buffer.  loud_scratch: the bytes of a loudness job's scratch.
    struct {
        uint64_t payload, blocks, pcm_frames, image, stage, tables, stats_rows, runs_list, loud_scratch;
    } need{};
};

namespace plan_detail {
inline const char* check_window(const BatchIn& x, const lacx_stream_info& f) {  // inside the stream (no wrap-around), then the arrays
    if (x.frames == 0) return "empty window";
    if (x.start >= f.frames || x.frames > f.frames - x.start) return "window outside the stream";
    if (!x.left || (f.channels == 2 && !x.right)) return "output arrays missing";
    return nullptr;
}
inline const char* check_source(const BatchIn& x, const lacx_stream_info& f) {  // the verify form's source against the stream
    const lacx_pcm& p = x.pcm;
    const uintptr_t a0 = (uintptr_t)p.data0, a1 = (uintptr_t)p.data1;
    const bool tensor = p.layout == LACX_PCM_PLANAR_I16 || p.layout == LACX_PCM_PLANAR_F32 || p.layout == LACX_PCM_INTERLEAVED_F32;
    const bool planar = p.layout == LACX_PCM_PLANAR_I32 || p.layout == LACX_PCM_PLANAR_I16 || p.layout == LACX_PCM_PLANAR_F32;
    if (p.layout > LACX_PCM_INTERLEAVED_I24 && !tensor) return "unknown source layout";
    if (p.channels != f.channels) return "source channel count does not match the stream";
    if ((!p.data0 && !x.host_src) || (planar && p.channels == 2 && !p.data1)) return "source arrays missing";
    if (x.frames != f.frames) return "source frame count does not match the stream";
    if (((p.layout == LACX_PCM_INTERLEAVED_I16 || p.layout == LACX_PCM_PLANAR_I16) && f.bit_depth != 16) ||
        (p.layout == LACX_PCM_INTERLEAVED_I24 && f.bit_depth != 24))
        return "source layout does not match the stream's bit depth";
    if (p.layout == LACX_PCM_PLANAR_I16) {
        if ((a0 & 1u) || (a1 & 1u)) return "source arrays are not 2-byte aligned";
    } else if ((p.layout != LACX_PCM_INTERLEAVED_I24 && (a0 & 3u)) || (planar && (a1 & 3u))) {
        return "source arrays are not 4-byte aligned";
    }
    return nullptr;
}
inline const char* check_arrays(const BatchIn& x, const lacx_stream_info& f) {  // lacx_decoder_decode's checks of the output arrays
    if (!x.left || (f.channels == 2 && !x.right)) return "output arrays missing";
    if (x.frames != f.frames) return "output arrays do not match the stream's frame count";
    return nullptr;
}
constexpr size_t up16(size_t v) { return (v + 15u) & ~(size_t)15u; }
// A judged item: its manifest parsed (a refusal keeps the parser's text) and compared with the stream it is to judge --
// the format and every block's frame count; a difference is an answer that needs no device.  expect: the rows' CRCs.
inline int check_manifest(const BatchIn& x, const lacx_stream_info& f, std::vector<uint32_t>& expect, std::string& why) {
    lacx_manifest_info mi{};
    std::vector<lacx_block_digest> rows((size_t)(x.manifest_size >= kManifestFixed ? (x.manifest_size - kManifestFixed) / 8u : 0u));
    const int rc = manifest_parse(x.manifest, x.manifest_size, &mi, rows.data(), (uint32_t)rows.size(), why);
    if (rc != LACX_OK) return rc;
    auto differs = [&](const std::string& field, uint64_t a, uint64_t b) {
        why = "[check-error] " + field + ": stream " + std::to_string(a) + ", manifest " + std::to_string(b);
        return LACX_E_MISMATCH;
    };
    if (mi.channels != f.channels) return differs("channels", f.channels, mi.channels);
    if (mi.bit_depth != f.bit_depth) return differs("bit depth", f.bit_depth, mi.bit_depth);
    if (mi.sample_rate != f.sample_rate) return differs("sample rate", f.sample_rate, mi.sample_rate);
    if (mi.frames != f.frames) return differs("frames", f.frames, mi.frames);
    if (mi.blocks != f.blocks) return differs("blocks", f.blocks, mi.blocks);
    expect.resize(mi.blocks);
    for (uint32_t b = 0; b < mi.blocks; ++b) {
        const uint32_t n = row_frames(x.lac, f.version, b);
        if (rows[b].frames != n) return differs("block " + std::to_string(b) + " frames", n, rows[b].frames);
        expect[b] = rows[b].crc32;
    }
    return LACX_OK;
}
}  // namespace plan_detail

// Plans n streams as one decode (a single stream is n = 1).  Every item is parsed and checked on the host; those that
// pass go to the device together: their payloads back to back in one buffer (the tail pad after the last), their block
// tables as global prefix sums, one lane per version-3 block and one per version-2 item, then one post pass over all of
// them.  Per item, code[i] and err[i] ("" = goes to the device).  pad_waves: every item's blocks start a new wave.
// Returns null, or why the job as a whole cannot run (nothing is laid out then).
// salvage: a salvage job (DecodeForm above): an item's blocks and frames are still the whole table's, its payload the
// bytes of its present blocks.
inline const char* plan_decode_job(const BatchIn* in, uint32_t n, DecodeForm form, int sample_type, bool pad_waves, DecodePlan& plan,
                                   std::vector<int>& code, std::vector<std::string>& err, bool salvage, bool blocks, bool stats, bool runs,
                                   uint64_t runs_list_cap, bool loudness, bool truepeak, uint32_t spectrum, const ArJobIn* ar, const CmpJobIn* cmp) {
    using namespace plan_detail;
    plan = DecodePlan{};
    plan.form = form;
    plan.sample_type = sample_type;
    plan.salvage = salvage;
    plan.blocks = blocks;
    plan.stats = stats;
    plan.runs = runs;
    plan.loudness = loudness;
    plan.truepeak = truepeak;
    plan.spectrum = spectrum;
    plan.accuraterip = ar != nullptr;
    plan.compare = cmp != nullptr;
    const bool window = plan.window(), own_pcm = plan.own_pcm(), wav = form == DecodeForm::wav, verify = form == DecodeForm::verify,
               digest = form == DecodeForm::digest, quiet = form == DecodeForm::blocks;
    code.assign(n, LACX_OK);
    err.assign(n, std::string());
    if (salvage && (sample_type != kWholeStreams || (form != DecodeForm::wav && form != DecodeForm::device && !quiet))) return "salvage is a whole-stream WAV or device job";
    if (stats && (!quiet || blocks || !salvage)) return "statistics are a salvage job in the blocks form without block digests";
    if (runs && (!quiet || blocks || stats || !salvage)) return "runs are a salvage job in the blocks form without block digests or statistics";
    if ((quiet && !blocks && !stats && !runs) || (blocks && !salvage)) return "block digests belong to a salvage job";
    if (loudness && (!digest || salvage)) return "loudness is a strict job in the digest form";
    if (truepeak && (!digest || salvage || loudness)) return "true peak is a strict job in the digest form";
    if (spectrum && (!digest || salvage || loudness || truepeak || !sp_logn(spectrum))) return "spectrum is a strict job in the digest form with a supported window";
    if (ar && (!digest || salvage || loudness || truepeak || spectrum)) return "rip checksums are a strict job in the digest form";
    if (cmp && (!digest || salvage || loudness || truepeak || spectrum || ar)) return "bit-compare is a strict job in the digest form";
    plan.items.reserve(n);
    uint32_t v3_blocks = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const BatchIn& x = in[i];
        PlanItem p{};
        lacx_stream_info& f = p.info;
        const char* why = nullptr;
        int c = salvage ? scan_stream(x.lac, x.size, &f, &p.present_blocks, &p.scan_flags, &why) : parse_stream(x.lac, x.size, &f, &why);
        if (c == LACX_OK && (why = window ? check_window(x, f) : verify ? check_source(x, f) : wav || digest || quiet ? nullptr : check_arrays(x, f)))
            c = LACX_E_INVALID;
        if (c == LACX_OK && runs && x.dets_why) why = x.dets_why, c = LACX_E_INVALID;
        std::string text;
        if (c == LACX_OK && blocks && x.manifest) {
            p.judged = true;
            if ((c = check_manifest(x, f, p.expect, text)) != LACX_OK) why = text.c_str();
        }
        if (c != LACX_OK) {
            code[i] = c;
            err[i] = why;
            continue;
        }
        plan.judged = plan.judged || p.judged;
        p.src = i;
        p.head = stream_head_bytes(f.version, f.blocks);
        uint32_t nb = f.blocks;
        uint64_t frames = f.frames, fr0 = 0;
        p.pay_bytes = x.size - p.head;
        if (salvage && f.version != 2) {  // the present blocks' bytes: not those of a cut block, not what trails the last
            p.pay_bytes = 0;
            for (uint32_t b = 0; b < p.present_blocks; ++b) p.pay_bytes += row_bytes(x.lac, b);
        }
        if (window && f.version != 2) {  // the blocks [blk_first, blk_first + nb) that hold the window's first and last frames
            const uint64_t last = x.start + x.frames - 1;
            uint64_t fr = 0, by = 0;
            for (uint32_t b = 0;; ++b) {  // (the parse guarantees that the window's last frame lies in a block)
                const uint32_t nfr = row_frames(x.lac, f.version, b), nby = row_bytes(x.lac, b);
                if (fr <= x.start && x.start < fr + nfr) p.blk_first = b, p.pay_src = by, fr0 = fr;
                if (last < fr + nfr) {
                    nb = b + 1 - p.blk_first;
                    p.pay_bytes = by + nby - p.pay_src;
                    frames = fr + nfr - fr0;
                    break;
                }
                fr += nfr;
                by += nby;
            }
        }
        if (!salvage) p.present_blocks = nb;  // (a window's blocks: all of them lie inside a file the strict parser took)
        if (window) {
            p.win = WindowOut{nullptr, nullptr, x.start - fr0, x.frames};
            p.image_at = plan.image_total;  // the host form's staging: left, then right
            p.image_size = 4 * x.frames * f.channels;
            plan.image_total += p.image_size;
        }
        if (wav) {
            p.image_at = plan.image_total;
            p.image_size = wav_image_bytes(f);
            plan.image_total += up16(p.image_size);
        }
        if (plan.post_units()) plan.total_units += (frames + 3u) / 4u;  // the post passes' units of 4 frames
        DecodeItem& y = p.item;
        y.frame0 = plan.total_frames;
        y.frames = frames;
        y.pay_off = plan.total_pay;
        y.block0 = (uint32_t)plan.total_blocks;
        y.blocks = nb;
        y.pay_bits = f.version == 2 ? (uint32_t)(8ull * (x.size - p.head)) : 0u;  // < 2^32: parse_stream
        y.channels = f.channels;
        y.stereo_mode = f.stereo_mode;
        y.bit_depth = f.bit_depth;
        y.version = f.version;
        if (own_pcm) {
            p.pcm_at = plan.pcm_total;
            plan.pcm_total += (frames + 3u) & ~3ull;
        }
        plan.total_blocks += nb;
        plan.total_frames += frames;
        plan.total_pay += p.pay_bytes;
        if (f.version != 2) v3_blocks += nb;
        plan.items.push_back(p);
    }
    if (plan.total_blocks >= (1ull << 31)) return "batch holds 2^31 blocks or more";
    const size_t m = plan.items.size(), T = (size_t)plan.total_blocks;
    plan.lane_blk.reserve(v3_blocks);
    for (uint32_t j = 0; j < m; ++j) {
        const DecodeItem& y = plan.items[j].item;
        if (y.version == 2) {
            plan.v2_items.push_back(j);
            continue;
        }
        if (pad_waves) while (plan.lane_blk.size() % 64u) plan.lane_blk.push_back(~0u);
        for (uint32_t b = 0; b < plan.items[j].present_blocks; ++b) plan.lane_blk.push_back(y.block0 + b);
    }
    if (verify && m == 1 && in[plan.items[0].src].host_src) {
        plan.host_src = in[plan.items[0].src].host_src;
        plan.host_src_bytes = in[plan.items[0].src].host_src_bytes;
        plan.src_at = up16(plan.total_pay + kDecodeTailPad);
    }
    TableLayout& at = plan.at;
    at.items = 0;
    at.byte_off = up16(sizeof(DecodeItem) * m);
    at.frame_off = at.byte_off + 8 * (T + 1);
    at.unit_off = at.frame_off + 8 * (T + 1);
    at.blk_item = at.unit_off + 8 * (m + 1);
    at.lane_blk = at.blk_item + 4 * T;
    at.v2_items = at.lane_blk + 4 * plan.lane_blk.size();
    const size_t end = at.v2_items + 4 * plan.v2_items.size();
    at.win = up16(end);
    at.res = digest ? at.win : at.win + sizeof(VerifySource) * m;
    if (blocks) {
        at.judged = at.win + 4 * m;
        at.raw = at.res = up16(at.judged + 4 * m);
        at.expect = at.raw + 4 * T;
    }
    if (stats) at.stats = up16(at.win + 4 * m);
    std::vector<RunsIn> rin;
    if (runs) {
        for (const PlanItem& p : plan.items) rin.push_back(RunsIn{in[p.src].dets, in[p.src].ndet, p.item.frames});
        at.runs = up16(at.win + 4 * m);
        plan.runs_at = runs_layout(at.runs, rin.data(), m);
        if (plan.runs_at.total_tiles >= (1ull << 31)) return "batch holds 2^31 tiles or more";
        for (const RunsIn& r : rin)  // (what runs_fill will reserve)
            for (uint32_t k = 0; k < r.ndet; ++k) plan.need.runs_list += runs_reserve(r.frames, r.dets[k].min_frames, runs_list_cap);
        plan.runs_list_cap = runs_list_cap;
    }
    if (loudness) {  // the items' addresses are plan_fill_tables's; the layout needs frames, channels and rates alone
        std::vector<LoudIn> lin;
        for (const PlanItem& p : plan.items) lin.push_back(LoudIn{nullptr, nullptr, p.item.frames, p.info.sample_rate, (uint32_t)LACX_PCM_PLANAR_I32, p.info.channels, p.info.bit_depth, false});
        if (const char* why = loud_check(lin.data(), m)) return why;
        at.loud = up16(at.res + sizeof(DigestWords) * m);
        plan.loud_at = loud_layout(at.loud, lin.data(), m);
        plan.need.loud_scratch = plan.loud_at.scratch;
    }
    if (truepeak) {  // as loudness: the items' addresses are plan_fill_tables's
        std::vector<TpIn> tin;
        for (const PlanItem& p : plan.items) tin.push_back(TpIn{nullptr, nullptr, p.item.frames, (uint32_t)LACX_PCM_PLANAR_I32, p.info.channels, p.info.bit_depth, false});
        if (const char* why = tp_check(tin.data(), m)) return why;
        at.peak = up16(at.res + sizeof(DigestWords) * m);
        plan.peak_at = tp_layout(at.peak, tin.data(), m);
    }
    if (spectrum) {  // likewise
        std::vector<SpIn> xin;
        for (const PlanItem& p : plan.items) xin.push_back(SpIn{nullptr, nullptr, p.item.frames, (uint32_t)LACX_PCM_PLANAR_I32, p.info.channels, p.info.bit_depth, false});
        if (const char* why = sp_check(xin.data(), m, sp_logn(spectrum))) return why;
        at.spec = up16(at.res + sizeof(DigestWords) * m);
        plan.spec_at = sp_layout(at.spec, xin.data(), m, sp_logn(spectrum));
    }
    if (ar) {  // likewise; a disc one of whose items was refused above (or is no 16-bit stereo) does not go to the device
        std::vector<uint32_t> where(n, ~0u);
        for (uint32_t j = 0; j < m; ++j) where[plan.items[j].src] = j;
        for (uint32_t k = 0; k < ar->ndiscs; ++k) {
            ArDiscIn d = ar->discs[k];
            bool whole = d.nsrc != 0 && d.src0 <= n && d.nsrc <= n - d.src0;
            for (uint32_t i = 0; whole && i < d.nsrc; ++i) {
                const uint32_t j = where[d.src0 + i];
                whole = j != ~0u && plan.items[j].info.channels == 2 && plan.items[j].info.bit_depth == 16 && plan.items[j].item.frames != 0;
            }
            if (!whole) continue;
            const uint32_t first = (uint32_t)plan.ar_src.size();
            for (uint32_t i = 0; i < d.nsrc; ++i) {
                const uint32_t j = where[d.src0 + i];
                plan.ar_src.push_back(ArSrcIn{nullptr, nullptr, plan.items[j].item.frames, (uint32_t)LACX_PCM_PLANAR_I32, j});
            }
            d.src0 = first, d.validate = false;
            plan.ar_discs.push_back(d);
            plan.ar_disc.push_back(k);
        }
        if (const char* why = ar_check(plan.ar_src.data(), plan.ar_discs.data(), plan.ar_discs.size())) return why;
        at.ar = up16(at.res + sizeof(DigestWords) * m);
        plan.ar_at = ar_layout(at.ar, plan.ar_src.data(), plan.ar_discs.data(), plan.ar_discs.size());
    }
    if (cmp) {  // likewise; a pair one of whose items was refused above does not go to the device
        std::vector<uint32_t> where(n, ~0u);
        for (uint32_t j = 0; j < m; ++j) {
            where[plan.items[j].src] = j;
            const PlanItem& p = plan.items[j];
            plan.cmp_src.push_back(CmpSrcIn{nullptr, nullptr, p.item.frames, (uint32_t)LACX_PCM_PLANAR_I32, j, (uint8_t)p.info.channels, (uint8_t)p.info.bit_depth, false});
        }
        for (uint32_t k = 0; k < cmp->npairs; ++k) {
            CmpPairIn q = cmp->pairs[k];
            if (q.a >= n || q.b >= n || where[q.a] == ~0u || where[q.b] == ~0u) continue;
            q.a = where[q.a], q.b = where[q.b];
            plan.cmp_pairs.push_back(q);
            plan.cmp_pair.push_back(k);
        }
        if (const char* why = cmp_check(plan.cmp_src.data(), plan.cmp_pairs.data(), plan.cmp_pairs.size())) return why;
        at.cmp = up16(at.res + sizeof(DigestWords) * m);
        plan.cmp_at = cmp_layout(at.cmp, plan.cmp_src.data(), plan.cmp_src.size(), plan.cmp_pairs.data(), plan.cmp_pairs.size());
    }
    at.size = cmp ? plan.cmp_at.size : ar ? plan.ar_at.size : spectrum ? plan.spec_at.size : truepeak ? plan.peak_at.size : loudness ? plan.loud_at.size : runs ? plan.runs_at.size : stats ? at.stats + kStatsRowBytes * T : blocks ? at.expect + (plan.judged ? 4 * T : 0) : salvage ? at.win + 4 * m : verify ? at.res + sizeof(VerifyWords) * m : digest ? at.res + sizeof(DigestWords) * m : window ? at.win + sizeof(WindowOut) * m : end;
    plan.need.payload = (plan.host_src ? plan.src_at + plan.host_src_bytes : plan.total_pay) + kDecodeTailPad;
    plan.need.blocks = T;
    plan.need.pcm_frames = own_pcm ? plan.pcm_total : 0;
    plan.need.image = wav || plan.host_window() ? up16(plan.image_total) : 0;  // k_wav_pack writes whole dwords, and only inside the image
    plan.need.stage = window ? plan.total_pay : 0;
    plan.need.tables = at.size;
    plan.need.stats_rows = stats ? T : 0;
    return nullptr;
}

// plan_decode_job without a bit-compare job: what every caller but the compare calls uses, its parameters defaulted as ever.
inline const char* plan_decode(const BatchIn* in, uint32_t n, DecodeForm form, int sample_type, bool pad_waves, DecodePlan& plan,
                               std::vector<int>& code, std::vector<std::string>& err, bool salvage = false, bool blocks = false,
                               bool stats = false, bool runs = false, uint64_t runs_list_cap = kRunsListCap, bool loudness = false, bool truepeak = false,
                               uint32_t spectrum = 0, const ArJobIn* ar = nullptr) {
    return plan_decode_job(in, n, form, sample_type, pad_waves, plan, code, err, salvage, blocks, stats, runs, runs_list_cap, loudness, truepeak, spectrum, ar, nullptr);
}

// What a salvage job reports for an item, from what every decode copies back anyway: the job's status words (status, by
// global block) and the item's present_blocks.  A block is lost with its lane's or the range check's status (1..9), or --
// behind the present ones, where nobody wrote a status word -- as LACX_BLOCK_MISSING.  faults: the lost blocks, ascending.
inline lacx_salvage_result salvage_report(const PlanItem& p, const uint8_t* lac, const uint32_t* status, std::vector<lacx_block_fault>& faults) {
    lacx_salvage_result r{};
    r.blocks = r.first_bad = p.item.blocks;
    r.frames = p.info.frames;
    r.flags = p.scan_flags;
    faults.clear();
    uint64_t frame = 0;
    for (uint32_t b = 0; b < p.item.blocks; ++b) {
        const uint32_t n = row_frames(lac, p.info.version, b);
        const uint32_t code = b >= p.present_blocks ? LACX_BLOCK_MISSING : status[p.item.block0 + b];
        if (code) {
            if (faults.empty()) r.first_bad = b;
            faults.push_back(lacx_block_fault{b, code, frame, n, 0});
            r.lost_frames += n;
        }
        frame += n;
    }
    r.bad_blocks = (uint32_t)faults.size();
    return r;
}

// The base addresses of the run's buffers, as the kernels will see them.
struct PlanBases {
    uint8_t* payload;
    int32_t* left;  // own PCM buffers
    int32_t* right;
    uint8_t* image;
};

// The plan's offsets as pointers: fills the tables (plan.at, plan.need.tables bytes at h), the verify form's initial result
// words (and the digest form's) among them.
inline void plan_fill_tables(const DecodePlan& plan, const BatchIn* in, const PlanBases& base, uint8_t* h) {
    const TableLayout& at = plan.at;
    const uint32_t m = (uint32_t)plan.items.size();
    auto* items = reinterpret_cast<DecodeItem*>(h + at.items);
    auto* byte_off = reinterpret_cast<unsigned long long*>(h + at.byte_off);
    auto* frame_off = reinterpret_cast<unsigned long long*>(h + at.frame_off);
    auto* unit_off = reinterpret_cast<unsigned long long*>(h + at.unit_off);
    auto* blk_item = reinterpret_cast<uint32_t*>(h + at.blk_item);
    auto* win = reinterpret_cast<WindowOut*>(h + at.win);
    auto* ver = reinterpret_cast<VerifySource*>(h + at.win);
    auto* res = reinterpret_cast<VerifyWords*>(h + at.res);
    byte_off[0] = frame_off[0] = unit_off[0] = 0;
    for (uint32_t j = 0; j < m; ++j) {
        const PlanItem& p = plan.items[j];
        const BatchIn& x = in[p.src];
        DecodeItem y = p.item;
        const bool v2 = y.version == 2, stereo = y.channels == 2;
        for (uint32_t b = 0; b < y.blocks; ++b) {
            const uint32_t g = y.block0 + b;
            const uint64_t sb = p.blk_first + b;  // the block within the stream
            frame_off[g + 1] = frame_off[g] + row_frames(x.lac, y.version, sb);
            // (a missing block of a salvage item has no bytes in the payload buffer, and no lane that would ask)
            byte_off[g + 1] = v2 || b >= p.present_blocks ? byte_off[g] : byte_off[g] + row_bytes(x.lac, sb);
            blk_item[g] = j;
        }
        // the version-2 item's bytes count in the byte offsets as one lump at its last block
        if (v2) byte_off[y.block0 + y.blocks] = y.pay_off + (y.pay_bits >> 3);
        unit_off[j + 1] = unit_off[j] + (y.frames + 3u) / 4u;
        y.left = plan.own_pcm() ? base.left + p.pcm_at : x.left;
        y.right = !stereo ? nullptr : plan.own_pcm() ? base.right + p.pcm_at : x.right;
        if (plan.form == DecodeForm::wav) y.wav = base.image + p.image_at;
        items[j] = y;
        if (plan.window()) {
            WindowOut w = p.win;
            uint8_t* stage = base.image + p.image_at;
            w.left = plan.host_window() ? (void*)stage : x.left;
            w.right = !stereo ? nullptr : plan.host_window() ? (void*)(stage + 4 * w.frames) : x.right;
            win[j] = w;
        }
        if (plan.form == DecodeForm::verify) {
            ver[j] = VerifySource{plan.host_src ? base.payload + plan.src_at : x.pcm.data0, x.pcm.data1, x.pcm.layout, 0};
            res[j] = VerifyWords{0, ~0ull, 0, 0, 0, 0};
        }
        if (plan.form == DecodeForm::digest) reinterpret_cast<DigestWords*>(h + at.res)[j] = DigestWords{0, 0};
        if (plan.salvage) reinterpret_cast<uint32_t*>(h + at.win)[j] = p.present_blocks;
        if (plan.stats) std::memset(h + at.stats + kStatsRowBytes * (size_t)y.block0, 0, kStatsRowBytes * (size_t)y.blocks);
        if (plan.blocks) {
            reinterpret_cast<uint32_t*>(h + at.judged)[j] = p.judged ? 1u : 0u;
            std::memset(h + at.raw + 4 * (size_t)y.block0, 0, 4 * (size_t)y.blocks);
            if (plan.judged) {
                uint32_t* e = reinterpret_cast<uint32_t*>(h + at.expect) + y.block0;
                for (uint32_t b = 0; b < y.blocks; ++b) e[b] = p.judged ? p.expect[b] : 0u;
            }
        }
    }
    if (plan.runs) {
        std::vector<RunsIn> rin;
        for (const PlanItem& p : plan.items) rin.push_back(RunsIn{in[p.src].dets, in[p.src].ndet, p.item.frames});
        RunsLayout y = plan.runs_at;
        runs_fill(y, rin.data(), m, plan.runs_list_cap, h);
    }
    if (plan.loudness) {  // every item as a planar int32 source: its place in the decoder's own PCM buffers
        std::vector<LoudIn> lin;
        for (const PlanItem& p : plan.items)
            lin.push_back(LoudIn{base.left + p.pcm_at, p.item.channels == 2 ? base.right + p.pcm_at : nullptr, p.item.frames, p.info.sample_rate,
                                 (uint32_t)LACX_PCM_PLANAR_I32, p.info.channels, p.info.bit_depth, false});
        loud_fill(plan.loud_at, lin.data(), m, h);
    }
    if (plan.truepeak) {  // the same sources; the rows are zeroed here
        std::vector<TpIn> tin;
        for (const PlanItem& p : plan.items)
            tin.push_back(TpIn{base.left + p.pcm_at, p.item.channels == 2 ? base.right + p.pcm_at : nullptr, p.item.frames, (uint32_t)LACX_PCM_PLANAR_I32,
                               p.info.channels, p.info.bit_depth, false});
        tp_fill(plan.peak_at, tin.data(), m, h);
    }
    if (plan.spectrum) {  // likewise, and the window and twiddle tables
        std::vector<SpIn> xin;
        for (const PlanItem& p : plan.items)
            xin.push_back(SpIn{base.left + p.pcm_at, p.item.channels == 2 ? base.right + p.pcm_at : nullptr, p.item.frames, (uint32_t)LACX_PCM_PLANAR_I32,
                               p.info.channels, p.info.bit_depth, false});
        sp_fill(plan.spec_at, xin.data(), m, h);
    }
    if (plan.accuraterip) {  // the discs' sources: their items' places in the decoder's own PCM buffers
        std::vector<ArSrcIn> src = plan.ar_src;
        for (ArSrcIn& x : src) x.data0 = base.left + plan.items[x.item].pcm_at, x.data1 = base.right + plan.items[x.item].pcm_at;
        ar_fill(plan.ar_at, src.data(), plan.ar_discs.data(), plan.ar_discs.size(), h);
    }
    if (plan.compare) {  // the sources: the items' places in the decoder's own PCM buffers
        std::vector<CmpSrcIn> src = plan.cmp_src;
        for (CmpSrcIn& x : src) x.data0 = base.left + plan.items[x.item].pcm_at, x.data1 = x.channels == 2 ? base.right + plan.items[x.item].pcm_at : nullptr;
        cmp_fill(plan.cmp_at, src.data(), h);
    }
    if (!plan.lane_blk.empty()) std::memcpy(h + at.lane_blk, plan.lane_blk.data(), 4 * plan.lane_blk.size());
    if (!plan.v2_items.empty()) std::memcpy(h + at.v2_items, plan.v2_items.data(), 4 * plan.v2_items.size());
}

// The kernels' arguments: the tables at `tables` (where the kernels see them), the run's payload, status and flag arrays.
inline DecodeArgs plan_args(const DecodePlan& plan, const uint8_t* tables, const uint8_t* payload, uint32_t* status, uint8_t* ms_flag) {
    const TableLayout& at = plan.at;
    DecodeArgs a;
    a.nitems = (uint32_t)plan.items.size();
    a.total_blocks = (uint32_t)plan.total_blocks;
    a.items = reinterpret_cast<const DecodeItem*>(tables + at.items);
    a.blk_item = reinterpret_cast<const uint32_t*>(tables + at.blk_item);
    a.lanes = (uint32_t)plan.lane_blk.size();
    a.lane_blk = reinterpret_cast<const uint32_t*>(tables + at.lane_blk);
    a.nv2 = (uint32_t)plan.v2_items.size();
    a.v2_items = reinterpret_cast<const uint32_t*>(tables + at.v2_items);
    a.payload = payload;
    a.byte_off = reinterpret_cast<const unsigned long long*>(tables + at.byte_off);
    a.frame_off = reinterpret_cast<const unsigned long long*>(tables + at.frame_off);
    a.status = status;
    a.ms_flag = ms_flag;
    a.wav = plan.form == DecodeForm::wav;
    a.unit_off = reinterpret_cast<const unsigned long long*>(tables + at.unit_off);
    a.total_units = plan.total_units;
    if (plan.window()) a.window = reinterpret_cast<const WindowOut*>(tables + at.win);
    a.f32 = plan.sample_type == LACX_SAMPLE_F32;
    if (plan.form == DecodeForm::verify) {
        a.verify = reinterpret_cast<const VerifySource*>(tables + at.win);
        a.verify_res = reinterpret_cast<VerifyWords*>(const_cast<uint8_t*>(tables) + at.res);
    }
    if (plan.salvage) a.present = reinterpret_cast<const uint32_t*>(tables + at.win);
    if (plan.blocks) {
        a.block_raw = reinterpret_cast<uint32_t*>(const_cast<uint8_t*>(tables) + at.raw);
        a.judged = reinterpret_cast<const uint32_t*>(tables + at.judged);
        if (plan.judged) a.block_expect = reinterpret_cast<const uint32_t*>(tables + at.expect);
        a.no_output = plan.form == DecodeForm::blocks;
    }
    // (a loudness job has no digest: launch_decode then ends with k_ms_inverse in place, and the loudness kernels follow it;
    // a true-peak, a spectrum, a rip-checksum and a bit-compare job likewise)
    if (plan.form == DecodeForm::digest && !plan.loudness && !plan.truepeak && !plan.spectrum && !plan.accuraterip && !plan.compare) a.digest = reinterpret_cast<DigestWords*>(const_cast<uint8_t*>(tables) + at.res);
    if (plan.stats || plan.runs) a.no_output = true;  // launch_decode ends with k_ms_inverse; k_stats_blocks follows it (plan_stats_args)
    return a;
}

// A stats job's arguments for k_stats_blocks: the decode's own and the accumulator rows inside the tables.
inline StatsArgs plan_stats_args(const DecodePlan& plan, const DecodeArgs& a, const uint8_t* tables) {
    StatsArgs s;
    s.dec = a;
    s.rows = reinterpret_cast<StatsAcc*>(const_cast<uint8_t*>(tables) + plan.at.stats);
    return s;
}

// A runs job's arguments for k_runs: the decode's own, the tables of runs_plan.h inside the tables, and the list buffer.
inline RunsArgs plan_runs_args(const DecodePlan& plan, const DecodeArgs& a, const uint8_t* tables, lacx_run* list) {
    RunsArgs r;
    r.dec = a;
    runs_args(plan.runs_at, plan.items.size(), tables, list, r);
    return r;
}

// A loudness job's arguments for the four loudness kernels: the tables of loudness_plan.h inside the tables, and the scratch.
inline LoudArgs plan_loud_args(const DecodePlan& plan, const uint8_t* tables, uint8_t* scratch) {
    return loud_args(plan.loud_at, plan.items.size(), tables, scratch, nullptr);
}

// A true-peak job's arguments for k_truepeak: the tables of truepeak_plan.h inside the tables.
inline TpArgs plan_peak_args(const DecodePlan& plan, uint8_t* tables) { return tp_args(plan.peak_at, plan.items.size(), tables, nullptr); }

// A spectrum job's arguments for k_spectrum: the tables of spectrum_plan.h inside the tables.
inline SpArgs plan_spec_args(const DecodePlan& plan, uint8_t* tables) { return sp_args(plan.spec_at, plan.items.size(), tables, nullptr); }

// A rip-checksum job's arguments for k_accuraterip: the tables of accuraterip_plan.h inside the tables.
inline ArArgs plan_ar_args(const DecodePlan& plan, uint8_t* tables) { return ar_args(plan.ar_at, tables, nullptr); }

// A bit-compare job's arguments for k_compare_search / k_compare_rows: the tables of compare_plan.h inside the tables; y: the
// plan's layout, or the caller's copy of it with the chosen offsets.
inline CmpArgs plan_cmp_args(const CmpLayout& y, uint8_t* tables) { return cmp_args(y, tables, nullptr); }

}  // namespace lacx
