// encode_plan.h -- the host-only half of the device-emit encoder's host side: how a call is cut into pipeline chunks,
// what every chunk's kernels are told (frame range, source offset, stream indices, share of the fused emit, its words in
// the per-chunk arrays), which mode the call runs in, the descriptors and regions of a many-streams job, and every
// capacity the run must provide.  Plain C++, no HIP, no lacx_encoder: api_pipeline.cpp runs a plan on the device,
// tests/native/sim_encode_plan.cpp prints plans on the host.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <string>
#include <vector>

#include "container.h"
#include "lacx.h"
#include "lacx_types.h"

namespace lacx {

constexpr int kStreams = 4;
constexpr int kMaxChunks = 16;
constexpr uint32_t kMinChunkBlocks = 192;  // >= 1.5 rounds of 1024-thread workgroups over 256 CUs
constexpr uint32_t kRangeItems = 256;      // stream indices per progress range of the packer (kPackerRangeItems, kernels.h)
struct Chunk {
    uint32_t first, count;
};

// The environment knobs a plan depends on (Knobs, encoder_impl.h, holds the rest): read once, when the encoder is created.
struct PlanKnobs {
    bool fused_emit = true;        // LACX_FUSED_EMIT != 0
    bool direct_packer = false;    // LACX_DIRECT_PACKER: the packer stores into pinned host memory itself (round-2 layout)
    bool packer = true;            // LACX_NO_PACKER unset
    bool persistent = true;        // LACX_NO_PERSISTENT unset: whole-block analysis as persistent workgroups
    bool lazy_repair = true;       // LACX_NO_LAZY_REPAIR unset
    bool front_halves = true;      // LACX_NO_FRONT_HALVES unset: a one-chunk shard's front kernels in two block halves on two streams
    uint64_t pinned_cap_bytes = 0; // LACX_PINNED_CAP_BYTES (tests force the regrow path with it)
    uint32_t pipe_chunks = 0;      // LACX_PIPE_CHUNKS
    std::string pipe_split;        // LACX_PIPE_SPLIT
};

inline bool rate_ok(uint32_t sr) { return sr == 44100 || sr == 48000 || sr == 96000 || sr == 192000; }
inline uint32_t blocks_for(uint64_t frames) { return (uint32_t)((frames + kMaxBlock - 1) / kMaxBlock); }

// What the encoder's settings contribute to every stream's parameters.
struct ParamBase {
    int zero_run = 1, partitioning = 1;
    uint32_t debug_skip = 0;  // test hooks / ablations (only a -DLACX_TEST_HOOKS library looks at it)
};
inline AnalyzeParams make_params(const ParamBase& pb, uint64_t frames, int channels, int stereo_mode, int bit_depth, int layout = 0) {
    AnalyzeParams prm{};
    prm.layout = layout;
    prm.frames = frames;
    prm.num_blocks = blocks_for(frames);
    prm.first_block = 0;
    prm.channels = channels;
    prm.stereo_mode = channels == 2 ? stereo_mode : 0;
    prm.bit_depth = bit_depth;
    prm.zero_run = pb.zero_run;
    prm.partitioning = pb.partitioning;
    prm.debug_skip = pb.debug_skip;
    return prm;
}

// Size of the pinned result reservation of one stream: 1.25 x the PCM at its source bit depth covers every realistic
// stream (the exact size is only known after the analysis; a stream that needs more is re-emitted into a regrown buffer
// resp. the batch runs once more with exact regions).  LACX_PINNED_CAP_BYTES overrides the estimate.
inline uint64_t pinned_reservation(uint64_t frames, int channels, int bit_depth, uint32_t nb, uint64_t pinned_cap_bytes) {
    if (pinned_cap_bytes > 0) return pinned_cap_bytes;
    return frames * (uint64_t)channels * ((unsigned)bit_depth / 8u) * 5u / 4u + (uint64_t)nb * 64u + 4096u;
}
// room in front of the payload for the container header + block table, so that a whole .lac is handed out without a copy
inline uint64_t prefix_bytes(uint32_t nb) { return (stream_head_bytes(nb) + 4095ull) & ~4095ull; }
// Stream indices that take part in the fused emit: all but those of a final block of <= 4096 frames in per-block stereo
// mode, which may be encoded both ways and compared afterwards (ref lac/encoder.cpp:336-340).
inline uint32_t fuse_items_of(uint64_t frames, uint32_t nb, int channels, int stereo_mode) {
    const uint64_t last_frames = frames - (uint64_t)(nb - 1) * kMaxBlock;
    const bool last_both_ways = channels == 2 && stereo_mode == 2 && last_frames <= (uint64_t)kFullCompareLimit;
    return (nb - (last_both_ways ? 1u : 0u)) * (uint32_t)channels;
}
inline uint32_t range_count(uint32_t items) { return (items + kRangeItems - 1u) / kRangeItems; }

// Host emit wants many chunks (emit of chunk i overlaps the analysis of chunk i+1); with the emit on the
// device the only host work is a copy, and two chunks (payload copy of one under the kernels of the other)
// measured best.
inline std::vector<Chunk> plan_chunks(const PlanKnobs& kn, uint32_t nb, bool device_emit = false, bool fused = false, bool upload = false) {
    uint32_t nchunks = nb / kMinChunkBlocks;
    // device emit without the fused path: 3 chunks up to an hour of stereo 48 kHz per call, 4 and 6 beyond (measured on a
    // 2 h shard).  With the fused emit + streaming packer nothing is left to overlap by chunking -- the payload leaves
    // while the analysis runs, and ingest / probes keep every CU busy by themselves -- and one launch set measured best
    // from 10 min to 2 h of audio (a chunked run only adds kernel boundaries).
    // With the input still in host memory the chunks pipeline the upload (the uploader thread copies chunk c + 1 while
    // chunk c's kernels are enqueued and run): four equal chunks measured best once the copies came from their own thread
    // and the packer's stream had a priority level of its own (10 min stream, WAV image -> .lac: 3.40 ms; 1:2:3 3.57,
    // 1:3:4 3.6, one chunk 4.65; round 3, copies issued by the calling thread: 1:3:4 3.75).
    const uint32_t dev_chunks = fused ? (upload ? 4u : 1u) : (nb >= 12000u ? 6u : (nb >= 6000u ? 4u : 3u));
    nchunks = std::max(1u, std::min(nchunks, device_emit ? dev_chunks : 8u));
    bool forced = false;
    if (kn.pipe_chunks >= 1 && kn.pipe_chunks <= (uint32_t)kMaxChunks) {  // tuning knob
        nchunks = std::min<uint32_t>(kn.pipe_chunks, nb);
        forced = true;
    }
    std::vector<Chunk> out;
    const char* split_env = kn.pipe_split.empty() ? nullptr : kn.pipe_split.c_str();  // tuning knob: relative chunk sizes, e.g. "5,3,1"
    // Device emit: three chunks on three streams of falling priority, the last one a little smaller -- its
    // emit is the only one whose PCIe writes are not hidden under another chunk's analysis (measured best).
    if (!split_env && !forced && device_emit && nchunks == 3u) split_env = (fused && upload) ? "1,2,3" : "5,5,4";
    if (const char* env = split_env) {
        std::vector<double> w;
        double sum = 0;
        for (const char* p = env; *p && w.size() < (size_t)kMaxChunks;) {
            char* end = nullptr;
            const double v = std::strtod(p, &end);
            if (end == p) break;
            if (v > 0) {
                w.push_back(v);
                sum += v;
            }
            p = (*end == ',') ? end + 1 : end;
        }
        if (!w.empty() && nb >= w.size()) {
            uint32_t f = 0;
            double acc = 0;
            for (size_t i = 0; i < w.size(); ++i) {
                acc += w[i];
                uint32_t end = i + 1 == w.size() ? nb : (uint32_t)(nb * (acc / sum));
                end = std::max(end, f + 1);
                end = std::min(end, nb - (uint32_t)(w.size() - 1 - i));
                out.push_back({f, end - f});
                f = end;
            }
            return out;
        }
    }
    const uint32_t per = (nb + nchunks - 1) / nchunks;
    for (uint32_t f = 0; f < nb; f += per) out.push_back({f, std::min(per, nb - f)});
    return out;
}

// Every capacity a run must provide (0: not needed); the encoder's buffers only ever grow.
struct Capacities {
    uint64_t dev_payload = 0;     // bytes of device payload
    uint64_t pinned_payload = 0;  // bytes of pinned payload behind ...
    uint64_t prefix = 0;          // ... this many bytes of prefix
    bool pinned_fresh = false;    // LACX_PINNED_CAP_BYTES: the pinned payload is reallocated on every call
    uint32_t ranges = 0;          // 64-bit words of pinned range flags
    uint32_t table_blocks = 0;    // blocks of the pinned block table
    uint32_t emitted = 0;         // 32-bit words of the pinned copy of the packed flags
    uint32_t sizes = 0;           // 64-bit words of the pinned copy of the size records
    uint64_t batch_table = 0;     // bytes of the device table of a many-streams job
};

// ---- one shard (encode_device_begin / _end) ---------------------------------------------------------------------------
struct ShardIn {
    uint64_t frames = 0;
    int channels = 1, bit_depth = 16, stereo_mode = 0;
    int layout = 0;         // PCM_PLANAR_I32 / PCM_INTERLEAVED_I16 / PCM_INTERLEAVED_I24
    bool host_src = false;  // the PCM is still in host memory: the chunks pipeline its upload
};
// Pipeline chunk c: blocks [first, first + count), frames [f0, f1).
struct ChunkPlan {
    uint32_t first = 0, count = 0;
    uint64_t f0 = 0, f1 = 0;
    uint64_t src_off = 0;      // bytes from the start of the source to frame f0 (of each array in the planar layout)
    uint32_t stream_base = 0;  // stream index (block * channels + channel) of its first channel block
    uint32_t fuse_items = 0;   // its stream indices [stream_base, stream_base + fuse_items) take part in the fused emit
    int stream = 0;            // which of the call's kStreams streams carries it
    // its words in the arrays with per-chunk entries: block_off (count + 1 entries per chunk), err_flag, the two rows of
    // tspan ([2][kMaxChunks]), work_ctr (8 words per chunk)
    uint32_t block_off_at = 0, err_at = 0, t_first_at = 0, t_last_at = 0, work_ctr_at = 0;
};
struct ShardPlan {
    ShardIn in;
    uint32_t nb = 0;
    uint64_t frame_bytes = 4;  // bytes per frame in the source (per array in the planar layout)
    bool fused = false;        // emit fused into the analysis kernel (else k_offsets + k_emit alone)
    bool packer = false;       // the streaming packer runs (and counts what it moved)
    bool drained = false;      // the packer packs into device memory and a copy engine drains it into the pinned buffer
    bool direct = false;       // packer / k_emit store into the pinned buffer themselves
    bool lazy = false;         // k_offsets / k_pack / k_emit only on demand; the block table comes from the size records
    bool persistent = false;   // persistent analysis workgroups: only for a shard that is one chunk
    bool front_halves = false; // eligible for the two-halves front launch: one chunk (and not on the auxiliary stream itself)
    uint32_t fuse_items = 0;   // of the whole shard
    uint32_t ranges = 0;       // progress ranges the packer reports (drained only)
    std::vector<ChunkPlan> chunks;
    Capacities cap;
};

inline ShardPlan plan_shard(const ShardIn& in, const PlanKnobs& kn) {
    ShardPlan p;
    p.in = in;
    const uint32_t nb = p.nb = blocks_for(in.frames), ch = (uint32_t)in.channels;
    p.frame_bytes = in.layout == 1 ? 2ull * ch : (in.layout == 2 ? 3ull * ch : 4ull);
    // Emit fused into the analysis kernel (default; LACX_FUSED_EMIT=0 leaves the bitstream to k_offsets + k_emit alone;
    // k_emit runs after the analysis in any case and picks up whatever the fused path did not write).
    p.fused = kn.fused_emit;
    const std::vector<Chunk> chunks = plan_chunks(kn, nb, true, p.fused, in.host_src);
    const bool one = chunks.size() == 1;
    p.fuse_items = p.fused ? fuse_items_of(in.frames, nb, in.channels, in.stereo_mode) : 0u;
    p.packer = p.fuse_items && kn.packer;
    // Default with the fused emit: the packer packs into device memory and a copy engine drains it (LACX_DIRECT_PACKER=1:
    // the packer's CUs store straight into pinned host memory, the round-2 layout).
    p.drained = p.fused && !kn.direct_packer && kn.packer && kn.pinned_cap_bytes == 0;
    p.direct = !p.drained;
    // Lazy repair: a one-chunk shard whose channel blocks all take part in the fused emit normally leaves k_pack and
    // k_emit nothing to do; they are not even enqueued, the gather kernel checks the packer's count and the host
    // enqueues them afterwards in the rare case (a packer wave that gave up, a bitstream longer than its slot).
    p.lazy = kn.lazy_repair && p.packer && one && p.fuse_items == nb * ch;
    // persistent analysis workgroups only for a shard that is one chunk: with several, the next chunk's ingest /
    // Levinson / probe kernels are meant to run beside this chunk's analysis, which persistent workgroups would not let in
    p.persistent = one && kn.persistent;
    p.front_halves = one && kn.front_halves;
    p.ranges = p.drained && p.packer ? range_count(p.fuse_items) : 0u;
    for (size_t c = 0; c < chunks.size(); ++c) {
        ChunkPlan k;
        k.first = chunks[c].first;
        k.count = chunks[c].count;
        k.f0 = (uint64_t)k.first * kMaxBlock;
        k.f1 = std::min<uint64_t>(in.frames, (uint64_t)(k.first + k.count) * kMaxBlock);
        k.src_off = k.f0 * p.frame_bytes;
        k.stream_base = k.first * ch;
        k.fuse_items = p.fuse_items > k.stream_base ? std::min(k.count * ch, p.fuse_items - k.stream_base) : 0u;
        k.stream = (int)(c % kStreams);
        k.block_off_at = k.first + (uint32_t)c;
        k.err_at = (uint32_t)c;
        k.t_first_at = (uint32_t)c;
        k.t_last_at = (uint32_t)(kMaxChunks + c);
        k.work_ctr_at = 8u * (uint32_t)c;
        p.chunks.push_back(k);
    }
    const uint64_t reservation = pinned_reservation(in.frames, in.channels, in.bit_depth, nb, kn.pinned_cap_bytes);
    p.cap.dev_payload = p.drained ? reservation + 64ull : 0ull;
    p.cap.ranges = p.drained ? range_count(nb * ch) + 1u : 0u;
    p.cap.pinned_payload = reservation;
    p.cap.prefix = prefix_bytes(nb);
    p.cap.pinned_fresh = kn.pinned_cap_bytes != 0;
    p.cap.table_blocks = nb;
    p.cap.emitted = p.fused ? nb * 2u : 0u;
    p.cap.sizes = p.lazy ? nb * ch : 0u;
    return p;
}

// Lazy path (k_offsets never ran): the block table and the payload's size from the size records the analysis kernel
// published, one per channel block (bit 62: valid, bits 0..59: bytes).  complete: every record had its valid bit.
struct SizeTable {
    unsigned long long total = 0;
    bool complete = true;
};
inline SizeTable table_from_size_records(const unsigned long long* recs, const BlockPlan* bplans, uint32_t nb, int channels,
                                         uint32_t* table) {
    SizeTable t;
    for (uint32_t b = 0; b < nb; ++b) {
        unsigned long long bytes = 0;
        for (int ch = 0; ch < channels; ++ch) {
            const unsigned long long rec = recs[(size_t)b * channels + ch];
            t.complete = t.complete && (rec >> 62) == 1ull;  // (kRecValid)
            bytes += rec & ((1ull << 60) - 1ull);
        }
        table[2 * (size_t)b] = bplans[b].frames;
        table[2 * (size_t)b + 1] = (uint32_t)bytes;
        t.total += bytes;
    }
    return t;
}

// ---- many streams as one job (encode_batch) --------------------------------------------------------------------------
inline bool is_import_layout(uint32_t layout) {
    return layout == LACX_PCM_PLANAR_I16 || layout == LACX_PCM_PLANAR_F32 || layout == LACX_PCM_INTERLEAVED_F32;
}
// the layout the import pass rewrites a source of that depth into (api_import.cpp)
inline int import_target_layout(int bit_depth) { return bit_depth == 16 ? (int)LACX_PCM_INTERLEAVED_I16 : (int)LACX_PCM_INTERLEAVED_I24; }

struct BatchPlan {
    std::vector<StreamDesc> streams;    // every field but left / right
    std::vector<uint8_t> imported;      // 1: the stream is in a tensor layout and goes through the import pass first
    std::vector<uint16_t> item_stream;  // the stream of every stream index
    uint32_t nb = 0, nitems = 0;
    int max_depth = 16;  // the staging slots have one stride for the whole set: the deepest material's
    size_t tab_bytes = 0, map_bytes = 0;  // device table: the descriptors (16-byte padded), then item_stream
    Capacities cap;  // (pinned_payload: the 4096-aligned regions of all streams)
};
// Validates the items in order (the first complaint wins, in the reference's wording) and lays the job out.  import_error:
// the check of a source in a tensor layout (import_source_error, api_import.cpp): its message, or null.  exact_caps: the
// second attempt's exact reservations (null: the estimate).  Returns LACX_OK, or LACX_E_INVALID with the message in *why.
inline int plan_batch(const lacx_batch_item* items, uint32_t n, const ParamBase& pb, const PlanKnobs& kn, const uint64_t* exact_caps,
                      const char* (*import_error)(const lacx_pcm&, int), BatchPlan* out, std::string* why) {
    auto fail = [&](const std::string& msg) { return *why = msg, LACX_E_INVALID; };
    BatchPlan& p = *out;
    p = BatchPlan{};
    p.streams.assign(n, StreamDesc{});
    p.imported.assign(n, 0);
    uint64_t region = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const lacx_batch_item& it = items[i];
        const std::string who = "stream " + std::to_string(i) + ": ";
        if (it.pcm.data0 == nullptr || it.frames == 0) return fail(who + "left channel must not be empty");
        if (!rate_ok(it.sample_rate)) return fail(who + "unsupported sample rate: " + std::to_string(it.sample_rate));
        if (!(it.bit_depth == 16 || it.bit_depth == 24)) return fail(who + "unsupported bit depth: " + std::to_string((int)it.bit_depth));
        if (it.stereo_mode > 2) return fail(who + "unsupported stereo mode: " + std::to_string((int)it.stereo_mode));
        if (it.pcm.channels != 1 && it.pcm.channels != 2) return fail(who + "unsupported channel count");
        int layout = 0;
        if (it.pcm.layout == LACX_PCM_PLANAR_I32) {
            if ((it.pcm.channels == 2) != (it.pcm.data1 != nullptr))
                return fail(who + "planar PCM: data1 must be the right channel of stereo input and null for mono");
        } else if (it.pcm.layout == LACX_PCM_INTERLEAVED_I16 || it.pcm.layout == LACX_PCM_INTERLEAVED_I24) {
            if ((it.pcm.layout == LACX_PCM_INTERLEAVED_I16 ? 16 : 24) != it.bit_depth) return fail(who + "PCM layout does not match the bit depth");
            layout = (int)it.pcm.layout;
        } else if (is_import_layout(it.pcm.layout)) {
            if (const char* bad = import_error(it.pcm, it.bit_depth)) return fail(who + bad);
            p.imported[i] = 1;
            layout = import_target_layout(it.bit_depth);
        } else {
            return fail(who + "unknown PCM layout");
        }
        const int channels = (int)it.pcm.channels;
        StreamDesc& sd = p.streams[i];
        sd.prm = make_params(pb, it.frames, channels, it.stereo_mode, it.bit_depth, layout);
        sd.prm.stream_base = p.nitems;
        sd.first_block = p.nb;
        sd.first_wg = p.nitems;
        sd.pad = i;  // the stream's number in the table (k_offsets)
        const uint32_t snb = sd.prm.num_blocks;
        sd.fuse_items = fuse_items_of(it.frames, snb, channels, it.stereo_mode);
        sd.out_base = region;
        // (LACX_PINNED_CAP_BYTES: tests force the second attempt with it)
        sd.out_cap = exact_caps ? exact_caps[i] : pinned_reservation(it.frames, channels, it.bit_depth, snb, kn.pinned_cap_bytes);
        region += (sd.out_cap + 4095u) & ~4095ull;
        if ((uint64_t)p.nb + snb > 0x7FFFFFFFull / kSlotsPerBlock) return fail("too many blocks in one batch");
        p.nb += snb;
        p.nitems += snb * (uint32_t)channels;
        p.max_depth = std::max(p.max_depth, (int)it.bit_depth);
    }
    if (n > 65535u) return fail("more than 65535 streams in one batch");
    p.item_stream.resize(p.nitems);
    for (uint32_t i = 0; i < n; ++i) {
        const AnalyzeParams& prm = p.streams[i].prm;
        std::fill_n(p.item_stream.begin() + prm.stream_base, prm.num_blocks * (uint32_t)prm.channels, (uint16_t)i);
    }
    p.tab_bytes = ((size_t)n * sizeof(StreamDesc) + 15) & ~(size_t)15;
    p.map_bytes = (size_t)p.nitems * sizeof(uint16_t);
    p.cap.pinned_payload = region;
    p.cap.table_blocks = p.nb;
    p.cap.emitted = p.nb * 2u;
    p.cap.batch_table = p.tab_bytes + p.map_bytes;
    return LACX_OK;
}
// Bytes of a stream of a batch, from the job's block table; *empty (nullable): one of its blocks has no bytes.
inline uint64_t batch_stream_bytes(const uint32_t* table, const StreamDesc& sd, bool* empty = nullptr) {
    uint64_t bytes = 0;
    for (uint32_t b = 0; b < sd.prm.num_blocks; ++b) {
        const uint32_t by = table[2 * ((size_t)sd.first_block + b) + 1];
        if (by == 0 && empty) *empty = true;
        bytes += by;
    }
    return bytes;
}

}  // namespace lacx
