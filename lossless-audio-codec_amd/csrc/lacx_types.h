// lacx_types.h -- records exchanged between the HIP kernels and the host side of the encoder.
#pragma once
#include <stddef.h>
#include <stdint.h>

struct lacx_block_info;  // lacx.h
struct lacx_run_detector;
struct lacx_run;
struct lacx_loudness_row;
struct lacx_truepeak_row;
struct lacx_spectrum_row;

namespace lacx {

constexpr int kMaxBlock = 16384;  // Block::MAX_BLOCK_SIZE        (ref src/codec/block/constants.hpp:6)
constexpr int kMaxParts = 256;    // 1 << MAX_PARTITION_ORDER     (ref constants.hpp:11)
constexpr int kMinPartition = 32; // MIN_PARTITION_SIZE           (ref constants.hpp:10)
constexpr int kMaxPartitionOrder = 8;
// zero bytes behind the decoder's payload buffer: the bit reader's bounded look-ahead past the last block (decode_core.h)
constexpr size_t kDecodeTailPad = 128;
constexpr int kProbe = 256;             // kStereoProbeSize             (ref src/codec/lac/encoder.cpp:19)
constexpr int kFullCompareLimit = 4096; // kStereoFullComparisonLimit   (ref lac/encoder.cpp:20)

// Channel kinds inside a stereo block.
enum : int { CH_L = 0, CH_R = 1, CH_M = 2, CH_S = 3 };

// A "slot" is one channel-segment that gets the full Block::Encoder analysis:
//   slot = window * 4 + channel,  window 0 = whole block, windows 1..3 = the three 256-frame probes
//   (ref lac/encoder.cpp:343-346).  Mono streams use slot 0 only.
constexpr int kSlotsPerBlock = 16;

// Quantised LPC candidates for one slot: orders {4,6,8,10,12} (ref block/encoder.cpp:41).
struct LpcSet {
    int16_t coef[5][13];  // coef[ci][1..used] valid, rest 0
    uint8_t used[5];      // 0 = candidate skipped
    uint8_t pad;
};

// Everything Block::Encoder::encode decides before it starts emitting bits
// (ref block/encoder.cpp:313-552), for one slot.
struct ChannelPlan {
    uint8_t predictor_type;   // 0 fixed, 1 FIR, 2 LPC
    uint8_t order;            // chosen_order
    uint8_t partition_order;  // 0..8
    uint8_t valid;            // 1 when the slot was analysed
    int16_t coef[12];         // coef[i-1] = Q15 coefficient i (LPC only)
    uint32_t payload_bytes;   // exact size of the emitted channel block
    uint64_t total_bits;      // best_total_bits (metadata + residual bits, padded to a byte)
    uint8_t part_mode_k[kMaxParts];  // (mode << 5) | k per partition
};

// Per-block stereo decision (ref lac/encoder.cpp:126-197, 321-373).
struct BlockPlan {
    uint8_t choose_ms;   // final LR(0)/MS(1) choice
    uint8_t uncertain;   // estimate_stereo_mode's flag
    uint8_t est_ms;      // estimate_stereo_mode's choose_ms
    uint8_t invalid;     // 1 if a sample was outside the bit depth (ref lac/encoder.cpp:82-102)
    uint32_t frames;     // frames in this block
    uint32_t first_bad;  // index (within block) of the first invalid sample, channel in bit 31
    uint32_t pad;
};

struct AnalyzeParams {
    uint64_t frames;       // total frames in the stream segment handed to the kernels
    uint32_t num_blocks;
    uint32_t first_block;  // blocks [first_block, first_block+num_blocks) are processed
    int32_t channels;      // 1 or 2
    int32_t stereo_mode;   // 0 LR, 1 MS, 2 per-block auto
    int32_t bit_depth;     // 16 / 24 (range validation); 0 = no validation (Block::Encoder path)
    int32_t zero_run;
    int32_t partitioning;
    uint32_t debug_skip;   // diagnostic ablation mask (timing experiments only; 0 in production)
    int32_t layout;        // PCM_PLANAR_I32 / PCM_INTERLEAVED_I16 / PCM_INTERLEAVED_I24 (analyze_core.h)
    uint32_t stream_base;  // fused emit: stream index (block * channels + channel) of the chunk's first channel block
};

// One input stream of a launch set.  A launch set covers the blocks of one or many streams (lacx_encode_batch: the files
// of a corpus as ONE job, ref src/codec/lac/encoder.cpp:404-435 keeps one pool over all blocks): global block g of the
// set belongs to the stream with first_block <= g < first_block + prm.num_blocks and is block g - first_block of it.
// Workspace arrays (plans, need masks, autocorrelations ...) are indexed by the global block, sample addresses and block
// geometry by the stream's own block number.
struct StreamDesc {
    AnalyzeParams prm;              // the stream's parameters; prm.stream_base = its first stream index (block * channels + channel, over the set)
    const int32_t* left;            // planar: left channel; interleaved layouts: the WAV data chunk
    const int32_t* right;           // planar: right channel (null for mono)
    uint32_t first_block;           // first global block
    uint32_t first_wg;              // first workgroup in the grid of the whole-block analysis kernel (channels per block)
    uint32_t fuse_items;            // stream indices [prm.stream_base, prm.stream_base + fuse_items) take part in the fused emit
    uint32_t pad;                   // the stream's number in a table of several
    unsigned long long out_base;    // byte offset of the stream's payload region in the result buffer
    unsigned long long out_cap;     // bytes reserved for it
};

// What every kernel gets: a table of streams in device memory, or -- one stream, the common case -- the descriptor
// itself in the kernel arguments (table == nullptr; no upload, no look-up).
struct BatchRef {
    const StreamDesc* table;
    uint32_t nstreams;
    uint32_t total_blocks;
    StreamDesc single;
};

// Verify form of the decoder (verify_core.h, k_verify): the source PCM an item's decoded samples are compared with, in its
// own layout, and the words the comparison leaves per item.
struct VerifySource {
    const void* data0;  // planar: left; interleaved layouts: the WAV data chunk
    const void* data1;  // planar: right (null for mono)
    uint32_t layout;    // PCM_PLANAR_I32 / PCM_INTERLEAVED_I16 / PCM_INTERLEAVED_I24 (analyze_core.h), or a tensor layout:
                        // PCM_PLANAR_I16 / PCM_PLANAR_F32 / PCM_INTERLEAVED_F32 (import_core.h)
    uint32_t pad;
};
struct VerifyWords {
    unsigned long long count;  // samples that differ (zeroed per call)
    unsigned long long key;    // lowest frame * 2 + channel that differs (all ones per call: none)
    int32_t decoded, source;   // the two values at `key` (filled by verify_fill_item when count != 0)
    uint32_t block;            // the block of that frame, counted in the item
    uint32_t pad;
};

// Digest form of the decoder (digest_core.h, k_digest.hip): what the kernel leaves per item, and -- the source form, a job
// without a decode -- the device-resident PCM that is digested in its own layout.
struct DigestWords {
    uint32_t raw;  // XOR of every unit's raw CRC-32 value shifted to the item's end (zeroed per call)
    uint32_t pad;
};
struct DigestSource {
    const void* data0;          // as VerifySource
    const void* data1;
    unsigned long long frames;  // >= 1
    uint32_t layout;
    uint8_t channels, bit_depth, pad[2];
};
constexpr unsigned long long kDigestClean = ~0ull;  // DigestPcmArgs::bad: no invalid sample (digest_bad_key, digest_core.h)
struct DigestPcmArgs {
    uint32_t nitems = 0;
    unsigned long long total_units = 0;
    const unsigned long long* unit_off = nullptr;  // [nitems + 1] prefix sums of ceil(frames / 4)
    const DigestSource* src = nullptr;
    DigestWords* res = nullptr;                    // [nitems], zero on entry
    unsigned long long* bad = nullptr;             // [nitems] lowest digest_bad_key per item, all ones on entry
};

// The decoder's job records (decode.hip; filled by the host-only plan, decode_plan.h).  One job decodes a batch of streams
// (items), its blocks numbered globally: see launch_decode (kernels.h).
struct DecodeItem {
    int32_t* left;                // the item's PCM from its frame 0 (16-byte aligned in the WAV form)
    int32_t* right;               // null for mono
    uint8_t* wav;                 // WAV form: the item's image (16-byte aligned; header is the host's), else null
    unsigned long long frame0;    // frame_off of the item's first block
    unsigned long long frames;
    unsigned long long pay_off;   // byte offset of the item's payload (where a version-2 item's lane starts)
    uint32_t block0, blocks;      // the item's global blocks
    uint32_t pay_bits;            // version 2 only: payload bits
    uint8_t channels, stereo_mode, bit_depth, version;
};
// Window form: an item's decoded frames are those of the blocks that overlap its window, from the first of them on.
struct WindowOut {
    void* left;                   // the window's samples from its frame 0 on: int32 or float32, 4-byte aligned
    void* right;                  // null for mono
    unsigned long long start;     // the window's first frame, counted in the item's decoded frames
    unsigned long long frames;    // >= 1
};
struct DecodeArgs {
    uint32_t nitems = 0, total_blocks = 0;
    const DecodeItem* items = nullptr;        // (window form: an item covers only the blocks its window needs)
    const uint32_t* blk_item = nullptr;       // [total_blocks] the item of every block
    // k_decode: lane g decodes block lane_blk[g] (~0u: idle); only version-3 blocks, an item's in consecutive lanes
    uint32_t lanes = 0;
    const uint32_t* lane_blk = nullptr;
    uint32_t nv2 = 0;                         // version-2 items, one lane each (k_decode_serial)
    const uint32_t* v2_items = nullptr;
    const uint8_t* payload = nullptr;         // followed by kDecodeTailPad zero bytes
    const unsigned long long* byte_off = nullptr;
    const unsigned long long* frame_off = nullptr;
    uint32_t* status = nullptr;
    uint8_t* ms_flag = nullptr;
    // wav = false: k_ms_inverse in place into every item's left / right; true: k_wav_pack into the items'
    // images (unit_off: [nitems + 1] prefix sums of ceil(frames / 4)), left / right then hold the pre-inverse samples
    bool wav = false;
    const unsigned long long* unit_off = nullptr;
    unsigned long long total_units = 0;
    // window form (non-null: k_window_out over the units of unit_off in place of k_ms_inverse / k_wav_pack): window[j]
    // says which of item j's decoded frames go where; f32: float32 samples scaled by 2^-(bit_depth - 1), else int32
    const WindowOut* window = nullptr;
    bool f32 = false;
    // verify form (non-null: k_verify over the units of unit_off in place of the other post passes, then k_verify_fill):
    // verify[j] is the source PCM of item j, verify_res[j] its result words (count 0 and key all ones on entry)
    const VerifySource* verify = nullptr;
    VerifyWords* verify_res = nullptr;
    // digest form (non-null: k_digest over the units of unit_off in place of the other post passes): digest[j] is item
    // j's result word (zero on entry)
    DigestWords* digest = nullptr;
    // salvage job (non-null: k_ms_inverse in place, then k_salvage_wav (wav) or k_salvage_blank over the final status
    // words, in place of the other post passes): present[j] = the blocks of item j that had a lane; the status words
    // of the others were written by nobody
    const uint32_t* present = nullptr;
    // block digests (non-null, salvage jobs only: k_digest_blocks behind k_ms_inverse, blockdigest_core.h): block_raw[g] is
    // global block g's raw word (zero on entry).  block_expect (non-null: k_digest_judge behind it, in front of the
    // salvage pass): the expected CRC-32 per global block, looked at for the blocks of the items with judged[j] != 0.
    // no_output: the blocks form -- the items lie in the decoder's own buffers and no salvage pass follows
    uint32_t* block_raw = nullptr;
    const uint32_t* block_expect = nullptr;
    const uint32_t* judged = nullptr;
    bool no_output = false;
};
// Block digests of device-resident source PCM (k_digest_blocks<true>): the digest form's sources on a regular grid.
struct BlockPcmArgs {
    DigestPcmArgs pcm;                             // (res is not used)
    uint32_t grid = 0;                             // frames per block, 256 .. 16384
    const unsigned long long* block_off = nullptr; // [nitems + 1] prefix sums of ceil(frames / grid)
    uint32_t* raw = nullptr;                       // [block_off[nitems]], zero on entry
};
// Audio statistics (k_stats_blocks, stats_core.h): one accumulator row per global block, all-zero bytes on entry.
struct StatsAcc;
// ... of a stats job's items behind k_ms_inverse: the blocks form of a salvage job without block digests
struct StatsArgs {
    DecodeArgs dec;
    StatsAcc* rows = nullptr;                      // [dec.total_blocks]
};
// ... of device-resident source PCM on a regular grid
struct StatsPcmArgs {
    DigestPcmArgs pcm;                             // (res is not used)
    uint32_t grid = 0;                             // frames per block, 256 .. 16384
    const unsigned long long* block_off = nullptr; // [nitems + 1] prefix sums of ceil(frames / grid)
    StatsAcc* rows = nullptr;                      // [block_off[nitems]]
};
// Run finder (k_runs, runs_core.h): the tables runs_plan.h lays out -- per item its detectors and rows, per detector its
// list region and counter (zero on entry), one row per (tile, detector) (zero on entry) -- and the list buffer.
struct RunsItem;
struct RunsList;
struct RunsRow;
struct RunsArgs {
    DecodeArgs dec;                                // stream form: the job k_runs follows (behind k_ms_inverse)
    uint32_t nitems = 0;
    unsigned long long total_tiles = 0;
    const unsigned long long* tile_off = nullptr;  // [nitems + 1] prefix sums of ceil(frames / kRunsTileFrames)
    const RunsItem* items = nullptr;               // [nitems]
    const lacx_run_detector* dets = nullptr;       // the items' detectors, an item's in a row
    RunsList* lists = nullptr;                     // one per detector
    RunsRow* rows = nullptr;
    lacx_run* runs = nullptr;                      // the list buffer
    const DigestSource* src = nullptr;             // source form: the items, and per item the lowest invalid sample's key
    unsigned long long* bad = nullptr;
};
// Stream inspection (k_inspect / k_inspect_serial, inspect_core.h): the decode's tables without its outputs (status and
// ms_flag are not used), one row per global block, and for a job with partition detail the entries of both channel blocks.
constexpr uint32_t kInspectPartSlots = 256;        // partition entries per channel block: 1 << kMaxPartitionOrder
static_assert(kInspectPartSlots == (uint32_t)kMaxParts, "a channel block has at most kMaxParts partitions");
struct InspectArgs {
    DecodeArgs dec;
    lacx_block_info* rows = nullptr;               // [dec.total_blocks]
    uint8_t* mode_k = nullptr;                     // [dec.total_blocks][2][256], zero on entry, or null
    uint32_t* part_bits = nullptr;                 // [dec.total_blocks][2][256], zero on entry, or null
};
// Loudness (k_loud_* of k_loudness.hip, loudness_core.h): the tables loudness_plan.h lays out and the job's scratch.
// One form for both jobs: an item is PCM in a layout -- a stream's is the decoder's planar int32 staging as k_ms_inverse
// left it (validate 0: its blocks' statuses say whether it counts), a source's its own (validate 1: an invalid sample
// lowers bad[j]).
constexpr uint32_t kLoudChunk = 256;               // frames per chunk, counted in the item's frames from 0
struct LoudFilter {                                // the K-weighting of one sample rate (loudness_plan.h makes it)
    double sb[3], sna[2];                          // shelf: b0 b1 b2, -a1 -a2
    double hb[3], hna[2];                          // high-pass
    double A[4][4];                                // kLoudChunk zero-input steps as a map of the four state words
};
struct LoudState {                                 // 32 bytes: shelf s1 s2, high-pass s1 s2
    double s[4];
};
struct LoudPartial {                               // 16 bytes: the chunk's sums in its first and its second sub-block
    double p[2];
};
struct LoudItem {
    const void* data0;                             // as DigestSource
    const void* data1;
    unsigned long long frames;                     // the item's frames: what may be loaded, and is validated
    unsigned long long used;                       // rows * sub: the frames that are filtered
    unsigned long long lane0;                      // the item's first record in the state and partial arrays
    unsigned long long row0;                       // the item's first row
    uint32_t chunks, rows;                         // ceil(frames / kLoudChunk), floor(frames / sub)
    uint32_t sub, layout;                          // frames per sub-block: sample_rate / 10
    uint8_t channels, bit_depth, rate, validate;   // rate: index into the filters
    uint32_t pad;
};
struct LoudArgs {
    uint32_t nitems = 0;
    unsigned long long total_chunks = 0, total_rows = 0;
    const LoudFilter* filters = nullptr;           // [4]: 44 100, 48 000, 96 000, 192 000
    const LoudItem* items = nullptr;               // [nitems]
    const unsigned long long* chunk_off = nullptr; // [nitems + 1] prefix sums of the items' chunks
    const unsigned long long* row_off = nullptr;   // [nitems + 1] prefix sums of the items' rows
    LoudState* states = nullptr;                   // [sum of chunks * channels], record lane0 + chunk * channels + channel
    LoudPartial* partials = nullptr;               // the same
    lacx_loudness_row* rows = nullptr;             // [total_rows]
    unsigned long long* bad = nullptr;             // [nitems] lowest digest_bad_key per item (all ones on entry), or null
};
// True peak (k_truepeak of k_truepeak.hip, truepeak_core.h): the tables truepeak_plan.h lays out.  One form for both jobs,
// as loudness has it: an item is PCM in a layout -- a stream's is the decoder's planar int32 staging as k_ms_inverse left
// it (validate 0), a source's its own (validate 1: an invalid sample lowers bad[j]).
constexpr uint32_t kTpTileFrames = 1024;           // outputs-frames n per workgroup, counted in the item's frames from 0
constexpr uint32_t kTpThreads = 256;               // ... four per lane
constexpr uint32_t kTpTaps = 12, kTpPhases = 4;
constexpr uint32_t kTpFlush = kTpTaps - 1;         // outputs-frames behind the item's last frame: n = frames .. frames + 10
constexpr uint32_t kTpHistory = 12;                // frames staged in front of a tile: three units, of which 11 frames are read
constexpr uint32_t kTpRowFrames = 16384;           // frames per row, counted from the item's frame 0
constexpr uint32_t kTpPosBits = 18;                // pos < 4 * (16384 + 11) < 2^18
struct TpAcc {                                     // 32 bytes: the device's row; all-zero bytes are the empty row
    unsigned long long key[2];                     // per channel max of peak << kTpPosBits | (2^kTpPosBits - 1 - pos)
    uint32_t sample_peak[2];                       // per channel max |x|
    uint32_t pad[2];
};
struct TpItem {
    const void* data0;                             // as DigestSource
    const void* data1;
    unsigned long long frames;
    unsigned long long row0;                       // the item's first row
    uint32_t tiles, rows;                          // ceil((frames + 11) / kTpTileFrames), ceil(frames / kTpRowFrames)
    uint32_t layout;
    uint8_t channels, bit_depth, validate, pad;
};
struct TpArgs {
    uint32_t nitems = 0;
    unsigned long long total_tiles = 0, total_rows = 0;
    const TpItem* items = nullptr;                 // [nitems]
    const unsigned long long* tile_off = nullptr;  // [nitems + 1] prefix sums of the items' tiles
    TpAcc* rows = nullptr;                         // [total_rows], zero on entry
    unsigned long long* bad = nullptr;             // [nitems] lowest digest_bad_key per item (all ones on entry), or null
};
// Spectrum (k_spectrum of k_spectrum.hip, spectrum_core.h): the tables spectrum_plan.h lays out.  One form for both jobs, as
// true peak has it.  A workgroup takes one row of one item: the windows whose first frame lies in the row's 16384 frames.
constexpr uint32_t kSpThreads = 256;
constexpr uint32_t kSpBands = 64;                  // uniform bands of N / 128 bins; the Nyquist bin belongs to the last
constexpr uint32_t kSpRowFrames = 16384;           // frames per row, counted from the item's frame 0
constexpr uint32_t kSpMinLog = 8, kSpMaxLog = 12;  // window lengths N = 256 .. 4096; the hop is N / 2
struct SpItem {
    const void* data0;                             // as DigestSource
    const void* data1;
    unsigned long long frames;
    unsigned long long row0;                       // the item's first row
    unsigned long long windows;                    // ceil(frames / (N / 2))
    uint32_t rows;                                 // ceil(frames / kSpRowFrames)
    uint32_t layout;
    uint8_t channels, bit_depth, validate, pad[5];
};
struct SpArgs {
    uint32_t nitems = 0;
    uint32_t logn = 0;                             // N = 1 << logn
    unsigned long long total_rows = 0;
    const SpItem* items = nullptr;                 // [nitems]
    const unsigned long long* row_off = nullptr;   // [nitems + 1] prefix sums of the items' rows
    const double* window = nullptr;                // [N] the periodic Hann window
    const double* twiddle = nullptr;               // [N / 2][2] cos, -sin of 2 pi k / N
    lacx_spectrum_row* rows = nullptr;             // [total_rows], zero on entry
    unsigned long long* bad = nullptr;             // [nitems] lowest digest_bad_key per item (all ones on entry), or null
};
// Rip checksums (k_accuraterip of k_accuraterip.hip, accuraterip_core.h): the tables accuraterip_plan.h lays out.  One form
// for both jobs: a disc is a run of sources, each PCM in a layout (a stream's is the decoder's planar int32 staging,
// validate 0; a source's its own, validate 1), and a list of spans over the disc's frames.
constexpr uint32_t kArThreads = 256;
constexpr uint32_t kArTileMults = 4096;            // multipliers per workgroup
constexpr uint32_t kArMaxRadius = 2939;            // 5 sectors of 588 frames less one frame
constexpr uint32_t kArSector = 588;
constexpr uint32_t kArStageWords = kArTileMults + kArThreads + 4u;  // a tile's words: M + offsets - 1, and up to 3 in front (units of four)
struct ArSource {                                  // 40 bytes
    const void* data0;                             // as DigestSource; always two channels of 16 bits
    const void* data1;
    unsigned long long start, frames;              // the source's first disc frame, its frames (> 0)
    uint32_t layout;
    uint32_t item;                                 // whose bad[] an invalid sample lowers
};
struct ArSpan {                                    // 48 bytes: sum over m = m_lo .. m_hi of m * x(frame1 + o + m - 1), every o in [-radius, radius]
    unsigned long long frame1;                     // the disc frame multiplier 1 reads at offset 0
    unsigned long long disc_frames;                // x is zero outside [0, disc_frames)
    uint32_t src0, nsrc;                           // the disc's sources, ascending by start, back to back from frame 0
    uint32_t m_lo, m_hi;                           // m_lo <= m_hi
    uint32_t sum0;                                 // sums[sum0 + radius + o]: the low halves; with keep_hi, sums[sum0 + 2 radius + 1 + radius + o]: low + high
    uint32_t radius;
    uint32_t lanes;                                // offsets per tile: a power of two <= kArThreads; kArThreads / lanes stripes share the multipliers
    uint8_t keep_hi, validate, pad[2];
};
// (constexpr: the host-only plan counts a span's tiles as the kernel does)
constexpr uint32_t ar_width(const ArSpan& s) { return 2u * s.radius + 1u; }
constexpr uint32_t ar_offset_tiles(const ArSpan& s) { return (ar_width(s) + s.lanes - 1u) / s.lanes; }
constexpr unsigned long long ar_span_tiles(const ArSpan& s) {
    return (unsigned long long)((s.m_hi - s.m_lo) / kArTileMults + 1u) * ar_offset_tiles(s);
}
struct ArArgs {
    uint32_t nspans = 0;
    unsigned long long total_tiles = 0;
    const ArSpan* spans = nullptr;                 // [nspans]
    const unsigned long long* tile_off = nullptr;  // [nspans + 1] prefix sums of the spans' tiles (multiplier tile major, offset tile minor)
    const ArSource* sources = nullptr;
    uint32_t* sums = nullptr;                      // zero on entry
    unsigned long long* bad = nullptr;             // [items] lowest digest_bad_key per item (all ones on entry), or null
};
// Bit-compare (k_compare_search / k_compare_rows of k_compare.hip, compare_core.h): the tables compare_plan.h lays out.  One
// form for both jobs, as for the rip checksums: a source is PCM in a layout (a stream's is the decoder's planar int32
// staging, validate 0; a source's its own, validate 1).  A pair names two sources; a span is a stretch of A's axis (both
// ends multiples of 4) on which A or the B window of the pair's offsets can be non-zero, and the search tiles it.
constexpr uint32_t kCmpThreads = 256;
constexpr uint32_t kCmpTileFrames = 2048;          // frames of A per search tile
constexpr uint32_t kCmpLaneOffsets = 4;            // consecutive offsets a search lane owns
constexpr uint32_t kCmpMaxRadius = 32767;
constexpr uint32_t kCmpRowFrames = 16384;          // frames per row, counted from the domain's first frame
constexpr uint32_t kCmpRowBytes = 96;              // sizeof(lacx_compare_row): per channel first, last, max_at, sum_abs, sum_sq (uint64), mismatches, max_abs (uint32)
constexpr unsigned long long kCmpNone = ~0ull;     // first / last / max_at of a row and channel in which nothing differs
constexpr uint32_t kCmpStageA = kCmpTileFrames;                                        // words per plane
constexpr uint32_t kCmpStageB = kCmpTileFrames + kCmpLaneOffsets * kCmpThreads;        // the window a full tile's offsets reach
struct CmpSource {                                 // 40 bytes
    const void* data0;                             // as DigestSource
    const void* data1;
    unsigned long long frames;
    uint32_t layout;
    uint32_t item;                                 // whose bad[] an invalid sample lowers
    uint8_t channels, bit_depth, validate, pad[5];
};
struct CmpPair {                                   // 48 bytes
    uint32_t a, b;                                 // its sources
    int32_t centre;
    uint32_t radius;
    long long chosen;                              // the offset the rows are made at: the host's, before k_compare_rows runs
    unsigned long long count0;                     // counts[count0 + (o - (centre - radius))]: mis[o]; radius 0: none
    unsigned long long row0;                       // its first row
    unsigned long long nrows;                      // ... and how many the chosen offset's domain has
};
struct CmpSpan {                                   // 32 bytes
    long long f_lo, f_hi;                          // A's frames [f_lo, f_hi), both multiples of 4, f_lo < f_hi
    uint32_t pair;
    uint32_t lanes;                                // threads across the offsets of a tile (each owns kCmpLaneOffsets): a power of two <= kCmpThreads
    uint32_t otiles;                               // offset tiles
    uint32_t pad;
};
// (constexpr: the host-only plan counts as the kernel does)
constexpr long long cmp_floor4(long long v) { return v & ~3ll; }  // (floors a negative frame too)
constexpr long long cmp_obase(const CmpPair& p) { return cmp_floor4((long long)p.centre - (long long)p.radius); }  // a tile's first offset is obase + a multiple of 4
constexpr uint32_t cmp_width(const CmpPair& p) { return 2u * p.radius + 1u; }
constexpr unsigned long long cmp_span_tiles(const CmpSpan& s) {
    return (unsigned long long)((s.f_hi - s.f_lo + kCmpTileFrames - 1) / kCmpTileFrames) * s.otiles;
}
// the union domain of offset o (lacx.h)
constexpr long long cmp_fmin(long long o) { return o > 0 ? -o : 0; }
constexpr long long cmp_fmax(unsigned long long na, unsigned long long nb, long long o) { return (long long)nb - o > (long long)na ? (long long)nb - o : (long long)na; }
struct CmpArgs {
    uint32_t npairs = 0, nspans = 0;
    unsigned long long total_tiles = 0, total_rows = 0;
    const CmpSource* sources = nullptr;
    const CmpPair* pairs = nullptr;                // [npairs]
    const CmpSpan* spans = nullptr;                // [nspans]
    const unsigned long long* tile_off = nullptr;  // [nspans + 1] prefix sums of the spans' tiles (frame tile major, offset tile minor)
    const unsigned long long* row_off = nullptr;   // [npairs + 1] prefix sums of the pairs' rows at their chosen offsets
    unsigned long long* counts = nullptr;          // zero on entry
    void* rows = nullptr;                          // lacx_compare_row [rows_cap]; every row of a pair is written whole
    unsigned long long* bad = nullptr;             // [items] lowest digest_bad_key per item (all ones on entry), or null
};
}  // namespace lacx
