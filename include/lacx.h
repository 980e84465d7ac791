/* lacx.h -- C ABI of the MI355X-native LAC block-encode path (liblacx.so).
 *
 * The reference (audexdev/Lossless-Audio-Codec, C++20) has no FFI layer: its encode boundary is two
 * C++ classes.  Each entry point below names the reference interface it replaces; the C++ mirror
 * classes with the reference's own signatures (lossless-audio-codec_amd/include/codec/...) are thin
 * wrappers over this ABI, and INTEGRATION.md shows the binding a reference maintainer would add.
 *
 *   lacx_encode            <- LAC::Encoder::encode          ref src/codec/lac/encoder.hpp:22-24, encoder.cpp:215-466
 *   lacx_encoder_create    <- LAC::Encoder::Encoder + set_zero_run_enabled / set_partitioning_enabled /
 *                             set_thread_count               ref src/codec/lac/encoder.hpp:14-29
 *   lacx_block_encode      <- Block::Encoder::encode        ref src/codec/block/encoder.hpp:15, encoder.cpp:313-838
 *   lacx_analyze           <- the decisions inside Block::Encoder::encode / estimate_stereo_mode
 *                                                            ref block/encoder.cpp:313-552, lac/encoder.cpp:126-197,321-373
 *   lacx_emit_from_plans   <- the emit half of Block::Encoder::encode + container write
 *                                                            ref block/encoder.cpp:554-838, lac/encoder.cpp:243-250,445-465
 *   lacx_wav_parse /
 *   lacx_encode_wav        <- read_wav + LAC::Encoder::encode as chained by the CLI
 *                                                            ref src/io/wav_io.cpp:167-277, src/main.cpp:640-675
 *   lacx_encode_shard /
 *   lacx_assemble          <- the block loop + block table concat of LAC::Encoder::encode, split so that
 *                             contiguous block ranges can be encoded by different GPUs/processes
 *                                                            ref lac/encoder.cpp:252-263, 445-465
 *   lacx_encoder_create_multi /
 *   lacx_encode_fanout_resident <- the worker pool of LAC::Encoder::encode with devices as the workers
 *                                                            ref lac/encoder.cpp:385-443, 445-465
 *   lacx_encode_batch_device <- one LAC::Encoder::encode per file of a corpus, as one device job
 *                                                            ref lac/encoder.cpp:215-466 (block pool :404-435)
 *   lacx_stream_parse /
 *   lacx_decode            <- LAC::Decoder::decode          ref src/codec/lac/decoder.hpp:10-24, decoder.cpp:76-303,
 *                                                            src/codec/block/decoder.cpp:64-520
 *   lacx_decoder_decode_wav <- the `decode` command's WAV writer ref src/main.cpp:127-182, 184-431
 *   lacx_decoder_decode_wav_batch_view, lacx_decoder_decode_batch_device <- many .lac streams as one device job
 *   lacx_decoder_decode_window, lacx_decoder_decode_window_batch_device <- frame windows of many streams as one job
 *   lacx_decoder_verify_batch_device,
 *   lacx_decoder_verify_wav <- the roundtrip comparison of `lac_cli selftest` (ref src/main.cpp:803-909) and of an
 *                             archive's "decode it again and compare" step: streams against their source PCM, on the device
 *   lacx_decoder_digest_batch_device,
 *   lacx_decoder_digest_pcm_batch_device,
 *   lacx_crc32_combine      <- the check the container has no field for (the reference's format carries no checksum of its
 *                             audio): CRC-32 of what streams decode to and of source PCM, made on the device
 *   lacx_decoder_salvage_wav, lacx_decoder_salvage_wav_batch_view,
 *   lacx_decoder_salvage_batch_device <- beyond the reference (like `flac -F`): decode through errors, the blocks of a
 *                             damaged or truncated stream that still decode, silence where one does not
 *   lacx_decoder_digest_blocks_batch_device, lacx_decoder_item_block_digests,
 *   lacx_decoder_digest_pcm_blocks_batch_device,
 *   lacx_manifest_build, lacx_manifest_parse,
 *   lacx_decoder_check_batch_device,
 *   lacx_decoder_salvage_wav_batch_view_checked,
 *   lacx_decoder_salvage_batch_device_checked <- damage that still decodes: one CRC-32 per block, kept in a manifest
 *                             beside the stream and honoured by the decoder (code 11, "digest mismatch")
 *   lacx_decoder_stats_batch_device, lacx_decoder_stats_pcm_batch_device,
 *   lacx_decoder_item_block_stats,
 *   lacx_stats_combine      <- what the audio is, not whether it decodes: per block and per stream peaks, energy, silence,
 *                             full-scale hits, channel equality and bit use, exact integers made on the device
 *   lacx_decoder_inspect_batch_device, lacx_decoder_item_block_info, lacx_decoder_item_partitions,
 *   lacx_inspect_combine, lacx_decoder_inspect_guard <- how a stream was coded and where its bits go: per block and per stream predictors, partition
 *                             orders, residual modes, bit and sample classes, read by a parse-only walk on the device
 *   lacx_decoder_runs_batch_device, lacx_decoder_runs_pcm_batch_device,
 *   lacx_decoder_item_runs  <- where the audio is silent, clips or holds one value: runs of consecutive frames that satisfy
 *                             a detector and reach a minimum length, found on the device
 *   lacx_decoder_loudness_batch_device, lacx_decoder_loudness_pcm_batch_device,
 *   lacx_decoder_item_loudness_rows,
 *   lacx_loudness_combine   <- how loud the audio is: ITU-R BS.1770 integrated, momentary and short-term loudness and the
 *                             loudness range of a stream or an album, the K-weighted energy made on the device
 *   lacx_decoder_truepeak_batch_device, lacx_decoder_truepeak_pcm_batch_device,
 *   lacx_decoder_item_truepeak_rows,
 *   lacx_truepeak_combine   <- how far the audio can be turned up: the ITU-R BS.1770 true peak (the maximum of the 4x
 *                             oversampled signal) of a stream or an album, in exact integers, made on the device
 *   lacx_decoder_spectrum_batch_device, lacx_decoder_spectrum_pcm_batch_device,
 *   lacx_decoder_item_spectrum_rows,
 *   lacx_spectrum_combine   <- whether the audio is what it claims to be: the long-term power spectrum in 64 bands (Hann
 *                             STFT in FP64) and the bandwidth of a stream, made on the device
 *   lacx_decoder_accuraterip_batch_device, lacx_decoder_accuraterip_pcm_batch_device,
 *   lacx_decoder_item_ar_tracks, lacx_decoder_item_ar_sums,
 *   lacx_ar_ids             <- whether the audio is an accurate rip, and of which pressing: the AccurateRip v1 / v2 track
 *                             checksums of a disc of CD audio at every read offset within a radius, made on the device
 *   lacx_decoder_compare_batch_device, lacx_decoder_compare_pcm_batch_device,
 *   lacx_decoder_item_compare_rows, lacx_decoder_item_compare_counts,
 *   lacx_compare_combine    <- how two streams relate: the differing samples at every offset within a radius and, at the
 *                             offset with the fewest, the null-test residual a - b in rows and totals, made on the device
 *   lacx_recovery_build, lacx_recovery_build_batch_view, lacx_recovery_parse,
 *   lacx_recovery_scan_batch, lacx_recovery_repair, lacx_recovery_repair_batch_view,
 *   lacx_decoder_item_bad_slices <- bringing lost bytes back: a parity sidecar ("LACR", Reed-Solomon over GF(2^8)) beside
 *                             the .lac file, made and used on the device; the manifest finds damage at the PCM level, this
 *                             sidecar locates and repairs it at the byte level
 *   lacx_transcode_batch    <- beyond the reference (like `flac --skip / --until`, joining and `flac -f` re-encoding): .lac in,
 *                             .lac out -- frame ranges of source streams cut and joined, re-channelled and re-quantised
 *                             losslessly, re-encoded as one batch, the PCM never leaving the device
 *
 * All analysis (and the decode) runs in hand-written HIP kernels on a gfx950 device; there is no CPU fallback: every
 * call that needs the device fails with LACX_E_DEVICE when none is usable.
 */
#ifndef LACX_H
#define LACX_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LACX_OK 0
#define LACX_E_INVALID 1 /* maps to std::invalid_argument (ref lac/encoder.cpp:220-241) */
#define LACX_E_RUNTIME 2 /* maps to std::runtime_error   (ref lac/encoder.cpp:447-449) */
#define LACX_E_DEVICE 3  /* HIP failure / no device: std::runtime_error in the C++ mirror */
#define LACX_E_MISMATCH 4 /* the stream decodes, but not to the given PCM */

#define LACX_MAX_BLOCK 16384u
#define LACX_SLOTS_PER_BLOCK 16u /* slot = window*4 + channel(L,R,M,S); window 0 = whole block, 1..3 = probes */

typedef struct lacx_encoder lacx_encoder;

typedef struct lacx_config {
    uint32_t sample_rate;         /* 44100 / 48000 / 96000 / 192000 */
    uint8_t bit_depth;            /* 16 / 24 */
    uint8_t stereo_mode;          /* 0 LR, 1 MS, 2 per-block auto (ignored for mono input) */
    uint8_t zero_run_enabled;     /* reference default: 1 */
    uint8_t partitioning_enabled; /* reference default: 1 */
    int32_t device;               /* HIP device ordinal, -1 = current device, LACX_DEVICE_ALL = every visible device
                                     (whole-stream calls fan the blocks out over them, see lacx_encoder_create_multi) */
    uint32_t emit_threads;        /* host emit worker threads, 0 = hardware concurrency */
    uint32_t flags;               /* LACX_FLAG_* */
} lacx_config;

#define LACX_DEVICE_ALL (-2)
#define LACX_FLAG_HOST_EMIT 1u /* keep the bit emit on the host (north_star layout); default: device-side emit */

/* Same layout as lacx::ChannelPlan (csrc/lacx_types.h). */
typedef struct lacx_channel_plan {
    uint8_t predictor_type; /* 0 fixed, 1 FIR, 2 LPC */
    uint8_t order;
    uint8_t partition_order;
    uint8_t valid;
    int16_t coef[12];
    uint32_t payload_bytes;
    uint64_t total_bits;
    uint8_t part_mode_k[256]; /* (mode << 5) | k */
} lacx_channel_plan;

/* Same layout as lacx::BlockPlan. */
typedef struct lacx_block_plan {
    uint8_t choose_ms;
    uint8_t uncertain;
    uint8_t est_ms;
    uint8_t invalid;
    uint32_t frames;
    uint32_t first_bad;
    uint32_t pad;
} lacx_block_plan;

typedef struct lacx_timing {
    double h2d_ms;          /* host -> device PCM copy (0 for device-resident input) */
    double analysis_ms;     /* all kernels, device timeline (hipEvent) */
    double ingest_ms;       /* k_ingest + k_levinson */
    double probe_ms;        /* k_analyze<4,64> + k_decide */
    double full_ms;         /* k_analyze<16,1024> (the dominant kernel), summed over its launches */
    double d2h_ms;          /* plan records device -> host, incl. stream sync */
    double emit_ms;         /* host emit tail after the last plan arrived, or (device emit) the k_emit kernels */
    double total_ms;        /* wall time of the call */
    uint64_t full_slots;    /* workgroups of the dominant kernel that did work */
    uint64_t probe_slots;
    uint32_t full_launches; /* launches of the dominant kernel in the call (one per pipeline chunk) */
    uint32_t regrows;       /* device emit: times the pinned result buffer had to be regrown and the emit re-run */
    double full_exec_ms;    /* device emit pipeline: k_analyze<16,1024> execution spans (first workgroup start to last
                               workgroup end, device clock), summed over its launches -- full_ms minus queueing */
    uint32_t emit_direct;   /* fused emit: channel blocks the streaming packer moved to the payload beside the analysis */
    uint32_t moved_by_k_pack; /* ... and those the repair kernel k_pack had to move afterwards (0 when the packer kept up) */
    uint32_t packer_gave_up;  /* packer waves that stopped after 20 ms without an awaited record (0 normally; when the
                                 packer cannot run beside the analysis -- a profiler that serialises kernels, a shared
                                 GPU -- every wave gives up and k_pack moves everything: correct, but slower) */
    uint32_t drain_copies;    /* copy-engine drain: range copies issued while the kernels ran (the tail copy not counted) */
    /* The payload drain depends on the calling thread: it polls pinned progress words and issues a copy per completed
       range.  These say how attentive it was (all in ms since the call began; 0 when the drain is not in use): */
    double drain_first_ms;    /* first range copy issued */
    double drain_last_ms;     /* last range copy issued */
    double poll_gap_max_ms;   /* longest interval between two looks at the progress words (a descheduled or busy host thread) */
    double kernels_done_ms;   /* the host saw the last kernel's completion word */
    double enqueue_ms;        /* everything enqueued (the call's launch phase) */
    uint32_t silent_copies;   /* channel blocks of nothing but zeros that were copies of the call's first one (plan and
                                 bitstream are the same for every such block of the same length) */
    uint32_t reserved0;
} lacx_timing;

int lacx_encoder_create(const lacx_config* cfg, lacx_encoder** out);
void lacx_encoder_destroy(lacx_encoder* enc);
const char* lacx_last_error(const lacx_encoder* enc);
void lacx_free(void* p);
void lacx_get_timing(const lacx_encoder* enc, lacx_timing* out);

/* sizeof() of a public struct as this library was built, by name without the prefix ("config", "channel_plan",
 * "block_plan", "timing", "pcm", "batch_item", "batch_out", "wav_info", "fanout_shard", "fanout_out", "fanout_stats",
 * "stream_info", "span", "decode_item", "window_item", "verify_item", "verify_result", "digest", "digest_source", "block_fault", "salvage_result", "block_digest", "manifest_info", "edit_segment", "edit_output", "edit_result"); 0 for an unknown name.  A binding that declares the structs itself (ctypes, cgo, JNI) checks its layout
 * against this before the first call that fills one. */
uint32_t lacx_sizeof(const char* struct_name);

/* Whole-stream encode of host planar int32 PCM (right == NULL => mono). *out is malloc'd; free with
 * lacx_free. Byte-identical to the reference's LAC::Encoder::encode output. */
int lacx_encode(lacx_encoder* enc, const int32_t* left, const int32_t* right, uint64_t frames,
                uint8_t** out, uint64_t* out_size);

/* Same, with the PCM already resident in device memory (d_*), e.g. torch tensors.  h_left/h_right are
 * the host copies the host-side emit reads; if NULL the library copies the PCM back itself.
 * `stream` is a hipStream_t (NULL = the encoder's own stream). */
int lacx_encode_device(lacx_encoder* enc, const int32_t* d_left, const int32_t* d_right,
                       const int32_t* h_left, const int32_t* h_right, uint64_t frames, void* stream,
                       uint8_t** out, uint64_t* out_size);

/* Device analysis only: fills bplans[nblocks] and plans[nblocks * LACX_SLOTS_PER_BLOCK]
 * (nblocks = ceil(frames / 16384)). Host pointers in. */
int lacx_analyze(lacx_encoder* enc, const int32_t* left, const int32_t* right, uint64_t frames,
                 lacx_block_plan* bplans, lacx_channel_plan* plans);
int lacx_analyze_device(lacx_encoder* enc, const int32_t* d_left, const int32_t* d_right, uint64_t frames,
                        void* stream, lacx_block_plan* bplans, lacx_channel_plan* plans);

/* Host-only: emit + container from plans (no device needed). */
int lacx_emit_from_plans(lacx_encoder* enc, const int32_t* left, const int32_t* right, uint64_t frames,
                         const lacx_block_plan* bplans, const lacx_channel_plan* plans, uint8_t** out,
                         uint64_t* out_size);

/* Shard interface for multi-GPU block-range splits: encodes the blocks of a frame range that starts
 * on a block boundary.  Returns the concatenated block payloads and a table of (frames, bytes) pairs
 * (2 * nblocks uint32).  Both malloc'd. */
int lacx_encode_shard(lacx_encoder* enc, const int32_t* left, const int32_t* right, uint64_t frames,
                      uint8_t** payload, uint64_t* payload_size, uint32_t** table, uint32_t* nblocks);
int lacx_encode_shard_device(lacx_encoder* enc, const int32_t* d_left, const int32_t* d_right,
                             const int32_t* h_left, const int32_t* h_right, uint64_t frames, void* stream,
                             uint8_t** payload, uint64_t* payload_size, uint32_t** table,
                             uint32_t* nblocks);

/* Zero-copy variant: *payload / *table point into buffers owned by the encoder (pinned host memory) that
 * stay valid until the next call on the same encoder. */
int lacx_encode_shard_device_view(lacx_encoder* enc, const int32_t* d_left, const int32_t* d_right,
                                  const int32_t* h_left, const int32_t* h_right, uint64_t frames, void* stream,
                                  const uint8_t** payload, uint64_t* payload_size, const uint32_t** table,
                                  uint32_t* nblocks);

/* Device-resident PCM in its source layout: the kernels read the WAV data chunk directly
 * with coalesced loads, 2 or 3 bytes per sample instead of the 4 of the planar int32 API. */
#define LACX_PCM_PLANAR_I32 0u      /* data0 = left, data1 = right (NULL for mono) */
#define LACX_PCM_INTERLEAVED_I16 1u /* data0 = interleaved little-endian int16 frames, 4-byte aligned */
#define LACX_PCM_INTERLEAVED_I24 2u /* data0 = interleaved packed 3-byte little-endian samples */
/* Tensor layouts (what torchaudio.load returns, what lacx_decoder_decode_window_batch_device writes); 3..15 and everything
 * above 18 are unknown layouts.  Accepted by lacx_encode_shard_pcm_device_view / _begin, lacx_encode_batch_device and
 * lacx_decoder_verify_batch_device; every other entry point that takes a lacx_pcm refuses them.
 * A float32 sample x stands for the integer x * 2^(bit_depth - 1) of the configured bit depth (encode) or of the stream's
 * (verify), the exact inverse of LACX_SAMPLE_F32.  It is a valid sample when that product is an integer inside
 * [-2^(b-1), 2^(b-1) - 1]: -0.0 is 0 and -1.0 the most negative sample; 1.0, NaN, +-Inf, denormals and anything off the grid
 * are not.  Nothing is ever rounded.  The encoder imports such a source into a buffer of its own with one kernel in
 * front of the analysis (interleaved int16 at depth 16, packed int24 at depth 24) and validates it in the same pass: an
 * integer outside the range fails the call with LACX_E_INVALID "<left|right> sample at index I is outside the configured PCM
 * bit depth", any other invalid value with "<left|right> sample at index I is not an exact B-bit PCM value" (all of left
 * first, then right; "stream i: " in front in a batch); no payload is returned and the encoder stays usable.  A mono
 * LACX_PCM_PLANAR_I16 source on a 4-byte aligned address is LACX_PCM_INTERLEAVED_I16 mono and is read in place.
 * Host checks, each LACX_E_INVALID: LACX_PCM_PLANAR_I16 at depth 24 "PCM layout does not match the configured bit depth",
 * a planar source whose data1 does not fit its channel count (the planar text), "PCM arrays are not 2-byte aligned" /
 * "PCM arrays are not 4-byte aligned".  Nothing outside [data, data + frames * channels * element size) is read. */
#define LACX_PCM_PLANAR_I16      16u /* data0 = left, data1 = right (NULL for mono): int16, 2-byte aligned, bit depth 16 only */
#define LACX_PCM_PLANAR_F32      17u /* data0 = left, data1 = right (NULL for mono): float32, 4-byte aligned               */
#define LACX_PCM_INTERLEAVED_F32 18u /* data0 = frames interleaved (L R L R ...): float32, 4-byte aligned                  */
typedef struct lacx_pcm {
    const void* data0;
    const void* data1;
    uint32_t layout;
    uint32_t channels; /* 1 or 2 */
} lacx_pcm;

/* Shard encode of device-resident PCM in any layout, device-side emit, zero-copy result (see
 * lacx_encode_shard_device_view).  The configured bit depth must match an interleaved layout. */
int lacx_encode_shard_pcm_device_view(lacx_encoder* enc, const lacx_pcm* d_pcm, uint64_t frames, void* stream,
                                      const uint8_t** payload, uint64_t* payload_size, const uint32_t** table,
                                      uint32_t* nblocks);

/* The same in two halves, for batch jobs (many files or shards through one process): _begin enqueues the whole
 * encode on the device and returns without waiting; _end waits for it and hands the result over.  One encode can be
 * in flight per encoder; with two encoders used alternately (begin A, end B, begin B, end A, ...) the device analyses
 * the next input while the previous one's last emit kernels are still pushing their payload over PCIe.  The result
 * views stay valid until the same encoder's next _begin. */
int lacx_encode_shard_pcm_device_begin(lacx_encoder* enc, const lacx_pcm* d_pcm, uint64_t frames, void* stream);
int lacx_encode_shard_end(lacx_encoder* enc, const uint8_t** payload, uint64_t* payload_size, const uint32_t** table,
                          uint32_t* nblocks);

/* Many streams as ONE job (BASELINE configs[4]: a mixed corpus; the reference keeps one pool over all blocks of a stream,
 * ref src/codec/lac/encoder.cpp:404-435 -- here the pool spans the blocks of all streams of the batch): one launch set
 * over every block of every stream instead of one per stream, so that short streams do not each pay the chain
 * ingest -> Levinson -> probes -> decision -> analysis by themselves.  Every stream keeps its own sample rate, bit depth,
 * channel count, stereo mode and layout; zero-run / partitioning switches come from the encoder's config.  Device-
 * resident PCM, device-side emit; out[i] views the stream's payload and block table inside the encoder's pinned result
 * buffer (valid until the next call on the encoder); lacx_assemble turns (payload, table) into the stream's .lac, the
 * bytes LAC::Encoder::encode gives for that stream alone.  Errors name the stream ("stream 3: left sample at index
 * ... is outside ..."). */
typedef struct lacx_batch_item {
    lacx_pcm pcm;         /* device-resident PCM of the stream */
    uint64_t frames;
    uint32_t sample_rate; /* 44100 / 48000 / 96000 / 192000 */
    uint8_t bit_depth;    /* 16 / 24 (an interleaved layout must match it) */
    uint8_t stereo_mode;  /* 0 LR, 1 MS, 2 per-block auto (ignored for mono) */
    uint8_t reserved[2];
} lacx_batch_item;
typedef struct lacx_batch_out {
    const uint8_t* payload;
    uint64_t payload_size;
    const uint32_t* table; /* (frames, bytes) per block */
    uint32_t nblocks;
    uint32_t reserved;
} lacx_batch_out;
int lacx_encode_batch_device(lacx_encoder* enc, const lacx_batch_item* items, uint32_t nstreams, void* stream,
                             lacx_batch_out* out);

/* WAV ingest (replaces read_wav + LAC::Encoder::encode of the CLI's encode command,
 * ref src/io/wav_io.cpp:167-277, src/main.cpp:640-675).  lacx_wav_parse walks the RIFF container in memory and
 * accepts / rejects exactly the files read_wav does (LACX_OK / LACX_E_INVALID, no device needed); lacx_encode_wav
 * copies the raw data chunk to the device as it is (2 or 3 bytes per sample), the kernels de-interleave and
 * sign-extend on load, and the complete .lac comes back -- the bytes the reference produces from the same file.
 * The encoder's sample_rate and bit_depth must match the file's. */
typedef struct lacx_wav_info {
    uint16_t channels;
    uint16_t bit_depth;
    uint32_t sample_rate;
    uint64_t frames;
    uint64_t data_offset; /* byte offset of the first sample in the file */
    uint64_t data_bytes;
} lacx_wav_info;
int lacx_wav_parse(const uint8_t* wav, uint64_t size, lacx_wav_info* out);
int lacx_encode_wav(lacx_encoder* enc, const uint8_t* wav, uint64_t size, uint8_t** out, uint64_t* out_size);
/* Zero-copy variant: *out points at the complete .lac inside the encoder's pinned result buffer (the device wrote the
 * payload there, header and block table are filled in in front of it); valid until the next call on the same encoder.
 * The upload is pipelined: the data chunk goes to the device in three pieces (1 : 3 : 4), each in front of its kernels. */
int lacx_encode_wav_view(lacx_encoder* enc, const uint8_t* wav, uint64_t size, const uint8_t** out, uint64_t* out_size);

/* Host-only: header + block table + payload concat of shards given in stream order. */
int lacx_assemble(const lacx_config* cfg, int channels, uint32_t nshards, const uint8_t* const* payloads,
                  const uint64_t* payload_sizes, const uint32_t* const* tables, const uint32_t* nblocks,
                  uint8_t** out, uint64_t* out_size);

/* ---- one stream over several devices (SURVEY 8(b) "multi-GPU fan-out lives entirely behind this shim", 8(e)) ----------
 * The reference's LAC::Encoder::encode spreads the blocks of a stream over its worker threads and concatenates their
 * payloads in block order (ref src/codec/lac/encoder.cpp:385-443 worker pool, :445-465 container).  An encoder created over
 * a device list does the same with devices as the workers: lacx_encode, lacx_encode_wav and lacx_encode_wav_view cut the
 * stream into contiguous block ranges [g*B/G, (g+1)*B/G) (lacx_fanout_range), one per lane; every lane has its own host
 * thread, streams, workspace and pinned result region on its device, uploads its range straight from the caller's buffer
 * and runs the single-device pipeline; the lanes exchange (payload bytes, block count) -- an RCCL all-gather of two u64
 * per lane over xGMI when the devices are distinct, a host-side sum otherwise (RCCL refuses two ranks on one device) --
 * and each lane copies its payload and its slice of the block table to its place in the final .lac.  The bytes do not
 * depend on the device list (blocks are independent).  Every other entry point of such an encoder runs on its first device.
 * devices: HIP ordinals, at most LACX_MAX_FANOUT; a device may appear more than once (a rehearsal of the fan-out on fewer
 * GPUs than lanes).  min_blocks_per_device: a stream is spread over fewer lanes when a lane would get fewer blocks than
 * this (0 = default 64; the reference uses min(threads, blocks) workers, encoder.cpp:385-390).
 * lacx_config.device = LACX_DEVICE_ALL in lacx_encoder_create is the list of every visible device.  LACX_FANOUT_EXCHANGE =
 * host | rccl (read at creation) forces the exchange. */
#define LACX_MAX_FANOUT 16u
int lacx_encoder_create_multi(const lacx_config* cfg, const int32_t* devices, uint32_t ndevices,
                              uint32_t min_blocks_per_device, lacx_encoder** out);
uint32_t lacx_encoder_lanes(const lacx_encoder* enc); /* 1 for a plain encoder */
/* The block range of lane `lane` of `nlanes` over a stream of `nblocks` blocks. */
void lacx_fanout_range(uint32_t nblocks, uint32_t nlanes, uint32_t lane, uint32_t* first, uint32_t* count);

/* Shards already resident in device memory, shards[g] on the device of lane g (every shard but the last a whole number of
 * blocks; LACX_PCM_PLANAR_I32 or an interleaved integer layout -- a tensor layout gives LACX_E_INVALID "PCM layout is not
 * supported by the fan-out"): every lane encodes its shard, the sizes are exchanged, out[g] views the lane's payload and block table in its
 * pinned result region (valid until the encoder's next call) with its byte offset in the stream's payload.  No
 * concatenation: lacx_assemble builds the .lac from the views where one contiguous buffer is wanted. */
typedef struct lacx_fanout_shard {
    lacx_pcm pcm; /* on the lane's device */
    uint64_t frames;
} lacx_fanout_shard;
typedef struct lacx_fanout_out {
    const uint8_t* payload;
    uint64_t payload_size;
    const uint32_t* table; /* (frames, bytes) per block */
    uint32_t nblocks;
    int32_t device;
    uint64_t byte_offset; /* of this payload inside the concatenated payload of the stream */
} lacx_fanout_out;
int lacx_encode_fanout_resident(lacx_encoder* enc, const lacx_fanout_shard* shards, uint32_t nshards, lacx_fanout_out* out);

#define LACX_EXCHANGE_HOST 1u
#define LACX_EXCHANGE_RCCL 2u
typedef struct lacx_fanout_stats {  /* of the encoder's last fanned-out call */
    uint32_t lanes_used;
    uint32_t exchange;               /* LACX_EXCHANGE_* */
    double exchange_ms;              /* longest lane: its shard finished -> every lane's sizes known (includes waiting for the slowest lane) */
    double concat_ms;                /* longest lane: table slice + payload copy into the final buffer */
    int32_t device[LACX_MAX_FANOUT];
    uint32_t blocks[LACX_MAX_FANOUT];
    uint64_t lane_frames[LACX_MAX_FANOUT];
    uint64_t payload_bytes[LACX_MAX_FANOUT];
    double encode_ms[LACX_MAX_FANOUT]; /* the lane's shard: upload, kernels, payload in its pinned region */
} lacx_fanout_stats;
int lacx_get_fanout_stats(const lacx_encoder* enc, lacx_fanout_stats* out);
int lacx_get_lane_timing(const lacx_encoder* enc, uint32_t lane, lacx_timing* out);
const char* lacx_fanout_exchange_note(const lacx_encoder* enc); /* which exchange the encoder uses, and why */

/* ---- decode: LAC::Decoder::decode, ref src/codec/lac/decoder.hpp:10-24, decoder.cpp:76-303,
 * src/codec/block/decoder.cpp:64-520.  The product's own check that a .lac gives back the PCM, on the device: one lane
 * per block (the format serialises everything inside a block), all blocks of the stream at once.
 * lacx_stream_parse: host only; the reference reader's structural rules for the header and the block table (versions 3
 * and 2), LACX_E_INVALID otherwise.  Two documented deviations from the reference reader: its 1 GiB cap on the decoded PCM
 * is not taken over (it would refuse the 2 h stream), and a compressed block must stay below 2^29 bytes (the device
 * reader's bit positions are 32-bit and relative to the block; the reference accepts any non-zero size that fits the
 * file -- no encoder produces such a block: 16384 frames x 2 channels cost at most a few hundred KiB).
 * lacx_decode: left / right (right may be null for mono) are caller-owned arrays of `frames` int32 each; a malformed
 * block, a sample outside the bit depth or a residual magnitude the encoder's domain cannot produce (>= 2^30) gives
 * LACX_E_RUNTIME ("[decode-error] block=N ..." in lacx_decode_last_error, the reference throws std::runtime_error with
 * that prefix, decoder.cpp:24-32).  device = -1: the current device.  device_ms (nullable): kernel time. */
typedef struct lacx_stream_info {
    uint32_t sample_rate;
    uint32_t blocks;
    uint64_t frames;
    uint8_t channels;
    uint8_t bit_depth;
    uint8_t stereo_mode;
    uint8_t version; /* 3, or the legacy 2 (no compressed block sizes: decoded by one lane) */
} lacx_stream_info;
int lacx_stream_parse(const uint8_t* lac, uint64_t size, lacx_stream_info* out);
int lacx_decode(int device, const uint8_t* lac, uint64_t size, int32_t* left, int32_t* right, uint64_t frames,
                float* device_ms);
const char* lacx_decode_last_error(void); /* of the calling thread */
/* The same through a decoder object (ref LAC::Decoder, src/codec/lac/decoder.hpp:10-24) whose device buffers, stream and
 * events live from call to call; lacx_decode keeps one such object per device for the life of the process, and calls on
 * one device take turns under a mutex.  device = -1: the device that is current at the first call. */
typedef struct lacx_decoder lacx_decoder;
int lacx_decoder_create(int device, lacx_decoder** out);
void lacx_decoder_destroy(lacx_decoder* dec);
int lacx_decoder_decode(lacx_decoder* dec, const uint8_t* lac, uint64_t size, int32_t* left, int32_t* right, uint64_t frames,
                        float* device_ms);
/* WAV image of a .lac (ref src/main.cpp:184-431 decode_lac_v3_to_mapped_wav, and write_wav_unchecked_samples for
 * version-2 streams): 44-byte canonical header + PCM + pad byte, byte-identical to the reference CLI's output file.
 * The same parse (lacx_stream_parse), error codes and "[decode-error] block=N ..." messages (lacx_decode_last_error) as
 * lacx_decoder_decode; the mid/side inverse, the bit-depth check and the interleave to 16 / 24-bit little-endian run on the
 * device in one pass after the block decode, and header + data cross PCIe as one copy.  Limits: lacx_stream_parse's --
 * the RIFF limit (36 + data + pad < 2^32) is kept, the reference's 1 GiB cap on the decoded PCM is not taken over (see
 * above).  On failure *out is null.  device_ms (nullable): kernel time (decode and pack).
 * lacx_decoder_decode_wav: *out is malloc'd, release it with lacx_free.
 * lacx_decoder_decode_wav_view: *out points into the decoder's pinned image buffer, valid until the decoder's next call
 * or lacx_decoder_destroy. */
int lacx_decoder_decode_wav(lacx_decoder* dec, const uint8_t* lac, uint64_t size,
                            uint8_t** out, uint64_t* out_size, float* device_ms);
int lacx_decoder_decode_wav_view(lacx_decoder* dec, const uint8_t* lac, uint64_t size,
                                 const uint8_t** out, uint64_t* out_size, float* device_ms);

/* Many streams as ONE decode.  A single stream never decodes in less than one block's serial chain, however few blocks
 * it has, and leaves most of the chip idle; a batch puts every block of every item into one launch (one lane per
 * version-3 block, one lane per version-2 item), so a collection costs about one chain.  Each item keeps its own rate,
 * depth, channels, stereo mode and container version.
 * Per-item outcome: one bad stream does not cost the others.  item_rc (nullable, n entries) receives LACX_OK or the
 * item's code, lacx_decoder_item_error(dec, i) the item's message from the last batch call ("" when it decoded): exactly
 * what the single-stream call reports for it (lacx_stream_parse's errors, "[decode-error] block=N ...").  The call
 * returns LACX_OK when every item decoded, else the lowest failing item's code with "stream i: <message>" in
 * lacx_decode_last_error; LACX_E_DEVICE only for a failure of the whole call (every item that parsed then carries it).
 * Parse errors are found on the host before any device call; without a device the per-item parse results are still
 * filled and the call returns LACX_E_DEVICE "no usable HIP device".  n = 0 or a null array: LACX_E_INVALID.
 * A batch and single-stream calls may alternate on one decoder.  device_ms (nullable): kernel time of the batch. */
typedef struct lacx_span {
    const uint8_t* data;
    uint64_t size;
} lacx_span;
/* lacs[i]: the items' .lac bytes.  out[i]: item i's WAV image (what lacx_decoder_decode_wav gives for it alone), {NULL, 0}
 * for a failed item.  _view: the images lie in the decoder's pinned image buffer (16-byte aligned each, one D2H copy for
 * all), valid until the decoder's next call; lacx_decoder_decode_wav_batch: each image malloc'd, release with lacx_free. */
int lacx_decoder_decode_wav_batch_view(lacx_decoder* dec, const lacx_span* lacs, uint32_t n, lacx_span* out, int* item_rc,
                                       float* device_ms);
int lacx_decoder_decode_wav_batch(lacx_decoder* dec, const lacx_span* lacs, uint32_t n, lacx_span* out, int* item_rc,
                                  float* device_ms);
/* Device-resident output: left / right (right NULL for mono) are caller-owned device arrays of `frames` int32 each on the
 * decoder's device (a torch tensor's data_ptr()); nothing outside [0, frames) is written.  A missing array or a frames
 * mismatch fails that item with LACX_E_INVALID (lacx_decoder_decode's messages).  The work goes on `stream` (a
 * hipStream_t, NULL = the null stream) behind what is already there; the call returns once the outputs are final and the
 * statuses checked.  The arrays of a failed item hold unspecified samples. */
typedef struct lacx_decode_item {
    const uint8_t* lac;
    uint64_t size;
    int32_t* left;
    int32_t* right;
    uint64_t frames;
} lacx_decode_item;
int lacx_decoder_decode_batch_device(lacx_decoder* dec, const lacx_decode_item* items, uint32_t n, void* stream,
                                     int* item_rc, float* device_ms);
const char* lacx_decoder_item_error(const lacx_decoder* dec, uint32_t i);

/* Frame windows: frames [start, start + frames) of each item, for a seek, a preview or random crops of a collection.
 * Every block decodes on its own (raw warm-up samples, fresh Rice state), so of a version-3 stream only the blocks that
 * overlap the window are decoded, and only their bytes cross PCIe; a batch of windows is one job of about one block's
 * serial chain.  Those blocks decode whole and all of their samples are checked against the bit depth: a window fails
 * if and only if one of its blocks would fail in a full decode, with the message the full decode gives for the lowest
 * failing block among them ("[decode-error] block=N ...", N counted in the stream); a damaged block outside the window
 * does not matter.  A version-2 stream has no compressed block sizes: it is decoded in full by one lane and then
 * windowed, at the cost of a full serial decode, and any of its blocks fails it.
 * Samples: LACX_SAMPLE_I32 the stream's integer samples, LACX_SAMPLE_F32 sample * 2^-(bit_depth - 1) (exact for 16- and
 * 24-bit samples).  The outputs need only 4-byte alignment; nothing outside [0, frames) is written, and a mono item's
 * right array is neither needed nor written.  Before any device call each item is parsed (lacx_stream_parse) and its
 * window and arrays checked: frames = 0 gives "empty window", start + frames beyond the stream (checked without
 * wrap-around) "window outside the stream", a missing array "output arrays missing", each LACX_E_INVALID.  An unknown
 * sample type, n = 0 or a null array fail the whole call with LACX_E_INVALID.
 * lacx_decoder_decode_window_batch_device: caller-owned device arrays on the decoder's device; per-item outcome, return
 * code, device-less behaviour and `stream` as lacx_decoder_decode_batch_device.  The arrays of a failed item hold
 * unspecified samples.
 * lacx_decoder_decode_window: one window into caller-owned host arrays, a batch of one: the window is copied to them
 * only once it has decoded, so a failing call leaves them untouched; its message carries no "stream 0: ".
 * device_ms (nullable): kernel time. */
#define LACX_SAMPLE_I32 0 /* int32, the stream's integer samples */
#define LACX_SAMPLE_F32 1 /* float32, sample * 2^-(bit_depth - 1): exact for 16- and 24-bit samples */
typedef struct lacx_window_item {
    const uint8_t* lac;
    uint64_t size;
    uint64_t start;  /* first frame of the window */
    uint64_t frames; /* >= 1, start + frames <= the stream's frame count */
    void* left;      /* `frames` samples of the call's sample type */
    void* right;     /* stereo only; ignored for a mono item, whose right array is never written */
} lacx_window_item;
int lacx_decoder_decode_window_batch_device(lacx_decoder* dec, const lacx_window_item* items, uint32_t n, int sample_type,
                                            void* stream, int* item_rc, float* device_ms);
int lacx_decoder_decode_window(lacx_decoder* dec, const uint8_t* lac, uint64_t size, uint64_t start, uint64_t frames,
                               int sample_type, void* left, void* right, float* device_ms);

/* Verification: does a .lac decode to exactly the PCM it was made from?  The stream is decoded into the decoder's own
 * buffers and compared there, sample by sample as full int32 values, with the source PCM in the source's own layout
 * (lacx_pcm, as on the encode side: planar int32 with 4-byte aligned arrays, interleaved int16 with a 4-byte aligned
 * base, packed interleaved int24 at any byte alignment, planar int16 with 2-byte aligned arrays -- depth 16 only --, planar
 * and interleaved float32 with 4-byte aligned arrays); no PCM crosses PCIe towards the host, only 32 bytes per item.
 * A float32 source sample that is no valid sample of the stream's bit depth (see LACX_PCM_PLANAR_F32) can never equal a
 * decoded one: it counts as a differing sample, and lacx_verify_result.source then holds x * 2^(b-1) rounded to nearest
 * (ties to even) and saturated to int32, INT32_MIN for a NaN.
 * Nothing outside [data, data + frames * channels * bytes per sample) of an interleaved source, or outside [0, frames)
 * of a planar array, is read.
 * lacx_decoder_verify_batch_device: many streams as one device job, versions 3 and 2.  Per-item outcome, return code,
 * lacx_decoder_item_error, device-less behaviour and `stream` exactly as lacx_decoder_decode_batch_device.  Checked per
 * item on the host before any device call, each LACX_E_INVALID: "unknown source layout", "source channel count does not
 * match the stream", "source arrays missing", "source frame count does not match the stream", "source layout does not
 * match the stream's bit depth" (an interleaved integer layout and planar int16 fix the depth), "source arrays are not 4-byte
 * aligned", "source arrays are not 2-byte aligned" (planar int16).  An item
 * that does not decode gets the decode's own code and message and a zeroed result.  An item that decodes to something
 * else gets LACX_E_MISMATCH, its result filled, and the message
 *   [verify-error] block=N channel=left|right frame=F decoded=X source=Y mismatches=M
 * results (nullable, n entries): all zero for an item that is identical to its source (and for one that failed).
 * lacx_decoder_verify_wav: a stream against a WAV file image in host memory (lacx_wav_parse's rules; an image it refuses
 * gives LACX_E_INVALID).  A difference in format gives LACX_E_MISMATCH "[verify-error] <field>: stream A, source B"
 * (field: channels, bit depth, sample rate, frames) without touching the device, and a zeroed result.  Otherwise the data
 * chunk is uploaded as it is, 2 or 3 bytes per sample, into the decoder's payload buffer behind the payload, and compared
 * as a batch of one: the message carries no "stream 0: ".
 * device_ms (nullable): kernel time (decode and compare). */
typedef struct lacx_verify_item {   /* 48 bytes */
    const uint8_t* lac;
    uint64_t size;
    lacx_pcm pcm;                   /* device-resident source, any LACX_PCM_* layout */
    uint64_t frames;
} lacx_verify_item;
typedef struct lacx_verify_result { /* 32 bytes */
    uint64_t mismatches;            /* samples that differ; 0 = identical */
    uint64_t frame;                 /* lowest differing frame (then lowest channel) */
    uint32_t block;                 /* the block of that frame, counted in the stream */
    uint8_t channel;
    uint8_t reserved[3];
    int32_t decoded, source;        /* the two values there */
} lacx_verify_result;
int lacx_decoder_verify_batch_device(lacx_decoder* dec, const lacx_verify_item* items, uint32_t n, void* stream,
                                     int* item_rc, lacx_verify_result* results, float* device_ms);
int lacx_decoder_verify_wav(lacx_decoder* dec, const uint8_t* lac, uint64_t size, const uint8_t* wav, uint64_t wav_size,
                            lacx_verify_result* result, float* device_ms);

/* Digests: what does a .lac decode to, without the source and without moving the PCM?  The stream is decoded into the
 * decoder's own buffers as for a verification, and the bytes its WAV data chunk would have -- interleaved little-endian,
 * bit_depth / 8 per sample -- are checksummed where they lie; the same kernel checksums device-resident source PCM in any
 * lacx_pcm layout, so that a pipeline can record the digest of what it hands to the encoder and later check the .lac alone
 * against that record.  The checksum is the standard CRC-32 (zlib, ISO-HDLC: reflected polynomial 0xEDB88320, init and
 * final xor 0xFFFFFFFF): data_crc32 is zlib.crc32 of the data chunk, wav_crc32 that of the whole file `lac_cli decode` /
 * lacx_decoder_decode_wav writes (canonical 44-byte header, data, pad byte), made on the host from data_crc32 with
 * lacx_crc32_combine.  CRC-32 is linear, so every thread digests four frames and the pieces are added up in any order;
 * no PCM crosses PCIe towards the host, only 8 bytes per item.
 * lacx_decoder_digest_batch_device: many streams as one device job, versions 3 and 2.  Per-item outcome, return code,
 * lacx_decoder_item_error, device-less behaviour, n = 0 / null arrays and `stream` exactly as
 * lacx_decoder_decode_batch_device.  An item that does not parse or does not decode gets the decode's own code and
 * message and a zeroed digest.
 * lacx_decoder_digest_pcm_batch_device: device-resident PCM on the decoder's device; the same layouts, alignments and
 * bounds as the verify form's sources (nothing outside the source's bytes is read), the same per-item outcome.  Checked
 * per item on the host before any device call, each LACX_E_INVALID: "unknown source layout", "unsupported channel count",
 * "source arrays missing", "source has no frames", "source frame count out of range" (2^56 and more), "unsupported sample
 * rate: R", "unsupported bit depth: B", "source layout does not match the stream's bit depth" (the verify form's text: an interleaved integer layout and
 * planar int16 fix the depth), "source arrays are not 4-byte aligned", "source arrays are not 2-byte aligned" (planar
 * int16).  Found on the device, LACX_E_INVALID with the encoder's texts (all of left first, then right, the lowest index):
 * a planar int32 sample outside the depth, or a float32 whose product is an integer outside it, "<left|right> sample at index I
 * is outside the configured PCM bit depth"; any other float32 that is no sample of the depth (see LACX_PCM_PLANAR_F32)
 * "<left|right> sample at index I is not an exact B-bit PCM value".  A failed item gets a zeroed digest.
 * out (n entries; nullable).  device_ms (nullable): kernel time (the decode, where there is one, and the digest).
 * lacx_crc32_combine: host only, no device: crc32(A || B) from crc32(A), crc32(B) and the length of B (zlib's
 * crc32_combine). */
typedef struct lacx_digest {          /* 32 bytes */
    uint32_t data_crc32;              /* CRC-32 of the WAV data chunk's bytes, pad byte excluded */
    uint32_t wav_crc32;               /* CRC-32 of the whole WAV file image (44-byte header + data + pad); 0 when wav_valid == 0 */
    uint64_t frames;
    uint64_t data_bytes;              /* frames * channels * bit_depth / 8 */
    uint32_t sample_rate;
    uint8_t channels, bit_depth;
    uint8_t wav_valid;                /* 0: the image would break the RIFF limit (36 + data + pad < 2^32): a source only */
    uint8_t reserved;
} lacx_digest;
typedef struct lacx_digest_source {   /* 40 bytes */
    lacx_pcm pcm;                     /* device-resident source, any LACX_PCM_* layout */
    uint64_t frames;
    uint32_t sample_rate;             /* 44100 / 48000 / 96000 / 192000 */
    uint8_t bit_depth;                /* 16 / 24 */
    uint8_t reserved[3];
} lacx_digest_source;
int lacx_decoder_digest_batch_device(lacx_decoder* dec, const lacx_span* lacs, uint32_t n, void* stream, int* item_rc,
                                     lacx_digest* out, float* device_ms);
int lacx_decoder_digest_pcm_batch_device(lacx_decoder* dec, const lacx_digest_source* src, uint32_t n, void* stream,
                                         int* item_rc, lacx_digest* out, float* device_ms);
uint32_t lacx_crc32_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b);

/* Salvage: decode through errors.  Every other decode entry point refuses an item at its lowest failing block; these
 * give back whatever still decodes.  A salvage decode of an item always yields the stream's full frame count, every
 * frame at its own position, described as the header and the block table describe the stream.  A block that decodes
 * holds exactly what the strict decode gives for it (mid/side inverse applied, both channels inside the bit depth).  A
 * block that does not is digital silence, every frame 0 in both channels -- nothing of a half-decoded block leaks out:
 *   1..6, 9  its lane ended with that status (the "[decode-error] block=N <text>" causes of the strict decode)
 *   7        one of its samples lies outside the bit depth after the inverse
 *   8        a version-2 block behind the first failing one ("not reached": that container has no sizes to find it by)
 *   10       LACX_BLOCK_MISSING, "payload missing": the file ends before the block's last byte
 * Truncation: for a version-3 stream the parse is lenient in exactly one respect, the payload's length.  Header and
 * block table must pass every rule of lacx_stream_parse (a damaged table fails the item with that parser's message); the
 * file may end early.  A block is present when its whole byte range lies inside the file; the others -- always a suffix
 * of the stream -- are missing and never decoded, and only the present blocks' bytes go to the device.  A short file is
 * flagged LACX_SALVAGE_TRUNCATED; bytes behind the last block's end are ignored and flagged LACX_SALVAGE_TRAILING.  A
 * truncated version-2 stream needs no such rule: it shows as a failing block of the serial lane, followed by 8s.
 * The device works in two passes in stream order, because status 7 is final only once every sample of a block has been
 * examined: the mid/side inverse with the range check in place, then one pass that only reads the final status words
 * and packs (WAV forms) or blanks (device form).  Against lacx_decoder_decode_wav the WAV forms pay one more write and
 * read of the PCM.  The status copy of every decode is the whole report: no second round trip.
 * Outcome: an item's code is LACX_OK whenever its container was accepted, even when every block is lost; the result
 * says how much was lost, lacx_decoder_item_faults which blocks.  An item whose container is refused keeps the strict
 * code and message.  item_rc, lacx_decoder_item_error, the return code ("stream i: <message>" of the lowest failing
 * item), LACX_E_DEVICE for a failure of the whole call, n = 0 / null arrays and device-less behaviour exactly as
 * lacx_decoder_decode_batch_device.  A clean stream gives the bytes lacx_decoder_decode_wav gives and no fault.
 * lacx_stream_scan: host only, the lenient parse: *info as lacx_stream_parse fills it (frames from the table),
 *   *present_blocks, *flags (LACX_SALVAGE_*).  What a caller of lacx_decoder_salvage_batch_device sizes its arrays by.
 * lacx_decoder_salvage_wav_batch_view: out[i] = item i's WAV image in the decoder's pinned image buffer (as
 *   lacx_decoder_decode_wav_batch_view), results[i] (n entries, nullable) its loss; zeroed for a refused item.
 * lacx_decoder_salvage_wav: a batch of one; *out malloc'd (lacx_free); the message carries no "stream 0: ".
 * lacx_decoder_salvage_batch_device: caller-owned device int32 arrays of items[i].frames each, the value
 *   lacx_stream_scan reports; nothing outside [0, frames) is written, a mono item's right array is not touched.  The work
 *   goes on `stream`, and the call returns when it is done.
 * lacx_decoder_item_faults: the lost blocks of item i of the decoder's last salvage call, ascending by block; valid until
 *   the decoder's next call.  LACX_E_INVALID for an index outside that call.
 * lacx_block_fault_text: "block header", "channel header", "residual", "padding", "sample overflow", "trailing bytes",
 *   "sample outside the bit depth", "not reached", "residual beyond 2^30", "payload missing" for 1..10, "digest mismatch" for 11 (LACX_BLOCK_DIGEST, below); "" for 0, else "?". */
#define LACX_BLOCK_MISSING 10u
#define LACX_SALVAGE_TRUNCATED 1u
#define LACX_SALVAGE_TRAILING 2u
typedef struct lacx_block_fault { /* 24 bytes */
    uint32_t block, code;         /* block counted in the stream; 1..10 */
    uint64_t frame;               /* first frame of the block in the stream */
    uint32_t frames, reserved;
} lacx_block_fault;
typedef struct lacx_salvage_result { /* 32 bytes */
    uint32_t blocks, bad_blocks;
    uint64_t frames, lost_frames;
    uint32_t first_bad; /* lowest lost block; == blocks when none */
    uint32_t flags;     /* LACX_SALVAGE_* */
} lacx_salvage_result;
int lacx_stream_scan(const uint8_t* lac, uint64_t size, lacx_stream_info* info, uint32_t* present_blocks, uint32_t* flags);
int lacx_decoder_salvage_wav_batch_view(lacx_decoder* dec, const lacx_span* lacs, uint32_t n, lacx_span* out, int* item_rc,
                                        lacx_salvage_result* results, float* device_ms);
int lacx_decoder_salvage_wav(lacx_decoder* dec, const uint8_t* lac, uint64_t size, uint8_t** out, uint64_t* out_size,
                             lacx_salvage_result* result, float* device_ms);
int lacx_decoder_salvage_batch_device(lacx_decoder* dec, const lacx_decode_item* items, uint32_t n, void* stream,
                                      int* item_rc, lacx_salvage_result* results, float* device_ms);
int lacx_decoder_item_faults(const lacx_decoder* dec, uint32_t i, const lacx_block_fault** faults, uint32_t* count);
const char* lacx_block_fault_text(uint32_t code);

/* Block digests and manifests: finding damage that still decodes.  Salvage sees a block only when its lane or the range
 * check refuses it; a flipped residual bit usually decodes cleanly to other samples inside the bit depth, and the LAC
 * container has no checksum.  A manifest is a sidecar kept beside the stream: one CRC-32 per block of what the stream
 * decodes to (the bytes that block has in the WAV data chunk), made on the device where the samples lie; the decoder
 * honours it: a block that decodes to something else is lost with code 11, LACX_BLOCK_DIGEST, "digest mismatch".
 * On the device k_digest_blocks runs behind the in-place mid/side inverse of a salvage job and adds every four-frame
 * unit's value up at the end of its BLOCK; with a manifest k_digest_judge then compares and stores status 11 in front of
 * the salvage pass, which blanks such a block like any other lost one.  4 bytes per block come back beside the statuses.
 * Manifest, big-endian like the container, 32 + 8 * blocks bytes: "LACM", version 1, channels, bit depth, 0, sample rate
 * u32, frames u64, blocks u32, data_crc32 u32 (of the whole data chunk: what lacx_decoder_digest_batch_device gives),
 * per block frames u32 and crc32 u32, and the zlib CRC-32 of all bytes before it.
 * lacx_decoder_digest_blocks_batch_device: lenient like salvage, versions 3 and 2: an item is LACX_OK whenever its
 *   container is accepted.  lacx_decoder_item_block_digests then gives item i's rows, valid until the decoder's next call:
 *   a row of a lost block carries its fault code (1..10) and crc32 0.  out[i] (nullable array) has data_crc32 / wav_crc32
 *   only when every block decoded, made on the host from the rows with lacx_crc32_combine -- what
 *   lacx_decoder_digest_batch_device gives for that stream; otherwise both are 0 and wav_valid is 0.
 * lacx_decoder_digest_pcm_blocks_batch_device: device-resident source PCM on a regular grid of block_frames frames (0
 *   means 16384; else 256..16384, anything else LACX_E_INVALID for the call); per-item checks, validation texts and bounds
 *   exactly those of lacx_decoder_digest_pcm_batch_device.  The rows through lacx_decoder_item_block_digests.
 * lacx_manifest_build: host only.  Refuses a row with code != 0 (LACX_E_INVALID, "manifest needs every block's digest:
 *   block N is lost") and rows that do not fit d.  *out is malloc'd (lacx_free).
 * lacx_manifest_parse: host only; rows nullable (rows_cap entries otherwise).  LACX_E_INVALID, each message starting
 *   "[manifest-error] " (lacx_decode_last_error): short input, wrong magic, wrong version, size != 32 + 8 * blocks, wrong
 *   own checksum, channels not 1 or 2, bit depth not 16 or 24, an unsupported sample rate, blocks = 0, a row of 0 or more
 *   than 16384 frames, a non-final row below 256 frames, rows that do not sum to frames, a data_crc32 that is not the
 *   lacx_crc32_combine of the rows.
 * lacx_decoder_check_batch_device: is this stream intact?  No fault and not truncated: LACX_OK.  A fault or a truncation:
 *   LACX_E_MISMATCH "[check-error] block=N <fault text> bad_blocks=M" (N the lowest bad block), results[i] filled as
 *   salvage fills it, the blocks through lacx_decoder_item_faults, code 11 among them.  A difference in format:
 *   LACX_E_MISMATCH "[check-error] <field>: stream A, manifest B" before any device work for that item (fields: channels,
 *   bit depth, sample rate, frames, blocks, block N frames).  A refused manifest: LACX_E_INVALID with the parser's text; a
 *   refused container keeps the strict code and text.  A version-2 block with status 8 is "not reached" and not judged.
 * lacx_decoder_salvage_wav_batch_view_checked / lacx_decoder_salvage_batch_device_checked: the salvage forms with a
 *   manifest per item; {NULL, 0} means plain salvage for that item.  A block whose digest differs is silence and is listed
 *   with code 11.  An item whose manifest is refused or does not fit fails as in check and yields nothing.
 * Everything else as lacx_decoder_decode_batch_device: the return code, "stream i: " prefixes, n = 0, null arrays,
 * device-less behaviour and `stream`. */
#define LACX_BLOCK_DIGEST 11u
typedef struct lacx_block_digest { /* 16 bytes */
    uint32_t frames, crc32;        /* crc32 of the block's bytes in the WAV data chunk; 0 for a lost block */
    uint32_t code, reserved;       /* 0, or why the block is lost (1..10) */
} lacx_block_digest;
typedef struct lacx_manifest_info { /* 24 bytes */
    uint32_t sample_rate, blocks;
    uint64_t frames;
    uint32_t data_crc32;
    uint8_t channels, bit_depth, reserved[2];
} lacx_manifest_info;
int lacx_decoder_digest_blocks_batch_device(lacx_decoder* dec, const lacx_span* lacs, uint32_t n, void* stream, int* item_rc,
                                            lacx_digest* out, float* device_ms);
int lacx_decoder_item_block_digests(const lacx_decoder* dec, uint32_t i, const lacx_block_digest** rows, uint32_t* count);
int lacx_decoder_digest_pcm_blocks_batch_device(lacx_decoder* dec, const lacx_digest_source* src, uint32_t n, uint32_t block_frames,
                                                void* stream, int* item_rc, lacx_digest* out, float* device_ms);
int lacx_manifest_build(const lacx_digest* d, const lacx_block_digest* rows, uint32_t count, uint8_t** out, uint64_t* size);
int lacx_manifest_parse(const uint8_t* m, uint64_t size, lacx_manifest_info* info, lacx_block_digest* rows, uint32_t rows_cap);
int lacx_decoder_check_batch_device(lacx_decoder* dec, const lacx_span* lacs, const lacx_span* manifests, uint32_t n, void* stream,
                                    int* item_rc, lacx_salvage_result* results, float* device_ms);
int lacx_decoder_salvage_wav_batch_view_checked(lacx_decoder* dec, const lacx_span* lacs, const lacx_span* manifests, uint32_t n,
                                                lacx_span* out, int* item_rc, lacx_salvage_result* results, float* device_ms);
int lacx_decoder_salvage_batch_device_checked(lacx_decoder* dec, const lacx_decode_item* items, const lacx_span* manifests, uint32_t n,
                                              void* stream, int* item_rc, lacx_salvage_result* results, float* device_ms);

/* Audio statistics: peaks, energy, silence and bit use, made on the device where the samples lie.  Decode, verify, digest
 * and check answer whether a stream decodes and to what bytes; these entry points answer what the audio is: is it digital
 * silence and where does the sound start and stop, does it hit full scale, is this stereo file two identical channels, is
 * this 24-bit file 16-bit audio with eight zero bits, what are its peak, DC and energy and where along the stream is the
 * energy.  Every quantity is an exact integer reduction over the final left / right samples of the stream's bit depth b;
 * nothing floating-point crosses this ABI (dBFS, RMS and the like are derived by the caller).
 * A stats job is the blocks form of a salvage job: k_stats_blocks runs behind the in-place mid/side inverse in the slot
 * k_digest_blocks has, every block's status final, and leaves one row per block (at most 16384 frames): about 100 bytes per
 * block come back, not the PCM.  The rows are the stream's energy and silence envelope.
 * lacx_channel_stats, per block and per channel: min, max; or_bits: OR of the samples' low b bits; full_scale: samples equal
 *   to -2^(b-1) or 2^(b-1)-1; zeros: samples equal to 0; sum; sum_sq (at most 16384 * 2^46).
 * lacx_block_stats: frames; code: 0, or why the block is lost (1..10, as lacx_block_digest.code); lead_zero_frames /
 *   trail_zero_frames: the leading / trailing frames whose samples are 0 in every channel (both equal frames for a silent
 *   block); differing: frames with left != right (0 for mono); ch[1] is all zero for mono.  A lost block's row has its
 *   frames and code, every other field 0.
 * lacx_stats, per item, made on the host from the rows by lacx_stats_combine: totals over the decoded blocks.
 *   silent_blocks: decoded blocks with lead_zero_frames == frames.  lead_zero_frames / trail_zero_frames: the frames before
 *   the first, and after the last, frame that is non-zero or lies in a lost block (a lost block is not known to be silent,
 *   so it counts as sound).  sum and sum_sq are 128-bit pairs: a stream may have 2^56 frames.  With no decoded block min
 *   and max are 0.
 * lacx_decoder_stats_batch_device: lenient exactly like lacx_decoder_digest_blocks_batch_device -- versions 3 and 2,
 *   truncated files, LACX_OK whenever the container is accepted; a refused container keeps the strict code and text and
 *   gets a zeroed result.  out: nullable array of n.
 * lacx_decoder_stats_pcm_batch_device: device-resident source PCM in any LACX_PCM_* layout on a regular grid of
 *   block_frames frames (0 means 16384; else 256..16384, anything else LACX_E_INVALID for the call); the per-item host
 *   checks, the device-found validation texts and the bounds are those of lacx_decoder_digest_pcm_blocks_batch_device.  A
 *   failed item gets a zeroed result and no rows.
 * lacx_decoder_item_block_stats: the rows of item i of the decoder's last stats call, valid until its next call;
 *   LACX_E_INVALID outside that call.
 * lacx_stats_combine: host only, no device: the totals of `count` rows (rows may be null when count is 0), public so that
 *   a caller can total a sub-range of rows (a window's blocks).  LACX_E_INVALID: null out, null rows with count > 0,
 *   channels not 1 or 2, bit depth not 16 or 24.
 * Everything else as lacx_decoder_decode_batch_device: the return code, "stream i: " prefixes, lacx_decoder_item_error,
 * n = 0, null arrays, device-less behaviour (host-side outcomes filled, then LACX_E_DEVICE) and `stream`.
 * Time (scripts/stats_bench.py, profiles/stats_bench.txt): on 48 four-minute stereo streams as one job 24.4 ms of
 * kernels, 1.9 ms below the block digests' job; k_stats_blocks alone 6.1 ms for 4.06 GB of PCM, which is not bound by
 * reading it once.  What bounds it is not measured yet. */
typedef struct lacx_channel_stats { /* 40 bytes */
    int32_t min, max;
    uint32_t or_bits, full_scale, zeros, reserved;
    int64_t sum;
    uint64_t sum_sq;
} lacx_channel_stats;
typedef struct lacx_block_stats {   /* 104 bytes */
    uint32_t frames, code;
    uint32_t lead_zero_frames, trail_zero_frames;
    uint32_t differing, reserved;
    lacx_channel_stats ch[2];
} lacx_block_stats;
typedef struct lacx_channel_totals { /* 64 bytes */
    int32_t min, max;
    uint32_t or_bits, reserved;
    uint64_t full_scale, zeros;
    uint64_t sum_lo;                /* sum as a signed 128-bit value: sum_hi * 2^64 + sum_lo */
    int64_t sum_hi;
    uint64_t sum_sq_lo, sum_sq_hi;  /* sum_sq as an unsigned 128-bit value */
} lacx_channel_totals;
typedef struct lacx_stats {         /* 192 bytes */
    uint64_t frames;
    uint32_t sample_rate;
    uint8_t channels, bit_depth, reserved[2];
    uint32_t blocks, lost_blocks;
    uint64_t lost_frames;
    uint32_t silent_blocks, reserved2;
    uint64_t lead_zero_frames, trail_zero_frames;
    uint64_t differing;
    lacx_channel_totals ch[2];
} lacx_stats;
int lacx_decoder_stats_batch_device(lacx_decoder* dec, const lacx_span* lacs, uint32_t n, void* stream, int* item_rc, lacx_stats* out,
                                    float* device_ms);
int lacx_decoder_stats_pcm_batch_device(lacx_decoder* dec, const lacx_digest_source* src, uint32_t n, uint32_t block_frames, void* stream,
                                        int* item_rc, lacx_stats* out, float* device_ms);
int lacx_decoder_item_block_stats(const lacx_decoder* dec, uint32_t i, const lacx_block_stats** rows, uint32_t* count);
int lacx_stats_combine(const lacx_block_stats* rows, uint32_t count, uint8_t channels, uint8_t bit_depth, uint32_t sample_rate,
                       lacx_stats* out);

/* Stream inspection: how a stream was coded and where its bits go.  Decode and salvage say whether a stream decodes,
 * digest and manifest to what bytes, recovery whether it can be repaired, stats what the audio is; these entry points
 * say which predictor, order and partition order every channel block got, which residual mode every partition, how the
 * bits divide into header, unary quotients, remainders, tags, escapes and padding, and how many samples sit in zero runs.
 * An inspection job is a parse-only walk: k_inspect (one lane per version-3 block) and k_inspect_serial (one lane per
 * version-2 stream) read the tokens, follow the Rice adaptation -- which depends on residual magnitudes alone -- and keep
 * a tally.  Nothing is synthesised and no PCM exists anywhere in the job; one lacx_block_info per block comes back.
 * Verdict of a block (code, the decoder's codes, lacx_block_fault_text): 0 the block parses, 1 block header, 2 channel
 *   header, 3 residual, 4 padding, 6 trailing bytes, 8 not reached (version 2, behind a block that does not parse), 9 a
 *   zigzag value of 2^30 or more, 10 the file does not hold the block.  Within one token a parse fault wins over
 *   anything else, as in the decoder.  Codes 5 (sample overflow) and 7 (sample outside the bit depth) need reconstructed
 *   samples: inspection NEVER reports them, and a block that fails with one of them in a decode inspects as 0 (or, for
 *   code 5, as whatever the parse finds behind the sample at which the decoder stopped).  lacx_decoder_check_* and
 *   lacx_decoder_stats_* are the tools for those codes.
 * lacx_channel_info, per channel block (160 bytes):
 *   predictor_type (0 fixed, 1 FIR, 2 LPC), order, partition_order; coef: the LPC coefficients as stored, zero beyond order.
 *   Bit classes, which sum to bits: header_bits (type, order, 16 per coefficient, control byte, 7 per partition),
 *   tag_bits (2 per tagged token), unary_bits (ones plus terminator, of residual codes and of run-length codes),
 *   remainder_bits (k-bit remainders, the run code's 2 bits, bin sign bits), escape_bits (32 per escape), pad_bits.
 *   Sample classes, which sum to the block's frames: rice_samples (bare codes of modes 0 and 3, tag 00 of mode 1, tag 11 of
 *   mode 2), run_samples (in run_tokens runs), escape_samples, bin_samples[t] (tags 00, 01, 10 of mode 2).
 *   mode_parts[m] / mode_samples[m]: partitions and samples by residual mode (0 adaptive Rice, 1 zero-run, 2 bin, 3 static).
 *   k_min / k_max: the parameter in force at the Rice-coded residuals (255 and 0 when there are none); unary_max: the
 *   longest quotient of any unary part; max_u / sum_u: over the zigzag magnitudes of all samples.
 * lacx_block_info, 336 bytes: frames and bytes from the block table (version 2 has no sizes: bytes is what the walk
 *   found); code; ms: 1 when the block is mid/side, by flag or by stream mode; channels; ch[1] is all zero for mono.
 *   8 * bytes == 8 * (per-block flag present) + ch[0].bits + ch[1].bits.  A block that does not parse or is missing
 *   keeps frames, bytes and code (bytes 0 for version 2); every other field is 0.
 * lacx_stream_report, 456 bytes, per item, made on the host from the rows by lacx_inspect_combine: integers only (bits
 *   per sample and shares are the caller's to derive).  Totals run over the blocks that parse: payload_bytes is the sum
 *   of their bytes, so 8 * payload_bytes == flag_bits + bits.  fixed_blocks[o], fir_blocks, lpc_blocks[o] (o = 1..32,
 *   [0] unused), partition_order_blocks[p] count channel blocks.  sum_u is a 128-bit pair.  k_min 255 / k_max 0 with no
 *   Rice-coded residual.
 * lacx_decoder_inspect_batch_device: lenient exactly like lacx_decoder_stats_batch_device -- versions 3 and 2, truncated
 *   files (their missing blocks get code 10), LACX_OK whenever the container is accepted; a refused container keeps the
 *   strict code and text and gets a zeroed report and no rows.  flags: 0 or LACX_INSPECT_PARTITIONS (anything else
 *   LACX_E_INVALID).  out_reports: nullable array of n.  The return code, "stream i: " prefixes, lacx_decoder_item_error,
 *   n = 0, null arrays, device-less behaviour (host-side outcomes filled, then LACX_E_DEVICE) and `stream` as
 *   lacx_decoder_stats_batch_device.  Inspection may alternate with every other job form on one decoder.
 * lacx_decoder_item_block_info: the rows of item i of the decoder's last inspection call, valid until its next call;
 *   LACX_E_INVALID outside that call.
 * lacx_decoder_item_partitions: with LACX_INSPECT_PARTITIONS, channel block `channel` of block `block` of item i:
 *   mode_k[p] = (mode << 5) | k of partition p's table entry, as lacx_channel_plan.part_mode_k, part_bits[p] the bits of
 *   its tokens; count = the partitions (0 for a block that does not parse).  LACX_E_INVALID when the last call did not ask
 *   for them or the indices are outside it.  Without the flag the partition buffer is neither allocated nor copied.
 * lacx_inspect_combine: host only, no device: the totals of `count` rows (rows may be null when count is 0), public so
 *   that a caller can total a sub-range.  info: the stream (format fields and head_bytes from it), or null: those are 0. */
#define LACX_INSPECT_PARTITIONS 1u
typedef struct lacx_channel_info { /* 160 bytes */
    uint8_t predictor_type, order, partition_order, k_min, k_max, reserved[3];
    int16_t coef[32];
    uint32_t bits, header_bits, tag_bits, unary_bits, remainder_bits, escape_bits, pad_bits;
    uint32_t rice_samples, run_tokens, run_samples, escape_samples, bin_samples[3];
    uint16_t mode_parts[4], mode_samples[4];
    uint32_t unary_max, max_u;
    uint64_t sum_u;
} lacx_channel_info;
typedef struct lacx_block_info {   /* 336 bytes */
    uint32_t frames, bytes, code;
    uint8_t ms, channels, reserved[2];
    lacx_channel_info ch[2];
} lacx_block_info;
typedef struct lacx_stream_report { /* 456 bytes */
    uint64_t frames, head_bytes, payload_bytes;
    uint32_t sample_rate;
    uint8_t channels, bit_depth, stereo_mode, version;
    uint32_t blocks, lost_blocks, ms_blocks, channel_blocks;
    uint32_t fixed_blocks[5], fir_blocks, lpc_blocks[33], partition_order_blocks[9];
    uint64_t mode_parts[4], mode_samples[4];
    uint64_t bits, flag_bits, header_bits, tag_bits, unary_bits, remainder_bits, escape_bits, pad_bits;
    uint64_t rice_samples, run_tokens, run_samples, escape_samples, bin_samples[3];
    uint64_t sum_u_lo, sum_u_hi;
    uint32_t max_u, unary_max;
    uint8_t k_min, k_max, reserved[6];
} lacx_stream_report;
int lacx_decoder_inspect_batch_device(lacx_decoder* dec, const lacx_span* lacs, uint32_t n, uint32_t flags, void* stream, int* item_rc,
                                      lacx_stream_report* out_reports, float* device_ms);
int lacx_decoder_item_block_info(const lacx_decoder* dec, uint32_t i, const lacx_block_info** rows, uint32_t* count);
int lacx_decoder_item_partitions(const lacx_decoder* dec, uint32_t i, uint32_t block, uint32_t channel, const uint8_t** mode_k,
                                 const uint32_t** part_bits, uint32_t* count);
int lacx_inspect_combine(const lacx_block_info* rows, uint32_t count, const lacx_stream_info* info, lacx_stream_report* out);
/* Diagnostic.  With LACX_INSPECT_GUARD=1 in the environment (read per call) an inspection job's tables buffer is made
 * larger than its plan asks by a guard -- 4096 bytes, and without LACX_INSPECT_PARTITIONS also the bytes the partition
 * entries of the job's blocks would take -- which is filled with a pattern on the device before the kernels run and read
 * back behind them: *guarded = its bytes in the decoder's last inspection call (0: no guard), *changed = those that no
 * longer hold the pattern.  A call that changed any fails as a whole with LACX_E_DEVICE. */
int lacx_decoder_inspect_guard(const lacx_decoder* dec, uint64_t* guarded, uint64_t* changed);

/* Runs: WHERE a stream is silent, clips or holds one value.  The statistics say whether and how often, one row per block;
 * these entry points give the intervals: "the pause runs from frame 1 234 567 to 1 301 222", "right clips for 37
 * consecutive samples at 0:41.3", "one value was held for 2 000 samples here".  The minimum-length filter runs on the device
 * where the samples lie (ordinary music crosses any small threshold at every zero crossing); what comes back is the runs
 * and a small row per tile of 1024 frames, not the PCM.  Everything is an exact integer; there is no tolerance anywhere.
 * A detector is {kind, channel, level, min_frames}.  channel: 0 (left), 1 (right) or LACX_RUN_ALL -- every channel of the
 *   item must satisfy the predicate in that frame; a detector on channel 1 finds nothing in a mono item.  min_frames >= 1.
 *   Samples x are the final left / right integers of the item's bit depth b, `level` is in those units (so a mixed batch
 *   carries its detectors per item: lacx_run_query says which of the call's detectors are the item's, like
 *   lacx_edit_output's segments; at most LACX_MAX_DETECTORS).  The frame predicate P(f):
 *   LACX_RUN_QUIET: -level <= x <= level for every selected channel (level 0: digital silence);
 *   LACX_RUN_PEAK:  x >= level or x <= -level - 1 for every selected channel (level 2^(b-1)-1: the statistics' full_scale);
 *   LACX_RUN_FLAT:  f >= 1, frame f - 1 is counted, and x[f] == x[f-1] for every selected channel; level must be 0.  A
 *                   stretch of N equal samples is N - 1 flagged frames.
 *   A frame of a lost or missing block satisfies no predicate and the first frame behind such a block is never FLAT: a
 *   lost block splits a run.
 * A run is a maximal interval [start, start + frames) of consecutive frames with P true, reported if and only if
 *   frames >= min_frames.  Per (item, detector): the complete list of runs ascending by start (lacx_decoder_item_runs;
 *   never truncated) and the totals lacx_run_totals: runs, frames (in runs), longest and longest_start (the lowest start
 *   among equals).
 * lacx_runs_result, per item: frames, lost_frames, blocks, lost_blocks as a salvage reports them; flags: LACX_RUNS_RERUN --
 *   the interior runs outgrew the list the plan reserves (min((frames + 1) / (min_frames + 1), R) entries per detector,
 *   R = 8192, or LACX_RUNS_LIST_CAP in the environment at lacx_decoder_create) and the kernel ran once more with the exact
 *   capacities its counters gave; det[k]: the totals of the item's k-th detector.
 * lacx_decoder_runs_batch_device: lenient exactly like lacx_decoder_stats_batch_device -- versions 3 and 2, truncated
 *   files, LACX_OK whenever the container is accepted; a refused container keeps the strict code and text and gets a
 *   zeroed result.  out: nullable array of n.
 * lacx_decoder_runs_pcm_batch_device: device-resident source PCM in any LACX_PCM_* layout; the per-item host checks, the
 *   device-found validation texts and the bounds are those of lacx_decoder_stats_pcm_batch_device.  A failed item gets a
 *   zeroed result and no runs.
 * Host checks of an item's detectors, each LACX_E_INVALID with its text in lacx_decoder_item_error: "detectors outside
 *   the call's array", "too many detectors", "item has no detectors", "unknown detector kind", "unknown detector
 *   channel", "detector needs min_frames >= 1", "flat detector takes no level".  A null detector array or ndets == 0 fails
 *   the whole call.
 * lacx_decoder_item_runs: the runs of detector `detector` of item `item` of the decoder's last runs call, valid until its
 *   next call; LACX_E_INVALID outside that call.
 * Everything else as lacx_decoder_decode_batch_device: the return code, "stream i: " prefixes, lacx_decoder_item_error,
 * n = 0, device-less behaviour (host-side outcomes filled, then LACX_E_DEVICE) and `stream`.
 * Time (scripts/runs_bench.py, profiles/runs_bench.txt): on 48 four-minute stereo streams as one job with three
 * detectors 39.6 ms of kernels, 2.6 ms below the stats job; k_runs alone 3.4 ms for 4.06 GB of PCM. */
#define LACX_RUN_QUIET 0u
#define LACX_RUN_PEAK  1u
#define LACX_RUN_FLAT  2u
#define LACX_RUN_ALL   255u
#define LACX_MAX_DETECTORS 8u            /* per item */
typedef struct lacx_run_detector { /* 16 bytes */
    uint8_t kind, channel, reserved[2];
    uint32_t level;
    uint64_t min_frames;
} lacx_run_detector;
typedef struct lacx_run_query {    /* 8 bytes: detectors first_detector .. first_detector + detectors - 1 of the call's array */
    uint32_t first_detector, detectors;
} lacx_run_query;
typedef struct lacx_run {          /* 16 bytes */
    uint64_t start, frames;
} lacx_run;
typedef struct lacx_run_totals {   /* 32 bytes */
    uint64_t runs, frames, longest, longest_start;
} lacx_run_totals;
typedef struct lacx_runs_result {  /* 296 bytes, per item */
    uint64_t frames, lost_frames;
    uint32_t sample_rate, blocks, lost_blocks, flags;
    uint8_t channels, bit_depth, detectors, reserved[5];
    lacx_run_totals det[LACX_MAX_DETECTORS];
} lacx_runs_result;
#define LACX_RUNS_RERUN 1u
int lacx_decoder_runs_batch_device(lacx_decoder* dec, const lacx_span* lacs, const lacx_run_query* queries, uint32_t n,
                                   const lacx_run_detector* dets, uint32_t ndets, void* stream, int* item_rc, lacx_runs_result* out,
                                   float* device_ms);
int lacx_decoder_runs_pcm_batch_device(lacx_decoder* dec, const lacx_digest_source* src, const lacx_run_query* queries, uint32_t n,
                                       const lacx_run_detector* dets, uint32_t ndets, void* stream, int* item_rc, lacx_runs_result* out,
                                       float* device_ms);
int lacx_decoder_item_runs(const lacx_decoder* dec, uint32_t item, uint32_t detector, const lacx_run** runs, uint64_t* count);

/* Loudness: ITU-R BS.1770-4 / EBU R 128 integrated, momentary and short-term loudness and the loudness range (EBU Tech
 * 3342), made on the device where the samples lie.  Stats gives peak and plain energy; loudness is the energy behind the
 * K-weighting filter, in 400 ms gating blocks, behind two gates.  Nothing is ever applied to the audio: gain is not
 * lossless, and these entry points only measure.  Out of scope: more than two channels, a lenient form (true peak: the next section).
 * Definition (csrc/loudness_core.h states every operation and its order):
 *   Input: the final left / right integer samples of the item's bit depth b, converted to double (exact); the scaling by
 *   2^-(b-1) is applied to energies on the host as the exact factor 4^-(b-1).
 *   K-weighting per sample rate fs, the coefficients made on the host in double from the analog prototype: a shelf
 *   (f0 = 1681.974450955533, G = 3.999843853973347 dB, Q = 0.7071752369554196; K = tan(pi f0 / fs), Vh = 10^(G/20),
 *   Vb = Vh^0.4996667741545416, a0 = 1 + K/Q + K^2; b = [(Vh + Vb K/Q + K^2)/a0, 2(K^2 - Vh)/a0, (Vh - Vb K/Q + K^2)/a0],
 *   a = [1, 2(K^2 - 1)/a0, (1 - K/Q + K^2)/a0]) feeding a high-pass (f0 = 38.13547087602444, Q = 0.5003270373238773,
 *   d = 1 + K/Q + K^2; b = [1, -2, 1], a = [1, 2(K^2 - 1)/d, (1 - K/Q + K^2)/d]); at 48 kHz the BS.1770 table to 9e-16.
 *   Each biquad in transposed direct form II (y = b0 x + s1; s1 = b1 x - a1 y + s2; s2 = b2 x - a2 y), four state words
 *   per channel, zero at frame 0.
 *   The stream is cut into chunks of 256 frames counted from the item's frame 0: every chunk is filtered from zero state
 *   (final state f[c]); s[0] = 0, s[c+1] = A s[c] + f[c] with A the 4x4 map of 256 zero-input steps; every chunk is
 *   filtered again from s[c] and the squares of the output are summed in frame order.  A sub-block is fs/10 frames; a
 *   chunk touches at most two and leaves one partial sum for each; a row entry is the sum, in chunk order, of the
 *   partials that fall into its sub-block.  An item has S = floor(frames / (fs/10)) rows; the frames behind the last
 *   complete sub-block are not filtered.  No floating-point atomics, every multiply-add that is fused is an fma: a row is
 *   the same bits from run to run, in any batch and at any place in a job.
 * lacx_loudness_row: energy[c] = the sum of squares of channel c's K-weighted samples over one sub-block (integer-scaled
 *   samples, so up to fs/10 * 4^(b-1) * ~2.5); energy[1] = 0 for mono.
 * lacx_loudness, per item or per album, made on the host from the rows by lacx_loudness_combine.  With e[s] = energy[0]
 *   (+ energy[1]) and n = fs/10: gating block j = 0 .. S-4: z_j = (e[j] + .. + e[j+3]) / (4 n 4^(b-1)), l_j = -0.691 +
 *   10 log10 z_j.  Mono is one channel of weight 1: a mono file reads 3.01 LU below its dual-mono form, as the standard
 *   says.  frames: the frames the rows cover (subblocks * n; summed over the sets); subblocks: S; gating_blocks;
 *   above_absolute: blocks with l_j > -70; above_relative: those also above relative_gate_lufs = the loudness of the mean
 *   z of the former - 10; integrated_lufs: the loudness of the mean z of the latter; momentary_max_lufs: max l_j;
 *   shortterm_max_lufs: the maximum over windows of 30 sub-blocks at every sub-block hop (-INFINITY when S < 30);
 *   range_lu: short-term windows at a hop of 10 sub-blocks, absolute gate -70, relative gate 20 LU below the loudness of
 *   the mean power of the absolutely gated ones, ascending sort, P95 - P10 with index floor((m-1) p + 0.5); 0 when
 *   nothing passes.  flags: LACX_LOUDNESS_TOO_SHORT (no gating block, S < 4): every level is -INFINITY, range 0;
 *   LACX_LOUDNESS_SILENT: no block above the absolute gate, integrated_lufs and relative_gate_lufs are -INFINITY.
 * lacx_decoder_loudness_batch_device: strict, exactly like lacx_decoder_digest_batch_device -- versions 3 and 2; the
 *   decode, the in-place mid/side inverse, then k_loud_states, k_loud_carry, k_loud_energy, k_loud_rows on the job's
 *   stream.  An item that does not parse or decode keeps the decode's own code and message, gets a zeroed result and no
 *   rows, and does not cost the other items.  out: nullable array of n.
 * lacx_decoder_loudness_pcm_batch_device: device-resident source PCM in any LACX_PCM_* layout; the per-item host checks,
 *   the device-found validation texts (every frame is validated, also those behind the last sub-block) and the bounds are
 *   those of lacx_decoder_digest_pcm_batch_device.  A failed item gets a zeroed result and no rows.
 * lacx_decoder_item_loudness_rows: the rows of item i of the decoder's last loudness call, valid until its next call;
 *   LACX_E_INVALID outside that call.
 * lacx_loudness_combine: host only, no device.  One set gives exactly the per-item totals the batch calls return (they
 *   use it).  Several sets give album loudness: gating blocks and short-term windows never straddle sets, gates and
 *   means run over the union, z is normalised per set by its own rate and depth, maxima are over all sets; sample_rate,
 *   channels and bit_depth are the first set's.  LACX_E_INVALID: null out, nsets == 0, a null array, null rows with a
 *   count > 0, channels not 1 or 2, bit depth not 16 or 24, a sample rate that is none of the four.
 * Everything else as lacx_decoder_digest_batch_device: the return code, "stream i: " prefixes, lacx_decoder_item_error,
 * n = 0, null arrays, device-less behaviour (host-side outcomes filled, then LACX_E_DEVICE) and `stream`.
 * Scratch: 32 bytes of state and 16 of partial sums per chunk and channel, about 5 % of the int32 PCM.
 * Time (scripts/loudness_bench.py, profiles/loudness_bench.txt): on 48 four-minute stereo streams as one job 30.5
 * ms of kernels, 6.2 ms above the statistics' job, and 58 ms of wall against 2.3 s for decode, copy and lfilter on the host;
 * k_loud_states and k_loud_energy 4.4 and 4.5 ms for 4.06 GB of PCM each, k_loud_carry 3.4 ms (8.7 ms for one 10-minute stream). */
typedef struct lacx_loudness_row { /* 16 bytes; energy[1] = 0 for mono */
    double energy[2];
} lacx_loudness_row;
typedef struct lacx_loudness {     /* 72 bytes */
    uint64_t frames;
    uint32_t sample_rate;
    uint8_t channels, bit_depth, flags, reserved;
    uint32_t subblocks, gating_blocks, above_absolute, above_relative;
    double integrated_lufs, relative_gate_lufs, momentary_max_lufs, shortterm_max_lufs, range_lu;
} lacx_loudness;
#define LACX_LOUDNESS_TOO_SHORT 1u
#define LACX_LOUDNESS_SILENT 2u
int lacx_decoder_loudness_batch_device(lacx_decoder* dec, const lacx_span* lacs, uint32_t n, void* stream, int* item_rc,
                                       lacx_loudness* out, float* device_ms);
int lacx_decoder_loudness_pcm_batch_device(lacx_decoder* dec, const lacx_digest_source* src, uint32_t n, void* stream,
                                           int* item_rc, lacx_loudness* out, float* device_ms);
int lacx_decoder_item_loudness_rows(const lacx_decoder* dec, uint32_t i, const lacx_loudness_row** rows, uint32_t* count);
int lacx_loudness_combine(const lacx_loudness_row* const* rows, const uint32_t* counts, const uint8_t* channels,
                          const uint8_t* bit_depths, const uint32_t* sample_rates, uint32_t nsets, lacx_loudness* out);

/* True peak: ITU-R BS.1770-4 Annex 2 / EBU R 128, the maximum of the 4x oversampled signal, made on the device where the
 * samples lie.  Loudness gives the gain a levelling tool writes into a tag; the true peak is the other half of the pair: how
 * much of that gain can be applied before the signal clips behind a D/A converter or a lossy encoder.  The largest sample
 * (stats) can miss a peak between samples by 3 dB and more.  Nothing is ever applied to the audio.  Out of scope: a lenient
 * form, more than two channels, applying gain.
 * Definition (csrc/truepeak_core.h is its only statement in code).  The Annex 2 filter is exact in integers:
 *   Coefficients c[p][k], phase p = 0..3, tap k = 0..11, the BS.1770-4 Annex 2 table times 8192 -- every entry of the
 *   table is a whole multiple of 2^-13:
 *     c[0] = {   14,   90, -161,  272,  -487, 1125, 7964,  -838,  390, -218,  122,  -68 }
 *     c[1] = { -239,  240, -424,  730, -1364, 3810, 6388, -1641,  832, -477,  271, -155 }
 *     c[2] = c[1] reversed, c[3] = c[0] reversed
 *   (sums 8205 / 7971 / 7971 / 8205, sums of magnitudes 11749 / 16571 / 16571 / 11749).
 *   For a channel x of an item of bit depth b, x[n] = 0 outside [0, frames): y[4n + p] = sum over k of c[p][k] x[n - k] for
 *   n = 0 .. frames + 10 -- the full convolution: the filter delays by about 5.9 frames, and the last peak lies in the 11
 *   flush frames behind the end.  y is an exact integer, |y| <= 16571 * 2^(b-1), and y / 8192 is the oversampled signal in
 *   sample units.  All four phases are used at every sample rate (the standard's lower factors at higher rates are a
 *   minimum; more phases never read lower).  Integer maxima do not depend on the order of evaluation: device, CPU twin and a
 *   numpy restatement agree bit for bit, and a row is the same bits in any batch.
 * lacx_truepeak_row: one per segment of 16384 frames counted from the item's frame 0 (the blocks of every stream the
 *   encoder writes, but the grid does not read the block table); output n belongs to segment min(n, frames - 1) / 16384, so
 *   the flush frames go to the last row.  Per channel: peak = max |y| over the row's outputs; pos = 4 (n - 16384 row) + p of
 *   the lowest output index that attains it, 0 when peak is 0 (pos < 4 * 16395); sample_peak = max |x| over the row's
 *   frames (-2^23 gives 8388608).  A mono item's second channel is all zero.
 * lacx_truepeak, made on the host from the rows by lacx_truepeak_combine.  One set: frames, sample_rate, channels,
 *   bit_depth and rows as given; per channel ch[c]: peak, position = 4n + p in the stream (the lowest on ties), sample_peak
 *   and sample_peak_row, the first row that holds it (a row carries no frame for it); peak_channel: the channel with the
 *   larger peak (0 on ties); true_peak = that peak / (8192 * 2^(b-1)), exact, the linear value a REPLAYGAIN_*_PEAK tag
 *   holds; true_peak_dbtp = 20 log10 of it; sample_peak_dbfs = 20 log10 (largest sample_peak / 2^(b-1)); both -INFINITY for
 *   all-zero audio.  flags: LACX_TRUEPEAK_OVER: a peak exceeds 8192 * 2^(b-1), an inter-sample over;
 *   LACX_TRUEPEAK_SAMPLE_FULL: a sample sits at full scale (|x| >= 2^(b-1) - 1).  set: 0.
 *   Several sets, an album: the totals of the set whose peak is largest -- depths are compared exactly, a 16-bit peak
 *   shifted by 8; the lowest index on ties -- with set its index; frames and rows are summed over the sets, flags are
 *   those of all sets, and sample_peak_dbfs is the largest of all sets.
 * lacx_decoder_truepeak_batch_device: strict, exactly like lacx_decoder_digest_batch_device -- versions 3 and 2; the
 *   decode, the in-place mid/side inverse, then k_truepeak (one launch) on the job's stream.  An item that does not parse or
 *   decode keeps the decode's own code and message, gets a zeroed result and no rows, and does not cost the other items.
 *   out: nullable array of n.
 * lacx_decoder_truepeak_pcm_batch_device: device-resident source PCM in any LACX_PCM_* layout; the per-item host checks,
 *   the device-found validation texts and the bounds are those of lacx_decoder_digest_pcm_batch_device.  A failed item gets a
 *   zeroed result and no rows.
 * lacx_decoder_item_truepeak_rows: the rows of item i of the decoder's last true-peak call, valid until its next call;
 *   LACX_E_INVALID outside that call.
 * lacx_truepeak_combine: host only, no device.  One set gives exactly the per-item totals the batch calls return (they use
 *   it).  LACX_E_INVALID: null out, nsets == 0, a null array, null rows with a count > 0, channels not 1 or 2, bit depth not
 *   16 or 24, a sample rate that is none of the four, a count that is not ceil(frames / 16384).
 * Everything else as lacx_decoder_loudness_batch_device.  No scratch: 32 bytes per 16384 frames inside the job's tables.
 * Time (scripts/truepeak_bench.py, profiles/truepeak_bench.txt): on 48 four-minute stereo 16-bit streams as one job
 * 22.3 ms of kernels, 2.3 ms below the statistics' job, and 46 ms of wall against 861 ms for decode plus a float64 conv1d
 * and amax in torch on the same device; k_truepeak alone 4.0 ms for 4.06 GB of PCM (1.3 ms for 1.02 GB at 24 bit). */
typedef struct lacx_truepeak_row { /* 32 bytes */
    uint64_t peak[2];
    uint32_t pos[2];
    uint32_t sample_peak[2];
} lacx_truepeak_row;
typedef struct lacx_truepeak_channel { /* 24 bytes */
    uint64_t peak, position;
    uint32_t sample_peak, sample_peak_row;
} lacx_truepeak_channel;
typedef struct lacx_truepeak {     /* 96 bytes */
    uint64_t frames;
    uint32_t sample_rate;
    uint8_t channels, bit_depth, flags, peak_channel;
    uint32_t rows, set;
    lacx_truepeak_channel ch[2];
    double true_peak, true_peak_dbtp, sample_peak_dbfs;
} lacx_truepeak;
#define LACX_TRUEPEAK_OVER 1u
#define LACX_TRUEPEAK_SAMPLE_FULL 2u
int lacx_decoder_truepeak_batch_device(lacx_decoder* dec, const lacx_span* lacs, uint32_t n, void* stream, int* item_rc,
                                       lacx_truepeak* out, float* device_ms);
int lacx_decoder_truepeak_pcm_batch_device(lacx_decoder* dec, const lacx_digest_source* src, uint32_t n, void* stream,
                                           int* item_rc, lacx_truepeak* out, float* device_ms);
int lacx_decoder_item_truepeak_rows(const lacx_decoder* dec, uint32_t i, const lacx_truepeak_row** rows, uint32_t* count);
int lacx_truepeak_combine(const lacx_truepeak_row* const* rows, const uint32_t* counts, const uint8_t* channels,
                          const uint8_t* bit_depths, const uint64_t* frames, const uint32_t* sample_rates, uint32_t nsets,
                          lacx_truepeak* out);

/* Spectrum: the long-term power spectrum of a stream in 64 uniform bands and its bandwidth, made on the device where the
 * samples lie.  Everything else here looks at the time domain; the question an archive of lossless audio gets asked most
 * -- is this really what it claims to be? -- is read off the spectrum: a "lossless" file made from a lossy one has a
 * brick-wall cutoff at 16 - 20 kHz, a 96 kHz file upsampled from 44.1 kHz has nothing above 22.05 kHz.  It only measures.
 * Out of scope: a lenient form, more than two channels, windows other than Hann, hops other than N / 2, per-window output
 * (a spectrogram), phase.
 * Definition (csrc/spectrum_core.h is its only statement in code).
 *   window: the window length N, one of 256, 512, 1024, 2048, 4096, one value per call (the binding's default is 2048);
 *   the hop is H = N / 2.  Window k of an item covers frames [k H, k H + N), k = 0 .. ceil(frames / H) - 1; frames at or
 *   behind the item's end are zeros; an item without frames has no windows and no rows.
 *   w[n] = 0.5 - 0.5 cos(2 pi n / N), the periodic Hann window.  The host makes the window and the twiddles (cos, -sin of
 *   2 pi k / N), every entry evaluated in long double and rounded once to double; the device never evaluates a sine or
 *   cosine, device and CPU twin read the same tables.
 *   A sample enters as (double)x, exact; w[n] x is one rounding.  Stereo items take both channels through one complex
 *   transform, z = w l + i w r, separated by L_k = (Z_k + conj Z_{N-k}) / 2, R_k = (Z_k - conj Z_{N-k}) / 2i; mono runs
 *   the same transform with a zero imaginary part.  The transform is a radix-2 decimation-in-frequency FFT whose every
 *   operation is fixed in the core (a' = a + b; d = a - b; b' = (fma(d.re, c, -(d.im s)), fma(d.re, s, d.im c)) with the
 *   twiddle (c, s)); |X|^2 = fma(x.re, x.re, x.im x.im).  The one-sided power of bin k is c_k |X_k|^2, c_0 = c_{N/2} = 1,
 *   c_k = 2 otherwise.  64 uniform bands: bin k < N / 2 belongs to band k / (N / 128), the Nyquist bin to band 63, summed in
 *   ascending bin order; the bands of a window add up to N sum (w[n] x[n])^2 up to rounding (Parseval).
 * lacx_spectrum_row: one per segment of 16384 frames counted from the item's frame 0 (true peak's row grid): per channel and
 *   band the sum, in window order, of the band powers of the windows whose FIRST frame lies in the segment: 16384 / H
 *   windows per full row.  1024 bytes per 16384 frames, about 1.8 MB for ten minutes.  A mono item's second channel is all
 *   zero; digital silence is +0.0 in every byte.  There are no floating-point atomics and nothing but the written fused
 *   multiply-adds is fused (the kernel, the totals and the CPU twin are compiled with -ffp-contract=off): a row is the same
 *   bits on the device and on the twin, from run to run, in any batch and at any place in a job.
 * lacx_spectrum, made on the host from the rows by lacx_spectrum_combine: frames, sample_rate, channels, bit_depth, rows,
 *   window as given, windows = ceil(frames / H), floor_db as given; per channel and band, with P the rows' powers added in
 *   row order, level_db = 10 log10(P / (windows (3 N^2 / 8) 2^(2b-3))), b the bit depth: the band's mean square relative to
 *   a full-scale sine (sum w^2 = 3 N / 8 exactly), so that a full-scale sine on an exact bin 2 .. N / 2 - 2 reads 0.00 dBFS
 *   summed over the bands it falls into (the zero-padded last windows of a short item read lower); -INFINITY for a zero
 *   band.  bandwidth_hz: the upper edge (band + 1) sample_rate / 128 of the highest band whose level is at least floor_db, 0
 *   when no band is; TPDF dither at 16 bits puts about -111 dBFS into each band, so at the bindings' default of -100 dither
 *   alone does not count as signal.  peak_band: the lowest band with the largest power (0 for silence).
 * lacx_decoder_spectrum_batch_device: strict, exactly like lacx_decoder_digest_batch_device -- versions 3 and 2; the
 *   decode, the in-place mid/side inverse, then k_spectrum (one launch) on the job's stream.  An item that does not parse or
 *   decode keeps the decode's own code and message, gets a zeroed result and no rows, and does not cost the other items.
 *   A window that is none of the five values fails the call with LACX_E_INVALID "unsupported spectrum window: W" and
 *   launches nothing.  out: nullable array of n.
 * lacx_decoder_spectrum_pcm_batch_device: device-resident source PCM in any LACX_PCM_* layout; the per-item host checks,
 *   the device-found validation texts and the bounds are those of lacx_decoder_digest_pcm_batch_device.  A failed item gets a
 *   zeroed result and no rows.
 * lacx_decoder_item_spectrum_rows: the rows of item i of the decoder's last spectrum call, valid until its next call;
 *   LACX_E_INVALID outside that call.
 * lacx_spectrum_combine: host only, no device; one item's rows give exactly the totals the batch calls return (they use
 *   it).  LACX_E_INVALID: a null argument (null rows with a count > 0), channels not 1 or 2, bit depth not 16 or 24, a
 *   sample rate that is none of the four, an unsupported window, a count that is not ceil(frames / 16384).
 * Everything else as lacx_decoder_truepeak_batch_device.  No scratch: the rows lie inside the job's tables.
 * Time (scripts/spectrum_bench.py, profiles/spectrum_bench.txt): on 48 four-minute stereo 16-bit streams as one job
 * 33.0 ms of kernels and 66.7 ms of wall at N = 2048 (30.7 / 65.4 ms at N = 256) against 146.7 ms (145.1 ms) for decode plus
 * torch.stft in float64 and the band sums on the same device; k_spectrum alone 14.4 ms (12.4 ms) for 4.06 GB of PCM. */
typedef struct lacx_spectrum_row { /* 1024 bytes */
    double power[2][64];
} lacx_spectrum_row;
typedef struct lacx_spectrum {     /* 1080 bytes */
    uint64_t frames, windows;
    uint32_t sample_rate, window, rows;
    uint8_t channels, bit_depth, peak_band[2];
    double floor_db;
    double bandwidth_hz[2];
    double level_db[2][64];
} lacx_spectrum;
int lacx_decoder_spectrum_batch_device(lacx_decoder* dec, const lacx_span* lacs, uint32_t n, uint32_t window, double floor_db,
                                       void* stream, int* item_rc, lacx_spectrum* out, float* device_ms);
int lacx_decoder_spectrum_pcm_batch_device(lacx_decoder* dec, const lacx_digest_source* src, uint32_t n, uint32_t window,
                                           double floor_db, void* stream, int* item_rc, lacx_spectrum* out, float* device_ms);
int lacx_decoder_item_spectrum_rows(const lacx_decoder* dec, uint32_t i, const lacx_spectrum_row** rows, uint32_t* count);
int lacx_spectrum_combine(const lacx_spectrum_row* rows, uint32_t count, uint8_t channels, uint8_t bit_depth, uint64_t frames,
                          uint32_t sample_rate, uint32_t window, double floor_db, lacx_spectrum* out);

/* Rip checksums: the two AccurateRip track checksums of a disc of CD audio (2 channels, 16 bit, 44100 Hz) at every read
 * offset within a radius, made on the device where the samples lie.  Ripping tools compare these sums with a database of
 * other people's rips of the same disc; a pressing whose audio is shifted by a few hundred samples shows at another offset.
 * The v1 sum is linear and follows from prefix sums at every offset; the v2 sum adds the high half of a 64-bit product and
 * has no such shortcut, so CPU tools give it at offset 0 only.  Here every (multiplier, offset) pair is one multiply on the
 * device.  Out of scope: the database lookup, cue sheets (track lengths come in as frames), the CTDB CRC, data tracks, a
 * lenient form, anything that is not 2 channels / 16 bit / 44100 Hz.
 * Definition (csrc/accuraterip_core.h is its only statement in code).  The formulas are the widely published
 * ones, written down without access to the database.
 *   Disc: an ordered list of S >= 1 whole sources, concatenated to D frames, and T track lengths n_0 .. n_(T-1) in frames, 1
 *   <= T <= 99, every n_t >= 1, their sum D; track t starts at disc frame s_t = n_0 + .. + n_(t-1).  Tracks and sources are
 *   independent partitions of the disc: one image with a cue sheet is S = 1, T > 1; one file per track is S = T.  Frame j is
 *   the word w[j] = (uint16)left[j] | (uint16)right[j] << 16; x(j) = w[j] for 0 <= j < D and 0 elsewhere.
 *   Sums: LACX_AR_FIRST / LACX_AR_LAST say that track 0 is the disc's first track / track T-1 its last.  lo_t = 2940 if t =
 *   0 and FIRST, else 1; hi_t = n_t - 2940 if t = T-1 and LAST, else n_t.  For 0 <= radius <= 2939, every offset o in
 *   [-radius, radius] and every track, with the multiplier m a uint32 and p = (uint64)m * x(s_t + o + m - 1):
 *     v1[t][o]   = sum over m = lo_t .. hi_t of lo32(p)              mod 2^32
 *     v2[t][o]   = sum over m = lo_t .. hi_t of lo32(p) + hi32(p)    mod 2^32
 *     s450[t][o] = sum over k = 1 .. 588 of lo32(k * x(s_t + o + 450 * 588 + k - 1))   mod 2^32, where n_t >= 451 * 588;
 *                  elsewhere 0 and the track carries LACX_AR_TRACK_NO_S450.
 *   An empty range (hi_t < lo_t) gives 0 and LACX_AR_TRACK_SHORT.  With both flags no sum reads outside [0, D); a partial
 *   disc reads zeros there.  Sums mod 2^32 do not depend on the order of evaluation: device, CPU twin and a numpy
 *   restatement agree bit for bit, in any batch.
 *   Ids (host only), given when every n_t is a multiple of 588 and both flags are set, else all 0 and LACX_AR_NO_IDS:
 *   lba_t = lba0 + s_t / 588, leadout = lba0 + D / 588; id1 = (sum of lba_t + leadout) mod 2^32; id2 = (sum of max(lba_t, 1)
 *   (t + 1) + leadout (T + 1)) mod 2^32; cddb = ((sum of digitsum((lba_t + 150) / 75)) mod 255) << 24 | ((leadout + 150) / 75
 *   - (lba_0 + 150) / 75) << 8 | T, integer divisions.
 * lacx_ar_disc: the disc's sources [first_source, first_source + sources) of the call's source array and its track lengths
 *   [first_track, first_track + tracks) of the call's track_frames array; tracks = 0: one track per source, its frames.
 * lacx_decoder_accuraterip_batch_device: strict, like lacx_decoder_digest_batch_device -- the decode, the in-place mid/side
 *   inverse, then k_accuraterip (one launch) on `stream`.  A disc's streams lie side by side in the decoder's buffers; a
 *   track boundary need not be a stream boundary, and an offset reaches into the neighbouring stream.  Refused per disc on
 *   the host before any device work, each LACX_E_INVALID: "disc has no sources", "sources outside the call's array",
 *   "tracks outside the call's array", "more than 99 tracks", "track T is empty", "track lengths do not sum to the disc's
 *   frames (A, B)", "radius above 2939", "unknown flags", "source k: not CD audio (C channels, B bit, R Hz)", "source k:
 *   <lacx_stream_parse's text>" (with that call's code).  A source that fails to decode fails its disc with the decode's
 *   own code and "source k: ..."; the disc gets a zeroed result and no sums, and does not cost the other discs.  disc_rc,
 *   out: nullable arrays of ndiscs.  lacx_decoder_item_error(dec, disc) is the disc's text.
 * lacx_decoder_accuraterip_pcm_batch_device: device-resident source PCM in any LACX_PCM_* layout that can hold 16-bit
 *   audio; the per-source host checks ("source k: <text>"), the device-found validation texts ("source k: <text>") and the
 *   bounds are those of lacx_decoder_digest_pcm_batch_device.
 * lacx_decoder_item_ar_tracks: per track of disc `disc` of the decoder's last rip-checksum call its start, frames, flags and
 *   the three sums at offset 0.  lacx_decoder_item_ar_sums: the sums of one track at every offset, count = 2 radius + 1,
 *   ordered o = -radius .. radius.  Both valid until the decoder's next call; LACX_E_INVALID outside that call, and for a
 *   disc that failed (it has no sums).
 * lacx_ar_ids: host only.  LACX_E_INVALID: null arguments, no tracks, more than 99, an empty track, unknown flags.  A disc
 *   that has no ids gives LACX_OK and zeros.
 * Everything else as lacx_decoder_truepeak_batch_device.  No scratch: 12 (2 radius + 1) bytes per track inside the tables.
 * Time (scripts/accuraterip_bench.py, profiles/accuraterip_bench.txt): on 48 four-minute stereo 16-bit streams as
 * four discs of twelve tracks 20.3 ms of kernels and 44.3 ms of wall at radius 0, 4.7 ms of kernels below the digest's job,
 * against 128.9 ms of wall for decode plus the same sums in torch int64 on the same device; at radius 2939 (2.99e12
 * multiplier-offset pairs) 201.4 ms of kernels and 226.1 ms of wall; k_accuraterip alone 1.91 ms and 180.8 ms. */
#define LACX_AR_FIRST 1u
#define LACX_AR_LAST 2u
#define LACX_AR_NO_IDS 4u            /* lacx_ar_result.flags only */
#define LACX_AR_TRACK_SHORT 1u
#define LACX_AR_TRACK_NO_S450 2u
typedef struct lacx_ar_disc {   /* 28 bytes */
    uint32_t first_source, sources;
    uint32_t first_track, tracks;
    uint32_t flags, radius, lba0;
} lacx_ar_disc;
typedef struct lacx_ar_id {     /* 12 bytes */
    uint32_t id1, id2, cddb;
} lacx_ar_id;
typedef struct lacx_ar_result { /* 32 bytes */
    uint64_t frames;
    uint32_t tracks, radius, flags;
    lacx_ar_id ids;
} lacx_ar_result;
typedef struct lacx_ar_track {  /* 32 bytes */
    uint64_t start, frames;
    uint32_t flags, v1, v2, s450;
} lacx_ar_track;
int lacx_decoder_accuraterip_batch_device(lacx_decoder* dec, const lacx_span* lacs, uint32_t nlacs, const uint64_t* track_frames,
                                          uint32_t ntracks, const lacx_ar_disc* discs, uint32_t ndiscs, void* stream, int* disc_rc,
                                          lacx_ar_result* out, float* device_ms);
int lacx_decoder_accuraterip_pcm_batch_device(lacx_decoder* dec, const lacx_digest_source* src, uint32_t nsrc,
                                              const uint64_t* track_frames, uint32_t ntracks, const lacx_ar_disc* discs, uint32_t ndiscs,
                                              void* stream, int* disc_rc, lacx_ar_result* out, float* device_ms);
int lacx_decoder_item_ar_tracks(const lacx_decoder* dec, uint32_t disc, const lacx_ar_track** tracks, uint32_t* count);
int lacx_decoder_item_ar_sums(const lacx_decoder* dec, uint32_t disc, uint32_t track, const uint32_t** v1, const uint32_t** v2,
                              const uint32_t** s450, uint32_t* count);
int lacx_ar_ids(const uint64_t* track_frames, uint32_t ntracks, uint32_t flags, uint32_t lba0, lacx_ar_id* out);

/* Bit-compare: how two streams relate -- whether they decode to the same samples, if not how many samples differ, where and
 * by how much (the null test: the peak and energy of a - b), and whether they become identical once one is shifted by up to
 * 32767 frames, as two CD drives with different read offsets or two pressings produce.  What other tool chains call
 * "bit-compare tracks" or "compare WAVs", made on the device where the samples lie.  Out of scope: comparing across bit
 * depths, sample rates or channel counts, a lenient form, a .lac against PCM in one call (lacx_decoder_verify_batch_device
 * does that at offset 0), sub-sample or fuzzy alignment, applying the shift (the edit calls do that), more than two channels.
 * Definition (csrc/compare_core.h is its only statement in code).  Everything is an exact integer and does not
 * depend on the order of evaluation, the batch or the place in a job: device, CPU twin and a numpy restatement agree byte for
 * byte.
 *   Pair: (a, b, centre, radius) -- two indices into the call's source array (one source may stand in many pairs and is
 *   decoded once; a == b is allowed), a signed centre and a radius, 0 <= radius <= 32767, |centre| + radius < 2^31; both
 *   sources of 1 or 2 channels, 16 or 24 bit, alike in channels, depth and sample rate, each of fewer than 2^32 frames.
 *   Pairing: with na, nb the frame counts, A(f) = a[f] for 0 <= f < na and 0 in every channel elsewhere, B likewise.  At
 *   offset o frame f of A is paired with frame f + o of B over the union domain f in [fmin(o), fmax(o)), fmin(o) = min(0,
 *   -o), fmax(o) = max(na, nb - o): audio one side has and the other lacks counts as differing from zeros.
 *   Search: for every o in [centre - radius, centre + radius], mis[o] = the (frame, channel) samples of the domain with
 *   A(f)[c] != B(f + o)[c], a uint64.  The chosen offset has the fewest mismatches; ties go to the smallest |o - centre|,
 *   then to the larger o.  At radius 0 there is no search and the chosen offset is the centre.
 *   Rows: at the chosen offset o* the domain is cut into rows of 16384 frames from fmin(o*).  Per row and channel, with d =
 *   A - B: the mismatches, the first and last differing frame and the lowest frame of max |d| (counted from the domain's
 *   first frame; LACX_COMPARE_NONE where nothing differs), max |d|, the sum of |d| and the sum of d^2 (|d| < 2^25).
 *   Totals (host, lacx_compare_combine): per channel and together the mismatches, the first and last differing frame, the
 *   peak difference with its frame (the lowest; the lower channel first), the sums as 128-bit integers, the rows that
 *   differ, and lead / tail: the frames at either end of the domain that only one side has (at most the domain) and which
 *   side (LACX_COMPARE_SIDE_*).  Frame positions of the totals are on A's axis as int64: they may be negative or >= na; 0
 *   where nothing differs.
 * lacx_decoder_compare_batch_device: strict, like lacx_decoder_digest_batch_device -- the decode, the in-place mid/side
 *   inverse, then k_compare_search (one launch; not launched where every pair has radius 0), a host look at 8 (2 radius + 1)
 *   bytes per pair, and k_compare_rows (one launch) on `stream`: two round trips where any radius is above 0, else one.
 *   Refused per pair on the host before any device work, each LACX_E_INVALID: "sources outside the call's array", "channel
 *   counts differ (A, B)", "bit depths differ (A, B)", "sample rates differ (A, B)", "radius above 32767", "centre out of
 *   range", "source k holds 2^32 frames or more", "source k: <lacx_stream_parse's text>" (with that call's code; k: the index
 *   in the call's array).  A source that fails to decode fails the pairs that name it with the decode's own code and "source
 *   k: ..." and does not cost the other pairs.  pair_rc, out: nullable arrays of npairs.  lacx_decoder_item_error(dec, pair)
 *   is the pair's text.
 * lacx_decoder_compare_pcm_batch_device: device-resident source PCM in any LACX_PCM_* layout; the per-source host checks
 *   ("source k: <text>"), the device-found validation texts ("source k: <text>") and the bounds are those of
 *   lacx_decoder_digest_pcm_batch_device.
 * lacx_decoder_item_compare_rows: the rows of pair `pair` of the decoder's last compare call.
 *   lacx_decoder_item_compare_counts: mis[] over its searched offsets, count = 2 radius + 1, ordered o = centre - radius ..
 *   centre + radius; a pair of radius 0 was not searched and gives count = 0.  Both valid until the decoder's next call;
 *   LACX_E_INVALID outside that call and for a pair that failed.
 * lacx_compare_combine: host only; the totals the batch calls return, from rows.  LACX_E_INVALID: null arguments, channels
 *   not 1 or 2, bit depth not 16 or 24, a row count that is not the domain's.
 * Everything else as lacx_decoder_truepeak_batch_device.  No scratch.
 * Time (scripts/compare_bench.py, profiles/compare_bench.txt): on 24 pairs of four-minute stereo 16-bit streams, each
 * a song against a copy shifted by up to 587 frames, 21.0 ms of kernels and 44.6 ms of wall at radius 0 (the digest's job on
 * the same 48 streams: 25.3 / 48.5 ms); at radius 588 94.9 ms of kernels, at radius 2939 (2.99e12 sample comparisons) 239.2 ms
 * of kernels and 263.1 ms of wall, the search and its round trip 216.8 ms; k_compare_rows alone 2.4 to 3.8 ms. */
#define LACX_COMPARE_NONE (~0ull)
#define LACX_COMPARE_SIDE_NONE 0u
#define LACX_COMPARE_SIDE_A 1u
#define LACX_COMPARE_SIDE_B 2u
typedef struct lacx_compare_pair {        /* 24 bytes */
    uint32_t a, b;
    int64_t centre;
    uint32_t radius, reserved;
} lacx_compare_pair;
typedef struct lacx_compare_channel_row { /* 48 bytes */
    uint64_t first, last, max_at;         /* frames from the domain's first; LACX_COMPARE_NONE: nothing differs */
    uint64_t sum_abs, sum_sq;
    uint32_t mismatches, max_abs;
} lacx_compare_channel_row;
typedef struct lacx_compare_row {         /* 96 bytes */
    lacx_compare_channel_row ch[2];
} lacx_compare_row;
typedef struct lacx_compare_channel {     /* 72 bytes */
    uint64_t mismatches;
    int64_t first, last, peak_at;
    uint64_t sum_abs_lo, sum_abs_hi, sum_sq_lo, sum_sq_hi;
    uint32_t peak, reserved;
} lacx_compare_channel;
typedef struct lacx_compare {             /* 296 bytes */
    int64_t offset;                       /* the chosen offset */
    int64_t domain_first;                 /* fmin(offset), on A's axis */
    uint64_t domain_frames;
    uint64_t frames_a, frames_b;
    uint64_t mismatches;                  /* all channels */
    int64_t first, last, peak_at;
    uint64_t sum_abs_lo, sum_abs_hi, sum_sq_lo, sum_sq_hi;
    uint64_t rows, rows_differ;
    uint64_t lead, tail;
    uint32_t peak, sample_rate;
    uint8_t peak_channel, channels, bit_depth, lead_side, tail_side, reserved[3];
    lacx_compare_channel ch[2];
} lacx_compare;
int lacx_decoder_compare_batch_device(lacx_decoder* dec, const lacx_span* lacs, uint32_t nlacs, const lacx_compare_pair* pairs, uint32_t npairs,
                                      void* stream, int* pair_rc, lacx_compare* out, float* device_ms);
int lacx_decoder_compare_pcm_batch_device(lacx_decoder* dec, const lacx_digest_source* src, uint32_t nsrc, const lacx_compare_pair* pairs,
                                          uint32_t npairs, void* stream, int* pair_rc, lacx_compare* out, float* device_ms);
int lacx_decoder_item_compare_rows(const lacx_decoder* dec, uint32_t pair, const lacx_compare_row** rows, uint32_t* count);
int lacx_decoder_item_compare_counts(const lacx_decoder* dec, uint32_t pair, const uint64_t** counts, uint32_t* count);
int lacx_compare_combine(const lacx_compare_row* rows, uint32_t count, uint8_t channels, uint8_t bit_depth, uint32_t sample_rate, uint64_t frames_a,
                         uint64_t frames_b, int64_t offset, lacx_compare* out);

/* Recovery data: repairing a damaged .lac file from a parity sidecar.  Digests, salvage and the manifest all end in "this
 * block is lost"; the container has no redundancy of its own.  A recovery sidecar ("LACR") kept beside the file brings the
 * exact original bytes back when the file has rotted or been cut short.  The two sidecars differ: the manifest (LACM)
 * finds damage at the PCM level -- a block that decodes to other samples --, the recovery sidecar locates and repairs
 * damage at the byte level and knows nothing of blocks; after a repair, lacx_decoder_check_batch_device with the manifest
 * confirms it.
 * The code is Reed-Solomon erasure coding over GF(2^8) (polynomial 0x11D, generator 2).  The protected object is the whole
 * file of L >= 1 bytes, cut into k = ceil(L / S) slices, the last counted as zero-extended to S; a slice's CRC-32 (zlib)
 * covers its real bytes only.  G = ceil(k / K) groups; slice i is member i div G of group i mod G -- interleaved, so a
 * burst spreads over the groups --, group g has ceil((k - g) / G) members.  Parity slice p of group g is
 * P[g][p][j] = XOR_i c(p, i) * D[g + i * G][j] with the Cauchy coefficient c(p, i) = 1 / (p XOR (r + i)); r + K <= 256
 * keeps the two index sets apart, so every square submatrix is invertible: a group is repairable exactly when its damaged
 * data slices number at most its usable parity slices, and any damaged byte range of up to (r * G - 1) * S + 1 bytes is
 * repaired.  Parameters: slice_bytes S a multiple of 16 in 64..65536 (default 4096), parity r in 1..32 (default 8),
 * group_data K in 1..256 - r (default 128); a zero field of lacx_recovery_params, or a null pointer, means the default.
 * Sidecar, big-endian, 40 + 4k + G * r * (S + 4) bytes:
 *   0 "LACR" | 4 version = 1 | 5 r | 6 K u16 | 8 S u32 | 12 L u64 | 20 file_crc32 u32 | 24 k u32 | 28 G u32 |
 *   32 CRC-32 of bytes 0..31 | 36 k slice CRC-32 u32 | 36 + 4k CRC-32 of the slice table |
 *   40 + 4k parity records in (g, p) order, each S bytes followed by their CRC-32 u32
 * The head (bytes 0 .. 40 + 4k) must be intact and consistent -- k = ceil(L / S), G = ceil(k / K), the parameter ranges,
 * file_crc32 the lacx_crc32_combine of the slice CRCs --, else the sidecar is refused: LACX_E_INVALID, the message starting
 * "[recovery-error] ".  The parity area is treated leniently, the way salvage treats a payload: a parity record counts
 * only when it lies wholly inside the sidecar and its CRC matches; a short sidecar is flagged
 * (LACX_REPAIR_SIDECAR_TRUNCATED), not refused, and bytes behind the last record are ignored.
 * On the device (k_recovery.hip): k_slice_crc makes one CRC-32 per slice and parity record, all items of a batch in one
 * launch; k_gf_combine computes out[o] = XOR_i M[o][i] * in[i] per group -- with the Cauchy rows it makes parity, with the
 * matrix the host solved (the inverse of the <= 32 x 32 Cauchy submatrix of the lowest usable parity rows, folded with the
 * surviving slices' coefficients) it rebuilds the lost slices.  A repair is two round trips: slice CRCs come down (4 bytes
 * per slice), solved matrices go up, the output comes down.
 * All calls take a lacx_decoder handle -- its device, stream and grow-only buffers -- and follow lacx_decoder_decode_batch_device:
 * item_rc, lacx_decoder_item_error, "stream i: " prefixes, n = 0 or null arrays LACX_E_INVALID; without a device the
 * host-side outcomes (refused files, sidecars and parameters) are still filled and the call returns LACX_E_DEVICE.
 * lacx_recovery_build_batch_view: out[i] = item i's sidecar in the decoder's pinned buffer, valid until its next call.
 *   Refuses a file that lacx_stream_parse refuses, with that parser's code and text, and parameters out of range with
 *   LACX_E_INVALID "[recovery-error] ..." (the whole call).  lacx_recovery_build: a batch of one, *out malloc'd (lacx_free).
 * lacx_recovery_parse: host only: the head's fields; parity_present = the records that lie wholly inside the sidecar
 *   (their checksums are not looked at), flags = LACX_REPAIR_SIDECAR_TRUNCATED or 0.
 * The input of scan and repair is the file's first min(size, L) bytes, zero-extended to L; a slice is damaged when the
 * CRC-32 of its bytes in that input is not the table's.  results[i]: first_bad = the lowest damaged slice (== slices when
 * none), parity_slices = G * r, bad_parity = those that are missing or fail their CRC, worst_group = the group with the
 * largest (damaged slices - usable parity slices), the lowest of equals, with its two counts; flags LACX_REPAIR_*.
 * lacx_decoder_item_bad_slices: the damaged slices of item i of the last scan or repair call, ascending, valid until the
 * decoder's next call.
 * lacx_recovery_scan_batch locates damage only: LACX_OK when intact and not truncated, else LACX_E_MISMATCH
 *   "[recovery-error] slice=N bad_slices=M repairable|unrepairable" (N = first_bad), the result filled.
 * lacx_recovery_repair_batch_view: out[i] in the decoder's pinned buffer.  An intact file: LACX_OK and a copy of its L
 *   bytes.  A fully repaired file: LACX_OK, L bytes; its repaired slices are digested again on the device and the file's
 *   combined CRC-32 equals file_crc32.  A group beyond capacity: LACX_E_MISMATCH "[recovery-error] group G: B damaged
 *   slices, P parity slices usable" for the lowest such group, LACX_REPAIR_UNREPAIRED set, out[i] = {NULL, 0}; with
 *   LACX_REPAIR_BEST_EFFORT out[i] is the L bytes with every repairable group repaired and the rest as found, the code
 *   still LACX_E_MISMATCH.  A rebuilt slice whose CRC differs (a CRC collision hid a damaged slice): LACX_E_MISMATCH
 *   "[recovery-error] repaired file does not match its checksum" and no output.  repaired_slices counts what the output
 *   holds rebuilt.  lacx_recovery_repair: a batch of one, *out malloc'd. */
typedef struct lacx_recovery_params { /* 8 bytes; zeros = defaults */
    uint32_t slice_bytes;
    uint16_t parity, group_data;
} lacx_recovery_params;
typedef struct lacx_recovery_info { /* 40 bytes */
    uint64_t file_bytes;
    uint32_t file_crc32, slice_bytes, slices, groups;
    uint16_t parity, group_data;
    uint32_t parity_present, flags, reserved;
} lacx_recovery_info;
typedef struct lacx_repair_result { /* 48 bytes */
    uint64_t file_bytes;
    uint32_t slices, bad_slices, repaired_slices, first_bad, parity_slices, bad_parity, worst_group, worst_group_bad,
        worst_group_parity, flags;
} lacx_repair_result;
#define LACX_REPAIR_TRUNCATED 1u         /* file shorter than L */
#define LACX_REPAIR_TRAILING 2u          /* bytes behind L ignored */
#define LACX_REPAIR_SIDECAR_TRUNCATED 4u
#define LACX_REPAIR_UNREPAIRED 8u
#define LACX_REPAIR_BEST_EFFORT 1u       /* call flag */
int lacx_recovery_build_batch_view(lacx_decoder* dec, const lacx_span* lacs, uint32_t n, const lacx_recovery_params* params, lacx_span* out,
                                   int* item_rc, float* device_ms);
int lacx_recovery_build(lacx_decoder* dec, const uint8_t* lac, uint64_t size, const lacx_recovery_params* params, uint8_t** out,
                        uint64_t* out_size, float* device_ms);
int lacx_recovery_parse(const uint8_t* sidecar, uint64_t size, lacx_recovery_info* info);
int lacx_recovery_scan_batch(lacx_decoder* dec, const lacx_span* files, const lacx_span* sidecars, uint32_t n, int* item_rc,
                             lacx_repair_result* results, float* device_ms);
int lacx_recovery_repair_batch_view(lacx_decoder* dec, const lacx_span* files, const lacx_span* sidecars, uint32_t n, uint32_t flags,
                                    lacx_span* out, int* item_rc, lacx_repair_result* results, float* device_ms);
int lacx_recovery_repair(lacx_decoder* dec, const uint8_t* file, uint64_t size, const uint8_t* sidecar, uint64_t sidecar_size, uint32_t flags,
                         uint8_t** out, uint64_t* out_size, lacx_repair_result* result, float* device_ms);
int lacx_decoder_item_bad_slices(const lacx_decoder* dec, uint32_t i, const uint32_t** slices, uint32_t* count);

/* ---- transcode: .lac in, .lac out.  Many outputs as ONE job, each a list of frame ranges (segments) of source streams,
 * optionally re-channelled and re-quantised losslessly, encoded as one batch; PCM never leaves the device.  out[i] is
 * byte for byte the file LAC::Encoder::encode gives for the edited PCM: a complete version-3 .lac, malloc'd (lacx_free);
 * a failed output gets {NULL, 0} and a zeroed result.  The encoder supplies the zero-run and partitioning switches;
 * sample rate, depth and channels come from the sources through the output's transforms.  A version-2 source comes
 * out as version 3.
 * The job has two phases with one host look at the statuses between them.  Phase 1, on the decoder: one window job in
 * the device form, every segment a window item whose arrays point into the decoder's planar int32 staging at the
 * segment's frame offset inside its output (window semantics unchanged: only the blocks a segment overlaps are decoded,
 * whole and checked; a segment fails if and only if one of them fails, "segment k: [decode-error] block=N ..." with the
 * strict decode's code; damage outside the windows does not matter); then one launch, k_edit, over all outputs: the
 * channel operation, then the depth change, both validated, into interleaved int16 / packed int24; then the PCM digest
 * kernel over that buffer (data_crc32).  Phase 2: lacx_encode_batch_device over the outputs that survived, lacx_assemble
 * per output, and with LACX_TRANSCODE_VERIFY the verify form on the decoder, every new stream against the buffer it was
 * encoded from: a difference gives LACX_E_MISMATCH "[transcode-error] output does not decode to its sources: <verify
 * text>" and no output, else verified = 1.
 * The window job checks every decoded sample against the stream's bit depth ("sample outside the bit depth"), so what is
 * staged always fits the source depth and no store cuts a sample off.
 * Transforms are refused, never approximated; nothing is rounded.  24 -> 16 needs every sample of the output to be a
 * multiple of 256 (the output sample is s >> 8); 16 -> 24 is s << 8; LACX_CH_FOLD needs left == right in every frame.  A
 * violation fails that output with LACX_E_INVALID "[transcode-error] frame F <left|right> sample V is not a multiple of 256"
 * or "[transcode-error] frame F: left L and right R differ": F counted in the output, the lowest frame; within a frame the
 * channel operation comes before the depth change and left before right.
 * Per output, on the host before any device work, each LACX_E_INVALID with the text in lacx_decoder_item_error(dec, i):
 * "output has no segments", "segments outside the call's array", "unknown channel operation", "unsupported bit depth: B",
 * "unknown stereo mode", "segment k: <lacx_stream_parse's text>", "segment k: empty window", "segment k: window outside
 * the stream" (without wrap-around), "segment k: <channels|bit depth|sample rate> differs from segment 0: A, B" (A segment
 * 0's), "channel operation needs a <stereo|mono> source"; k counts inside the output.
 * The whole call, each LACX_E_INVALID: null arrays, nouts == 0, unknown flags, a fan-out encoder, an encoder on another
 * device than the decoder's, and whatever lacx_encode_batch_device refuses (its text).  Without a device the host
 * outcomes are still filled and the call returns LACX_E_DEVICE.  One failed output does not cost the others; the return
 * code is the lowest failing output's, "output i: <message>" in lacx_decode_last_error.  Both handles are locked for the
 * whole call (two transcode jobs that share one take turns; their other entry points take no lock).  device_ms (nullable): kernel time of phase 1 and the verification (the encode's: lacx_get_timing). */
#define LACX_TO_END UINT64_MAX
typedef struct lacx_edit_segment {   /* 32 bytes */
    const uint8_t* lac; uint64_t size;   /* a source stream, version 3 or 2 */
    uint64_t start, frames;              /* frames [start, start+frames); frames == LACX_TO_END: to the stream's end */
} lacx_edit_segment;
#define LACX_CH_KEEP 0u   /* channels as decoded */
#define LACX_CH_LEFT 1u   /* stereo -> mono: left */
#define LACX_CH_RIGHT 2u  /* stereo -> mono: right */
#define LACX_CH_FOLD 3u   /* stereo -> mono, only if left == right in every frame */
#define LACX_CH_SWAP 4u   /* stereo: channels exchanged */
#define LACX_CH_DUAL 5u   /* mono -> stereo: the channel twice */
typedef struct lacx_edit_output {    /* 16 bytes */
    uint32_t first_segment, segments;    /* its segments, in order, in the call's segment array; >= 1 */
    uint8_t bit_depth;                   /* 0 keep; 16 or 24 */
    uint8_t channel_op;                  /* LACX_CH_* */
    uint8_t stereo_mode;                 /* of the output: 0 LR, 1 MS, 2 auto; ignored for a mono output */
    uint8_t reserved[5];
} lacx_edit_output;
typedef struct lacx_edit_result {    /* 40 bytes */
    uint64_t frames, lac_bytes;
    uint32_t blocks, data_crc32;         /* zlib CRC-32 of the output PCM as WAV data bytes (lacx_digest.data_crc32) */
    uint32_t sample_rate;
    uint8_t channels, bit_depth, verified, reserved;
    uint64_t source_lac_bytes;           /* sum of its segments' stream sizes, each distinct (lac, size) once */
} lacx_edit_result;
#define LACX_TRANSCODE_VERIFY 1u
int lacx_transcode_batch(lacx_decoder* dec, lacx_encoder* enc,
                         const lacx_edit_segment* segs, uint32_t nsegs,
                         const lacx_edit_output* outs, uint32_t nouts, uint32_t flags,
                         lacx_span* out, int* item_rc, lacx_edit_result* results, float* device_ms);

/* Block::Encoder::encode drop-in for one channel block of n <= 16384 samples of ANY int32 value: blocks inside the 25-bit
 * mid/side domain of validated 16 / 24-bit input run on the streaming kernels, wider ones on a kernel of their own that
 * follows the reference through its int32-overflow order fallback (ref lpc.cpp:24-36, 188-229) and up to k = 31.
 * More than 16384 samples: LACX_E_INVALID (the LAC container cannot carry such a block). */
int lacx_block_encode(lacx_encoder* enc, const int32_t* pcm, uint32_t n, uint8_t** out, uint64_t* out_size);
int lacx_block_plan_only(lacx_encoder* enc, const int32_t* pcm, uint32_t n, lacx_channel_plan* plan);

/* Kernel-level probes for parity tests: exact autocorrelation + Q15 candidate sets of one channel
 * block as the device computes them. acorr[13]; coef[5*13]; used[5]. */
int lacx_debug_lpc(lacx_encoder* enc, const int32_t* pcm, uint32_t n, int64_t* acorr, int16_t* coef,
                   uint8_t* used);

/* Diagnostic builds (-DLACX_STAMPS) only: per-phase shader-cycle sums of k_analyze<16,1024>; returns 0 in
 * production builds. out[40]; out[32] = number of waves accumulated. */
int lacx_debug_stamps(unsigned long long* out32);

/* Host-side worker threads the encoder's emit pool runs besides the calling thread (creates the pool; no device
 * needed).  emit_threads = 1 must give 0: the reference's set_thread_count(1) means one thread in total
 * (ref src/codec/lac/encoder.cpp:385-390). */
int lacx_debug_emit_workers(lacx_encoder* enc);

/* Number of visible HIP devices (0 when the runtime or a GPU is missing); does not initialise one. */
int lacx_device_count(void);

#ifdef __cplusplus
}
#endif
#endif
