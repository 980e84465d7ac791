// container.h -- the .lac container, reader and writer: the one module that knows the layout.  A stream is a 10-byte frame
// header (ref src/codec/frame/frame_header.hpp:25-36), a big-endian block count, one table row per block -- (frames,
// compressed bytes), 8 bytes, in version 3; frames alone, 4 bytes, in the legacy version 2, which is only read -- and the
// block payloads back to back.  Plain C++, no HIP, no encoder object: the encode entry points and decode_plan.h use it,
// tests/native/sim_container.cpp drives it on the host.
#pragma once
#include <cstdint>

#include "lacx.h"
#include "lacx_types.h"

namespace lacx {

inline uint32_t be32(const uint8_t* p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3]; }
inline void put32(uint8_t* p, uint32_t v) {
    p[0] = (uint8_t)(v >> 24);
    p[1] = (uint8_t)(v >> 16);
    p[2] = (uint8_t)(v >> 8);
    p[3] = (uint8_t)v;
}

struct StreamParams {
    uint32_t sample_rate;
    uint8_t bit_depth;
    uint8_t channels;
    uint8_t stereo_mode;  // header value: 0 for mono
};

constexpr uint64_t kFrameHeaderBytes = 10;             // then the block count ...
constexpr uint64_t kTableAt = kFrameHeaderBytes + 4u;  // ... then the table
// header + block table: 4 bytes per block in version 2 (no compressed sizes, ref lac/decoder.cpp:100-104), else 8
constexpr uint64_t table_row_bytes(int version) { return version == 2 ? 4u : 8u; }
inline uint64_t stream_head_bytes(int version, uint32_t blocks) { return kTableAt + table_row_bytes(version) * blocks; }
inline uint64_t stream_head_bytes(uint32_t blocks) { return stream_head_bytes(3, blocks); }  // what the encoder writes

// Row b of the table of a stream whose head lies at lac (the caller knows that it is there: parse_stream).
inline uint32_t row_frames(const uint8_t* lac, int version, uint64_t b) { return be32(lac + kTableAt + table_row_bytes(version) * b); }
inline uint32_t row_bytes(const uint8_t* lac, uint64_t b) { return be32(lac + kTableAt + 8u * b + 4u); }  // version 3

// ---- writer (version 3) -----------------------------------------------------------------------------------------------
// What every stream-level refusal of a block size says (a row's size must be 1 .. 2^32 - 1 bytes).
constexpr const char* kBlockSizeError = "encoded block size is outside format limits";

inline void write_frame_header(const StreamParams& sp, uint8_t* o) {
    o[0] = 0x4C;
    o[1] = 0x41;
    o[2] = 3;
    o[3] = sp.channels;
    o[4] = sp.stereo_mode;
    o[5] = (uint8_t)((sp.sample_rate >> 8) & 0xFF);
    o[6] = (uint8_t)(sp.sample_rate & 0xFF);
    o[7] = (uint8_t)((sp.sample_rate >> 16) & 0xFF);
    o[8] = sp.bit_depth;
    o[9] = 0;
}
// The frame header and the block count of a stream of nb blocks: the first kTableAt bytes at lac.
inline void write_stream_start(const StreamParams& sp, uint32_t nb, uint8_t* lac) {
    write_frame_header(sp, lac);
    put32(lac + kFrameHeaderBytes, nb);
}
// Rows [first, first + n) of the table at lac, from n (frames, bytes) pairs.  Callers with disjoint row ranges may run in
// parallel.  False: a row of no bytes (every row is written all the same; the stream is not one to hand out).
inline bool write_rows(uint8_t* lac, uint64_t first, const uint32_t* rows, uint32_t n) {
    bool ok = true;
    uint8_t* p = lac + kTableAt + 8u * first;
    for (uint32_t i = 0; i < n; ++i, p += 8) {
        ok = ok && rows[2 * (size_t)i + 1] != 0;
        put32(p, rows[2 * (size_t)i]);
        put32(p + 4, rows[2 * (size_t)i + 1]);
    }
    return ok;
}
// Rows of the host emit: block b has bplans[b].frames frames and lies at bytes [offsets[b], offsets[b + 1]) of the
// payload.  False: a block of no bytes, or of more than a row can say.
inline bool rows_from_offsets(const uint64_t* offsets, const BlockPlan* bplans, uint32_t nb, uint32_t* rows) {
    for (uint32_t b = 0; b < nb; ++b) {
        const uint64_t size = offsets[b + 1] - offsets[b];
        if (size == 0 || size > 0xFFFFFFFFull) return false;
        rows[2 * (size_t)b] = bplans[b].frames;
        rows[2 * (size_t)b + 1] = (uint32_t)size;
    }
    return true;
}

// ---- reader -----------------------------------------------------------------------------------------------------------
// Container header + block table: the structural rules of the reference's reader (src/codec/frame/frame_header.hpp:48-74,
// lac/decoder.cpp:84-145) -- sync, version 3, channels, stereo mode (0 for mono), one of the four sample rates, depth,
// reserved byte; at least one block; every block 1..16384 frames, non-final ones at least 256; non-zero compressed
// sizes that add up to the file; at most 6 912 000 000 samples and a WAV that RIFF can hold.  NOT taken over: its cap on
// the decoded PCM (1 GiB) and the block count that follows from it, which would refuse the 2 h stream of BASELINE
// configs[3].  The legacy version-2 container (no compressed sizes, hence no parallelism) is read too: one lane walks it.
// Returns LACX_OK, or LACX_E_INVALID with the message in *why.
namespace container_detail {
// The walk both readers share.  present == null: the strict reader.  Else the lenient one (scan_stream): the two rules on
// the length of a version-3 payload are not applied, *present = the blocks whose whole byte range lies inside the file
// (the others are a suffix) and *flags says how the file's length differs from what the table states.
inline int walk_stream(const uint8_t* lac, uint64_t size, lacx_stream_info* out, const char** why, uint32_t* present, uint32_t* flags) {
    const bool lenient = present != nullptr;
    auto fail = [&](const char* msg) { return *why = msg, LACX_E_INVALID; };
    if (!lac || !out) return fail("null argument");
    if (size == 0) return fail("[decode-error] empty input");
    if (size < kFrameHeaderBytes || lac[0] != 0x4C || lac[1] != 0x41 || (lac[2] != 3 && lac[2] != 2)) return fail("[decode-error] invalid frame header");
    const int version = lac[2], ch = lac[3], sm = lac[4], bd = lac[8];
    const uint32_t sr = ((uint32_t)lac[5] << 8) | lac[6] | ((uint32_t)lac[7] << 16);
    const bool rate_ok = sr == 44100 || sr == 48000 || sr == 96000 || sr == 192000;
    if ((ch != 1 && ch != 2) || sm > 2 || (ch == 1 && sm != 0) || !rate_ok || (bd != 16 && bd != 24) || lac[9] != 0)
        return fail("[decode-error] invalid frame header");
    if (size < kTableAt) return fail("[decode-error] invalid block count");
    const uint32_t nb = be32(lac + kFrameHeaderBytes);
    if (nb == 0) return fail("[decode-error] invalid block count");
    const uint64_t head = stream_head_bytes(version, nb);
    if (size < head) return fail("[decode-error] truncated block size table");
    uint64_t frames = 0, pay = 0;
    uint32_t inside = 0;  // rows whose bytes end inside the file: a prefix, the sizes being positive
    for (uint32_t b = 0; b < nb; ++b) {
        const uint32_t n = row_frames(lac, version, b);
        if (n == 0 || n > (uint32_t)kMaxBlock || (b + 1 < nb && n < 256u)) return fail("[decode-error] invalid block size");
        frames += n;
        if (frames > 6912000000ull) return fail("[decode-error] total samples exceed maximum");
        if (version >= 3) {
            const uint32_t by = row_bytes(lac, b);
            // The device reader's bit positions are 32-bit and relative to the block: a block must stay below 2^29 bytes.
            // (The reference takes any non-zero size that fits the file; a block this long -- a Rice token at k = 0 may
            // carry a unary part of up to 2^30 bits -- is a documented deviation, see lacx.h.)
            if (by == 0 || by >= (1u << 29)) return fail("[decode-error] invalid compressed block size");
            pay += by;
            if (!lenient && pay > size) return fail("[decode-error] compressed block sizes exceed frame payload");
            if (head + pay <= size) inside = b + 1;
        }
    }
    const uint64_t wav_bytes = frames * (uint64_t)ch * (uint64_t)(bd / 8);
    if (36u + wav_bytes + (wav_bytes & 1u) > 0xFFFFFFFFull) return fail("[decode-error] decoded WAV data exceeds RIFF limit");
    if (!lenient && version >= 3 && head + pay != size) return fail("[decode-error] block payloads do not fill the file");
    if (version == 2 && size - head >= (1ull << 29)) return fail("[decode-error] version-2 payload too large for the serial reader");
    out->sample_rate = sr;
    out->blocks = nb;
    out->frames = frames;
    out->channels = (uint8_t)ch;
    out->bit_depth = (uint8_t)bd;
    out->stereo_mode = (uint8_t)sm;
    out->version = (uint8_t)version;
    if (lenient) {  // (a version-2 stream has no sizes to miss: every block is the serial lane's to find)
        *present = version >= 3 ? inside : nb;
        *flags = version < 3 || head + pay == size ? 0u : head + pay > size ? LACX_SALVAGE_TRUNCATED : LACX_SALVAGE_TRAILING;
    }
    return LACX_OK;
}
}  // namespace container_detail

inline int parse_stream(const uint8_t* lac, uint64_t size, lacx_stream_info* out, const char** why) {
    return container_detail::walk_stream(lac, size, out, why, nullptr, nullptr);
}

// The lenient reader of the salvage decode: parse_stream's rules and messages for the header and the block table, but a
// version-3 file may end early or carry bytes behind its last block.  *present_blocks: the blocks whose whole byte range
// [start, start + bytes) lies inside the file -- the missing ones are always a suffix; *flags: LACX_SALVAGE_TRUNCATED for
// a file shorter than its table states, LACX_SALVAGE_TRAILING for a longer one (the bytes behind the last block are
// ignored).  A stream parse_stream accepts gives the same info, every block present and no flag; version 2 is read as
// parse_stream reads it.
inline int scan_stream(const uint8_t* lac, uint64_t size, lacx_stream_info* out, uint32_t* present_blocks, uint32_t* flags, const char** why) {
    if (!present_blocks || !flags) return *why = "null argument", LACX_E_INVALID;
    *present_blocks = 0, *flags = 0;
    return container_detail::walk_stream(lac, size, out, why, present_blocks, flags);
}

}  // namespace lacx
