// inspect_rows.h -- the rows of the stream inspection (lacx.h) as the host side finishes them from what the lanes left,
// and their per-stream totals.  Host only, no HIP: the C ABI (api_decode.cpp) and tests/native/sim_inspect.cpp, which
// calls the same row builder and the same combine the ABI calls.
#pragma once
#include <cstdint>
#include <cstring>
#include <vector>

#include "container.h"
#include "lacx.h"

namespace lacx {

// The rows of an inspected item: the lanes' rows for the blocks that had a lane (a version-3 item's present blocks, every
// block of a version-2 item), and for the blocks the file does not hold their frames and bytes from the table and
// code 10.  dev: the device rows, the item's first block's first.
inline void inspect_rows_of_item(const uint8_t* lac, int version, uint32_t blocks, uint32_t present, const lacx_block_info* dev,
                                 std::vector<lacx_block_info>& rows) {
    rows.assign(blocks, lacx_block_info{});
    for (uint32_t b = 0; b < blocks; ++b) {
        if (b < present) {
            rows[b] = dev[b];
            continue;
        }
        rows[b].frames = row_frames(lac, version, b);
        rows[b].bytes = version == 2 ? 0u : row_bytes(lac, b);
        rows[b].code = LACX_BLOCK_MISSING;
    }
}

// lacx_inspect_combine: the totals of rows (lacx.h).  The 128-bit sum in two words with the carry by hand.
inline lacx_stream_report inspect_combine(const lacx_block_info* rows, uint32_t count, const lacx_stream_info* info) {
    lacx_stream_report t{};
    if (info) {
        t.sample_rate = info->sample_rate;
        t.channels = info->channels;
        t.bit_depth = info->bit_depth;
        t.stereo_mode = info->stereo_mode;
        t.version = info->version;
        t.head_bytes = stream_head_bytes(info->version, info->blocks);
    }
    t.blocks = count;
    t.k_min = 255;
    for (uint32_t b = 0; b < count; ++b) {
        const lacx_block_info& r = rows[b];
        t.frames += r.frames;
        if (r.code) {
            ++t.lost_blocks;
            continue;
        }
        t.payload_bytes += r.bytes;
        t.ms_blocks += r.ms ? 1u : 0u;
        uint64_t chbits = 0;
        for (uint32_t c = 0; c < r.channels && c < 2u; ++c) {
            const lacx_channel_info& s = r.ch[c];
            ++t.channel_blocks;
            if (s.predictor_type == 0 && s.order <= 4) ++t.fixed_blocks[s.order];
            else if (s.predictor_type == 1) ++t.fir_blocks;
            else if (s.predictor_type == 2 && s.order <= 32) ++t.lpc_blocks[s.order];
            if (s.partition_order <= 8) ++t.partition_order_blocks[s.partition_order];
            for (uint32_t m = 0; m < 4u; ++m) {
                t.mode_parts[m] += s.mode_parts[m];
                t.mode_samples[m] += s.mode_samples[m];
            }
            chbits += s.bits;
            t.header_bits += s.header_bits;
            t.tag_bits += s.tag_bits;
            t.unary_bits += s.unary_bits;
            t.remainder_bits += s.remainder_bits;
            t.escape_bits += s.escape_bits;
            t.pad_bits += s.pad_bits;
            t.rice_samples += s.rice_samples;
            t.run_tokens += s.run_tokens;
            t.run_samples += s.run_samples;
            t.escape_samples += s.escape_samples;
            for (uint32_t k = 0; k < 3u; ++k) t.bin_samples[k] += s.bin_samples[k];
            const uint64_t lo = t.sum_u_lo + s.sum_u;
            t.sum_u_hi += lo < s.sum_u ? 1u : 0u;
            t.sum_u_lo = lo;
            if (s.max_u > t.max_u) t.max_u = s.max_u;
            if (s.unary_max > t.unary_max) t.unary_max = s.unary_max;
            if (s.k_min < t.k_min) t.k_min = s.k_min;
            if (s.k_max > t.k_max) t.k_max = s.k_max;
        }
        t.bits += chbits;
        t.flag_bits += 8ull * r.bytes - chbits;  // the per-block stereo flag, where the stream has one
    }
    return t;
}

}  // namespace lacx
