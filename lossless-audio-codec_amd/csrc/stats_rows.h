// stats_rows.h -- the rows of the audio statistics (lacx.h) as the host side finishes them from what the device
// accumulated (StatsAcc, stats_core.h), and their totals.  Host only, no HIP: the C ABI (api_decode.cpp) and
// tests/native/sim_stats.cpp, which calls the same row builders the ABI calls.
#pragma once
#include <cstdint>
#include <cstring>
#include <vector>

#include "container.h"
#include "lacx.h"
#include "stats_core.h"

namespace lacx {

// One decoded block of `frames` (>= 1) frames from its accumulator row: the encodings of stats_core.h undone.
inline lacx_block_stats stats_row_finish(const StatsAcc& a, uint32_t frames, uint32_t channels) {
    lacx_block_stats r{};
    r.frames = frames;
    r.lead_zero_frames = frames - a.first_nz;  // (first_nz == 0: no non-zero frame, the block is silent)
    r.trail_zero_frames = frames - a.last_nz;
    r.differing = a.differing;
    for (uint32_t c = 0; c < channels; ++c) {
        const StatsChan& s = a.ch[c];
        lacx_channel_stats& o = r.ch[c];
        o.min = (int32_t)(kStatsBias - s.min_enc);
        o.max = (int32_t)(s.max_enc - kStatsBias - 1u);
        o.or_bits = s.or_bits;
        o.full_scale = s.full_scale;
        o.zeros = s.zeros;
        o.sum = (int64_t)s.sum;
        o.sum_sq = s.sum_sq;
    }
    return r;
}

// The rows of a decoded item: every block's frames from the stream's table, its fault code where it has one (every
// other field then 0), and where it decoded its statistics.  acc: the device rows, the item's first block's first.
inline void stats_rows_of_decoded(const uint8_t* lac, int version, uint32_t blocks, uint32_t channels, const std::vector<lacx_block_fault>& faults,
                                  const StatsAcc* acc, std::vector<lacx_block_stats>& rows) {
    rows.assign(blocks, lacx_block_stats{});
    for (uint32_t b = 0; b < blocks; ++b) rows[b].frames = row_frames(lac, version, b);
    for (const lacx_block_fault& f : faults) rows[f.block].code = f.code;
    for (uint32_t b = 0; b < blocks; ++b)
        if (!rows[b].code) rows[b] = stats_row_finish(acc[b], rows[b].frames, channels);
}

// The rows of a source item of `frames` frames on a regular grid of `grid` frames: nb blocks, the last the remainder.
inline void stats_rows_of_source(unsigned long long frames, uint32_t grid, uint32_t nb, uint32_t channels, const StatsAcc* acc,
                                 std::vector<lacx_block_stats>& rows) {
    rows.assign(nb, lacx_block_stats{});
    for (uint32_t b = 0; b < nb; ++b)
        rows[b] = stats_row_finish(acc[b], b + 1u < nb ? grid : (uint32_t)(frames - (unsigned long long)grid * b), channels);
}

// lacx_stats_combine: the totals of rows (lacx.h).  128-bit sums in two words with the carry by hand.
inline lacx_stats stats_combine(const lacx_block_stats* rows, uint32_t count, uint8_t channels, uint8_t bit_depth, uint32_t sample_rate) {
    lacx_stats t{};
    t.sample_rate = sample_rate;
    t.channels = channels;
    t.bit_depth = bit_depth;
    t.blocks = count;
    bool any = false;
    for (uint32_t b = 0; b < count; ++b) {
        const lacx_block_stats& r = rows[b];
        t.frames += r.frames;
        if (r.code) {
            ++t.lost_blocks;
            t.lost_frames += r.frames;
            continue;
        }
        if (r.lead_zero_frames == r.frames) ++t.silent_blocks;
        t.differing += r.differing;
        for (uint32_t c = 0; c < channels; ++c) {
            const lacx_channel_stats& s = r.ch[c];
            lacx_channel_totals& o = t.ch[c];
            if (r.frames) {
                o.min = any ? (s.min < o.min ? s.min : o.min) : s.min;
                o.max = any ? (s.max > o.max ? s.max : o.max) : s.max;
            }
            o.or_bits |= s.or_bits;
            o.full_scale += s.full_scale;
            o.zeros += s.zeros;
            const uint64_t add = (uint64_t)s.sum, lo = o.sum_lo + add;  // sign-extended to 128 bits
            o.sum_hi = (int64_t)((uint64_t)o.sum_hi + (s.sum < 0 ? ~0ull : 0ull) + (lo < add ? 1u : 0u));
            o.sum_lo = lo;
            const uint64_t sq = o.sum_sq_lo + s.sum_sq;
            o.sum_sq_hi += sq < s.sum_sq ? 1u : 0u;
            o.sum_sq_lo = sq;
        }
        any = any || r.frames != 0;
    }
    // the frames in front of the first, and behind the last, frame that is non-zero or lies in a lost block
    for (uint32_t b = 0; b < count; ++b) {
        const lacx_block_stats& r = rows[b];
        if (r.code) break;
        t.lead_zero_frames += r.lead_zero_frames;
        if (r.lead_zero_frames != r.frames) break;
    }
    for (uint32_t b = count; b-- > 0;) {
        const lacx_block_stats& r = rows[b];
        if (r.code) break;
        t.trail_zero_frames += r.trail_zero_frames;
        if (r.trail_zero_frames != r.frames) break;
    }
    return t;
}

}  // namespace lacx
