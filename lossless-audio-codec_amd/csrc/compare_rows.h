// compare_rows.h -- the totals of a bit-compare (lacx.h: lacx_compare) as the host side makes them from the rows the device
// wrote (lacx_compare_row, compare_core.h), and the choice of the offset from the searched counts.  Host only, no HIP: the C
// ABI (api_decode.cpp) and tests/native/sim_compare.cpp, which calls what the ABI calls.
#pragma once
#include <cstdint>

#include "lacx.h"
#include "lacx_types.h"

namespace lacx {

// The chosen offset from mis[centre - radius .. centre + radius]: the fewest mismatches; ties to the smallest |o - centre|,
// then to the larger o.
inline long long cmp_choose(const unsigned long long* counts, long long centre, uint32_t radius) {
    uint32_t best = radius;  // (the centre: distance 0)
    for (uint32_t d = 1; d <= radius; ++d) {  // by growing distance, the larger offset first: a later one must be strictly better
        if (counts[radius + d] < counts[best]) best = radius + d;
        if (counts[radius - d] < counts[best]) best = radius - d;
    }
    return centre - (long long)radius + (long long)best;
}

// the rows of the domain at offset o
inline unsigned long long cmp_rows_at(unsigned long long na, unsigned long long nb, long long o) {
    const unsigned long long len = (unsigned long long)(cmp_fmax(na, nb, o) - cmp_fmin(o));
    return (len + kCmpRowFrames - 1u) / kCmpRowFrames;
}

namespace cmp_detail {
inline void add128(uint64_t& lo, uint64_t& hi, uint64_t v) {  // the carry by hand, as stats_rows.h
    const uint64_t s = lo + v;
    hi += s < v ? 1u : 0u;
    lo = s;
}
}  // namespace cmp_detail

// lacx_compare_combine: the totals of `count` rows (the caller has checked that count is the domain's).
inline lacx_compare cmp_combine(const lacx_compare_row* rows, uint64_t count, uint8_t channels, uint8_t bit_depth, uint32_t sample_rate, uint64_t na,
                                uint64_t nb, long long o) {
    using cmp_detail::add128;
    lacx_compare t{};
    const long long dom0 = cmp_fmin(o), dom1 = cmp_fmax(na, nb, o);
    t.offset = o, t.domain_first = dom0, t.domain_frames = (uint64_t)(dom1 - dom0);
    t.frames_a = na, t.frames_b = nb, t.sample_rate = sample_rate, t.channels = channels, t.bit_depth = bit_depth;
    t.rows = count;
    for (uint64_t r = 0; r < count; ++r) {
        bool differs = false;
        for (uint32_t c = 0; c < channels; ++c) {
            const lacx_compare_channel_row& s = rows[r].ch[c];
            if (s.mismatches == 0) continue;
            differs = true;
            lacx_compare_channel& x = t.ch[c];
            const long long first = dom0 + (long long)s.first, last = dom0 + (long long)s.last, at = dom0 + (long long)s.max_at;
            if (x.mismatches == 0) x.first = first;  // (rows ascend)
            x.last = last;
            if (s.max_abs > x.peak) x.peak = s.max_abs, x.peak_at = at;
            x.mismatches += s.mismatches;
            add128(x.sum_abs_lo, x.sum_abs_hi, s.sum_abs);
            add128(x.sum_sq_lo, x.sum_sq_hi, s.sum_sq);
        }
        t.rows_differ += differs ? 1u : 0u;
    }
    for (uint32_t c = 0; c < channels; ++c) {
        const lacx_compare_channel& x = t.ch[c];
        if (x.mismatches == 0) continue;
        if (t.mismatches == 0 || x.first < t.first) t.first = x.first;
        if (t.mismatches == 0 || x.last > t.last) t.last = x.last;
        if (x.peak > t.peak || (x.peak == t.peak && x.peak_at < t.peak_at)) t.peak = x.peak, t.peak_at = x.peak_at, t.peak_channel = (uint8_t)c;
        t.mismatches += x.mismatches;
        add128(t.sum_abs_lo, t.sum_abs_hi, x.sum_abs_lo);
        t.sum_abs_hi += x.sum_abs_hi;
        add128(t.sum_sq_lo, t.sum_sq_hi, x.sum_sq_lo);
        t.sum_sq_hi += x.sum_sq_hi;
    }
    // lead and tail: A holds [0, na), B holds [-o, nb - o) on A's axis
    const uint64_t len = t.domain_frames, lead = (uint64_t)(o < 0 ? -o : o);
    t.lead = lead < len ? lead : len;
    t.lead_side = (uint8_t)(o == 0 ? LACX_COMPARE_SIDE_NONE : o < 0 ? LACX_COMPARE_SIDE_A : LACX_COMPARE_SIDE_B);
    const long long ea = (long long)na, eb = (long long)nb - o;
    const uint64_t tail = (uint64_t)(ea > eb ? ea - eb : eb - ea);
    t.tail = tail < len ? tail : len;
    t.tail_side = (uint8_t)(ea == eb ? LACX_COMPARE_SIDE_NONE : ea > eb ? LACX_COMPARE_SIDE_A : LACX_COMPARE_SIDE_B);
    return t;
}

}  // namespace lacx
