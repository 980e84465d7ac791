// spectrum_rows.h -- the host-only end of a spectrum job: the totals of one item from its rows.  Plain C++; lacx.h states
// every rule.  lacx_spectrum_combine is spectrum_of_rows.  (The device's rows are the ABI's: nothing to unpack.)
// Compiled with -ffp-contract=off like the rows' makers: the band totals are plain additions in row order.
#pragma once
#include <cmath>
#include <cstdint>
#include <limits>

#include "lacx.h"
#include "lacx_types.h"
#include "spectrum_plan.h"

namespace lacx {

struct SpSet {
    const lacx_spectrum_row* rows;
    uint32_t count;
    uint8_t channels, bit_depth;
    uint64_t frames;
    uint32_t sample_rate, window;
    double floor_db;
};

// Per channel and band P = the rows' powers added in row order; level = 10 log10(P / (windows (3 N^2 / 8) 2^(2b-3))),
// -inf for a zero band; bandwidth: the upper edge of the highest band at or above the floor; peak_band: the lowest band
// with the largest power.
inline lacx_spectrum spectrum_of_rows(const SpSet& s) {
    const double ninf = -std::numeric_limits<double>::infinity();
    lacx_spectrum t{};
    const uint32_t logn = sp_logn(s.window);
    t.frames = s.frames, t.sample_rate = s.sample_rate, t.channels = s.channels, t.bit_depth = s.bit_depth, t.rows = s.count;
    t.window = s.window, t.windows = logn ? sp_windows(s.frames, logn) : 0u;
    t.floor_db = s.floor_db;
    const double n = (double)s.window;
    const double full = (double)t.windows * (3.0 * n * n / 8.0) * std::ldexp(1.0, 2 * (int)s.bit_depth - 3);  // exact factors
    for (uint32_t c = 0; c < 2u; ++c) {
        double best = 0.0;
        for (uint32_t b = 0; b < kSpBands; ++b) {
            double p = 0.0;
            for (uint32_t i = 0; c < s.channels && i < s.count; ++i) p = p + s.rows[i].power[c][b];
            t.level_db[c][b] = p > 0.0 ? 10.0 * std::log10(p / full) : ninf;
            if (p > best) best = p, t.peak_band[c] = (uint8_t)b;
            if (t.level_db[c][b] >= s.floor_db) t.bandwidth_hz[c] = (double)(b + 1u) * (double)s.sample_rate / (2.0 * kSpBands);
        }
    }
    return t;
}

}  // namespace lacx
