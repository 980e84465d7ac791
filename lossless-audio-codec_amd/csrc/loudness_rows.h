// loudness_rows.h -- the host-only end of a loudness job: the totals of BS.1770-4 / EBU R 128 / EBU Tech 3342 from the rows
// the device leaves (one per sub-block of fs / 10 frames: the K-weighted energy per channel), for one set of rows -- an item
// -- or several -- an album.  Plain C++ in double; lacx.h states every rule.  lacx_loudness_combine is this function.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>
#include <vector>

#include "lacx.h"

namespace lacx {

struct LoudSet {
    const lacx_loudness_row* rows;
    uint32_t count;
    uint8_t channels, bit_depth;
    uint32_t sample_rate;
};

inline double loud_lufs(double z) { return -0.691 + 10.0 * std::log10(z); }  // (z = 0: -INFINITY)

inline lacx_loudness loudness_combine(const LoudSet* sets, uint32_t nsets) {
    const double ninf = -std::numeric_limits<double>::infinity();
    lacx_loudness out{};
    out.integrated_lufs = out.relative_gate_lufs = out.momentary_max_lufs = out.shortterm_max_lufs = ninf;
    if (nsets) out.sample_rate = sets[0].sample_rate, out.channels = sets[0].channels, out.bit_depth = sets[0].bit_depth;
    std::vector<double> gate_z, range_z;  // the gating blocks' and the range's short-term windows' powers, over all sets
    for (uint32_t k = 0; k < nsets; ++k) {
        const LoudSet& s = sets[k];
        const uint32_t S = s.count;
        const double n = (double)(s.sample_rate / 10u);
        const double full = std::ldexp(1.0, 2 * (s.bit_depth - 1));  // 4^(b-1)
        out.frames += (uint64_t)S * (s.sample_rate / 10u);
        out.subblocks += S;
        std::vector<double> e(S);
        for (uint32_t i = 0; i < S; ++i) e[i] = s.channels == 2 ? s.rows[i].energy[0] + s.rows[i].energy[1] : s.rows[i].energy[0];
        for (uint32_t j = 0; j + 4u <= S; ++j) {
            const double z = (((e[j] + e[j + 1]) + e[j + 2]) + e[j + 3]) / (4.0 * n * full);
            gate_z.push_back(z);
            out.momentary_max_lufs = std::max(out.momentary_max_lufs, loud_lufs(z));
        }
        for (uint32_t j = 0; j + 30u <= S; ++j) {
            double sum = 0.0;
            for (uint32_t i = 0; i < 30u; ++i) sum += e[j + i];
            const double z = sum / (30.0 * n * full);
            out.shortterm_max_lufs = std::max(out.shortterm_max_lufs, loud_lufs(z));
            if (j % 10u == 0u) range_z.push_back(z);
        }
    }
    out.gating_blocks = (uint32_t)gate_z.size();
    if (gate_z.empty()) {  // every level -INFINITY, range 0
        out.flags = LACX_LOUDNESS_TOO_SHORT;
        out.shortterm_max_lufs = ninf;
        return out;
    }
    // integrated: the absolute gate, then the relative gate 10 LU below the loudness of what passed
    double sum = 0.0;
    for (double z : gate_z)
        if (loud_lufs(z) > -70.0) sum += z, ++out.above_absolute;
    if (out.above_absolute == 0) {
        out.flags = LACX_LOUDNESS_SILENT;
    } else {
        out.relative_gate_lufs = loud_lufs(sum / out.above_absolute) - 10.0;
        sum = 0.0;
        for (double z : gate_z) {
            const double l = loud_lufs(z);
            if (l > -70.0 && l > out.relative_gate_lufs) sum += z, ++out.above_relative;
        }
        if (out.above_relative) out.integrated_lufs = loud_lufs(sum / out.above_relative);
    }
    // range: the same with 20 LU over the short-term windows at a hop of 10 sub-blocks
    sum = 0.0;
    uint32_t m = 0;
    for (double z : range_z)
        if (loud_lufs(z) > -70.0) sum += z, ++m;
    if (m) {
        const double gate = loud_lufs(sum / m) - 20.0;
        std::vector<double> l;
        for (double z : range_z)
            if (loud_lufs(z) > -70.0 && loud_lufs(z) > gate) l.push_back(loud_lufs(z));
        if (!l.empty()) {
            std::sort(l.begin(), l.end());
            const size_t hi = (size_t)std::floor((double)(l.size() - 1) * 0.95 + 0.5), lo = (size_t)std::floor((double)(l.size() - 1) * 0.10 + 0.5);
            out.range_lu = l[hi] - l[lo];
        }
    }
    return out;
}

inline lacx_loudness loudness_of_rows(const lacx_loudness_row* rows, uint32_t count, uint8_t channels, uint8_t bit_depth, uint32_t sample_rate) {
    const LoudSet s{rows, count, channels, bit_depth, sample_rate};
    return loudness_combine(&s, 1);
}

}  // namespace lacx
