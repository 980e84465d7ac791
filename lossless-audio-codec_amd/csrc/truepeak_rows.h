// truepeak_rows.h -- the host-only end of a true-peak job: the rows as the ABI has them from the packed rows the device
// leaves (TpAcc), and the totals from the rows, for one set of rows -- an item -- or several -- an album.  Plain C++, exact
// integers up to the three doubles at the end; lacx.h states every rule.  lacx_truepeak_combine is truepeak_combine.
#pragma once
#include <cmath>
#include <cstdint>
#include <limits>
#include <vector>

#include "lacx.h"
#include "lacx_types.h"

namespace lacx {

// One device row unpacked: peak = key >> kTpPosBits, pos = 2^kTpPosBits - 1 - the key's low bits; pos 0 for a zero peak.
inline lacx_truepeak_row truepeak_row_of(const TpAcc& a) {
    const unsigned long long mask = (1ull << kTpPosBits) - 1u;
    lacx_truepeak_row r{};
    for (int c = 0; c < 2; ++c) {
        r.peak[c] = a.key[c] >> kTpPosBits;
        r.pos[c] = r.peak[c] ? (uint32_t)(mask - (a.key[c] & mask)) : 0u;
        r.sample_peak[c] = a.sample_peak[c];
    }
    return r;
}
inline void truepeak_rows_of(const TpAcc* acc, uint32_t count, std::vector<lacx_truepeak_row>& rows) {
    rows.resize(count);
    for (uint32_t i = 0; i < count; ++i) rows[i] = truepeak_row_of(acc[i]);
}

struct TpSet {
    const lacx_truepeak_row* rows;
    uint32_t count;
    uint8_t channels, bit_depth;
    uint64_t frames;
    uint32_t sample_rate;
};

// The totals of one set.  Per channel the largest peak at its lowest position in the stream (rows are in stream order and
// pos ascends inside a row, so the first row that holds the largest wins), the largest sample and the first row that holds it.
inline lacx_truepeak truepeak_of_rows(const TpSet& s) {
    const double ninf = -std::numeric_limits<double>::infinity();
    lacx_truepeak t{};
    t.frames = s.frames, t.sample_rate = s.sample_rate, t.channels = s.channels, t.bit_depth = s.bit_depth, t.rows = s.count;
    for (uint32_t c = 0; c < s.channels; ++c) {
        lacx_truepeak_channel& ch = t.ch[c];
        for (uint32_t i = 0; i < s.count; ++i) {
            const lacx_truepeak_row& r = s.rows[i];
            if (r.peak[c] > ch.peak) ch.peak = r.peak[c], ch.position = 4ull * kTpRowFrames * i + r.pos[c];
            if (r.sample_peak[c] > ch.sample_peak) ch.sample_peak = r.sample_peak[c], ch.sample_peak_row = i;
        }
    }
    const uint64_t full = 1ull << (s.bit_depth - 1);  // 2^(b-1)
    t.peak_channel = t.ch[1].peak > t.ch[0].peak ? 1 : 0;
    const uint64_t peak = t.ch[t.peak_channel].peak;
    const uint32_t sample = t.ch[1].sample_peak > t.ch[0].sample_peak ? t.ch[1].sample_peak : t.ch[0].sample_peak;
    t.true_peak = (double)peak / (8192.0 * (double)full);  // exact: peak < 2^38, the divisor a power of two
    t.true_peak_dbtp = peak ? 20.0 * std::log10(t.true_peak) : ninf;
    t.sample_peak_dbfs = sample ? 20.0 * std::log10((double)sample / (double)full) : ninf;
    if (peak > 8192ull * full) t.flags |= LACX_TRUEPEAK_OVER;
    if (sample >= full - 1u) t.flags |= LACX_TRUEPEAK_SAMPLE_FULL;
    return t;
}

// One set: its totals.  Several: the album -- the totals of the set with the largest peak (depths compared exactly, a
// 16-bit peak shifted by 8; the lowest index on ties) with `set` its index, frames and rows summed over the sets, the flags
// of all sets, and sample_peak_dbfs the largest of all sets.
inline lacx_truepeak truepeak_combine(const TpSet* sets, uint32_t nsets) {
    lacx_truepeak out{};
    uint64_t best = 0, frames = 0;
    uint32_t rows = 0;
    uint8_t flags = 0;
    double sample_db = -std::numeric_limits<double>::infinity();
    for (uint32_t k = 0; k < nsets; ++k) {
        const lacx_truepeak t = truepeak_of_rows(sets[k]);
        const uint64_t norm = t.ch[t.peak_channel].peak << (24 - sets[k].bit_depth);
        if (k == 0 || norm > best) out = t, out.set = k, best = norm;
        frames += t.frames, rows += t.rows, flags |= t.flags;
        if (t.sample_peak_dbfs > sample_db) sample_db = t.sample_peak_dbfs;
    }
    out.frames = frames, out.rows = rows, out.flags = flags, out.sample_peak_dbfs = sample_db;
    return out;
}

}  // namespace lacx
