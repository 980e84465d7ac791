// spectrum_plan.h -- the host-only plan of a spectrum job (lacx.h: lacx_decoder_spectrum_*): the window and twiddle tables,
// per item its windows, rows and place in the row array, the tables the kernel reads and writes.  Plain C++, no HIP:
// decode_plan.h puts these tables behind a digest-form job's (the stream form), api_decode.cpp behind the source form's;
// tests/native/sim_spectrum.cpp runs the same plan on the host.
// The tables, from a 16-byte aligned base: items [m] (SpItem) | row_off [m + 1] (uint64) | window [N] (double) | twiddle
// [N / 2][2] (double) | rows [R] (lacx_spectrum_row, 1024 bytes), R = the sum of the items' rows; every part 16-byte
// aligned.  The rows are zeroed here and go to the device with the tables; they are what comes back.  There is no scratch.
// Window and twiddles: every entry is evaluated in long double and rounded once to double; the device never evaluates a
// sine or cosine.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>

#include "lacx.h"
#include "lacx_types.h"

namespace lacx {

struct SpIn {  // one item that goes to the device
    const void* data0;
    const void* data1;
    uint64_t frames;
    uint32_t layout;
    uint8_t channels, bit_depth;
    bool validate;  // source form
};

struct SpLayout {
    size_t base = 0, items = 0, row_off = 0, window = 0, twiddle = 0, rows = 0, size = 0;  // byte offsets in the tables; size: their end
    uint32_t logn = 0;
    uint64_t total_rows = 0;
};

// log2 of a supported window length, 0 for any other value
inline uint32_t sp_logn(uint32_t window) {
    for (uint32_t b = kSpMinLog; b <= kSpMaxLog; ++b)
        if (window == (1u << b)) return b;
    return 0;
}
// (an item without frames has no windows and no rows)
inline uint64_t sp_windows(uint64_t frames, uint32_t logn) {
    const uint64_t hop = 1ull << (logn - 1u);
    return frames / hop + (frames % hop ? 1u : 0u);
}
inline uint64_t sp_rows(uint64_t frames) { return frames / kSpRowFrames + (frames % kSpRowFrames ? 1u : 0u); }

constexpr long double kSpPi = 3.14159265358979323846264338327950288L;
inline double sp_window_at(uint32_t n, uint32_t logn) { return (double)(0.5L - 0.5L * cosl(2.0L * kSpPi * (long double)n / (long double)(1u << logn))); }
inline double sp_twiddle_cos(uint32_t k, uint32_t logn) { return (double)cosl(2.0L * kSpPi * (long double)k / (long double)(1u << logn)); }
inline double sp_twiddle_sin(uint32_t k, uint32_t logn) { return (double)-sinl(2.0L * kSpPi * (long double)k / (long double)(1u << logn)); }

inline SpLayout sp_layout(size_t base, const SpIn* in, size_t m, uint32_t logn) {
    auto up16 = [](size_t x) { return (x + 15u) & ~(size_t)15u; };
    SpLayout y;
    y.logn = logn;
    for (size_t j = 0; j < m; ++j) y.total_rows += sp_rows(in[j].frames);
    const size_t n = (size_t)1 << logn;
    y.base = y.items = base;
    y.row_off = y.items + sizeof(SpItem) * m;
    y.window = up16(y.row_off + 8 * (m + 1));
    y.twiddle = y.window + 8 * n;
    y.rows = y.twiddle + 8 * n;
    y.size = y.rows + sizeof(lacx_spectrum_row) * (size_t)y.total_rows;
    return y;
}

// Why the job as a whole cannot run, or null: a workgroup per row, and an item's windows and rows are 32-bit counts.
inline const char* sp_check(const SpIn* in, size_t m, uint32_t logn) {
    uint64_t rows = 0;
    for (size_t j = 0; j < m; ++j) {
        if (sp_windows(in[j].frames, logn) >= (1ull << 31)) return "item holds 2^31 windows or more";
        rows += sp_rows(in[j].frames);
        if (rows >= (1ull << 31)) return "batch holds 2^31 rows or more";
    }
    return nullptr;
}

// Fills the tables at h (the tables' first byte, not the base's).
inline void sp_fill(const SpLayout& y, const SpIn* in, size_t m, uint8_t* h) {
    auto* items = reinterpret_cast<SpItem*>(h + y.items);
    auto* row_off = reinterpret_cast<unsigned long long*>(h + y.row_off);
    row_off[0] = 0;
    for (size_t j = 0; j < m; ++j) {
        const SpIn& x = in[j];
        SpItem it{};
        it.data0 = x.data0;
        it.data1 = x.channels == 2 ? x.data1 : nullptr;
        it.frames = x.frames;
        it.row0 = row_off[j];
        it.windows = sp_windows(x.frames, y.logn);
        it.rows = (uint32_t)sp_rows(x.frames);
        it.layout = x.layout;
        it.channels = x.channels, it.bit_depth = x.bit_depth;
        it.validate = x.validate ? 1 : 0;
        items[j] = it;
        row_off[j + 1] = row_off[j] + it.rows;
    }
    std::memset(h + y.row_off + 8 * (m + 1), 0, y.window - (y.row_off + 8 * (m + 1)));  // the padding
    const uint32_t n = 1u << y.logn;
    auto* window = reinterpret_cast<double*>(h + y.window);
    auto* twiddle = reinterpret_cast<double*>(h + y.twiddle);
    for (uint32_t i = 0; i < n; ++i) window[i] = sp_window_at(i, y.logn);
    for (uint32_t k = 0; k < n / 2u; ++k) twiddle[2u * k] = sp_twiddle_cos(k, y.logn), twiddle[2u * k + 1u] = sp_twiddle_sin(k, y.logn);
    std::memset(h + y.rows, 0, y.size - y.rows);  // the rows: +0.0 in every byte
}

// The kernel's arguments: the tables at `tables` (where the kernel sees them).
inline SpArgs sp_args(const SpLayout& y, size_t m, uint8_t* tables, unsigned long long* bad) {
    SpArgs a;
    a.nitems = (uint32_t)m;
    a.logn = y.logn;
    a.total_rows = y.total_rows;
    a.items = reinterpret_cast<const SpItem*>(tables + y.items);
    a.row_off = reinterpret_cast<const unsigned long long*>(tables + y.row_off);
    a.window = reinterpret_cast<const double*>(tables + y.window);
    a.twiddle = reinterpret_cast<const double*>(tables + y.twiddle);
    a.rows = reinterpret_cast<lacx_spectrum_row*>(tables + y.rows);
    a.bad = bad;
    return a;
}

}  // namespace lacx
