// loudness_plan.h -- the host-only plan of a loudness job (lacx.h: lacx_decoder_loudness_*): the K-weighting coefficients
// and the chunk map A per sample rate, per item its chunks, rows and places in the state, partial and row arrays, the
// tables the kernels read and the capacity of the job's scratch.  Plain C++, no HIP: decode_plan.h puts these tables behind
// a digest-form job's (the stream form), api_decode.cpp behind the source form's; tests/native/sim_loudness.cpp runs the
// same plan on the host.
// The tables, from a 16-byte aligned base: filters [4] (LoudFilter) | items [m] (LoudItem) | chunk_off [m + 1] (uint64)
// | row_off [m + 1] (uint64).  Nothing in them comes back.
// The scratch is the run's own, device only (LoudLayout::scratch bytes): states [L] (LoudState, 32 bytes) | partials [L]
// (LoudPartial, 16 bytes) | rows [R] (lacx_loudness_row, 16 bytes), L = the sum of chunks * channels, R = the sum of rows:
// 48 bytes per chunk and channel, about 5 % of the int32 PCM.  Every record is written by exactly one lane before it is
// read; nothing needs zeroing.  The rows are what comes back.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>

#include "lacx.h"
#include "loudness_core.h"

namespace lacx {

constexpr uint32_t kLoudRates[4] = {44100u, 48000u, 96000u, 192000u};
inline int loud_rate_index(uint32_t fs) {
    for (int k = 0; k < 4; ++k)
        if (kLoudRates[k] == fs) return k;
    return -1;
}

// The K-weighting of sample rate fs from the analog prototype (lacx.h), in double, and A by running loud_step without
// input on the four unit states.  The prototype's numbers go through volatile words: tan and pow are then the running C
// library's on every side -- the product's and the twin's -- and never a compiler's own evaluation at build time, whose
// last bit may differ between compilers.
inline LoudFilter loud_filter(uint32_t fs) {
    volatile double rate = (double)fs, shelf_f0 = 1681.974450955533, shelf_g = 3.999843853973347, shelf_q = 0.7071752369554196;
    volatile double vb_exp = 0.4996667741545416, hp_f0 = 38.13547087602444, hp_q = 0.5003270373238773, ten = 10.0;
    const double pi = 3.141592653589793;
    LoudFilter k{};
    {
        const double K = std::tan(pi * shelf_f0 / rate), Q = shelf_q;
        const double Vh = std::pow(ten, shelf_g / 20.0), Vb = std::pow(Vh, vb_exp);
        const double a0 = 1.0 + K / Q + K * K;
        k.sb[0] = (Vh + Vb * K / Q + K * K) / a0;
        k.sb[1] = 2.0 * (K * K - Vh) / a0;
        k.sb[2] = (Vh - Vb * K / Q + K * K) / a0;
        k.sna[0] = -(2.0 * (K * K - 1.0) / a0);
        k.sna[1] = -((1.0 - K / Q + K * K) / a0);
    }
    {
        const double K = std::tan(pi * hp_f0 / rate), Q = hp_q;
        const double d = 1.0 + K / Q + K * K;
        k.hb[0] = 1.0, k.hb[1] = -2.0, k.hb[2] = 1.0;
        k.hna[0] = -(2.0 * (K * K - 1.0) / d);
        k.hna[1] = -((1.0 - K / Q + K * K) / d);
    }
    for (int j = 0; j < 4; ++j) {
        LoudState s{{0.0, 0.0, 0.0, 0.0}};
        s.s[j] = 1.0;
        for (uint32_t t = 0; t < kLoudChunk; ++t) (void)loud_step(k, s, 0.0);
        for (int i = 0; i < 4; ++i) k.A[i][j] = s.s[i];
    }
    return k;
}

struct LoudIn {  // one item that goes to the device
    const void* data0;
    const void* data1;
    uint64_t frames;
    uint32_t sample_rate, layout;
    uint8_t channels, bit_depth;
    bool validate;  // source form
};

struct LoudLayout {
    size_t base = 0, filters = 0, items = 0, chunk_off = 0, row_off = 0, size = 0;  // byte offsets in the tables; size: their end
    uint64_t total_chunks = 0, total_lanes = 0, total_rows = 0;
    uint64_t states = 0, partials = 0, rows = 0, scratch = 0;  // byte offsets in the scratch; scratch: its capacity
};

inline uint64_t loud_chunks(uint64_t frames) { return (frames + kLoudChunk - 1u) / kLoudChunk; }
inline uint64_t loud_rows(uint64_t frames, uint32_t sample_rate) { return frames / (sample_rate / 10u); }

inline LoudLayout loud_layout(size_t base, const LoudIn* in, size_t m) {
    LoudLayout y;
    for (size_t j = 0; j < m; ++j) {
        y.total_chunks += loud_chunks(in[j].frames);
        y.total_lanes += loud_chunks(in[j].frames) * in[j].channels;
        y.total_rows += loud_rows(in[j].frames, in[j].sample_rate);
    }
    y.base = y.filters = base;
    y.items = y.filters + 4 * sizeof(LoudFilter);
    y.chunk_off = y.items + sizeof(LoudItem) * m;
    y.row_off = y.chunk_off + 8 * (m + 1);
    y.size = y.row_off + 8 * (m + 1);
    y.states = 0;
    y.partials = y.states + sizeof(LoudState) * y.total_lanes;
    y.rows = y.partials + sizeof(LoudPartial) * y.total_lanes;
    y.scratch = y.rows + sizeof(lacx_loudness_row) * y.total_rows;
    return y;
}

// Why the job as a whole cannot run, or null: an item's chunks and rows are 32-bit counts in its record.
inline const char* loud_check(const LoudIn* in, size_t m) {
    for (size_t j = 0; j < m; ++j)
        if (loud_chunks(in[j].frames) >= (1ull << 32)) return "item holds 2^32 loudness chunks or more";
    return nullptr;
}

// Fills the tables at h (the tables' first byte, not the base's).
inline void loud_fill(const LoudLayout& y, const LoudIn* in, size_t m, uint8_t* h) {
    auto* filters = reinterpret_cast<LoudFilter*>(h + y.filters);
    auto* items = reinterpret_cast<LoudItem*>(h + y.items);
    auto* chunk_off = reinterpret_cast<unsigned long long*>(h + y.chunk_off);
    auto* row_off = reinterpret_cast<unsigned long long*>(h + y.row_off);
    for (int k = 0; k < 4; ++k) filters[k] = loud_filter(kLoudRates[k]);
    uint64_t lane = 0;
    chunk_off[0] = row_off[0] = 0;
    for (size_t j = 0; j < m; ++j) {
        const LoudIn& x = in[j];
        LoudItem it{};
        it.data0 = x.data0;
        it.data1 = x.channels == 2 ? x.data1 : nullptr;
        it.frames = x.frames;
        it.sub = x.sample_rate / 10u;
        it.rows = (uint32_t)loud_rows(x.frames, x.sample_rate);
        it.used = (uint64_t)it.rows * it.sub;
        it.chunks = (uint32_t)loud_chunks(x.frames);
        it.lane0 = lane;
        it.row0 = row_off[j];
        it.layout = x.layout;
        it.channels = x.channels, it.bit_depth = x.bit_depth;
        it.rate = (uint8_t)loud_rate_index(x.sample_rate);
        it.validate = x.validate ? 1 : 0;
        items[j] = it;
        lane += (uint64_t)it.chunks * x.channels;
        chunk_off[j + 1] = chunk_off[j] + it.chunks;
        row_off[j + 1] = row_off[j] + it.rows;
    }
}

// The kernels' arguments: the tables at `tables` and the scratch at `scratch` (where the kernels see them).
inline LoudArgs loud_args(const LoudLayout& y, size_t m, const uint8_t* tables, uint8_t* scratch, unsigned long long* bad) {
    LoudArgs a;
    a.nitems = (uint32_t)m;
    a.total_chunks = y.total_chunks;
    a.total_rows = y.total_rows;
    a.filters = reinterpret_cast<const LoudFilter*>(tables + y.filters);
    a.items = reinterpret_cast<const LoudItem*>(tables + y.items);
    a.chunk_off = reinterpret_cast<const unsigned long long*>(tables + y.chunk_off);
    a.row_off = reinterpret_cast<const unsigned long long*>(tables + y.row_off);
    a.states = reinterpret_cast<LoudState*>(scratch + y.states);
    a.partials = reinterpret_cast<LoudPartial*>(scratch + y.partials);
    a.rows = reinterpret_cast<lacx_loudness_row*>(scratch + y.rows);
    a.bad = bad;
    return a;
}

}  // namespace lacx
