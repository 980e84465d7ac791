// truepeak_plan.h -- the host-only plan of a true-peak job (lacx.h: lacx_decoder_truepeak_*): per item its tiles, rows and
// place in the row array, the tables the kernel reads and writes.  Plain C++, no HIP: decode_plan.h puts these tables
// behind a digest-form job's (the stream form), api_decode.cpp behind the source form's; tests/native/sim_truepeak.cpp runs
// the same plan on the host.
// The tables, from a 16-byte aligned base: items [m] (TpItem) | tile_off [m + 1] (uint64) | rows [R] (TpAcc, 32 bytes,
// 16-byte aligned), R = the sum of the items' rows.  The rows are zeroed here -- all-zero bytes are the empty row -- and go
// to the device with the tables; they are what comes back.  There is no scratch.
#pragma once
#include <cstdint>
#include <cstring>

#include "lacx.h"
#include "lacx_types.h"

namespace lacx {

struct TpIn {  // one item that goes to the device
    const void* data0;
    const void* data1;
    uint64_t frames;
    uint32_t layout;
    uint8_t channels, bit_depth;
    bool validate;  // source form
};

struct TpLayout {
    size_t base = 0, items = 0, tile_off = 0, rows = 0, size = 0;  // byte offsets in the tables; size: their end
    uint64_t total_tiles = 0, total_rows = 0;
};

// (an item without frames has no outputs, no tiles and no rows)
inline uint64_t tp_tiles(uint64_t frames) { return frames ? (frames + kTpFlush + kTpTileFrames - 1u) / kTpTileFrames : 0u; }
inline uint64_t tp_rows(uint64_t frames) { return (frames + kTpRowFrames - 1u) / kTpRowFrames; }

inline TpLayout tp_layout(size_t base, const TpIn* in, size_t m) {
    TpLayout y;
    for (size_t j = 0; j < m; ++j) {
        y.total_tiles += tp_tiles(in[j].frames);
        y.total_rows += tp_rows(in[j].frames);
    }
    y.base = y.items = base;
    y.tile_off = y.items + sizeof(TpItem) * m;
    y.rows = (y.tile_off + 8 * (m + 1) + 15u) & ~(size_t)15u;
    y.size = y.rows + sizeof(TpAcc) * (size_t)y.total_rows;
    return y;
}

// Why the job as a whole cannot run, or null: a workgroup per tile, and an item's tiles and rows are 32-bit counts.
inline const char* tp_check(const TpIn* in, size_t m) {
    uint64_t tiles = 0;
    for (size_t j = 0; j < m; ++j) {
        if (tp_tiles(in[j].frames) >= (1ull << 31)) return "batch holds 2^31 tiles or more";
        tiles += tp_tiles(in[j].frames);
    }
    return tiles >= (1ull << 31) ? "batch holds 2^31 tiles or more" : nullptr;
}

// Fills the tables at h (the tables' first byte, not the base's).
inline void tp_fill(const TpLayout& y, const TpIn* in, size_t m, uint8_t* h) {
    auto* items = reinterpret_cast<TpItem*>(h + y.items);
    auto* tile_off = reinterpret_cast<unsigned long long*>(h + y.tile_off);
    tile_off[0] = 0;
    uint64_t row = 0;
    for (size_t j = 0; j < m; ++j) {
        const TpIn& x = in[j];
        TpItem it{};
        it.data0 = x.data0;
        it.data1 = x.channels == 2 ? x.data1 : nullptr;
        it.frames = x.frames;
        it.row0 = row;
        it.tiles = (uint32_t)tp_tiles(x.frames);
        it.rows = (uint32_t)tp_rows(x.frames);
        it.layout = x.layout;
        it.channels = x.channels, it.bit_depth = x.bit_depth;
        it.validate = x.validate ? 1 : 0;
        items[j] = it;
        row += it.rows;
        tile_off[j + 1] = tile_off[j] + it.tiles;
    }
    std::memset(h + y.tile_off + 8 * (m + 1), 0, y.size - (y.tile_off + 8 * (m + 1)));  // the padding and the rows
}

// The kernel's arguments: the tables at `tables` (where the kernel sees them).
inline TpArgs tp_args(const TpLayout& y, size_t m, uint8_t* tables, unsigned long long* bad) {
    TpArgs a;
    a.nitems = (uint32_t)m;
    a.total_tiles = y.total_tiles;
    a.total_rows = y.total_rows;
    a.items = reinterpret_cast<const TpItem*>(tables + y.items);
    a.tile_off = reinterpret_cast<const unsigned long long*>(tables + y.tile_off);
    a.rows = reinterpret_cast<TpAcc*>(tables + y.rows);
    a.bad = bad;
    return a;
}

}  // namespace lacx
