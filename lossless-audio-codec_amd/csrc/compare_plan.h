// compare_plan.h -- the host-only plan of a bit-compare job (lacx.h: lacx_decoder_compare_*): the source table, the pairs,
// the spans the search tiles and their tile counts, the zeroed counts, the rows' capacity, the capacity checks and the
// per-pair refusals.  Plain C++, no HIP: decode_plan.h puts these tables behind a digest-form job's (the stream form),
// api_decode.cpp behind the source form's; tests/native/sim_compare.cpp runs the same plan on the host.
// The tables, from a 16-byte aligned base: sources [S] (CmpSource) | spans [Q] (CmpSpan) | tile_off [Q + 1] (uint64) | pairs
// [P] (CmpPair) | row_off [P + 1] (uint64) | counts [N] (uint64, 16-byte aligned, zeroed here) | rows [R] (lacx_compare_row,
// 16-byte aligned, not initialised: k_compare_rows writes every row it is asked for whole).  There is no scratch.
// A pair of radius > 0 gets 2 radius + 1 counts and one or two spans: the stretches of A's axis, rounded out to multiples of
// 4, on which A ([0, na)) or the B window of its offsets ([-(centre + radius), nb - (centre - radius))) can be non-zero;
// where the two touch they are one span.  Everywhere else both sides are zero and nothing differs.  A pair of radius 0 gets
// neither: its offset is its centre.  Tiles are counted, not listed (tile_off), as for the rip checksums.
// The split of a workgroup between offsets and stripes of frames is chosen per pair (cmp_lanes): the smallest power of two
// of lanes, four offsets each, that holds the pair's offsets, at most kCmpThreads.
// Rows: a pair's rows depend on the chosen offset, so the plan reserves the most any offset of the pair can have (row0, the
// domain is longest at one end of the range) and the choice (cmp_set_chosen) fixes nrows and row_off; pairs and row_off go
// to the device again before k_compare_rows where there was a search.
#pragma once
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "compare_rows.h"
#include "lacx.h"
#include "lacx_types.h"

namespace lacx {

struct CmpSrcIn {  // one source of the job
    const void* data0;
    const void* data1;
    uint64_t frames;
    uint32_t layout;
    uint32_t item;  // its place in the job's bad[] array
    uint8_t channels, bit_depth;
    bool validate;  // source form
};

struct CmpPairIn {
    uint32_t a, b;  // in the job's CmpSrcIn array
    long long centre;
    uint32_t radius;
};

struct CmpFmt {  // what a refusal looks at
    uint64_t frames;
    uint32_t sample_rate;
    uint8_t channels, bit_depth;
};

struct CmpLayout {
    size_t base = 0, sources = 0, spans = 0, tile_off = 0, pairs = 0, row_off = 0, counts = 0, rows = 0, size = 0;  // byte offsets in the tables; size: their end
    uint64_t total_tiles = 0, total_counts = 0, rows_cap = 0;
    bool search = false;  // any pair has a radius above 0
    std::vector<CmpSource> src;  // (addresses null until cmp_fill)
    std::vector<CmpSpan> span;
    std::vector<unsigned long long> tiles;    // [spans + 1]
    std::vector<CmpPair> pair;
    std::vector<unsigned long long> row_offs;  // [pairs + 1], by the chosen offsets
    size_t choice_bytes() const { return counts - pairs; }  // pairs, row_off and the padding behind them: what the choice changes
};

// Why a pair is refused, or "": both sources have passed their own checks.
inline std::string cmp_pair_why(const lacx_compare_pair& p, const CmpFmt* fmt, uint32_t nsrc) {
    if (p.a >= nsrc || p.b >= nsrc) return "sources outside the call's array";
    const CmpFmt &x = fmt[p.a], &y = fmt[p.b];
    if (x.channels != y.channels) return "channel counts differ (" + std::to_string((int)x.channels) + ", " + std::to_string((int)y.channels) + ")";
    if (x.bit_depth != y.bit_depth) return "bit depths differ (" + std::to_string((int)x.bit_depth) + ", " + std::to_string((int)y.bit_depth) + ")";
    if (x.sample_rate != y.sample_rate) return "sample rates differ (" + std::to_string(x.sample_rate) + ", " + std::to_string(y.sample_rate) + ")";
    if (p.radius > kCmpMaxRadius) return "radius above " + std::to_string(kCmpMaxRadius);
    const long long lim = 1ll << 31;
    if (p.centre <= -lim || p.centre >= lim || (p.centre < 0 ? -p.centre : p.centre) + (long long)p.radius >= lim) return "centre out of range";
    if (x.frames >> 32) return "source " + std::to_string(p.a) + " holds 2^32 frames or more";
    if (y.frames >> 32) return "source " + std::to_string(p.b) + " holds 2^32 frames or more";
    return "";
}

// the offset slots of a pair's tiles: from cmp_obase to its last offset
inline uint32_t cmp_slots(long long centre, uint32_t radius) { return (uint32_t)(centre + (long long)radius - cmp_floor4(centre - (long long)radius) + 1); }
inline uint32_t cmp_lanes(long long centre, uint32_t radius) {
    uint32_t lanes = 1;
    while (kCmpLaneOffsets * lanes < cmp_slots(centre, radius) && lanes < kCmpThreads) lanes *= 2u;
    return lanes;
}

// the spans of a pair of radius > 0 (0, 1 or 2), ascending
inline uint32_t cmp_spans_of(uint64_t na, uint64_t nb, long long centre, uint32_t radius, long long* lo, long long* hi) {
    const long long r[2][2] = {{0, (long long)na}, {-(centre + (long long)radius), (long long)nb - (centre - (long long)radius)}};
    uint32_t n = 0;
    for (int k = 0; k < 2; ++k) {
        if (r[k][1] <= r[k][0]) continue;
        lo[n] = cmp_floor4(r[k][0]), hi[n] = cmp_floor4(r[k][1] + 3);
        ++n;
    }
    if (n == 2 && lo[1] <= hi[0] && lo[0] <= hi[1]) {  // they touch: one span
        lo[0] = lo[0] < lo[1] ? lo[0] : lo[1];
        hi[0] = hi[0] > hi[1] ? hi[0] : hi[1];
        n = 1;
    } else if (n == 2 && lo[1] < lo[0]) {
        const long long l = lo[0], h = hi[0];
        lo[0] = lo[1], hi[0] = hi[1], lo[1] = l, hi[1] = h;
    }
    return n;
}

// the rows a pair can have at most: the domain's length is convex in the offset, so longest at one end of the range
inline uint64_t cmp_rows_cap(uint64_t na, uint64_t nb, long long centre, uint32_t radius) {
    const uint64_t lo = cmp_rows_at(na, nb, centre - (long long)radius), hi = cmp_rows_at(na, nb, centre + (long long)radius);
    return lo > hi ? lo : hi;
}

// Fixes the chosen offsets (one per pair), and with them nrows and row_off.
inline void cmp_set_chosen(CmpLayout& y, const long long* chosen) {
    y.row_offs.assign(y.pair.size() + 1, 0);
    for (size_t k = 0; k < y.pair.size(); ++k) {
        CmpPair& p = y.pair[k];
        p.chosen = chosen[k];
        p.nrows = cmp_rows_at(y.src[p.a].frames, y.src[p.b].frames, p.chosen);
        y.row_offs[k + 1] = y.row_offs[k] + p.nrows;
    }
}

// Lays the job out.  Every pair has passed cmp_pair_why.  Addresses are not needed yet.  The chosen offsets start as the
// centres: final where no pair has a radius.
inline CmpLayout cmp_layout(size_t base, const CmpSrcIn* in, size_t nsrc, const CmpPairIn* pairs, size_t npairs) {
    CmpLayout y;
    for (size_t i = 0; i < nsrc; ++i) {
        CmpSource s{};
        s.frames = in[i].frames, s.layout = in[i].layout, s.item = in[i].item, s.channels = in[i].channels, s.bit_depth = in[i].bit_depth, s.validate = in[i].validate ? 1 : 0;
        y.src.push_back(s);
    }
    y.tiles.push_back(0);
    std::vector<long long> centres;
    for (size_t k = 0; k < npairs; ++k) {
        const CmpPairIn& q = pairs[k];
        const uint64_t na = in[q.a].frames, nb = in[q.b].frames;
        CmpPair p{};
        p.a = q.a, p.b = q.b, p.centre = (int32_t)q.centre, p.radius = q.radius, p.chosen = q.centre;
        p.count0 = y.total_counts, p.row0 = y.rows_cap;
        y.rows_cap += cmp_rows_cap(na, nb, q.centre, q.radius);
        if (q.radius) {
            y.search = true;
            y.total_counts += cmp_width(p);
            long long lo[2], hi[2];
            const uint32_t n = cmp_spans_of(na, nb, q.centre, q.radius, lo, hi);
            for (uint32_t i = 0; i < n; ++i) {
                CmpSpan s{};
                s.f_lo = lo[i], s.f_hi = hi[i], s.pair = (uint32_t)k, s.lanes = cmp_lanes(q.centre, q.radius);
                s.otiles = (cmp_slots(q.centre, q.radius) + kCmpLaneOffsets * s.lanes - 1u) / (kCmpLaneOffsets * s.lanes);
                y.span.push_back(s);
                y.tiles.push_back(y.tiles.back() + cmp_span_tiles(s));
            }
        }
        y.pair.push_back(p);
        centres.push_back(q.centre);
    }
    cmp_set_chosen(y, centres.data());
    y.total_tiles = y.tiles.back();
    auto up16 = [](size_t v) { return (v + 15u) & ~(size_t)15u; };
    y.base = y.sources = base;
    y.spans = y.sources + sizeof(CmpSource) * y.src.size();
    y.tile_off = y.spans + sizeof(CmpSpan) * y.span.size();
    y.pairs = y.tile_off + 8 * y.tiles.size();
    y.row_off = y.pairs + sizeof(CmpPair) * y.pair.size();
    y.counts = up16(y.row_off + 8 * (y.pair.size() + 1));
    y.rows = up16(y.counts + 8 * (size_t)y.total_counts);
    y.size = y.rows + (size_t)kCmpRowBytes * (size_t)y.rows_cap;
    return y;
}

// Why the job as a whole cannot run, or null: a workgroup per tile and per row.
inline const char* cmp_check(const CmpSrcIn* in, const CmpPairIn* pairs, size_t npairs) {
    uint64_t tiles = 0, rows = 0, counts = 0;
    for (size_t k = 0; k < npairs; ++k) {
        const CmpPairIn& q = pairs[k];
        const uint64_t na = in[q.a].frames, nb = in[q.b].frames;
        if ((na >> 32) || (nb >> 32)) return "source holds 2^32 frames or more";
        rows += cmp_rows_cap(na, nb, q.centre, q.radius);
        if (q.radius) {
            const uint32_t lanes = cmp_lanes(q.centre, q.radius);
            const uint64_t otiles = (cmp_slots(q.centre, q.radius) + kCmpLaneOffsets * lanes - 1u) / (kCmpLaneOffsets * lanes);
            tiles += ((na + nb + 2ull * q.radius + 8u) / kCmpTileFrames + 2u) * otiles;  // an upper bound
            counts += 2ull * q.radius + 1u;
        }
        if (tiles >= (1ull << 31)) return "batch holds 2^31 search tiles or more";
        if (rows >= (1ull << 31)) return "batch holds 2^31 rows or more";
        if (counts >= (1ull << 31)) return "batch holds 2^31 counts or more";
    }
    return nullptr;
}

// Writes pairs and row_off as they stand (the choice) at h (the tables' first byte, not the base's).
inline void cmp_fill_choice(const CmpLayout& y, uint8_t* h) {
    if (!y.pair.empty()) std::memcpy(h + y.pairs, y.pair.data(), sizeof(CmpPair) * y.pair.size());
    std::memcpy(h + y.row_off, y.row_offs.data(), 8 * y.row_offs.size());
}

// Fills the tables at h but for the rows; in: the sources cmp_layout saw, now with their addresses.
inline void cmp_fill(const CmpLayout& y, const CmpSrcIn* in, uint8_t* h) {
    auto* src = reinterpret_cast<CmpSource*>(h + y.sources);
    for (size_t i = 0; i < y.src.size(); ++i) {
        src[i] = y.src[i];
        src[i].data0 = in[i].data0;
        src[i].data1 = in[i].data1;
    }
    if (!y.span.empty()) std::memcpy(h + y.spans, y.span.data(), sizeof(CmpSpan) * y.span.size());
    std::memcpy(h + y.tile_off, y.tiles.data(), 8 * y.tiles.size());
    cmp_fill_choice(y, h);
    const size_t end = y.row_off + 8 * y.row_offs.size();
    std::memset(h + end, 0, y.rows - end);  // the padding and the counts
}

// The kernels' arguments: the tables at `tables` (where the kernels see them).
inline CmpArgs cmp_args(const CmpLayout& y, uint8_t* tables, unsigned long long* bad) {
    CmpArgs a;
    a.npairs = (uint32_t)y.pair.size();
    a.nspans = (uint32_t)y.span.size();
    a.total_tiles = y.total_tiles;
    a.total_rows = y.row_offs.back();
    a.sources = reinterpret_cast<const CmpSource*>(tables + y.sources);
    a.pairs = reinterpret_cast<const CmpPair*>(tables + y.pairs);
    a.spans = reinterpret_cast<const CmpSpan*>(tables + y.spans);
    a.tile_off = reinterpret_cast<const unsigned long long*>(tables + y.tile_off);
    a.row_off = reinterpret_cast<const unsigned long long*>(tables + y.row_off);
    a.counts = reinterpret_cast<unsigned long long*>(tables + y.counts);
    a.rows = tables + y.rows;
    a.bad = bad;
    return a;
}

// The choice from the counts as the device left them (at the tables' y.counts); a pair of radius 0 keeps its centre.
inline void cmp_choose_all(CmpLayout& y, const unsigned long long* counts) {
    std::vector<long long> chosen(y.pair.size());
    for (size_t k = 0; k < y.pair.size(); ++k) {
        const CmpPair& p = y.pair[k];
        chosen[k] = p.radius ? cmp_choose(counts + p.count0, p.centre, p.radius) : (long long)p.centre;
    }
    cmp_set_chosen(y, chosen.data());
}

// What the ABI gives back for pair k, from its rows as the device left them (the tables' y.rows + pair.row0).
inline lacx_compare cmp_result(const CmpLayout& y, size_t k, const lacx_compare_row* rows, uint32_t sample_rate) {
    const CmpPair& p = y.pair[k];
    const CmpSource& a = y.src[p.a];
    return cmp_combine(rows, p.nrows, a.channels, a.bit_depth, sample_rate, a.frames, y.src[p.b].frames, p.chosen);
}

}  // namespace lacx
