// accuraterip_plan.h -- the host-only plan of a rip-checksum job (lacx.h: lacx_decoder_accuraterip_*): per disc its source
// table, its tracks and their spans, the tile counts, the zeroed sums, the capacity checks, the per-disc refusals and the
// disc ids.  Plain C++, no HIP: decode_plan.h puts these tables behind a digest-form job's (the stream form), api_decode.cpp
// behind the source form's; tests/native/sim_accuraterip.cpp runs the same plan on the host.
// The tables, from a 16-byte aligned base: sources [S] (ArSource) | spans [P] (ArSpan) | tile_off [P + 1] (uint64) |
// sums [N] (uint32, 16-byte aligned).  A disc's sums are [track][v1 | v2 | s450][2 radius + 1], ordered o = -radius ..
// radius; they are zeroed here, go to the device with the tables and are what comes back.  There is no scratch.
// A track gives one span for v1 / v2 (multipliers lo_t .. hi_t from the track's first frame, the high halves kept) unless its
// range is empty, and one for s450 (multipliers 1 .. 588 from the track's frame 450 * 588, low halves only) where it is long
// enough: to the kernel the two are alike.  Tiles are not listed: a span's tiles are counted (tile_off) and a workgroup finds
// its span by bisection and its (multiplier tile, offset tile) by division (ar_tile).
// The split of a workgroup between offsets and multiplier stripes is chosen per disc (ar_lanes): the smallest power of two
// that holds 2 radius + 1 offsets, at most kArThreads -- at radius 0 all 256 threads stripe the multipliers of one offset
// and the job is one pass over the PCM; from radius 128 on every thread owns an offset.
#pragma once
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "lacx.h"
#include "lacx_types.h"

namespace lacx {

struct ArSrcIn {  // one source of a disc
    const void* data0;
    const void* data1;
    uint64_t frames;
    uint32_t layout;
    uint32_t item;  // its place in the job's bad[] array
};

struct ArDiscIn {
    uint32_t src0, nsrc;           // its sources in the job's ArSrcIn array
    const uint64_t* track_frames;  // [ntracks]
    uint32_t ntracks;
    uint32_t flags, radius;
    bool validate;                 // source form
};

struct ArTrackAt {
    uint64_t start, frames;
    uint32_t flags;  // LACX_AR_TRACK_*
};
struct ArDiscAt {
    uint64_t frames;
    uint32_t track0, ntracks;  // in ArLayout::tracks
    uint32_t radius, flags;
    uint64_t sum0;             // its first sum
};

struct ArLayout {
    size_t base = 0, sources = 0, spans = 0, tile_off = 0, sums = 0, size = 0;  // byte offsets in the tables; size: their end
    uint64_t total_tiles = 0, total_sums = 0;
    std::vector<ArSource> src;  // (addresses null until ar_fill)
    std::vector<ArSpan> span;
    std::vector<unsigned long long> tiles;  // [spans + 1]
    std::vector<ArDiscAt> discs;
    std::vector<ArTrackAt> tracks;
};

inline uint32_t ar_lanes(uint32_t radius) {
    uint32_t lanes = 1;
    while (lanes < 2u * radius + 1u && lanes < kArThreads) lanes *= 2u;
    return lanes;
}

// the multiplier range of track t of T: lo .. hi, empty where hi < lo
inline void ar_range(uint32_t t, uint32_t T, uint64_t frames, uint32_t flags, int64_t& lo, int64_t& hi) {
    lo = t == 0 && (flags & LACX_AR_FIRST) ? 5 * kArSector : 1;
    hi = t + 1 == T && (flags & LACX_AR_LAST) ? (int64_t)frames - 5 * (int64_t)kArSector : (int64_t)frames;
}

// Why a disc is refused, or "": D its sources' frames together.
inline std::string ar_disc_why(uint32_t nsrc, uint64_t D, const uint64_t* track_frames, uint32_t ntracks, uint32_t flags, uint32_t radius) {
    if (nsrc == 0) return "disc has no sources";
    if (ntracks == 0) return "disc has no tracks";
    if (ntracks > 99) return "more than 99 tracks";
    uint64_t sum = 0;
    bool wrapped = false;
    for (uint32_t t = 0; t < ntracks; ++t) {
        if (track_frames[t] == 0) return "track " + std::to_string(t) + " is empty";
        wrapped = wrapped || sum + track_frames[t] < sum;
        sum += track_frames[t];
    }
    if (wrapped || sum != D) return "track lengths do not sum to the disc's frames (" + std::to_string(sum) + ", " + std::to_string(D) + ")";
    if (radius > kArMaxRadius) return "radius above " + std::to_string(kArMaxRadius);
    if (flags & ~(uint32_t)(LACX_AR_FIRST | LACX_AR_LAST)) return "unknown flags";
    return "";
}

// The disc ids (lacx.h), given where the disc is whole and every track a whole number of sectors; else zeros and false.
inline bool ar_ids(const uint64_t* track_frames, uint32_t ntracks, uint32_t flags, uint32_t lba0, lacx_ar_id& out) {
    out = lacx_ar_id{0, 0, 0};
    const uint32_t whole = LACX_AR_FIRST | LACX_AR_LAST;
    if ((flags & whole) != whole || ntracks == 0) return false;
    for (uint32_t t = 0; t < ntracks; ++t)
        if (track_frames[t] % kArSector) return false;
    auto digits = [](uint64_t v) {
        uint64_t s = 0;
        for (; v; v /= 10u) s += v % 10u;
        return s;
    };
    uint64_t lba = lba0, id1 = 0, id2 = 0, dsum = 0;
    for (uint32_t t = 0; t < ntracks; ++t) {
        id1 += lba;
        id2 += (lba ? lba : 1u) * (t + 1u);
        dsum += digits((lba + 150u) / 75u);
        lba += track_frames[t] / kArSector;
    }
    const uint64_t leadout = lba;
    out.id1 = (uint32_t)(id1 + leadout);
    out.id2 = (uint32_t)(id2 + leadout * (ntracks + 1u));
    out.cddb = (uint32_t)((dsum % 255u) << 24) | (uint32_t)(((leadout + 150u) / 75u - ((uint64_t)lba0 + 150u) / 75u) << 8) | ntracks;
    return true;
}

// Lays the job out.  Every disc has passed ar_disc_why; its sources have frames > 0.  Addresses are not needed yet.
inline ArLayout ar_layout(size_t base, const ArSrcIn* in, const ArDiscIn* discs, size_t ndiscs) {
    ArLayout y;
    y.tiles.push_back(0);
    for (size_t k = 0; k < ndiscs; ++k) {
        const ArDiscIn& d = discs[k];
        ArDiscAt at{};
        at.track0 = (uint32_t)y.tracks.size(), at.ntracks = d.ntracks, at.radius = d.radius, at.flags = d.flags, at.sum0 = y.total_sums;
        const uint32_t src0 = (uint32_t)y.src.size();
        for (uint32_t i = 0; i < d.nsrc; ++i) {
            const ArSrcIn& s = in[d.src0 + i];
            y.src.push_back(ArSource{nullptr, nullptr, at.frames, s.frames, s.layout, s.item});
            at.frames += s.frames;
        }
        const uint64_t width = 2ull * d.radius + 1u;
        uint64_t start = 0;
        for (uint32_t t = 0; t < d.ntracks; ++t) {
            const uint64_t n = d.track_frames[t];
            ArTrackAt tr{start, n, 0};
            ArSpan sp{};
            sp.disc_frames = at.frames, sp.src0 = src0, sp.nsrc = d.nsrc, sp.radius = d.radius, sp.lanes = ar_lanes(d.radius);
            sp.validate = d.validate ? 1 : 0;
            int64_t lo, hi;
            ar_range(t, d.ntracks, n, d.flags, lo, hi);
            const uint64_t row = at.sum0 + 3u * width * t;
            if (hi < lo) {
                tr.flags |= LACX_AR_TRACK_SHORT;
            } else {
                sp.frame1 = start, sp.m_lo = (uint32_t)lo, sp.m_hi = (uint32_t)hi, sp.sum0 = (uint32_t)row, sp.keep_hi = 1;
                y.span.push_back(sp);
                y.tiles.push_back(y.tiles.back() + ar_span_tiles(sp));
            }
            if (n < 451ull * kArSector) {
                tr.flags |= LACX_AR_TRACK_NO_S450;
            } else {
                sp.frame1 = start + 450ull * kArSector, sp.m_lo = 1, sp.m_hi = kArSector, sp.sum0 = (uint32_t)(row + 2u * width), sp.keep_hi = 0;
                y.span.push_back(sp);
                y.tiles.push_back(y.tiles.back() + ar_span_tiles(sp));
            }
            y.tracks.push_back(tr);
            start += n;
        }
        y.total_sums += 3u * width * d.ntracks;
        y.discs.push_back(at);
    }
    y.total_tiles = y.tiles.back();
    y.base = y.sources = base;
    y.spans = y.sources + sizeof(ArSource) * y.src.size();
    y.tile_off = y.spans + sizeof(ArSpan) * y.span.size();
    y.sums = (y.tile_off + 8 * y.tiles.size() + 15u) & ~(size_t)15u;
    y.size = y.sums + 4 * (size_t)y.total_sums;
    return y;
}

// Why the job as a whole cannot run, or null: a workgroup per tile, multipliers and sum indices are 32-bit.
inline const char* ar_check(const ArSrcIn* in, const ArDiscIn* discs, size_t ndiscs) {
    uint64_t tiles = 0, sums = 0;
    for (size_t k = 0; k < ndiscs; ++k) {
        const ArDiscIn& d = discs[k];
        const uint64_t width = 2ull * d.radius + 1u, otiles = (width + ar_lanes(d.radius) - 1u) / ar_lanes(d.radius);
        uint64_t frames = 0;
        for (uint32_t i = 0; i < d.nsrc; ++i) {
            if (in[d.src0 + i].frames >> 56) return "source frame count out of range";
            frames += in[d.src0 + i].frames;
        }
        if (frames >> 32) return "disc holds 2^32 frames or more";
        for (uint32_t t = 0; t < d.ntracks; ++t) tiles += (d.track_frames[t] / kArTileMults + 2u) * otiles;  // an upper bound: the s450 span's included
        sums += 3u * width * d.ntracks;
        if (tiles >= (1ull << 31)) return "batch holds 2^31 tiles or more";
        if (sums >= (1ull << 31)) return "batch holds 2^31 sums or more";
    }
    return nullptr;
}

// Fills the tables at h (the tables' first byte, not the base's); in: the sources ar_layout saw, now with their addresses.
inline void ar_fill(const ArLayout& y, const ArSrcIn* in, const ArDiscIn* discs, size_t ndiscs, uint8_t* h) {
    auto* src = reinterpret_cast<ArSource*>(h + y.sources);
    size_t at = 0;
    for (size_t k = 0; k < ndiscs; ++k)
        for (uint32_t i = 0; i < discs[k].nsrc; ++i, ++at) {
            src[at] = y.src[at];
            src[at].data0 = in[discs[k].src0 + i].data0;
            src[at].data1 = in[discs[k].src0 + i].data1;
        }
    if (!y.span.empty()) std::memcpy(h + y.spans, y.span.data(), sizeof(ArSpan) * y.span.size());
    std::memcpy(h + y.tile_off, y.tiles.data(), 8 * y.tiles.size());
    std::memset(h + y.tile_off + 8 * y.tiles.size(), 0, y.size - (y.tile_off + 8 * y.tiles.size()));  // the padding and the sums
}

// The kernel's arguments: the tables at `tables` (where the kernel sees them).
inline ArArgs ar_args(const ArLayout& y, uint8_t* tables, unsigned long long* bad) {
    ArArgs a;
    a.nspans = (uint32_t)y.span.size();
    a.total_tiles = y.total_tiles;
    a.spans = reinterpret_cast<const ArSpan*>(tables + y.spans);
    a.tile_off = reinterpret_cast<const unsigned long long*>(tables + y.tile_off);
    a.sources = reinterpret_cast<const ArSource*>(tables + y.sources);
    a.sums = reinterpret_cast<uint32_t*>(tables + y.sums);
    a.bad = bad;
    return a;
}

// What the ABI gives back for disc k, from the sums as the device left them (at the tables' y.sums).
inline lacx_ar_result ar_result(const ArLayout& y, size_t k, uint32_t lba0, const uint64_t* track_frames) {
    const ArDiscAt& d = y.discs[k];
    lacx_ar_result r{};
    r.frames = d.frames, r.tracks = d.ntracks, r.radius = d.radius, r.flags = d.flags;
    if (!ar_ids(track_frames, d.ntracks, d.flags, lba0, r.ids)) r.flags |= LACX_AR_NO_IDS;
    return r;
}
inline void ar_tracks(const ArLayout& y, size_t k, const uint32_t* sums, std::vector<lacx_ar_track>& out) {
    const ArDiscAt& d = y.discs[k];
    const uint64_t width = 2ull * d.radius + 1u;
    out.resize(d.ntracks);
    for (uint32_t t = 0; t < d.ntracks; ++t) {
        const ArTrackAt& tr = y.tracks[d.track0 + t];
        const uint32_t* row = sums + d.sum0 + 3u * width * t + d.radius;
        out[t] = lacx_ar_track{tr.start, tr.frames, tr.flags, row[0], row[width], row[2u * width]};
    }
}

}  // namespace lacx
