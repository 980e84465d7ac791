// compare_core.h -- the per-thread code of the bit-compare job (k_compare_search and k_compare_rows of k_compare.hip): how
// two streams relate, in exact integers.  This file is the only statement of the definition in code (lacx.h and DESIGN §6b
// state it in words).
// A(f) = a[f] inside [0, na), 0 in every channel elsewhere; B likewise.  At offset o frame f of A is paired with frame f + o
// of B, over the union domain f in [min(0, -o), max(na, nb - o)).
//   search: mis[o] = the (frame, channel) samples of the domain with A(f)[c] != B(f + o)[c], for every o in [centre -
//           radius, centre + radius].  Outside the domain both sides are zero, so a sum over any superset of it is the same
//           number: the plan tiles the stretches of A's axis on which A or the B window can be non-zero (CmpSpan).
//   rows:   at the chosen offset the domain in rows of kCmpRowFrames frames from its first frame; per row and channel, with d
//           = A - B: the mismatches, the first and last differing frame, max |d| and its lowest position (positions counted
//           from the domain's first frame, kCmpNone where there is none), the sums of |d| and of d^2.
// Search: a workgroup takes a tile -- up to kCmpTileFrames frames of one span and 4 * lanes consecutive offsets from a
// multiple of 4 on (cmp_tile).  It stages A's frames and the B window as words: one word per frame for mono and for 16-bit
// stereo (both channels in one word, compared by halves), two planes of words for 24-bit stereo.  Thread tid owns the four
// offsets of lane tid % lanes and walks the quads of frames of its stripe tid / lanes (cmp_search_lane): four words of A (the
// same address in every lane of a stripe) and eight of B (consecutive across lanes) feed 16 comparisons.  A lane whose
// offsets lie outside the pair's range still reads inside the stage; its counts are not used.
// Everything is a count, a minimum, a maximum or an integer sum: no result depends on the order of evaluation, and the
// device, the CPU twin and a numpy restatement agree byte for byte, in any batch.
// Written like accuraterip_core.h: the same source compiles into the gfx950 kernels and into a host program the tests run
// under AddressSanitizer / UBSan (tests/native/sim_compare.cpp).
#pragma once
#include <cstdint>

#include "lacx.h"
#include "stats_core.h"

namespace lacx {

static_assert(sizeof(CmpSource) == 40 && sizeof(CmpPair) == 48 && sizeof(CmpSpan) == 32, "the plan lays the tables out by these sizes");
static_assert(sizeof(lacx_compare_row) == kCmpRowBytes && sizeof(lacx_compare_channel_row) * 2 == kCmpRowBytes, "the row");
static_assert(kCmpTileFrames % 4u == 0 && kCmpLaneOffsets == 4u && (kCmpThreads & (kCmpThreads - 1u)) == 0, "the tiling");
static_assert(kCmpRowFrames % 4u == 0 && kCmpNone == LACX_COMPARE_NONE, "rows");

LACX_HDF uint32_t cmp_planes(const CmpSource& s) { return s.channels == 2 && s.bit_depth == 24 ? 2u : 1u; }

// the staged word of one frame: plane 0 of one, or plane p of two
LACX_HDF uint32_t cmp_word(const CmpSource& s, int32_t l, int32_t r, uint32_t plane) {
    if (s.bit_depth == 16) return ((uint32_t)l & 0xFFFFu) | (s.channels == 2 ? (uint32_t)r << 16 : 0u);
    return plane ? (uint32_t)r : (uint32_t)l;
}

// The samples of frames g0 .. g0 + 3 of a source (g0 a multiple of 4, possibly negative), zeros outside it.  Where all four
// exist they are one stats_load_source of four frames; at the source's end, four loads of one frame.  note(item, key): an
// invalid sample of a validated source (key as stats_load_source).
template <typename Note>
LACX_HDF void cmp_load_unit(const CmpSource& s, long long g0, int32_t* l, int32_t* r, Note note) {
    l[0] = l[1] = l[2] = l[3] = 0;
    r[0] = r[1] = r[2] = r[3] = 0;
    if (g0 < 0 || g0 >= (long long)s.frames) return;  // (g0 a multiple of 4: g0 < 0 means all four are negative)
    unsigned long long key = kDigestClean;
    if ((unsigned long long)g0 + 4u <= s.frames) {
        stats_load_source((unsigned long long)g0, 4u, s.channels, s.bit_depth, s.data0, s.data1, s.layout, key, l, r);
    } else {
#pragma unroll
        for (uint32_t i = 0; i < 3u; ++i) {
            if ((unsigned long long)g0 + i >= s.frames) continue;
            int32_t sl[4] = {0, 0, 0, 0}, sr[4] = {0, 0, 0, 0};
            stats_load_source((unsigned long long)g0 + i, 1u, s.channels, s.bit_depth, s.data0, s.data1, s.layout, key, sl, sr);
            l[i] = sl[0], r[i] = sr[0];
        }
    }
    if (s.channels != 2) r[0] = r[1] = r[2] = r[3] = 0;
    if (s.validate && key != kDigestClean) note(s.item, key);
}

// The samples of frames g .. g + 3 for any g: the one or two units of four they lie in.  A negative g floors.
template <typename Note>
LACX_HDF void cmp_load_frames(const CmpSource& s, long long g, int32_t* l, int32_t* r, Note note) {
    const long long g0 = cmp_floor4(g);
    const uint32_t sh = (uint32_t)(g - g0);
    if (sh == 0) {
        cmp_load_unit(s, g0, l, r, note);
        return;
    }
    int32_t l8[8], r8[8];
    cmp_load_unit(s, g0, l8, r8, note);
    cmp_load_unit(s, g0 + 4, l8 + 4, r8 + 4, note);
#pragma unroll
    for (uint32_t i = 0; i < 4u; ++i) {  // (selects, not an index that varies: the arrays stay in registers)
        l[i] = sh == 1u ? l8[i + 1u] : sh == 2u ? l8[i + 2u] : l8[i + 3u];
        r[i] = sh == 1u ? r8[i + 1u] : sh == 2u ? r8[i + 2u] : r8[i + 3u];
    }
}

// Tile t of a span: frame tile t / offset tiles, offset tile t % offset tiles.
struct CmpTile {
    long long g0;      // A's frame of stage A's word 0, a multiple of 4
    uint32_t count;    // frames, a multiple of 4, <= kCmpTileFrames
    long long o0;      // the offset of lane 0's first: cmp_obase + a multiple of 4 * lanes
    long long b0;      // B's frame of stage B's word 0: g0 + o0, a multiple of 4
    uint32_t units_a, units_b;  // the units of four frames staged per plane
};
LACX_HDF CmpTile cmp_tile(const CmpSpan& s, const CmpPair& p, unsigned long long t) {
    CmpTile y;
    y.g0 = s.f_lo + (long long)(t / s.otiles) * (long long)kCmpTileFrames;
    const long long left = s.f_hi - y.g0;
    y.count = left < (long long)kCmpTileFrames ? (uint32_t)left : kCmpTileFrames;
    y.o0 = cmp_obase(p) + (long long)(t % s.otiles) * (long long)(kCmpLaneOffsets * s.lanes);
    y.b0 = y.g0 + y.o0;
    y.units_a = y.count / 4u;
    y.units_b = y.units_a + s.lanes;  // count + 4 lanes words: lane l reads words 4 q + 4 l .. + 7
    return y;
}
// Whether a tile has nothing to count: A's frames all lie outside A and the B window all outside B, so every word it would
// stage is zero.  (A span is long where the radius is: most of its tiles at most offsets are like this.)
LACX_HDF bool cmp_tile_empty(const CmpTile& y, unsigned long long na, unsigned long long nb) {
    const bool a_out = y.g0 >= (long long)na || y.g0 + (long long)y.count <= 0;
    const bool b_out = y.b0 >= (long long)nb || y.b0 + 4ll * (long long)y.units_b <= 0;
    return a_out && b_out;
}

// One staged unit: plane `plane` of frames g0 .. g0 + 3 of a source as words.
template <typename Note>
LACX_HDF void cmp_stage_unit(const CmpSource& s, long long g0, uint32_t nplanes, uint32_t* w0, uint32_t* w1, Note note) {
    int32_t l[4], r[4];
    cmp_load_unit(s, g0, l, r, note);
#pragma unroll
    for (uint32_t i = 0; i < 4u; ++i) {
        w0[i] = cmp_word(s, l[i], r[i], 0u);
        if (nplanes == 2u) w1[i] = cmp_word(s, l[i], r[i], 1u);
    }
}

// the samples in which two staged words differ: by halves (16 bit: a channel each) or whole (24 bit: the word is a sample)
template <bool kHalves>
LACX_HDF uint32_t cmp_differ(uint32_t a, uint32_t b) {
    const uint32_t x = a ^ b;
    if (kHalves) return ((x & 0xFFFFu) != 0u ? 1u : 0u) + ((x >> 16) != 0u ? 1u : 0u);
    return x != 0u ? 1u : 0u;
}

// Thread tid of a tile whose words are staged (one plane: a at the plane's A words, b at its B words): adds the mismatches
// of its four offsets y.o0 + 4 (tid % lanes) .. + 3 over its stripe of the tile's quads of frames to cnt[0 .. 3].
template <bool kHalves>
LACX_HDF void cmp_search_lane(const uint32_t* a, const uint32_t* b, const CmpSpan& s, const CmpTile& y, uint32_t tid, uint32_t* cnt) {
    const uint32_t lane = tid & (s.lanes - 1u), stripe = tid / s.lanes, stripes = kCmpThreads / s.lanes;
    const uint32_t* bl = b + 4u * lane;
    for (uint32_t q = stripe; q < y.units_a; q += stripes) {
        uint32_t av[4], bv[8];
        __builtin_memcpy(av, __builtin_assume_aligned(a + 4u * q, 16), 16);
        __builtin_memcpy(bv, __builtin_assume_aligned(bl + 4u * q, 16), 32);
#pragma unroll
        for (uint32_t j = 0; j < 4u; ++j)
#pragma unroll
            for (uint32_t i = 0; i < 4u; ++i) cnt[j] += cmp_differ<kHalves>(av[i], bv[i + j]);
    }
}

// ---- rows ----
LACX_HDF void cmp_row_clear(lacx_compare_channel_row& c) {
    c.first = c.last = c.max_at = kCmpNone;
    c.sum_abs = c.sum_sq = 0;
    c.mismatches = c.max_abs = 0;
}

// a += b; b's frames may lie before or behind a's
LACX_HDF void cmp_row_merge(lacx_compare_channel_row& a, const lacx_compare_channel_row& b) {
    if (b.mismatches == 0) return;
    if (a.mismatches == 0) {
        a = b;
        return;
    }
    a.first = b.first < a.first ? b.first : a.first;
    a.last = b.last > a.last ? b.last : a.last;
    if (b.max_abs > a.max_abs || (b.max_abs == a.max_abs && b.max_at < a.max_at)) a.max_abs = b.max_abs, a.max_at = b.max_at;
    a.sum_abs += b.sum_abs;
    a.sum_sq += b.sum_sq;
    a.mismatches += b.mismatches;
}

// one sample pair at domain position pos; positions arrive ascending within a thread
LACX_HDF void cmp_row_sample(lacx_compare_channel_row& c, unsigned long long pos, int32_t x, int32_t y) {
    if (x == y) return;
    const int32_t d = x - y;  // |d| < 2^25
    const uint32_t m = (uint32_t)(d < 0 ? -d : d);
    if (c.mismatches == 0) c.first = pos;
    c.last = pos;
    if (m > c.max_abs) c.max_abs = m, c.max_at = pos;
    c.sum_abs += m;
    c.sum_sq += (unsigned long long)m * m;
    ++c.mismatches;
}

// the frames [start, end) on A's axis of row `row` of a pair at its chosen offset
LACX_HDF void cmp_row_range(const CmpPair& p, unsigned long long na, unsigned long long nb, unsigned long long row, long long& start, long long& end) {
    const long long dom0 = cmp_fmin(p.chosen), dom1 = cmp_fmax(na, nb, p.chosen);
    start = dom0 + (long long)(row * kCmpRowFrames);
    end = dom1 - start > (long long)kCmpRowFrames ? start + (long long)kCmpRowFrames : dom1;
}

// Thread tid of the workgroup that makes row `row` of a pair: its share of the row -- A's units of four from the one that
// holds the row's first frame on, every kCmpThreads-th -- into acc[0 .. 1], which it clears first.  A's units are aligned;
// B's frames f + o are not where o mod 4 != 0 (cmp_load_frames).
template <typename Note>
LACX_HDF void cmp_row_thread(const CmpSource* sources, const CmpPair& p, unsigned long long row, uint32_t tid, lacx_compare_channel_row* acc, Note note) {
    const CmpSource& a = sources[p.a];
    const CmpSource& b = sources[p.b];
    cmp_row_clear(acc[0]);
    cmp_row_clear(acc[1]);
    long long start, end;
    cmp_row_range(p, a.frames, b.frames, row, start, end);
    const long long dom0 = cmp_fmin(p.chosen), u0 = cmp_floor4(start);
    for (long long g = u0 + 4ll * (long long)tid; g < end; g += 4ll * (long long)kCmpThreads) {
        int32_t al[4], ar[4], bl[4], br[4];
        cmp_load_unit(a, g, al, ar, note);
        cmp_load_frames(b, g + p.chosen, bl, br, note);
#pragma unroll
        for (uint32_t i = 0; i < 4u; ++i) {
            const long long f = g + (long long)i;
            if (f < start || f >= end) continue;
            const unsigned long long pos = (unsigned long long)(f - dom0);
            cmp_row_sample(acc[0], pos, al[i], bl[i]);
            if (a.channels == 2) cmp_row_sample(acc[1], pos, ar[i], br[i]);
        }
    }
}

}  // namespace lacx
