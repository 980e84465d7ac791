// accuraterip_core.h -- the per-thread code of the rip-checksum job (k_accuraterip of k_accuraterip.hip): the AccurateRip
// v1 / v2 track checksums and the 450th-sector sum of a disc of 16-bit stereo audio at every read offset within a radius, in
// exact integers.  This file is the only statement of the definition in code (lacx.h and DESIGN §6b state it in words).
// A disc is D frames; frame j is the word w[j] = (uint16)left[j] | (uint16)right[j] << 16 and x(j) = w[j] inside [0, D), 0
// elsewhere.  A span asks for
//   lo[o] = sum over m = m_lo .. m_hi of lo32(m * x(frame1 + o + m - 1))      (v1, s450)
//   hi[o] = sum over the same m       of hi32(m * x(frame1 + o + m - 1))      (v2 = lo + hi)
// for every offset o in [-radius, radius], all mod 2^32; m * x is the 64-bit product of two 32-bit words.  The sum of the
// high halves has no shortcut through prefix sums: every (multiplier, offset) pair is one multiply.  Sums mod 2^32 do not
// depend on the order of evaluation: the device, the CPU twin and a numpy restatement agree bit for bit, in any batch.
// A workgroup takes a tile: up to kArTileMults multipliers of one span and `lanes` consecutive offsets.  It stages the
// count + lanes - 1 words the tile reads (ar_load_unit: units of four disc frames through stats_load_source -- every PCM
// layout, its bounds and its validation keys -- mapped to (source, frame) through the disc's source table, zeros outside the
// disc); then thread tid owns offset tid % lanes and walks the multipliers m0 + tid / lanes, + kArThreads / lanes, ...
// (ar_lane): consecutive threads read consecutive staged words.  Below a full workgroup of offsets the stripes share the
// multiplier range, so that no lane idles at a small radius; the kernel adds the stripes' parts before its atomics.
// The product: (uint64)m * x in plain C++, which the compiler makes one v_mad_u64_u32 of, and two 32-bit adds.
// Written like stats_core.h: the same source compiles into the gfx950 kernel and into a host program the tests run under
// AddressSanitizer / UBSan (tests/native/sim_accuraterip.cpp).
#pragma once
#include <cstdint>

#include "lacx.h"
#include "stats_core.h"

namespace lacx {

static_assert(sizeof(ArSource) == 40 && sizeof(ArSpan) == 48, "the plan lays the tables out by these sizes");
static_assert(kArStageWords % 4u == 0 && kArStageWords >= 3u + kArTileMults + kArThreads - 1u, "a tile's words fit the stage");
static_assert((kArThreads & (kArThreads - 1u)) == 0 && 2u * kArMaxRadius + 1u == 10u * kArSector - 1u, "the tiling");

// the disc's word of one frame
LACX_HDF uint32_t ar_word(int32_t l, int32_t r) { return ((uint32_t)l & 0xFFFFu) | ((uint32_t)r << 16); }

// one (multiplier, offset) pair
LACX_HDF void ar_add(uint32_t m, uint32_t x, uint32_t& lo, uint32_t& hi) {
    const unsigned long long p = (unsigned long long)m * x;
    lo += (uint32_t)p;
    hi += (uint32_t)(p >> 32);
}

// Tile t of a span: multiplier tile t / offset tiles, offset tile t % offset tiles.
struct ArTile {
    uint32_t m0, count;  // the multipliers m0 .. m0 + count - 1
    uint32_t o0;         // the tile's first offset is o0 - radius
    long long first;     // the disc frame of stage[0]: the multiple of 4 at or below the first frame the tile reads
    uint32_t pad, units; // stage[pad] is that first frame; the units of four frames the tile stages
};
LACX_HDF ArTile ar_tile(const ArSpan& s, unsigned long long t) {
    const uint32_t ot = ar_offset_tiles(s);
    ArTile y;
    y.o0 = (uint32_t)(t % ot) * s.lanes;
    y.m0 = s.m_lo + (uint32_t)(t / ot) * kArTileMults;
    const uint32_t left = s.m_hi - y.m0;  // + 1 multipliers are left
    y.count = left < kArTileMults ? left + 1u : kArTileMults;
    const long long g = (long long)s.frame1 + (long long)y.m0 - 1 + (long long)y.o0 - (long long)s.radius;
    y.first = g & ~3ll;  // (floors a negative frame too)
    y.pad = (uint32_t)(g - y.first);
    y.units = (y.pad + y.count + s.lanes - 1u + 3u) / 4u;
    return y;
}

// the source that holds disc frame g < disc_frames: the last whose start is at or below g
LACX_HDF uint32_t ar_source_of(const ArSource* src, uint32_t n, unsigned long long g) {
    uint32_t k = 0, hi = n;
    while (hi - k > 1u) {
        const uint32_t mid = k + (hi - k) / 2u;
        if (src[mid].start <= g) k = mid;
        else hi = mid;
    }
    return k;
}

// The words of disc frames g0 .. g0 + 3 (g0 a multiple of 4, possibly negative), zeros outside the disc.  Where the four
// frames are one aligned unit of one source they are one stats_load_source of four frames; across a source seam, at a
// source whose start is no multiple of 4 and at the disc's ends, four loads of one frame.  note(item, key): an invalid
// sample of a validated source (key as stats_load_source).
template <typename Note>
LACX_HDF void ar_load_unit(const ArSpan& s, const ArSource* sources, long long g0, uint32_t* w, Note note) {
    w[0] = w[1] = w[2] = w[3] = 0u;
    if (g0 + 3 < 0 || g0 >= (long long)s.disc_frames) return;
    const ArSource* src = sources + s.src0;
    if (g0 >= 0) {
        const ArSource& a = src[ar_source_of(src, s.nsrc, (unsigned long long)g0)];
        const unsigned long long f0 = (unsigned long long)g0 - a.start;
        if ((f0 & 3u) == 0 && f0 + 4u <= a.frames) {
            unsigned long long key = kDigestClean;
            int32_t l[4] = {0, 0, 0, 0}, r[4] = {0, 0, 0, 0};
            stats_load_source(f0, 4u, 2, 16, a.data0, a.data1, a.layout, key, l, r);
#pragma unroll
            for (uint32_t i = 0; i < 4u; ++i) w[i] = ar_word(l[i], r[i]);
            if (s.validate && key != kDigestClean) note(a.item, key);
            return;
        }
    }
#pragma unroll
    for (uint32_t i = 0; i < 4u; ++i) {
        const long long g = g0 + (long long)i;
        if (g < 0 || g >= (long long)s.disc_frames) continue;
        const ArSource& a = src[ar_source_of(src, s.nsrc, (unsigned long long)g)];
        unsigned long long key = kDigestClean;
        int32_t l[4] = {0, 0, 0, 0}, r[4] = {0, 0, 0, 0};
        stats_load_source((unsigned long long)g - a.start, 1u, 2, 16, a.data0, a.data1, a.layout, key, l, r);
        w[i] = ar_word(l[0], r[0]);
        if (s.validate && key != kDigestClean) note(a.item, key);
    }
}

// Thread tid of a tile whose words are staged: the sums of its offset (y.o0 + tid % lanes - radius) over its stripe of the
// tile's multipliers.  A thread whose offset lies behind the span's last still reads inside the stage; its sums are not used.
LACX_HDF void ar_lane(const uint32_t* stage, const ArSpan& s, const ArTile& y, uint32_t tid, uint32_t& lo, uint32_t& hi) {
    const uint32_t stripe = tid / s.lanes, stripes = kArThreads / s.lanes;
    const uint32_t* at = stage + y.pad + (tid & (s.lanes - 1u));
    lo = hi = 0u;
    if (s.lanes == kArThreads) {  // every thread an offset (radius >= 128, where the work is): the multiplier and the trip count are
                                  // the same in all lanes -- eight pairs per turn, the reads at constant distances
        uint32_t k = 0;
        for (; k + 8u <= y.count; k += 8u) {
#pragma unroll
            for (uint32_t i = 0; i < 8u; ++i) ar_add(y.m0 + k + i, at[k + i], lo, hi);
        }
        for (; k < y.count; ++k) ar_add(y.m0 + k, at[k], lo, hi);
        return;
    }
    for (uint32_t k = stripe; k < y.count; k += stripes) ar_add(y.m0 + k, at[k], lo, hi);
}

}  // namespace lacx
