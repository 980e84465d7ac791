// loudness_core.h -- the per-thread code of the loudness job (k_loud_states, k_loud_carry, k_loud_energy, k_loud_rows of
// k_loudness.hip): the K-weighting of ITU-R BS.1770 over the final samples of an item, as a blocked linear recurrence.
// The filter is a serial chain over the whole stream.  It is linear, so the state behind a chunk of kLoudChunk frames
// that starts in state s is A s + f, with f the state the chunk reaches from zero and A the map of kLoudChunk zero-input
// steps.  That cuts the chain into independent pieces:
//   1  loud_chunk_states   every chunk from zero state: its final state f[c]
//   2  loud_carry_lane     per (item, channel), serially: s[0] = 0, s[c + 1] = A s[c] + f[c]  (loud_carry_step); s[c]
//                          takes f[c]'s place
//   3  loud_chunk_energy   every chunk again from s[c]: the squares of the high-pass output, summed in frame order into
//                          the chunk's two partial sums -- the frames in the sub-block of its first frame, and the frames
//                          in the next (a sub-block is fs / 10 >= 4410 frames, so a chunk touches at most two); a piece
//                          without frames is +0.0
//   4  loud_row            per (item, sub-block, channel): the partials that fall into the sub-block, added in chunk order
// This file is the definition of every operation and its order.  The two biquads are in transposed direct form II, the
// shelf feeding the high-pass; every multiply-add below that is fused is written as an fma and nothing else may be fused:
// the kernel's translation unit and the CPU twin are compiled with -ffp-contract=off.  There are no floating-point
// atomics.  With IEEE add, multiply and fma on both sides a row is the same bits on the device and on the host, from run
// to run, in any batch and at any place in a job.
// Samples come through stats_load_source: a unit of four frames of PCM in any layout -- the decoder's planar int32 staging
// as k_ms_inverse left it is the planar int32 layout -- with its loads, bounds and validation keys.  Every frame of the
// item is loaded and validated; only the frames in front of LoudItem::used (the complete sub-blocks) are filtered.
// Written like stats_core.h: the same source compiles into the gfx950 kernels and into a host program the tests run under
// AddressSanitizer / UBSan (tests/native/sim_loudness.cpp).
#pragma once
#include <cstdint>

#include "lacx.h"
#include "stats_core.h"

namespace lacx {

static_assert(sizeof(LoudState) == 32 && sizeof(LoudPartial) == 16 && sizeof(lacx_loudness_row) == 16, "the plan's scratch sizes");

// one frame of one channel through both biquads: the high-pass output
LACX_HDF double loud_step(const LoudFilter& k, LoudState& st, double x) {
    const double y = __builtin_fma(k.sb[0], x, st.s[0]);
    st.s[0] = __builtin_fma(k.sb[1], x, __builtin_fma(k.sna[0], y, st.s[1]));
    st.s[1] = __builtin_fma(k.sb[2], x, k.sna[1] * y);
    const double z = __builtin_fma(k.hb[0], y, st.s[2]);
    st.s[2] = __builtin_fma(k.hb[1], y, __builtin_fma(k.hna[0], z, st.s[3]));
    st.s[3] = __builtin_fma(k.hb[2], y, k.hna[1] * z);
    return z;
}

// s = A s + f, every row from its last column to its first
LACX_HDF void loud_carry_step(const LoudFilter& k, LoudState& s, const LoudState& f) {
    LoudState n;
#pragma unroll
    for (int i = 0; i < 4; ++i)
        n.s[i] = __builtin_fma(k.A[i][0], s.s[0], __builtin_fma(k.A[i][1], s.s[1], __builtin_fma(k.A[i][2], s.s[2], __builtin_fma(k.A[i][3], s.s[3], f.s[i]))));
    s = n;
}

// Walks chunk c of the item unit by unit: fn(frame, left, right) for every frame in front of `used`, in frame order.  The
// frames behind `used` are loaded too (validated, not filtered).  key: the lowest invalid sample's key (digest_bad_key).
template <typename Fn>
LACX_HDF void loud_walk(const LoudItem& it, uint32_t c, unsigned long long& key, Fn fn) {
    const unsigned long long first = (unsigned long long)kLoudChunk * c;
    const unsigned long long end = it.frames - first >= kLoudChunk ? first + kLoudChunk : it.frames;
    for (unsigned long long f0 = first; f0 < end; f0 += 4u) {
        const uint32_t nf = it.frames - f0 >= 4u ? 4u : (uint32_t)(it.frames - f0);
        int32_t l[4] = {0, 0, 0, 0}, r[4] = {0, 0, 0, 0};
        stats_load_source(f0, nf, it.channels, it.bit_depth, it.data0, it.data1, it.layout, key, l, r);
#pragma unroll
        for (uint32_t i = 0; i < 4u; ++i)
            if (i < nf && f0 + i < it.used) fn(f0 + i, l[i], r[i]);
    }
}

// Pass 1.  out[channel] = the state chunk c reaches from zero (both channels of a stereo item in one walk).
LACX_HDF void loud_chunk_states(const LoudFilter& k, const LoudItem& it, uint32_t c, LoudState* out, unsigned long long& key) {
    const bool stereo = it.channels == 2;
    LoudState a{{0.0, 0.0, 0.0, 0.0}}, b = a;
    loud_walk(it, c, key, [&](unsigned long long, int32_t l, int32_t r) {
        (void)loud_step(k, a, (double)l);
        if (stereo) (void)loud_step(k, b, (double)r);
    });
    out[0] = a;
    if (stereo) out[1] = b;
}

// Pass 2.  Per (item, channel), serially: st = the item's records, `channels` apart per chunk.
// (The kernel takes the same steps in the same order with a whole wave, which fetches 64 chunks' f at once: k_loud_carry.)
LACX_HDF void loud_carry_lane(const LoudFilter& k, LoudState* st, uint32_t chunks, uint32_t channels, uint32_t channel) {
    LoudState s{{0.0, 0.0, 0.0, 0.0}};
    for (uint32_t c = 0; c < chunks; ++c) {
        LoudState* at = st + (unsigned long long)c * channels + channel;
        const LoudState f = *at;
        *at = s;
        loud_carry_step(k, s, f);
    }
}

// Pass 3.  start[channel] = s[c]; out[channel] = the chunk's two partial sums.
LACX_HDF void loud_chunk_energy(const LoudFilter& k, const LoudItem& it, uint32_t c, const LoudState* start, LoudPartial* out) {
    const bool stereo = it.channels == 2;
    LoudState a = start[0], b = stereo ? start[1] : LoudState{{0.0, 0.0, 0.0, 0.0}};
    // frames from here on lie in the sub-block behind that of the chunk's first frame
    const unsigned long long split = ((unsigned long long)kLoudChunk * c / it.sub + 1u) * it.sub;
    double pa0 = 0.0, pa1 = 0.0, pb0 = 0.0, pb1 = 0.0;
    unsigned long long key = kDigestClean;  // (pass 1 reported it)
    loud_walk(it, c, key, [&](unsigned long long f, int32_t l, int32_t r) {
        const double za = loud_step(k, a, (double)l);
        if (f < split) pa0 = __builtin_fma(za, za, pa0);
        else pa1 = __builtin_fma(za, za, pa1);
        if (stereo) {
            const double zb = loud_step(k, b, (double)r);
            if (f < split) pb0 = __builtin_fma(zb, zb, pb0);
            else pb1 = __builtin_fma(zb, zb, pb1);
        }
    });
    out[0] = LoudPartial{{pa0, pa1}};
    if (stereo) out[1] = LoudPartial{{pb0, pb1}};
}

// Pass 4.  Entry (s, channel) of the item's rows: parts = the item's records.  The chunk that holds the sub-block's first
// frame gives its second partial where it began in the sub-block in front (it straddles), else its first; every later
// chunk up to the one that holds the sub-block's last frame gives its first.
LACX_HDF double loud_row(const LoudPartial* parts, uint32_t channels, uint32_t channel, uint32_t sub, uint32_t s) {
    const unsigned long long a = (unsigned long long)s * sub, b = a + sub - 1u;
    const unsigned long long c0 = a / kLoudChunk, c1 = b / kLoudChunk;
    double e = parts[c0 * channels + channel].p[a % kLoudChunk != 0u ? 1 : 0];
    for (unsigned long long c = c0 + 1u; c <= c1; ++c) e = e + parts[c * channels + channel].p[0];
    return e;
}

}  // namespace lacx
