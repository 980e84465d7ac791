// truepeak_core.h -- the per-thread code of the true-peak job (k_truepeak of k_truepeak.hip): the maximum of the 4x
// oversampled signal of ITU-R BS.1770-4 Annex 2 over the final samples of an item, in exact integers.  This file is the
// only statement of the definition in code (lacx.h and DESIGN §6b state it in words).
// The Annex 2 interpolator is a 48-tap FIR in four phases of 12 taps; every coefficient of its table is a whole multiple of
// 2^-13, so 8192 times the oversampled signal of integer PCM is an integer:
//   y[4n + p] = sum over k of c[p][k] * x[n - k],   n = 0 .. frames + 10,   x = 0 outside [0, frames)
// and |y| <= 16571 * 2^(b-1) at bit depth b.  Integer sums and integer maxima do not depend on the order of evaluation:
// the device, the CPU twin and a numpy restatement agree bit for bit, in any batch and at any place in a job.
// A workgroup takes a tile of kTpTileFrames outputs-frames n, a thread four of them: it loads frames n0 .. n0 + 3 as one
// unit through stats_load_source (every PCM layout, its bounds and its validation keys), the tile's first three threads
// also the three units in front of the tile, and after the tile is staged every thread reads the 16 staged samples
// x[n0 - 12 .. n0 + 3] and evaluates 4 frames x 4 phases x 12 taps (tp_channel).  Samples in front of frame 0 and behind
// the item's last frame are zeros, never a neighbour's PCM.
// Arithmetic.  Depth 16: |x| <= 2^15 and the sums stay below 16571 * 2^15 < 2^31: 32-bit sums.  Depth 24: the sums reach
// 16571 * 2^23 > 2^31, so the sample is split x = xh * 4096 + xl (xl = x & 4095 in [0, 4096), xh = x >> 12 in [-2048, 2048)),
// the two sums stay below 16571 * 2^12 < 2^27 each, and y = hi * 4096 + lo in 64 bits.  Every factor of either path -- the
// samples of depth 16, both halves of depth 24, every coefficient (|c| <= 7964) -- fits 16 bits signed, so two taps are one
// 16-bit dot product with a 32-bit accumulator (tp_dot2: v_dot2c_i32_i16 on the device, the same sum on the host): six per
// output at depth 16, twelve at depth 24, over neighbouring samples packed in pairs once per thread -- no 64-bit multiply-add
// anywhere.  The sums are formed in unsigned words and a factor is cut to its low 16 bits on both sides: a sample that is no
// sample of the depth (the item then fails and has no rows) overflows nothing and gives the same bits everywhere.
// Per (tile, channel) the result is one packed key, peak << kTpPosBits | (2^kTpPosBits - 1 - pos): its maximum is the
// largest peak at the lowest position.  A zero peak has no key (key 0: the empty row).
// Written like stats_core.h: the same source compiles into the gfx950 kernel and into a host program the tests run under
// AddressSanitizer / UBSan (tests/native/sim_truepeak.cpp).
#pragma once
#include <cstdint>

#include "lacx.h"
#include "stats_core.h"

namespace lacx {

// the BS.1770-4 Annex 2 table times 8192; phases 2 and 3 are phases 1 and 0 reversed
LACX_HDF constexpr int32_t tp_coef(uint32_t p, uint32_t k) {
    constexpr int32_t c0[kTpTaps] = {14, 90, -161, 272, -487, 1125, 7964, -838, 390, -218, 122, -68};
    constexpr int32_t c1[kTpTaps] = {-239, 240, -424, 730, -1364, 3810, 6388, -1641, 832, -477, 271, -155};
    return p == 0 ? c0[k] : p == 1 ? c1[k] : p == 2 ? c1[kTpTaps - 1u - k] : c0[kTpTaps - 1u - k];
}
constexpr int32_t kTpPeakGain = 16571;  // the largest sum of magnitudes of a phase: |y| <= kTpPeakGain * 2^(b-1)
constexpr int32_t kTpUnity = 8192;      // y / kTpUnity is the oversampled signal in sample units

namespace tp_detail {
constexpr int32_t phase_sum(uint32_t p, bool magnitudes) {
    int32_t s = 0;
    for (uint32_t k = 0; k < kTpTaps; ++k) s += magnitudes && tp_coef(p, k) < 0 ? -tp_coef(p, k) : tp_coef(p, k);
    return s;
}
static_assert(phase_sum(0, false) == 8205 && phase_sum(1, false) == 7971 && phase_sum(2, false) == 7971 && phase_sum(3, false) == 8205, "the table's sums");
static_assert(phase_sum(0, true) == 11749 && phase_sum(1, true) == kTpPeakGain && phase_sum(2, true) == kTpPeakGain && phase_sum(3, true) == 11749,
              "the table's sums of magnitudes");
static_assert((long long)kTpPeakGain << 15 < 1ll << 31, "depth 16 stays inside 32 bits");
static_assert((long long)kTpPeakGain << 12 < 1ll << 27, "both halves of the depth-24 split stay inside 32 bits");
static_assert(4ull * (kTpRowFrames + kTpFlush) <= 1ull << kTpPosBits && 38u + kTpPosBits <= 64u, "the packed key: 16571 * 2^23 < 2^38");
static_assert(kTpTileFrames == 4u * kTpThreads && kTpRowFrames % kTpTileFrames == 0 && kTpHistory % 4u == 0 && kTpHistory >= kTpFlush, "the tiling");
}  // namespace tp_detail

static_assert(sizeof(TpAcc) == 32 && sizeof(lacx_truepeak_row) == 32, "the plan lays the rows out 32 bytes apart");

// two 16-bit values as one word: lo in bits 0 .. 15, hi in bits 16 .. 31
LACX_HDF constexpr uint32_t tp_pack(int32_t lo, int32_t hi) { return ((uint32_t)lo & 0xFFFFu) | ((uint32_t)hi << 16); }
// taps 2m and 2m + 1 of phase p, packed
LACX_HDF constexpr uint32_t tp_coef2(uint32_t p, uint32_t m) { return tp_pack(tp_coef(p, 2u * m), tp_coef(p, 2u * m + 1u)); }
// acc + a.lo * b.lo + a.hi * b.hi, the halves as signed 16-bit values, in 32 bits without saturation
LACX_HDF uint32_t tp_dot2(uint32_t a, uint32_t b, uint32_t acc) {
#if defined(__HIP_DEVICE_COMPILE__)
    typedef short tp_short2 __attribute__((ext_vector_type(2)));
    tp_short2 va, vb;
    __builtin_memcpy(&va, &a, 4);
    __builtin_memcpy(&vb, &b, 4);
    return (uint32_t)__builtin_amdgcn_sdot2(va, vb, (int)acc, false);
#else
    const int32_t lo = (int32_t)(int16_t)(uint16_t)(a & 0xFFFFu) * (int32_t)(int16_t)(uint16_t)(b & 0xFFFFu);
    const int32_t hi = (int32_t)(int16_t)(uint16_t)(a >> 16) * (int32_t)(int16_t)(uint16_t)(b >> 16);
    return acc + (uint32_t)lo + (uint32_t)hi;
#endif
}

LACX_HDF uint32_t tp_abs(int32_t x) { return x < 0 ? 0u - (uint32_t)x : (uint32_t)x; }

// Frames f0 .. f0 + 3 of the item (f0 a multiple of 4), zeros where the item has none; key as stats_load_source.
LACX_HDF void tp_load_unit(const TpItem& it, unsigned long long f0, unsigned long long& key, int32_t* l, int32_t* r) {
#pragma unroll
    for (uint32_t i = 0; i < 4u; ++i) l[i] = 0, r[i] = 0;
    if (f0 >= it.frames) return;
    const uint32_t nf = it.frames - f0 >= 4u ? 4u : (uint32_t)(it.frames - f0);
    stats_load_source(f0, nf, it.channels, it.bit_depth, it.data0, it.data1, it.layout, key, l, r);
}

// The row all of a tile's outputs belong to.  Output n belongs to segment min(n, frames - 1) / kTpRowFrames; a tile is
// aligned to kTpTileFrames, which divides kTpRowFrames, so its outputs in front of `frames` share one segment, and its
// outputs from `frames` on (the flush tail) belong to the segment of frame frames - 1: one row per tile.
LACX_HDF uint32_t tp_tile_row(unsigned long long tile_start, unsigned long long frames) {
    return (uint32_t)((tile_start < frames ? tile_start : frames - 1u) / kTpRowFrames);
}

// One channel of one thread.  w[j] = x[n0 - 12 + j], j = 0 .. 15; pos0 = 4 * (n0 - the row's first frame).  The key of the
// largest |y[4 (n0 + i) + p]|, i < 4, at its lowest position; 0 where they are all zero.  (An output behind frames + 10
// sees twelve zeros and is zero: nothing needs masking.)
template <bool kDeep>
LACX_HDF unsigned long long tp_channel(const int32_t* w, uint32_t pos0) {
    // q[j] = (w[j + 1], w[j]): taps 2m and 2m + 1 of output frame i read x[n0 + i - 2m] and the sample in front of it, q[11 + i - 2m]
    [[maybe_unused]] uint32_t ql[15], qh[15];
#pragma unroll
    for (uint32_t j = 1; j < 15u; ++j) {
        if constexpr (kDeep) {
            ql[j] = tp_pack(w[j + 1u] & 4095, w[j] & 4095);
            qh[j] = tp_pack(w[j + 1u] >> 12, w[j] >> 12);
        } else {
            ql[j] = tp_pack(w[j + 1u], w[j]);
        }
    }
    unsigned long long best = 0;
    uint32_t at = 0;
#pragma unroll
    for (uint32_t i = 0; i < 4u; ++i) {
#pragma unroll
        for (uint32_t p = 0; p < kTpPhases; ++p) {
            unsigned long long mag;
            uint32_t lo = 0, hi = 0;
#pragma unroll
            for (uint32_t m = 0; m < kTpTaps / 2u; ++m) {
                lo = tp_dot2(ql[11u + i - 2u * m], tp_coef2(p, m), lo);
                if constexpr (kDeep) hi = tp_dot2(qh[11u + i - 2u * m], tp_coef2(p, m), hi);
            }
            if constexpr (kDeep) {
                const long long y = (long long)(int32_t)hi * 4096 + (long long)(int32_t)lo;
                mag = (unsigned long long)(y < 0 ? -y : y);
            } else {
                mag = tp_abs((int32_t)lo);
            }
            if (mag > best) best = mag, at = 4u * i + p;  // in position order: the lowest position of the largest
        }
    }
    const unsigned long long mask = (1ull << kTpPosBits) - 1u;
    return best ? (best << kTpPosBits) | (mask - ((pos0 + at) & mask)) : 0ull;
}

// A thread's part of its tile's row: both channels' keys and the largest |x| of its own four frames.
struct TpLane {
    unsigned long long key[2];
    uint32_t sample_peak[2];
};
LACX_HDF void tp_merge(TpLane& a, const TpLane& b) {
#pragma unroll
    for (uint32_t c = 0; c < 2u; ++c) {
        a.key[c] = a.key[c] > b.key[c] ? a.key[c] : b.key[c];
        a.sample_peak[c] = stats_umax(a.sample_peak[c], b.sample_peak[c]);
    }
}

// wl / wr: the thread's 16 staged samples per channel (wr unused for mono); l / r: its own unit as loaded.
LACX_HDF TpLane tp_lane(const int32_t* wl, const int32_t* wr, const int32_t* l, const int32_t* r, bool stereo, bool deep, uint32_t pos0) {
    TpLane t{{0, 0}, {0, 0}};
    t.key[0] = deep ? tp_channel<true>(wl, pos0) : tp_channel<false>(wl, pos0);
    if (stereo) t.key[1] = deep ? tp_channel<true>(wr, pos0) : tp_channel<false>(wr, pos0);
#pragma unroll
    for (uint32_t i = 0; i < 4u; ++i) {
        t.sample_peak[0] = stats_umax(t.sample_peak[0], tp_abs(l[i]));
        if (stereo) t.sample_peak[1] = stats_umax(t.sample_peak[1], tp_abs(r[i]));
    }
    return t;
}

}  // namespace lacx
