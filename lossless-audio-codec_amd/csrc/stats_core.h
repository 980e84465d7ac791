// stats_core.h -- the per-thread code of the audio statistics (k_stats_blocks of k_stats.hip): per BLOCK of a stream, or per
// block_frames frames of device-resident source PCM, and per channel the minimum, maximum, OR of the samples' bits, the
// counts of full-scale and of zero samples, the sum and the sum of squares; per block the leading and trailing frames that
// are zero in every channel and the frames whose channels differ.  All of it exact integer arithmetic.
// A thread takes one unit of four frames, as in blockdigest_core.h: a unit spans at most two blocks, so it yields one
// partial record, or two, each for the block it belongs to; a frame's place inside its block is part of the record (the
// lead / trail fields).
// Stream form: the samples are read AFTER k_ms_inverse ran in place and the range check is final, with the loads and the
// frame_off / present / status rules of block_unit_decoded: a block counts when it had a lane (index < present) and its
// status is 0.
// Source form: the loads, bounds and validation keys are digest_unit_source's own -- the unit is loaded once (no byte
// outside [0, frames * block_align) of an interleaved source, no element outside [0, frames) of a planar array, the partial
// last unit element by element) and split at the grid; an invalid sample lowers the item's key exactly as there.
//
// A record (StatsAcc) is also the device's accumulator row of a block.  Every field's identity is all-zero bytes, so a
// zeroed row is an empty one and nobody initialises rows but with zeros:
//   min_enc = 2^23 - min, max_enc = max + 2^23 + 1   both grow (a maximum), both are >= 1 once a sample was seen
//   first_nz = frames from the block's first non-zero frame to the block's end, last_nz = frames from the block's start
//   to its last non-zero frame, inclusive           both a maximum, 0: no non-zero frame
//   or_bits an OR; full_scale, zeros, differing, sum (two's complement), sum_sq sums
// Every combination is an integer max / or / add: the result does not depend on the order in which records arrive.
// Written like blockdigest_core.h: the same source compiles into the gfx950 kernel and into a host program the tests run
// under AddressSanitizer / UBSan (tests/native/sim_stats.cpp).
#pragma once
#include <cstdint>

#include "digest_core.h"

namespace lacx {

constexpr uint32_t kStatsBias = 0x800000u;  // 2^23: samples of either depth lie in [-2^23, 2^23)

struct StatsChan {  // 40 bytes
    uint32_t min_enc, max_enc, or_bits, full_scale, zeros, pad;
    unsigned long long sum, sum_sq;
};
struct alignas(8) StatsAcc {  // 96 bytes: a unit's partial record, a wave's, and the device row of a global block
    uint32_t first_nz, last_nz, differing, pad;
    StatsChan ch[2];
};
static_assert(sizeof(StatsChan) == 40 && sizeof(StatsAcc) == 96, "the device rows are 96 bytes apart");

struct StatsUnit {
    uint32_t b0;       // the block of the unit's first frame, counted in the item
    uint32_t n0, n1;   // frames of the unit in block b0 and in b0 + 1 (n1 == 0: the unit lies in one block)
    bool use0, use1;   // the block counts (stream form: it decoded)
    StatsAcc p0, p1;
};

LACX_HDF uint32_t stats_umax(uint32_t a, uint32_t b) { return a > b ? a : b; }

// a += b, field by field (the one combination there is: lanes, waves, workgroups and rows all use it)
LACX_HDF void stats_chan_merge(StatsChan& a, const StatsChan& b) {
    a.min_enc = stats_umax(a.min_enc, b.min_enc);
    a.max_enc = stats_umax(a.max_enc, b.max_enc);
    a.or_bits |= b.or_bits;
    a.full_scale += b.full_scale;
    a.zeros += b.zeros;
    a.sum += b.sum;
    a.sum_sq += b.sum_sq;
}
LACX_HDF void stats_merge(StatsAcc& a, const StatsAcc& b, bool stereo) {
    a.first_nz = stats_umax(a.first_nz, b.first_nz);
    a.last_nz = stats_umax(a.last_nz, b.last_nz);
    a.differing += b.differing;
    stats_chan_merge(a.ch[0], b.ch[0]);
    if (stereo) stats_chan_merge(a.ch[1], b.ch[1]);
}

// one sample into its channel's record (unsigned arithmetic throughout: an invalid source sample may be any int32)
LACX_HDF void stats_sample(StatsChan& c, int32_t x, uint32_t mask, int32_t lo, int32_t hi) {
    c.min_enc = stats_umax(c.min_enc, kStatsBias - (uint32_t)x);
    c.max_enc = stats_umax(c.max_enc, (uint32_t)x + kStatsBias + 1u);
    c.or_bits |= (uint32_t)x & mask;
    c.full_scale += x == lo || x == hi ? 1u : 0u;
    c.zeros += x == 0 ? 1u : 0u;
    c.sum += (unsigned long long)(long long)x;
    c.sum_sq += (unsigned long long)((long long)x * (long long)x);
}

// one frame into its block's record.  to_end: frames from this one to the block's end (>= 1); from_start: frames from
// the block's start to this one, inclusive (>= 1)
LACX_HDF void stats_frame(StatsAcc& a, int32_t l, int32_t r, bool stereo, int bit_depth, uint32_t to_end, uint32_t from_start) {
    const bool deep = bit_depth == 24;
    const uint32_t mask = deep ? 0xFFFFFFu : 0xFFFFu;
    const int32_t lo = deep ? -0x800000 : -32768, hi = deep ? 0x7FFFFF : 32767;
    stats_sample(a.ch[0], l, mask, lo, hi);
    if (stereo) stats_sample(a.ch[1], r, mask, lo, hi);
    if (l != 0 || (stereo && r != 0)) {
        a.first_nz = stats_umax(a.first_nz, to_end);
        a.last_nz = stats_umax(a.last_nz, from_start);
    }
    a.differing += stereo && l != r ? 1u : 0u;
}

// The unit's nf frames l / r, of which the first k lie in block b0 = [start0, split) and the others in b0 + 1 =
// [split, end1) (item frames), into the unit's one or two records.
LACX_HDF void stats_split(StatsUnit& u, const int32_t* l, const int32_t* r, uint32_t nf, uint32_t k, unsigned long long f0,
                          unsigned long long start0, unsigned long long split, unsigned long long end1, bool stereo, int bit_depth) {
    u.n0 = k;
    u.n1 = nf - k;
#pragma unroll
    for (uint32_t i = 0; i < 4u; ++i) {
        if (i < k) stats_frame(u.p0, l[i], r[i], stereo, bit_depth, (uint32_t)(split - f0 - i), (uint32_t)(f0 + i - start0) + 1u);
        else if (i < nf) stats_frame(u.p1, l[i], r[i], stereo, bit_depth, (uint32_t)(end1 - f0 - i), (uint32_t)(f0 + i - split) + 1u);
    }
}

// Stream form.  Frames f0 .. f0 + 3 of an item (f0 a multiple of 4) from left / right as k_ms_inverse left them, loaded
// as block_unit_decoded loads them: one 16-byte load per channel where the array's base is 16-byte aligned, else dword
// loads, the partial last unit element by element.  The scratch behind a missing or lost block is loaded (inside the
// buffer) and its record then not used.  frame_off and status are the item's own, frame_base the value of frame_off[0].
LACX_HDF StatsUnit stats_unit_decoded(unsigned long long f0, uint32_t num_blocks, uint32_t present, int channels, int bit_depth,
                                      unsigned long long frames, const unsigned long long* __restrict__ frame_off,
                                      unsigned long long frame_base, const int32_t* __restrict__ left,
                                      const int32_t* __restrict__ right, const uint32_t* __restrict__ status) {
    const uint32_t nf = frames - f0 >= 4u ? 4u : (uint32_t)(frames - f0);
    const bool stereo = channels == 2;
    int32_t l[4] = {0, 0, 0, 0}, r[4] = {0, 0, 0, 0};
    if (nf == 4u && ((uintptr_t)left & 15u) == 0 && (!stereo || ((uintptr_t)right & 15u) == 0)) {
        __builtin_memcpy(l, __builtin_assume_aligned(left + f0, 16), 16);
        if (stereo) __builtin_memcpy(r, __builtin_assume_aligned(right + f0, 16), 16);
    } else {  // (fixed trip counts throughout: the arrays stay in registers)
#pragma unroll
        for (uint32_t i = 0; i < 4u; ++i) {
            if (i < nf) {
                l[i] = left[f0 + i];
                if (stereo) r[i] = right[f0 + i];
            }
        }
    }
    StatsUnit u{};
    u.b0 = verify_block_of_frame(frame_off, num_blocks, frame_base, f0);
    const unsigned long long start0 = frame_off[u.b0] - frame_base;
    const unsigned long long split = frame_off[u.b0 + 1] - frame_base;  // frames from here on belong to block b0 + 1
    const uint32_t k = split - f0 >= nf ? nf : (uint32_t)(split - f0);
    u.use0 = u.b0 < present && status[u.b0] == 0u;
    unsigned long long end1 = split;
    if (k < nf) {  // (then block b0 + 1 exists: the unit's last frame lies in it)
        u.use1 = u.b0 + 1u < present && status[u.b0 + 1u] == 0u;
        end1 = frame_off[u.b0 + 2] - frame_base;
    }
    stats_split(u, l, r, nf, k, f0, start0, split, end1, stereo, bit_depth);
    return u;
}

// The source form's loads: frames f0 .. f0 + 3 (f0 a multiple of 4; nf of them exist) of device-resident PCM in its own
// layout, exactly as digest_unit_source loads and validates them:
//   planar int32 / float32   one 16-byte load per channel where the row's base is 16-byte aligned, else dword loads
//   planar int16             8 bytes per channel where the row's base is 8-byte aligned, else int16 loads
//   interleaved int16        8 (mono) or 16 (stereo) bytes from a 4-byte aligned base, as dwords
//   interleaved int24        12 or 24 bytes: dwords where the base is 4-byte aligned, bytes otherwise
//   interleaved float32      16 (mono) or 32 (stereo) bytes where the base is 16-byte aligned, else dword loads
// and the partial last unit element by element (verify_src_raw).  Floats go through f32_to_pcm at the item's depth.  A
// sample that is no sample of the depth lowers `key` (digest_bad_key) and fails the item.
LACX_HDF void stats_load_source(unsigned long long f0, uint32_t nf, int channels, int bit_depth, const void* __restrict__ src0,
                                const void* __restrict__ src1, uint32_t layout, unsigned long long& key, int32_t* sl, int32_t* sr) {
    const bool stereo = channels == 2;
    if (nf == 4u) {
        if (layout == (uint32_t)PCM_PLANAR_I32 || layout == (uint32_t)PCM_PLANAR_F32) {
            const int32_t* a = static_cast<const int32_t*>(src0) + f0;
            if (((uintptr_t)src0 & 15u) == 0) {
                __builtin_memcpy(sl, __builtin_assume_aligned(a, 16), 16);
            } else {
                sl[0] = a[0], sl[1] = a[1], sl[2] = a[2], sl[3] = a[3];
            }
            if (stereo) {
                const int32_t* b = static_cast<const int32_t*>(src1) + f0;
                if (((uintptr_t)src1 & 15u) == 0) {
                    __builtin_memcpy(sr, __builtin_assume_aligned(b, 16), 16);
                } else {
                    sr[0] = b[0], sr[1] = b[1], sr[2] = b[2], sr[3] = b[3];
                }
            }
        } else if (layout == (uint32_t)PCM_PLANAR_I16) {
            import_detail::load_i16x4(static_cast<const int16_t*>(src0) + f0, ((uintptr_t)src0 & 7u) == 0, 4u, sl);
            if (stereo) import_detail::load_i16x4(static_cast<const int16_t*>(src1) + f0, ((uintptr_t)src1 & 7u) == 0, 4u, sr);
        } else if (layout == (uint32_t)PCM_INTERLEAVED_F32) {
            const bool wide = ((uintptr_t)src0 & 15u) == 0;
            if (stereo) {
                uint32_t w[8];
                const uint32_t* p = static_cast<const uint32_t*>(src0) + 2ull * f0;
                import_detail::load_u32x4(p, wide, 4u, w);
                import_detail::load_u32x4(p + 4, wide, 4u, w + 4);
#pragma unroll
                for (uint32_t i = 0; i < 4u; ++i) sl[i] = (int32_t)w[2u * i], sr[i] = (int32_t)w[2u * i + 1u];
            } else {
                uint32_t w[4];
                import_detail::load_u32x4(static_cast<const uint32_t*>(src0) + f0, wide, 4u, w);
#pragma unroll
                for (uint32_t i = 0; i < 4u; ++i) sl[i] = (int32_t)w[i];
            }
        } else if (layout == (uint32_t)PCM_INTERLEAVED_I16) {
            uint32_t w[4];
            if (stereo) {
                __builtin_memcpy(w, __builtin_assume_aligned(static_cast<const uint8_t*>(src0) + 4ull * f0, 4), 16);
#pragma unroll
                for (uint32_t i = 0; i < 4u; ++i) sl[i] = (int16_t)(w[i] & 0xFFFFu), sr[i] = (int32_t)w[i] >> 16;
            } else {
                __builtin_memcpy(w, __builtin_assume_aligned(static_cast<const uint8_t*>(src0) + 2ull * f0, 4), 8);
                sl[0] = (int16_t)(w[0] & 0xFFFFu), sl[1] = (int32_t)w[0] >> 16;
                sl[2] = (int16_t)(w[1] & 0xFFFFu), sl[3] = (int32_t)w[1] >> 16;
            }
        } else {
            uint32_t w[7] = {0, 0, 0, 0, 0, 0, 0};
            const bool dwords = ((uintptr_t)src0 & 3u) == 0;
            if (stereo) {
                const uint8_t* p = static_cast<const uint8_t*>(src0) + 6ull * f0;
                if (dwords) __builtin_memcpy(w, __builtin_assume_aligned(p, 4), 24);
                else __builtin_memcpy(w, p, 24);
#pragma unroll
                for (uint32_t i = 0; i < 4u; ++i) sl[i] = get24(w, 2u * i), sr[i] = get24(w, 2u * i + 1u);
            } else {
                const uint8_t* p = static_cast<const uint8_t*>(src0) + 3ull * f0;
                if (dwords) __builtin_memcpy(w, __builtin_assume_aligned(p, 4), 12);
                else __builtin_memcpy(w, p, 12);
#pragma unroll
                for (uint32_t i = 0; i < 4u; ++i) sl[i] = get24(w, i);
            }
        }
    } else {
#pragma unroll
        for (uint32_t i = 0; i < 3u; ++i) {
            if (i < nf) {
                sl[i] = verify_src_raw(src0, src1, layout, channels, f0 + i, 0u);
                if (stereo) sr[i] = verify_src_raw(src0, src1, layout, channels, f0 + i, 1u);
            }
        }
    }
    const bool f32 = verify_is_f32(layout), ranged = layout == (uint32_t)PCM_PLANAR_I32;
    const int32_t lo = bit_depth == 16 ? -32768 : -0x800000, hi = bit_depth == 16 ? 32767 : 0x7FFFFF;
#pragma unroll
    for (uint32_t i = 0; i < 4u; ++i) {
        if (i >= nf) continue;
        int kl = 0, kr = 0;
        if (f32) {
            kl = f32_to_pcm((uint32_t)sl[i], bit_depth, sl[i]);
            if (stereo) kr = f32_to_pcm((uint32_t)sr[i], bit_depth, sr[i]);
        } else if (ranged) {
            kl = sl[i] < lo || sl[i] > hi ? 1 : 0;
            kr = stereo && (sr[i] < lo || sr[i] > hi) ? 1 : 0;
        }
        if (kl) {
            const unsigned long long k = digest_bad_key(0u, f0 + i, kl);
            key = k < key ? k : key;
        }
        if (kr) {
            const unsigned long long k = digest_bad_key(1u, f0 + i, kr);
            key = k < key ? k : key;
        }
    }
}

// Source form.  Blocks lie on a regular grid of `grid` frames (256 .. 16384), the last one shorter; every block counts.
LACX_HDF StatsUnit stats_unit_source(unsigned long long f0, uint32_t grid, int channels, int bit_depth, unsigned long long frames,
                                     const void* __restrict__ src0, const void* __restrict__ src1, uint32_t layout,
                                     unsigned long long& key) {
    const uint32_t nf = frames - f0 >= 4u ? 4u : (uint32_t)(frames - f0);
    int32_t l[4] = {0, 0, 0, 0}, r[4] = {0, 0, 0, 0};
    stats_load_source(f0, nf, channels, bit_depth, src0, src1, layout, key, l, r);
    StatsUnit u{};
    const unsigned long long b = f0 / grid;
    u.b0 = (uint32_t)b;
    const unsigned long long start0 = b * grid;
    unsigned long long split = start0 + grid;
    if (split > frames) split = frames;
    const uint32_t k = split - f0 >= nf ? nf : (uint32_t)(split - f0);
    u.use0 = true;
    unsigned long long end1 = split;
    if (k < nf) {
        u.use1 = true;
        end1 = split + grid;
        if (end1 > frames) end1 = frames;
    }
    stats_split(u, l, r, nf, k, f0, start0, split, end1, channels == 2, bit_depth);
    return u;
}

}  // namespace lacx
