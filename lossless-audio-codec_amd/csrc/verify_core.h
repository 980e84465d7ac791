// verify_core.h -- the per-thread code of the decoder's verify form (k_verify of decode.hip): the decoded samples of four
// consecutive frames, taken from the decoder's scratch as k_wav_pack takes them, compared with the same four frames of the
// source PCM in the source's own layout.  Nothing is stored but what differs: a bit per differing sample goes back to the
// caller, who adds the bits up per item.  Written like decode_core.h so that the same source compiles into the gfx950
// kernel and into a host program the tests run under AddressSanitizer / UBSan (tests/native/sim_verify.cpp): every load
// of the source is in here, and the twin hands it buffers of exactly frames * block_align bytes at every base alignment
// a layout permits.
#pragma once
#include <cstdint>

#include "decode_core.h"
#include "import_core.h"

namespace lacx {

// The block that holds frame f (block_of_frame of decode.hip): the regular layout is a guess that one comparison
// confirms, any other table is searched.  frame_off: the item's own num_blocks + 1 entries, frame_base its first.
LACX_HDF uint32_t verify_block_of_frame(const unsigned long long* __restrict__ frame_off, uint32_t num_blocks,
                                        unsigned long long frame_base, unsigned long long f) {
    uint32_t g = (uint32_t)(f / (unsigned long long)kMaxBlock);
    if (g >= num_blocks) g = num_blocks - 1u;
    if (frame_off[g] - frame_base <= f && f < frame_off[g + 1] - frame_base) return g;
    uint32_t lo = 0, hi = num_blocks;  // frame_off[lo] <= f < frame_off[hi]
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (frame_off[mid] - frame_base <= f) lo = mid;
        else hi = mid;
    }
    return lo;
}

// sample k of packed little-endian 3-byte samples held in dwords (w has one spare dword behind the last one in use);
// sext24: analyze_core.h
LACX_HDF int32_t get24(const uint32_t* w, uint32_t k) {
    const uint32_t b = 3u * k;
    const unsigned long long two = ((unsigned long long)w[(b >> 2) + 1u] << 32) | w[b >> 2];
    return sext24((uint32_t)(two >> (8u * (b & 3u))));
}

// One sample of the source, read element by element: channel c of frame f, as it lies there -- an integer sample, or the
// bits of a float32.  The partial last unit of an item and the report of the first mismatch come through here; it touches
// the bytes of that sample only.
LACX_HDF int32_t verify_src_raw(const void* __restrict__ src0, const void* __restrict__ src1, uint32_t layout, int channels,
                                unsigned long long f, uint32_t c) {
    if (layout == (uint32_t)PCM_PLANAR_I32 || layout == (uint32_t)PCM_PLANAR_F32) return static_cast<const int32_t*>(c ? src1 : src0)[f];
    if (layout == (uint32_t)PCM_PLANAR_I16) return static_cast<const int16_t*>(c ? src1 : src0)[f];
    const unsigned long long k = f * (unsigned long long)channels + c;
    if (layout == (uint32_t)PCM_INTERLEAVED_F32) return static_cast<const int32_t*>(src0)[k];
    if (layout == (uint32_t)PCM_INTERLEAVED_I16) return static_cast<const int16_t*>(src0)[k];
    const uint8_t* p = static_cast<const uint8_t*>(src0) + 3ull * k;
    return sext24((uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16));
}
LACX_HDF bool verify_is_f32(uint32_t layout) { return layout == (uint32_t)PCM_PLANAR_F32 || layout == (uint32_t)PCM_INTERLEAVED_F32; }
// The same as a sample value.  A float32 that is no sample of the depth (f32_to_pcm, import_core.h) gives the product
// rounded to nearest and saturated, INT32_MIN for a NaN, and *invalid: it differs from whatever was decoded.
LACX_HDF int32_t verify_src_sample(const void* __restrict__ src0, const void* __restrict__ src1, uint32_t layout, int channels,
                                   unsigned long long f, uint32_t c, int bit_depth = 0, bool* invalid = nullptr) {
    int32_t v = verify_src_raw(src0, src1, layout, channels, f, c);
    if (verify_is_f32(layout)) {
        const bool bad = f32_to_pcm((uint32_t)v, bit_depth, v) != 0;
        if (invalid) *invalid = bad;
    }
    return v;
}

// One thread's work: frames f0 .. f0 + 3 of an item (f0 a multiple of 4).  left / right, frame_off, ms_flag and status are
// the item's own, as in wav_pack_unit: the decoded samples arrive as one 16-byte load per channel, the block -- MS flag
// and status -- is looked up per frame (a unit spans at most two blocks, whose flags may differ), the mid/side inverse
// and the bit-depth check are applied (status 7 on a block that decoded).  The source's four frames:
//   planar int32      one 16-byte load per channel where the item's base is 16-byte aligned (uniform per item), else
//                     dword loads; the bases are 4-byte aligned
//   interleaved int16 8 (mono) or 16 (stereo) bytes from a 4-byte aligned base, as dwords
//   interleaved int24 12 or 24 bytes: dwords where the base is 4-byte aligned (the unit's offset is a multiple of 12),
//                     bytes otherwise; sign-extended from bit 23
//   planar int16      8 bytes per channel where the row's base is 8-byte aligned, else int16 loads (2-byte aligned bases)
//   planar float32    as planar int32, then every float through f32_to_pcm at the item's depth
//   interleaved float32  16 (mono) or 32 (stereo) bytes where the base is 16-byte aligned, else dword loads; likewise
// and the partial last unit element by element, so that no byte outside [0, frames * block_align) of an interleaved
// source and no element outside [0, frames) of a planar array is read.  The full int32 values are compared: a planar
// source sample that equals the decoded one only modulo 2^24 differs.  Only frames of blocks with status 0 count.
// Returns a bit per differing sample, bit 2 * i + c for channel c of frame f0 + i: their number is the unit's share of
// the item's count, and 2 * f0 + the lowest bit's index its candidate for the first-mismatch key frame * 2 + channel.
LACX_HDF uint32_t verify_unit(unsigned long long f0, uint32_t num_blocks, int channels, int bit_depth, unsigned long long frames,
                              const unsigned long long* __restrict__ frame_off, unsigned long long frame_base,
                              const int32_t* __restrict__ left, const int32_t* __restrict__ right,
                              const uint8_t* __restrict__ ms_flag, uint32_t* __restrict__ status,
                              const void* __restrict__ src0, const void* __restrict__ src1, uint32_t layout) {
    const uint32_t nf = frames - f0 >= 4u ? 4u : (uint32_t)(frames - f0);
    const bool stereo = channels == 2;
    int32_t l[4] = {0, 0, 0, 0}, r[4] = {0, 0, 0, 0}, sl[4] = {0, 0, 0, 0}, sr[4] = {0, 0, 0, 0};
    if (nf == 4u) {
        __builtin_memcpy(l, __builtin_assume_aligned(left + f0, 16), 16);  // f0 is a multiple of 4: 16-byte aligned
        if (stereo) __builtin_memcpy(r, __builtin_assume_aligned(right + f0, 16), 16);
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
    } else {  // (fixed trip counts throughout: the arrays stay in registers)
#pragma unroll
        for (uint32_t i = 0; i < 3u; ++i) {
            if (i < nf) {
                l[i] = left[f0 + i];
                sl[i] = verify_src_raw(src0, src1, layout, channels, f0 + i, 0u);
                if (stereo) {
                    r[i] = right[f0 + i];
                    sr[i] = verify_src_raw(src0, src1, layout, channels, f0 + i, 1u);
                }
            }
        }
    }
    uint32_t inval = 0;  // float sources: bit 2 * i + c for a value that is no sample of the depth
    if (verify_is_f32(layout)) {
#pragma unroll
        for (uint32_t i = 0; i < 4u; ++i) {
            if (f32_to_pcm((uint32_t)sl[i], bit_depth, sl[i]) != 0) inval |= 1u << (2u * i);
            if (stereo && f32_to_pcm((uint32_t)sr[i], bit_depth, sr[i]) != 0) inval |= 2u << (2u * i);
        }
    }
    const uint32_t b0 = verify_block_of_frame(frame_off, num_blocks, frame_base, f0);
    const unsigned long long split = frame_off[b0 + 1] - frame_base;  // frames from here on belong to block b0 + 1
    const uint32_t b1 = f0 + nf > split ? b0 + 1u : b0;
    const uint32_t st0 = status[b0], st1 = status[b1];
    const bool ms0 = stereo && ms_flag[b0] != 0, ms1 = stereo && ms_flag[b1] != 0;
    const long long lo = bit_depth == 16 ? -32768 : -0x800000, hi = bit_depth == 16 ? 32767 : 0x7FFFFF;
    bool bad0 = false, bad1 = false;
    uint32_t differ = 0;
#pragma unroll
    for (uint32_t i = 0; i < 4u; ++i) {
        const bool second = f0 + i >= split;
        long long a = l[i], b = r[i];
        if (second ? ms1 : ms0) {  // ref lac/decoder.cpp:48-65
            const long long m = a, s = b;
            a = m + ((s + (s & 1)) >> 1);
            b = a - s;
        }
        const bool bad = i < nf && (a < lo || a > hi || (stereo && (b < lo || b > hi)));
        bad0 = bad0 || (bad && !second);
        bad1 = bad1 || (bad && second);
        const bool compared = i < nf && (second ? st1 : st0) == 0u;  // only blocks that decoded
        if (compared && ((int32_t)a != sl[i] || ((inval >> (2u * i)) & 1u))) differ |= 1u << (2u * i);
        if (compared && stereo && ((int32_t)b != sr[i] || ((inval >> (2u * i)) & 2u))) differ |= 2u << (2u * i);
    }
    // blocks that did not decode are not checked (their status already fails the item)
    if (bad0 && st0 == 0u) status_max(&status[b0], 7u);
    if (bad1 && st1 == 0u) status_max(&status[b1], 7u);
    return differ;
}

// An item whose comparison found a difference: the block and the two values at its first-mismatch key (one thread per
// item after k_verify; the decoded value is made from the scratch again, the source read element by element; bit_depth:
// the item's, which a float32 source is scaled by).
LACX_HDF void verify_fill_item(uint32_t num_blocks, int channels, const unsigned long long* __restrict__ frame_off,
                               unsigned long long frame_base, const int32_t* __restrict__ left,
                               const int32_t* __restrict__ right, const uint8_t* __restrict__ ms_flag,
                               const void* __restrict__ src0, const void* __restrict__ src1, uint32_t layout, VerifyWords& w,
                               int bit_depth = 0) {
    if (w.count == 0) return;
    const unsigned long long f = w.key >> 1;
    const uint32_t c = (uint32_t)(w.key & 1u);
    const uint32_t blk = verify_block_of_frame(frame_off, num_blocks, frame_base, f);
    long long a = left[f], b = channels == 2 ? right[f] : 0;
    if (channels == 2 && ms_flag[blk] != 0) {
        const long long m = a, s = b;
        a = m + ((s + (s & 1)) >> 1);
        b = a - s;
    }
    w.decoded = (int32_t)(c ? b : a);
    w.source = verify_src_sample(src0, src1, layout, channels, f, c, bit_depth);
    w.block = blk;
}

}  // namespace lacx
