// digest_core.h -- the per-thread code of the decoder's digest form (k_digest of k_digest.hip): the final PCM values of
// four consecutive frames of an item, taken either from the decoder's scratch as k_wav_pack / verify_unit take them or
// from device-resident source PCM in its own layout with the loads verify_unit has, formed into the bytes those frames
// have in a WAV data chunk (interleaved little-endian, 2 or 3 bytes per sample) and digested: the unit's raw CRC-32
// value (crc32_core.h) and its byte count.  The kernel shifts every unit's value to the item's end and adds them up.
// Written like verify_core.h: the same source compiles into the gfx950 kernel and into a host program the tests run under
// AddressSanitizer / UBSan (tests/native/sim_digest.cpp); every load of the scratch and of a source is in here, and the
// twin hands it buffers of exactly frames * block_align bytes at every base alignment a layout permits.
#pragma once
#include <cstdint>

#include "crc32_core.h"
#include "verify_core.h"

namespace lacx {

constexpr uint32_t kDigestThreads = 256;  // units per workgroup of k_digest
static_assert(kDigestUnitFrames == 4, "the unit's loads are those of wav_pack_unit / verify_unit: four frames");

struct DigestPiece {
    uint32_t raw;    // raw CRC-32 value of the unit's bytes
    uint32_t bytes;  // their number: frames in the unit * block_align, at most 24
};
// the source form's key of an invalid sample: all of left before right (the encoder's order), then the lowest index;
// bit 0: 1 not an exact sample of the depth, 0 an integer outside it (ImportBad's low bits)
LACX_HDF unsigned long long digest_bad_key(uint32_t channel, unsigned long long frame, int kind) {
    return ((unsigned long long)channel << 63) | (frame << 1) | (kind == 2 ? 1u : 0u);
}

// the bytes of nf frames (l / r: final sample values; only the low bit_depth bits of each are used) as a raw value
LACX_HDF DigestPiece digest_bytes(const int32_t* l, const int32_t* r, uint32_t nf, int channels, int bit_depth) {
    const bool stereo = channels == 2, deep = bit_depth == 24;
    const uint32_t mask = deep ? 0xFFFFFFu : 0xFFFFu, bps = deep ? 3u : 2u;
    uint32_t reg = 0;
#pragma unroll
    for (uint32_t i = 0; i < 4u; ++i) {
        if (i < nf) {  // a sample enters whole; its third byte is eight more steps of the register
            reg = crc_raw_bytes(reg, (uint32_t)l[i] & mask, 2u);
            if (deep) reg = crc_raw_bytes(reg, 0u, 1u);
            if (stereo) {
                reg = crc_raw_bytes(reg, (uint32_t)r[i] & mask, 2u);
                if (deep) reg = crc_raw_bytes(reg, 0u, 1u);
            }
        }
    }
    return DigestPiece{reg, nf * (uint32_t)channels * bps};
}

// Stream form.  One thread's work: frames f0 .. f0 + 3 of an item (f0 a multiple of 4), exactly as wav_pack_unit and
// verify_unit obtain them: one 16-byte load per channel from the decoder's scratch (the partial last unit element by
// element), the block -- MS flag and status -- looked up per frame (a unit spans at most two blocks, whose flags may
// differ), the mid/side inverse, and the bit-depth check (status 7 on a block that decoded).  Only frames of blocks with
// status 0 count: the samples of any other block enter as zeros (its status already fails the item).
LACX_HDF DigestPiece digest_unit_decoded(unsigned long long f0, uint32_t num_blocks, int channels, int bit_depth,
                                         unsigned long long frames, const unsigned long long* __restrict__ frame_off,
                                         unsigned long long frame_base, const int32_t* __restrict__ left,
                                         const int32_t* __restrict__ right, const uint8_t* __restrict__ ms_flag,
                                         uint32_t* __restrict__ status) {
    const uint32_t nf = frames - f0 >= 4u ? 4u : (uint32_t)(frames - f0);
    const bool stereo = channels == 2;
    int32_t l[4] = {0, 0, 0, 0}, r[4] = {0, 0, 0, 0};
    if (nf == 4u) {
        __builtin_memcpy(l, __builtin_assume_aligned(left + f0, 16), 16);  // f0 is a multiple of 4: 16-byte aligned
        if (stereo) __builtin_memcpy(r, __builtin_assume_aligned(right + f0, 16), 16);
    } else {  // (fixed trip counts throughout: the arrays stay in registers)
#pragma unroll
        for (uint32_t i = 0; i < 3u; ++i) {
            if (i < nf) {
                l[i] = left[f0 + i];
                if (stereo) r[i] = right[f0 + i];
            }
        }
    }
    const uint32_t b0 = verify_block_of_frame(frame_off, num_blocks, frame_base, f0);
    const unsigned long long split = frame_off[b0 + 1] - frame_base;  // frames from here on belong to block b0 + 1
    const uint32_t b1 = f0 + nf > split ? b0 + 1u : b0;
    const uint32_t st0 = status[b0], st1 = status[b1];
    const bool ms0 = stereo && ms_flag[b0] != 0, ms1 = stereo && ms_flag[b1] != 0;
    const long long lo = bit_depth == 16 ? -32768 : -0x800000, hi = bit_depth == 16 ? 32767 : 0x7FFFFF;
    bool bad0 = false, bad1 = false;
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
        const bool counted = (second ? st1 : st0) == 0u;  // only blocks that decoded
        l[i] = counted ? (int32_t)a : 0;
        r[i] = counted ? (int32_t)b : 0;
    }
    // blocks that did not decode are not checked (their status already fails the item)
    if (bad0 && st0 == 0u) status_max(&status[b0], 7u);
    if (bad1 && st1 == 0u) status_max(&status[b1], 7u);
    return digest_bytes(l, r, nf, channels, bit_depth);
}

// Source form.  The same four frames of device-resident PCM in the source's own layout, loaded as verify_unit loads them:
//   planar int32 / float32   one 16-byte load per channel where the row's base is 16-byte aligned, else dword loads
//   planar int16             8 bytes per channel where the row's base is 8-byte aligned, else int16 loads
//   interleaved int16        8 (mono) or 16 (stereo) bytes from a 4-byte aligned base, as dwords
//   interleaved int24        12 or 24 bytes: dwords where the base is 4-byte aligned, bytes otherwise
//   interleaved float32      16 (mono) or 32 (stereo) bytes where the base is 16-byte aligned, else dword loads
// and the partial last unit element by element (verify_src_raw): no byte outside [0, frames * block_align) of an
// interleaved source and no element outside [0, frames) of a planar array is read.  Floats go through f32_to_pcm at the
// item's depth.  A sample that is no sample of the depth -- a planar int32 outside it, a float that is not exact --
// lowers `key` (digest_bad_key) and fails the item; what it contributes to the digest is then of no account.
LACX_HDF DigestPiece digest_unit_source(unsigned long long f0, int channels, int bit_depth, unsigned long long frames,
                                        const void* __restrict__ src0, const void* __restrict__ src1, uint32_t layout,
                                        unsigned long long& key) {
    const uint32_t nf = frames - f0 >= 4u ? 4u : (uint32_t)(frames - f0);
    const bool stereo = channels == 2;
    int32_t sl[4] = {0, 0, 0, 0}, sr[4] = {0, 0, 0, 0};
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
    return digest_bytes(sl, sr, nf, channels, bit_depth);
}

}  // namespace lacx
