// salvage_core.h -- the per-thread code of the decoder's salvage job (k_salvage_wav and k_salvage_blank of decode.hip):
// the second of two passes in stream order.  The first is k_ms_inverse, in place: status 7 is final only once every
// sample of a block has been examined, so nothing may leave before that pass is done.  This one only reads final status
// words -- no atomics -- and writes what the caller gets: the samples of the blocks that decoded, zeros for every frame
// of a block that is lost (a non-zero status, or a block the file no longer holds: index >= present).  Written like
// verify_core.h so that the same source compiles into the gfx950 kernels and into a host program the tests run under
// AddressSanitizer / UBSan (tests/native/sim_salvage.cpp), with buffers of exactly the plan's capacities.  Kept apart
// from wav_pack_unit of decode.hip on purpose: shared inline helpers change k_wav_pack's register allocation.
#pragma once
#include <cstdint>

#include "decode_core.h"

namespace lacx {

// The block that holds frame f (block_of_frame of decode.hip): the regular layout is a guess that one comparison
// confirms, any other table is searched.  frame_off: the item's own num_blocks + 1 entries, frame_base its first.
LACX_HDF uint32_t salvage_block_of_frame(const unsigned long long* __restrict__ frame_off, uint32_t num_blocks,
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

// Block b of an item is lost: nobody decoded it (the status word of such a block was written by nobody and is not
// looked at), or its lane or the range check refused it.
LACX_HDF bool salvage_lost(const uint32_t* __restrict__ status, uint32_t b, uint32_t present) {
    return b >= present || status[b] != 0u;
}

LACX_HDF uint32_t salvage_pack16(int32_t a, int32_t b) { return ((uint32_t)a & 0xFFFFu) | ((uint32_t)b << 16); }
// four 24-bit samples, low three bytes each, little-endian: three dwords
LACX_HDF void salvage_pack24(int32_t a, int32_t b, int32_t c, int32_t d, uint32_t* w) {
    const uint32_t ua = (uint32_t)a & 0xFFFFFFu, ub = (uint32_t)b & 0xFFFFFFu, uc = (uint32_t)c & 0xFFFFFFu, ud = (uint32_t)d;
    w[0] = ua | (ub << 24);
    w[1] = (ub >> 8) | (uc << 16);
    w[2] = (uc >> 16) | (ud << 8);
}

// One thread's work (k_salvage_wav): frames f0 .. f0 + 3 of an item (f0 a multiple of 4) into the data region of its WAV
// image, laid out as wav_pack_unit lays it out -- one 16-byte load per channel, 8 / 12 / 16 / 24 bytes of dword stores at
// 44 + f0 * block_align (always 4-byte aligned), the last unit byte by byte and with it the RIFF pad byte of an odd data
// size.  left / right hold the samples AFTER the mid/side inverse (k_ms_inverse ran): they are packed as they are.  A
// unit may straddle two blocks of different fate, and non-final blocks may have any length from 256 frames on, so the
// block is looked up per frame; every frame of a lost block leaves as zero.  The scratch behind a missing block was
// written by nobody: it is loaded (inside the buffer: an item's frames are the whole table's) and then not used.
// frame_off and status are the item's own (num_blocks entries from its first block), frame_base the value of
// frame_off[0], present the item's present blocks.  wav_data: the image's first byte (the header is the host's).
LACX_HDF void salvage_wav_unit(unsigned long long f0, uint32_t num_blocks, uint32_t present, int channels, int bit_depth,
                               unsigned long long frames, const unsigned long long* __restrict__ frame_off,
                               unsigned long long frame_base, const int32_t* __restrict__ left,
                               const int32_t* __restrict__ right, const uint32_t* __restrict__ status,
                               uint8_t* __restrict__ wav_data) {
    const uint32_t nf = frames - f0 >= 4u ? 4u : (uint32_t)(frames - f0);
    const bool stereo = channels == 2;
    int32_t l[4] = {0, 0, 0, 0}, r[4] = {0, 0, 0, 0};
    if (nf == 4u) {
        __builtin_memcpy(l, __builtin_assume_aligned(left + f0, 16), 16);  // f0 is a multiple of 4: 16-byte aligned
        if (stereo) __builtin_memcpy(r, __builtin_assume_aligned(right + f0, 16), 16);
    } else {  // (fixed trip counts throughout: l / r stay in registers)
#pragma unroll
        for (uint32_t i = 0; i < 3u; ++i) {
            if (i < nf) {
                l[i] = left[f0 + i];
                if (stereo) r[i] = right[f0 + i];
            }
        }
    }
    const uint32_t b0 = salvage_block_of_frame(frame_off, num_blocks, frame_base, f0);
    const unsigned long long split = frame_off[b0 + 1] - frame_base;  // frames from here on belong to block b0 + 1
    const uint32_t b1 = f0 + nf > split ? b0 + 1u : b0;
    const bool lost0 = salvage_lost(status, b0, present), lost1 = salvage_lost(status, b1, present);
#pragma unroll
    for (uint32_t i = 0; i < 4u; ++i) {
        const bool lost = f0 + i >= split ? lost1 : lost0;
        l[i] = lost ? 0 : l[i];
        r[i] = lost ? 0 : r[i];
    }

    const uint32_t bps = (uint32_t)bit_depth / 8u, align = (uint32_t)channels * bps;
    uint8_t* dst = static_cast<uint8_t*>(__builtin_assume_aligned(wav_data + 44 + f0 * align, 4));
    if (nf == 4u) {
        uint32_t w[6];
        if (bps == 2u) {
            if (stereo) {
                w[0] = salvage_pack16(l[0], r[0]), w[1] = salvage_pack16(l[1], r[1]), w[2] = salvage_pack16(l[2], r[2]),
                w[3] = salvage_pack16(l[3], r[3]);
                __builtin_memcpy(dst, w, 16);
            } else {
                w[0] = salvage_pack16(l[0], l[1]), w[1] = salvage_pack16(l[2], l[3]);
                __builtin_memcpy(dst, w, 8);
            }
        } else if (stereo) {
            salvage_pack24(l[0], r[0], l[1], r[1], w);
            salvage_pack24(l[2], r[2], l[3], r[3], w + 3);
            __builtin_memcpy(dst, w, 24);
        } else {
            salvage_pack24(l[0], l[1], l[2], l[3], w);
            __builtin_memcpy(dst, w, 12);
        }
    } else {
#pragma unroll
        for (uint32_t i = 0; i < 3u; ++i) {
#pragma unroll
            for (uint32_t c = 0; c < 2u; ++c) {
                const uint32_t v = (uint32_t)(c ? r[i] : l[i]);
#pragma unroll
                for (uint32_t k = 0; k < 3u; ++k)
                    if (i < nf && c < (uint32_t)channels && k < bps) dst[i * align + c * bps + k] = (uint8_t)(v >> (8u * k));
            }
        }
    }
    if (f0 + nf == frames && ((frames * align) & 1ull)) dst[nf * align] = 0;  // RIFF pad byte
}

// One tile of 1024 frames of one LOST block (k_salvage_blank, the device form): zeros into the caller's arrays, the share
// of thread `tid` of 256.  f0: the block's first frame in left / right, n its frames; the arrays are only 4-byte aligned
// (a row of an odd-length tensor), so every sample leaves as a dword store of its own.  Nothing outside the block's
// frames is written; right is null for a mono item and then not touched.
LACX_HDF void salvage_blank_tile(uint32_t tile, unsigned long long f0, uint32_t n, int32_t* __restrict__ left,
                                 int32_t* __restrict__ right, uint32_t tid) {
    for (uint32_t i = tile * 1024u + tid; i < n && i < (tile + 1u) * 1024u; i += 256u) {
        left[f0 + i] = 0;
        if (right) right[f0 + i] = 0;
    }
}

}  // namespace lacx
