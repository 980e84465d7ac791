// blockdigest_core.h -- the per-thread code of the block digests (k_digest_blocks and k_digest_judge of k_blockdigest.hip):
// the CRC-32 of what every BLOCK of a stream decodes to, or of every block_frames frames of device-resident source PCM.
// A thread takes one unit of four frames, as in digest_core.h, but a unit's value now goes to the end of its block, not
// of its item.  Non-final blocks may have any length from 256 frames on, so a unit spans at most two blocks: its first k
// frames are a piece of block b0 that ends at that block's end (distance 0), the rest a piece at the start of b0 + 1
// (distance: that block's bytes less the piece's).  A unit that lies in one block is one piece.
// Stream form: the samples are read AFTER k_ms_inverse ran in place and the range check is final, as a salvage job leaves
// them: no inverse here, no status written; a block counts when it had a lane (index < present) and its status is 0.
// Source form: the loads, bounds and validation keys are digest_unit_source's own -- a piece of fewer than four frames is
// that function's partial unit, element by element, which needs no alignment of its first frame.
// Written like digest_core.h: the same source compiles into the gfx950 kernels and into a host program the tests run
// under AddressSanitizer / UBSan (tests/native/sim_blockdigest.cpp).
#pragma once
#include <cstdint>

#include "digest_core.h"

namespace lacx {

constexpr uint32_t kBlockDigestMismatch = 11;  // LACX_BLOCK_DIGEST: the status k_digest_judge stores

struct BlockUnit {
    uint32_t b0;                        // the block of the unit's first frame, counted in the item
    DigestPiece p0, p1;                 // p1.bytes == 0: the unit lies in one block
    unsigned long long dist0, dist1;    // bytes from the piece's end to the end of its block
    bool use0, use1;                    // the block counts (stream form: it decoded)
};

// the bytes of frames [i0, i1) of a unit's four (digest_bytes over a sub-range)
LACX_HDF DigestPiece digest_bytes_range(const int32_t* l, const int32_t* r, uint32_t i0, uint32_t i1, int channels, int bit_depth) {
    const bool stereo = channels == 2, deep = bit_depth == 24;
    const uint32_t mask = deep ? 0xFFFFFFu : 0xFFFFu, bps = deep ? 3u : 2u;
    uint32_t reg = 0;
#pragma unroll
    for (uint32_t i = 0; i < 4u; ++i) {
        if (i >= i0 && i < i1) {
            reg = crc_raw_bytes(reg, (uint32_t)l[i] & mask, 2u);
            if (deep) reg = crc_raw_bytes(reg, 0u, 1u);
            if (stereo) {
                reg = crc_raw_bytes(reg, (uint32_t)r[i] & mask, 2u);
                if (deep) reg = crc_raw_bytes(reg, 0u, 1u);
            }
        }
    }
    return DigestPiece{reg, (i1 > i0 ? i1 - i0 : 0u) * (uint32_t)channels * bps};
}

// Stream form.  Frames f0 .. f0 + 3 of an item (f0 a multiple of 4) from left / right as k_ms_inverse left them: one
// 16-byte load per channel where the array's base is 16-byte aligned (the decoder's own buffers always are; a caller's
// array of the device form need not be), else dword loads, the partial last unit element by element.  The scratch
// behind a missing block was written by nobody: it is loaded (inside the buffer: an item's frames are the whole
// table's) and then not used.  frame_off and status are the item's own, frame_base the value of frame_off[0].
LACX_HDF BlockUnit block_unit_decoded(unsigned long long f0, uint32_t num_blocks, uint32_t present, int channels, int bit_depth,
                                      unsigned long long frames, const unsigned long long* __restrict__ frame_off,
                                      unsigned long long frame_base, const int32_t* __restrict__ left,
                                      const int32_t* __restrict__ right, const uint32_t* __restrict__ status) {
    const uint32_t nf = frames - f0 >= 4u ? 4u : (uint32_t)(frames - f0);
    const bool stereo = channels == 2;
    const uint32_t align = (uint32_t)channels * ((uint32_t)bit_depth / 8u);
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
    BlockUnit u{};
    u.b0 = verify_block_of_frame(frame_off, num_blocks, frame_base, f0);
    const unsigned long long split = frame_off[u.b0 + 1] - frame_base;  // frames from here on belong to block b0 + 1
    const uint32_t k = split - f0 >= nf ? nf : (uint32_t)(split - f0);
    u.use0 = u.b0 < present && status[u.b0] == 0u;
    u.p0 = digest_bytes_range(l, r, 0u, k, channels, bit_depth);
    u.dist0 = (split - f0 - k) * align;
    if (k < nf) {  // (then block b0 + 1 exists: the unit's last frame lies in it)
        u.use1 = u.b0 + 1u < present && status[u.b0 + 1u] == 0u;
        u.p1 = digest_bytes_range(l, r, k, nf, channels, bit_depth);
        u.dist1 = (frame_off[u.b0 + 2] - frame_base - f0 - nf) * align;
    }
    return u;
}

// Source form.  Blocks lie on a regular grid of `grid` frames (256 .. 16384), the last one shorter.
LACX_HDF BlockUnit block_unit_source(unsigned long long f0, uint32_t grid, int channels, int bit_depth, unsigned long long frames,
                                     const void* __restrict__ src0, const void* __restrict__ src1, uint32_t layout,
                                     unsigned long long& key) {
    const unsigned long long end = frames - f0 >= 4u ? f0 + 4u : frames;  // behind the unit's last frame
    const uint32_t align = (uint32_t)channels * ((uint32_t)bit_depth / 8u);
    BlockUnit u{};
    const unsigned long long b = f0 / grid;
    u.b0 = (uint32_t)b;
    unsigned long long split = (b + 1u) * grid;
    if (split > frames) split = frames;
    const unsigned long long cut = split < end ? split : end;
    u.use0 = true;
    u.p0 = digest_unit_source(f0, channels, bit_depth, cut, src0, src1, layout, key);  // (cut < f0 + 4: its partial unit)
    u.dist0 = (split - cut) * align;
    if (cut < end) {
        unsigned long long next = split + grid;
        if (next > frames) next = frames;
        u.use1 = true;
        u.p1 = digest_unit_source(cut, channels, bit_depth, end, src0, src1, layout, key);  // fewer than four frames
        u.dist1 = (next - end) * align;
    }
    return u;
}

// k_digest_judge, one global block: a block that had a lane, decoded and has an expected value is finalised -- the init
// term and the final xor depend on its byte count alone -- and compared; a difference makes it lost with status 11.
// Nobody else writes a status word at that point.  status / raw / expect: the job's, by global block.
LACX_HDF void judge_block(uint32_t g, uint32_t block_in_item, uint32_t present, bool judged, uint32_t block_frames, uint32_t align,
                          const uint32_t* __restrict__ raw, const uint32_t* __restrict__ expect, uint32_t* __restrict__ status) {
    if (!judged || block_in_item >= present || status[g] != 0u) return;
    if (crc_finish(raw[g], (unsigned long long)block_frames * align) != expect[g]) status[g] = kBlockDigestMismatch;
}

}  // namespace lacx
