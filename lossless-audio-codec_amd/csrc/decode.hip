// decode.hip -- CDNA4 (gfx950) kernels of the LAC v3 decoder (the product's own check that a .lac it
// produced gives back the PCM, on a box where the reference is absent).
//
// What the format allows to run in parallel is the block: inside a block the two channel bitstreams follow each other
// byte-aligned but without a length field, every token's length depends on the Rice parameter, and the Rice parameter
// depends on every sample decoded before it (ref src/codec/block/decoder.cpp:64-520, src/codec/rice/rice.hpp:45-114).
// So: ONE LANE PER BLOCK, both channels one after the other, all blocks of every stream of the job at once -- the
// duration is one block's serial chain whatever the streams' length (up to the chip's ~65 000 resident lanes = 18 h of
// audio), and the throughput comes from the number of blocks.  Per-lane state that must be indexed lives in LDS, one
// column per lane: the last 256 residual magnitudes of the stateful Rice adaptation and the predictor's history.
//   k_decode        bitstream -> residuals -> samples (fixed / FIR / LPC synthesis), planar int32, per-block status
//   k_decode_serial the same for a legacy version-2 stream (no compressed block sizes): one lane walks it
//   k_ms_inverse    mid/side -> left/right where the block's flag says so, and the bit-depth range check
//                                                                        (ref src/codec/lac/decoder.cpp:48-65,30-46)
//   k_wav_pack      the same per-sample work as k_ms_inverse, written as the data region of a canonical WAV image
//                   (interleaved little-endian 16 / 24-bit, ref src/main.cpp:150-182) instead of back into left/right
//   k_window_out    the same per-sample work over the blocks a frame window needs, the window's frames written as
//                   int32 or float32 into the caller's arrays (lacx_decoder_decode_window*)
//   k_verify        the same per-sample work, compared with the source PCM in its own layout instead of stored: a count
//                   of differing samples and the first of them per item (lacx_decoder_verify_*; verify_core.h)
//   (k_digest       the same per-sample work, digested instead of stored: k_digest.hip, launched from launch_decode)
//   k_salvage_wav   salvage job (decode through errors): after k_ms_inverse, the WAV image from the final status words --
//                   the blocks that decoded as they are, zeros for every frame of a lost one (salvage_core.h)
//   k_salvage_blank the same for caller-owned arrays: zeros over the lost blocks, nothing else touched
// Every launch decodes a batch of streams (items) as one job; a single stream is a batch of one.
// The adaptive Rice parameter uses the encoder's division-free formulation (kmean / biased_k of analyze_core.h, proven
// against Rice::adapt_k there); it assumes zigzag residuals below 2^30 like the encoder does, and a stream with a larger
// one is refused (status 9) rather than decoded differently from the reference.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "decode_core.h"
#include "kernels.h"
#include "salvage_core.h"
#include "verify_core.h"

namespace lacx {

namespace {

// A pointer read from memory (an item descriptor) is generic to the compiler, and its loads and stores would be flat
// ones; these all point into global memory, and the round trip through the global address space says so.
template <typename T>
__device__ __forceinline__ T* global_ptr(T* p) {
    return (T*)(__attribute__((address_space(1))) T*)(uintptr_t)p;
}

}  // namespace

// One lane per version-3 block: lane g decodes block lane_blk[g] of the global tables (~0u: an idle lane), whatever item
// it belongs to (blk_item); the item's descriptor gives the block's format and output arrays.  The host lays the lanes
// out so that an item's blocks sit in consecutive lanes (see launch_decode).  64 LDS columns per wave.
__global__ __launch_bounds__(kDecThreads) void k_decode(uint32_t lanes, const uint32_t* __restrict__ lane_blk,
                                                        const uint32_t* __restrict__ blk_item,
                                                        const DecodeItem* __restrict__ items,
                                                        const uint8_t* __restrict__ payload,
                                                        const unsigned long long* __restrict__ byte_off,
                                                        const unsigned long long* __restrict__ frame_off,
                                                        uint32_t* __restrict__ status, uint8_t* __restrict__ ms_flag) {
    extern __shared__ __align__(16) unsigned char dec_raw[];
    DecMem dm = dec_mem(dec_raw, blockDim.x);
    const int lane = (int)threadIdx.x;
    DecWave wave;
    const uint32_t g = blockIdx.x * kDecThreads + threadIdx.x;
    if (g >= lanes) return;
    const uint32_t blk = lane_blk[g];
    if (blk == ~0u) return;
    const DecodeItem& it = items[blk_item[blk]];
    decode_block_lane(blk, it.channels, it.stereo_mode, payload, byte_off, frame_off, it.frame0, global_ptr(it.left),
                      global_ptr(it.right), status, ms_flag, dm, lane, wave);
}

// The legacy version-2 container carries no compressed block sizes (ref lac/decoder.cpp:209-219): block i starts where
// block i-1 ended, so ONE lane walks a whole stream.  One lane per version-2 item (v2_items: their indices); launched only
// when the batch has such items.  Kept for completeness of the reader (the encoder has written version 3 only since).
__global__ __launch_bounds__(kDecThreads) void k_decode_serial(uint32_t nv2, const uint32_t* __restrict__ v2_items,
                                                               const DecodeItem* __restrict__ items,
                                                               const uint8_t* __restrict__ payload,
                                                               const unsigned long long* __restrict__ frame_off,
                                                               uint32_t* __restrict__ status, uint8_t* __restrict__ ms_flag) {
    extern __shared__ __align__(16) unsigned char dec_raw[];
    DecMem dm = dec_mem(dec_raw, kDecThreads);
    DecWave wave;
    const uint32_t g = blockIdx.x * kDecThreads + threadIdx.x;
    if (g >= nv2) return;
    const DecodeItem& it = items[v2_items[g]];
    decode_serial_lane(it.blocks, it.channels, it.stereo_mode, payload + it.pay_off, it.pay_bits, frame_off + it.block0, it.frame0,
                       global_ptr(it.left), global_ptr(it.right), status + it.block0, ms_flag + it.block0, dm, (int)threadIdx.x, wave);
}

// grid = (all blocks of the batch, tiles): the samples of block blockIdx.x in tiles of 1024, in place in its item's arrays
__global__ __launch_bounds__(256) void k_ms_inverse(const uint32_t* __restrict__ blk_item,
                                                    const DecodeItem* __restrict__ items,
                                                    const unsigned long long* __restrict__ frame_off,
                                                    const uint8_t* __restrict__ ms_flag, uint32_t* __restrict__ status) {
    const uint32_t blk = blockIdx.x, tile = blockIdx.y;
    if (status[blk]) return;  // (uniform) the block did not decode
    const DecodeItem& it = items[blk_item[blk]];
    const unsigned long long f0 = frame_off[blk];
    const uint32_t n = (uint32_t)(frame_off[blk + 1] - f0);
    ms_inverse_tile(blk, tile, it.channels, it.bit_depth, f0 - it.frame0, n, global_ptr(it.left), global_ptr(it.right), ms_flag,
                    status, threadIdx.x);
}

// The block that holds frame f: the regular layout (every block but the last 16384 frames) is a guess that one
// comparison confirms; any other table (non-final blocks may be any length from 256 frames on) is searched.
// frame_off: the stream's own num_blocks + 1 entries, frame_base the value of its first (f counts from there).
__device__ __forceinline__ uint32_t block_of_frame(const unsigned long long* __restrict__ frame_off, uint32_t num_blocks,
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
__device__ __forceinline__ uint32_t pack16(int32_t a, int32_t b) { return ((uint32_t)a & 0xFFFFu) | ((uint32_t)b << 16); }
// four 24-bit samples, low three bytes each, little-endian: three dwords
__device__ __forceinline__ void pack24(int32_t a, int32_t b, int32_t c, int32_t d, uint32_t* w) {
    const uint32_t ua = (uint32_t)a & 0xFFFFFFu, ub = (uint32_t)b & 0xFFFFFFu, uc = (uint32_t)c & 0xFFFFFFu, ud = (uint32_t)d;
    w[0] = ua | (ub << 24);
    w[1] = (ub >> 8) | (uc << 16);
    w[2] = (uc >> 16) | (ud << 8);
}

// One thread per unit of four consecutive frames of the stream (frames 4u .. 4u+3): 8, 12, 16 or 24 bytes of the image at
// 44 + 4u * block_align, always 4-byte aligned, so a whole unit leaves as dword stores (x2 / x3 / x4+x2) and the
// samples arrive as one 16-byte load per channel.  Block boundaries may fall anywhere (non-final blocks of any length
// from 256 frames on, odd ones included), so the block -- MS flag and status -- is looked up per frame; a unit spans at
// most two blocks.  The last unit is written byte by byte and writes the RIFF pad byte when the data size is odd.
// wav_data: the image's first byte (the 44-byte header is the host's).  wav_pack_unit is one thread's work (k_wav_pack):
// frame_off, ms_flag and status are the stream's own (num_blocks entries from its first block), frame_base the value of
// frame_off[0].
__device__ __forceinline__ void wav_pack_unit(unsigned long long f0, uint32_t num_blocks, int channels, int bit_depth,
                                              unsigned long long frames, const unsigned long long* __restrict__ frame_off,
                                              unsigned long long frame_base, const int32_t* __restrict__ left,
                                              const int32_t* __restrict__ right, const uint8_t* __restrict__ ms_flag,
                                              uint32_t* __restrict__ status, uint8_t* __restrict__ wav_data) {
    const uint32_t nf = frames - f0 >= 4u ? 4u : (uint32_t)(frames - f0);
    const bool stereo = channels == 2;
    int32_t l[4] = {0, 0, 0, 0}, r[4] = {0, 0, 0, 0};
    if (nf == 4u) {
        const int4 a = *reinterpret_cast<const int4*>(left + f0);  // f0 is a multiple of 4: 16-byte aligned
        l[0] = a.x, l[1] = a.y, l[2] = a.z, l[3] = a.w;
        if (stereo) {
            const int4 b = *reinterpret_cast<const int4*>(right + f0);
            r[0] = b.x, r[1] = b.y, r[2] = b.z, r[3] = b.w;
        }
    } else {  // (fixed trip counts throughout: l / r stay in registers)
#pragma unroll
        for (uint32_t i = 0; i < 3u; ++i) {
            if (i < nf) {
                l[i] = left[f0 + i];
                if (stereo) r[i] = right[f0 + i];
            }
        }
    }
    const uint32_t b0 = block_of_frame(frame_off, num_blocks, frame_base, f0);
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
        l[i] = (int32_t)a;
        r[i] = (int32_t)b;
        const bool bad = i < nf && (a < lo || a > hi || (stereo && (b < lo || b > hi)));
        bad0 = bad0 || (bad && !second);
        bad1 = bad1 || (bad && second);
    }
    // blocks that did not decode are not checked (their status already fails the call)
    if (bad0 && st0 == 0u) atomicMax(&status[b0], 7u);
    if (bad1 && st1 == 0u) atomicMax(&status[b1], 7u);

    const uint32_t bps = (uint32_t)bit_depth / 8u, align = (uint32_t)channels * bps;
    uint8_t* dst = static_cast<uint8_t*>(__builtin_assume_aligned(wav_data + 44 + f0 * align, 4));
    if (nf == 4u) {
        uint32_t w[6];
        if (bps == 2u) {
            if (stereo) {
                w[0] = pack16(l[0], r[0]), w[1] = pack16(l[1], r[1]), w[2] = pack16(l[2], r[2]), w[3] = pack16(l[3], r[3]);
                __builtin_memcpy(dst, w, 16);
            } else {
                w[0] = pack16(l[0], l[1]), w[1] = pack16(l[2], l[3]);
                __builtin_memcpy(dst, w, 8);
            }
        } else if (stereo) {
            pack24(l[0], r[0], l[1], r[1], w);
            pack24(l[2], r[2], l[3], r[3], w + 3);
            __builtin_memcpy(dst, w, 24);
        } else {
            pack24(l[0], l[1], l[2], l[3], w);
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

// Every item of a batch in one launch: thread u handles unit u of the concatenated unit ranges (unit_off: [nitems + 1]
// prefix sums of the items' ceil(frames / 4)), found by a binary search there.  Each item's PCM starts at a multiple of
// 4 frames and its image at a 16-byte boundary, so every unit keeps the aligned 16-byte loads and dword stores.  The search runs once per workgroup, on its first unit (uniform: scalar loads, and the item's
// descriptor in scalar registers); only a workgroup that spans items searches again per thread, among the later items.
__global__ __launch_bounds__(256) void k_wav_pack(uint32_t nitems, unsigned long long total_units,
                                                  const unsigned long long* __restrict__ unit_off,
                                                  const DecodeItem* __restrict__ items,
                                                  const unsigned long long* __restrict__ frame_off,
                                                  const uint8_t* __restrict__ ms_flag, uint32_t* __restrict__ status) {
    const unsigned long long first = (unsigned long long)blockIdx.x * 256u;
    uint32_t lo = 0, hi = nitems;  // unit_off[lo] <= first < unit_off[hi]
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (unit_off[mid] <= first) lo = mid;
        else hi = mid;
    }
    const unsigned long long u = first + threadIdx.x;
    if (u >= total_units) return;
    if (unit_off[lo + 1] >= first + 256u) {  // (uniform) the whole workgroup lies in item lo
        const DecodeItem& it = items[lo];
        wav_pack_unit(4ull * (u - unit_off[lo]), it.blocks, it.channels, it.bit_depth, it.frames, frame_off + it.block0, it.frame0,
                      global_ptr(it.left), global_ptr(it.right), ms_flag + it.block0, status + it.block0, global_ptr(it.wav));
        return;
    }
    uint32_t l2 = lo, h2 = nitems;  // unit_off[l2] <= u < unit_off[h2]
    while (h2 - l2 > 1u) {
        const uint32_t mid = l2 + (h2 - l2) / 2u;
        if (unit_off[mid] <= u) l2 = mid;
        else h2 = mid;
    }
    const DecodeItem& it = items[l2];
    wav_pack_unit(4ull * (u - unit_off[l2]), it.blocks, it.channels, it.bit_depth, it.frames, frame_off + it.block0, it.frame0,
                  global_ptr(it.left), global_ptr(it.right), ms_flag + it.block0, status + it.block0, global_ptr(it.wav));
}

// Window form: one thread per unit of four decoded frames of an item (frames 4u .. 4u+3 of the blocks that
// overlap its window, in the decoder's scratch, where each item starts at a multiple of 4 frames).  The same per-frame
// work as wav_pack_unit -- 16-byte loads, the block looked up per frame, the mid/side inverse, the bit-depth check of
// every decoded sample (status 7 on a block that decoded) -- and then a store of the frames that fall inside the window
// (w_start / w_frames, in decoded frames) at f - w_start of out_l / out_r: int32, or float32 scaled by
// 2^-(bit_depth - 1) (exact: a 16- or 24-bit sample and its scaled value are both exact in float32).  The outputs are
// only element-aligned (a row of an odd-length tensor), so every sample leaves as a dword store of its own; nothing
// outside [0, w_frames) is written, and out_r is not touched for a mono item.  (Kept apart from wav_pack_unit: shared
// inline helpers change k_wav_pack's register allocation.)
__device__ __forceinline__ void window_out_unit(unsigned long long f0, uint32_t num_blocks, int channels, int bit_depth,
                                                unsigned long long frames, const unsigned long long* __restrict__ frame_off,
                                                unsigned long long frame_base, const int32_t* __restrict__ left,
                                                const int32_t* __restrict__ right, const uint8_t* __restrict__ ms_flag,
                                                uint32_t* __restrict__ status, unsigned long long w_start,
                                                unsigned long long w_frames, uint32_t* __restrict__ out_l,
                                                uint32_t* __restrict__ out_r, bool f32) {
    const uint32_t nf = frames - f0 >= 4u ? 4u : (uint32_t)(frames - f0);
    const bool stereo = channels == 2;
    int32_t l[4] = {0, 0, 0, 0}, r[4] = {0, 0, 0, 0};
    if (nf == 4u) {
        const int4 a = *reinterpret_cast<const int4*>(left + f0);  // f0 is a multiple of 4: 16-byte aligned
        l[0] = a.x, l[1] = a.y, l[2] = a.z, l[3] = a.w;
        if (stereo) {
            const int4 b = *reinterpret_cast<const int4*>(right + f0);
            r[0] = b.x, r[1] = b.y, r[2] = b.z, r[3] = b.w;
        }
    } else {
#pragma unroll
        for (uint32_t i = 0; i < 3u; ++i) {
            if (i < nf) {
                l[i] = left[f0 + i];
                if (stereo) r[i] = right[f0 + i];
            }
        }
    }
    const uint32_t b0 = block_of_frame(frame_off, num_blocks, frame_base, f0);
    const unsigned long long split = frame_off[b0 + 1] - frame_base;  // frames from here on belong to block b0 + 1
    const uint32_t b1 = f0 + nf > split ? b0 + 1u : b0;
    const uint32_t st0 = status[b0], st1 = status[b1];
    const bool ms0 = stereo && ms_flag[b0] != 0, ms1 = stereo && ms_flag[b1] != 0;
    const long long lo = bit_depth == 16 ? -32768 : -0x800000, hi = bit_depth == 16 ? 32767 : 0x7FFFFF;
    const float scale = bit_depth == 16 ? 1.f / 32768.f : 1.f / 8388608.f;
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
        const unsigned long long g = f0 + i - w_start;  // (below the window it wraps to beyond it)
        if (i < nf && g < w_frames) {
            out_l[g] = f32 ? __float_as_uint((float)(int32_t)a * scale) : (uint32_t)(int32_t)a;
            if (stereo) out_r[g] = f32 ? __float_as_uint((float)(int32_t)b * scale) : (uint32_t)(int32_t)b;
        }
    }
    // blocks that did not decode are not checked (their status already fails the item)
    if (bad0 && st0 == 0u) atomicMax(&status[b0], 7u);
    if (bad1 && st1 == 0u) atomicMax(&status[b1], 7u);
}

// Every window item of a batch in one launch, laid out as k_wav_pack: thread u handles unit u of the concatenated unit
// ranges of the items' decoded frames (unit_off: [nitems + 1] prefix sums of ceil(frames / 4)); the item is found once
// per workgroup by a uniform binary search, and again per thread only in a workgroup that spans items.
__global__ __launch_bounds__(256) void k_window_out(uint32_t nitems, unsigned long long total_units,
                                                    const unsigned long long* __restrict__ unit_off,
                                                    const DecodeItem* __restrict__ items, const WindowOut* __restrict__ win,
                                                    const unsigned long long* __restrict__ frame_off,
                                                    const uint8_t* __restrict__ ms_flag, uint32_t* __restrict__ status,
                                                    int f32) {
    const unsigned long long first = (unsigned long long)blockIdx.x * 256u;
    uint32_t lo = 0, hi = nitems;  // unit_off[lo] <= first < unit_off[hi]
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (unit_off[mid] <= first) lo = mid;
        else hi = mid;
    }
    const unsigned long long u = first + threadIdx.x;
    if (u >= total_units) return;
    uint32_t j = lo;
    if (unit_off[lo + 1] < first + 256u) {  // (uniform) the workgroup spans items: this thread's, among the later ones
        uint32_t h2 = nitems;  // unit_off[j] <= u < unit_off[h2]
        while (h2 - j > 1u) {
            const uint32_t mid = j + (h2 - j) / 2u;
            if (unit_off[mid] <= u) j = mid;
            else h2 = mid;
        }
    }
    const DecodeItem& it = items[j];
    const WindowOut& w = win[j];
    window_out_unit(4ull * (u - unit_off[j]), it.blocks, it.channels, it.bit_depth, it.frames, frame_off + it.block0, it.frame0,
                    global_ptr(it.left), global_ptr(it.right), ms_flag + it.block0, status + it.block0, w.start, w.frames,
                    global_ptr(static_cast<uint32_t*>(w.left)), global_ptr(static_cast<uint32_t*>(w.right)), f32 != 0);
}

// Verify form: laid out as k_wav_pack and k_window_out -- thread u handles unit u of the concatenated unit
// ranges of the items' frames, the item found once per workgroup by a uniform binary search and again per thread only in a
// workgroup that spans items -- and verify_unit (verify_core.h) compares the unit's decoded frames with the item's source
// ver[j] instead of storing them.  What leaves: res[j].count += the differing samples, res[j].key = min(frame * 2 + channel)
// over them (the host sets 0 and all ones per call).  A wave in which nothing differs -- the common case -- issues no
// atomic at all.  Otherwise, in a workgroup that lies in one item, the wave reduces first: the count is the sum of the
// ballots' populations over the eight sample positions of a unit, and the wave's lowest key is that of the lowest lane
// that differs (the keys rise with the lane), which issues the wave's one atomicAdd and one atomicMin.  In a workgroup
// that spans items the lanes of a wave may belong to different items, and each lane that differs reports for itself.
__global__ __launch_bounds__(256) void k_verify(uint32_t nitems, unsigned long long total_units,
                                                const unsigned long long* __restrict__ unit_off,
                                                const DecodeItem* __restrict__ items, const VerifySource* __restrict__ ver,
                                                VerifyWords* __restrict__ res,
                                                const unsigned long long* __restrict__ frame_off,
                                                const uint8_t* __restrict__ ms_flag, uint32_t* __restrict__ status) {
    const unsigned long long first = (unsigned long long)blockIdx.x * 256u;
    uint32_t lo = 0, hi = nitems;  // unit_off[lo] <= first < unit_off[hi]
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (unit_off[mid] <= first) lo = mid;
        else hi = mid;
    }
    const unsigned long long u = first + threadIdx.x;
    const bool one_item = unit_off[lo + 1] >= first + 256u;  // (uniform) the whole workgroup lies in item lo
    uint32_t j = lo, differ = 0;
    unsigned long long f0 = 0;
    if (u < total_units) {
        if (!one_item) {  // this thread's item, among the later ones
            uint32_t h2 = nitems;  // unit_off[j] <= u < unit_off[h2]
            while (h2 - j > 1u) {
                const uint32_t mid = j + (h2 - j) / 2u;
                if (unit_off[mid] <= u) j = mid;
                else h2 = mid;
            }
        }
        const DecodeItem& it = items[j];
        const VerifySource& s = ver[j];
        f0 = 4ull * (u - unit_off[j]);
        differ = verify_unit(f0, it.blocks, it.channels, it.bit_depth, it.frames, frame_off + it.block0, it.frame0,
                             global_ptr(it.left), global_ptr(it.right), ms_flag + it.block0, status + it.block0,
                             global_ptr(s.data0), global_ptr(s.data1), s.layout);
    }
    const unsigned long long any = __ballot(differ != 0u);
    if (any == 0ull) return;
    const unsigned long long key = 2ull * f0 + (uint32_t)(__ffs((int)differ) - 1);
    if (one_item) {
        uint32_t n = 0;
#pragma unroll
        for (uint32_t b = 0; b < 8u; ++b) n += (uint32_t)__popcll(__ballot(((differ >> b) & 1u) != 0u));
        if ((threadIdx.x & 63u) == (uint32_t)(__ffsll((long long)any) - 1)) {
            atomicAdd(&res[j].count, (unsigned long long)n);
            atomicMin(&res[j].key, key);
        }
    } else if (differ) {
        atomicAdd(&res[j].count, (unsigned long long)__popc(differ));
        atomicMin(&res[j].key, key);
    }
}

// One thread per item, after k_verify: the block and the two values at an item's first mismatch (verify_fill_item).
__global__ __launch_bounds__(64) void k_verify_fill(uint32_t nitems, const DecodeItem* __restrict__ items,
                                                    const VerifySource* __restrict__ ver, VerifyWords* __restrict__ res,
                                                    const unsigned long long* __restrict__ frame_off,
                                                    const uint8_t* __restrict__ ms_flag) {
    const uint32_t j = blockIdx.x * 64u + threadIdx.x;
    if (j >= nitems) return;
    const DecodeItem& it = items[j];
    const VerifySource& s = ver[j];
    verify_fill_item(it.blocks, it.channels, frame_off + it.block0, it.frame0, global_ptr(it.left), global_ptr(it.right),
                     ms_flag + it.block0, global_ptr(s.data0), global_ptr(s.data1), s.layout, res[j], it.bit_depth);
}

// Salvage job, WAV form: laid out as k_wav_pack -- thread u handles unit u of the concatenated unit ranges of
// the items' frames, the item found once per workgroup by a uniform binary search and again per thread only in a workgroup
// that spans items.  Runs after k_ms_inverse: it reads the inverted samples and the FINAL status words, and writes every
// byte of every image's data region (salvage_wav_unit).  present[j]: the blocks of item j that had a lane.
__global__ __launch_bounds__(256) void k_salvage_wav(uint32_t nitems, unsigned long long total_units,
                                                     const unsigned long long* __restrict__ unit_off,
                                                     const DecodeItem* __restrict__ items, const uint32_t* __restrict__ present,
                                                     const unsigned long long* __restrict__ frame_off,
                                                     const uint32_t* __restrict__ status) {
    const unsigned long long first = (unsigned long long)blockIdx.x * 256u;
    uint32_t lo = 0, hi = nitems;  // unit_off[lo] <= first < unit_off[hi]
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (unit_off[mid] <= first) lo = mid;
        else hi = mid;
    }
    const unsigned long long u = first + threadIdx.x;
    if (u >= total_units) return;
    uint32_t j = lo;
    if (unit_off[lo + 1] < first + 256u) {  // (uniform) the workgroup spans items: this thread's, among the later ones
        uint32_t h2 = nitems;  // unit_off[j] <= u < unit_off[h2]
        while (h2 - j > 1u) {
            const uint32_t mid = j + (h2 - j) / 2u;
            if (unit_off[mid] <= u) j = mid;
            else h2 = mid;
        }
    }
    const DecodeItem& it = items[j];
    salvage_wav_unit(4ull * (u - unit_off[j]), it.blocks, present[j], it.channels, it.bit_depth, it.frames, frame_off + it.block0,
                     it.frame0, global_ptr(it.left), global_ptr(it.right), status + it.block0, global_ptr(it.wav));
}

// Salvage job, device form: grid = (all blocks of the batch, tiles) like k_ms_inverse, after it.  A block that decoded
// leaves at once (uniform: its item's record and present count as scalar loads, then one status word), so a healthy
// stream pays the launch and those loads; a lost block's frames in the caller's arrays become zeros (salvage_blank_tile).
__global__ __launch_bounds__(256) void k_salvage_blank(const uint32_t* __restrict__ blk_item, const DecodeItem* __restrict__ items,
                                                       const uint32_t* __restrict__ present,
                                                       const unsigned long long* __restrict__ frame_off,
                                                       const uint32_t* __restrict__ status) {
    const uint32_t blk = blockIdx.x, tile = blockIdx.y;
    const uint32_t j = blk_item[blk];
    const DecodeItem& it = items[j];
    if (!salvage_lost(status + it.block0, blk - it.block0, present[j])) return;  // (uniform) the block decoded
    const unsigned long long f0 = frame_off[blk];
    const uint32_t n = (uint32_t)(frame_off[blk + 1] - f0);
    salvage_blank_tile(tile, f0 - it.frame0, n, global_ptr(it.left), it.channels == 2 ? global_ptr(it.right) : nullptr, threadIdx.x);
}

hipError_t launch_decode(const DecodeArgs& a, hipStream_t stream) {
    const size_t smem = kDecBytesPerCol * kDecThreads;
    if (a.lanes) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_decode),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(k_decode, dim3((a.lanes + kDecThreads - 1) / kDecThreads), dim3(kDecThreads), smem, stream,
                           a.lanes, a.lane_blk, a.blk_item, a.items, a.payload, a.byte_off, a.frame_off, a.status, a.ms_flag);
    }
    if (a.nv2) {  // version-2 items: a batch without any pays nothing for them
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_decode_serial),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(k_decode_serial, dim3((a.nv2 + kDecThreads - 1) / kDecThreads), dim3(kDecThreads), smem,
                           stream, a.nv2, a.v2_items, a.items, a.payload, a.frame_off, a.status, a.ms_flag);
    }
    if (a.present) {  // salvage: two passes in stream order (status 7 is final only after the first)
        if (a.total_blocks) {
            hipLaunchKernelGGL(k_ms_inverse, dim3(a.total_blocks, kMaxBlock / 1024), dim3(256), 0, stream, a.blk_item, a.items,
                               a.frame_off, a.ms_flag, a.status);
            if (a.block_raw) {  // the block digests of what decoded, then the judge: status 11 before anything leaves
                hipError_t e = launch_digest_blocks(a, stream);
                if (e != hipSuccess) return e;
            }
            if (a.no_output) return hipGetLastError();  // the blocks form: nothing leaves but statuses and digests
            if (a.wav) {
                if (a.total_units)
                    hipLaunchKernelGGL(k_salvage_wav, dim3((uint32_t)((a.total_units + 255u) / 256u)), dim3(256), 0, stream, a.nitems,
                                       a.total_units, a.unit_off, a.items, a.present, a.frame_off, a.status);
            } else {
                hipLaunchKernelGGL(k_salvage_blank, dim3(a.total_blocks, kMaxBlock / 1024), dim3(256), 0, stream, a.blk_item, a.items,
                                   a.present, a.frame_off, a.status);
            }
        }
    } else if (a.digest) {
        if (a.total_units) return launch_digest(a, stream);
    } else if (a.verify) {
        if (a.total_units) {
            hipLaunchKernelGGL(k_verify, dim3((uint32_t)((a.total_units + 255u) / 256u)), dim3(256), 0, stream, a.nitems,
                               a.total_units, a.unit_off, a.items, a.verify, a.verify_res, a.frame_off, a.ms_flag, a.status);
            hipLaunchKernelGGL(k_verify_fill, dim3((a.nitems + 63u) / 64u), dim3(64), 0, stream, a.nitems, a.items, a.verify,
                               a.verify_res, a.frame_off, a.ms_flag);
        }
    } else if (a.window) {
        if (a.total_units)
            hipLaunchKernelGGL(k_window_out, dim3((uint32_t)((a.total_units + 255u) / 256u)), dim3(256), 0, stream, a.nitems,
                               a.total_units, a.unit_off, a.items, a.window, a.frame_off, a.ms_flag, a.status, a.f32 ? 1 : 0);
    } else if (a.wav) {
        if (a.total_units)
            hipLaunchKernelGGL(k_wav_pack, dim3((uint32_t)((a.total_units + 255u) / 256u)), dim3(256), 0, stream, a.nitems,
                               a.total_units, a.unit_off, a.items, a.frame_off, a.ms_flag, a.status);
    } else if (a.total_blocks) {
        hipLaunchKernelGGL(k_ms_inverse, dim3(a.total_blocks, kMaxBlock / 1024), dim3(256), 0, stream, a.blk_item, a.items,
                           a.frame_off, a.ms_flag, a.status);
    }
    return hipGetLastError();
}

}  // namespace lacx
