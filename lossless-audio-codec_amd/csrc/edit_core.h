// edit_core.h -- the per-thread code of the edit pass (k_edit of k_edit.hip), the one kernel of a transcode job
// (lacx_transcode_batch, api_transcode.cpp) that is new: it stands between the window job that splices every output's
// segments into planar int32 staging rows and the encoder's front kernels.  It applies an output's channel operation and
// its lossless depth change, validates both, and writes the layout those kernels read fastest (interleaved int16 at depth
// 16, packed interleaved int24 at depth 24).  Written like import_core.h, whose loads and int24 packing it shares (import_quad
// itself is left as it is: its store is restated below, so that k_import's code does not change): the same source compiles
// into the gfx950 kernel and into a host program the tests run under AddressSanitizer / UBSan (tests/native/sim_edit.cpp);
// every load of the staging and every store of the destination is in here, and the twin hands it heap blocks of exactly
// the planned sizes.
#pragma once
#include <cstdint>

#include "import_core.h"

namespace lacx {

// lacx_edit_output.channel_op (include/lacx.h: LACX_CH_*)
enum : int { CH_KEEP = 0, CH_LEFT = 1, CH_RIGHT = 2, CH_FOLD = 3, CH_SWAP = 4, CH_DUAL = 5, CH_OPS = 6 };

constexpr uint32_t kEditQuad = kImportQuad;            // frames per thread
constexpr uint32_t kEditThreads = kImportThreads;      // threads per workgroup
constexpr uint32_t kEditUnitFrames = kImportUnitFrames;  // frames per unit: one workgroup, inside one output

// One output of an edit job.  left / right: its staging rows, 16-byte aligned, `frames` int32 each (right: stereo sources
// only).  dst: 16-byte aligned, frames * channels_out * (dst_depth / 8) bytes.
struct EditItem {
    const int32_t* left;
    const int32_t* right;
    void* dst;
    unsigned long long frames;
    uint8_t src_channels, channel_op, src_depth, dst_depth, pad[4];
};
// What an output's validation leaves: the lowest frame * 4 + kind of a violation -- kind 0: left and right differ (FOLD),
// 1 / 2: the output's left / right sample is no multiple of 256 (24 -> 16).  Within a frame the channel operation comes
// first, then left before right.  All ones: none.
struct EditBad {
    unsigned long long key;
};
constexpr unsigned long long kEditClean = ~0ull;

// The job: the outputs' table with the prefix sums of their unit counts.
struct EditJob {
    const EditItem* table;
    const unsigned long long* unit_off;  // [nitems + 1]
    uint32_t nitems, pad;
    unsigned long long total_units;
};

LACX_HDF uint32_t edit_channels_out(uint32_t src_channels, uint32_t channel_op) {
    return channel_op == (uint32_t)CH_KEEP || channel_op == (uint32_t)CH_SWAP ? src_channels : channel_op == (uint32_t)CH_DUAL ? 2u : 1u;
}

// One sample through an output's depth change; false: a 24-bit sample that 16 bits cannot carry.  Nothing is rounded.
LACX_HDF bool edit_depth(int32_t s, int src_depth, int dst_depth, int32_t& out) {
    if (src_depth == dst_depth) return out = s, true;
    if (dst_depth == 24) return out = (int32_t)((uint32_t)s << 8), true;
    out = s >> 8;
    return (s & 0xFF) == 0;
}

// The quad's store, import_quad's restated: frames f0 .. f0 + nf - 1 (f0 a multiple of 4, nf 1..4; l / r the channels'
// samples, r unused for mono) into dst, interleaved int16 (depth 16) or packed int24 (depth 24), dst 16-byte aligned.  A
// whole quad's 8 / 16 or 12 / 24 bytes go out as dwords at their natural alignment, a partial one as elements / bytes:
// nothing outside [dst, dst + frames * channels * depth / 8) is written.  The staged samples lie inside the source depth
// (the window job checks every decoded sample against it: status 7), so nothing is cut off here.
LACX_HDF void edit_store_quad(void* dst, int depth, bool stereo, unsigned long long f0, uint32_t nf, const int32_t* l, const int32_t* r) {
    using namespace import_detail;
    int32_t s[8];  // the quad's samples in stream order
    const uint32_t ns = stereo ? 2u * nf : nf;
#pragma unroll
    for (uint32_t i = 0; i < 4u; ++i) {
        if (stereo) s[2u * i] = l[i], s[2u * i + 1u] = r[i];
        else s[i] = l[i], s[4u + i] = 0;
    }
    if (depth == 16) {
        int16_t* d = static_cast<int16_t*>(dst) + f0 * (stereo ? 2u : 1u);
        if (nf == 4u) {
            uint32_t w[4];
#pragma unroll
            for (uint32_t i = 0; i < 4u; ++i) w[i] = ((uint32_t)s[2u * i] & 0xFFFFu) | ((uint32_t)s[2u * i + 1u] << 16);
            if (stereo) __builtin_memcpy(__builtin_assume_aligned(d, 16), w, 16);
            else __builtin_memcpy(__builtin_assume_aligned(d, 8), w, 8);
        } else {
#pragma unroll
            for (uint32_t i = 0; i < 6u; ++i)
                if (i < ns) d[i] = (int16_t)s[i];
        }
    } else {
        uint8_t* d = static_cast<uint8_t*>(dst) + 3u * f0 * (stereo ? 2u : 1u);
        if (nf == 4u) {
            uint32_t w[6];
            pack24x4(s, w);
            if (stereo) {
                pack24x4(s + 4, w + 3);
                __builtin_memcpy(__builtin_assume_aligned(d, 8), w, 24);
            } else {
                __builtin_memcpy(__builtin_assume_aligned(d, 4), w, 12);
            }
        } else {
#pragma unroll
            for (uint32_t i = 0; i < 6u; ++i) {
                if (i < ns) {
                    const uint32_t v = (uint32_t)s[i];
                    d[3u * i] = (uint8_t)v, d[3u * i + 1u] = (uint8_t)(v >> 8), d[3u * i + 2u] = (uint8_t)(v >> 16);
                }
            }
        }
    }
}

// One thread's work: frames f0 .. f0 + 3 of an output (f0 a multiple of 4, below it.frames).  Loads: 16 bytes per staging
// row, the output's partial last quad element by element: nothing outside [0, frames) of a row is read.  Stores:
// edit_store_quad: nothing outside [dst, dst + frames * channels_out * dst_depth / 8) is written.  A frame
// that breaks a rule is stored as if it did not (FOLD: the left sample; a narrowed sample: s >> 8) and lowers key.
LACX_HDF void edit_quad(const EditItem& it, unsigned long long f0, unsigned long long& key) {
    using namespace import_detail;
    const uint32_t nf = it.frames - f0 >= 4u ? 4u : (uint32_t)(it.frames - f0);
    const bool src_stereo = it.src_channels == 2;
    uint32_t a[4] = {0, 0, 0, 0}, b[4] = {0, 0, 0, 0};
    load_u32x4(reinterpret_cast<const uint32_t*>(it.left) + f0, true, nf, a);
    if (src_stereo) load_u32x4(reinterpret_cast<const uint32_t*>(it.right) + f0, true, nf, b);
    const uint32_t op = it.channel_op;
    const bool stereo = edit_channels_out(it.src_channels, op) == 2u;
    int32_t l[4] = {0, 0, 0, 0}, r[4] = {0, 0, 0, 0};
#pragma unroll
    for (uint32_t i = 0; i < 4u; ++i) {
        if (i >= nf) continue;
        const int32_t sl = (int32_t)a[i], sr = (int32_t)b[i];
        const int32_t ol = op == (uint32_t)CH_RIGHT || op == (uint32_t)CH_SWAP ? sr : sl;
        const int32_t orr = op == (uint32_t)CH_SWAP || op == (uint32_t)CH_DUAL ? sl : sr;
        unsigned long long k = kEditClean;
        if (!edit_depth(orr, it.src_depth, it.dst_depth, r[i]) && stereo) k = 4u * (f0 + i) + 2u;
        if (!edit_depth(ol, it.src_depth, it.dst_depth, l[i])) k = 4u * (f0 + i) + 1u;
        if (op == (uint32_t)CH_FOLD && sl != sr) k = 4u * (f0 + i);
        key = k < key ? k : key;
    }
    edit_store_quad(it.dst, it.dst_depth, stereo, f0, nf, l, r);
}

}  // namespace lacx
