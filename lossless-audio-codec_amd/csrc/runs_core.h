// runs_core.h -- the per-thread code of the run finder (k_runs of k_runs.hip): where along a stream, or along device-resident
// source PCM, the frames that satisfy a detector's predicate (lacx.h: QUIET, PEAK, FLAT) lie as runs of consecutive frames,
// and which of those runs reach min_frames.  All of it exact integer arithmetic.
// A thread takes one unit of four frames, as in stats_core.h; a workgroup of kRunsThreads threads takes one TILE of
// kRunsTileFrames consecutive frames of one item (an item's tiles start at its frame 0, so no tile spans items).  Per
// detector a thread turns its unit into a 4-bit mask (runs_mask), the mask into a summary (runs_summary), the summaries of
// the tile's threads combine with the associative operator runs_combine -- a segmented scan, which gives every thread the
// length of the run that enters its unit -- and the thread then walks its four frames (runs_walk): a run that ends in the
// unit is the tile's LEAD where it reaches back to the tile's first frame, and is otherwise emitted if it reaches
// min_frames; the run that leaves the tile's last unit is the tile's TRAIL.  Lead and trail are the tile's row; the host
// stitches the runs that touch tile edges from the rows (runs_rows.h).
// A frame that does not exist (behind the item's end) or lies in a block that does not count (stream form: missing or
// lost) satisfies no predicate, so it ends a run like any other frame outside it.
// Stream form: the samples are read AFTER k_ms_inverse ran in place, with the loads and the frame_off / present / status
// rules of stats_unit_decoded.  Source form: the loads, bounds and validation keys are stats_load_source's own.
// Written like stats_core.h: the same source compiles into the gfx950 kernel and into a host program the tests run under
// AddressSanitizer / UBSan (tests/native/sim_runs.cpp).
#pragma once
#include <cstdint>

#include "lacx.h"
#include "stats_core.h"

namespace lacx {

constexpr uint32_t kRunsThreads = 256;                                  // units per workgroup of k_runs
constexpr uint32_t kRunsTileFrames = kRunsThreads * kDigestUnitFrames;  // 1024
static_assert(16384u % kRunsTileFrames == 0, "a tile divides the largest block");
constexpr uint32_t kRunsAll = 0x80000000u;  // a summary: bit 31 every frame is set, below it the trailing set frames

// The device tables of a runs job (runs_plan.h lays them out): per item its detectors and its first row; per (item,
// detector) the list region of its interior runs and the counter, which counts every run whether it was stored or not.
struct RunsItem {  // 16 bytes
    unsigned long long row0;  // the item's rows: row0 + tile * ndet + detector
    uint32_t det0, ndet;      // its detectors: det0 .. det0 + ndet - 1 of the job's
};
struct RunsList {  // 24 bytes, one per detector of the job
    unsigned long long off, cap;  // entries off .. off + cap - 1 of the job's list buffer
    unsigned long long count;     // zero on entry
};
struct RunsRow {  // 4 bytes, zero on entry
    uint16_t lead, trail;  // the set frames at the tile's start and at its end (both kRunsTileFrames: every frame)
};
static_assert(sizeof(RunsItem) == 16 && sizeof(RunsList) == 24 && sizeof(RunsRow) == 4 && sizeof(lacx_run_detector) == 16 && sizeof(lacx_run) == 16,
              "the device tables of a runs job have fixed strides");

struct RunsUnit {
    int32_t l[4], r[4];
    uint32_t counted;  // bit i: frame f0 + i exists and its block counts
};

// (a then b) of two summaries
LACX_HDF uint32_t runs_combine(uint32_t a, uint32_t b) {
    return (b & kRunsAll) ? ((a & kRunsAll) | ((a & ~kRunsAll) + (b & ~kRunsAll))) : b;
}
constexpr uint32_t kRunsIdentity = kRunsAll;  // every frame of no frames

LACX_HDF uint32_t runs_summary(uint32_t mask) {
    if (mask == 15u) return kRunsAll | 4u;
    return (mask & 8u) ? ((mask & 4u) ? ((mask & 2u) ? 3u : 2u) : 1u) : 0u;
}

LACX_HDF bool runs_sample(uint32_t kind, uint32_t level, int32_t x, int32_t prev) {
    const long long v = x, lv = level;
    if (kind == LACX_RUN_QUIET) return v >= -lv && v <= lv;
    if (kind == LACX_RUN_PEAK) return v >= lv || v <= -lv - 1;
    return x == prev;  // LACX_RUN_FLAT
}

// The unit's frames that satisfy detector d.  pl / pr / pc: the frame in front of the unit -- its samples and whether it
// is counted (false for the item's frame 0).
LACX_HDF uint32_t runs_mask(const lacx_run_detector& d, const RunsUnit& u, int32_t pl, int32_t pr, bool pc, bool stereo) {
    const bool left = d.channel != 1u, right = stereo && d.channel != 0u;
    if (!left && !right) return 0u;  // channel 1 of a mono item
    uint32_t mask = 0;
#pragma unroll
    for (uint32_t i = 0; i < 4u; ++i) {
        const int32_t ql = i ? u.l[i - 1u] : pl, qr = i ? u.r[i - 1u] : pr;
        const bool qc = i ? ((u.counted >> (i - 1u)) & 1u) != 0 : pc;
        bool p = ((u.counted >> i) & 1u) != 0 && (d.kind != LACX_RUN_FLAT || qc);
        if (left) p = p && runs_sample(d.kind, d.level, u.l[i], ql);
        if (right) p = p && runs_sample(d.kind, d.level, u.r[i], qr);
        mask |= p ? 1u << i : 0u;
    }
    return mask;
}

struct RunsWalk {
    uint32_t lead;  // != 0: the run that starts at the tile's first frame ended in this unit, this long
    uint32_t exit;  // the set frames at the unit's end, with those that entered where every frame is set
};

// The unit's four frames from f0 on (item frames) with `enter` set frames in front of them inside the tile, which starts
// at tile_start.  emit(start, frames) for every run that ends here, does not start the tile and reaches min_frames.
template <typename Emit>
LACX_HDF RunsWalk runs_walk(uint32_t mask, uint32_t enter, unsigned long long f0, unsigned long long tile_start, unsigned long long min_frames,
                            Emit emit) {
    RunsWalk w{0u, enter};
#pragma unroll
    for (uint32_t i = 0; i < 4u; ++i) {
        if ((mask >> i) & 1u) {
            ++w.exit;
        } else if (w.exit) {
            const unsigned long long start = f0 + i - w.exit;
            if (start == tile_start) w.lead = w.exit;
            else if (w.exit >= min_frames) emit(start, (unsigned long long)w.exit);
            w.exit = 0;
        }
    }
    return w;
}

// Stream form.  Frames f0 .. f0 + 3 of an item (f0 a multiple of 4, f0 < frames) from left / right as k_ms_inverse left
// them, loaded as stats_unit_decoded loads them; a frame counts when its block had a lane (index < present) and its
// status is 0.  frame_off and status are the item's own, frame_base the value of frame_off[0].
LACX_HDF RunsUnit runs_unit_decoded(unsigned long long f0, uint32_t num_blocks, uint32_t present, int channels, unsigned long long frames,
                                    const unsigned long long* __restrict__ frame_off, unsigned long long frame_base,
                                    const int32_t* __restrict__ left, const int32_t* __restrict__ right, const uint32_t* __restrict__ status) {
    const uint32_t nf = frames - f0 >= 4u ? 4u : (uint32_t)(frames - f0);
    const bool stereo = channels == 2;
    RunsUnit u{{0, 0, 0, 0}, {0, 0, 0, 0}, 0u};
    if (nf == 4u && ((uintptr_t)left & 15u) == 0 && (!stereo || ((uintptr_t)right & 15u) == 0)) {
        __builtin_memcpy(u.l, __builtin_assume_aligned(left + f0, 16), 16);
        if (stereo) __builtin_memcpy(u.r, __builtin_assume_aligned(right + f0, 16), 16);
    } else {
#pragma unroll
        for (uint32_t i = 0; i < 4u; ++i) {
            if (i < nf) {
                u.l[i] = left[f0 + i];
                if (stereo) u.r[i] = right[f0 + i];
            }
        }
    }
    const uint32_t b0 = verify_block_of_frame(frame_off, num_blocks, frame_base, f0);
    const unsigned long long split = frame_off[b0 + 1] - frame_base;  // frames from here on belong to block b0 + 1
    const uint32_t k = split - f0 >= nf ? nf : (uint32_t)(split - f0);
    const bool use0 = b0 < present && status[b0] == 0u;
    const bool use1 = k < nf && b0 + 1u < present && status[b0 + 1u] == 0u;  // (k < nf: block b0 + 1 exists)
    const uint32_t all = (1u << nf) - 1u, first = (1u << k) - 1u;
    u.counted = (use0 ? first : 0u) | (use1 ? all & ~first : 0u);
    return u;
}

// Source form: every frame that exists counts; an invalid sample lowers `key` exactly as in stats_unit_source.
LACX_HDF RunsUnit runs_unit_source(unsigned long long f0, int channels, int bit_depth, unsigned long long frames, const void* __restrict__ src0,
                                   const void* __restrict__ src1, uint32_t layout, unsigned long long& key) {
    const uint32_t nf = frames - f0 >= 4u ? 4u : (uint32_t)(frames - f0);
    RunsUnit u{{0, 0, 0, 0}, {0, 0, 0, 0}, (1u << nf) - 1u};
    stats_load_source(f0, nf, channels, bit_depth, src0, src1, layout, key, u.l, u.r);
    return u;
}

}  // namespace lacx
