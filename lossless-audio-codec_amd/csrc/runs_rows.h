// runs_rows.h -- the runs of one (item, detector) as the host side finishes them from what the device left (runs_core.h):
// the runs that touch a tile edge stitched from the tiles' rows, merged with the interior runs of the device's list, sorted
// by start, and their totals.  Host only, no HIP: the C ABI (api_decode.cpp) and tests/native/sim_runs.cpp, which calls
// the same code the ABI calls.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "lacx.h"
#include "runs_core.h"
#include "runs_plan.h"

namespace lacx {

// The runs that touch a tile edge.  rows: the item's, row of (tile, detector) at rows[tile * ndet + det].  A tile whose
// lead is its whole length only extends the run that is open; any other tile closes it with its lead and opens the next
// with its trail.  A run as long as the stream is one addition per tile.
inline void runs_stitch(uint64_t frames, const RunsRow* rows, uint32_t ndet, uint32_t det, uint64_t min_frames, std::vector<lacx_run>& out) {
    const uint64_t tiles = (frames + kRunsTileFrames - 1u) / kRunsTileFrames;
    uint64_t start = 0, open = 0;  // the open run: `open` frames from `start` on, up to the current tile's first frame
    for (uint64_t t = 0; t < tiles; ++t) {
        const uint64_t at = t * kRunsTileFrames, n = frames - at < kRunsTileFrames ? frames - at : kRunsTileFrames;
        const RunsRow& r = rows[t * ndet + det];
        if (r.lead == n) {  // every frame of the tile
            if (!open) start = at;
            open += n;
            continue;
        }
        if (open + r.lead) {
            if (!open) start = at;
            if (open + r.lead >= min_frames) out.push_back(lacx_run{start, open + r.lead});
        }
        open = r.trail;
        start = at + n - r.trail;
    }
    if (open && open >= min_frames) out.push_back(lacx_run{start, open});
}

// The finished list of a detector: stitched and interior runs (the first min(count, cap) entries the device stored), by
// start.
inline void runs_finish(uint64_t frames, const RunsRow* rows, uint32_t ndet, uint32_t det, uint64_t min_frames, const lacx_run* interior,
                        uint64_t stored, std::vector<lacx_run>& out) {
    out.assign(interior, interior + stored);
    runs_stitch(frames, rows, ndet, det, min_frames, out);
    std::sort(out.begin(), out.end(), [](const lacx_run& a, const lacx_run& b) { return a.start < b.start; });
}

inline lacx_run_totals runs_totals(const std::vector<lacx_run>& runs) {
    lacx_run_totals t{};
    t.runs = runs.size();
    for (const lacx_run& r : runs) {
        t.frames += r.frames;
        if (r.frames > t.longest) t.longest = r.frames, t.longest_start = r.start;
    }
    return t;
}

// Item j's finished lists and their totals from the job's tables at h (runs_plan.h, as they came back from the device)
// and the entries of its list buffer.  The caller fills what the job knows beside the runs: losses, format, flags.
inline lacx_runs_result runs_item_result(const RunsLayout& y, const uint8_t* h, const lacx_run* entries, size_t j, uint64_t frames,
                                         std::vector<std::vector<lacx_run>>& out) {
    const RunsItem& it = reinterpret_cast<const RunsItem*>(h + y.items)[j];
    const auto* dets = reinterpret_cast<const lacx_run_detector*>(h + y.dets);
    const auto* lists = reinterpret_cast<const RunsList*>(h + y.lists);
    const RunsRow* rows = reinterpret_cast<const RunsRow*>(h + y.rows) + it.row0;
    lacx_runs_result res{};
    res.frames = frames;
    res.detectors = (uint8_t)it.ndet;
    out.assign(it.ndet, {});
    for (uint32_t k = 0; k < it.ndet; ++k) {
        const RunsList& l = lists[it.det0 + k];
        runs_finish(frames, rows, it.ndet, k, dets[it.det0 + k].min_frames, entries + l.off, l.count < l.cap ? l.count : l.cap, out[k]);
        res.det[k] = runs_totals(out[k]);
    }
    return res;
}

}  // namespace lacx
