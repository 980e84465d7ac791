// runs_plan.h -- the host-only plan of a runs job (lacx.h: lacx_decoder_runs_*): the checks of an item's detectors, the
// tables k_runs reads and writes (runs_core.h) and the list reservation.  Plain C++, no HIP: decode_plan.h puts these
// tables behind a salvage job's (the stream form), api_decode.cpp behind the source form's; tests/native/sim_runs.cpp runs
// the same plan on the host.
// The tables, from a 16-byte aligned base: tile_off [m + 1] (uint64) | items [m] (RunsItem) | dets [D] (lacx_run_detector)
// | lists [D] (RunsList) | rows [sum of tiles * detectors] (RunsRow).  lists and rows are what comes back.
// The list buffer is the run's own (RunsLayout::list_entries entries of lacx_run): detector q of the job owns
// [lists[q].off, lists[q].off + lists[q].cap).
#pragma once
#include <cstdint>
#include <cstring>
#include <vector>

#include "lacx.h"
#include "lacx_types.h"
#include "runs_core.h"

namespace lacx {

constexpr uint64_t kRunsListCap = 8192;  // R: the entries reserved per detector at most (lacx.h)

// An item's detectors inside the call's array, or why not (lacx.h's texts).
inline const char* check_detectors(const lacx_run_query& q, const lacx_run_detector* dets, uint32_t ndets) {
    if (q.first_detector > ndets || q.detectors > ndets - q.first_detector) return "detectors outside the call's array";
    if (q.detectors > LACX_MAX_DETECTORS) return "too many detectors";
    if (q.detectors == 0) return "item has no detectors";
    for (uint32_t k = 0; k < q.detectors; ++k) {
        const lacx_run_detector& d = dets[q.first_detector + k];
        if (d.kind > LACX_RUN_FLAT) return "unknown detector kind";
        if (d.channel > 1u && d.channel != LACX_RUN_ALL) return "unknown detector channel";
        if (d.min_frames == 0) return "detector needs min_frames >= 1";
        if (d.kind == LACX_RUN_FLAT && d.level != 0) return "flat detector takes no level";
    }
    return nullptr;
}

// The most runs of at least min_frames frames that `frames` frames hold -- runs need a frame between them -- capped at R.
inline uint64_t runs_reserve(uint64_t frames, uint64_t min_frames, uint64_t cap) {
    const uint64_t most = min_frames > frames ? 0u : (frames + 1u) / (min_frames + 1u);
    return most < cap ? most : cap;
}

struct RunsIn {  // one item that goes to the device
    const lacx_run_detector* dets;
    uint32_t ndet;
    uint64_t frames;
};

struct RunsLayout {
    size_t base = 0, tile_off = 0, items = 0, dets = 0, lists = 0, rows = 0, size = 0;  // byte offsets in the tables; size: their end
    uint64_t total_tiles = 0, total_dets = 0, total_rows = 0;
    uint64_t list_entries = 0;  // the list buffer, set by runs_fill / runs_recap
};

inline RunsLayout runs_layout(size_t base, const RunsIn* in, size_t m) {
    RunsLayout y;
    for (size_t j = 0; j < m; ++j) {
        const uint64_t tiles = (in[j].frames + kRunsTileFrames - 1u) / kRunsTileFrames;
        y.total_tiles += tiles;
        y.total_dets += in[j].ndet;
        y.total_rows += tiles * in[j].ndet;
    }
    y.base = y.tile_off = base;
    y.items = y.tile_off + 8 * (m + 1);
    y.dets = y.items + sizeof(RunsItem) * m;
    y.lists = y.dets + sizeof(lacx_run_detector) * (size_t)y.total_dets;
    y.rows = y.lists + sizeof(RunsList) * (size_t)y.total_dets;
    y.size = y.rows + sizeof(RunsRow) * (size_t)y.total_rows;
    return y;
}

// Fills the tables at h (the tables' first byte, not the base's); the lists reserve runs_reserve entries each.
inline void runs_fill(RunsLayout& y, const RunsIn* in, size_t m, uint64_t list_cap, uint8_t* h) {
    auto* tile_off = reinterpret_cast<unsigned long long*>(h + y.tile_off);
    auto* items = reinterpret_cast<RunsItem*>(h + y.items);
    auto* dets = reinterpret_cast<lacx_run_detector*>(h + y.dets);
    auto* lists = reinterpret_cast<RunsList*>(h + y.lists);
    uint64_t row = 0, det = 0, entry = 0;
    tile_off[0] = 0;
    for (size_t j = 0; j < m; ++j) {
        const uint64_t tiles = (in[j].frames + kRunsTileFrames - 1u) / kRunsTileFrames;
        tile_off[j + 1] = tile_off[j] + tiles;
        items[j] = RunsItem{row, (uint32_t)det, in[j].ndet};
        for (uint32_t k = 0; k < in[j].ndet; ++k, ++det) {
            dets[det] = in[j].dets[k];
            const uint64_t cap = runs_reserve(in[j].frames, in[j].dets[k].min_frames, list_cap);
            lists[det] = RunsList{entry, cap, 0};
            entry += cap;
        }
        row += tiles * in[j].ndet;
    }
    std::memset(h + y.rows, 0, y.size - y.rows);
    y.list_entries = entry;
}

// What the counters say once k_runs ran: true where a list outgrew its capacity.
inline bool runs_overflowed(const RunsLayout& y, const uint8_t* h) {
    const auto* lists = reinterpret_cast<const RunsList*>(h + y.lists);
    for (uint64_t q = 0; q < y.total_dets; ++q)
        if (lists[q].count > lists[q].cap) return true;
    return false;
}

// The lists once more with exactly the capacities the counters gave, the counters zero again.
inline void runs_recap(RunsLayout& y, uint8_t* h) {
    auto* lists = reinterpret_cast<RunsList*>(h + y.lists);
    uint64_t entry = 0;
    for (uint64_t q = 0; q < y.total_dets; ++q) {
        lists[q] = RunsList{entry, lists[q].count, 0};
        entry += lists[q].cap;
    }
    y.list_entries = entry;
}

// k_runs's arguments: the tables at `tables` (where the kernel sees them) and the list buffer.
inline void runs_args(const RunsLayout& y, size_t m, const uint8_t* tables, lacx_run* list, RunsArgs& a) {
    uint8_t* t = const_cast<uint8_t*>(tables);
    a.nitems = (uint32_t)m;
    a.total_tiles = y.total_tiles;
    a.tile_off = reinterpret_cast<const unsigned long long*>(t + y.tile_off);
    a.items = reinterpret_cast<const RunsItem*>(t + y.items);
    a.dets = reinterpret_cast<const lacx_run_detector*>(t + y.dets);
    a.lists = reinterpret_cast<RunsList*>(t + y.lists);
    a.rows = reinterpret_cast<RunsRow*>(t + y.rows);
    a.runs = list;
}

}  // namespace lacx
