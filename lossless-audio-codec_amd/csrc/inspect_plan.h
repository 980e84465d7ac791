// inspect_plan.h -- the plan of an inspection job (lacx_decoder_inspect_batch_device), host only, no HIP.  A form of
// plan_decode that leaves plan_decode alone: the items are read by the lenient reader and laid out exactly as a salvage
// job's -- payloads back to back, the block tables as global prefix sums, one lane per present version-3 block and one
// per version-2 item -- and then everything a decode needs beyond that is taken away again: no PCM buffers, no image, no
// stage, no status words, no post-pass units.  Behind the salvage job's tables come the rows, which only ever travel
// from the device to the host, and with LACX_INSPECT_PARTITIONS the partition entries.
#pragma once
#include "decode_plan.h"

namespace lacx {

constexpr size_t kInspectRowBytes = 336;        // sizeof(lacx_block_info)
constexpr size_t kInspectPartModeBytes = 2 * kInspectPartSlots;      // per block: mode_k [2][256]
constexpr size_t kInspectPartBitsBytes = 2 * kInspectPartSlots * 4;  // per block: part_bits [2][256]
static_assert(sizeof(lacx_block_info) == kInspectRowBytes && sizeof(lacx_channel_info) == 160, "the rows have fixed sizes (lacx.h)");

struct InspectPlan {
    DecodePlan base;  // items, lanes, totals and the uploaded tables: items .. present [m], base.at.size bytes
    bool partitions = false;
    // inside the tables buffer, behind the uploaded part, device to host only: rows [T] (16-byte aligned), then for a job
    // with partition detail mode_k [T][2][256] (bytes) | part_bits [T][2][256] (words, 16-byte aligned)
    size_t at_rows = 0, at_mode_k = 0, at_part_bits = 0;
    // What the run must provide: payload bytes (kDecodeTailPad behind the last block included), tables bytes (the
    // uploaded part, the rows and the partition entries), rows and part_rows: how many of each lie in there.
    struct {
        uint64_t payload, tables, rows, part_rows;
    } need{};
};

inline const char* plan_inspect(const BatchIn* in, uint32_t n, bool partitions, bool pad_waves, InspectPlan& plan, std::vector<int>& code,
                                std::vector<std::string>& err) {
    using plan_detail::up16;
    plan = InspectPlan{};
    plan.partitions = partitions;
    DecodePlan& b = plan.base;
    if (const char* whole = plan_decode(in, n, DecodeForm::blocks, kWholeStreams, pad_waves, b, code, err, true, true)) return whole;
    // a salvage job's items and tables, and nothing of its decode: no block digests, no PCM, no post pass
    b.blocks = b.judged = false;
    b.total_units = 0;
    b.pcm_total = 0;
    for (PlanItem& p : b.items) p.pcm_at = 0;
    const size_t m = b.items.size(), T = (size_t)b.total_blocks;
    // What is kept of the tables is the plain salvage job's: everything up to v2_items, then present [m] (uint32) at
    // `win`, 16-byte aligned (TableLayout, decode_plan.h).  The block digests' tables lay behind that and are dropped.  A
    // change to that order in plan_decode must be made here too; the layout is checked rather than trusted.
    if (b.at.win != up16(b.at.v2_items + 4 * b.v2_items.size()) || b.at.judged != b.at.win + 4 * m || b.at.raw < b.at.judged + 4 * m)
        return "the salvage job's table layout is not the one the inspection plan was written for";
    b.at.res = b.at.win;
    b.at.size = b.at.judged;  // the end of present [m]: the salvage job's size without block digests
    b.at.judged = b.at.raw = b.at.expect = 0;
    plan.at_rows = up16(b.at.size);
    plan.at_mode_k = plan.at_rows + kInspectRowBytes * T;
    plan.at_part_bits = up16(plan.at_mode_k + (partitions ? kInspectPartModeBytes * T : 0));
    b.need.blocks = b.need.pcm_frames = b.need.image = b.need.stage = b.need.stats_rows = 0;
    b.need.tables = partitions ? plan.at_part_bits + kInspectPartBitsBytes * T : plan.at_mode_k;
    plan.need.payload = b.need.payload;
    plan.need.tables = b.need.tables;
    plan.need.rows = T;
    plan.need.part_rows = partitions ? T : 0;
    return nullptr;
}

// The kernels' arguments: the decode's own tables (plan_args of the base plan) and the rows behind them.
inline InspectArgs plan_inspect_args(const InspectPlan& plan, const uint8_t* tables, const uint8_t* payload) {
    InspectArgs a;
    a.dec = plan_args(plan.base, tables, payload, nullptr, nullptr);
    uint8_t* t = const_cast<uint8_t*>(tables);
    a.rows = reinterpret_cast<lacx_block_info*>(t + plan.at_rows);
    if (plan.partitions) {
        a.mode_k = t + plan.at_mode_k;
        a.part_bits = reinterpret_cast<uint32_t*>(t + plan.at_part_bits);
    }
    return a;
}

}  // namespace lacx
