// edit_plan.h -- the host-only half of a transcode job (lacx_transcode_batch, api_transcode.cpp): the per-output checks,
// the mapping of segments to the window items of phase 1, where every output's staging rows and destination lie with the
// capacities the run must provide, the unit prefix sums of k_edit and its per-output transform table (EditItem,
// edit_core.h).  Plain C++, no HIP: api_transcode.cpp runs a plan on the device, tests/native/dump_edit_plan.cpp prints it.
#pragma once
#include <cstdint>
#include <set>
#include <string>
#include <utility>
#include <vector>

#include "container.h"
#include "edit_core.h"
#include "lacx.h"

namespace lacx {

constexpr uint64_t kEditDstAlign = 256;   // every output's destination starts on such a boundary ...
constexpr uint64_t kEditLookAhead = 16;   // ... and has this much behind it (the staging loads of the front kernels, api_import.cpp)
constexpr uint64_t kEditRowAlign = 4;     // staging rows start on a multiple of this many int32 (16-byte loads)

// One segment that goes to the device: a window item of phase 1.
struct EditWindow {
    uint32_t out;   // its output among the plan's (EditPlan::outs)
    uint32_t k;     // its number inside that output
    uint32_t seg;   // its index in the call's segment array
    uint64_t start, frames;  // the window, LACX_TO_END resolved
    uint64_t at;    // its first frame inside the output
    uint8_t channels;
};

// One output that goes to the device (j counts these; the outputs that failed their checks are not among them).
struct EditOut {
    uint32_t src;  // its index in the call's output array
    uint32_t first_window, windows;
    uint64_t frames;
    uint32_t sample_rate, blocks;
    uint8_t src_channels, src_depth, channels, bit_depth, channel_op, stereo_mode;
    uint64_t stage_left, stage_right;  // staging: the rows' first elements (int32), multiples of kEditRowAlign; right: stereo sources
    uint64_t dst_at, dst_bytes;        // destination: byte offset (a multiple of kEditDstAlign) and frames * channels * bit_depth / 8
    uint64_t source_lac_bytes;         // its segments' stream sizes, each distinct (lac, size) once
};

struct EditPlan {
    std::vector<EditOut> outs;
    std::vector<EditWindow> windows;
    std::vector<unsigned long long> unit_off;  // [outs + 1]: prefix sums of ceil(frames / kEditUnitFrames)
    uint64_t stage_elems = 0;  // capacity of the staging, int32 elements
    uint64_t dst_bytes = 0;    // capacity of the destination buffer
};

namespace edit_detail {
constexpr uint64_t up(uint64_t v, uint64_t a) { return (v + a - 1u) / a * a; }
inline const char* check_window(uint64_t start, uint64_t frames, const lacx_stream_info& f) {  // the window form's rules (decode_plan.h)
    if (frames == 0) return "empty window";
    if (start >= f.frames || frames > f.frames - start) return "window outside the stream";
    return nullptr;
}
}  // namespace edit_detail

// Plans nouts outputs over the call's nsegs segments.  Every output is checked on the host, in this order: its segment
// range, channel operation, bit depth and stereo mode; then segment by segment the parse, the window and the format against
// segment 0's; then the channel operation against the sources' channel count.  Per output, code[i] and err[i] ("" = goes
// to the device).  Those that pass are laid out in call order.
inline void plan_edit(const lacx_edit_segment* segs, uint32_t nsegs, const lacx_edit_output* outs, uint32_t nouts, EditPlan& plan,
                      std::vector<int>& code, std::vector<std::string>& err) {
    using namespace edit_detail;
    plan = EditPlan{};
    code.assign(nouts, LACX_OK);
    err.assign(nouts, std::string());
    plan.unit_off.assign(1, 0ull);
    for (uint32_t i = 0; i < nouts; ++i) {
        const lacx_edit_output& o = outs[i];
        auto refuse = [&](const std::string& why) { code[i] = LACX_E_INVALID, err[i] = why; };
        if (o.segments == 0) { refuse("output has no segments"); continue; }
        if (o.first_segment >= nsegs || o.segments > nsegs - o.first_segment) { refuse("segments outside the call's array"); continue; }
        if (o.channel_op >= (uint32_t)CH_OPS) { refuse("unknown channel operation"); continue; }
        if (o.bit_depth != 0 && o.bit_depth != 16 && o.bit_depth != 24) { refuse("unsupported bit depth: " + std::to_string((int)o.bit_depth)); continue; }
        if (o.stereo_mode > 2) { refuse("unknown stereo mode"); continue; }
        EditOut e{};
        e.src = i;
        e.first_window = (uint32_t)plan.windows.size();
        lacx_stream_info f0{};
        std::set<std::pair<uintptr_t, uint64_t>> seen;  // its distinct sources (a join may have many thousands of segments)
        for (uint32_t k = 0; k < o.segments && code[i] == LACX_OK; ++k) {
            const lacx_edit_segment& s = segs[o.first_segment + k];
            const std::string seg = "segment " + std::to_string(k) + ": ";
            lacx_stream_info f{};
            const char* why = "";
            if (parse_stream(s.lac, s.size, &f, &why) != LACX_OK) { refuse(seg + why); break; }
            const uint64_t frames = s.frames == LACX_TO_END && s.start < f.frames ? f.frames - s.start : s.frames;
            if (const char* w = check_window(s.start, frames, f)) { refuse(seg + w); break; }
            if (k == 0) f0 = f;
            auto differs = [&](const char* field, uint64_t a, uint64_t b) {
                refuse(seg + field + " differs from segment 0: " + std::to_string(a) + ", " + std::to_string(b));
            };
            if (f.channels != f0.channels) { differs("channels", f0.channels, f.channels); break; }
            if (f.bit_depth != f0.bit_depth) { differs("bit depth", f0.bit_depth, f.bit_depth); break; }
            if (f.sample_rate != f0.sample_rate) { differs("sample rate", f0.sample_rate, f.sample_rate); break; }
            plan.windows.push_back(EditWindow{(uint32_t)plan.outs.size(), k, o.first_segment + k, s.start, frames, e.frames, f.channels});
            e.frames += frames;
            if (seen.insert({(uintptr_t)s.lac, s.size}).second) e.source_lac_bytes += s.size;
        }
        if (code[i] == LACX_OK) {
            const bool wants_stereo = o.channel_op == CH_LEFT || o.channel_op == CH_RIGHT || o.channel_op == CH_FOLD || o.channel_op == CH_SWAP;
            if (wants_stereo && f0.channels != 2) refuse("channel operation needs a stereo source");
            else if (o.channel_op == CH_DUAL && f0.channels != 1) refuse("channel operation needs a mono source");
        }
        if (code[i] != LACX_OK) {
            plan.windows.resize(e.first_window);
            continue;
        }
        e.windows = o.segments;
        e.sample_rate = f0.sample_rate;
        e.src_channels = f0.channels;
        e.src_depth = f0.bit_depth;
        e.channels = (uint8_t)edit_channels_out(f0.channels, o.channel_op);
        e.bit_depth = o.bit_depth ? o.bit_depth : f0.bit_depth;
        e.channel_op = o.channel_op;
        e.stereo_mode = e.channels == 2 ? o.stereo_mode : 0;
        e.blocks = (uint32_t)((e.frames + LACX_MAX_BLOCK - 1u) / LACX_MAX_BLOCK);
        const uint64_t row = up(e.frames, kEditRowAlign);
        e.stage_left = plan.stage_elems;
        e.stage_right = f0.channels == 2 ? plan.stage_elems + row : 0;
        plan.stage_elems += row * f0.channels;
        e.dst_at = plan.dst_bytes;
        e.dst_bytes = e.frames * e.channels * (uint64_t)(e.bit_depth / 8);
        plan.dst_bytes += up(e.dst_bytes + kEditLookAhead, kEditDstAlign);
        plan.unit_off.push_back(plan.unit_off.back() + (e.frames + kEditUnitFrames - 1u) / kEditUnitFrames);
        plan.outs.push_back(e);
    }
}

// The transform table of k_edit: output j's staging rows inside `stage` and its destination inside `dst`.
inline void edit_fill_items(const EditPlan& plan, const int32_t* stage, uint8_t* dst, EditItem* items) {
    for (size_t j = 0; j < plan.outs.size(); ++j) {
        const EditOut& e = plan.outs[j];
        items[j] = EditItem{stage + e.stage_left, e.src_channels == 2 ? stage + e.stage_right : nullptr, dst + e.dst_at, e.frames,
                            e.src_channels, e.channel_op, e.src_depth, e.bit_depth, {0, 0, 0, 0}};
    }
}

// The words of a violation k_edit left (EditBad::key), from the staged samples of its frame.
inline std::string edit_bad_message(unsigned long long key, uint32_t channel_op, int32_t staged_left, int32_t staged_right) {
    const unsigned long long frame = key >> 2;
    const uint32_t kind = (uint32_t)(key & 3u);
    if (kind == 0)
        return "[transcode-error] frame " + std::to_string(frame) + ": left " + std::to_string(staged_left) + " and right " +
               std::to_string(staged_right) + " differ";
    const int32_t ol = channel_op == CH_RIGHT || channel_op == CH_SWAP ? staged_right : staged_left;
    const int32_t orr = channel_op == CH_SWAP || channel_op == CH_DUAL ? staged_left : staged_right;
    return "[transcode-error] frame " + std::to_string(frame) + (kind == 1 ? " left sample " : " right sample ") +
           std::to_string(kind == 1 ? ol : orr) + " is not a multiple of 256";
}

}  // namespace lacx
