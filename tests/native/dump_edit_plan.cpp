// dump_edit_plan.cpp -- prints the plans edit_plan.h makes, one line of JSON per case, for tests/test_edit_plan_host.py to
// compare with the rules restated in Python.  Built from edit_plan.h alone (no HIP), plain and under AddressSanitizer +
// UBSan.  The transform table is filled over heap blocks of exactly the planned capacities, and every row and destination
// is touched at its first and last byte, so a plan that lays something outside its capacity stops the sanitized build.
//
// A case (little-endian, in a file of frames <u32 size><bytes>):
//   u32 nstreams, nsegs, nouts, pad | per stream: u64 size, bytes | per segment: u32 stream, pad; u64 start, frames
//   | per output: the 16 bytes of lacx_edit_output
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "edit_plan.h"

using namespace lacx;

namespace {

template <class T>
T take(const uint8_t*& p) {
    T v;
    std::memcpy(&v, p, sizeof(T));
    p += sizeof(T);
    return v;
}

std::string quoted(const std::string& s) {
    std::string out = "\"";
    for (char c : s) {
        if (c == '"' || c == '\\') out += '\\';
        out += c;
    }
    return out + "\"";
}

std::string run_case(const uint8_t* p) {
    const uint32_t nstreams = take<uint32_t>(p), nsegs = take<uint32_t>(p), nouts = take<uint32_t>(p);
    (void)take<uint32_t>(p);
    std::vector<std::vector<uint8_t>> streams(nstreams);  // heap blocks of exactly the streams' sizes
    for (auto& s : streams) {
        const uint64_t n = take<uint64_t>(p);
        s.assign(p, p + n);
        p += n;
    }
    std::vector<lacx_edit_segment> segs(nsegs);
    for (auto& s : segs) {
        const uint32_t k = take<uint32_t>(p);
        (void)take<uint32_t>(p);
        static const uint8_t nothing = 0;
        s.lac = streams[k].empty() ? &nothing : streams[k].data();  // (an empty stream is not a null pointer)
        s.size = streams[k].size();
        s.start = take<uint64_t>(p);
        s.frames = take<uint64_t>(p);
    }
    std::vector<lacx_edit_output> outs(nouts);
    for (auto& o : outs) o = take<lacx_edit_output>(p);
    EditPlan plan;
    std::vector<int> code;
    std::vector<std::string> err;
    plan_edit(segs.data(), nsegs, outs.data(), nouts, plan, code, err);
    std::vector<int32_t> stage(plan.stage_elems);
    std::vector<uint8_t> dst(plan.dst_bytes);
    std::vector<EditItem> items(plan.outs.size());
    edit_fill_items(plan, stage.data(), dst.data(), items.data());
    std::string o = "{\"code\": [";
    for (size_t i = 0; i < code.size(); ++i) o += (i ? ", " : "") + std::to_string(code[i]);
    o += "], \"err\": [";
    for (size_t i = 0; i < err.size(); ++i) o += (i ? ", " : "") + quoted(err[i]);
    o += "], \"outs\": [";
    for (size_t j = 0; j < plan.outs.size(); ++j) {
        const EditOut& e = plan.outs[j];
        const EditItem& it = items[j];
        // the rows and the destination, first and last byte: inside the planned capacities or the sanitizer says so
        int32_t* left = const_cast<int32_t*>(it.left);
        left[0] = 1, left[e.frames - 1] = 1;
        if (it.right) const_cast<int32_t*>(it.right)[0] = 1, const_cast<int32_t*>(it.right)[e.frames - 1] = 1;
        static_cast<uint8_t*>(it.dst)[0] = 1, static_cast<uint8_t*>(it.dst)[e.dst_bytes + kEditLookAhead - 1] = 1;
        const uint64_t vals[] = {e.src, e.first_window, e.windows, e.frames, e.sample_rate, e.blocks, e.src_channels, e.src_depth, e.channels,
                                 e.bit_depth, e.channel_op, e.stereo_mode, e.stage_left, e.stage_right, e.dst_at, e.dst_bytes, e.source_lac_bytes,
                                 (uint64_t)(it.left - stage.data()), it.right ? (uint64_t)(it.right - stage.data()) : 0u,
                                 (uint64_t)(static_cast<uint8_t*>(it.dst) - dst.data()), it.frames, it.src_channels, it.channel_op, it.src_depth, it.dst_depth};
        o += j ? ", [" : "[";
        for (size_t v = 0; v < sizeof(vals) / sizeof(vals[0]); ++v) o += (v ? ", " : "") + std::to_string(vals[v]);
        o += "]";
    }
    o += "], \"windows\": [";
    for (size_t w = 0; w < plan.windows.size(); ++w) {
        const EditWindow& x = plan.windows[w];
        o += (w ? ", [" : "[") + std::to_string(x.out) + ", " + std::to_string(x.k) + ", " + std::to_string(x.seg) + ", " + std::to_string(x.start) + ", " +
             std::to_string(x.frames) + ", " + std::to_string(x.at) + ", " + std::to_string((int)x.channels) + "]";
    }
    o += "], \"unit_off\": [";
    for (size_t i = 0; i < plan.unit_off.size(); ++i) o += (i ? ", " : "") + std::to_string(plan.unit_off[i]);
    o += "], \"stage_elems\": " + std::to_string(plan.stage_elems) + ", \"dst_bytes\": " + std::to_string(plan.dst_bytes) + "}";
    return o;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    if (std::string(argv[1]) == "--messages") {  // the violation texts: KEY OP LEFT RIGHT per further argument quadruple
        for (int i = 2; i + 3 < argc; i += 4)
            std::printf("%s\n", edit_bad_message(std::stoull(argv[i]), (uint32_t)std::stoul(argv[i + 1]), (int32_t)std::stol(argv[i + 2]), (int32_t)std::stol(argv[i + 3])).c_str());
        return 0;
    }
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<uint8_t> data;
    uint8_t buf[65536];
    for (size_t n; (n = std::fread(buf, 1, sizeof(buf), f)) > 0;) data.insert(data.end(), buf, buf + n);
    std::fclose(f);
    size_t at = 0, cases = 0;
    while (at + 4 <= data.size()) {
        uint32_t size;
        std::memcpy(&size, data.data() + at, 4);
        at += 4;
        const std::vector<uint8_t> one(data.begin() + at, data.begin() + at + size);  // a block of exactly the case's size
        at += size;
        std::printf("%zu %s\n", cases++, run_case(one.data()).c_str());
    }
    std::printf("done %zu\n", cases);
    return 0;
}
