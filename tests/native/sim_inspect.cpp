// tests/native/sim_inspect.cpp -- TEST INFRASTRUCTURE: the stream inspection's lane code (csrc/inspect_core.h) on the host.
//
// One "lane" per present block of a version-3 stream and one per version-2 stream -- the work of k_inspect and
// k_inspect_serial, one lane after the other -- over a job planned by plan_inspect (csrc/inspect_plan.h, the code
// api_decode.cpp runs) whose tables plan_fill_tables fills.  Every buffer is a heap allocation of exactly the capacity
// the plan states: the payload with its tail pad, the tables with the rows and the partition entries inside them, lane
// memory of kInspectBytesPerCol * cols.  The rows start as 0xA5 bytes (a lane must write every byte of its row), the
// partition entries as zeros (launch_inspect's memset).  The host side is the product's: inspect_rows_of_item and
// inspect_combine (csrc/inspect_rows.h).  It is not part of the product and is not a fallback.
//
// Built twice by tests/inspecttwin.py: a plain -O2 shared library for ctypes, and (-DSIM_INSPECT_MAIN) a sanitized program
// that walks a file of batch cases and prints one digest line per case.
#define SIM_JOB_SIMULATOR
#include "sim_job.h"

#include "inspect_core.h"
#include "inspect_plan.h"
#include "inspect_rows.h"

using namespace lacx;
using namespace simjob;

namespace {

void shuffle(std::vector<uint32_t>& v, uint32_t seed) {
    uint64_t s = 0x9E3779B97F4A7C15ull * (seed + 1u);
    for (size_t i = v.size(); i > 1; --i) {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        std::swap(v[i - 1], v[(size_t)((s >> 33) % i)]);
    }
}

struct Out {  // what the caller of the ABI would see
    std::vector<int> code;
    std::vector<std::vector<lacx_block_info>> rows;
    std::vector<lacx_stream_report> reports;
    std::vector<uint32_t> block0;  // ~0u: refused
    std::vector<uint8_t> mode_k;
    std::vector<uint32_t> part_bits;
    uint32_t over = 0;
};

// n streams as one inspection job.  cols: 1 or 64 columns of lane memory, the lane being the last; gather_seed (a batch of
// one version-3 stream only): the blocks' payloads back to back in a shuffled order, each lane with two-entry tables of
// its own.  False where the plan refuses the job as a whole.
bool run_job(const uint8_t* const* lacs, const uint64_t* sizes, uint32_t n, bool partitions, int cols, uint32_t gather_seed, bool pad_waves, Out& out) {
    std::vector<BatchIn> in(n);
    for (uint32_t i = 0; i < n; ++i) in[i] = BatchIn{lacs[i], sizes[i], nullptr, nullptr, 0};
    InspectPlan plan;
    std::vector<std::string> err;
    if (plan_inspect(in.data(), n, partitions, pad_waves, plan, out.code, err)) return false;
    const DecodePlan& base = plan.base;
    out.rows.assign(n, {});
    out.reports.assign(n, lacx_stream_report{});
    out.block0.assign(n, ~0u);
    if (base.items.empty()) return true;
    const size_t T = (size_t)base.total_blocks;
    Heap<uint8_t> payload(plan.need.payload), tables(plan.need.tables);
    plan_fill_tables(base, in.data(), PlanBases{payload.p, nullptr, nullptr, nullptr}, tables.p);
    const InspectArgs s = plan_inspect_args(plan, tables.p, payload.p);
    std::memset(s.rows, 0xA5, kInspectRowBytes * plan.need.rows);
    const DecodeArgs& a = s.dec;
    Heap<unsigned char> raw(kInspectBytesPerCol * (size_t)cols, 0xA5);
    DecMem dm = inspect_mem(raw.p, (uint32_t)cols);
    const int lane = cols - 1;
    DecWave wave;
    if (gather_seed && n == 1 && a.items[0].version == 3) {
        const DecodeItem& it = a.items[0];
        const uint32_t present = base.items[0].present_blocks;
        std::vector<uint32_t> order(present);
        for (uint32_t b = 0; b < present; ++b) order[b] = b;
        shuffle(order, gather_seed);
        unsigned long long cur = 0;
        std::vector<unsigned long long> at(present);
        for (uint32_t b : order) {
            const unsigned long long bytes = a.byte_off[b + 1] - a.byte_off[b];
            at[b] = cur;
            std::memcpy(payload.p + cur, lacs[0] + base.items[0].head + a.byte_off[b], bytes);
            cur += bytes;
        }
        for (uint32_t b = 0; b < present; ++b) {
            const unsigned long long bo[2] = {at[b], at[b] + (a.byte_off[b + 1] - a.byte_off[b])};
            const unsigned long long fo[2] = {a.frame_off[b], a.frame_off[b + 1]};
            inspect_block_lane(0, it.channels, it.stereo_mode, a.payload, bo, fo, s.rows + b, s.mode_k ? s.mode_k + (size_t)b * 2u * kInspectPartSlots : nullptr,
                               s.part_bits ? s.part_bits + (size_t)b * 2u * kInspectPartSlots : nullptr, dm, lane, wave);
        }
    } else {
        place_payload(base, in.data(), payload.p);
        for (uint32_t g = 0; g < a.lanes; ++g) {  // k_inspect
            const uint32_t blk = a.lane_blk[g];
            if (blk == ~0u) continue;
            const DecodeItem& it = a.items[a.blk_item[blk]];
            inspect_block_lane(blk, it.channels, it.stereo_mode, a.payload, a.byte_off, a.frame_off, s.rows, s.mode_k, s.part_bits, dm, lane, wave);
        }
        for (uint32_t g = 0; g < a.nv2; ++g) {  // k_inspect_serial
            const DecodeItem& it = a.items[a.v2_items[g]];
            const size_t slots = (size_t)it.block0 * 2u * kInspectPartSlots;
            inspect_serial_lane(it.blocks, it.channels, it.stereo_mode, a.payload + it.pay_off, it.pay_bits, a.frame_off + it.block0,
                                s.rows + it.block0, s.mode_k ? s.mode_k + slots : nullptr, s.part_bits ? s.part_bits + slots : nullptr, dm, lane,
                                wave);
        }
    }
    out.over = wave.over;
    for (const PlanItem& p : base.items) {
        const uint32_t i = p.src;
        inspect_rows_of_item(lacs[i], p.info.version, p.item.blocks, p.present_blocks, s.rows + p.item.block0, out.rows[i]);
        out.reports[i] = inspect_combine(out.rows[i].data(), (uint32_t)out.rows[i].size(), &p.info);
        out.block0[i] = p.item.block0;
    }
    if (partitions) {
        out.mode_k.assign(s.mode_k, s.mode_k + kInspectPartModeBytes * T);
        out.part_bits.assign(s.part_bits, s.part_bits + kInspectPartBitsBytes / 4 * T);
    }
    return true;
}

// A case: u32 flags (1: partitions, 2: pad_waves), u32 cols, u32 gather_seed, u32 n, then per stream u64 size and the bytes.
// The line: the plan's outcome per item and one hash over every row, report and (asked for) partition entry.
bool case_line(const uint8_t* blob, uint64_t size, std::string& line) {
    Reader rd{blob, blob + size};
    const uint32_t flags = rd.get<uint32_t>(), cols = rd.get<uint32_t>(), seed = rd.get<uint32_t>(), n = rd.get<uint32_t>();
    if (!rd.ok || (cols != 1u && cols != 64u)) return false;
    std::vector<std::unique_ptr<Exact>> own;
    std::vector<const uint8_t*> lacs;
    std::vector<uint64_t> sizes;
    for (uint32_t i = 0; i < n; ++i) {
        const uint64_t sz = rd.get<uint64_t>();
        const std::vector<uint8_t> bytes = rd.array<uint8_t>(sz);
        if (!rd.ok) return false;
        own.emplace_back(new Exact(sz, 0));  // exactly the stream's bytes: the host side reads its table in place
        if (sz) std::memcpy(own.back()->data, bytes.data(), sz);
        lacs.push_back(own.back()->data);
        sizes.push_back(sz);
    }
    Out out;
    if (!run_job(lacs.data(), sizes.data(), n, (flags & 1u) != 0, (int)cols, seed, (flags & 2u) != 0, out)) return false;
    uint64_t h = kFnvStart;
    line.clear();
    for (uint32_t i = 0; i < n; ++i) {
        line += std::to_string(out.code[i]) + ",";
        h = fnv(out.rows[i].data(), out.rows[i].size() * sizeof(lacx_block_info), h);
        h = fnv(&out.reports[i], sizeof(lacx_stream_report), h);
    }
    h = fnv(out.mode_k.data(), out.mode_k.size(), h);
    h = fnv(out.part_bits.data(), out.part_bits.size() * 4u, h);
    char buf[64];
    std::snprintf(buf, sizeof buf, " %016llx over=%u", (unsigned long long)h, out.over);
    line += buf;
    return true;
}

}  // namespace

extern "C" {

// n streams as one job.  Out: item_rc[n]; block0[n] (the item's first row among rows_out, ~0u: refused); rows_out: the
// accepted items' rows back to back in item order (cap rows at most, else -2); reports[n]; with partitions mode_k_out /
// part_bits_out [rows][2][256] in the same order; *over: the furthest byte a load reached past the end of its block.
int sim_inspect(const uint8_t* const* lacs, const uint64_t* sizes, uint32_t n, uint32_t flags, int cols, uint32_t gather_seed, int* item_rc,
                uint32_t* block0, lacx_block_info* rows_out, uint64_t cap, lacx_stream_report* reports, uint8_t* mode_k_out,
                uint32_t* part_bits_out, uint32_t* over) {
    if (cols != 1 && cols != 64) return -1;
    Out out;
    if (!run_job(lacs, sizes, n, (flags & 1u) != 0, cols, gather_seed, (flags & 2u) != 0, out)) return -1;
    uint64_t at = 0;
    for (uint32_t i = 0; i < n; ++i) {
        item_rc[i] = out.code[i];
        reports[i] = out.reports[i];
        block0[i] = out.block0[i] == ~0u ? ~0u : (uint32_t)at;
        const size_t k = out.rows[i].size();
        if (at + k > cap) return -2;
        if (k) std::memcpy(rows_out + at, out.rows[i].data(), k * sizeof(lacx_block_info));
        if ((flags & 1u) && k) {
            std::memcpy(mode_k_out + at * kInspectPartModeBytes, out.mode_k.data() + (size_t)out.block0[i] * kInspectPartModeBytes, k * kInspectPartModeBytes);
            std::memcpy(part_bits_out + at * 2u * kInspectPartSlots, out.part_bits.data() + (size_t)out.block0[i] * 2u * kInspectPartSlots, k * kInspectPartBitsBytes);
        }
        at += k;
    }
    *over = out.over;
    return 0;
}

// the plain build's line for a case of the sanitized program (cap bytes at line, NUL-terminated); -1: a case it refuses
int sim_inspect_line(const uint8_t* blob, uint64_t size, char* line, uint32_t cap) {
    std::string s;
    if (!case_line(blob, size, s) || s.size() + 1 > cap) return -1;
    std::memcpy(line, s.c_str(), s.size() + 1);
    return 0;
}

}  // extern "C"

#ifdef SIM_INSPECT_MAIN
int main(int argc, char** argv) {
    if (argc < 2) return 2;
    return for_each_case(argv[1], [](const uint8_t* blob, uint32_t size, uint32_t index) {
        std::string line;
        if (!case_line(blob, size, line)) return false;
        std::printf("%u %s\n", index, line.c_str());
        return true;
    });
}
#endif
