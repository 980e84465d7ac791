// sim_recovery.cpp -- the CPU twin of the recovery data: csrc/recovery_plan.h run as api_recovery.cpp runs it, with
// csrc/recovery_core.h's per-thread code looped over every workgroup, thread and lane the kernels of k_recovery.hip would
// launch.  The arena, the table buffer and the out buffer are heap blocks of exactly the plan's capacities, and the
// "kernels" read the tables from the table buffer, not from the plan: a read or write outside a stated capacity is a heap
// overflow AddressSanitizer sees.  Built from those two headers alone (no HIP), as a shared library for the host tests
// and, with -DSIM_RECOVERY_MAIN, as a program of its own that runs plain or under AddressSanitizer + UBSan.
//
// A case: u8 kind (0 build, 1 scan, 2 repair), then little-endian
//   build:  u32 n, u32 S, u32 r, u32 K (zeros = defaults), n x (u64 size, bytes)
//   others: u32 n, u32 flags, n x (u64 file size, bytes, u64 sidecar size, bytes)
// Its answer: per item i32 code, u32 length and text of the message, (scan, repair) the 48-byte result, u32 count and the
// damaged slices, u64 output size (all ones: none) and the output.
#include <cstdio>
#include <memory>

#include "recovery_plan.h"
#include "sim_job.h"

using namespace lacx;

namespace {

struct Reader {
    const uint8_t* p;
    uint64_t left;
    bool ok = true;
    template <class T>
    T get() {
        T v{};
        if (left < sizeof(T)) return ok = false, v;
        std::memcpy(&v, p, sizeof(T));
        p += sizeof(T), left -= sizeof(T);
        return v;
    }
    lacx_span span() {
        const uint64_t n = get<uint64_t>();
        if (!ok || left < n) return ok = false, lacx_span{nullptr, 0};
        lacx_span s{p, n};
        p += n, left -= n;
        return s;
    }
};

struct Writer {
    std::vector<uint8_t> bytes;
    template <class T>
    void put(const T& v) {
        const uint8_t* q = reinterpret_cast<const uint8_t*>(&v);
        bytes.insert(bytes.end(), q, q + sizeof(T));
    }
    void put(const uint8_t* q, uint64_t n) { bytes.insert(bytes.end(), q, q + n); }
};

// exactly n bytes (one at least, so that the block exists)
std::unique_ptr<uint8_t[]> block(uint64_t n) { return std::unique_ptr<uint8_t[]>(new uint8_t[n ? n : 1]); }

struct Device {
    std::unique_ptr<uint8_t[]> arena, tables, out;
};

void run_ups(Device& dev, const std::vector<RecUp>& ups) {
    for (const RecUp& u : ups) {
        if (u.src) std::memcpy(dev.arena.get() + u.at, u.src, u.bytes);
        else std::memset(dev.arena.get() + u.at, 0, u.bytes);
    }
}

template <uint32_t kOuts>
void run_tier(const RecoveryArgs& a, uint32_t tier) {
    for (uint32_t wg = 0; wg < a.tier_wgs[tier]; ++wg) {
        const uint32_t ti = gf_task_of(a.tasks, a.tier_t0[tier], a.tier_t0[tier + 1], wg);
        const GfTask t = a.tasks[ti];
        for (uint32_t thread = 0; thread < kGfThreads; ++thread) {
            const uint32_t col = (wg - t.wg0) * kGfThreads + thread;
            if (col >= t.words) continue;
            gf_combine_column<kOuts>(t, a.refs, a.mat, a.arena, col);
        }
    }
}

// launch_recovery, then the copies down
void run_stage(Device& dev, const RecStage& stage, const std::vector<RecDown>& downs, std::vector<uint32_t>& crc) {
    crc.assign(stage.ranges.size(), 0);
    if (!stage.empty()) {
        dev.tables = block(stage.size);
        stage.fill(dev.tables.get());
        uint8_t* meta = dev.tables.get();
        RecoveryArgs a;
        a.arena = dev.arena.get();
        a.tasks = reinterpret_cast<const GfTask*>(meta + stage.at_tasks);
        std::copy(stage.tier_t0, stage.tier_t0 + kGfTiers + 1, a.tier_t0);
        std::copy(stage.tier_wgs, stage.tier_wgs + kGfTiers, a.tier_wgs);
        a.refs = reinterpret_cast<const unsigned long long*>(meta + stage.at_refs);
        a.mat = meta + stage.at_mat;
        a.ranges = reinterpret_cast<const CrcRange*>(meta + stage.at_ranges);
        a.nranges = (uint32_t)stage.ranges.size();
        a.crc = reinterpret_cast<uint32_t*>(meta + stage.at_crc);
        run_tier<8>(a, 0);
        run_tier<16>(a, 1);
        run_tier<32>(a, 2);
        for (uint32_t q = 0; q < a.nranges; ++q) {
            const CrcRange r = a.ranges[q];
            uint32_t v = 0;
            for (uint32_t lane = 0; lane < 64u; ++lane) v ^= slice_crc_lane(a.arena, r, lane);
            a.crc[q] = crc_finish(v, r.len);
        }
        if (a.nranges) std::memcpy(crc.data(), a.crc, 4ull * a.nranges);
    }
    for (const RecDown& x : downs) std::memcpy(dev.out.get() + x.out_at, dev.arena.get() + x.at, x.bytes);
}

void answer(Writer& w, int code, const std::string& err, const lacx_repair_result* res, const std::vector<uint32_t>* bad, const lacx_span& out) {
    w.put<int32_t>(code);
    w.put<uint32_t>((uint32_t)err.size());
    w.put(reinterpret_cast<const uint8_t*>(err.data()), err.size());
    if (res) w.put(*res);
    if (bad) {
        w.put<uint32_t>((uint32_t)bad->size());
        for (uint32_t s : *bad) w.put<uint32_t>(s);
    }
    w.put<uint64_t>(out.data ? out.size : ~0ull);
    if (out.data) w.put(out.data, out.size);
}

bool run_build(Reader& in, Writer& w) {
    const uint32_t n = in.get<uint32_t>();
    lacx_recovery_params prm{in.get<uint32_t>(), 0, 0};
    prm.parity = (uint16_t)in.get<uint32_t>(), prm.group_data = (uint16_t)in.get<uint32_t>();
    std::vector<lacx_span> files(n);
    for (lacx_span& f : files) f = in.span();
    if (!in.ok) return false;
    uint32_t S, r, K;
    std::string why;
    if (rec_params(&prm, S, r, K, why) != LACX_OK) {
        for (uint32_t i = 0; i < n; ++i) answer(w, LACX_E_INVALID, why, nullptr, nullptr, lacx_span{nullptr, 0});
        return true;
    }
    std::vector<int> code(n, LACX_OK);
    std::vector<std::string> err(n);
    std::vector<lacx_span> out(n, lacx_span{nullptr, 0});
    RecBuildPlan plan;
    plan_recovery_build(files.data(), n, S, r, K, plan, code, err);
    Device dev;
    dev.arena = block(plan.arena_bytes);
    dev.out = block(plan.out_bytes);
    std::vector<uint32_t> crc;
    run_ups(dev, plan.ups);
    run_stage(dev, plan.stage, plan.downs, crc);
    recovery_build_finish(plan, crc.data(), dev.out.get(), out.data());
    for (uint32_t i = 0; i < n; ++i) answer(w, code[i], err[i], nullptr, nullptr, out[i]);
    return true;
}

bool run_repair(Reader& in, Writer& w, bool repair) {
    const uint32_t n = in.get<uint32_t>(), flags = in.get<uint32_t>();
    std::vector<lacx_span> files(n), sides(n);
    for (uint32_t i = 0; i < n; ++i) files[i] = in.span(), sides[i] = in.span();
    if (!in.ok) return false;
    std::vector<int> code;
    std::vector<std::string> err;
    std::vector<lacx_span> out(n, lacx_span{nullptr, 0});
    std::vector<lacx_repair_result> res(n, lacx_repair_result{});
    std::vector<std::vector<uint32_t>> bad(n);
    RecRepairPlan plan;
    plan_recovery_scan(files.data(), sides.data(), n, plan, code, err);
    Device dev;
    dev.arena = block(plan.arena_bytes);
    std::vector<uint32_t> crc;
    run_ups(dev, plan.ups);
    run_stage(dev, plan.scan, {}, crc);
    recovery_classify(plan, crc.data(), !repair, code, err);
    if (repair) {
        plan_recovery_fix(plan, flags, code, err);
        dev.out = block(plan.out_bytes);
        run_stage(dev, plan.fix, plan.downs, crc);
        recovery_fix_finish(plan, crc.data(), dev.out.get(), out.data(), code, err);
    }
    for (const RecItem& it : plan.items) res[it.src] = it.res, bad[it.src] = it.bad;
    for (uint32_t i = 0; i < n; ++i) answer(w, code[i], err[i], &res[i], &bad[i], out[i]);
    return true;
}

bool run_case(const uint8_t* blob, uint64_t size, Writer& w) {
    Reader in{blob, size};
    const uint8_t kind = in.get<uint8_t>();
    if (!in.ok || kind > 2) return false;
    return kind == 0 ? run_build(in, w) : run_repair(in, w, kind == 2);
}

}  // namespace

extern "C" {

// the answer's size, or -1 for a malformed case, or -2 where `cap` is too small
long long sim_recovery(const uint8_t* blob, uint64_t size, uint8_t* out, uint64_t cap) {
    Writer w;
    if (!run_case(blob, size, w)) return -1;
    if (w.bytes.size() > cap) return -2;
    std::memcpy(out, w.bytes.data(), w.bytes.size());
    return (long long)w.bytes.size();
}

uint32_t sim_gf_mul4(uint32_t w, uint32_t c) { return gf_mul4(w, c); }
uint32_t sim_gf_inv(uint32_t a) { return gf_inv((uint8_t)a); }
// A: b x b in place; 1 where it was inverted
int sim_gf_invert(uint8_t* A, uint32_t b) {
    std::vector<uint8_t> M(A, A + (size_t)b * b);
    if (!gf_invert(M, b)) return 0;
    std::memcpy(A, M.data(), M.size());
    return 1;
}
int sim_recovery_parse(const uint8_t* m, uint64_t size, lacx_recovery_info* info, char* msg, uint32_t cap) {
    RecGeometry geo;
    std::string why;
    const int rc = recovery_parse(m, size, geo, info, why);
    std::snprintf(msg, cap, "%s", why.c_str());
    return rc;
}
}

#ifdef SIM_RECOVERY_MAIN
// file of cases (u32 length, case)*: prints "<index> <length of the answer> <its CRC-32>" per case and "done <count>"
int main(int argc, char** argv) {
    if (argc < 2) return 2;
    return simjob::for_each_case(argv[1], [](const uint8_t* blob, uint32_t size, uint32_t i) {
        Writer w;
        if (!run_case(blob, size, w)) return false;
        return std::printf("%u %zu %08x\n", i, w.bytes.size(), recovery_detail::crc32_of(w.bytes.data(), w.bytes.size())) > 0;
    });
}
#endif
