// recovery_plan.h -- the host side of the recovery data (lacx.h).  Host only, no HIP: the C ABI
// (api_recovery.cpp) and the CPU twin (tests/native/sim_recovery.cpp) run the same plan, the twin with every buffer at
// exactly the capacity stated here.  It holds the geometry, the "LACR" sidecar's builder and parser, the rule that
// classifies slices, the per-group erasure solve, the task tables of recovery_core.h and the byte counts of every buffer.
//
// The protected object is the whole .lac file of L >= 1 bytes, cut into k = ceil(L / S) slices (the last zero-extended
// to S; a slice's CRC-32 covers its real bytes only).  G = ceil(k / K) groups; slice i is member i div G of group
// i mod G, so a burst spreads over the groups.  Parity slice p of group g: XOR_i c(p, i) * D[g + i * G] with the Cauchy
// coefficient c(p, i) = 1 / (p XOR (r + i)) in GF(2^8); r + K <= 256 keeps the two index sets apart, so every square
// submatrix is invertible and a group is repairable exactly when it has at least as many usable parity slices as
// damaged data slices.
// Sidecar, big-endian:
//   0 "LACR" | 4 version = 1 | 5 r | 6 K u16 | 8 S u32 | 12 L u64 | 20 file_crc32 u32 | 24 k u32 | 28 G u32 |
//   32 CRC-32 of bytes 0..31 | 36 k slice CRC-32 u32 | 36 + 4k CRC-32 of the slice table |
//   40 + 4k parity records in (g, p) order, each S bytes followed by their CRC-32 u32
// One device arena holds a job's bytes; every offset into it is a multiple of 4 and every slice's S bytes lie inside it.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "lacx.h"
#include "recovery_core.h"

namespace lacx {

constexpr uint32_t kRecSliceDefault = 4096, kRecParityDefault = 8, kRecGroupDefault = 128;
constexpr uint32_t kRecMaxSlices = 1u << 28;
constexpr uint64_t kRecTableAt = 36;

namespace recovery_detail {
inline uint32_t rget32(const uint8_t* p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3]; }
inline void rput32(uint8_t* p, uint32_t v) { p[0] = (uint8_t)(v >> 24), p[1] = (uint8_t)(v >> 16), p[2] = (uint8_t)(v >> 8), p[3] = (uint8_t)v; }
inline uint32_t crc32_of(const uint8_t* p, uint64_t n) {
    uint32_t r = 0xFFFFFFFFu;
    for (uint64_t i = 0; i < n; ++i) r = crc_raw_bytes(r, p[i], 1u);
    return r ^ 0xFFFFFFFFu;
}
inline uint64_t up16(uint64_t v) { return (v + 15u) & ~15ull; }
inline int refuse(std::string& why, const std::string& text) {
    why = "[recovery-error] " + text;
    return LACX_E_INVALID;
}
}  // namespace recovery_detail

struct RecGeometry {
    uint32_t S = 0, r = 0, K = 0, k = 0, G = 0;
    uint64_t L = 0;
    uint64_t head_bytes() const { return 40ull + 4ull * k; }
    uint64_t record_bytes() const { return (uint64_t)S + 4u; }
    uint64_t records() const { return (uint64_t)G * r; }
    uint64_t sidecar_bytes() const { return head_bytes() + records() * record_bytes(); }
    uint32_t members(uint32_t g) const { return (k - g + G - 1u) / G; }  // k_g
    uint32_t slice_len(uint32_t i) const { return i + 1u < k ? S : (uint32_t)(L - (uint64_t)(k - 1u) * S); }
};
inline uint8_t rec_coef(uint32_t r, uint32_t p, uint32_t i) { return gf_inv((uint8_t)(p ^ (r + i))); }

// zeros = defaults; the ranges of lacx.h
inline int rec_params(const lacx_recovery_params* prm, uint32_t& S, uint32_t& r, uint32_t& K, std::string& why) {
    using namespace recovery_detail;
    S = prm && prm->slice_bytes ? prm->slice_bytes : kRecSliceDefault;
    r = prm && prm->parity ? prm->parity : kRecParityDefault;
    K = prm && prm->group_data ? prm->group_data : kRecGroupDefault;
    if (S < 64u || S > 65536u || (S & 15u)) return refuse(why, "slice_bytes " + std::to_string(S) + " is not a multiple of 16 in 64..65536");
    if (r < 1u || r > 32u) return refuse(why, "parity " + std::to_string(r) + " is not in 1..32");
    if (K < 1u || K > 256u - r) return refuse(why, "group_data " + std::to_string(K) + " is not in 1..256 - parity");
    return LACX_OK;
}
inline int rec_geometry(uint64_t L, uint32_t S, uint32_t r, uint32_t K, RecGeometry& geo, std::string& why) {
    using namespace recovery_detail;
    if (L == 0) return refuse(why, "file_bytes is 0");
    const uint64_t k = L / S + (L % S != 0);
    if (k >= kRecMaxSlices) return refuse(why, "the file needs " + std::to_string(k) + " slices, 2^28 or more");
    geo.S = S, geo.r = r, geo.K = K, geo.L = L, geo.k = (uint32_t)k, geo.G = (uint32_t)((k + K - 1u) / K);
    return LACX_OK;
}

// The head (bytes 0 .. 40 + 4k) must be intact and consistent; the parity area is looked at by nobody here.
// info->parity_present: the parity records that lie wholly inside the sidecar.
inline int recovery_parse(const uint8_t* m, uint64_t size, RecGeometry& geo, lacx_recovery_info* info, std::string& why) {
    using namespace recovery_detail;
    if (!m || size < 40u) return refuse(why, "short input");
    if (std::memcmp(m, "LACR", 4) != 0) return refuse(why, "wrong magic");
    if (m[4] != 1) return refuse(why, "unsupported version: " + std::to_string((int)m[4]));
    if (rget32(m + 32) != crc32_of(m, 32)) return refuse(why, "checksum of the header differs");
    lacx_recovery_params prm{rget32(m + 8), m[5], (uint16_t)((m[6] << 8) | m[7])};
    // (a zero field is no default here)
    if (prm.slice_bytes == 0) return refuse(why, "slice_bytes 0 is not a multiple of 16 in 64..65536");
    if (prm.parity == 0) return refuse(why, "parity 0 is not in 1..32");
    if (prm.group_data == 0) return refuse(why, "group_data 0 is not in 1..256 - parity");
    uint32_t S, r, K;
    if (rec_params(&prm, S, r, K, why) != LACX_OK) return LACX_E_INVALID;
    const uint64_t L = ((uint64_t)rget32(m + 12) << 32) | rget32(m + 16);
    const uint32_t k = rget32(m + 24), G = rget32(m + 28);
    RecGeometry f;
    if (rec_geometry(L, S, r, K, f, why) != LACX_OK) return LACX_E_INVALID;
    if (k != f.k) return refuse(why, "slices " + std::to_string(k) + ", file_bytes and slice_bytes give " + std::to_string(f.k));
    if (G != f.G) return refuse(why, "groups " + std::to_string(G) + ", slices and group_data give " + std::to_string(f.G));
    if (size < f.head_bytes()) return refuse(why, "slice table is cut short");
    if (rget32(m + kRecTableAt + 4ull * k) != crc32_of(m + kRecTableAt, 4ull * k)) return refuse(why, "checksum of the slice table differs");
    uint32_t all = 0;
    for (uint32_t i = 0; i < k; ++i) {
        const uint32_t c = rget32(m + kRecTableAt + 4ull * i);
        all = i ? crc32_combine(all, c, f.slice_len(i)) : c;
    }
    if (all != rget32(m + 20)) return refuse(why, "file_crc32 is not the combination of the slice checksums");
    geo = f;
    if (info) {
        *info = lacx_recovery_info{};
        info->file_bytes = L, info->file_crc32 = all, info->slice_bytes = S, info->slices = k, info->groups = G;
        info->parity = (uint16_t)r, info->group_data = (uint16_t)K;
        info->parity_present = (uint32_t)std::min<uint64_t>(f.records(), (size - f.head_bytes()) / f.record_bytes());
        info->flags = size < f.sidecar_bytes() ? LACX_REPAIR_SIDECAR_TRUNCATED : 0u;
    }
    return LACX_OK;
}

// ---- the tables of one launch set: k_gf_combine over the tasks, tier by tier, then k_slice_crc over the ranges ------
struct RecStage {
    std::vector<CrcRange> ranges;
    std::vector<GfTask> tier_tasks[kGfTiers];
    std::vector<unsigned long long> refs;
    std::vector<uint8_t> mat;
    // layout (finish): byte offsets into the table buffer
    std::vector<GfTask> tasks;
    uint32_t tier_t0[kGfTiers + 1] = {}, tier_wgs[kGfTiers] = {};
    uint64_t at_ranges = 0, at_crc = 0, at_tasks = 0, at_refs = 0, at_mat = 0, size = 0;

    bool empty() const { return ranges.empty() && tasks.empty(); }
    // M: nout rows of nin coefficients -> the task's tier layout; returns m_at
    uint32_t add_matrix(const std::vector<uint8_t>& M, uint32_t nin, uint32_t nout) {
        const uint32_t outs = gf_tier_outs(gf_tier_of(nout)), at = (uint32_t)mat.size();
        mat.resize(at + (size_t)nin * outs, 0);
        for (uint32_t o = 0; o < nout; ++o)
            for (uint32_t i = 0; i < nin; ++i) mat[at + (size_t)i * outs + o] = M[(size_t)o * nin + i];
        return at;
    }
    void add_task(const std::vector<unsigned long long>& in, const std::vector<unsigned long long>& out, uint32_t m_at, uint32_t words) {
        GfTask t{};
        t.in_at = (uint32_t)refs.size();
        refs.insert(refs.end(), in.begin(), in.end());
        t.out_at = (uint32_t)refs.size();
        refs.insert(refs.end(), out.begin(), out.end());
        t.m_at = m_at, t.nin = (uint16_t)in.size(), t.nout = (uint16_t)out.size(), t.words = words;
        tier_tasks[gf_tier_of(t.nout)].push_back(t);
    }
    void finish() {
        tasks.clear();
        for (uint32_t tier = 0; tier < kGfTiers; ++tier) {
            tier_t0[tier] = (uint32_t)tasks.size();
            uint32_t wg = 0;
            for (GfTask t : tier_tasks[tier]) {
                t.wg0 = wg;
                wg += (t.words + kGfThreads - 1u) / kGfThreads;
                tasks.push_back(t);
            }
            tier_wgs[tier] = wg;
        }
        tier_t0[kGfTiers] = (uint32_t)tasks.size();
        at_ranges = 0;
        at_crc = at_ranges + sizeof(CrcRange) * ranges.size();
        at_tasks = recovery_detail::up16(at_crc + 4ull * ranges.size());
        at_refs = at_tasks + recovery_detail::up16(sizeof(GfTask) * tasks.size());
        at_mat = at_refs + recovery_detail::up16(8ull * refs.size());
        size = at_mat + recovery_detail::up16(mat.size());
    }
    // dst: `size` bytes
    void fill(uint8_t* dst) const {
        std::memset(dst, 0, (size_t)size);
        if (!ranges.empty()) std::memcpy(dst + at_ranges, ranges.data(), sizeof(CrcRange) * ranges.size());
        if (!tasks.empty()) std::memcpy(dst + at_tasks, tasks.data(), sizeof(GfTask) * tasks.size());
        if (!refs.empty()) std::memcpy(dst + at_refs, refs.data(), 8ull * refs.size());
        if (!mat.empty()) std::memcpy(dst + at_mat, mat.data(), mat.size());
    }
};

// arena[at, at + bytes) = src, or zeros where src is null; out[out_at, ...) = arena[at, ...)
struct RecUp {
    uint64_t at;
    const uint8_t* src;
    uint64_t bytes;
};
struct RecDown {
    uint64_t at, out_at, bytes;
};

// ---- build ------------------------------------------------------------------------------------------------------------
struct RecBuildItem {
    uint32_t src = 0;  // the caller's index
    RecGeometry geo;
    uint64_t file_at = 0, par_at = 0, out_at = 0;
    uint32_t range0 = 0;  // k data ranges, then G * r parity ranges
};
struct RecBuildPlan {
    std::vector<RecBuildItem> items;  // the items that go to the device
    RecStage stage;
    std::vector<RecUp> ups;
    std::vector<RecDown> downs;
    uint64_t arena_bytes = 0, out_bytes = 0;  // capacities; tables: stage.size
};

// code / err: n entries; an item whose code is not LACX_OK on entry is left alone (the caller's container check).
inline void plan_recovery_build(const lacx_span* files, uint32_t n, uint32_t S, uint32_t r, uint32_t K, RecBuildPlan& plan, std::vector<int>& code,
                                std::vector<std::string>& err) {
    using namespace recovery_detail;
    std::map<uint32_t, uint32_t> cauchy_at;  // members -> m_at
    for (uint32_t i = 0; i < n; ++i) {
        if (code[i] != LACX_OK) continue;
        RecBuildItem it;
        it.src = i;
        if ((code[i] = rec_geometry(files[i].data ? files[i].size : 0, S, r, K, it.geo, err[i])) != LACX_OK) continue;
        const RecGeometry& f = it.geo;
        it.file_at = plan.arena_bytes;
        it.par_at = it.file_at + (uint64_t)f.k * S;
        plan.arena_bytes = up16(it.par_at + f.records() * f.record_bytes());
        it.out_at = plan.out_bytes;
        plan.out_bytes = up16(it.out_at + f.sidecar_bytes());
        plan.ups.push_back(RecUp{it.file_at, files[i].data, f.L});
        if ((uint64_t)f.k * S > f.L) plan.ups.push_back(RecUp{it.file_at + f.L, nullptr, (uint64_t)f.k * S - f.L});
        plan.downs.push_back(RecDown{it.par_at, it.out_at + f.head_bytes(), f.records() * f.record_bytes()});
        it.range0 = (uint32_t)plan.stage.ranges.size();
        for (uint32_t s = 0; s < f.k; ++s) plan.stage.ranges.push_back(CrcRange{it.file_at + (uint64_t)s * S, f.slice_len(s), 0});
        for (uint64_t q = 0; q < f.records(); ++q) plan.stage.ranges.push_back(CrcRange{it.par_at + q * f.record_bytes(), S, 0});
        for (uint32_t g = 0; g < f.G; ++g) {
            const uint32_t kg = f.members(g);
            auto hit = cauchy_at.find(kg);
            if (hit == cauchy_at.end()) {
                std::vector<uint8_t> M((size_t)r * kg);
                for (uint32_t p = 0; p < r; ++p)
                    for (uint32_t m = 0; m < kg; ++m) M[(size_t)p * kg + m] = rec_coef(r, p, m);
                hit = cauchy_at.emplace(kg, plan.stage.add_matrix(M, kg, r)).first;
            }
            std::vector<unsigned long long> in(kg), out(r);
            for (uint32_t m = 0; m < kg; ++m) in[m] = it.file_at + (uint64_t)(g + (uint64_t)m * f.G) * S;
            for (uint32_t p = 0; p < r; ++p) out[p] = it.par_at + ((uint64_t)g * r + p) * f.record_bytes();
            plan.stage.add_task(in, out, hit->second, S / 4u);
        }
        plan.items.push_back(it);
    }
    plan.stage.finish();
}

// The sidecars' heads and record checksums around the parity bytes the device left in `out` (plan.out_bytes); crc: the
// stage's words.  spans[src] = the item's sidecar.
inline void recovery_build_finish(const RecBuildPlan& plan, const uint32_t* crc, uint8_t* out, lacx_span* spans) {
    using namespace recovery_detail;
    for (const RecBuildItem& it : plan.items) {
        const RecGeometry& f = it.geo;
        uint8_t* m = out + it.out_at;
        const uint32_t* c = crc + it.range0;
        std::memcpy(m, "LACR", 4);
        m[4] = 1, m[5] = (uint8_t)f.r, m[6] = (uint8_t)(f.K >> 8), m[7] = (uint8_t)f.K;
        rput32(m + 8, f.S);
        rput32(m + 12, (uint32_t)(f.L >> 32)), rput32(m + 16, (uint32_t)f.L);
        uint32_t all = 0;
        for (uint32_t s = 0; s < f.k; ++s) {
            rput32(m + kRecTableAt + 4ull * s, c[s]);
            all = s ? crc32_combine(all, c[s], f.slice_len(s)) : c[s];
        }
        rput32(m + 20, all);
        rput32(m + 24, f.k), rput32(m + 28, f.G);
        rput32(m + 32, crc32_of(m, 32));
        rput32(m + kRecTableAt + 4ull * f.k, crc32_of(m + kRecTableAt, 4ull * f.k));
        for (uint64_t q = 0; q < f.records(); ++q) rput32(m + f.head_bytes() + q * f.record_bytes() + f.S, c[f.k + q]);
        if (spans) spans[it.src] = lacx_span{m, f.sidecar_bytes()};
    }
}

// ---- scan and repair --------------------------------------------------------------------------------------------------
struct RecItem {
    uint32_t src = 0;
    RecGeometry geo;
    const uint8_t* side = nullptr;
    uint64_t file_at = 0, par_at = 0, out_at = 0;
    uint32_t par_present = 0;            // records wholly inside the sidecar
    uint32_t range0 = 0;                 // scan stage: k data ranges, then par_present parity ranges
    std::vector<uint32_t> bad;           // damaged data slices, ascending
    std::vector<uint8_t> par_ok;         // [G * r]
    std::vector<uint32_t> repaired;      // the slices the fix stage rebuilds, in the order of its ranges
    uint32_t fix_range0 = 0;
    bool output = false;                 // the fix stage brings its L bytes down
    lacx_repair_result res{};
    uint32_t first_short = ~0u, short_bad = 0, short_parity = 0;  // lowest group beyond capacity
};
struct RecRepairPlan {
    std::vector<RecItem> items;
    RecStage scan, fix;
    std::vector<RecUp> ups;
    std::vector<RecDown> downs;          // (fix)
    uint64_t arena_bytes = 0, out_bytes = 0;  // capacities; tables: max(scan.size, fix.size)
};

// The input of item i is its file's first min(size, L) bytes, zero-extended to L.  A refused sidecar fails the item.
inline void plan_recovery_scan(const lacx_span* files, const lacx_span* sides, uint32_t n, RecRepairPlan& plan, std::vector<int>& code,
                               std::vector<std::string>& err) {
    using namespace recovery_detail;
    code.assign(n, LACX_OK);
    err.assign(n, std::string());
    for (uint32_t i = 0; i < n; ++i) {
        RecItem it;
        it.src = i;
        lacx_recovery_info info;
        if ((code[i] = recovery_parse(sides[i].data, sides[i].size, it.geo, &info, err[i])) != LACX_OK) continue;
        if (!files[i].data && files[i].size) {
            code[i] = refuse(err[i], "null file");
            continue;
        }
        const RecGeometry& f = it.geo;
        const uint64_t have = std::min<uint64_t>(files[i].size, f.L);
        it.side = sides[i].data;
        it.par_present = info.parity_present;
        it.res.file_bytes = f.L, it.res.slices = f.k, it.res.parity_slices = (uint32_t)f.records();
        it.res.flags = (files[i].size < f.L ? LACX_REPAIR_TRUNCATED : 0u) | (files[i].size > f.L ? LACX_REPAIR_TRAILING : 0u) | info.flags;
        it.file_at = plan.arena_bytes;
        it.par_at = it.file_at + (uint64_t)f.k * f.S;
        plan.arena_bytes = up16(it.par_at + it.par_present * f.record_bytes());
        if (have) plan.ups.push_back(RecUp{it.file_at, files[i].data, have});
        if ((uint64_t)f.k * f.S > have) plan.ups.push_back(RecUp{it.file_at + have, nullptr, (uint64_t)f.k * f.S - have});
        if (it.par_present) plan.ups.push_back(RecUp{it.par_at, sides[i].data + f.head_bytes(), it.par_present * f.record_bytes()});
        it.range0 = (uint32_t)plan.scan.ranges.size();
        for (uint32_t s = 0; s < f.k; ++s) plan.scan.ranges.push_back(CrcRange{it.file_at + (uint64_t)s * f.S, f.slice_len(s), 0});
        for (uint32_t q = 0; q < it.par_present; ++q) plan.scan.ranges.push_back(CrcRange{it.par_at + q * f.record_bytes(), f.S, 0});
        plan.items.push_back(std::move(it));
    }
    plan.scan.finish();
}

// What the scan stage's words say: the damaged slices, the usable parity records, the result, and per group whether it
// can be repaired.  scan_answer: the item's outcome is that of lacx_recovery_scan_batch (else repair decides later).
inline void recovery_classify(RecRepairPlan& plan, const uint32_t* crc, bool scan_answer, std::vector<int>& code, std::vector<std::string>& err) {
    using namespace recovery_detail;
    for (RecItem& it : plan.items) {
        const RecGeometry& f = it.geo;
        const uint32_t* c = crc + it.range0;
        for (uint32_t s = 0; s < f.k; ++s)
            if (c[s] != rget32(it.side + kRecTableAt + 4ull * s)) it.bad.push_back(s);
        it.par_ok.assign((size_t)f.records(), 0);
        for (uint32_t q = 0; q < it.par_present; ++q)
            it.par_ok[q] = c[f.k + q] == rget32(it.side + f.head_bytes() + q * f.record_bytes() + f.S) ? 1 : 0;
        std::vector<uint32_t> group_bad(f.G, 0), group_par(f.G, 0);
        for (uint32_t s : it.bad) ++group_bad[s % f.G];
        uint32_t usable = 0;
        for (uint64_t q = 0; q < f.records(); ++q) group_par[q / f.r] += it.par_ok[q], usable += it.par_ok[q];
        lacx_repair_result& res = it.res;
        res.bad_slices = (uint32_t)it.bad.size();
        res.first_bad = it.bad.empty() ? f.k : it.bad[0];
        res.bad_parity = res.parity_slices - usable;
        long long worst = -1000;
        for (uint32_t g = 0; g < f.G; ++g) {
            const long long deficit = (long long)group_bad[g] - (long long)group_par[g];
            if (deficit > worst) worst = deficit, res.worst_group = g, res.worst_group_bad = group_bad[g], res.worst_group_parity = group_par[g];
            if (deficit > 0 && it.first_short == ~0u) it.first_short = g, it.short_bad = group_bad[g], it.short_parity = group_par[g];
        }
        if (it.first_short != ~0u) res.flags |= LACX_REPAIR_UNREPAIRED;
        if (scan_answer && (res.bad_slices || (res.flags & LACX_REPAIR_TRUNCATED))) {
            code[it.src] = LACX_E_MISMATCH;
            err[it.src] = "[recovery-error] slice=" + std::to_string(res.first_bad) + " bad_slices=" + std::to_string(res.bad_slices) +
                          (it.first_short == ~0u ? " repairable" : " unrepairable");
        }
    }
}

// A (b x b, row-major) -> its inverse by Gauss-Jordan in GF(2^8); false where it is singular.
inline bool gf_invert(std::vector<uint8_t>& A, uint32_t b) {
    std::vector<uint8_t> I((size_t)b * b, 0);
    for (uint32_t d = 0; d < b; ++d) I[(size_t)d * b + d] = 1;
    for (uint32_t col = 0; col < b; ++col) {
        uint32_t piv = col;
        while (piv < b && A[(size_t)piv * b + col] == 0) ++piv;
        if (piv == b) return false;
        if (piv != col)
            for (uint32_t j = 0; j < b; ++j) std::swap(A[(size_t)piv * b + j], A[(size_t)col * b + j]), std::swap(I[(size_t)piv * b + j], I[(size_t)col * b + j]);
        const uint8_t inv = gf_inv(A[(size_t)col * b + col]);
        for (uint32_t j = 0; j < b; ++j) A[(size_t)col * b + j] = gf_mul(A[(size_t)col * b + j], inv), I[(size_t)col * b + j] = gf_mul(I[(size_t)col * b + j], inv);
        for (uint32_t row = 0; row < b; ++row) {
            const uint8_t f = A[(size_t)row * b + col];
            if (row == col || f == 0) continue;
            for (uint32_t j = 0; j < b; ++j) A[(size_t)row * b + j] ^= gf_mul(f, A[(size_t)col * b + j]), I[(size_t)row * b + j] ^= gf_mul(f, I[(size_t)col * b + j]);
        }
    }
    A.swap(I);
    return true;
}

// The matrix that rebuilds the lost members of a group from its lowest usable parity rows and the surviving members:
// lost.size() rows of rows.size() + surv.size() coefficients (rows.size() == lost.size()).
inline bool recovery_solve(uint32_t r, const std::vector<uint32_t>& rows, const std::vector<uint32_t>& lost, const std::vector<uint32_t>& surv,
                           std::vector<uint8_t>& M) {
    const uint32_t b = (uint32_t)lost.size(), nin = b + (uint32_t)surv.size();
    std::vector<uint8_t> A((size_t)b * b);
    for (uint32_t j = 0; j < b; ++j)
        for (uint32_t l = 0; l < b; ++l) A[(size_t)j * b + l] = rec_coef(r, rows[j], lost[l]);
    if (!gf_invert(A, b)) return false;
    M.assign((size_t)b * nin, 0);
    for (uint32_t l = 0; l < b; ++l) {
        for (uint32_t j = 0; j < b; ++j) M[(size_t)l * nin + j] = A[(size_t)l * b + j];
        for (uint32_t s = 0; s < surv.size(); ++s) {
            uint8_t v = 0;
            for (uint32_t j = 0; j < b; ++j) v ^= gf_mul(A[(size_t)l * b + j], rec_coef(r, rows[j], surv[s]));
            M[(size_t)l * nin + b + s] = v;
        }
    }
    return true;
}

// The fix stage: every group that can be repaired gets one task (in place, into the arena's copy of the file), the
// rebuilt slices are digested again, and the items that yield an output get their place in the out buffer.  An item with
// a group beyond capacity fails here, and yields an output only with LACX_REPAIR_BEST_EFFORT.
inline void plan_recovery_fix(RecRepairPlan& plan, uint32_t flags, std::vector<int>& code, std::vector<std::string>& err) {
    using namespace recovery_detail;
    for (RecItem& it : plan.items) {
        const RecGeometry& f = it.geo;
        const bool beyond = it.first_short != ~0u;
        if (beyond) {
            code[it.src] = LACX_E_MISMATCH;
            err[it.src] = "[recovery-error] group " + std::to_string(it.first_short) + ": " + std::to_string(it.short_bad) + " damaged slices, " +
                          std::to_string(it.short_parity) + " parity slices usable";
            if (!(flags & LACX_REPAIR_BEST_EFFORT)) continue;
        }
        std::vector<std::vector<uint32_t>> lost(f.G);
        for (uint32_t s : it.bad) lost[s % f.G].push_back(s / f.G);
        it.fix_range0 = (uint32_t)plan.fix.ranges.size();
        for (uint32_t g = 0; g < f.G; ++g) {
            if (lost[g].empty()) continue;
            std::vector<uint32_t> rows, surv;
            for (uint32_t p = 0; p < f.r && rows.size() < lost[g].size(); ++p)
                if (it.par_ok[(size_t)g * f.r + p]) rows.push_back(p);
            if (rows.size() < lost[g].size()) continue;  // beyond capacity: as found
            for (uint32_t m = 0, at = 0; m < f.members(g); ++m) {
                if (at < lost[g].size() && lost[g][at] == m) ++at;
                else surv.push_back(m);
            }
            std::vector<uint8_t> M;
            if (!recovery_solve(f.r, rows, lost[g], surv, M)) {  // (no Cauchy submatrix is singular)
                code[it.src] = LACX_E_RUNTIME;
                err[it.src] = "[recovery-error] group " + std::to_string(g) + ": singular system";
                continue;
            }
            std::vector<unsigned long long> in, out;
            for (uint32_t p : rows) in.push_back(it.par_at + ((uint64_t)g * f.r + p) * f.record_bytes());
            for (uint32_t m : surv) in.push_back(it.file_at + (uint64_t)(g + (uint64_t)m * f.G) * f.S);
            for (uint32_t m : lost[g]) {
                const uint32_t s = g + m * f.G;
                out.push_back(it.file_at + (uint64_t)s * f.S);
                it.repaired.push_back(s);
                plan.fix.ranges.push_back(CrcRange{it.file_at + (uint64_t)s * f.S, f.slice_len(s), 0});
            }
            plan.fix.add_task(in, out, plan.fix.add_matrix(M, (uint32_t)in.size(), (uint32_t)out.size()), f.S / 4u);
        }
        if (code[it.src] == LACX_E_RUNTIME) continue;
        it.output = true;
        it.out_at = plan.out_bytes;
        plan.out_bytes = up16(it.out_at + f.L);
        plan.downs.push_back(RecDown{it.file_at, it.out_at, f.L});
    }
    plan.fix.finish();
}

// What the fix stage's words say: a rebuilt slice whose CRC-32 is not the table's means the file does not combine to
// file_crc32 -- a slice the table vouched for was damaged after all.  out: the out buffer (null: no device ran).
inline void recovery_fix_finish(RecRepairPlan& plan, const uint32_t* crc, const uint8_t* out, lacx_span* spans, std::vector<int>& code,
                                std::vector<std::string>& err) {
    using namespace recovery_detail;
    for (RecItem& it : plan.items) {
        if (!it.output) continue;
        bool same = true;
        for (size_t q = 0; q < it.repaired.size(); ++q) same = same && crc[it.fix_range0 + q] == rget32(it.side + kRecTableAt + 4ull * it.repaired[q]);
        if (!same) {
            it.output = false;
            code[it.src] = LACX_E_MISMATCH;
            err[it.src] = "[recovery-error] repaired file does not match its checksum";
            continue;
        }
        it.res.repaired_slices = (uint32_t)it.repaired.size();
        if (spans && out) spans[it.src] = lacx_span{out + it.out_at, it.geo.L};
    }
}

}  // namespace lacx
