// tests/native/sim_stats.cpp -- TEST INFRASTRUCTURE: the audio statistics (csrc/stats_core.h, csrc/stats_rows.h) on the host,
// accumulated the way k_stats_blocks accumulates them.
//
// Stream jobs: what lacx_decoder_stats_batch_device runs on the device, one lane and one thread after the other -- the job
// planned by plan_decode(..., salvage, stats) and its tables filled by plan_fill_tables (csrc/decode_plan.h, the code
// api_decode.cpp runs), the lane code over the present blocks, ms_inverse_tile as k_ms_inverse's grid runs it, then the
// units as the workgroups and waves of k_stats_blocks take them: a wave of 64 full units of one counted block through the
// six xor-shuffle levels, its record left for the workgroup's first thread, which combines consecutive waves of one block
// and flushes one set; every other unit flushed by itself, a straddling unit as two records.  A flush into a row is the
// kernel's set of atomics: the same integer max / or / add, one after the other.
// Every buffer is a heap allocation of exactly the capacity the plan states -- the accumulator rows among them, inside the
// tables -- so that a build with AddressSanitizer reports any access outside them.
// Source jobs: one item of generated PCM in a layout, in allocations that END exactly at the source's last byte behind a
// base at the byte offset the case asks for, on a grid; optionally one element replaced by a raw 32-bit word (an invalid
// sample).
// It is not part of the product and is not a fallback.
//
// Built twice by tests/statstwin.py: a plain -O2 shared library for ctypes, and (-DSIM_STATS_MAIN) a sanitized program
// that runs a file of cases and prints one line per case.
#define SIM_JOB_SIMULATOR
#include "sim_job.h"

#include "import_msg.h"
#include "stats_rows.h"

using namespace lacx;
using namespace simjob;

namespace {

constexpr int kFill = 0xCD;
static_assert(sizeof(StatsAcc) == kStatsRowBytes, "the plan lays the accumulator rows out kStatsRowBytes apart");

struct UnitLane {
    bool valid = false, stereo = false;
    uint32_t j = 0, g0 = 0;
    StatsUnit su{};
};

// the kernel's flush: a record into a block's row, field by field
void flush(StatsAcc* rows, uint32_t g, const StatsAcc& a, bool stereo, uint64_t* sets) {
    stats_merge(rows[g], a, stereo);
    ++*sets;
}

// k_stats_blocks: workgroups of kDigestThreads units, waves of 64.  unit(j, f0, lane) is the kernel's per-item branch.
// sets: the sets of atomics issued.  Returns false where the lanes of a fast wave disagree on its record.
template <typename Unit>
bool accumulate_like_kernel(uint32_t nitems, unsigned long long total_units, const unsigned long long* unit_off, Unit unit, StatsAcc* rows,
                            uint64_t* sets) {
    for (unsigned long long first = 0; first < total_units; first += kDigestThreads) {
        uint32_t lo = 0;
        while (lo + 1 < nitems && unit_off[lo + 1] <= first) ++lo;
        const bool one_item = unit_off[lo + 1] >= first + kDigestThreads;
        StatsAcc wave_acc[kDigestThreads / 64u];
        uint32_t wave_blk[kDigestThreads / 64u], wave_stereo[kDigestThreads / 64u];
        for (uint32_t w = 0; w < kDigestThreads / 64u; ++w) {
            std::vector<UnitLane> ln(64);
            for (uint32_t lane = 0; lane < 64u; ++lane) {
                const unsigned long long u = first + 64u * w + lane;
                UnitLane& t = ln[lane];
                t.valid = u < total_units;
                if (!t.valid) continue;
                t.j = lo;
                if (!one_item) while (unit_off[t.j + 1] <= u) ++t.j;
                unit(t.j, (unsigned long long)kDigestUnitFrames * (u - unit_off[t.j]), t);
            }
            bool fast = true;
            for (uint32_t lane = 0; lane < 64u; ++lane) fast = fast && ln[lane].valid && ln[lane].su.n0 == kDigestUnitFrames && ln[lane].g0 == ln[0].g0;
            if (fast) {
                if (ln[0].su.use0) {
                    std::vector<StatsAcc> v(64), nv(64);
                    for (uint32_t lane = 0; lane < 64u; ++lane) v[lane] = ln[lane].su.p0;
                    for (uint32_t level = 0; level < 6u; ++level) {
                        for (uint32_t lane = 0; lane < 64u; ++lane) {
                            nv[lane] = v[lane];
                            stats_merge(nv[lane], v[lane ^ (1u << level)], ln[lane].stereo);
                        }
                        v = nv;
                    }
                    for (uint32_t lane = 1; lane < 64u; ++lane)
                        if (std::memcmp(&v[lane], &v[0], sizeof(StatsAcc)) != 0) return false;
                    wave_acc[w] = v[0];
                }
            } else {
                for (uint32_t lane = 0; lane < 64u; ++lane) {
                    const UnitLane& t = ln[lane];
                    if (!t.valid) continue;
                    if (t.su.use0 && t.su.n0) flush(rows, t.g0, t.su.p0, t.stereo, sets);
                    if (t.su.use1 && t.su.n1) flush(rows, t.g0 + 1u, t.su.p1, t.stereo, sets);
                }
            }
            const bool has = fast && ln[0].su.use0;
            wave_blk[w] = has ? ln[0].g0 : ~0u;
            wave_stereo[w] = ln[0].stereo ? 1u : 0u;
        }
        StatsAcc acc{};
        uint32_t blk = ~0u;
        bool st = false;
        for (uint32_t w = 0; w < kDigestThreads / 64u; ++w) {
            if (wave_blk[w] != blk) {
                if (blk != ~0u) flush(rows, blk, acc, st, sets);
                acc = StatsAcc{};
                blk = wave_blk[w];
                st = wave_stereo[w] != 0u;
            }
            if (blk != ~0u) stats_merge(acc, wave_acc[w], st);
        }
        if (blk != ~0u) flush(rows, blk, acc, st, sets);
    }
    return true;
}

struct Job {
    SalvageIn src;
    DecodePlan plan;
    std::vector<int> code;
    std::vector<std::string> err;
    std::unique_ptr<Run> run;
    uint64_t sets = 0;
    Job(const uint8_t* const* lacs, const uint64_t* sizes, uint32_t n) : src(lacs, sizes, n, false) {}
};

bool run(uint32_t n, int cols, bool zero_status, Job& j) {
    const BatchIn* in = j.src.in.data();
    if (plan_decode(in, n, DecodeForm::blocks, kWholeStreams, false, j.plan, j.code, j.err, true, false, true)) return false;
    if (j.plan.need.stats_rows != j.plan.total_blocks || j.plan.at.stats + kStatsRowBytes * j.plan.need.stats_rows != j.plan.need.tables) return false;
    j.run.reset(new Run(j.plan, in, (uint32_t)kDecodeTailPad, kFill, zero_status ? 0 : kFill));
    const DecodeArgs& a = j.run->a;
    place_payload(j.plan, in, j.run->payload.p);
    if (j.plan.items.empty()) return true;
    if (!a.present || a.block_raw || !a.no_output) return false;
    const StatsArgs s = plan_stats_args(j.plan, a, j.run->tables.p);
    Lane ln(cols, 0);
    run_lanes(a, ln);
    run_ms_inverse(a);
    // k_stats_blocks
    return accumulate_like_kernel(a.nitems, a.total_units, a.unit_off, [&](uint32_t item, unsigned long long f0, UnitLane& t) {
        const DecodeItem& it = a.items[item];
        t.stereo = it.channels == 2;
        t.su = stats_unit_decoded(f0, it.blocks, a.present[item], it.channels, it.bit_depth, it.frames, a.frame_off + it.block0, it.frame0,
                                  it.left, it.right, a.status + it.block0);
        t.g0 = it.block0 + t.su.b0;
    }, s.rows, &j.sets);
}

// the rows and totals of every planned item, made by the code the host side makes them with (stats_rows.h, called by
// collect of api_decode.cpp): fn(p, rows, totals)
template <typename Fn>
void results(const Job& j, Fn fn) {
    const StatsAcc* acc = reinterpret_cast<const StatsAcc*>(j.run->tables.p + j.plan.at.stats);
    salvage_records(j.plan, j.src.in.data(), j.run->st.p, false,
                    [&](const PlanItem& p, const lacx_salvage_result&, const std::vector<lacx_block_fault>& faults, const uint64_t*) {
        std::vector<lacx_block_stats> rows;
        stats_rows_of_decoded(j.src.in[p.src].lac, p.info.version, p.item.blocks, p.info.channels, faults, acc + p.item.block0, rows);
        const lacx_stats t = stats_combine(rows.data(), (uint32_t)rows.size(), p.info.channels, p.info.bit_depth, p.info.sample_rate);
        return fn(p, rows, t);
    });
}

std::string hex(uint64_t h) {
    char s[24];
    std::snprintf(s, sizeof(s), "%016llx", (unsigned long long)h);
    return s;
}

}  // namespace

extern "C" {

// n streams as one stats job.  Per input i, rec[2 * i] = the plan's code for it (0: it went to the device; then)
// rec[2 * i + 1] = its blocks.  rows: per accepted item in input order its lacx_block_stats records; totals: lacx_stats[n]
// (zero for a refused item).  msg: the refused items' messages, '\n' between inputs.  *sets: the sets of atomics
// k_stats_blocks would issue.  Returns the rows written, -1 where the job cannot be planned, rows_cap is too small or
// the lanes of a wave disagree.
int64_t sim_stats(const uint8_t* const* lacs, const uint64_t* sizes, uint32_t n, int cols, int zero_status, uint64_t* rec,
                  lacx_block_stats* rows, uint64_t rows_cap, lacx_stats* totals, char* msg, uint32_t msg_cap, uint64_t* sets) {
    if (cols != 1 && cols != 64) return -1;
    Job j(lacs, sizes, n);
    if (!run(n, cols, zero_status != 0, j)) return -1;
    std::string all;
    for (uint32_t i = 0; i < n; ++i) {
        rec[2 * i] = (uint64_t)j.code[i], rec[2 * i + 1] = 0;
        totals[i] = lacx_stats{};
        all += (i ? "\n" : "") + j.err[i];
    }
    std::snprintf(msg, msg_cap, "%s", all.c_str());
    uint64_t nrows = 0;
    bool fits = true;
    results(j, [&](const PlanItem& p, const std::vector<lacx_block_stats>& got, const lacx_stats& t) {
        if (nrows + got.size() > rows_cap) return fits = false;
        for (const lacx_block_stats& r : got) rows[nrows++] = r;
        rec[2 * p.src + 1] = got.size();
        totals[p.src] = t;
        return true;
    });
    *sets = j.sets;
    return fits ? (int64_t)nrows : -1;
}

// A stream case (little-endian, written by tests/statstwin.py): u32 n, u32 flags (4: 64 columns, 8: zero_status), then per
// stream u64 size and the bytes.  One line: "<index> <item>;<item>;..." with item = "!<code>" (refused by the plan) or
// "<blocks> <hash of the rows> <hash of the totals>".
int sim_stats_line(const uint8_t* blob, uint64_t size, uint32_t index, char* line, uint32_t cap) {
    if (size < 8) return -1;
    uint32_t n, flags;
    std::memcpy(&n, blob, 4), std::memcpy(&flags, blob + 4, 4);
    std::vector<std::unique_ptr<Heap<uint8_t>>> own;  // every stream an exact allocation of its own
    std::vector<const uint8_t*> lacs(n);
    std::vector<uint64_t> sizes(n);
    uint64_t at = 8;
    for (uint32_t i = 0; i < n; ++i) {
        if (size - at < 8) return -1;
        std::memcpy(&sizes[i], blob + at, 8);
        at += 8;
        if (size - at < sizes[i]) return -1;
        own.emplace_back(new Heap<uint8_t>(sizes[i]));
        std::memcpy(own.back()->p, blob + at, sizes[i]);
        at += sizes[i];
        lacs[i] = own.back()->p;
    }
    Job j(lacs.data(), sizes.data(), n);
    if (!run(n, (flags & 4u) ? 64 : 1, (flags & 8u) != 0, j)) return -1;
    std::vector<std::string> item(n);
    for (uint32_t i = 0; i < n; ++i) item[i] = "!" + std::to_string(j.code[i]);
    results(j, [&](const PlanItem& p, const std::vector<lacx_block_stats>& got, const lacx_stats& t) {
        item[p.src] = std::to_string(got.size()) + " " + hex(fnv(got.data(), got.size() * sizeof(lacx_block_stats), kFnvStart)) + " " +
                      hex(fnv(&t, sizeof(t), kFnvStart));
        return true;
    });
    std::string out = std::to_string(index) + " ";
    for (uint32_t i = 0; i < n; ++i) out += (i ? ";" : "") + item[i];
    if (out.size() + 1 > cap) return -1;
    std::memcpy(line, out.c_str(), out.size() + 1);
    return 0;
}

// The source form at unit level: one item of `frames` frames whose sample (c, f) is samples[c * frames + f] (for a float
// layout the exact float of that sample at the depth), laid out as `layout` in allocations that end with the source's
// last byte behind a base `offset` bytes behind a 16-byte aligned address (a planar right array at the same offset),
// measured on a grid of `grid` frames as k_stats_blocks<true> does.  bad_frame != all ones: element (bad_frame,
// bad_channel) of a 4-byte layout is the raw word bad_word instead.  *key: the lowest invalid sample's key (all ones:
// none), msg the text the product words it with.  Returns the blocks, -1 where rows_cap is too small or the lanes of a
// wave disagree.
int64_t sim_stats_source(uint32_t layout, uint32_t channels, uint32_t bit_depth, uint64_t frames, uint32_t grid, uint32_t offset,
                         const int32_t* samples, uint64_t bad_frame, uint32_t bad_channel, uint32_t bad_word, lacx_block_stats* rows,
                         uint64_t rows_cap, lacx_stats* totals, uint64_t* key, char* msg, uint32_t msg_cap, uint64_t* sets) {
    const uint32_t eb = elem_bytes(layout);
    const bool pl = planar(layout), f32 = layout == (uint32_t)PCM_PLANAR_F32 || layout == (uint32_t)PCM_INTERLEAVED_F32;
    const uint64_t bytes0 = pl ? frames * eb : frames * channels * eb;
    const bool two_rows = pl && channels == 2;
    Exact e0(bytes0, offset % 16u), e1(two_rows ? bytes0 : 0, offset % 16u);
    uint8_t* s0 = e0.data;
    uint8_t* s1 = two_rows ? e1.data : nullptr;
    for (uint64_t f = 0; f < frames; ++f)
        for (uint32_t c = 0; c < channels; ++c) {
            int32_t v = samples[c * frames + f];
            if (f32) {
                const float x = (float)v / (float)(1 << (bit_depth - 1));
                std::memcpy(&v, &x, 4);
            }
            if (f == bad_frame && c == bad_channel && eb == 4u) v = (int32_t)bad_word;
            put_elem(s0, s1, layout, channels, f, c, v);
        }
    const uint64_t nb = (frames + grid - 1) / grid;
    if (nb > rows_cap) return -1;
    Heap<StatsAcc> acc(nb);  // exactly the blocks' rows, zeroed
    const unsigned long long unit_off[2] = {0, (frames + 3u) / 4u};
    unsigned long long bad = kDigestClean;
    *sets = 0;
    const bool agreed = accumulate_like_kernel(1, unit_off[1], unit_off, [&](uint32_t, unsigned long long f0, UnitLane& t) {
        unsigned long long k = kDigestClean;
        t.stereo = channels == 2;
        t.su = stats_unit_source(f0, grid, (int)channels, (int)bit_depth, frames, s0, s1, layout, k);
        if (k < bad) bad = k;
        t.g0 = t.su.b0;
    }, acc.p, sets);
    if (!agreed) return -1;
    *key = bad;
    *totals = lacx_stats{};
    msg[0] = 0;
    if (bad != kDigestClean) {  // as digest_pcm_run of api_decode.cpp words it: a zeroed result and no rows
        ImportBad b{{kImportClean, kImportClean}};
        b.key[bad >> 63] = bad & ~(1ull << 63);
        int ch = 0;
        unsigned long long index = 0;
        std::string text;
        (void)import_bad_message(b, (int)bit_depth, &ch, &index, text);
        std::snprintf(msg, msg_cap, "%s", text.c_str());
        return 0;
    }
    std::vector<lacx_block_stats> got;
    stats_rows_of_source(frames, grid, (uint32_t)nb, channels, acc.p, got);
    for (uint64_t b = 0; b < nb; ++b) rows[b] = got[b];
    *totals = stats_combine(got.data(), (uint32_t)nb, (uint8_t)channels, (uint8_t)bit_depth, 0);
    return (int64_t)nb;
}

// stats_rows.h's totals through plain C
void sim_stats_combine(const lacx_block_stats* rows, uint32_t count, uint32_t channels, uint32_t bit_depth, uint32_t rate, lacx_stats* out) {
    *out = stats_combine(rows, count, (uint8_t)channels, (uint8_t)bit_depth, rate);
}

}  // extern "C"

#ifdef SIM_STATS_MAIN
// sim_stats_san CASES: every case of the file (per case: a 32-bit little-endian size, a type byte, then the bytes).
// Type 0: a stream case (sim_stats_line).  Type 1: a source case -- u32 layout, channels, bit_depth, grid, offset, u64 frames,
// u64 bad_frame, u32 bad_channel, bad_word, i32 samples[channels * frames] -- whose line is "<index> <key> <blocks> <hash of
// the rows> <hash of the totals> <message>".  "done <count>" at the end.
int main(int argc, char** argv) {
    if (argc != 2) return 2;
    std::vector<char> line(1 << 20);
    return for_each_case(argv[1], [&](const uint8_t* blob, uint32_t size, uint32_t i) {
        if (size < 1) return false;
        if (blob[0] == 0) {
            if (sim_stats_line(blob + 1, size - 1, i, line.data(), (uint32_t)line.size())) return false;
        } else {
            Reader rd{blob + 1, blob + size};
            const uint32_t layout = rd.get<uint32_t>(), channels = rd.get<uint32_t>(), depth = rd.get<uint32_t>(), grid = rd.get<uint32_t>();
            const uint32_t offset = rd.get<uint32_t>();
            const uint64_t frames = rd.get<uint64_t>(), bad_frame = rd.get<uint64_t>();
            const uint32_t bad_channel = rd.get<uint32_t>(), bad_word = rd.get<uint32_t>();
            if (!rd.ok || grid == 0 || (uint64_t)(rd.end - rd.p) != 4ull * channels * frames) return false;
            Heap<int32_t> samples(channels * frames);
            std::memcpy(samples.p, rd.p, 4ull * channels * frames);
            const uint64_t cap = frames / grid + 2;
            std::vector<lacx_block_stats> rows(cap);
            lacx_stats t{};
            uint64_t key = 0, sets = 0;
            char msg[256];
            const int64_t nb = sim_stats_source(layout, channels, depth, frames, grid, offset, samples.p, bad_frame, bad_channel, bad_word,
                                                rows.data(), cap, &t, &key, msg, sizeof(msg), &sets);
            if (nb < 0) return false;
            const std::string s = std::to_string(i) + " " + std::to_string(key) + " " + std::to_string(nb) + " " +
                                  hex(fnv(rows.data(), (uint64_t)nb * sizeof(lacx_block_stats), kFnvStart)) + " " + hex(fnv(&t, sizeof(t), kFnvStart)) +
                                  " " + msg;
            std::snprintf(line.data(), line.size(), "%s", s.c_str());
        }
        return std::puts(line.data()) >= 0;
    });
}
#endif
