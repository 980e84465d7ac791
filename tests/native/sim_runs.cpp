// tests/native/sim_runs.cpp -- TEST INFRASTRUCTURE: the run finder (csrc/runs_core.h, csrc/runs_plan.h, csrc/runs_rows.h) on the
// host, combined the way k_runs combines it.
//
// Stream jobs: what lacx_decoder_runs_batch_device runs on the device, one lane and one thread after the other -- the job
// planned by plan_decode(..., salvage, runs) and its tables filled by plan_fill_tables (csrc/decode_plan.h, the code
// api_decode.cpp runs), the lane code over the present blocks, ms_inverse_tile as k_ms_inverse's grid runs it, then the
// tiles as the workgroups of k_runs take them: every thread's unit, the frame in front of it through the workgroup's
// arrays (thread 0: the unit in front of the tile), per detector the mask and the summary, the inclusive scan over the 64
// lanes of a wave in six shuffle steps, the waves' totals combined in front of each wave, the walk of the four frames, the
// append through the list's counter with its capacity test, and the tile's row.  Where a counter outgrew its list the
// lists are laid out once more with the counters' capacities and the tiles run again, as api_decode.cpp does it; then
// runs_rows.h finishes the lists.
// Every buffer is a heap allocation of exactly the capacity the plan states -- the tables and the list buffer among them
// -- so that a build with AddressSanitizer reports any access outside them.
// Source jobs: one item of generated PCM in a layout, in allocations that END exactly at the source's last byte behind a
// base at the byte offset the case asks for; optionally one element replaced by a raw 32-bit word (an invalid sample).
// It is not part of the product and is not a fallback.
//
// Built twice by tests/runstwin.py: a plain -O2 shared library for ctypes, and (-DSIM_RUNS_MAIN) a sanitized program that
// runs a file of cases and prints one line per case.
#define SIM_JOB_SIMULATOR
#include "sim_job.h"

#include "import_msg.h"
#include "runs_rows.h"

using namespace lacx;
using namespace simjob;

namespace {

constexpr int kFill = 0xCD;

// k_runs over host pointers.  unit(j, f0) is the kernel's per-item branch; frames_of(j), stereo_of(j) the item's.
template <typename Unit, typename Frames, typename Stereo>
void runs_like_kernel(const RunsArgs& a, Unit unit, Frames frames_of, Stereo stereo_of) {
    constexpr uint32_t kWaves = kRunsThreads / 64u;
    for (unsigned long long tile = 0; tile < a.total_tiles; ++tile) {
        uint32_t j = 0;
        while (j + 1 < a.nitems && a.tile_off[j + 1] <= tile) ++j;
        const unsigned long long t = tile - a.tile_off[j], tile_start = t * kRunsTileFrames, frames = frames_of(j);
        const bool stereo = stereo_of(j);
        const RunsItem ri = a.items[j];
        std::vector<RunsUnit> u(kRunsThreads, RunsUnit{{0, 0, 0, 0}, {0, 0, 0, 0}, 0u});
        RunsUnit before{{0, 0, 0, 0}, {0, 0, 0, 0}, 0u};
        int32_t last_l[kRunsThreads], last_r[kRunsThreads];
        uint32_t last_c[kRunsThreads];
        for (uint32_t tid = 0; tid < kRunsThreads; ++tid) {
            const unsigned long long f0 = tile_start + kDigestUnitFrames * tid;
            if (f0 < frames) u[tid] = unit(j, f0);
            if (tid == 0u && t != 0u) before = unit(j, f0 - 4u);
            last_l[tid] = u[tid].l[3], last_r[tid] = u[tid].r[3], last_c[tid] = u[tid].counted >> 3;
        }
        for (uint32_t d = 0; d < ri.ndet; ++d) {
            const lacx_run_detector& det = a.dets[ri.det0 + d];
            uint32_t mask[kRunsThreads], excl[kRunsThreads], wave_tot[kWaves];
            for (uint32_t w = 0; w < kWaves; ++w) {
                uint32_t v[64], nv[64];
                for (uint32_t lane = 0; lane < 64u; ++lane) {
                    const uint32_t tid = 64u * w + lane;
                    const int32_t pl = tid ? last_l[tid - 1u] : before.l[3], pr = tid ? last_r[tid - 1u] : before.r[3];
                    const bool pc = (tid ? last_c[tid - 1u] : before.counted >> 3) != 0u;
                    mask[tid] = runs_mask(det, u[tid], pl, pr, pc, stereo);
                    v[lane] = runs_summary(mask[tid]);
                }
                for (uint32_t step = 1; step < 64u; step <<= 1) {  // __shfl_up: a lane below `step` keeps its own
                    for (uint32_t lane = 0; lane < 64u; ++lane) nv[lane] = lane >= step ? runs_combine(v[lane - step], v[lane]) : v[lane];
                    std::memcpy(v, nv, sizeof(v));
                }
                for (uint32_t lane = 0; lane < 64u; ++lane) excl[64u * w + lane] = lane ? v[lane - 1u] : kRunsIdentity;
                wave_tot[w] = v[63];
            }
            RunsList* list = &a.lists[ri.det0 + d];
            for (uint32_t tid = 0; tid < kRunsThreads; ++tid) {
                uint32_t prefix = kRunsIdentity;
                for (uint32_t w = 0; w < tid / 64u; ++w) prefix = runs_combine(prefix, wave_tot[w]);
                const uint32_t enter = runs_combine(prefix, excl[tid]) & ~kRunsAll;
                const unsigned long long f0 = tile_start + kDigestUnitFrames * tid;
                const RunsWalk w = runs_walk(mask[tid], enter, f0, tile_start, det.min_frames, [&](unsigned long long start, unsigned long long n) {
                    const unsigned long long at = list->count++;  // the counter counts every run; the store has the capacity test
                    if (at < list->cap) a.runs[list->off + at] = lacx_run{start, n};
                });
                RunsRow* row = &a.rows[ri.row0 + t * ri.ndet + d];
                if (w.lead) row->lead = (uint16_t)w.lead;
                if (tid == kRunsThreads - 1u) {
                    row->trail = (uint16_t)w.exit;
                    if (w.exit == kRunsTileFrames) row->lead = (uint16_t)w.exit;
                }
            }
        }
    }
}

// The host side behind the kernel (runs_fetch of api_decode.cpp): the second run with exact capacities where a counter
// outgrew its list.  list: the list buffer, replaced by one of exactly the new size.  again(list) runs the tiles.
template <typename Again>
bool rerun_if_outgrown(RunsLayout& y, uint8_t* tables, std::unique_ptr<Heap<lacx_run>>& list, Again again) {
    if (!runs_overflowed(y, tables)) return false;
    runs_recap(y, tables);
    list.reset(new Heap<lacx_run>(y.list_entries, kFill));
    again(list->p);
    return true;
}

struct Job {
    SalvageIn src;
    DecodePlan plan;
    std::vector<int> code;
    std::vector<std::string> err;
    std::unique_ptr<Run> run;
    std::unique_ptr<Heap<lacx_run>> list;
    RunsLayout y;
    bool rerun = false;
    Job(const uint8_t* const* lacs, const uint64_t* sizes, uint32_t n) : src(lacs, sizes, n, false) {}
};

bool run(uint32_t n, const lacx_run_query* queries, const lacx_run_detector* dets, uint32_t ndets, int cols, bool zero_status, uint64_t list_cap, Job& j) {
    std::vector<BatchIn>& in = j.src.in;
    for (uint32_t i = 0; i < n; ++i) {  // (resolve_queries of api_decode.cpp)
        in[i].dets_why = check_detectors(queries[i], dets, ndets);
        if (!in[i].dets_why) in[i].dets = dets + queries[i].first_detector, in[i].ndet = queries[i].detectors;
    }
    if (plan_decode(in.data(), n, DecodeForm::blocks, kWholeStreams, false, j.plan, j.code, j.err, true, false, false, true, list_cap)) return false;
    if (j.plan.runs_at.size != j.plan.need.tables) return false;
    j.run.reset(new Run(j.plan, in.data(), (uint32_t)kDecodeTailPad, kFill, zero_status ? 0 : kFill));
    const DecodeArgs& a = j.run->a;
    place_payload(j.plan, in.data(), j.run->payload.p);
    j.y = j.plan.runs_at;
    j.y.list_entries = j.plan.need.runs_list;
    if (j.plan.items.empty()) return true;
    if (!a.present || a.block_raw || !a.no_output) return false;
    j.list.reset(new Heap<lacx_run>(j.plan.need.runs_list, kFill));
    RunsArgs r = plan_runs_args(j.plan, a, j.run->tables.p, j.list->p);
    Lane ln(cols, 0);
    run_lanes(a, ln);
    run_ms_inverse(a);
    auto tiles = [&] {
        runs_like_kernel(r, [&](uint32_t item, unsigned long long f0) {
            const DecodeItem& it = a.items[item];
            return runs_unit_decoded(f0, it.blocks, a.present[item], it.channels, it.frames, a.frame_off + it.block0, it.frame0, it.left, it.right,
                                     a.status + it.block0);
        }, [&](uint32_t item) { return a.items[item].frames; }, [&](uint32_t item) { return a.items[item].channels == 2; });
    };
    tiles();
    j.rerun = rerun_if_outgrown(j.y, j.run->tables.p, j.list, [&](lacx_run* list) {
        r.runs = list;
        tiles();
    });
    return !runs_overflowed(j.y, j.run->tables.p);
}

// the result and the lists of every planned item, made by the code the host side makes them with: fn(p, result, lists)
template <typename Fn>
void results(const Job& j, Fn fn) {
    size_t at = 0;
    salvage_records(j.plan, j.src.in.data(), j.run->st.p, false,
                    [&](const PlanItem& p, const lacx_salvage_result& s, const std::vector<lacx_block_fault>&, const uint64_t*) {
        std::vector<std::vector<lacx_run>> lists;
        lacx_runs_result r = runs_item_result(j.y, j.run->tables.p, j.list->p, at++, p.item.frames, lists);
        r.lost_frames = s.lost_frames, r.sample_rate = p.info.sample_rate, r.blocks = s.blocks, r.lost_blocks = s.bad_blocks;
        r.flags = j.rerun ? LACX_RUNS_RERUN : 0u;
        r.channels = p.info.channels, r.bit_depth = p.info.bit_depth;
        return fn(p, r, lists);
    });
}

std::string hex(uint64_t h) {
    char s[24];
    std::snprintf(s, sizeof(s), "%016llx", (unsigned long long)h);
    return s;
}

uint64_t hash_lists(const std::vector<std::vector<lacx_run>>& lists) {
    uint64_t h = kFnvStart;
    for (const auto& l : lists) {
        const uint64_t n = l.size();
        h = fnv(&n, 8, h);
        h = fnv(l.data(), 16 * n, h);
    }
    return h;
}

}  // namespace

extern "C" {

// n streams as one runs job.  rec[i] = the plan's code for input i (0: it went to the device).  results: lacx_runs_result[n]
// (zero for a refused item).  runs / counts: the lists of every accepted item and detector, one behind the other in input
// order; counts[8 * i + k] = the runs of detector k of input i.  msg: the refused items' messages, '\n' between inputs.
// Returns the runs written, -1 where the job cannot be planned, runs_cap is too small or a list is still outgrown.
int64_t sim_runs(const uint8_t* const* lacs, const uint64_t* sizes, uint32_t n, const lacx_run_query* queries, const lacx_run_detector* dets,
                 uint32_t ndets, int cols, int zero_status, uint64_t list_cap, uint64_t* rec, lacx_runs_result* res, lacx_run* runs,
                 uint64_t runs_cap, uint64_t* counts, char* msg, uint32_t msg_cap) {
    if (cols != 1 && cols != 64) return -1;
    Job j(lacs, sizes, n);
    if (!run(n, queries, dets, ndets, cols, zero_status != 0, list_cap, j)) return -1;
    std::string all;
    for (uint32_t i = 0; i < n; ++i) {
        rec[i] = (uint64_t)j.code[i];
        res[i] = lacx_runs_result{};
        for (uint32_t k = 0; k < 8u; ++k) counts[8 * i + k] = 0;
        all += (i ? "\n" : "") + j.err[i];
    }
    std::snprintf(msg, msg_cap, "%s", all.c_str());
    // the lists in input order (the plan's order is the input's, without the refused)
    uint64_t total = 0;
    bool fits = true;
    results(j, [&](const PlanItem& p, const lacx_runs_result& r, const std::vector<std::vector<lacx_run>>& lists) {
        res[p.src] = r;
        for (size_t k = 0; k < lists.size(); ++k) {
            if (total + lists[k].size() > runs_cap) return fits = false;
            for (const lacx_run& x : lists[k]) runs[total++] = x;
            counts[8 * p.src + k] = lists[k].size();
        }
        return true;
    });
    return fits ? (int64_t)total : -1;
}

// A stream case (little-endian, written by tests/runstwin.py): u32 n, u32 flags (4: 64 columns, 8: zero_status), u64
// list_cap, u32 ndets, the detectors, n queries, then per stream u64 size and the bytes.  One line: "<index> <item>;..."
// with item = "!<code>" (refused by the plan) or "<hash of the result> <hash of the lists>".
int sim_runs_line(const uint8_t* blob, uint64_t size, uint32_t index, char* line, uint32_t cap) {
    Reader rd{blob, blob + size};
    const uint32_t n = rd.get<uint32_t>(), flags = rd.get<uint32_t>();
    const uint64_t list_cap = rd.get<uint64_t>();
    const uint32_t ndets = rd.get<uint32_t>();
    const std::vector<lacx_run_detector> dets = rd.array<lacx_run_detector>(ndets);
    const std::vector<lacx_run_query> queries = rd.array<lacx_run_query>(n);
    if (!rd.ok) return -1;
    std::vector<std::unique_ptr<Heap<uint8_t>>> own;  // every stream an exact allocation of its own
    std::vector<const uint8_t*> lacs(n);
    std::vector<uint64_t> sizes(n);
    for (uint32_t i = 0; i < n; ++i) {
        sizes[i] = rd.get<uint64_t>();
        if (!rd.ok || (uint64_t)(rd.end - rd.p) < sizes[i]) return -1;
        own.emplace_back(new Heap<uint8_t>(sizes[i]));
        std::memcpy(own.back()->p, rd.p, sizes[i]);
        rd.p += sizes[i];
        lacs[i] = own.back()->p;
    }
    Job j(lacs.data(), sizes.data(), n);
    if (!run(n, queries.data(), dets.data(), ndets, (flags & 4u) ? 64 : 1, (flags & 8u) != 0, list_cap, j)) return -1;
    std::vector<std::string> item(n);
    for (uint32_t i = 0; i < n; ++i) item[i] = "!" + std::to_string(j.code[i]);
    results(j, [&](const PlanItem& p, const lacx_runs_result& r, const std::vector<std::vector<lacx_run>>& lists) {
        item[p.src] = hex(fnv(&r, sizeof(r), kFnvStart)) + " " + hex(hash_lists(lists));
        return true;
    });
    std::string out = std::to_string(index) + " ";
    for (uint32_t i = 0; i < n; ++i) out += (i ? ";" : "") + item[i];
    if (out.size() + 1 > cap) return -1;
    std::memcpy(line, out.c_str(), out.size() + 1);
    return 0;
}

// The source form: one item of `frames` frames whose sample (c, f) is samples[c * frames + f] (for a float layout the
// exact float of that sample at the depth), laid out as `layout` in allocations that end with the source's last byte
// behind a base `offset` bytes behind a 16-byte aligned address (a planar right array at the same offset), searched with
// the ndet detectors as k_runs<true> does.  bad_frame != all ones: element (bad_frame, bad_channel) of a 4-byte layout is
// the raw word bad_word instead.  *key: the lowest invalid sample's key (all ones: none), msg the text the product words it
// with (then a zeroed result and no runs).  counts[k]: the runs of detector k, the lists one behind the other in runs.
// Returns the runs written, -1 where runs_cap is too small or the detectors are refused.
int64_t sim_runs_source(uint32_t layout, uint32_t channels, uint32_t bit_depth, uint64_t frames, uint32_t offset, const int32_t* samples,
                        const lacx_run_detector* dets, uint32_t ndet, uint64_t list_cap, uint64_t bad_frame, uint32_t bad_channel, uint32_t bad_word,
                        lacx_runs_result* res, lacx_run* runs, uint64_t runs_cap, uint64_t* counts, uint64_t* key, char* msg, uint32_t msg_cap) {
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
    const lacx_run_query q{0, ndet};
    if (check_detectors(q, dets, ndet)) return -1;
    const RunsIn in{dets, ndet, frames};
    RunsLayout y = runs_layout(0, &in, 1);
    Heap<uint8_t> tables(y.size);  // exactly the tables
    runs_fill(y, &in, 1, list_cap, tables.p);
    std::unique_ptr<Heap<lacx_run>> list(new Heap<lacx_run>(y.list_entries, kFill));
    RunsArgs a;
    runs_args(y, 1, tables.p, list->p, a);
    unsigned long long bad = kDigestClean;
    auto tiles = [&] {
        runs_like_kernel(a, [&](uint32_t, unsigned long long f0) {
            unsigned long long k = kDigestClean;
            const RunsUnit u = runs_unit_source(f0, (int)channels, (int)bit_depth, frames, s0, s1, layout, k);
            if (k < bad) bad = k;
            return u;
        }, [&](uint32_t) { return frames; }, [&](uint32_t) { return channels == 2; });
    };
    tiles();
    const bool rerun = rerun_if_outgrown(y, tables.p, list, [&](lacx_run* l) {
        a.runs = l;
        tiles();
    });
    if (runs_overflowed(y, tables.p)) return -1;
    *key = bad;
    *res = lacx_runs_result{};
    for (uint32_t k = 0; k < 8u; ++k) counts[k] = 0;
    msg[0] = 0;
    if (bad != kDigestClean) {  // as digest_pcm_run of api_decode.cpp words it: a zeroed result and no runs
        ImportBad b{{kImportClean, kImportClean}};
        b.key[bad >> 63] = bad & ~(1ull << 63);
        int ch = 0;
        unsigned long long index = 0;
        std::string text;
        (void)import_bad_message(b, (int)bit_depth, &ch, &index, text);
        std::snprintf(msg, msg_cap, "%s", text.c_str());
        return 0;
    }
    std::vector<std::vector<lacx_run>> lists;
    *res = runs_item_result(y, tables.p, list->p, 0, frames, lists);
    res->blocks = (uint32_t)((frames + kMaxBlock - 1u) / kMaxBlock);
    res->flags = rerun ? LACX_RUNS_RERUN : 0u;
    res->channels = (uint8_t)channels, res->bit_depth = (uint8_t)bit_depth;
    uint64_t total = 0;
    for (size_t k = 0; k < lists.size(); ++k) {
        if (total + lists[k].size() > runs_cap) return -1;
        for (const lacx_run& x : lists[k]) runs[total++] = x;
        counts[k] = lists[k].size();
    }
    return (int64_t)total;
}

// runs_rows.h's stitching of fabricated rows through plain C: rows[tile] = lead | trail << 16 of one detector.  Returns the
// runs written (at most cap).
int64_t sim_runs_stitch(uint64_t frames, const uint32_t* packed, uint64_t min_frames, lacx_run* out, uint64_t cap) {
    const uint64_t tiles = (frames + kRunsTileFrames - 1u) / kRunsTileFrames;
    std::vector<RunsRow> rows(tiles);
    for (uint64_t t = 0; t < tiles; ++t) rows[t] = RunsRow{(uint16_t)(packed[t] & 0xFFFFu), (uint16_t)(packed[t] >> 16)};
    std::vector<lacx_run> got;
    runs_finish(frames, rows.data(), 1, 0, min_frames, nullptr, 0, got);
    if (got.size() > cap) return -1;
    for (size_t k = 0; k < got.size(); ++k) out[k] = got[k];
    return (int64_t)got.size();
}

// the plan's list reservation and detector checks through plain C
uint64_t sim_runs_reserve(uint64_t frames, uint64_t min_frames, uint64_t cap) { return runs_reserve(frames, min_frames, cap); }
const char* sim_runs_check(const lacx_run_query* q, const lacx_run_detector* dets, uint32_t ndets) {
    const char* why = check_detectors(*q, dets, ndets);
    return why ? why : "";
}

// The runs form of the plan for n streams: out[0..7] = tables, runs_list, the layout's base, lists, rows, total_tiles,
// total_dets, total_rows; raw: the filled tables (made-up base addresses: nothing is dereferenced).  -1 where it cannot be
// planned or raw_cap is too small.
int sim_runs_plan(const uint8_t* const* lacs, const uint64_t* sizes, uint32_t n, const lacx_run_query* queries, const lacx_run_detector* dets,
                  uint32_t ndets, uint64_t list_cap, uint64_t* out, uint8_t* raw, uint64_t raw_cap) {
    Job j(lacs, sizes, n);
    std::vector<BatchIn>& in = j.src.in;
    for (uint32_t i = 0; i < n; ++i) {
        in[i].dets_why = check_detectors(queries[i], dets, ndets);
        if (!in[i].dets_why) in[i].dets = dets + queries[i].first_detector, in[i].ndet = queries[i].detectors;
    }
    if (plan_decode(in.data(), n, DecodeForm::blocks, kWholeStreams, false, j.plan, j.code, j.err, true, false, false, true, list_cap)) return -1;
    const RunsLayout& y = j.plan.runs_at;
    const uint64_t v[8] = {j.plan.need.tables, j.plan.need.runs_list, y.base, y.lists, y.rows, y.total_tiles, y.total_dets, y.total_rows};
    for (int k = 0; k < 8; ++k) out[k] = v[k];
    if (j.plan.need.tables > raw_cap) return -1;
    Heap<uint8_t> tables(j.plan.need.tables, kFill);
    plan_fill_tables(j.plan, in.data(), PlanBases{nullptr, nullptr, nullptr, nullptr}, tables.p);
    std::memcpy(raw, tables.p, j.plan.need.tables);
    return 0;
}

}  // extern "C"

#ifdef SIM_RUNS_MAIN
// sim_runs_san CASES: every case of the file (per case: a 32-bit little-endian size, a type byte, then the bytes).
// Type 0: a stream case (sim_runs_line).  Type 1: a source case -- u32 layout, channels, bit_depth, offset, ndet, u64 frames,
// list_cap, bad_frame, u32 bad_channel, bad_word, the detectors, i32 samples[channels * frames] -- whose line is "<index> <key>
// <hash of the result> <hash of the lists> <message>".  "done <count>" at the end.
int main(int argc, char** argv) {
    if (argc != 2) return 2;
    std::vector<char> line(1 << 20);
    return for_each_case(argv[1], [&](const uint8_t* blob, uint32_t size, uint32_t i) {
        if (size < 1) return false;
        if (blob[0] == 0) {
            if (sim_runs_line(blob + 1, size - 1, i, line.data(), (uint32_t)line.size())) return false;
        } else {
            Reader rd{blob + 1, blob + size};
            const uint32_t layout = rd.get<uint32_t>(), channels = rd.get<uint32_t>(), depth = rd.get<uint32_t>(), offset = rd.get<uint32_t>();
            const uint32_t ndet = rd.get<uint32_t>();
            const uint64_t frames = rd.get<uint64_t>(), list_cap = rd.get<uint64_t>(), bad_frame = rd.get<uint64_t>();
            const uint32_t bad_channel = rd.get<uint32_t>(), bad_word = rd.get<uint32_t>();
            const std::vector<lacx_run_detector> dets = rd.array<lacx_run_detector>(ndet);
            if (!rd.ok || ndet > 8u || (uint64_t)(rd.end - rd.p) != 4ull * channels * frames) return false;
            Heap<int32_t> samples(channels * frames);
            std::memcpy(samples.p, rd.p, 4ull * channels * frames);
            const uint64_t cap = (frames + 2) * ndet;
            std::vector<lacx_run> runs(cap);
            lacx_runs_result r{};
            uint64_t key = 0, counts[8];
            char msg[256];
            const int64_t got = sim_runs_source(layout, channels, depth, frames, offset, samples.p, dets.data(), ndet, list_cap, bad_frame, bad_channel,
                                                bad_word, &r, runs.data(), cap, counts, &key, msg, sizeof(msg));
            if (got < 0) return false;
            uint64_t h = fnv(counts, sizeof(counts), kFnvStart);
            h = fnv(runs.data(), 16ull * (uint64_t)got, h);
            const std::string s = std::to_string(i) + " " + std::to_string(key) + " " + hex(fnv(&r, sizeof(r), kFnvStart)) + " " + hex(h) + " " + msg;
            std::snprintf(line.data(), line.size(), "%s", s.c_str());
        }
        return std::puts(line.data()) >= 0;
    });
}
#endif
