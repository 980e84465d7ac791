// tests/native/sim_compare.cpp -- TEST INFRASTRUCTURE: the bit-compare job (csrc/compare_core.h, csrc/compare_plan.h,
// csrc/compare_rows.h) on the host, run the way k_compare_search and k_compare_rows of k_compare.hip run it.
//
// Stream jobs: what lacx_decoder_compare_batch_device runs on the device, one lane after the other -- the job planned by
// plan_decode_job(..., digest form, the pairs) and its tables filled by plan_fill_tables (csrc/decode_plan.h, the code
// api_decode.cpp runs), the lane code over the blocks, ms_inverse_tile as k_ms_inverse's grid runs it, then the search: per
// tile the units staged in arrays of exactly the kernel's LDS sizes (filled with a byte pattern: every word must be written
// before it is read), every lane's walk over its stripe, and the lanes' counts of the pair's offsets added into the job's
// counts; the host's choice (cmp_choose_all, cmp_fill_choice); then the rows: per row every thread's record, merged as the
// kernel's tree merges them, written whole.  The tables are exactly the plan's size, the rows a byte pattern before they are
// written.  Source jobs: sources of given PCM in a layout, in allocations that END exactly at the source's last byte behind a
// base at the byte offset the case asks for; optionally one element replaced by a raw 32-bit word (an invalid sample).
// A case (little-endian, written by tests/comparetwin.py): u8 form (0 streams, 1 sources), u32 sources, u32 pairs, then per
// pair u32 a, u32 b, i64 centre, u32 radius, then per source -- streams: u64 size and the bytes; sources: u32 layout, u32
// offset, u32 channels, u32 bit depth, u32 sample rate, u64 frames, u64 bad_frame, u32 bad_channel, u32 bad_word, i32
// left[frames], i32 right[frames].
// It is not part of the product and is not a fallback.
//
// Built twice by tests/comparetwin.py: a plain -O2 shared library for ctypes, and (-DSIM_COMPARE_MAIN) a sanitized program
// that runs a file of cases and prints one line per case.
#define SIM_JOB_SIMULATOR
#include "sim_job.h"

#include "compare_core.h"
#include "import_msg.h"

using namespace lacx;
using namespace simjob;

namespace {

constexpr int kFill = 0xCD;

// launch_compare_search: every tile, every lane of each
void run_search(const CmpArgs& a) {
    for (unsigned long long tile = 0; tile < a.total_tiles; ++tile) {
        uint32_t j = 0;
        while (j + 1 < a.nspans && a.tile_off[j + 1] <= tile) ++j;
        const CmpSpan sp = a.spans[j];
        const CmpPair pr = a.pairs[sp.pair];
        const CmpSource sa = a.sources[pr.a], sb = a.sources[pr.b];
        const CmpTile y = cmp_tile(sp, pr, tile - a.tile_off[j]);
        if (cmp_tile_empty(y, sa.frames, sb.frames)) continue;
        const uint32_t planes = cmp_planes(sa);
        Heap<uint32_t> stage_a(2u * kCmpStageA, kFill), stage_b(2u * kCmpStageB, kFill);  // (malloc: 16-byte aligned)
        auto note = [&](uint32_t item, unsigned long long key) {
            if (key < a.bad[item]) a.bad[item] = key;
        };
        if (y.units_a > kCmpStageA / 4u || y.units_b > kCmpStageB / 4u) std::abort();
        for (uint32_t u = 0; u < y.units_a; ++u) {
            uint32_t w0[4], w1[4];
            cmp_stage_unit(sa, y.g0 + 4ll * (long long)u, planes, w0, w1, note);
            std::memcpy(stage_a.p + 4u * u, w0, 16);
            if (planes == 2u) std::memcpy(stage_a.p + kCmpStageA + 4u * u, w1, 16);
        }
        for (uint32_t u = 0; u < y.units_b; ++u) {
            uint32_t w0[4], w1[4];
            cmp_stage_unit(sb, y.b0 + 4ll * (long long)u, planes, w0, w1, note);
            std::memcpy(stage_b.p + 4u * u, w0, 16);
            if (planes == 2u) std::memcpy(stage_b.p + kCmpStageB + 4u * u, w1, 16);
        }
        const long long first = (long long)pr.centre - (long long)pr.radius;
        for (uint32_t tid = 0; tid < kCmpThreads; ++tid) {
            uint32_t cnt[4] = {0, 0, 0, 0};
            if (sa.bit_depth == 16) {
                cmp_search_lane<true>(stage_a.p, stage_b.p, sp, y, tid, cnt);
            } else {
                cmp_search_lane<false>(stage_a.p, stage_b.p, sp, y, tid, cnt);
                if (planes == 2u) cmp_search_lane<false>(stage_a.p + kCmpStageA, stage_b.p + kCmpStageB, sp, y, tid, cnt);
            }
            for (uint32_t k = 0; k < 4u; ++k) {  // the stripes' parts and the atomics: adds into the zeroed counts
                const long long at = y.o0 + (long long)(4u * (tid & (sp.lanes - 1u)) + k) - first;
                if (at >= 0 && at < (long long)cmp_width(pr)) a.counts[pr.count0 + (unsigned long long)at] += cnt[k];
            }
        }
    }
}

// launch_compare_rows: every row, every thread of each, the kernel's tree
void run_rows(const CmpArgs& a) {
    for (unsigned long long row = 0; row < a.total_rows; ++row) {
        uint32_t j = 0;
        while (j + 1 < a.npairs && a.row_off[j + 1] <= row) ++j;
        const CmpPair pr = a.pairs[j];
        const unsigned long long r = row - a.row_off[j];
        if (r >= pr.nrows) std::abort();
        Heap<lacx_compare_channel_row> acc(2u * kCmpThreads, kFill);
        for (uint32_t tid = 0; tid < kCmpThreads; ++tid) {
            lacx_compare_channel_row mine[2];
            cmp_row_thread(a.sources, pr, r, tid, mine, [&](uint32_t item, unsigned long long key) {
                if (key < a.bad[item]) a.bad[item] = key;
            });
            acc.p[tid] = mine[0], acc.p[kCmpThreads + tid] = mine[1];
        }
        for (uint32_t step = kCmpThreads / 2u; step >= 1u; step >>= 1)
            for (uint32_t tid = 0; tid < step; ++tid) {
                cmp_row_merge(acc.p[tid], acc.p[tid + step]);
                cmp_row_merge(acc.p[kCmpThreads + tid], acc.p[kCmpThreads + tid + step]);
            }
        lacx_compare_row out;
        out.ch[0] = acc.p[0], out.ch[1] = acc.p[kCmpThreads];
        std::memcpy(static_cast<uint8_t*>(a.rows) + kCmpRowBytes * (pr.row0 + r), &out, sizeof(out));
    }
}

// compare_kernels of api_decode.cpp: the search, the choice, the rows; the tables at `tables`
void run_compare(CmpLayout& y, uint8_t* tables, unsigned long long* bad) {
    if (y.search) {
        run_search(cmp_args(y, tables, bad));
        cmp_choose_all(y, reinterpret_cast<const unsigned long long*>(tables + y.counts));
        cmp_fill_choice(y, tables);
    }
    run_rows(cmp_args(y, tables, bad));
}

struct PairOut {
    int code = 0;  // 0: it has an answer; else the ABI's code (a decode failure: LACX_E_RUNTIME)
    std::string text;
    lacx_compare totals{};
    std::vector<lacx_compare_row> rows;
    std::vector<uint64_t> counts;
};

struct SourceCase {
    uint32_t layout, offset, channels, depth, rate;
    uint64_t frames, bad_frame;
    uint32_t bad_channel, bad_word;
    const uint8_t* samples;  // i32 left[frames], right[frames], unaligned
};
struct Case {
    uint8_t form;
    std::vector<lacx_compare_pair> pairs;
    std::vector<std::pair<const uint8_t*, uint64_t>> lacs;
    std::vector<SourceCase> srcs;
};

bool read_case(const uint8_t* blob, uint64_t size, Case& c) {
    Reader rd{blob, blob + size};
    c.form = rd.get<uint8_t>();
    const uint32_t ns = rd.get<uint32_t>(), np = rd.get<uint32_t>();
    if (!rd.ok || c.form > 1 || ns > (1u << 20) || np > (1u << 20)) return false;
    for (uint32_t k = 0; k < np; ++k) {
        lacx_compare_pair p{};
        p.a = rd.get<uint32_t>(), p.b = rd.get<uint32_t>(), p.centre = rd.get<int64_t>(), p.radius = rd.get<uint32_t>();
        c.pairs.push_back(p);
    }
    for (uint32_t i = 0; rd.ok && i < ns; ++i) {
        if (c.form == 0) {
            const uint64_t bytes = rd.get<uint64_t>();
            if (!rd.ok || bytes > (uint64_t)(rd.end - rd.p)) return false;
            c.lacs.emplace_back(rd.p, bytes);
            rd.p += bytes;
        } else {
            SourceCase s{};
            s.layout = rd.get<uint32_t>(), s.offset = rd.get<uint32_t>(), s.channels = rd.get<uint32_t>(), s.depth = rd.get<uint32_t>(), s.rate = rd.get<uint32_t>();
            s.frames = rd.get<uint64_t>(), s.bad_frame = rd.get<uint64_t>(), s.bad_channel = rd.get<uint32_t>(), s.bad_word = rd.get<uint32_t>();
            if (!rd.ok || s.frames > (uint64_t)(rd.end - rd.p) / 8u) return false;
            s.samples = rd.p;
            rd.p += 8u * s.frames;
            c.srcs.push_back(s);
        }
    }
    return rd.ok && rd.p == rd.end;
}

// the host's refusals, as api_decode.cpp's cmp_resolve makes them; then the accepted pairs over the sources they name
struct Accepted {
    std::vector<uint32_t> used, order, which;
    std::vector<CmpPairIn> pairs;
};
void resolve(const Case& c, const std::vector<CmpFmt>& fmt, const std::vector<int>& src_code, const std::vector<std::string>& src_why, std::vector<PairOut>& out,
             Accepted& acc) {
    const uint32_t ns = (uint32_t)fmt.size();
    acc.used.assign(ns, ~0u);
    for (size_t k = 0; k < c.pairs.size(); ++k) {
        const lacx_compare_pair& x = c.pairs[k];
        PairOut& o = out[k];
        if (x.a >= ns || x.b >= ns) {
            o.code = LACX_E_INVALID, o.text = "sources outside the call's array";
            continue;
        }
        for (uint32_t at : {x.a, x.b})
            if (!o.code && src_code[at] != LACX_OK) o.code = src_code[at], o.text = "source " + std::to_string(at) + ": " + src_why[at];
        if (o.code) continue;
        o.text = cmp_pair_why(x, fmt.data(), ns);
        if (!o.text.empty()) {
            o.code = LACX_E_INVALID;
            continue;
        }
        for (uint32_t at : {x.a, x.b})
            if (acc.used[at] == ~0u) acc.used[at] = (uint32_t)acc.order.size(), acc.order.push_back(at);
        acc.pairs.push_back(CmpPairIn{acc.used[x.a], acc.used[x.b], (long long)x.centre, x.radius});
        acc.which.push_back((uint32_t)k);
    }
}

void take(const CmpLayout& y, size_t slot, const uint8_t* tables, uint32_t rate, PairOut& o) {
    const CmpPair& p = y.pair[slot];
    const auto* rows = reinterpret_cast<const lacx_compare_row*>(tables + y.rows) + p.row0;
    o.rows.assign(rows, rows + p.nrows);
    o.totals = cmp_result(y, slot, o.rows.data(), rate);
    if (p.radius) {
        const auto* counts = reinterpret_cast<const uint64_t*>(tables + y.counts) + p.count0;
        o.counts.assign(counts, counts + cmp_width(p));
    }
}

bool run_stream_case(const Case& c, std::vector<PairOut>& out) {
    const uint32_t ns = (uint32_t)c.lacs.size();
    std::vector<CmpFmt> fmt(ns);
    std::vector<int> src_code(ns, LACX_OK);
    std::vector<std::string> src_why(ns);
    for (uint32_t i = 0; i < ns; ++i) {
        lacx_stream_info f{};
        const char* why = nullptr;
        src_code[i] = parse_stream(c.lacs[i].first, c.lacs[i].second, &f, &why);
        if (src_code[i] != LACX_OK) src_why[i] = why ? why : "";
        else if (f.frames == 0) src_code[i] = LACX_E_INVALID, src_why[i] = "source has no frames";
        fmt[i] = CmpFmt{f.frames, f.sample_rate, (uint8_t)f.channels, (uint8_t)f.bit_depth};
    }
    Accepted acc;
    resolve(c, fmt, src_code, src_why, out, acc);
    if (acc.pairs.empty()) return true;
    std::vector<std::unique_ptr<Heap<uint8_t>>> own;  // every stream an exact allocation of its own
    std::vector<BatchIn> in;
    for (uint32_t at : acc.order) {
        own.emplace_back(new Heap<uint8_t>(c.lacs[at].second));
        std::memcpy(own.back()->p, c.lacs[at].first, c.lacs[at].second);
        in.push_back(BatchIn{own.back()->p, c.lacs[at].second, nullptr, nullptr, 0});
    }
    const CmpJobIn job{acc.pairs.data(), (uint32_t)acc.pairs.size()};
    DecodePlan plan;
    std::vector<int> code;
    std::vector<std::string> err;
    if (plan_decode_job(in.data(), (uint32_t)in.size(), DecodeForm::digest, kWholeStreams, false, plan, code, err, false, false, false, false, kRunsListCap, false, false, 0,
                        nullptr, &job))
        return false;
    if (plan.cmp_at.size != plan.need.tables) return false;
    Run run(plan, in.data(), (uint32_t)kDecodeTailPad, kFill, kFill);
    place_payload(plan, in.data(), run.payload.p);
    if (plan.items.empty()) return false;
    if (run.a.digest || run.a.present || run.a.verify || run.a.window || run.a.wav) return false;  // launch_decode must end with k_ms_inverse in place
    Lane ln(1, 0);
    run_lanes(run.a, ln);
    run_ms_inverse(run.a);
    CmpLayout y = plan.cmp_at;
    std::memset(run.tables.p + y.rows, kFill, y.size - y.rows);
    run_compare(y, run.tables.p, nullptr);
    std::vector<uint32_t> status(in.size(), 0);  // per input its first failing block's status
    for (const PlanItem& p : plan.items)
        for (uint32_t b = 0; b < p.item.blocks && !status[p.src]; ++b) status[p.src] = run.st.p[p.item.block0 + b];
    for (size_t a = 0; a < acc.pairs.size(); ++a) {
        const uint32_t k = acc.which[a];
        PairOut& o = out[k];
        for (uint32_t at : {c.pairs[k].a, c.pairs[k].b}) {
            const uint32_t i = acc.used[at];
            if (o.code) continue;
            if (code[i] != LACX_OK) o.code = code[i], o.text = "source " + std::to_string(at) + ": " + err[i];
            else if (status[i]) o.code = LACX_E_RUNTIME, o.text = "source " + std::to_string(at) + ": status " + std::to_string(status[i]);
        }
        if (o.code) continue;
        size_t slot = 0;
        while (slot < plan.cmp_pair.size() && plan.cmp_pair[slot] != a) ++slot;
        if (slot == plan.cmp_pair.size()) return false;
        take(y, slot, run.tables.p, fmt[c.pairs[k].a].sample_rate, o);
    }
    return true;
}

const char* source_why(const SourceCase& s) {  // check_digest_source's, as far as a case can go wrong
    if (s.channels != 1 && s.channels != 2) return "unsupported channel count";
    if (s.frames == 0) return "source has no frames";
    return nullptr;
}

bool run_source_case(const Case& c, std::vector<PairOut>& out) {
    const uint32_t ns = (uint32_t)c.srcs.size();
    std::vector<CmpFmt> fmt(ns);
    std::vector<int> src_code(ns, LACX_OK);
    std::vector<std::string> src_why(ns);
    for (uint32_t i = 0; i < ns; ++i) {
        const SourceCase& s = c.srcs[i];
        if (const char* why = source_why(s)) src_code[i] = LACX_E_INVALID, src_why[i] = why;
        fmt[i] = CmpFmt{s.frames, s.rate, (uint8_t)s.channels, (uint8_t)s.depth};
    }
    Accepted acc;
    resolve(c, fmt, src_code, src_why, out, acc);
    if (acc.pairs.empty()) return true;
    std::vector<std::unique_ptr<Exact>> own;
    std::vector<CmpSrcIn> in;
    for (uint32_t at : acc.order) {
        const SourceCase& s = c.srcs[at];
        const uint32_t eb = elem_bytes(s.layout);
        const bool pl = planar(s.layout), f32 = s.layout == (uint32_t)PCM_PLANAR_F32 || s.layout == (uint32_t)PCM_INTERLEAVED_F32;
        const uint64_t bytes0 = pl ? s.frames * eb : s.frames * s.channels * eb;
        own.emplace_back(new Exact(bytes0, s.offset % 16u));
        uint8_t* s0 = own.back()->data;
        uint8_t* s1 = nullptr;
        if (pl && s.channels == 2) {
            own.emplace_back(new Exact(bytes0, s.offset % 16u));
            s1 = own.back()->data;
        }
        for (uint64_t f = 0; f < s.frames; ++f)
            for (uint32_t ch = 0; ch < s.channels; ++ch) {
                int32_t v;
                std::memcpy(&v, s.samples + 4u * (ch * s.frames + f), 4);
                if (f32) {
                    const float x = (float)v / (s.depth == 16 ? 32768.0f : 8388608.0f);
                    std::memcpy(&v, &x, 4);
                }
                if (f == s.bad_frame && ch == s.bad_channel && eb == 4u) v = (int32_t)s.bad_word;
                put_elem(s0, s1, s.layout, (int)s.channels, f, ch, v);
            }
        in.push_back(CmpSrcIn{s0, s1, s.frames, s.layout, (uint32_t)in.size(), (uint8_t)s.channels, (uint8_t)s.depth, true});
    }
    if (cmp_check(in.data(), acc.pairs.data(), acc.pairs.size())) return false;
    CmpLayout y = cmp_layout(0, in.data(), in.size(), acc.pairs.data(), acc.pairs.size());
    Heap<uint8_t> tables(y.size, kFill);
    std::vector<unsigned long long> bad(in.size(), kDigestClean);
    cmp_fill(y, in.data(), tables.p);
    run_compare(y, tables.p, bad.data());
    for (size_t a = 0; a < acc.pairs.size(); ++a) {
        const uint32_t k = acc.which[a];
        PairOut& o = out[k];
        for (uint32_t at : {c.pairs[k].a, c.pairs[k].b}) {
            const unsigned long long key = bad[acc.used[at]];
            if (o.code || key == kDigestClean) continue;
            ImportBad b{{kImportClean, kImportClean}};  // as api_decode.cpp words it
            b.key[key >> 63] = key & ~(1ull << 63);
            int ch = 0;
            unsigned long long index = 0;
            std::string text;
            (void)import_bad_message(b, (int)c.srcs[at].depth, &ch, &index, text);
            o.code = LACX_E_INVALID, o.text = "source " + std::to_string(at) + ": " + text;
        }
        if (!o.code) take(y, a, tables.p, fmt[c.pairs[k].a].sample_rate, o);
    }
    return true;
}

bool run_case(const uint8_t* blob, uint64_t size, std::vector<PairOut>& out) {
    Case c;
    if (!read_case(blob, size, c)) return false;
    out.assign(c.pairs.size(), PairOut{});
    return c.form == 0 ? run_stream_case(c, out) : run_source_case(c, out);
}

std::string hex(uint64_t h) {
    char s[24];
    std::snprintf(s, sizeof(s), "%016llx", (unsigned long long)h);
    return s;
}

}  // namespace

extern "C" {

// A case as one job.  Per pair k: rec[4 k] = its code (0: it has an answer), rec[4 k + 1] = its rows, rec[4 k + 2] = its
// counts, rec[4 k + 3] = 0; totals: lacx_compare[pairs]; rows, counts: the pairs' one behind the other; msg: the pairs' texts,
// '\n' between them.  Returns the rows written, -1 where the case cannot be read or run or a capacity is too small.
int64_t sim_cmp_run(const uint8_t* blob, uint64_t size, uint64_t* rec, lacx_compare* totals, lacx_compare_row* rows, uint64_t rows_cap, uint64_t* counts,
                    uint64_t counts_cap, char* msg, uint32_t msg_cap) {
    std::vector<PairOut> out;
    if (!run_case(blob, size, out)) return -1;
    std::string all;
    uint64_t at = 0, ct = 0;
    for (size_t k = 0; k < out.size(); ++k) {
        const PairOut& o = out[k];
        if (at + o.rows.size() > rows_cap || ct + o.counts.size() > counts_cap) return -1;
        rec[4 * k] = (uint64_t)o.code, rec[4 * k + 1] = o.rows.size(), rec[4 * k + 2] = o.counts.size(), rec[4 * k + 3] = 0;
        totals[k] = o.totals;
        if (!o.rows.empty()) std::memcpy(rows + at, o.rows.data(), sizeof(lacx_compare_row) * o.rows.size());
        if (!o.counts.empty()) std::memcpy(counts + ct, o.counts.data(), 8 * o.counts.size());
        at += o.rows.size(), ct += o.counts.size();
        all += (k ? "\n" : "") + o.text;
    }
    if (all.size() + 1 > msg_cap) return -1;
    std::memcpy(msg, all.c_str(), all.size() + 1);
    return (int64_t)at;
}

// One line for a case: "<index> <pair>;<pair>;..." with pair = "!<code> <text>" or "<rows> <hash of the rows> <hash of the
// counts> <hash of the totals>".
int sim_cmp_line(const uint8_t* blob, uint64_t size, uint32_t index, char* line, uint32_t cap) {
    std::vector<PairOut> out;
    if (!run_case(blob, size, out)) return -1;
    std::string s = std::to_string(index) + " ";
    for (size_t k = 0; k < out.size(); ++k) {
        const PairOut& o = out[k];
        s += k ? ";" : "";
        if (o.code) s += "!" + std::to_string(o.code) + " " + o.text;
        else
            s += std::to_string(o.rows.size()) + " " + hex(fnv(o.rows.data(), sizeof(lacx_compare_row) * o.rows.size(), kFnvStart)) + " " +
                 hex(fnv(o.counts.data(), 8 * o.counts.size(), kFnvStart)) + " " + hex(fnv(&o.totals, sizeof(o.totals), kFnvStart));
    }
    if (s.size() + 1 > cap) return -1;
    std::memcpy(line, s.c_str(), s.size() + 1);
    return 0;
}

// compare_rows.h's totals through plain C (what lacx_compare_combine calls)
void sim_cmp_combine(const lacx_compare_row* rows, uint64_t count, uint8_t channels, uint8_t bit_depth, uint32_t rate, uint64_t na, uint64_t nb, int64_t o,
                     lacx_compare* out) {
    *out = cmp_combine(rows, count, channels, bit_depth, rate, na, nb, o);
}

// the choice alone
int64_t sim_cmp_choose(const uint64_t* counts, int64_t centre, uint32_t radius) {
    return cmp_choose(reinterpret_cast<const unsigned long long*>(counts), centre, radius);
}

// the plan of one pair of frame counts: out[0] = search tiles, [1] = spans, [2] = lanes, [3] = offset tiles, [4] = rows
// reserved, [5] = counts, [6] = the tables' size from base 0, [7] = the capacity check's own tile bound must not be below [0]:
// 1 where it holds; then per span f_lo, f_hi.  why: the refusal's text ("" = planned).  Returns 0, -1 where refused.
int sim_cmp_plan(uint64_t na, uint64_t nb, uint32_t rate_a, uint32_t rate_b, uint32_t ch_a, uint32_t ch_b, uint32_t depth_a, uint32_t depth_b, uint32_t ia,
                 uint32_t ib, uint32_t nsrc, int64_t centre, uint32_t radius, int64_t* out, char* why, uint32_t why_cap) {
    std::vector<CmpFmt> fmt(2);
    fmt[0] = CmpFmt{na, rate_a, (uint8_t)ch_a, (uint8_t)depth_a}, fmt[1] = CmpFmt{nb, rate_b, (uint8_t)ch_b, (uint8_t)depth_b};
    lacx_compare_pair p{};
    p.a = ia, p.b = ib, p.centre = centre, p.radius = radius;
    std::vector<CmpFmt> all(nsrc > 2 ? nsrc : 2, fmt[0]);
    if (ia < all.size()) all[ia] = fmt[0];
    if (ib < all.size() && ib != ia) all[ib] = fmt[1];
    const std::string text = cmp_pair_why(p, all.data(), nsrc);
    if (text.size() + 1 > why_cap) return -2;
    std::memcpy(why, text.c_str(), text.size() + 1);
    if (!text.empty()) return -1;
    const CmpSrcIn in[2] = {{nullptr, nullptr, na, 0, 0, (uint8_t)ch_a, (uint8_t)depth_a, false}, {nullptr, nullptr, nb, 0, 1, (uint8_t)ch_b, (uint8_t)depth_b, false}};
    const CmpPairIn q{0, 1, centre, radius};
    if (cmp_check(in, &q, 1)) return -3;
    const CmpLayout y = cmp_layout(0, in, 2, &q, 1);
    out[0] = (int64_t)y.total_tiles, out[1] = (int64_t)y.span.size(), out[2] = y.span.empty() ? 0 : y.span[0].lanes, out[3] = y.span.empty() ? 0 : y.span[0].otiles;
    out[4] = (int64_t)y.rows_cap, out[5] = (int64_t)y.total_counts, out[6] = (int64_t)y.size;
    const uint32_t lanes = cmp_lanes(centre, radius);
    const uint64_t otiles = (cmp_slots(centre, radius) + 4u * lanes - 1u) / (4u * lanes);
    out[7] = radius == 0 || ((na + nb + 2ull * radius + 8u) / kCmpTileFrames + 2u) * otiles >= y.total_tiles ? 1 : 0;
    for (size_t i = 0; i < y.span.size(); ++i) out[8 + 2 * i] = y.span[i].f_lo, out[9 + 2 * i] = y.span[i].f_hi;
    return 0;
}

uint32_t sim_cmp_tile_frames(void) { return kCmpTileFrames; }
uint32_t sim_cmp_row_frames(void) { return kCmpRowFrames; }
uint32_t sim_cmp_max_radius(void) { return kCmpMaxRadius; }

}  // extern "C"

#ifdef SIM_COMPARE_MAIN
// sim_compare_san CASES: every case of the file (per case: a 32-bit little-endian size, then the bytes), one line each
// (sim_cmp_line), "done <count>" at the end.
int main(int argc, char** argv) {
    if (argc != 2) return 2;
    std::vector<char> line(1 << 20);
    return for_each_case(argv[1], [&](const uint8_t* blob, uint32_t size, uint32_t i) {
        if (sim_cmp_line(blob, size, i, line.data(), (uint32_t)line.size())) return false;
        return std::puts(line.data()) >= 0;
    });
}
#endif
