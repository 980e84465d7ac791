// tests/native/sim_accuraterip.cpp -- TEST INFRASTRUCTURE: the rip-checksum job (csrc/accuraterip_core.h,
// csrc/accuraterip_plan.h) on the host, run the way k_accuraterip of k_accuraterip.hip runs it.
//
// Stream jobs: what lacx_decoder_accuraterip_batch_device runs on the device, one lane after the other -- the job planned by
// plan_decode(..., digest form, the discs) and its tables filled by plan_fill_tables (csrc/decode_plan.h, the code
// api_decode.cpp runs), the lane code over the blocks, ms_inverse_tile as k_ms_inverse's grid runs it, then k_accuraterip:
// per tile the units staged in an array of exactly the kernel's LDS size (filled with a byte pattern: every word must be
// written before it is read), every lane's walk over its stripe of the multipliers, and the lanes' sums added into the
// job's sums.  The scratch PCM starts as a byte pattern too: a sample a lane must not read would change a sum.  Source
// jobs: sources of given PCM in a layout, in allocations that END exactly at the source's last byte behind a base at the
// byte offset the case asks for; optionally one element replaced by a raw 32-bit word (an invalid sample).
// A case (little-endian, written by tests/artwin.py): u8 form (0 streams, 1 sources), u32 discs, then per disc u32 sources,
// u32 tracks (0: one per source), u32 flags, u32 radius, u32 lba0, u64 track_frames[tracks], then per source -- streams: u64
// size and the bytes; sources: u32 layout, u32 offset, u64 frames, u64 bad_frame, u32 bad_channel, u32 bad_word, i32
// left[frames], i32 right[frames].
// It is not part of the product and is not a fallback.
//
// Built twice by tests/artwin.py: a plain -O2 shared library for ctypes, and (-DSIM_ACCURATERIP_MAIN) a sanitized program
// that runs a file of cases and prints one line per case.
#define SIM_JOB_SIMULATOR
#include "sim_job.h"

#include "accuraterip_core.h"
#include "import_msg.h"

using namespace lacx;
using namespace simjob;

namespace {

constexpr int kFill = 0xCD;

// launch_accuraterip: every tile, every lane of each
void run_accuraterip(const ArArgs& a) {
    for (unsigned long long tile = 0; tile < a.total_tiles; ++tile) {
        uint32_t j = 0;
        while (j + 1 < a.nspans && a.tile_off[j + 1] <= tile) ++j;
        const ArSpan sp = a.spans[j];
        const ArTile y = ar_tile(sp, tile - a.tile_off[j]);
        Heap<uint32_t> stage(kArStageWords, kFill);
        for (uint32_t u = 0; u < y.units; ++u)
            ar_load_unit(sp, a.sources, y.first + 4ll * (long long)u, stage.p + 4u * u, [&](uint32_t item, unsigned long long key) {
                if (key < a.bad[item]) a.bad[item] = key;
            });
        for (uint32_t tid = 0; tid < kArThreads; ++tid) {
            uint32_t lo, hi;
            ar_lane(stage.p, sp, y, tid, lo, hi);
            const uint32_t o = y.o0 + (tid & (sp.lanes - 1u));
            if (o >= ar_width(sp)) continue;
            a.sums[sp.sum0 + o] += lo;  // the atomics: wrapping adds into the zeroed sums
            if (sp.keep_hi) a.sums[sp.sum0 + ar_width(sp) + o] += lo + hi;
        }
    }
}

struct DiscOut {
    int code = 0;  // 0: it has sums; else the ABI's code (a decode failure: LACX_E_RUNTIME)
    std::string text;
    lacx_ar_result result{};
    std::vector<lacx_ar_track> tracks;
    std::vector<uint32_t> sums;  // [track][3][width]
};

struct SourceCase {
    uint32_t layout, offset;
    uint64_t frames, bad_frame;
    uint32_t bad_channel, bad_word;
    const uint8_t* samples;  // i32 left[frames], right[frames], unaligned
};
struct DiscCase {
    uint32_t nsrc, ntracks, flags, radius, lba0;
    std::vector<uint64_t> tracks;
    std::vector<std::pair<const uint8_t*, uint64_t>> lacs;
    std::vector<SourceCase> srcs;
};

bool read_case(const uint8_t* blob, uint64_t size, uint8_t& form, std::vector<DiscCase>& discs) {
    Reader rd{blob, blob + size};
    form = rd.get<uint8_t>();
    const uint32_t n = rd.get<uint32_t>();
    if (!rd.ok || form > 1 || n > (1u << 20)) return false;
    discs.resize(n);
    for (DiscCase& d : discs) {
        d.nsrc = rd.get<uint32_t>(), d.ntracks = rd.get<uint32_t>(), d.flags = rd.get<uint32_t>(), d.radius = rd.get<uint32_t>(), d.lba0 = rd.get<uint32_t>();
        if (!rd.ok) return false;
        d.tracks = rd.array<uint64_t>(d.ntracks);
        for (uint32_t i = 0; rd.ok && i < d.nsrc; ++i) {
            if (form == 0) {
                const uint64_t bytes = rd.get<uint64_t>();
                if (!rd.ok || bytes > (uint64_t)(rd.end - rd.p)) return false;
                d.lacs.emplace_back(rd.p, bytes);
                rd.p += bytes;
            } else {
                SourceCase s{};
                s.layout = rd.get<uint32_t>(), s.offset = rd.get<uint32_t>(), s.frames = rd.get<uint64_t>(), s.bad_frame = rd.get<uint64_t>();
                s.bad_channel = rd.get<uint32_t>(), s.bad_word = rd.get<uint32_t>();
                if (!rd.ok || s.frames > (uint64_t)(rd.end - rd.p) / 8u) return false;
                s.samples = rd.p;
                rd.p += 8u * s.frames;
                d.srcs.push_back(s);
            }
        }
        if (!rd.ok) return false;
    }
    return rd.p == rd.end;
}

std::string not_cd(int channels, int depth, uint32_t rate) {
    return "not CD audio (" + std::to_string(channels) + " channels, " + std::to_string(depth) + " bit, " + std::to_string(rate) + " Hz)";
}

// the host's refusal of a disc whose sources are all good, as api_decode.cpp's ar_resolve makes it
bool accept(DiscCase& d, const std::vector<uint64_t>& frames, DiscOut& o) {
    if (d.nsrc == 0) return o.code = LACX_E_INVALID, o.text = "disc has no sources", false;
    uint64_t total = 0;
    for (uint64_t f : frames) total += f;
    if (d.ntracks == 0) d.tracks = frames;
    o.text = ar_disc_why(d.nsrc, total, d.tracks.data(), (uint32_t)d.tracks.size(), d.flags, d.radius);
    if (!o.text.empty()) o.code = LACX_E_INVALID;
    return o.code == 0;
}

void take(const ArLayout& y, size_t slot, const uint32_t* sums, const DiscCase& d, DiscOut& o) {
    const ArDiscAt& at = y.discs[slot];
    o.result = ar_result(y, slot, d.lba0, d.tracks.data());
    ar_tracks(y, slot, sums, o.tracks);
    o.sums.assign(sums + at.sum0, sums + at.sum0 + 3ull * (2ull * at.radius + 1u) * at.ntracks);
}

bool run_stream_case(std::vector<DiscCase>& discs, std::vector<DiscOut>& out) {
    std::vector<std::unique_ptr<Heap<uint8_t>>> own;  // every stream an exact allocation of its own
    std::vector<BatchIn> in;
    std::vector<ArDiscIn> adiscs;
    std::vector<uint32_t> which;
    for (size_t k = 0; k < discs.size(); ++k) {
        DiscCase& d = discs[k];
        std::vector<uint64_t> frames;
        for (uint32_t i = 0; i < d.nsrc && out[k].code == 0; ++i) {
            lacx_stream_info f{};
            const char* why = nullptr;
            const int c = parse_stream(d.lacs[i].first, d.lacs[i].second, &f, &why);
            if (c != LACX_OK) out[k].code = c, out[k].text = "source " + std::to_string(i) + ": " + (why ? why : "");
            else if (f.channels != 2 || f.bit_depth != 16 || f.sample_rate != 44100)
                out[k].code = LACX_E_INVALID, out[k].text = "source " + std::to_string(i) + ": " + not_cd(f.channels, f.bit_depth, f.sample_rate);
            frames.push_back(f.frames);
        }
        if (out[k].code || !accept(d, frames, out[k])) continue;
        adiscs.push_back(ArDiscIn{(uint32_t)in.size(), d.nsrc, d.tracks.data(), (uint32_t)d.tracks.size(), d.flags, d.radius, false});
        which.push_back((uint32_t)k);
        for (const auto& l : d.lacs) {
            own.emplace_back(new Heap<uint8_t>(l.second));
            std::memcpy(own.back()->p, l.first, l.second);
            in.push_back(BatchIn{own.back()->p, l.second, nullptr, nullptr, 0});
        }
    }
    if (adiscs.empty()) return true;
    const ArJobIn job{adiscs.data(), (uint32_t)adiscs.size()};
    DecodePlan plan;
    std::vector<int> code;
    std::vector<std::string> err;
    if (plan_decode(in.data(), (uint32_t)in.size(), DecodeForm::digest, kWholeStreams, false, plan, code, err, false, false, false, false, kRunsListCap, false, false, 0, &job))
        return false;
    if (plan.ar_at.size != plan.need.tables) return false;
    Run run(plan, in.data(), (uint32_t)kDecodeTailPad, kFill, kFill);
    place_payload(plan, in.data(), run.payload.p);
    if (plan.items.empty()) return false;
    if (run.a.digest || run.a.present || run.a.verify || run.a.window || run.a.wav) return false;  // launch_decode must end with k_ms_inverse in place
    Lane ln(1, 0);
    run_lanes(run.a, ln);
    run_ms_inverse(run.a);
    run_accuraterip(plan_ar_args(plan, run.tables.p));
    const auto* sums = reinterpret_cast<const uint32_t*>(run.tables.p + plan.ar_at.sums);
    std::vector<uint32_t> status(in.size(), 0);  // per input its first failing block's status
    for (const PlanItem& p : plan.items)
        for (uint32_t b = 0; b < p.item.blocks && !status[p.src]; ++b) status[p.src] = run.st.p[p.item.block0 + b];
    for (size_t a = 0; a < adiscs.size(); ++a) {
        DiscOut& o = out[which[a]];
        for (uint32_t i = 0; i < adiscs[a].nsrc && o.code == 0; ++i) {
            const uint32_t at = adiscs[a].src0 + i;
            if (code[at] != LACX_OK) o.code = code[at], o.text = "source " + std::to_string(i) + ": " + err[at];
            else if (status[at]) o.code = LACX_E_RUNTIME, o.text = "source " + std::to_string(i) + ": status " + std::to_string(status[at]);
        }
        if (o.code) continue;
        size_t slot = 0;
        while (slot < plan.ar_disc.size() && plan.ar_disc[slot] != a) ++slot;
        if (slot == plan.ar_disc.size()) return false;
        take(plan.ar_at, slot, sums, discs[which[a]], o);
    }
    return true;
}

bool run_source_case(std::vector<DiscCase>& discs, std::vector<DiscOut>& out) {
    std::vector<std::unique_ptr<Exact>> own;
    std::vector<ArSrcIn> in;
    std::vector<ArDiscIn> adiscs;
    std::vector<uint32_t> which;
    for (size_t k = 0; k < discs.size(); ++k) {
        DiscCase& d = discs[k];
        std::vector<uint64_t> frames;
        for (const SourceCase& s : d.srcs) frames.push_back(s.frames);
        for (uint32_t i = 0; i < d.nsrc && out[k].code == 0; ++i)
            if (frames[i] == 0) out[k].code = LACX_E_INVALID, out[k].text = "source " + std::to_string(i) + ": source has no frames";
        if (out[k].code || !accept(d, frames, out[k])) continue;
        adiscs.push_back(ArDiscIn{(uint32_t)in.size(), d.nsrc, d.tracks.data(), (uint32_t)d.tracks.size(), d.flags, d.radius, true});
        which.push_back((uint32_t)k);
        for (const SourceCase& s : d.srcs) {
            const uint32_t eb = elem_bytes(s.layout);
            const bool pl = planar(s.layout), f32 = s.layout == (uint32_t)PCM_PLANAR_F32 || s.layout == (uint32_t)PCM_INTERLEAVED_F32;
            const uint64_t bytes0 = pl ? s.frames * eb : s.frames * 2u * eb;
            own.emplace_back(new Exact(bytes0, s.offset % 16u));
            uint8_t* s0 = own.back()->data;
            uint8_t* s1 = nullptr;
            if (pl) {
                own.emplace_back(new Exact(bytes0, s.offset % 16u));
                s1 = own.back()->data;
            }
            for (uint64_t f = 0; f < s.frames; ++f)
                for (uint32_t c = 0; c < 2u; ++c) {
                    int32_t v;
                    std::memcpy(&v, s.samples + 4u * (c * s.frames + f), 4);
                    if (f32) {
                        const float x = (float)v / 32768.0f;
                        std::memcpy(&v, &x, 4);
                    }
                    if (f == s.bad_frame && c == s.bad_channel && eb == 4u) v = (int32_t)s.bad_word;
                    put_elem(s0, s1, s.layout, 2, f, c, v);
                }
            in.push_back(ArSrcIn{s0, s1, s.frames, s.layout, (uint32_t)in.size()});
        }
    }
    if (adiscs.empty()) return true;
    if (ar_check(in.data(), adiscs.data(), adiscs.size())) return false;
    const ArLayout y = ar_layout(0, in.data(), adiscs.data(), adiscs.size());
    Heap<uint8_t> tables(y.size, kFill);
    std::vector<unsigned long long> bad(in.size(), kDigestClean);
    ar_fill(y, in.data(), adiscs.data(), adiscs.size(), tables.p);
    run_accuraterip(ar_args(y, tables.p, bad.data()));
    const auto* sums = reinterpret_cast<const uint32_t*>(tables.p + y.sums);
    for (size_t a = 0; a < adiscs.size(); ++a) {
        DiscOut& o = out[which[a]];
        for (uint32_t i = 0; i < adiscs[a].nsrc && o.code == 0; ++i) {
            const unsigned long long key = bad[adiscs[a].src0 + i];
            if (key == kDigestClean) continue;
            ImportBad b{{kImportClean, kImportClean}};  // as api_decode.cpp words it
            b.key[key >> 63] = key & ~(1ull << 63);
            int ch = 0;
            unsigned long long index = 0;
            std::string text;
            (void)import_bad_message(b, 16, &ch, &index, text);
            o.code = LACX_E_INVALID, o.text = "source " + std::to_string(i) + ": " + text;
        }
        if (!o.code) take(y, a, sums, discs[which[a]], o);
    }
    return true;
}

bool run_case(const uint8_t* blob, uint64_t size, std::vector<DiscOut>& out) {
    uint8_t form = 0;
    std::vector<DiscCase> discs;
    if (!read_case(blob, size, form, discs)) return false;
    out.assign(discs.size(), DiscOut{});
    return form == 0 ? run_stream_case(discs, out) : run_source_case(discs, out);
}

std::string hex(uint64_t h) {
    char s[24];
    std::snprintf(s, sizeof(s), "%016llx", (unsigned long long)h);
    return s;
}

}  // namespace

extern "C" {

// A case as one job.  Per disc k: rec[4 k] = its code (0: it has sums), rec[4 k + 1] = its tracks, rec[4 k + 2] = its first
// word in sums, rec[4 k + 3] = its first record in tracks; results: lacx_ar_result[discs]; sums: per disc with sums
// [track][v1 | v2 | s450][2 radius + 1]; msg: the discs' texts, '\n' between them.  Returns the words written to sums, -1
// where the case cannot be read or run or a capacity is too small.
int64_t sim_ar_run(const uint8_t* blob, uint64_t size, uint64_t* rec, lacx_ar_result* results, uint32_t* sums, uint64_t sums_cap, lacx_ar_track* tracks,
                   uint64_t tracks_cap, char* msg, uint32_t msg_cap) {
    std::vector<DiscOut> out;
    if (!run_case(blob, size, out)) return -1;
    std::string all;
    uint64_t at = 0, tr = 0;
    for (size_t k = 0; k < out.size(); ++k) {
        const DiscOut& o = out[k];
        if (at + o.sums.size() > sums_cap || tr + o.tracks.size() > tracks_cap) return -1;
        rec[4 * k] = (uint64_t)o.code, rec[4 * k + 1] = o.tracks.size(), rec[4 * k + 2] = at, rec[4 * k + 3] = tr;
        results[k] = o.result;
        if (!o.sums.empty()) std::memcpy(sums + at, o.sums.data(), 4 * o.sums.size());
        if (!o.tracks.empty()) std::memcpy(tracks + tr, o.tracks.data(), sizeof(lacx_ar_track) * o.tracks.size());
        at += o.sums.size(), tr += o.tracks.size();
        all += (k ? "\n" : "") + o.text;
    }
    if (all.size() + 1 > msg_cap) return -1;
    std::memcpy(msg, all.c_str(), all.size() + 1);
    return (int64_t)at;
}

// One line for a case: "<index> <disc>;<disc>;..." with disc = "!<code> <text>" or "<tracks> <hash of the sums> <hash of the
// tracks> <hash of the result>".
int sim_ar_line(const uint8_t* blob, uint64_t size, uint32_t index, char* line, uint32_t cap) {
    std::vector<DiscOut> out;
    if (!run_case(blob, size, out)) return -1;
    std::string s = std::to_string(index) + " ";
    for (size_t k = 0; k < out.size(); ++k) {
        const DiscOut& o = out[k];
        s += k ? ";" : "";
        if (o.code) s += "!" + std::to_string(o.code) + " " + o.text;
        else
            s += std::to_string(o.tracks.size()) + " " + hex(fnv(o.sums.data(), 4 * o.sums.size(), kFnvStart)) + " " +
                 hex(fnv(o.tracks.data(), sizeof(lacx_ar_track) * o.tracks.size(), kFnvStart)) + " " + hex(fnv(&o.result, sizeof(o.result), kFnvStart));
    }
    if (s.size() + 1 > cap) return -1;
    std::memcpy(line, s.c_str(), s.size() + 1);
    return 0;
}

// accuraterip_plan.h's ids through plain C (what lacx_ar_ids calls); returns 1 where the disc has ids
int sim_ar_ids(const uint64_t* track_frames, uint32_t ntracks, uint32_t flags, uint32_t lba0, lacx_ar_id* out) {
    return ar_ids(track_frames, ntracks, flags, lba0, *out) ? 1 : 0;
}

// the plan's split: offsets per tile at a radius, and the kernel's multiplier tile
uint32_t sim_ar_lanes(uint32_t radius) { return ar_lanes(radius); }
uint32_t sim_ar_tile_mults(void) { return kArTileMults; }

// the tiles the plan counts for one disc of one source (the capacity check's own count must not be below it); -1 where refused
int64_t sim_ar_tiles(const uint64_t* track_frames, uint32_t ntracks, uint32_t flags, uint32_t radius) {
    uint64_t total = 0;
    for (uint32_t t = 0; t < ntracks; ++t) total += track_frames[t];
    if (!ar_disc_why(1, total, track_frames, ntracks, flags, radius).empty()) return -1;
    const ArSrcIn in{nullptr, nullptr, total, 0, 0};
    const ArDiscIn d{0, 1, track_frames, ntracks, flags, radius, false};
    if (ar_check(&in, &d, 1)) return -1;
    return (int64_t)ar_layout(0, &in, &d, 1).total_tiles;
}

}  // extern "C"

#ifdef SIM_ACCURATERIP_MAIN
// sim_accuraterip_san CASES: every case of the file (per case: a 32-bit little-endian size, then the bytes), one line each
// (sim_ar_line), "done <count>" at the end.
int main(int argc, char** argv) {
    if (argc != 2) return 2;
    std::vector<char> line(1 << 20);
    return for_each_case(argv[1], [&](const uint8_t* blob, uint32_t size, uint32_t i) {
        if (sim_ar_line(blob, size, i, line.data(), (uint32_t)line.size())) return false;
        return std::puts(line.data()) >= 0;
    });
}
#endif
