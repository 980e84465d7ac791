// tests/native/sim_blockdigest.cpp -- TEST INFRASTRUCTURE: the block digests (csrc/blockdigest_core.h, csrc/manifest.h) on
// the host, summed the way k_digest_blocks sums them.
//
// Stream jobs: what lacx_decoder_digest_blocks_batch_device / lacx_decoder_check_batch_device / the *_checked salvage
// forms run on the device, one lane and one thread after the other -- the job planned by plan_decode(..., salvage,
// blocks) and its tables filled by plan_fill_tables (csrc/decode_plan.h, the code api_decode.cpp runs), the lane code over
// the present blocks, ms_inverse_tile as k_ms_inverse's grid runs it, then the units as the workgroups and waves of
// k_digest_blocks take them: a wave of 64 full units of one block through the six-level lane tree and the five-level
// factor tree, its value left for the workgroup's first thread, which adds up consecutive waves of one block; every other
// unit shifted by itself, a straddling unit as two pieces.  Then judge_block per global block and the salvage pass.
// Every buffer is a heap allocation of exactly the capacity the plan states, so that a build with AddressSanitizer
// reports any access outside them.
// Source jobs: one item of generated PCM in a layout, in allocations that END exactly at the source's last byte behind a
// base at the byte offset the case asks for, on a grid.
// It is not part of the product and is not a fallback.
//
// Built twice by tests/blockdigesttwin.py: a plain -O2 shared library for ctypes, and (-DSIM_BLOCKDIGEST_MAIN) a
// sanitized program that runs a file of cases and prints one line per case.
#define SIM_JOB_SIMULATOR
#include "sim_job.h"

#include "blockdigest_core.h"

using namespace lacx;
using namespace simjob;

namespace {

constexpr int kFill = 0xCD;

struct UnitLane {
    bool valid = false;
    uint32_t j = 0, align = 0, fmt = 0, g0 = 0;
    BlockUnit bu{};
};

// k_digest_blocks: workgroups of kDigestThreads units, waves of 64.  unit(j, f0, lane) is the kernel's per-item branch.
// atomics: the atomicXor calls issued.  Returns false where the lanes of a fast wave disagree on its value.
template <typename Unit>
bool sum_like_kernel(uint32_t nitems, unsigned long long total_units, const unsigned long long* unit_off, Unit unit, uint32_t* raw,
                     uint64_t* atomics) {
    for (unsigned long long first = 0; first < total_units; first += kDigestThreads) {
        uint32_t lo = 0;
        while (lo + 1 < nitems && unit_off[lo + 1] <= first) ++lo;
        const bool one_item = unit_off[lo + 1] >= first + kDigestThreads;
        uint32_t wave_sum[kDigestThreads / 64u], wave_blk[kDigestThreads / 64u];
        for (uint32_t w = 0; w < kDigestThreads / 64u; ++w) {
            UnitLane ln[64];
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
            for (uint32_t lane = 0; lane < 64u; ++lane)
                fast = fast && ln[lane].valid && ln[lane].bu.p0.bytes == kDigestUnitFrames * ln[lane].align && ln[lane].g0 == ln[0].g0;
            uint32_t wave_value = 0;
            if (fast) {
                if (ln[0].bu.use0) {
                    const uint32_t* tree = kCrcTables.tree[ln[0].fmt];
                    uint32_t v[64], factor[64], nv[64];
                    for (uint32_t lane = 0; lane < 64u; ++lane) v[lane] = ln[lane].bu.p0.raw;
                    for (uint32_t level = 0; level < 6u; ++level) {
                        for (uint32_t lane = 0; lane < 64u; ++lane) {
                            const uint32_t other = v[lane ^ (1u << level)];
                            const bool upper = ((lane >> level) & 1u) != 0u;
                            nv[lane] = crc_mul(upper ? other : v[lane], tree[level]) ^ (upper ? v[lane] : other);
                        }
                        std::memcpy(v, nv, sizeof(v));
                    }
                    for (uint32_t lane = 0; lane < 64u; ++lane) {
                        const unsigned long long dist = ln[lane].bu.dist0 - (unsigned long long)(kDigestUnitFrames * ln[lane].align) * (63u - lane);
                        const uint32_t d = crc_reduce(dist);
                        factor[lane] = ((d >> (lane & 31u)) & 1u) != 0u ? kCrcTables.pow8[lane & 31u] : kCrcOne;
                    }
                    for (uint32_t level = 0; level < 5u; ++level) {
                        for (uint32_t lane = 0; lane < 64u; ++lane) nv[lane] = crc_mul(factor[lane], factor[lane ^ (1u << level)]);
                        std::memcpy(factor, nv, sizeof(factor));
                    }
                    wave_value = crc_mul(v[0], factor[0]);
                    for (uint32_t lane = 1; lane < 64u; ++lane)
                        if (crc_mul(v[lane], factor[lane]) != wave_value) return false;
                }
            } else {
                for (uint32_t lane = 0; lane < 64u; ++lane) {
                    const UnitLane& t = ln[lane];
                    if (!t.valid) continue;
                    if (t.bu.use0 && t.bu.p0.bytes) raw[t.g0] ^= crc_shift(t.bu.p0.raw, t.bu.dist0), ++*atomics;
                    if (t.bu.use1 && t.bu.p1.bytes) raw[t.g0 + 1u] ^= crc_shift(t.bu.p1.raw, t.bu.dist1), ++*atomics;
                }
            }
            const bool has = fast && ln[0].bu.use0;
            wave_sum[w] = has ? wave_value : 0u;
            wave_blk[w] = has ? ln[0].g0 : ~0u;
        }
        uint32_t acc = 0, blk = ~0u;
        for (uint32_t w = 0; w < kDigestThreads / 64u; ++w) {
            if (wave_blk[w] != blk) {
                if (blk != ~0u && acc) raw[blk] ^= acc, ++*atomics;
                acc = 0;
                blk = wave_blk[w];
            }
            acc ^= wave_sum[w];
        }
        if (blk != ~0u && acc) raw[blk] ^= acc, ++*atomics;
    }
    return true;
}

struct Job {
    SalvageIn src;
    DecodePlan plan;
    std::vector<int> code;
    std::vector<std::string> err;
    std::unique_ptr<Run> run;
    uint64_t atomics = 0;
    Job(const uint8_t* const* lacs, const uint64_t* sizes, uint32_t n, int form) : src(lacs, sizes, n, form == 2) {}
};

// form: 0 the blocks form, 1 the WAV form, 2 the device form.  mans[i] null: no manifest for item i.
bool run(const uint8_t* const* mans, const uint64_t* man_sizes, uint32_t n, int form, int cols, bool zero_status, Job& j) {
    for (uint32_t i = 0; i < n; ++i)
        if (mans && mans[i]) j.src.in[i].manifest = mans[i], j.src.in[i].manifest_size = man_sizes[i];
    const BatchIn* in = j.src.in.data();
    const DecodeForm f = form == 0 ? DecodeForm::blocks : form == 1 ? DecodeForm::wav : DecodeForm::device;
    if (plan_decode(in, n, f, kWholeStreams, false, j.plan, j.code, j.err, true, true)) return false;
    j.run.reset(new Run(j.plan, in, (uint32_t)kDecodeTailPad, kFill, zero_status ? 0 : kFill));
    const DecodeArgs& a = j.run->a;
    place_payload(j.plan, in, j.run->payload.p);
    if (j.plan.items.empty()) return true;
    if (!a.present || !a.block_raw) return false;
    Lane ln(cols, 0);
    run_lanes(a, ln);
    run_ms_inverse(a);
    // k_digest_blocks
    const bool agreed = sum_like_kernel(a.nitems, a.total_units, a.unit_off, [&](uint32_t item, unsigned long long f0, UnitLane& t) {
        const DecodeItem& it = a.items[item];
        t.align = (uint32_t)it.channels * (it.bit_depth / 8u);
        t.fmt = crc_format(it.channels, it.bit_depth);
        t.bu = block_unit_decoded(f0, it.blocks, a.present[item], it.channels, it.bit_depth, it.frames, a.frame_off + it.block0, it.frame0,
                                  it.left, it.right, a.status + it.block0);
        t.g0 = it.block0 + t.bu.b0;
    }, a.block_raw, &j.atomics);
    if (!agreed) return false;
    if (a.block_expect) {  // k_digest_judge
        for (uint32_t g = 0; g < a.total_blocks; ++g) {
            const uint32_t item = a.blk_item[g];
            const DecodeItem& it = a.items[item];
            judge_block(g, g - it.block0, a.present[item], a.judged[item] != 0u, (uint32_t)(a.frame_off[g + 1] - a.frame_off[g]),
                        (uint32_t)it.channels * (it.bit_depth / 8u), a.block_raw, a.block_expect, a.status);
        }
    }
    if (!a.no_output) run_salvage_pass(a);
    return true;
}

// the rows of a planned item, made by the code the host side makes them with (manifest.h, called by collect of api_decode.cpp)
std::vector<lacx_block_digest> rows_of(const Job& j, const PlanItem& p, const std::vector<lacx_block_fault>& faults) {
    std::vector<lacx_block_digest> rows;
    rows_of_decoded(j.src.in[p.src].lac, p.info.version, p.item.blocks, p.info.channels, p.info.bit_depth, faults, j.run->a.block_raw + p.item.block0, rows);
    return rows;
}

// "<frames:crc:code,...>" of the digest lines
std::string rows_text(const std::vector<lacx_block_digest>& rows) {
    std::string s;
    for (size_t b = 0; b < rows.size(); ++b)
        s += (b ? "," : "") + std::to_string(rows[b].frames) + ":" + std::to_string(rows[b].crc32) + ":" + std::to_string(rows[b].code);
    return s;
}

}  // namespace

extern "C" {

// n streams as one job with block digests (form: 0 blocks, 1 WAV, 2 device); mans[i] null or item i's manifest.
// Per input i, rec[8 * i ..] = the plan's code for it (0: it went to the device; then) blocks, bad_blocks, frames,
// lost_frames, first_bad, flags, and `at` as sim_salvage states it.  rows: per accepted item in input order three words
// per block -- frames, crc32, code.  msg: the refused items' messages, '\n' between inputs.  *atomics: the atomicXor
// calls k_digest_blocks would issue.  Returns need.image (WAV form), the frames written (device form) or 0, -1 where the
// job cannot be planned, an output is too small or the lanes of a wave disagree.
int64_t sim_blockdigest(const uint8_t* const* lacs, const uint64_t* sizes, const uint8_t* const* mans, const uint64_t* man_sizes, uint32_t n,
                        int form, int cols, int zero_status, uint64_t* rec, uint32_t* rows, uint64_t rows_cap, uint8_t* image,
                        uint64_t image_cap, int32_t* left, int32_t* right, uint64_t pcm_cap, char* msg, uint32_t msg_cap, uint64_t* atomics) {
    if ((cols != 1 && cols != 64) || form < 0 || form > 2) return -1;
    Job j(lacs, sizes, n, form);
    if (!run(mans, man_sizes, n, form, cols, zero_status != 0, j)) return -1;
    std::string all;
    for (uint32_t i = 0; i < n; ++i) {
        rec[8 * i] = (uint64_t)j.code[i];
        all += (i ? "\n" : "") + j.err[i];
    }
    std::snprintf(msg, msg_cap, "%s", all.c_str());
    uint64_t nrows = 0, written = 0;
    bool fits = true;
    salvage_records(j.plan, j.src.in.data(), j.run->st.p, form == 2,
                    [&](const PlanItem& p, const lacx_salvage_result& r, const std::vector<lacx_block_fault>& faults, const uint64_t* q) {
        if (nrows + r.blocks > rows_cap || (form == 2 && q[6] + r.frames > pcm_cap)) return fits = false;
        const std::vector<lacx_block_digest> got = rows_of(j, p, faults);
        for (uint32_t b = 0; b < r.blocks; ++b, ++nrows) rows[3 * nrows] = got[b].frames, rows[3 * nrows + 1] = got[b].crc32, rows[3 * nrows + 2] = got[b].code;
        std::memcpy(rec + 8 * p.src + 1, q, 7 * sizeof(uint64_t));
        if (form == 2) {
            std::memcpy(left + q[6], j.src.in[p.src].left, 4 * r.frames);
            if (j.src.in[p.src].right) std::memcpy(right + q[6], j.src.in[p.src].right, 4 * r.frames);
            written = q[6] + r.frames;
        }
        return true;
    });
    if (!fits) return -1;
    *atomics = j.atomics;
    if (form == 2) return (int64_t)written;
    if (form == 0) return 0;
    if (j.plan.need.image > image_cap) return -1;
    std::memcpy(image, j.run->image.p, j.plan.need.image);
    return (int64_t)j.plan.need.image;
}

// A stream case (little-endian, written by tests/blockdigesttwin.py): u32 n, u32 flags (bits 0-1 the form, 4: 64 columns,
// 8: zero_status), then per stream u64 size, the bytes, u64 manifest size (all ones: none) and its bytes.  One line:
// "<index> <item>;<item>;..." with item = "!<code>" (refused by the plan) or "<hash of what the caller gets> <flags>
// <frames:crc:code,...>".
int sim_blockdigest_line(const uint8_t* blob, uint64_t size, uint32_t index, char* line, uint32_t cap) {
    if (size < 8) return -1;
    uint32_t n, flags;
    std::memcpy(&n, blob, 4), std::memcpy(&flags, blob + 4, 4);
    std::vector<std::unique_ptr<Heap<uint8_t>>> own;  // every stream and manifest an exact allocation of its own
    std::vector<const uint8_t*> lacs(n), mans(n);
    std::vector<uint64_t> sizes(n), msizes(n);
    uint64_t at = 8;
    auto take = [&](uint64_t len) -> const uint8_t* {
        if (size - at < len) return nullptr;
        own.emplace_back(new Heap<uint8_t>(len));
        std::memcpy(own.back()->p, blob + at, len);
        at += len;
        return own.back()->p;
    };
    for (uint32_t i = 0; i < n; ++i) {
        if (size - at < 8) return -1;
        std::memcpy(&sizes[i], blob + at, 8);
        at += 8;
        if (!(lacs[i] = take(sizes[i]))) return -1;
        if (size - at < 8) return -1;
        std::memcpy(&msizes[i], blob + at, 8);
        at += 8;
        mans[i] = nullptr;
        if (msizes[i] != ~0ull && !(mans[i] = take(msizes[i]))) return -1;
    }
    const int form = (int)(flags & 3u);
    if (form > 2) return -1;
    Job j(lacs.data(), sizes.data(), n, form);
    if (!run(mans.data(), msizes.data(), n, form, (flags & 4u) ? 64 : 1, (flags & 8u) != 0, j)) return -1;
    std::vector<std::string> item(n);
    for (uint32_t i = 0; i < n; ++i) item[i] = "!" + std::to_string(j.code[i]);
    salvage_records(j.plan, j.src.in.data(), j.run->st.p, form == 2,
                    [&](const PlanItem& p, const lacx_salvage_result& r, const std::vector<lacx_block_fault>& faults, const uint64_t*) {
        const uint64_t h = form == 0 ? kFnvStart : salvage_hash(p, j.src.in[p.src], j.run->image.p, form == 2, r.frames);
        char hex[24];
        std::snprintf(hex, sizeof(hex), "%016llx", (unsigned long long)h);
        item[p.src] = std::string(hex) + " " + std::to_string(r.flags) + " " + rows_text(rows_of(j, p, faults));
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
// digested on a grid of `grid` frames as k_digest_blocks<true> does.  rows: three words per block (frames, crc32, 0).
// *key: the lowest invalid sample's key (all ones: none).  Returns the blocks, -1 where rows_cap is too small or the
// lanes of a wave disagree.
int64_t sim_blockdigest_source(uint32_t layout, uint32_t channels, uint32_t bit_depth, uint64_t frames, uint32_t grid, uint32_t offset,
                               const int32_t* samples, uint32_t* rows, uint64_t rows_cap, uint64_t* key, uint64_t* atomics) {
    const uint32_t eb = elem_bytes(layout);
    const bool pl = planar(layout), f32 = layout == (uint32_t)PCM_PLANAR_F32 || layout == (uint32_t)PCM_INTERLEAVED_F32;
    const uint64_t bytes0 = pl ? frames * eb : frames * channels * eb;
    // exact allocations: malloc returns 16-byte aligned memory; we need base % 16 == offset and end == allocation end
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
            put_elem(s0, s1, layout, channels, f, c, v);
        }
    const uint64_t nb = (frames + grid - 1) / grid;
    if (nb > rows_cap) return -1;
    std::vector<uint32_t> raw(nb, 0);
    const unsigned long long unit_off[2] = {0, (frames + 3u) / 4u};
    unsigned long long bad = kDigestClean;
    *atomics = 0;
    const bool agreed = sum_like_kernel(1, unit_off[1], unit_off, [&](uint32_t, unsigned long long f0, UnitLane& t) {
        unsigned long long k = kDigestClean;
        t.align = channels * (bit_depth / 8u);
        t.fmt = crc_format((int)channels, (int)bit_depth);
        t.bu = block_unit_source(f0, grid, (int)channels, (int)bit_depth, frames, s0, s1, layout, k);
        if (k < bad) bad = k;
        t.g0 = t.bu.b0;
    }, raw.data(), atomics);
    if (!agreed) return -1;
    *key = bad;
    std::vector<lacx_block_digest> got;
    rows_of_source(frames, grid, (uint32_t)nb, channels, bit_depth, raw.data(), got);  // as digest_pcm_run of api_decode.cpp does
    for (uint64_t b = 0; b < nb; ++b) rows[3 * b] = got[b].frames, rows[3 * b + 1] = got[b].crc32, rows[3 * b + 2] = got[b].code;
    return (int64_t)nb;
}

// manifest.h through plain C: build (rows: three words per block; returns the size or -1, why in msg) and parse (returns
// the code; info[6] = channels, bit depth, sample rate, frames, blocks, data_crc32; rows as above)
int64_t sim_manifest_build(uint32_t channels, uint32_t bit_depth, uint32_t rate, uint64_t frames, uint32_t data_crc32, const uint32_t* rows,
                           uint32_t count, uint8_t* out, uint64_t cap, char* msg, uint32_t msg_cap) {
    lacx_digest d{};
    d.channels = (uint8_t)channels, d.bit_depth = (uint8_t)bit_depth, d.sample_rate = rate, d.frames = frames, d.data_crc32 = data_crc32;
    std::vector<lacx_block_digest> r(count);
    for (uint32_t b = 0; b < count; ++b) r[b] = lacx_block_digest{rows[3 * b], rows[3 * b + 1], rows[3 * b + 2], 0};
    std::vector<uint8_t> m;
    std::string why;
    if (manifest_build(d, r.data(), count, m, why) != LACX_OK || m.size() > cap) {
        std::snprintf(msg, msg_cap, "%s", why.c_str());
        return -1;
    }
    std::memcpy(out, m.data(), m.size());
    return (int64_t)m.size();
}

int sim_manifest_parse(const uint8_t* m, uint64_t size, uint64_t* info, uint32_t* rows, uint32_t rows_cap, char* msg, uint32_t msg_cap) {
    Heap<uint8_t> exact(size);  // the parser reads nothing behind the input
    if (size) std::memcpy(exact.p, m, size);
    lacx_manifest_info f{};
    std::vector<lacx_block_digest> r(rows_cap);
    std::string why;
    const int rc = manifest_parse(exact.p, size, &f, rows ? r.data() : nullptr, rows_cap, why);
    std::snprintf(msg, msg_cap, "%s", why.c_str());
    if (rc != LACX_OK) return rc;
    const uint64_t q[6] = {f.channels, f.bit_depth, f.sample_rate, f.frames, f.blocks, f.data_crc32};
    std::memcpy(info, q, sizeof(q));
    for (uint32_t b = 0; rows && b < f.blocks; ++b) rows[3 * b] = r[b].frames, rows[3 * b + 1] = r[b].crc32, rows[3 * b + 2] = r[b].code;
    return rc;
}

}  // extern "C"

#ifdef SIM_BLOCKDIGEST_MAIN
// sim_blockdigest_san CASES: every case of the file (per case: a 32-bit little-endian size, a type byte, then the bytes).
// Type 0: a stream case (sim_blockdigest_line).  Type 1: a source case -- u32 layout, channels, bit_depth, grid, offset,
// u64 frames, i32 samples[channels * frames] -- whose line is "<index> <key> <frames:crc:code,...>".  "done <count>" at
// the end.
int main(int argc, char** argv) {
    if (argc != 2) return 2;
    std::vector<char> line(1 << 22);
    return for_each_case(argv[1], [&](const uint8_t* blob, uint32_t size, uint32_t i) {
        if (size < 1) return false;
        if (blob[0] == 0) {
            if (sim_blockdigest_line(blob + 1, size - 1, i, line.data(), (uint32_t)line.size())) return false;
        } else {
            Reader rd{blob + 1, blob + size};
            const uint32_t layout = rd.get<uint32_t>(), channels = rd.get<uint32_t>(), depth = rd.get<uint32_t>(), grid = rd.get<uint32_t>();
            const uint32_t offset = rd.get<uint32_t>();
            const uint64_t frames = rd.get<uint64_t>();
            if (!rd.ok || (uint64_t)(rd.end - rd.p) != 4ull * channels * frames) return false;
            Heap<int32_t> samples(channels * frames);
            std::memcpy(samples.p, rd.p, 4ull * channels * frames);
            const uint64_t cap = frames / grid + 2;
            std::vector<uint32_t> rows(3 * cap);
            uint64_t key = 0, atomics = 0;
            const int64_t nb = sim_blockdigest_source(layout, channels, depth, frames, grid, offset, samples.p, rows.data(), cap, &key, &atomics);
            if (nb < 0) return false;
            std::string s = std::to_string(i) + " " + std::to_string(key) + " ";
            for (int64_t b = 0; b < nb; ++b)
                s += (b ? "," : "") + std::to_string(rows[3 * b]) + ":" + std::to_string(rows[3 * b + 1]) + ":" + std::to_string(rows[3 * b + 2]);
            std::snprintf(line.data(), line.size(), "%s", s.c_str());
        }
        return std::puts(line.data()) >= 0;
    });
}
#endif
