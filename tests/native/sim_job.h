// tests/native/sim_job.h -- TEST INFRASTRUCTURE: the device job of the decoder family on the host, once, and the small
// tools every twin under tests/native/ is written with.  It is not part of the product and is not a fallback.
//
// The tools: exact allocations (Heap, Exact: an access outside them is a heap overflow AddressSanitizer reports), the
// case reader (Reader), the chained hash of the digest lines (fnv), the PCM layouts (planar, elem_bytes, put_elem) and the
// loop every sanitized program's main walks its case file with (for_each_case).
//
// The simulator (for a twin that defines SIM_JOB_SIMULATOR ahead of this header): a job planned by plan_decode runs as the
// product launches it -- Run holds every buffer at exactly the plan's capacity and the tables plan_fill_tables fills,
// place_payload puts the items' payload where the plan says, run_lanes is k_decode / k_decode_serial one lane after the
// other, run_ms_inverse is k_ms_inverse's grid, run_salvage_pass is k_salvage_wav / k_salvage_blank, and salvage_records is
// the host side's report.  A change to how the product launches its passes is made here, for every twin.
#pragma once

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#ifdef SIM_JOB_SIMULATOR
#include "decode_core.h"
#include "decode_plan.h"
#include "salvage_core.h"
#endif

namespace simjob {

template <typename T>
struct Heap {  // exactly n elements, nothing behind them
    T* p;
    explicit Heap(size_t n, int fill = 0) : p(static_cast<T*>(std::malloc(n ? n * sizeof(T) : 1))) {
        if (n) std::memset(p, fill, n * sizeof(T));
    }
    ~Heap() { std::free(p); }
    Heap(const Heap&) = delete;
    Heap& operator=(const Heap&) = delete;
};

// `bytes` bytes whose first lies `offset` bytes behind a 16-byte aligned address (malloc's) and whose last is the last of
// the allocation
struct Exact {
    uint8_t* raw;
    uint8_t* data;
    Exact(uint64_t bytes, uint64_t offset) : raw(static_cast<uint8_t*>(std::malloc(offset + bytes ? offset + bytes : 1))), data(raw + offset) {}
    ~Exact() { std::free(raw); }
    Exact(const Exact&) = delete;
    Exact& operator=(const Exact&) = delete;
};

struct Reader {  // little-endian words and arrays off a case; ok turns false at the first that does not fit
    const uint8_t* p;
    const uint8_t* end;
    bool ok = true;
    template <typename T>
    T get() {
        T v{};
        if ((size_t)(end - p) < sizeof(T)) return ok = false, v;
        std::memcpy(&v, p, sizeof(T));
        p += sizeof(T);
        return v;
    }
    template <typename T>
    std::vector<T> array(uint64_t n) {
        std::vector<T> v;
        if (n > (uint64_t)(end - p) / sizeof(T)) return ok = false, v;
        v.resize(n);
        if (n) std::memcpy(v.data(), p, n * sizeof(T));
        p += n * sizeof(T);
        return v;
    }
};

constexpr uint64_t kFnvStart = 0xCBF29CE484222325ull;

// FNV-1a over bytes, chained through h (start with kFnvStart): how two builds' outputs are compared without moving them
inline uint64_t fnv(const void* data, uint64_t bytes, uint64_t h) {
    const uint8_t* p = static_cast<const uint8_t*>(data);
    for (uint64_t i = 0; i < bytes; ++i) {
        h ^= p[i];
        h *= 0x100000001B3ull;
    }
    return h;
}

// the lacx_pcm layouts by number (lacx_types.h's PcmLayout): 0 planar int32, 1 / 2 interleaved int16 / int24, 16 planar
// int16, 17 / 18 planar / interleaved float32
inline bool planar(uint32_t layout) { return layout == 0u || layout == 16u || layout == 17u; }
inline uint32_t elem_bytes(uint32_t layout) { return layout == 1u || layout == 16u ? 2u : layout == 2u ? 3u : 4u; }
// element (f, c) of a source in `layout`: the low elem_bytes of v, little-endian
inline void put_elem(uint8_t* src0, uint8_t* src1, uint32_t layout, uint32_t channels, uint64_t f, uint32_t c, int32_t v) {
    const uint32_t eb = elem_bytes(layout);
    uint8_t* p = planar(layout) ? (c ? src1 : src0) + eb * f : src0 + eb * (f * channels + c);
    for (uint32_t k = 0; k < eb; ++k) p[k] = (uint8_t)((uint32_t)v >> (8 * k));
}

// A case file: per case a 32-bit little-endian size, then the bytes.  fn(blob, size, index) -> false stops with code 4.
// Every case is an exact allocation of its own: the case reader is checked too.  Prints "done <count>" at the end.
// Returns the program's exit code: 2 no file, 3 a short case, 4 a case fn refuses, 0.
template <typename Fn>
int for_each_case(const char* path, Fn fn, unsigned long first = 0, unsigned long count = ~0ul) {
    FILE* f = std::fopen(path, "rb");
    if (!f) return 2;
    unsigned long done = 0;
    uint8_t sz[4];
    for (unsigned long i = 0; done < count && std::fread(sz, 1, 4, f) == 4; ++i) {
        const uint32_t size = sz[0] | (sz[1] << 8) | (sz[2] << 16) | ((uint32_t)sz[3] << 24);
        if (i < first) {
            std::fseek(f, (long)size, SEEK_CUR);
            continue;
        }
        Heap<uint8_t> blob(size);
        if (std::fread(blob.p, 1, size, f) != size) return 3;
        if (!fn(blob.p, size, (uint32_t)i)) return 4;
        ++done;
    }
    std::fclose(f);
    std::printf("done %lu\n", done);
    return 0;
}

// ---- the simulator ----
#ifdef SIM_JOB_SIMULATOR

using namespace lacx;

// The buffers of a run, each of exactly the plan's capacity, the tables filled with their addresses, and the kernels'
// arguments.  pad: the zero bytes behind the payload in place of kDecodeTailPad; fill: what flag, image and the scratch PCM
// start as; status_fill: what the status words start as.
struct Run {
    Heap<uint8_t> payload, tables, flag, image;
    Heap<int32_t> L, R;
    Heap<uint32_t> st;
    DecodeArgs a;
    Run(const DecodePlan& p, const BatchIn* in, uint32_t pad = (uint32_t)kDecodeTailPad, int fill = 0, int status_fill = 0)
        : payload(p.need.payload - kDecodeTailPad + pad), tables(p.need.tables), flag(p.need.blocks, fill), image(p.need.image, fill),
          L(p.need.pcm_frames, fill), R(p.need.pcm_frames, fill), st(p.need.blocks, status_fill) {
        plan_fill_tables(p, in, PlanBases{payload.p, L.p, R.p, image.p}, tables.p);
        a = plan_args(p, tables.p, payload.p, st.p, flag.p);
    }
};

struct Lane {  // one column of lane memory (the last of `cols`) and the wave policy
    Heap<unsigned char> raw;
    DecMem dm;
    int lane;
    DecWave wave;
    Lane(int cols, int never_lean) : raw(kDecBytesPerCol * (size_t)cols, 0xA5), dm(dec_mem(raw.p, (uint32_t)cols)), lane(cols - 1) {
        wave.never_lean = never_lean != 0;
    }
};

// every item's payload range where the plan puts it
inline void place_payload(const DecodePlan& plan, const BatchIn* in, uint8_t* payload) {
    for (const PlanItem& p : plan.items) std::memcpy(payload + p.item.pay_off, in[p.src].lac + p.head + p.pay_src, p.pay_bytes);
}

// k_decode: lane g decodes block lane_blk[g]; k_decode_serial: one lane per version-2 item
inline void run_lanes(const DecodeArgs& a, Lane& ln) {
    for (uint32_t g = 0; g < a.lanes; ++g) {
        const uint32_t blk = a.lane_blk[g];
        if (blk == ~0u) continue;
        const DecodeItem& it = a.items[a.blk_item[blk]];
        decode_block_lane(blk, it.channels, it.stereo_mode, a.payload, a.byte_off, a.frame_off, it.frame0, it.left, it.right, a.status,
                          a.ms_flag, ln.dm, ln.lane, ln.wave);
    }
    for (uint32_t g = 0; g < a.nv2; ++g) {
        const DecodeItem& it = a.items[a.v2_items[g]];
        decode_serial_lane(it.blocks, it.channels, it.stereo_mode, a.payload + it.pay_off, it.pay_bits, a.frame_off + it.block0, it.frame0,
                           it.left, it.right, a.status + it.block0, a.ms_flag + it.block0, ln.dm, ln.lane, ln.wave);
    }
}

// k_ms_inverse: grid (blocks, 16 tiles) x 256 threads
inline void run_ms_inverse(const DecodeArgs& a) {
    for (uint32_t blk = 0; blk < a.total_blocks; ++blk) {
        if (a.status[blk]) continue;
        const DecodeItem& it = a.items[a.blk_item[blk]];
        const unsigned long long f0 = a.frame_off[blk];
        const uint32_t n = (uint32_t)(a.frame_off[blk + 1] - f0);
        for (uint32_t tile = 0; tile < (uint32_t)kMaxBlock / 1024u; ++tile)
            for (uint32_t tid = 0; tid < 256u; ++tid)
                ms_inverse_tile(blk, tile, it.channels, it.bit_depth, f0 - it.frame0, n, it.left, it.right, a.ms_flag, a.status, tid);
    }
}

// The salvage pass in stream order.  WAV form: k_salvage_wav, thread u of the concatenated unit ranges.  Device form:
// k_salvage_blank over the lost blocks, grid (blocks, 16 tiles) x 256 threads.
inline void run_salvage_pass(const DecodeArgs& a) {
    if (a.wav) {
        uint32_t item = 0;
        for (unsigned long long u = 0; u < a.total_units; ++u) {
            while (a.unit_off[item + 1] <= u) ++item;
            const DecodeItem& it = a.items[item];
            salvage_wav_unit(4ull * (u - a.unit_off[item]), it.blocks, a.present[item], it.channels, it.bit_depth, it.frames,
                             a.frame_off + it.block0, it.frame0, it.left, it.right, a.status + it.block0, it.wav);
        }
        return;
    }
    for (uint32_t blk = 0; blk < a.total_blocks; ++blk) {
        const uint32_t item = a.blk_item[blk];
        const DecodeItem& it = a.items[item];
        if (!salvage_lost(a.status + it.block0, blk - it.block0, a.present[item])) continue;
        const unsigned long long f0 = a.frame_off[blk];
        const uint32_t n = (uint32_t)(a.frame_off[blk + 1] - f0);
        for (uint32_t tile = 0; tile < (uint32_t)kMaxBlock / 1024u; ++tile)
            for (uint32_t tid = 0; tid < 256u; ++tid)
                salvage_blank_tile(tile, f0 - it.frame0, n, it.left, it.channels == 2 ? it.right : nullptr, tid);
    }
}

// A salvage job's inputs.  Device form: the caller's arrays, one allocation per item and channel of exactly the frames
// lacx_stream_scan tells the caller to allocate, filled 0x5A (a mono item has no right array at all).
struct SalvageIn {
    std::vector<BatchIn> in;
    std::vector<std::unique_ptr<Heap<int32_t>>> own;
    SalvageIn(const uint8_t* const* lacs, const uint64_t* sizes, uint32_t n, bool device) : in(n) {
        for (uint32_t i = 0; i < n; ++i) {
            lacx_stream_info info{};
            uint32_t present = 0, flags = 0;
            const char* why = nullptr;
            int32_t *l = nullptr, *r = nullptr;
            uint64_t frames = 0;
            if (device && scan_stream(lacs[i], sizes[i], &info, &present, &flags, &why) == LACX_OK) {
                frames = info.frames;
                own.emplace_back(new Heap<int32_t>(frames, 0x5A));
                l = own.back()->p;
                if (info.channels == 2) {
                    own.emplace_back(new Heap<int32_t>(frames, 0x5A));
                    r = own.back()->p;
                }
            }
            in[i] = BatchIn{lacs[i], sizes[i], l, r, frames};
        }
    }
};

// The host side's report per planned item, in plan order: fn(p, r, faults, rec) with rec = the eight words of input p.src
// behind its first -- blocks, bad_blocks, frames, lost_frames, first_bad, flags, and `at`: the WAV form's image offset, or
// (device) the offset of the item's frames among the callers' arrays back to back.
template <typename Fn>
void salvage_records(const DecodePlan& plan, const BatchIn* in, const uint32_t* status, bool device, Fn fn) {
    uint64_t at = 0;
    for (const PlanItem& p : plan.items) {
        std::vector<lacx_block_fault> faults;
        const lacx_salvage_result r = salvage_report(p, in[p.src].lac, status, faults);
        const uint64_t rec[7] = {r.blocks, r.bad_blocks, r.frames, r.lost_frames, r.first_bad, r.flags, device ? at : p.image_at};
        if (!fn(p, r, faults, rec)) return;
        if (device) at += r.frames;
    }
}

// the hash of what the caller of a salvage form gets: the device form's left then right, or the image's data region and pad
inline uint64_t salvage_hash(const PlanItem& p, const BatchIn& in, const uint8_t* image, bool device, uint64_t frames) {
    if (!device) return fnv(image + p.image_at + 44, p.image_size - 44, kFnvStart);
    const uint64_t h = fnv(in.left, 4 * frames, kFnvStart);
    return in.right ? fnv(in.right, 4 * frames, h) : h;
}
#endif  // SIM_JOB_SIMULATOR

}  // namespace simjob
