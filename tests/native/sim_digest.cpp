// tests/native/sim_digest.cpp -- TEST INFRASTRUCTURE: the digest form's per-thread code (csrc/digest_core.h over
// csrc/crc32_core.h) on the host.
//
// One "thread" per unit of four frames of an item, one after the other, and the units' values added up the way k_digest
// adds them: a group of 64 consecutive full units (a wave's fast path) through the tree of per-format constants and one
// shift to the item's end, every other unit shifted by its own distance (the general path); then the init term and the
// final xor, as the host side does.  The decoder's scratch holds exactly `frames` samples per channel, and a source is a
// heap allocation that ENDS exactly at frames * block_align bytes (frames elements for a planar array) behind a base at
// the byte offset the case asks for, so that a build with AddressSanitizer reports any load past what the product
// guarantees.  It is not part of the product and is not a fallback.
//
// A case (little-endian words, written by tests/digesttwin.py):
//   u32 channels, bit_depth, layout, nblocks, noffsets, reserved;  u64 frames
//   u32 block_frames[nblocks], ms[nblocks], status[nblocks]
//   i32 left[frames], right[frames] (stereo)      the decoder's scratch: mid/side where ms says so
//   i32 src_left[frames], src_right[frames]       the source's elements: integer samples, or the bits of a float32
//   u32 offsets[noffsets]                         base alignments: byte offsets from a 16-byte aligned address
// Every offset is one run and one line:
//   "<case> <offset> <crc of the decoded form> <crc of the source form> <source key> <status,status,...>"
// Built twice by tests/digesttwin.py: a plain -O2 shared library for ctypes, and (-DSIM_DIGEST_MAIN) a sanitized program
// that walks a file of cases.
#include "digest_core.h"
#include "sim_job.h"

using namespace lacx;
using namespace simjob;

namespace {

// k_digest's sum over the units of one item: piece(u) is unit u's value and byte count
template <typename Piece>
uint32_t sum_units(uint64_t frames, uint32_t channels, uint32_t bit_depth, Piece piece) {
    const uint32_t align = channels * (bit_depth / 8), unit_bytes = kDigestUnitFrames * align;
    const uint64_t units = (frames + kDigestUnitFrames - 1) / kDigestUnitFrames, total = frames * align;
    const uint32_t* tree = kCrcTables.tree[crc_format((int)channels, (int)bit_depth)];
    uint32_t raw = 0;
    for (uint64_t u0 = 0; u0 < units; u0 += 64) {
        DigestPiece pc[64];
        uint32_t n = 0;
        bool full = true;
        for (; n < 64 && u0 + n < units; ++n) {
            pc[n] = piece(u0 + n);
            full = full && pc[n].bytes == unit_bytes;
        }
        if (n == 64 && full) {  // the fast path: the tree over the lanes, then one shift
            uint32_t v[64];
            for (uint32_t i = 0; i < 64; ++i) v[i] = pc[i].raw;
            for (uint32_t level = 0; level < 6; ++level)
                for (uint32_t i = 0; i < 64; i += 2u << level) v[i] = crc_mul(v[i], tree[level]) ^ v[i + (1u << level)];
            raw ^= crc_shift(v[0], total - (u0 + 64) * unit_bytes);
        } else {  // the general path: every unit by itself
            for (uint32_t i = 0; i < n; ++i) raw ^= crc_shift(pc[i].raw, total - (u0 + i) * unit_bytes - pc[i].bytes);
        }
    }
    return crc_finish(raw, total);
}

}  // namespace

extern "C" {

uint32_t sim_digest_unit_frames() { return kDigestUnitFrames; }
uint32_t sim_digest_threads() { return kDigestThreads; }
uint32_t sim_crc_mul(uint32_t a, uint32_t b) { return crc_mul(a, b); }
uint32_t sim_crc_shift(uint32_t r, uint64_t n) { return crc_shift(r, n); }
uint32_t sim_crc32_combine(uint32_t a, uint32_t b, uint64_t len_b) { return crc32_combine(a, b, len_b); }
uint32_t sim_crc32_wav_header(uint32_t channels, uint32_t bit_depth, uint32_t rate, uint64_t data_bytes) {
    return crc32_wav_header(channels, bit_depth, rate, data_bytes);
}

// Runs every offset of one case; appends one line each to *out.  Returns 0, or -1 for a malformed case.
int sim_digest_case(const uint8_t* blob, uint64_t size, uint32_t index, std::string* out) {
    Reader rd{blob, blob + size};
    const uint32_t channels = rd.get<uint32_t>(), bit_depth = rd.get<uint32_t>(), layout = rd.get<uint32_t>();
    const uint32_t nb = rd.get<uint32_t>(), noff = rd.get<uint32_t>();
    (void)rd.get<uint32_t>();
    const uint64_t frames = rd.get<uint64_t>();
    const bool known = layout <= 2 || (layout >= 16 && layout <= 18);
    if (!rd.ok || (channels != 1 && channels != 2) || (bit_depth != 16 && bit_depth != 24) || !known || nb == 0 || frames == 0) return -1;
    const std::vector<uint32_t> bf = rd.array<uint32_t>(nb), ms32 = rd.array<uint32_t>(nb), st_in = rd.array<uint32_t>(nb);
    const std::vector<int32_t> dl = rd.array<int32_t>(frames), dr = rd.array<int32_t>(channels == 2 ? frames : 0);
    const std::vector<int32_t> sl = rd.array<int32_t>(frames), sr = rd.array<int32_t>(channels == 2 ? frames : 0);
    const std::vector<uint32_t> offsets = rd.array<uint32_t>(noff);
    if (!rd.ok) return -1;
    std::vector<unsigned long long> frame_off(nb + 1, 0);
    std::vector<uint8_t> ms(nb);
    for (uint32_t b = 0; b < nb; ++b) frame_off[b + 1] = frame_off[b] + bf[b], ms[b] = (uint8_t)ms32[b];
    if (frame_off[nb] != frames) return -1;
    const bool two_rows = planar(layout) && channels == 2;
    const uint64_t bytes = (uint64_t)elem_bytes(layout) * frames * (planar(layout) ? 1u : channels);
    for (uint32_t off : offsets) {
        // the decoder's scratch: exactly `frames` samples per channel, 16-byte aligned (malloc), status per run
        int32_t* L = static_cast<int32_t*>(std::malloc(4 * frames));
        int32_t* R = channels == 2 ? static_cast<int32_t*>(std::malloc(4 * frames)) : nullptr;
        std::memcpy(L, dl.data(), 4 * frames);
        if (R) std::memcpy(R, dr.data(), 4 * frames);
        std::vector<uint32_t> status(st_in);
        Exact s0(bytes, off), s1(two_rows ? bytes : 0, off);
        uint8_t* p1 = two_rows ? s1.data : nullptr;
        for (uint64_t f = 0; f < frames; ++f) {
            put_elem(s0.data, p1, layout, channels, f, 0, sl[f]);
            if (channels == 2) put_elem(s0.data, p1, layout, channels, f, 1, sr[f]);
        }
        const uint32_t decoded = sum_units(frames, channels, bit_depth, [&](uint64_t u) {
            return digest_unit_decoded(kDigestUnitFrames * u, nb, (int)channels, (int)bit_depth, frames, frame_off.data(), 0, L, R, ms.data(),
                                       status.data());
        });
        unsigned long long key = kDigestClean;
        const uint32_t source = sum_units(frames, channels, bit_depth, [&](uint64_t u) {
            return digest_unit_source(kDigestUnitFrames * u, (int)channels, (int)bit_depth, frames, s0.data, p1, layout, key);
        });
        char head[160];
        std::snprintf(head, sizeof(head), "%u %u %u %u %llu ", index, off, decoded, source, key);
        *out += head;
        for (uint32_t b = 0; b < nb; ++b) *out += (b ? "," : "") + std::to_string(status[b]);
        *out += "\n";
        std::free(L);
        std::free(R);
    }
    return 0;
}

// ctypes form: the lines into a caller's buffer
int sim_digest_lines(const uint8_t* blob, uint64_t size, uint32_t index, char* lines, uint64_t cap) {
    std::string out;
    if (sim_digest_case(blob, size, index, &out)) return -1;
    if (out.size() + 1 > cap) return -2;
    std::memcpy(lines, out.c_str(), out.size() + 1);
    return 0;
}

}  // extern "C"

#ifdef SIM_DIGEST_MAIN
// sim_digest_san CASES: every case of the file (per case: a 32-bit little-endian size, then the bytes), its lines on
// stdout, "done <cases>" at the end.
int main(int argc, char** argv) {
    if (argc != 2) return 2;
    return for_each_case(argv[1], [](const uint8_t* blob, uint32_t size, uint32_t i) {
        std::string out;
        return !sim_digest_case(blob, size, i, &out) && std::fputs(out.c_str(), stdout) >= 0;
    });
}
#endif
