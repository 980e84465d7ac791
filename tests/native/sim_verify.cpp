// tests/native/sim_verify.cpp -- TEST INFRASTRUCTURE: the verify form's per-thread code (csrc/verify_core.h) on the host.
//
// One "thread" per unit of four frames of an item, one after the other, the units' answers added up the way k_verify's
// waves and atomics add them (a count, the lowest key), then verify_fill_item -- the work of k_verify / k_verify_fill for
// one item.  The source PCM is a heap allocation that ENDS exactly at frames * block_align bytes (frames int32 for a
// planar array) behind a base at the byte offset the case asks for, and the decoded scratch holds exactly `frames`
// samples, so that a build with AddressSanitizer reports any load past what the product guarantees.  It is not part of
// the product and is not a fallback.
//
// A case (little-endian words, written by tests/vertwin.py):
//   u32 channels, bit_depth, layout, nblocks, noffsets, ngroups;  u64 frames
//   u32 block_frames[nblocks], ms[nblocks], status[nblocks]
//   i32 left[frames], right[frames] (stereo)      the decoder's scratch: mid/side where ms says so
//   i32 src_left[frames], src_right[frames]       the source's samples (written into the layout here)
//   u32 offsets[noffsets]                         base alignments: byte offsets from a 16-byte aligned address
//   per group: u32 nedits, then nedits x (u64 frame, u32 channel, i32 value); nedits = ~0: every sample ^ 1
// Every (offset, group) pair is one run and one line:
//   "<case> <offset> <group> <mismatches> <key> <decoded> <source> <block> <status,status,...>"
// Built twice by tests/vertwin.py: a plain -O2 shared library for ctypes, and (-DSIM_VERIFY_MAIN) a sanitized program
// that walks a file of cases.
#include "sim_job.h"
#include "verify_core.h"

using namespace lacx;
using namespace simjob;

extern "C" {

// Runs every (offset, group) pair of one case; appends one line each to *out.  Returns 0, or -1 for a malformed case.
int sim_verify_case(const uint8_t* blob, uint64_t size, uint32_t index, std::string* out) {
    Reader rd{blob, blob + size};
    const uint32_t channels = rd.get<uint32_t>(), bit_depth = rd.get<uint32_t>(), layout = rd.get<uint32_t>();
    const uint32_t nb = rd.get<uint32_t>(), noff = rd.get<uint32_t>(), ngroups = rd.get<uint32_t>();
    const uint64_t frames = rd.get<uint64_t>();
    if (!rd.ok || (channels != 1 && channels != 2) || layout > 2 || nb == 0 || frames == 0) return -1;
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
    for (uint32_t g = 0; g < ngroups; ++g) {
        const uint32_t nedits = rd.get<uint32_t>();
        struct Edit {
            uint64_t f;
            uint32_t c;
            int32_t v;
        };
        std::vector<Edit> edits;
        for (uint32_t e = 0; nedits != ~0u && e < nedits; ++e) {
            Edit x;
            x.f = rd.get<uint64_t>(), x.c = rd.get<uint32_t>(), x.v = rd.get<int32_t>();
            if (!rd.ok || x.f >= frames || x.c >= channels) return -1;
            edits.push_back(x);
        }
        if (!rd.ok) return -1;
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
                put_elem(s0.data, p1, layout, channels, f, 0, nedits == ~0u ? sl[f] ^ 1 : sl[f]);
                if (channels == 2) put_elem(s0.data, p1, layout, channels, f, 1, nedits == ~0u ? sr[f] ^ 1 : sr[f]);
            }
            for (const Edit& x : edits) put_elem(s0.data, p1, layout, channels, x.f, x.c, x.v);
            VerifyWords w{0, ~0ull, 0, 0, 0, 0};
            for (uint64_t u = 0; u < (frames + 3) / 4; ++u) {  // k_verify, thread by thread
                const uint32_t differ = verify_unit(4 * u, nb, (int)channels, (int)bit_depth, frames, frame_off.data(), 0, L, R,
                                                    ms.data(), status.data(), s0.data, p1, layout);
                if (!differ) continue;
                w.count += (unsigned)__builtin_popcount(differ);
                const unsigned long long key = 8 * u + (unsigned)__builtin_ctz(differ);
                if (key < w.key) w.key = key;
            }
            verify_fill_item(nb, (int)channels, frame_off.data(), 0, L, R, ms.data(), s0.data, p1, layout, w);  // k_verify_fill
            char head[160];
            std::snprintf(head, sizeof(head), "%u %u %u %llu %llu %d %d %u ", index, off, g, w.count, w.key, w.decoded, w.source,
                          w.block);
            *out += head;
            for (uint32_t b = 0; b < nb; ++b) *out += (b ? "," : "") + std::to_string(status[b]);
            *out += "\n";
            std::free(L);
            std::free(R);
        }
    }
    return 0;
}

// ctypes form: the lines into a caller's buffer
int sim_verify_lines(const uint8_t* blob, uint64_t size, uint32_t index, char* lines, uint64_t cap) {
    std::string out;
    if (sim_verify_case(blob, size, index, &out)) return -1;
    if (out.size() + 1 > cap) return -2;
    std::memcpy(lines, out.c_str(), out.size() + 1);
    return 0;
}

}  // extern "C"

#ifdef SIM_VERIFY_MAIN
// sim_verify_san CASES: every case of the file (per case: a 32-bit little-endian size, then the bytes), its lines on
// stdout, "done <cases>" at the end.
int main(int argc, char** argv) {
    if (argc != 2) return 2;
    return for_each_case(argv[1], [](const uint8_t* blob, uint32_t size, uint32_t i) {
        std::string out;
        return !sim_verify_case(blob, size, i, &out) && std::fputs(out.c_str(), stdout) >= 0;
    });
}
#endif
