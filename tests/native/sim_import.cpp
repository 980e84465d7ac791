// tests/native/sim_import.cpp -- TEST INFRASTRUCTURE: the import pass's per-thread code (csrc/import_core.h) on the host.
//
// One "workgroup" per unit of kImportUnitFrames frames, its threads one after the other, the threads' keys reduced the way
// k_import's waves and atomics reduce them (the lowest per channel).  Every source row is a heap allocation that ENDS
// exactly at its last element, behind a base at the element offset the case asks for from a 16-byte aligned address; the
// destination holds exactly frames * channels * bit_depth / 8 bytes.  A build with AddressSanitizer therefore reports
// any load or store outside what the product guarantees.  It is not part of the product and is not a fallback.
//
// A case (little-endian, written by tests/importtwin.py):
//   u32 layout, channels, bit_depth, offset (elements);  u64 frames
//   planar: left[frames], right[frames] (stereo); interleaved: frames * channels elements (int16, or float32 bits)
// The right row of a planar source starts (offset + frames) elements behind a 16-byte aligned address: the alignment it has
// as the second row of a [2, frames] tensor whose first row starts at `offset`.
// Answer: u32 alias, u32 code, u64 key_left, u64 key_right, u64 nbytes, the destination's bytes, u32 message length, message.
// Built twice by tests/importtwin.py: a plain -O2 shared library for ctypes, and (-DSIM_IMPORT_MAIN) a sanitized program
// that walks a file of cases and writes a file of answers.
#include "import_msg.h"
#include "sim_job.h"

using namespace lacx;
using namespace simjob;

namespace {

void put(std::string& out, const void* p, size_t n) { out.append(static_cast<const char*>(p), n); }

}  // namespace

extern "C" {

uint32_t sim_import_unit_frames() { return kImportUnitFrames; }

// One case; its answer is appended to *out.  Returns 0, or -1 for a malformed case.
int sim_import_case(const uint8_t* blob, uint64_t size, std::string* out) {
    if (size < 24) return -1;
    uint32_t head[4];
    uint64_t frames;
    std::memcpy(head, blob, 16);
    std::memcpy(&frames, blob + 16, 8);
    const uint32_t layout = head[0], channels = head[1], depth = head[2], offset = head[3];
    const bool planar = layout != (uint32_t)PCM_INTERLEAVED_F32;
    const bool known = layout == (uint32_t)PCM_PLANAR_I16 || layout == (uint32_t)PCM_PLANAR_F32 || layout == (uint32_t)PCM_INTERLEAVED_F32;
    if (!known || (channels != 1 && channels != 2) ||
        (depth != 16 && depth != 24) || frames == 0 || offset > 15 || (layout == (uint32_t)PCM_PLANAR_I16 && depth != 16))
        return -1;
    const uint64_t esz = layout == (uint32_t)PCM_PLANAR_I16 ? 2 : 4;
    const uint64_t row = frames * esz * (planar ? 1 : channels);
    if (size != 24 + frames * channels * esz) return -1;
    Exact s0(row, offset * esz), s1(planar && channels == 2 ? row : 0, ((offset + frames) * esz) % 16u);
    std::memcpy(s0.data, blob + 24, row);
    if (planar && channels == 2) std::memcpy(s1.data, blob + 24 + row, row);
    const uint64_t nbytes = frames * channels * (depth / 8);
    ImportItem it{};
    it.src0 = s0.data;
    it.src1 = planar && channels == 2 ? s1.data : nullptr;
    it.frames = frames;
    it.layout = layout;
    it.channels = (uint8_t)channels;
    it.bit_depth = (uint8_t)depth;
    const uint32_t alias = import_is_alias(layout, channels, it.src0) ? 1u : 0u;
    ImportBad bad{{kImportClean, kImportClean}};
    uint8_t* dst = static_cast<uint8_t*>(std::malloc(nbytes));  // exact (16-byte aligned, as the encoder's buffer is)
    if (alias) {
        std::memcpy(dst, it.src0, nbytes);  // what the front kernels read in place
    } else {
        it.dst = dst;
        const uint64_t units = (frames + kImportUnitFrames - 1) / kImportUnitFrames;
        for (uint64_t u = 0; u < units; ++u) {  // k_import, workgroup by workgroup, thread by thread
            for (uint32_t t = 0; t < kImportThreads; ++t) {
                const unsigned long long f0 = u * kImportUnitFrames + (unsigned long long)kImportQuad * t;
                unsigned long long kl = kImportClean, kr = kImportClean;
                if (f0 < frames) import_quad(it, f0, kl, kr);
                if (kl < bad.key[0]) bad.key[0] = kl;
                if (kr < bad.key[1]) bad.key[1] = kr;
            }
        }
    }
    int ch = 0;
    unsigned long long idx = 0;
    std::string msg;
    const uint32_t code = import_bad_message(bad, (int)depth, &ch, &idx, msg) ? 1u : 0u;  // LACX_E_INVALID / LACX_OK
    const uint32_t mlen = (uint32_t)msg.size();
    put(*out, &alias, 4), put(*out, &code, 4), put(*out, &bad.key[0], 8), put(*out, &bad.key[1], 8), put(*out, &nbytes, 8);
    put(*out, dst, nbytes), put(*out, &mlen, 4), put(*out, msg.data(), mlen);
    std::free(dst);
    return 0;
}

// ctypes form: the answer into a caller's buffer; returns its length, -1 for a malformed case, -2 when it does not fit
long long sim_import_answer(const uint8_t* blob, uint64_t size, uint8_t* answer, uint64_t cap) {
    std::string out;
    if (sim_import_case(blob, size, &out)) return -1;
    if (out.size() > cap) return -2;
    std::memcpy(answer, out.data(), out.size());
    return (long long)out.size();
}

// f32_to_pcm for one value: returns the kind, *v the value
int sim_f32_to_pcm(uint32_t bits, int depth, int32_t* v) { return f32_to_pcm(bits, depth, *v); }

}  // extern "C"

#ifdef SIM_IMPORT_MAIN
// sim_import_san CASES ANSWERS: every case of the file (per case: a 32-bit little-endian size, then the bytes), the answers
// back to back into ANSWERS, "done <cases>" on stdout.
int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* o = std::fopen(argv[2], "wb");
    if (!o) return 2;
    const int rc = for_each_case(argv[1], [&](const uint8_t* blob, uint32_t size, uint32_t) {
        std::string out;
        return !sim_import_case(blob, size, &out) && std::fwrite(out.data(), 1, out.size(), o) == out.size();
    });
    std::fclose(o);
    return rc;
}
#endif
