// sim_edit.cpp -- the CPU twin of k_edit (csrc/k_edit.hip): edit_core.h's per-thread code driven over an output the way the
// kernel drives it -- unit by unit, thread by thread, the keys reduced to their minimum as the wave reduction and the
// atomicMin do -- on heap blocks of exactly the planned sizes: staging rows of `frames` int32, a destination of
// frames * channels * depth / 8 bytes.  Built plain and under AddressSanitizer + UBSan (tests/test_edit_twin_host.py); a load
// or store outside a block stops the sanitized build.  Every case also runs on a destination with guard bytes behind it,
// which must come back untouched.
//
// A case (little-endian, in a file of frames <u32 size><bytes>): u32 src_channels, channel_op, src_depth, dst_depth;
// u64 frames; int32 left[frames]; int32 right[frames] (stereo sources).  Answer: "<case> <key> <guards intact> <dst as hex>".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "edit_core.h"

using namespace lacx;

namespace {

constexpr size_t kGuard = 64;

unsigned long long run_output(const EditItem& it) {
    unsigned long long bad = kEditClean;
    const unsigned long long units = (it.frames + kEditUnitFrames - 1u) / kEditUnitFrames;
    for (unsigned long long unit = 0; unit < units; ++unit) {
        for (uint32_t t = 0; t < kEditThreads; ++t) {
            const unsigned long long f0 = unit * kEditUnitFrames + kEditQuad * t;
            unsigned long long key = kEditClean;
            if (f0 < it.frames) edit_quad(it, f0, key);
            bad = key < bad ? key : bad;
        }
    }
    return bad;
}

void run_case(size_t index, const uint8_t* p) {
    uint32_t head[4];
    unsigned long long frames;
    std::memcpy(head, p, 16);
    std::memcpy(&frames, p + 16, 8);
    p += 24;
    const size_t row = (size_t)frames * 4;
    int32_t* left = static_cast<int32_t*>(std::malloc(row));  // (malloc: 16-byte aligned, exactly the row)
    int32_t* right = head[0] == 2 ? static_cast<int32_t*>(std::malloc(row)) : nullptr;
    std::memcpy(left, p, row);
    if (right) std::memcpy(right, p + row, row);
    const size_t bytes = (size_t)frames * edit_channels_out(head[0], head[1]) * (head[3] / 8);
    uint8_t* exact = static_cast<uint8_t*>(std::malloc(bytes));
    uint8_t* guarded = static_cast<uint8_t*>(std::malloc(bytes + kGuard));
    std::memset(exact, 0xEE, bytes);
    std::memset(guarded, 0xA5, bytes + kGuard);
    EditItem it{left, right, exact, frames, (uint8_t)head[0], (uint8_t)head[1], (uint8_t)head[2], (uint8_t)head[3], {0, 0, 0, 0}};
    const unsigned long long key = run_output(it);
    it.dst = guarded;
    const unsigned long long key2 = run_output(it);
    bool intact = key == key2 && std::memcmp(exact, guarded, bytes) == 0;
    for (size_t i = 0; i < kGuard; ++i) intact = intact && guarded[bytes + i] == 0xA5;
    std::string hex(2 * bytes, '0');
    for (size_t i = 0; i < bytes; ++i) hex[2 * i] = "0123456789abcdef"[exact[i] >> 4], hex[2 * i + 1] = "0123456789abcdef"[exact[i] & 15];
    std::printf("%zu %llu %d %s\n", index, key, intact ? 1 : 0, hex.c_str());
    std::free(left), std::free(right), std::free(exact), std::free(guarded);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<uint8_t> data;
    uint8_t buf[65536];
    for (size_t n; (n = std::fread(buf, 1, sizeof(buf), f)) > 0;) data.insert(data.end(), buf, buf + n);
    std::fclose(f);
    size_t at = 0, cases = 0;
    while (at + 4 <= data.size()) {
        uint32_t size;
        std::memcpy(&size, data.data() + at, 4);
        at += 4;
        const std::vector<uint8_t> one(data.begin() + at, data.begin() + at + size);
        at += size;
        run_case(cases++, one.data());
    }
    std::printf("done %zu\n", cases);
    return 0;
}
