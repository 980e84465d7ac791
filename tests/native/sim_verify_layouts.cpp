// tests/native/sim_verify_layouts.cpp -- TEST INFRASTRUCTURE: the verify form's per-thread code (csrc/verify_core.h) on the
// host for sources in ANY layout, the tensor layouts among them (tests/native/sim_verify.cpp builds its sources itself, in
// the three integer layouts only).  The caller hands over the decoder's scratch and the source exactly as the kernel would
// see them (numpy arrays, at whatever base alignment it chose); the units' answers are added up the way k_verify's waves
// and atomics add them, then verify_fill_item.  Not part of the product and not a fallback.
#include <cstdint>
#include <vector>

#include "verify_core.h"

using namespace lacx;

extern "C" {

// out: count, key, decoded, source, block.  status: [nb], updated in place.
int sim_verify_layout(uint32_t channels, uint32_t bit_depth, uint32_t layout, uint32_t nb, const uint32_t* block_frames,
                      const uint8_t* ms, uint32_t* status, const int32_t* left, const int32_t* right, uint64_t frames,
                      const void* src0, const void* src1, long long* out) {
    std::vector<unsigned long long> frame_off(nb + 1, 0);
    for (uint32_t b = 0; b < nb; ++b) frame_off[b + 1] = frame_off[b] + block_frames[b];
    if (frame_off[nb] != frames || ((uintptr_t)left & 15u) || (right && ((uintptr_t)right & 15u))) return -1;
    VerifyWords w{0, ~0ull, 0, 0, 0, 0};
    for (uint64_t u = 0; u < (frames + 3) / 4; ++u) {  // k_verify, thread by thread
        const uint32_t differ = verify_unit(4 * u, nb, (int)channels, (int)bit_depth, frames, frame_off.data(), 0, left, right, ms,
                                            status, src0, src1, layout);
        if (!differ) continue;
        w.count += (unsigned)__builtin_popcount(differ);
        const unsigned long long key = 8 * u + (unsigned)__builtin_ctz(differ);
        if (key < w.key) w.key = key;
    }
    verify_fill_item(nb, (int)channels, frame_off.data(), 0, left, right, ms, src0, src1, layout, w, (int)bit_depth);  // k_verify_fill
    out[0] = (long long)w.count, out[1] = (long long)w.key, out[2] = w.decoded, out[3] = w.source, out[4] = w.block;
    return 0;
}

}  // extern "C"
