// tests/native/sim_decode.cpp -- TEST INFRASTRUCTURE: the decoder's lane code (csrc/decode_core.h) on the host.
//
// One "lane" per block of a version-3 stream (or one lane for a version-2 stream), then the mid/side pass over every
// block that decoded -- the work of k_decode / k_decode_serial / k_ms_inverse, one lane after the other.  Every buffer
// the device path hands to a lane is a heap allocation of its own, of exactly the size the device path guarantees
// (api_decode.cpp), so that a build with AddressSanitizer reports any access the bounds argument at BitIn does not
// cover:  payload = the blocks' bytes + the tail pad (zeroed), left / right = exactly `frames` samples,
// lane memory = kDecBytesPerCol * cols.  It is not part of the product and is not a fallback.
//
// Built twice by tests/dectwin.py: a plain -O2 shared library for ctypes, and (-DSIM_DECODE_MAIN) a sanitized program that
// walks a corpus file through every switch setting and prints one digest line per stream.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "decode_core.h"

using namespace lacx;

namespace {

uint32_t be32(const uint8_t* p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3]; }

// a permutation of 0..n-1 from a seed (the order in which the gathered layout places the blocks)
void shuffle(std::vector<uint32_t>& v, uint32_t seed) {
    uint64_t s = 0x9E3779B97F4A7C15ull * (seed + 1u);
    for (size_t i = v.size(); i > 1; --i) {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        std::swap(v[i - 1], v[(size_t)((s >> 33) % i)]);
    }
}

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

}  // namespace

constexpr uint32_t kSimDefaultPad = ~0u;
// the bounds argument at BitIn: the derived worst overshoot of a trip must fit the pad the product appends
static_assert(kDecodeTailPad >= 25, "kDecodeTailPad is below the overshoot the comment at BitIn derives");

extern "C" {

uint32_t sim_tail_pad(void) { return (uint32_t)kDecodeTailPad; }

// FNV-1a over n samples, chained through `h` (start with 0): how the two builds' PCM is compared without moving it
uint64_t sim_hash(const int32_t* x, uint64_t n, uint64_t h) {
    if (h == 0) h = 0xCBF29CE484222325ull;
    for (uint64_t i = 0; i < n; ++i) {
        h ^= (uint32_t)x[i];
        h *= 0x100000001B3ull;
    }
    return h;
}

// A whole .lac that lacx_stream_parse accepts.  never_lean: the wave policy (DecWave); cols: 1 or 64 columns of lane
// memory, the lane being the last column; gather_seed: 0 = the payload as it lies in the stream, else the blocks'
// payloads back to back in a shuffled order (what gather_ranges makes of a window batch: a block's successor in memory
// is not its successor in the stream); pad: the zero bytes behind the payload -- kSimDefaultPad (~0) = kDecodeTailPad, what
// the device path appends; any other value only to show that a shorter pad is reported.
// Out: status[blocks], ms[blocks], left[frames], right[frames] (stereo), *over = the furthest byte a load reached past
// the end of the block it was reading.  Returns 0, or -1 for a stream the container walk cannot take.
int sim_decode(const uint8_t* lac, uint64_t size, int never_lean, int cols, uint32_t gather_seed, uint32_t pad,
               uint32_t* status, uint8_t* ms, int32_t* left, int32_t* right, uint32_t* over) {
    if (size < 14 || (lac[2] != 2 && lac[2] != 3) || (cols != 1 && cols != 64)) return -1;
    if (pad == kSimDefaultPad) pad = (uint32_t)kDecodeTailPad;
    const int version = lac[2], channels = lac[3], stereo_mode = lac[4], bit_depth = lac[8];
    const uint32_t nb = be32(lac + 10);
    const uint64_t entry = version == 3 ? 8u : 4u, head = 14 + entry * nb;
    if (nb == 0 || size < head) return -1;
    std::vector<unsigned long long> byte_off(nb + 1, 0), frame_off(nb + 1, 0);
    for (uint32_t b = 0; b < nb; ++b) {
        frame_off[b + 1] = frame_off[b] + be32(lac + 14 + entry * b);
        byte_off[b + 1] = version == 3 ? byte_off[b] + be32(lac + 18 + 8ull * b) : 0;
    }
    const uint64_t total_pay = size - head, frames = frame_off[nb];
    if (version == 3 && byte_off[nb] != total_pay) return -1;
    if (version == 2) byte_off[nb] = total_pay;  // one lump at the last block, as the device tables have it

    // where each block's payload lies in the buffer: stream order, or gathered
    std::vector<unsigned long long> at(byte_off.begin(), byte_off.end() - 1);
    Heap<uint8_t> payload(total_pay + pad);
    if (version == 3 && gather_seed) {
        std::vector<uint32_t> order(nb);
        for (uint32_t b = 0; b < nb; ++b) order[b] = b;
        shuffle(order, gather_seed);
        unsigned long long cur = 0;
        for (uint32_t b : order) {
            at[b] = cur;
            std::memcpy(payload.p + cur, lac + head + byte_off[b], byte_off[b + 1] - byte_off[b]);
            cur += byte_off[b + 1] - byte_off[b];
        }
    } else {
        std::memcpy(payload.p, lac + head, total_pay);
    }
    Heap<int32_t> L(frames), R(channels == 2 ? frames : 0);
    Heap<uint32_t> st(nb);
    Heap<uint8_t> flag(nb);
    Heap<unsigned char> raw(kDecBytesPerCol * (size_t)cols, 0xA5);
    DecMem dm = dec_mem(raw.p, (uint32_t)cols);
    const int lane = cols - 1;
    DecWave wave;
    wave.never_lean = never_lean != 0;
    int32_t* rp = channels == 2 ? R.p : nullptr;
    if (version == 2) {
        decode_serial_lane(nb, channels, stereo_mode, payload.p, (uint32_t)(8ull * total_pay), frame_off.data(), 0, L.p, rp,
                           st.p, flag.p, dm, lane, wave);
    } else {
        for (uint32_t b = 0; b < nb; ++b) {  // the block's own two-entry tables: its place in the buffer, its frames
            const unsigned long long bo[2] = {at[b], at[b] + (byte_off[b + 1] - byte_off[b])};
            const unsigned long long fo[2] = {frame_off[b], frame_off[b + 1]};
            decode_block_lane(0, channels, stereo_mode, payload.p, bo, fo, 0, L.p, rp, st.p + b, flag.p + b, dm, lane, wave);
        }
    }
    for (uint32_t b = 0; b < nb; ++b) {  // k_ms_inverse: grid (blocks, 16 tiles) x 256 threads
        if (st.p[b]) continue;
        const uint32_t n = (uint32_t)(frame_off[b + 1] - frame_off[b]);
        for (uint32_t tile = 0; tile < (uint32_t)kMaxBlock / 1024u; ++tile)
            for (uint32_t tid = 0; tid < 256u; ++tid)
                ms_inverse_tile(b, tile, channels, bit_depth, frame_off[b], n, L.p, rp, flag.p, st.p, tid);
    }
    std::memcpy(status, st.p, nb * sizeof(uint32_t));
    std::memcpy(ms, flag.p, nb);
    std::memcpy(left, L.p, frames * sizeof(int32_t));
    if (channels == 2) std::memcpy(right, R.p, frames * sizeof(int32_t));
    *over = wave.over;
    return 0;
}

// One line per stream: what the first setting gave, and whether every other setting gave the same.
//   "<index> <over> <pcm hash of the blocks that decoded> <same: 1|0> <status,status,...>"
// settings: bit s set = run setting s, s = never_lean | (cols == 64) << 1 | gathered << 2.  0 = four of the eight, in
// which every switch takes both values and every pair of switches all four combinations: settings 0 3 5 6 for an even
// index, their complements 1 2 4 7 for an odd one (a corpus of tens of thousands then sees all eight, at half the time).
int sim_digest(const uint8_t* lac, uint64_t size, uint32_t index, uint32_t settings, uint32_t pad, char* line, uint32_t cap) {
    if (size < 14) return -1;
    const int version = lac[2], channels = lac[3];
    const uint32_t nb = be32(lac + 10);
    const uint64_t entry = version == 3 ? 8u : 4u;
    if (nb == 0 || size < 14 + entry * nb) return -1;
    uint64_t frames = 0;
    std::vector<uint32_t> fr(nb);
    for (uint32_t b = 0; b < nb; ++b) frames += fr[b] = be32(lac + 14 + entry * b);
    if (settings == 0) settings = (index & 1u) ? 0x96u : 0x69u;
    std::vector<uint32_t> st0, st(nb);
    std::vector<uint8_t> ms0, ms(nb);
    std::vector<int32_t> l0, r0, l(frames), r(channels == 2 ? frames : 0);
    uint32_t over = 0, same = 1;
    bool first = true;
    for (uint32_t s = 0; s < 8; ++s) {
        if (!((settings >> s) & 1u)) continue;
        uint32_t ov = 0;
        if (sim_decode(lac, size, s & 1, (s & 2) ? 64 : 1, (s & 4) ? index + 1u : 0u, pad, st.data(), ms.data(), l.data(),
                       r.data(), &ov))
            return -1;
        if (ov > over) over = ov;
        if (first) {
            st0 = st, ms0 = ms, l0 = l, r0 = r;
            first = false;
            continue;
        }
        if (st != st0) same = 0;
        uint64_t f0 = 0;
        for (uint32_t b = 0; b < nb; f0 += fr[b], ++b) {
            if (st0[b] || st[b]) continue;
            if (ms[b] != ms0[b] || std::memcmp(&l[f0], &l0[f0], 4ull * fr[b]) ||
                (channels == 2 && std::memcmp(&r[f0], &r0[f0], 4ull * fr[b])))
                same = 0;
        }
    }
    if (first) return -1;
    uint64_t h = 0, f0 = 0;
    for (uint32_t b = 0; b < nb; f0 += fr[b], ++b) {
        if (st0[b]) continue;
        h = sim_hash(&l0[f0], fr[b], h);
        if (channels == 2) h = sim_hash(&r0[f0], fr[b], h);
        h = sim_hash(reinterpret_cast<const int32_t*>(&fr[b]), 1, h ^ ms0[b]);
    }
    int n = std::snprintf(line, cap, "%u %u %016llx %u ", index, over, (unsigned long long)h, same);
    for (uint32_t b = 0; b < nb && n > 0 && (uint32_t)n + 12 < cap; ++b)
        n += std::snprintf(line + n, cap - (uint32_t)n, b ? ",%u" : "%u", st0[b]);
    return (n > 0 && (uint32_t)n + 12 < cap) ? 0 : -1;
}

}  // extern "C"

#ifdef SIM_DECODE_MAIN
// sim_decode_san CORPUS FIRST COUNT SETTINGS PAD (PAD 4294967295 = kDecodeTailPad): streams [FIRST, FIRST + COUNT) of a corpus file (per stream: a 32-bit
// little-endian size, then the bytes), one digest line each on stdout, "done <count>" at the end.
int main(int argc, char** argv) {
    if (argc != 6) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    const unsigned long first = std::strtoul(argv[2], nullptr, 10), count = std::strtoul(argv[3], nullptr, 10);
    const uint32_t settings = (uint32_t)std::strtoul(argv[4], nullptr, 10), pad = (uint32_t)std::strtoul(argv[5], nullptr, 10);
    std::vector<char> line(1 << 20);
    unsigned long done = 0;
    for (unsigned long i = 0; i < first + count; ++i) {
        uint8_t sz[4];
        if (std::fread(sz, 1, 4, f) != 4) break;
        const uint32_t size = sz[0] | (sz[1] << 8) | (sz[2] << 16) | ((uint32_t)sz[3] << 24);
        if (i < first) {
            std::fseek(f, (long)size, SEEK_CUR);
            continue;
        }
        Heap<uint8_t> lac(size);  // the stream itself, exact too: the container walk is checked with it
        if (std::fread(lac.p, 1, size, f) != size) return 3;
        if (sim_digest(lac.p, size, (uint32_t)i, settings, pad, line.data(), (uint32_t)line.size())) return 4;
        std::puts(line.data());
        ++done;
    }
    std::fclose(f);
    std::printf("done %lu\n", done);
    return 0;
}
#endif
