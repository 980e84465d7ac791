// Driver for the sanitizer build of the kernel-phase simulator (tests/test_native_units.py): runs the analysis
// and emit phases over a handful of block shapes and materials; AddressSanitizer / UBSan abort on any
// out-of-bounds LDS-image access, shift or overflow in the phase code the HIP kernels are built from.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "lacx_types.h"

extern "C" int sim_block_encode(const int32_t* x, uint32_t n, int zero_run, int partitioning, int force_wide, uint8_t* out,
                                uint32_t cap);
extern "C" int sim_block_plan(const int32_t* x, uint32_t n, int zero_run, int partitioning, int geo, int force_wide,
                              lacx::ChannelPlan* out);

int main() {
    uint64_t s = 0x9E3779B97F4A7C15ull;
    auto rnd = [&s]() {
        s ^= s << 13;
        s ^= s >> 7;
        s ^= s << 17;
        return (uint32_t)(s >> 32);
    };
    const uint32_t sizes[] = {16384, 16383, 4097, 4096, 257, 256, 33, 2, 1};
    std::vector<uint8_t> out(16384 * 8 + 64);
    int runs = 0;
    for (int kind = 0; kind < 6; ++kind) {
        for (uint32_t n : sizes) {
            std::vector<int32_t> x(n);
            int32_t walk = 0;
            for (uint32_t i = 0; i < n; ++i) {
                const int32_t r = (int32_t)(rnd() % 65536u) - 32768;
                switch (kind) {
                    case 0: x[i] = r; break;                                       // white noise, 16 bit
                    case 1: x[i] = r * 256 + (int32_t)(rnd() & 255u); break;       // loud 24 bit: 64-bit paths
                    case 2: x[i] = 0; break;                                       // silence
                    case 3: x[i] = (rnd() % 97u == 0) ? (r >> 6) : 0; break;       // sparse: zero runs
                    case 4: walk += (r >> 10); x[i] = walk; break;                 // random walk
                    default: x[i] = (int32_t)(i & 3u) - 1; break;                  // +-1: bin mode
                }
            }
            for (int wide = 0; wide < 8; wide += (n > 1000 ? 3 : 1)) {
                if (sim_block_encode(x.data(), n, 1, 1, wide, out.data(), (uint32_t)out.size()) < 0) return 2;
                ++runs;
            }
            lacx::ChannelPlan plan;
            if (n <= 256 && sim_block_plan(x.data(), n, 1, 1, 1, 0, &plan) != 0) return 3;
        }
    }
    // Look-alikes of the families `geometry` and `tokens` of tests/narrowrecipes.py, not the corpus blocks themselves (the
    // generator here is this file's own, and nothing here asserts which plan wins; the corpus with its asserted coverage
    // runs through the unsanitized simulator in tests/test_narrow_blocks_host.py): stretches of n >> p samples whose
    // character changes from each to the next at sizes whose borders fall inside 16-sample chunks (p is a parameter of
    // the recipe, not the order that wins), and the token material (sparse spikes, zero outside the first stretch, short
    // zero runs, outliers with long unary parts, bin material), under both partitioning flags.
    const uint32_t geo_sizes[] = {4097, 8223, 12289, 16383, 16384};
    for (uint32_t n : geo_sizes) {
        for (int p = 5; p <= 8; ++p) {
            if ((n >> p) < 32u) continue;
            std::vector<int32_t> x(n);
            const uint32_t base = n >> p;
            for (uint32_t i = 0; i < n; ++i) {
                uint32_t part = i / base;
                if (part >= (1u << p)) part = (1u << p) - 1u;
                const int32_t r = (int32_t)(rnd() % 65536u) - 32768;
                switch (part % 5u) {
                    case 0: x[i] = (i - part * base == base / 2) ? 1 : 0; break;   // zeros with one 1
                    case 1: x[i] = (int32_t)(rnd() % 5u) - 2; break;                // 0 / +-1 / +-2
                    case 2: x[i] = r >> 10; break;                                  // quiet
                    case 3: x[i] = r >> 3; break;                                   // medium
                    default: x[i] = r * 16; break;                                  // loud
                }
            }
            for (int pt = 0; pt < 2; ++pt) {
                if (sim_block_encode(x.data(), n, 1, pt, 0, out.data(), (uint32_t)out.size()) < 0) return 4;
                ++runs;
            }
        }
    }
    const uint32_t token_sizes[] = {16384, 12289};
    for (uint32_t n : token_sizes) {
        for (int kind = 0; kind < 5; ++kind) {
            std::vector<int32_t> x(n, 0);
            uint32_t next = 40, zeros = 0;
            for (uint32_t i = 0; i < n; ++i) {
                const int32_t sign = (rnd() & 1u) ? 1 : -1;
                switch (kind) {
                    case 0:  // a spike of up to 2^20 every 600..900 samples
                        if (i == next) {
                            x[i] = sign * (int32_t)(1024u + rnd() % (1u << 20));
                            next += 600u + rnd() % 300u;
                        }
                        break;
                    case 1: x[i] = (i < 100u && i % 17u == 3u) ? (int32_t)(100u + rnd() % 4900u) : 0; break;
                    case 2:  // bursts between zero runs of 1..5 and of 20..60
                        if (zeros) {
                            --zeros;
                        } else {
                            x[i] = sign * (int32_t)(1u + rnd() % 30u);
                            if (rnd() % 7u == 0) zeros = (rnd() % 5u < 3u) ? 1u + rnd() % 5u : 20u + rnd() % 41u;
                        }
                        break;
                    case 3: x[i] = sign * (int32_t)((i % 1500u == 700u) ? 270u + rnd() % 2700u : 4u + rnd() % 9u); break;
                    default:
                        x[i] = (i % (n >> 3) == 0) ? (int32_t)(16384u + rnd() % (1u << 20))
                                                   : ((i % 5u == 0) ? 0 : sign * (int32_t)(1u + (rnd() & 1u)));
                        break;
                }
            }
            for (int pt = 0; pt < 2; ++pt) {
                if (sim_block_encode(x.data(), n, 1, pt, pt ? 0 : 1, out.data(), (uint32_t)out.size()) < 0) return 5;
                ++runs;
            }
        }
    }
    std::printf("sanitized simulator runs: %d\n", runs);
    return 0;
}
