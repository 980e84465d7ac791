// manifest.h -- the sidecar of block digests (lacx.h): its bytes, its builder and its parser, and the rows of block digests
// themselves as the host side finishes them from what the device summed.  Host only, no HIP: the C ABI (api_decode.cpp),
// the plan (decode_plan.h: a judged item's expected values) and tests/native/sim_blockdigest.cpp, which calls the same
// row builders the ABI calls.
// Big-endian like the container, 32 + 8 * blocks bytes:
//   0 "LACM" | 4 version = 1 | 5 channels | 6 bit depth | 7 zero | 8 sample rate u32 | 12 frames u64 | 20 blocks u32 |
//   24 data_crc32 u32 (of the whole data chunk) | 28 rows: frames u32, crc32 u32 | end - 4: zlib CRC-32 of all before it
#pragma once
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "container.h"
#include "crc32_core.h"
#include "lacx.h"

namespace lacx {

constexpr uint64_t kManifestRowsAt = 28, kManifestFixed = 32;
constexpr uint32_t kManifestMaxRow = 16384, kManifestMinRow = 256;  // Block::MAX_BLOCK_SIZE; the container's non-final minimum

namespace manifest_detail {
inline uint32_t mget32(const uint8_t* p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3]; }
inline void mput32(uint8_t* p, uint32_t v) { p[0] = (uint8_t)(v >> 24), p[1] = (uint8_t)(v >> 16), p[2] = (uint8_t)(v >> 8), p[3] = (uint8_t)v; }
inline uint32_t crc32_of(const uint8_t* p, uint64_t n) {
    uint32_t r = 0xFFFFFFFFu;
    for (uint64_t i = 0; i < n; ++i) r = crc_raw_bytes(r, p[i], 1u);
    return r ^ 0xFFFFFFFFu;
}
}  // namespace manifest_detail

// rows: null, or at least rows_cap entries (fewer than the manifest's blocks is refused).  why: "[manifest-error] ...".
inline int manifest_parse(const uint8_t* m, uint64_t size, lacx_manifest_info* info, lacx_block_digest* rows, uint32_t rows_cap,
                          std::string& why) {
    using namespace manifest_detail;
    auto fail = [&](const std::string& text) {
        why = "[manifest-error] " + text;
        return LACX_E_INVALID;
    };
    if (!m || size < kManifestFixed) return fail("short input");
    if (std::memcmp(m, "LACM", 4) != 0) return fail("wrong magic");
    if (m[4] != 1) return fail("unsupported version: " + std::to_string((int)m[4]));
    lacx_manifest_info f{};
    f.channels = m[5];
    f.bit_depth = m[6];
    f.sample_rate = mget32(m + 8);
    f.frames = ((uint64_t)mget32(m + 12) << 32) | mget32(m + 16);
    f.blocks = mget32(m + 20);
    f.data_crc32 = mget32(m + 24);
    if (size != kManifestFixed + 8ull * f.blocks) return fail("size is not 32 + 8 * blocks");
    if (mget32(m + size - 4) != crc32_of(m, size - 4)) return fail("checksum of the manifest itself differs");
    if (f.channels != 1 && f.channels != 2) return fail("unsupported channel count: " + std::to_string((int)f.channels));
    if (f.bit_depth != 16 && f.bit_depth != 24) return fail("unsupported bit depth: " + std::to_string((int)f.bit_depth));
    if (f.sample_rate != 44100 && f.sample_rate != 48000 && f.sample_rate != 96000 && f.sample_rate != 192000)
        return fail("unsupported sample rate: " + std::to_string(f.sample_rate));
    if (m[7] != 0) return fail("reserved byte is not zero");
    if (f.blocks == 0) return fail("no blocks");
    if (rows && rows_cap < f.blocks) return fail("rows array holds " + std::to_string(rows_cap) + " entries, the manifest " + std::to_string(f.blocks));
    const uint32_t align = (uint32_t)f.channels * (f.bit_depth / 8u);
    uint64_t sum = 0;
    uint32_t all = 0;
    for (uint32_t b = 0; b < f.blocks; ++b) {
        const uint32_t n = mget32(m + kManifestRowsAt + 8ull * b), c = mget32(m + kManifestRowsAt + 8ull * b + 4);
        if (n == 0 || n > kManifestMaxRow) return fail("block " + std::to_string(b) + " has " + std::to_string(n) + " frames");
        if (b + 1 < f.blocks && n < kManifestMinRow) return fail("block " + std::to_string(b) + " is not the last and has " + std::to_string(n) + " frames");
        sum += n;
        all = b ? crc32_combine(all, c, (unsigned long long)n * align) : c;
    }
    if (sum != f.frames) return fail("rows hold " + std::to_string(sum) + " frames, the header says " + std::to_string(f.frames));
    if (all != f.data_crc32) return fail("data_crc32 is not the combination of the rows");
    if (info) *info = f;
    for (uint32_t b = 0; rows && b < f.blocks; ++b)
        rows[b] = lacx_block_digest{mget32(m + kManifestRowsAt + 8ull * b), mget32(m + kManifestRowsAt + 8ull * b + 4), 0, 0};
    return LACX_OK;
}

// The manifest of digest d with its `count` rows; refuses what manifest_parse would refuse.
inline int manifest_build(const lacx_digest& d, const lacx_block_digest* rows, uint32_t count, std::vector<uint8_t>& out, std::string& why) {
    using namespace manifest_detail;
    for (uint32_t b = 0; b < count; ++b)
        if (rows[b].code != 0) {
            why = "manifest needs every block's digest: block " + std::to_string(b) + " is lost";
            return LACX_E_INVALID;
        }
    out.assign((size_t)(kManifestFixed + 8ull * count), 0);
    uint8_t* m = out.data();
    std::memcpy(m, "LACM", 4);
    m[4] = 1, m[5] = d.channels, m[6] = d.bit_depth;
    mput32(m + 8, d.sample_rate);
    mput32(m + 12, (uint32_t)(d.frames >> 32)), mput32(m + 16, (uint32_t)d.frames);
    mput32(m + 20, count);
    mput32(m + 24, d.data_crc32);
    for (uint32_t b = 0; b < count; ++b) mput32(m + kManifestRowsAt + 8ull * b, rows[b].frames), mput32(m + kManifestRowsAt + 8ull * b + 4, rows[b].crc32);
    mput32(m + out.size() - 4, crc32_of(m, out.size() - 4));
    const int rc = manifest_parse(m, out.size(), nullptr, nullptr, 0, why);
    if (rc != LACX_OK) out.clear();
    return rc;
}

// The rows of a decoded item: every block's frames from the stream's table, its fault code where it has one, and where it
// decoded its finished CRC-32.  raw: the words the device summed, the item's first block's first.
inline void rows_of_decoded(const uint8_t* lac, int version, uint32_t blocks, uint32_t channels, uint32_t bit_depth,
                            const std::vector<lacx_block_fault>& faults, const uint32_t* raw, std::vector<lacx_block_digest>& rows) {
    const uint32_t align = channels * (bit_depth / 8u);
    rows.assign(blocks, lacx_block_digest{});
    for (uint32_t b = 0; b < blocks; ++b) rows[b].frames = row_frames(lac, version, b);
    for (const lacx_block_fault& f : faults) rows[f.block].code = f.code;
    for (uint32_t b = 0; b < blocks; ++b)
        if (!rows[b].code) rows[b].crc32 = crc_finish(raw[b], (unsigned long long)rows[b].frames * align);
}

// The rows of a source item of `frames` frames on a regular grid of `grid` frames: nb blocks, the last the remainder.
inline void rows_of_source(unsigned long long frames, uint32_t grid, uint32_t nb, uint32_t channels, uint32_t bit_depth, const uint32_t* raw,
                           std::vector<lacx_block_digest>& rows) {
    const uint32_t align = channels * (bit_depth / 8u);
    rows.assign(nb, lacx_block_digest{});
    for (uint32_t b = 0; b < nb; ++b) {
        rows[b].frames = b + 1u < nb ? grid : (uint32_t)(frames - (unsigned long long)grid * b);
        rows[b].crc32 = crc_finish(raw[b], (unsigned long long)rows[b].frames * align);
    }
}

}  // namespace lacx
