// crc32_core.h -- CRC-32 (zlib / ISO-HDLC: reflected polynomial 0xEDB88320, init and final xor 0xFFFFFFFF) in the form
// the digest kernel needs (k_digest.hip, digest_core.h): as arithmetic in GF(2)[x] mod P, so that the pieces of a message
// can be digested in any order and added up.  In the reflected representation bit 31 of a word is x^0 and bit 0 is x^31.
//   raw(M)      the CRC register after the bytes M, starting from 0, without the final xor: M(x) * x^32 mod P
//   shift(r, n) r * x^(8n) mod P: what r becomes when n more bytes of zeros follow
//   raw(p_0 .. p_k) = XOR_i shift(raw(p_i), bytes behind piece i)
//   crc32(M)    = raw(M) ^ shift(0xFFFFFFFF, |M|) ^ 0xFFFFFFFF
// P is primitive (x^(2^32 - 1) = 1 and no smaller exponent: not for any of the cofactors 3, 5, 17, 257, 65537), and 8 is
// coprime to 2^32 - 1, so a distance in bytes may be reduced mod 2^32 - 1.  No carry-less multiply instruction is assumed:
// one multiply is 32 shift / xor steps.  Host and device, no HIP types (tests/native/sim_digest.cpp compiles it with g++).
#pragma once
#include <cstdint>

#ifndef LACX_HDF
#if defined(__HIPCC__)
#define LACX_HDF __host__ __device__ __forceinline__
#else
#define LACX_HDF inline
#endif
#endif

namespace lacx {

constexpr uint32_t kCrcPoly = 0xEDB88320u;
constexpr uint32_t kCrcOne = 0x80000000u;  // x^0

// one step of the register: r * x mod P
LACX_HDF constexpr uint32_t crc_step(uint32_t r) { return (r >> 1) ^ (kCrcPoly & (0u - (r & 1u))); }

// a * b mod P
LACX_HDF constexpr uint32_t crc_mul(uint32_t a, uint32_t b) {
    uint32_t p = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int i = 0; i < 32; ++i) {
        p ^= b & (0u - (a >> 31));  // the coefficient of x^i in a
        a <<= 1;
        b = crc_step(b);
    }
    return p;
}

// x^(8 * 2^i) for a distance's bit i, and per sample format (index: crc_format) x^(8 * unit_bytes * 2^level): the
// factors of the kernel's tree over the 64 units of a wave
struct CrcTables {
    uint32_t pow8[32];
    uint32_t tree[4][6];
};
constexpr uint32_t kDigestUnitFrames = 4;  // frames per unit (digest_core.h)
LACX_HDF constexpr uint32_t crc_format(int channels, int bit_depth) { return (bit_depth == 24 ? 2u : 0u) + (channels == 2 ? 1u : 0u); }
constexpr CrcTables crc_make_tables() {
    CrcTables t{};
    uint32_t p = kCrcOne;
    for (int i = 0; i < 8; ++i) p = crc_step(p);  // x^8
    for (int i = 0; i < 32; ++i) {
        t.pow8[i] = p;
        p = crc_mul(p, p);
    }
    for (int ch = 1; ch <= 2; ++ch) {
        for (int bd = 16; bd <= 24; bd += 8) {
            const uint32_t bytes = kDigestUnitFrames * (uint32_t)ch * (uint32_t)(bd / 8);
            uint32_t q = kCrcOne;
            for (int i = 0; i < 32; ++i)
                if ((bytes >> i) & 1u) q = crc_mul(q, t.pow8[i]);
            for (int level = 0; level < 6; ++level) {
                t.tree[crc_format(ch, bd)][level] = q;
                q = crc_mul(q, q);
            }
        }
    }
    return t;
}
constexpr CrcTables kCrcTables = crc_make_tables();

// a byte distance mod 2^32 - 1
LACX_HDF constexpr uint32_t crc_reduce(unsigned long long n) {
    n = (n >> 32) + (n & 0xFFFFFFFFull);  // 2^32 = 1
    n = (n >> 32) + (n & 0xFFFFFFFFull);
    return n == 0xFFFFFFFFull ? 0u : (uint32_t)n;
}

// r * x^(8n) mod P: square-and-multiply over the table, one multiply per set bit of the reduced distance
LACX_HDF constexpr uint32_t crc_shift(uint32_t r, unsigned long long n) {
    uint32_t d = crc_reduce(n);
    for (int i = 0; i < 32 && d; ++i, d >>= 1)
        if (d & 1u) r = crc_mul(r, kCrcTables.pow8[i]);
    return r;
}

// raw of up to four bytes held in the low `nbytes` bytes of w (little-endian: the lowest byte comes first in the
// message), continued from register r
LACX_HDF constexpr uint32_t crc_raw_bytes(uint32_t r, uint32_t w, uint32_t nbytes) {
    r ^= w;
    for (uint32_t i = 0; i < 8u * nbytes; ++i) r = crc_step(r);
    return r;
}

// the CRC-32 of the bytes whose raw value is `raw`
LACX_HDF constexpr uint32_t crc_finish(uint32_t raw, unsigned long long len) { return raw ^ crc_shift(0xFFFFFFFFu, len) ^ 0xFFFFFFFFu; }

// crc32(A || B) from crc32(A), crc32(B) and |B| (zlib's crc32_combine): the init terms of A || B and of A differ by the
// shift over B, which also carries A's final xor
LACX_HDF constexpr uint32_t crc32_combine(uint32_t crc_a, uint32_t crc_b, unsigned long long len_b) { return crc_shift(crc_a, len_b) ^ crc_b; }

// CRC-32 of the canonical 44-byte header of the WAV image the decoder writes (wav_header of api_decode.cpp; ref
// src/main.cpp:127-148): data_bytes = frames * channels * bit_depth / 8, below 2^32 - 36
LACX_HDF constexpr uint32_t crc32_wav_header(uint32_t channels, uint32_t bit_depth, uint32_t sample_rate, unsigned long long data_bytes) {
    const uint32_t align = channels * (bit_depth / 8u), data = (uint32_t)data_bytes, pad = data & 1u;
    const uint32_t words[11] = {0x46464952u /* RIFF */, 36u + data + pad, 0x45564157u /* WAVE */, 0x20746D66u /* fmt  */, 16u,
                                1u | (channels << 16), sample_rate, sample_rate * align, align | (bit_depth << 16),
                                0x61746164u /* data */, data};
    uint32_t r = 0xFFFFFFFFu;
    for (int i = 0; i < 11; ++i) r = crc_raw_bytes(r, words[i], 4u);
    return r ^ 0xFFFFFFFFu;
}

}  // namespace lacx
