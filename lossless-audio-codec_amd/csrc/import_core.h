// import_core.h -- the per-thread code of the import pass (k_import of k_import.hip) and the float-to-sample rule the
// verify form shares with it (verify_core.h).  The import pass stands in front of the encoder's front kernels: it rewrites
// device-resident PCM in one of the tensor layouts -- planar int16, planar float32, interleaved float32 -- into one of the
// layouts those kernels read (interleaved int16 at depth 16, packed interleaved int24 at depth 24), in a buffer the encoder
// owns, and validates every float on the way.  Written like decode_core.h / verify_core.h: the same source compiles into
// the gfx950 kernel and into a host program the tests run under AddressSanitizer / UBSan (tests/native/sim_import.cpp);
// every load of the source and every store of the destination is in here, and the twin hands it heap blocks of exactly
// frames * channels * element size bytes at every base alignment a layout permits.
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

// lacx_pcm.layout codes of the tensor layouts (include/lacx.h: LACX_PCM_PLANAR_I16 ...); 0..2: analyze_core.h
enum : int { PCM_PLANAR_I16 = 16, PCM_PLANAR_F32 = 17, PCM_INTERLEAVED_F32 = 18 };

constexpr uint32_t kImportQuad = 4;        // frames per thread
constexpr uint32_t kImportThreads = 256;   // threads per workgroup
constexpr uint32_t kImportUnitFrames = kImportQuad * kImportThreads;  // frames per unit: one workgroup, inside one item

// A float32 sample x of a stream of depth b stands for the integer x * 2^(b-1), the inverse of LACX_SAMPLE_F32.  Decided
// on the bits of x alone -- no floating-point instruction, so neither fast-math nor a denormal mode can change the
// answer: 0 valid (v = the sample), 1 the product is an integer outside [-2^(b-1), 2^(b-1) - 1], 2 anything else (a
// fraction, a denormal, an infinity, a NaN).  For 1 and 2, v = the product rounded to nearest (ties to even) and
// saturated to int32, INT32_MIN for a NaN: what the verify form reports as the source's value.
LACX_HDF int f32_to_pcm(uint32_t bits, int depth, int32_t& v) {
    const uint32_t e = (bits >> 23) & 0xFFu, frac = bits & 0x7FFFFFu;
    const bool neg = (bits >> 31) != 0u;
    if (e == 255u) {
        v = frac || neg ? INT32_MIN : INT32_MAX;
        return 2;
    }
    if (e == 0u) {  // zero (either sign), or a denormal: below 2^-102 even at depth 24
        v = 0;
        return frac ? 2 : 0;
    }
    const int sh = (int)e - 127 + (depth - 1) - 23;  // |product| = m * 2^sh
    const uint32_t m = frac | 0x800000u;
    long long mag;
    bool exact = true;
    if (sh >= 8) {
        mag = 1ll << 31;  // m >= 2^23: at least 2^31
    } else if (sh >= 0) {
        mag = (long long)m << sh;
    } else if (sh < -24) {
        mag = 0;  // below one half
        exact = false;
    } else {
        const uint32_t r = (uint32_t)-sh, q = m >> r, rem = m & ((1u << r) - 1u), half = 1u << (r - 1u);
        exact = rem == 0u;
        mag = (long long)q + (rem > half || (rem == half && (q & 1u)) ? 1 : 0);
    }
    long long s = neg ? -mag : mag;
    if (s > (long long)INT32_MAX) s = INT32_MAX;
    if (s < (long long)INT32_MIN) s = INT32_MIN;
    v = (int32_t)s;
    if (!exact) return 2;
    const long long lim = 1ll << (depth - 1);
    return s < -lim || s > lim - 1 ? 1 : 0;
}

// One source of an import job.  dst: 16-byte aligned, frames * channels * (bit_depth / 8) bytes, interleaved int16
// (depth 16) or packed interleaved int24 (depth 24).
struct ImportItem {
    const void* src0;  // planar: left; interleaved: the frames
    const void* src1;  // planar stereo: right
    void* dst;
    unsigned long long frames;
    uint32_t layout;   // PCM_PLANAR_I16 / PCM_PLANAR_F32 / PCM_INTERLEAVED_F32
    uint8_t channels, bit_depth, pad[2];
};
// What an item's validation leaves: per channel the lowest invalid frame * 2 + (1: not an exact sample, 0: an integer
// outside the bit depth); all ones: none.
struct ImportBad {
    unsigned long long key[2];
};
constexpr unsigned long long kImportClean = ~0ull;

// The job: a table of items with the prefix sums of their unit counts, or -- one item, the common case -- the item itself
// in the kernel arguments (table == nullptr: no upload, no look-up).
struct ImportJob {
    const ImportItem* table;
    const unsigned long long* unit_off;  // [nitems + 1]
    uint32_t nitems, pad;
    unsigned long long total_units;
    ImportItem single;
};

namespace import_detail {
// four 24-bit samples as three little-endian dwords
LACX_HDF void pack24x4(const int32_t* s, uint32_t* w) {
    const uint32_t a = (uint32_t)s[0] & 0xFFFFFFu, b = (uint32_t)s[1] & 0xFFFFFFu, c = (uint32_t)s[2] & 0xFFFFFFu,
                   d = (uint32_t)s[3] & 0xFFFFFFu;
    w[0] = a | (b << 24);
    w[1] = (b >> 8) | (c << 16);
    w[2] = (c >> 16) | (d << 8);
}
// four consecutive elements of a row: one wide load where the row's base allows it (uniform per item), else one load per
// element; `n` < 4 elements (the item's last quad) always one by one
LACX_HDF void load_i16x4(const int16_t* p, bool wide, uint32_t n, int32_t* out) {
    if (n == 4u && wide) {
        int16_t t[4];
        __builtin_memcpy(t, __builtin_assume_aligned(p, 8), 8);
        out[0] = t[0], out[1] = t[1], out[2] = t[2], out[3] = t[3];
    } else {
#pragma unroll
        for (uint32_t i = 0; i < 4u; ++i)
            if (i < n) out[i] = p[i];
    }
}
LACX_HDF void load_u32x4(const uint32_t* p, bool wide, uint32_t n, uint32_t* out) {
    if (n == 4u && wide) {
        __builtin_memcpy(out, __builtin_assume_aligned(p, 16), 16);
    } else {
#pragma unroll
        for (uint32_t i = 0; i < 4u; ++i)
            if (i < n) out[i] = p[i];
    }
}
}  // namespace import_detail

// One thread's work: frames f0 .. f0 + 3 of an item (f0 a multiple of 4, below it.frames).  Loads:
//   planar int16        8 bytes per channel where the row's base is 8-byte aligned, else int16 loads (an odd-length left
//                       row leaves the right row 2-byte aligned only)
//   planar float32      16 bytes per channel where the row's base is 16-byte aligned, else dword loads
//   interleaved float32 16 (mono) or 32 (stereo) bytes where the base is 16-byte aligned, else dword loads
// and the item's partial last quad element by element: nothing outside [src, src + frames * channels * element size) is
// read.  A float that is no sample of the item's depth is stored as 0 and lowers key_l / key_r (ImportBad).  Stores: the
// quad's 8 / 16 (int16) or 12 / 24 (int24) bytes as dwords at their natural alignment, the partial quad as elements /
// bytes: nothing outside [dst, dst + frames * channels * bit_depth / 8) is written.
LACX_HDF void import_quad(const ImportItem& it, unsigned long long f0, unsigned long long& key_l, unsigned long long& key_r) {
    using namespace import_detail;
    const uint32_t nf = it.frames - f0 >= 4u ? 4u : (uint32_t)(it.frames - f0);
    const bool stereo = it.channels == 2;
    const int depth = it.bit_depth;
    int32_t l[4] = {0, 0, 0, 0}, r[4] = {0, 0, 0, 0};
    if (it.layout == (uint32_t)PCM_PLANAR_I16) {
        load_i16x4(static_cast<const int16_t*>(it.src0) + f0, ((uintptr_t)it.src0 & 7u) == 0, nf, l);
        if (stereo) load_i16x4(static_cast<const int16_t*>(it.src1) + f0, ((uintptr_t)it.src1 & 7u) == 0, nf, r);
    } else {
        uint32_t bl[4] = {0, 0, 0, 0}, br[4] = {0, 0, 0, 0};
        const bool wide0 = ((uintptr_t)it.src0 & 15u) == 0;
        if (it.layout == (uint32_t)PCM_PLANAR_F32 || !stereo) {
            load_u32x4(static_cast<const uint32_t*>(it.src0) + f0, wide0, nf, bl);
            if (stereo) load_u32x4(static_cast<const uint32_t*>(it.src1) + f0, ((uintptr_t)it.src1 & 15u) == 0, nf, br);
        } else {
            const uint32_t* p = static_cast<const uint32_t*>(it.src0) + 2u * f0;
            uint32_t w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            load_u32x4(p, wide0, nf >= 2u ? 4u : 2u * nf, w);
            if (nf > 2u) load_u32x4(p + 4, wide0, 2u * nf - 4u, w + 4);
#pragma unroll
            for (uint32_t i = 0; i < 4u; ++i) bl[i] = w[2u * i], br[i] = w[2u * i + 1u];
        }
#pragma unroll
        for (uint32_t i = 0; i < 4u; ++i) {
            if (i >= nf) continue;
            int32_t v;
            int kind = f32_to_pcm(bl[i], depth, v);
            l[i] = kind ? 0 : v;
            if (kind) {
                const unsigned long long k = 2u * (f0 + i) + (kind == 2 ? 1u : 0u);
                key_l = k < key_l ? k : key_l;
            }
            if (stereo) {
                kind = f32_to_pcm(br[i], depth, v);
                r[i] = kind ? 0 : v;
                if (kind) {
                    const unsigned long long k = 2u * (f0 + i) + (kind == 2 ? 1u : 0u);
                    key_r = k < key_r ? k : key_r;
                }
            }
        }
    }
    int32_t s[8];  // the quad's samples in stream order
    const uint32_t ns = stereo ? 2u * nf : nf;
#pragma unroll
    for (uint32_t i = 0; i < 4u; ++i) {
        if (stereo) s[2u * i] = l[i], s[2u * i + 1u] = r[i];
        else s[i] = l[i], s[4u + i] = 0;
    }
    if (depth == 16) {
        int16_t* d = static_cast<int16_t*>(it.dst) + f0 * (stereo ? 2u : 1u);
        if (nf == 4u) {
            uint32_t w[4];
#pragma unroll
            for (uint32_t i = 0; i < 4u; ++i) w[i] = ((uint32_t)s[2u * i] & 0xFFFFu) | ((uint32_t)s[2u * i + 1u] << 16);
            if (stereo) __builtin_memcpy(__builtin_assume_aligned(d, 16), w, 16);
            else __builtin_memcpy(__builtin_assume_aligned(d, 8), w, 8);
        } else {
#pragma unroll
            for (uint32_t i = 0; i < 6u; ++i)
                if (i < ns) d[i] = (int16_t)s[i];
        }
    } else {
        uint8_t* d = static_cast<uint8_t*>(it.dst) + 3u * f0 * (stereo ? 2u : 1u);
        if (nf == 4u) {
            uint32_t w[6];
            pack24x4(s, w);
            if (stereo) {
                pack24x4(s + 4, w + 3);
                __builtin_memcpy(__builtin_assume_aligned(d, 8), w, 24);
            } else {
                __builtin_memcpy(__builtin_assume_aligned(d, 4), w, 12);
            }
        } else {
#pragma unroll
            for (uint32_t i = 0; i < 6u; ++i) {
                if (i < ns) {
                    const uint32_t v = (uint32_t)s[i];
                    d[3u * i] = (uint8_t)v, d[3u * i + 1u] = (uint8_t)(v >> 8), d[3u * i + 2u] = (uint8_t)(v >> 16);
                }
            }
        }
    }
}

// A mono planar int16 source on a 4-byte aligned address IS interleaved int16 mono: it needs no import.
LACX_HDF bool import_is_alias(uint32_t layout, uint32_t channels, const void* src0) {
    return layout == (uint32_t)PCM_PLANAR_I16 && channels == 1u && ((uintptr_t)src0 & 3u) == 0;
}

}  // namespace lacx
