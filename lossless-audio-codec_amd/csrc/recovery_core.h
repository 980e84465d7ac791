// recovery_core.h -- the per-thread code of the recovery data (lacx.h): Reed-Solomon erasure coding over
// GF(2^8) (polynomial 0x11D, generator 2) on four bytes packed in a 32-bit word, and the lane code of the slice CRC-32.
// Arithmetic in crc32_core.h fashion: shifts and xors, no lookup table, no LDS.  Host and device, no HIP types
// (k_recovery.hip runs it on the device, recovery_plan.h and tests/native/sim_recovery.cpp on the host).
//   xtime4(w)   every byte of w times 2
//   mul4(w, c)  every byte of w times the constant c: the XOR of the w * 2^b for the set bits b of c
// One combine computes out[o] = XOR_i M[o][i] * in[i] for a task's slices, a thread owning one word column: it forms the
// eight w * 2^b once per input word and XORs them into the accumulators of the outputs whose coefficient has bit b.  The
// coefficient does not depend on the column, so on the device it is a scalar value and its bit tests are uniform branches.
#pragma once
#include <cstdint>
#include <cstring>

#include "crc32_core.h"

#ifndef LACX_UNIFORM
#if defined(__HIP_DEVICE_COMPILE__)
#define LACX_UNIFORM(x) ((uint32_t)__builtin_amdgcn_readfirstlane((int)(x)))  // the same in every lane: keep it in an SGPR
#else
#define LACX_UNIFORM(x) ((uint32_t)(x))
#endif
#endif

namespace lacx {

LACX_HDF constexpr uint32_t gf_xtime4(uint32_t w) { return ((w & 0x7F7F7F7Fu) << 1) ^ (((w >> 7) & 0x01010101u) * 0x1Du); }

LACX_HDF constexpr uint32_t gf_mul4(uint32_t w, uint32_t c) {
    uint32_t acc = 0;
    for (int b = 0; b < 8; ++b) {
        if ((c >> b) & 1u) acc ^= w;
        w = gf_xtime4(w);
    }
    return acc;
}
LACX_HDF constexpr uint8_t gf_mul(uint8_t a, uint8_t b) { return (uint8_t)gf_mul4(a, b); }
// a^254 = 1 / a (a != 0)
LACX_HDF constexpr uint8_t gf_inv(uint8_t a) {
    uint8_t r = 1, s = a;
    for (int i = 1; i < 8; ++i) {
        s = gf_mul(s, s);  // a^(2^i)
        r = gf_mul(r, s);
    }
    return r;
}

// ---- task tables (filled by recovery_plan.h) -----------------------------------------------------------------------
// Every address is a byte offset into one arena, a multiple of 4.  A byte range whose CRC-32 is wanted:
struct CrcRange {
    unsigned long long at;
    uint32_t len;  // >= 1; the words of the range are ceil(len / 4): the arena holds all of the last one
    uint32_t pad;
};
// One combine: refs[in_at .. + nin) and refs[out_at .. + nout) are the slices' offsets, `words` dwords each; the
// coefficients of input i are the kTier bytes at mat + m_at + i * kTier (output o's at byte o; zero from nout on), kTier
// the task's tier: the smallest of 8 / 16 / 32 that holds nout.  wg0: the task's first workgroup in its tier's launch.
struct GfTask {
    uint32_t in_at, out_at, m_at, wg0;
    uint16_t nin, nout;
    uint32_t words;
};
constexpr uint32_t kGfThreads = 256;   // a workgroup's word columns
constexpr uint32_t kCrcThreads = 256;  // four waves, one range each
constexpr uint32_t kGfTiers = 3;
LACX_HDF constexpr uint32_t gf_tier_outs(uint32_t tier) { return 8u << tier; }
LACX_HDF constexpr uint32_t gf_tier_of(uint32_t nout) { return nout <= 8u ? 0u : nout <= 16u ? 1u : 2u; }

// One launch set (launch_recovery, kernels.h): k_gf_combine over the tasks of every tier that has some, then k_slice_crc
// over the ranges, which may lie in slices the tasks wrote.
struct RecoveryArgs {
    uint8_t* arena = nullptr;
    const GfTask* tasks = nullptr;  // tier by tier: tier's tasks are [tier_t0[tier], tier_t0[tier + 1]), tier_wgs[tier] workgroups
    uint32_t tier_t0[kGfTiers + 1] = {}, tier_wgs[kGfTiers] = {};
    const unsigned long long* refs = nullptr;
    const uint8_t* mat = nullptr;   // 4-byte aligned, like every m_at
    const CrcRange* ranges = nullptr;
    uint32_t nranges = 0;
    uint32_t* crc = nullptr;        // [nranges]
};

// The task of workgroup wg among tasks [t0, t1) of one tier (wg0 ascending, tasks[t0].wg0 == 0): a uniform search.
LACX_HDF uint32_t gf_task_of(const GfTask* tasks, uint32_t t0, uint32_t t1, uint32_t wg) {
    uint32_t lo = t0, hi = t1;  // tasks[lo].wg0 <= wg < tasks[hi].wg0
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (tasks[mid].wg0 <= wg) lo = mid;
        else hi = mid;
    }
    return lo;
}

// Word column `col` of task t (col < t.words is the caller's predicate): nothing but that column of the task's slices
// is read or written.
template <uint32_t kOuts>
LACX_HDF void gf_combine_column(const GfTask& t, const unsigned long long* refs, const uint8_t* mat, uint8_t* arena, uint32_t col) {
    uint32_t acc[kOuts];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (uint32_t o = 0; o < kOuts; ++o) acc[o] = 0;
    const uint32_t* coef = reinterpret_cast<const uint32_t*>(mat + t.m_at);
    const uint32_t nin = t.nin;
    uint32_t next = reinterpret_cast<const uint32_t*>(arena + refs[t.in_at])[col];
    for (uint32_t i = 0; i < nin; ++i) {
        uint32_t pw[8];
        pw[0] = next;
        if (i + 1u < nin) next = reinterpret_cast<const uint32_t*>(arena + refs[t.in_at + i + 1u])[col];  // in flight over the arithmetic
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int b = 1; b < 8; ++b) pw[b] = gf_xtime4(pw[b - 1]);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (uint32_t q = 0; q < kOuts / 4u; ++q) {
            const uint32_t four = LACX_UNIFORM(coef[i * (kOuts / 4u) + q]);  // the coefficients of outputs 4q .. 4q + 3
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
            for (uint32_t o = 0; o < 4u; ++o) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
                for (uint32_t b = 0; b < 8u; ++b)
                    if ((four >> (8u * o + b)) & 1u) acc[4u * q + o] ^= pw[b];
            }
        }
    }
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (uint32_t o = 0; o < kOuts; ++o)
        if (o < t.nout) reinterpret_cast<uint32_t*>(arena + refs[t.out_at + o])[col] = acc[o];
}

// ---- slice CRC: one wave per range ------------------------------------------------------------------------------------
// In the reflected representation a little-endian word IS its four bytes' polynomial, and a range of len bytes has
//   raw = XOR_j w_j * x^(8 * (len - 4j))        (the last word masked to the bytes the range holds)
// Lane l takes the words l, l + 64, ...: a wave reads 256 consecutive bytes per step, and the lane's sum is a Horner chain
// in x^(8 * 256), moved to the range's end by one shift.  The XOR over the 64 lanes is the range's raw value.
constexpr uint32_t kCrcX256 = crc_shift(kCrcOne, 256);
LACX_HDF uint32_t slice_crc_lane(const uint8_t* arena, const CrcRange& r, uint32_t lane) {
    const uint32_t nw = (r.len + 3u) / 4u;
    if (lane >= nw) return 0u;
    const uint32_t* w = reinterpret_cast<const uint32_t*>(arena + r.at);
    uint32_t acc = 0, j = lane;
    for (; j < nw; j += 64u) {
        uint32_t v = w[j];
        const uint32_t held = r.len - 4u * j;  // bytes of the range from this word on
        if (held < 4u) v &= (1u << (8u * held)) - 1u;
        acc = crc_mul(acc, kCrcX256) ^ v;
    }
    j -= 64u;  // the lane's last word
    return crc_shift(acc, (unsigned long long)(r.len - 4u * j));
}

}  // namespace lacx
