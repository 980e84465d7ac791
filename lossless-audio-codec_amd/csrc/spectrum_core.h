// spectrum_core.h -- the per-thread code of the spectrum job (k_spectrum of k_spectrum.hip): the banded long-term power
// spectrum of the final samples of an item, per row of 16384 frames.  This file is the only statement of the definition
// in code (lacx.h and DESIGN §6b state it in words).
//   N: the window length, 256 .. 4096, a power of two; the hop is H = N / 2.  Window k of an item covers frames
//   [k H, k H + N), zeros at and behind the item's end, k = 0 .. ceil(frames / H) - 1.
//   z[n] = w[n] * (double)l[n] + i w[n] * (double)r[n] (mono: a zero imaginary part), w the periodic Hann window out of the
//   plan's table: one rounding per product.  Z = the N-point DFT of z; L_k = (Z_k + conj Z_{N-k}) / 2,
//   R_k = (Z_k - conj Z_{N-k}) / 2i; the one-sided power of bin k is c_k |X_k|^2, c_0 = c_{N/2} = 1, c_k = 2 otherwise;
//   bin k < N / 2 belongs to band k / (N / 128), the Nyquist bin to band 63; a row is the sum of the band powers of the
//   windows whose first frame lies in its 16384 frames.
// The transform is a radix-2 decimation-in-frequency FFT in place: natural order in, bit-reversed order out, log2 N stages
// of N / 2 butterflies with halves h = N / 2, N / 4 .. 1.  Butterfly b of the stage with half h works on i = (b / h) 2 h +
// b % h and j = i + h with the twiddle t = (c, s) = table[(b % h) (N / 2 h)] = (cos, -sin)(2 pi (b % h) / 2 h):
//   a' = a + b                                 (two additions)
//   d  = a - b                                 (two subtractions)
//   b' = (fma(d.re, c, -(d.im s)), fma(d.re, s, d.im c))
// The butterflies of a stage touch disjoint pairs, so their order inside a stage does not matter: the device runs them
// on 256 threads with a barrier between stages, the twin one after the other.  Every operation and its order are fixed
// here -- which multiply-adds are fused (each written as __builtin_fma; the translation units that include this file are
// compiled with -ffp-contract=off, so nothing else is), the bin order inside a band (ascending, the Nyquist bin last),
// the window order inside a row (ascending) -- and the device never evaluates a sine or cosine: device and twin read the
// same tables.  A row is therefore the same bits on the device and on the twin, in any batch and at any place in a job.
// Where a point lies in the two arrays of N doubles (re, im) is sp_at: a layout, not part of the definition.
// Written like truepeak_core.h: the same source compiles into the gfx950 kernel and into a host program the tests run
// under AddressSanitizer / UBSan (tests/native/sim_spectrum.cpp).
#pragma once
#include <cstdint>

#include "lacx.h"
#include "stats_core.h"

namespace lacx {

static_assert(sizeof(lacx_spectrum_row) == 16u * kSpBands, "the plan lays the rows out 1024 bytes apart");
static_assert(kSpMinLog >= 7u && (1u << kSpMinLog) / (2u * kSpBands) >= 1u, "a band holds at least one bin");
static_assert(kSpRowFrames % (1u << (kSpMaxLog - 1u)) == 0, "a row holds whole hops");

// The place of point i in the LDS arrays: a swizzle inside every run of 64 points (k_spectrum.hip's header says what it
// is for).  The second 16 of every 32 points are mirrored (low four bits inverted), and the second 32 of every 64 swap
// their halves.  A bijection on [0, N) for every N that is a multiple of 64.
LACX_HDF constexpr uint32_t sp_at(uint32_t i) { return i ^ ((i & 16u) ? 15u : 0u) ^ ((i & 32u) ? 16u : 0u); }

// the low `bits` bits of k in reverse order
LACX_HDF constexpr uint32_t sp_rev(uint32_t k, uint32_t bits) {
    k = ((k >> 1) & 0x55555555u) | ((k & 0x55555555u) << 1);
    k = ((k >> 2) & 0x33333333u) | ((k & 0x33333333u) << 2);
    k = ((k >> 4) & 0x0F0F0F0Fu) | ((k & 0x0F0F0F0Fu) << 4);
    k = ((k >> 8) & 0x00FF00FFu) | ((k & 0x00FF00FFu) << 8);
    k = (k >> 16) | (k << 16);
    return k >> (32u - bits);
}

// Unit u of window k: frames k H + 4 u .. + 3 of the item through stats_load_source (zeros where the item has none), times
// the window, into points 4 u .. 4 u + 3.  key as stats_load_source.
LACX_HDF void sp_load_unit(const SpItem& it, uint32_t logn, unsigned long long k, uint32_t u, const double* __restrict__ window,
                           unsigned long long& key, double* re, double* im) {
    const unsigned long long f0 = (k << (logn - 1u)) + 4u * u;
    int32_t l[4] = {0, 0, 0, 0}, r[4] = {0, 0, 0, 0};
    if (f0 < it.frames) {
        const uint32_t nf = it.frames - f0 >= 4u ? 4u : (uint32_t)(it.frames - f0);
        stats_load_source(f0, nf, it.channels, it.bit_depth, it.data0, it.data1, it.layout, key, l, r);
    }
    const bool stereo = it.channels == 2;
#pragma unroll
    for (uint32_t i = 0; i < 4u; ++i) {
        const double w = window[4u * u + i];
        re[sp_at(4u * u + i)] = w * (double)l[i];
        im[sp_at(4u * u + i)] = stereo ? w * (double)r[i] : 0.0;
    }
}

// Butterfly b (0 .. N / 2 - 1) of the stage with half h (a power of two, N / 2 .. 1).
LACX_HDF void sp_butterfly(uint32_t logn, uint32_t h, uint32_t b, const double* __restrict__ twiddle, double* re, double* im) {
    const uint32_t q = b & (h - 1u), i = ((b - q) << 1) + q, j = i + h;
    const uint32_t t = q * ((1u << (logn - 1u)) / h);
    const double c = twiddle[2u * t], s = twiddle[2u * t + 1u];
    const uint32_t pi = sp_at(i), pj = sp_at(j);
    const double ar = re[pi], ai = im[pi], br = re[pj], bi = im[pj];
    const double dr = ar - br, di = ai - bi;
    re[pi] = ar + br;
    im[pi] = ai + bi;
    re[pj] = __builtin_fma(dr, c, -(di * s));
    im[pj] = __builtin_fma(dr, s, di * c);
}

// The one-sided power of bin k (0 .. N / 2) of channel c out of the transformed window.
LACX_HDF double sp_bin_power(uint32_t logn, uint32_t c, uint32_t k, const double* re, const double* im) {
    const uint32_t n = 1u << logn;
    const uint32_t pk = sp_at(sp_rev(k, logn)), pn = sp_at(sp_rev((n - k) & (n - 1u), logn));
    const double zr = re[pk], zi = im[pk], yr = re[pn], yi = im[pn];  // Z_k, Z_{N-k}
    const double xr = c == 0u ? 0.5 * (zr + yr) : 0.5 * (zi + yi);
    const double xi = c == 0u ? 0.5 * (zi - yi) : 0.5 * (yr - zr);
    const double p = __builtin_fma(xr, xr, xi * xi);
    return k == 0u || k == n / 2u ? p : 2.0 * p;
}

// The power of band `band` of channel c of one window: its bins in ascending order, the Nyquist bin behind band 63's.
LACX_HDF double sp_band_power(uint32_t logn, uint32_t c, uint32_t band, const double* re, const double* im) {
    const uint32_t per = (1u << logn) / (2u * kSpBands);
    double s = sp_bin_power(logn, c, band * per, re, im);
    for (uint32_t t = 1; t < per; ++t) s = s + sp_bin_power(logn, c, band * per + t, re, im);
    if (band == kSpBands - 1u) s = s + sp_bin_power(logn, c, kSpBands * per, re, im);
    return s;
}

// The windows of row r of an item: [first, end).
LACX_HDF void sp_row_windows(const SpItem& it, uint32_t logn, uint32_t r, unsigned long long& first, unsigned long long& end) {
    const unsigned long long per = kSpRowFrames >> (logn - 1u);
    first = (unsigned long long)r * per;
    end = first + per < it.windows ? first + per : it.windows;
}

}  // namespace lacx
