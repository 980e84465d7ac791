"""Seeded corpora for the software x87 model (csrc/x87.h) and for k_levinson, with their expectations.

Operations: about 2^20 operand pairs (a, b) and one int64 each.  Expected values come from the machine's long double
(numpy.longdouble, asserted to be the x87 extended format), never from x87.h.  Nothing is filtered out after generation:
a zero divisor is prevented where operands are made, and every element is compared for all seven operations.

Tables: [13] int64 autocorrelation tables, from signals through the oracle's autocorr and synthetic ones, with
oracle.levinson_q15 for the five candidate orders as the expectation; placements() lays them out as launch sets for
k_levinson (blocks x 16 slots, stream shapes, need_probe words) and says which LpcSets the kernel must write.

A zero is compared by its significand alone: x87.h gives a zero the exponent -(2^20), and neither xf_lt nor xf_to_q15 nor
any operation on it looks at its sign.
"""
from __future__ import annotations

import functools
from collections import namedtuple

import numpy as np

LD = np.longdouble
TOP = 1 << 63
ALL1 = (1 << 64) - 1
ZERO_E = -(1 << 20)
OPS = ("add", "sub", "mul", "div", "from_i64")  # raw (m, e, s) results, in this order
INT_OPS = ("lt", "q15")
CANDS = (4, 6, 8, 10, 12)
MAX_BLOCK = 16384
PROBE = 256
FULL_COMPARE_LIMIT = 4096
SLOTS = 16

_RAW = np.dtype([("m", "<u8"), ("se", "<u2"), ("pad", "V6")])


def assert_long_double_is_x87():
    fi = np.finfo(LD)
    assert LD().itemsize == 16 and fi.nmant == 63 and fi.maxexp == 16384, "numpy.longdouble is not the x87 extended format here"
    one = LD(1)
    assert one + np.ldexp(one, -63) != one and one + np.ldexp(one, -64) == one


# ---------------------------------------------------------------------------------------------------------------------
# long double <-> (m, e, s)
# ---------------------------------------------------------------------------------------------------------------------
def ld_make(m, e, s):
    """long double array of value (-1)^s * m * 2^(e - 63); m == 0 gives a zero."""
    m = np.asarray(m, dtype=np.uint64)
    raw = np.zeros(m.shape, dtype=_RAW)
    raw["m"] = m
    be = np.where(m == 0, 0, np.asarray(e, dtype=np.int64) + 16383)
    assert ((be >= 0) & (be < 32767)).all()
    raw["se"] = (be | (np.asarray(s, dtype=np.int64) << 15)).astype(np.uint16)
    return raw.view(LD)


def ld_parts(x):
    """(m, e, s) of a long double array; zeros as x87.h writes them (m 0, e -(2^20))."""
    x = np.ascontiguousarray(x, dtype=LD)
    raw = x.view(_RAW)
    m = raw["m"].copy()
    se = raw["se"].astype(np.int64)
    assert ((m == 0) | ((m >> np.uint64(63)) == 1)).all(), "denormal in the corpus"
    assert ((se & 0x7FFF) != 0x7FFF).all(), "inf / nan in the corpus"
    e = np.where(m == 0, ZERO_E, (se & 0x7FFF) - 16383).astype(np.int32)
    s = (se >> 15).astype(np.uint32)
    return m, e, s


# ---------------------------------------------------------------------------------------------------------------------
# operations corpus
# ---------------------------------------------------------------------------------------------------------------------
OpsCorpus = namedtuple("OpsCorpus", "n in_m in_e in_s in_i classes")


def _rnd(rng, n, elo=-70, ehi=70):
    """tests/native/test_x87.cpp's rnd_ld: random significand (sometimes masked), moderate exponent, random sign."""
    m = rng.integers(0, 1 << 64, n, dtype=np.uint64) | np.uint64(TOP)
    mode = rng.integers(0, 8, n)
    m = np.where(mode == 0, m & np.uint64(0xFFFFFFFF00000000), m)
    m = np.where(mode == 1, m & np.uint64(0xFFFFFFFFFFFFF800), m)
    m = np.where(mode == 2, np.uint64(TOP), m)
    return m, rng.integers(elo, ehi, n).astype(np.int32), rng.integers(0, 2, n).astype(np.uint32)


def _u64(vals):
    return np.array([int(v) & ALL1 for v in vals], dtype=np.uint64)


def _base(rng, n):
    am, ae, as_ = _rnd(rng, n)
    bm, be, bs = _rnd(rng, n)
    i = np.arange(n)
    x = ld_make(am, ae, as_)
    # near-equal operands
    sel = i % 5 == 0
    k = rng.integers(-3, 4, n).astype(LD)
    j = rng.integers(0, 70, n)
    near = x * (LD(1) + np.ldexp(k, -j))
    nm, ne, ns = ld_parts(near)
    bm, be, bs = np.where(sel, nm, bm), np.where(sel, ne, be), np.where(sel, ns, bs)
    # the same value some binades down
    sel = i % 11 == 0
    bm, be, bs = np.where(sel, am, bm), np.where(sel, ae - rng.integers(0, 140, n).astype(np.int32), be), np.where(sel, as_, bs)
    # exponent distances around the 64- and 128-bit alignment borders, either way round
    sel = i % 13 == 0
    dist = np.array([0, 1, 62, 63, 64, 65, 66, 126, 127, 128, 129, 130], dtype=np.int32)[rng.integers(0, 12, n)]
    dist = np.where(rng.integers(0, 2, n) == 1, dist, -dist)
    ym, _, ys = _rnd(rng, n)
    bm, be, bs = np.where(sel, ym, bm), np.where(sel, ae + dist, be), np.where(sel, ys, bs)
    # zero operands (the divisor stays non-zero: xf_div requires it)
    sel = i % 97 == 0
    am, ae = np.where(sel, np.uint64(0), am), np.where(sel, ZERO_E, ae).astype(np.int32)
    zero_b = bm == 0  # a near-equal operand that came out as zero
    bm, be, bs = np.where(zero_b, np.uint64(TOP), bm), np.where(zero_b, 0, be).astype(np.int32), np.where(zero_b, 0, bs).astype(np.uint32)
    return am, ae, as_, bm, be.astype(np.int32), bs.astype(np.uint32)


def _with_random_b(rng, a):
    am, ae, as_ = a
    bm, be, bs = _rnd(rng, am.size)
    return am, ae, as_, bm, be, bs


def _q15_half(rng, n):
    """Q15 inputs next to half-integers: (k + 1/2 + d * 2^-j) / 32768, d in -2..2."""
    k = rng.integers(-35000, 35000, n).astype(LD) + LD(0.5)
    d = rng.integers(-2, 3, n).astype(LD)
    c = (k + np.ldexp(d, -rng.integers(0, 60, n))) / LD(32768)
    return _with_random_b(rng, ld_parts(c))


def _q15_range(rng, n):
    """Q15 inputs over every binade from far below one half of 2^-15 to far outside int16."""
    return _with_random_b(rng, _rnd(rng, n, -78, 6))


def _signs(rng, n):
    return rng.integers(0, 2, n).astype(np.uint32)


def _exps(rng, n):
    return rng.integers(-40, 40, n).astype(np.int32)


def _div_patterns(rng, n):
    """Quotients whose 32-bit halves are all zeros or all ones: a = round(q * b) for a chosen q, so a / b lands on q or
    next to it."""
    hi = rng.integers(1 << 31, 1 << 32, n, dtype=np.uint64)
    lo = rng.integers(0, 1 << 32, n, dtype=np.uint64)
    kind = np.arange(n) % 4
    qm = np.where(kind == 0, (hi << np.uint64(32)) | np.uint64(0xFFFFFFFF),      # low half all ones
         np.where(kind == 1, hi << np.uint64(32),                                 # low half zero
         np.where(kind == 2, np.uint64(0xFFFFFFFF00000000) | lo,                  # high half all ones
                  np.uint64(0x8000000000000000) | lo)))                           # high half: the top bit alone
    bm, be, bs = _rnd(rng, n, -40, 40)
    a = ld_make(qm, _exps(rng, n), _signs(rng, n)) * ld_make(bm, be, bs)
    am, ae, as_ = ld_parts(a)
    return am, ae, as_, bm, be, bs


def _div_exact(rng, n):
    """a = q * b with 32-bit q and b: the product is exact, so is the quotient (remainder 0, low half 0)."""
    q = rng.integers(1 << 31, 1 << 32, n, dtype=np.uint64) << np.uint64(32)
    b = rng.integers(1 << 31, 1 << 32, n, dtype=np.uint64) << np.uint64(32)
    kind = np.arange(n) % 4
    b = np.where(kind == 3, rng.integers(0, 1 << 64, n, dtype=np.uint64) | np.uint64(TOP), b)  # any b, q a power of two
    q = np.where(kind == 3, np.uint64(TOP), q)
    be, bs = _exps(rng, n), _signs(rng, n)
    a = ld_make(q, _exps(rng, n), _signs(rng, n)) * ld_make(b, be, bs)
    am, ae, as_ = ld_parts(a)
    return am, ae, as_, b, be, bs


def _div_edge_divisors(rng, n):
    am, ae, as_ = _rnd(rng, n, -40, 40)
    bm = np.where(np.arange(n) % 2 == 0, np.uint64(TOP), np.uint64(ALL1))
    return am, ae, as_, bm, _exps(rng, n), _signs(rng, n)


def _neighbour_significands(rng, n):
    """Equal significands and a.m = b.m +- 1, at equal and at other exponents."""
    am = rng.integers(0, 1 << 64, n, dtype=np.uint64) | np.uint64(TOP)
    am = np.where(am == np.uint64(ALL1), np.uint64(ALL1 - 1), am)
    am = np.where(am == np.uint64(TOP), np.uint64(TOP + 1), am)
    kind = np.arange(n) % 3
    bm = np.where(kind == 0, am, np.where(kind == 1, am + np.uint64(1), am - np.uint64(1)))
    ae = _exps(rng, n)
    de = np.array([0, 0, 0, 1, -1, 2, -2, 63, -64], dtype=np.int32)[rng.integers(0, 9, n)]
    return am, ae, _signs(rng, n), bm, ae + de, _signs(rng, n)


def _sum_carries(rng, n):
    """Roundings that carry out of bit 63 in the adder: an all-ones significand plus at least half a unit in the last
    place (d = 64: the other operand starts at the guard bit); 2^63 minus a little, d >= 66, rounds back up to 2^63."""
    kind = np.arange(n) % 2
    am = np.where(kind == 0, np.uint64(ALL1), np.uint64(TOP))
    ae, as_ = _exps(rng, n), _signs(rng, n)
    bm = rng.integers(0, 1 << 64, n, dtype=np.uint64) | np.uint64(TOP)
    d = np.where(kind == 0, 64, rng.integers(66, 131, n)).astype(np.int32)
    # kind 0 carries in xf_add with equal signs (and in xf_sub with different ones); kind 1 the other way round
    flip = rng.integers(0, 2, n).astype(np.uint32)
    return am, ae, as_, bm, ae - d, as_ ^ flip


def _mul_carries(rng, n):
    """Products in [2^127 - 2^62, 2^127): normalised by one bit they round up to 2^64."""
    am = rng.integers(0, 1 << 64, n, dtype=np.uint64) | np.uint64(TOP)
    am = np.where(am == np.uint64(TOP), np.uint64(TOP + 12345), am)
    bm = _u64(((1 << 127) - 1) // int(a) for a in am)
    return am, _exps(rng, n), _signs(rng, n), bm, _exps(rng, n), _signs(rng, n)


def _cancel(rng, n):
    """b = a or b = -a (one of a + b, a - b cancels completely), and differences that lose 64 bits or more: 2^63 at
    exponent e + 1 against all ones at exponent e."""
    am, ae, as_ = _rnd(rng, n, -40, 40)
    kind = np.arange(n) % 3
    am = np.where(kind == 2, np.uint64(TOP), am)
    bm = np.where(kind == 2, np.uint64(ALL1), am)
    be = np.where(kind == 2, ae - 1, ae).astype(np.int32)
    flip = rng.integers(0, 2, n).astype(np.uint32)
    return am, ae, as_, bm, be, as_ ^ flip


def _add_ties(rng, n):
    """Exactly half a unit in the last place in the adder: b = 2^63 at distance 64 (a's last bit even or odd), or an odd
    b one binade down with no carry."""
    kind = np.arange(n) % 2
    am = rng.integers(0, 1 << 64, n, dtype=np.uint64) | np.uint64(TOP)
    am = np.where(am == np.uint64(TOP), np.uint64(TOP + 2), am)
    quarter = np.uint64((1 << 62) - 1)
    am = np.where(kind == 1, (am & quarter) | np.uint64(TOP), am)
    bm = np.where(kind == 1, (rng.integers(0, 1 << 64, n, dtype=np.uint64) & quarter) | np.uint64(TOP) | np.uint64(1), np.uint64(TOP))
    ae, as_ = _exps(rng, n), _signs(rng, n)
    d = np.where(kind == 1, 1, 64).astype(np.int32)
    flip = np.where(kind == 1, 0, rng.integers(0, 2, n)).astype(np.uint32)
    # with the larger operand second half of the time
    am2, ae2, as2, bm2, be2, bs2 = am, ae, as_, bm, ae - d, as_ ^ flip
    sw = rng.integers(0, 2, n) == 1
    return (np.where(sw, bm2, am2), np.where(sw, be2, ae2).astype(np.int32), np.where(sw, bs2, as2).astype(np.uint32),
            np.where(sw, am2, bm2), np.where(sw, ae2, be2).astype(np.int32), np.where(sw, as2, bs2).astype(np.uint32))


def _sticky_decides(rng, n):
    """Differences whose rounding is decided below the 128-bit window of the adder: the part of b inside the window
    leaves exactly half a unit in the last place with an even last bit, and the bit of b shifted out below the window
    makes it less than half that is taken away, so the result rounds up where a tie would round down.  Odd a.m against
    all ones at distance 65; a.m = 2^63 against 0xFF..FD, 0xFF..FE, 0xFF..FF at distance 66 (one bit of normalisation)."""
    kind = np.arange(n) % 2
    am = np.where(kind == 0, rng.integers(0, 1 << 64, n, dtype=np.uint64) | np.uint64(TOP + 1), np.uint64(TOP))
    am = np.where(am == np.uint64(TOP + 1), np.uint64(TOP + 3), am)
    bm = np.where(kind == 0, np.uint64(ALL1), np.uint64(ALL1) - rng.integers(0, 3, n).astype(np.uint64))
    ae, as_ = _exps(rng, n), _signs(rng, n)
    d = np.where(kind == 0, 65, 66).astype(np.int32)
    flip = rng.integers(0, 2, n).astype(np.uint32)  # a + b subtracts with different signs, a - b with equal ones
    return am, ae, as_, bm, ae - d, as_ ^ flip


def _mul_ties(rng, n):
    """a.m = A << 32 (A odd, 32 bits), b.m = B << 31 (B odd, 33 bits): the product is A * B << 63, half a unit in the last
    place whenever it reaches 2^127."""
    A = rng.integers(1 << 31, 1 << 32, n, dtype=np.uint64) | np.uint64(1)
    B = rng.integers(1 << 32, 1 << 33, n, dtype=np.uint64) | np.uint64(1)
    return A << np.uint64(32), _exps(rng, n), _signs(rng, n), B << np.uint64(31), _exps(rng, n), _signs(rng, n)


_SPECIAL = (("q15_half", _q15_half, 1 << 16), ("q15_range", _q15_range, 1 << 15), ("div_patterns", _div_patterns, 1 << 14),
            ("div_exact", _div_exact, 1 << 13), ("div_edge_divisors", _div_edge_divisors, 1 << 12),
            ("neighbours", _neighbour_significands, 1 << 13), ("sum_carries", _sum_carries, 1 << 13),
            ("mul_carries", _mul_carries, 1 << 12), ("cancel", _cancel, 1 << 13), ("add_ties", _add_ties, 1 << 13),
            ("mul_ties", _mul_ties, 1 << 12), ("sticky_decides", _sticky_decides, 1 << 12))
OPS_TOTAL = 1 << 20


@functools.lru_cache(None)
def ops_corpus(seed=8087):
    assert_long_double_is_x87()
    rng = np.random.default_rng(seed)
    n_special = sum(k for _, _, k in _SPECIAL)
    parts = [("base", _base(rng, OPS_TOTAL - n_special), OPS_TOTAL - n_special)]
    parts += [(name, fn(rng, k), k) for name, fn, k in _SPECIAL]
    cols = [np.concatenate([p[1][c] for p in parts]) for c in range(6)]
    n = cols[0].size
    assert n == OPS_TOTAL
    classes, pos = {}, 0
    for name, _, k in parts:
        classes[name] = (pos, pos + k)
        pos += k
    in_m = np.stack([cols[0], cols[3]]).astype(np.uint64)
    in_e = np.stack([cols[1], cols[4]]).astype(np.int32)
    in_s = np.stack([cols[2], cols[5]]).astype(np.uint32)
    in_e[in_m == 0] = ZERO_E
    assert (in_m[1] != 0).all(), "a zero divisor"
    # int64 inputs: test_x87.cpp's (random bits shifted down, either sign), and the edges every 64th element
    iv = (rng.integers(0, 1 << 64, n, dtype=np.uint64) >> rng.integers(0, 64, n).astype(np.uint64)).view(np.int64)
    iv = np.where(rng.integers(0, 2, n) == 1, iv, (np.uint64(0) - iv.view(np.uint64)).view(np.int64))
    edge = np.array([np.iinfo(np.int64).min, 1, -1, 0, np.iinfo(np.int64).max, -np.iinfo(np.int64).max, 1 << 62, -(1 << 53) - 1],
                    dtype=np.int64)
    idx = np.arange(n)
    iv = np.where(idx % 64 == 0, edge[(idx // 64) % edge.size], iv)
    for a in (in_m, in_e, in_s, iv):
        a.setflags(write=False)
    return OpsCorpus(n, in_m, in_e, in_s, np.ascontiguousarray(iv), classes)


OpsResult = namedtuple("OpsResult", "out_m out_e out_s out_i")


def _round_half_away(x):
    f = np.floor(np.abs(x))
    return np.copysign(f + ((np.abs(x) - f) >= 0.5), x)  # |x| - f is exact


@functools.lru_cache(None)
def ops_expected(seed=8087):
    """The seven operations in the machine's long double."""
    c = ops_corpus(seed)
    a = ld_make(c.in_m[0], c.in_e[0], c.in_s[0])
    b = ld_make(c.in_m[1], c.in_e[1], c.in_s[1])
    with np.errstate(all="raise"):
        res = [a + b, a - b, a * b, a / b, c.in_i.astype(LD)]
        lt = (a < b).astype(np.int32)
        # static_cast<double>, std::round(c * 32768.0), clamp (ref src/codec/lpc/lpc.cpp:73-78, 179)
        scaled = _round_half_away(a.astype(np.float64) * 32768.0)
        q15 = np.clip(scaled, -32768.0, 32767.0).astype(np.int32)
    parts = [ld_parts(r) for r in res]
    out = OpsResult(np.stack([p[0] for p in parts]), np.stack([p[1] for p in parts]), np.stack([p[2] for p in parts]),
                    np.stack([lt, q15]))
    for arr in out:
        arr.setflags(write=False)
    return out


def _hex_operand(c, which, i):
    return f"{'-' if c.in_s[which, i] else '+'}0x{int(c.in_m[which, i]):016X}p{int(c.in_e[which, i]) - 63:+d}"


def compare_ops(c, want, got, what):
    """Every element of every operation; the message names the operation and the operands in hex."""
    for k, op in enumerate(OPS):
        zero = (want.out_m[k] == 0) & (got.out_m[k] == 0)
        bad = (want.out_m[k] != got.out_m[k]) | (~zero & ((want.out_e[k] != got.out_e[k]) | (want.out_s[k] != got.out_s[k])))
        if bad.any():
            i = int(np.flatnonzero(bad)[0])
            arg = f"v = {int(c.in_i[i])} (0x{int(c.in_i[i]) & ALL1:016X})" if op == "from_i64" else \
                f"a = {_hex_operand(c, 0, i)}, b = {_hex_operand(c, 1, i)}"
            raise AssertionError(
                f"{what}: xf_{op} differs from long double at {int(bad.sum())} of {c.n} elements; first at {i}: {arg}: got "
                f"(m 0x{int(got.out_m[k, i]):016X}, e {int(got.out_e[k, i])}, s {int(got.out_s[k, i])}), long double gives "
                f"(m 0x{int(want.out_m[k, i]):016X}, e {int(want.out_e[k, i])}, s {int(want.out_s[k, i])})")
    for k, op in enumerate(INT_OPS):
        bad = want.out_i[k] != got.out_i[k]
        if bad.any():
            i = int(np.flatnonzero(bad)[0])
            raise AssertionError(
                f"{what}: xf_{'lt' if op == 'lt' else 'to_q15'} differs from long double at {int(bad.sum())} of {c.n} elements; "
                f"first at {i}: a = {_hex_operand(c, 0, i)}, b = {_hex_operand(c, 1, i)}: got {int(got.out_i[k, i])}, "
                f"long double gives {int(want.out_i[k, i])}")


def _tie_parity(mag):
    """None, or the last kept bit (0 / 1) when the exact magnitude `mag` lies half-way between two 64-bit significands."""
    bits = mag.bit_length()
    if bits <= 64:
        return None
    drop = bits - 64
    if mag & ((1 << drop) - 1) != 1 << (drop - 1):
        return None
    return (mag >> drop) & 1


def ops_class_counts(c, want):
    """How often each class the device-specific code needs occurs, from the operands and the long double results alone."""
    am, bm, ae, be = c.in_m[0], c.in_m[1], c.in_e[0].astype(np.int64), c.in_e[1].astype(np.int64)
    same_sign = c.in_s[0] == c.in_s[1]
    nz = am != 0
    n = {}
    q = want.out_m[3]
    qlo, qhi = q & np.uint64(0xFFFFFFFF), q >> np.uint64(32)
    n["div quotient low half 0"] = int((nz & (qlo == 0)).sum())
    n["div quotient low half all ones"] = int((qlo == 0xFFFFFFFF).sum())
    n["div quotient high half all ones"] = int((qhi == 0xFFFFFFFF).sum())
    n["div quotient high half 0x80000000"] = int((qhi == 0x80000000).sum())
    n["div by 0x8000000000000000"] = int((nz & (bm == np.uint64(TOP))).sum())
    n["div by 0xFFFFFFFFFFFFFFFF"] = int((nz & (bm == np.uint64(ALL1))).sum())
    n["equal significands"] = int((am == bm).sum())
    n["a.m = b.m + 1"] = int((nz & (am == bm + np.uint64(1))).sum())
    n["a.m = b.m - 1"] = int((nz & (am + np.uint64(1) == bm) & (am != np.uint64(ALL1))).sum())
    d = ae - be
    for k, op in ((0, "add"), (1, "sub")):
        eff_same = same_sign if k == 0 else ~same_sign  # the adder adds magnitudes
        rm, re = want.out_m[k], want.out_e[k].astype(np.int64)
        n[f"{op} rounding carries out of bit 63 (all ones + half ulp)"] = int(
            (eff_same & (am == np.uint64(ALL1)) & (d == 64) & (rm == np.uint64(TOP)) & (re == ae + 1)).sum())
        n[f"{op} rounding carries out of bit 63 (2^63 - tiny)"] = int(
            (nz & ~eff_same & (am == np.uint64(TOP)) & (d >= 66) & (rm == np.uint64(TOP)) & (re == ae)).sum())
        n[f"{op} rounding decided below the 128-bit window"] = int(
            (~eff_same & ((((am & np.uint64(1)) == 1) & (am > np.uint64(TOP + 1)) & (bm == np.uint64(ALL1)) & (d == 65) & (rm == am) & (re == ae))
                          | ((am == np.uint64(TOP)) & (bm >= np.uint64(ALL1 - 2)) & (d == 66) & (rm == np.uint64(TOP)) & (re == ae)))).sum())
        n[f"{op} cancels completely"] = int((nz & (rm == 0)).sum())
        n[f"{op} loses 64 bits or more"] = int((nz & (rm != 0) & (re <= np.maximum(ae, be) - 64)).sum())
    pow2 = (am == np.uint64(TOP)) & (bm == np.uint64(TOP))
    n["mul rounding carries out of bit 63"] = int((nz & ~pow2 & (want.out_m[2] == np.uint64(TOP))).sum())
    # exact divisions, ties: exact integer arithmetic over the constructed classes (Python integers)
    exact = 0
    ties = {(op, p): 0 for op in ("add", "sub", "mul", "div") for p in (0, 1)}
    for name in ("div_patterns", "div_exact", "neighbours", "sum_carries", "add_ties", "mul_ties", "cancel"):
        lo, hi = c.classes[name]
        for i in range(lo, hi):
            a, b = int(am[i]), int(bm[i])
            if a == 0:
                continue
            shift = 64 if a < b else 63
            rem = (a << shift) % b
            exact += rem == 0
            if 2 * rem == b:
                ties[("div", ((a << shift) // b) & 1)] += 1
            p = _tie_parity(a * b)
            if p is not None:
                ties[("mul", p)] += 1
            dist = int(d[i])
            if -64 <= dist <= 64:
                x, y = (a << dist, b) if dist >= 0 else (a, b << -dist)
                for op, sgn in (("add", 1), ("sub", -1)):
                    eff = sgn if same_sign[i] else -sgn
                    p = _tie_parity(abs(x + eff * y))
                    if p is not None:
                        ties[(op, p)] += 1
    n["exact divisions"] = int(exact)
    for (op, p), cnt in ties.items():
        n[f"{op} tie, last bit {'odd' if p else 'even'}"] = cnt
    for name, v in (("INT64_MIN", np.iinfo(np.int64).min), ("+1", 1), ("-1", -1), ("0", 0)):
        n[f"from_i64 {name}"] = int((c.in_i == v).sum())
    n["a is zero"] = int((~nz).sum())
    half = c.classes["q15_half"]
    n["q15 next to a half-integer"] = half[1] - half[0]
    n["q15 saturates high"] = int((want.out_i[1] == 32767).sum())
    n["q15 saturates low"] = int((want.out_i[1] == -32768).sum())
    return n


# A division never ties: a.m * 2^k = (2 q + 1) * b.m would need the odd number 2 q + 1 of 65 significant bits to divide a
# 64-bit significand times a power of two.  So "rem == other" in xf_div is dead code, and the recipe asserts the count is 0.
IMPOSSIBLE_CLASSES = ("div tie, last bit even", "div tie, last bit odd")
MIN_CLASS_COUNT = 300


# ---------------------------------------------------------------------------------------------------------------------
# Levinson tables
# ---------------------------------------------------------------------------------------------------------------------
def levinson_long_double(r, order):
    """ref src/codec/lpc/lpc.cpp:98-186 in numpy.longdouble scalars: (used, coeffs[order + 1], clamped_high, clamped_low).
    A second statement of the recursion beside the oracle's, kept for what the oracle does not tell: whether k hit a
    clamp."""
    eps, lim, one = LD("1e-8"), LD("0.999"), LD(1)
    R = [LD(int(v)) for v in r[:order + 1]]  # int64 -> long double, exact below 2^64
    if R[0] < one:
        R[0] = one
    a = [LD(0)] * (order + 1)
    prev = [LD(0)] * (order + 1)
    E = R[0]
    achieved, hi, lo = 0, False, False
    for i in range(1, order + 1):
        acc = LD(0)
        for j in range(1, i):
            acc = acc + prev[j] * R[i - j]
        if E < eps:
            break
        k = (R[i] - acc) / E
        if k > lim:
            k, hi = lim, True
        if k < -lim:
            k, lo = -lim, True
        e_new = (one - k * k) * E
        if e_new < eps:
            break
        a[i] = k
        for j in range(1, i):
            a[j] = prev[j] - k * prev[i - j]
        prev[1:i + 1] = a[1:i + 1]
        E = e_new
        achieved = i
    co = np.zeros(order + 1, dtype=np.int16)
    for j in range(1, achieved + 1):
        co[j] = int(np.clip(_round_half_away(np.float64(a[j]) * 32768.0), -32768.0, 32767.0))
    return achieved, co, hi, lo


def _constructed_signals(n, amp):
    i = np.arange(n, dtype=np.int64)
    fam = {
        "constant": np.full(n, amp),
        "alternating": np.where(i % 2 == 0, amp, -amp),
        "period3": np.array([amp, 0, -amp])[i % 3],
        "period4": np.array([amp, amp, -amp, -amp])[i % 4],
        "period6": np.array([amp, amp, 0, -amp, -amp, 0])[i % 6],
        "ramp": (i * 2 * amp) // max(n - 1, 1) - amp,
        "sine0.37": np.floor(amp * np.sin(0.37 * i)),
        "sine0.011": np.floor(amp * np.sin(0.011 * i)),
        "sine3.1": np.floor(amp * np.sin(3.1 * i)),
        "parabola": (4 * amp * i * (n - 1 - i)) // max((n - 1) * (n - 1), 1) - amp // 2,
        "single": np.where(i == n // 3, amp, 0),
        "zeros": np.zeros(n),
    }
    return {k: np.asarray(v).astype(np.int64).astype(np.int32) for k, v in fam.items()}


WINDOWS = (256, 4096, 16384)
AMPLITUDES = {16: (1, 32767), 24: ((1 << 23) - 1, (1 << 24) - 1)}  # 2^24 - 1: the side channel's extreme
SYNTH_KINDS = ("music", "noise", "silence", "near_silence", "sparse", "ramp", "walk", "tone", "mixed")


@functools.lru_cache(None)
def signals(depth):
    """[(name, int32 pcm)]: the nine synth kinds and the constructed families over windows of 256, 4096 and 16384."""
    import __graft_entry__ as ge

    synth = ge.load_pkg().synth
    out = []
    for kind in SYNTH_KINDS:
        pcm, _ = synth.synth_pcm(16384, 1, depth, 48000, seed=31 + depth, kind=kind)
        for n in WINDOWS:
            out.append((f"{kind}/{depth}/{n}", np.ascontiguousarray(pcm[:n])))
    for amp in AMPLITUDES[depth]:
        for n in WINDOWS:
            for name, pcm in _constructed_signals(n, amp).items():
                out.append((f"{name}/{amp}/{n}", pcm))
    return out


def stopping_tables():
    """R = {1, t zeros, then +-5, -+7 alternating}: E stays 1 through the zero lags, the first |k| above the clamp leaves
    E = 1 - 0.999^2, and two steps later the energy falls below 1e-8: the solve stops short of order 12."""
    out = []
    for t in range(0, 10):
        for first in (5, -5):
            r = np.zeros(13, dtype=np.int64)
            r[0] = 1
            v, w = first, -7 if first > 0 else 7
            for k in range(t + 1, 13):
                r[k] = v if (k - t) % 2 == 1 else w
            out.append(r)
    return out


def random_tables(rng, count, depth):
    """Seeded int64 tables as no PCM gives them: small R[0] under large lags (these stop at every order), negative R[0]
    and INT64_MIN as wrapped sums produce them, full 64-bit noise."""
    big = 40 if depth == 16 else 63
    out = []
    for t in range(count):
        kind = t % 8
        if kind < 5:  # small energy, lags of a few times its size
            r0 = int(rng.integers(1, 40))
            span = int(rng.integers(1, 4)) * r0
            r = rng.integers(-span, span + 1, 13)
            r[0] = r0
        elif kind == 5:  # decaying, nearly singular
            r0 = int(rng.integers(1, 1 << int(rng.integers(2, big))))
            r = (r0 * np.cos(np.arange(13) * float(rng.uniform(0.01, 3.0)))).astype(np.int64) + rng.integers(-2, 3, 13)
            r[0] = r0
        elif kind == 6:  # any 64-bit words
            bits = int(rng.integers(8, big + 1))
            r = rng.integers(-(1 << bits), (1 << bits) - 1, 13, endpoint=True)
        else:  # wrapped energies
            bits = int(rng.integers(8, big + 1))
            r = rng.integers(-(1 << bits), (1 << bits) - 1, 13, endpoint=True)
            r[0] = [np.iinfo(np.int64).min if depth == 24 else -(1 << 40), -1, 0, -int(rng.integers(1, 1 << 30))][(t // 8) % 4]
        out.append(np.asarray(r, dtype=np.int64))
    return out


TableSet = namedtuple("TableSet", "tables used coef names n_signal")
RANDOM_TABLES = {16: 2600, 24: 2600}


@functools.lru_cache(None)
def table_set(depth):
    """Every table of one bit depth with the oracle's answer for the five candidates (used[n][5], coef[n][5][13])."""
    import oracleshim

    tabs, names = [], []
    for name, pcm in signals(depth):
        tabs.append(oracleshim.autocorr(pcm, 12))
        names.append(name)
    n_signal = len(tabs)
    for k, r in enumerate(stopping_tables()):
        tabs.append(r)
        names.append(f"stop{k}")
    rng = np.random.default_rng(1987 + depth)
    for k, r in enumerate(random_tables(rng, RANDOM_TABLES[depth], depth)):
        tabs.append(r)
        names.append(f"random{k}")
    tables = np.ascontiguousarray(np.stack(tabs), dtype=np.int64)
    used = np.zeros((len(tabs), 5), dtype=np.uint8)
    coef = np.zeros((len(tabs), 5, 13), dtype=np.int16)
    for t in range(len(tabs)):
        for ci, cand in enumerate(CANDS):
            u, co = oracleshim.levinson_q15(tables[t], cand)
            used[t, ci] = u
            coef[t, ci, :cand + 1] = co
    for a in (tables, used, coef):
        a.setflags(write=False)
    return TableSet(tables, used, coef, tuple(names), n_signal)


def expected_for_mvo(ts, idx, mvo):
    """The oracle's answers for tables idx as a slot of highest valid order mvo holds them: a candidate above mvo is
    skipped (used 0, no coefficients), ref block/encoder.cpp:41."""
    used = ts.used[idx].copy()
    coef = ts.coef[idx].copy()
    skip = np.asarray(CANDS)[None, :] > np.asarray(mvo)[:, None]
    used[skip] = 0
    coef[skip] = 0
    return used, coef


# ---------------------------------------------------------------------------------------------------------------------
# placements: launch sets for k_levinson
# ---------------------------------------------------------------------------------------------------------------------
LPCSET = np.dtype([("coef", "<i2", (5, 13)), ("used", "u1", (5,)), ("pad", "u1")])
assert LPCSET.itemsize == 136
SENTINEL = 0x5A
SHORT_FINALS = (1, 2, 5, 7, 9, 11, 13, 33)

Placement = namedtuple("Placement", "name streams as_table blocks acorr need_probe table_idx written mvo")


def _stream_blocks(frames):
    return (frames + MAX_BLOCK - 1) // MAX_BLOCK


def _need_probe_word(rng, b):
    """Probe masks with holes, all-zero words, and the two values the product writes (0xFFF0, 0)."""
    return [0xFFF0, 0, int(rng.integers(0, 1 << 16)) & 0xFFF0, 0xFFFF, 0x8010, int(rng.integers(0, 1 << 16))][b % 6]


def _layout(name, ts, streams, as_table, rng, offset):
    """streams: [(frames, channels, stereo_mode)].  Tables go to the slots in the kernel's lane order (slot-major: lane
    id = slot * blocks + block), alternating between tables that stop early and tables that run to order 12, so that
    every wave holds both."""
    blocks = sum(_stream_blocks(f) for f, _, _ in streams)
    stop = np.flatnonzero(ts.used[:, 4] < 12)
    full = np.flatnonzero(ts.used[:, 4] == 12)
    table_idx = np.zeros((blocks, SLOTS), dtype=np.int64)
    lane = np.arange(blocks * SLOTS)
    pick = np.where(lane % 2 == 0, stop[(lane // 2 + offset) % stop.size], full[(lane // 2 + offset) % full.size])
    table_idx[lane % blocks, lane // blocks] = pick
    need = np.array([_need_probe_word(rng, b) for b in range(blocks)], dtype=np.uint32)
    written = np.zeros((blocks, SLOTS), dtype=bool)
    mvo = np.zeros((blocks, SLOTS), dtype=np.int32)
    b0 = 0
    for frames, ch, sm in streams:
        nb = _stream_blocks(frames)
        for k in range(nb):
            n = min(MAX_BLOCK, frames - k * MAX_BLOCK)
            for slot in range(SLOTS):
                win, c = slot >> 2, slot & 3
                if win == 0:
                    live = c == 0 if ch == 1 else (c < 2 if sm == 0 else (c >= 2 if sm == 1 else True))
                    size = n
                else:
                    live = ch == 2 and sm == 2 and n > FULL_COMPARE_LIMIT and bool((int(need[b0 + k]) >> slot) & 1)
                    size = PROBE
                written[b0 + k, slot] = live
                mvo[b0 + k, slot] = min(size - 1, 32) if size > 1 else 0
        b0 += nb
    acorr = np.ascontiguousarray(ts.tables[table_idx])
    return Placement(name, tuple(streams), as_table, blocks, acorr, need, table_idx, written, mvo)


@functools.lru_cache(None)
def placements(depth):
    """Single-stream launch sets (37 blocks, one per short final block and stream shape; 259 blocks) and stream tables
    (the same shapes as streams of one set).  Block counts are no multiple of 16, so a wave mixes slots; 259 blocks fill
    sixteen workgroups and part of a seventeenth."""
    ts = table_set(depth)
    rng = np.random.default_rng(4242 + depth)
    shapes = [(1, 0), (2, 0), (2, 1), (2, 2)]
    out = []
    for k, last in enumerate(SHORT_FINALS):
        ch, sm = shapes[k % 4]
        out.append(_layout(f"single/{ch}ch/mode{sm}/37 blocks/last {last}", ts, [(36 * MAX_BLOCK + last, ch, sm)], False, rng, 131 * k))
    out.append(_layout("single/2ch/mode2/259 blocks/last 5000", ts, [(258 * MAX_BLOCK + 5000, 2, 2)], False, rng, 977))
    out.append(_layout("single as table/2ch/mode2/37 blocks", ts, [(36 * MAX_BLOCK + 4097, 2, 2)], True, rng, 555))
    streams = []
    for k, last in enumerate(SHORT_FINALS + (4096, 4097, 16384, 300)):
        ch, sm = shapes[(k + 1) % 4]
        streams.append(((k % 5) * MAX_BLOCK + last, ch, sm))
    streams.append((203 * MAX_BLOCK + 77, 2, 2))
    streams.append((21 * MAX_BLOCK + 3, 1, 0))
    out.append(_layout(f"table/{len(streams)} streams", ts, streams, True, rng, 2024))
    return tuple(out)


def expected_lpcs(depth, pl):
    """The LpcSet array the kernel must leave: the sentinel where it must not write."""
    ts = table_set(depth)
    want = np.zeros((pl.blocks, SLOTS), dtype=LPCSET)
    want.view(np.uint8)[...] = SENTINEL
    w = pl.written
    used, coef = expected_for_mvo(ts, pl.table_idx[w], pl.mvo[w])
    rec = np.zeros(used.shape[0], dtype=LPCSET)
    rec["coef"], rec["used"], rec["pad"] = coef, used, 0
    want[w] = rec
    return want


def sentinel_lpcs(blocks):
    a = np.zeros((blocks, SLOTS), dtype=LPCSET)
    a.view(np.uint8)[...] = SENTINEL
    return a


def compare_lpcs(pl, want, got, what):
    """Byte for byte; the message names the block, slot and candidate."""
    if np.array_equal(want.view(np.uint8), got.view(np.uint8)):
        return
    for b in range(pl.blocks):
        for slot in range(SLOTS):
            w, g = want[b, slot], got[b, slot]
            if w.tobytes() == g.tobytes():
                continue
            where = f"{what}: {pl.name}: block {b} slot {slot} (table {int(pl.table_idx[b, slot])}, mvo {int(pl.mvo[b, slot])})"
            if not pl.written[b, slot]:
                raise AssertionError(f"{where}: the kernel must skip this slot, but the sentinel is gone")
            if g.tobytes() == bytes([SENTINEL]) * LPCSET.itemsize:
                raise AssertionError(f"{where}: the kernel wrote nothing")
            for ci, cand in enumerate(CANDS):
                if int(w["used"][ci]) != int(g["used"][ci]) or not np.array_equal(w["coef"][ci], g["coef"][ci]):
                    raise AssertionError(f"{where} candidate {cand}: used {int(g['used'][ci])}, coefficients {g['coef'][ci].tolist()}; "
                                         f"the oracle: used {int(w['used'][ci])}, coefficients {w['coef'][ci].tolist()}")
            raise AssertionError(f"{where}: pad is {int(g['pad'])}, not 0")
