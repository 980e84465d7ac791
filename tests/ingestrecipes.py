"""Corpus and reference of the ingest-kernel tests (tests/test_ingest_recipes_host.py, tests/test_gpu_ingest_tables.py):
what k_ingest and k_stereo (csrc/k_front.hip) must write for a launch set, word for word, restated in exact integers.
Plain helper module: numpy, Python integers, planref and the oracle; importable without a GPU.

Per block and channel L, R, M = floor((L + R) / 2), S = L - R (ref simd/neon.cpp:14-30):
  lag sums     sum over n >= k of x[n] x[n - k], k = 0..12, inside the block, and inside each of the three 256-frame probe
               windows with the samples before the window absent (ref lpc.cpp:80-96, lac/encoder.cpp:343-346);
  proxy sums   zigzag sums of the samples, of their first differences and of their first sums, the block's first sample
               raw in all three (ref lac/encoder.cpp:146-178);
  bad index    the lowest index outside the bit depth per channel (ref lac/encoder.cpp:82-102);
  plan, masks  the rule of stereo_block (ref lac/encoder.cpp:179-196).
Every word nobody may write keeps the sentinel byte.  The reference is laid out the way the kernel works -- 4096-sample
tiles with twelve samples of history, per-tile partial sums -- so that the mistakes such a kernel can make can be switched
on by name (FAULTS) and the corpus shown to see each of them."""
from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

import planref

BLOCK = planref.BLOCK
PROBE = planref.PROBE
LIMIT = planref.FULL_COMPARE_LIMIT
SLOTS = planref.SLOTS
TILE = 4096
SENTINEL = 0xA5
P32, I16, I24 = 0, 1, 2  # PCM_PLANAR_I32, PCM_INTERLEAVED_I16, PCM_INTERLEAVED_I24 (csrc/analyze_core.h)
LAYOUT_NAMES = {P32: "planar int32", I16: "interleaved int16", I24: "interleaved int24"}
NONE = 0xFFFFFFFF

BPLAN = np.dtype([("choose_ms", "u1"), ("uncertain", "u1"), ("est_ms", "u1"), ("invalid", "u1"), ("frames", "<u4"),
                  ("first_bad", "<u4"), ("pad", "<u4")])  # BlockPlan, csrc/lacx_types.h
assert BPLAN.itemsize == 16

# The oracle's order of its twelve sums (oracle/lac_oracle.c, laco_stereo_estimate): s[kind * 4 + channel], kind = raw,
# difference, anti-difference, channel = L, R, M, S -- the kernel's sums[block][kind * 4 + channel] is the same order.
ORACLE_SUM = tuple(range(12))

LENGTHS = (1, 2, 12, 13, 14, 15, 16, 17, 255, 256, 257, 4095, 4096, 4097, 4111, 4112, 4113, 8191, 8192, 8193, 12289,
           16383, 16384)

# The mistakes the reference can be asked to make (expect_stream(..., faults)), and the corpus streams that must see each.
# Two readings are fixed here.  A lag "cut to 63 bits" loses bit 63, the sign: no lag of 25-bit samples over 16384 frames
# reaches 2^62 in magnitude (16384 * (2^24 - 1)^2 < 2^62), so a signed 63-bit accumulator would hold them all.  A proxy sum
# stays below 2^41 (16384 zigzags below 2^27): only its cut to 32 bits is a mistake a corpus can see.
FAULTS = {
    "no_tile_carry": ("history not carried over a tile seam", ("impulses",)),
    "carry_group_off": ("carry taken one group off", ("impulses",)),
    "tail_not_zeroed": ("samples past the block end not zeroed", ("len4097",)),
    "prev_block_history": ("previous block's tail used as history and for the head difference", ("tailhead",)),
    "prev_block_head": ("previous block's tail used for the head difference only", ("tailzero",)),
    "window_history": ("window history not zeroed", ("s37768",)),
    "m_truncated": ("M by truncating division", ("neg_odd",)),
    "sum_cut32": ("a proxy sum cut to 32 bits", ("big_sums",)),
    "lag_cut32": ("a lag cut to 32 bits", ("len256",)),
    "lag_cut63": ("a lag cut to 63 bits (the sign lost)", ("alt_fs24",)),
    "tile_partial32": ("a whole tile's partial sum wrapped at 2^32", ("big_sums",)),
    "any_bad": ("any bad index instead of the lowest", ("bad_several16",)),
    "right_first": ("right reported before left", ("bad_several24",)),
    "pct_lt": ("the 1 % rule with < for <=", ("boundary_1pct",)),
    "silent_small": ("the silent-block rule applied at nb <= 4096", ("zero_small",)),
}


# ---------------------------------------------------------------------------------------------------------------------
# streams and launch sets
# ---------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True, eq=False)
class Stream:
    name: str
    left: np.ndarray          # int32
    right: np.ndarray | None  # None: mono
    stereo_mode: int          # 0 LR, 1 MS, 2 per block
    bit_depth: int            # 0, 16, 24
    layout: int = P32
    offset: int = 0           # bytes behind a 16-byte aligned address
    at_end: bool = False      # placed at the very end of an allocation

    @property
    def frames(self):
        return int(self.left.size)

    @property
    def channels(self):
        return 1 if self.right is None else 2

    @property
    def blocks(self):
        return (self.frames + BLOCK - 1) // BLOCK

    @property
    def mode(self):  # (make_params: a mono stream's stereo mode is 0)
        return self.stereo_mode if self.right is not None else 0

    def shape(self):
        return (self.frames, self.channels, self.stereo_mode, self.bit_depth, self.layout)

    def arrays(self):
        """The stream's arrays as bytes in its layout: one for an interleaved layout, one per channel for the planar one."""
        chans = [self.left] if self.right is None else [self.left, self.right]
        if self.layout == P32:
            return [x.astype("<i4").tobytes() for x in chans]
        a = chans[0] if self.right is None else np.stack(chans, axis=1).ravel()
        if self.layout == I16:
            assert a.min() >= -32768 and a.max() <= 32767
            return [a.astype("<i2").tobytes()]
        assert a.min() >= -(1 << 23) and a.max() < (1 << 23)
        return [np.ascontiguousarray(a.astype("<i4").view(np.uint8).reshape(-1, 4)[:, :3]).tobytes()]

    def variant(self, **kw):
        d = dict(name=self.name, left=self.left, right=self.right, stereo_mode=self.stereo_mode, bit_depth=self.bit_depth,
                 layout=self.layout, offset=self.offset, at_end=self.at_end)
        d.update(kw)
        return Stream(**d)


@dataclass(frozen=True, eq=False)
class LaunchSet:
    name: str
    streams: tuple
    as_table: bool

    @property
    def blocks(self):
        return sum(s.blocks for s in self.streams)


@dataclass
class Tables:
    """What the hook returns for one run, or the reference's expectation of it.  strict[b] False: block b belongs to an
    invalid stream -- only badidx, invalid, first_bad, frames and the masks are compared (the kernel's proxy sums may be
    garbled for out-of-range input)."""
    sums: np.ndarray        # uint64 [blocks][12]
    badidx: np.ndarray      # uint32 [blocks][2]
    acorr: np.ndarray       # int64 [blocks][16][13]
    bplans: np.ndarray      # BPLAN [blocks]
    need_probe: np.ndarray  # uint32 [blocks]
    need_full: np.ndarray   # uint32 [blocks]
    strict: np.ndarray | None = None


def sentinel_tables(blocks, repeat=None):
    lead = (blocks,) if repeat is None else (repeat, blocks)

    def arr(shape, dtype):
        return np.frombuffer(bytes([SENTINEL]) * (int(np.prod(shape)) * np.dtype(dtype).itemsize), dtype=dtype).reshape(shape).copy()

    return Tables(arr(lead + (12,), np.uint64), arr(lead + (2,), np.uint32), arr(lead + (SLOTS, 13), np.int64),
                  arr(lead, BPLAN), arr(lead, np.uint32), arr(lead, np.uint32), np.ones(blocks, dtype=bool))


# ---------------------------------------------------------------------------------------------------------------------
# exact arithmetic
# ---------------------------------------------------------------------------------------------------------------------
def _dot(a, b):
    """sum a[i] b[i] as a Python integer; int64 arrays of magnitude below 2^26 and at most 2^15 elements.  The operands are
    split at 12 bits: no partial sum reaches 2^44."""
    ah, al, bh, bl = a >> 12, a & 4095, b >> 12, b & 4095
    return (int(np.dot(ah, bh)) << 24) + ((int(np.dot(ah, bl)) + int(np.dot(al, bh))) << 12) + int(np.dot(al, bl))


def _wrap64(v):
    v &= (1 << 64) - 1
    return v - (1 << 64) if v >> 63 else v


def _segment_lags(cur, hist):
    """Lags 0..12 of `cur` with the twelve samples `hist` in front of it."""
    ext = np.concatenate([hist, cur])
    m = cur.size
    return [_dot(cur, ext[12 - k:12 - k + m]) for k in range(13)]


def _before(x, at, count, floor):
    """x[at - count : at] with zeros where the index falls below `floor`."""
    out = np.zeros(count, dtype=np.int64)
    lo = max(at - count, floor)
    if at > lo:
        out[count - (at - lo):] = x[lo:at]
    return out


def block_lags(x, bs, nb, faults=frozenset()):
    """The 13 lag sums of block x[bs : bs + nb] (x: the channel's whole stream, int64), tile by tile."""
    total = [0] * 13
    for base in range(0, nb, TILE):
        cur = x[bs + base:bs + min(base + TILE, nb)]
        if "tail_not_zeroed" in faults and cur.size % 16:
            cur = np.concatenate([cur, np.full(16 - cur.size % 16, x[bs + nb - 1], dtype=np.int64)])
        if base == 0:
            hist = _before(x, bs, 12, 0 if "prev_block_history" in faults else bs)
        elif "no_tile_carry" in faults:
            hist = np.zeros(12, dtype=np.int64)
        elif "carry_group_off" in faults:
            hist = _before(x, bs + base - 4, 12, bs)
        else:
            hist = _before(x, bs + base, 12, bs)
        for k, v in enumerate(_segment_lags(cur, hist)):
            total[k] += v
    return _cut_lags(total, faults)


def window_lags(x, ws, faults=frozenset()):
    """The 13 lag sums of the probe window x[ws : ws + 256]."""
    hist = _before(x, ws, 12, 0) if "window_history" in faults else np.zeros(12, dtype=np.int64)
    return _cut_lags(_segment_lags(x[ws:ws + PROBE], hist), faults)


def _cut_lags(lags, faults):
    for v in lags:
        assert -(1 << 63) <= v < (1 << 63), "a lag sum outside int64: the kernel's accumulator would wrap"
    if "lag_cut32" in faults:
        lags = [((v + (1 << 31)) & 0xFFFFFFFF) - (1 << 31) for v in lags]
    if "lag_cut63" in faults:
        lags = [v & ((1 << 63) - 1) for v in lags]
    return lags


def plain_lags(seg):
    """The definition, in Python integers: for the short cases."""
    v = [int(t) for t in seg]
    return [sum(v[n] * v[n - k] for n in range(k, len(v))) for k in range(13)]


def _zz(v):
    return np.where(v >= 0, v << 1, ((-(v + 1)) << 1) | 1)


def block_sums(x, bs, nb, faults=frozenset()):
    """(raw, difference, anti-difference) zigzag sums of block x[bs : bs + nb] as Python integers."""
    cur = x[bs:bs + nb]
    prev = np.concatenate([[0], cur[:-1]])
    raw = _zz(cur)
    dif, ant = _zz(cur - prev), _zz(cur + prev)
    if ("prev_block_history" in faults or "prev_block_head" in faults) and bs > 0:
        dif[0], ant[0] = _zz(cur[0] - x[bs - 1]), _zz(cur[0] + x[bs - 1])
    else:
        dif[0] = ant[0] = raw[0]
    out = []
    for z in (raw, dif, ant):
        if "tile_partial32" in faults:
            s = sum(int(z[b:b + TILE].sum()) & 0xFFFFFFFF for b in range(0, nb, TILE))
        else:
            s = int(z.sum())  # below 2^27 * 2^14
        out.append(s & 0xFFFFFFFF if "sum_cut32" in faults else s)
    return out


def approx_rice_bits(total, count):  # ref lac/encoder.cpp:43-57
    if count == 0:
        return 0
    mean = (total + (count >> 1)) // count
    k = 0
    while k < 31 and (1 << k) < mean:
        k += 1
    return min((total >> k) + count * (k + 1), (1 << 64) - 1)


def estimate(sums12, nb, faults=frozenset()):
    """(est_ms, uncertain, lr, ms) of the twelve sums: ref lac/encoder.cpp:114-124, 179-196."""
    bits = [approx_rice_bits(s, nb) for s in sums12]
    chbits, active = [], False
    for c in range(4):
        raw, dif, ant = bits[c], bits[4 + c], bits[8 + c]
        chbits.append(min(raw, dif, ant))
        active = active or raw < dif or ant < dif
    lr, ms = chbits[0] + chbits[1], chbits[2] + chbits[3]
    smaller, diff = min(lr, ms), abs(lr - ms)
    close = diff < smaller // 100 if "pct_lt" in faults else diff <= smaller // 100
    return int(ms < lr), int(smaller == 0 or diff == 0 or active or close), lr, ms, active


def mid_side64(l, r, faults=frozenset()):
    s = l + r
    if "m_truncated" in faults:
        m = np.where(s < 0, -((-s) >> 1), s >> 1)
    else:
        m = s >> 1
    return m, l - r


def validates(st: Stream):
    """Whether the kernel checks the sample range: not where the container cannot hold an out-of-range value."""
    if st.bit_depth == 0 or st.layout == I16:
        return False
    return not (st.layout == I24 and st.bit_depth == 24)


# ---------------------------------------------------------------------------------------------------------------------
# the expectation
# ---------------------------------------------------------------------------------------------------------------------
def expect_stream(st: Stream, faults=frozenset(), oracle=None) -> Tables:
    """The tables of the stream's blocks.  oracle (tests/oracleshim.py) given and no fault asked for: est_ms and uncertain
    are the oracle's own (and must be what the restated rule gives)."""
    faults = frozenset(faults)
    nblk = st.blocks
    t = sentinel_tables(nblk)
    stereo = st.right is not None
    mode = st.mode
    est = stereo and mode == 2
    l = st.left.astype(np.int64)
    chans = [l]
    if stereo:
        r = st.right.astype(np.int64)
        m, s = mid_side64(l, r, faults)
        chans = [l, r, m, s]
        assert max(int(np.abs(c).max()) for c in chans) < (1 << 26)
    used = (0,) if not stereo else ((0, 1), (2, 3), (0, 1, 2, 3))[mode]
    lo, hi = (-32768, 32767) if st.bit_depth == 16 else (-(1 << 23), (1 << 23) - 1)
    check = validates(st)
    any_invalid = False
    for b in range(nblk):
        bs = b * BLOCK
        nb = min(BLOCK, st.frames - bs)
        for c in used:
            t.acorr[b, c] = [_wrap64(v) for v in block_lags(chans[c], bs, nb, faults)]
        if est and nb > LIMIT:
            for w in (1, 2, 3):
                a = planref.slot_window(nb, 4 * w)[0]
                for c in range(4):
                    t.acorr[b, 4 * w + c] = [_wrap64(v) for v in window_lags(chans[c], bs + a, faults)]
        sums12 = None
        if est:
            per = [block_sums(chans[c], bs, nb, faults) for c in range(4)]
            sums12 = [per[c][kind] for kind in range(3) for c in range(4)]
            t.sums[b] = sums12
        bad = [NONE, NONE]
        if check:
            for c in range(st.channels):
                seg = chans[c][bs:bs + nb]
                idx = np.flatnonzero((seg < lo) | (seg > hi))
                if idx.size:
                    bad[c] = int(idx[-1] if "any_bad" in faults else idx[0])
        t.badidx[b] = bad
        bp = t.bplans[b]
        bp["choose_ms"] = bp["uncertain"] = bp["est_ms"] = 0
        bp["frames"], bp["pad"] = nb, 0
        bp["invalid"] = int(bad[0] != NONE or bad[1] != NONE)
        order = (1, 0) if "right_first" in faults else (0, 1)
        bp["first_bad"] = next((bad[c] | (c << 31) for c in order if bad[c] != NONE), NONE)
        any_invalid = any_invalid or bool(bp["invalid"])
        nprobe = nfull = 0
        if not stereo:
            nfull = 0x1
        elif mode == 0:
            nfull = 0x3
        elif mode == 1:
            nfull, bp["choose_ms"] = 0xC, 1
        else:
            est_ms, uncertain, _, _, _ = estimate(sums12, nb, faults)
            if oracle is not None and not faults:
                o = oracle.stereo_estimate(st.left[bs:bs + nb], st.right[bs:bs + nb])
                assert (int(o.choose_ms), int(o.uncertain)) == (est_ms, uncertain), (st.name, b)
                est_ms, uncertain = int(o.choose_ms), int(o.uncertain)
            bp["est_ms"] = bp["choose_ms"] = est_ms
            bp["uncertain"] = uncertain
            silent = sums12[0] == 0 and sums12[1] == 0
            if not uncertain:
                nfull = 0xC if est_ms else 0x3
            elif nb <= LIMIT and not ("silent_small" in faults and silent):
                nfull = 0xF
            elif silent:
                nfull, bp["choose_ms"] = 0x3, 0
            else:
                nprobe = 0xFFF0
        t.need_probe[b], t.need_full[b] = nprobe, nfull
    t.strict[:] = not any_invalid
    return t


def concat(parts) -> Tables:
    return Tables(*[np.concatenate([getattr(p, f) for p in parts]) for f in
                    ("sums", "badidx", "acorr", "bplans", "need_probe", "need_full", "strict")])


def differences(want: Tables, got: Tables, what="") -> list:
    """Every word of `got` that is not `want`'s, as readable lines (an empty list: equal)."""
    out = []
    sent = sentinel_tables(1)

    def word(name, b, idx, g, w, s):
        tag = " (the sentinel: nothing may be written here)" if w == s else (" (the sentinel: never written)" if g == s else "")
        out.append(f"{what} block {b} {name}{list(idx)}: device {g:#x}, reference {w:#x}{tag}")

    for b in range(want.bplans.shape[0]):
        strict = bool(want.strict[b])
        for name in (("sums", "acorr") if strict else ()) + ("badidx", "need_probe", "need_full"):
            w, g = getattr(want, name)[b], getattr(got, name)[b]
            if not np.array_equal(w, g):
                s = int(getattr(sent, name).reshape(-1)[0])
                for idx in np.argwhere(np.atleast_1d(w != g))[:8]:
                    word(name, b, idx, int(np.atleast_1d(g)[tuple(idx)]), int(np.atleast_1d(w)[tuple(idx)]), s)
        for f in BPLAN.names if strict else ("invalid", "frames", "first_bad"):
            if want.bplans[b][f] != got.bplans[b][f]:
                out.append(f"{what} block {b} plan.{f}: device {int(got.bplans[b][f]):#x}, reference {int(want.bplans[b][f]):#x}")
    return out


# ---------------------------------------------------------------------------------------------------------------------
# content
# ---------------------------------------------------------------------------------------------------------------------
def _hash(n, seed):
    """n 64-bit words that depend on nothing but (index, seed): splitmix64."""
    x = np.arange(1, n + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64((seed * 0xD1B54A32D192ED03) & ((1 << 64) - 1))
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def noise(n, bits, seed):
    return ((_hash(n, seed) >> np.uint64(20)) % np.uint64(1 << bits)).astype(np.int64) - (1 << (bits - 1))


def walk(n, bits, step, seed):
    """A random walk with steps in [-step, step] that is folded back into the depth's range."""
    d = ((_hash(n, seed) >> np.uint64(20)) % np.uint64(2 * step + 1)).astype(np.int64) - step
    span = 1 << bits
    w = np.cumsum(d) % (2 * span - 2)  # a triangle wave of the unbounded walk: continuous, inside [-2^(bits-1), 2^(bits-1))
    w = np.where(w < span - 1, w, 2 * span - 2 - w)
    return w - (1 << (bits - 1))


def music(n, bits, seed):
    """Left / right with a common part and a small difference, some noise on top: a mix of estimates."""
    a, b = walk(n, bits - 1, 1 << (bits - 9), seed), walk(n, bits - 3, 1 << (bits - 11), seed + 1)
    c = noise(n, bits - 8, seed + 2)
    return a + b // 2, a - b // 2 + c


def _i32(x):
    return np.ascontiguousarray(x, dtype=np.int32)


def _stream(name, l, r, mode, depth, **kw):
    full = 1 << (depth - 1) if depth else 1 << 23
    kw.setdefault("layout", P32)
    return Stream(name, _i32(l), None if r is None else _i32(r), mode, depth, **kw), full


def boundary_1pct():
    """One block whose estimate sits exactly on the 1 % rule: diff == smaller // 100, nothing else uncertain.  Left is a
    staircase of `a` stairs of +2 on a pedestal of 3000, right the constant 1000: every channel's difference sum is by far
    its smallest (not `active`) and small enough for k = 0, so its bits are sum + n with
        sums  L 6000 + 4a   R 2000   M 4000 + 2a   S 4000 + 4a      (the head sample counts raw),
    lr = 8000 + 4a + 2n, ms - lr = 2a, and 2a == (8000 + 4a + 2n) // 100 at n = 16384, a = 208."""
    n, a = BLOCK, 208
    steps = np.zeros(n, dtype=np.int64)
    steps[8:8 + 3 * a:3] = 2
    return 3000 + np.cumsum(steps), np.full(n, 1000, dtype=np.int64)


@functools.lru_cache(maxsize=None)
def corpus():
    """name -> Stream: every distinct content / shape of the corpus, planar int32 at offset 0 unless named otherwise."""
    out = {}

    def add(name, l, r, mode, depth, **kw):
        st, _ = _stream(name, l, r, mode, depth, **kw)
        assert name not in out
        out[name] = st
        return st

    # block lengths: the thread seam and cnt 0..16, a tail wave on the per-sample path behind waves on the span path, the
    # tile seam and its carry, the full-compare limit on both sides
    for i, nb in enumerate(LENGTHS):
        depth = (16, 24)[i & 1]
        l, r = music(nb, depth, 100 + i)
        add(f"len{nb}", l, r, 2, depth)
    # streams and launch sets of 1, 7, 8, 9, 17, 33 blocks
    l, r = music(BLOCK + 1, 16, 201)
    add("s16385", l, None, 2, 16)
    l, r = music(2 * BLOCK + 300, 24, 202)
    add("s33068", l, r, 0, 24)
    add("s33068ms", l, r, 1, 24)
    l, r = music(2 * BLOCK + 5000, 16, 203)
    add("s37768", l, r + noise(l.size, 9, 204), 2, 16)
    l, r = music(7 * BLOCK - 100, 24, 207)
    add("b7", l, r, 2, 24)
    l, r = music(8 * BLOCK, 16, 208)
    add("b8", l, r, 0, 16)
    l, r = music(8 * BLOCK + 1, 24, 209)
    add("b9", l, r, 1, 24)
    l, r = music(17 * BLOCK - 4000, 24, 217)
    add("b17", l, None, 0, 24)
    l, r = music(33 * BLOCK - 12000, 16, 233)
    add("b33", l, r, 2, 16)
    # magnitudes
    fs = (1 << 23) - 1
    alt = np.where(np.arange(BLOCK) & 1, -fs, fs)
    add("alt_fs24", alt, -alt, 2, 24)                        # S = +-(2^24 - 2): lag 0 near 2^62, the odd lags near -2^62
    add("const_fs24", np.full(BLOCK + 17, fs), np.full(BLOCK + 17, -fs - 1), 2, 24)
    add("const_fs16", np.full(4113, 32767), None, 0, 16, layout=I16)
    add("const_min16", np.full(4113, -32768), np.full(4113, -32768), 2, 16, layout=I16)
    k = np.arange(15)
    add("neg_odd", -3 - 2 * k, np.zeros(15), 2, 16)          # L + R negative and odd: floor, not truncation
    l, r = np.zeros(2 * TILE + 1, dtype=np.int64), np.zeros(2 * TILE + 1, dtype=np.int64)
    l[TILE - 1], l[TILE], r[TILE - 1], r[TILE] = 5000000, -7000000, 3, -8000000
    add("impulses", l, r, 2, 24)                             # the last frame of a tile and the first of the next
    l, r = np.zeros(BLOCK + 5000, dtype=np.int64), np.zeros(BLOCK + 5000, dtype=np.int64)
    l[BLOCK - 1], r[BLOCK - 1] = 1000, -999
    add("tailzero", l, r, 2, 16)                             # block 1 all zero behind a non-zero last sample
    l, r = l.copy(), r.copy()
    l[BLOCK], r[BLOCK] = 7, 5
    add("tailhead", l, r, 2, 16)                             # ... and with a head sample that would meet that history
    add("big_sums", noise(BLOCK, 24, 301), noise(BLOCK, 24, 302), 2, 24)  # every one of the twelve sums above 2^32
    # validation: planar int32 one past either bound
    for depth in (16, 24):
        hi = (1 << (depth - 1)) - 1
        lo = -hi - 1
        bl, br = music(2 * TILE + 8, depth, 400 + depth)
        bl, br = np.clip(bl, lo + 1, hi - 1), np.clip(br, lo + 1, hi - 1)
        x = bl.copy()
        x[0] = hi + 1
        add(f"bad_first{depth}", x, br, 2, depth)
        x = br.copy()
        x[-1] = lo - 1
        add(f"bad_last{depth}", bl, x, 2, depth)             # right only: bit 31
        x = bl.copy()
        x[TILE - 1], x[TILE] = hi + 1, lo - 1
        add(f"bad_seam{depth}", x, None, 0, depth)
        x = bl.copy()
        x[TILE] = lo - 1
        add(f"bad_seam_next{depth}", x, None, 0, depth)
        x, y = bl.copy(), br.copy()
        x[[6000, 300, 8100]] = hi + 1, lo - 1, hi + 1
        y[100] = hi + 1
        add(f"bad_several{depth}", x, y, 0, depth)           # the lowest index; left before right
        x = br.copy()
        x[5] = hi + 1
        add(f"bad_ms{depth}", bl, x, 1, depth)               # forced mid/side still validates left / right
        l2, r2 = music(BLOCK + 50, depth, 420 + depth)
        l2, r2 = np.clip(l2, lo + 1, hi - 1), np.clip(r2, lo + 1, hi - 1)
        l2[BLOCK + 49] = lo - 1
        add(f"bad_block1_{depth}", l2, r2, 2, depth)
    bl, _ = music(300, 16, 440)
    x = bl.copy()
    x[17] = 40000
    add("bad_i24_d16", x, None, 0, 16, layout=I24)           # a 24-bit container at depth 16 validates
    add("wide_i24_d24", x * 100, x * 50, 2, 24, layout=I24)  # ... at depth 24 it does not
    # decisions
    z = np.zeros(5000, dtype=np.int64)
    add("zero_big", z, z, 2, 16)                             # silence above the limit: left/right, no probes
    y = z.copy()
    y[2500] = 1
    add("zero_big_r1", z, y, 2, 16)                          # one non-zero sample in R only: probes
    add("zero_small", z[:LIMIT], z[:LIMIT], 2, 16)           # uncertain at nb <= 4096: both pairs
    add("certain_lr", walk(6000, 15, 40, 501), np.zeros(6000), 2, 16)
    w = walk(6000, 15, 40, 502)
    add("certain_ms", w, w + 3 + (np.arange(6000) // 1500), 2, 16)
    add("boundary_1pct", *boundary_1pct(), 2, 16)
    # layouts: the same content in all three, on the span path and off it
    # (lay2 ends on a whole wave of full chunks: placed at the end of an allocation, the last span fetch ends with it;
    #  lay1 ends in a tail wave on the per-sample path behind waves on the span path -- an even number of frames, so that
    #  its int16 form can end an allocation on the 4-byte alignment the API asks for)
    l, r = music(BLOCK + 5120, 16, 600)
    add("lay2", l, r, 2, 16)
    add("lay1", l[:BLOCK + 4114], None, 0, 16)
    return out


LAYOUT_OFFSETS = {P32: (0, 4, 8, 12), I16: (0, 4, 8, 12), I24: (0, 4, 8, 12, 1, 2, 3)}


def layout_variants(name):
    """The stream `name` in every layout at every offset the API's rules allow, and once per layout at the very end of an
    allocation."""
    base = corpus()[name]
    out = []
    for layout, offsets in LAYOUT_OFFSETS.items():
        for off in offsets:
            out.append(base.variant(name=f"{name}|{LAYOUT_NAMES[layout]}+{off}", layout=layout, offset=off))
        out.append(base.variant(name=f"{name}|{LAYOUT_NAMES[layout]} at the end", layout=layout, at_end=True))
    return out


@functools.lru_cache(maxsize=None)
def tables():
    """The stream tables of the corpus: several streams in one launch set, mixing mono, LR, MS and per-block stereo and
    the depths; 23, 14 and 9 blocks."""
    c = corpus()
    return (
        LaunchSet("lengths", tuple(c[f"len{nb}"] for nb in LENGTHS), True),
        LaunchSet("mixed", (c["s16385"], c["s33068"], c["len4097"], c["s33068ms"], c["s37768"], c["alt_fs24"], c["bad_several16"]), True),
        LaunchSet("magnitudes", (c["const_fs24"], c["const_fs16"], c["impulses"], c["tailhead"], c["zero_big_r1"], c["big_sums"], c["neg_odd"]), True),
    )


_memo = {}


def expected(st: Stream, oracle=None) -> Tables:
    """expect_stream without faults, once per content and shape (layout and placement do not change a word)."""
    key = (id(st.left), id(st.right), st.stereo_mode, st.bit_depth, validates(st))
    if key not in _memo:
        _memo[key] = (expect_stream(st, oracle=oracle), st)  # (the stream is kept: its arrays' ids stay taken)
    return _memo[key][0]


def expected_set(ls: LaunchSet, oracle=None) -> Tables:
    return concat([expected(s, oracle) for s in ls.streams])
