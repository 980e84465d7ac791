"""Bit-compare off the device: where its expectations come from, the pairs the tests run on, and the CPU twin.

  window(x, lo, hi)                     frames lo .. hi - 1 of a stream, zeros outside it
  mismatches(a, b, o)                   mis[o] by the definition: zero-extend, shift, != -- never the code under test
  counts(pair) / choose(counts, ...)    mis[] over the pair's offsets, and the tie rule in plain Python
  rows(pair, o) / totals(pair, o, rows) the rows at an offset (abs, int64 sums) and the totals in Python integers
  mistaken(pair, kind)                  the answer a named mistake would give: what the corpus must tell from the right one
  corpus()                              frozen seeded pairs over every class the plan and the kernels tell apart
  run(case) / source_case / stream_case the CPU twin (tests/native/sim_compare.cpp: csrc/decode_plan.h's compare job,
                                        csrc/compare_plan.h, csrc/compare_core.h as the kernels run it, csrc/compare_rows.h)
  line / run_sanitized                  the same through the build with AddressSanitizer + UBSan, a program of its own
                                        (a sanitizer is never loaded into Python)
  cleared(key, cases)                   cases that may go to a device: the sanitized twin has passed them

Everything is exact integer arithmetic: answers are compared byte for byte."""
from __future__ import annotations

import ctypes as C
import struct
import sys
from collections import namedtuple

import numpy as np

import twinbuild

SRC = twinbuild.NATIVE + "/sim_compare.cpp"
ENV = dict(ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
NONE = (1 << 64) - 1
ROW, MAX_RADIUS = 16384, 32767
SIDE_NONE, SIDE_A, SIDE_B = 0, 1, 2
P32, I16, I24, P16, PF32, IF32 = 0, 1, 2, 16, 17, 18  # LACX_PCM_*
LAYOUTS_16 = (P32, I16, P16, PF32, IF32)
LAYOUTS_24 = (P32, I24, PF32, IF32)

CH_ROW_T = np.dtype([("first", "<u8"), ("last", "<u8"), ("max_at", "<u8"), ("sum_abs", "<u8"), ("sum_sq", "<u8"), ("mismatches", "<u4"), ("max_abs", "<u4")])
ROW_T = np.dtype([("ch", CH_ROW_T, (2,))])
CH_T = np.dtype([("mismatches", "<u8"), ("first", "<i8"), ("last", "<i8"), ("peak_at", "<i8"), ("sum_abs_lo", "<u8"), ("sum_abs_hi", "<u8"),
                 ("sum_sq_lo", "<u8"), ("sum_sq_hi", "<u8"), ("peak", "<u4"), ("reserved", "<u4")])
TOTAL_T = np.dtype([("offset", "<i8"), ("domain_first", "<i8"), ("domain_frames", "<u8"), ("frames_a", "<u8"), ("frames_b", "<u8"), ("mismatches", "<u8"),
                    ("first", "<i8"), ("last", "<i8"), ("peak_at", "<i8"), ("sum_abs_lo", "<u8"), ("sum_abs_hi", "<u8"), ("sum_sq_lo", "<u8"),
                    ("sum_sq_hi", "<u8"), ("rows", "<u8"), ("rows_differ", "<u8"), ("lead", "<u8"), ("tail", "<u8"), ("peak", "<u4"), ("sample_rate", "<u4"),
                    ("peak_channel", "u1"), ("channels", "u1"), ("bit_depth", "u1"), ("lead_side", "u1"), ("tail_side", "u1"), ("reserved", "u1", (3,)),
                    ("ch", CH_T, (2,))])
assert (CH_ROW_T.itemsize, ROW_T.itemsize, CH_T.itemsize, TOTAL_T.itemsize) == (48, 96, 72, 296)

# a, b: (channels, frames) int32; same: b is a itself (one source, named twice); planted: the offset the pair was built around
Pair = namedtuple("Pair", "name a b centre radius depth rate same planted", defaults=(16, 44100, False, None))


# ---- expectations -----------------------------------------------------------------------------------------------------
def window(x, lo, hi):
    """Frames lo .. hi - 1 of x (channels, n) as int64, zeros outside [0, n)."""
    out = np.zeros((x.shape[0], hi - lo), np.int64)
    a, b = max(lo, 0), min(hi, x.shape[1])
    if a < b:
        out[:, a - lo:b - lo] = x[:, a:b]
    return out


def domain(na, nb, o):
    return min(0, -o), max(na, nb - o)


def paired(a, b, o):
    """(f0, A, B): the union domain's first frame and both sides over it."""
    f0, f1 = domain(a.shape[1], b.shape[1], o)
    return f0, window(a, f0, f1), window(b, f0 + o, f1 + o)


def mismatches(a, b, o) -> int:
    _, A, B = paired(a, b, o)
    return int((A != B).sum())


def mismatches_restricted(a, b, o) -> int:
    """The same number without the stretch of the domain where both sides are zero: A against B's window over [0, na),
    and B's non-zero samples paired with frames outside it.  For the pair whose union domains would not fit."""
    na, nb = a.shape[1], b.shape[1]
    inside = int((a.astype(np.int64) != window(b, o, na + o)).sum())
    j = np.arange(nb) - o  # A's frame of B's frame j + o
    outside = (j < 0) | (j >= na)
    return inside + int(np.count_nonzero(b[:, outside]))


def counts_wide(a, b, centre, radius):
    """mismatches_restricted at every offset of a wide range at once: sliding windows over B padded with zeros."""
    na, nb = a.shape[1], b.shape[1]
    lo, hi = centre - radius, centre + radius
    pad_l, pad_r = max(0, -lo), max(0, na + hi - nb)
    bp = np.concatenate([np.zeros((b.shape[0], pad_l), np.int32), b, np.zeros((b.shape[0], pad_r), np.int32)], axis=1)  # bp[j + pad_l] = B(j)
    nz = np.concatenate([[0], np.cumsum(np.count_nonzero(bp, axis=0))])  # non-zero samples of B in front of a frame
    out = np.zeros(hi - lo + 1, np.uint64)
    for c in range(a.shape[0]):
        win = np.lib.stride_tricks.sliding_window_view(bp[c], na)  # win[k] = B(k - pad_l .. k - pad_l + na - 1)
        for k0 in range(0, hi - lo + 1, 4096):
            k1 = min(k0 + 4096, hi - lo + 1)
            out[k0:k1] += (win[lo + pad_l + k0:lo + pad_l + k1] != a[c]).sum(axis=1).astype(np.uint64)
    o = np.arange(lo, hi + 1)
    inside = nz[o + pad_l + na] - nz[o + pad_l]  # B's non-zero samples paired with frames [0, na)
    return out + (nz[-1] - inside).astype(np.uint64)


_counts = {}


def counts(p):
    """mis[] over centre - radius .. centre + radius as uint64, computed once per pair and shared."""
    if p.name not in _counts:
        if p.radius > 1000:
            c = counts_wide(p.a, p.b, p.centre, p.radius)
        else:
            c = np.array([mismatches(p.a, p.b, o) for o in range(p.centre - p.radius, p.centre + p.radius + 1)], np.uint64)
        c.setflags(write=False)
        _counts[p.name] = c
    return _counts[p.name]


def choose(c, centre, radius) -> int:
    """The fewest mismatches; ties to the smallest |o - centre|, then to the larger o."""
    offs = range(centre - radius, centre + radius + 1)
    return min(offs, key=lambda o: (int(c[o - (centre - radius)]), abs(o - centre), -o))


def rows(p, o):
    """The rows of the pair at offset o as ROW_T, by the definition."""
    f0, A, B = paired(p.a, p.b, o)
    d = A - B
    n = d.shape[1]
    out = np.zeros((n + ROW - 1) // ROW, ROW_T)
    out["ch"]["first"] = out["ch"]["last"] = out["ch"]["max_at"] = NONE
    for r in range(len(out)):
        for c in range(d.shape[0]):
            x = np.abs(d[c, r * ROW:(r + 1) * ROW])
            at = np.nonzero(x)[0]
            if not len(at):
                continue
            rec = out["ch"][r][c]
            rec["first"], rec["last"], rec["mismatches"] = r * ROW + at[0], r * ROW + at[-1], len(at)
            rec["max_abs"], rec["max_at"] = x.max(), r * ROW + int(np.argmax(x))  # (argmax: the lowest)
            rec["sum_abs"], rec["sum_sq"] = int(x.sum()), int((x * x).sum())
    return out


def totals(p, o, rws):
    """The totals in Python integers from rows (ROW_T) -> a TOTAL_T record."""
    na, nb, ch = p.a.shape[1], p.b.shape[1], p.a.shape[0]
    f0, f1 = domain(na, nb, o)
    t = np.zeros((), TOTAL_T)
    t["offset"], t["domain_first"], t["domain_frames"], t["frames_a"], t["frames_b"] = o, f0, f1 - f0, na, nb
    t["sample_rate"], t["channels"], t["bit_depth"], t["rows"] = p.rate, ch, p.depth, len(rws)
    t["rows_differ"] = sum(1 for r in rws if any(int(r["ch"][c]["mismatches"]) for c in range(ch)))
    all_abs = all_sq = all_mis = 0
    best = None  # (-peak, at, channel)
    firsts, lasts = [], []
    for c in range(ch):
        recs = [r["ch"][c] for r in rws if int(r["ch"][c]["mismatches"])]
        if not recs:
            continue
        x = t["ch"][c]
        mis, sa, sq = sum(int(r["mismatches"]) for r in recs), sum(int(r["sum_abs"]) for r in recs), sum(int(r["sum_sq"]) for r in recs)
        peak = max(int(r["max_abs"]) for r in recs)
        at = f0 + min(int(r["max_at"]) for r in recs if int(r["max_abs"]) == peak)
        x["mismatches"], x["first"], x["last"], x["peak"], x["peak_at"] = mis, f0 + int(recs[0]["first"]), f0 + int(recs[-1]["last"]), peak, at
        x["sum_abs_lo"], x["sum_abs_hi"], x["sum_sq_lo"], x["sum_sq_hi"] = sa & NONE, sa >> 64, sq & NONE, sq >> 64
        all_abs, all_sq, all_mis = all_abs + sa, all_sq + sq, all_mis + mis
        firsts.append(int(x["first"])), lasts.append(int(x["last"]))
        best = min(best, (-peak, at, c)) if best else (-peak, at, c)
    if best:
        t["mismatches"], t["first"], t["last"] = all_mis, min(firsts), max(lasts)
        t["peak"], t["peak_at"], t["peak_channel"] = -best[0], best[1], best[2]
        t["sum_abs_lo"], t["sum_abs_hi"], t["sum_sq_lo"], t["sum_sq_hi"] = all_abs & NONE, all_abs >> 64, all_sq & NONE, all_sq >> 64
    n = f1 - f0
    t["lead"], t["lead_side"] = min(abs(o), n), SIDE_NONE if o == 0 else SIDE_A if o < 0 else SIDE_B
    ea, eb = na, nb - o
    t["tail"], t["tail_side"] = min(abs(ea - eb), n), SIDE_NONE if ea == eb else SIDE_A if ea > eb else SIDE_B
    return t


Want = namedtuple("Want", "offset counts rows totals")
_want = {}


def expected(p):
    """What a pair's answer is held to, computed once and shared: the chosen offset, mis[] (empty at radius 0), the rows
    and the totals."""
    if p.name not in _want:
        c = counts(p) if p.radius else np.zeros(0, np.uint64)
        o = choose(c, p.centre, p.radius) if p.radius else p.centre
        r = rows(p, o)
        r.setflags(write=False)
        _want[p.name] = Want(o, c, r, totals(p, o, r))
    return _want[p.name]


# ---- mistakes: what a wrong implementation would answer -------------------------------------------------------------------
MISTAKES = ("no zero-extension at the start", "no zero-extension at the end", "< for <= at the last offset", "a B window one frame short",
            "o mod 4 != 0 read as aligned", "a negative frame rounded toward zero", "24-bit stereo compared on one word", "frames counted instead of samples",
            "lanes behind the last offset added in", "a row's position relative to the row", "the wrong tie rule")


def mistaken(p, kind):
    """(counts, offset, rows) as the named mistake would make them; compare with expected(p)."""
    w = expected(p)
    offs = list(range(p.centre - p.radius, p.centre + p.radius + 1))
    na, nb = p.a.shape[1], p.b.shape[1]

    def recount(f):
        return np.array([f(o) for o in offs], np.uint64) if p.radius else w.counts  # (radius 0: there are no counts)

    c, o, r = w.counts, w.offset, w.rows
    if kind == "no zero-extension at the start":  # the domain starts at 0: B's frames in front of A are never seen
        c = recount(lambda o: int((window(p.a, 0, max(na, nb - o)) != window(p.b, o, max(na, nb - o) + o)).sum()))
    elif kind == "no zero-extension at the end":  # the domain ends with A
        c = recount(lambda o: int((window(p.a, min(0, -o), na) != window(p.b, min(0, -o) + o, na + o)).sum()))
    elif not p.radius and kind in ("< for <= at the last offset", "a B window one frame short", "lanes behind the last offset added in"):
        pass
    elif kind == "< for <= at the last offset":  # the last offset is never counted
        c = w.counts.copy()
        c[-1] = 0
    elif kind == "a B window one frame short":  # the last frame the largest offset reaches reads as zero
        last = offs[-1]
        f1 = domain(na, nb, last)[1]
        short = p.b.copy()
        j = f1 - 1 + last
        if 0 <= j < nb:
            short[:, j] = 0
        c = w.counts.copy()
        c[-1] = mismatches(p.a, short, last)
    elif kind == "o mod 4 != 0 read as aligned":  # the rows pair A's unit with B's unit at the floored offset
        r = rows(p._replace(name=p.name + "|aligned"), w.offset - w.offset % 4)
    elif kind == "a negative frame rounded toward zero":  # B's frame -k of a unit read as frame 0's unit: frames shifted by the remainder
        c = recount(lambda o: mismatches(p.a, p.b, o if o >= 0 else -((-o) // 4 * 4) if (-o) % 4 else o))
    elif kind == "24-bit stereo compared on one word":  # only the left channel is compared
        c = recount(lambda o: mismatches(p.a[:1], p.b[:1], o))
    elif kind == "frames counted instead of samples":
        def frames(o):
            _, A, B = paired(p.a, p.b, o)
            return int((A != B).any(axis=0).sum())
        c = recount(frames)
    elif kind == "lanes behind the last offset added in":  # the offsets past the last fold back onto the last
        c = w.counts.copy()
        c[-1] += mismatches(p.a, p.b, offs[-1] + 1)
    elif kind == "a row's position relative to the row":
        r = w.rows.copy()
        for k in range(len(r)):
            for f in ("first", "last", "max_at"):
                v = r["ch"][f][k]
                r["ch"][f][k] = np.where(v == NONE, v, v - np.uint64(k * ROW))
    elif kind == "the wrong tie rule" and not p.radius:
        pass
    elif kind == "the wrong tie rule":  # the smaller offset wins a tie
        o = min(offs, key=lambda x: (int(w.counts[x - offs[0]]), abs(x - p.centre), x))
    else:
        raise KeyError(kind)
    if c is not w.counts and p.radius:
        o = choose(c, p.centre, p.radius)
    return c, o, r


def sees(p, kind) -> bool:
    """Whether the pair tells the mistake from the definition."""
    w = expected(p)
    c, o, r = mistaken(p, kind)
    return c.tobytes() != w.counts.tobytes() or o != w.offset or r.tobytes() != w.rows.tobytes()


# ---- pairs ----------------------------------------------------------------------------------------------------------------
def noise(frames, channels, depth, seed):
    g = np.random.default_rng(seed)
    lim = 1 << (depth - 1)
    return g.integers(-lim, lim, (channels, frames), dtype=np.int64).astype(np.int32)


def shifted(x, o, frames=None):
    """b with b[j] = x[j - o]: at offset o, A(f) = x[f] meets B(f + o) = x[f].  Frames shifted in are zeros."""
    n = x.shape[1] if frames is None else frames
    return window(x, -o, n - o).astype(np.int32)


def plant(b, where, seed):
    """b with a few samples changed (each to a value it did not have)."""
    b = b.copy()
    g = np.random.default_rng(seed)
    for ch, f in where:
        b[ch, f] = b[ch, f] + 1 if b[ch, f] < 0 else b[ch, f] - 1 - int(g.integers(0, 3))
    return b


def quiet_ends(x, n):
    """x with n silent frames at either end, as a disc has them: a drive-offset copy then loses nothing."""
    x = x.copy()
    x[:, :n] = 0
    x[:, x.shape[1] - n:] = 0
    return x


TILE = 2048  # the search tile's frames (asserted against the twin in the tests)
LENGTHS = (1, 2, 3, 4, 5, 6, 7, 8, 9, 4095, 4096, 4097, TILE - 1, TILE, TILE + 1, 16383, 16384, 16385, 2 * 16384 + 5)
PLANTED = (1, -1, 2, -2, 3, -3, 4, -4, 255, -255, 256, -256, 257, -257)
RADII = (0, 1, 127, 128, 300, 600)  # 600: more than one offset tile of 4 * 256 offsets

_corpus = None


def corpus():
    """Frozen seeds, every pair small.  See test_the_corpus_holds_its_classes for what it promises."""
    global _corpus
    if _corpus is not None:
        return _corpus
    ps, seed = [], 7100

    def add(name, a, b, centre=0, radius=0, depth=16, same=False, planted=None):
        ps.append(Pair(name, a, b, centre, radius, depth, 44100 if depth == 16 else 96000, same, planted))

    for k, n in enumerate(LENGTHS):  # lengths; na != nb both ways; mono / stereo and 16 / 24 in turn
        seed += 1
        ch, depth = 1 + k % 2, (16, 24)[(k // 2) % 2]
        x = noise(n, ch, depth, seed)
        other = noise(n + 1 + k % 3, ch, depth, seed + 500)
        other[:, :n] = x  # b = a and a little more: the tail differs
        add("len|%d" % n, x, other, 0, min(3, n) if k % 4 else 0, depth)
        add("len|%d|longer-a" % n, other, x, 0, 1, depth)
    for depth in (16, 24):  # both ends of the range: |d| reaches 2^b - 1
        lim = 1 << (depth - 1)
        for ch in (1, 2):
            a = np.full((ch, 37), lim - 1, np.int32)
            b = np.full((ch, 37), -lim, np.int32)
            a[:, 5:9] = -lim
            b[:, 5:9] = lim - 1
            add("range|%d|%d" % (depth, ch), a, b, 0, 2, depth)
    x = noise(5000, 2, 16, 7300)
    add("identical", x, x.copy(), 0, 8)
    add("same-index", x, x, 0, 5, same=True)
    base = {(ch, depth): quiet_ends(noise(6000, ch, depth, 7400 + 10 * ch + depth), 400) for ch in (1, 2) for depth in (16, 24)}
    for k, o in enumerate(PLANTED):  # drive-offset copies, with and without a few differing samples
        ch, depth = 1 + k % 2, (16, 24)[(k // 2) % 2]
        x = base[(ch, depth)]
        radius = (300, 300, 127, 128)[k % 4] if abs(o) < 100 else 300
        add("shift|%d" % o, x, shifted(x, o), 0, radius, depth, planted=o)
        add("shift|%d|diffs" % o, x, plant(shifted(x, o), [(0, 1000), (ch - 1, 3000), (0, 4501)], 7500 + k), 0, radius, depth, planted=o)
    for r in (1, 127, 128, 300):  # the planted offset at +- radius exactly
        x = base[(2, 16)]
        add("edge|+%d" % r, x, shifted(x, r), 0, r, planted=r)
        add("edge|-%d" % r, x, plant(shifted(x, -r), [(1, 2000)], 7600 + r), 0, r, planted=-r)
    x = base[(2, 24)]
    add("edge|centre", x, shifted(x, 1000 + 128), 1000, 128, 24, planted=1128)  # a centre != 0, the planted offset at its edge
    # a tie: audio of period 8 gives equal counts 8 offsets apart; +4 and -4 tie around centre 0 and the larger wins
    # (b is a rotated by half a period, every sample non-zero: both offsets lose half a period at either end)
    period = np.tile(noise(8, 2, 16, 7700) | 1, (1, 500))
    add("tie", period, np.roll(period, 4, axis=1), 0, 5)
    tie2 = np.tile(noise(4, 1, 16, 7701) | 1, (1, 300))
    add("tie|mono", tie2, np.roll(tie2, 2, axis=1), 0, 2)
    # a window beyond both streams entirely: every offset counts all non-zero samples
    y = noise(700, 2, 16, 7800)
    add("beyond", y, noise(900, 2, 16, 7801), 5000, 40)
    add("beyond|negative", y, noise(900, 2, 16, 7801), -5000, 3)
    # the largest radius against a few thousand frames
    z = quiet_ends(noise(3000, 2, 16, 7900), 100)
    add("r32767", z, shifted(z, 20000, 3000 + 20000), 0, 32767, planted=20000)
    # where the differences lie
    x = noise(40000, 2, 16, 8000)
    add("right-only", x, plant(x, [(1, 3), (1, 16383), (1, 16384), (1, 39999)], 8001), 0, 0)
    lead = np.concatenate([noise(5, 2, 16, 8002), x[:, :9000]], axis=1)
    add("lead-only", x[:, :9000], lead, 5, 0)    # b = five frames of its own, then a: at offset 5 only the lead differs
    add("tail-only", x[:, :9000], np.concatenate([x[:, :9000], noise(7, 2, 16, 8003)], axis=1), 0, 2)
    last = x[:, :2 * ROW].copy()
    last[0, ROW - 1] ^= 1
    add("row-last-frame", x[:, :2 * ROW], last, 0, 0)
    m = noise(20000, 1, 24, 8100)
    add("mono24|row2", m, plant(m, [(0, ROW + 7)], 8101), 0, 1, 24)
    for r in RADII:  # every split of a workgroup the plan has, and more than one offset tile
        x = base[(2, 16)]
        add("radius|%d" % r, x, plant(shifted(x, min(r, 2)), [(0, 777)], 8200 + r), 0, r)
    assert len({p.name for p in ps}) == len(ps)
    _corpus = ps
    return _corpus


def small_corpus():
    return [p for p in corpus() if p.name != "r32767"]


# ---- a pair's answer, whoever made it -------------------------------------------------------------------------------------
def check(p, got, what=""):
    """One pair of the twin (or of the device, as a TwinPair) against the restatement, byte for byte."""
    w = expected(p)
    assert got.code == 0, (p.name, what, got.text)
    assert got.counts.dtype == np.uint64 and got.counts.tobytes() == w.counts.tobytes(), (p.name, what, "counts")
    assert int(got.totals["offset"]) == w.offset, (p.name, what, int(got.totals["offset"]), w.offset)
    assert got.rows.tobytes() == w.rows.tobytes(), (p.name, what, "rows")
    assert got.totals.tobytes() == w.totals.tobytes(), (p.name, what, "totals")


# ---- the twin ---------------------------------------------------------------------------------------------------------
_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(twinbuild.shared_lib("sim_compare", [SRC]))
        _lib.sim_cmp_run.restype = C.c_int64
        _lib.sim_cmp_choose.restype = C.c_int64
        for f in ("sim_cmp_tile_frames", "sim_cmp_row_frames", "sim_cmp_max_radius"):
            getattr(_lib, f).restype = C.c_uint32
    return _lib


def sanitized_exe():
    """The sanitized program's path, or (None, why) where the sanitizer runtime is missing."""
    return twinbuild.sanitized_exe("sim_compare_san", [SRC], ["-DSIM_COMPARE_MAIN"])


def job(pairs):
    """Corpus pairs as one job: (sources, [(a, b, centre, radius)]); a pair marked `same` names one source twice."""
    sources, recs = [], []
    for p in pairs:
        ia = len(sources)
        sources.append((p.a, p.depth, p.rate))
        if p.same:
            ib = ia
        else:
            ib = len(sources)
            sources.append((p.b, p.depth, p.rate))
        recs.append((ia, ib, p.centre, p.radius))
    return sources, recs


def _head(form, sources, recs):
    return struct.pack("<BII", form, len(sources), len(recs)) + b"".join(struct.pack("<IIqI", a, b, c, r) for a, b, c, r in recs)


def layout_for(layout, depth):
    """The layout itself where it can hold the depth, else planar int32."""
    return layout if layout in (LAYOUTS_16 if depth == 16 else LAYOUTS_24) else P32


def source_case(sources, recs, layout=P32, offset=0, bad=None) -> bytes:
    """sources: [(pcm (channels, frames) int32, depth, rate)] as one source job, every source in `layout` (where it holds the
    depth) at base offset `offset`.  bad = (source, frame, channel, raw 32-bit word): that element of a 4-byte layout is
    the raw word instead."""
    out = [_head(1, sources, recs)]
    for i, (x, depth, rate) in enumerate(sources):
        bf, bc, bw = bad[1:] if bad and bad[0] == i else (NONE, 0, 0)
        lay = layout_for(layout, depth)
        off = offset if lay == layout else (offset + 3) // 4 * 4  # (planar int32 in the other's place: 4-byte aligned, as the ABI asks)
        out.append(struct.pack("<IIIIIQQII", lay, off, x.shape[0], depth, rate, x.shape[1], bf, bc, bw))
        right = x[1] if x.shape[0] == 2 else np.zeros(x.shape[1], np.int32)
        out.append(np.asarray(x[0], "<i4").tobytes() + np.asarray(right, "<i4").tobytes())
    return b"".join(out)


def stream_case(lacs, recs) -> bytes:
    out = [_head(0, lacs, recs)]
    for x in lacs:
        out.append(struct.pack("<Q", len(x)) + x)
    return b"".join(out)


def encode(oracle, sources):
    return [oracle.encode(x[0], x[1] if x.shape[0] == 2 else None, rate, depth, 2) for x, depth, rate in sources]


TwinPair = namedtuple("TwinPair", "code text totals rows counts")
_vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731


def run(case: bytes):
    """A case on the plain twin -> [TwinPair] (rows ROW_T, counts uint64, totals a TOTAL_T record; None for a pair without
    an answer)."""
    _, ns, n = struct.unpack_from("<BII", case, 0)
    recs = [struct.unpack_from("<IIqI", case, 9 + 20 * k) for k in range(n)]
    rows_cap = n * 8 + len(case) // (4 * ROW) * 4 + sum(abs(c) + r for _, _, c, r in recs) // ROW * 2 + 64
    counts_cap = sum(2 * r + 1 for _, _, _, r in recs) + 1
    rec, tot = np.zeros(4 * n, np.uint64), np.zeros(n, TOTAL_T)
    rws, cnt = np.zeros(rows_cap, ROW_T), np.zeros(counts_cap, np.uint64)
    msg = C.create_string_buffer(1 << 16)
    got = lib().sim_cmp_run(case, C.c_uint64(len(case)), _vp(rec), _vp(tot), _vp(rws), C.c_uint64(rows_cap), _vp(cnt), C.c_uint64(counts_cap), msg,
                            C.c_uint32(len(msg)))
    assert got >= 0, "the twin could not run the case"
    texts = msg.value.decode().split("\n")
    out, at, ct = [], 0, 0
    for k in range(n):
        code, nr, nc = (int(v) for v in rec[4 * k:4 * k + 3])
        if code:
            out.append(TwinPair(code, texts[k], tot[k].copy(), None, None))
            continue
        out.append(TwinPair(0, "", tot[k].copy(), rws[at:at + nr].copy(), cnt[ct:ct + nc].copy()))
        at, ct = at + nr, ct + nc
    return out


def twin_combine(rws, channels, depth, rate, na, nb, o):
    out = np.zeros((), TOTAL_T)
    rws = np.ascontiguousarray(rws)
    lib().sim_cmp_combine(_vp(rws), C.c_uint64(len(rws)), C.c_uint8(channels), C.c_uint8(depth), C.c_uint32(rate), C.c_uint64(na), C.c_uint64(nb),
                          C.c_int64(o), _vp(out))
    return out


def twin_choose(c, centre, radius) -> int:
    c = np.ascontiguousarray(c, np.uint64)
    return int(lib().sim_cmp_choose(_vp(c), C.c_int64(centre), C.c_uint32(radius)))


Plan = namedtuple("Plan", "rc why tiles spans lanes otiles rows counts size bound_ok span_at")


def twin_plan(na, nb, centre=0, radius=0, fmt_a=(44100, 2, 16), fmt_b=(44100, 2, 16), ia=0, ib=1, nsrc=2):
    out = np.zeros(16, np.int64)
    why = C.create_string_buffer(256)
    rc = lib().sim_cmp_plan(C.c_uint64(na), C.c_uint64(nb), C.c_uint32(fmt_a[0]), C.c_uint32(fmt_b[0]), C.c_uint32(fmt_a[1]), C.c_uint32(fmt_b[1]),
                            C.c_uint32(fmt_a[2]), C.c_uint32(fmt_b[2]), C.c_uint32(ia), C.c_uint32(ib), C.c_uint32(nsrc), C.c_int64(centre),
                            C.c_uint32(radius), _vp(out), why, C.c_uint32(len(why)))
    v = [int(x) for x in out]
    return Plan(rc, why.value.decode(), v[0], v[1], v[2], v[3], v[4], v[5], v[6], bool(v[7]), [(v[8 + 2 * i], v[9 + 2 * i]) for i in range(v[1])])


# ---- the sanitized program ----------------------------------------------------------------------------------------------
def line(case: bytes, index: int) -> str:
    """The plain build's line for a case (what the sanitized program must print for it)."""
    buf = C.create_string_buffer(1 << 20)
    rc = lib().sim_cmp_line(case, C.c_uint64(len(case)), C.c_uint32(index), buf, C.c_uint32(len(buf)))
    assert rc == 0
    return buf.value.decode()


def run_sanitized(cases, exe=None, workers=8):
    """Every case through the sanitized program, split over a few processes: (lines, returncode, stderr)."""
    if exe is None:
        exe, why = sanitized_exe()
        assert exe, why
    return twinbuild.run_cases(exe, cases, ENV, workers=workers, prefix="lac_cmp_")


def cleared(key, cases):
    """cases, once the sanitized twin has shown in this run that a compare job over each stays inside buffers of exactly the
    plan's capacities and answers as the plain build does.  Fails, never skips, where that cannot be shown."""
    def make():
        return list(cases), lambda c, i: line(c, i).split(" ", 1)[1], None, list(cases)

    return twinbuild.cleared("compare", key, sys.modules[__name__], make)
