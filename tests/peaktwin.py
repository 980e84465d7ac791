"""True peak off the device: where its expectations come from, the signals the tests run on, and the CPU twin.

  TABLE                                 the BS.1770-4 Annex 2 coefficients times 8192, written down here a second time
  oversampled(x)                        np.convolve of the int64 channel with each phase: y[n, p], n = 0 .. frames + 10
  expected_rows(left, right)            maxima, first positions and rows from it in numpy -- never the code under test
  expected_totals(sets)                 the totals of rows, restated in Python integers and floats
  corpus()                              frozen seeded items over history, tile, row and flush borders
  ebu_cases() / ebu_item                the sine cases of EBU Tech 3341 (15 - 19)
  run(lacs) / run_sources(...)          the CPU twin (tests/native/sim_truepeak.cpp: csrc/decode_plan.h's true-peak job and
                                        csrc/truepeak_core.h as k_truepeak runs it), plain build
  case / source_case / line / run_sanitized   the same through the build with AddressSanitizer + UBSan, a program of its own
                                        (a sanitizer is never loaded into Python)
  cleared(key, lacs)                    streams that may go to a device: the sanitized twin has passed them

Everything is exact integer arithmetic up to the three doubles of the totals: rows are compared byte for byte."""
from __future__ import annotations

import ctypes as C
import math
import struct
import sys
from collections import namedtuple

import numpy as np

import dectwin
import salvagetwin
import twinbuild

SRC = twinbuild.NATIVE + "/sim_truepeak.cpp"
ENV = dict(ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
FORMATS = ((1, 16, 44100), (2, 16, 48000), (1, 24, 96000), (2, 24, 192000))  # loudtwin.FORMATS
TILE, ROW, TAPS, FLUSH = 1024, 16384, 12, 11
OVER, SAMPLE_FULL = 1, 2
CLEAN = (1 << 64) - 1
NONE = (1 << 64) - 1

_C0 = (14, 90, -161, 272, -487, 1125, 7964, -838, 390, -218, 122, -68)
_C1 = (-239, 240, -424, 730, -1364, 3810, 6388, -1641, 832, -477, 271, -155)
TABLE = np.array([_C0, _C1, _C1[::-1], _C0[::-1]], np.int64)
TABLE.setflags(write=False)

ROW_T = np.dtype([("peak", "<u8", (2,)), ("pos", "<u4", (2,)), ("sample_peak", "<u4", (2,))])
CH_T = np.dtype([("peak", "<u8"), ("position", "<u8"), ("sample_peak", "<u4"), ("sample_peak_row", "<u4")])
TOT_T = np.dtype([("frames", "<u8"), ("rate", "<u4"), ("channels", "u1"), ("depth", "u1"), ("flags", "u1"), ("peak_channel", "u1"),
                  ("rows", "<u4"), ("set", "<u4"), ("ch", CH_T, (2,)), ("true_peak", "<f8"), ("dbtp", "<f8"), ("sample_dbfs", "<f8")])
assert (ROW_T.itemsize, CH_T.itemsize, TOT_T.itemsize) == (32, 24, 96)


# ---- expectations -----------------------------------------------------------------------------------------------------
def oversampled(x):
    """(frames + 11, 4) int64: y[n, p] = sum_k TABLE[p][k] x[n - k], x zero outside the item -- the full convolution."""
    x = np.asarray(x, np.int64)
    return np.stack([np.convolve(x, TABLE[p]) for p in range(4)], axis=1)


def expected_rows(left, right):
    """ROW_T[ceil(frames / 16384)]: per row and channel max |y|, its first position 4 (n - 16384 row) + p (0 for a zero
    peak) and max |x|; output n belongs to row min(n, frames - 1) // 16384.  A mono item's second channel is zero."""
    frames = len(left)
    nrows = (frames + ROW - 1) // ROW
    out = np.zeros(nrows, ROW_T)
    for c, x in enumerate((left, right)):
        if x is None:
            continue
        y = np.abs(oversampled(x)).reshape(-1)  # index 4 n + p
        ax = np.abs(np.asarray(x, np.int64))
        for r in range(nrows):
            first = ROW * r
            end = ROW * (r + 1) if r + 1 < nrows else frames + FLUSH  # the flush frames go to the last row
            seg = y[4 * first:4 * end]
            peak = int(seg.max())
            out[r]["peak"][c] = peak
            out[r]["pos"][c] = int(np.argmax(seg)) if peak else 0  # argmax: the first that attains it
            out[r]["sample_peak"][c] = int(ax[first:min(frames, ROW * (r + 1))].max())
    return out


Channel = namedtuple("Channel", "peak position sample_peak sample_peak_row")
Totals = namedtuple("Totals", "frames rate channels depth flags peak_channel rows set ch true_peak dbtp sample_dbfs")


def _set_totals(rows, channels, depth, frames, rate):
    ch = []
    for c in range(2):
        peak = position = sample = sample_row = 0
        for i, r in enumerate(rows):
            if c < channels and int(r["peak"][c]) > peak:
                peak, position = int(r["peak"][c]), 4 * ROW * i + int(r["pos"][c])
            if c < channels and int(r["sample_peak"][c]) > sample:
                sample, sample_row = int(r["sample_peak"][c]), i
        ch.append(Channel(peak, position, sample, sample_row))
    full = 1 << (depth - 1)
    who = 1 if ch[1].peak > ch[0].peak else 0
    peak, sample = ch[who].peak, max(ch[0].sample_peak, ch[1].sample_peak)
    flags = (OVER if peak > 8192 * full else 0) | (SAMPLE_FULL if sample >= full - 1 else 0)
    tp = peak / (8192.0 * full)
    return Totals(frames, rate, channels, depth, flags, who, len(rows), 0, tuple(ch), tp, 20.0 * math.log10(tp) if peak else -math.inf,
                  20.0 * math.log10(sample / full) if sample else -math.inf)


def expected_totals(sets):
    """sets: [(rows ROW_T, channels, depth, frames, rate)] -> Totals.  Several sets: the set with the largest peak, depths
    compared exactly (a 16-bit peak shifted by 8), the lowest index on ties; frames and rows summed, flags of all, the largest
    sample_dbfs of all."""
    per = [_set_totals(*s) for s in sets]
    norm = [t.ch[t.peak_channel].peak << (24 - t.depth) for t in per]
    w = norm.index(max(norm))
    flags = 0
    for t in per:
        flags |= t.flags
    return per[w]._replace(set=w, frames=sum(t.frames for t in per), rows=sum(t.rows for t in per), flags=flags, sample_dbfs=max(t.sample_dbfs for t in per))


# ---- records, whoever made them ---------------------------------------------------------------------------------------
def rows_of(records):
    """ctypes TruePeakRow records (the product's) or a ROW_T array (the twin's) -> a ROW_T array."""
    if isinstance(records, np.ndarray):
        return records
    return np.frombuffer(bytes(records) if isinstance(records, C.Array) else b"".join(bytes(r) for r in records), ROW_T)


def totals_of(record):
    t = record if isinstance(record, (np.void, np.ndarray)) else np.frombuffer(bytes(record), TOT_T)[0]
    ch = tuple(Channel(int(c["peak"]), int(c["position"]), int(c["sample_peak"]), int(c["sample_peak_row"])) for c in t["ch"])
    return Totals(int(t["frames"]), int(t["rate"]), int(t["channels"]), int(t["depth"]), int(t["flags"]), int(t["peak_channel"]), int(t["rows"]),
                  int(t["set"]), ch, float(t["true_peak"]), float(t["dbtp"]), float(t["sample_dbfs"]))


ZERO_TOTALS = totals_of(np.zeros(1, TOT_T)[0])


def same_totals(got, want):
    """Integers and the exact true_peak equal; the two logarithms within 1e-12 dB (equal where infinite)."""
    assert got[:10] == want[:10], (got, want)
    for g, w in zip(got[10:], want[10:]):
        assert (g == w) if math.isinf(w) or math.isinf(g) else abs(g - w) <= 1e-12, (got, want)


# ---- signals ----------------------------------------------------------------------------------------------------------
Item = namedtuple("Item", "name channels depth rate left right")
FRAME_COUNTS = (1, 3, 4, 5, 11, 12, 13,  # shorter than the history
                1013, 1014,  # frames + 11 fills one tile exactly; a second tile holding only flush outputs
                1023, 1024, 1025, 1035, 16373, 16384, 16385, 32768 + 7)


def _noise(frames, depth, seed):
    lim = 1 << (depth - 1)
    return np.random.default_rng(seed).integers(-lim, lim, frames, dtype=np.int64).astype(np.int32)


def _impulses(frames, at):
    x = np.zeros(frames, np.int32)
    for q, v in at:
        x[q] = v
    return x


def worst_case(depth, negative=False):
    """Twelve samples x[n - k] = sign(c[1][k]) * full scale (negative: the opposite signs), in time order."""
    lo, hi = -(1 << (depth - 1)), (1 << (depth - 1)) - 1
    s = [(hi if (c > 0) != negative else lo) for c in _C1]
    return np.array(s[::-1], np.int32)  # x[n - 11] .. x[n]


_corpus = None


def corpus():
    """Frozen seeds.  Per format: noise at every frame count.  Then, at 16 and 24 bit: unit and full-scale impulses at frame
    0, at the last frame, and around n = 1023 / 1024 and 16383 / 16384, so that the maximum (five frames behind an impulse,
    phase 3: TABLE[3][5] = TABLE[0][6] = 7964 tie, the lower position wins) falls on either side of tile and row borders and
    into the flush tail; the worst-case sign pattern and its negative across a tile border; full negative scale throughout;
    two equal peaks in one row and in two; channels with different peaks; a silent channel."""
    global _corpus
    if _corpus is not None:
        return _corpus
    items, seed = [], 9000
    for ch, depth, rate in FORMATS:
        for frames in FRAME_COUNTS:
            seed += 1
            items.append(Item("noise|n%d|%dch%d" % (frames, ch, depth), ch, depth, rate, _noise(frames, depth, 2 * seed),
                              _noise(frames, depth, 2 * seed + 1) if ch == 2 else None))
    for depth, rate in ((16, 48000), (24, 192000)):
        lo, hi = -(1 << (depth - 1)), (1 << (depth - 1)) - 1
        tag = "2ch%d" % depth

        def add(name, left, right):
            items.append(Item("%s|%s" % (name, tag), 2, depth, rate, left, right))

        for border, frames in ((TILE, TILE + 16), (ROW, ROW + 16)):
            for d in (-12, -11, -6, -5, -1, 0, 1, 11):  # the peak lies at border + d + 5
                q = border + d
                add("impulse|b%d%+d" % (border, d), _impulses(frames, [(q, 1)]), _impulses(frames, [(q, lo if d % 2 else hi)]))
        for frames in (1, 12, TILE, TILE + 1, ROW, ROW + 1):  # at frame 0 and at the last frame: the peak in the flush tail
            add("impulse|ends%d" % frames, _impulses(frames, [(0, hi)]), _impulses(frames, [(frames - 1, lo)]))
        for neg in (False, True):
            x = np.zeros(2000, np.int32)
            x[TILE - 5:TILE + 7] = worst_case(depth, neg)  # twelve samples astride the tile border
            add("worst|%s" % ("neg" if neg else "pos"), x, x[::-1].copy())
        add("dc|full-negative", np.full(ROW + 5, lo, np.int32), np.full(ROW + 5, hi, np.int32))
        add("ties|one-row", _impulses(6000, [(100, 1000), (5000, 1000)]), _impulses(6000, [(5000, -1000), (100, 1000)]))
        add("ties|two-rows", _impulses(ROW + 3000, [(200, hi), (ROW + 2000, hi)]), _impulses(ROW + 3000, [(ROW + 2000, 7), (ROW - 3, 7)]))
        add("silent-right", _noise(1500, depth, 77 + depth), np.zeros(1500, np.int32))
        items.append(Item("impulse|mono-last|1ch%d" % depth, 1, depth, 44100 if depth == 16 else 96000, _impulses(TILE + 2, [(TILE + 1, lo)]), None))
    assert len({it.name for it in items}) == len(items)
    _corpus = items
    return _corpus


_expected = {}


def item_rows(it):
    """The expectation of an item's rows, computed once and shared (callers do not change it)."""
    if it.name not in _expected:
        rows = expected_rows(it.left, it.right)
        rows.setflags(write=False)
        _expected[it.name] = rows
    return _expected[it.name]


def item_totals(it):
    return expected_totals([(item_rows(it), it.channels, it.depth, len(it.left), it.rate)])


def ebu_cases():
    """[(name, divisor of fs, phase in degrees, amplitude)]: the sine cases 15 - 19 of EBU Tech 3341."""
    return [("15", 4, 0.0, 0.5), ("16", 4, 45.0, 0.5), ("17", 6, 60.0, 0.5), ("18", 8, 67.5, 0.5), ("19", 4, 45.0, 1.4125)]


def ebu_item(name, div, phase, amp, depth, rate=48000):
    """One second at `rate`, a sine at rate / div with a 0.1 s linear fade in and out, rounded and clipped to the depth (an
    amplitude above 1 clips, as the standard's +3 dB case does)."""
    n = np.arange(rate, dtype=np.float64)
    fade = np.minimum(1.0, np.minimum(n, rate - 1 - n) / (0.1 * rate))
    full = float(1 << (depth - 1))
    x = np.rint(amp * full * fade * np.sin(2.0 * np.pi * n / div + math.radians(phase)))
    x = np.clip(x, -full, full - 1).astype(np.int32)
    return Item("ebu%s|2ch%d" % (name, depth), 2, depth, rate, x, x.copy())


# ---- the twin ---------------------------------------------------------------------------------------------------------
_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(twinbuild.shared_lib("sim_truepeak", [SRC]))
        _lib.sim_peak_streams.restype = C.c_int64
        _lib.sim_peak_sources.restype = C.c_int64
        _lib.sim_peak_table.restype = None
        _lib.sim_peak_combine.restype = None
    return _lib


def sanitized_exe():
    """The sanitized program's path, or (None, why) where the sanitizer runtime is missing."""
    return twinbuild.sanitized_exe("sim_truepeak_san", [SRC], ["-DSIM_TRUEPEAK_MAIN"])


def twin_table():
    out = np.zeros(48, np.int32)
    lib().sim_peak_table(out.ctypes.data_as(C.c_void_p))
    return out.reshape(4, 12)


TwinItem = namedtuple("TwinItem", "code message status rows totals")
_vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731


def run(lacs):
    """n streams as one true-peak job on the CPU twin -> [TwinItem] (rows: ROW_T, or None without a result)."""
    n = len(lacs)
    ptrs = (C.c_char_p * n)(*lacs)
    sizes = (C.c_uint64 * n)(*[len(x) for x in lacs])
    cap = n + sum(sum(dectwin._shape(x)[1]) // ROW for x in lacs if salvagetwin._head_ok(x))
    rec = np.zeros(3 * n, np.uint64)
    rows = np.zeros(cap, ROW_T)
    totals = np.zeros(n, TOT_T)
    msg = C.create_string_buffer(1 << 16)
    got = lib().sim_peak_streams(ptrs, sizes, C.c_uint32(n), _vp(rec), _vp(rows), C.c_uint64(cap), _vp(totals), msg, C.c_uint32(len(msg)))
    assert got >= 0, "the twin could not run the job"
    msgs = msg.value.decode().split("\n")
    items, at = [], 0
    for i in range(n):
        code, nr, status = int(rec[3 * i]), int(rec[3 * i + 1]), int(rec[3 * i + 2])
        if code or status:
            items.append(TwinItem(code, msgs[i], status, None, totals_of(totals[i])))
            continue
        items.append(TwinItem(0, "", 0, rows[at:at + nr].copy(), totals_of(totals[i])))
        at += nr
    return items


SourceSpec = namedtuple("SourceSpec", "layout channels depth rate offset left right bad", defaults=(None,))
SourceOut = namedtuple("SourceOut", "key message rows totals")


def run_sources(specs):
    """[SourceSpec] as one source job on the twin -> [SourceOut].  bad = (frame, channel, raw 32-bit word)."""
    n = len(specs)
    u32 = lambda xs: np.array(xs, np.uint32)  # noqa: E731
    samples = [np.ascontiguousarray(np.concatenate([np.asarray(s.left, np.int32)] + ([np.asarray(s.right, np.int32)] if s.channels == 2 else [])))
               for s in specs]
    ptrs = (C.c_void_p * n)(*[x.ctypes.data for x in samples])
    frames = np.array([len(s.left) for s in specs], np.uint64)
    bad = [s.bad if s.bad else (NONE, 0, 0) for s in specs]
    cap = int(sum(len(s.left) // ROW + 1 for s in specs))
    rows, counts, totals, keys = np.zeros(cap, ROW_T), np.zeros(n, np.uint32), np.zeros(n, TOT_T), np.zeros(n, np.uint64)
    msg = C.create_string_buffer(1 << 14)
    got = lib().sim_peak_sources(C.c_uint32(n), _vp(u32([s.layout for s in specs])), _vp(u32([s.channels for s in specs])),
                                 _vp(u32([s.depth for s in specs])), _vp(u32([s.rate for s in specs])), _vp(u32([s.offset for s in specs])),
                                 _vp(frames), ptrs, _vp(np.array([b[0] for b in bad], np.uint64)), _vp(u32([b[1] for b in bad])),
                                 _vp(u32([b[2] for b in bad])), _vp(rows), C.c_uint64(cap), _vp(counts), _vp(totals), _vp(keys), msg, C.c_uint32(len(msg)))
    assert got >= 0, "the twin could not run the sources"
    msgs = msg.value.decode().split("\n")
    out, at = [], 0
    for k in range(n):
        if int(keys[k]) != CLEAN:
            out.append(SourceOut(int(keys[k]), msgs[k], None, totals_of(totals[k])))
            continue
        out.append(SourceOut(CLEAN, "", rows[at:at + int(counts[k])].copy(), totals_of(totals[k])))
        at += int(counts[k])
    return out


def twin_combine(sets):
    """csrc/truepeak_rows.h's totals of [(rows ROW_T, channels, depth, frames, rate)] -> Totals."""
    n = len(sets)
    arrays = [np.ascontiguousarray(np.asarray(s[0], ROW_T)) for s in sets]
    ptrs = (C.c_void_p * n)(*[a.ctypes.data for a in arrays])
    out = np.zeros(1, TOT_T)
    lib().sim_peak_combine(ptrs, _vp(np.array([len(a) for a in arrays], np.uint32)), _vp(np.array([s[1] for s in sets], np.uint8)),
                           _vp(np.array([s[2] for s in sets], np.uint8)), _vp(np.array([s[3] for s in sets], np.uint64)),
                           _vp(np.array([s[4] for s in sets], np.uint32)), C.c_uint32(n), _vp(out))
    return totals_of(out[0])


# ---- the sanitized program ----------------------------------------------------------------------------------------------
def case(lacs) -> bytes:
    body = struct.pack("<I", len(lacs))
    for x in lacs:
        body += struct.pack("<Q", len(x)) + x
    return b"\0" + body


def source_case(spec) -> bytes:
    samples = np.concatenate([np.asarray(spec.left, np.int32)] + ([np.asarray(spec.right, np.int32)] if spec.channels == 2 else []))
    bf, bc, bw = spec.bad if spec.bad else (NONE, 0, 0)
    return b"\1" + struct.pack("<IIIIIQQII", spec.layout, spec.channels, spec.depth, spec.rate, spec.offset, len(spec.left), bf, bc, bw) + \
        samples.astype("<i4").tobytes()


def _hash(data: bytes) -> str:
    h = 0xCBF29CE484222325
    for b in data:
        h = ((h ^ b) * 0x100000001B3) & CLEAN
    return "%016x" % h


def _totals_bytes(t):
    a = np.zeros(1, TOT_T)
    for name, v in zip(TOT_T.names, t):
        if name == "ch":
            for c in range(2):
                a[0]["ch"][c] = tuple(v[c])
        else:
            a[0][name] = v
    return a.tobytes()


def line(blob: bytes, index: int) -> str:
    """The plain build's line for a case (what the sanitized program must print for it)."""
    if blob[0] == 0:
        buf = C.create_string_buffer(1 << 20)
        rc = lib().sim_peak_line(blob[1:], C.c_uint64(len(blob) - 1), C.c_uint32(index), buf, C.c_uint32(len(buf)))
        assert rc == 0
        return buf.value.decode()
    layout, channels, depth, rate, offset, frames, bf, bc, bw = struct.unpack_from("<IIIIIQQII", blob, 1)
    x = np.frombuffer(blob, "<i4", offset=1 + struct.calcsize("<IIIIIQQII")).astype(np.int32)
    spec = SourceSpec(layout, channels, depth, rate, offset, x[:frames], x[frames:] if channels == 2 else None, None if bf == NONE else (bf, bc, bw))
    (o,) = run_sources([spec])
    rows = o.rows if o.rows is not None else np.zeros(0, ROW_T)
    return "%d %d %d %s %s %s" % (index, o.key, len(rows), _hash(rows.tobytes()), _hash(_totals_bytes(o.totals)), o.message)


def run_sanitized(cases, exe=None, workers=8):
    """Every case through the sanitized program, split over a few processes: (lines, returncode, stderr)."""
    if exe is None:
        exe, why = sanitized_exe()
        assert exe, why
    return twinbuild.run_cases(exe, cases, ENV, workers=workers, prefix="lac_peak_")


BATCH = 16


def cleared(key, lacs, sources=()):
    """lacs (and source specs), once the sanitized twin has shown in this run that a true-peak job over them stays inside
    buffers of exactly the plan's capacities and answers as the plain build does.  Fails, never skips, where that cannot be
    shown."""
    def make():
        cases = [case(lacs[at:at + BATCH]) for at in range(0, len(lacs), BATCH)] + [source_case(s) for s in sources]
        return cases, lambda c, i: line(c, i).split(" ", 1)[1], None, list(lacs)

    return twinbuild.cleared("true peak", key, sys.modules[__name__], make)
