"""Spectrum off the device: where its expectations come from, the signals the tests run on, and the CPU twin.

  expected_rows(left, right, window)    numpy.fft.rfft in float64 over w x, bands and rows summed in Python -- never the
                                        code under test
  expected_totals(rows, ...)            the totals of rows, restated in Python
  parseval_rows(left, right, window)    N sum (w x)^2 per row and channel with math.fsum: independent of any FFT
  corpus() / assert_content(items)      frozen seeded items over window, hop and row borders, and what they must contain
  run(lacs, window) / run_sources(...)  the CPU twin (tests/native/sim_spectrum.cpp: csrc/decode_plan.h's spectrum job and
                                        csrc/spectrum_core.h as k_spectrum runs it), plain build
  case / source_case / line / run_sanitized   the same through the build with AddressSanitizer + UBSan, a program of its own
                                        (a sanitizer is never loaded into Python)
  cleared(key, window, lacs, sources)   shapes that may go to a device: the sanitized twin has passed them

Tolerance.  The twin's FFT (radix-2, FP64, fixed order) and numpy's differ in rounding only.  The error of a band is held
relative to the TOTAL power of its row and channel -- a band that holds only another band's rounding noise has no
meaningful relative error: |twin - numpy| / total <= BAND_TOL.  BAND_TOL is 16 times the largest such value measured on the
CPU over the whole corpus (test_spectrum_twin_host.py prints it), ROW_TOL's convention in loudtwin.py."""
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

SRC = twinbuild.NATIVE + "/sim_spectrum.cpp"
FP = "-ffp-contract=off"  # as the kernel's translation unit is compiled (Makefile)
ENV = dict(ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
FORMATS = ((1, 16, 44100), (2, 16, 96000), (1, 24, 96000), (2, 24, 44100))
WINDOWS = (256, 512, 1024, 2048, 4096)
ROW, BANDS = 16384, 64
CLEAN = (1 << 64) - 1
NONE = (1 << 64) - 1
FLOOR = -100.0
BAND_TOL = 16 * 3.2e-16  # measured: 3.16e-16 (the largest |twin - numpy| / row-channel total over the corpus, on the CPU)

ROW_T = np.dtype([("power", "<f8", (2, BANDS))])
TOT_T = np.dtype([("frames", "<u8"), ("windows", "<u8"), ("rate", "<u4"), ("window", "<u4"), ("rows", "<u4"), ("channels", "u1"), ("depth", "u1"),
                  ("peak_band", "u1", (2,)), ("floor_db", "<f8"), ("bandwidth_hz", "<f8", (2,)), ("level_db", "<f8", (2, BANDS))])
assert (ROW_T.itemsize, TOT_T.itemsize) == (1024, 1080)


# ---- expectations -----------------------------------------------------------------------------------------------------
def hann(window):
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(window) / window)


def _windows(x, window):
    """(windows, N) float64: w x per window, zeros behind the item's end."""
    hop, frames = window // 2, len(x)
    nw = -(-frames // hop)
    xp = np.concatenate([np.asarray(x, np.float64), np.zeros(window)])
    idx = hop * np.arange(nw)[:, None] + np.arange(window)[None, :]
    return xp[idx] * hann(window)[None, :]


def expected_rows(left, right, window):
    """(rows, 2, 64) float64 by numpy.fft.rfft; window k belongs to row k * hop // 16384; a mono item's second channel is 0."""
    frames, hop, per = len(left), window // 2, window // 128
    nrows = -(-frames // ROW)
    out = np.zeros((nrows, 2, BANDS))
    for c, x in enumerate((left, right)):
        if x is None:
            continue
        p = np.abs(np.fft.rfft(_windows(x, window), axis=1)) ** 2
        p[:, 1:-1] *= 2.0
        bands = p[:, :-1].reshape(len(p), BANDS, per).sum(axis=2)
        bands[:, BANDS - 1] += p[:, -1]
        for k in range(len(p)):
            out[k * hop // ROW, c] += bands[k]
    return out


def parseval_rows(left, right, window):
    """(rows, 2) float: N sum (w x)^2 over the windows of each row, by math.fsum."""
    frames, hop = len(left), window // 2
    nrows = -(-frames // ROW)
    out = np.zeros((nrows, 2))
    for c, x in enumerate((left, right)):
        if x is None:
            continue
        e = _windows(x, window) ** 2
        per = ROW // hop
        for r in range(nrows):
            out[r, c] = window * math.fsum(e[r * per:(r + 1) * per].ravel().tolist())
    return out


Totals = namedtuple("Totals", "frames windows rate window rows channels depth peak_band floor_db bandwidth_hz level_db")


def expected_totals(rows, channels, depth, frames, rate, window, floor_db=FLOOR):
    """rows: (R, 2, 64) -> Totals, restated: P added in row order, level = 10 log10(P / (windows 3 N^2 / 8 2^(2b-3)))."""
    nw = -(-frames // (window // 2))
    full = float(nw) * (3.0 * window * window / 8.0) * 2.0 ** (2 * depth - 3)
    peak, bw, level = [0, 0], [0.0, 0.0], [[-math.inf] * BANDS for _ in range(2)]
    for c in range(channels):
        best = 0.0
        for b in range(BANDS):
            p = 0.0
            for r in rows:
                p = p + float(r[c][b])
            if p > 0.0:
                level[c][b] = 10.0 * math.log10(p / full)
            if p > best:
                best, peak[c] = p, b
            if level[c][b] >= floor_db:
                bw[c] = (b + 1) * rate / 128.0
    return Totals(frames, nw, rate, window, len(rows), channels, depth, tuple(peak), floor_db, tuple(bw), tuple(tuple(x) for x in level))


def rows_of(records):
    """ctypes SpectrumRow records (the product's) or a ROW_T array (the twin's) -> a ROW_T array."""
    if isinstance(records, np.ndarray):
        return records
    return np.frombuffer(bytes(records) if isinstance(records, C.Array) else b"".join(bytes(r) for r in records), ROW_T)


def totals_of(record):
    t = record if isinstance(record, (np.void, np.ndarray)) else np.frombuffer(bytes(record), TOT_T)[0]
    return Totals(int(t["frames"]), int(t["windows"]), int(t["rate"]), int(t["window"]), int(t["rows"]), int(t["channels"]), int(t["depth"]),
                  tuple(int(x) for x in t["peak_band"]), float(t["floor_db"]), tuple(float(x) for x in t["bandwidth_hz"]),
                  tuple(tuple(float(x) for x in ch) for ch in t["level_db"]))


def same_totals(got, want):
    """Integers, the floor and the bandwidths equal; the levels within 1e-9 dB (equal where infinite)."""
    assert got[:10] == want[:10], (got[:10], want[:10])
    for g, w in zip(np.ravel(got.level_db), np.ravel(want.level_db)):
        assert (g == w) if math.isinf(w) or math.isinf(g) else abs(g - w) <= 1e-9, (g, w)


def band_error(got, want):
    """The largest |got - want| / (that row-channel's total in `want`) over (row, channel, band); got, want: (R, 2, 64)."""
    total = want.sum(axis=2, keepdims=True)
    diff = np.abs(got - want)
    # (no item of the corpus is silent in one channel of a row and not in the other: a stereo item's channels share a transform)
    assert np.all(diff[np.broadcast_to(total == 0.0, diff.shape)] == 0.0), "a silent row and channel is zero exactly"
    return float(np.max(diff / np.where(total == 0.0, 1.0, total), initial=0.0))


# ---- signals ----------------------------------------------------------------------------------------------------------
Item = namedtuple("Item", "name window channels depth rate left right")
FRAMES_256 = (1, 127, 128, 129, 255, 256, 257, 16383, 16384, 16385, 16384 + 129, 2 * 16384 + 1)
FRAMES_4096 = (4095, 4096, 4097, 16385)
CUTOFF_BAND = 40  # the band-limited item's highest band with signal: sines on bins 1 .. 2 * 40 of 256, a band edge minus two bins


def _noise(frames, depth, seed):
    lim = 1 << (depth - 1)
    return np.random.default_rng(seed).integers(-lim, lim, frames, dtype=np.int64).astype(np.int32)


def sine(frames, window, k, amp, phase=0.0):
    """round(amp cos(2 pi k n / window + phase)): a sine on exact bin k."""
    n = np.arange(frames, dtype=np.float64)
    return np.rint(amp * np.cos(2.0 * np.pi * k * n / window + phase)).astype(np.int32)


def band_limited(frames, depth, seed, window=256, top=2 * CUTOFF_BAND, fade=2048):
    """Sines on every bin 1 .. top with frozen phases and exact zeros above, 18 dB below what fills the scale, under a
    raised-cosine fade in and out: without the fade the cut at the item's end splatters into every band (about -70 dBFS);
    with it the band above the cutoff reads about -106 dBFS."""
    n = np.arange(frames, dtype=np.float64)
    rng = np.random.default_rng(seed)
    x = np.zeros(frames)
    for k in range(1, top + 1):
        x += np.cos(2.0 * np.pi * k * n / window + rng.uniform(0.0, 2.0 * np.pi))
    x *= (1 << (depth - 1)) / (32.0 * math.sqrt(top))
    ramp = 0.5 - 0.5 * np.cos(np.pi * np.arange(fade) / fade)
    x[:fade] *= ramp
    x[-fade:] *= ramp[::-1]
    return np.rint(x).astype(np.int32)


_corpus = None


def corpus():
    """Frozen seeds.  N = 256: noise in every format at every frame count of FRAMES_256; N = 4096: noise in every format
    at FRAMES_4096; N = 512, 1024, 2048: one stereo item of 16385 frames each.  Then the constructed content, stereo with
    different channels, at N = 256 and 16384 + 129 frames unless said otherwise."""
    global _corpus
    if _corpus is not None:
        return _corpus
    items, seed = [], 7000
    for window, counts in ((256, FRAMES_256), (4096, FRAMES_4096)):
        for ch, depth, rate in FORMATS:
            for frames in counts:
                seed += 1
                items.append(Item("noise|N%d|n%d|%dch%d" % (window, frames, ch, depth), window, ch, depth, rate, _noise(frames, depth, 2 * seed),
                                  _noise(frames, depth, 2 * seed + 1) if ch == 2 else None))
    for k, window in enumerate((512, 1024, 2048)):
        ch, depth, rate = FORMATS[1 + 2 * (k % 2)]
        items.append(Item("noise|N%d|n16385|%dch%d" % (window, ch, depth), window, ch, depth, rate, _noise(16385, depth, 7900 + 2 * k), _noise(16385, depth, 7901 + 2 * k)))
    F = ROW + 129
    for depth, rate in ((16, 96000), (24, 44100)):
        lo, hi = -(1 << (depth - 1)), (1 << (depth - 1)) - 1
        tag = "2ch%d" % depth

        def add(name, left, right, window=256):
            items.append(Item("%s|N%d|%s" % (name, window, tag), window, 2, depth, rate, np.asarray(left, np.int32), np.asarray(right, np.int32)))

        add("silence", np.zeros(F, np.int32), np.zeros(F, np.int32))
        a, b = np.zeros(F, np.int32), np.zeros(F, np.int32)
        # at frame 0, where the window is zero; inside later windows on both sides of the row edge.  Both channels have
        # comparable power in every row: a stereo item's channels share a transform, and the rounding noise of a channel
        # 1e4 times louder than the other would be held to the quiet one's total
        a[0], a[200], a[ROW + 70], b[64], b[ROW + 90] = hi, hi, lo, lo, hi
        add("impulse", a, b)
        for kl, kr in ((2, 64), (64, 126), (126, 2)):  # bins 2, N / 4 and N / 2 - 2 at N = 256
            add("sine|k%d-k%d" % (kl, kr), sine(F, 256, kl, hi), sine(F, 256, kr, hi, 0.7))
        add("sine|k2-k2046", sine(16385, 4096, 2, hi), sine(16385, 4096, 2046, hi, 0.3), 4096)
        add("dc", np.full(F, hi, np.int32), np.full(F, lo, np.int32))
        alt = np.where(np.arange(F) % 2 == 0, hi, lo).astype(np.int32)
        add("nyquist", alt, (-(alt.astype(np.int64)) // 2).astype(np.int32))
        add("cross|k10-k100", sine(F, 256, 10, hi), sine(F, 256, 100, hi, 1.1))  # bands 5 and 50
    items.append(Item("noise|full24|N256|2ch24", 256, 2, 24, 44100, _noise(F, 24, 7991), _noise(F, 24, 7992)))
    items.append(Item("bandlimit|N256|2ch24", 256, 2, 24, 44100, band_limited(2 * ROW + 1, 24, 7993), band_limited(2 * ROW + 1, 24, 7994, top=2 * CUTOFF_BAND - 20)))
    # 1024 windows of which only the last is cut: the zero-padded tail costs 10 log10(1 - 0.5 / 1024) = -0.002 dB
    items.append(Item("sine|level|N256|1ch16", 256, 1, 16, 44100, sine(8 * ROW, 256, 64, 32767), None))
    assert len({it.name for it in items}) == len(items)
    _corpus = items
    return _corpus


def assert_content(items):
    """The corpus holds what the tests rely on: formats, window lengths, shapes and the classes of content."""
    by = lambda w: {len(it.left) for it in items if it.window == w}  # noqa: E731
    assert {(it.channels, it.depth, it.rate) for it in items} == set(FORMATS)
    assert {it.window for it in items} == set(WINDOWS)
    assert set(FRAMES_256) <= by(256) and set(FRAMES_4096) <= by(4096) and all(16385 in by(w) for w in (512, 1024, 2048))
    count = lambda key: sum(1 for it in items if it.name.startswith(key))  # noqa: E731
    assert count("silence|") == 2 and count("impulse|") == 2 and count("sine|k") == 8 and count("dc|") == 2 and count("nyquist|") == 2
    assert count("noise|full24") == 1 and count("cross|") == 2 and count("bandlimit|") == 1 and count("sine|level") == 1
    for it in items:
        lim = 1 << (it.depth - 1)
        for x in (it.left, it.right):
            assert x is None or (x.dtype == np.int32 and x.min() >= -lim and x.max() < lim), it.name
        if it.channels == 2 and not it.name.startswith("silence"):
            assert not np.array_equal(it.left, it.right), it.name
    for it in items:
        if it.name.startswith("silence"):
            assert not it.left.any() and not it.right.any()
        if it.name.startswith(("sine|k", "dc|", "nyquist|")):
            assert int(np.abs(it.left.astype(np.int64)).max()) >= (1 << (it.depth - 1)) - 1, it.name
        if it.name.startswith("noise|full24"):
            assert int(np.abs(it.left.astype(np.int64)).max()) > 0.999 * (1 << 23)


_expected = {}


def item_rows(it):
    """The restatement of an item's rows, computed once and shared (callers do not change it)."""
    if it.name not in _expected:
        rows = expected_rows(it.left, it.right, it.window)
        rows.setflags(write=False)
        _expected[it.name] = rows
    return _expected[it.name]


def item_totals(it, rows=None, floor_db=FLOOR):
    return expected_totals(item_rows(it) if rows is None else rows, it.channels, it.depth, len(it.left), it.rate, it.window, floor_db)


# ---- the twin ---------------------------------------------------------------------------------------------------------
_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(twinbuild.shared_lib("sim_spectrum", [SRC], flags=(FP,)))
        _lib.sim_spec_streams.restype = C.c_int64
        _lib.sim_spec_sources.restype = C.c_int64
        _lib.sim_spec_combine.restype = None
    return _lib


def sanitized_exe():
    """The sanitized program's path, or (None, why) where the sanitizer runtime is missing."""
    return twinbuild.sanitized_exe("sim_spectrum_san", [SRC], ["-DSIM_SPECTRUM_MAIN", FP])


_vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731


def twin_tables(window):
    """(window [N], twiddle [N / 2, 2]) as csrc/spectrum_plan.h makes them, or None for an unsupported window."""
    w, tw = np.zeros(max(window, 1)), np.zeros(max(window, 1))
    if lib().sim_spec_tables(C.c_uint32(window), _vp(w), _vp(tw)) != 0:
        return None
    return w, tw.reshape(-1, 2)


def twin_check(frames, window):
    """sp_check's refusal for items of these frame counts, or ""."""
    msg = C.create_string_buffer(256)
    a = np.array(frames, np.uint64)
    lib().sim_spec_check(_vp(a), C.c_uint32(len(a)), C.c_uint32(window), msg, C.c_uint32(len(msg)))
    return msg.value.decode()


TwinItem = namedtuple("TwinItem", "code message status rows")


def run(lacs, window):
    """n streams as one spectrum job on the CPU twin -> [TwinItem] (rows: ROW_T, or None without a result)."""
    n = len(lacs)
    ptrs = (C.c_char_p * n)(*lacs)
    sizes = (C.c_uint64 * n)(*[len(x) for x in lacs])
    cap = n + sum(sum(dectwin._shape(x)[1]) // ROW for x in lacs if salvagetwin._head_ok(x))
    rec = np.zeros(3 * n, np.uint64)
    rows = np.zeros(cap, ROW_T)
    msg = C.create_string_buffer(1 << 16)
    got = lib().sim_spec_streams(ptrs, sizes, C.c_uint32(n), C.c_uint32(window), _vp(rec), _vp(rows), C.c_uint64(cap), msg, C.c_uint32(len(msg)))
    assert got >= 0, "the twin could not run the job"
    msgs = msg.value.decode().split("\n")
    items, at = [], 0
    for i in range(n):
        code, nr, status = int(rec[3 * i]), int(rec[3 * i + 1]), int(rec[3 * i + 2])
        if code or status:
            items.append(TwinItem(code, msgs[i], status, None))
            continue
        items.append(TwinItem(0, "", 0, rows[at:at + nr].copy()))
        at += nr
    return items


SourceSpec = namedtuple("SourceSpec", "window layout channels depth offset left right bad", defaults=(None,))
SourceOut = namedtuple("SourceOut", "key message rows")


def spec_of(it, layout=0, offset=0, bad=None):
    return SourceSpec(it.window, layout, it.channels, it.depth, offset, it.left, it.right, bad)


def run_sources(specs):
    """[SourceSpec] of ONE window length as one source job on the twin -> [SourceOut].  bad = (frame, channel, raw word)."""
    n = len(specs)
    (window,) = {s.window for s in specs}
    u32 = lambda xs: np.array(xs, np.uint32)  # noqa: E731
    samples = [np.ascontiguousarray(np.concatenate([np.asarray(s.left, np.int32)] + ([np.asarray(s.right, np.int32)] if s.channels == 2 else [])))
               for s in specs]
    ptrs = (C.c_void_p * n)(*[x.ctypes.data for x in samples])
    frames = np.array([len(s.left) for s in specs], np.uint64)
    bad = [s.bad if s.bad else (NONE, 0, 0) for s in specs]
    cap = int(sum(len(s.left) // ROW + 1 for s in specs))
    rows, counts, keys = np.zeros(cap, ROW_T), np.zeros(n, np.uint32), np.zeros(n, np.uint64)
    msg = C.create_string_buffer(1 << 14)
    got = lib().sim_spec_sources(C.c_uint32(n), C.c_uint32(window), _vp(u32([s.layout for s in specs])), _vp(u32([s.channels for s in specs])),
                                 _vp(u32([s.depth for s in specs])), _vp(u32([s.offset for s in specs])), _vp(frames), ptrs,
                                 _vp(np.array([b[0] for b in bad], np.uint64)), _vp(u32([b[1] for b in bad])), _vp(u32([b[2] for b in bad])),
                                 _vp(rows), C.c_uint64(cap), _vp(counts), _vp(keys), msg, C.c_uint32(len(msg)))
    assert got >= 0, "the twin could not run the sources"
    msgs = msg.value.decode().split("\n")
    out, at = [], 0
    for k in range(n):
        if int(keys[k]) != CLEAN:
            out.append(SourceOut(int(keys[k]), msgs[k], None))
            continue
        out.append(SourceOut(CLEAN, "", rows[at:at + int(counts[k])].copy()))
        at += int(counts[k])
    return out


_twin_rows = {}


def twin_rows(it):
    """The plain twin's rows of a corpus item as a planar int32 source, computed once: ROW_T."""
    if it.name not in _twin_rows:
        (o,) = run_sources([spec_of(it)])
        o.rows.setflags(write=False)
        _twin_rows[it.name] = o.rows
    return _twin_rows[it.name]


def twin_combine(rows, channels, depth, frames, rate, window, floor_db=FLOOR):
    """csrc/spectrum_rows.h's totals of ROW_T rows -> (Totals, the record's bytes)."""
    a = np.ascontiguousarray(np.asarray(rows, ROW_T))
    out = np.zeros(1, TOT_T)
    lib().sim_spec_combine(_vp(a), C.c_uint32(len(a)), C.c_uint8(channels), C.c_uint8(depth), C.c_uint64(frames), C.c_uint32(rate), C.c_uint32(window),
                           C.c_double(floor_db), _vp(out))
    return totals_of(out[0]), out.tobytes()


# ---- the sanitized program ----------------------------------------------------------------------------------------------
def case(lacs, window) -> bytes:
    body = struct.pack("<II", window, len(lacs))
    for x in lacs:
        body += struct.pack("<Q", len(x)) + x
    return b"\0" + body


_HEAD = "<IIIIIQQII"


def source_case(spec) -> bytes:
    samples = np.concatenate([np.asarray(spec.left, np.int32)] + ([np.asarray(spec.right, np.int32)] if spec.channels == 2 else []))
    bf, bc, bw = spec.bad if spec.bad else (NONE, 0, 0)
    return b"\1" + struct.pack(_HEAD, spec.window, spec.layout, spec.channels, spec.depth, spec.offset, len(spec.left), bf, bc, bw) + samples.astype("<i4").tobytes()


def _hash(data: bytes) -> str:
    h = 0xCBF29CE484222325
    for b in data:
        h = ((h ^ b) * 0x100000001B3) & CLEAN
    return "%016x" % h


def line(blob: bytes, index: int) -> str:
    """The plain build's line for a case (what the sanitized program must print for it)."""
    if blob[0] == 0:
        buf = C.create_string_buffer(1 << 20)
        rc = lib().sim_spec_line(blob[1:], C.c_uint64(len(blob) - 1), C.c_uint32(index), buf, C.c_uint32(len(buf)))
        assert rc == 0
        return buf.value.decode()
    window, layout, channels, depth, offset, frames, bf, bc, bw = struct.unpack_from(_HEAD, blob, 1)
    x = np.frombuffer(blob, "<i4", offset=1 + struct.calcsize(_HEAD)).astype(np.int32)
    spec = SourceSpec(window, layout, channels, depth, offset, x[:frames], x[frames:] if channels == 2 else None, None if bf == NONE else (bf, bc, bw))
    (o,) = run_sources([spec])
    rows = o.rows if o.rows is not None else np.zeros(0, ROW_T)
    return "%d %d %d %s %s" % (index, o.key, len(rows), _hash(rows.tobytes()), o.message)


def run_sanitized(cases, exe=None, workers=8):
    """Every case through the sanitized program, split over a few processes: (lines, returncode, stderr)."""
    if exe is None:
        exe, why = sanitized_exe()
        assert exe, why
    return twinbuild.run_cases(exe, cases, ENV, workers=workers, prefix="lac_spec_")


BATCH = 16


def cleared(key, window, lacs, sources=()):
    """lacs at `window` (and source specs), once the sanitized twin has shown in this run that a spectrum job over them stays
    inside buffers of exactly the plan's capacities and answers as the plain build does.  Fails, never skips, where that
    cannot be shown."""
    def make():
        cases = [case(lacs[at:at + BATCH], window) for at in range(0, len(lacs), BATCH)] + [source_case(s) for s in sources]
        return cases, lambda c, i: line(c, i).split(" ", 1)[1], None, list(lacs)

    return twinbuild.cleared("spectrum", (key, window), sys.modules[__name__], make)
