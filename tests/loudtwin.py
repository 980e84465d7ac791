"""Loudness off the device: where its expectations come from, the signals the tests run on, and the CPU twin.

  coefficients(fs)                      the K-weighting biquads from the analog prototype, recomputed in Python
  expected_rows(left, right, rate)      the rows: scipy.signal.lfilter in float64, run sequentially over the whole channel,
                                        numpy sums over sub-blocks -- never the code under test
  expected_totals(sets)                 BS.1770-4 / Tech 3342 totals of rows, restated in plain Python floats
  corpus() / assert_content             frozen seeded items over chunk, sub-block, gating-block, container-block and
                                        short-term borders, with content that exercises both gates
  ebu_cases()                           1 kHz sines in the manner of EBU Tech 3341
  run(lacs) / run_sources(...)          the CPU twin (tests/native/sim_loudness.cpp: csrc/decode_plan.h's loudness job and
                                        csrc/loudness_core.h as the four kernels run it), plain build
  case / source_case / line / run_sanitized   the same through the build with AddressSanitizer + UBSan, a program of its own
                                        (a sanitizer is never loaded into Python)
  cleared(key, lacs)                    streams that may go to a device: the sanitized twin has passed them

ROW_TOL is a measured number: the largest relative difference between a row of the plain twin and the same row of the
expectation over the whole corpus (test_loudness_twin_host.py prints it), times 16 for other scipy / libm builds.  The
twin itself is deterministic."""
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

SRC = twinbuild.NATIVE + "/sim_loudness.cpp"
FP = "-ffp-contract=off"  # as the kernels' translation unit is compiled (Makefile)
ENV = dict(ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
FORMATS = ((1, 16, 44100), (2, 16, 48000), (1, 24, 96000), (2, 24, 192000))  # statstwin.FORMATS
RATES = (44100, 48000, 96000, 192000)
CHUNK = 256
TOO_SHORT, SILENT = 1, 2
CLEAN = (1 << 64) - 1
NONE = (1 << 64) - 1

# measured on the corpus (plain twin against scipy 1.15.3): largest d = |E - E_ref| / max(E_ref, 2^-40 * largest row)
ROW_MEASURED = 2.71e-11  # (the decaying filter tail behind a sound: rows 2^-30 and less of the item's largest)
ROW_TOL = 16 * ROW_MEASURED
TOTALS_TOL = 4.35 * ROW_TOL * 4  # LU, end to end against scipy: 10 log10(1 + e) ~ 4.35 e
COMBINE_TOL = 1e-9  # LU, the product's combine against the restatement over the same rows

ROW_T = np.dtype([("energy", "<f8", (2,))])
TOT_T = np.dtype([("frames", "<u8"), ("rate", "<u4"), ("channels", "u1"), ("depth", "u1"), ("flags", "u1"), ("reserved", "u1"),
                  ("subblocks", "<u4"), ("gating_blocks", "<u4"), ("above_absolute", "<u4"), ("above_relative", "<u4"),
                  ("integrated", "<f8"), ("relative_gate", "<f8"), ("momentary_max", "<f8"), ("shortterm_max", "<f8"), ("range", "<f8")])
assert (ROW_T.itemsize, TOT_T.itemsize) == (16, 72)

Totals = namedtuple("Totals", "frames rate channels depth flags subblocks gating_blocks above_absolute above_relative "
                              "integrated relative_gate momentary_max shortterm_max range")
LEVELS = ("integrated", "relative_gate", "momentary_max", "shortterm_max", "range")


# ---- expectations -----------------------------------------------------------------------------------------------------
def coefficients(fs):
    """((b, a) of the shelf, (b, a) of the high-pass) for sample rate fs."""
    f0, G, Q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    K = math.tan(math.pi * f0 / fs)
    Vh = math.pow(10.0, G / 20.0)
    Vb = math.pow(Vh, 0.4996667741545416)
    a0 = 1.0 + K / Q + K * K
    shelf = ([(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0],
             [1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0])
    f0, Q = 38.13547087602444, 0.5003270373238773
    K = math.tan(math.pi * f0 / fs)
    d = 1.0 + K / Q + K * K
    return shelf, ([1.0, -2.0, 1.0], [1.0, 2.0 * (K * K - 1.0) / d, (1.0 - K / Q + K * K) / d])


def expected_rows(left, right, rate):
    """(S, 2) float64: per sub-block and channel the sum of squares of the K-weighted integer samples (0 for a mono item's
    second column)."""
    from scipy.signal import lfilter
    n = rate // 10
    S = len(left) // n
    out = np.zeros((S, 2))
    (sb, sa), (hb, ha) = coefficients(rate)
    for c, x in enumerate((left, right)):
        if x is None or S == 0:
            continue
        y = lfilter(hb, ha, lfilter(sb, sa, np.asarray(x[:S * n], np.float64)))
        out[:, c] = (y * y).reshape(S, n).sum(axis=1)
    return out


def lufs(z):
    return -0.691 + 10.0 * math.log10(z) if z > 0.0 else -math.inf


def expected_totals(sets):
    """sets: [(rows (S, 2), channels, depth, rate)] -> Totals, in plain Python floats."""
    gate_z, range_z, mom, st = [], [], -math.inf, -math.inf
    frames = subblocks = 0
    for rows, channels, depth, rate in sets:
        n = rate // 10
        full = float(4 ** (depth - 1))
        e = [float(r[0]) + float(r[1]) if channels == 2 else float(r[0]) for r in rows]
        S = len(e)
        frames += S * n
        subblocks += S
        for j in range(S - 3):
            z = (e[j] + e[j + 1] + e[j + 2] + e[j + 3]) / (4.0 * n * full)
            gate_z.append(z)
            mom = max(mom, lufs(z))
        for j in range(S - 29):
            z = sum(e[j:j + 30]) / (30.0 * n * full)
            st = max(st, lufs(z))
            if j % 10 == 0:
                range_z.append(z)
    _, channels, depth, rate = sets[0]
    if not gate_z:
        return Totals(frames, rate, channels, depth, TOO_SHORT, subblocks, 0, 0, 0, -math.inf, -math.inf, -math.inf, -math.inf, 0.0)
    above = [z for z in gate_z if lufs(z) > -70.0]
    flags, integrated, rel, kept = 0, -math.inf, -math.inf, []
    if not above:
        flags = SILENT
    else:
        rel = lufs(sum(above) / len(above)) - 10.0
        kept = [z for z in above if lufs(z) > rel]
        if kept:
            integrated = lufs(sum(kept) / len(kept))
    lra = 0.0
    loud = [z for z in range_z if lufs(z) > -70.0]
    if loud:
        gate = lufs(sum(loud) / len(loud)) - 20.0
        l = sorted(lufs(z) for z in loud if lufs(z) > gate)
        if l:
            lra = l[int(math.floor((len(l) - 1) * 0.95 + 0.5))] - l[int(math.floor((len(l) - 1) * 0.10 + 0.5))]
    return Totals(frames, rate, channels, depth, flags, subblocks, len(gate_z), len(above), len(kept), integrated, rel, mom, st, lra)


def block_levels(rows, channels, depth, rate):
    """The loudness of every gating block of one set (for assert_content)."""
    n, full = rate // 10, float(4 ** (depth - 1))
    e = [float(r[0]) + float(r[1]) if channels == 2 else float(r[0]) for r in rows]
    return [lufs((e[j] + e[j + 1] + e[j + 2] + e[j + 3]) / (4.0 * n * full)) for j in range(len(e) - 3)]


def row_error(got, want):
    """The largest d = |E - E_ref| / max(E_ref, 2^-40 * the item's largest row) over an item's rows (0 for none)."""
    got, want = np.asarray(got, np.float64).reshape(-1, 2), np.asarray(want, np.float64).reshape(-1, 2)
    assert got.shape == want.shape
    if want.size == 0:
        return 0.0
    floor = want.max() * 2.0 ** -40
    if floor == 0.0:
        return 0.0 if not got.any() else math.inf
    return float((np.abs(got - want) / np.maximum(want, floor)).max())


def close_totals(got, want, tol):
    """Counts and flags exact, every level within tol LU (equal where infinite)."""
    assert got[:9] == want[:9], (got, want)
    for name in LEVELS:
        g, w = getattr(got, name), getattr(want, name)
        assert (g == w) if math.isinf(w) or math.isinf(g) else abs(g - w) <= tol, (name, g, w, tol)


# ---- records, whoever made them ---------------------------------------------------------------------------------------
def rows_of(records):
    """ctypes LoudnessRow records (the product's) or a ROW_T array (the twin's) -> (S, 2) float64."""
    if isinstance(records, np.ndarray):
        a = records
    else:
        a = np.frombuffer(bytes(records) if isinstance(records, C.Array) else b"".join(bytes(r) for r in records), ROW_T)
    return np.array(a["energy"], np.float64).reshape(-1, 2)


def totals_of(record):
    t = record if isinstance(record, (np.void, np.ndarray)) else np.frombuffer(bytes(record), TOT_T)[0]
    return Totals(int(t["frames"]), int(t["rate"]), int(t["channels"]), int(t["depth"]), int(t["flags"]), int(t["subblocks"]),
                  int(t["gating_blocks"]), int(t["above_absolute"]), int(t["above_relative"]), float(t["integrated"]), float(t["relative_gate"]),
                  float(t["momentary_max"]), float(t["shortterm_max"]), float(t["range"]))


# ---- signals ----------------------------------------------------------------------------------------------------------
Item = namedtuple("Item", "name channels depth rate left right")
KINDS = ("noise", "tone", "silence_sound_silence", "dither", "loud_quiet")


def frame_counts(rate):
    n = rate // 10
    return (1, 255, 256, 257, n - 1, n, n + 1, 4 * n - 1, 4 * n, 4 * n + 1, 16383, 16384, 16385, 30 * n, 30 * n + 1, 5 * rate + 777)


def _sine(frames, rate, depth, dbfs, freq=997.0, phase=0.0):
    t = np.arange(frames, dtype=np.float64)
    return np.rint(10.0 ** (dbfs / 20.0) * (1 << (depth - 1)) * np.sin(2.0 * np.pi * freq * t / rate + phase)).astype(np.int32)


def content(kind, frames, depth, rate, seed):
    """One channel of `kind`."""
    rng = np.random.default_rng(seed)
    lim = 1 << (depth - 1)
    if kind == "noise":  # full scale
        return rng.integers(-lim, lim, frames, dtype=np.int64).astype(np.int32)
    if kind == "tone":
        return _sine(frames, rate, depth, -6.0, phase=seed % 7)
    if kind == "silence_sound_silence":  # digital silence, sound, and its filter tail decaying into near-zero rows
        x = (rng.integers(-lim, lim, frames, dtype=np.int64) >> 2).astype(np.int32)
        x[:frames // 3] = 0
        x[frames - frames // 3:] = 0
        return x
    if kind == "dither":  # 1 LSB: under the absolute gate at either depth
        return rng.integers(-1, 2, frames, dtype=np.int64).astype(np.int32)
    assert kind == "loud_quiet"  # the relative gate cuts the second half
    x = _sine(frames, rate, depth, -10.0, phase=seed % 5)
    x[frames // 2:] = _sine(frames - frames // 2, rate, depth, -40.0, phase=seed % 3)
    return x


def make_item(kind, frames, channels, depth, rate, seed, tag="n"):
    left = content(kind, frames, depth, rate, 2 * seed)
    right = content(kind, frames, depth, rate, 2 * seed + 1) if channels == 2 else None
    return Item("%s|%s%d|%dch%d" % (kind, tag, frames, channels, depth), channels, depth, rate, left, right)


_corpus = None


def corpus():
    """Frozen seeds: per format every frame count (the content kinds in turn) and every content kind at 30 n + 1 frames."""
    global _corpus
    if _corpus is None:
        items, seed = [], 7000
        for ch, depth, rate in FORMATS:
            for k, frames in enumerate(frame_counts(rate)):
                seed += 1
                items.append(make_item(KINDS[(k + depth + ch) % 2], frames, ch, depth, rate, seed))
            for kind in KINDS:
                seed += 1
                items.append(make_item(kind, 30 * (rate // 10) + 1, ch, depth, rate, seed, tag="content"))
        _corpus = items
    return _corpus


_expected = {}


def item_rows(it):
    """The expectation of an item's rows, computed once and shared (callers do not change it)."""
    if it.name not in _expected:
        rows = expected_rows(it.left, it.right, it.rate)
        rows.setflags(write=False)
        _expected[it.name] = rows
    return _expected[it.name]


def item_totals(it):
    return expected_totals([(item_rows(it), it.channels, it.depth, it.rate)])


def assert_content(items):
    """On the expectation alone: each gate does remove blocks, and no block lies within 1e-3 LU of a gate."""
    for it in items:
        t = item_totals(it)
        levels = block_levels(item_rows(it), it.channels, it.depth, it.rate)
        assert all(abs(l + 70.0) > 1e-3 for l in levels if not math.isinf(l)), it.name
        assert all(abs(l - t.relative_gate) > 1e-3 for l in levels if not math.isinf(l) and not math.isinf(t.relative_gate)), it.name
        kind = it.name.split("|")[0]
        if "|content" not in it.name:
            continue
        if kind == "dither":
            assert t.gating_blocks > 0 and t.above_absolute == 0 and t.flags == SILENT, it.name
        if kind == "silence_sound_silence":
            assert 0 < t.above_absolute < t.gating_blocks, it.name
            assert min(l for l in levels if not math.isinf(l)) < -200.0, "a decaying tail into near-zero rows"
        if kind == "loud_quiet":
            assert 0 < t.above_relative < t.above_absolute == t.gating_blocks, it.name
        if kind in ("noise", "tone"):
            assert t.above_relative == t.gating_blocks > 0, it.name


def ebu_cases(rate=48000, depth=16, channels=2):
    """[(name, [(seconds, dBFS)], expected LUFS)]: 1 kHz sines in the manner of EBU Tech 3341's cases."""
    return [("23", [(20, -23.0)], -23.0), ("33", [(20, -33.0)], -33.0),
            ("36-23-36", [(10, -36.0), (60, -23.0), (10, -36.0)], -23.0),
            ("72-36-23-36-72", [(10, -72.0), (10, -36.0), (60, -23.0), (10, -36.0), (10, -72.0)], -23.0),
            ("26-20-26", [(20, -26.0), (20.1, -20.0), (20, -26.0)], -23.0)]


def ebu_item(name, parts, rate=48000, depth=16, channels=2):
    x = np.concatenate([_sine(int(round(sec * rate)), rate, depth, db, freq=1000.0) for sec, db in parts])
    return Item("ebu" + name + "|%dch%d@%d" % (channels, depth, rate), channels, depth, rate, x, x.copy() if channels == 2 else None)


# ---- the twin ---------------------------------------------------------------------------------------------------------
_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(twinbuild.shared_lib("sim_loudness", [SRC], flags=(FP,)))
        _lib.sim_loud_streams.restype = C.c_int64
        _lib.sim_loud_sources.restype = C.c_int64
        _lib.sim_loud_filters.restype = None
        _lib.sim_loud_combine.restype = None
    return _lib


def sanitized_exe():
    """The sanitized program's path, or (None, why) where the sanitizer runtime is missing."""
    return twinbuild.sanitized_exe("sim_loudness_san", [SRC], ["-DSIM_LOUDNESS_MAIN", FP])


def twin_filters():
    """{rate: 26 doubles}: shelf b, shelf -a, high-pass b, high-pass -a, A row by row -- as csrc/loudness_plan.h makes them."""
    out = np.zeros(4 * 26)
    lib().sim_loud_filters(out.ctypes.data_as(C.c_void_p))
    return {rate: out[26 * k:26 * k + 26].copy() for k, rate in enumerate(RATES)}


TwinItem = namedtuple("TwinItem", "code message status rows totals")
_vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731


def run(lacs, rows_cap=None):
    """n streams as one loudness job on the CPU twin -> [TwinItem] (rows: (S, 2) float64, or None without a result)."""
    n = len(lacs)
    ptrs = (C.c_char_p * n)(*lacs)
    sizes = (C.c_uint64 * n)(*[len(x) for x in lacs])
    cap = rows_cap if rows_cap is not None else 1 + sum(sum(dectwin._shape(x)[1]) // 4410 for x in lacs if salvagetwin._head_ok(x))
    rec = np.zeros(3 * n, np.uint64)
    rows = np.zeros(cap, ROW_T)
    totals = np.zeros(n, TOT_T)
    msg = C.create_string_buffer(1 << 16)
    got = lib().sim_loud_streams(ptrs, sizes, C.c_uint32(n), _vp(rec), _vp(rows), C.c_uint64(cap), _vp(totals), msg, C.c_uint32(len(msg)))
    assert got >= 0, "the twin could not run the job"
    msgs = msg.value.decode().split("\n")
    items, at = [], 0
    for i in range(n):
        code, nr, status = int(rec[3 * i]), int(rec[3 * i + 1]), int(rec[3 * i + 2])
        if code or status:
            items.append(TwinItem(code, msgs[i], status, None, totals_of(totals[i])))
            continue
        items.append(TwinItem(0, "", 0, rows_of(rows[at:at + nr]), totals_of(totals[i])))
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
    cap = int(sum(len(s.left) // (s.rate // 10) for s in specs)) + 1
    rows, counts, totals, keys = np.zeros(cap, ROW_T), np.zeros(n, np.uint32), np.zeros(n, TOT_T), np.zeros(n, np.uint64)
    msg = C.create_string_buffer(1 << 14)
    got = lib().sim_loud_sources(C.c_uint32(n), _vp(u32([s.layout for s in specs])), _vp(u32([s.channels for s in specs])),
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
        out.append(SourceOut(CLEAN, "", rows_of(rows[at:at + int(counts[k])]), totals_of(totals[k])))
        at += int(counts[k])
    return out


def twin_combine(sets):
    """csrc/loudness_rows.h's totals of [(rows (S, 2), channels, depth, rate)] -> Totals."""
    n = len(sets)
    arrays = [np.ascontiguousarray(np.asarray(r, np.float64).reshape(-1, 2)) for r, _, _, _ in sets]
    ptrs = (C.c_void_p * n)(*[a.ctypes.data for a in arrays])
    out = np.zeros(1, TOT_T)
    lib().sim_loud_combine(ptrs, _vp(np.array([len(a) for a in arrays], np.uint32)), _vp(np.array([s[1] for s in sets], np.uint8)),
                           _vp(np.array([s[2] for s in sets], np.uint8)), _vp(np.array([s[3] for s in sets], np.uint32)), C.c_uint32(n), _vp(out))
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


def line(blob: bytes, index: int) -> str:
    """The plain build's line for a case (what the sanitized program must print for it)."""
    if blob[0] == 0:
        buf = C.create_string_buffer(1 << 20)
        rc = lib().sim_loud_line(blob[1:], C.c_uint64(len(blob) - 1), C.c_uint32(index), buf, C.c_uint32(len(buf)))
        assert rc == 0
        return buf.value.decode()
    layout, channels, depth, rate, offset, frames, bf, bc, bw = struct.unpack_from("<IIIIIQQII", blob, 1)
    x = np.frombuffer(blob, "<i4", offset=1 + struct.calcsize("<IIIIIQQII")).astype(np.int32)
    spec = SourceSpec(layout, channels, depth, rate, offset, x[:frames], x[frames:] if channels == 2 else None, None if bf == NONE else (bf, bc, bw))
    (o,) = run_sources([spec])
    rows = np.zeros(0 if o.rows is None else len(o.rows), ROW_T)
    if o.rows is not None:
        rows["energy"] = o.rows
    return "%d %d %d %s %s %s" % (index, o.key, len(rows), _hash(rows.tobytes()), _hash(_totals_bytes(o.totals)), o.message)


def _totals_bytes(t):
    a = np.zeros(1, TOT_T)
    for name, v in zip(TOT_T.names, (t.frames, t.rate, t.channels, t.depth, t.flags, 0, t.subblocks, t.gating_blocks, t.above_absolute, t.above_relative,
                                     t.integrated, t.relative_gate, t.momentary_max, t.shortterm_max, t.range)):
        a[0][name] = v
    return a.tobytes()


def run_sanitized(cases, exe=None, workers=8):
    """Every case through the sanitized program, split over a few processes: (lines, returncode, stderr)."""
    if exe is None:
        exe, why = sanitized_exe()
        assert exe, why
    return twinbuild.run_cases(exe, cases, ENV, workers=workers, prefix="lac_loud_")


BATCH = 16


def cleared(key, lacs, sources=()):
    """lacs (and source specs), once the sanitized twin has shown in this run that a loudness job over them stays inside
    buffers of exactly the plan's capacities and answers as the plain build does.  Fails, never skips, where that cannot be
    shown."""
    def make():
        cases = [case(lacs[at:at + BATCH]) for at in range(0, len(lacs), BATCH)] + [source_case(s) for s in sources]
        return cases, lambda c, i: line(c, i).split(" ", 1)[1], None, list(lacs)

    return twinbuild.cleared("loudness", key, sys.modules[__name__], make)
