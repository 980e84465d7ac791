"""Audio statistics off the device: where their expectations come from, the signals the tests run on, and their CPU twin.

  expected_rows(left, right, depth, blocks, lost)   [Row] per block with numpy / Python ints from the PCM -- never the twin
  expected_totals(rows, channels, depth, rate)      Totals from those rows, restated in Python ints
  signal / content_items / shape_items              seeded signals that hold what statistics are about (silence at the
                                                    edges, full-scale samples, equal channels, unused bits, ...);
                                                    assert_content checks on the expectation that they do
  rows_of / totals_of                               the product's ctypes records, or the twin's, as Row / Totals
  run(lacs, ...)                                    the CPU twin (tests/native/sim_stats.cpp: csrc/decode_plan.h's stats job,
                                                    stats_core.h accumulated as k_stats_blocks accumulates), plain build
  source_rows(...)                                  the source form at unit level: one item in a layout at a base offset
  case / source_case / line / run_sanitized         the same through the build with AddressSanitizer + UBSan, a program of
                                                    its own (a sanitizer is never loaded into Python)
  cleared(key, lacs)                                streams that may go to a device: the sanitized twin has passed them"""
from __future__ import annotations

import ctypes as C
import struct
import sys
from collections import namedtuple

import numpy as np

import dectwin
import salvagetwin
import twinbuild

SRC = twinbuild.NATIVE + "/sim_stats.cpp"
LAYOUTS = {"planar_i32": 0, "inter_i16": 1, "inter_i24": 2, "planar_i16": 16, "planar_f32": 17, "inter_f32": 18}
CLEAN = (1 << 64) - 1
NONE = (1 << 64) - 1
ENV = dict(ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
FORMATS = ((1, 16, 44100), (2, 16, 48000), (1, 24, 96000), (2, 24, 192000))
SIZES = (1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 16383, 16384, 16385, 2 * 16384 + 1)  # unit, wave, workgroup and block borders
BLOCK = 16384

# ch: ((min, max, or_bits, full_scale, zeros, sum, sum_sq),) * 2 -- the second all zero for mono
Row = namedtuple("Row", "frames code lead trail differing ch")
Totals = namedtuple("Totals", "frames rate channels depth blocks lost_blocks lost_frames silent_blocks lead trail differing ch")
ZERO_CH = (0, 0, 0, 0, 0, 0, 0)

CH_T = np.dtype([("min", "<i4"), ("max", "<i4"), ("or_bits", "<u4"), ("full_scale", "<u4"), ("zeros", "<u4"), ("reserved", "<u4"),
                 ("sum", "<i8"), ("sum_sq", "<u8")])
ROW_T = np.dtype([("frames", "<u4"), ("code", "<u4"), ("lead", "<u4"), ("trail", "<u4"), ("differing", "<u4"), ("reserved", "<u4"),
                  ("ch", CH_T, (2,))])
TCH_T = np.dtype([("min", "<i4"), ("max", "<i4"), ("or_bits", "<u4"), ("reserved", "<u4"), ("full_scale", "<u8"), ("zeros", "<u8"),
                  ("sum_lo", "<u8"), ("sum_hi", "<i8"), ("sum_sq_lo", "<u8"), ("sum_sq_hi", "<u8")])
TOT_T = np.dtype([("frames", "<u8"), ("rate", "<u4"), ("channels", "u1"), ("depth", "u1"), ("reserved", "u1", (2,)), ("blocks", "<u4"),
                  ("lost_blocks", "<u4"), ("lost_frames", "<u8"), ("silent_blocks", "<u4"), ("reserved2", "<u4"), ("lead", "<u8"),
                  ("trail", "<u8"), ("differing", "<u8"), ("ch", TCH_T, (2,))])
assert (CH_T.itemsize, ROW_T.itemsize, TCH_T.itemsize, TOT_T.itemsize) == (40, 104, 64, 192)

_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(twinbuild.shared_lib("sim_stats", [SRC]))
        _lib.sim_stats.restype = C.c_int64
        _lib.sim_stats_source.restype = C.c_int64
        _lib.sim_stats_combine.restype = None
    return _lib


def sanitized_exe():
    """The sanitized program's path, or (None, why) where the sanitizer runtime is missing."""
    return twinbuild.sanitized_exe("sim_stats_san", [SRC], ["-DSIM_STATS_MAIN"])


# ---- expectations -----------------------------------------------------------------------------------------------------
def _channel(x, depth):
    lim = 1 << (depth - 1)
    o = x.astype(object)
    return (int(x.min()), int(x.max()), int(np.bitwise_or.reduce(x.astype(np.int64) & ((1 << depth) - 1))),
            int(np.count_nonzero((x == -lim) | (x == lim - 1))), int(x.size - np.count_nonzero(x)), int(sum(o)), int(sum(o * o)))


def expected_rows(left, right, depth, blocks, lost=None):
    """[Row] of PCM cut into blocks of `blocks` frames; lost[b] = a fault code (or True) marks a lost block: frames and
    code, every other field 0."""
    rows, at = [], 0
    for b, n in enumerate(blocks):
        code = lost[b] if lost is not None else 0
        if code:
            rows.append(Row(n, code, 0, 0, 0, (ZERO_CH, ZERO_CH)))
            at += n
            continue
        l = np.asarray(left[at:at + n], np.int32)
        r = None if right is None else np.asarray(right[at:at + n], np.int32)
        nz = np.flatnonzero(l != 0 if r is None else (l != 0) | (r != 0))
        lead, trail = (n, n) if nz.size == 0 else (int(nz[0]), int(n - 1 - nz[-1]))
        rows.append(Row(n, 0, lead, trail, 0 if r is None else int(np.count_nonzero(l != r)),
                        (_channel(l, depth), ZERO_CH if r is None else _channel(r, depth))))
        at += n
    return rows


def expected_totals(rows, channels, depth, rate):
    """The per-item record restated in Python ints: totals over the decoded blocks, the lead / trail rule with a lost block
    counting as sound."""
    good = [r for r in rows if not r.code]
    ch = []
    for c in range(2):
        if c >= channels:
            ch.append(ZERO_CH)
            continue
        parts = [r.ch[c] for r in good]
        bits = 0
        for p in parts:
            bits |= p[2]
        ch.append((min((p[0] for p in parts), default=0), max((p[1] for p in parts), default=0), bits, sum(p[3] for p in parts),
                   sum(p[4] for p in parts), sum(p[5] for p in parts), sum(p[6] for p in parts)))
    lead = trail = 0
    for r in rows:
        if r.code:
            break
        lead += r.lead
        if r.lead != r.frames:
            break
    for r in reversed(rows):
        if r.code:
            break
        trail += r.trail
        if r.trail != r.frames:
            break
    return Totals(sum(r.frames for r in rows), rate, channels, depth, len(rows), len(rows) - len(good), sum(r.frames for r in rows if r.code),
                  sum(1 for r in good if r.lead == r.frames), lead, trail, sum(r.differing for r in good), tuple(ch))


def wasted_bits(totals):
    bits = totals.ch[0][2] | totals.ch[1][2]
    return totals.depth if bits == 0 else (bits & -bits).bit_length() - 1


def grid_blocks(frames, grid=BLOCK):
    return [min(grid, frames - a) for a in range(0, frames, grid)]


# ---- records, whoever made them, as Row / Totals ------------------------------------------------------------------------
def _ch_of(c):
    return (int(c["min"]), int(c["max"]), int(c["or_bits"]), int(c["full_scale"]), int(c["zeros"]), int(c["sum"]), int(c["sum_sq"]))


def _tch_of(c):
    return (int(c["min"]), int(c["max"]), int(c["or_bits"]), int(c["full_scale"]), int(c["zeros"]),
            (int(c["sum_hi"]) << 64) + int(c["sum_lo"]), (int(c["sum_sq_hi"]) << 64) + int(c["sum_sq_lo"]))


def rows_of(records):
    """ctypes BlockStats records (the product's) or a ROW_T array (the twin's) -> [Row]."""
    a = records if isinstance(records, np.ndarray) else np.frombuffer(b"".join(bytes(r) for r in records), ROW_T)
    return [Row(int(r["frames"]), int(r["code"]), int(r["lead"]), int(r["trail"]), int(r["differing"]), (_ch_of(r["ch"][0]), _ch_of(r["ch"][1])))
            for r in a]


def totals_of(record):
    """A ctypes Stats record (the product's) or a TOT_T element (the twin's) -> Totals."""
    t = record if isinstance(record, (np.void, np.ndarray)) else np.frombuffer(bytes(record), TOT_T)[0]
    return Totals(int(t["frames"]), int(t["rate"]), int(t["channels"]), int(t["depth"]), int(t["blocks"]), int(t["lost_blocks"]),
                  int(t["lost_frames"]), int(t["silent_blocks"]), int(t["lead"]), int(t["trail"]), int(t["differing"]),
                  (_tch_of(t["ch"][0]), _tch_of(t["ch"][1])))


def row_records(rows):
    """[Row] -> a ROW_T array (fabricated rows for lacx_stats_combine)."""
    a = np.zeros(len(rows), ROW_T)
    for k, r in enumerate(rows):
        a[k]["frames"], a[k]["code"], a[k]["lead"], a[k]["trail"], a[k]["differing"] = r.frames, r.code, r.lead, r.trail, r.differing
        for c in range(2):
            for name, v in zip(("min", "max", "or_bits", "full_scale", "zeros", "sum", "sum_sq"), r.ch[c]):
                a[k]["ch"][c][name] = v
    return a


# ---- signals ----------------------------------------------------------------------------------------------------------
Item = namedtuple("Item", "name channels depth rate left right")


def _noise(frames, depth, seed, shift=3):
    rng = np.random.default_rng(seed)
    lim = 1 << (depth - 1)
    return (rng.integers(-lim, lim, frames, dtype=np.int64) >> shift).astype(np.int32)


def signal(frames, channels, depth, seed, lead=0, trail=0):
    """Noise a few bits below full scale (never 0 at a frame that is to sound) with `lead` / `trail` zero frames at its ends."""
    out = []
    for c in range(channels):
        x = _noise(frames, depth, seed * 2 + c)
        x[x == 0] = 1
        x[:min(lead, frames)] = 0
        if trail:
            x[max(0, frames - trail):] = 0
        out.append(x)
    return out[0], out[1] if channels == 2 else None


def plant_full_scale(left, right, depth, places):
    """-2^(b-1) and 2^(b-1)-1 alternately at `places` in each channel (the right channel the other way round)."""
    lo, hi = -(1 << (depth - 1)), (1 << (depth - 1)) - 1
    for k, f in enumerate(places):
        if f < left.size:
            left[f] = (lo, hi)[k & 1]
            if right is not None:
                right[f] = (hi, lo)[k & 1]


def content_items():
    """The signals statistics are about; assert_content states what they hold."""
    items = []
    for k, (ch, depth, rate) in enumerate(FORMATS):  # zero frames at both ends over a block border, every residue mod 4
        frames = 2 * BLOCK + 300
        l, r = signal(frames, ch, depth, 100 + k, lead=BLOCK + 8 + k, trail=300 + 1 + k)
        items.append(Item("edges%d" % k, ch, depth, rate, l, r))
    for ch, depth, rate in FORMATS:
        tag = "%dch%d" % (ch, depth)
        l, r = signal(3 * BLOCK, ch, depth, 200 + depth + ch)  # a wholly silent block between two sounding ones
        l[BLOCK:2 * BLOCK] = 0
        if r is not None:
            r[BLOCK:2 * BLOCK] = 0
        items.append(Item("silent_middle|" + tag, ch, depth, rate, l, r))
        l, r = signal(2 * BLOCK + 1, ch, depth, 300 + depth + ch)  # full scale at a unit's first and last frame and on both
        plant_full_scale(l, r, depth, (40, 43, BLOCK - 1, BLOCK))  # sides of a block border, in each channel
        if r is not None:  # a stretch with left == right and one frame in it where they differ
            r[1000:3000] = l[1000:3000]
            r[2000] = l[2000] + 1
        items.append(Item("planted|" + tag, ch, depth, rate, l, r))
        items.append(Item("zero|" + tag, ch, depth, rate, np.zeros(BLOCK + 5, np.int32), np.zeros(BLOCK + 5, np.int32) if ch == 2 else None))
        l, r = signal(BLOCK + 7, ch, depth, 400 + depth + ch)  # negative DC: noise around -2^(b-3)
        l = (l >> 2) - (1 << (depth - 3))
        items.append(Item("negative_dc|" + tag, ch, depth, rate, l.astype(np.int32), None if r is None else ((r >> 2) - (1 << (depth - 3))).astype(np.int32)))
        if ch == 2:
            l, _ = signal(BLOCK + 9, 1, depth, 500 + depth)
            items.append(Item("dual_mono|" + tag, ch, depth, rate, l, l.copy()))
        if depth == 24:  # 16-bit audio in a 24-bit file: every sample a multiple of 256
            l, r = signal(BLOCK + 3, ch, 16, 600 + ch)
            items.append(Item("wasted8|" + tag, ch, depth, rate, l * 256, None if r is None else r * 256))
    return items


def item_rows(it, blocks=None):
    return expected_rows(it.left, it.right, it.depth, blocks or grid_blocks(it.left.size))


def assert_content(items):
    """On the expectation alone: the signals hold what the issue lists."""
    rows = {it.name: item_rows(it) for it in items}
    tot = {it.name: expected_totals(rows[it.name], it.channels, it.depth, it.rate) for it in items}
    edges = [tot["edges%d" % k] for k in range(4)]
    assert sorted(t.lead % 4 for t in edges) == [0, 1, 2, 3] and all(t.lead > BLOCK for t in edges)  # over a block border
    assert sorted(t.trail % 4 for t in edges) == [0, 1, 2, 3] and all(t.trail > 300 for t in edges)
    assert all(t.silent_blocks == 2 for t in edges)
    for ch, depth, _ in FORMATS:
        tag = "%dch%d" % (ch, depth)
        mid = rows["silent_middle|" + tag]
        assert [r.lead == r.frames for r in mid] == [False, True, False] and tot["silent_middle|" + tag].silent_blocks == 1
        assert tot["silent_middle|" + tag].lead == 0 and tot["silent_middle|" + tag].trail == 0
        planted = rows["planted|" + tag]
        assert all(planted[b].ch[c][3] >= 1 for b in (0, 1) for c in range(ch)), "full scale on both sides of the border, in each channel"
        assert planted[0].ch[0][0] == -(1 << (depth - 1)) and planted[0].ch[0][1] == (1 << (depth - 1)) - 1
        if ch == 2:
            l, r = next((it.left, it.right) for it in items if it.name == "planted|" + tag)
            assert np.count_nonzero(l[1000:3000] != r[1000:3000]) == 1
            assert tot["dual_mono|" + tag].differing == 0 and tot["planted|" + tag].differing > 1
        z = tot["zero|" + tag]
        assert wasted_bits(z) == depth and z.lead == z.trail == z.frames and z.silent_blocks == z.blocks == 2
        assert all(tot["negative_dc|" + tag].ch[c][5] < 0 for c in range(ch))
        if depth == 24:
            assert wasted_bits(tot["wasted8|" + tag]) == 8


def shape_items():
    """Every format at every border size, with zero frames at the ends (every residue mod 4 over the sizes) and full-scale
    samples where there is room: [Item]."""
    items, seed = [], 0
    for ch, depth, rate in FORMATS:
        for frames in SIZES:
            seed += 1
            room = frames >= 16
            l, r = signal(frames, ch, depth, 1000 + seed, lead=seed % 4 if room else 0, trail=(seed // 4) % 4 if room else 0)
            if room:
                plant_full_scale(l, r, depth, (8, 11, BLOCK - 1, BLOCK))
            items.append(Item("n%d|%dch%d" % (frames, ch, depth), ch, depth, rate, l, r))
    return items


def spliced_parts(ch, depth):
    """The PCM of the spliced three-block stream of 257 / 258 / 259 frames: [(left, right)], a part's ends silent."""
    return [signal(n, ch, depth, 900 + n + depth + ch, lead=n % 4, trail=(n + 1) % 4) for n in (257, 258, 259)]


# ---- the twin ---------------------------------------------------------------------------------------------------------
TwinItem = namedtuple("TwinItem", "code message rows totals")


def run(lacs, cols=1, zero_status=False):
    """n streams as one stats job on the CPU twin -> ([TwinItem], sets of atomics)."""
    n = len(lacs)
    ptrs = (C.c_char_p * n)(*lacs)
    sizes = (C.c_uint64 * n)(*[len(x) for x in lacs])
    shapes = [dectwin._shape(x) if salvagetwin._head_ok(x) else (0, []) for x in lacs]
    nblocks = sum(nb for nb, _ in shapes) + 1
    rec = np.zeros(2 * n, np.uint64)
    rows = np.zeros(nblocks, ROW_T)
    totals = np.zeros(n, TOT_T)
    msg = C.create_string_buffer(1 << 16)
    sets = C.c_uint64()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    got = lib().sim_stats(ptrs, sizes, C.c_uint32(n), int(cols), int(zero_status), vp(rec), vp(rows), C.c_uint64(nblocks), vp(totals), msg,
                          C.c_uint32(len(msg)), C.byref(sets))
    assert got >= 0, "the twin could not run the job"
    msgs = msg.value.decode().split("\n")
    items, at = [], 0
    for i in range(n):
        code, nb = int(rec[2 * i]), int(rec[2 * i + 1])
        if code:
            items.append(TwinItem(code, msgs[i], None, totals_of(totals[i])))
            continue
        items.append(TwinItem(0, "", rows_of(rows[at:at + nb]), totals_of(totals[i])))
        at += nb
    return items, sets.value


def source_rows(layout, channels, depth, grid, offset, left, right=None, bad=None, as_line=False):
    """The source form on the twin -> ([Row], Totals, key, message, sets).  bad = (frame, channel, raw 32-bit word)."""
    frames = len(left)
    samples = np.concatenate([np.asarray(left, np.int32)] + ([np.asarray(right, np.int32)] if channels == 2 else []))
    cap = frames // grid + 2
    rows, totals = np.zeros(cap, ROW_T), np.zeros(1, TOT_T)
    key, sets = C.c_uint64(), C.c_uint64()
    msg = C.create_string_buffer(256)
    bf, bc, bw = bad if bad else (NONE, 0, 0)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    nb = lib().sim_stats_source(C.c_uint32(layout), C.c_uint32(channels), C.c_uint32(depth), C.c_uint64(frames), C.c_uint32(grid),
                                C.c_uint32(offset), vp(samples), C.c_uint64(bf), C.c_uint32(bc), C.c_uint32(bw), vp(rows), C.c_uint64(cap),
                                vp(totals), C.byref(key), msg, C.c_uint32(len(msg)), C.byref(sets))
    assert nb >= 0, "the twin could not run the source"
    if as_line:  # what the sanitized program prints for this case behind its index
        return "%d %d %s %s %s" % (key.value, nb, _hash(rows[:nb].tobytes()), _hash(totals.tobytes()), msg.value.decode())
    return rows_of(rows[:nb]), totals_of(totals[0]), key.value, msg.value.decode(), sets.value


def twin_combine(rows, channels, depth, rate):
    """csrc/stats_rows.h's totals of fabricated rows -> Totals."""
    a, out = row_records(rows), np.zeros(1, TOT_T)
    lib().sim_stats_combine(a.ctypes.data_as(C.c_void_p), C.c_uint32(len(rows)), C.c_uint32(channels), C.c_uint32(depth), C.c_uint32(rate),
                            out.ctypes.data_as(C.c_void_p))
    return totals_of(out[0])


# ---- the sanitized program ----------------------------------------------------------------------------------------------
def case(lacs, cols=1, zero_status=False) -> bytes:
    body = struct.pack("<II", len(lacs), (4 if cols == 64 else 0) | (8 if zero_status else 0))
    for x in lacs:
        body += struct.pack("<Q", len(x)) + x
    return b"\0" + body


def source_case(layout, channels, depth, grid, offset, left, right=None, bad=None) -> bytes:
    samples = np.concatenate([np.asarray(left, np.int32)] + ([np.asarray(right, np.int32)] if channels == 2 else []))
    bf, bc, bw = bad if bad else (NONE, 0, 0)
    return b"\1" + struct.pack("<IIIIIQQII", layout, channels, depth, grid, offset, len(left), bf, bc, bw) + samples.astype("<i4").tobytes()


def _hash(data: bytes) -> str:
    h = 0xCBF29CE484222325
    for b in data:
        h = ((h ^ b) * 0x100000001B3) & CLEAN
    return "%016x" % h


def line(blob: bytes, index: int) -> str:
    """The plain build's line for a stream case (what the sanitized program must print for it)."""
    assert blob[0] == 0
    buf = C.create_string_buffer(1 << 20)
    rc = lib().sim_stats_line(blob[1:], C.c_uint64(len(blob) - 1), C.c_uint32(index), buf, C.c_uint32(len(buf)))
    assert rc == 0
    return buf.value.decode()


def run_sanitized(cases, exe=None, workers=8):
    """Every case through the sanitized program, split over a few processes: (lines, returncode, stderr)."""
    if exe is None:
        exe, why = sanitized_exe()
        assert exe, why
    return twinbuild.run_cases(exe, cases, ENV, workers=workers, prefix="lac_stats_")


BATCH = 64


def cleared(key, lacs):
    """lacs, once the sanitized twin has shown in this run that a stats job over them stays inside buffers of exactly the
    plan's capacities -- both status fills, 1 and 64 columns, in batches -- and answers as the plain build does.  Fails,
    never skips, where that cannot be shown."""
    def make():
        cases = []
        for at in range(0, len(lacs), BATCH):
            part = lacs[at:at + BATCH]
            cases.append(case(part, cols=1, zero_status=False))
            cases.append(case(part, cols=64, zero_status=True))
        return cases, lambda c, i: line(c, i).split(" ", 1)[1], None, list(lacs)

    return twinbuild.cleared("stats", key, sys.modules[__name__], make)
