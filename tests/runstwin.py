"""Runs off the device: where their expectations come from, the signals the tests run on, and their CPU twin.

  frame_mask(det, left, right, counted)            the frame predicate as a boolean numpy mask -- never the twin
  runs_of(mask, min_frames) / totals_of(runs)      run lengths from the mask's differences; the totals in Python ints
  expected(det, left, right, counted)              (runs, totals) of one detector
  counted_of(blocks, lost)                         which frames lie in blocks that count
  border_item / shape_items / ... / assert_content  seeded signals built for the borders of the kernel (unit 4, wave 256, tile
                                                    1024, block 16384); assert_content checks on the expectation that they
                                                    hold what they are for
  run(lacs, detectors, ...)                        the CPU twin (tests/native/sim_runs.cpp: csrc/decode_plan.h's runs job,
                                                    runs_core.h combined as k_runs combines it, runs_rows.h), plain build
  source_runs(...)                                 the source form: one item in a layout at a base offset
  case / source_case / line / run_sanitized        the same through the build with AddressSanitizer + UBSan, a program of
                                                    its own (a sanitizer is never loaded into Python)
  cleared(key, lacs, detectors)                    streams that may go to a device: the sanitized twin has passed them"""
from __future__ import annotations

import ctypes as C
import struct
import sys
from collections import namedtuple

import numpy as np

import lacmutate
import lacstreams
import salvagetwin
import twinbuild

SRC = twinbuild.NATIVE + "/sim_runs.cpp"
LAYOUTS = {"planar_i32": 0, "inter_i16": 1, "inter_i24": 2, "planar_i16": 16, "planar_f32": 17, "inter_f32": 18}
CLEAN = NONE = (1 << 64) - 1
ENV = dict(ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
QUIET, PEAK, FLAT, ALL = 0, 1, 2, 255
UNIT, WAVE, TILE, BLOCK = 4, 256, 1024, 16384
DEFAULT_CAP = 8192  # kRunsListCap
RERUN = 1
FORMATS = ((1, 16, 44100), (2, 16, 48000), (1, 24, 96000), (2, 24, 192000))
# each border - 1, exact, + 1: unit, wave, tile, block (and the workgroup, which is the tile)
SIZES = (1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 16383, 16384, 16385, 2 * 16384 + 1)

Det = namedtuple("Det", "kind channel level min_frames")
Totals = namedtuple("Totals", "runs frames longest longest_start")
Result = namedtuple("Result", "frames lost_frames rate blocks lost_blocks flags channels depth detectors totals")

DET_T = np.dtype([("kind", "u1"), ("channel", "u1"), ("reserved", "u1", (2,)), ("level", "<u4"), ("min_frames", "<u8")])
QUERY_T = np.dtype([("first", "<u4"), ("count", "<u4")])
RUN_T = np.dtype([("start", "<u8"), ("frames", "<u8")])
TOT_T = np.dtype([("runs", "<u8"), ("frames", "<u8"), ("longest", "<u8"), ("longest_start", "<u8")])
RES_T = np.dtype([("frames", "<u8"), ("lost_frames", "<u8"), ("rate", "<u4"), ("blocks", "<u4"), ("lost_blocks", "<u4"), ("flags", "<u4"),
                  ("channels", "u1"), ("depth", "u1"), ("detectors", "u1"), ("reserved", "u1", (5,)), ("det", TOT_T, (8,))])
assert (DET_T.itemsize, QUERY_T.itemsize, RUN_T.itemsize, TOT_T.itemsize, RES_T.itemsize) == (16, 8, 16, 32, 296)

_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(twinbuild.shared_lib("sim_runs", [SRC]))
        _lib.sim_runs.restype = C.c_int64
        _lib.sim_runs_source.restype = C.c_int64
        _lib.sim_runs_stitch.restype = C.c_int64
        _lib.sim_runs_reserve.restype = C.c_uint64
        _lib.sim_runs_check.restype = C.c_char_p
    return _lib


def sanitized_exe():
    """The sanitized program's path, or (None, why) where the sanitizer runtime is missing."""
    return twinbuild.sanitized_exe("sim_runs_san", [SRC], ["-DSIM_RUNS_MAIN"])


# ---- expectations -----------------------------------------------------------------------------------------------------
def full_scale(depth):
    return (1 << (depth - 1)) - 1


def counted_of(blocks, lost=None):
    """Per frame: its block counts (it is neither lost nor missing)."""
    out = np.ones(sum(blocks), bool)
    at = 0
    for b, n in enumerate(blocks):
        if lost is not None and lost[b]:
            out[at:at + n] = False
        at += n
    return out


def frame_mask(det, left, right, counted=None):
    """P(f) of a detector for every frame, from the words of include/lacx.h."""
    n = len(left)
    counted = np.ones(n, bool) if counted is None else counted
    chans = [c for c, x in ((0, left), (1, right)) if x is not None and det.channel in (c, ALL)]
    if not chans:
        return np.zeros(n, bool)
    mask = counted.copy()
    if det.kind == FLAT:
        mask[1:] &= counted[:-1]
        mask[:1] = False
    for c in chans:
        x = np.asarray(right if c else left, np.int64)
        if det.kind == QUIET:
            mask &= (x >= -det.level) & (x <= det.level)
        elif det.kind == PEAK:
            mask &= (x >= det.level) | (x <= -det.level - 1)
        else:
            mask[1:] &= x[1:] == x[:-1]
    return mask


def runs_of(mask, min_frames):
    """[(start, frames)] of the maximal stretches of True that reach min_frames."""
    d = np.diff(np.concatenate([[0], mask.astype(np.int8), [0]]))
    starts, ends = np.flatnonzero(d == 1), np.flatnonzero(d == -1)
    return [(int(s), int(e - s)) for s, e in zip(starts, ends) if e - s >= min_frames]


def totals_of(runs):
    longest = max((n for _, n in runs), default=0)
    return Totals(len(runs), sum(n for _, n in runs), longest, next((s for s, n in runs if n == longest), 0) if runs else 0)


def expected(det, left, right, counted=None):
    runs = runs_of(frame_mask(det, left, right, counted), det.min_frames)
    return runs, totals_of(runs)


def reserve(frames, min_frames, cap=DEFAULT_CAP):
    return min((frames + 1) // (min_frames + 1), cap)


def pieces_of(frames, quiet_runs, pad=0):
    """The complement of the runs inside [0, frames), each piece widened by pad, clipped, merged where pieces touch --
    restated over a boolean array."""
    sound = np.ones(frames, bool)
    for s, n in quiet_runs:
        sound[s:s + n] = False
    keep = np.zeros(frames, bool)
    for s, n in runs_of(sound, 1):
        keep[max(0, s - pad):min(frames, s + n + pad)] = True
    # pieces that touch merge: a boolean array merges them by itself, but two pieces with nothing between them that did
    # not overlap must merge too -- they do, being adjacent True frames
    return runs_of(keep, 1)


# ---- signals ----------------------------------------------------------------------------------------------------------
Item = namedtuple("Item", "name channels depth rate left right")
LEVEL = 3  # the QUIET level the planted stretches are built for


def loud(frames, channels, depth, seed):
    """Noise that satisfies no detector of the tests: 100 <= |x| <= 2^(b-2), never two equal samples in a row."""
    out = []
    for c in range(channels):
        rng = np.random.default_rng(seed * 2 + c)
        x = rng.integers(100, 1 << (depth - 2), frames, dtype=np.int64)
        x[1:][x[1:] == x[:-1]] += 1
        x[1::2] = -x[1::2]  # (alternating signs: equal neighbours are impossible)
        out.append(x.astype(np.int32))
    return out[0], out[1] if channels == 2 else None


def plant_quiet(left, right, start, n, which=ALL):
    """|x| <= LEVEL over [start, start + n), no two neighbours equal, in the channels `which`."""
    vals = np.array([1, -2, 3, -3, 2, -1], np.int32)
    for c, x in ((0, left), (1, right)):
        if x is not None and which in (c, ALL):
            x[start:start + n] = vals[(np.arange(n) + c) % 6]


def plant_peak(left, right, depth, start, n, which=ALL, sign=0):
    """Full scale over [start, start + n): +, - alternating from `sign` on (so no two neighbours are equal)."""
    fs = np.array([full_scale(depth), -full_scale(depth) - 1], np.int32)
    for c, x in ((0, left), (1, right)):
        if x is not None and which in (c, ALL):
            x[start:start + n] = fs[(np.arange(n) + sign + c) % 2]


def plant_flat(left, right, start, n, value=777):
    """n equal samples from start on in every channel (a value that is neither quiet nor a peak): n - 1 flagged frames."""
    for x in (left, right):
        if x is not None:
            x[start:start + n] = value


BORDER_FRAMES = BLOCK + TILE + 7
# (start, frames) of the quiet stretches of border_item, and what each is for
BORDER_QUIET = {"starts_at_0": (0, 6), "inside_a_lane": (9, 2), "exactly_min": (14, 5), "min_less_1": (22, 4), "wave": (253, 7), "tile": (1020, 10),
                "two_tiles": (2040, 2061), "three_tiles": (5115, 3080), "block": (BLOCK - 4, 10), "ends_at_last": (BORDER_FRAMES - 6, 6)}
BORDER_PEAK = {"left+": (300, 3, 0, 0), "left-": (310, 1, 0, 1), "right+": (320, 3, 1, 1), "right-": (330, 1, 1, 0), "both": (9 * TILE - 2, 5, ALL, 0)}
BORDER_FLAT = {"tile": (10 * TILE - 3, 7), "lane": (9002, 3), "block": (BLOCK - 2, 5)}


def border_detectors(depth):
    """Eight detectors on one item: every kind, every channel choice, min_frames at and around the planted lengths."""
    fs = full_scale(depth)
    return [Det(QUIET, ALL, LEVEL, 1), Det(QUIET, ALL, LEVEL, 5), Det(QUIET, 0, LEVEL, 5), Det(QUIET, 1, LEVEL, 2), Det(PEAK, ALL, fs, 1),
            Det(PEAK, 0, fs, 1), Det(PEAK, 1, fs, 3), Det(FLAT, ALL, 0, 1)]


def border_item(channels, depth, rate, seed=1):
    left, right = loud(BORDER_FRAMES, channels, depth, seed)
    for s, n in BORDER_QUIET.values():
        plant_quiet(left, right, s, n)
    plant_quiet(left, right, 12000, 40, which=0)  # quiet in the left channel alone
    for s, n, which, sign in BORDER_PEAK.values():
        plant_peak(left, right, depth, s, n, which, sign)
    for s, n in BORDER_FLAT.values():
        plant_flat(left, right, s, n, 777)
    # (the FLAT stretch over the block border lies inside the quiet one there: equal quiet samples)
    plant_flat(left, right, BORDER_FLAT["block"][0], BORDER_FLAT["block"][1], 2)
    return Item("borders|%dch%d" % (channels, depth), channels, depth, rate, left, right)


def shape_items():
    """Every format at every border size: quiet everywhere but for one loud frame in the middle (none for sizes below 3), so
    a run starts at frame 0, one ends at the item's last frame, they cross every border inside, and neighbours in a batch
    end and begin with runs that must not join."""
    items = []
    for k, (ch, depth, rate) in enumerate(FORMATS):
        for frames in SIZES:
            left, right = loud(frames, ch, depth, 1000 + frames + k)
            plant_quiet(left, right, 0, frames)
            if frames >= 3:
                for x in (left, right):
                    if x is not None:
                        x[frames // 2] = 5000
            items.append(Item("n%d|%dch%d" % (frames, ch, depth), ch, depth, rate, left, right))
    return items


def shape_detectors():
    return [Det(QUIET, ALL, LEVEL, 1), Det(QUIET, ALL, LEVEL, 128), Det(PEAK, ALL, 5000, 1)]


ALT_FRAMES = 2 * TILE + 1


def alternating_item(channels=1, depth=16, rate=44100):
    """0, loud, 0, loud, ... with an odd frame count: QUIET(0) with min_frames 1 finds (frames + 1) / 2 runs, the bound."""
    left, right = loud(ALT_FRAMES, channels, depth, 77)
    for x in (left, right):
        if x is not None:
            x[0::2] = 0
    return Item("alternating|%dch%d" % (channels, depth), channels, depth, rate, left, right)


def every_frame_item(channels, depth, rate):
    """Noise over the whole range, both full-scale values among it: QUIET at 2^(b-1) - 1 misses only -2^(b-1)."""
    rng = np.random.default_rng(depth + channels)
    lim = 1 << (depth - 1)
    chans = [rng.integers(-lim + 1, lim, 3000, dtype=np.int64).astype(np.int32) for _ in range(channels)]
    chans[0][[0, 1500]] = -lim
    chans[-1][[700, 2999]] = lim - 1
    return Item("every|%dch%d" % (channels, depth), channels, depth, rate, chans[0], chans[1] if channels == 2 else None)


def every_frame_detectors(depth):
    lim = 1 << (depth - 1)
    return [Det(QUIET, ALL, lim - 1, 1), Det(QUIET, ALL, lim, 1), Det(QUIET, ALL, 0xFFFFFFFF, 1), Det(PEAK, ALL, lim - 1, 1), Det(PEAK, 0, lim - 1, 1)]


def spliced_parts(ch, depth):
    """The PCM of the spliced three-block stream of 257 / 258 / 259 frames: quiet and flat across both block borders."""
    left, right = loud(257 + 258 + 259, ch, depth, 900 + depth + ch)
    plant_quiet(left, right, 250, 12)
    plant_flat(left, right, 512, 6)
    plant_quiet(left, right, 770, 4)  # ... and to the stream's last frame
    cuts = (0, 257, 515, 774)
    return [(left[a:b], None if right is None else right[a:b]) for a, b in zip(cuts, cuts[1:])]


def spliced_detectors():
    return [Det(QUIET, ALL, LEVEL, 2), Det(FLAT, ALL, 0, 1), Det(FLAT, 0, 0, 5)]


def lossy_parts(ch, depth):
    """Three blocks of 257 / 258 / 259 frames for a stream whose middle block will be lost: one value held from inside
    block 0 to inside block 2, so that the frames behind the lost block equal the (lost) frames in front of them, and a
    quiet stretch over the first border."""
    left, right = loud(257 + 258 + 259, ch, depth, 950 + depth + ch)
    plant_flat(left, right, 240, 300, 1)  # |1| <= LEVEL: quiet and flat from 240 to 539, over the whole of block 1
    cuts = (0, 257, 515, 774)
    return [(left[a:b], None if right is None else right[a:b]) for a, b in zip(cuts, cuts[1:])]


def lossy_detectors():
    return [Det(QUIET, ALL, LEVEL, 1), Det(FLAT, ALL, 0, 1), Det(FLAT, ALL, 0, 24), Det(QUIET, ALL, 1 << 23, 1)]


def assert_content():
    """On the expectation alone: the constructed cases hold what they are for."""
    it = border_item(2, 16, 48000)
    dets = border_detectors(16)
    all1, _ = expected(dets[0], it.left, it.right)
    assert all(tuple(v) in all1 for v in BORDER_QUIET.values()) and len(all1) == len(BORDER_QUIET), all1
    q = BORDER_QUIET
    assert q["inside_a_lane"][0] // UNIT == (sum(q["inside_a_lane"]) - 1) // UNIT  # inside one lane
    assert q["exactly_min"][0] // UNIT != (sum(q["exactly_min"]) - 1) // UNIT  # across a lane border
    for name, size in (("wave", WAVE), ("tile", TILE), ("block", BLOCK)):
        assert q[name][0] // size + 1 == (sum(q[name]) - 1) // size
    assert q["two_tiles"][0] // TILE + 3 == (sum(q["two_tiles"]) - 1) // TILE and q["three_tiles"][0] // TILE + 4 == (sum(q["three_tiles"]) - 1) // TILE
    assert sum(q["ends_at_last"]) == BORDER_FRAMES and BORDER_FRAMES % UNIT != 0
    all5, _ = expected(dets[1], it.left, it.right)
    assert q["exactly_min"] in all5 and q["min_less_1"] not in all5 and q["inside_a_lane"] not in all5
    left5, _ = expected(dets[2], it.left, it.right)
    assert (12000, 40) in left5 and (12000, 40) not in all5
    for k, want in ((4, [(9214, 5)]), (5, [(300, 3), (310, 1), (9214, 5)]), (6, [(320, 3), (9214, 5)])):
        assert expected(dets[k], it.left, it.right)[0] == want, k
    vals = np.concatenate([it.left[300:303], it.left[310:311], it.right[320:323], it.right[330:331]])
    assert {32767, -32768} <= set(vals.tolist())  # both signs in each channel
    assert set(it.left[300:311].tolist()) >= {32767, -32768} and set(it.right[320:331].tolist()) >= {32767, -32768}
    flat, _ = expected(dets[7], it.left, it.right)
    assert flat == sorted((s + 1, n - 1) for s, n in BORDER_FLAT.values())  # N equal samples: N - 1 frames
    mono = border_item(1, 24, 96000)
    assert expected(Det(QUIET, 1, LEVEL, 1), mono.left, None)[0] == [] and expected(Det(FLAT, 1, 0, 1), mono.left, None)[0] == []
    alt = alternating_item()
    runs, tot = expected(Det(QUIET, ALL, 0, 1), alt.left, alt.right)
    assert tot.runs == (ALT_FRAMES + 1) // 2 == reserve(ALT_FRAMES, 1) and tot.frames == tot.runs
    for ch, depth, rate in FORMATS:
        ev = every_frame_item(ch, depth, rate)
        d = every_frame_detectors(depth)
        assert expected(d[0], ev.left, ev.right)[0] == [(1, 1499), (1501, 1499)]  # -2^(b-1) alone is not quiet at 2^(b-1) - 1
        assert expected(d[1], ev.left, ev.right)[0] == [(0, 3000)] == expected(d[2], ev.left, ev.right)[0]
    for it in shape_items():
        runs, _ = expected(shape_detectors()[0], it.left, it.right)
        n = it.left.size
        assert runs == ([(0, n)] if n < 3 else [(0, n // 2), (n // 2 + 1, n - n // 2 - 1)]), it.name
    parts = spliced_parts(2, 16)
    l, r = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    assert expected(spliced_detectors()[0], l, r)[0] == [(250, 12), (770, 4)] and expected(spliced_detectors()[1], l, r)[0] == [(513, 5)]
    parts = lossy_parts(2, 16)
    l, r = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    counted = counted_of([257, 258, 259], [False, True, False])
    assert expected(lossy_detectors()[0], l, r, counted)[0] == [(240, 17), (515, 25)]  # the lost block splits the run
    assert expected(lossy_detectors()[1], l, r, counted)[0] == [(241, 16), (516, 24)]  # the first frame behind it is not FLAT
    assert expected(lossy_detectors()[2], l, r, counted)[0] == [(516, 24)] and expected(lossy_detectors()[1], l, r)[0] == [(241, 299)]


# ---- records, whoever made them ---------------------------------------------------------------------------------------
def det_records(dets):
    a = np.zeros(max(1, len(dets)), DET_T)
    for k, d in enumerate(dets):
        a[k]["kind"], a[k]["channel"], a[k]["level"], a[k]["min_frames"] = d.kind, d.channel, d.level, d.min_frames
    return a


def tables(per_item):
    """per_item: [[Det]] -> (DET_T array, QUERY_T array, count)."""
    flat = [d for dets in per_item for d in dets]
    q = np.zeros(max(1, len(per_item)), QUERY_T)
    at = 0
    for i, dets in enumerate(per_item):
        q[i]["first"], q[i]["count"] = at, len(dets)
        at += len(dets)
    return det_records(flat), q, len(flat)


def result_of(record):
    """A ctypes RunsResult (the product's) or a RES_T element (the twin's) -> Result."""
    t = record if isinstance(record, (np.void, np.ndarray)) else np.frombuffer(bytes(record), RES_T)[0]
    return Result(int(t["frames"]), int(t["lost_frames"]), int(t["rate"]), int(t["blocks"]), int(t["lost_blocks"]), int(t["flags"]), int(t["channels"]),
                  int(t["depth"]), int(t["detectors"]),
                  tuple(Totals(int(d["runs"]), int(d["frames"]), int(d["longest"]), int(d["longest_start"])) for d in t["det"]))


def expected_result(dets, left, right, depth, rate, blocks, lost=None, flags=0):
    """(Result, [runs per detector]) of an item from its PCM."""
    counted = counted_of(blocks, lost)
    lists = [expected(d, left, right, counted)[0] for d in dets]
    tots = tuple(totals_of(l) for l in lists) + (Totals(0, 0, 0, 0),) * (8 - len(dets))
    lostb = [bool(x) for x in lost] if lost is not None else [False] * len(blocks)
    return Result(sum(blocks), sum(n for n, l in zip(blocks, lostb) if l), rate, len(blocks), sum(lostb), flags, 1 if right is None else 2, depth,
                  len(dets), tots), lists


def grid_blocks(frames, grid=BLOCK):
    return [min(grid, frames - a) for a in range(0, frames, grid)]


# ---- the twin ---------------------------------------------------------------------------------------------------------
TwinItem = namedtuple("TwinItem", "code message result lists")


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def run(lacs, per_item, cols=1, zero_status=False, list_cap=DEFAULT_CAP, runs_cap=1 << 20):
    """n streams as one runs job on the CPU twin -> [TwinItem].  per_item: [[Det]] per stream."""
    n = len(lacs)
    ptrs = (C.c_char_p * n)(*lacs)
    sizes = (C.c_uint64 * n)(*[len(x) for x in lacs])
    dets, queries, ndets = tables(per_item)
    rec, res = np.zeros(n, np.uint64), np.zeros(n, RES_T)
    runs, counts = np.zeros(runs_cap, RUN_T), np.zeros(8 * n, np.uint64)
    msg = C.create_string_buffer(1 << 16)
    got = lib().sim_runs(ptrs, sizes, C.c_uint32(n), _vp(queries), _vp(dets), C.c_uint32(ndets), int(cols), int(zero_status), C.c_uint64(list_cap),
                         _vp(rec), _vp(res), _vp(runs), C.c_uint64(runs_cap), _vp(counts), msg, C.c_uint32(len(msg)))
    assert got >= 0, "the twin could not run the job"
    msgs = msg.value.decode().split("\n")
    items, at = [], 0
    for i in range(n):
        if rec[i]:
            items.append(TwinItem(int(rec[i]), msgs[i], result_of(res[i]), None))
            continue
        lists = []
        for k in range(len(per_item[i])):
            c = int(counts[8 * i + k])
            lists.append([(int(r["start"]), int(r["frames"])) for r in runs[at:at + c]])
            at += c
        items.append(TwinItem(0, "", result_of(res[i]), lists))
    return items


def source_runs(layout, channels, depth, offset, left, right, dets, list_cap=DEFAULT_CAP, bad=None, as_line=False):
    """The source form on the twin -> (Result, [runs per detector], key, message).  bad = (frame, channel, raw 32-bit word)."""
    frames = len(left)
    samples = np.concatenate([np.asarray(left, np.int32)] + ([np.asarray(right, np.int32)] if channels == 2 else []))
    cap = (frames + 2) * len(dets)
    runs, counts, res = np.zeros(cap, RUN_T), np.zeros(8, np.uint64), np.zeros(1, RES_T)
    key = C.c_uint64()
    msg = C.create_string_buffer(256)
    bf, bc, bw = bad if bad else (NONE, 0, 0)
    got = lib().sim_runs_source(C.c_uint32(layout), C.c_uint32(channels), C.c_uint32(depth), C.c_uint64(frames), C.c_uint32(offset), _vp(samples),
                                _vp(det_records(dets)), C.c_uint32(len(dets)), C.c_uint64(list_cap), C.c_uint64(bf), C.c_uint32(bc), C.c_uint32(bw),
                                _vp(res), _vp(runs), C.c_uint64(cap), _vp(counts), C.byref(key), msg, C.c_uint32(len(msg)))
    assert got >= 0, "the twin could not run the source"
    if as_line:  # what the sanitized program prints for this case behind its index
        return "%d %s %s %s" % (key.value, _hash(res.tobytes()), _hash(counts.tobytes() + runs[:got].tobytes()), msg.value.decode())
    lists, at = [], 0
    for k in range(len(dets)):
        c = int(counts[k])
        lists.append([(int(r["start"]), int(r["frames"])) for r in runs[at:at + c]])
        at += c
    return result_of(res[0]), lists, key.value, msg.value.decode()


def stitch(frames, rows, min_frames):
    """csrc/runs_rows.h's stitching of fabricated (lead, trail) rows of one detector -> [(start, frames)]."""
    packed = np.array([lead | (trail << 16) for lead, trail in rows], np.uint32)
    out = np.zeros(len(rows) + 2, RUN_T)
    got = lib().sim_runs_stitch(C.c_uint64(frames), _vp(packed), C.c_uint64(min_frames), _vp(out), C.c_uint64(len(out)))
    assert got >= 0
    return [(int(r["start"]), int(r["frames"])) for r in out[:got]]


def rows_of_mask(mask):
    """The (lead, trail) rows the kernel leaves for a mask: per tile of 1024 frames the leading set frames, and -- for a
    full tile -- the trailing ones."""
    rows = []
    for at in range(0, len(mask), TILE):
        m = mask[at:at + TILE]
        off = np.flatnonzero(~m)
        lead = len(m) if off.size == 0 else int(off[0])
        trail = 0 if len(m) < TILE else TILE if off.size == 0 else TILE - 1 - int(off[-1])  # (a partial tile ends inside itself)
        rows.append((lead, trail))
    return rows


def check_text(query, dets, ndets=None):
    """check_detectors of csrc/runs_plan.h for a query (first, count) over [Det] -> its text, "" where it passes."""
    q = np.zeros(1, QUERY_T)
    q[0]["first"], q[0]["count"] = query
    return lib().sim_runs_check(_vp(q), _vp(det_records(dets)), C.c_uint32(len(dets) if ndets is None else ndets)).decode()


PLAN = "tables runs_list base lists rows total_tiles total_dets total_rows".split()


def plan(lacs, per_item, list_cap=DEFAULT_CAP):
    """The runs form of plan_decode for the streams -> dict of PLAN, and `raw`: the tables plan_fill_tables fills."""
    n = len(lacs)
    ptrs = (C.c_char_p * n)(*lacs)
    sizes = (C.c_uint64 * n)(*[len(x) for x in lacs])
    dets, queries, ndets = tables(per_item)
    out, raw = np.zeros(8, np.uint64), np.zeros(1 << 22, np.uint8)
    assert lib().sim_runs_plan(ptrs, sizes, C.c_uint32(n), _vp(queries), _vp(dets), C.c_uint32(ndets), C.c_uint64(list_cap), _vp(out), _vp(raw),
                               C.c_uint64(raw.size)) == 0
    p = dict(zip(PLAN, (int(v) for v in out)))
    p["raw"] = raw[:p["tables"]].tobytes()
    return p


# ---- streams: what the twin tests and the device tests run on ------------------------------------------------------------
def _encode(oracle, it):
    return oracle.encode(it.left, it.right, it.rate, it.depth, 0)


def _splice(oracle, parts, rate, depth):
    lacs = [oracle.encode(l, r, rate, depth, 0) for l, r in parts]
    return lacstreams.splice(lacstreams.splice(lacs[0], lacs[1]), lacs[2])


def build_streams(oracle):
    """[(name, stream, Item, block frames, [Det])]: per format the border item with eight detectors, the border sizes, the
    every-frame item and the spliced 257 / 258 / 259 stream; the alternation; a version-2 form of some."""
    out = []
    for ch, depth, rate in FORMATS:
        it = border_item(ch, depth, rate)
        out.append((it.name, _encode(oracle, it), it, grid_blocks(it.left.size), border_detectors(depth)))
        ev = every_frame_item(ch, depth, rate)
        out.append((ev.name, _encode(oracle, ev), ev, grid_blocks(ev.left.size), every_frame_detectors(depth)))
        parts = spliced_parts(ch, depth)
        sp = Item("splice|%dch%d" % (ch, depth), ch, depth, rate, np.concatenate([l for l, _ in parts]),
                     np.concatenate([r for _, r in parts]) if ch == 2 else None)
        out.append((sp.name, _splice(oracle, parts, rate, depth), sp, [257, 258, 259], spliced_detectors()))
    for it in shape_items():
        out.append((it.name, _encode(oracle, it), it, grid_blocks(it.left.size), shape_detectors()))
    alt = alternating_item()
    out.append((alt.name, _encode(oracle, alt), alt, grid_blocks(alt.left.size), [Det(QUIET, ALL, 0, 1), Det(QUIET, 0, 0, 2)]))
    for name, lac, it, blocks, dets in [x for x in out if x[0].startswith(("borders", "splice"))]:
        out.append(("v2|" + name, lacstreams.to_v2(lac), it, blocks, dets))
    return out


def check_item(name, item, it, blocks, dets, lost=None, flags=0):
    want, lists = expected_result(dets, it.left, it.right, it.depth, it.rate, blocks, lost, flags)
    assert item.code == 0 and item.lists == lists, name
    assert item.result == want, name


def damaged(oracle):
    """[(name, stream, [Det])] with lost blocks: the constructed three-block stream with its middle block damaged (a lost
    block inside a quiet and flat run), the same cut short inside its last block (lost at the end), with its first block
    damaged (lost at the start), and as version 2 (the blocks behind the damage are not reached)."""
    out = []
    for ch, depth, rate in ((2, 16, 48000), (1, 24, 96000)):
        lac = _splice(oracle, lossy_parts(ch, depth), rate, depth)
        for which in (1, 0):
            ent, pays = lacmutate._payloads(lac)
            pays[which] = pays[which][:1] + bytes([0x7F]) + pays[which][2:] if lac[4] == 2 else bytes([0x7F]) + pays[which][1:]
            bad = lacmutate._rebuild(lac, ent, pays)
            out.append(("lost%d|%dch%d" % (which, ch, depth), bad, lossy_detectors()))
            if which == 1:
                out.append(("lost1-v2|%dch%d" % (ch, depth), lacstreams.to_v2(bad), lossy_detectors()))
        out.append(("cut|%dch%d" % (ch, depth), lac[:-5], lossy_detectors()))
        out.append(("clean|%dch%d" % (ch, depth), lac, lossy_detectors()))
    return out


def check_damaged(oracle, name, lac, dets, item):
    exp = salvagetwin.expected(oracle, lac)
    blocks = [n for n, _ in lacmutate.table(lac)[1]]
    it = Item(name, lac[3], lac[8], salvagetwin.rate(lac), exp.left, exp.right)
    check_item(name, item, it, blocks, dets, exp.lost, item.result.flags)
    return exp



# ---- the sanitized program ----------------------------------------------------------------------------------------------
def case(lacs, per_item, cols=1, zero_status=False, list_cap=DEFAULT_CAP) -> bytes:
    dets, queries, ndets = tables(per_item)
    body = struct.pack("<IIQI", len(lacs), (4 if cols == 64 else 0) | (8 if zero_status else 0), list_cap, ndets)
    body += dets[:ndets].tobytes() + queries[:len(lacs)].tobytes()
    for x in lacs:
        body += struct.pack("<Q", len(x)) + x
    return b"\0" + body


def source_case(layout, channels, depth, offset, left, right, dets, list_cap=DEFAULT_CAP, bad=None) -> bytes:
    samples = np.concatenate([np.asarray(left, np.int32)] + ([np.asarray(right, np.int32)] if channels == 2 else []))
    bf, bc, bw = bad if bad else (NONE, 0, 0)
    return (b"\1" + struct.pack("<IIIIIQQQII", layout, channels, depth, offset, len(dets), len(left), list_cap, bf, bc, bw) +
            det_records(dets)[:len(dets)].tobytes() + samples.astype("<i4").tobytes())


def _hash(data: bytes) -> str:
    h = 0xCBF29CE484222325
    for b in data:
        h = ((h ^ b) * 0x100000001B3) & CLEAN
    return "%016x" % h


def line(blob: bytes, index: int) -> str:
    """The plain build's line for a stream case (what the sanitized program must print for it)."""
    assert blob[0] == 0
    buf = C.create_string_buffer(1 << 20)
    rc = lib().sim_runs_line(blob[1:], C.c_uint64(len(blob) - 1), C.c_uint32(index), buf, C.c_uint32(len(buf)))
    assert rc == 0
    return buf.value.decode()


def run_sanitized(cases, exe=None, workers=8):
    """Every case through the sanitized program, split over a few processes: (lines, returncode, stderr)."""
    if exe is None:
        exe, why = sanitized_exe()
        assert exe, why
    return twinbuild.run_cases(exe, cases, ENV, workers=workers, prefix="lac_runs_")


BATCH = 64


def cleared(key, lacs, per_item, list_cap=DEFAULT_CAP):
    """lacs, once the sanitized twin has shown in this run that a runs job over them with these detectors stays inside
    buffers of exactly the plan's capacities -- both status fills, 1 and 64 columns, in batches -- and answers as the
    plain build does.  Fails, never skips, where that cannot be shown."""
    def make():
        cases = []
        for at in range(0, len(lacs), BATCH):
            part, dets = lacs[at:at + BATCH], per_item[at:at + BATCH]
            cases.append(case(part, dets, cols=1, zero_status=False, list_cap=list_cap))
            cases.append(case(part, dets, cols=64, zero_status=True, list_cap=list_cap))
        return cases, lambda c, i: line(c, i).split(" ", 1)[1], None, list(lacs)

    return twinbuild.cleared("runs", key, sys.modules[__name__], make)
