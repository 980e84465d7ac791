"""Rip checksums off the device: where their expectations come from, the discs the tests run on, and the CPU twin.

  words(disc)                           the disc's 32-bit words, (uint16)left | (uint16)right << 16
  expected(disc)                        the three sums at every offset, restated in numpy: uint64 products, & 0xFFFFFFFF, >> 32
                                        -- never the code under test
  expected_prefix(disc)                 v1 and s450 a second, independent way: prefix sums P0 = sum x(j), P1 = sum j x(j)
  v2_bigint(disc, t, o)                 one v2 in Python integers
  expected_ids(tracks, ...)             the disc ids in plain Python
  corpus()                              frozen seeded discs over every class the plan and the kernel tell apart
  run(case) / source_case / stream_case the CPU twin (tests/native/sim_accuraterip.cpp: csrc/decode_plan.h's rip-checksum job,
                                        csrc/accuraterip_plan.h and csrc/accuraterip_core.h as k_accuraterip runs it), plain
  line / run_sanitized                  the same through the build with AddressSanitizer + UBSan, a program of its own
                                        (a sanitizer is never loaded into Python)
  cleared(key, cases)                   cases that may go to a device: the sanitized twin has passed them

Everything is exact integer arithmetic mod 2^32: sums are compared byte for byte."""
from __future__ import annotations

import ctypes as C
import struct
import sys
from collections import namedtuple

import numpy as np

import twinbuild

SRC = twinbuild.NATIVE + "/sim_accuraterip.cpp"
ENV = dict(ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
SECTOR, EDGE, MAX_RADIUS = 588, 2940, 2939
S450_AT, S450_MIN = 450 * 588, 451 * 588
FIRST, LAST, NO_IDS = 1, 2, 4
TRACK_SHORT, TRACK_NO_S450 = 1, 2
MASK = 0xFFFFFFFF
NONE = (1 << 64) - 1
P32, I16, P16, PF32, IF32 = 0, 1, 16, 17, 18  # the layouts that can hold 16-bit audio
RADII = (0, 1, 31, 32, 127, 128, 300, 2939)

TRACK_T = np.dtype([("start", "<u8"), ("frames", "<u8"), ("flags", "<u4"), ("v1", "<u4"), ("v2", "<u4"), ("s450", "<u4")])
RESULT_T = np.dtype([("frames", "<u8"), ("tracks", "<u4"), ("radius", "<u4"), ("flags", "<u4"), ("id1", "<u4"), ("id2", "<u4"), ("cddb", "<u4")])
assert (TRACK_T.itemsize, RESULT_T.itemsize) == (32, 32)

Disc = namedtuple("Disc", "name sources tracks radius first last lba0", defaults=(0,))


def flags_of(disc):
    return (FIRST if disc.first else 0) | (LAST if disc.last else 0)


def track_frames(disc):
    return list(disc.tracks) if disc.tracks is not None else [len(l) for l, _ in disc.sources]


def words(disc):
    left = np.concatenate([np.asarray(l, np.int64) for l, _ in disc.sources])
    right = np.concatenate([np.asarray(r, np.int64) for _, r in disc.sources])
    return ((left & 0xFFFF) | ((right & 0xFFFF) << 16)).astype(np.uint32)


def ranges(disc):
    """Per track (start, frames, lo, hi, flags): the multiplier range lo .. hi (empty where hi < lo) and the LACX_AR_TRACK_* flags."""
    out, start, tf = [], 0, track_frames(disc)
    for t, n in enumerate(tf):
        lo = EDGE if t == 0 and disc.first else 1
        hi = n - EDGE if t == len(tf) - 1 and disc.last else n
        out.append((start, n, lo, hi, (TRACK_SHORT if hi < lo else 0) | (TRACK_NO_S450 if n < S450_MIN else 0)))
        start += n
    return out


# ---- expectations -----------------------------------------------------------------------------------------------------
def _padded(disc):
    """x over disc frames -pad .. D + pad - 1 as uint64, zeros outside the disc; pad."""
    x = words(disc)
    pad = disc.radius + 1
    return np.concatenate([np.zeros(pad, np.uint64), x.astype(np.uint64), np.zeros(pad + SECTOR, np.uint64)]), pad


def _brute(xp, at, lo, hi, radius):
    """sum over m = lo .. hi of the halves of m * xp[at + o + m - 1], every o in [-radius, radius]: (low sums, high sums)."""
    m = np.arange(lo, hi + 1, dtype=np.uint64)
    win = np.lib.stride_tricks.sliding_window_view(xp, len(m))
    first = at + lo - 1 - radius  # the window of o = -radius
    los, his = np.zeros(2 * radius + 1, np.uint32), np.zeros(2 * radius + 1, np.uint32)
    step = max(1, (1 << 22) // len(m))
    for k in range(0, 2 * radius + 1, step):
        p = win[first + k:first + min(k + step, 2 * radius + 1)] * m  # uint64 products: 32 x 32 bits
        los[k:k + p.shape[0]] = ((p & np.uint64(MASK)).sum(axis=1) & np.uint64(MASK)).astype(np.uint32)
        his[k:k + p.shape[0]] = ((p >> np.uint64(32)).sum(axis=1) & np.uint64(MASK)).astype(np.uint32)
    return los, his


Sums = namedtuple("Sums", "v1 v2 s450 flags")
_expected = {}


def expected(disc, kinds=("v1", "v2", "s450")):
    """The sums of every track at every offset, (T, 2 radius + 1) uint32 each, by the definition: computed once per disc and
    shared (callers do not change it).  kinds: what to compute (the others stay zero)."""
    key = (disc.name, kinds)
    if key in _expected:
        return _expected[key]
    xp, pad = _padded(disc)
    rs = ranges(disc)
    w = 2 * disc.radius + 1
    v1, v2, s450 = (np.zeros((len(rs), w), np.uint32) for _ in range(3))
    for t, (start, n, lo, hi, flags) in enumerate(rs):
        if hi >= lo and ("v1" in kinds or "v2" in kinds):
            a, b = _brute(xp, pad + start, lo, hi, disc.radius)
            v1[t], v2[t] = a, a + b  # uint32: wraps
        if not flags & TRACK_NO_S450 and "s450" in kinds:
            s450[t] = _brute(xp, pad + start + S450_AT, 1, SECTOR, disc.radius)[0]
    for a in (v1, v2, s450):
        a.setflags(write=False)
    _expected[key] = Sums(v1, v2, s450, [r[4] for r in rs])
    return _expected[key]


def expected_prefix(disc):
    """v1 and s450 from prefix sums, mod 2^32: with P0[i] = sum of x(j) and P1[i] = sum of j x(j) over j < i,
    v1 = (P1[b + 1] - P1[a]) - (s + o - 1) (P0[b + 1] - P0[a]), a = s + o + lo - 1, b = s + o + hi - 1."""
    xp, pad = _padded(disc)
    j = np.maximum(np.arange(len(xp), dtype=np.int64) - pad, 0).astype(np.uint64)  # (x is zero where j < 0)
    P0 = np.concatenate([np.zeros(1, np.uint64), np.cumsum(xp, dtype=np.uint64)])
    P1 = np.concatenate([np.zeros(1, np.uint64), np.cumsum(xp * j, dtype=np.uint64)])  # wraps mod 2^64: a multiple of 2^32
    o = np.arange(-disc.radius, disc.radius + 1, dtype=np.int64)

    def linear(s, lo, hi):
        a, b = s + o + lo - 1 + pad, s + o + hi - 1 + pad  # indices into the padded arrays
        d1 = (P1[b + 1] - P1[a]) & np.uint64(MASK)
        d0 = (P0[b + 1] - P0[a]) & np.uint64(MASK)
        base = ((s + o - 1) % (1 << 32)).astype(np.uint64)  # s + o - 1 mod 2^32
        return ((d1 - base * d0) & np.uint64(MASK)).astype(np.uint32)

    rs = ranges(disc)
    v1, s450 = (np.zeros((len(rs), len(o)), np.uint32) for _ in range(2))
    for t, (start, n, lo, hi, flags) in enumerate(rs):
        if hi >= lo:
            v1[t] = linear(start, lo, hi)
        if not flags & TRACK_NO_S450:
            s450[t] = linear(start + S450_AT, 1, SECTOR)
    return v1, s450


def v2_bigint(disc, t, o):
    x = [int(v) for v in words(disc)]
    start, n, lo, hi, _ = ranges(disc)[t]
    total = 0
    for m in range(lo, hi + 1):
        j = start + o + m - 1
        p = m * (x[j] if 0 <= j < len(x) else 0)
        total += (p & MASK) + (p >> 32)
    return total & MASK


Ids = namedtuple("Ids", "id1 id2 cddb")


def expected_ids(tracks, first=True, last=True, lba0=0):
    """The ids in plain Python; zeros where the disc has none (a partial disc, a track that is no whole number of sectors)."""
    if not (first and last) or any(n % SECTOR for n in tracks):
        return Ids(0, 0, 0)
    lbas, lba = [], lba0
    for n in tracks:
        lbas.append(lba)
        lba += n // SECTOR
    leadout, T = lba, len(tracks)
    digits = sum(sum(int(c) for c in str((v + 150) // 75)) for v in lbas)
    return Ids((sum(lbas) + leadout) & MASK, (sum(max(v, 1) * (t + 1) for t, v in enumerate(lbas)) + leadout * (T + 1)) & MASK,
               (((digits % 255) << 24) | (((leadout + 150) // 75 - (lba0 + 150) // 75) << 8) | T) & MASK)


# ---- discs --------------------------------------------------------------------------------------------------------------
def noise(frames, seed):
    g = np.random.default_rng(seed)
    return (g.integers(-32768, 32768, frames, dtype=np.int64).astype(np.int32), g.integers(-32768, 32768, frames, dtype=np.int64).astype(np.int32))


def constant(frames, value):
    return (np.full(frames, value, np.int32), np.full(frames, value, np.int32))


def split(pcm, lengths):
    """One source cut into sources of the given lengths."""
    left, right = pcm
    assert sum(lengths) == len(left)
    out, at = [], 0
    for n in lengths:
        out.append((left[at:at + n], right[at:at + n]))
        at += n
    return out


THREE = (7000, 6500, 9001)
EDGE_LENGTHS = (1, 2939, 2940, 2941, 5879, 5880, 5881)
TILE_LENGTHS = (4095, 4096, 4097, 8192, 8193)  # a middle track's multipliers 1 .. n on either side of the kernel's tile of 4096
SEAMS = (5001, 99, 121, 6000, 5280)           # five sources, two shorter than the radius 300 next to each other
SEAM_TRACKS = (8000, 8501)
BIG = 266000                                   # the smallest order of track with an s450: >= 451 * 588 = 265188

_corpus = None


def corpus():
    """Frozen seeds, every disc small but `big`.  The three-track disc of noise in one source at every radius (2 radius + 1
    on both sides of every split the plan has: 1, 4, 64, 128, 256 offsets per tile, two and 23 offset tiles); all four flag
    combinations (a partial disc reads zeros in front of frame 0 and behind the last); one source per track; five sources
    under two tracks with no boundary in common; tracks of 1 .. 5881 frames as first, last and only track; a middle track
    around the multiplier tile; words 0xFFFFFFFF and 0x80008000 throughout, zeros; one track of 266000 frames with an s450."""
    global _corpus
    if _corpus is not None:
        return _corpus
    discs, seed = [], 4100
    total = sum(THREE)
    for radius in RADII:
        seed += 1
        discs.append(Disc("three|r%d" % radius, [noise(total, seed)], THREE, radius, True, True))
    for first in (False, True):
        for last in (False, True):
            seed += 1
            discs.append(Disc("flags|%d%d" % (first, last), [noise(total, seed)], THREE, 300, first, last))
    discs.append(Disc("per-track", split(noise(total, 4201), THREE), None, 128, True, True))
    discs.append(Disc("sectors", split(noise(588 * 37, 4202), (588 * 12, 588 * 10, 588 * 15)), None, 1, True, True, 32))
    discs.append(Disc("seams", split(noise(sum(SEAMS), 4203), SEAMS), SEAM_TRACKS, 300, True, True))
    discs.append(Disc("seams|partial", split(noise(sum(SEAMS), 4204), SEAMS), SEAM_TRACKS, 32, False, False))
    for n in EDGE_LENGTHS:
        seed += 1
        discs.append(Disc("edge|first%d" % n, [noise(n + 6500 + 7000, seed)], (n, 6500, 7000), 1, True, True))
        discs.append(Disc("edge|last%d" % n, [noise(n + 6500 + 7000, seed + 50)], (7000, 6500, n), 32, True, True))
        discs.append(Disc("edge|only%d" % n, [noise(n, seed + 100)], (n,), 1 if n > 1 else 0, True, True))
    for n in TILE_LENGTHS:
        seed += 1
        discs.append(Disc("tile|%d" % n, [noise(3000 + n + 3000, seed + 200)], (3000, n, 3000), 31, False, False))
    discs.append(Disc("ones", [constant(total, -1)], THREE, 128, True, True))
    discs.append(Disc("lowest", [constant(total, -32768)], THREE, 128, True, False))
    discs.append(Disc("zeros", [constant(total, 0)], THREE, 31, True, True))
    discs.append(Disc("big|r2939", [noise(BIG, 4301)], (BIG,), 2939, True, True))
    discs.append(Disc("big|r8", [noise(BIG, 4301)], (BIG,), 8, True, True))
    assert len({d.name for d in discs}) == len(discs)
    _corpus = discs
    return _corpus


def small_corpus():
    return [d for d in corpus() if not d.name.startswith("big|")]


def disc_expected(disc):
    """What a disc's sums are held to: the definition restated, but for big|r2939, whose 1.6e9 pairs are held by the prefix
    sums (v1, s450; v2 by big|r8 and by Python integers at a handful of offsets)."""
    if disc.name == "big|r2939":
        v1, s450 = expected_prefix(disc)
        return Sums(v1, None, s450, [r[4] for r in ranges(disc)])
    return expected(disc)


# ---- a disc's answer, whoever made it -------------------------------------------------------------------------------------
def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def check(disc, got, what=""):
    """One disc of the twin (or of the device, as a TwinDisc) against the restatements, the flags and the ids."""
    want = disc_expected(disc)
    tf = track_frames(disc)
    assert got.code == 0, (disc.name, what, got.text)
    assert same(got.v1, want.v1) and same(got.s450, want.s450), (disc.name, what)
    if want.v2 is not None:
        assert same(got.v2, want.v2), (disc.name, what)
    assert [int(f) for f in got.tracks["flags"]] == want.flags and [int(n) for n in got.tracks["frames"]] == tf, (disc.name, what)
    assert [int(s) for s in got.tracks["start"]] == [sum(tf[:t]) for t in range(len(tf))]
    r = disc.radius
    assert (got.tracks["v1"] == got.v1[:, r]).all() and (got.tracks["v2"] == got.v2[:, r]).all() and (got.tracks["s450"] == got.s450[:, r]).all()
    ids = expected_ids(tf, disc.first, disc.last, disc.lba0)
    res = got.result
    assert (int(res["id1"]), int(res["id2"]), int(res["cddb"])) == tuple(ids), disc.name
    assert int(res["flags"]) == flags_of(disc) | (0 if any(ids) else NO_IDS)
    assert (int(res["frames"]), int(res["tracks"]), int(res["radius"])) == (sum(tf), len(tf), r)


# ---- the twin ---------------------------------------------------------------------------------------------------------
_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(twinbuild.shared_lib("sim_accuraterip", [SRC]))
        _lib.sim_ar_run.restype = C.c_int64
        _lib.sim_ar_tiles.restype = C.c_int64
        _lib.sim_ar_lanes.restype = C.c_uint32
        _lib.sim_ar_tile_mults.restype = C.c_uint32
    return _lib


def sanitized_exe():
    """The sanitized program's path, or (None, why) where the sanitizer runtime is missing."""
    return twinbuild.sanitized_exe("sim_accuraterip_san", [SRC], ["-DSIM_ACCURATERIP_MAIN"])


def _head(form, discs):
    return struct.pack("<BI", form, len(discs))


def _disc_head(d):
    tf = list(d.tracks) if d.tracks is not None else []
    return struct.pack("<IIIII", len(d.sources), len(tf), flags_of(d), d.radius, d.lba0) + struct.pack("<%dQ" % len(tf), *tf)


def source_case(discs, layout=P32, offset=0, bad=None) -> bytes:
    """Discs as one source job, every source in `layout` at base offset `offset`.  bad = (disc, source, frame, channel, raw
    32-bit word): that element of a 4-byte layout is the raw word instead."""
    out = [_head(1, discs)]
    for k, d in enumerate(discs):
        out.append(_disc_head(d))
        for i, (l, r) in enumerate(d.sources):
            bf, bc, bw = bad[2:] if bad and bad[:2] == (k, i) else (NONE, 0, 0)
            out.append(struct.pack("<IIQQII", layout, offset, len(l), bf, bc, bw))
            out.append(np.asarray(l, "<i4").tobytes() + np.asarray(r, "<i4").tobytes())
    return b"".join(out)


def stream_case(discs, lacs) -> bytes:
    """Discs as one stream job; lacs[k]: the streams of disc k, one per source."""
    out = [_head(0, discs)]
    for d, mine in zip(discs, lacs):
        out.append(_disc_head(d._replace(sources=mine)))
        for x in mine:
            out.append(struct.pack("<Q", len(x)) + x)
    return b"".join(out)


TwinDisc = namedtuple("TwinDisc", "code text result tracks v1 v2 s450")
_vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731


def _count(case):
    return struct.unpack_from("<I", case, 1)[0]


def run(case: bytes, sums_cap=None):
    """A case on the plain twin -> [TwinDisc] (v1 / v2 / s450: (tracks, 2 radius + 1) uint32, None for a disc without sums)."""
    n = _count(case)
    cap = sums_cap or max(1 << 16, len(case))  # (3 sums per track and offset; a case carries 8 bytes per frame)
    rec, results = np.zeros(4 * n, np.uint64), np.zeros(n, RESULT_T)
    sums, tracks = np.zeros(cap, np.uint32), np.zeros(99 * n, TRACK_T)
    msg = C.create_string_buffer(1 << 16)
    got = lib().sim_ar_run(case, C.c_uint64(len(case)), _vp(rec), _vp(results), _vp(sums), C.c_uint64(cap), _vp(tracks), C.c_uint64(len(tracks)),
                           msg, C.c_uint32(len(msg)))
    if got < 0 and sums_cap is None:
        return run(case, 3 * 99 * 5879 * max(1, n))
    assert got >= 0, "the twin could not run the case"
    texts = msg.value.decode().split("\n")
    out = []
    for k in range(n):
        code, nt, at, tr = (int(v) for v in rec[4 * k:4 * k + 4])
        if code:
            out.append(TwinDisc(code, texts[k], results[k].copy(), None, None, None, None))
            continue
        w = 2 * int(results[k]["radius"]) + 1
        s = sums[at:at + 3 * w * nt].reshape(nt, 3, w).copy()
        out.append(TwinDisc(0, "", results[k].copy(), tracks[tr:tr + nt].copy(), s[:, 0], s[:, 1], s[:, 2]))
    return out


def twin_ids(tracks, first=True, last=True, lba0=0):
    out = np.zeros(3, np.uint32)
    tf = np.array(tracks, np.uint64)
    has = lib().sim_ar_ids(_vp(tf), C.c_uint32(len(tf)), C.c_uint32((FIRST if first else 0) | (LAST if last else 0)), C.c_uint32(lba0), _vp(out))
    return bool(has), Ids(*(int(v) for v in out))


def twin_tiles(tracks, first, last, radius):
    tf = np.array(tracks, np.uint64)
    return int(lib().sim_ar_tiles(_vp(tf), C.c_uint32(len(tf)), C.c_uint32((FIRST if first else 0) | (LAST if last else 0)), C.c_uint32(radius)))


# ---- the sanitized program ----------------------------------------------------------------------------------------------
def line(case: bytes, index: int) -> str:
    """The plain build's line for a case (what the sanitized program must print for it)."""
    buf = C.create_string_buffer(1 << 20)
    rc = lib().sim_ar_line(case, C.c_uint64(len(case)), C.c_uint32(index), buf, C.c_uint32(len(buf)))
    assert rc == 0
    return buf.value.decode()


def run_sanitized(cases, exe=None, workers=8):
    """Every case through the sanitized program, split over a few processes: (lines, returncode, stderr)."""
    if exe is None:
        exe, why = sanitized_exe()
        assert exe, why
    return twinbuild.run_cases(exe, cases, ENV, workers=workers, prefix="lac_ar_")


def cleared(key, cases):
    """cases, once the sanitized twin has shown in this run that a rip-checksum job over each stays inside buffers of exactly
    the plan's capacities and answers as the plain build does.  Fails, never skips, where that cannot be shown."""
    def make():
        return list(cases), lambda c, i: line(c, i).split(" ", 1)[1], None, list(cases)

    return twinbuild.cleared("rip checksum", key, sys.modules[__name__], make)
