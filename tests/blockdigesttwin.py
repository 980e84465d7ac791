"""Block digests and manifests off the device: where their expectations come from, and their CPU twin.

  data_bytes(left, right, depth)   the bytes samples have in a WAV data chunk, built with numpy
  expected_rows(exp, lac)          [(frames, crc32, lost)] per block from salvagetwin.expected: zlib.crc32 over data_bytes
  manifest_of(...)/manifest_for(exp, lac)   the manifest format restated with struct -- never the code under test
  run(lacs, manifests, form, ...)  the CPU twin (tests/native/sim_blockdigest.cpp: csrc/decode_plan.h, blockdigest_core.h
                                   summed as k_digest_blocks sums, the judge, the salvage pass), plain build through ctypes
  source_rows(...)                 the source form at unit level: one item in a layout at a base offset, on a grid
  case / source_case / line / run_sanitized   the same through the build with AddressSanitizer + UBSan, a program of its
                                   own (a sanitizer is never loaded into Python)
  cleared(key, lacs, manifests)    streams that may go to a device: the sanitized twin has passed them in this run"""
from __future__ import annotations

import ctypes as C
import struct
import sys
import zlib
from collections import namedtuple

import numpy as np

import dectwin
import lacmutate
import salvagetwin
import twinbuild

SRC = twinbuild.NATIVE + "/sim_blockdigest.cpp"
DIGEST = 11  # LACX_BLOCK_DIGEST
FORM_BLOCKS, FORM_WAV, FORM_DEVICE = 0, 1, 2
LAYOUTS = {"planar_i32": 0, "inter_i16": 1, "inter_i24": 2, "planar_i16": 16, "planar_f32": 17, "inter_f32": 18}
CLEAN = (1 << 64) - 1
ENV = dict(ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")

# code: the plan's code for the item (0: it went to the device); rows: [(frames, crc32, code)]
Item = namedtuple("Item", "code message blocks bad_blocks frames lost_frames first_bad flags rows image left right")

_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(twinbuild.shared_lib("sim_blockdigest", [SRC]))
        _lib.sim_blockdigest.restype = C.c_int64
        _lib.sim_blockdigest_source.restype = C.c_int64
        _lib.sim_manifest_build.restype = C.c_int64
    return _lib


def sanitized_exe():
    """The sanitized program's path, or (None, why) where the sanitizer runtime is missing."""
    return twinbuild.sanitized_exe("sim_blockdigest_san", [SRC], ["-DSIM_BLOCKDIGEST_MAIN"])


# ---- expectations -----------------------------------------------------------------------------------------------------
def data_bytes(left, right, depth) -> bytes:
    """Interleaved little-endian, depth / 8 bytes per sample: the WAV data chunk of these samples."""
    a = np.asarray(left, np.int32) if right is None else np.stack([np.asarray(left, np.int32), np.asarray(right, np.int32)], 1).ravel()
    if depth == 16:
        return a.astype("<i2").tobytes()
    return np.ascontiguousarray(a.astype("<i4").view(np.uint8).reshape(-1, 4)[:, :3]).tobytes()


def block_crcs(left, right, depth, frames):
    """zlib.crc32 of every block's bytes; frames: the blocks' frame counts."""
    out, at = [], 0
    for n in frames:
        out.append(zlib.crc32(data_bytes(left[at:at + n], None if right is None else right[at:at + n], depth)))
        at += n
    return out


def expected_rows(exp, lac):
    """[(frames, crc32, lost)] of what a salvage decode of `lac` gives (salvagetwin.expected): a lost block has crc32 0."""
    frames = [n for n, _ in lacmutate.table(lac)[1]]
    crcs = block_crcs(exp.left, exp.right, lac[8], frames)
    return [(n, 0 if lost else c, lost) for n, c, lost in zip(frames, crcs, exp.lost)]


def manifest_of(channels, depth, rate, frames, rows) -> bytes:
    """The manifest format restated: rows = [(frames, crc32)]; data_crc32 is zlib's combination of the rows."""
    align = channels * (depth // 8)
    head = b"LACM" + struct.pack(">BBBBIQI", 1, channels, depth, 0, rate, frames, len(rows))
    whole = 0
    for k, (n, c) in enumerate(rows):
        whole = c if k == 0 else _combine(whole, c, n * align)
    body = head + struct.pack(">I", whole) + b"".join(struct.pack(">II", n, c) for n, c in rows)
    return body + struct.pack(">I", zlib.crc32(body))


def _combine(a, b, len_b):
    """crc32(A + B) from crc32(A), crc32(B), len(B): crc32(A + zeros(len B)) ^ crc32(zeros(len B)) ^ crc32(B), in 1 MiB steps."""
    zeros, left = 0, len_b
    while left:
        step = min(left, 1 << 20)
        chunk = bytes(step)
        a, zeros, left = zlib.crc32(chunk, a), zlib.crc32(chunk, zeros), left - step
    return a ^ zeros ^ b


def manifest_for(exp, lac) -> bytes:
    """The manifest of a stream every block of which decodes, from its expectation."""
    rows = expected_rows(exp, lac)
    assert not any(lost for _, _, lost in rows)
    return manifest_of(lac[3], lac[8], salvagetwin.rate(lac), exp.frames, [(n, c) for n, c, _ in rows])


_base_rows = {}


def judged_expectation(exp, lac, base_exp, base):
    """A stream judged by the manifest of `base` (same block frames): (the expectation with every silently wrong block --
    one the oracle decodes without fault to bytes whose zlib CRC-32 differs from the base's row -- lost with code 11 and
    silent, those blocks, the number of blocks whose samples differ from the base's although the CRC-32 is the same)."""
    if base not in _base_rows:
        _base_rows[base] = expected_rows(base_exp, base)
    rows, base_rows = expected_rows(exp, lac), _base_rows[base]
    assert [n for n, _, _ in rows] == [n for n, _, _ in base_rows]  # the mutant keeps its base's frame counts
    edges = np.concatenate([[0], np.cumsum([n for n, _, _ in rows])])
    wrong, collisions = [], 0
    lost2, known2 = list(exp.lost), list(exp.known)
    left2, right2 = exp.left.copy(), None if exp.right is None else exp.right.copy()
    for b, ((n, c, lost), (_, bc, _)) in enumerate(zip(rows, base_rows)):
        if lost:
            continue
        a, e = edges[b], edges[b + 1]
        differs = not np.array_equal(exp.left[a:e], base_exp.left[a:e]) or (exp.right is not None and not np.array_equal(exp.right[a:e], base_exp.right[a:e]))
        collisions += differs and c == bc
        if c != bc:
            wrong.append(b)
            lost2[b], known2[b] = True, DIGEST
            left2[a:e] = 0
            if right2 is not None:
                right2[a:e] = 0
    return exp._replace(left=left2, right=right2, lost=lost2, known=known2), wrong, collisions


# ---- the twin ---------------------------------------------------------------------------------------------------------
def run(lacs, manifests=None, form=FORM_BLOCKS, cols=1, zero_status=False):
    """n streams as one job with block digests on the CPU twin -> ([Item], atomics)."""
    n = len(lacs)
    manifests = manifests or [None] * n
    ptrs = (C.c_char_p * n)(*lacs)
    sizes = (C.c_uint64 * n)(*[len(x) for x in lacs])
    mptrs = (C.c_char_p * n)(*manifests)
    msizes = (C.c_uint64 * n)(*[0 if m is None else len(m) for m in manifests])
    shapes = [dectwin._shape(x) if salvagetwin._head_ok(x) else (0, []) for x in lacs]
    nblocks = sum(nb for nb, _ in shapes) + 1
    npcm = sum(sum(fr) for _, fr in shapes) + 1
    nimage = sum((44 + sum(fr) * x[3] * (x[8] // 8) + 1 + 15) // 16 * 16 for x, (_, fr) in zip(lacs, shapes) if fr) + 16
    rec = np.zeros(8 * n, np.uint64)
    rows = np.zeros(3 * nblocks, np.uint32)
    image = np.zeros(nimage if form == FORM_WAV else 1, np.uint8)
    left = np.full(npcm if form == FORM_DEVICE else 1, salvagetwin.SENTINEL, np.int32)
    right = np.full(npcm if form == FORM_DEVICE else 1, salvagetwin.SENTINEL, np.int32)
    msg = C.create_string_buffer(1 << 16)
    atomics = C.c_uint64()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    got = lib().sim_blockdigest(ptrs, sizes, mptrs, msizes, C.c_uint32(n), int(form), int(cols), int(zero_status), vp(rec), vp(rows),
                                C.c_uint64(nblocks), vp(image), C.c_uint64(image.size), vp(left), vp(right), C.c_uint64(left.size), msg,
                                C.c_uint32(len(msg)), C.byref(atomics))
    assert got >= 0, "the twin could not run the job"
    msgs = msg.value.decode().split("\n")
    items, at_row = [], 0
    for i, lac in enumerate(lacs):
        code, nb, bad, frames, lostf, first, flags, at = (int(v) for v in rec[8 * i:8 * i + 8])
        if code:
            items.append(Item(code, msgs[i], 0, 0, 0, 0, 0, 0, None, None, None, None))
            continue
        r = [tuple(int(v) for v in rows[3 * (at_row + b):3 * (at_row + b) + 3]) for b in range(nb)]
        at_row += nb
        size = 44 + frames * lac[3] * (lac[8] // 8)
        size += size & 1
        items.append(Item(0, "", nb, bad, frames, lostf, first, flags, r,
                          image[at:at + size].tobytes() if form == FORM_WAV else None,
                          left[at:at + frames].copy() if form == FORM_DEVICE else None,
                          right[at:at + frames].copy() if form == FORM_DEVICE and lac[3] == 2 else None))
    return items, atomics.value


def source_rows(layout, channels, depth, grid, offset, left, right=None):
    """The source form on the twin -> ([(frames, crc32, code)], key, atomics)."""
    frames = len(left)
    samples = np.concatenate([np.asarray(left, np.int32)] + ([np.asarray(right, np.int32)] if channels == 2 else []))
    cap = frames // grid + 2
    rows = np.zeros(3 * cap, np.uint32)
    key, atomics = C.c_uint64(), C.c_uint64()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    nb = lib().sim_blockdigest_source(C.c_uint32(layout), C.c_uint32(channels), C.c_uint32(depth), C.c_uint64(frames), C.c_uint32(grid),
                                      C.c_uint32(offset), vp(samples), vp(rows), C.c_uint64(cap), C.byref(key), C.byref(atomics))
    assert nb >= 0, "the twin could not run the source"
    return [tuple(int(v) for v in rows[3 * b:3 * b + 3]) for b in range(nb)], key.value, atomics.value


def twin_manifest_build(channels, depth, rate, frames, data_crc32, rows):
    """csrc/manifest.h's builder -> bytes, or the refusal's text."""
    flat = np.array([v for r in rows for v in r], np.uint32) if rows else np.zeros(3, np.uint32)
    out = np.zeros(32 + 8 * len(rows) + 8, np.uint8)
    msg = C.create_string_buffer(1 << 12)
    size = lib().sim_manifest_build(C.c_uint32(channels), C.c_uint32(depth), C.c_uint32(rate), C.c_uint64(frames), C.c_uint32(data_crc32),
                                    flat.ctypes.data_as(C.c_void_p), C.c_uint32(len(rows)), out.ctypes.data_as(C.c_void_p),
                                    C.c_uint64(out.size), msg, C.c_uint32(len(msg)))
    return out[:size].tobytes() if size >= 0 else msg.value.decode()


def twin_manifest_parse(m: bytes):
    """csrc/manifest.h's parser -> (code, message, info dict, [(frames, crc32, code)])."""
    cap = max(1, (len(m) - 32) // 8) if len(m) >= 32 else 1
    info, rows = np.zeros(6, np.uint64), np.zeros(3 * cap, np.uint32)
    msg = C.create_string_buffer(1 << 12)
    rc = lib().sim_manifest_parse(m, C.c_uint64(len(m)), info.ctypes.data_as(C.c_void_p), rows.ctypes.data_as(C.c_void_p), C.c_uint32(cap),
                                  msg, C.c_uint32(len(msg)))
    d = dict(zip("channels bit_depth sample_rate frames blocks data_crc32".split(), (int(v) for v in info)))
    return rc, msg.value.decode(), d, [tuple(int(v) for v in rows[3 * b:3 * b + 3]) for b in range(d["blocks"] if rc == 0 else 0)]


# ---- the sanitized program ----------------------------------------------------------------------------------------------
def case(lacs, manifests=None, form=FORM_BLOCKS, cols=1, zero_status=False) -> bytes:
    manifests = manifests or [None] * len(lacs)
    flags = int(form) | (4 if cols == 64 else 0) | (8 if zero_status else 0)
    body = struct.pack("<II", len(lacs), flags)
    for x, m in zip(lacs, manifests):
        body += struct.pack("<Q", len(x)) + x + (struct.pack("<Q", CLEAN) if m is None else struct.pack("<Q", len(m)) + m)
    return b"\0" + body


def source_case(layout, channels, depth, grid, offset, left, right=None) -> bytes:
    samples = np.concatenate([np.asarray(left, np.int32)] + ([np.asarray(right, np.int32)] if channels == 2 else []))
    return b"\1" + struct.pack("<IIIIIQ", layout, channels, depth, grid, offset, len(left)) + samples.astype("<i4").tobytes()


def line(blob: bytes, index: int) -> str:
    """The plain build's line for a stream case (what the sanitized program must print for it)."""
    assert blob[0] == 0
    buf = C.create_string_buffer(1 << 22)
    rc = lib().sim_blockdigest_line(blob[1:], C.c_uint64(len(blob) - 1), C.c_uint32(index), buf, C.c_uint32(len(buf)))
    assert rc == 0
    return buf.value.decode()


def run_sanitized(cases, exe=None, workers=8):
    """Every case through the sanitized program, split over a few processes: (lines, returncode, stderr)."""
    if exe is None:
        exe, why = sanitized_exe()
        assert exe, why
    return twinbuild.run_cases(exe, cases, ENV, workers=workers, prefix="lac_blockdigest_")


BATCH = 64


def cleared(key, lacs, manifests):
    """(lacs, manifests), once the sanitized twin has shown in this run that a job with block digests over each of them
    stays inside buffers of exactly the plan's capacities -- all three forms, both status fills, 1 and 64 columns, in
    batches -- and answers as the plain build does.  Fails, never skips, where that cannot be shown."""
    def make():
        cases = []
        for at in range(0, len(lacs), BATCH):
            part, mans = lacs[at:at + BATCH], manifests[at:at + BATCH]
            k = at // BATCH
            cases.append(case(part, mans, FORM_BLOCKS, cols=64 if k & 1 else 1, zero_status=bool(k & 2)))
            cases.append(case(part, mans, FORM_WAV, cols=1 if k & 1 else 64, zero_status=bool(k & 1)))
            cases.append(case(part, mans, FORM_DEVICE, cols=64 if k & 2 else 1, zero_status=not (k & 1)))
        return cases, lambda c, i: line(c, i).split(" ", 1)[1], None, (list(lacs), list(manifests))

    return twinbuild.cleared("block digest", key, sys.modules[__name__], make)
