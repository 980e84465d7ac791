"""The decoder's CPU twin (tests/native/sim_decode.cpp over csrc/decode_core.h): built here, called through ctypes (the plain
-O2 build) or run as a program over a corpus file (the build with AddressSanitizer + UBSan, which needs its runtime
first in the process and so cannot be loaded into Python).

  decode(lac, never_lean, cols, gathered, pad) -> Result(status, ms, left, right, over)
  digest(lac, index, settings, pad)            -> the line the sanitized program prints for that stream
  run_sanitized(streams, settings, pad)        -> (lines, returncode, stderr) of the sanitized program over `streams`

A setting is never_lean | (cols == 64) << 1 | gathered << 2; ALL_SETTINGS runs the eight of them, HALF_SETTINGS four
per stream (0 3 5 6 or 1 2 4 7 by the stream's index: every switch both ways, every pair of switches all four ways).  The digest line holds
the statuses and a hash of the PCM of the first setting, the largest overshoot of any, and whether all agreed."""
from __future__ import annotations

import ctypes as C
import os
import struct
from collections import namedtuple

import numpy as np

import twinbuild

SRC = os.path.join(twinbuild.NATIVE, "sim_decode.cpp")
DEFAULT_PAD = 0xFFFFFFFF  # "what the device path appends": the twin takes kDecodeTailPad from lacx_types.h itself
ALL_SETTINGS = 0xFF
HALF_SETTINGS = 0   # four settings per stream that vary every switch and every pair of switches (see sim_digest)
ENV = dict(ASAN_OPTIONS="detect_leaks=0:verify_asan_link_order=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")

Result = namedtuple("Result", "status ms left right over")
Line = namedtuple("Line", "index over pcm_hash same status")

_lib = None


def lib():
    """The plain build."""
    global _lib
    if _lib is None:
        _lib = C.CDLL(twinbuild.shared_lib("sim_decode", [SRC]))
        _lib.sim_hash.restype = C.c_uint64
        _lib.sim_tail_pad.restype = C.c_uint32
    return _lib


def sanitized_exe(extra=(), name="sim_decode_san"):
    """The sanitized program's path, or (None, why) where the sanitizer runtime is missing."""
    return twinbuild.sanitized_exe(name, [SRC], ["-DSIM_DECODE_MAIN"], extra)


def tail_pad() -> int:
    """kDecodeTailPad as compiled into the twin (and into the product: the same header)."""
    return lib().sim_tail_pad()


def _shape(lac):
    nb = struct.unpack(">I", lac[10:14])[0]
    entry = 8 if lac[2] == 3 else 4
    frames = [struct.unpack(">I", lac[14 + entry * b:18 + entry * b])[0] for b in range(nb)]
    return nb, frames


def decode(lac: bytes, never_lean=False, cols=1, gathered=0, pad=DEFAULT_PAD) -> Result:
    nb, frames = _shape(lac)
    total = sum(frames)
    status = np.zeros(nb, np.uint32)
    ms = np.zeros(nb, np.uint8)
    left = np.zeros(total, np.int32)
    right = np.zeros(total if lac[3] == 2 else 0, np.int32)
    over = C.c_uint32()
    rc = lib().sim_decode(lac, C.c_uint64(len(lac)), int(never_lean), int(cols), C.c_uint32(gathered), C.c_uint32(pad),
                          status.ctypes.data_as(C.c_void_p), ms.ctypes.data_as(C.c_void_p), left.ctypes.data_as(C.c_void_p),
                          right.ctypes.data_as(C.c_void_p), C.byref(over))
    assert rc == 0, "the twin's container walk refused a stream"
    return Result(status, ms, left, right if lac[3] == 2 else None, over.value)


def pcm_hash(lac: bytes, res: Result) -> int:
    """The hash the digest line carries: the PCM, MS flag and length of every block with status 0."""
    _, frames = _shape(lac)
    h, f0 = 0, 0
    for b, n in enumerate(frames):
        if res.status[b] == 0:
            h = lib().sim_hash(res.left[f0:f0 + n].ctypes.data_as(C.c_void_p), C.c_uint64(n), C.c_uint64(h))
            if res.right is not None:
                h = lib().sim_hash(res.right[f0:f0 + n].ctypes.data_as(C.c_void_p), C.c_uint64(n), C.c_uint64(h))
            h = lib().sim_hash(np.array([n], np.int32).ctypes.data_as(C.c_void_p), C.c_uint64(1), C.c_uint64(h ^ int(res.ms[b])))
        f0 += n
    return h


def parse_line(text: str) -> Line:
    index, over, h, same, st = text.split()
    return Line(int(index), int(over), int(h, 16), int(same), [int(s) for s in st.split(",")])


def digest(lac: bytes, index: int, settings=ALL_SETTINGS, pad=DEFAULT_PAD) -> Line:
    """The plain build's digest line (what the sanitized program must print for the same stream)."""
    buf = C.create_string_buffer(1 << 20)
    rc = lib().sim_digest(lac, C.c_uint64(len(lac)), C.c_uint32(index), C.c_uint32(settings), C.c_uint32(pad), buf, C.c_uint32(len(buf)))
    assert rc == 0
    return parse_line(buf.value.decode())


def run_sanitized(streams, settings=ALL_SETTINGS, pad=DEFAULT_PAD, exe=None, workers=8):
    """Every stream through the sanitized program, split over a few processes.  Returns (lines, returncode, stderr):
    lines[i] is None where a process stopped before stream i (a sanitizer report: returncode != 0, the report in stderr)."""
    if exe is None:
        exe, why = sanitized_exe()
        assert exe, why
    # slices of about equal bytes, so that the long streams do not land in one process
    lines, rc, err = twinbuild.run_cases(exe, streams, ENV, lambda path, a, n: [path, str(a), str(n), str(settings), str(pad)],
                                         workers=workers, slices=True, prefix="lac_corpus_")
    return [parse_line(t) if t else None for t in lines], rc, err


# ---- batches: sim_decode_batch / sim_batch_digest / sim_plan_dump (jobs planned by csrc/decode_plan.h) ----
BatchItem = namedtuple("BatchItem", "refused status ms left right start frames blk_first blocks")
FORMS = {"wav": 0, "device": 1, "host": 2, "verify": 3}  # DecodeForm
WHOLE, I32, F32 = -1, 0, 1                                 # sample type: whole streams, or windows of that type


def _job(lacs, windows):
    n = len(lacs)
    ptrs = (C.c_char_p * n)(*lacs)
    sizes = (C.c_uint64 * n)(*[len(x) for x in lacs])
    start = (C.c_uint64 * n)(*[w[0] for w in windows]) if windows else None
    frames = (C.c_uint64 * n)(*[w[1] for w in windows]) if windows else None
    return n, ptrs, sizes, start, frames


def decode_batch(lacs, windows=None, pad_waves=False, never_lean=False, cols=1):
    """n streams as one job (windows: [(start, frames)] per stream, or whole streams) -> ([BatchItem], over).  An item's
    left / right are the scratch PCM of the blocks it covers (blocks from blk_first on); a window is
    left[start:start + frames] of that."""
    n, ptrs, sizes, start, frames = _job(lacs, windows)
    shapes = [_shape(x) if len(x) >= 14 and x[2] in (2, 3) else (0, []) for x in lacs]
    nblocks = sum(min(nb, len(fr)) for nb, fr in shapes) + 1
    npcm = sum((sum(fr) + 3) // 4 * 4 for _, fr in shapes) + 4
    rec = np.zeros(8 * n, np.uint64)
    status, ms = np.zeros(nblocks, np.uint32), np.zeros(nblocks, np.uint8)
    left, right = np.zeros(npcm, np.int32), np.zeros(npcm, np.int32)
    over = C.c_uint32()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    rc = lib().sim_decode_batch(ptrs, sizes, C.c_uint32(n), start, frames, int(pad_waves), int(never_lean), int(cols), vp(rec),
                                vp(status), vp(ms), vp(left), vp(right), C.byref(over))
    assert rc == 0
    items = []
    for i, lac in enumerate(lacs):
        refused, at, got, w0, wn, b0, nb, g0 = (int(v) for v in rec[8 * i:8 * i + 8])
        if refused:
            items.append(BatchItem(True, None, None, None, None, 0, 0, 0, 0))
            continue
        items.append(BatchItem(False, status[g0:g0 + nb], ms[g0:g0 + nb], left[at:at + got],
                               right[at:at + got] if lac[3] == 2 else None, w0, wn, b0, nb))
    return items, over.value


def batch_case(lacs, windows=None, pad_waves=False, never_lean=False, cols=1) -> bytes:
    """The case blob sim_batch_digest reads."""
    flags = int(pad_waves) | (2 if windows else 0) | (4 if never_lean else 0) | (8 if cols == 64 else 0)
    out = struct.pack("<II", len(lacs), flags)
    for i, lac in enumerate(lacs):
        s, f = windows[i] if windows else (0, 0)
        out += struct.pack("<QQQ", s, f, len(lac)) + lac
    return out


def batch_digest(case: bytes, index: int) -> str:
    """The plain build's line for a batch case (what the sanitized program must print for it)."""
    buf = C.create_string_buffer(1 << 20)
    rc = lib().sim_batch_digest(case, C.c_uint64(len(case)), C.c_uint32(index), buf, C.c_uint32(len(buf)))
    assert rc == 0
    return buf.value.decode()


def run_sanitized_batches(cases, exe=None):
    """Every batch case through the sanitized program (its `batch` mode): (lines, returncode, stderr)."""
    if exe is None:
        exe, why = sanitized_exe()
        assert exe, why
    return twinbuild.run_cases(exe, cases, ENV, lambda path, a, n: ["batch", path], prefix="lac_batches_")


ITEM_DTYPE = np.dtype([("left", "<u8"), ("right", "<u8"), ("wav", "<u8"), ("frame0", "<u8"), ("frames", "<u8"), ("pay_off", "<u8"),
                       ("block0", "<u4"), ("blocks", "<u4"), ("pay_bits", "<u4"), ("channels", "u1"), ("stereo_mode", "u1"),
                       ("bit_depth", "u1"), ("version", "u1")])
WINDOW_DTYPE = np.dtype([("left", "<u8"), ("right", "<u8"), ("start", "<u8"), ("frames", "<u8")])
SOURCE_DTYPE = np.dtype([("data0", "<u8"), ("data1", "<u8"), ("layout", "<u4"), ("pad", "<u4")])
WORDS_DTYPE = np.dtype([("count", "<u8"), ("key", "<u8"), ("decoded", "<i4"), ("source", "<i4"), ("block", "<u4"), ("pad", "<u4")])
HEAD = ("m total_blocks total_frames total_pay total_units pcm_total image_total src_at host_src_bytes lanes nv2 "
        "o_items o_byte o_frame o_unit o_bitem o_lane o_v2 o_win o_res o_size need_payload need_blocks need_pcm need_image "
        "need_stage need_tables sizeof_item sizeof_window sizeof_source sizeof_words tail_pad").split()
ITEM = "src blk_first pay_src pay_bytes head pcm_at image_at image_size frames win_start win_frames blocks".split()


def base(k, i=0):
    """The made-up address sim_plan_dump gives buffer k (0 payload, 1 left, 2 right, 3 image, 4 / 5 the caller's left /
    right, 6 / 7 the sources) of input i."""
    return ((k + 1) << 40) + (i << 32)


def plan_dump(lacs, form, windows=None, sample_type=WHOLE, pad_waves=False, host_src_bytes=0):
    """The product's plan of a job and its filled tables: a dict of the HEAD fields, `items` (dicts of ITEM), `rc` and
    `msg` per input, and the tables: item, byte_off, frame_off, unit_off, blk_item, lane_blk, v2_items, window / source /
    words where the form has them, and `raw`."""
    n, ptrs, sizes, start, frames = _job(lacs, windows)
    L = lib()
    L.sim_plan_dump.restype = C.c_int64
    head = np.zeros(len(HEAD), np.uint64)
    item = np.zeros(len(ITEM) * n, np.uint64)
    rc = np.zeros(n, np.int32)
    msg = C.create_string_buffer(1 << 16)
    cap = 1 << 22
    raw = np.zeros(cap, np.uint8)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    size = L.sim_plan_dump(ptrs, sizes, C.c_uint32(n), start, frames, FORMS[form], int(sample_type), int(pad_waves),
                           C.c_uint64(host_src_bytes), vp(head), vp(item), vp(rc), msg, C.c_uint32(len(msg)), vp(raw), C.c_uint64(cap))
    assert size >= 0, msg.value
    p = {k: int(v) for k, v in zip(HEAD, head)}
    m, T = p["m"], p["total_blocks"]
    p["items"] = [dict(zip(ITEM, (int(v) for v in item[len(ITEM) * j:len(ITEM) * (j + 1)]))) for j in range(m)]
    p["rc"], p["msg"] = rc.tolist(), msg.value.decode().split("\n")
    p["raw"] = raw = raw[:size]
    tab = lambda off, dtype, count: np.frombuffer(raw, dtype=dtype, count=count, offset=off)  # noqa: E731
    p["item"] = tab(p["o_items"], ITEM_DTYPE, m)
    p["byte_off"], p["frame_off"] = tab(p["o_byte"], "<u8", T + 1), tab(p["o_frame"], "<u8", T + 1)
    p["unit_off"], p["blk_item"] = tab(p["o_unit"], "<u8", m + 1), tab(p["o_bitem"], "<u4", T)
    p["lane_blk"], p["v2_items"] = tab(p["o_lane"], "<u4", p["lanes"]), tab(p["o_v2"], "<u4", p["nv2"])
    if sample_type != WHOLE:
        p["window"] = tab(p["o_win"], WINDOW_DTYPE, m)
    if form == "verify":
        p["source"], p["words"] = tab(p["o_win"], SOURCE_DTYPE, m), tab(p["o_res"], WORDS_DTYPE, m)
    return p
