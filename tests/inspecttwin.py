"""The stream inspection off the device: its CPU twin (tests/native/sim_inspect.cpp: csrc/inspect_plan.h's job, the lanes
of csrc/inspect_core.h one after the other, csrc/inspect_rows.h's host side), built only through twinbuild.

  run(lacs, partitions, cols, gather_seed, pad_waves)  the plain build -> ([item_rc], [rows as lacinspect dicts, or None where refused],
                                                       [report dicts], over)
  codes(lacs, cols)                                    only the blocks' verdicts, for whole corpora
  case / line / run_sanitized                          the same through the build with AddressSanitizer + UBSan, a program
                                                       of its own (a sanitizer is never loaded into Python)
  cleared(key, lacs)                                   streams that may go to a device: the sanitized twin has passed them

The expectation for the rows is never the twin: it is tests/lacinspect.py."""
from __future__ import annotations

import ctypes as C
import struct
import sys

import numpy as np

import __graft_entry__ as ge
import lacinspect
import twinbuild

lacx = ge.load_pkg().lacx  # the ctypes records (no library is loaded for them)

SRC = twinbuild.NATIVE + "/sim_inspect.cpp"
ENV = dict(ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
BATCH = 64

_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(twinbuild.shared_lib("sim_inspect", [SRC]))
    return _lib


def sanitized_exe():
    return twinbuild.sanitized_exe("sim_inspect_san", [SRC], ["-DSIM_INSPECT_MAIN"])


def _blocks(lac):
    return struct.unpack(">I", lac[10:14])[0] if len(lac) >= 14 else 0


def run(lacs, partitions=False, cols=1, gather_seed=0, pad_waves=False):
    n = len(lacs)
    bufs = [C.create_string_buffer(bytes(x), max(1, len(x))) for x in lacs]
    ptrs = (C.c_void_p * max(1, n))(*[C.addressof(b) for b in bufs])
    sizes = (C.c_uint64 * max(1, n))(*[len(x) for x in lacs])
    cap = sum(min(_blocks(x), 1 << 20) for x in lacs)
    rc = (C.c_int * max(1, n))()
    block0 = (C.c_uint32 * max(1, n))()
    rows = (lacx.BlockInfo * max(1, cap))()
    reports = (lacx.StreamReport * max(1, n))()
    mk = (C.c_uint8 * (512 * cap if partitions else 1))()
    pb = (C.c_uint32 * (512 * cap if partitions else 1))()
    over = C.c_uint32()
    flags = (1 if partitions else 0) | (2 if pad_waves else 0)
    got = lib().sim_inspect(ptrs, sizes, C.c_uint32(n), C.c_uint32(flags), C.c_int(cols), C.c_uint32(gather_seed), rc, block0, rows,
                            C.c_uint64(cap), reports, mk, pb, C.byref(over))
    assert got == 0, "the twin could not run the job (%d)" % got
    out = []
    for i in range(n):
        if block0[i] == 0xFFFFFFFF:
            out.append(None)
            continue
        item = []
        for b in range(_blocks(lacs[i])):
            g = block0[i] + b
            d = lacinspect.from_ctypes(rows[g])
            if partitions:
                for c in range(2):
                    count = sum(d["ch"][c]["mode_parts"])
                    at = (g * 2 + c) * 256
                    assert not any(mk[at + count:at + 256]) and not any(pb[at + count:at + 256]), "entries behind the partitions"
                    d["ch"][c]["partitions"] = [(mk[at + p], pb[at + p]) for p in range(count)]
            item.append(d)
        out.append(item)
    return list(rc[:n]), out, [lacinspect.report_from_ctypes(reports[i]) for i in range(n)], over.value


def codes(lacs, cols=1):
    """Only the verdicts: per stream the list of its blocks' codes (None where refused) -- the whole-corpus form of run()."""
    n = len(lacs)
    bufs = [C.create_string_buffer(bytes(x), max(1, len(x))) for x in lacs]
    ptrs = (C.c_void_p * max(1, n))(*[C.addressof(b) for b in bufs])
    sizes = (C.c_uint64 * max(1, n))(*[len(x) for x in lacs])
    cap = sum(min(_blocks(x), 1 << 20) for x in lacs)
    rc, block0 = (C.c_int * max(1, n))(), (C.c_uint32 * max(1, n))()
    rows = np.zeros(max(1, cap) * 84, np.uint32)  # 336 bytes a row: frames, bytes, code, ...
    reports = (lacx.StreamReport * max(1, n))()
    over = C.c_uint32()
    got = lib().sim_inspect(ptrs, sizes, C.c_uint32(n), C.c_uint32(0), C.c_int(cols), C.c_uint32(0), rc, block0,
                            rows.ctypes.data_as(C.c_void_p), C.c_uint64(cap), reports, None, None, C.byref(over))
    assert got == 0, "the twin could not run the job (%d)" % got
    code = rows.reshape(-1, 84)[:, 2]
    return [None if block0[i] == 0xFFFFFFFF else code[block0[i]:block0[i] + _blocks(lacs[i])].tolist() for i in range(n)], over.value


def case(lacs, partitions=False, cols=1, gather_seed=0, pad_waves=False) -> bytes:
    body = struct.pack("<IIII", (1 if partitions else 0) | (2 if pad_waves else 0), cols, gather_seed, len(lacs))
    for x in lacs:
        body += struct.pack("<Q", len(x)) + bytes(x)
    return body


def line(blob: bytes) -> str:
    buf = C.create_string_buffer(1 << 16)
    rc = lib().sim_inspect_line(blob, C.c_uint64(len(blob)), buf, C.c_uint32(len(buf)))
    assert rc == 0
    return buf.value.decode()


def run_sanitized(cases, exe=None, workers=8):
    if exe is None:
        exe, why = sanitized_exe()
        assert exe, why
    return twinbuild.run_cases(exe, cases, ENV, workers=workers, prefix="lac_inspect_")


def cleared(key, lacs):
    """lacs, once the sanitized twin has shown in this run that an inspection job over them stays inside buffers of exactly
    the plan's capacities -- with and without partition detail, 1 and 64 columns, in batches -- and answers as the plain
    build does.  Fails, never skips, where that cannot be shown."""
    def make():
        cases = []
        for at in range(0, len(lacs), BATCH):
            part = lacs[at:at + BATCH]
            cases.append(case(part, partitions=False, cols=1))
            cases.append(case(part, partitions=True, cols=64))
        return cases, lambda c, i: line(c), None, list(lacs)

    return twinbuild.cleared("inspect", key, sys.modules[__name__], make)
