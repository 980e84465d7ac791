"""The verify form's CPU twin (tests/native/sim_verify.cpp over csrc/verify_core.h): built here, called through ctypes (the
plain -O2 build) or run as a program over a file of cases (the build with AddressSanitizer + UBSan, which needs its
runtime first in the process and so cannot be loaded into Python), and the numpy brute force both are compared with.

  Case(...)                     one item: block table, decoded PCM, source PCM, base offsets, groups of edits
  case.blob()                   the bytes the twin reads
  case.expected()               {(offset, group): Line} by numpy, without the twin
  run_plain(cases)              the plain build's lines, {(case, offset, group): Line}
  run_sanitized(cases)          (lines, returncode, stderr) of the sanitized program

A Line is (mismatches, key, decoded, source, block, status); key = frame * 2 + channel of the first mismatch, 2^64 - 1
when there is none (decoded, source and block are then zero)."""
from __future__ import annotations

import ctypes as C
import struct
from collections import namedtuple

import numpy as np

import twinbuild

SRC = twinbuild.NATIVE + "/sim_verify.cpp"
PLANAR, I16, I24 = 0, 1, 2
ALL_DIFFERENT = 0xFFFFFFFF  # a group's edit count that stands for "every sample ^ 1"
NO_KEY = (1 << 64) - 1

Line = namedtuple("Line", "mismatches key decoded source block status")

_lib = None


def lib():
    """The plain build."""
    global _lib
    if _lib is None:
        _lib = C.CDLL(twinbuild.shared_lib("sim_verify", [SRC]))
    return _lib


def sanitized_exe():
    """The sanitized program's path, or (None, why) where the sanitizer runtime is missing."""
    return twinbuild.sanitized_exe("sim_verify_san", [SRC], ["-DSIM_VERIFY_MAIN"])


def to_scratch(left, right, block_frames, ms):
    """What the block decode leaves in the decoder's PCM buffers for this PCM: mid/side in the blocks whose flag is set
    (the inverse of ref src/codec/lac/decoder.cpp:48-65), left/right elsewhere."""
    l = np.array(left, dtype=np.int64)
    r = None if right is None else np.array(right, dtype=np.int64)
    f0 = 0
    for n, flag in zip(block_frames, ms):
        if flag and r is not None:
            a, b = l[f0:f0 + n].copy(), r[f0:f0 + n].copy()
            s = a - b
            l[f0:f0 + n] = a - ((s + (s & 1)) >> 1)
            r[f0:f0 + n] = s
        f0 += n
    return l.astype(np.int32), None if r is None else r.astype(np.int32)


class Case:
    def __init__(self, channels, bit_depth, layout, block_frames, ms, status, left, right, offsets, groups):
        """left / right: the PCM the stream decodes to, which is also the source before a group's edits.  groups: a list
        of edit lists [(frame, channel, value), ...], or ALL_DIFFERENT."""
        self.channels, self.bit_depth, self.layout = channels, bit_depth, layout
        self.block_frames, self.ms, self.status = list(block_frames), list(ms), list(status)
        self.left = np.asarray(left, dtype=np.int32)
        self.right = None if right is None else np.asarray(right, dtype=np.int32)
        self.frames = int(self.left.size)
        assert sum(self.block_frames) == self.frames and (channels == 2) == (right is not None)
        self.offsets, self.groups = list(offsets), list(groups)

    def blob(self) -> bytes:
        nb = len(self.block_frames)
        sl, sr = to_scratch(self.left, self.right, self.block_frames, self.ms)
        out = [struct.pack("<6IQ", self.channels, self.bit_depth, self.layout, nb, len(self.offsets), len(self.groups), self.frames),
               struct.pack(f"<{3 * nb}I", *self.block_frames, *self.ms, *self.status),
               sl.tobytes(), b"" if sr is None else sr.tobytes(),
               self.left.tobytes(), b"" if self.right is None else self.right.tobytes(),
               struct.pack(f"<{len(self.offsets)}I", *self.offsets)]
        for g in self.groups:
            if g == ALL_DIFFERENT:
                out.append(struct.pack("<I", ALL_DIFFERENT))
            else:
                out.append(struct.pack("<I", len(g)) + b"".join(struct.pack("<QIi", f, c, v) for f, c, v in g))
        return b"".join(out)

    def expected(self) -> dict:
        """Brute force: the decoded PCM against the edited source, sample by sample, over the blocks with status 0."""
        dec = np.stack([self.left] if self.right is None else [self.left, self.right], axis=1).astype(np.int64)  # [frame, channel]
        block_of = np.repeat(np.arange(len(self.block_frames)), self.block_frames)
        counted = (np.asarray(self.status)[block_of] == 0)[:, None]
        out = {}
        for gi, g in enumerate(self.groups):
            src = dec.copy()
            if g == ALL_DIFFERENT:
                src ^= 1
            else:
                for f, c, v in g:
                    src[f, c] = v
            diff = (src != dec) & counted
            n = int(diff.sum())
            if n:
                key = int(np.flatnonzero(diff.reshape(-1))[0])  # row-major over [frame, channel]: frame * channels + channel
                f, c = divmod(key, self.channels)
                line = Line(n, 2 * f + c, int(dec[f, c]), int(src[f, c]), int(block_of[f]), tuple(self.status))
            else:
                line = Line(0, NO_KEY, 0, 0, 0, tuple(self.status))
            for off in self.offsets:
                out[(off, gi)] = line
        return out


def parse_lines(text: str) -> dict:
    out = {}
    for ln in text.splitlines():
        if not ln or ln.startswith("done"):
            continue
        case, off, grp, n, key, dec, src, blk, st = ln.split()
        out[(int(case), int(off), int(grp))] = Line(int(n), int(key), int(dec), int(src), int(blk), tuple(int(s) for s in st.split(",")))
    return out


def run_plain(cases) -> dict:
    out = {}
    buf = C.create_string_buffer(1 << 20)
    for i, case in enumerate(cases):
        blob = case.blob()
        rc = lib().sim_verify_lines(blob, C.c_uint64(len(blob)), C.c_uint32(i), buf, C.c_uint64(len(buf)))
        assert rc == 0, (i, rc)
        out.update(parse_lines(buf.value.decode()))
    return out


def run_sanitized(cases, exe=None):
    """(lines, returncode, stderr): a sanitizer report ends the program with a non-zero code and the report in stderr."""
    if exe is None:
        exe, why = sanitized_exe()
        assert exe, why
    env = dict(ASAN_OPTIONS="detect_leaks=0:verify_asan_link_order=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    lines, rc, err = twinbuild.run_cases(exe, [case.blob() for case in cases], env, prefix="verify_cases_", timeout=600)
    return parse_lines("\n".join(lines)), rc, err
