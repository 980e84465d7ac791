"""The digest form's CPU twin (tests/native/sim_digest.cpp over csrc/digest_core.h and csrc/crc32_core.h): built here, called
through ctypes (the plain -O2 build) or run as a program over a file of cases (the build with AddressSanitizer + UBSan,
which needs its runtime first in the process and so cannot be loaded into Python), and the zlib / numpy expectation both
are compared with.

  UNIT, THREADS                 frames per unit and units per workgroup, as the twin exports them
  shift / mul / combine / wav_header_crc   crc32_core.h's functions
  Case(...)                     one item: block table, the PCM it decodes to, a source layout, base offsets
  case.blob()                   the bytes the twin reads
  case.expected()               {offset: Line} from zlib.crc32 over numpy-built bytes, without the twin
  run_plain(cases)              the plain build's lines, {(case, offset): Line}
  run_sanitized(cases)          (lines, returncode, stderr) of the sanitized program

A Line is (decoded, source, key, status): the CRC-32 of the data bytes as the stream form and as the source form make it,
the source form's key of the lowest invalid sample (2^64 - 1: none), the blocks' statuses afterwards."""
from __future__ import annotations

import ctypes as C
import struct
import zlib
from collections import namedtuple

import numpy as np

import twinbuild
import vertwin
import wavutil as W

SRC = twinbuild.NATIVE + "/sim_digest.cpp"
P32, I16, I24, P16, PF32, IF32 = 0, 1, 2, 16, 17, 18
LAYOUTS = {16: (P32, I16, P16, PF32, IF32), 24: (P32, I24, PF32, IF32)}
# base offsets from a 16-byte aligned address that each layout permits (its element alignment), wide and narrow load paths
OFFSETS = {P32: (0, 4, 8, 12), I16: (0, 4), I24: (0, 1, 2, 3), P16: (0, 2, 4, 6, 8), PF32: (0, 4, 8), IF32: (0, 4, 8, 12)}
NO_KEY = (1 << 64) - 1
POLY = 0xEDB88320

Line = namedtuple("Line", "decoded source key status")

_lib = None


def lib():
    """The plain build."""
    global _lib
    if _lib is None:
        L = C.CDLL(twinbuild.shared_lib("sim_digest", [SRC]))
        for name in ("sim_digest_unit_frames", "sim_digest_threads", "sim_crc_mul", "sim_crc_shift", "sim_crc32_combine",
                     "sim_crc32_wav_header"):
            getattr(L, name).restype = C.c_uint32
        L.sim_crc_mul.argtypes = [C.c_uint32, C.c_uint32]
        L.sim_crc_shift.argtypes = [C.c_uint32, C.c_uint64]
        L.sim_crc32_combine.argtypes = [C.c_uint32, C.c_uint32, C.c_uint64]
        L.sim_crc32_wav_header.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64]
        _lib = L
    return _lib


def unit_frames() -> int:
    return int(lib().sim_digest_unit_frames())


def threads() -> int:
    return int(lib().sim_digest_threads())


def mul(a, b):
    return int(lib().sim_crc_mul(a, b))


def shift(r, n):
    return int(lib().sim_crc_shift(r, n))


def combine(a, b, len_b):
    return int(lib().sim_crc32_combine(a, b, len_b))


def wav_header_crc(channels, bit_depth, rate, data_bytes):
    return int(lib().sim_crc32_wav_header(channels, bit_depth, rate, data_bytes))


def sanitized_exe():
    """The sanitized program's path, or (None, why) where the sanitizer runtime is missing."""
    return twinbuild.sanitized_exe("sim_digest_san", [SRC], ["-DSIM_DIGEST_MAIN"])


# ---- the polynomial arithmetic again, on Python integers (bit i of a normal-order integer = the coefficient of x^i) ----
def _bitrev32(v):
    return int(f"{v:032b}"[::-1], 2)


P_NORMAL = (1 << 32) | _bitrev32(POLY)  # x^32 + ... + 1


def poly_mod(a):
    while a.bit_length() > 32:
        a ^= P_NORMAL << (a.bit_length() - 33)
    return a


def poly_mul(a, b):
    out = 0
    while b:
        if b & 1:
            out ^= a
        a <<= 1
        b >>= 1
    return poly_mod(out)


def poly_xpow(e):
    """x^e mod P by square-and-multiply on big integers."""
    out, base = 1, 2
    while e:
        if e & 1:
            out = poly_mul(out, base)
        base = poly_mul(base, base)
        e >>= 1
    return out


def shift_ref(r, nbytes):
    """r * x^(8 * nbytes) mod P for a register value in the reflected representation."""
    return _bitrev32(poly_mul(_bitrev32(r), poly_xpow(8 * nbytes)))


def source_elements(left, right, bit_depth, layout):
    """The elements of a source in that layout, as int32 words: the samples, or the bits of sample * 2^-(bit_depth - 1)."""
    def one(x):
        x = np.asarray(x, dtype=np.int32)
        if layout in (PF32, IF32):
            return (x.astype(np.float32) / np.float32(1 << (bit_depth - 1))).view(np.int32)
        return x
    return one(left), None if right is None else one(right)


class Case:
    def __init__(self, channels, bit_depth, layout, block_frames, ms, status, left, right, offsets=None, src_left=None, src_right=None):
        """left / right: the PCM the stream decodes to, which is also what the source holds, unless src_left / src_right
        give the source's elements themselves (int32 words: samples, or float32 bits)."""
        self.channels, self.bit_depth, self.layout = channels, bit_depth, layout
        self.block_frames, self.ms, self.status = list(block_frames), list(ms), list(status)
        self.left = np.asarray(left, dtype=np.int32)
        self.right = None if right is None else np.asarray(right, dtype=np.int32)
        self.frames = int(self.left.size)
        assert sum(self.block_frames) == self.frames and (channels == 2) == (right is not None)
        self.offsets = list(OFFSETS[layout] if offsets is None else offsets)
        sl, sr = source_elements(self.left, self.right, bit_depth, layout)
        self.src_left = sl if src_left is None else np.asarray(src_left, dtype=np.int32)
        self.src_right = sr if src_right is None else np.asarray(src_right, dtype=np.int32)
        self.source_key = NO_KEY  # what the source form reports; a case with invalid elements sets it

    def blob(self) -> bytes:
        nb = len(self.block_frames)
        sl, sr = vertwin.to_scratch(self.left, self.right, self.block_frames, self.ms)
        return b"".join([struct.pack("<6IQ", self.channels, self.bit_depth, self.layout, nb, len(self.offsets), 0, self.frames),
                         struct.pack(f"<{3 * nb}I", *self.block_frames, *self.ms, *self.status),
                         sl.tobytes(), b"" if sr is None else sr.tobytes(),
                         self.src_left.tobytes(), b"" if self.src_right is None else self.src_right.tobytes(),
                         struct.pack(f"<{len(self.offsets)}I", *self.offsets)])

    def data_bytes(self, decoded_form: bool) -> bytes:
        """The WAV data chunk of the PCM (numpy / wavutil); for the stream form with the frames of every block that did
        not decode as zeros."""
        l, r = self.left.copy(), None if self.right is None else self.right.copy()
        if decoded_form:
            f0 = 0
            for n, st in zip(self.block_frames, self.status):
                if st:
                    l[f0:f0 + n] = 0
                    if r is not None:
                        r[f0:f0 + n] = 0
                f0 += n
        return W.pcm_bytes(l, r, self.bit_depth)

    def expected(self) -> dict:
        line = Line(zlib.crc32(self.data_bytes(True)), zlib.crc32(self.data_bytes(False)), self.source_key, tuple(self.status))
        return {off: line for off in self.offsets}


def parse_lines(text: str) -> dict:
    out = {}
    for ln in text.splitlines():
        if not ln or ln.startswith("done"):
            continue
        case, off, dec, src, key, st = ln.split()
        out[(int(case), int(off))] = Line(int(dec), int(src), int(key), tuple(int(s) for s in st.split(",")))
    return out


def run_plain(cases) -> dict:
    out = {}
    buf = C.create_string_buffer(1 << 16)
    for i, case in enumerate(cases):
        blob = case.blob()
        rc = lib().sim_digest_lines(blob, C.c_uint64(len(blob)), C.c_uint32(i), buf, C.c_uint64(len(buf)))
        assert rc == 0, (i, rc)
        out.update(parse_lines(buf.value.decode()))
    return out


def run_sanitized(cases, exe=None):
    """(lines, returncode, stderr): a sanitizer report ends the program with a non-zero code and the report in stderr."""
    if exe is None:
        exe, why = sanitized_exe()
        assert exe, why
    env = dict(ASAN_OPTIONS="detect_leaks=0:verify_asan_link_order=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    lines, rc, err = twinbuild.run_cases(exe, [case.blob() for case in cases], env, prefix="digest_cases_", timeout=600)
    return parse_lines("\n".join(lines)), rc, err
