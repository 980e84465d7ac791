"""The import pass's CPU twin (tests/native/sim_import.cpp over csrc/import_core.h) and the verify form's twin for sources
in any layout (tests/native/sim_verify_layouts.cpp over csrc/verify_core.h): built here, called through ctypes (the plain
-O2 build) or -- the import twin -- run as a program over a file of cases (the build with AddressSanitizer + UBSan, which
needs its runtime first in the process and so cannot be loaded into Python), and the numpy conversions both are compared
with.

  Case(layout, channels, bit_depth, offset, left, right)   one source; left / right: int16 or float32 arrays
  case.expected()               Answer by numpy, without the twin
  run_plain(cases)              the plain build's Answers
  run_sanitized(cases)          (Answers, returncode, stderr) of the sanitized program
  verify_layout(...)            lacx_verify_result's fields for one item through verify_core.h
  unit_frames()                 frames per import unit (one workgroup of the kernel)

An Answer is (alias, code, message, dst): dst the destination bytes (interleaved int16 / packed int24; for an alias the
source bytes the kernels read in place), code 0 / 1 (LACX_OK / LACX_E_INVALID)."""
from __future__ import annotations

import ctypes as C
import os
import struct
import tempfile
from collections import namedtuple

import numpy as np

import twinbuild

SRC = twinbuild.NATIVE + "/sim_import.cpp"
SRC_VERIFY = twinbuild.NATIVE + "/sim_verify_layouts.cpp"
PLANAR_I32, INTERLEAVED_I16, INTERLEAVED_I24 = 0, 1, 2
PLANAR_I16, PLANAR_F32, INTERLEAVED_F32 = 16, 17, 18
NO_KEY = (1 << 64) - 1

Answer = namedtuple("Answer", "alias code message dst")

_lib = None


def lib():
    """The plain build (both twins)."""
    global _lib
    if _lib is None:
        _lib = C.CDLL(twinbuild.shared_lib("sim_import", [SRC, SRC_VERIFY]))
        _lib.sim_import_answer.restype = C.c_longlong
        _lib.sim_import_unit_frames.restype = C.c_uint32
    return _lib


def unit_frames() -> int:
    return int(lib().sim_import_unit_frames())


def sanitized_exe():
    """The sanitized program's path, or (None, why) where the sanitizer runtime is missing."""
    return twinbuild.sanitized_exe("sim_import_san", [SRC], ["-DSIM_IMPORT_MAIN"])


def to_float(samples, bit_depth) -> np.ndarray:
    """LACX_SAMPLE_F32: sample * 2^-(bit_depth - 1), exact in float32."""
    return (np.asarray(samples, dtype=np.int64).astype(np.float64) * 2.0 ** -(bit_depth - 1)).astype(np.float32)


def classify(x: np.ndarray, bit_depth: int):
    """The float rule in float64 (where x * 2^(b-1) is exact for every finite float32): (kind, value) arrays; kind 0 a
    sample, 1 an integer outside the depth, 2 anything else; value = the sample where kind is 0, else 0."""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(invalid="ignore"):  # (signalling NaNs among the inputs)
        p = x.astype(np.float64) * 2.0 ** (bit_depth - 1)
    finite = np.isfinite(p)
    bits = x.view(np.uint32)
    denormal = ((bits >> 23) & 0xFF == 0) & ((bits & 0x7FFFFF) != 0)
    integer = finite & ~denormal & (np.where(finite, p, 0.0) == np.floor(np.where(finite, p, 0.0)))
    lim = 1 << (bit_depth - 1)
    inside = integer & (np.where(integer, p, 0.0) >= -lim) & (np.where(integer, p, 0.0) <= lim - 1)
    kind = np.where(inside, 0, np.where(integer, 1, 2))
    value = np.where(inside, np.where(inside, p, 0.0), 0.0).astype(np.int64)
    return kind, value


def invalid_values(depth):
    """The corpus of float values around the rule's edges: (value, kind), kind 0 a sample, 1 an integer outside the depth,
    2 not an exact sample."""
    f32 = lambda bits: np.array([bits], dtype=np.uint32).view(np.float32)[0]
    step = np.float32(2.0 ** -(depth - 1))
    g = np.float32(1000 * float(step))  # a grid point; its neighbours in float32 are off the grid
    return [
        (np.nextafter(g, np.float32(1)), 2), (np.nextafter(g, np.float32(-1)), 2),
        (np.nextafter(-g, np.float32(1)), 2), (np.nextafter(-g, np.float32(-1)), 2),
        (np.float32(2.0 ** -depth), 2),                      # half a step: 2^-16 at depth 16, 2^-24 at depth 24
        (np.float32(2.0 ** -(depth - 1)), 0),                # one step (2^-23 at depth 24) is a sample
        (f32(0x00000001), 2), (f32(0x807FFFFF), 2),          # denormals
        (np.float32(np.nan), 2), (f32(0xFFC00001), 2), (np.float32(np.inf), 2), (np.float32(-np.inf), 2),
        (np.float32(1.0), 1), (np.float32(-1.0), 0), (np.float32(-1.0) - step, 1), (np.float32(1.0) - step, 0),
        (np.float32(-0.0), 0), (np.float32(2.0), 1), (np.float32(-3.0e38), 1), (np.float32(1.5) * step, 2),
    ]


def pack(samples: np.ndarray, bit_depth: int) -> bytes:
    """[frames, channels] integer samples as interleaved int16 / packed int24 bytes."""
    s = np.ascontiguousarray(samples, dtype=np.int64).reshape(-1)
    if bit_depth == 16:
        return s.astype("<i2").tobytes()
    return (s & 0xFFFFFF).astype("<u4").view(np.uint8).reshape(-1, 4)[:, :3].tobytes()


class Case:
    def __init__(self, layout, channels, bit_depth, offset, left, right=None):
        """left / right: the channels' elements (int16 for PLANAR_I16, else float32; any bit pattern).  offset: elements
        between a 16-byte aligned address and the source's base."""
        self.layout, self.channels, self.bit_depth, self.offset = layout, channels, bit_depth, offset
        dt = np.int16 if layout == PLANAR_I16 else np.float32
        self.left = np.ascontiguousarray(left, dtype=dt)
        self.right = None if right is None else np.ascontiguousarray(right, dtype=dt)
        self.frames = int(self.left.size)
        assert (channels == 2) == (right is not None)

    def blob(self) -> bytes:
        rows = [self.left] if self.right is None else [self.left, self.right]
        data = np.stack(rows, axis=1).tobytes() if self.layout == INTERLEAVED_F32 else b"".join(r.tobytes() for r in rows)
        return struct.pack("<4IQ", self.layout, self.channels, self.bit_depth, self.offset, self.frames) + data

    def is_alias(self) -> bool:
        return self.layout == PLANAR_I16 and self.channels == 1 and (2 * self.offset) % 4 == 0

    def expected(self) -> Answer:
        rows = [self.left] if self.right is None else [self.left, self.right]
        if self.layout == PLANAR_I16:
            vals = [r.astype(np.int64) for r in rows]
            kinds = [np.zeros(self.frames, dtype=np.int64) for _ in rows]
        else:
            both = [classify(r, self.bit_depth) for r in rows]
            kinds, vals = [k for k, _ in both], [v for _, v in both]
        code, message = 0, ""
        for name, kind in zip(("left", "right"), kinds):  # all of left first, then right
            bad = np.flatnonzero(kind)
            if bad.size:
                i = int(bad[0])
                what = "is outside the configured PCM bit depth" if kind[i] == 1 else f"is not an exact {self.bit_depth}-bit PCM value"
                code, message = 1, f"{name} sample at index {i} {what}"
                break
        return Answer(int(self.is_alias()), code, message, pack(np.stack(vals, axis=1), self.bit_depth))


def parse_answers(data: bytes) -> list:
    out, at = [], 0
    while at < len(data):
        alias, code, _kl, _kr, nbytes = struct.unpack_from("<IIQQQ", data, at)
        at += 32
        dst = data[at:at + nbytes]
        at += nbytes
        (mlen,) = struct.unpack_from("<I", data, at)
        at += 4
        out.append(Answer(alias, code, data[at:at + mlen].decode(), dst))
        at += mlen
    return out


def run_plain(cases) -> list:
    out = []
    for case in cases:
        blob = case.blob()
        buf = C.create_string_buffer(len(blob) + 512)
        n = lib().sim_import_answer(blob, C.c_uint64(len(blob)), buf, C.c_uint64(len(buf)))
        assert n >= 0, n
        out.extend(parse_answers(buf.raw[:n]))
    return out


def run_sanitized(cases, exe=None):
    """(answers, returncode, stderr): a sanitizer report ends the program with a non-zero code and the report in stderr."""
    if exe is None:
        exe, why = sanitized_exe()
        assert exe, why
    with tempfile.TemporaryDirectory(prefix="import_cases_") as d:
        dst = os.path.join(d, "answers.bin")
        env = dict(ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
        _, rc, err = twinbuild.run_cases(exe, [case.blob() for case in cases], env, lambda path, a, n: [path, dst], prefix="import_cases_",
                                         timeout=600)
        answers = parse_answers(open(dst, "rb").read()) if os.path.exists(dst) and rc == 0 else []
    return answers, rc, err


def f32_to_pcm(x, bit_depth):
    """(kind, value) of one float32 through the product's own rule (import_core.h)."""
    v = C.c_int32()
    bits = int(np.array([x], dtype=np.float32).view(np.uint32)[0])
    kind = lib().sim_f32_to_pcm(C.c_uint32(bits), C.c_int(bit_depth), C.byref(v))
    return int(kind), int(v.value)


def aligned(n, dtype, offset=0) -> np.ndarray:
    """n elements of dtype whose first lies `offset` elements behind a 16-byte aligned address."""
    item = np.dtype(dtype).itemsize
    raw = np.zeros((n + offset) * item + 16, dtype=np.uint8)
    start = (-raw.ctypes.data) % 16 + offset * item
    return raw[start:start + n * item].view(dtype)


VerifyLine = namedtuple("VerifyLine", "mismatches key decoded source block status")


def verify_layout(channels, bit_depth, layout, block_frames, ms, status, scratch_left, scratch_right, src0, src1) -> VerifyLine:
    """One item through verify_core.h: scratch_*: what the block decode leaves (vertwin.to_scratch), src0 / src1: numpy
    arrays in the source's own layout at the base alignment the caller gave them."""
    frames = int(sum(block_frames))
    left = aligned(frames, np.int32)
    left[:] = scratch_left
    right = None
    if channels == 2:
        right = aligned(frames, np.int32)
        right[:] = scratch_right
    bf = np.asarray(block_frames, dtype=np.uint32)
    msf = np.asarray(ms, dtype=np.uint8)
    st = np.asarray(status, dtype=np.uint32).copy()
    out = (C.c_longlong * 5)()
    rc = lib().sim_verify_layout(C.c_uint32(channels), C.c_uint32(bit_depth), C.c_uint32(layout), C.c_uint32(bf.size),
                                 C.c_void_p(bf.ctypes.data), C.c_void_p(msf.ctypes.data), C.c_void_p(st.ctypes.data),
                                 C.c_void_p(left.ctypes.data), C.c_void_p(right.ctypes.data if right is not None else None),
                                 C.c_uint64(frames), C.c_void_p(src0.ctypes.data),
                                 C.c_void_p(src1.ctypes.data if src1 is not None else None), out)
    assert rc == 0, rc
    return VerifyLine(int(out[0]), int(out[1]) & NO_KEY, int(out[2]), int(out[3]), int(out[4]), tuple(int(s) for s in st))
