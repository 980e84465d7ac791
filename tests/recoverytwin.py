"""An independent restatement of the recovery data (include/lacx.h, "Recovery data"): GF(2^8) by log / exp tables and numpy
look-ups (the product multiplies by shifts and xors), zlib.crc32, struct for the bytes.  It builds sidecars, classifies
slices and repairs by Gaussian elimination on the equations themselves (the product inverts the Cauchy submatrix and folds
it into one matrix).  Also the harness of the CPU twin, tests/native/sim_recovery.cpp: the plain build as a library, the
sanitized build as a program of its own, and cleared(), which lets a job to the device only after the sanitized twin has
passed it in this run."""
import ctypes as C
import struct
import sys
import zlib
from collections import namedtuple

import numpy as np

import twinbuild

OK, INVALID, RUNTIME, DEVICE, MISMATCH = 0, 1, 2, 3, 4
TRUNCATED, TRAILING, SIDECAR_TRUNCATED, UNREPAIRED = 1, 2, 4, 8
BEST_EFFORT = 1
# (S, r, K): the parameter sets of the tests
SETS = [(64, 1, 1), (64, 2, 4), (80, 3, 5), (256, 4, 16), (4096, 8, 128), (64, 32, 224)]

# ---- the field: polynomial 0x11D, generator 2 ---------------------------------------------------------------------------
EXP = np.zeros(510, np.uint8)
LOG = np.zeros(256, np.int32)
_v = 1
for _i in range(255):
    EXP[_i] = EXP[_i + 255] = _v
    LOG[_v] = _i
    _v <<= 1
    if _v & 0x100:
        _v ^= 0x11D
MUL = np.zeros((256, 256), np.uint8)  # MUL[c][x] = c * x
for _c in range(1, 256):
    MUL[_c, 1:] = EXP[LOG[_c] + LOG[1:256]]


def inv(a: int) -> int:
    assert a != 0
    return int(EXP[255 - LOG[a]])


def coef(r: int, p: int, i: int) -> int:
    return inv(p ^ (r + i))


# ---- geometry and sidecar -----------------------------------------------------------------------------------------------
Geometry = namedtuple("Geometry", "S r K L k G")


def geometry(L, S, r, K) -> Geometry:
    k = -(-L // S)
    return Geometry(S, r, K, L, k, -(-k // K))


def members(geo, g):
    return list(range(g, geo.k, geo.G))


def _matrix(data: bytes, geo) -> np.ndarray:
    """(k, S): the slices, the last zero-extended."""
    m = np.zeros(geo.k * geo.S, np.uint8)
    m[:len(data)] = np.frombuffer(data, np.uint8)
    return m.reshape(geo.k, geo.S)


def slice_crcs(data: bytes, geo):
    return [zlib.crc32(data[i * geo.S:(i + 1) * geo.S]) for i in range(geo.k)]


def parity(D: np.ndarray, geo, g: int, p: int) -> np.ndarray:
    acc = np.zeros(geo.S, np.uint8)
    for i, s in enumerate(members(geo, g)):
        acc ^= MUL[coef(geo.r, p, i)][D[s]]
    return acc


def build(data: bytes, S=4096, r=8, K=128) -> bytes:
    geo = geometry(len(data), S, r, K)
    D = _matrix(data, geo)
    first = b"LACR" + struct.pack(">BBHIQIII", 1, r, K, S, len(data), zlib.crc32(data), geo.k, geo.G)
    table = b"".join(struct.pack(">I", c) for c in slice_crcs(data, geo))
    out = [first, struct.pack(">I", zlib.crc32(first)), table, struct.pack(">I", zlib.crc32(table))]
    for g in range(geo.G):
        for p in range(r):
            rec = parity(D, geo, g, p).tobytes()
            out.append(rec + struct.pack(">I", zlib.crc32(rec)))
    return b"".join(out)


def _combine(a, b, len_b):
    """zlib's crc32_combine restated with zlib.crc32 itself, which is affine in (bytes, start value): crc32(A + B) =
    crc32(B) ^ crc32(zeros, crc32(A)) ^ crc32(zeros)."""
    zeros = b"\0" * len_b
    return b ^ zlib.crc32(zeros, a) ^ zlib.crc32(zeros)


def rehead(side: bytes, table=None, **fields) -> bytes:
    """The sidecar with head fields and / or slice table replaced and both head checksums made right again (the parity area
    as it is): what a forger who knows the format would write."""
    f = dict(zip("version r K S L file_crc k G".split(), struct.unpack(">BBHIQIII", side[4:32])))
    k_old = f["k"]
    f.update(fields)
    old_table = side[36:36 + 4 * k_old]
    new_table = old_table if table is None else b"".join(struct.pack(">I", c) for c in table)
    first = side[:4] + struct.pack(">BBHIQIII", *[f[n] for n in "version r K S L file_crc k G".split()])
    return first + struct.pack(">I", zlib.crc32(first)) + new_table + struct.pack(">I", zlib.crc32(new_table)) + side[40 + 4 * k_old:]


class Refused(ValueError):
    pass


def parse(side: bytes):
    """(Geometry, file_crc32, [slice crc], records wholly inside, flags) or Refused("[recovery-error] ...")."""
    def no(text):
        raise Refused("[recovery-error] " + text)
    if len(side) < 40:
        no("short input")
    if side[:4] != b"LACR":
        no("wrong magic")
    version, r, K, S, L, file_crc, k, G = struct.unpack(">BBHIQIII", side[4:32])
    if version != 1:
        no("unsupported version: %d" % version)
    if struct.unpack(">I", side[32:36])[0] != zlib.crc32(side[:32]):
        no("checksum of the header differs")
    if S < 64 or S > 65536 or S % 16:
        no("slice_bytes %d is not a multiple of 16 in 64..65536" % S)
    if not 1 <= r <= 32:
        no("parity %d is not in 1..32" % r)
    if not 1 <= K <= 256 - r:
        no("group_data %d is not in 1..256 - parity" % K)
    if L == 0:
        no("file_bytes is 0")
    geo = geometry(L, S, r, K)
    if geo.k >= 1 << 28:
        no("the file needs %d slices, 2^28 or more" % geo.k)
    if k != geo.k:
        no("slices %d, file_bytes and slice_bytes give %d" % (k, geo.k))
    if G != geo.G:
        no("groups %d, slices and group_data give %d" % (G, geo.G))
    if len(side) < 40 + 4 * k:
        no("slice table is cut short")
    table = side[36:36 + 4 * k]
    if struct.unpack(">I", side[36 + 4 * k:40 + 4 * k])[0] != zlib.crc32(table):
        no("checksum of the slice table differs")
    crcs = list(struct.unpack(">%dI" % k, table))
    allc = crcs[0]
    for i in range(1, k):
        allc = _combine(allc, crcs[i], S if i + 1 < k else L - (k - 1) * S)
    if allc != file_crc:
        no("file_crc32 is not the combination of the slice checksums")
    full = 40 + 4 * k + G * r * (S + 4)
    present = min(G * r, (len(side) - 40 - 4 * k) // (S + 4))
    return geo, file_crc, crcs, present, (SIDECAR_TRUNCATED if len(side) < full else 0)


# result: (file_bytes, slices, bad_slices, repaired_slices, first_bad, parity_slices, bad_parity, worst_group,
#          worst_group_bad, worst_group_parity, flags); out: bytes or None
Outcome = namedtuple("Outcome", "code message result bad out")
ZERO = (0,) * 11


def _judge(file: bytes, side: bytes):
    geo, file_crc, crcs, present, flags = parse(side)
    data = file[:geo.L] + b"\0" * max(0, geo.L - len(file))
    flags |= (TRUNCATED if len(file) < geo.L else 0) | (TRAILING if len(file) > geo.L else 0)
    bad = [i for i, c in enumerate(slice_crcs(data, geo)) if c != crcs[i]]
    at = 40 + 4 * geo.k
    records, usable = [], []
    for q in range(geo.G * geo.r):
        rec = side[at + q * (geo.S + 4):at + (q + 1) * (geo.S + 4)]
        good = q < present and struct.unpack(">I", rec[geo.S:])[0] == zlib.crc32(rec[:geo.S])
        records.append(np.frombuffer(rec[:geo.S], np.uint8) if good else None)
        usable.append(good)
    gbad = [sum(1 for s in bad if s % geo.G == g) for g in range(geo.G)]
    gpar = [sum(usable[g * geo.r:(g + 1) * geo.r]) for g in range(geo.G)]
    worst = max(range(geo.G), key=lambda g: (gbad[g] - gpar[g], -g))
    short = [g for g in range(geo.G) if gbad[g] > gpar[g]]
    if short:
        flags |= UNREPAIRED
    result = [geo.L, geo.k, len(bad), 0, bad[0] if bad else geo.k, geo.G * geo.r, geo.G * geo.r - sum(usable), worst, gbad[worst], gpar[worst], flags]
    return geo, crcs, data, bad, records, usable, gbad, gpar, short, result


def scan(file: bytes, side: bytes) -> Outcome:
    try:
        geo, crcs, data, bad, records, usable, gbad, gpar, short, result = _judge(file, side)
    except Refused as e:
        return Outcome(INVALID, str(e), ZERO, [], None)
    if bad or result[10] & TRUNCATED:
        text = "[recovery-error] slice=%d bad_slices=%d %s" % (result[4], len(bad), "unrepairable" if short else "repairable")
        return Outcome(MISMATCH, text, tuple(result), bad, None)
    return Outcome(OK, "", tuple(result), bad, None)


def _solve(A, rhs):
    """x with A x = rhs over GF(2^8): A (b, b) ints, rhs (b, S) uint8; elimination on the augmented rows."""
    b = len(A)
    A = [list(row) for row in A]
    rhs = [row.copy() for row in rhs]
    for col in range(b):
        piv = next(j for j in range(col, b) if A[j][col])
        A[col], A[piv], rhs[col], rhs[piv] = A[piv], A[col], rhs[piv], rhs[col]
        f = inv(A[col][col])
        A[col] = [int(MUL[f][v]) for v in A[col]]
        rhs[col] = MUL[f][rhs[col]]
        for j in range(b):
            if j != col and A[j][col]:
                f = A[j][col]
                A[j] = [v ^ int(MUL[f][w]) for v, w in zip(A[j], A[col])]
                rhs[j] = rhs[j] ^ MUL[f][rhs[col]]
    return rhs


def repair(file: bytes, side: bytes, best_effort=False) -> Outcome:
    try:
        geo, crcs, data, bad, records, usable, gbad, gpar, short, result = _judge(file, side)
    except Refused as e:
        return Outcome(INVALID, str(e), ZERO, [], None)
    code, text = OK, ""
    if short:
        g = short[0]
        code, text = MISMATCH, "[recovery-error] group %d: %d damaged slices, %d parity slices usable" % (g, gbad[g], gpar[g])
        if not best_effort:
            return Outcome(code, text, tuple(result), bad, None)
    D = _matrix(data, geo).copy()
    repaired = []
    for g in range(geo.G):
        mem = members(geo, g)
        lost = [i for i, s in enumerate(mem) if s in set(bad)]
        if not lost or g in short:
            continue
        rows = [p for p in range(geo.r) if usable[g * geo.r + p]][:len(lost)]
        rhs = []
        for p in rows:
            acc = records[g * geo.r + p].copy()
            for i, s in enumerate(mem):
                if i not in lost:
                    acc ^= MUL[coef(geo.r, p, i)][D[s]]
            rhs.append(acc)
        x = _solve([[coef(geo.r, p, i) for i in lost] for p in rows], rhs)
        for i, row in zip(lost, x):
            D[mem[i]] = row
            repaired.append(mem[i])
    out = D.reshape(-1)[:geo.L].tobytes()
    if any(zlib.crc32(out[s * geo.S:(s + 1) * geo.S]) != crcs[s] for s in repaired):
        return Outcome(MISMATCH, "[recovery-error] repaired file does not match its checksum", tuple(result), bad, None)
    result[3] = len(repaired)
    return Outcome(code, text, tuple(result), bad, out)


# ---- the CPU twin ---------------------------------------------------------------------------------------------------------
SRC = twinbuild.NATIVE + "/sim_recovery.cpp"
_lib = None


class Info(C.Structure):
    _fields_ = [("file_bytes", C.c_uint64), ("file_crc32", C.c_uint32), ("slice_bytes", C.c_uint32), ("slices", C.c_uint32),
                ("groups", C.c_uint32), ("parity", C.c_uint16), ("group_data", C.c_uint16), ("parity_present", C.c_uint32),
                ("flags", C.c_uint32), ("reserved", C.c_uint32)]


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(twinbuild.shared_lib("sim_recovery", [SRC]))
        _lib.sim_recovery.restype = C.c_longlong
        _lib.sim_recovery.argtypes = [C.c_char_p, C.c_uint64, C.c_void_p, C.c_uint64]
        _lib.sim_gf_mul4.restype = C.c_uint32
        _lib.sim_gf_mul4.argtypes = [C.c_uint32, C.c_uint32]
        _lib.sim_gf_inv.restype = C.c_uint32
        _lib.sim_gf_invert.argtypes = [C.c_void_p, C.c_uint32]
        _lib.sim_recovery_parse.argtypes = [C.c_char_p, C.c_uint64, C.POINTER(Info), C.c_char_p, C.c_uint32]
    return _lib


def sanitized_exe():
    """The sanitized program's path, or (None, why) where the sanitizer runtime is missing."""
    return twinbuild.sanitized_exe("sim_recovery_san", [SRC], ["-DSIM_RECOVERY_MAIN"])


def build_case(files, S=0, r=0, K=0) -> bytes:
    return b"\0" + struct.pack("<IIII", len(files), S, r, K) + b"".join(struct.pack("<Q", len(x)) + x for x in files)


def repair_case(files, sides, best_effort=False, scan_only=False) -> bytes:
    body = struct.pack("<II", len(files), BEST_EFFORT if best_effort else 0)
    for x, s in zip(files, sides):
        body += struct.pack("<Q", len(x)) + x + struct.pack("<Q", len(s)) + s
    return (b"\1" if scan_only else b"\2") + body


def answer(case: bytes) -> bytes:
    """The plain build's answer to a case, as bytes."""
    cap = 4096 + 3 * len(case) + (1 << 20)
    while True:
        buf = C.create_string_buffer(cap)
        n = lib().sim_recovery(case, C.c_uint64(len(case)), buf, C.c_uint64(cap))
        if n == -2:
            cap *= 4
            continue
        assert n >= 0, "malformed case"
        return buf.raw[:n]


def outcomes(case: bytes, blob: bytes = None):
    """The answer of a case as [Outcome] (a build's result is ZERO and its bad list empty)."""
    blob = answer(case) if blob is None else blob
    n = struct.unpack_from("<I", case, 1)[0]
    at, out = 0, []
    for _ in range(n):
        code, mlen = struct.unpack_from("<iI", blob, at)
        at += 8
        text = blob[at:at + mlen].decode()
        at += mlen
        result, bad = ZERO, []
        if case[0] != 0:
            L, *rest = struct.unpack_from("<Q10I", blob, at)
            result = (L, *rest)
            at += 48
            nbad = struct.unpack_from("<I", blob, at)[0]
            bad = list(struct.unpack_from("<%dI" % nbad, blob, at + 4))
            at += 4 + 4 * nbad
        size = struct.unpack_from("<Q", blob, at)[0]
        at += 8
        data = None
        if size != (1 << 64) - 1:
            data = blob[at:at + size]
            at += size
        out.append(Outcome(code, text, result, bad, data))
    assert at == len(blob)
    return out


def run_sanitized(cases, exe=None, workers=8):
    """Every case through the sanitized program, split over a few processes: (lines, returncode, stderr)."""
    if exe is None:
        exe, why = sanitized_exe()
        assert exe, why
    env = dict(ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    return twinbuild.run_cases(exe, cases, env, workers=workers, prefix="lac_recovery_")


def digest_line(blob: bytes) -> str:
    return "%d %08x" % (len(blob), zlib.crc32(blob))


def cleared(key, cases):
    """[the plain build's answer per case], once the sanitized twin has shown in this run that each of these jobs stays inside
    buffers of exactly the plan's capacities and answers as the plain build does.  Fails, never skips, where that cannot
    be shown."""
    def make():
        answers = [answer(c) for c in cases]
        return cases, lambda c, i: digest_line(answers[i]), None, answers

    return twinbuild.cleared("recovery", key, sys.modules[__name__], make)
