"""Recovery data without a device: the CPU twin (tests/native/sim_recovery.cpp -- csrc/recovery_plan.h run as the C ABI
runs it, csrc/recovery_core.h looped over every thread the kernels would launch, every buffer at exactly the plan's
capacity; plain as a library and under AddressSanitizer + UBSan as a program of its own) against recoverytwin, a
restatement with log / exp tables, zlib.crc32 and struct.  No expectation comes from the code under test."""
import ctypes as C
import functools
import glob
import itertools
import os
import struct
import zlib

import numpy as np
import pytest

import recoverytwin as rt

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SMALL_SETS = [(64, 2, 4), (80, 3, 5)]


def _read(path):
    with open(path, "rb") as f:
        return f.read()


FIXTURES = {os.path.basename(p)[:-4]: _read(p) for d in ("small", "decode_wav") for p in sorted(glob.glob(os.path.join(GOLDEN, d, "*.lac")))}
BASE = FIXTURES["n2400_mono16_selftest"]  # 1406 bytes: 22 slices of 64 in 6 uneven groups, 18 slices of 80 in 4


def _bytes(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def _hit(data, S, slices):
    """data with one byte changed in each of the given slices."""
    b = bytearray(data)
    for s in slices:
        at = min(s * S + (7 * s) % S, len(b) - 1) if (s + 1) * S > len(b) else s * S + (7 * s) % S
        b[at] ^= 0x5A
    return bytes(b)


def _hit_parity(side, geo, records):
    b = bytearray(side)
    for q in records:
        b[40 + 4 * geo.k + q * (geo.S + 4) + (q * 5) % (geo.S + 4)] ^= 0x21  # in the record or in its checksum
    return bytes(b)


# ---- the field ------------------------------------------------------------------------------------------------------------
def test_packed_multiply_matches_the_table():
    """All 256 coefficients over 64 words that together hold every byte value in every byte position."""
    lib = rt.lib()
    vals = np.arange(256, dtype=np.uint8)
    for shift in range(4):
        words = np.roll(vals, 64 * shift).reshape(4, 64).T.copy().view("<u4").ravel()  # byte b of word j = a different value
        assert sorted(np.roll(vals, 64 * shift).tolist()) == list(range(256))
        for c in range(256):
            for w in words:
                want = int(np.frombuffer(rt.MUL[c][np.frombuffer(struct.pack("<I", int(w)), np.uint8)].tobytes(), "<u4")[0])
                assert lib.sim_gf_mul4(int(w), c) == want, (c, hex(int(w)))
    for a in range(1, 256):
        assert lib.sim_gf_inv(a) == rt.inv(a) and rt.MUL[a][rt.inv(a)] == 1


@pytest.mark.parametrize("r,K", [(2, 4), (3, 5)])
def test_every_square_cauchy_submatrix_is_inverted(r, K):
    lib = rt.lib()
    count = 0
    for b in range(1, r + 1):
        for rows in itertools.combinations(range(r), b):
            for cols in itertools.combinations(range(K), b):
                A = [[rt.coef(r, p, i) for i in cols] for p in rows]
                buf = (C.c_uint8 * (b * b))(*[v for row in A for v in row])
                assert lib.sim_gf_invert(buf, b) == 1, (rows, cols)
                inv = [[buf[j * b + l] for l in range(b)] for j in range(b)]
                for j in range(b):
                    for l in range(b):
                        acc = 0
                        for m in range(b):
                            acc ^= int(rt.MUL[A[j][m]][inv[m][l]])
                        assert acc == (1 if j == l else 0), (rows, cols)
                count += 1
    assert count == sum(len(list(itertools.combinations(range(r), b))) * len(list(itertools.combinations(range(K), b))) for b in range(1, r + 1))


# ---- geometry and sidecar bytes ---------------------------------------------------------------------------------------
def _twin_build(files, S, r, K):
    return rt.outcomes(rt.build_case(files, S, r, K))


def test_geometry_cases():
    """k < K, k no multiple of G, and L mod S in {0, 1, 3, 4, S - 1}: the bytes are the restatement's, the head says so."""
    for S, r, K in [(64, 2, 4), (80, 3, 5), (256, 4, 16)]:
        lengths = [1, 3, S - 1, S, S + 1, 2 * S + 3, 3 * S + 4, (K - 1) * S, K * S + 1, (2 * K + 1) * S + S - 1, 5 * K * S // 2 + 4]
        files = [_bytes(L, L + S) for L in lengths]
        assert {L % S for L in lengths} >= {0, 1, 3, 4, S - 1}
        geos = [rt.geometry(L, S, r, K) for L in lengths]
        assert any(g.k < K for g in geos) and any(g.k % g.G for g in geos)
        for data, geo, got in zip(files, geos, _twin_build(files, S, r, K)):
            assert got.code == rt.OK and got.out == rt.build(data, S, r, K), (S, len(data))
            assert len(got.out) == 40 + 4 * geo.k + geo.G * r * (S + 4)
            info, msg = rt.Info(), C.create_string_buffer(256)
            assert rt.lib().sim_recovery_parse(got.out, len(got.out), C.byref(info), msg, 256) == 0
            assert (info.file_bytes, info.file_crc32, info.slice_bytes, info.slices, info.groups, info.parity, info.group_data,
                    info.parity_present, info.flags) == (len(data), zlib.crc32(data), S, geo.k, geo.G, r, K, geo.G * r, 0)
            assert [len(rt.members(geo, g)) for g in range(geo.G)] == [-(-(geo.k - g) // geo.G) for g in range(geo.G)]


@pytest.mark.parametrize("S,r,K", rt.SETS)
def test_sidecar_bytes_of_every_golden_stream(S, r, K):
    names = sorted(FIXTURES)
    for name, got in zip(names, _twin_build([FIXTURES[n] for n in names], S, r, K)):
        assert got.code == rt.OK and got.out == rt.build(FIXTURES[name], S, r, K), name


def test_default_parameters_and_parameter_ranges():
    got = _twin_build([BASE], 0, 0, 0)[0]
    assert got.out == rt.build(BASE, 4096, 8, 128)
    for (S, r, K), text in [((48, 2, 4), "slice_bytes 48 is not a multiple of 16 in 64..65536"), ((72, 2, 4), "slice_bytes 72 is not a multiple of 16 in 64..65536"),
                            ((65552, 2, 4), "slice_bytes 65552 is not a multiple of 16 in 64..65536"), ((64, 33, 4), "parity 33 is not in 1..32"),
                            ((64, 32, 225), "group_data 225 is not in 1..256 - parity"), ((64, 1, 256), "group_data 256 is not in 1..256 - parity")]:
        got = _twin_build([BASE], S, r, K)[0]
        assert (got.code, got.message, got.out) == (rt.INVALID, "[recovery-error] " + text, None)
    assert _twin_build([BASE], 65536, 32, 224)[0].code == rt.OK and _twin_build([BASE], 64, 1, 255)[0].code == rt.OK


# ---- the parser -----------------------------------------------------------------------------------------------------------
def _parse_both(side):
    info, msg = rt.Info(), C.create_string_buffer(512)
    rc = rt.lib().sim_recovery_parse(side, len(side), C.byref(info), msg, 512)
    try:
        rt.parse(side)
        twin = ""
    except rt.Refused as e:
        twin = str(e)
    assert msg.value.decode() == twin and (rc == 0) == (twin == "")
    return twin


def test_every_refusal_of_the_parser():
    S, r, K = 64, 2, 4
    side = rt.build(BASE, S, r, K)
    geo = rt.geometry(len(BASE), S, r, K)
    table = list(struct.unpack(">%dI" % geo.k, side[36:36 + 4 * geo.k]))
    assert _parse_both(side) == ""
    flip = lambda at: side[:at] + bytes([side[at] ^ 1]) + side[at + 1:]  # noqa: E731
    cases = {
        "short input": side[:39],
        "wrong magic": b"LACM" + side[4:],
        "unsupported version: 2": rt.rehead(side, version=2),
        "checksum of the header differs": flip(13),
        "slice_bytes 0 is not a multiple of 16 in 64..65536": rt.rehead(side, S=0),
        "slice_bytes 72 is not a multiple of 16 in 64..65536": rt.rehead(side, S=72),
        "slice_bytes 131072 is not a multiple of 16 in 64..65536": rt.rehead(side, S=131072),
        "parity 0 is not in 1..32": rt.rehead(side, r=0),
        "parity 33 is not in 1..32": rt.rehead(side, r=33),
        "group_data 0 is not in 1..256 - parity": rt.rehead(side, K=0),
        "group_data 255 is not in 1..256 - parity": rt.rehead(side, K=255),
        "file_bytes is 0": rt.rehead(side, L=0),
        "the file needs %d slices, 2^28 or more" % (1 << 28): rt.rehead(side, L=64 << 28),
        "slices %d, file_bytes and slice_bytes give %d" % (geo.k + 1, geo.k): rt.rehead(side, k=geo.k + 1),
        "slices %d, file_bytes and slice_bytes give %d" % (geo.k, geo.k + 1): rt.rehead(side, L=len(BASE) + 64),
        "groups %d, slices and group_data give %d" % (geo.G + 1, geo.G): rt.rehead(side, G=geo.G + 1),
        "slice table is cut short": side[:40 + 4 * geo.k - 1],
        "checksum of the slice table differs": flip(36 + 9),
        # rewritten consistently, but wrongly: both head checksums are right and the combine rule still refuses it
        "file_crc32 is not the combination of the slice checksums": rt.rehead(side, file_crc=zlib.crc32(BASE) ^ 1),
    }
    for text, bad in cases.items():
        assert _parse_both(bad) == "[recovery-error] " + text, text
    assert _parse_both(rt.rehead(side, table=[table[0] ^ 4] + table[1:])) == "[recovery-error] file_crc32 is not the combination of the slice checksums"
    assert _parse_both(side[:40 + 4 * geo.k]) == "" and _parse_both(side + b"xyz") == ""  # the parity area is nobody's business here
    # a refused sidecar fails its item, in scan and in repair, and the others go on
    for scan_only in (False, True):
        a, b = rt.outcomes(rt.repair_case([BASE, BASE], [cases["wrong magic"], side], scan_only=scan_only))
        assert (a.code, a.message, a.result, a.out) == (rt.INVALID, "[recovery-error] wrong magic", rt.ZERO, None)
        assert b.code == rt.OK and (scan_only or b.out == BASE)


# ---- repair ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def repair_jobs():
    """[(name, case, [expected Outcome])]: every job of the repair tests, the expectation from recoverytwin alone."""
    jobs = []

    def add(name, files, sides, best_effort=False, scan_only=False):
        want = [rt.scan(f, s) if scan_only else rt.repair(f, s, best_effort) for f, s in zip(files, sides)]
        jobs.append((name, rt.repair_case(files, sides, best_effort, scan_only), want))
        return want

    for S, r, K in SMALL_SETS:
        tag = "S%d r%d K%d " % (S, r, K)
        side = rt.build(BASE, S, r, K)
        geo = rt.geometry(len(BASE), S, r, K)
        full = len(side)
        # every single lost slice, and the intact file
        files = [BASE] + [_hit(BASE, S, [s]) for s in range(geo.k)]
        want = add(tag + "single", files, [side] * len(files))
        assert all(w.code == rt.OK and w.out == BASE for w in want) and [w.bad for w in want[1:]] == [[s] for s in range(geo.k)]
        add(tag + "single scan", files, [side] * len(files), scan_only=True)
        # every b-subset of a group, b <= r: groups 0 (the most members) and G - 1 (the fewest)
        for g in (0, geo.G - 1):
            subsets = [c for b in range(1, r + 1) for c in itertools.combinations(rt.members(geo, g), b)]
            want = add(tag + "subsets of group %d" % g, [_hit(BASE, S, c) for c in subsets], [side] * len(subsets))
            assert all(w.code == rt.OK and w.out == BASE and w.result[3] == len(c) for w, c in zip(want, subsets))
            # b = r + 1: refused, naming the group and the counts; best effort gives the rest
            beyond = [c for c in itertools.combinations(rt.members(geo, g), r + 1)]
            other = (g + 1) % geo.G
            files = [_hit(BASE, S, list(c) + [other]) for c in beyond]
            want = add(tag + "beyond group %d" % g, files, [side] * len(files))
            assert all((w.code, w.message, w.out) == (rt.MISMATCH, "[recovery-error] group %d: %d damaged slices, %d parity slices usable" % (g, r + 1, r), None)
                       and w.result[10] & rt.UNREPAIRED for w in want)
            want = add(tag + "beyond group %d best effort" % g, files, [side] * len(files), best_effort=True)
            for w, c, f in zip(want, beyond, files):
                assert w.code == rt.MISMATCH and w.result[3] == 1 and w.result[10] & rt.UNREPAIRED
                assert w.out == _hit(BASE, S, c) and w.out != f  # the other group's slice is back, this group's are as found
            add(tag + "beyond group %d scan" % g, files, [side] * len(files), scan_only=True)
        # lost data plus lost parity: the lowest usable rows are not rows 0 .. b - 1
        mem = rt.members(geo, 1)
        files, sides = [], []
        for b in range(1, r + 1):
            for gone in itertools.combinations(range(r), r - b):  # exactly b parity records stay usable
                files.append(_hit(BASE, S, mem[:b]))
                sides.append(_hit_parity(side, geo, [1 * r + p for p in gone]))
        want = add(tag + "data and parity", files, sides)
        assert all(w.code == rt.OK and w.out == BASE for w in want) and any(w.result[6] for w in want)
        files = [_hit(BASE, S, mem[:r])]
        want = add(tag + "one parity too few", files, [_hit_parity(side, geo, [r])])
        assert want[0].message == "[recovery-error] group 1: %d damaged slices, %d parity slices usable" % (r, r - 1)
        # a burst of r * G slices at every start
        n = r * geo.G
        files = [BASE[:a * S] + _bytes(min(len(BASE), (a + n) * S) - a * S, a) + BASE[(a + n) * S:] for a in range(geo.k - n + 1)]
        want = add(tag + "burst", files, [side] * len(files))
        assert all(w.code == rt.OK and w.out == BASE and w.result[2] >= n - 1 for w in want)
        # truncation at every slice border and one byte to either side, and trailing bytes
        cuts = sorted({c for s in range(geo.k + 1) for c in (s * S - 1, s * S, s * S + 1) if 0 <= c <= len(BASE) - 1})
        want = add(tag + "truncation", [BASE[:c] for c in cuts], [side] * len(cuts))
        assert all(w.result[10] & rt.TRUNCATED for w in want) and {w.code for w in want} == {rt.OK, rt.MISMATCH}
        assert all(w.out == BASE for w in want if w.code == rt.OK)
        add(tag + "truncation scan", [BASE[:c] for c in cuts], [side] * len(cuts), scan_only=True)
        want = add(tag + "trailing", [BASE + b"tail", _hit(BASE, S, [2]) + b"\0" * 70], [side, side])
        assert all(w.code == rt.OK and w.out == BASE and w.result[10] == rt.TRAILING for w in want)
        # a sidecar cut inside and between parity records: the records that are whole still count
        at = 40 + 4 * geo.k
        cuts = [at, at + 1, at + S, at + S + 3, at + S + 4, at + S + 5, at + r * (S + 4), at + r * (S + 4) + S + 3, full - (S + 4), full - 1]
        files = [_hit(BASE, S, [0, geo.G + 1])] * len(cuts)  # one slice in group 0, one in group 1
        want = add(tag + "short sidecar", files, [side[:c] for c in cuts])
        assert all(w.result[10] & rt.SIDECAR_TRUNCATED for w in want) and {w.code for w in want} == {rt.OK, rt.MISMATCH}
        add(tag + "short sidecar best effort", files, [side[:c] for c in cuts], best_effort=True)
        # a damaged head is refused
        heads = [side[:at_] + bytes([side[at_] ^ 0x80]) + side[at_ + 1:] for at_ in (0, 4, 5, 9, 19, 23, 27, 31, 33, 36, 36 + 4 * geo.k - 1, 36 + 4 * geo.k + 2)]
        want = add(tag + "damaged head", [BASE] * len(heads), heads)
        assert all(w.code == rt.INVALID and w.message.startswith("[recovery-error] ") and w.out is None for w in want)
        # the checksum mismatch: the table entry of a damaged slice forged to that slice's own CRC (both head checksums and
        # file_crc32 made consistent): the slice passes as good, its group's other lost slice is rebuilt from it -- wrongly
        a, b = mem[0], mem[1]
        hurt = _hit(BASE, S, [a, b])
        table = list(struct.unpack(">%dI" % geo.k, side[36:36 + 4 * geo.k]))
        table[a] = zlib.crc32(hurt[a * S:(a + 1) * S])
        forged = rt.rehead(side, table=table, file_crc=zlib.crc32(_hit(BASE, S, [a])))
        want = add(tag + "checksum mismatch", [hurt, hurt], [forged, side])
        assert (want[0].code, want[0].message, want[0].out, want[0].bad) == (rt.MISMATCH, "[recovery-error] repaired file does not match its checksum", None, [b])
        assert want[1].code == rt.OK and want[1].out == BASE
        add(tag + "checksum mismatch best effort", [hurt], [forged], best_effort=True)
    # the other parameter sets, on a stream with uneven groups: a burst, a cut, lost parity, beyond capacity
    big = FIXTURES["n16421_st16"]
    for S, r, K in [(64, 1, 1), (256, 4, 16), (4096, 8, 128), (64, 32, 224)]:
        side = rt.build(big, S, r, K)
        geo = rt.geometry(len(big), S, r, K)
        n = r * geo.G
        burst = big[:S] + _bytes(min(n * S, len(big) - S), S) + big[S + n * S:]
        files = [big, burst, big[:len(big) - n * S + S - 1], _hit(big, S, rt.members(geo, 0)[:r + 1]) if len(rt.members(geo, 0)) > r else big[:7]]
        sides = [side, side, _hit_parity(side, geo, [n - 1]), side]
        for best in (False, True):
            add("S%d r%d K%d mixed%s" % (S, r, K, " best effort" if best else ""), files, sides, best_effort=best)
    return jobs


def _same(name, got, want):
    assert len(got) == len(want), name
    for i, (g, w) in enumerate(zip(got, want)):
        assert (g.code, g.message, g.result, g.bad) == (w.code, w.message, w.result, w.bad), (name, i)
        assert g.out == w.out, (name, i)


def test_repair_cases():
    """Every single lost slice, every b-subset of a group for b <= r, b = r + 1 refused with the group and the counts, lost
    data plus lost parity, a burst of r * G slices at every start, truncation at every slice border and a byte to either
    side, trailing bytes, a sidecar cut inside and between parity records, a damaged head, the constructed checksum
    mismatch and best effort: the twin answers as the restatement does, item by item."""
    jobs = repair_jobs()
    for name, case, want in jobs:
        _same(name, rt.outcomes(case), want)
    assert len(jobs) >= 40 and sum(len(w) for _, _, w in jobs) > 500


def test_the_burst_of_the_issue():
    """n16421_st16 with S = 256, r = 4, K = 16: 167 slices in 11 groups, any 44 consecutive slices come back."""
    data = FIXTURES["n16421_st16"]
    geo = rt.geometry(len(data), 256, 4, 16)
    assert (len(data), geo.k, geo.G) == (42652, 167, 11)
    side = rt.build(data, 256, 4, 16)
    hurt = data[:5 * 256] + bytes(44 * 256) + data[49 * 256:]
    got = rt.outcomes(rt.repair_case([hurt], [side]))[0]
    assert got.code == rt.OK and got.out == data and got.bad == list(range(5, 49)) and got.result[3] == 44
    longest = (4 * 11 - 1) * 256 + 1  # a byte range of this length touches at most r * G slices wherever it starts
    hurt = data[:300] + bytes(b ^ 0xFF for b in data[300:300 + longest]) + data[300 + longest:]
    assert rt.outcomes(rt.repair_case([hurt], [side]))[0].out == data


def test_sanitized_run():
    """The same jobs, and the builds of every golden stream, as a program under AddressSanitizer + UBSan with every buffer
    at exactly the plan's capacity: no report, and the plain build's answers byte for byte."""
    exe, why = rt.sanitized_exe()
    if exe is None:
        pytest.skip(why)
    names = sorted(FIXTURES)
    cases = [case for _, case, _ in repair_jobs()] + [rt.build_case([FIXTURES[n] for n in names], S, r, K) for S, r, K in rt.SETS]
    cases.append(rt.build_case([BASE], 0, 0, 0))
    lines, rc, err = rt.run_sanitized(cases, exe)
    assert rc == 0, err
    for i, c in enumerate(cases):
        assert lines[i] is not None and lines[i].split(" ", 1)[1] == rt.digest_line(rt.answer(c)), i
