"""crc32_core.h and digest_core.h on the host (tests/native/sim_digest.cpp), plain and under AddressSanitizer + UBSan.
The GF(2) arithmetic against big-integer polynomial powers and zlib; the unit against zlib.crc32 of numpy-built data
bytes: every layout, mono and stereo, both depths, every base offset the layout permits in source buffers that end
exactly where the source ends, frame counts around the unit and the wave border, constant audio, blocks of odd lengths
with alternating mid/side flags, and a block that did not decode."""
import os
import random
import zlib

import numpy as np
import pytest

import digesttwin as D
import wavutil as W

M32 = (1 << 32) - 1


@pytest.fixture(scope="module")
def unit():
    u, t = D.unit_frames(), D.threads()
    assert (u, t) == (4, 256)  # the loads of wav_pack_unit / verify_unit; k_verify's workgroup
    return u


def _distances():
    out = {0, 1, 2, 3}
    for k in range(1, 41):
        out |= {(1 << k) - 1, 1 << k, (1 << k) + 1}
    for m in (1, 2, 3, 1 << 8, (1 << 28) + 5):  # around multiples of the multiplicative order of x
        out |= {m * M32 - 1, m * M32, m * M32 + 1}
    return sorted(out)


def test_shift_against_big_integer_powers():
    rng = random.Random(5)
    assert D.poly_xpow(M32) == 1 and all(D.poly_xpow(M32 // q) != 1 for q in (3, 5, 17, 257, 65537))  # P is primitive
    for n in _distances():
        for r in (0x80000000, 0xFFFFFFFF, 1, rng.getrandbits(32)):
            assert D.shift(r, n) == D.shift_ref(r, n), (r, n)
    assert D.shift(0x12345678, 0) == 0x12345678 and D.shift(0x12345678, M32) == 0x12345678
    assert D.shift(0, 12345) == 0
    for _ in range(50):  # the multiply itself: commutative, and against the big-integer product
        a, b = rng.getrandbits(32), rng.getrandbits(32)
        want = D._bitrev32(D.poly_mul(D._bitrev32(a), D._bitrev32(b)))
        assert D.mul(a, b) == D.mul(b, a) == want


def test_shift_is_what_zero_bytes_do():
    """raw(M || 0^n) = shift(raw(M), n), with zlib as the register: crc32 with init 0 and no final xor is crc32(M, ~0) ^ ~0."""
    rng = random.Random(6)
    for n in (0, 1, 7, 8, 24, 255, 4096, 100003):
        m = rng.randbytes(rng.randrange(1, 40))
        raw = zlib.crc32(m, M32) ^ M32
        assert D.shift(raw, n) == zlib.crc32(m + bytes(n), M32) ^ M32, n


def test_combine_against_zlib():
    rng = random.Random(7)
    for _ in range(300):
        m = rng.randbytes(rng.choice((0, 1, 2, 3, 24, 25, 1000, 70001)))
        cut = rng.randrange(0, len(m) + 1) if rng.random() < 0.8 else rng.choice((0, len(m)))  # empty halves included
        a, b = m[:cut], m[cut:]
        assert D.combine(zlib.crc32(a), zlib.crc32(b), len(b)) == zlib.crc32(m), (len(a), len(b))
    assert D.combine(0, 0, 0) == 0 and D.combine(zlib.crc32(b"abc"), 0, 0) == zlib.crc32(b"abc")
    # three parts, as the WAV image is put together: header, data, pad
    h, d = rng.randbytes(44), rng.randbytes(999)
    assert D.combine(D.combine(zlib.crc32(h), zlib.crc32(d), len(d)), zlib.crc32(b"\0"), 1) == zlib.crc32(h + d + b"\0")


def test_wav_header_crc():
    for ch, bits, rate, frames in ((1, 16, 44100, 1), (2, 16, 48000, 28_800_000), (1, 24, 96000, 333), (2, 24, 192000, 16421),
                                   (1, 16, 48000, (1 << 31) - 100)):
        z = np.zeros(min(frames, 8), dtype=np.int32)
        data = frames * ch * bits // 8
        header = bytearray(W.make_wav(z, z if ch == 2 else None, rate, bits)[:44])
        header[4:8] = (36 + data + (data & 1)).to_bytes(4, "little")
        header[40:44] = data.to_bytes(4, "little")
        assert D.wav_header_crc(ch, bits, rate, data) == zlib.crc32(bytes(header)), (ch, bits, rate, frames)


def _pcm(frames, channels, bit_depth, seed):
    rng = np.random.default_rng(seed)
    lo, hi = (-32768, 32767) if bit_depth == 16 else (-0x800000, 0x7FFFFF)
    left = rng.integers(lo, hi + 1, frames, dtype=np.int64)
    left[:min(frames, 3)] = (lo, hi, -1)[:min(frames, 3)]  # the range's ends, where the mid/side inverse is widest
    right = rng.integers(lo, hi + 1, frames, dtype=np.int64) if channels == 2 else None
    if right is not None:
        right[:min(frames, 3)] = (hi, lo, 0)[:min(frames, 3)]
    return left.astype(np.int32), None if right is None else right.astype(np.int32)


def _cases(unit):
    cases, seed = [], 0
    sizes = list(range(1, 10)) + [unit * 64 - 1, unit * 64, unit * 64 + 1]
    for channels in (1, 2):
        for bit_depth in (16, 24):
            for layout in D.LAYOUTS[bit_depth]:
                for frames in sizes:
                    seed += 1
                    left, right = _pcm(frames, channels, bit_depth, seed)
                    ms = [seed & 1] if channels == 2 else [0]
                    cases.append(D.Case(channels, bit_depth, layout, [frames], ms, [0], left, right))
                # constant audio: all-zero bytes and all-0xFF bytes (every sample -1)
                for value in (0, -1):
                    frames = unit * 64 + 3
                    x = np.full(frames, value, dtype=np.int32)
                    cases.append(D.Case(channels, bit_depth, layout, [frames], [0], [0], x, x if channels == 2 else None))
                # mid/side and left/right blocks alternating, odd non-final block lengths: units span the boundaries;
                # 2 * 64 units and more, so that the tree and the per-unit path both take part
                lens = [257, 301, 259, 43]
                left, right = _pcm(sum(lens), channels, bit_depth, 1000 + seed)
                flags = [1, 0, 1, 0] if channels == 2 else [0, 0, 0, 0]
                cases.append(D.Case(channels, bit_depth, layout, lens, flags, [0] * 4, left, right))
                # a block that did not decode is excluded (its frames enter the stream form as zeros)
                for status in ([0, 3, 0, 0], [8, 0, 0, 5]):
                    cases.append(D.Case(channels, bit_depth, layout, lens, flags, status, left, right))
    return cases


@pytest.fixture(scope="module")
def cases(unit):
    return _cases(unit)


@pytest.fixture(scope="module")
def expected(cases):
    out = {}
    for i, case in enumerate(cases):
        for off, line in case.expected().items():
            out[(i, off)] = line
    return out


def test_the_cases_cover_what_they_intend(cases, expected, unit):
    assert {c.layout for c in cases} == {D.P32, D.I16, D.I24, D.P16, D.PF32, D.IF32}
    assert {(c.channels, c.bit_depth) for c in cases} == {(1, 16), (2, 16), (1, 24), (2, 24)}
    assert {c.frames for c in cases} >= set(range(1, 10)) | {unit * 64 - 1, unit * 64, unit * 64 + 1}
    assert len(cases) > 250 and len(expected) > 900
    for c in cases:  # every offset keeps the layout's element alignment, and the narrow load paths are all there
        elem = {D.I24: 1, D.I16: 4, D.P16: 2}.get(c.layout, 4)
        assert all(o % elem == 0 for o in c.offsets) and len(c.offsets) >= 2
    excluded = [c for c in cases if any(c.status)]
    assert excluded and all(c.data_bytes(True) != c.data_bytes(False) for c in excluded)
    consts = [c for c in cases if c.frames == unit * 64 + 3 and len(c.block_frames) == 1]
    assert {bytes(set(c.data_bytes(False))) for c in consts} == {b"\x00", b"\xff"}


def test_twin_against_zlib(cases, expected):
    got = D.run_plain(cases)
    assert set(got) == set(expected)
    wrong = [(k, got[k], expected[k]) for k in sorted(expected) if got[k] != expected[k]]
    assert not wrong, wrong[:5]


def test_invalid_source_samples_lower_the_key(unit):
    """The source form's validation: all of left before right, then the lowest index; bit 0 tells the two kinds apart."""
    frames = unit * 64 + 2
    left, right = _pcm(frames, 2, 16, 77)

    def key(channel, frame, inexact):
        return (channel << 63) | (frame << 1) | inexact

    cases = []
    sl, sr = left.copy(), right.copy()
    sl[200], sr[5] = 40000, -40000  # planar int32 outside the depth: left is named although right's index is lower
    c = D.Case(2, 16, D.P32, [frames], [0], [0], left, right, src_left=sl, src_right=sr)
    c.source_key = key(0, 200, 0)
    cases.append(c)
    c = D.Case(2, 16, D.P32, [frames], [0], [0], left, right, src_right=sr)
    c.source_key = key(1, 5, 0)
    cases.append(c)
    fl, fr = D.source_elements(left, right, 16, D.PF32)
    for layout in (D.PF32, D.IF32):
        bl, br = fl.copy(), fr.copy()
        bl[frames - 1] = np.float32(0.5 + 2.0 ** -17).view(np.int32)  # off the 16-bit grid, in the partial last unit
        br[3] = np.float32(np.nan).view(np.int32)
        c = D.Case(2, 16, layout, [frames], [0], [0], left, right, src_left=bl, src_right=br)
        c.source_key = key(0, frames - 1, 1)
        cases.append(c)
        br2 = fr.copy()
        br2[3], br2[9] = np.float32(np.nan).view(np.int32), np.float32(1.0).view(np.int32)  # NaN; 1.0 is outside the depth
        c = D.Case(2, 16, layout, [frames], [0], [0], left, right, src_right=br2)
        c.source_key = key(1, 3, 1)
        cases.append(c)
    got = D.run_plain(cases)
    for i, c in enumerate(cases):
        for off in c.offsets:
            assert got[(i, off)].key == c.source_key, (i, off)
            assert got[(i, off)].decoded == zlib.crc32(c.data_bytes(True))  # the stream form does not look at the source


def test_sanitized_twin_prints_the_same(cases, expected):
    exe, why = D.sanitized_exe()
    if exe is None:
        pytest.skip(why)
    lines, rc, err = D.run_sanitized(cases, exe)
    assert rc == 0 and err == "", err
    assert lines == D.run_plain(cases) == expected
