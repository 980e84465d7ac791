"""verify_unit / verify_fill_item of csrc/verify_core.h on the host (tests/native/sim_verify.cpp), plain and under
AddressSanitizer + UBSan: whole items in every layout, at every base alignment the layout permits, in source buffers
that end exactly where the source ends, against a numpy brute force.  Frames 1 .. 16 384 + 37, mono and stereo, both
depths, one block and two blocks (the first of 257 frames, the two MS flags different, so that a unit spans the
boundary), and every placement of a difference that the device tests use."""
import numpy as np
import pytest

import vertwin as V

FRAMES = (1, 2, 3, 4, 5, 255, 256, 257, 258, 261, 16384 + 37)
OFFSETS = {V.PLANAR: (0, 4, 8, 12), V.I16: (0, 4), V.I24: (0, 1, 2, 3)}


def _pcm(frames, channels, bit_depth, seed):
    rng = np.random.default_rng(seed)
    lo, hi = (-32768, 32767) if bit_depth == 16 else (-0x800000, 0x7FFFFF)
    left = rng.integers(lo, hi + 1, frames, dtype=np.int64)
    left[:min(frames, 3)] = (lo, hi, -1)[:min(frames, 3)]  # the range's ends, where the mid/side inverse is widest
    right = rng.integers(lo, hi + 1, frames, dtype=np.int64) if channels == 2 else None
    if right is not None:
        right[:min(frames, 3)] = (hi, lo, 0)[:min(frames, 3)]
    return left.astype(np.int32), None if right is None else right.astype(np.int32)


def _other(v, bit_depth):
    """A value of the depth that differs from v."""
    return int(v) - 1 if int(v) > 0 else int(v) + 1


def _groups(case_left, case_right, frames, channels, bit_depth, layout, block_frames):
    L, R = case_left, case_right
    last = frames - 1
    groups = [[], [(0, 0, _other(L[0], bit_depth))], [(last, channels - 1, _other((R if channels == 2 else L)[last], bit_depth))]]
    if len(block_frames) == 2:
        b = block_frames[0]
        groups.append([(b - 1, 0, _other(L[b - 1], bit_depth))])             # the last frame of block 0
        groups.append([(b, channels - 1, _other((R if channels == 2 else L)[b], bit_depth))])  # the first frame of block 1
        groups.append([(b - 1, channels - 1, 5), (b, 0, 6), (b + 1, 0, 7)] if frames > b + 1 else [(b - 1, 0, 5), (b, 0, 6)])
    mid = frames // 2
    if channels == 2:  # both channels of one frame: channel 0 is reported, the count is 2
        groups.append([(mid, 0, _other(L[mid], bit_depth)), (mid, 1, _other(R[mid], bit_depth))])
        groups.append([(mid, 1, _other(R[mid], bit_depth))])  # the right channel alone
    if frames >= 2:  # two differing frames: the lower is reported
        groups.append([(last, 0, _other(L[last], bit_depth)), (frames // 3, 0, _other(L[frames // 3], bit_depth))])
    if bit_depth == 24:  # only the top byte, only the low byte
        groups.append([(mid, 0, int(L[mid]) ^ 0x400000)])
        if layout == V.I24:  # ... and its sign bit (wrapped to the depth below)
            groups.append([(mid, 0, int(L[mid]) ^ 0x800000)])
        groups.append([(mid, 0, int(L[mid]) ^ 0x01)])
    if layout == V.PLANAR:  # equal modulo 2^24 is not equal
        groups.append([(mid, 0, int(L[mid]) + (1 << 24))])
        groups.append([(last, channels - 1, int((R if channels == 2 else L)[last]) - (1 << 24))])
    groups.append(V.ALL_DIFFERENT)
    return groups


def _cases():
    cases, seed = [], 0
    for frames in FRAMES:
        for channels in (1, 2):
            for bit_depth, layout in ((16, V.PLANAR), (16, V.I16), (24, V.PLANAR), (24, V.I24)):
                tables = [([frames], [0]), ([frames], [1])] if channels == 2 else [([frames], [0])]
                if frames > 257:
                    tables += [([257, frames - 257], [0, 1]), ([257, frames - 257], [1, 0])] if channels == 2 else \
                              [([257, frames - 257], [0, 0])]
                for block_frames, ms in tables:
                    seed += 1
                    left, right = _pcm(frames, channels, bit_depth, seed)
                    groups = _groups(left, right, frames, channels, bit_depth, layout, block_frames)
                    groups = [g if g == V.ALL_DIFFERENT else [(f, c, _wrap(v, bit_depth, layout)) for f, c, v in g] for g in groups]
                    cases.append(V.Case(channels, bit_depth, layout, block_frames, ms, [0] * len(block_frames), left, right,
                                        OFFSETS[layout], groups))
    # only blocks with status 0 are compared: differences in both blocks, the second one did not decode (and the reverse)
    left, right = _pcm(300, 2, 16, 999)
    edits = [[(10, 1, _other(right[10], 16)), (256, 0, _other(left[256], 16)), (257, 0, _other(left[257], 16)), (299, 1, _other(right[299], 16))],
             V.ALL_DIFFERENT]
    for status in ([0, 3], [8, 0], [5, 7]):
        cases.append(V.Case(2, 16, V.I16, [257, 43], [1, 0], status, left, right, OFFSETS[V.I16], edits))
    return cases


def _wrap(v, bit_depth, layout):
    """An interleaved layout holds a value of the depth; a planar array any int32."""
    if layout == V.PLANAR:
        return v
    bits = bit_depth
    v &= (1 << bits) - 1
    return v - (1 << bits) if v >> (bits - 1) else v


@pytest.fixture(scope="module")
def cases():
    return _cases()


@pytest.fixture(scope="module")
def expected(cases):
    out = {}
    for i, case in enumerate(cases):
        for (off, grp), line in case.expected().items():
            out[(i, off, grp)] = line
    return out


def test_the_brute_force_sees_what_the_cases_intend(cases, expected):
    """The expectations themselves: the placements give the counts and positions they were built for."""
    assert len(cases) > 150 and len(expected) > 4000
    seen_two_block = seen_top = 0
    for i, case in enumerate(cases):
        off = case.offsets[0]
        assert expected[(i, off, 0)] == V.Line(0, V.NO_KEY, 0, 0, 0, tuple(case.status)) or any(case.status)
        if not any(case.status):
            assert expected[(i, off, 1)][:2] == (1, 0)  # the first frame, the left channel
            assert expected[(i, off, 2)][:2] == (1, 2 * (case.frames - 1) + case.channels - 1)
            assert expected[(i, off, len(case.groups) - 1)].mismatches == case.frames * case.channels
            if len(case.block_frames) == 2:
                seen_two_block += 1
                assert expected[(i, off, 3)].key == 2 * 256 and expected[(i, off, 3)].block == 0
                assert expected[(i, off, 4)].key == 2 * 257 + case.channels - 1 and expected[(i, off, 4)].block == 1
            if case.layout == V.PLANAR:
                g = len(case.groups) - 3
                e = expected[(i, off, g)]
                assert e.mismatches == 1 and e.source - e.decoded == 1 << 24
                seen_top += 1
    assert seen_two_block >= 24 and seen_top >= 40
    # a block that did not decode is not compared
    tail = {tuple(c.status): i for i, c in enumerate(cases) if any(c.status)}
    assert expected[(tail[(0, 3)], 0, 0)][:2] == (2, 2 * 10 + 1) and expected[(tail[(0, 3)], 0, 1)].mismatches == 2 * 257
    assert expected[(tail[(8, 0)], 0, 0)][:2] == (2, 2 * 257) and expected[(tail[(8, 0)], 0, 0)].block == 1
    assert expected[(tail[(5, 7)], 4, 1)] == V.Line(0, V.NO_KEY, 0, 0, 0, (5, 7))


def test_twin_against_brute_force(cases, expected):
    got = V.run_plain(cases)
    assert set(got) == set(expected)
    wrong = [(k, got[k], expected[k]) for k in sorted(expected) if got[k] != expected[k]]
    assert not wrong, wrong[:5]


def test_sanitized_twin_prints_the_same(cases, expected):
    exe, why = V.sanitized_exe()
    if exe is None:
        pytest.skip(why)
    lines, rc, err = V.run_sanitized(cases, exe)
    assert rc == 0, err
    assert lines == V.run_plain(cases) == expected
