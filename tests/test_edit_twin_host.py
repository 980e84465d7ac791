"""The edit pass's CPU twin (tests/native/sim_edit.cpp over csrc/edit_core.h) against numpy: every channel operation at both
depths and both depth changes, output lengths around a quad and a unit, the first violation in every place a thread can
meet it, on heap blocks of exactly the planned sizes -- plain and as a stand-alone program under AddressSanitizer + UBSan."""
import struct

import numpy as np
import pytest

import editcases as E
import twinbuild
import wavutil

SRC = twinbuild.NATIVE + "/sim_edit.cpp"
CLEAN = (1 << 64) - 1
LENGTHS = (1, 2, 3, 4, 5, 1023, 1024, 1025, 4097)
STEREO_OPS, MONO_OPS = (E.KEEP, E.LEFT, E.RIGHT, E.FOLD, E.SWAP), (E.KEEP, E.DUAL)


def _pcm(rng, n, depth, step=1):
    lim = 1 << (depth - 1)
    return (rng.integers(-lim // step, lim // step, n, dtype=np.int64) * step).astype(np.int32)


class Case:
    def __init__(self, left, right, depth, op, to_depth):
        self.left, self.right, self.depth, self.op, self.to = left, right, depth, op, to_depth

    def blob(self):
        rows = self.left.astype("<i4").tobytes() + (b"" if self.right is None else self.right.astype("<i4").tobytes())
        return struct.pack("<4IQ", 1 if self.right is None else 2, self.op, self.depth, self.to, self.left.size) + rows

    def expected(self):
        """(key, destination bytes) by numpy: the lowest frame * 4 + kind (0 differ, 1 left / 2 right no multiple of 256)."""
        keys = []
        if self.op == E.FOLD:
            keys += [4 * int(f) for f in np.flatnonzero(self.left != self.right)[:1]]
        l, r, depth, error = E.apply(self.left, self.right, self.depth, self.op, self.to)
        if self.depth == 24 and self.to == 16:
            ol, orr, _, _ = E.apply(self.left, self.right, self.depth, self.op, 24)
            keys += [4 * int(f) + 1 for f in np.flatnonzero(ol & 0xFF)[:1]]
            if orr is not None:
                keys += [4 * int(f) + 2 for f in np.flatnonzero(orr & 0xFF)[:1]]
        key = min(keys) if keys else CLEAN
        assert (error is None) == (key == CLEAN)
        if error:  # the words the product makes of the key name the same frame and channel
            kind = ("", " left sample", " right sample")[key & 3]
            assert error.startswith(f"[transcode-error] frame {key >> 2}{':' if key & 3 == 0 else kind}")
        return key, wavutil.pcm_bytes(l, r, depth)


def grid():
    rng = np.random.default_rng(20260)
    out = []
    for n in LENGTHS:
        for depth in (16, 24):
            for to in (16, 24):
                step = 256 if (depth, to) == (24, 16) else 1
                for op in STEREO_OPS:
                    left = _pcm(rng, n, depth, step)
                    out.append(Case(left, left.copy() if op == E.FOLD else _pcm(rng, n, depth, step), depth, op, to))
                for op in MONO_OPS:
                    out.append(Case(_pcm(rng, n, depth, step), None, depth, op, to))
    return out


def violations():
    """The first violation in frame 0, off a multiple of 4, in the last partial quad, in the last frame of a unit; two
    violations; left and right in one frame; a difference and a narrowing violation in one frame."""
    rng = np.random.default_rng(20261)
    out = []
    for n, places in ((4097, (0, 5, 1023, 2047, 4096)), (1025, (1022, 1024)), (3, (2,)), (1, (0,)), (1023, (1020, 1022))):
        for at in places:
            later = [f for f in (at + 1, at + 3, n - 1) if at < f < n][:1]
            for op in (E.KEEP, E.SWAP, E.RIGHT, E.LEFT):  # narrowing: left only, right only, both in the frame
                for which in ((0,), (1,), (0, 1)):
                    rows = [_pcm(rng, n, 24, 256), _pcm(rng, n, 24, 256)]
                    for w in which:
                        rows[w][at] |= 1 + int(rng.integers(0, 255))
                        for f in later:
                            rows[1 - w][f] |= 0x80
                    out.append(Case(rows[0], rows[1], 24, op, 16))
            for to in (16, 24):  # FOLD: a difference, alone and with a narrowing violation in the same and in an earlier frame
                left = _pcm(rng, n, 24, 256 if to == 16 else 1)
                right = left.copy()
                right[at] ^= 0x100
                for f in later:
                    right[f] ^= 0x200
                out.append(Case(left, right, 24, E.FOLD, to))
                if to == 16:
                    both = Case(left.copy(), right.copy(), 24, E.FOLD, 16)
                    both.left[at] |= 3
                    out.append(both)
                    if at:
                        early = Case(left.copy(), right.copy(), 24, E.FOLD, 16)
                        early.left[at - 1] |= 1
                        early.right[at - 1] |= 1
                        out.append(early)
            mono = _pcm(rng, n, 24, 256)
            mono[at] += 1
            out += [Case(mono, None, 24, E.KEEP, 16), Case(mono.copy(), None, 24, E.DUAL, 16)]
    return out


@pytest.fixture(scope="module")
def corpus():
    return grid() + violations()


def _answers(exe, cases, env=None):
    lines, rc, err = twinbuild.run_cases(exe, [c.blob() for c in cases], env or {}, prefix="edit_cases_")
    assert rc == 0, err
    out = []
    for i, t in enumerate(lines):
        index, key, intact, *hexed = t.split(" ")
        assert int(index) == i and intact == "1", (i, "guard bytes behind the destination were written, or two runs differ")
        out.append((int(key), bytes.fromhex(hexed[0] if hexed else "")))
    return out


@pytest.fixture(scope="module")
def plain(corpus):
    return _answers(twinbuild.program("sim_edit", [SRC], ["-O2", "-std=c++20"]), corpus)


def test_twin_matches_numpy(corpus, plain):
    assert len(plain) == len(corpus)
    kinds = set()
    for i, (c, (key, dst)) in enumerate(zip(corpus, plain)):
        want_key, want_dst = c.expected()
        assert key == want_key, (i, c.op, c.depth, c.to, c.left.size)
        assert dst == want_dst, (i, c.op, c.depth, c.to, c.left.size)
        kinds.add(CLEAN if key == CLEAN else key & 3)
    assert kinds == {CLEAN, 0, 1, 2}


def test_left_comes_before_right_and_the_lowest_frame_wins(corpus, plain):
    seen = 0
    for c, (key, _) in zip(corpus, plain):
        if c.right is None or c.op not in (E.KEEP, E.SWAP) or (c.depth, c.to) != (24, 16) or key == CLEAN:
            continue
        l, r, _, _ = E.apply(c.left, c.right, 24, c.op, 24)
        f = key >> 2
        assert not (l[:f] & 0xFF).any() and not (r[:f] & 0xFF).any()
        if (l[f] & 0xFF) and (r[f] & 0xFF):
            assert key & 3 == 1
            seen += 1
    assert seen >= 8


def test_sanitized_twin_reports_nothing(corpus, plain):
    exe, why = twinbuild.sanitized_exe("sim_edit_san", [SRC])
    if exe is None:
        pytest.skip(why)
    env = dict(ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    assert _answers(exe, corpus, env) == plain
