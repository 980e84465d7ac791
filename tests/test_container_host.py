"""The .lac container (csrc/container.h: the version-3 writer, parse_stream) without a device: tests/native/sim_container.cpp
-- built from the header alone, with no ROCm include path, plain and as a stand-alone AddressSanitizer + UBSan program --
writes heads from rows and reads them back; the bytes are compared with the heads of the oracle's streams."""
import functools
import glob
import itertools
import json
import os
import subprocess

import numpy as np
import pytest

import twinbuild

ROOT = twinbuild.ROOT
SRC = os.path.join(twinbuild.NATIVE, "sim_container.cpp")
BLOCK = 16384


@functools.lru_cache(maxsize=None)
def _exe(sanitized):
    if sanitized:
        return twinbuild.sanitized_exe("sim_container_san", [SRC], ["-Wall", "-Werror"])
    return twinbuild.program("sim_container", [SRC], ["-std=c++20", "-Wall", "-Werror", "-O1"]), ""


@functools.lru_cache(maxsize=None)
def _run(commands):
    """The driver's answers to a tuple of command lines: the plain build's, which the sanitized program must repeat without
    a report."""
    exe, _ = _exe(False)
    text = "\n".join(commands) + "\n"
    plain = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert plain.returncode == 0, plain.stderr
    san, why = _exe(True)
    if san is not None:
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
        checked = subprocess.run([san], input=text, capture_output=True, text=True, env=env)
        assert checked.returncode == 0 and "ERROR" not in checked.stderr and "runtime error" not in checked.stderr, checked.stderr[-4000:]
        assert checked.stdout == plain.stdout
    out = [json.loads(line) for line in plain.stdout.splitlines()]
    assert len(out) == len(commands)
    return out


def test_the_sanitized_program_builds():
    exe, why = _exe(True)
    if exe is None:
        pytest.skip("sanitizer runtime not available: " + why)


def _split(lac):
    """Header fields, rows and head of a version-3 stream, read here with the layout as docs/format.md of the reference
    states it: 10-byte frame header, big-endian u32 block count, (u32 frames, u32 bytes) per block."""
    assert lac[:3] == b"LA\x03" and lac[9] == 0
    nb = int.from_bytes(lac[10:14], "big")
    head = 14 + 8 * nb
    rows = [int(v) for v in np.frombuffer(lac[14:head], dtype=">u4")]
    fields = dict(channels=lac[3], stereo_mode=lac[4], sample_rate=lac[5] << 8 | lac[6] | lac[7] << 16, bit_depth=lac[8])
    assert head + sum(rows[1::2]) == len(lac)
    return fields, rows, lac[:head]


def _write_cmd(f, rows, cuts=()):
    nb = len(rows) // 2
    return (f"write {f['sample_rate']} {f['bit_depth']} {f['channels']} {f['stereo_mode']} {nb} {len(cuts)} " +
            " ".join(map(str, list(cuts) + list(rows))))


def _check_written(got, f, rows, head=None):
    nb = len(rows) // 2
    assert got["ok"] == 1 and got["head_bytes"] == 14 + 8 * nb and got["rows"] == list(rows)
    if head is not None:
        assert bytes.fromhex(got["head"]) == head
    assert got["parse"] == dict(f, rc=0, why="", blocks=nb, frames=sum(rows[0::2]), version=3)


FORMATS = list(itertools.product((1, 2), (44100, 48000, 96000, 192000), (16, 24)))


@pytest.fixture(scope="module")
def oracle_streams(oracle):
    """One oracle stream per block count and format: 1, 2 and 3 blocks of a few hundred frames past the block boundary,
    513 blocks of silence (the head is what is compared; the stereo modes rotate over the stereo formats)."""
    out = []
    for nb in (1, 2, 3, 513):
        for i, (ch, sr, bd) in enumerate(FORMATS):
            frames = (nb - 1) * BLOCK + 300 + 7 * i
            if nb == 513:
                left = np.zeros(frames, np.int32)
                left[::4099] = 1 + i
            else:
                left = ((np.arange(frames, dtype=np.int64) * (37 + i)) % 2001 - 1000).astype(np.int32)
            right = (left[::-1] // 2).astype(np.int32).copy() if ch == 2 else None
            sm = i % 3 if ch == 2 else 0
            out.append((nb, oracle.encode(left, right, sr, bd, sm, threads=4)))
    return out


def test_heads_equal_the_oracles(oracle_streams):
    cases = [_split(lac) for _, lac in oracle_streams]
    assert sorted({len(rows) // 2 for _, rows, _ in cases}) == [1, 2, 3, 513]
    assert {(f["channels"], f["sample_rate"], f["bit_depth"]) for f, _, _ in cases} == set(FORMATS)
    assert {f["stereo_mode"] for f, _, _ in cases} == {0, 1, 2}
    for (f, rows, head), got in zip(cases, _run(tuple(_write_cmd(f, rows) for f, rows, _ in cases))):
        _check_written(got, f, rows, head)


def test_heads_equal_the_committed_streams():
    files = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "small", "*.lac")) +
                   glob.glob(os.path.join(ROOT, "tests", "golden", "decode_wav", "*.lac")))
    assert len(files) >= 15
    cases = [_split(open(p, "rb").read()) for p in files]
    for (f, rows, head), got in zip(cases, _run(tuple(_write_cmd(f, rows) for f, rows, _ in cases))):
        _check_written(got, f, rows, head)


def test_rows_written_in_slices_equal_rows_written_at_once(oracle_streams):
    """Two and three disjoint slices (the fan-out's lanes each write their own), in any order: the same head."""
    picks = [_split(lac) for nb, lac in oracle_streams if nb in (3, 513)][::5]
    grid = []
    for f, rows, head in picks:
        nb = len(rows) // 2
        for cuts in ((1,), (nb - 1,), (nb // 2,), (1, 2), (1, nb - 1), (nb // 3, nb - nb // 3)):
            if all(0 < a < nb for a in cuts) and list(cuts) == sorted(set(cuts)):
                grid.append((f, rows, head, cuts))
    assert {len(c) for *_, c in grid} == {1, 2} and len(grid) >= 12
    for (f, rows, head, cuts), got in zip(grid, _run(tuple(_write_cmd(f, rows, cuts) for f, rows, _, cuts in grid))):
        _check_written(got, f, rows, head)


def test_a_row_of_no_bytes_is_refused():
    f = dict(sample_rate=48000, bit_depth=16, channels=2, stereo_mode=2)
    good = [BLOCK, 100, BLOCK, 200, BLOCK, 300, BLOCK, 400, 77, 5]
    cmds = []
    for at in (0, 2, 4):  # first, middle, last
        rows = list(good)
        rows[2 * at + 1] = 0
        cmds += [_write_cmd(f, rows), _write_cmd(f, rows, (2,)), _write_cmd(f, rows, (1, 4))]
    for got in _run(tuple(cmds)):
        assert got["ok"] == 0
        assert got["parse"]["rc"] == 1 and got["parse"]["why"] == "[decode-error] invalid compressed block size"
    one, = _run((_write_cmd(f, [5, 0]),))
    assert one["ok"] == 0
    _check_written(_run((_write_cmd(f, good),))[0], f, good)


def test_rows_from_offsets_and_their_limits():
    ok, = _run((f"offsets 3 {BLOCK} {BLOCK} 9 0 10 4294967305 4294967306",))
    assert ok == dict(ok=1, rows=[BLOCK, 10, BLOCK, 4294967295, 9, 1])  # a difference of 2^32 - 1 is the largest row
    over, = _run((f"offsets 3 {BLOCK} {BLOCK} 9 0 10 4294967306 4294967307",))
    assert over == dict(ok=0, rows=[])  # 2^32
    for at in (0, 1, 2):  # an empty block first, in the middle, last
        offs = [0, 10, 20, 30]
        offs[at + 1:] = [v - 10 for v in offs[at + 1:]]
        empty, = _run((f"offsets 3 {BLOCK} {BLOCK} 9 " + " ".join(map(str, offs)),))
        assert empty == dict(ok=0, rows=[])
    one, = _run(("offsets 1 300 0 4294967295",))
    assert one == dict(ok=1, rows=[300, 4294967295])
