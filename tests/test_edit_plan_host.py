"""The host-only plan of a transcode job (csrc/edit_plan.h) against its rules restated in Python: the per-output checks with
every refusal text, the mapping of segments to window items, the staging and destination layout with its alignments and
capacities, the unit prefix sums and the transform table.  tests/native/dump_edit_plan.cpp is built from edit_plan.h alone
(no HIP), plain and as a stand-alone program under AddressSanitizer + UBSan; both must print the same plans."""
import json
import struct
import subprocess

import pytest

import editcases as E
import lacstreams
import twinbuild

SRC = twinbuild.NATIVE + "/dump_edit_plan.cpp"
TO_END = (1 << 64) - 1
UNIT, ROW_ALIGN, DST_ALIGN, LOOK_AHEAD = 1024, 4, 256, 16
OK, INVALID = 0, 1


def fake(channels, depth, rate, frames, mode=0, version=3):
    """A container parse_stream accepts (the plan never looks into the payload): blocks of 16384 frames, 5 bytes each."""
    sizes = [16384] * (frames // 16384) + ([frames % 16384] if frames % 16384 else [])
    header = bytes([0x4C, 0x41, 3, channels, mode if channels == 2 else 0, (rate >> 8) & 0xFF, rate & 0xFF, rate >> 16, depth, 0])
    lac = lacstreams._build(header, [(n, 5) for n in sizes], b"\x00" * (5 * len(sizes)))
    return lacstreams.to_v2(lac) if version == 2 else lac


def head(lac):
    """(channels, depth, rate, frames) of a stream this file made, or the parser's refusal of the three broken ones."""
    if len(lac) == 0:
        return "[decode-error] empty input"
    if len(lac) < 10 or lac[:2] != b"LA" or lac[2] not in (2, 3):
        return "[decode-error] invalid frame header"
    nb = struct.unpack(">I", lac[10:14])[0]
    row = 8 if lac[2] == 3 else 4
    if len(lac) < 14 + row * nb:
        return "[decode-error] truncated block size table"
    frames = sum(struct.unpack(">I", lac[14 + row * b:18 + row * b])[0] for b in range(nb))
    return lac[3], lac[8], (lac[5] << 8) | lac[6] | (lac[7] << 16), frames


def up(v, a):
    return (v + a - 1) // a * a


def model(streams, segs, outs):
    """The rules: outs = [(first, count, depth, op, mode)], segs = [(stream, start, frames)]."""
    code, err, planned, windows, unit_off, stage, dst = [], [], [], [], [0], 0, 0
    for i, (first, count, depth, op, mode) in enumerate(outs):
        why = None
        if count == 0:
            why = "output has no segments"
        elif first >= len(segs) or count > len(segs) - first:
            why = "segments outside the call's array"
        elif op > 5:
            why = "unknown channel operation"
        elif depth not in (0, 16, 24):
            why = f"unsupported bit depth: {depth}"
        elif mode > 2:
            why = "unknown stereo mode"
        mine, frames_out, seen, source_bytes, f0 = [], 0, set(), 0, None
        for k in range(count if why is None else 0):
            stream, start, frames = segs[first + k]
            h = head(streams[stream])
            if isinstance(h, str):
                why = f"segment {k}: {h}"
                break
            if frames == TO_END and start < h[3]:
                frames = h[3] - start
            if frames == 0:
                why = f"segment {k}: empty window"
            elif start >= h[3] or frames > h[3] - start:
                why = f"segment {k}: window outside the stream"
            if why:
                break
            f0 = f0 or h
            for field, a, b in (("channels", f0[0], h[0]), ("bit depth", f0[1], h[1]), ("sample rate", f0[2], h[2])):
                if a != b and not why:
                    why = f"segment {k}: {field} differs from segment 0: {a}, {b}"
            if why:
                break
            mine.append([len(planned), k, first + k, start, frames, frames_out, h[0]])
            frames_out += frames
            if stream not in seen:
                source_bytes += len(streams[stream])
            seen.add(stream)
        if why is None and op in (E.LEFT, E.RIGHT, E.FOLD, E.SWAP) and f0[0] != 2:
            why = "channel operation needs a stereo source"
        if why is None and op == E.DUAL and f0[0] != 1:
            why = "channel operation needs a mono source"
        code.append(INVALID if why else OK)
        err.append(why or "")
        if why:
            continue
        ch = f0[0] if op in (E.KEEP, E.SWAP) else 2 if op == E.DUAL else 1
        to = depth or f0[1]
        row = up(frames_out, ROW_ALIGN)
        left, right = stage, stage + row if f0[0] == 2 else 0
        nbytes = frames_out * ch * to // 8
        planned.append([i, len(windows), count, frames_out, f0[2], (frames_out + 16383) // 16384, f0[0], f0[1], ch, to, op, mode if ch == 2 else 0,
                        left, right, dst, nbytes, source_bytes, left, right, dst, frames_out, f0[0], op, f0[1], to])
        windows += mine
        stage += row * f0[0]
        dst += up(nbytes + LOOK_AHEAD, DST_ALIGN)
        unit_off.append(unit_off[-1] + (frames_out + UNIT - 1) // UNIT)
    return dict(code=code, err=err, outs=planned, windows=windows, unit_off=unit_off, stage_elems=stage, dst_bytes=dst)


def blob(streams, segs, outs):
    b = struct.pack("<4I", len(streams), len(segs), len(outs), 0)
    b += b"".join(struct.pack("<Q", len(s)) + s for s in streams)
    b += b"".join(struct.pack("<IIQQ", s, 0, start, frames) for s, start, frames in segs)
    return b + b"".join(struct.pack("<IIBBB5x", first, count, depth, op, mode) for first, count, depth, op, mode in outs)


def cases():
    st16 = fake(2, 16, 48000, 40000, 2)
    st16b = fake(2, 16, 48000, 20001, 1)
    v2 = fake(2, 16, 48000, 40000, 2, version=2)
    mono24 = fake(1, 24, 96000, 20000)
    st24 = fake(2, 24, 48000, 1023)
    st16_44 = fake(2, 16, 44100, 5000)
    real = E.sources()["st16_auto"].lac
    streams = [st16, st16b, v2, mono24, st24, st16_44, b"", b"XX" + st16[2:], st16[:20], real]
    out = []
    # layouts: every length around a quad and a unit, mono and stereo, every operation and depth change, several outputs
    lengths = (1, 2, 3, 4, 5, 1023, 1024, 1025, 4097, 16385)
    segs = [(0, 7, n) for n in lengths] + [(3, 3, n) for n in lengths]
    outs = [(k, 1, 0, E.KEEP, 2) for k in range(len(segs))]
    out.append((streams, segs, outs))
    segs = [(0, 0, TO_END), (0, 39999, TO_END), (1, 5, 100), (2, 16383, 2), (3, 0, TO_END), (4, 0, TO_END), (9, 1, 39999), (0, 100, 300), (0, 200, 300)]
    outs = [(0, 1, 0, E.KEEP, 0), (0, 4, 24, E.SWAP, 1), (1, 2, 0, E.LEFT, 2), (2, 1, 0, E.RIGHT, 2), (2, 2, 0, E.FOLD, 2), (4, 1, 16, E.DUAL, 2),
               (4, 1, 0, E.DUAL, 1), (5, 1, 16, E.KEEP, 2), (5, 1, 16, E.FOLD, 0), (6, 1, 24, E.KEEP, 2), (7, 2, 0, E.KEEP, 2), (0, 9, 0, E.KEEP, 2)]
    out.append((streams, segs, outs))
    # every refusal, between outputs that pass
    segs = [(0, 0, 10), (0, 40000, 1), (0, 39999, 2), (0, 0, 0), (0, 1, TO_END - 1), (0, 40000, TO_END), (3, 0, 10), (4, 0, 10), (5, 0, 10),
            (6, 0, 1), (7, 0, 1), (8, 0, 1), (0, 0, 10), (4, 0, 10), (0, 0, 10), (5, 0, 10)]
    good = (0, 1, 0, E.KEEP, 2)
    outs = [good, (0, 0, 0, E.KEEP, 2), (16, 1, 0, E.KEEP, 2), (15, 2, 0, E.KEEP, 2), (0, 17, 0, E.KEEP, 2), (12, 2, 0, E.KEEP, 2), (14, 2, 0, E.KEEP, 2), (0, 1, 0, 6, 2), (0, 1, 0, 255, 2),
            (0, 1, 8, E.KEEP, 2), (0, 1, 32, E.KEEP, 2), (0, 1, 0, E.KEEP, 3), good, (1, 1, 0, E.KEEP, 2), (2, 1, 0, E.KEEP, 2), (3, 1, 0, E.KEEP, 2),
            (4, 1, 0, E.KEEP, 2), (5, 1, 0, E.KEEP, 2), (0, 2, 0, E.KEEP, 2), (0, 7, 0, E.KEEP, 2), (7, 2, 0, E.KEEP, 2), (0, 9, 0, E.KEEP, 2),
            (6, 1, 0, E.LEFT, 2), (6, 1, 0, E.RIGHT, 2), (6, 1, 0, E.FOLD, 2), (6, 1, 0, E.SWAP, 2), (0, 1, 0, E.DUAL, 2), (9, 1, 0, E.KEEP, 2),
            (10, 1, 0, E.KEEP, 2), (11, 1, 0, E.KEEP, 2), (0, 1, 0, 9, 99), (6, 1, 0, E.DUAL, 3), good]
    out.append((streams, segs, outs))
    out.append((streams, [(0, 0, 1)], [(0, 0, 0, E.KEEP, 2)]))  # nothing goes to the device
    return out


@pytest.fixture(scope="module")
def plain_exe():
    return twinbuild.program("dump_edit_plan", [SRC], ["-O2", "-std=c++20"])


def _plans(exe, env=None):
    lines, rc, err = twinbuild.run_cases(exe, [blob(*c) for c in cases()], env or {}, prefix="edit_plan_")
    assert rc == 0, err
    return [json.loads(t.split(" ", 1)[1]) for t in lines]


def test_plans_follow_the_rules(plain_exe):
    got = _plans(plain_exe)
    assert len(got) == len(cases())
    texts = set()
    for c, g in zip(cases(), got):
        want = model(*c)
        assert g == want
        texts |= {t.split(": ", 1)[1] if t.startswith("segment ") else t for t in want["err"] if t}
        for o in g["outs"]:
            assert o[12] % ROW_ALIGN == 0 and o[13] % ROW_ALIGN == 0 and o[14] % DST_ALIGN == 0  # 16-byte rows, 256-byte destinations
    assert texts >= {"output has no segments", "segments outside the call's array", "unknown channel operation", "unsupported bit depth: 8",
                     "unknown stereo mode", "empty window", "window outside the stream", "channels differs from segment 0: 2, 1",
                     "bit depth differs from segment 0: 16, 24", "sample rate differs from segment 0: 48000, 44100",
                     "channel operation needs a stereo source", "channel operation needs a mono source", "[decode-error] empty input",
                     "[decode-error] invalid frame header", "[decode-error] truncated block size table"}


def test_sanitized_build_prints_the_same_plans(plain_exe):
    exe, why = twinbuild.sanitized_exe("dump_edit_plan_san", [SRC])
    if exe is None:
        pytest.skip(why)
    env = dict(ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    assert _plans(exe, env) == _plans(plain_exe)


def test_violation_texts(plain_exe):
    quads = [(4 * 7 + 0, E.FOLD, 5, -6), (4 * 0 + 1, E.KEEP, 257, 512), (4 * 1023 + 2, E.KEEP, 256, -1), (4 * 9 + 1, E.SWAP, 256, 3),
             (4 * 9 + 2, E.SWAP, 5, 256), (4 * 2 + 1, E.RIGHT, 256, 77), (4 * 2 + 2, E.DUAL, 1, 0), (4 * (2 ** 40) + 1, E.LEFT, -255, 0)]
    done = subprocess.run([plain_exe, "--messages", *[str(v) for q in quads for v in q]], capture_output=True, text=True, check=True)
    assert done.stdout.splitlines() == [
        "[transcode-error] frame 7: left 5 and right -6 differ", "[transcode-error] frame 0 left sample 257 is not a multiple of 256",
        "[transcode-error] frame 1023 right sample -1 is not a multiple of 256", "[transcode-error] frame 9 left sample 3 is not a multiple of 256",
        "[transcode-error] frame 9 right sample 5 is not a multiple of 256", "[transcode-error] frame 2 left sample 77 is not a multiple of 256",
        "[transcode-error] frame 2 right sample 1 is not a multiple of 256", f"[transcode-error] frame {2 ** 40} left sample -255 is not a multiple of 256"]
