"""The salvage decode (decode through errors) off the device: where its expectations come from, and its CPU twin.

  expected(oracle, lac)     what a salvage decode of `lac` must give, from the oracle and the file's length alone -- never
                            from the code under test: Expected(left, right, lost, known, present, flags, frames)
  wav_image(exp, lac)       the WAV file image of that
  run(lacs, ...)            the CPU twin (tests/native/sim_salvage.cpp: csrc/decode_plan.h, decode_core.h, salvage_core.h),
                            plain build through ctypes -> [Item]
  case / digest / run_sanitized   the same jobs through the build with AddressSanitizer + UBSan, a program of its own
                            (a sanitizer is never loaded into Python)
  truncations(lac)          the truncation family: a version-3 stream cut inside every block and exactly at every border
  check(item, exp, status)  one item of the twin or of the device against expected() and the decode twin's statuses
  cleared(...)              streams that may go to a device: the sanitized twin has passed them in this run

Version 3: every present block is cut out into a one-block stream of its own and handed to the oracle (decode_ex).
Accepted with the largest zigzag value below 2^30: the block's samples.  Refused: zeros, lost.  Accepted with a larger
value: zeros, code 9, the documented device limit (taken from the oracle's own max_u).  Missing blocks follow from the file
length.  Version 2 has no sizes: the oracle's channel-block reader (channel_block_end) walks the payload block by block
as the one lane does; a block it cannot walk is lost with everything behind it (8, not reached), a block it walks is cut
out and judged like a version-3 block -- refused there (the bit-depth check, which the device runs after the walk: 7)
the walk goes on, which is the one exception mutantjudge allows too.  The oracle's verdict on the whole version-2 stream
must agree: its refused block is the first lost one."""
from __future__ import annotations

import ctypes as C
import struct
import sys
from collections import namedtuple

import numpy as np

import dectwin
import lacmutate
import lacstreams
import twinbuild
import wavutil

SRC = twinbuild.NATIVE + "/sim_salvage.cpp"
LIMIT = 1 << 30
MISSING, NOT_REACHED, BEYOND = 10, 8, 9
TRUNCATED, TRAILING = 1, 2
SENTINEL = 0x5A5A5A5A
DERIVED_OVERSHOOT = 25   # bytes: the figure the comment at BitIn (csrc/decode_core.h) derives

# lost[b]: block b is silence; known[b]: the code where the expectation itself states one (8, 9, 10), else None
Expected = namedtuple("Expected", "left right lost known present flags frames")
# codes[b]: 0 or the fault code; image: the WAV form's image (its 44 header bytes still 0xCD); left / right: the device form
Item = namedtuple("Item", "refused message blocks bad_blocks frames lost_frames first_bad flags codes image left right")

_lib = None
_blocks = {}


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(twinbuild.shared_lib("sim_salvage", [SRC]))
        _lib.sim_salvage.restype = C.c_int64
    return _lib


def sanitized_exe():
    """The sanitized program's path, or (None, why) where the sanitizer runtime is missing."""
    return twinbuild.sanitized_exe("sim_salvage_san", [SRC], ["-DSIM_SALVAGE_MAIN"])


# ---- expectations -----------------------------------------------------------------------------------------------------
def _one_block(oracle, header, n, payload):
    """The oracle on one block as a stream of its own -> (left, right, max_u); left is None where it refuses."""
    lac = lacstreams._build(header, [(n, len(payload))], payload)
    if lac not in _blocks:
        left, right, _, max_u = oracle.decode_ex(lac)
        _blocks[lac] = (left, right, max_u)
    return _blocks[lac]


def _walk_v2(oracle, lac, ent, head):
    """The byte range of every block of a version-2 stream the oracle's reader can walk, in order; shorter where it stops."""
    channels, flagged = lac[3], lac[3] == 2 and lac[4] == 2
    out, off = [], head
    for n, _ in ent:
        at = off
        if flagged:
            if at >= len(lac) or lac[at] > 1:
                break
            at += 1
        for _ in range(channels):
            size = oracle.channel_block_end(lac[at:], n)
            if size is None:
                at = None
                break
            at += size
        if at is None:
            break
        out.append((off, at))
        off = at
    return out


def expected(oracle, lac) -> Expected:
    version, ent, head = lacmutate.table(lac)
    nb, stereo = len(ent), lac[3] == 2
    frames = [n for n, _ in ent]
    total = sum(frames)
    left = np.zeros(total, np.int32)
    right = np.zeros(total, np.int32) if stereo else None
    lost, known = [True] * nb, [None] * nb
    edges = np.concatenate([[0], np.cumsum(frames)]).astype(np.int64)
    flags = 0
    if version == 3:
        ranges, off = [], head
        for _, size in ent:
            if off + size > len(lac):
                break
            ranges.append((off, off + size))
            off += size
        end = head + sum(s for _, s in ent)
        flags = TRUNCATED if len(lac) < end else TRAILING if len(lac) > end else 0
        present = len(ranges)
        for b in range(present, nb):
            known[b] = MISSING
    else:
        ranges = _walk_v2(oracle, lac, ent, head)
        present = nb
        for b in range(len(ranges) + 1, nb):  # (the block the walk stopped in has the lane's own status)
            known[b] = NOT_REACHED
    stopped = False
    for b, (a, e) in enumerate(ranges):
        if stopped:
            known[b] = NOT_REACHED
            continue
        bl, br, max_u = _one_block(oracle, lac[:2] + b"\x03" + lac[3:10], frames[b], lac[a:e])  # (a version-3 stream of its own)
        if version == 2 and b + 1 == nb and e != len(lac):
            bl = None  # trailing frame payload behind the last block: the serial lane's status 6
        if max_u >= LIMIT:  # the device refuses what it cannot decode as the reference does; one lane then stops its walk
            known[b] = BEYOND if bl is not None else None
            stopped = version == 2
            continue
        if bl is None:
            continue
        lost[b] = False
        left[edges[b]:edges[b + 1]] = bl
        if stereo:
            right[edges[b]:edges[b + 1]] = br
    if version == 2:  # the oracle's verdict on the stream as a whole must be the walk's
        _, _, bad, max_u = oracle.decode_ex(lac)
        first = next((b for b in range(nb) if lost[b]), None)
        assert max_u >= LIMIT or bad == first, "version 2: the oracle refuses block %r, the walk loses block %r first" % (bad, first)
    return Expected(left, right, lost, known, present, flags, total)


def rate(lac):
    return (lac[5] << 8) | lac[6] | (lac[7] << 16)


def wav_image(exp: Expected, lac) -> bytes:
    return wavutil.make_wav(exp.left, exp.right, rate(lac), lac[8])


def truncations(lac):
    """(parameters, bytes): a version-3 stream cut exactly at every block border (the table's end included) and inside
    every block -- one byte in, in the middle, one byte short."""
    _, ent, head = lacmutate.table(lac)
    off = head
    for b, (_, size) in enumerate(ent):
        yield "border%d" % b, lac[:off]
        for name, d in (("first", 1), ("mid", size // 2), ("last", size - 1)):
            if 0 < d < size:
                yield "in%d.%s" % (b, name), lac[:off + d]
        off += size


def constructed():
    """(name, stream, the decode twin's statuses -- of the uncut parent for a cut stream): what the mutation corpus need
    not hold.  `stitch257`: three 257-frame blocks as one stream (a fixture's only block, spliced: borders at frames 257
    and 514, no multiple of four) with each block, each pair and all three broken in turn, and every cut of the whole
    stream and of the one with its middle block broken.  `nine`: a block whose first escape token carries 2^30 (status
    9) between two blocks of lacmutate's equal-blocks stream, and cut."""
    import lacgrammar as g  # noqa: F401  (lacmutate's bases build on it)
    one = lacmutate.bases()["small/n257_st16_ms"]
    lac = lacstreams.splice(lacstreams.splice(one, one), one)
    ent, pays = lacmutate._payloads(lac)
    out = []

    def broken(which):
        p2 = list(pays)
        for b in which:
            p2[b] = pays[b][:1] + bytes([0x7F]) + pays[b][2:]  # an unknown predictor type behind the flag byte
        return lacmutate._rebuild(lac, ent, p2)

    for which in ((0,), (1,), (2,), (0, 1), (1, 2), (0, 2), (0, 1, 2)):
        m = broken(which)
        out.append(("stitch257|broken%s" % "".join(map(str, which)), m, dectwin.decode(m).status))
    for parent, tag in ((lac, "whole"), (broken((1,)), "broken1")):
        status = dectwin.decode(parent).status
        out += [("stitch257|%s|cut|%s" % (tag, par), t, status) for par, t in truncations(parent)]
    eq = lacmutate.equal_blocks("mono", 1)
    esc = bytearray(lacmutate.escape_base(24))
    _, (e_ent,), e_head = lacmutate.table(bytes(esc))
    lacmutate._set_bits(esc, 8 * e_head + 24 + 7 + 2, 32, 1 << 30)
    ent, pays = lacmutate._payloads(eq)
    nine = lacstreams._build(eq[:10], [ent[0], e_ent, ent[1]], pays[0] + bytes(esc[e_head:]) + pays[1])
    status = dectwin.decode(nine).status
    out.append(("nine|between", nine, status))
    out += [("nine|cut|%s" % par, t, status) for par, t in truncations(nine)]
    return out


def check(what, lac, exp: Expected, status, codes, result, image=None, left=None, right=None):
    """One salvaged item against expected(): the lost blocks, their codes (the expectation's own where it states one, else
    the decode twin's `status` of that block), the result fields, and the image or the planar arrays."""
    nb = len(exp.lost)
    frames = [n for n, _ in lacmutate.table(lac)[1]]
    assert len(codes) == nb, what
    for b in range(nb):
        assert (codes[b] != 0) == exp.lost[b], "%s: block %d has code %d, expected %s" % (what, b, codes[b], "lost" if exp.lost[b] else "decoded")
        if exp.known[b] is not None:
            assert codes[b] == exp.known[b], "%s: block %d has code %d, expected %d" % (what, b, codes[b], exp.known[b])
        elif exp.lost[b] and status is not None:
            assert codes[b] == status[b] and 1 <= codes[b] <= 9, "%s: block %d has code %d, the decode twin says %d" % (what, b, codes[b], status[b])
    bad = [b for b in range(nb) if exp.lost[b]]
    want = (nb, len(bad), exp.frames, sum(frames[b] for b in bad), bad[0] if bad else nb, exp.flags)
    assert tuple(result) == want, "%s: result %r, expected %r" % (what, tuple(result), want)
    if image is not None:
        full = wav_image(exp, lac)
        assert len(image) == len(full) and bytes(image[44:]) == full[44:], "%s: the image's data differs" % what
    if left is not None:
        assert np.array_equal(left, exp.left), "%s: left differs" % what
        assert (right is None) == (exp.right is None) and (right is None or np.array_equal(right, exp.right)), "%s: right differs" % what


# ---- the twin ---------------------------------------------------------------------------------------------------------
def _head_ok(lac):
    return len(lac) >= 14 and lac[2] in (2, 3) and len(lac) >= 14 + (8 if lac[2] == 3 else 4) * struct.unpack(">I", lac[10:14])[0]


def run(lacs, device=False, cols=1, never_lean=False, zero_status=False):
    """n streams as one salvage job on the CPU twin -> ([Item], over)."""
    n = len(lacs)
    ptrs = (C.c_char_p * n)(*lacs)
    sizes = (C.c_uint64 * n)(*[len(x) for x in lacs])
    shapes = [dectwin._shape(x) if _head_ok(x) else (0, []) for x in lacs]
    nblocks = sum(nb for nb, _ in shapes) + 1
    npcm = sum(sum(fr) for _, fr in shapes) + 1
    nimage = sum((44 + sum(fr) * x[3] * (x[8] // 8) + 1 + 15) // 16 * 16 for x, (_, fr) in zip(lacs, shapes) if fr) + 16
    rec = np.zeros(8 * n, np.uint64)
    codes = np.zeros(nblocks, np.uint32)
    image = np.zeros(nimage if not device else 1, np.uint8)
    left = np.full(npcm if device else 1, SENTINEL, np.int32)
    right = np.full(npcm if device else 1, SENTINEL, np.int32)
    msg = C.create_string_buffer(1 << 16)
    over = C.c_uint32()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    got = lib().sim_salvage(ptrs, sizes, C.c_uint32(n), int(device), int(cols), int(never_lean), int(zero_status), vp(rec), vp(codes),
                            C.c_uint64(codes.size), vp(image), C.c_uint64(image.size), vp(left), vp(right), C.c_uint64(left.size), msg,
                            C.c_uint32(len(msg)), C.byref(over))
    assert got >= 0, "the twin could not plan the job"
    msgs = msg.value.decode().split("\n")
    items, at_code = [], 0
    for i, lac in enumerate(lacs):
        refused, nb, bad, frames, lostf, first, flags, at = (int(v) for v in rec[8 * i:8 * i + 8])
        if refused:
            items.append(Item(True, msgs[i], 0, 0, 0, 0, 0, 0, None, None, None, None))
            continue
        c = codes[at_code:at_code + nb].tolist()
        at_code += nb
        size = 44 + frames * lac[3] * (lac[8] // 8)
        size += size & 1
        items.append(Item(False, "", nb, bad, frames, lostf, first, flags, c,
                          None if device else image[at:at + size].tobytes(),
                          left[at:at + frames].copy() if device else None,
                          right[at:at + frames].copy() if device and lac[3] == 2 else None))
    return items, over.value


PLAN_HEAD = ("m total_blocks total_frames total_pay total_units pcm_total image_total lanes nv2 o_items o_byte o_frame o_unit o_bitem "
             "o_lane o_v2 o_present o_size need_payload need_blocks need_pcm need_image need_stage tail_pad").split()
PLAN_ITEM = "src present flags pay_bytes head pcm_at image_at image_size frames blocks block0 pay_off".split()


def plan_dump(lacs, device=False):
    """The product's plan of a salvage job and its filled tables (csrc/decode_plan.h): the PLAN_HEAD fields, `items` (dicts
    of PLAN_ITEM), `rc` and `msg` per input, and the tables item, byte_off, frame_off, unit_off, blk_item, lane_blk,
    v2_items, present.  The made-up base addresses are dectwin.base's."""
    n = len(lacs)
    ptrs = (C.c_char_p * n)(*lacs)
    sizes = (C.c_uint64 * n)(*[len(x) for x in lacs])
    L = lib()
    L.sim_salvage_plan.restype = C.c_int64
    head = np.zeros(len(PLAN_HEAD), np.uint64)
    item = np.zeros(len(PLAN_ITEM) * n, np.uint64)
    rc = np.zeros(n, np.int32)
    msg = C.create_string_buffer(1 << 16)
    raw = np.zeros(1 << 22, np.uint8)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    size = L.sim_salvage_plan(ptrs, sizes, C.c_uint32(n), int(device), vp(head), vp(item), vp(rc), msg, C.c_uint32(len(msg)), vp(raw),
                              C.c_uint64(raw.size))
    assert size >= 0, msg.value
    p = {k: int(v) for k, v in zip(PLAN_HEAD, head)}
    m, T = p["m"], p["total_blocks"]
    p["items"] = [dict(zip(PLAN_ITEM, (int(v) for v in item[len(PLAN_ITEM) * j:len(PLAN_ITEM) * (j + 1)]))) for j in range(m)]
    p["rc"], p["msg"] = rc.tolist(), msg.value.decode().split("\n")
    p["need_tables"] = size
    raw = raw[:size]
    tab = lambda off, dtype, count: np.frombuffer(raw, dtype=dtype, count=count, offset=off)  # noqa: E731
    p["item"] = tab(p["o_items"], dectwin.ITEM_DTYPE, m)
    p["byte_off"], p["frame_off"] = tab(p["o_byte"], "<u8", T + 1), tab(p["o_frame"], "<u8", T + 1)
    p["unit_off"], p["blk_item"] = tab(p["o_unit"], "<u8", m + 1), tab(p["o_bitem"], "<u4", T)
    p["lane_blk"], p["v2_items"] = tab(p["o_lane"], "<u4", p["lanes"]), tab(p["o_v2"], "<u4", p["nv2"])
    p["present"] = tab(p["o_present"], "<u4", m)
    return p


def result_of(item):
    return (item.blocks, item.bad_blocks, item.frames, item.lost_frames, item.first_bad, item.flags)


def case(lacs, device=False, cols=1, never_lean=False, zero_status=False) -> bytes:
    flags = int(device) | (2 if cols == 64 else 0) | (4 if never_lean else 0) | (8 if zero_status else 0)
    return struct.pack("<II", len(lacs), flags) + b"".join(struct.pack("<Q", len(x)) + x for x in lacs)


def digest(blob: bytes, index: int) -> str:
    """The plain build's line for a case (what the sanitized program must print for it)."""
    buf = C.create_string_buffer(1 << 22)
    rc = lib().sim_salvage_digest(blob, C.c_uint64(len(blob)), C.c_uint32(index), buf, C.c_uint32(len(buf)))
    assert rc == 0
    return buf.value.decode()


def run_sanitized(cases, exe=None, workers=8):
    """Every case through the sanitized program, split over a few processes: (lines, returncode, stderr)."""
    if exe is None:
        exe, why = sanitized_exe()
        assert exe, why
    return twinbuild.run_cases(exe, cases, dectwin.ENV, workers=workers, prefix="lac_salvage_")


BATCH = 64


def cleared(key, lacs):
    """`lacs`, once the sanitized twin has shown in this run that a salvage job over each of them stays inside buffers of
    exactly the plan's capacities -- both forms, both status fills, 1 and 64 columns, in batches -- and answers as the
    plain build does.  Fails, never skips, where that cannot be shown."""
    def make():
        cases = []
        for at in range(0, len(lacs), BATCH):
            part = lacs[at:at + BATCH]
            k = at // BATCH
            cases.append(case(part, device=False, cols=64 if k & 1 else 1, never_lean=bool(k & 2), zero_status=bool(k & 1)))
            cases.append(case(part, device=True, cols=1 if k & 1 else 64, never_lean=not (k & 2), zero_status=not (k & 1)))

        def check(i, text):
            over = int(text.split()[1])
            assert over <= DERIVED_OVERSHOOT, "case %d: a load reached %d bytes past its block" % (i, over)

        return cases, lambda c, i: digest(c, i).split(" ", 1)[1], check, list(lacs)

    return twinbuild.cleared("salvage", key, sys.modules[__name__], make)
