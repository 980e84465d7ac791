"""The encoder's host-side plans (csrc/encode_plan.h: plan_chunks, plan_shard, plan_batch, the table from size records)
without a device: the arithmetic that decides what the encode kernels are told, printed by tests/native/sim_encode_plan.cpp
-- built from the header alone, with no ROCm include path, plain and as a stand-alone AddressSanitizer + UBSan program --
and compared with the rules as they are stated here, by brute force where there is one."""
import functools
import itertools
import json
import os
import re
import subprocess

import pytest

import twinbuild

SRC = os.path.join(twinbuild.NATIVE, "sim_encode_plan.cpp")
BLOCK, STREAMS, MAX_CHUNKS, MIN_CHUNK_BLOCKS, RANGE_ITEMS, BOTH_WAYS = 16384, 4, 16, 192, 256, 4096
PLANAR_I32, INTER_I16, INTER_I24, PLANAR_I16, PLANAR_F32, INTER_F32 = 0, 1, 2, 16, 17, 18


@functools.lru_cache(maxsize=None)
def _exe(sanitized):
    if sanitized:
        return twinbuild.sanitized_exe("sim_encode_plan_san", [SRC], ["-Wall", "-Werror"])
    return twinbuild.program("sim_encode_plan", [SRC], ["-std=c++20", "-Wall", "-Werror", "-O1"]), ""


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


# ---- chunk plans ----
def _weights(split):
    """strtod's view of a split list: numbers separated by single commas, up to 16, only the positive ones."""
    w, pos = [], 0
    while pos < len(split) and len(w) < MAX_CHUNKS:
        m = re.match(r"[+-]?(\d+\.?\d*|\.\d+)", split[pos:])
        if not m:
            break
        if float(m.group(0)) > 0:
            w.append(float(m.group(0)))
        pos += m.end()
        if split[pos:pos + 1] == ",":
            pos += 1
    return w


def _want_chunks(nb, device_emit, fused, upload, pipe_chunks, split):
    """The documented rule: one chunk per 192 blocks, at most 8 (host emit) / 3, 4 from 6000, 6 from 12000 blocks (device
    emit, unfused) / 1 (fused) / 4 (fused, input still on the host); LACX_PIPE_CHUNKS 1..16 forces the count; LACX_PIPE_SPLIT
    gives relative sizes; three unforced device-emit chunks default to 5:5:4, or 1:2:3 with the fused emit and an upload."""
    n = nb // MIN_CHUNK_BLOCKS
    device_max = (4 if upload else 1) if fused else (6 if nb >= 12000 else 4 if nb >= 6000 else 3)
    n = max(1, min(n, device_max if device_emit else 8))
    forced = 1 <= pipe_chunks <= MAX_CHUNKS
    if forced:
        n = min(pipe_chunks, nb)
    if not split and not forced and device_emit and n == 3:
        split = "1,2,3" if fused and upload else "5,5,4"
    w = _weights(split)
    if w and nb >= len(w):
        out, first, acc = [], 0, 0.0
        for i, x in enumerate(w):
            acc += x
            end = nb if i + 1 == len(w) else int(nb * (acc / sum(w)))
            end = min(max(end, first + 1), nb - (len(w) - 1 - i))
            out.append([first, end - first])
            first = end
        return out
    per = -(-nb // n)
    return [[f, min(per, nb - f)] for f in range(0, nb, per)]


NBS = [1, 2, 3, 5, 191, 192, 383, 384, 768, 5999, 6000, 12000, 21094]
PIPELINES = [(0, 0, 0), (1, 0, 0), (1, 1, 0), (1, 1, 1)]  # host emit, device emit unfused, fused, fused + upload
SPLITS = ["", "5,3,1", "1,2,3", "0,0", "x", ",".join(["1"] * 17) + ",1,1,1,1,1"]


def test_chunk_plans():
    grid = list(itertools.product(NBS, PIPELINES, [0, 1, 3, 16, 17], SPLITS))
    cmds = tuple(f"chunks {nb} {de} {fu} {up} {pc} {sp or '-'}" for nb, (de, fu, up), pc, sp in grid)
    for (nb, (de, fu, up), pc, sp), got in zip(grid, _run(cmds)):
        chunks = got["chunks"]
        assert all(c > 0 for _, c in chunks), (nb, de, fu, up, pc, sp)
        assert chunks[0][0] == 0 and sum(c for _, c in chunks) == nb
        assert all(a[0] + a[1] == b[0] for a, b in zip(chunks, chunks[1:]))
        assert 1 <= len(chunks) <= MAX_CHUNKS
        assert chunks == _want_chunks(nb, de, fu, up, pc, sp), (nb, de, fu, up, pc, sp)
    # the documented defaults at three chunks, spelled out
    assert _want_chunks(768, 1, 0, 0, 0, "") == [[0, 274], [274, 274], [548, 220]]  # 5:5:4
    assert _run(("chunks 768 1 0 0 0 -", "chunks 700 1 1 1 3 -", "chunks 600 0 0 0 0 -")) == \
        [{"chunks": [[0, 274], [274, 274], [548, 220]]}, {"chunks": [[0, 234], [234, 234], [468, 232]]},
         {"chunks": [[0, 200], [200, 200], [400, 200]]}]


# ---- shard plans ----
KNOB_NAMES = ("fused", "direct", "packer", "persistent", "lazy", "halves")


def _shard_cmd(frames, ch, bd, mode, layout, host, knobs, pinned, pipe_chunks, split=""):
    return (f"shard {frames} {ch} {bd} {mode} {layout} {host} " + " ".join(str(int(knobs[k])) for k in KNOB_NAMES) +
            f" {pinned} {pipe_chunks} {split or '-'}")


def _up(v, k):
    return (v + k - 1) // k * k


def _check_shard(got, frames, ch, bd, mode, layout, host, knobs, pinned, pipe_chunks, split=""):
    nb = -(-frames // BLOCK)
    frame_bytes = {PLANAR_I32: 4, INTER_I16: 2 * ch, INTER_I24: 3 * ch}[layout]
    chunks = _want_chunks(nb, 1, knobs["fused"], host, pipe_chunks, split)
    both_ways = ch == 2 and mode == 2 and frames - (nb - 1) * BLOCK <= BOTH_WAYS
    fuse = (nb - both_ways) * ch if knobs["fused"] else 0
    packer = bool(fuse and knobs["packer"])
    drained = bool(knobs["fused"] and not knobs["direct"] and knobs["packer"] and pinned == 0)
    one = len(chunks) == 1
    want = dict(nb=nb, frame_bytes=frame_bytes, fused=knobs["fused"], packer=packer, drained=drained, direct=not drained,
                lazy=bool(knobs["lazy"] and packer and one and fuse == nb * ch), persistent=bool(one and knobs["persistent"]),
                front_halves=bool(one and knobs["halves"]), fuse_items=fuse,
                ranges=-(-fuse // RANGE_ITEMS) if drained and packer else 0)
    assert {k: int(got[k]) for k in want} == {k: int(v) for k, v in want.items()}
    reservation = pinned or frames * ch * (bd // 8) * 5 // 4 + nb * 64 + 4096
    assert got["cap"] == dict(dev_payload=reservation + 64 if drained else 0, pinned_payload=reservation, prefix=_up(14 + 8 * nb, 4096),
                              pinned_fresh=int(pinned != 0), ranges=-(-nb * ch // RANGE_ITEMS) + 1 if drained else 0, table_blocks=nb,
                              emitted=2 * nb if knobs["fused"] else 0, sizes=nb * ch if want["lazy"] else 0, batch_table=0)
    assert [[k["first"], k["count"]] for k in got["chunks"]] == chunks
    for c, k in enumerate(got["chunks"]):
        assert (k["f0"], k["f1"]) == (k["first"] * BLOCK, min(frames, (k["first"] + k["count"]) * BLOCK)) and k["f0"] < k["f1"]
        assert k["src_off"] == k["f0"] * frame_bytes
        assert k["stream_base"] == k["first"] * ch
        # brute force: the chunk's stream indices that lie below the shard's fuse_items, and they are a prefix of its own
        mine = [i for i in range(k["first"] * ch, (k["first"] + k["count"]) * ch) if i < fuse] if nb <= 4096 else None
        if mine is not None:
            assert k["fuse_items"] == len(mine) and mine == list(range(k["stream_base"], k["stream_base"] + len(mine)))
        assert (k["stream"], k["block_off_at"], k["err_at"], k["t_first_at"], k["t_last_at"], k["work_ctr_at"]) == \
            (c % STREAMS, k["first"] + c, c, c, MAX_CHUNKS + c, 8 * c)
    assert sum(k["fuse_items"] for k in got["chunks"]) == fuse
    # the per-chunk words of block_off do not overlap: count + 1 entries each
    assert all(a["block_off_at"] + a["count"] + 1 == b["block_off_at"] for a, b in zip(got["chunks"], got["chunks"][1:]))


DEFAULT = dict(fused=1, direct=0, packer=1, persistent=1, lazy=1, halves=1)


def test_shard_geometry():
    """Frame ranges, source offsets per layout, stream indices and fuse shares over block counts, last-block lengths on both
    sides of the both-ways limit, stereo modes and mono."""
    grid = []
    for blocks, rem, (ch, mode), layout, host, fused, pipe_chunks in itertools.product(
            (0, 1, 2, 5, 800), (0, 1, 4096, 4097), ((2, 2), (2, 0), (2, 1), (1, 0)), (PLANAR_I32, INTER_I16, INTER_I24), (0, 1), (1, 0), (0, 3)):
        frames = blocks * BLOCK + (rem or BLOCK)
        grid.append((frames, ch, 24 if layout == INTER_I24 else 16, mode, layout, host, dict(DEFAULT, fused=fused), 0, pipe_chunks))
    for args, got in zip(grid, _run(tuple(_shard_cmd(*a) for a in grid))):
        _check_shard(got, *args)
    # a forced split beats the default one, and the last block is encoded both ways exactly up to 4096 frames
    a, b = _run((_shard_cmd(BLOCK * 5 + 4096, 2, 16, 2, 0, 1, DEFAULT, 0, 0, "1,2,3"), _shard_cmd(BLOCK * 5 + 4097, 2, 16, 2, 0, 1, DEFAULT, 0, 0, "1,2,3")))
    assert [k["count"] for k in a["chunks"]] == [1, 2, 3] and (a["fuse_items"], b["fuse_items"]) == (10, 12)
    assert [k["fuse_items"] for k in a["chunks"]] == [2, 4, 4] and not a["lazy"]


def test_shard_modes_and_sizes_over_the_knob_grid():
    shapes = [(BLOCK * 5 + 321, 2, 16, 2), (BLOCK * 3 + 5, 1, 24, 0), (BLOCK * 1024 + 7, 2, 16, 2), (100, 2, 16, 2), (BLOCK * 300, 2, 24, 1)]
    grid = []
    for (frames, ch, bd, mode), bits, pinned, pipe_chunks, host in itertools.product(shapes, itertools.product((0, 1), repeat=6), (0, 20000), (0, 3), (0, 1)):
        grid.append((frames, ch, bd, mode, 0, host, dict(zip(KNOB_NAMES, bits)), pinned, pipe_chunks))
    for args, got in zip(grid, _run(tuple(_shard_cmd(*a) for a in grid))):
        _check_shard(got, *args)
    # the default call on device input: one chunk, drained, lazy, persistent, front halves
    got, short = _run((_shard_cmd(BLOCK * 1024, 2, 16, 2, 0, 0, DEFAULT, 0, 0), _shard_cmd(BLOCK * 1024 + 7, 2, 16, 2, 0, 0, DEFAULT, 0, 0)))
    assert len(got["chunks"]) == 1 and got["drained"] and got["lazy"] and got["persistent"] and got["front_halves"]
    assert (got["ranges"], got["cap"]["ranges"]) == (8, 9)
    # (a last block that is encoded both ways stays out of the fused emit: k_emit has work, so no lazy repair)
    assert (short["nb"], short["fuse_items"], short["lazy"], short["ranges"], short["cap"]["ranges"]) == (1025, 2048, 0, 8, 10)


# ---- the batch ----
def _item(frames, rate=48000, depth=16, mode=2, ch=2, layout=PLANAR_I32, d0=1, d1=None, cap=0):
    return (frames, rate, depth, mode, ch, layout, d0, (1 if ch == 2 and layout in (PLANAR_I32, PLANAR_I16, PLANAR_F32) else 0) if d1 is None else d1, cap)


def _batch_cmd(items, pinned=0, exact=False):
    return f"batch {len(items)} {pinned} {int(exact)} " + " ".join(" ".join(map(str, it)) for it in items)


MIXED = [_item(BLOCK * 2 + 100),                                  # the last block is encoded both ways
         _item(5000, depth=24, ch=1, mode=0),                     # one block
         _item(BLOCK * 3, mode=0, layout=INTER_I16),
         _item(BLOCK + 4097, rate=96000, depth=24, layout=PLANAR_F32),  # through the import pass
         _item(BLOCK + 4097, rate=44100, depth=24, ch=1, mode=1, layout=INTER_I24),
         _item(1, rate=192000, layout=PLANAR_I16)]


def _check_batch(got, items, pinned=0, exact=False):
    assert got["rc"] == 0
    nb = nitems = region = 0
    spans, want_map = [], []
    for i, ((frames, rate, depth, mode, ch, layout, d0, d1, cap), s) in enumerate(zip(items, got["streams"])):
        snb = -(-frames // BLOCK)
        imported = layout in (PLANAR_I16, PLANAR_F32, INTER_F32)
        want_layout = (INTER_I16 if depth == 16 else INTER_I24) if imported else layout
        both_ways = ch == 2 and mode == 2 and frames - (snb - 1) * BLOCK <= BOTH_WAYS
        out_cap = cap if exact else (pinned or frames * ch * (depth // 8) * 5 // 4 + snb * 64 + 4096)
        assert s == dict(frames=frames, num_blocks=snb, channels=ch, stereo_mode=mode if ch == 2 else 0, bit_depth=depth, layout=want_layout,
                         zero_run=1, partitioning=0, debug_skip=7, stream_base=nitems, first_block=nb, first_wg=nitems,
                         fuse_items=(snb - both_ways) * ch, pad=i, out_base=region, out_cap=out_cap, imported=int(imported), null_ptrs=1), i
        assert s["out_base"] % 4096 == 0
        spans.append((s["out_base"], s["out_base"] + s["out_cap"]))
        want_map += [i] * (snb * ch)
        region += _up(out_cap, 4096)
        nb, nitems = nb + snb, nitems + snb * ch
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])) and spans[-1][1] <= region
    assert (got["nb"], got["nitems"], got["max_depth"]) == (nb, nitems, max([16] + [it[2] for it in items]))
    assert got["item_stream"] == want_map
    assert (got["tab_bytes"], got["map_bytes"]) == (_up(len(items) * got["sizeof_desc"], 16), 2 * nitems)
    assert got["cap"] == dict(dev_payload=0, pinned_payload=region, prefix=0, pinned_fresh=0, ranges=0, table_blocks=nb, emitted=2 * nb, sizes=0,
                              batch_table=got["tab_bytes"] + got["map_bytes"])


def test_batch_layout_of_a_mixed_set():
    exact = [it[:-1] + (1000 * (i + 1) + i,) for i, it in enumerate(MIXED)]
    plain, small, asked, both, sixteen = _run((_batch_cmd(MIXED), _batch_cmd(MIXED, pinned=20000), _batch_cmd(exact, exact=True),
                                               _batch_cmd(exact, pinned=20000, exact=True), _batch_cmd(MIXED[:1] + MIXED[2:3])))
    _check_batch(plain, MIXED)
    _check_batch(small, MIXED, pinned=20000)
    _check_batch(asked, exact, exact=True)            # exact capacities are honoured ...
    _check_batch(both, exact, pinned=20000, exact=True)  # ... also over the knob
    _check_batch(sixteen, MIXED[:1] + MIXED[2:3])
    assert plain["max_depth"] == 24 and sixteen["max_depth"] == 16
    assert [s["out_cap"] for s in asked["streams"]] == [it[-1] for it in exact]


BAD_ITEMS = [
    (_item(BLOCK, d0=0), "left channel must not be empty"),
    (_item(0), "left channel must not be empty"),
    (_item(BLOCK, rate=12345), "unsupported sample rate: 12345"),
    (_item(BLOCK, depth=20), "unsupported bit depth: 20"),
    (_item(BLOCK, mode=3), "unsupported stereo mode: 3"),
    (_item(BLOCK, ch=3, d1=0), "unsupported channel count"),
    (_item(BLOCK, d1=0), "planar PCM: data1 must be the right channel of stereo input and null for mono"),
    (_item(BLOCK, ch=1, d1=1), "planar PCM: data1 must be the right channel of stereo input and null for mono"),
    (_item(BLOCK, depth=24, layout=INTER_I16), "PCM layout does not match the bit depth"),
    (_item(BLOCK, depth=16, layout=INTER_I24), "PCM layout does not match the bit depth"),
    (_item(BLOCK, layout=99), "unknown PCM layout"),
    (_item(BLOCK, layout=PLANAR_F32, d0=3), "refused by the import check"),
]


def test_batch_validation_messages():
    """One bad input per message, behind a good stream: the message names the stream and is the first complaint."""
    good = _item(BLOCK + 1)
    got = _run(tuple(_batch_cmd([good, bad]) for bad, _ in BAD_ITEMS) + (_batch_cmd([good, BAD_ITEMS[2][0], BAD_ITEMS[3][0]]),))
    assert [(g["rc"], g["msg"]) for g in got[:-1]] == [(1, "stream 1: " + msg) for _, msg in BAD_ITEMS]
    assert got[-1] == dict(rc=1, msg="stream 1: unsupported sample rate: 12345")


def test_batch_limits():
    limit = 0x7FFFFFFF // 16  # blocks of one job
    ok_small, over_one, over_two, too_many, most = _run((
        _batch_cmd([_item(BLOCK * 3)]),
        _batch_cmd([_item(BLOCK * (limit + 1))]),
        _batch_cmd([_item(BLOCK * (limit - 1)), _item(BLOCK * 2)]),
        _batch_cmd([_item(1, ch=1, mode=0)] * 65536),
        _batch_cmd([_item(1, ch=1, mode=0)] * 65535)))
    assert ok_small["rc"] == 0
    assert over_one == over_two == dict(rc=1, msg="too many blocks in one batch")
    assert too_many == dict(rc=1, msg="more than 65535 streams in one batch")
    assert most["rc"] == 0 and most["nitems"] == 65535 and most["item_stream"] == list(range(65535))


# ---- the lazy path's table ----
VALID, MS = 1 << 62, 1 << 61


def test_table_from_size_records():
    frames = [BLOCK, BLOCK, 777]
    sizes = [[1000, 2000], [3, 4], [50000, 60001]]
    recs = [VALID | (MS if b == 1 else 0) | by for b, row in enumerate(sizes) for by in row]
    missing = list(recs)
    missing[3] &= ~VALID  # a record whose valid bit never arrived
    mono = [VALID | 5, VALID | 6, VALID | 7]
    full, holed, one = _run((f"sizes 3 2 {' '.join(map(str, frames + recs))}", f"sizes 3 2 {' '.join(map(str, frames + missing))}",
                             f"sizes 3 1 {' '.join(map(str, frames + mono))}"))
    table = [v for f, row in zip(frames, sizes) for v in (f, sum(row))]
    assert full == dict(total=sum(map(sum, sizes)), complete=1, table=table, tail_bytes=7 + 110001, tail_empty=0)
    assert holed == dict(full, complete=0)
    assert one == dict(total=18, complete=1, table=[BLOCK, 5, BLOCK, 6, 777, 7], tail_bytes=13, tail_empty=0)
    empty, = _run((f"sizes 2 1 {BLOCK} 9 {VALID | 8} {VALID}",))  # a block of no bytes: the batch reports it
    assert empty == dict(total=8, complete=1, table=[BLOCK, 8, 9, 0], tail_bytes=0, tail_empty=1)
