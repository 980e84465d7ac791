"""The decoder's host-side plan (csrc/decode_plan.h: plan_decode, plan_fill_tables) without a device: the code that
decides where the decode kernels read and write, driven through the twin's exports (tests/native/sim_decode.cpp).

Window range: every window between candidate boundaries against a brute force over the block table.  Layout: a mixed batch
(stereo v3, mono v3, v2, one bad item) in every form, with and without pad-to-waves -- alignments, disjoint ranges, table
sections, prefix sums, lanes, capacities.  Batch twin: the lane code over such plans, every buffer at exactly the plan's
capacity, plain and under AddressSanitizer + UBSan (a child program), against sim_decode of each stream alone -- which
test_decode_mutants_host.py judges against the oracle."""
import glob
import itertools
import os
import struct

import numpy as np
import pytest

import dectwin
import lacgrammar as g
import lacstreams

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BAD = b"LA\x03" + bytes(29)  # does not parse
BAD_MESSAGE = "[decode-error] invalid frame header"


def _read(path):
    with open(path, "rb") as f:
        return f.read()


def _streams():
    out = {os.path.basename(p)[:-4]: _read(p) for d in ("small", "decode_wav") for p in sorted(glob.glob(os.path.join(GOLDEN, d, "*.lac")))}
    out.update({"v2:" + n: lacstreams.to_v2(g.build(n).lac) for n in g.V2_SUBSET})
    return out


STREAMS = _streams()


def _table(lac):
    """[(frames, bytes)] per block; bytes is None in version 2."""
    nb = struct.unpack(">I", lac[10:14])[0]
    if lac[2] == 3:
        return [struct.unpack(">II", lac[14 + 8 * b:22 + 8 * b]) for b in range(nb)]
    return [(struct.unpack(">I", lac[14 + 4 * b:18 + 4 * b])[0], None) for b in range(nb)]


def _brute(lac, start, frames):
    """What a window must decode: (blk_first, blocks, pay_src, pay_bytes, decoded frames, the window's start in them)."""
    tab = _table(lac)
    if lac[2] == 2:  # no compressed sizes: the whole stream
        return 0, len(tab), 0, len(lac) - 14 - 4 * len(tab), sum(n for n, _ in tab), start
    f0 = by0 = 0
    hit = []  # (block, its first frame, its first byte) of every block that holds a frame of the window
    for b, (n, by) in enumerate(tab):
        if f0 < start + frames and start < f0 + n:
            hit.append((b, f0, by0))
        f0, by0 = f0 + n, by0 + by
    first, last = hit[0], hit[-1]
    return (first[0], len(hit), first[2], last[2] + tab[last[0]][1] - first[2],
            last[1] + tab[last[0]][0] - first[1], start - first[1])


def _boundaries(lac):
    total, edges, f0 = sum(n for n, _ in _table(lac)), set(), 0
    for n, _ in _table(lac):
        f0 += n
        edges.update((f0 - 1, f0, f0 + 1))
    edges.update((0, total - 1))
    return sorted(e for e in edges if 0 <= e < total)


@pytest.mark.parametrize("name", sorted(STREAMS))
def test_window_block_range_against_brute_force(name):
    """Every window whose first and last frame both lie among: every block border -1 / 0 / +1, frame 0, the last frame."""
    lac = STREAMS[name]
    edges = _boundaries(lac)
    wins = [(a, b - a + 1) for a, b in itertools.combinations_with_replacement(edges, 2)]
    p = dectwin.plan_dump([lac] * len(wins), "device", windows=wins, sample_type=dectwin.I32)
    assert p["m"] == len(wins) and not any(p["rc"])
    for j, (it, win) in enumerate(zip(p["items"], wins)):
        got = (it["blk_first"], it["blocks"], it["pay_src"], it["pay_bytes"], it["frames"], it["win_start"])
        assert got == _brute(lac, *win), (name, win)
        assert it["win_frames"] == win[1] and int(p["window"][j]["start"]) == it["win_start"]
        if lac[2] == 2:
            assert (it["blk_first"], it["blocks"], it["frames"]) == (0, len(_table(lac)), sum(n for n, _ in _table(lac)))


def test_a_stream_that_does_not_parse_keeps_its_message():
    p = dectwin.plan_dump([BAD], "host")
    assert p["m"] == 0 and p["rc"] == [1] and p["msg"] == [BAD_MESSAGE]


# ---- layout ----
MIXED = ["n16421_st16", "n33_mono16", "v2:sweep_03" if "sweep_03" in g.V2_SUBSET else "v2:" + g.V2_SUBSET[0], None, "st24_ms_20481", "n257_st16_ms"]
JOBS = [("wav", dectwin.WHOLE), ("device", dectwin.WHOLE), ("host", dectwin.WHOLE), ("verify", dectwin.WHOLE),
        ("device", dectwin.F32), ("host", dectwin.I32)]


def _mixed():
    return [BAD if n is None else STREAMS[n] for n in MIXED]


def _disjoint(ranges):
    ranges = sorted(ranges)
    return all(a[1] <= b[0] for a, b in zip(ranges, ranges[1:]))


def _up(v, k):
    return (v + k - 1) // k * k


@pytest.mark.parametrize("pad_waves", [False, True])
@pytest.mark.parametrize("form,sample_type", JOBS)
def test_layout_of_a_mixed_batch(form, sample_type, pad_waves):
    lacs = _mixed()
    window = sample_type != dectwin.WHOLE
    totals = [sum(n for n, _ in _table(x)) if x is not BAD else 1 for x in lacs]
    wins = [(len(x) % 7, min(5000, t - len(x) % 7)) for x, t in zip(lacs, totals)] if window else None  # (some across a border)
    p = dectwin.plan_dump(lacs, form, windows=wins, sample_type=sample_type, pad_waves=pad_waves)
    bad = MIXED.index(None)
    # the bad item is absent from the device list and keeps its own message
    assert p["rc"] == [int(i == bad) for i in range(len(lacs))] and p["msg"][bad] == BAD_MESSAGE
    assert [it["src"] for it in p["items"]] == [i for i in range(len(lacs)) if i != bad]
    m, T, items, rec = p["m"], p["total_blocks"], p["items"], p["item"]
    own_pcm = form != "device" or window
    # PCM: from a multiple of 4 frames, disjoint, the total the sum of the rounded sizes
    if own_pcm:
        assert all(it["pcm_at"] % 4 == 0 for it in items)
        assert _disjoint([(it["pcm_at"], it["pcm_at"] + it["frames"]) for it in items])
        assert p["pcm_total"] == sum(_up(it["frames"], 4) for it in items) == p["need_pcm"]
        for j, it in enumerate(items):
            assert int(rec[j]["left"]) == dectwin.base(1) + 4 * it["pcm_at"]
            assert int(rec[j]["right"]) == (dectwin.base(2) + 4 * it["pcm_at"] if rec[j]["channels"] == 2 else 0)
    else:
        assert p["need_pcm"] == 0
        for j, it in enumerate(items):
            assert int(rec[j]["left"]) == dectwin.base(4, it["src"])
            assert int(rec[j]["right"]) == (dectwin.base(5, it["src"]) if rec[j]["channels"] == 2 else 0)
    # images: 16-byte aligned (WAV), disjoint, inside the stated capacity
    if form == "wav" or (form == "host" and window):
        spans = [(it["image_at"], it["image_at"] + it["image_size"]) for it in items]
        assert _disjoint(spans) and max(e for _, e in spans) <= p["need_image"] and p["need_image"] % 16 == 0
        if form == "wav":
            assert all(a % 16 == 0 for a, _ in spans)
            assert [int(r["wav"]) for r in rec] == [dectwin.base(3) + a for a, _ in spans]
            for it, r in zip(items, rec):
                data = int(r["frames"]) * int(r["channels"]) * (int(r["bit_depth"]) // 8)
                assert it["image_size"] == 44 + data + (data & 1)
        else:
            for j, (a, _) in enumerate(spans):
                w = p["window"][j]
                assert int(w["left"]) == dectwin.base(3) + a and a % 4 == 0
                assert int(w["right"]) == (dectwin.base(3) + a + 4 * int(w["frames"]) if rec[j]["channels"] == 2 else 0)
    else:
        assert p["need_image"] == 0
        assert all(int(r["wav"]) == 0 for r in rec)
    if form == "device" and window:
        assert [int(w["left"]) for w in p["window"]] == [dectwin.base(4, it["src"]) for it in items]
    # table sections: in order, disjoint, inside the size; the 8-byte tables 8-aligned
    lanes, nv2 = p["lanes"], p["nv2"]
    sections = [(p["o_items"], p["sizeof_item"] * m), (p["o_byte"], 8 * (T + 1)), (p["o_frame"], 8 * (T + 1)), (p["o_unit"], 8 * (m + 1)),
                (p["o_bitem"], 4 * T), (p["o_lane"], 4 * lanes), (p["o_v2"], 4 * nv2)]
    if window:
        sections.append((p["o_win"], p["sizeof_window"] * m))
    if form == "verify":
        sections += [(p["o_win"], p["sizeof_source"] * m), (p["o_res"], p["sizeof_words"] * m)]
    for (a, n), (b, _) in zip(sections, sections[1:]):
        assert a + n <= b
    assert sections[-1][0] + sections[-1][1] <= p["o_size"] == p["need_tables"] == len(p["raw"])
    assert all(p[k] % 8 == 0 for k in ("o_items", "o_byte", "o_frame", "o_unit", "o_win", "o_res"))
    # prefix sums
    byte_off, frame_off = p["byte_off"].astype(np.int64), p["frame_off"].astype(np.int64)
    assert byte_off[0] == 0 and frame_off[0] == 0 and int(byte_off[T]) == p["total_pay"] and int(frame_off[T]) == p["total_frames"]
    assert (np.diff(byte_off) >= 0).all() and (np.diff(frame_off) > 0).all()
    assert p["need_blocks"] == T == sum(it["blocks"] for it in items)
    for j, it in enumerate(items):
        r, lac = rec[j], lacs[it["src"]]
        b0, nb = int(r["block0"]), int(r["blocks"])
        assert (int(r["frame0"]), int(r["pay_off"])) == (int(frame_off[b0]), int(byte_off[b0]))
        assert (p["blk_item"][b0:b0 + nb] == j).all()
        tab = _table(lac)[it["blk_first"]:it["blk_first"] + nb]
        assert np.diff(frame_off[b0:b0 + nb + 1]).tolist() == [n for n, _ in tab]
        if r["version"] == 2:  # one lump at the item's last block
            assert np.diff(byte_off[b0:b0 + nb + 1]).tolist() == [0] * (nb - 1) + [it["pay_bytes"]]
            assert int(r["pay_bits"]) == 8 * it["pay_bytes"] == 8 * (len(lac) - it["head"])
        else:
            assert np.diff(byte_off[b0:b0 + nb + 1]).tolist() == [by for _, by in tab]
        assert int(p["unit_off"][j + 1] - p["unit_off"][j]) == (it["frames"] + 3) // 4
    assert p["total_units"] == (0 if (form in ("device", "host") and not window) else int(p["unit_off"][m]))
    # lanes: every v3 block exactly once, an item's blocks in consecutive lanes; with padding every item starts a wave
    lane_blk = p["lane_blk"].tolist()
    v3 = [j for j in range(m) if rec[j]["version"] == 3]
    assert p["v2_items"].tolist() == [j for j in range(m) if rec[j]["version"] == 2] and nv2 >= 1
    real = [b for b in lane_blk if b != 0xFFFFFFFF]
    assert sorted(real) == sorted(b for j in v3 for b in range(int(rec[j]["block0"]), int(rec[j]["block0"] + rec[j]["blocks"])))
    assert len(real) == len(set(real))
    for j in v3:
        at = lane_blk.index(int(rec[j]["block0"]))
        assert lane_blk[at:at + int(rec[j]["blocks"])] == list(range(int(rec[j]["block0"]), int(rec[j]["block0"] + rec[j]["blocks"])))
        assert not pad_waves or at % 64 == 0
    if pad_waves:
        assert len(lane_blk) > len(real)  # the fillers are ~0 (and nothing else is: `real` above)
    else:
        assert lane_blk == real
    # capacities
    assert p["need_payload"] == p["total_pay"] + p["tail_pad"] and p["tail_pad"] == dectwin.tail_pad()
    assert p["total_pay"] == sum(it["pay_bytes"] for it in items)
    assert _disjoint([(int(r["pay_off"]), int(r["pay_off"]) + it["pay_bytes"]) for r, it in zip(rec, items)])
    assert p["need_stage"] == (p["total_pay"] if window else 0)
    if form == "verify":
        assert [(int(s["data0"]), int(s["data1"]), int(s["layout"])) for s in p["source"]] == \
            [(dectwin.base(6, it["src"]), dectwin.base(7, it["src"]), 0) for it in items]
        assert all(int(w["count"]) == 0 and int(w["key"]) == 2 ** 64 - 1 for w in p["words"])


@pytest.mark.parametrize("name", ["n4096_st16", "n33_mono16", "st24_ms_20481"])
def test_verify_wav_source_lies_behind_the_pad(name):
    lac = STREAMS[name]
    src_bytes = sum(n for n, _ in _table(lac)) * lac[3] * (lac[8] // 8)
    p = dectwin.plan_dump([lac], "verify", host_src_bytes=src_bytes)
    assert p["m"] == 1 and p["host_src_bytes"] == src_bytes
    assert p["src_at"] % 16 == 0 and p["total_pay"] + p["tail_pad"] <= p["src_at"] < p["total_pay"] + p["tail_pad"] + 16
    assert p["need_payload"] >= p["src_at"] + src_bytes
    assert int(p["source"][0]["data0"]) == dectwin.base(0) + p["src_at"] and int(p["source"][0]["layout"]) == (1 if lac[8] == 16 else 2)


# ---- the batch twin ----
def _alone(lac):
    return dectwin.decode(lac)


def _batch_jobs():
    """(streams, windows or None, pad_waves, never_lean, cols)"""
    lacs = _mixed()
    jobs = [(lacs, None, pad, lean, cols) for pad, lean, cols in ((False, False, 1), (True, True, 64), (True, False, 1))]
    wins = []
    for lac in lacs:
        if lac is BAD:
            wins.append((0, 1))
            continue
        edges = _boundaries(lac)
        wins.append((edges[len(edges) // 2] - 1, 3) if len(edges) > 2 else (0, 1))
    jobs += [(lacs, wins, pad, False, 64 if pad else 1) for pad in (False, True)]
    big = STREAMS["st24_ms_20481"]  # one stream, every border window, as one job
    bw = [(e - 1, 2) for e in _boundaries(big) if 1 <= e < sum(n for n, _ in _table(big)) - 1]
    jobs.append(([big] * len(bw), bw, False, False, 1))
    return jobs


def test_batch_twin_equals_every_stream_alone():
    """Plain build: each item's PCM, flags and statuses from sim_decode_batch are what sim_decode gives for that stream
    alone (a window: the blocks it covers, and the window cut out of them)."""
    for lacs, wins, pad, lean, cols in _batch_jobs():
        items, over = dectwin.decode_batch(lacs, wins, pad_waves=pad, never_lean=lean, cols=cols)
        assert over <= 25
        for i, (lac, it) in enumerate(zip(lacs, items)):
            assert it.refused == (lac is BAD)
            if it.refused:
                continue
            want = _alone(lac)
            fr = [n for n, _ in _table(lac)]
            f0, f1 = sum(fr[:it.blk_first]), sum(fr[:it.blk_first + it.blocks])
            assert np.array_equal(it.status, want.status[it.blk_first:it.blk_first + it.blocks]) and not it.status.any()
            assert np.array_equal(it.ms, want.ms[it.blk_first:it.blk_first + it.blocks])
            assert np.array_equal(it.left, want.left[f0:f1])
            assert (want.right is None and it.right is None) or np.array_equal(it.right, want.right[f0:f1])
            if wins:
                s, n = wins[i]
                assert (it.frames, f0 + it.start) == (n, s)
                assert np.array_equal(it.left[it.start:it.start + n], want.left[s:s + n])


def test_batch_twin_sanitized():
    """The same jobs through the sanitized child program, every buffer at exactly the plan's capacity: no report, and the
    lines (hashes of every item's PCM, statuses, overshoot) of the plain build."""
    exe, why = dectwin.sanitized_exe()
    if exe is None:
        pytest.skip(why)
    cases = [dectwin.batch_case(*job) for job in _batch_jobs()]
    lines, rc, err = dectwin.run_sanitized_batches(cases, exe=exe)
    assert rc == 0 and "ERROR" not in err and "runtime error" not in err, err
    assert lines == [dectwin.batch_digest(c, i) for i, c in enumerate(cases)]
    assert all("-" in ln.split(" ", 2)[2].split(";") for ln in lines[:5])  # the bad item of the mixed batches is refused
