"""The runs form of the decoder's host-side plan (csrc/decode_plan.h over csrc/runs_plan.h) without a device, driven through
the twin's export (tests/native/sim_runs.cpp): where the run finder's tables lie behind a salvage job's, what
plan_fill_tables puts into them, and what the list buffer reserves.  The plans of the existing forms are pinned by
test_decode_plan_host.py."""
import glob
import os

import numpy as np

import lacstreams
import runstwin as rw
import salvagetwin

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ITEM_T = np.dtype([("row0", "<u8"), ("det0", "<u4"), ("ndet", "<u4")])
LIST_T = np.dtype([("off", "<u8"), ("cap", "<u8"), ("count", "<u8")])


def _read(path):
    with open(path, "rb") as f:
        return f.read()


def _batch():
    lacs = [_read(p) for p in sorted(glob.glob(os.path.join(GOLDEN, "small", "*.lac")))[:6]]
    lacs.append(_read(os.path.join(GOLDEN, "decode_wav", "st16_lr_3blk.lac")))
    lacs.append(lacstreams.to_v2(lacs[-1]))
    lacs.append(lacs[-2][:-5])  # truncated: the plan still covers the whole table
    return lacs


def _dets(i):
    all_kinds = [rw.Det(rw.QUIET, rw.ALL, 3, 1), rw.Det(rw.PEAK, 0, 100, 3), rw.Det(rw.FLAT, 1, 0, 2), rw.Det(rw.QUIET, 0, 0, 5000), rw.Det(rw.QUIET, 1, 9, 1 << 60)]
    return (all_kinds * 2)[i % 3:i % 3 + 1 + i % 8]


def test_layout_and_filled_tables():
    lacs = _batch()
    per_item = [_dets(i) for i in range(len(lacs))]
    assert {len(d) for d in per_item} >= {1, 8}
    bad = b"XX" + lacs[0][2:]
    for cap in (rw.DEFAULT_CAP, 16):
        p = rw.plan(lacs[:4] + [bad] + lacs[4:], per_item[:4] + [per_item[0]] + per_item[4:], list_cap=cap)  # (the refused item is not laid out)
        ref = salvagetwin.plan_dump(lacs)
        m = ref["m"]
        frames = [it["frames"] for it in ref["items"]]
        tiles = [(f + rw.TILE - 1) // rw.TILE for f in frames]
        ndet = [len(d) for d in per_item]
        D = sum(ndet)
        # behind present [m], 16-byte aligned: tile_off [m + 1] | items [m] | dets [D] | lists [D] | rows; nothing behind the rows
        assert p["base"] == (ref["o_present"] + 4 * m + 15) // 16 * 16 and p["base"] % 16 == 0
        assert p["lists"] == p["base"] + 8 * (m + 1) + 16 * m + 16 * D and p["rows"] == p["lists"] + 24 * D
        assert (p["total_tiles"], p["total_dets"], p["total_rows"]) == (sum(tiles), D, sum(t * n for t, n in zip(tiles, ndet)))
        assert p["tables"] == p["rows"] + 4 * p["total_rows"] == len(p["raw"])
        raw = p["raw"]
        # everything in front of the runs tables is the salvage job's own
        assert np.array_equal(np.frombuffer(raw, "<u4", m, ref["o_present"]), ref["present"])
        assert np.array_equal(np.frombuffer(raw, "<u8", m + 1, ref["o_unit"]), ref["unit_off"])
        assert np.array_equal(np.frombuffer(raw, "<u8", len(ref["frame_off"]), ref["o_frame"]), ref["frame_off"])
        tile_off = np.frombuffer(raw, "<u8", m + 1, p["base"])
        assert tile_off.tolist() == np.concatenate([[0], np.cumsum(tiles)]).tolist()
        items = np.frombuffer(raw, ITEM_T, m, p["base"] + 8 * (m + 1))
        assert items["ndet"].tolist() == ndet and items["det0"].tolist() == np.concatenate([[0], np.cumsum(ndet)[:-1]]).tolist()
        assert items["row0"].tolist() == np.concatenate([[0], np.cumsum([t * n for t, n in zip(tiles, ndet)])[:-1]]).tolist()
        dets = np.frombuffer(raw, rw.DET_T, D, p["base"] + 8 * (m + 1) + 16 * m)
        flat = [d for ds in per_item for d in ds]
        assert [(int(d["kind"]), int(d["channel"]), int(d["level"]), int(d["min_frames"])) for d in dets] == [tuple(d) for d in flat]
        lists = np.frombuffer(raw, LIST_T, D, p["lists"])
        want = [rw.reserve(f, d.min_frames, cap) for f, ds in zip(frames, per_item) for d in ds]
        assert lists["cap"].tolist() == want and lists["off"].tolist() == np.concatenate([[0], np.cumsum(want)[:-1]]).tolist()
        assert not lists["count"].any() and p["runs_list"] == sum(want)
        assert not np.frombuffer(raw, "u1", offset=p["rows"]).any()  # the rows are zeroed with the rest
    assert 0 in want and any(0 < w < 16 for w in want) and 16 in want


def test_nothing_to_lay_out_for_refused_items():
    lac = _read(os.path.join(GOLDEN, "small", "n257_st16_ms.lac"))
    p = rw.plan([b"XX" + lac[2:], lac], [[rw.Det(rw.QUIET, rw.ALL, 0, 1)], [rw.Det(7, 0, 0, 1)]])
    assert (p["total_tiles"], p["total_dets"], p["total_rows"], p["runs_list"]) == (0, 0, 0, 0) and p["tables"] == p["rows"] == p["base"] + 8
