"""Bit-compare on the host alone: the plan (csrc/compare_plan.h through tests/native/sim_compare.cpp) -- layout, tile counts,
capacities and every refusal with its text -- and lacx_compare_combine of the product's library against Python integers,
128-bit sums included.  No device."""
import ctypes as C

import numpy as np
import pytest

import __graft_entry__ as ge
import comparetwin as ct


@pytest.fixture(scope="module")
def lx():
    return ge.load_pkg().lacx


def test_abi_sizes(lx):
    for name, t, size in (("compare_pair", lx.ComparePair, 24), ("compare_channel_row", lx.CompareChannelRow, 48), ("compare_row", lx.CompareRow, 96),
                          ("compare_channel", lx.CompareChannel, 72), ("compare", lx.Compare, 296)):
        assert lx.lib().lacx_sizeof(name.encode()) == C.sizeof(t) == size
    assert (ct.ROW_T.itemsize, ct.TOTAL_T.itemsize) == (C.sizeof(lx.CompareRow), C.sizeof(lx.Compare))
    assert lx.COMPARE_NONE == ct.NONE and lx.COMPARE_MAX_RADIUS == ct.MAX_RADIUS and lx.COMPARE_ROW_FRAMES == ct.ROW


def test_radius_0_plans_no_search():
    p = ct.twin_plan(5000, 7000, 0, 0)
    assert (p.rc, p.tiles, p.spans, p.counts) == (0, 0, 0, 0) and p.rows == 1
    p = ct.twin_plan(5000, 7000, -40000, 0)  # B lies 40000 frames in front of A: the domain is [0, 47000)
    assert p.rows == (47000 + ct.ROW - 1) // ct.ROW and p.tiles == 0
    p = ct.twin_plan(16384, 16384, 0, 0)
    assert p.rows == 1 and ct.twin_plan(16385, 3, 0, 0).rows == 2


def test_the_split_of_a_workgroup():
    """The smallest power of two of lanes, four offsets each, that holds the pair's offsets from a multiple of 4 on."""
    for centre, radius, lanes, otiles in ((0, 1, 2, 1), (1, 1, 1, 1), (0, 2, 2, 1), (0, 3, 2, 1), (0, 4, 4, 1), (0, 127, 64, 1), (0, 128, 128, 1), (0, 300, 256, 1),
                                          (0, 511, 256, 1), (0, 512, 256, 2), (2, 510, 256, 1), (0, 32767, 256, 64), (1, 32767, 256, 65)):
        p = ct.twin_plan(6000, 6000, centre, radius)
        first = (centre - radius) // 4 * 4
        slots = centre + radius - first + 1
        assert (p.lanes, p.otiles) == (lanes, otiles) and 4 * p.lanes * p.otiles >= slots > 4 * p.lanes * (p.otiles - 1), (centre, radius)
        assert p.counts == 2 * radius + 1 and p.bound_ok


def test_spans_and_tiles():
    """The stretches of A's axis on which A or the B window can be non-zero, rounded out to multiples of 4; one span where
    they touch, two where a gap lies between them; tiles of the search tile's frames times the offset tiles."""
    T = ct.TILE
    p = ct.twin_plan(6000, 6000, 0, 300)
    assert p.span_at == [(-300, 6300)] and p.tiles == (6600 + T - 1) // T
    p = ct.twin_plan(6001, 10, 0, 2)  # B's window [-2, 12) inside A's [0, 6001)
    assert p.span_at == [(-4, 6004)]
    p = ct.twin_plan(700, 900, 5000, 40)  # B's window [-5040, -4060): a gap to A
    assert p.span_at == [(-5040, -4060), (0, 700)] and p.tiles == 1 + 1
    p = ct.twin_plan(700, 900, -5000, 3)
    assert p.span_at == [(0, 700), (4996, 5904)]
    p = ct.twin_plan(T, T, 0, 600)  # two offset tiles
    assert p.otiles == 2 and p.span_at == [(-600, T + 600)] and p.tiles == 2 * ((T + 1200 + T - 1) // T)
    for na, nb, c, r in ((1, 1, 0, 1), (T - 1, T + 1, 3, 7), (3000, 23000, 0, 32767), (2 ** 32 - 1, 2 ** 32 - 1, 0, 0), (100, 100, 2 ** 31 - 2, 1)):
        p = ct.twin_plan(na, nb, c, r)
        assert p.rc == 0 and p.bound_ok and all(lo % 4 == 0 and hi % 4 == 0 and lo < hi for lo, hi in p.span_at)


def test_the_rows_capacity_holds_every_offset():
    """The plan reserves the rows of the longest domain of the range; the domain is longest at one of its ends."""
    for na, nb, c, r in ((5000, 7000, 0, 300), (40000, 100, -20000, 32767), (16384, 16384, 0, 1), (9, 16385, 16380, 5)):
        p = ct.twin_plan(na, nb, c, r)
        most = max((max(na, nb - o) - min(0, -o) + ct.ROW - 1) // ct.ROW for o in range(c - r, c + r + 1))
        assert p.rows == most, (na, nb, c, r)
    one = ct.twin_plan(5000, 7000, 0, 300)
    assert one.size >= 2 * 40 + 48 + 32 + 16 + 16 + 8 * 601 + 96 * one.rows  # sources, pair, span, tile_off, row_off, counts, rows


def test_every_refusal_with_its_text():
    f = (44100, 2, 16)
    for kw, text in ((dict(ia=0, ib=2), "sources outside the call's array"), (dict(ia=5, ib=0, nsrc=5), "sources outside the call's array"),
                     (dict(fmt_b=(44100, 1, 16)), "channel counts differ (2, 1)"), (dict(fmt_a=(44100, 2, 24)), "bit depths differ (24, 16)"),
                     (dict(fmt_a=(44100, 1, 24), fmt_b=(48000, 2, 16)), "channel counts differ (1, 2)"), (dict(fmt_b=(48000, 2, 16)), "sample rates differ (44100, 48000)"),
                     (dict(radius=32768), "radius above 32767"), (dict(centre=2 ** 31), "centre out of range"), (dict(centre=-2 ** 31), "centre out of range"),
                     (dict(centre=2 ** 31 - 1, radius=1), "centre out of range"), (dict(centre=-(2 ** 31 - 5), radius=5), "centre out of range"),
                     (dict(centre=2 ** 40), "centre out of range"), (dict(na=2 ** 32), "source 0 holds 2^32 frames or more"),
                     (dict(nb=2 ** 32 + 7), "source 1 holds 2^32 frames or more")):
        args = dict(na=1000, nb=1000, centre=0, radius=0, fmt_a=f, fmt_b=f)
        args.update(kw)
        p = ct.twin_plan(**args)
        assert (p.rc, p.why) == (-1, text), kw
    assert ct.twin_plan(1000, 1000, 2 ** 31 - 2, 1).rc == 0 and ct.twin_plan(1000, 1000, -(2 ** 31 - 1), 0).rc == 0 and ct.twin_plan(1000, 1000, 0, 32767).rc == 0
    assert ct.twin_plan(1000, 1000, 0, 0, ia=0, ib=0, nsrc=1).rc == 0  # a == b is allowed


def test_the_tie_rule():
    for counts, centre, want in (([5, 5, 5], 0, 0), ([3, 5, 3], 0, 1), ([3, 5, 3, 9, 9], 10, 10), ([3, 5, 4, 9, 9], 10, 8), ([3, 5, 4, 5, 3], -2, -4 + 4), ([2, 9, 9, 9, 9, 9, 2], 0, 3),
                                 ([9, 1, 9, 9, 9, 1, 9], 5, 7), ([1, 9, 9, 9, 9, 9, 2], 0, -3), ([7], 4, 4)):
        r = len(counts) // 2
        assert ct.twin_choose(counts, centre, r) == ct.choose(np.array(counts, np.uint64), centre, r) == want, counts


def _rows_of(recs):
    rws = np.zeros(len(recs), ct.ROW_T)
    rws["ch"]["first"] = rws["ch"]["last"] = rws["ch"]["max_at"] = ct.NONE
    for k, chans in enumerate(recs):
        for c, rec in chans.items():
            rws["ch"][k][c] = rec
    return rws


def test_combine_against_python_integers(lx):
    """lacx_compare_combine of the product, the twin's and Python integers on rows whose sums pass 2^64 and 2^65."""
    big = 2 ** 64 - 5
    rws = _rows_of([{0: (3, 16000, 3, big, big, 900, 2 ** 25 - 1), 1: (0, 1, 1, 7, 49, 2, 7)}, {}, {0: (2 * ct.ROW + 1, 2 * ct.ROW + 9, 2 * ct.ROW + 9, big, big, 5, 2 ** 25 - 1)},
                    {0: (3 * ct.ROW, 3 * ct.ROW + 1, 3 * ct.ROW, big, 10, 2, 11), 1: (3 * ct.ROW + 4, 3 * ct.ROW + 4, 3 * ct.ROW + 4, 1, 1, 1, 2 ** 25 - 1)}])
    na, nb, o = 3 * ct.ROW + 100, 3 * ct.ROW + 40, 77  # the domain [-77, 3 ROW + 100): four rows
    p = ct.Pair("combine", np.zeros((2, na), np.int32), np.zeros((2, nb), np.int32), 0, 0, 24, 96000)
    want = ct.totals(p, o, rws)
    assert int(want["sum_abs_hi"]) == 2 and int(want["ch"][0]["sum_sq_hi"]) == 2 and int(want["ch"][0]["sum_sq_lo"]) == 0 and int(want["peak_channel"]) == 0 and int(want["peak_at"]) == 3 - 77
    assert int(want["rows_differ"]) == 3 and int(want["first"]) == -77 and int(want["lead"]) == 77 and int(want["lead_side"]) == ct.SIDE_B and int(want["tail_side"]) == ct.SIDE_A
    twin = ct.twin_combine(rws, 2, 24, 96000, na, nb, o)
    assert twin.tobytes() == want.tobytes()
    rows = [lx.CompareRow.from_buffer_copy(rws[k].tobytes()) for k in range(len(rws))]
    got = lx.compare_combine(rows, 2, 24, 96000, na, nb, o)
    assert bytes(got) == want.tobytes()
    assert got.sum_abs == 3 * big + 8 and got.sum_sq == 2 * big + 60 and not got.identical
    assert got.peak_dbfs == pytest.approx(20 * np.log10((2 ** 25 - 1) / 2 ** 23)) and got.rms_dbfs == pytest.approx(10 * np.log10((2 * big + 60) / (2 * got.domain_frames) / 2.0 ** 46))
    # mono: channel 1 is not looked at; nothing differs: zeros and -inf
    got = lx.compare_combine(rows[1:2], 1, 16, 44100, 100, 100, 0)
    assert got.identical and got.rows == 1 and got.rows_differ == 0 and got.peak_dbfs == float("-inf") and got.rms_dbfs == float("-inf") and got.lead == got.tail == 0
    for args, text in (((rows, 3, 24, 96000, na, nb, o), "unsupported channel count"), ((rows, 2, 20, 96000, na, nb, o), "unsupported bit depth: 20"),
                       ((rows[:3], 2, 24, 96000, na, nb, o), "row count is not the domain's"), ((rows, 2, 24, 96000, 2 ** 32, nb, o), "frames or offset out of range")):
        with pytest.raises(ValueError, match=text):
            lx.compare_combine(*args)


def test_combine_is_the_corpus_totals(lx):
    """From the restatement's rows the product's totals are the restatement's, on pairs of every format."""
    by = {p.name: p for p in ct.corpus()}
    for name in ("shift|3|diffs", "shift|-2|diffs", "range|24|2", "range|16|1", "lead-only", "tail-only", "right-only", "beyond", "len|1", "identical"):
        p, w = by[name], ct.expected(by[name])
        rows = [lx.CompareRow.from_buffer_copy(w.rows[k].tobytes()) for k in range(len(w.rows))]
        got = lx.compare_combine(rows, p.a.shape[0], p.depth, p.rate, p.a.shape[1], p.b.shape[1], w.offset)
        assert bytes(got) == w.totals.tobytes(), name
