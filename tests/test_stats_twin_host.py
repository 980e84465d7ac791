"""Audio statistics without a device: the CPU twin (tests/native/sim_stats.cpp -- csrc/decode_plan.h's stats job,
csrc/stats_core.h accumulated as k_stats_blocks accumulates it with the wave and workgroup combination and the per-lane
path, csrc/stats_rows.h's rows and totals, every buffer at exactly the plan's capacity; plain and under AddressSanitizer +
UBSan as a program of its own) against expectations that never come from the code under test: numpy reductions and Python
ints over the PCM the streams and sources were made from (tests/statstwin.py).  Equality is exact everywhere."""
import os

import numpy as np
import pytest

import lacmutate
import lacstreams
import salvagetwin as st
import statstwin as sw

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GRIDS = (256, 257, 1000, 16384)


def _fixture(name):
    with open(os.path.join(GOLDEN, name), "rb") as f:
        return f.read()


def _layouts(depth):
    names = ["planar_i32", "planar_f32", "inter_f32", "inter_i16" if depth == 16 else "inter_i24"] + (["planar_i16"] if depth == 16 else [])
    return [(n, sw.LAYOUTS[n]) for n in names]


def _offsets(name):
    """Every base offset a layout permits, counted from a 16-byte aligned address."""
    step = 1 if name == "inter_i24" else 2 if name == "planar_i16" else 4
    return range(0, 16, step)


def test_the_signals_hold_what_statistics_are_about():
    sw.assert_content(sw.content_items())
    shapes = sw.shape_items()
    tots = [sw.expected_totals(sw.item_rows(it), it.channels, it.depth, it.rate) for it in shapes]
    big = [t for t in tots if t.frames >= 16]
    assert {t.lead % 4 for t in big} == {0, 1, 2, 3} and {t.trail % 4 for t in big} == {0, 1, 2, 3}
    assert any(t.ch[0][3] for t in tots) and len(shapes) == len(sw.FORMATS) * len(sw.SIZES)


# ---- unit level: the source form -----------------------------------------------------------------------------------
def _source_cases(channels, depth, wide):
    """(grid, frames, left, right, layout name, layout, offset) over the grids' border sizes; wide: every permitted offset."""
    for grid in GRIDS:
        counts = [1, 3, 4, 5, grid - 1, grid, grid + 1, grid + 3, 2 * grid - 1, 2 * grid + 2] if grid < 16384 else [16383, 16385, 2 * 16384 + 1]
        for frames in counts:
            room = frames >= 16
            seed = frames * 7 + grid
            left, right = sw.signal(frames, channels, depth, seed, lead=seed % 4 if room else 0, trail=(seed // 4) % 5 if room else 0)
            if room:
                sw.plant_full_scale(left, right, depth, (8, 11, grid - 1, grid))
            for name, layout in _layouts(depth):
                offsets = _offsets(name) if wide and grid < 16384 and frames <= grid + 3 else [0, 4 if name != "planar_i16" else 2]
                for off in offsets:
                    yield grid, frames, left, right, name, layout, off


@pytest.mark.parametrize("depth", [16, 24])
@pytest.mark.parametrize("channels", [1, 2])
def test_source_form_every_layout_offset_grid(channels, depth):
    """Every layout, channel count and depth at every base offset its alignment permits, in exact-size buffers, on grids
    256, 257, 1000 and 16384 with frame counts around the grid's multiples: every row and the totals are numpy's."""
    cases, wants = 0, {}
    for grid, frames, left, right, name, layout, off in _source_cases(channels, depth, True):
        if (grid, frames) not in wants:
            rows = sw.expected_rows(left, right, depth, sw.grid_blocks(frames, grid))
            wants[(grid, frames)] = (rows, sw.expected_totals(rows, channels, depth, 0))
        rows, totals, key, msg, _ = sw.source_rows(layout, channels, depth, grid, off, left, right)
        assert key == sw.CLEAN and msg == "" and rows == wants[(grid, frames)][0] and totals == wants[(grid, frames)][1], (name, grid, frames, off)
        cases += 1
    print("source cases:", cases)


def test_full_block_costs_sixteen_sets_of_atomics():
    """A 16384-frame block whose units start a workgroup: one set per workgroup, 16 in all; a straddled border adds the
    straddler's two records; a lone partial unit is one."""
    left, _ = sw.signal(16384, 1, 16, 5)
    assert sw.source_rows(sw.LAYOUTS["planar_i32"], 1, 16, 16384, 0, left)[4] == 16
    left, right = sw.signal(2 * 16384, 2, 24, 6)
    assert sw.source_rows(sw.LAYOUTS["inter_i24"], 2, 24, 16384, 1, left, right)[4] == 32
    left, _ = sw.signal(1000 + 1024, 1, 16, 7)  # grid 1000: the unit at frames 1000..1003 lies in block 1; waves 3 and 4 cross the border
    rows, _, _, _, sets = sw.source_rows(sw.LAYOUTS["planar_i32"], 1, 16, 1000, 0, left)
    assert [r.frames for r in rows] == [1000, 1000, 24] and sets > 3
    assert sw.source_rows(sw.LAYOUTS["planar_i32"], 1, 16, 256, 0, left[:3])[4] == 1


INVALID = (("planar_i32", 24, 0x01000000, "is outside the configured PCM bit depth", 0), ("planar_i32", 16, 0xFFFF0000, "is outside the configured PCM bit depth", 0),
           ("planar_f32", 24, 0x3E99999A, "is not an exact 24-bit PCM value", 1), ("inter_f32", 16, 0x3E99999A, "is not an exact 16-bit PCM value", 1))


def test_an_invalid_sample_fails_the_item_as_the_digest_form_words_it():
    """One planar int32 outside the depth, one inexact float: the key is digest_bad_key's (channel << 63 | frame << 1 | kind),
    the message the digest form's, the result zeroed and without rows."""
    for name, depth, word, what, kind in INVALID:
        for channels in (1, 2):
            for frame, ch in ((0, 0), (1001, channels - 1), (2000, 0)):
                left, right = sw.signal(2001, channels, depth, 11)
                rows, totals, key, msg, _ = sw.source_rows(sw.LAYOUTS[name], channels, depth, 1000, 4, left, right, bad=(frame, ch, word))
                assert key == (ch << 63) | (frame << 1) | kind, (name, frame, ch)
                assert msg == "%s sample at index %d %s" % ("right" if ch else "left", frame, what)
                assert rows == [] and totals == sw.Totals(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, (sw.ZERO_CH, sw.ZERO_CH))


def test_source_form_sanitized():
    """A selection of the unit-level cases, and the invalid samples, as a program under AddressSanitizer + UBSan: no
    report, and the answers of the plain build, which the tests above hold to numpy."""
    exe, why = sw.sanitized_exe()
    if exe is None:
        pytest.skip(why)
    cases, wants = [], []
    for depth in (16, 24):
        for channels in (1, 2):
            for grid, frames in ((256, 255), (256, 257), (257, 516), (1000, 2001), (257, 1), (16384, 16385)):
                left, right = sw.signal(frames, channels, depth, frames + grid, lead=frames % 4 if frames > 16 else 0, trail=3 if frames > 16 else 0)
                sw.plant_full_scale(left, right, depth, (4, 7, grid - 1, grid))
                for name, layout in _layouts(depth):
                    for off in (_offsets(name) if frames < 3000 else [0]):
                        cases.append(sw.source_case(layout, channels, depth, grid, off, left, right))
                        wants.append(sw.source_rows(layout, channels, depth, grid, off, left, right, as_line=True))
    for name, depth, word, _, _ in INVALID:
        left, right = sw.signal(2001, 2, depth, 11)
        for bad in ((0, 0, word), (1001, 1, word)):
            cases.append(sw.source_case(sw.LAYOUTS[name], 2, depth, 1000, 4, left, right, bad=bad))
            wants.append(sw.source_rows(sw.LAYOUTS[name], 2, depth, 1000, 4, left, right, bad=bad, as_line=True))
    lines, rc, err = sw.run_sanitized(cases, exe)
    assert rc == 0 and err == "", err
    for i, (got, want) in enumerate(zip(lines, wants)):
        assert got is not None and got.split(" ", 1)[1] == want, (i, got, want)


# ---- stream level -----------------------------------------------------------------------------------------------------
def _encode(oracle, it):
    return oracle.encode(it.left, it.right, it.rate, it.depth, 0)  # (left / right coding: full-scale samples in both channels)


@pytest.fixture(scope="module")
def streams(oracle):
    """[(name, stream, Item, block frames)]: the content signals, every format at every border size, and per format the
    spliced three-block stream of 257 / 258 / 259 frames."""
    out = []
    for it in sw.content_items() + sw.shape_items():
        out.append((it.name, _encode(oracle, it), it, sw.grid_blocks(it.left.size)))
    for ch, depth, rate in sw.FORMATS:
        parts = sw.spliced_parts(ch, depth)
        lacs = [oracle.encode(l, r, rate, depth, 0) for l, r in parts]
        it = sw.Item("splice|%dch%d" % (ch, depth), ch, depth, rate, np.concatenate([l for l, _ in parts]),
                     np.concatenate([r for _, r in parts]) if ch == 2 else None)
        out.append((it.name, lacstreams.splice(lacstreams.splice(lacs[0], lacs[1]), lacs[2]), it, [257, 258, 259]))
    return out


def _check(name, item, it, blocks, lost=None):
    want = sw.expected_rows(it.left, it.right, it.depth, blocks, lost)
    assert item.code == 0 and item.rows == want, name
    assert item.totals == sw.expected_totals(want, it.channels, it.depth, it.rate), name


def test_streams_rows_and_totals(streams):
    """The content and the shapes as batches, forward and reversed, so that items and blocks start inside other items'
    waves and workgroups: every row and every total is numpy's, with 1 and 64 columns and both status fills."""
    for order, cols, zero in ((streams, 1, False), (streams[::-1], 64, True)):
        for at in range(0, len(order), 32):
            part = order[at:at + 32]
            items, _ = sw.run([lac for _, lac, _, _ in part], cols=cols, zero_status=zero)
            for (name, _, it, blocks), item in zip(part, items):
                _check(name, item, it, blocks)


def _damaged():
    """The recipes of the block digests' device test: a damaged block between two good ones, a truncated stream, a clean
    one and its version-2 form."""
    lac = _fixture("decode_wav/st16_lr_3blk.lac")
    ent, pays = lacmutate._payloads(lac)
    pays[1] = pays[1][:1] + bytes([0x7F]) + pays[1][2:] if lac[4] == 2 else bytes([0x7F]) + pays[1][1:]
    return [lacmutate._rebuild(lac, ent, pays), lac[:-5], lac, lacstreams.to_v2(lac)]


def test_lost_and_missing_blocks(oracle):
    """Lost rows are zeroed with their codes, the totals are over the decoded blocks, and a lost block counts as sound for
    the lead / trail rule; a refused container is refused by the plan with the parser's text."""
    lacs = _damaged()
    exps = [st.expected(oracle, x) for x in lacs]
    assert exps[0].lost == [False, True, False] and exps[1].lost == [False, False, True] and not any(exps[2].lost) and not any(exps[3].lost)
    refused = b"XX" + lacs[2][2:]
    items, _ = sw.run(lacs + [refused])
    for x, exp, item in zip(lacs, exps, items):
        blocks = [n for n, _ in lacmutate.table(x)[1]]
        it = sw.Item("", x[3], x[8], st.rate(x), exp.left, exp.right)
        assert [r.code != 0 for r in item.rows] == exp.lost
        _check("", item, it, blocks, [r.code for r in item.rows])
        assert item.totals.lost_blocks == sum(exp.lost) and item.totals.lost_frames == sum(n for n, l in zip(blocks, exp.lost) if l)
    assert items[1].rows[2].code == 10 and 1 <= items[0].rows[1].code <= 9 and items[1].totals.trail == 0
    assert items[2].rows == items[3].rows and items[2].totals == items[3].totals
    assert items[4].code == 1 and items[4].message == "[decode-error] invalid frame header" and items[4].rows is None


def test_sanitized_twin_agrees_and_stays_inside_its_buffers(streams):
    """Every stream above and the damaged ones as a program of their own under AddressSanitizer + UBSan: no report with
    every buffer -- the accumulator rows among them -- at exactly the plan's capacity, and the plain build's answers."""
    exe, why = sw.sanitized_exe()
    if exe is None:
        pytest.skip(why)
    lacs = [lac for _, lac, _, _ in streams] + _damaged()
    sw.cleared("host", lacs + lacs[::-1])
    cases = [sw.case(lacs[:8])]
    lines, rc, err = sw.run_sanitized(cases, exe)
    assert rc == 0 and err == "", err  # (cleared asserts the exit code; the stderr of a clean run is empty)
