"""Runs without a device: the CPU twin (tests/native/sim_runs.cpp -- csrc/decode_plan.h's runs job, csrc/runs_core.h combined
as k_runs combines it with the lane scan, the step across waves, the append with its capacity test and the second run with
exact capacities, csrc/runs_rows.h's stitching and totals, every buffer at exactly the plan's capacity; plain and under
AddressSanitizer + UBSan as a program of its own) against expectations that never come from the code under test: a boolean
numpy mask per detector and the run lengths from its differences, over the PCM the streams and sources were made from
(tests/runstwin.py).  Equality is exact for every run, every total and every result field."""
import pytest

import runstwin as rw


def _layouts(depth):
    names = ["planar_i32", "planar_f32", "inter_f32", "inter_i16" if depth == 16 else "inter_i24"] + (["planar_i16"] if depth == 16 else [])
    return [(n, rw.LAYOUTS[n]) for n in names]


def _offsets(name):
    """Every base offset a layout permits, counted from a 16-byte aligned address."""
    step = 1 if name == "inter_i24" else 2 if name == "planar_i16" else 4
    return range(0, 16, step)


def test_the_signals_hold_what_they_are_for():
    rw.assert_content()


# ---- the source form --------------------------------------------------------------------------------------------------
def _check_source(it, dets, layout, off, cap=rw.DEFAULT_CAP, flags=0):
    want, lists = rw.expected_result(dets, it.left, it.right, it.depth, 0, rw.grid_blocks(it.left.size), flags=flags)
    res, got, key, msg = rw.source_runs(layout, it.channels, it.depth, off, it.left, it.right, dets, list_cap=cap)
    assert key == rw.CLEAN and msg == "" and got == lists and res == want, (it.name, layout, off)


@pytest.mark.parametrize("channels,depth,rate", rw.FORMATS)
def test_source_form_every_layout_at_every_offset(channels, depth, rate):
    """The border item with its eight detectors in every layout at every base offset its alignment permits, in buffers
    that end with the source's last byte; the border sizes in every layout at two offsets."""
    it = rw.border_item(channels, depth, rate)
    for name, layout in _layouts(depth):
        for off in _offsets(name):
            _check_source(it, rw.border_detectors(depth), layout, off)
    for it in rw.shape_items():
        if (it.channels, it.depth) == (channels, depth):
            for name, layout in _layouts(depth):
                for off in (0, 4 if name != "planar_i16" else 2):
                    _check_source(it, rw.shape_detectors(), layout, off)


def test_source_form_alternation_reaches_the_bound_and_reruns_under_a_small_cap():
    it = rw.alternating_item()
    dets = [rw.Det(rw.QUIET, rw.ALL, 0, 1), rw.Det(rw.QUIET, rw.ALL, 0, 2)]
    _check_source(it, dets, rw.LAYOUTS["planar_i32"], 0)
    _check_source(it, dets, rw.LAYOUTS["inter_i16"], 4, cap=16, flags=rw.RERUN)
    assert rw.lib().sim_runs_reserve(rw.ALT_FRAMES, 1, rw.DEFAULT_CAP) == (rw.ALT_FRAMES + 1) // 2


def test_every_frame_and_mono_right():
    for ch, depth, rate in rw.FORMATS:
        _check_source(rw.every_frame_item(ch, depth, rate), rw.every_frame_detectors(depth), rw.LAYOUTS["planar_i32"], 0)
    mono = rw.border_item(1, 16, 44100)
    dets = [rw.Det(rw.QUIET, 1, rw.LEVEL, 1), rw.Det(rw.FLAT, 1, 0, 1), rw.Det(rw.PEAK, 1, 0, 1), rw.Det(rw.QUIET, 0, rw.LEVEL, 1)]
    res, lists, _, _ = rw.source_runs(rw.LAYOUTS["inter_i16"], 1, 16, 0, mono.left, None, dets)
    assert lists[:3] == [[], [], []] and lists[3] and res.totals[0] == rw.Totals(0, 0, 0, 0)


INVALID = (("planar_i32", 24, 0x01000000, "is outside the configured PCM bit depth", 0), ("planar_i32", 16, 0xFFFF0000, "is outside the configured PCM bit depth", 0),
           ("planar_f32", 24, 0x3E99999A, "is not an exact 24-bit PCM value", 1), ("inter_f32", 16, 0x3E99999A, "is not an exact 16-bit PCM value", 1))


def test_an_invalid_sample_fails_the_item_as_the_digest_form_words_it():
    dets = [rw.Det(rw.QUIET, rw.ALL, 3, 1), rw.Det(rw.FLAT, rw.ALL, 0, 1)]
    for name, depth, word, what, kind in INVALID:
        for channels in (1, 2):
            for frame, ch in ((0, 0), (1024, channels - 1), (2000, 0)):  # (1024: a tile's first frame, which the tile in front loads too)
                left, right = rw.loud(2001, channels, depth, 11)
                res, lists, key, msg = rw.source_runs(rw.LAYOUTS[name], channels, depth, 4, left, right, dets, bad=(frame, ch, word))
                assert key == (ch << 63) | (frame << 1) | kind, (name, frame, ch)
                assert msg == "%s sample at index %d %s" % ("right" if ch else "left", frame, what)
                assert lists == [[], []] and res == rw.Result(0, 0, 0, 0, 0, 0, 0, 0, 0, (rw.Totals(0, 0, 0, 0),) * 8)


def test_source_form_sanitized():
    """A selection of the cases above, the rerun and the invalid samples, as a program under AddressSanitizer + UBSan: no
    report, and the answers of the plain build, which the tests above hold to numpy."""
    exe, why = rw.sanitized_exe()
    if exe is None:
        pytest.skip(why)
    cases, wants = [], []

    def add(*args, **kw):
        cases.append(rw.source_case(*args, **kw))
        wants.append(rw.source_runs(*args, as_line=True, **kw))
    for ch, depth, rate in rw.FORMATS:
        it = rw.border_item(ch, depth, rate)
        for name, layout in _layouts(depth):
            for off in _offsets(name):
                add(layout, ch, depth, off, it.left, it.right, rw.border_detectors(depth))
        for it in rw.shape_items():
            if (it.channels, it.depth) == (ch, depth) and it.left.size < 2000:
                for name, layout in _layouts(depth):
                    add(layout, ch, depth, 4 if name != "planar_i16" else 2, it.left, it.right, rw.shape_detectors())
    alt = rw.alternating_item()
    add(rw.LAYOUTS["planar_i16"], 1, 16, 2, alt.left, None, [rw.Det(rw.QUIET, rw.ALL, 0, 1)], list_cap=16)
    for name, depth, word, _, _ in INVALID:
        left, right = rw.loud(2001, 2, depth, 11)
        for bad in ((0, 0, word), (1024, 1, word)):
            add(rw.LAYOUTS[name], 2, depth, 4, left, right, [rw.Det(rw.FLAT, rw.ALL, 0, 1)], bad=bad)
    lines, rc, err = rw.run_sanitized(cases, exe)
    assert rc == 0 and err == "", err
    for i, (got, want) in enumerate(zip(lines, wants)):
        assert got is not None and got.split(" ", 1)[1] == want, (i, got, want)


# ---- stream level -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def streams(oracle):
    return rw.build_streams(oracle)


def test_streams_batches_forward_and_reversed(streams):
    """Everything as batches, forward and reversed, so that items begin and end with runs beside other items' runs (they
    must not join), with 1 and 64 columns and both status fills: every run, total and result field is numpy's."""
    for order, cols, zero in ((streams, 1, False), (streams[::-1], 64, True)):
        for at in range(0, len(order), 32):
            part = order[at:at + 32]
            items = rw.run([x[1] for x in part], [x[4] for x in part], cols=cols, zero_status=zero)
            for (name, _, it, blocks, dets), item in zip(part, items):
                rw.check_item(name, item, it, blocks, dets)
    names = [x[0] for x in streams]
    assert any(n.startswith("v2|") for n in names) and len({(x[2].channels, x[2].depth) for x in streams}) == 4


def test_forced_small_capacity_reruns_with_the_complete_list(streams):
    """R = 16: the alternation's 1025 runs (and the border item's) outgrow the lists, the tiles run once more with the
    counters' capacities, LACX_RUNS_RERUN is set for the job's items and every list is complete."""
    part = [x for x in streams if x[0].startswith(("alternating", "borders|2ch16", "n3|"))]
    items = rw.run([x[1] for x in part], [x[4] for x in part], list_cap=16)
    for (name, _, it, blocks, dets), item in zip(part, items):
        rw.check_item(name, item, it, blocks, dets, flags=rw.RERUN)
    alt = next(item for x, item in zip(part, items) if x[0].startswith("alternating"))
    assert alt.result.totals[0].runs == (rw.ALT_FRAMES + 1) // 2 > 16
    # without the knob nothing outgrows anything: the reservation is exact
    assert all(item.result.flags == 0 for item in rw.run([x[1] for x in part], [x[4] for x in part]))


def test_lost_and_missing_blocks(oracle):
    """A lost block splits a run, the first frame behind it is never FLAT, and a refused container is refused by the plan
    with the parser's text."""
    cases = rw.damaged(oracle)
    refused = b"XX" + cases[0][1][2:]
    items = rw.run([x[1] for x in cases] + [refused], [x[2] for x in cases] + [rw.lossy_detectors()])
    lost = {}
    for (name, lac, dets), item in zip(cases, items):
        lost[name] = rw.check_damaged(oracle, name, lac, dets, item).lost
        assert item.result.flags == 0
    assert lost["lost1|2ch16"] == [False, True, False] and lost["lost0|2ch16"] == [True, False, False] and lost["cut|2ch16"] == [False, False, True]
    assert lost["lost1-v2|2ch16"] == [False, True, True] and not any(lost["clean|1ch24"])
    by = {name: item for (name, _, _), item in zip(cases, items)}
    assert by["lost1|2ch16"].lists[0] == [(240, 17), (515, 25)] and by["lost1|2ch16"].lists[1] == [(241, 16), (516, 24)]
    assert by["clean|2ch16"].lists[1] == [(241, 299)] and by["cut|2ch16"].lists[3] == [(0, 515)] and by["lost0|2ch16"].lists[3] == [(257, 517)]
    assert items[-1].code == 1 and items[-1].message == "[decode-error] invalid frame header" and items[-1].lists is None


def test_refused_detectors_fail_their_item_alone(streams):
    name, lac, it, blocks, dets = streams[0]
    items = rw.run([lac, lac, lac], [dets, [rw.Det(3, 0, 0, 1)], [rw.Det(rw.FLAT, 0, 1, 1)]])
    rw.check_item(name, items[0], it, blocks, dets)
    assert (items[1].code, items[1].message) == (1, "unknown detector kind") and (items[2].code, items[2].message) == (1, "flat detector takes no level")


def test_sanitized_twin_agrees_and_stays_inside_its_buffers(streams, oracle):
    """Every stream above and the damaged ones as a program of their own under AddressSanitizer + UBSan: no report with
    every buffer -- the tables and the list buffer among them -- at exactly the plan's capacity, under the default and the
    forced small R, and the plain build's answers."""
    exe, why = rw.sanitized_exe()
    if exe is None:
        pytest.skip(why)
    lacs = [x[1] for x in streams] + [x[1] for x in rw.damaged(oracle)]
    dets = [x[4] for x in streams] + [x[2] for x in rw.damaged(oracle)]
    rw.cleared("host", lacs + lacs[::-1], dets + dets[::-1])
    rw.cleared("host-small", lacs, dets, list_cap=16)
