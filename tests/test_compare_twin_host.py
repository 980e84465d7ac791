"""Bit-compare without a device: the CPU twin (tests/native/sim_compare.cpp -- csrc/decode_plan.h's compare job and
csrc/compare_plan.h's tables, csrc/compare_core.h run as k_compare_search and k_compare_rows run it, csrc/compare_rows.h's
choice and totals, every buffer at exactly the plan's capacity; plain and under AddressSanitizer + UBSan as a program of its
own) against expectations that never come from the code under test: the definition restated in numpy and Python integers
(tests/comparetwin.py).  Everything is exact: counts, rows and totals are compared byte for byte, no tolerance.

The whole corpus runs in the source form (planar int32: what the decoder's staging is once k_ms_inverse ran), a set of pairs
in every layout that holds their depth; the stream form -- the decode in front of the same kernels -- runs on pairs of every
format, and on a job with a damaged stream."""
import numpy as np
import pytest

import comparetwin as ct
import lacmutate


@pytest.fixture(scope="module")
def small_out():
    """The small corpus as ONE source job of the plain twin."""
    ps = ct.small_corpus()
    src, recs = ct.job(ps)
    return list(zip(ps, ct.run(ct.source_case(src, recs))))


def test_the_corpus_holds_its_classes():
    """On the expectation alone: every class the issue names is there, so that no test passes vacuously."""
    ps = ct.corpus()
    by = {p.name: p for p in ps}
    assert ct.TILE == ct.lib().sim_cmp_tile_frames() and ct.ROW == ct.lib().sim_cmp_row_frames() and ct.MAX_RADIUS == ct.lib().sim_cmp_max_radius()
    want = set(range(1, 10)) | {4095, 4096, 4097, ct.TILE - 1, ct.TILE, ct.TILE + 1, 16383, 16384, 16385, 2 * 16384 + 5}
    assert {p.a.shape[1] for p in ps if p.name.startswith("len|") and "longer" not in p.name} == want
    for n in want:  # na != nb in both directions
        assert by["len|%d" % n].a.shape[1] < by["len|%d" % n].b.shape[1] and by["len|%d|longer-a" % n].a.shape[1] > by["len|%d|longer-a" % n].b.shape[1]
    assert {(p.a.shape[0], p.depth) for p in ps} == {(1, 16), (2, 16), (1, 24), (2, 24)}
    for depth in (16, 24):  # both ends of the range: |d| reaches 2^b - 1
        for ch in (1, 2):
            assert int(ct.expected(by["range|%d|%d" % (depth, ch)]).totals["peak"]) == (1 << depth) - 1
    w = ct.expected(by["identical"])
    assert w.offset == 0 and int(w.totals["mismatches"]) == 0 and int(w.counts[8]) == 0 and w.counts[:8].all() and w.counts[9:].all()
    assert by["same-index"].same and by["same-index"].a is by["same-index"].b and ct.job([by["same-index"]])[1][0][:2] == (0, 0)
    # planted offsets: the unique minimum of the restatement, with and without differing samples
    planted = {}
    for p in ps:
        if p.planted is None:
            continue
        w = ct.expected(p)
        at = p.planted - (p.centre - p.radius)
        assert w.offset == p.planted and (np.delete(w.counts, at) > w.counts[at]).all(), p.name
        planted.setdefault(p.planted, set()).add(int(w.counts[at]) == 0)
    assert all(planted[o] == {True, False} for o in ct.PLANTED)
    for r in (1, 127, 128, 300):  # +- radius exactly
        assert by["edge|+%d" % r].planted == by["edge|+%d" % r].radius == r and by["edge|-%d" % r].planted == -r
    assert by["edge|centre"].planted == by["edge|centre"].centre + by["edge|centre"].radius and by["edge|centre"].centre != 0
    # a tie: two offsets with equal counts at equal distance, the larger wins; the restatement's rule and the twin's agree
    for name in ("tie", "tie|mono"):
        w, p = ct.expected(by[name]), by[name]
        k = w.offset - (p.centre - p.radius)
        mirror = 2 * p.radius - k
        assert w.offset > p.centre and w.counts[mirror] == w.counts[k] == w.counts.min(), name
        assert ct.twin_choose(w.counts, p.centre, p.radius) == w.offset
    # a window beyond both streams entirely: every offset counts all non-zero samples
    for name in ("beyond", "beyond|negative"):
        p = by[name]
        every = int(np.count_nonzero(p.a)) + int(np.count_nonzero(p.b))
        assert p.centre != 0 and abs(p.centre) - p.radius > max(p.a.shape[1], p.b.shape[1]) and (ct.expected(p).counts == every).all()
        assert ct.expected(p).offset == p.centre
    assert {0, 1, 127, 128, 300, 600} <= {p.radius for p in ps}
    assert ct.twin_plan(6000, 6000, 0, 300).otiles == 1 and ct.twin_plan(6000, 6000, 0, 600).otiles == 2  # more than one offset tile
    big = by["r32767"]
    assert big.radius == ct.MAX_RADIUS and 2000 <= big.a.shape[1] <= 5000 and ct.expected(big).offset == big.planted
    # where the differences lie
    t = ct.expected(by["right-only"]).totals
    assert int(t["ch"][0]["mismatches"]) == 0 and int(t["ch"][1]["mismatches"]) == 4 and int(t["rows_differ"]) == 3
    t = ct.expected(by["lead-only"]).totals
    assert int(t["lead"]) == 5 and int(t["lead_side"]) == ct.SIDE_B and int(t["tail"]) == 0 and int(t["first"]) == -5 and int(t["last"]) == -1
    t = ct.expected(by["tail-only"]).totals
    assert int(t["tail"]) == 7 and int(t["tail_side"]) == ct.SIDE_B and int(t["lead"]) == 0 and int(t["first"]) >= 9000 and int(t["offset"]) == 0
    r = ct.expected(by["row-last-frame"]).rows
    assert len(r) == 2 and int(r["ch"][0][0]["first"]) == int(r["ch"][0][0]["last"]) == ct.ROW - 1 and int(r["ch"][1][0]["mismatches"]) == 0


# the mistakes the corpus catches, and for each one pair that sees it (the restatement made wrong that way answers differently)
SEEN_BY = {
    "no zero-extension at the start": "len|5|longer-a",
    "no zero-extension at the end": "len|6",
    "< for <= at the last offset": "edge|-128",
    "a B window one frame short": "tail-only",
    "o mod 4 != 0 read as aligned": "shift|3|diffs",
    "a negative frame rounded toward zero": "shift|-3",
    "24-bit stereo compared on one word": "shift|-2|diffs",
    "frames counted instead of samples": "radius|1",
    "lanes behind the last offset added in": "edge|+300",
    "a row's position relative to the row": "mono24|row2",
    "the wrong tie rule": "tie",
}


def test_the_corpus_sees_every_named_mistake(small_out):
    by = {p.name: p for p in ct.corpus()}
    got = {p.name: g for p, g in small_out}
    assert set(SEEN_BY) == set(ct.MISTAKES)
    for kind, name in SEEN_BY.items():
        assert ct.sees(by[name], kind), (kind, name)
        ct.check(by[name], got[name], kind)  # and the twin is on the right side of it
    p = by["shift|-2|diffs"]
    assert p.depth == 24 and p.a.shape[0] == 2


def test_the_twin_is_the_restatement_byte_for_byte(small_out):
    for p, got in small_out:
        ct.check(p, got)
    assert sum(1 for p, g in small_out if len(g.counts) == 0) >= 5  # radius 0: not searched


def test_answers_do_not_depend_on_the_batch(small_out):
    """A pair's answer is the same bytes alone, and in the batch reversed."""
    ps = ct.small_corpus()[::-1]
    src, recs = ct.job(ps)
    for p, g in zip(ps, ct.run(ct.source_case(src, recs))):
        ct.check(p, g, "reversed")
    pick = next(p for p in ps if p.name == "shift|257|diffs")
    (alone,) = ct.run(ct.source_case(*ct.job([pick])))
    ct.check(pick, alone, "alone")


def test_the_largest_radius():
    p = next(p for p in ct.corpus() if p.name == "r32767")
    for o in (-32767, -3001, 0, 2999, 19999, 20000, 32767):  # the wide restatement is the plain one
        assert int(ct.counts(p)[o + 32767]) == ct.mismatches(p.a, p.b, o) == ct.mismatches_restricted(p.a, p.b, o)
    (got,) = ct.run(ct.source_case(*ct.job([p])))
    ct.check(p, got)


def test_one_source_in_many_pairs():
    by = {p.name: p for p in ct.corpus()}
    x = by["shift|3"]
    others = [by["shift|3"].b, by["shift|-3|diffs"].b if by["shift|-3|diffs"].a.shape == x.a.shape and by["shift|-3|diffs"].depth == x.depth else x.b, x.a]
    src = [(x.a, x.depth, x.rate)] + [(b, x.depth, x.rate) for b in others]
    recs = [(0, 1, 0, 8), (0, 2, 0, 8), (0, 3, 0, 8), (1, 0, 0, 8), (0, 0, 2, 1)]
    out = ct.run(ct.source_case(src, recs))
    for (a, b, c, r), g in zip(recs, out):
        ct.check(ct.Pair("many|%d|%d" % (a, b), src[a][0], src[b][0], c, r, x.depth, x.rate), g)
    assert int(out[0].totals["offset"]) == 3 and int(out[3].totals["offset"]) == -3 and int(out[2].totals["mismatches"]) == 0


LAYOUT_PAIRS = ("shift|3|diffs", "shift|-2|diffs", "shift|-1", "shift|2", "len|7", "len|4097", "len|9|longer-a", "mono24|row2", "range|24|2", "range|16|1", "radius|300")
LAYOUTS = ((ct.I16, (0, 4)), (ct.I24, (0, 1, 6)), (ct.P16, (0, 2, 6)), (ct.PF32, (0, 4)), (ct.IF32, (0, 8)), (ct.P32, (4, 12)))


def layout_cases():
    by = {p.name: p for p in ct.corpus()}
    ps = [by[n] for n in LAYOUT_PAIRS]
    src, recs = ct.job(ps)
    return [(layout, off, ps, ct.source_case(src, recs, layout, off)) for layout, offs in LAYOUTS for off in offs]


def test_every_layout_gives_the_planar_answer():
    """Every layout that holds the depth, at a nonzero byte offset, every source ending at the end of its allocation."""
    for layout, off, ps, case in layout_cases():
        assert any(ct.layout_for(layout, p.depth) == layout for p in ps)
        for p, g in zip(ps, ct.run(case)):
            ct.check(p, g, (layout, off))


def invalid_cases():
    by = {p.name: p for p in ct.corpus()}
    ps = [by["shift|1"], by["shift|-1|diffs"], by["identical"]]
    src, recs = ct.job(ps)
    return ps, [(ct.source_case(src, recs, ct.P32, 0, (2, 17, 0, 0x01000000)), "source 2: left sample at index 17 is outside the configured PCM bit depth"),
                (ct.source_case(src, recs, ct.PF32, 0, (3, 5000, 0, 0x3E99999A)), "source 3: left sample at index 5000 is not an exact 16-bit PCM value")]


def test_an_invalid_sample_fails_its_pairs_alone():
    ps, cases = invalid_cases()
    for case, text in cases:
        a, b, c = ct.run(case)
        assert b.code == 1 and b.text == text and b.rows is None and not b.totals.tobytes().strip(b"\0")
        ct.check(ps[0], a)
        ct.check(ps[2], c)


# ---- the stream form ---------------------------------------------------------------------------------------------------
STREAM_PAIRS = ("shift|3|diffs", "shift|-2|diffs", "shift|-1", "shift|2", "len|7", "len|16385", "len|4097|longer-a", "same-index", "tail-only", "mono24|row2", "radius|300",
                "beyond")


@pytest.fixture(scope="module")
def streams(oracle):
    by = {p.name: p for p in ct.corpus()}
    ps = [by[n] for n in STREAM_PAIRS]
    return ps, {p.name: ct.encode(oracle, ct.job([p])[0]) for p in ps}


def stream_job(ps, lacs_by):
    lacs, recs = [], []
    for p in ps:
        mine = lacs_by[p.name]
        recs.append((len(lacs), len(lacs) + len(mine) - 1, p.centre, p.radius))
        lacs += mine
    return lacs, recs


def test_stream_form_is_the_source_form_behind_a_decode(streams):
    ps, lacs_by = streams
    for order in (slice(None), slice(None, None, -1)):
        lacs, recs = stream_job(ps[order], lacs_by)
        for p, g in zip(ps[order], ct.run(ct.stream_case(lacs, recs))):
            ct.check(p, g)


def _broken(lac):
    """The stream with one byte of its second block's payload changed: that block does not decode."""
    ent, pays = lacmutate._payloads(lac)
    pays[1] = pays[1][:1] + bytes([0x7F]) + pays[1][2:] if lac[4] == 2 else bytes([0x7F]) + pays[1][1:]
    return lacmutate._rebuild(lac, ent, pays)


def damaged_case(oracle):
    """Three streams of 17000 frames, the middle one damaged; pairs (0, 2), (0, 1), (1, 1), (2, 0)."""
    xs = [ct.noise(17000, 2, 16, 9000), ct.noise(17000, 2, 16, 9001)]
    xs.append(ct.plant(ct.shifted(xs[0], 2), [(1, 9000)], 9002))
    lacs = ct.encode(oracle, [(x, 16, 44100) for x in xs])
    lacs[1] = _broken(lacs[1])
    return xs, lacs, [(0, 2, 0, 4), (0, 1, 0, 4), (1, 1, 0, 0), (2, 0, -1, 3)]


def test_a_damaged_stream_fails_its_pairs_alone(oracle):
    xs, lacs, recs = damaged_case(oracle)
    a, b, c, d = ct.run(ct.stream_case(lacs, recs))
    assert b.code == 2 and b.text.startswith("source 1: status ") and b.rows is None and not b.totals.tobytes().strip(b"\0")
    assert c.code == 2 and c.text.startswith("source 1: status ")
    ct.check(ct.Pair("damaged|02", xs[0], xs[2], 0, 4), a)
    ct.check(ct.Pair("damaged|20", xs[2], xs[0], -1, 3), d)
    assert int(a.totals["offset"]) == 2 and int(d.totals["offset"]) == -2
    bad = [lacs[0], b"XX" + lacs[1][2:], lacs[2]]
    a, b, c, d = ct.run(ct.stream_case(bad, recs))
    assert b.code != 0 and b.text == "source 1: [decode-error] invalid frame header"
    ct.check(ct.Pair("damaged|02", xs[0], xs[2], 0, 4), a)


def test_sanitized(streams, oracle):
    """The sanitized program passes every shape that later goes to the device -- the whole corpus as sources, the layouts, the
    invalid samples, the stream pairs forward and reversed, the damaged job -- with no report and the plain build's answers,
    which the tests above hold to numpy."""
    exe, why = ct.sanitized_exe()
    assert exe, why
    ps, lacs_by = streams
    small = ct.small_corpus()
    cases = [ct.source_case(*ct.job(small[at:at + 12])) for at in range(0, len(small), 12)] + [ct.source_case(*ct.job(small[::-1][:9]))]
    cases += [ct.source_case(*ct.job([p])) for p in ct.corpus() if p.name == "r32767"]
    cases += [c for _, _, _, c in layout_cases()] + [c for c, _ in invalid_cases()[1]]
    cases += [ct.stream_case(*stream_job(ps, lacs_by)), ct.stream_case(*stream_job(ps[::-1], lacs_by))]
    xs, lacs, recs = damaged_case(oracle)
    cases.append(ct.stream_case(lacs, recs))
    lines, rc, err = ct.run_sanitized(cases, exe)
    assert rc == 0, err
    for i, c in enumerate(cases):
        assert lines[i] is not None and lines[i].split(" ", 1)[1] == ct.line(c, i).split(" ", 1)[1], i
    print("sanitized cases:", len(cases))
