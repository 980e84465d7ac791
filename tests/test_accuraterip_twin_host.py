"""Rip checksums without a device: the CPU twin (tests/native/sim_accuraterip.cpp -- csrc/decode_plan.h's rip-checksum job and
csrc/accuraterip_plan.h's tables, csrc/accuraterip_core.h run as k_accuraterip runs it, every buffer at exactly the plan's
capacity; plain and under AddressSanitizer + UBSan as a program of its own) against expectations that never come from the code
under test: the definition restated in numpy's uint64 and, for v1 and s450, prefix sums (tests/artwin.py).  Everything is
exact: sums are compared byte for byte, no tolerance.

The whole corpus runs in the source form (planar int32: what the decoder's staging is once k_ms_inverse ran), discs with
source seams in every layout that holds 16-bit audio; the stream form -- the decode in front of the same kernel -- runs on the
discs that differ in how sources and tracks partition them, and on a disc with a damaged stream."""
import numpy as np
import pytest

import artwin as aw
import lacmutate


_same, check = aw.same, aw.check


@pytest.fixture(scope="module")
def small_out():
    """The small corpus as ONE source job of the plain twin."""
    discs = aw.small_corpus()
    return list(zip(discs, aw.run(aw.source_case(discs))))


def test_the_corpus_holds_its_classes():
    """On the expectation alone: every class the issue names is there."""
    discs = aw.corpus()
    by = {d.name: d for d in discs}
    assert {d.radius for d in discs if d.name.startswith("three|")} == set(aw.RADII)
    assert {(d.first, d.last) for d in discs if d.name.startswith("flags|")} == {(a, b) for a in (False, True) for b in (False, True)}
    # partial discs read zeros in front of frame 0 and behind the last frame
    s, n, lo, hi, _ = aw.ranges(by["flags|00"])[0]
    assert s + (-300) + lo - 1 < 0
    s, n, lo, hi, _ = aw.ranges(by["flags|00"])[2]
    assert s + 300 + hi - 1 >= sum(aw.THREE)
    # sources and tracks: one source, one per track, five under two tracks with no boundary in common and two seams inside one window
    assert len(by["three|r0"].sources) == 1 and len(by["three|r0"].tracks) == 3
    assert by["per-track"].tracks is None and len(by["per-track"].sources) == 3
    seams = np.cumsum(aw.SEAMS)[:-1]
    assert len(aw.SEAMS) == 5 and len(aw.SEAM_TRACKS) == 2 and aw.SEAM_TRACKS[0] not in seams
    assert aw.SEAMS[1] < by["seams"].radius and aw.SEAMS[2] < by["seams"].radius and seams[2] - seams[0] < 2 * by["seams"].radius + 1
    assert any(int(s) % 4 for s in seams)  # a source that starts at no multiple of 4: units straddle it
    # short tracks: empty and one-term ranges as first, last and only track
    count = lambda r: max(r[3] - r[2] + 1, 0)  # noqa: E731
    for n in aw.EDGE_LENGTHS:
        first, last, only = (aw.ranges(by["edge|%s%d" % (w, n)]) for w in ("first", "last", "only"))
        assert (count(first[0]), bool(first[0][4] & aw.TRACK_SHORT)) == (max(n - 2939, 0), n < 2940)
        assert (count(last[2]), bool(last[2][4] & aw.TRACK_SHORT)) == (max(n - 2940, 0), n < 2941)
        assert (count(only[0]), bool(only[0][4] & aw.TRACK_SHORT)) == (max(n - 5879, 0), n < 5880)
    assert {1, 0} <= {count(r) for n in aw.EDGE_LENGTHS for w in ("first", "last", "only") for r in aw.ranges(by["edge|%s%d" % (w, n)])}
    # a middle track on either side of the multiplier tile
    M = aw.lib().sim_ar_tile_mults()
    assert {aw.ranges(by["tile|%d" % n])[1][3] for n in aw.TILE_LENGTHS} >= {M - 1, M, M + 1}
    # contents: the largest high halves, zeros, noise
    assert (aw.words(by["ones"]) == 0xFFFFFFFF).all() and (aw.words(by["lowest"]) == 0x80008000).all() and not aw.words(by["zeros"]).any()
    assert int(aw.expected(by["ones"]).v2[1][128]) != int(aw.expected(by["ones"]).v1[1][128])
    assert not aw.expected(by["zeros"]).v2.any()
    # the big track: the smallest order with an s450, held at 2939 by the prefix sums and at 8 by the definition
    assert aw.BIG >= aw.S450_MIN > aw.BIG - 1000 and by["big|r2939"].radius == 2939 and by["big|r8"].radius == 8
    assert not aw.ranges(by["big|r8"])[0][4] and all(aw.ranges(d)[0][4] & aw.TRACK_NO_S450 for d in aw.small_corpus())
    assert aw.disc_expected(by["big|r2939"]).v2 is None and aw.disc_expected(by["big|r8"]).s450.any()
    assert any(aw.expected_ids(aw.track_frames(d), d.first, d.last, d.lba0) != (0, 0, 0) for d in discs)


def test_the_twin_is_the_restatement_bit_for_bit(small_out):
    for disc, got in small_out:
        check(disc, got)
    assert sum(1 for d, g in small_out if any(f & aw.TRACK_SHORT for f in g.tracks["flags"])) >= 9


def test_sums_do_not_depend_on_the_batch(small_out):
    """A disc's sums are the same bits alone, and in the batch reversed."""
    discs = aw.small_corpus()[::-1]
    back = aw.run(aw.source_case(discs))
    fwd = {d.name: g for d, g in small_out}
    for d, g in zip(discs, back):
        assert _same(g.v1, fwd[d.name].v1) and _same(g.v2, fwd[d.name].v2) and _same(g.s450, fwd[d.name].s450), d.name
    pick = next(d for d in discs if d.name == "seams")
    (alone,) = aw.run(aw.source_case([pick]))
    assert _same(alone.v2, fwd["seams"].v2)


def test_the_big_track():
    """266 000 frames: at radius 2939 v1 and s450 are the prefix sums', v2 is Python integers' at a handful of offsets; at
    radius 8 all three are the definition's; and the two runs agree where they overlap."""
    by = {d.name: d for d in aw.corpus()}
    (wide,) = aw.run(aw.source_case([by["big|r2939"]]))
    (narrow,) = aw.run(aw.source_case([by["big|r8"]]))
    check(by["big|r2939"], wide)
    check(by["big|r8"], narrow)
    mid = slice(2939 - 8, 2939 + 9)
    assert _same(wide.v1[:, mid], narrow.v1) and _same(wide.v2[:, mid], narrow.v2) and _same(wide.s450[:, mid], narrow.s450)
    for o in (-2939, -301, 2939):
        assert int(wide.v2[0][o + 2939]) == aw.v2_bigint(by["big|r2939"], 0, o), o


LAYOUTS = ((aw.I16, (0, 4)), (aw.P16, (0, 2, 6)), (aw.PF32, (0, 4)), (aw.IF32, (0, 8)), (aw.P32, (4, 12)))


def layout_cases():
    by = {d.name: d for d in aw.corpus()}
    discs = [by["seams"], by["seams|partial"], by["three|r31"], by["edge|only5881"]]
    return [(layout, off, discs, aw.source_case(discs, layout, off)) for layout, offs in LAYOUTS for off in offs]


def test_every_layout_gives_the_planar_sums():
    for layout, off, discs, case in layout_cases():
        for d, g in zip(discs, aw.run(case)):
            check(d, g, (layout, off))


def invalid_cases():
    by = {d.name: d for d in aw.corpus()}
    discs = [by["three|r1"], by["seams"], by["per-track"]]
    return [(aw.source_case(discs, aw.P32, 0, (1, 3, 17, 1, 0x00010000)), "source 3: right sample at index 17 is outside the configured PCM bit depth"),
            (aw.source_case(discs, aw.PF32, 0, (1, 0, 5000, 0, 0x3E99999A)), "source 0: left sample at index 5000 is not an exact 16-bit PCM value"),
            (aw.source_case(discs, aw.P32, 0, (1, 1, 98, 0, 0xFFFF0000)), "source 1: left sample at index 98 is outside the configured PCM bit depth")]


def test_an_invalid_sample_fails_its_disc_alone():
    by = {d.name: d for d in aw.corpus()}
    for case, text in invalid_cases():
        a, b, c = aw.run(case)
        assert b.code == 1 and b.text == text and b.v1 is None and not b.result.tobytes().strip(b"\0")
        check(by["three|r1"], a)
        check(by["per-track"], c)


# ---- the stream form ---------------------------------------------------------------------------------------------------
STREAM_DISCS = ("three|r32", "per-track", "seams", "seams|partial", "sectors", "edge|only5880", "tile|4097")


def encode(oracle, disc):
    return [oracle.encode(l, r, 44100, 16, 2) for l, r in disc.sources]


@pytest.fixture(scope="module")
def streams(oracle):
    by = {d.name: d for d in aw.corpus()}
    discs = [by[n] for n in STREAM_DISCS]
    return discs, [encode(oracle, d) for d in discs]


def test_stream_form_is_the_source_form_behind_a_decode(streams):
    """One job of the discs, forward and reversed: a disc's streams lie side by side in the decoder's buffers, a track
    boundary need not be a stream boundary, and an offset reaches into the neighbouring stream."""
    discs, lacs = streams
    for order in (slice(None), slice(None, None, -1)):
        for d, g in zip(discs[order], aw.run(aw.stream_case(discs[order], lacs[order]))):
            check(d, g)


def _broken(lac):
    """The stream with one byte of its second block's payload changed: that block does not decode."""
    ent, pays = lacmutate._payloads(lac)
    pays[1] = pays[1][:1] + bytes([0x7F]) + pays[1][2:] if lac[4] == 2 else bytes([0x7F]) + pays[1][1:]
    return lacmutate._rebuild(lac, ent, pays)


def damaged_case(oracle):
    """Three discs; the middle one's second stream of three is damaged."""
    by = {d.name: d for d in aw.corpus()}
    a, c = by["three|r1"], by["seams|partial"]
    b = aw.Disc("damaged", aw.split(aw.noise(3 * 17000, 4400), (17000,) * 3), None, 31, True, True)
    lacs = [encode(oracle, a), encode(oracle, b), encode(oracle, c)]
    lacs[1][1] = _broken(lacs[1][1])
    return [a, b, c], lacs


def test_a_damaged_stream_fails_its_disc_alone(oracle):
    discs, lacs = damaged_case(oracle)
    a, b, c = aw.run(aw.stream_case(discs, lacs))
    assert b.code == 2 and b.text.startswith("source 1: status ") and b.v1 is None and not b.result.tobytes().strip(b"\0")
    check(discs[0], a)
    check(discs[2], c)
    bad = [lacs[0], [lacs[1][0], b"XX" + lacs[1][1][2:], lacs[1][2]], lacs[2]]
    a, b, c = aw.run(aw.stream_case(discs, bad))
    assert b.code != 0 and b.text == "source 1: [decode-error] invalid frame header"
    check(discs[0], a)


def test_sanitized(streams, oracle):
    """The sanitized program passes every shape that later goes to the device -- the whole corpus as sources, the layouts, the
    invalid samples, the stream discs forward and reversed, the damaged disc -- with no report and the plain build's answers,
    which the tests above hold to numpy."""
    exe, why = aw.sanitized_exe()
    assert exe, why
    discs, lacs = streams
    small = aw.small_corpus()
    cases = [aw.source_case(small[at:at + 6]) for at in range(0, len(small), 6)] + [aw.source_case(small[::-1][:7])]
    cases += [aw.source_case([d]) for d in aw.corpus() if d.name.startswith("big|")]
    cases += [c for _, _, _, c in layout_cases()] + [c for c, _ in invalid_cases()]
    cases += [aw.stream_case(discs, lacs), aw.stream_case(discs[::-1], lacs[::-1]), aw.stream_case(*damaged_case(oracle))]
    lines, rc, err = aw.run_sanitized(cases, exe)
    assert rc == 0, err
    for i, c in enumerate(cases):
        assert lines[i] is not None and lines[i].split(" ", 1)[1] == aw.line(c, i).split(" ", 1)[1], i
    print("sanitized cases:", len(cases))
