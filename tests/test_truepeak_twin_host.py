"""True peak without a device: the CPU twin (tests/native/sim_truepeak.cpp -- csrc/decode_plan.h's true-peak job and
csrc/truepeak_plan.h's tables, csrc/truepeak_core.h run as k_truepeak runs it, csrc/truepeak_rows.h's rows and totals, every
buffer at exactly the plan's capacity; plain and under AddressSanitizer + UBSan as a program of its own) against an
expectation that never comes from the code under test: np.convolve of the int64 channel with each phase (tests/peaktwin.py).
Everything is exact: rows are compared byte for byte, no tolerance.

The whole corpus runs in the source form (planar int32: what the decoder's staging is once k_ms_inverse ran), every layout at
every base offset; the stream form -- the decode in front of the same kernel -- runs on the corpus' items of up to 16385
frames, on spliced and version-2 streams and on a damaged one, and is held to the source form bit for bit."""
import os

import numpy as np
import pytest

import lacmutate
import lacstreams
import peaktwin as pt
import statstwin as sw

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
P32 = sw.LAYOUTS["planar_i32"]


def _fixture(name):
    with open(os.path.join(GOLDEN, name), "rb") as f:
        return f.read()


def _spec(it, layout=P32, offset=0, bad=None):
    return pt.SourceSpec(layout, it.channels, it.depth, it.rate, offset, it.left, it.right, bad)


def _same(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def corpus_out():
    """The whole corpus as ONE source job of the plain twin: [(Item, SourceOut)]."""
    items = pt.corpus()
    return list(zip(items, pt.run_sources([_spec(it) for it in items])))


def test_the_corpus_covers_what_it_claims():
    """On the expectation alone: the frame counts, maxima on either side of tile and row borders and in the flush tail, a
    depth-24 peak no 32-bit sum holds, equal peaks, channels that differ."""
    items = pt.corpus()
    by = {it.name: it for it in items}
    assert len(items) == len(pt.FORMATS) * len(pt.FRAME_COUNTS) + 2 * (16 + 6 + 2 + 1 + 2 + 1 + 1)
    assert {1013 + pt.FLUSH, 1014 + pt.FLUSH} == {pt.TILE, pt.TILE + 1}
    peaks = set()
    for d in (-12, -11, -6, -5, -1, 0, 1, 11):
        for border in (pt.TILE, pt.ROW):
            t = pt.item_totals(by["impulse|b%d%+d|2ch24" % (border, d)])
            assert t.ch[0].position == 4 * (border + d + 5) + 3 and t.ch[0].peak == 7964
            peaks.add((t.ch[0].position // 4 - border) >= 0)
    assert peaks == {False, True}
    for frames in (1, 12, pt.TILE, pt.ROW, pt.ROW + 1):
        t = pt.item_totals(by["impulse|ends%d|2ch16" % frames])
        assert t.ch[1].position // 4 == frames - 1 + 5 >= frames, "the right channel's peak lies in the flush tail"
        assert len(pt.item_rows(by["impulse|ends%d|2ch16" % frames])) == (frames + pt.ROW - 1) // pt.ROW
    for depth in (16, 24):
        for sign in ("pos", "neg"):
            t = pt.item_totals(by["worst|%s|2ch%d" % (sign, depth)])
            full = 1 << (depth - 1)
            assert 16571 * (full - 1) <= t.ch[0].peak <= 16571 * full and t.flags == pt.OVER | pt.SAMPLE_FULL
            assert (t.ch[0].peak >= 1 << 31) == (depth == 24)
        dc = pt.item_totals(by["dc|full-negative|2ch%d" % depth])
        assert dc.ch[0].peak >= 8205 * (1 << (depth - 1)) and dc.ch[0].position < 4 * 12 and dc.ch[0].peak != dc.ch[1].peak
    assert pt.item_totals(by["silent-right|2ch24"]).ch[1] == pt.Channel(0, 0, 0, 0)
    assert pt.item_totals(by["impulse|mono-last|1ch16"]).ch[0].position == 4 * (pt.TILE + 1 + 5) + 3


def test_rows_are_the_restatements_bit_for_bit(corpus_out):
    """Every row of the plain twin is the numpy restatement's, byte for byte; the totals likewise (the two logarithms to
    1e-12 dB: libm's against Python's)."""
    for it, out in corpus_out:
        assert out.key == pt.CLEAN and _same(out.rows, pt.item_rows(it)), it.name
        pt.same_totals(out.totals, pt.item_totals(it))
        pt.same_totals(pt.twin_combine([(out.rows, it.channels, it.depth, len(it.left), it.rate)]), pt.item_totals(it))
        if it.channels == 1:
            assert not out.rows["peak"][:, 1].any() and not out.rows["sample_peak"][:, 1].any(), it.name


def _layouts(depth):
    names = ["planar_f32", "inter_f32", "inter_i16" if depth == 16 else "inter_i24"] + (["planar_i16"] if depth == 16 else [])
    return [(n, sw.LAYOUTS[n]) for n in names]


def _offsets(name):
    step = 1 if name == "inter_i24" else 2 if name == "planar_i16" else 4
    return range(0, 16, step)


def layout_specs():
    """Every layout of every format at every base offset its alignment permits, in exact-size buffers: (name, spec, item)."""
    out = []
    for k, (ch, depth, rate) in enumerate(pt.FORMATS):
        it = pt.Item("layout|%dch%d" % (ch, depth), ch, depth, rate, pt._noise(pt.TILE + 257 + k, depth, 600 + k),
                     pt._noise(pt.TILE + 257 + k, depth, 700 + k) if ch == 2 else None)
        for name, layout in _layouts(depth) + [("planar_i32", P32)]:
            for off in _offsets(name):
                out.append(("%s+%d %s" % (name, off, it.name), _spec(it, layout, off), it))
    return out


def test_every_layout_and_offset_gives_the_planar_rows():
    cases = layout_specs()
    outs = pt.run_sources([s for _, s, _ in cases])
    for (name, _, it), o in zip(cases, outs):
        assert o.key == pt.CLEAN and _same(o.rows, pt.item_rows(it)), name
        pt.same_totals(o.totals, pt.item_totals(it))


def test_rows_do_not_depend_on_the_batch(corpus_out):
    """An item's rows are the same bits alone and as the last item of a batch of seven."""
    picks = [it for it, _ in corpus_out if it.name.startswith("noise|") and len(it.left) in (13, 1014, 16385)]
    assert len(picks) == 12
    by_name = {it.name: out for it, out in corpus_out}
    for it in picks:
        (alone,) = pt.run_sources([_spec(it)])
        others = [x for x in picks if x is not it][:6]
        last = pt.run_sources([_spec(x) for x in others] + [_spec(it)])[-1]
        assert _same(alone.rows, by_name[it.name].rows) and _same(alone.rows, last.rows) and alone.totals == last.totals, it.name


def test_a_silent_item_between_two_full_scale_ones():
    """History in front of frame 0 and samples behind the last frame are zeros, never the neighbouring item's PCM."""
    loud = pt.Item("loud", 2, 24, 48000, np.full(1500, -(1 << 23), np.int32), np.full(1500, (1 << 23) - 1, np.int32))
    quiet = pt.Item("quiet", 2, 24, 48000, np.zeros(1030, np.int32), np.zeros(1030, np.int32))
    a, b, c = pt.run_sources([_spec(loud), _spec(quiet), _spec(loud)])
    assert b.rows.tobytes() == bytes(32) and b.totals.true_peak == 0.0 and b.totals.flags == 0
    assert _same(a.rows, c.rows) and _same(a.rows, pt.expected_rows(loud.left, loud.right))


INVALID = (("planar_i32", 24, 0x01000000, "is outside the configured PCM bit depth", 0), ("planar_i32", 16, 0xFFFF0000, "is outside the configured PCM bit depth", 0),
           ("planar_f32", 24, 0x3E99999A, "is not an exact 24-bit PCM value", 1), ("inter_f32", 16, 0x3E99999A, "is not an exact 16-bit PCM value", 1))


def invalid_specs():
    out = []
    for name, depth, word, what, kind in INVALID:
        for channels in (1, 2):
            it = pt.Item("invalid", channels, depth, 48000, pt._noise(pt.TILE + 300, depth, 11), pt._noise(pt.TILE + 300, depth, 12) if channels == 2 else None)
            for frame, ch in ((0, 0), (1021, channels - 1), (pt.TILE + 299, 0)):  # the second: also loaded as a tile's history
                text = "%s sample at index %d %s" % ("right" if ch else "left", frame, what)
                out.append((_spec(it, sw.LAYOUTS[name], 4, (frame, ch, word)), (ch << 63) | (frame << 1) | kind, text))
    return out


def test_an_invalid_sample_fails_the_item_as_the_digest_form_words_it():
    """A planar int32 outside the depth, a float off the grid: the digest form's key and text, a zeroed result and no rows;
    a good item in the same job is not touched."""
    cases = invalid_specs()
    good = pt.corpus()[9]
    outs = pt.run_sources([s for s, _, _ in cases] + [_spec(good)])
    for (spec, key, text), o in zip(cases, outs):
        assert o.key == key and o.message == text and o.rows is None and o.totals == pt.ZERO_TOTALS, text
    assert _same(outs[-1].rows, pt.item_rows(good))


# ---- the stream form ---------------------------------------------------------------------------------------------------
def small_corpus():
    return [it for it in pt.corpus() if len(it.left) <= 16400]


def _broken(lac):
    """tests/golden/decode_wav/st16_lr_3blk.lac with the byte change test_gpu_stats.py makes: its second block does not decode."""
    ent, pays = lacmutate._payloads(lac)
    pays[1] = pays[1][:1] + bytes([0x7F]) + pays[1][2:] if lac[4] == 2 else bytes([0x7F]) + pays[1][1:]
    return lacmutate._rebuild(lac, ent, pays)


def spliced(oracle):
    """Per format the spliced stream of 257 / 258 / 259-frame blocks with its version-2 form: [(stream, Item)]."""
    out = []
    for ch, depth, rate in pt.FORMATS:
        parts = sw.spliced_parts(ch, depth)
        lacs = [oracle.encode(l, r, rate, depth, 0) for l, r in parts]
        it = pt.Item("splice|%dch%d" % (ch, depth), ch, depth, rate, np.concatenate([l for l, _ in parts]),
                     np.concatenate([r for _, r in parts]) if ch == 2 else None)
        lac = lacstreams.splice(lacstreams.splice(lacs[0], lacs[1]), lacs[2])
        out += [(lac, it), (lacstreams.to_v2(lac), it)]
    return out


@pytest.fixture(scope="module")
def streams(oracle):
    """[(stream, Item)]: the small corpus through the CPU encoder, and the spliced streams."""
    return [(oracle.encode(it.left, it.right, it.rate, it.depth, 2 if it.channels == 2 else 0), it) for it in small_corpus()] + spliced(oracle)


def test_stream_form_is_the_source_form_behind_a_decode(streams):
    """One job of all small streams, forward and reversed: the rows are the restatement's bit for bit -- the row grid counts
    in the item's frames, whatever the container's blocks are (a spliced stream of 257 / 258 / 259-frame blocks and its
    version-2 form give the rows of the same PCM in one block)."""
    assert len(small_corpus()) == len(pt.corpus()) - len(pt.FORMATS) - 2
    for order in (streams, streams[::-1]):
        got = pt.run([lac for lac, _ in order])
        for (lac, it), g in zip(order, got):
            assert g.code == 0 and g.status == 0 and _same(g.rows, pt.item_rows(it)), it.name
            pt.same_totals(g.totals, pt.item_totals(it))


def damaged_trio(oracle):
    it = pt.corpus()[12]
    clean = oracle.encode(it.left, it.right, it.rate, it.depth, 2 if it.channels == 2 else 0)
    base = _fixture("decode_wav/st16_lr_3blk.lac")
    return [clean, _broken(base), base], it


def test_a_damaged_stream_between_two_clean_ones(oracle):
    lacs, it = damaged_trio(oracle)
    a, b, c = pt.run(lacs)
    assert b.code == 0 and 1 <= b.status <= 9 and b.rows is None and b.totals == pt.ZERO_TOTALS
    (alone_c,) = pt.run([lacs[2]])
    assert a.status == 0 and _same(a.rows, pt.item_rows(it))
    assert c.status == 0 and _same(c.rows, alone_c.rows) and c.totals == alone_c.totals and len(c.rows) == 3
    refused = pt.run([lacs[0], b"XX" + lacs[0][2:], lacs[0][:12]])
    assert [r.code != 0 for r in refused] == [False, True, True] and refused[1].message == "[decode-error] invalid frame header"
    assert _same(refused[0].rows, pt.item_rows(it))


def test_sanitized(streams, oracle):
    """The sanitized program passes every shape that later goes to the device -- the whole corpus and the standard's sine
    cases as sources, every layout and offset, the invalid samples, the small streams in one job and in batches, the damaged
    trio -- with no report and the plain build's answers, which the tests above hold to numpy."""
    exe, why = pt.sanitized_exe()
    assert exe, why
    specs = [_spec(it) for it in pt.corpus()] + [s for _, s, _ in layout_specs()] + [s for s, _, _ in invalid_specs()]
    specs += [_spec(pt.ebu_item(name, div, phase, amp, depth)) for name, div, phase, amp in pt.ebu_cases() for depth in (16, 24)]
    lacs = [lac for lac, _ in streams]
    cases = [pt.source_case(s) for s in specs] + [pt.case(lacs), pt.case(lacs[::-1])] + [pt.case(lacs[at:at + 7]) for at in range(0, len(lacs), 7)]
    cases.append(pt.case(damaged_trio(oracle)[0]))
    lines, rc, err = pt.run_sanitized(cases, exe)
    assert rc == 0, err
    for i, c in enumerate(cases):
        assert lines[i] is not None and lines[i].split(" ", 1)[1] == pt.line(c, i).split(" ", 1)[1], i
    print("sanitized cases:", len(cases))
