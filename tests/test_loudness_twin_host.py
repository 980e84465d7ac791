"""Loudness without a device: the CPU twin (tests/native/sim_loudness.cpp -- csrc/decode_plan.h's loudness job and
csrc/loudness_plan.h's tables, csrc/loudness_core.h run as the four kernels run it, csrc/loudness_rows.h's totals, every buffer
at exactly the plan's capacity; plain and under AddressSanitizer + UBSan as a program of its own) against expectations that
never come from the code under test: scipy.signal.lfilter over the whole channel, numpy sums, and the totals restated in
Python floats (tests/loudtwin.py).

The whole corpus runs in the source form (planar int32: what the decoder's staging is once k_ms_inverse ran); the stream
form -- the decode in front of the same passes -- runs on the corpus' items of up to 16385 frames or four sub-blocks, on
spliced and version-2 streams and on a damaged one, and is held to the source form bit for bit."""
import math
import os

import numpy as np
import pytest

import lacmutate
import lacstreams
import loudtwin as lt
import statstwin as sw

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
P32 = sw.LAYOUTS["planar_i32"]


def _fixture(name):
    with open(os.path.join(GOLDEN, name), "rb") as f:
        return f.read()


def _spec(it, layout=P32, offset=0, bad=None):
    return lt.SourceSpec(layout, it.channels, it.depth, it.rate, offset, it.left, it.right, bad)


def _same(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def corpus_out():
    """The whole corpus as ONE source job of the plain twin: [(Item, SourceOut)]."""
    items = lt.corpus()
    return list(zip(items, lt.run_sources([_spec(it) for it in items])))


def test_the_signals_exercise_both_gates():
    items = lt.corpus()
    lt.assert_content(items)
    assert len(items) == len(lt.FORMATS) * (16 + len(lt.KINDS)) and len({it.name for it in items}) == len(items)


def test_row_tolerance_is_the_measured_one(corpus_out):
    """Every row of the plain twin against scipy: d = |E - E_ref| / max(E_ref, 2^-40 * the item's largest row) stays within
    ROW_TOL = 16 * the value measured here (printed); a measured value above 1e-9 would be a finding, not a tolerance."""
    worst, where = 0.0, ""
    for it, out in corpus_out:
        assert out.key == lt.CLEAN and out.rows.shape == lt.item_rows(it).shape, it.name
        d = lt.row_error(out.rows, lt.item_rows(it))
        if d > worst:
            worst, where = d, it.name
    print("largest row difference over the corpus: %.3e at %s (ROW_MEASURED %.3e, ROW_TOL %.3e)" % (worst, where, lt.ROW_MEASURED, lt.ROW_TOL))
    assert lt.ROW_TOL == 16 * lt.ROW_MEASURED and lt.TOTALS_TOL == 4.35 * lt.ROW_TOL * 4
    assert worst < 1e-9
    assert worst <= lt.ROW_TOL


def test_totals_end_to_end_and_over_the_same_rows(corpus_out):
    """The product's totals over the twin's rows: against the restatement over the same rows counts and flags exact and every
    level within 1e-9 LU; end to end against scipy within 4.35 * ROW_TOL * 4 LU."""
    for it, out in corpus_out:
        lt.close_totals(out.totals, lt.expected_totals([(out.rows, it.channels, it.depth, it.rate)]), lt.COMBINE_TOL)
        lt.close_totals(out.totals, lt.item_totals(it), lt.TOTALS_TOL)
        if it.channels == 1:
            assert not out.rows[:, 1].any(), it.name


def test_the_standards_cases():
    """EBU Tech 3341's cases as stereo 1 kHz sines at 48 kHz / 16 bit, rounded to integers, full length, through the twin:
    each within the standard's 0.1 LU; the restatement's own values are the ones worked out for these quantised signals; a mono
    -23 dBFS tone reads -26.0."""
    cases = lt.ebu_cases()
    items = [lt.ebu_item(name, parts) for name, parts, _ in cases] + [lt.ebu_item("23", [(20, -23.0)], channels=1)]
    outs = lt.run_sources([_spec(it) for it in items])
    want = [w for _, _, w in cases] + [-26.0]
    got = [o.totals.integrated for o in outs]
    print("integrated:", ["%.4f" % g for g in got])
    for it, g, w in zip(items, got, want):
        assert abs(g - w) <= 0.1, (it.name, g, w)
    for g, restated in zip(got, (-22.993, -32.991, -23.014, -23.014, -22.979, -26.004)):
        assert abs(g - restated) < 2e-3, (g, restated)
    it = lt.ebu_item("36-23-36@44", [(10, -36.0), (60, -23.0), (10, -36.0)], rate=44100, depth=24)
    (o,) = lt.run_sources([_spec(it)])
    assert abs(o.totals.integrated + 23.011) < 2e-3
    lt.close_totals(o.totals, lt.item_totals(it), lt.TOTALS_TOL)


def test_silence_and_short_items():
    for ch, depth, rate in lt.FORMATS:
        n = rate // 10
        zero = lt.Item("zero", ch, depth, rate, np.zeros(5 * n + 3, np.int32), np.zeros(5 * n + 3, np.int32) if ch == 2 else None)
        short = lt.make_item("noise", 4 * n - 1, ch, depth, rate, 77)
        z, s = lt.run_sources([_spec(zero), _spec(short)])
        assert z.rows.shape == (5, 2) and not z.rows.any() and z.totals.flags == lt.SILENT and z.totals.integrated == -math.inf
        assert s.rows.shape == (3, 2) and s.totals.flags == lt.TOO_SHORT and s.totals.gating_blocks == 0 and s.totals.range == 0.0


def _layouts(depth):
    names = ["planar_f32", "inter_f32", "inter_i16" if depth == 16 else "inter_i24"] + (["planar_i16"] if depth == 16 else [])
    return [(n, sw.LAYOUTS[n]) for n in names]


def _offsets(name):
    step = 1 if name == "inter_i24" else 2 if name == "planar_i16" else 4
    return range(0, 16, step)


def layout_specs():
    """Every layout of every format at every base offset its alignment permits, in exact-size buffers: (name, spec, planar spec)."""
    out = []
    for k, (ch, depth, rate) in enumerate(lt.FORMATS):
        n = rate // 10
        it = lt.make_item("noise", n + 257 + k, ch, depth, rate, 300 + k)
        for name, layout in _layouts(depth) + [("planar_i32", P32)]:
            for off in _offsets(name):
                out.append(("%s+%d %s" % (name, off, it.name), _spec(it, layout, off), it))
    return out


def test_every_layout_and_offset_gives_the_planar_rows():
    cases = layout_specs()
    outs = lt.run_sources([s for _, s, _ in cases])
    want = {}
    for (name, _, it), o in zip(cases, outs):
        if it.name not in want:
            (want[it.name],) = lt.run_sources([_spec(it)])
        assert o.key == lt.CLEAN and _same(o.rows, want[it.name].rows) and o.totals == want[it.name].totals, name


def test_rows_do_not_depend_on_the_batch_or_the_base(corpus_out):
    """An item's rows are the same bits alone, as the last item of a batch of seven, and in source form at base offsets of
    0..3 samples."""
    by_name = {it.name: (it, out) for it, out in corpus_out}
    picks = [it for it, _ in corpus_out if it.left.size in (it.rate // 10 + 1, 4 * (it.rate // 10) + 1, 16385)]
    assert len(picks) == 12
    for it in picks:
        (alone,) = lt.run_sources([_spec(it)])
        others = [x for x in picks if x is not it][:6]
        last = lt.run_sources([_spec(x) for x in others] + [_spec(it)])[-1]
        assert _same(alone.rows, by_name[it.name][1].rows) and _same(alone.rows, last.rows) and alone.totals == last.totals, it.name
        for off in (4, 8, 12):
            (moved,) = lt.run_sources([_spec(it, offset=off)])
            assert _same(alone.rows, moved.rows), (it.name, off)


INVALID = (("planar_i32", 24, 0x01000000, "is outside the configured PCM bit depth", 0), ("planar_i32", 16, 0xFFFF0000, "is outside the configured PCM bit depth", 0),
           ("planar_f32", 24, 0x3E99999A, "is not an exact 24-bit PCM value", 1), ("inter_f32", 16, 0x3E99999A, "is not an exact 16-bit PCM value", 1))


def invalid_specs():
    out = []
    for name, depth, word, what, kind in INVALID:
        for channels in (1, 2):
            rate = 48000
            it = lt.make_item("noise", 4800 + 300, channels, depth, rate, 11)
            for frame, ch in ((0, 0), (2001, channels - 1), (4800 + 299, 0)):  # the last: behind the last complete sub-block
                text = "%s sample at index %d %s" % ("right" if ch else "left", frame, what)
                out.append((_spec(it, sw.LAYOUTS[name], 4, (frame, ch, word)), (ch << 63) | (frame << 1) | kind, text))
    return out


def test_an_invalid_sample_fails_the_item_as_the_digest_form_words_it():
    """A planar int32 outside the depth, a float off the grid -- also in the frames that are not filtered: the digest form's
    key and text, a zeroed result and no rows; a good item in the same job is not touched."""
    cases = invalid_specs()
    good = lt.make_item("tone", 9600 + 5, 2, 16, 48000, 5)
    outs = lt.run_sources([s for s, _, _ in cases] + [_spec(good)])
    for (spec, key, text), o in zip(cases, outs):
        assert o.key == key and o.message == text and o.rows is None and o.totals == lt.totals_of(np.zeros(1, lt.TOT_T)[0]), text
    (alone,) = lt.run_sources([_spec(good)])
    assert _same(outs[-1].rows, alone.rows)


# ---- the stream form ---------------------------------------------------------------------------------------------------
def small_corpus():
    return [it for it in lt.corpus() if it.left.size <= max(16385, 4 * (it.rate // 10) + 1)]


def _broken(lac):
    """tests/golden/decode_wav/st16_lr_3blk.lac with the byte change test_gpu_stats.py makes: its second block does not decode."""
    ent, pays = lacmutate._payloads(lac)
    pays[1] = pays[1][:1] + bytes([0x7F]) + pays[1][2:] if lac[4] == 2 else bytes([0x7F]) + pays[1][1:]
    return lacmutate._rebuild(lac, ent, pays)


@pytest.fixture(scope="module")
def streams(oracle):
    """[(stream, Item)]: the small corpus through the CPU encoder, and per format the spliced stream of 257 / 258 / 259-frame
    blocks with its version-2 form."""
    out = [(oracle.encode(it.left, it.right, it.rate, it.depth, 2 if it.channels == 2 else 0), it) for it in small_corpus()]
    for ch, depth, rate in lt.FORMATS:
        parts = sw.spliced_parts(ch, depth)
        lacs = [oracle.encode(l, r, rate, depth, 0) for l, r in parts]
        it = lt.Item("splice|%dch%d" % (ch, depth), ch, depth, rate, np.concatenate([l for l, _ in parts]),
                     np.concatenate([r for _, r in parts]) if ch == 2 else None)
        lac = lacstreams.splice(lacstreams.splice(lacs[0], lacs[1]), lacs[2])
        out += [(lac, it), (lacstreams.to_v2(lac), it)]
    return out


def test_stream_form_is_the_source_form_behind_a_decode(streams, corpus_out):
    """One job of all small streams, forward and reversed: the rows are those of the planar source form bit for bit (chunks
    count in the item's frames, whatever the container's blocks are), the totals the same records."""
    assert len(small_corpus()) == 13 * len(lt.FORMATS)
    source = {it.name: out for it, out in corpus_out}
    for order in (streams, streams[::-1]):
        got = lt.run([lac for lac, _ in order])
        for (lac, it), g in zip(order, got):
            if it.name not in source:
                (source[it.name],) = lt.run_sources([_spec(it)])
            assert g.code == 0 and g.status == 0 and _same(g.rows, source[it.name].rows) and g.totals == source[it.name].totals, it.name


def damaged_trio(oracle):
    it = lt.make_item("tone", 2 * 4800 + 11, 2, 16, 48000, 31)
    clean = oracle.encode(it.left, it.right, it.rate, it.depth, 2)
    base = _fixture("decode_wav/st16_lr_3blk.lac")
    return [clean, _broken(base), base], it


def test_a_damaged_stream_between_two_clean_ones(oracle):
    lacs, it = damaged_trio(oracle)
    a, b, c = lt.run(lacs)
    assert b.code == 0 and 1 <= b.status <= 9 and b.rows is None and b.totals == lt.totals_of(np.zeros(1, lt.TOT_T)[0])
    (alone_a,), (alone_c,) = lt.run([lacs[0]]), lt.run([lacs[2]])
    assert a.status == 0 and _same(a.rows, alone_a.rows) and a.totals == alone_a.totals and lt.row_error(a.rows, lt.item_rows(it)) <= lt.ROW_TOL
    assert c.status == 0 and _same(c.rows, alone_c.rows) and c.totals == alone_c.totals
    refused = lt.run([lacs[0], b"XX" + lacs[0][2:], lacs[0][:12]])
    assert [r.code != 0 for r in refused] == [False, True, True] and refused[1].message == "[decode-error] invalid frame header"
    assert _same(refused[0].rows, alone_a.rows)


def test_sanitized(streams, oracle):
    """The sanitized program passes every shape that later goes to the device -- the whole corpus and the standard's cases as
    sources, every layout and offset, the invalid samples, the small streams in one job and in batches, the damaged trio --
    with no report and the plain build's answers, which the tests above hold to scipy."""
    exe, why = lt.sanitized_exe()
    assert exe, why
    specs = [_spec(it) for it in lt.corpus()] + [s for _, s, _ in layout_specs()] + [s for s, _, _ in invalid_specs()]
    specs += [_spec(lt.ebu_item(name, parts)) for name, parts, _ in lt.ebu_cases()[2::2]]
    lacs = [lac for lac, _ in streams]
    cases = [lt.source_case(s) for s in specs] + [lt.case(lacs), lt.case(lacs[::-1])] + [lt.case(lacs[at:at + 7]) for at in range(0, len(lacs), 7)]
    cases.append(lt.case(damaged_trio(oracle)[0]))
    lines, rc, err = lt.run_sanitized(cases, exe)
    assert rc == 0, err
    for i, c in enumerate(cases):
        assert lines[i] is not None and lines[i].split(" ", 1)[1] == lt.line(c, i).split(" ", 1)[1], i
    print("sanitized cases:", len(cases))
