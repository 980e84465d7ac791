"""Spectrum without a device: the CPU twin (tests/native/sim_spectrum.cpp -- csrc/decode_plan.h's spectrum job and
csrc/spectrum_plan.h's tables, csrc/spectrum_core.h run as k_spectrum runs it, every buffer at exactly the plan's capacity;
plain and under AddressSanitizer + UBSan as a program of its own) against expectations that never come from the code under
test (tests/spectwin.py): numpy.fft.rfft in float64 per (row, channel, band) within BAND_TOL of the row-channel's total, and
N sum (w x)^2 by math.fsum, which needs no FFT at all.

The whole corpus runs in the source form (planar int32: what the decoder's staging is once k_ms_inverse ran), all six
layouts at base offsets 0 and 4; the stream form -- the decode in front of the same kernel -- runs on the corpus' items of
up to 16385 frames, on spliced and version-2 streams and on a damaged one, and is held to the source form bit for bit."""
import os

import numpy as np
import pytest

import lacmutate
import lacstreams
import spectwin as st
import statstwin as sw

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
P32 = sw.LAYOUTS["planar_i32"]


def _fixture(name):
    with open(os.path.join(GOLDEN, name), "rb") as f:
        return f.read()


def _same(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def test_the_corpus_covers_what_it_claims():
    st.assert_content(st.corpus())
    by = {it.name: it for it in st.corpus()}
    # a window that straddles the row edge, and a last row of one window
    it = by["noise|N256|n16513|2ch16"]
    assert len(st.item_rows(it)) == 2 and -(-len(it.left) // 128) == 128 + 2
    assert len(st.item_rows(by["noise|N256|n16385|1ch16"])) == 2 and -(-16385 // 128) == 128 + 1
    # the restatement sees the constructed content where it was put
    t = st.item_totals(by["sine|k2-k64|N256|2ch16"])
    assert t.peak_band == (1, 32)
    assert st.item_totals(by["sine|k126-k2|N256|2ch24"]).peak_band == (63, 1) and st.item_totals(by["dc|N256|2ch16"]).peak_band == (0, 0)
    assert st.item_totals(by["nyquist|N256|2ch24"]).peak_band == (63, 63) and st.item_totals(by["cross|k10-k100|N256|2ch16"]).peak_band == (5, 50)
    assert st.item_totals(by["sine|k2-k2046|N4096|2ch24"]).peak_band == (0, 63)


def test_rows_are_the_restatements_within_band_tol():
    """Per (row, channel, band): |twin - numpy| / (that row-channel's total) <= BAND_TOL.  The cross-talk items are this
    check: in the left channel the band of the right channel's sine is the restatement's, zero up to noise.  Prints the
    measured figure BAND_TOL is 16 times of."""
    worst = (0.0, "")
    for it in st.corpus():
        rows = st.twin_rows(it)["power"]
        e = st.band_error(rows, st.item_rows(it))
        worst = max(worst, (e, it.name))
        assert e <= st.BAND_TOL, (it.name, e)
        if it.channels == 1:
            assert st.twin_rows(it)["power"][:, 1].tobytes() == bytes(8 * st.BANDS * len(rows)), it.name
    print("largest |twin - numpy| / total: %.3g on %s; BAND_TOL %.3g" % (worst[0], worst[1], st.BAND_TOL))
    by = {it.name: it for it in st.corpus()}
    for depth in (16, 24):
        it = by["cross|k10-k100|N256|2ch%d" % depth]
        rows, want = st.twin_rows(it)["power"], st.item_rows(it)
        for r in range(len(rows)):
            assert abs(rows[r, 0, 50] - want[r, 0, 50]) <= st.BAND_TOL * want[r, 0].sum()
            assert abs(rows[r, 1, 5] - want[r, 1, 5]) <= st.BAND_TOL * want[r, 1].sum()
        # row 0 holds whole windows only: nothing but the rounding of the samples lies in the other channel's band (the cut
        # at the item's end puts real power into every band of the last row, in the restatement too)
        assert rows[0, 0, 50] < 1e-9 * rows[0, 0, 5] and rows[0, 1, 5] < 1e-9 * rows[0, 1, 50]


def test_silence_is_plus_zero_in_every_byte():
    for it in st.corpus():
        if it.name.startswith("silence"):
            assert st.twin_rows(it).tobytes() == bytes(1024 * 2), it.name


def test_the_bands_add_up_to_the_windowed_energy():
    """Parseval, independent of any FFT: per row and channel the 64 bands sum to N sum (w x)^2 (math.fsum) within BAND_TOL."""
    worst = 0.0
    for it in st.corpus():
        total = st.twin_rows(it)["power"].sum(axis=2)
        want = st.parseval_rows(it.left, it.right, it.window)
        assert np.all(total[want == 0.0] == 0.0), it.name
        e = float(np.max(np.abs(total - want) / np.where(want == 0.0, 1.0, want)))
        worst = max(worst, e)
        assert e <= st.BAND_TOL, (it.name, e)
    print("largest |sum of bands - N sum (w x)^2| / the latter: %.3g" % worst)


def _layouts(depth):
    names = ["planar_i32", "planar_f32", "inter_f32", "inter_i16" if depth == 16 else "inter_i24"] + (["planar_i16"] if depth == 16 else [])
    return [(n, sw.LAYOUTS[n]) for n in names]


def layout_specs():
    """All six layouts at base offsets 0 and 4, in exact-size buffers, one item per format and a window length each:
    (name, spec, item)."""
    out = []
    for k, (ch, depth, rate) in enumerate(st.FORMATS):
        window = (256, 512, 2048, 4096)[k]
        frames = 2 * window + 131 + k
        it = st.Item("layout|N%d|%dch%d" % (window, ch, depth), window, ch, depth, rate, st._noise(frames, depth, 600 + k),
                     st._noise(frames, depth, 700 + k) if ch == 2 else None)
        for name, layout in _layouts(depth):
            for off in (0, 4):
                out.append(("%s+%d %s" % (name, off, it.name), st.spec_of(it, layout, off), it))
    return out


def test_every_layout_and_offset_gives_the_planar_rows():
    cases = layout_specs()
    assert {s.layout for _, s, _ in cases} == set(sw.LAYOUTS[n] for n in ("planar_i32", "planar_f32", "inter_f32", "inter_i16", "inter_i24", "planar_i16"))
    for name, spec, it in cases:
        (o,) = st.run_sources([spec])
        assert o.key == st.CLEAN and _same(o.rows, st.twin_rows(it)), name
        assert st.band_error(o.rows["power"], st.item_rows(it)) <= st.BAND_TOL, name


def test_rows_do_not_depend_on_the_batch():
    """An item's rows are the same bits alone and as the last item of a batch of seven."""
    picks = [it for it in st.corpus() if it.window == 256 and it.name.startswith("noise|N256|") and len(it.left) in (129, 257, 16385)]
    assert len(picks) == 12
    for it in picks:
        others = [x for x in picks if x is not it][:6]
        last = st.run_sources([st.spec_of(x) for x in others] + [st.spec_of(it)])[-1]
        assert _same(st.twin_rows(it), last.rows), it.name


INVALID = (("planar_i32", 24, 0x01000000, "is outside the configured PCM bit depth", 0), ("planar_i32", 16, 0xFFFF0000, "is outside the configured PCM bit depth", 0),
           ("planar_f32", 24, 0x3E99999A, "is not an exact 24-bit PCM value", 1), ("inter_f32", 16, 0x3E99999A, "is not an exact 16-bit PCM value", 1))


def invalid_specs():
    out = []
    for name, depth, word, what, kind in INVALID:
        for channels in (1, 2):
            it = st.Item("invalid", 256, channels, depth, 44100, st._noise(700, depth, 11), st._noise(700, depth, 12) if channels == 2 else None)
            for frame, ch in ((0, 0), (385, channels - 1), (699, 0)):
                text = "%s sample at index %d %s" % ("right" if ch else "left", frame, what)
                out.append((st.spec_of(it, sw.LAYOUTS[name], 4, (frame, ch, word)), (ch << 63) | (frame << 1) | kind, text))
    return out


def test_an_invalid_sample_fails_the_item_as_the_digest_form_words_it():
    cases = invalid_specs()
    good = st.corpus()[9]
    outs = st.run_sources([s for s, _, _ in cases] + [st.spec_of(good)])
    for (spec, key, text), o in zip(cases, outs):
        assert o.key == key and o.message == text and o.rows is None, text
    assert _same(outs[-1].rows, st.twin_rows(good))


# ---- the stream form ---------------------------------------------------------------------------------------------------
def small_corpus(window):
    return [it for it in st.corpus() if it.window == window and len(it.left) <= 16400]


def _broken(lac):
    """tests/golden/decode_wav/st16_lr_3blk.lac with the byte change test_gpu_stats.py makes: its second block does not decode."""
    ent, pays = lacmutate._payloads(lac)
    pays[1] = pays[1][:1] + bytes([0x7F]) + pays[1][2:] if lac[4] == 2 else bytes([0x7F]) + pays[1][1:]
    return lacmutate._rebuild(lac, ent, pays)


def spliced(oracle, window=256):
    """Per format the spliced stream of 257 / 258 / 259-frame blocks with its version-2 form: [(stream, Item)]."""
    out = []
    for ch, depth, rate in st.FORMATS:
        parts = sw.spliced_parts(ch, depth)
        lacs = [oracle.encode(l, r, rate, depth, 0) for l, r in parts]
        it = st.Item("splice|N%d|%dch%d" % (window, ch, depth), window, ch, depth, rate, np.concatenate([l for l, _ in parts]),
                     np.concatenate([r for _, r in parts]) if ch == 2 else None)
        lac = lacstreams.splice(lacstreams.splice(lacs[0], lacs[1]), lacs[2])
        out += [(lac, it), (lacstreams.to_v2(lac), it)]
    return out


@pytest.fixture(scope="module")
def streams(oracle):
    """{window: [(stream, Item)]}: the small corpus through the CPU encoder, and at N = 256 the spliced streams."""
    out = {w: [(oracle.encode(it.left, it.right, it.rate, it.depth, 2 if it.channels == 2 else 0), it) for it in small_corpus(w)] for w in st.WINDOWS}
    out[256] += spliced(oracle)
    return out


def test_stream_form_is_the_source_form_behind_a_decode(streams):
    """One job per window length of all its small streams, forward and reversed: the rows are the source form's bit for bit --
    the row grid counts in the item's frames, whatever the container's blocks are."""
    assert sum(len(v) for v in streams.values()) >= 60
    for window, some in streams.items():
        for order in (some, some[::-1]):
            got = st.run([lac for lac, _ in order], window)
            for (lac, it), g in zip(order, got):
                assert g.code == 0 and g.status == 0 and _same(g.rows, st.twin_rows(it)), it.name


def damaged_trio(oracle):
    it = {x.name: x for x in st.corpus()}["noise|N256|n257|2ch16"]
    clean = oracle.encode(it.left, it.right, it.rate, it.depth, 2)
    base = _fixture("decode_wav/st16_lr_3blk.lac")
    return [clean, _broken(base), base], it


def test_a_damaged_stream_between_two_clean_ones(oracle):
    lacs, it = damaged_trio(oracle)
    a, b, c = st.run(lacs, 256)
    assert b.code == 0 and 1 <= b.status <= 9 and b.rows is None
    (alone_c,) = st.run([lacs[2]], 256)
    assert a.status == 0 and _same(a.rows, st.twin_rows(it))
    assert c.status == 0 and _same(c.rows, alone_c.rows) and len(c.rows) == 3
    refused = st.run([lacs[0], b"XX" + lacs[0][2:], lacs[0][:12]], 256)
    assert [r.code != 0 for r in refused] == [False, True, True] and refused[1].message == "[decode-error] invalid frame header"
    assert _same(refused[0].rows, st.twin_rows(it))


def test_sanitized(streams, oracle):
    """The sanitized program passes every shape that later goes to the device -- the whole corpus as sources, every layout
    and offset, the invalid samples, the small streams per window length forward and reversed, the damaged trio -- with no
    report and the plain build's answers, which the tests above hold to numpy."""
    exe, why = st.sanitized_exe()
    assert exe, why
    specs = [st.spec_of(it) for it in st.corpus()] + [s for _, s, _ in layout_specs()] + [s for s, _, _ in invalid_specs()]
    cases = [st.source_case(s) for s in specs]
    for window, some in streams.items():
        lacs = [lac for lac, _ in some]
        cases += [st.case(lacs, window), st.case(lacs[::-1], window)]
    cases.append(st.case(damaged_trio(oracle)[0], 256))
    lines, rc, err = st.run_sanitized(cases, exe)
    assert rc == 0, err
    for i, c in enumerate(cases):
        assert lines[i] is not None and lines[i].split(" ", 1)[1] == st.line(c, i).split(" ", 1)[1], i
    print("sanitized cases:", len(cases))
