"""The true-peak entry points without a device: the new structs against the library's own sizeof, the Annex 2 table's sums
and symmetry, the sine cases of EBU Tech 3341 on the numpy restatement and on the CPU twin (so that a wrong digit in the table
cannot pass), lacx_truepeak_combine against the totals restated in Python (tests/peaktwin.py), album combination, ties, the
checks of the call's arguments, and what a call does for its items before any device work."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import __graft_entry__ as ge
import peaktwin as pt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NEW = ("lacx_decoder_truepeak_batch_device", "lacx_decoder_truepeak_pcm_batch_device", "lacx_decoder_item_truepeak_rows", "lacx_truepeak_combine")
FAKE = 1 << 40  # a "device address" that is never dereferenced: every call here stops before the device
P32 = 0


@pytest.fixture(scope="module")
def pkg():
    mod = ge.load_pkg()
    if not os.path.exists(mod.lacx.LIB_PATH):
        mod.lacx.build()
    return mod


@pytest.fixture
def dec(pkg):
    h = C.c_void_p()
    assert pkg.lacx.lib().lacx_decoder_create(C.c_int(-1), C.byref(h)) == pkg.lacx.OK
    yield h
    pkg.lacx.lib().lacx_decoder_destroy(h)


def _fixture(name):
    with open(os.path.join(GOLDEN, name), "rb") as f:
        return f.read()


def _last_error(pkg):
    return pkg.lacx.lib().lacx_decode_last_error().decode()


def _spec(it, layout=P32, offset=0, bad=None):
    return pt.SourceSpec(layout, it.channels, it.depth, it.rate, offset, it.left, it.right, bad)


def test_symbols_and_structs(pkg):
    L, lx = pkg.lacx.lib(), pkg.lacx
    header = open(os.path.join(ROOT, "include", "lacx.h")).read()
    for name in NEW:
        assert hasattr(L, name) and name in lx.EXPORTS
        assert re.search(rf"\b{name}\s*\(", header), name
        assert header.index(name) < header.index("#ifndef LACX_H"), name  # listed in the comment block at the top
    structs = lx.abi_structs()
    for name, cls, size in (("truepeak_row", lx.TruePeakRow, 32), ("truepeak_channel", lx.TruePeakChannel, 24), ("truepeak", lx.TruePeak, 96)):
        assert structs[name] is cls and L.lacx_sizeof(name.encode()) == C.sizeof(cls) == size == {32: pt.ROW_T, 24: pt.CH_T, 96: pt.TOT_T}[size].itemsize, name
    assert (lx.TRUEPEAK_OVER, lx.TRUEPEAK_SAMPLE_FULL, lx.TRUEPEAK_ROW_FRAMES) == (pt.OVER, pt.SAMPLE_FULL, pt.ROW)
    assert "true peak: the next section" in header and "Out of scope: true peak" not in header


def test_the_tables_sums_and_symmetry():
    """The sums 8205 / 7971 / 7971 / 8205, the sums of magnitudes 11749 / 16571 / 16571 / 11749, phases 2 and 3 the reverse
    of 1 and 0 -- on the restatement's table and on the one compiled into the twin (csrc/truepeak_core.h), which are equal."""
    for t in (pt.TABLE, pt.twin_table().astype(np.int64)):
        assert t.shape == (4, 12)
        assert t.sum(axis=1).tolist() == [8205, 7971, 7971, 8205]
        assert np.abs(t).sum(axis=1).tolist() == [11749, 16571, 16571, 11749]
        assert (t[2] == t[1][::-1]).all() and (t[3] == t[0][::-1]).all()
    assert (pt.TABLE == pt.twin_table()).all()
    core = open(os.path.join(ROOT, "lossless-audio-codec_amd", "csrc", "truepeak_core.h")).read()
    assert "static_assert(phase_sum(0, false) == 8205" in core and "phase_sum(1, true) == kTpPeakGain" in core and "kTpPeakGain = 16571" in core


# what the restatement reads for each case, in dB from 20 log10 A (worked out with numpy on these signals)
EBU_READS = (-0.197, +0.045, -0.295, -0.007, +0.044)


@pytest.mark.parametrize("depth", [24, 16])
def test_the_sine_cases_of_ebu_tech_3341(depth):
    """Cases 15 - 19: one second at 48 kHz, amplitude A with a 0.1 s linear fade in and out (an abrupt start reads up to 0.7
    dB high with the standard's own filter): fs/4 at 0 and 45 degrees, fs/6 at 60, fs/8 at 67.5 at A = 0.5, and fs/4 at 45
    degrees at A = 1.4125.  Restatement and twin must lie within +0.2 / -0.4 dB of 20 log10 A, that document's tolerance;
    the over flag on the +3 dB case and on no other; the largest sample of fs/4 at 45 degrees reads 3 dB low."""
    items = [pt.ebu_item(name, div, phase, amp, depth) for name, div, phase, amp in pt.ebu_cases()]
    twins = pt.run_sources([_spec(it) for it in items])
    for (name, div, phase, amp), it, twin, reads in zip(pt.ebu_cases(), items, twins, EBU_READS):
        want = pt.item_totals(it)
        nominal = 20.0 * math.log10(amp)
        for who, t in (("restatement", want), ("twin", twin.totals)):
            d = t.dbtp - nominal
            print("case %s depth %d %s: %+.4f dB from nominal" % (name, depth, who, d))
            assert -0.4 <= d <= 0.2, (name, who, d)
            assert bool(t.flags & pt.OVER) == (name == "19"), (name, who)
        assert abs((want.dbtp - nominal) - reads) < 2e-3, (name, want.dbtp - nominal)
        assert twin.rows.tobytes() == pt.item_rows(it).tobytes() and twin.totals[:10] == want[:10], name
    assert abs(pt.item_totals(items[1]).sample_dbfs - (20.0 * math.log10(0.5) - 3.01)) < 0.01


def _rows_of(it):
    return pt.item_rows(it)


def test_combine_of_one_set_is_the_restatement(pkg):
    """lacx_truepeak_combine over the restatement's rows of every corpus item: the restated totals, integers exact."""
    lx = pkg.lacx
    for it in pt.corpus():
        rows = _rows_of(it)
        got = lx.truepeak_combine([(rows.tobytes(), it.channels, it.depth, len(it.left), it.rate)])
        pt.same_totals(pt.totals_of(got), pt.item_totals(it))
        assert got.set == 0 and got.rows == len(rows) and got.position == pt.item_totals(it).ch[got.peak_channel].position
        if it.channels == 1:
            assert got.ch[1].peak == 0 and got.ch[1].sample_peak == 0


def test_silence(pkg):
    lx = pkg.lacx
    rows = pt.expected_rows(np.zeros(20000, np.int32), np.zeros(20000, np.int32))
    assert rows.tobytes() == bytes(64)
    got = lx.truepeak_combine([(rows.tobytes(), 2, 16, 20000, 48000)])
    assert got.true_peak == 0.0 and got.true_peak_dbtp == -math.inf and got.sample_peak_dbfs == -math.inf and got.flags == 0 and got.rows == 2
    pt.same_totals(pt.totals_of(got), pt.expected_totals([(rows, 2, 16, 20000, 48000)]))


def test_ties_take_the_lowest_position(pkg):
    """Two equal peaks: the first row wins in the totals, the lower position inside a row; an impulse's own two equal
    outputs (TABLE[3][5] = TABLE[0][6]) give the earlier one."""
    lx = pkg.lacx
    by = {it.name: it for it in pt.corpus()}
    it = by["ties|two-rows|2ch24"]
    t = pt.totals_of(lx.truepeak_combine([(_rows_of(it).tobytes(), 2, 24, len(it.left), it.rate)]))
    assert _rows_of(it)["peak"][0, 0] == _rows_of(it)["peak"][1, 0] and t.ch[0].position == 4 * (200 + 5) + 3 and t.ch[0].sample_peak_row == 0
    assert t.ch[1].position == 4 * (pt.ROW - 3 + 5) + 3 and t.ch[1].position // (4 * pt.ROW) == 1, "the flush of a row's last frames lies in the next row"
    it = by["ties|one-row|2ch16"]
    assert _rows_of(it)["pos"][0].tolist() == [4 * 105 + 3, 4 * 105 + 3]
    one = pt.expected_rows(np.array([0, 0, 1, 0], np.int32), None)
    assert one["peak"][0, 0] == 7964 and one["pos"][0, 0] == 4 * (2 + 5) + 3


def test_album_combination(pkg):
    """Several sets: the largest peak wins, a 16-bit peak shifted by 8 against a 24-bit one, the lowest index on ties; frames
    and rows add up, the flags are those of all sets."""
    lx = pkg.lacx
    by = {it.name: it for it in pt.corpus()}
    a, b, c = by["noise|n16385|2ch16"], by["worst|pos|2ch24"], by["noise|n1025|1ch24"]
    sets = [(_rows_of(x), x.channels, x.depth, len(x.left), x.rate) for x in (a, b, c)]
    got = lx.truepeak_combine([(s[0].tobytes(),) + s[1:] for s in sets])
    want = pt.expected_totals(sets)
    pt.same_totals(pt.totals_of(got), want)
    pt.same_totals(pt.twin_combine(sets), want)
    assert got.set == 1 and got.bit_depth == 24 and got.frames == 16385 + 2000 + 1025 and got.rows == 2 + 1 + 1 and got.over
    # exactly equal peaks at different depths: 1000 at 16 bit is 256000 at 24 bit
    x16 = pt.expected_rows(np.array([0] * 20 + [1000] + [0] * 20, np.int32), None)
    x24 = pt.expected_rows(np.array([0] * 20 + [256000] + [0] * 20, np.int32), None)
    assert int(x16["peak"][0, 0]) << 8 == int(x24["peak"][0, 0])
    for order, depths in (((x16, x24), (16, 24)), ((x24, x16), (24, 16))):
        t = lx.truepeak_combine([(r.tobytes(), 1, d, 41, 48000) for r, d in zip(order, depths)])
        assert t.set == 0 and t.bit_depth == depths[0] and t.frames == 82
    louder = pt.expected_rows(np.array([0] * 20 + [256001] + [0] * 20, np.int32), None)
    assert lx.truepeak_combine([(x16.tobytes(), 1, 16, 41, 48000), (louder.tobytes(), 1, 24, 41, 48000)]).set == 1


def test_argument_checks(pkg, dec):
    L, lx = pkg.lacx.lib(), pkg.lacx
    spans, srcs = (lx.Span * 1)(), (lx.DigestSource * 1)()
    assert L.lacx_decoder_truepeak_batch_device(dec, None, 1, None, None, None, None) == lx.E_INVALID and _last_error(pkg) == "null argument or empty batch"
    assert L.lacx_decoder_truepeak_batch_device(dec, spans, 0, None, None, None, None) == lx.E_INVALID
    assert L.lacx_decoder_truepeak_batch_device(None, spans, 1, None, None, None, None) == lx.E_INVALID and _last_error(pkg) == "null decoder"
    assert L.lacx_decoder_truepeak_pcm_batch_device(dec, None, 1, None, None, None, None) == lx.E_INVALID and _last_error(pkg) == "null argument or empty batch"
    assert L.lacx_decoder_truepeak_pcm_batch_device(dec, srcs, 0, None, None, None, None) == lx.E_INVALID
    assert L.lacx_decoder_truepeak_pcm_batch_device(None, srcs, 1, None, None, None, None) == lx.E_INVALID and _last_error(pkg) == "null decoder"
    rows, count = C.POINTER(lx.TruePeakRow)(), C.c_uint32(5)
    assert L.lacx_decoder_item_truepeak_rows(dec, 0, C.byref(rows), C.byref(count)) == lx.E_INVALID and count.value == 0
    assert _last_error(pkg) == "no such item in the last true peak call"
    assert L.lacx_decoder_item_truepeak_rows(dec, 0, None, C.byref(count)) == lx.E_INVALID and _last_error(pkg) == "null argument"
    ok = bytes(32)
    for sets, text in (([], "null argument or no sets"), ([(ok, 3, 16, 5, 48000)], "unsupported channel count"), ([(ok, 2, 8, 5, 48000)], "unsupported bit depth: 8"),
                       ([(ok, 2, 16, 5, 22050)], "unsupported sample rate: 22050"), ([(ok, 2, 16, 16385, 48000)], "row count does not match the frames"),
                       ([(ok, 2, 16, 0, 48000)], "row count does not match the frames")):
        with pytest.raises(ValueError, match=text):
            lx.truepeak_combine(sets)
    out = lx.TruePeak()
    out.frames = 9
    assert L.lacx_truepeak_combine(None, None, None, None, None, None, 1, C.byref(out)) == lx.E_INVALID and bytes(out) == bytes(96)
    d = lx.Decoder()
    for call in (lambda: d.truepeak_batch([]), lambda: d.truepeak_pcm_batch([])):
        with pytest.raises(ValueError):
            call()
    d.close()


def test_item_checks_before_the_device(pkg, dec):
    """The container is judged per item on the host, strictly: a refused one keeps the parser's code and text, a zeroed
    result and no rows; without a device the items that pass carry LACX_E_DEVICE and the call returns it.  (With a device
    only items that fail on the host are in the batch, so that nothing runs on it.)"""
    L, lx = pkg.lacx.lib(), pkg.lacx
    have_device = lx.device_count() > 0
    st16 = _fixture("small/n257_st16_ms.lac")
    cases = [(b"XX" + st16[2:], lx.E_INVALID, "[decode-error] invalid frame header"), (st16[:12], lx.E_INVALID, None)]
    if not have_device:
        cases += [(st16, lx.E_DEVICE, "no usable HIP device")]
    n = len(cases)
    keep = [(C.c_uint8 * len(x)).from_buffer_copy(x) for x, _, _ in cases]
    spans = (lx.Span * n)(*[lx.Span(C.cast(b, C.POINTER(C.c_uint8)), len(b)) for b in keep])
    rcs = (C.c_int * n)(*([-1] * n))
    out = (lx.TruePeak * n)()
    for o in out:
        o.frames, o.rows = 9, 9
    ms = C.c_float(5.0)
    rc = L.lacx_decoder_truepeak_batch_device(dec, spans, n, None, rcs, out, C.byref(ms))
    assert ms.value == 0.0
    whole = _last_error(pkg)
    digest_rcs = (C.c_int * n)(*([-1] * n))
    L.lacx_decoder_digest_batch_device(dec, spans, n, None, digest_rcs, None, None)
    for i, (x, code, msg) in enumerate(cases):
        text = L.lacx_decoder_item_error(dec, i).decode()
        assert digest_rcs[i] == code == rcs[i] and text.startswith(msg or "[decode-error] "), "as the digest form judges it"
        assert bytes(out[i]) == bytes(96), i
    rc = L.lacx_decoder_truepeak_batch_device(dec, spans, n, None, rcs, out, C.byref(ms))
    for i, (x, code, msg) in enumerate(cases):
        text = L.lacx_decoder_item_error(dec, i).decode()
        assert rcs[i] == code and (text == msg if msg else text.startswith("[decode-error] ")), (i, text)
        rows, count = C.POINTER(lx.TruePeakRow)(), C.c_uint32(5)
        assert L.lacx_decoder_item_truepeak_rows(dec, i, C.byref(rows), C.byref(count)) == lx.OK and count.value == 0
    if have_device:
        assert rc == lx.E_INVALID and whole == "stream 0: [decode-error] invalid frame header"
    else:
        assert rc == lx.E_DEVICE and whole == "no usable HIP device"
    d = lx.Decoder()
    if have_device:
        with pytest.raises(lx.BatchDecodeError) as e:
            d.truepeak_batch([cases[0][0]])
        assert e.value.errors == {0: cases[0][2]} and e.value.results == [None]
        with pytest.raises(RuntimeError, match=r"^\[decode-error\] invalid frame header$"):
            d.truepeak(cases[0][0])
    else:
        with pytest.raises(RuntimeError, match="no usable HIP device"):
            d.truepeak(st16)
    d.close()


def test_source_checks_are_the_digest_forms(pkg, dec):
    """truepeak_pcm judges every item as lacx_decoder_digest_pcm_batch_device does: the same texts, a zeroed result, no rows."""
    L, lx = pkg.lacx.lib(), pkg.lacx
    have_device = lx.device_count() > 0
    P = lx.PCM_PLANAR_I32
    cases = [(None, FAKE, P, 2, 257, 48000, 16), (FAKE, FAKE, 3, 2, 257, 48000, 16), (FAKE, FAKE, P, 3, 257, 48000, 16), (FAKE, FAKE, P, 2, 0, 48000, 16),
             (FAKE, FAKE, P, 2, 1 << 56, 48000, 16), (FAKE, FAKE, P, 2, 257, 22050, 16), (FAKE, FAKE, P, 2, 257, 48000, 8),
             (FAKE + 2, FAKE, P, 2, 257, 48000, 16), (FAKE, None, lx.PCM_INTERLEAVED_I24, 2, 257, 48000, 16)]
    n = len(cases)
    items = (lx.DigestSource * n)()
    for k, (d0, d1, layout, ch, frames, rate, depth) in enumerate(cases):
        items[k] = lx.DigestSource(lx.Pcm(d0, d1, layout, ch), frames, rate, depth)
    rcs = (C.c_int * n)(*([-1] * n))
    rc = L.lacx_decoder_digest_pcm_batch_device(dec, items, n, None, rcs, None, None)
    texts = [L.lacx_decoder_item_error(dec, i).decode() for i in range(n)]
    assert all(rcs[i] == lx.E_INVALID and texts[i] for i in range(n)) and len(set(texts)) == n
    rcs = (C.c_int * n)(*([-1] * n))
    out = (lx.TruePeak * n)()
    for o in out:
        o.frames = 9
    rc2 = L.lacx_decoder_truepeak_pcm_batch_device(dec, items, n, None, rcs, out, None)
    for i in range(n):
        assert rcs[i] == lx.E_INVALID and L.lacx_decoder_item_error(dec, i).decode() == texts[i], i
        assert bytes(out[i]) == bytes(96), i
        rows, count = C.POINTER(lx.TruePeakRow)(), C.c_uint32(5)
        assert L.lacx_decoder_item_truepeak_rows(dec, i, C.byref(rows), C.byref(count)) == lx.OK and count.value == 0
    assert rc == rc2 == (lx.E_INVALID if have_device else lx.E_DEVICE)
