"""The spectrum entry points without a device: the new structs against the library's own sizeof, the plan's window and
twiddle tables against numpy.longdouble, sp_check, lacx_spectrum_combine against the totals restated in Python
(tests/spectwin.py) on the twin's rows, the level of a full-scale sine, the bandwidth of the band-limited item, the checks
of the call's arguments, and what a call does for its items before any device work."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import __graft_entry__ as ge
import spectwin as st

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NEW = ("lacx_decoder_spectrum_batch_device", "lacx_decoder_spectrum_pcm_batch_device", "lacx_decoder_item_spectrum_rows", "lacx_spectrum_combine")
FAKE = 1 << 40  # a "device address" that is never dereferenced: every call here stops before the device


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


def test_symbols_and_structs(pkg):
    L, lx = pkg.lacx.lib(), pkg.lacx
    header = open(os.path.join(ROOT, "include", "lacx.h")).read()
    for name in NEW:
        assert hasattr(L, name) and name in lx.EXPORTS
        assert re.search(rf"\b{name}\s*\(", header), name
        assert header.index(name) < header.index("#ifndef LACX_H"), name  # listed in the comment block at the top
    structs = lx.abi_structs()
    for name, cls, dt in (("spectrum_row", lx.SpectrumRow, st.ROW_T), ("spectrum", lx.Spectrum, st.TOT_T)):
        assert structs[name] is cls and L.lacx_sizeof(name.encode()) == C.sizeof(cls) == dt.itemsize, name
    assert (lx.SPECTRUM_WINDOWS, lx.SPECTRUM_BANDS, lx.SPECTRUM_ROW_FRAMES) == (st.WINDOWS, st.BANDS, st.ROW)
    for word in ("a lenient form", "more than two channels", "windows other than Hann", "hops other than N / 2", "a spectrogram", "phase"):
        assert word in header[header.index("/* Spectrum:"):header.index("typedef struct lacx_spectrum_row")], word


def test_the_plans_tables_are_long_double_rounded_once():
    """Window and twiddles of every length, bit for bit what numpy.longdouble evaluation rounded to double gives."""
    pi = np.arccos(np.longdouble(-1))
    assert np.finfo(np.longdouble).nmant >= 63, "this check needs an extended long double"
    for window in st.WINDOWS:
        w, tw = st.twin_tables(window)
        n = np.arange(window).astype(np.longdouble)
        want = np.longdouble(0.5) - np.longdouble(0.5) * np.cos(np.longdouble(2) * pi * n / np.longdouble(window))
        assert np.array_equal(w, want.astype(np.float64)), window
        ang = np.longdouble(2) * pi * np.arange(window // 2).astype(np.longdouble) / np.longdouble(window)
        assert np.array_equal(tw[:, 0], np.cos(ang).astype(np.float64)) and np.array_equal(tw[:, 1], (-np.sin(ang)).astype(np.float64)), window
        assert w[0] == 0.0 and w[window // 2] == 1.0 and abs(float(np.sum(w * w)) - 3.0 * window / 8.0) < 1e-9
    assert st.twin_tables(128) is None and st.twin_tables(8192) is None and st.twin_tables(1000) is None


def test_sp_check_refuses_counts_of_2_to_the_31_or_more():
    assert st.twin_check([5, 16385, 1 << 30], 256) == ""
    assert st.twin_check([((1 << 31) - 1) * 128], 256) == "" and st.twin_check([(1 << 31) * 128], 256) == "item holds 2^31 windows or more"
    assert st.twin_check([(1 << 31) * 2048 - 2047], 4096) == "item holds 2^31 windows or more"
    most = ((1 << 31) - 1) * 2048  # 2^31 - 1 windows at N = 4096: 2^28 rows
    assert st.twin_check([most] * 7, 4096) == "" and st.twin_check([most] * 8, 4096) == "batch holds 2^31 rows or more"


def _rows(it):
    return st.twin_rows(it)


def test_combine_is_the_restated_totals(pkg):
    """lacx_spectrum_combine over the twin's rows: integers byte for byte, levels within 1e-9 dB of the Python totals; the
    twin's own build of spectrum_rows.h gives the same record byte for byte."""
    lx = pkg.lacx
    for it in st.corpus():
        rows = _rows(it)
        for floor in (st.FLOOR, -60.0):
            got = lx.spectrum_combine(rows.tobytes(), it.channels, it.depth, len(it.left), it.rate, it.window, floor)
            want = st.expected_totals(rows["power"], it.channels, it.depth, len(it.left), it.rate, it.window, floor)
            st.same_totals(st.totals_of(got), want)
            assert bytes(got) == st.twin_combine(rows, it.channels, it.depth, len(it.left), it.rate, it.window, floor)[1], it.name
        assert got.windows == -(-len(it.left) // (it.window // 2)) and got.rows == len(rows) == -(-len(it.left) // st.ROW)
    by = {it.name: it for it in st.corpus()}
    it = by["silence|N256|2ch16"]
    t = lx.spectrum_combine(_rows(it).tobytes(), 2, 16, len(it.left), it.rate, 256)
    assert all(x == -math.inf for ch in t.level_db for x in ch) and list(t.bandwidth_hz) == [0.0, 0.0] and list(t.peak_band) == [0, 0]


def test_a_full_scale_sine_reads_zero_dbfs(pkg):
    """Summed over the bands it falls into, within 0.01 dB: on an item of 1024 windows of which only the last is cut (the
    zero-padded tail costs 10 log10(1 - 0.5 / 1024) = -0.002 dB, the amplitude 32767 / 32768 another -0.0003 dB)."""
    lx = pkg.lacx
    it = {x.name: x for x in st.corpus()}["sine|level|N256|1ch16"]
    for rows in (st.item_rows(it), _rows(it)["power"]):
        t = st.expected_totals(rows, 1, 16, len(it.left), it.rate, 256)
        assert t.windows == 1024 and t.peak_band[0] == 32
        near = [t.level_db[0][b] for b in (31, 32, 33)]  # bin 64 in band 32, its Hann neighbours 63 and 65 in bands 31 and 32
        assert abs(10.0 * math.log10(sum(10.0 ** (x / 10.0) for x in near))) <= 0.01, near
    got = lx.spectrum_combine(_rows(it).tobytes(), 1, 16, len(it.left), it.rate, 256)
    assert abs(10.0 * math.log10(sum(10.0 ** (got.level_db[0][b] / 10.0) for b in (31, 32, 33)))) <= 0.01
    assert got.peak_band[0] == 32 and got.peak_hz(0) == 32.5 * 44100 / 128.0


def test_the_band_limited_items_bandwidth_is_its_construction(pkg):
    """Sines on bins 1 .. 2 c of 256 (left c = 40, right c = 30): the highest sine sits on the first bin of band c, a band
    edge minus two bins, so that its Hann neighbour stays inside the band; the edge comes from the construction."""
    lx = pkg.lacx
    it = {x.name: x for x in st.corpus()}["bandlimit|N256|2ch24"]
    edges = ((st.CUTOFF_BAND + 1) * it.rate / 128.0, (st.CUTOFF_BAND - 10 + 1) * it.rate / 128.0)
    assert st.item_totals(it).bandwidth_hz == edges, "the restatement first"
    got = lx.spectrum_combine(_rows(it).tobytes(), 2, 24, len(it.left), it.rate, 256)
    assert tuple(got.bandwidth_hz) == edges and got.floor_db == st.FLOOR
    assert lx.spectrum_combine(_rows(it).tobytes(), 2, 24, len(it.left), it.rate, 256, -200.0).bandwidth_hz[0] == it.rate / 2.0


def test_argument_checks(pkg, dec):
    L, lx = pkg.lacx.lib(), pkg.lacx
    spans, srcs = (lx.Span * 1)(), (lx.DigestSource * 1)()
    f = C.c_double(-100.0)
    assert L.lacx_decoder_spectrum_batch_device(dec, None, 1, 2048, f, None, None, None, None) == lx.E_INVALID and _last_error(pkg) == "null argument or empty batch"
    assert L.lacx_decoder_spectrum_batch_device(dec, spans, 0, 2048, f, None, None, None, None) == lx.E_INVALID
    assert L.lacx_decoder_spectrum_batch_device(None, spans, 1, 2048, f, None, None, None, None) == lx.E_INVALID and _last_error(pkg) == "null decoder"
    assert L.lacx_decoder_spectrum_pcm_batch_device(dec, None, 1, 2048, f, None, None, None, None) == lx.E_INVALID and _last_error(pkg) == "null argument or empty batch"
    assert L.lacx_decoder_spectrum_pcm_batch_device(None, srcs, 1, 2048, f, None, None, None, None) == lx.E_INVALID and _last_error(pkg) == "null decoder"
    for window in (0, 128, 1000, 2049, 8192):  # fails the call, before any item is looked at
        rcs = (C.c_int * 1)(-7)
        assert L.lacx_decoder_spectrum_batch_device(dec, spans, 1, window, f, None, rcs, None, None) == lx.E_INVALID and rcs[0] == -7
        assert _last_error(pkg) == "unsupported spectrum window: %d" % window
        assert L.lacx_decoder_spectrum_pcm_batch_device(dec, srcs, 1, window, f, None, rcs, None, None) == lx.E_INVALID and rcs[0] == -7
        assert _last_error(pkg) == "unsupported spectrum window: %d" % window
    rows, count = C.POINTER(lx.SpectrumRow)(), C.c_uint32(5)
    assert L.lacx_decoder_item_spectrum_rows(dec, 0, C.byref(rows), C.byref(count)) == lx.E_INVALID and count.value == 0
    assert _last_error(pkg) == "no such item in the last spectrum call"
    assert L.lacx_decoder_item_spectrum_rows(dec, 0, None, C.byref(count)) == lx.E_INVALID and _last_error(pkg) == "null argument"
    ok = bytes(1024)
    for args, text in (((ok, 3, 16, 5, 48000), "unsupported channel count"), ((ok, 2, 8, 5, 48000), "unsupported bit depth: 8"),
                       ((ok, 2, 16, 5, 22050), "unsupported sample rate: 22050"), ((ok, 2, 16, 16385, 48000), "row count does not match the frames"),
                       ((ok, 2, 16, 0, 48000), "row count does not match the frames"), ((ok, 2, 16, 5, 48000, 300), "unsupported spectrum window: 300")):
        with pytest.raises(ValueError, match=text):
            lx.spectrum_combine(*args)
    out = lx.Spectrum()
    out.frames = 9
    assert L.lacx_spectrum_combine(None, 1, 2, 16, 5, 48000, 2048, f, C.byref(out)) == lx.E_INVALID and bytes(out) == bytes(1080)
    d = lx.Decoder()
    for call in (lambda: d.spectrum_batch([]), lambda: d.spectrum_pcm_batch([]), lambda: d.spectrum_batch([b"x"], window=300),
                 lambda: d.spectrum_pcm_batch([((FAKE, FAKE, 0, 2, 257), 48000, 16)], window=300)):
        with pytest.raises(ValueError):
            call()
    d.close()


def test_item_checks_before_the_device(pkg, dec):
    """The container is judged per item on the host, strictly, as the digest form judges it: a refused one keeps the
    parser's code and text, a zeroed result and no rows; without a device the items that pass carry LACX_E_DEVICE."""
    L, lx = pkg.lacx.lib(), pkg.lacx
    have_device = lx.device_count() > 0
    st16 = _fixture("small/n257_st16_ms.lac")
    cases = [(b"XX" + st16[2:], lx.E_INVALID, "[decode-error] invalid frame header"), (st16[:12], lx.E_INVALID, None)]
    if not have_device:
        cases += [(st16, lx.E_DEVICE, "no usable HIP device")]
    n = len(cases)
    keep = [(C.c_uint8 * len(x)).from_buffer_copy(x) for x, _, _ in cases]
    spans = (lx.Span * n)(*[lx.Span(C.cast(b, C.POINTER(C.c_uint8)), len(b)) for b in keep])
    digest_rcs = (C.c_int * n)(*([-1] * n))
    L.lacx_decoder_digest_batch_device(dec, spans, n, None, digest_rcs, None, None)
    rcs = (C.c_int * n)(*([-1] * n))
    out = (lx.Spectrum * n)()
    for o in out:
        o.frames, o.rows = 9, 9
    ms = C.c_float(5.0)
    rc = L.lacx_decoder_spectrum_batch_device(dec, spans, n, 512, C.c_double(-100.0), None, rcs, out, C.byref(ms))
    assert ms.value == 0.0
    for i, (x, code, msg) in enumerate(cases):
        text = L.lacx_decoder_item_error(dec, i).decode()
        assert digest_rcs[i] == code == rcs[i] and (text == msg if msg else text.startswith("[decode-error] ")), (i, text)
        assert bytes(out[i]) == bytes(1080), i
        rows, count = C.POINTER(lx.SpectrumRow)(), C.c_uint32(5)
        assert L.lacx_decoder_item_spectrum_rows(dec, i, C.byref(rows), C.byref(count)) == lx.OK and count.value == 0
    assert rc == (lx.E_INVALID if have_device else lx.E_DEVICE)
    d = lx.Decoder()
    if have_device:
        with pytest.raises(lx.BatchDecodeError) as e:
            d.spectrum_batch([cases[0][0]])
        assert e.value.errors == {0: cases[0][2]} and e.value.results == [None]
    else:
        with pytest.raises(RuntimeError, match="no usable HIP device"):
            d.spectrum(st16)
    d.close()


def test_source_checks_are_the_digest_forms(pkg, dec):
    """spectrum_pcm judges every item as lacx_decoder_digest_pcm_batch_device does: the same texts, a zeroed result, no rows."""
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
    out = (lx.Spectrum * n)()
    for o in out:
        o.frames = 9
    rc2 = L.lacx_decoder_spectrum_pcm_batch_device(dec, items, n, 2048, C.c_double(-100.0), None, rcs, out, None)
    for i in range(n):
        assert rcs[i] == lx.E_INVALID and L.lacx_decoder_item_error(dec, i).decode() == texts[i], i
        assert bytes(out[i]) == bytes(1080), i
        rows, count = C.POINTER(lx.SpectrumRow)(), C.c_uint32(5)
        assert L.lacx_decoder_item_spectrum_rows(dec, i, C.byref(rows), C.byref(count)) == lx.OK and count.value == 0
    assert rc == rc2 == (lx.E_INVALID if have_device else lx.E_DEVICE)
