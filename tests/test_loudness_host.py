"""The loudness entry points without a device: the new structs against the library's own sizeof, the K-weighting coefficients
against the BS.1770 table and the Python formula, lacx_loudness_combine against the totals restated in plain Python floats
(tests/loudtwin.py) over rows that scipy made, album combination, the flags, the checks of the call's arguments, and what
a call does for its items before any device work."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import __graft_entry__ as ge
import loudtwin as lt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NEW = ("lacx_decoder_loudness_batch_device", "lacx_decoder_loudness_pcm_batch_device", "lacx_decoder_item_loudness_rows", "lacx_loudness_combine")
FAKE = 1 << 40  # a "device address" that is never dereferenced: every call here stops before the device
# ITU-R BS.1770-4, table 1 and 2 (48 kHz)
TABLE_48K = {"shelf_b": (1.53512485958697, -2.69169618940638, 1.19839281085285), "shelf_a": (-1.69065929318241, 0.73248077421585),
             "hp_a": (-1.99004745483398, 0.99007225036621)}


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
    for name, cls, size in (("loudness_row", lx.LoudnessRow, 16), ("loudness", lx.Loudness, 72)):
        assert structs[name] is cls and L.lacx_sizeof(name.encode()) == C.sizeof(cls) == size, name
    t = lx.Loudness
    assert (t.frames.offset, t.sample_rate.offset, t.channels.offset, t.bit_depth.offset, t.flags.offset, t.subblocks.offset, t.gating_blocks.offset,
            t.above_absolute.offset, t.above_relative.offset, t.integrated_lufs.offset, t.relative_gate_lufs.offset, t.momentary_max_lufs.offset,
            t.shortterm_max_lufs.offset, t.range_lu.offset) == (0, 8, 12, 13, 14, 16, 20, 24, 28, 32, 40, 48, 56, 64)
    for field, name in (("flags", "flags"), ("subblocks", "subblocks"), ("integrated", "integrated_lufs"), ("range", "range_lu")):
        assert lt.TOT_T.fields[field][1] == getattr(t, name).offset
    assert (lx.LOUDNESS_TOO_SHORT, lx.LOUDNESS_SILENT) == (lt.TOO_SHORT, lt.SILENT)
    for text in ("#define LACX_LOUDNESS_TOO_SHORT 1u", "#define LACX_LOUDNESS_SILENT 2u"):
        assert text in header


def test_coefficients_are_the_standards_and_the_formulas():
    """csrc/loudness_plan.h's coefficients (through the twin): at 48 kHz the BS.1770 table to within 1e-14, at every rate
    the Python formula exactly or to 1 ulp; A is 256 zero-input steps of the same filter."""
    from scipy.signal import lfilter
    filters = lt.twin_filters()
    k = filters[48000]
    table = TABLE_48K["shelf_b"] + tuple(-x for x in TABLE_48K["shelf_a"]) + (1.0, -2.0, 1.0) + tuple(-x for x in TABLE_48K["hp_a"])
    worst = max(abs(a - b) for a, b in zip(k[:10], table))
    print("48 kHz against the table:", worst)
    assert worst <= 1e-14
    for rate in lt.RATES:
        (sb, sa), (hb, ha) = lt.coefficients(rate)
        want = sb + [-sa[1], -sa[2]] + hb + [-ha[1], -ha[2]]
        for got, w in zip(filters[rate][:10], want):
            assert got == w or abs(got - w) <= math.ulp(w), (rate, got, w)
        # A's column j: the state 256 zero-input steps after unit state j -- an impulse response of each biquad's state
        A = filters[rate][10:].reshape(4, 4)
        assert np.all(A[:2, 2:] == 0.0), "the high-pass state does not feed the shelf"
        for j in range(2):  # shelf states alone: lfilter's zi is the same transposed form
            zi = np.zeros(2)
            zi[j] = 1.0
            _, zf = lfilter(sb, sa, np.zeros(lt.CHUNK), zi=zi)
            assert np.allclose(A[:2, j], zf, rtol=1e-9, atol=1e-300), (rate, j)


def _close(got, want, tol):
    lt.close_totals(got, want, tol)


def test_combine_is_the_restatement_over_the_same_rows(pkg):
    """lacx_loudness_combine over rows scipy made for the whole corpus: counts and flags exact, every level within 1e-9 LU
    (sums of under 2^32 positive doubles, 10 log10(1 + e) ~ 4.35 e); the twin's copy of the same code agrees bit for bit."""
    lx = pkg.lacx
    items = lt.corpus()
    lt.assert_content(items)
    flags = set()
    for it in items:
        rows = lt.item_rows(it)
        got = lx.loudness_combine([(rows, it.channels, it.depth, it.rate)])
        want = lt.item_totals(it)
        _close(lt.totals_of(got), want, lt.COMBINE_TOL)
        assert bytes(got) == lt._totals_bytes(lt.twin_combine([(rows, it.channels, it.depth, it.rate)])), it.name
        assert got.frames == (it.left.size // (it.rate // 10)) * (it.rate // 10) and got.sample_rate == it.rate
        assert got.too_short == (it.left.size < 4 * (it.rate // 10)) and (got.shortterm_max_lufs == -math.inf) == (got.subblocks < 30), it.name
        if got.too_short:
            assert got.range_lu == 0.0 and all(getattr(got, n) == -math.inf for n in ("integrated_lufs", "relative_gate_lufs", "momentary_max_lufs", "shortterm_max_lufs"))
        flags.add(got.flags)
    assert flags == {0, lt.TOO_SHORT, lt.SILENT}


def test_silence_and_short_items(pkg):
    lx = pkg.lacx
    silent = lx.loudness_combine([(np.zeros((40, 2)), 2, 16, 48000)])
    assert silent.flags == lx.LOUDNESS_SILENT and silent.integrated_lufs == -math.inf and silent.momentary_max_lufs == -math.inf
    assert silent.gating_blocks == 37 and silent.above_absolute == 0 and silent.range_lu == 0.0 and silent.gain == math.inf
    for S in (0, 1, 3):
        short = lx.loudness_combine([(np.ones((S, 2)), 2, 16, 48000)])
        assert short.flags == lx.LOUDNESS_TOO_SHORT and short.gating_blocks == 0 and short.subblocks == S and short.frames == 4800 * S
    assert lx.loudness_combine([(np.ones((4, 2)), 2, 16, 48000)]).flags in (0, lx.LOUDNESS_SILENT)


def test_album_combination(pkg):
    """Several sets: gates and means over the union, z normalised per set by its own rate and depth, nothing straddles
    sets; a set combined with itself keeps its integrated loudness; mono reads 3.01 LU below its dual-mono form."""
    lx = pkg.lacx
    items = [it for it in lt.corpus() if "|content" in it.name]
    pairs = [(a, b) for a in items for b in items if a.name < b.name and a.rate != b.rate][:24]
    assert pairs
    for a, b in pairs:
        sets = [(lt.item_rows(x), x.channels, x.depth, x.rate) for x in (a, b)]
        got = lx.loudness_combine(sets)
        _close(lt.totals_of(got), lt.expected_totals(sets), lt.COMBINE_TOL)
        assert got.gating_blocks == sum(max(0, len(s[0]) - 3) for s in sets) and (got.sample_rate, got.channels, got.bit_depth) == (a.rate, a.channels, a.depth)
    for it in items:
        one = (lt.item_rows(it), it.channels, it.depth, it.rate)
        single, double = lx.loudness_combine([one]), lx.loudness_combine([one, one])
        assert double.gating_blocks == 2 * single.gating_blocks and double.frames == 2 * single.frames
        assert single.integrated_lufs == double.integrated_lufs or abs(single.integrated_lufs - double.integrated_lufs) <= lt.COMBINE_TOL
    mono = next(it for it in items if it.channels == 1 and it.name.startswith("tone"))
    rows = np.array(lt.item_rows(mono))
    dual = rows.copy()
    dual[:, 1] = dual[:, 0]
    d = lx.loudness_combine([(dual, 2, mono.depth, mono.rate)]).integrated_lufs - lx.loudness_combine([(rows, 1, mono.depth, mono.rate)]).integrated_lufs
    assert abs(d - 10.0 * math.log10(2.0)) < 1e-9


def test_argument_checks(pkg, dec):
    L, lx = pkg.lacx.lib(), pkg.lacx
    spans, srcs = (lx.Span * 1)(), (lx.DigestSource * 1)()
    assert L.lacx_decoder_loudness_batch_device(dec, None, 1, None, None, None, None) == lx.E_INVALID and _last_error(pkg) == "null argument or empty batch"
    assert L.lacx_decoder_loudness_batch_device(dec, spans, 0, None, None, None, None) == lx.E_INVALID
    assert L.lacx_decoder_loudness_batch_device(None, spans, 1, None, None, None, None) == lx.E_INVALID and _last_error(pkg) == "null decoder"
    assert L.lacx_decoder_loudness_pcm_batch_device(dec, None, 1, None, None, None, None) == lx.E_INVALID and _last_error(pkg) == "null argument or empty batch"
    assert L.lacx_decoder_loudness_pcm_batch_device(dec, srcs, 0, None, None, None, None) == lx.E_INVALID
    assert L.lacx_decoder_loudness_pcm_batch_device(None, srcs, 1, None, None, None, None) == lx.E_INVALID and _last_error(pkg) == "null decoder"
    rows, count = C.POINTER(lx.LoudnessRow)(), C.c_uint32(5)
    assert L.lacx_decoder_item_loudness_rows(dec, 0, C.byref(rows), C.byref(count)) == lx.E_INVALID and count.value == 0
    assert _last_error(pkg) == "no such item in the last loudness call"
    assert L.lacx_decoder_item_loudness_rows(dec, 0, None, C.byref(count)) == lx.E_INVALID and _last_error(pkg) == "null argument"
    ok = np.ones((5, 2))
    for sets, text in (([], "null argument or no sets"), ([(ok, 3, 16, 48000)], "unsupported channel count"), ([(ok, 2, 8, 48000)], "unsupported bit depth: 8"),
                       ([(ok, 2, 16, 22050)], "unsupported sample rate: 22050")):
        with pytest.raises(ValueError, match=text):
            lx.loudness_combine(sets)
    out = lx.Loudness()
    out.frames = 9
    assert L.lacx_loudness_combine(None, None, None, None, None, 1, C.byref(out)) == lx.E_INVALID and bytes(out) == bytes(72)
    d = lx.Decoder()
    for call in (lambda: d.loudness_batch([]), lambda: d.loudness_pcm_batch([])):
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
    out = (lx.Loudness * n)()
    for o in out:
        o.frames, o.subblocks = 9, 9
    ms = C.c_float(5.0)
    rc = L.lacx_decoder_loudness_batch_device(dec, spans, n, None, rcs, out, C.byref(ms))
    assert ms.value == 0.0
    whole = _last_error(pkg)
    digest_rcs = (C.c_int * n)(*([-1] * n))
    L.lacx_decoder_digest_batch_device(dec, spans, n, None, digest_rcs, None, None)
    for i, (x, code, msg) in enumerate(cases):
        assert digest_rcs[i] == code and L.lacx_decoder_item_error(dec, i).decode().startswith(msg or "[decode-error] "), "as the digest form judges it"
    rc = L.lacx_decoder_loudness_batch_device(dec, spans, n, None, rcs, out, C.byref(ms))
    for i, (x, code, msg) in enumerate(cases):
        text = L.lacx_decoder_item_error(dec, i).decode()
        assert rcs[i] == code and (text == msg if msg else text.startswith("[decode-error] ")), (i, text)
        assert bytes(out[i]) == bytes(72), i
        if code == lx.E_INVALID:  # the strict parser's own code and text
            assert L.lacx_stream_parse(keep[i], len(x), C.byref(lx.StreamInfo())) == code and _last_error(pkg) == text
        rows, count = C.POINTER(lx.LoudnessRow)(), C.c_uint32(5)
        assert L.lacx_decoder_item_loudness_rows(dec, i, C.byref(rows), C.byref(count)) == lx.OK and count.value == 0
    if have_device:
        assert rc == lx.E_INVALID and whole == "stream 0: [decode-error] invalid frame header"
    else:
        assert rc == lx.E_DEVICE and whole == "no usable HIP device"
    d = lx.Decoder()
    if have_device:
        with pytest.raises(lx.BatchDecodeError) as e:
            d.loudness_batch([cases[0][0]])
        assert e.value.errors == {0: cases[0][2]} and e.value.results == [None]
        with pytest.raises(RuntimeError, match=r"^\[decode-error\] invalid frame header$"):
            d.loudness(cases[0][0])
    else:
        with pytest.raises(RuntimeError, match="no usable HIP device"):
            d.loudness(st16)
    d.close()


def test_source_checks_are_the_digest_forms(pkg, dec):
    """loudness_pcm judges every item as lacx_decoder_digest_pcm_batch_device does: the same texts, a zeroed result, no rows."""
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
    out = (lx.Loudness * n)()
    for o in out:
        o.frames = 9
    rc2 = L.lacx_decoder_loudness_pcm_batch_device(dec, items, n, None, rcs, out, None)
    for i in range(n):
        assert rcs[i] == lx.E_INVALID and L.lacx_decoder_item_error(dec, i).decode() == texts[i], i
        assert bytes(out[i]) == bytes(72), i
        rows, count = C.POINTER(lx.LoudnessRow)(), C.c_uint32(5)
        assert L.lacx_decoder_item_loudness_rows(dec, i, C.byref(rows), C.byref(count)) == lx.OK and count.value == 0
    assert rc == rc2 == (lx.E_INVALID if have_device else lx.E_DEVICE)
