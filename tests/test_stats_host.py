"""The audio statistics' entry points without a device: the new structs against the library's own sizeof, lacx_stats_combine
against Python ints on fabricated rows (the 128-bit carries, the lead / trail rule with lost rows, mono), the checks of the
call's arguments, and what a call does for its items before any device work."""
import ctypes as C
import os
import re

import pytest

import __graft_entry__ as ge
import statstwin as sw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NEW = ("lacx_decoder_stats_batch_device", "lacx_decoder_stats_pcm_batch_device", "lacx_decoder_item_block_stats", "lacx_stats_combine")
FAKE = 1 << 40  # a "device address" that is never dereferenced: every call here stops before the device
LO24, HI24 = -(1 << 23), (1 << 23) - 1


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
    for name, cls, size in (("channel_stats", lx.ChannelStats, 40), ("block_stats", lx.BlockStats, 104), ("channel_totals", lx.ChannelTotals, 64),
                            ("stats", lx.Stats, 192)):
        assert structs[name] is cls and L.lacx_sizeof(name.encode()) == C.sizeof(cls) == size, name
    # the twin's and the tests' own numpy view of the same records
    assert (sw.CH_T.itemsize, sw.ROW_T.itemsize, sw.TCH_T.itemsize, sw.TOT_T.itemsize) == (40, 104, 64, 192)
    c, b, t, s = lx.ChannelStats, lx.BlockStats, lx.ChannelTotals, lx.Stats
    assert (c.min.offset, c.max.offset, c.or_bits.offset, c.full_scale.offset, c.zeros.offset, c.sum.offset, c.sum_sq.offset) == (0, 4, 8, 12, 16, 24, 32)
    assert (b.frames.offset, b.code.offset, b.lead_zero_frames.offset, b.trail_zero_frames.offset, b.differing.offset, b.ch.offset) == (0, 4, 8, 12, 16, 24)
    assert (t.full_scale.offset, t.zeros.offset, t.sum_lo.offset, t.sum_hi.offset, t.sum_sq_lo.offset, t.sum_sq_hi.offset) == (16, 24, 32, 40, 48, 56)
    assert (s.frames.offset, s.sample_rate.offset, s.channels.offset, s.bit_depth.offset, s.blocks.offset, s.lost_blocks.offset, s.lost_frames.offset,
            s.silent_blocks.offset, s.lead_zero_frames.offset, s.trail_zero_frames.offset, s.differing.offset, s.ch.offset) == (0, 8, 12, 13, 16, 20, 24, 32, 40, 48, 56, 64)
    for field in ("min", "or_bits", "sum", "sum_sq"):
        assert sw.CH_T.fields[field][1] == getattr(c, field).offset
    for field, name in (("lead", "lead_zero_frames"), ("differing", "differing"), ("ch", "ch")):
        assert sw.ROW_T.fields[field][1] == getattr(b, name).offset
    for field, name in (("lost_frames", "lost_frames"), ("trail", "trail_zero_frames"), ("ch", "ch")):
        assert sw.TOT_T.fields[field][1] == getattr(s, name).offset


def _combine(lx, rows, channels, depth, rate=48000):
    """lacx_stats_combine on fabricated rows -> (Totals, the Stats record)."""
    recs = [lx.BlockStats.from_buffer_copy(r.tobytes()) for r in sw.row_records(rows)]
    out = lx.stats_combine(recs, channels, depth, rate)
    return sw.totals_of(out), out


def _full(frames, value, channels=2, depth=24):
    """A row of `frames` frames all equal to `value` in every channel."""
    lim = 1 << (depth - 1)
    ch = (value, value, value & ((1 << depth) - 1), frames if value in (-lim, lim - 1) else 0, frames if value == 0 else 0, frames * value, frames * value * value)
    silent = frames if value == 0 else 0
    return sw.Row(frames, 0, silent, silent, 0, (ch, ch if channels == 2 else sw.ZERO_CH))


def _row(frames, lead, trail, lo, hi, channels=2, code=0):
    if code:
        return sw.Row(frames, code, 0, 0, 0, (sw.ZERO_CH, sw.ZERO_CH))
    ch = (lo, hi, 0xFFFF, 0, lead + trail, 3 * frames, 7 * frames)
    return sw.Row(frames, 0, lead, trail, 5 if channels == 2 else 0, (ch, ch if channels == 2 else sw.ZERO_CH))


def test_combine_carries_into_the_upper_words(pkg):
    """17 rows of 16384 frames at -2^23 in both channels: sum_sq needs bit 64, and the negative sum's upper word is all ones."""
    lx = pkg.lacx
    rows = [_full(16384, LO24)] * 17
    want = sw.expected_totals(rows, 2, 24, 48000)
    got, rec = _combine(lx, rows, 2, 24)
    assert got == want
    for c in (0, 1):
        assert rec.ch[c].sum_sq_hi == 1 and rec.ch[c].sum_hi == -1 and rec.ch[c].sum < 0
        assert rec.ch[c].sum == 17 * 16384 * LO24 and rec.ch[c].sum_sq == 17 * 16384 * (1 << 46) and rec.ch[c].sum_sq >> 64 == 1
        assert rec.ch[c].full_scale == 17 * 16384
    assert rec.wasted_bits == 23 and rec.peak == 1 << 23 and rec.dual_mono and rec.peak_dbfs == 0.0
    # sixteen rows still fit 64 bits; a positive sum carries too
    got16, rec16 = _combine(lx, rows[:16], 2, 24)
    assert got16 == sw.expected_totals(rows[:16], 2, 24, 48000) and rec16.ch[0].sum_sq_hi == 1 and rec16.ch[0].sum_sq_lo == 0
    big = [sw.Row(16384, 0, 0, 0, 0, ((1, HI24, 1, 0, 0, (1 << 63) - 1, (1 << 64) - 1), sw.ZERO_CH))] * 3
    gotb, recb = _combine(lx, big, 1, 24)
    assert gotb == sw.expected_totals(big, 1, 24, 48000) and recb.ch[0].sum_hi == 1 and recb.ch[0].sum_sq_hi == 2
    assert sw.twin_combine(rows, 2, 24, 48000) == want and sw.twin_combine(big, 1, 24, 48000) == gotb


@pytest.mark.parametrize("channels", [1, 2])
def test_combine_lead_trail_rule_and_lost_rows(pkg, channels):
    """Lost rows in front, in the middle and at the end: a lost block counts as sound for lead / trail and adds nothing to
    the totals; silent blocks extend the silence to the next block."""
    lx = pkg.lacx
    silent, sound = _full(1000, 0, channels, 16), _row(1000, 10, 20, -5, 9, channels)
    lost = _row(1000, 0, 0, 0, 0, channels, code=3)
    tail = _full(7, 0, channels, 16)
    cases = {
        "plain": [silent, silent, sound, silent, tail],
        "lost in front": [lost, silent, sound, silent],
        "lost in the middle": [silent, lost, sound, silent, silent],
        "lost at the end": [silent, sound, silent, lost],
        "lost between silence": [silent, lost, silent],
        "all silent": [silent, silent, tail],
        "all lost": [lost, lost],
        "one sounding row": [sound],
        "none": [],
    }
    want_edges = {"plain": (2010, 1027), "lost in front": (0, 1020), "lost in the middle": (1000, 2020), "lost at the end": (1010, 0),
                  "lost between silence": (1000, 1000), "all silent": (2007, 2007), "all lost": (0, 0), "one sounding row": (10, 20), "none": (0, 0)}
    for name, rows in cases.items():
        want = sw.expected_totals(rows, channels, 16, 44100)
        assert (want.lead, want.trail) == want_edges[name], name  # the restatement itself, against figures worked out by hand
        got, rec = _combine(lx, rows, channels, 16, 44100)
        assert got == want, name
        assert sw.twin_combine(rows, channels, 16, 44100) == want, name
        assert rec.lost_blocks == sum(1 for r in rows if r.code) and rec.lost_frames == 1000 * rec.lost_blocks
        assert bytes(rec.ch[1]) == bytes(64) or channels == 2
    _, rec = _combine(lx, cases["all lost"], channels, 16)
    assert (rec.ch[0].min, rec.ch[0].max, rec.peak, rec.wasted_bits) == (0, 0, 0, 16) and rec.peak_dbfs == float("-inf")
    # min / max come from decoded rows only, and not from the zeros of a lost one
    rows = [lost, _row(10, 0, 0, 3, 9, channels), _row(10, 0, 0, 5, 12, channels)]
    got, rec = _combine(lx, rows, channels, 16)
    assert (rec.ch[0].min, rec.ch[0].max) == (3, 12) and got == sw.expected_totals(rows, channels, 16, 48000)


def test_combine_arguments(pkg):
    L, lx = pkg.lacx.lib(), pkg.lacx
    rows = (lx.BlockStats * 1)()
    out = lx.Stats()
    out.frames = 9
    assert L.lacx_stats_combine(rows, 1, 2, 16, 48000, None) == lx.E_INVALID and _last_error(pkg) == "null argument"
    assert L.lacx_stats_combine(None, 1, 2, 16, 48000, C.byref(out)) == lx.E_INVALID and _last_error(pkg) == "null argument" and out.frames == 0
    assert L.lacx_stats_combine(rows, 1, 3, 16, 48000, C.byref(out)) == lx.E_INVALID and _last_error(pkg) == "unsupported channel count"
    assert L.lacx_stats_combine(rows, 1, 2, 8, 48000, C.byref(out)) == lx.E_INVALID and _last_error(pkg) == "unsupported bit depth: 8"
    assert L.lacx_stats_combine(None, 0, 1, 24, 96000, C.byref(out)) == lx.OK
    assert (out.frames, out.blocks, out.channels, out.bit_depth, out.sample_rate) == (0, 0, 1, 24, 96000)
    with pytest.raises(ValueError, match="unsupported channel count"):
        lx.stats_combine([], 0, 16)


def test_whole_call_arguments(pkg, dec):
    L, lx = pkg.lacx.lib(), pkg.lacx
    lac = _fixture("small/n257_st16_ms.lac")
    buf = (C.c_uint8 * len(lac)).from_buffer_copy(lac)
    spans = (lx.Span * 1)(lx.Span(C.cast(buf, C.POINTER(C.c_uint8)), len(lac)))
    srcs = (lx.DigestSource * 1)(lx.DigestSource(lx.Pcm(FAKE, FAKE, lx.PCM_PLANAR_I32, 2), 257, 48000, 16))
    calls = {
        "stats": lambda d, a, n: L.lacx_decoder_stats_batch_device(d, a and spans, n, None, None, None, None),
        "stats_pcm": lambda d, a, n: L.lacx_decoder_stats_pcm_batch_device(d, a and srcs, n, 0, None, None, None, None),
    }
    for name, call in calls.items():
        assert call(dec, True, 0) == lx.E_INVALID and _last_error(pkg) == "null argument or empty batch", name
        assert call(dec, None, 1) == lx.E_INVALID and _last_error(pkg) == "null argument or empty batch", name
        assert call(None, True, 1) == lx.E_INVALID and _last_error(pkg) == "null decoder", name
    for grid in (1, 255, 16385, 1 << 31):
        assert L.lacx_decoder_stats_pcm_batch_device(dec, srcs, 1, grid, None, None, None, None) == lx.E_INVALID
        assert _last_error(pkg) == "block_frames must be 0 or 256..16384"
    rows, count = C.POINTER(lx.BlockStats)(), C.c_uint32(5)
    assert L.lacx_decoder_item_block_stats(dec, 0, C.byref(rows), C.byref(count)) == lx.E_INVALID and count.value == 0
    assert _last_error(pkg) == "no such item in the last stats call"
    assert L.lacx_decoder_item_block_stats(dec, 0, None, C.byref(count)) == lx.E_INVALID and _last_error(pkg) == "null argument"
    d = lx.Decoder()
    for call in (lambda: d.stats_batch([]), lambda: d.stats_pcm_batch([]),
                 lambda: d.stats_pcm_batch([((FAKE, FAKE, 0, 2, 257), 48000, 16)], block_frames=255),
                 lambda: d.stats_pcm_batch([((FAKE, FAKE, 0, 2, 257), 48000, 16)], block_frames=16385)):
        with pytest.raises(ValueError):
            call()
    d.close()


def test_item_checks_before_the_device(pkg, dec):
    """The container is judged per item on the host, leniently: a refused one keeps the strict code and text and a zeroed
    result; without a device the items that pass carry LACX_E_DEVICE and the call returns it.  (With a device only items
    that fail on the host are in the batch, so that nothing runs on it.)"""
    L, lx = pkg.lacx.lib(), pkg.lacx
    have_device = lx.device_count() > 0
    st16 = _fixture("small/n257_st16_ms.lac")
    cases = [(b"XX" + st16[2:], lx.E_INVALID, "[decode-error] invalid frame header"), (st16[:12], lx.E_INVALID, None)]
    if not have_device:
        cases += [(st16, lx.E_DEVICE, "no usable HIP device"), (st16[:-1], lx.E_DEVICE, "no usable HIP device")]  # (a truncated file is no refusal)
    n = len(cases)
    keep = [(C.c_uint8 * len(x)).from_buffer_copy(x) for x, _, _ in cases]
    spans = (lx.Span * n)(*[lx.Span(C.cast(b, C.POINTER(C.c_uint8)), len(b)) for b in keep])
    rcs = (C.c_int * n)(*([-1] * n))
    out = (lx.Stats * n)()
    for o in out:
        o.frames, o.blocks = 9, 9
    ms = C.c_float(5.0)
    rc = L.lacx_decoder_stats_batch_device(dec, spans, n, None, rcs, out, C.byref(ms))
    assert ms.value == 0.0
    whole = _last_error(pkg)
    for i, (x, code, msg) in enumerate(cases):
        text = L.lacx_decoder_item_error(dec, i).decode()
        assert rcs[i] == code and (text == msg if msg else text.startswith("[decode-error] ")), (i, text)
        assert bytes(out[i]) == bytes(192), i
        if code == lx.E_INVALID:  # the strict parser's own code and text
            assert L.lacx_stream_parse(keep[i], len(x), C.byref(lx.StreamInfo())) == code and _last_error(pkg) == text
        rows, count = C.POINTER(lx.BlockStats)(), C.c_uint32(5)
        assert L.lacx_decoder_item_block_stats(dec, i, C.byref(rows), C.byref(count)) == lx.OK and count.value == 0
    if have_device:
        assert rc == lx.E_INVALID and whole == "stream 0: [decode-error] invalid frame header"
    else:
        assert rc == lx.E_DEVICE and whole == "no usable HIP device"
    d = lx.Decoder()
    if have_device:
        with pytest.raises(lx.BatchDecodeError) as e:
            d.stats_batch([cases[0][0]])
        assert e.value.errors == {0: cases[0][2]} and e.value.results == [None]
        with pytest.raises(RuntimeError, match=r"^\[decode-error\] invalid frame header$"):
            d.stats(cases[0][0])
    else:
        with pytest.raises(RuntimeError, match="no usable HIP device"):
            d.stats(st16)
    d.close()


def test_source_checks_are_the_digest_forms(pkg, dec):
    """stats_pcm judges every item as lacx_decoder_digest_pcm_blocks_batch_device does: the same texts, a zeroed result, no rows."""
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
    rc = L.lacx_decoder_digest_pcm_blocks_batch_device(dec, items, n, 1000, None, rcs, None, None)
    texts = [L.lacx_decoder_item_error(dec, i).decode() for i in range(n)]
    assert all(rcs[i] == lx.E_INVALID and texts[i] for i in range(n)) and len(set(texts)) == n
    rcs = (C.c_int * n)(*([-1] * n))
    out = (lx.Stats * n)()
    for o in out:
        o.frames = 9
    rc2 = L.lacx_decoder_stats_pcm_batch_device(dec, items, n, 1000, None, rcs, out, None)
    for i in range(n):
        assert rcs[i] == lx.E_INVALID and L.lacx_decoder_item_error(dec, i).decode() == texts[i], i
        assert bytes(out[i]) == bytes(192), i
        rows, count = C.POINTER(lx.BlockStats)(), C.c_uint32(5)
        assert L.lacx_decoder_item_block_stats(dec, i, C.byref(rows), C.byref(count)) == lx.OK and count.value == 0
    assert rc == rc2 == (lx.E_INVALID if have_device else lx.E_DEVICE)
