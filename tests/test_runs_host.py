"""The run finder's entry points without a device: the new structs against the library's own sizeof, the stitching of
csrc/runs_rows.h on fabricated rows against the Python restatement, every host check and its text, what a call does for its
items before any device work, the helpers' conversions, and the split / trim interval arithmetic as pure Python."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import __graft_entry__ as ge
import runstwin as rw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NEW = ("lacx_decoder_runs_batch_device", "lacx_decoder_runs_pcm_batch_device", "lacx_decoder_item_runs")
FAKE = 1 << 40  # a "device address" that is never dereferenced: every call here stops before the device
CHECKS = (((0, 9), "detectors outside the call's array"), ((8, 1), "detectors outside the call's array"), ((0xFFFFFFFF, 2), "detectors outside the call's array"),
          ((0, 0), "item has no detectors"))


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
    for name, cls, size in (("run_detector", lx.RunDetector, 16), ("run_query", lx.RunQuery, 8), ("run", lx.Run, 16), ("run_totals", lx.RunTotals, 32),
                            ("runs_result", lx.RunsResult, 296)):
        assert structs[name] is cls and L.lacx_sizeof(name.encode()) == C.sizeof(cls) == size, name
    assert (rw.DET_T.itemsize, rw.QUERY_T.itemsize, rw.RUN_T.itemsize, rw.TOT_T.itemsize, rw.RES_T.itemsize) == (16, 8, 16, 32, 296)
    d, r, t = lx.RunDetector, lx.RunsResult, lx.RunTotals
    assert (d.kind.offset, d.channel.offset, d.level.offset, d.min_frames.offset) == (0, 1, 4, 8)
    assert (r.frames.offset, r.lost_frames.offset, r.sample_rate.offset, r.blocks.offset, r.lost_blocks.offset, r.flags.offset, r.channels.offset,
            r.bit_depth.offset, r.detectors.offset, r.det.offset) == (0, 8, 16, 20, 24, 28, 32, 33, 34, 40)
    assert (t.runs.offset, t.frames.offset, t.longest.offset, t.longest_start.offset) == (0, 8, 16, 24)
    for name, value in (("LACX_RUN_QUIET", lx.RUN_QUIET), ("LACX_RUN_PEAK", lx.RUN_PEAK), ("LACX_RUN_FLAT", lx.RUN_FLAT), ("LACX_RUN_ALL", lx.RUN_ALL),
                        ("LACX_MAX_DETECTORS", lx.MAX_DETECTORS), ("LACX_RUNS_RERUN", lx.RUNS_RERUN)):
        assert re.search(rf"#define {name}\s+{value}u", header), name
    assert (rw.QUIET, rw.PEAK, rw.FLAT, rw.ALL, rw.RERUN) == (lx.RUN_QUIET, lx.RUN_PEAK, lx.RUN_FLAT, lx.RUN_ALL, lx.RUNS_RERUN)


# ---- stitching ----------------------------------------------------------------------------------------------------------
def _mask(frames, stretches):
    m = np.zeros(frames, bool)
    for s, n in stretches:
        m[s:s + n] = True
    return m


def _edge_runs(mask, min_frames):
    """The runs of a mask that touch a tile edge (what the rows must give): the others are the kernel's."""
    return [(s, n) for s, n in rw.runs_of(mask, min_frames) if s % rw.TILE == 0 or (s + n) % rw.TILE == 0 or s // rw.TILE != (s + n - 1) // rw.TILE]


STITCH = {
    "all-set tiles in front": (5 * 1024 + 3, [(0, 2048 + 17)]),
    "all-set tiles in the middle": (6 * 1024, [(1000, 24 + 3 * 1024 + 5)]),
    "all-set tiles at the end": (4 * 1024 + 100, [(2000, 48 + 2 * 1024 + 100)]),
    "all-set to a full last tile": (4 * 1024, [(1500, 4096 - 1500)]),
    "the whole item": (3 * 1024 + 1, [(0, 3 * 1024 + 1)]),
    "the whole item, one partial tile": (7, [(0, 7)]),
    "lead and trail of one tile are two runs": (3 * 1024, [(1000, 24 + 10), (2048 - 10, 10 + 20)]),
    "a run ends at a tile's last frame": (3 * 1024, [(1000, 24), (2048, 5)]),
    "lead alone, trail alone": (2 * 1024 + 9, [(0, 3), (1020, 4), (2048, 9)]),
}


@pytest.mark.parametrize("name", sorted(STITCH))
def test_stitching_of_fabricated_rows(name):
    frames, stretches = STITCH[name]
    mask = _mask(frames, stretches)
    for min_frames in (1, 5, 34, 2049, 3 * 1024 + 29, 1 << 40):
        assert rw.stitch(frames, rw.rows_of_mask(mask), min_frames) == _edge_runs(mask, min_frames), (name, min_frames)


def test_a_run_of_exactly_min_frames_over_three_tiles():
    """1024 + 2 frames from a tile's last frame to the first of the tile after the next: min_frames at, and one above, its length."""
    frames = 4 * 1024
    mask = _mask(frames, [(1023, 1026)])
    rows = rw.rows_of_mask(mask)
    assert rows == [(0, 1), (1024, 1024), (1, 0), (0, 0)]
    assert rw.stitch(frames, rows, 1026) == [(1023, 1026)] and rw.stitch(frames, rows, 1027) == []


def test_list_reservation_is_the_exact_bound():
    L = rw.lib()
    for frames in (1, 2, 3, 4, 5, 1023, 1024, 1025, 2049):
        for m in (1, 2, 3, 5, 1024, frames, frames + 1, (1 << 64) - 1):
            most = 0  # the most runs of >= m frames with a frame between them: k * m + (k - 1) <= frames
            while (most + 1) * m + most <= frames:
                most += 1
            assert L.sim_runs_reserve(C.c_uint64(frames), C.c_uint64(m), C.c_uint64(1 << 62)) == most == (frames + 1) // (m + 1), (frames, m)
            assert L.sim_runs_reserve(C.c_uint64(frames), C.c_uint64(m), C.c_uint64(3)) == min(most, 3)


# ---- host checks ------------------------------------------------------------------------------------------------------------
def test_detector_checks_and_their_texts():
    good = [rw.Det(rw.QUIET, rw.ALL, 5, 1)] * 8
    assert rw.check_text((0, 8), good) == "" and rw.check_text((7, 1), good) == "" and rw.check_text((8, 0), good) == "item has no detectors"
    for query, text in CHECKS:
        assert rw.check_text(query, good) == text, query
    assert rw.check_text((0, 9), good * 2) == "too many detectors"
    for det, text in ((rw.Det(3, 0, 0, 1), "unknown detector kind"), (rw.Det(rw.QUIET, 2, 0, 1), "unknown detector channel"),
                      (rw.Det(rw.PEAK, 254, 0, 1), "unknown detector channel"), (rw.Det(rw.QUIET, 0, 0, 0), "detector needs min_frames >= 1"),
                      (rw.Det(rw.FLAT, rw.ALL, 1, 1), "flat detector takes no level")):
        assert rw.check_text((1, 2), [good[0], good[0], det]) == text
        assert rw.check_text((0, 2), [good[0], good[0], det]) == ""  # (outside the item's detectors: not looked at)
    assert rw.check_text((0, 3), [rw.Det(rw.FLAT, 0, 0, 1), rw.Det(rw.QUIET, 1, 0xFFFFFFFF, (1 << 64) - 1), rw.Det(rw.PEAK, rw.ALL, 0, 1)]) == ""


def _call_args(lx, lac):
    buf = (C.c_uint8 * len(lac)).from_buffer_copy(lac)
    spans = (lx.Span * 1)(lx.Span(C.cast(buf, C.POINTER(C.c_uint8)), len(lac)))
    srcs = (lx.DigestSource * 1)(lx.DigestSource(lx.Pcm(FAKE, FAKE, lx.PCM_PLANAR_I32, 2), 257, 48000, 16))
    dets = (lx.RunDetector * 1)(lx.RunDetector(lx.RUN_QUIET, lx.RUN_ALL, (C.c_uint8 * 2)(), 0, 1))
    queries = (lx.RunQuery * 1)(lx.RunQuery(0, 1))
    return buf, spans, srcs, dets, queries


def test_whole_call_arguments(pkg, dec):
    L, lx = pkg.lacx.lib(), pkg.lacx
    _keep, spans, srcs, dets, queries = _call_args(lx, _fixture("small/n257_st16_ms.lac"))
    calls = {
        "runs": lambda d, a, q, n, dt, nd: L.lacx_decoder_runs_batch_device(d, a and spans, q and queries, n, dt and dets, nd, None, None, None, None),
        "runs_pcm": lambda d, a, q, n, dt, nd: L.lacx_decoder_runs_pcm_batch_device(d, a and srcs, q and queries, n, dt and dets, nd, None, None, None, None),
    }
    for name, call in calls.items():
        assert call(dec, True, True, 0, True, 1) == lx.E_INVALID and _last_error(pkg) == "null argument or empty batch", name
        assert call(dec, None, True, 1, True, 1) == lx.E_INVALID and _last_error(pkg) == "null argument or empty batch", name
        assert call(dec, True, None, 1, True, 1) == lx.E_INVALID and _last_error(pkg) == "null argument or empty batch", name
        assert call(None, True, True, 1, True, 1) == lx.E_INVALID and _last_error(pkg) == "null decoder", name
        assert call(dec, True, True, 1, None, 1) == lx.E_INVALID and _last_error(pkg) == "no detectors", name
        assert call(dec, True, True, 1, True, 0) == lx.E_INVALID and _last_error(pkg) == "no detectors", name
    runs, count = C.POINTER(lx.Run)(), C.c_uint64(5)
    assert L.lacx_decoder_item_runs(dec, 0, 0, C.byref(runs), C.byref(count)) == lx.E_INVALID and count.value == 0
    assert _last_error(pkg) == "no such item in the last runs call"
    assert L.lacx_decoder_item_runs(dec, 0, 0, None, C.byref(count)) == lx.E_INVALID and _last_error(pkg) == "null argument"
    d = lx.Decoder()
    for call in (lambda: d.runs_batch([], [lx.quiet()]), lambda: d.runs_pcm_batch([], [lx.quiet()]), lambda: d.runs_batch([b"x"], [])):
        with pytest.raises(ValueError):
            call()
    d.close()


def test_item_checks_before_the_device(pkg, dec):
    """Container and detectors are judged per item on the host: a refused container keeps the strict code and text, refused
    detectors their text, both a zeroed result and no runs; without a device the items that pass carry LACX_E_DEVICE and
    the call returns it.  (With a device only items that fail on the host are in the batch, so that nothing runs on it.)"""
    L, lx = pkg.lacx.lib(), pkg.lacx
    have_device = lx.device_count() > 0
    st16 = _fixture("small/n257_st16_ms.lac")
    D = lambda kind, ch, level, m: lx.RunDetector(kind, ch, (C.c_uint8 * 2)(), level, m)  # noqa: E731
    dets = [D(0, 255, 0, 1), D(3, 0, 0, 1), D(0, 2, 0, 1), D(0, 0, 0, 0), D(2, 0, 7, 1)] + [D(1, 1, 9, 2)] * 9
    # (stream, query, code, text)
    cases = [(b"XX" + st16[2:], (0, 1), lx.E_INVALID, "[decode-error] invalid frame header"), (st16[:12], (0, 1), lx.E_INVALID, None),
             (st16, (1, 1), lx.E_INVALID, "unknown detector kind"), (st16, (2, 1), lx.E_INVALID, "unknown detector channel"),
             (st16, (3, 1), lx.E_INVALID, "detector needs min_frames >= 1"), (st16, (4, 2), lx.E_INVALID, "flat detector takes no level"),
             (st16, (5, 9), lx.E_INVALID, "too many detectors"), (st16, (5, 0), lx.E_INVALID, "item has no detectors"),
             (st16, (13, 2), lx.E_INVALID, "detectors outside the call's array"), (st16, (15, 0), lx.E_INVALID, "detectors outside the call's array")]
    if not have_device:
        cases += [(st16, (0, 1), lx.E_DEVICE, "no usable HIP device"), (st16[:-1], (5, 8), lx.E_DEVICE, "no usable HIP device")]
    n = len(cases)
    keep = [(C.c_uint8 * len(x[0])).from_buffer_copy(x[0]) for x in cases]
    spans = (lx.Span * n)(*[lx.Span(C.cast(b, C.POINTER(C.c_uint8)), len(b)) for b in keep])
    queries = (lx.RunQuery * n)(*[lx.RunQuery(*x[1]) for x in cases])
    darr = (lx.RunDetector * len(dets))(*dets)
    rcs = (C.c_int * n)(*([-1] * n))
    out = (lx.RunsResult * n)()
    for o in out:
        o.frames, o.blocks = 9, 9
    ms = C.c_float(5.0)
    rc = L.lacx_decoder_runs_batch_device(dec, spans, queries, n, darr, len(dets), None, rcs, out, C.byref(ms))
    assert ms.value == 0.0
    whole = _last_error(pkg)
    for i, (x, _q, code, msg) in enumerate(cases):
        text = L.lacx_decoder_item_error(dec, i).decode()
        assert rcs[i] == code and (text == msg if msg else text.startswith("[decode-error] ")), (i, text)
        assert bytes(out[i]) == bytes(296), i
        runs, count = C.POINTER(lx.Run)(), C.c_uint64(5)
        assert L.lacx_decoder_item_runs(dec, i, 0, C.byref(runs), C.byref(count)) == lx.E_INVALID and count.value == 0
        assert _last_error(pkg) == "no such detector of that item in the last runs call"
    if have_device:
        assert rc == lx.E_INVALID and whole == "stream 0: [decode-error] invalid frame header"
    else:
        assert rc == lx.E_DEVICE and whole == "no usable HIP device"
    d = lx.Decoder()
    if have_device:
        with pytest.raises(lx.BatchDecodeError) as e:
            d.runs_batch([cases[0][0], st16], [[lx.quiet()], [lx.RunDetector(2, 0, (C.c_uint8 * 2)(), 1, 1)]])
        assert e.value.errors == {0: cases[0][3], 1: "flat detector takes no level"} and e.value.results == [None, None]
        with pytest.raises(RuntimeError, match=r"^\[decode-error\] invalid frame header$"):
            d.runs(cases[0][0], [lx.quiet()])
    else:
        with pytest.raises(RuntimeError, match="no usable HIP device"):
            d.runs(st16, [lx.quiet()])
    d.close()


def test_source_checks_are_the_digest_forms(pkg, dec):
    """runs_pcm judges every item as lacx_decoder_digest_pcm_batch_device does -- the same texts, a zeroed result, no runs --
    and then its detectors."""
    L, lx = pkg.lacx.lib(), pkg.lacx
    have_device = lx.device_count() > 0
    P = lx.PCM_PLANAR_I32
    cases = [(None, FAKE, P, 2, 257, 48000, 16), (FAKE, FAKE, 3, 2, 257, 48000, 16), (FAKE, FAKE, P, 3, 257, 48000, 16), (FAKE, FAKE, P, 2, 0, 48000, 16),
             (FAKE, FAKE, P, 2, 1 << 56, 48000, 16), (FAKE, FAKE, P, 2, 257, 22050, 16), (FAKE, FAKE, P, 2, 257, 48000, 8),
             (FAKE + 2, FAKE, P, 2, 257, 48000, 16), (FAKE, None, lx.PCM_INTERLEAVED_I24, 2, 257, 48000, 16)]
    n = len(cases)
    items = (lx.DigestSource * (n + 1))()
    for k, (d0, d1, layout, ch, frames, rate, depth) in enumerate(cases):
        items[k] = lx.DigestSource(lx.Pcm(d0, d1, layout, ch), frames, rate, depth)
    items[n] = lx.DigestSource(lx.Pcm(FAKE, FAKE, P, 2), 257, 48000, 16)  # a good source with refused detectors
    rcs = (C.c_int * n)(*([-1] * n))
    rc = L.lacx_decoder_digest_pcm_batch_device(dec, items, n, None, rcs, None, None)
    texts = [L.lacx_decoder_item_error(dec, i).decode() for i in range(n)] + ["flat detector takes no level"]
    assert all(rcs[i] == lx.E_INVALID and texts[i] for i in range(n)) and len(set(texts)) == n + 1
    dets = (lx.RunDetector * 2)(lx.RunDetector(0, 255, (C.c_uint8 * 2)(), 0, 1), lx.RunDetector(2, 255, (C.c_uint8 * 2)(), 3, 1))
    queries = (lx.RunQuery * (n + 1))(*([lx.RunQuery(0, 1)] * n + [lx.RunQuery(1, 1)]))
    rcs = (C.c_int * (n + 1))(*([-1] * (n + 1)))
    out = (lx.RunsResult * (n + 1))()
    for o in out:
        o.frames = 9
    rc2 = L.lacx_decoder_runs_pcm_batch_device(dec, items, queries, n + 1, dets, 2, None, rcs, out, None)
    for i in range(n + 1):
        assert rcs[i] == lx.E_INVALID and L.lacx_decoder_item_error(dec, i).decode() == texts[i], i
        assert bytes(out[i]) == bytes(296), i
    assert rc == rc2 == (lx.E_INVALID if have_device else lx.E_DEVICE)


# ---- the binding's helpers --------------------------------------------------------------------------------------------------
def test_helpers_convert_per_item(pkg):
    lx = pkg.lacx
    q = lx.quiet(dbfs=-60, seconds=0.1)
    for depth, rate, level, frames in ((16, 44100, 32, 4410), (24, 48000, 8388, 4800), (16, 96000, 32, 9600)):
        d = q.resolve(depth, rate)
        assert (d.kind, d.channel, d.level, d.min_frames) == (lx.RUN_QUIET, lx.RUN_ALL, level, frames)
        assert level == (1 << (depth - 1)) * 10 ** (-60 / 20) // 1
    assert [(lx.peak().resolve(b, 1).level, lx.peak().resolve(b, 1).kind) for b in (16, 24)] == [(32767, 1), (8388607, 1)]  # stats' full_scale
    assert lx.peak(dbfs=-6, channel="right", min_frames=3).resolve(16, 1).level == 16422 and lx.peak(level=9, channel="left").resolve(24, 1).channel == 0
    d = lx.flat(seconds=0.5, channel="right").resolve(16, 8000)
    assert (d.kind, d.channel, d.level, d.min_frames) == (lx.RUN_FLAT, 1, 0, 4000)
    assert lx.quiet().resolve(16, 1).min_frames == 1 and lx.quiet(seconds=1e-9).resolve(16, 44100).min_frames == 1 and lx.quiet().resolve(24, 1).level == 0
    for bad in (lambda: lx.quiet(level=1, dbfs=-3), lambda: lx.flat(min_frames=2, seconds=1.0), lambda: lx.quiet(channel="centre")):
        with pytest.raises((ValueError, KeyError)):
            bad()
    queries, dets, ndets, resolved = lx.Decoder._detector_tables([q, lx.peak()], 2, [(16, 44100), (24, 48000)])  # one list for all items
    assert ndets == 4 and [(x.first_detector, x.detectors) for x in queries] == [(0, 2), (2, 2)]
    assert [dets[k].level for k in range(4)] == [32, 32767, 8388, 8388607]
    queries, dets, ndets, resolved = lx.Decoder._detector_tables([[q], [lx.flat(), lx.peak()]], 2, [(16, 44100), None])  # one list per item
    assert ndets == 3 and [(x.first_detector, x.detectors) for x in queries] == [(0, 1), (1, 2)] and len(resolved[1]) == 2


# ---- split / trim: the interval arithmetic ------------------------------------------------------------------------------------
def test_sound_pieces_pad_merge_clip_and_all_silence(pkg):
    lx = pkg.lacx
    sp = lx.sound_pieces
    assert sp(100, []) == [(0, 100)] and sp(100, [(0, 100)]) == [] and sp(100, [(0, 100)], pad=7) == []
    assert sp(100, [(0, 10), (40, 20), (90, 10)]) == [(10, 30), (60, 30)]
    assert sp(100, [(0, 10), (40, 20), (90, 10)], pad=5) == [(5, 40), (55, 40)]
    assert sp(100, [(0, 10), (40, 20), (90, 10)], pad=10) == [(0, 100)]  # the pieces touch at 50: merged; clipped at both ends
    assert sp(100, [(0, 10), (40, 20), (90, 10)], pad=9) == [(1, 48), (51, 48)]
    assert sp(100, [(40, 20)], pad=1000) == [(0, 100)] and sp(100, [(10, 80)]) == [(0, 10), (90, 10)]
    rng = np.random.default_rng(5)
    for _ in range(200):
        frames = int(rng.integers(1, 400))
        mask = rng.random(frames) < rng.random()
        quiet_runs = rw.runs_of(mask, int(rng.integers(1, 6)))
        pad = int(rng.integers(0, 12))
        assert sp(frames, quiet_runs, pad) == rw.pieces_of(frames, quiet_runs, pad), (frames, quiet_runs, pad)
