"""The import pass and the tensor layouts without a device: import_quad of csrc/import_core.h on the host
(tests/native/sim_import.cpp), plain and under AddressSanitizer + UBSan, against numpy conversions; the float rule and the
exact error texts over a corpus of invalid values; the verify form's new layouts through csrc/verify_core.h
(tests/native/sim_verify_layouts.cpp) against the planar int32 source with the same alteration; lacx.pcm_of over numpy
arrays of every accepted and refused shape, dtype and stride; and the host-side source checks of the verify entry point."""
import ctypes as C
import os

import numpy as np
import pytest

import __graft_entry__ as ge
import importtwin as T
import vertwin as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FAKE = 1 << 40  # a "device address" that is never dereferenced: every call here stops before the device
UNIT = T.unit_frames()
FRAMES = (1, 2, 3, 15, 16, 17, 255, 257, 4095, 4097, 16383, 16384, 16385, 16421, UNIT - 1, UNIT, UNIT + 1)
FORMATS = ((T.PLANAR_I16, 16), (T.PLANAR_F32, 16), (T.PLANAR_F32, 24), (T.INTERLEAVED_F32, 16), (T.INTERLEAVED_F32, 24))


def _pcm(frames, channels, bit_depth, seed):
    rng = np.random.default_rng(seed)
    lo, hi = -(1 << (bit_depth - 1)), (1 << (bit_depth - 1)) - 1
    out = []
    for c in range(channels):
        x = rng.integers(lo, hi + 1, frames, dtype=np.int64)
        x[:min(frames, 4)] = ((lo, hi, -1, 0), (hi, lo, 0, 1))[c][:min(frames, 4)]  # the range's ends
        out.append(x)
    return out


def _elements(layout, samples, bit_depth):
    return [s.astype(np.int16) if layout == T.PLANAR_I16 else T.to_float(s, bit_depth) for s in samples]


def _grid_cases():
    cases, seed = [], 0
    for frames in FRAMES:
        for channels in (1, 2):
            for layout, depth in FORMATS:
                for offset in (0, 1, 2, 3):
                    seed += 1
                    cases.append(T.Case(layout, channels, depth, offset, *_elements(layout, _pcm(frames, channels, depth, seed), depth)))
    return cases


def _corpus_cases():
    """(case, description): one or two bad values planted into valid material."""
    out, seed = [], 5000
    frames = 2 * UNIT + 5
    positions = (0, frames - 1, UNIT - 1, UNIT, 255, 256)  # first, last, either side of a unit border and of a wave's
    for depth in (16, 24):
        for layout in (T.PLANAR_F32, T.INTERLEAVED_F32):
            values = T.invalid_values(depth)
            for vi, (val, kind) in enumerate(values):  # every value: at a rotating position, in a rotating channel
                seed += 1
                rows = _elements(layout, _pcm(frames, 2, depth, seed), depth)
                pos, ch = positions[vi % len(positions)], vi % 2
                rows[ch][pos] = val
                out.append((T.Case(layout, 2, depth, vi % 4, *rows), (depth, ch, pos, kind)))
            bad = np.float32(0.3)  # off the grid at either depth
            for pos in positions:  # every position, mono
                seed += 1
                rows = _elements(layout, _pcm(frames, 1, depth, seed), depth)
                rows[0][pos] = bad
                out.append((T.Case(layout, 1, depth, 1, *rows), (depth, 0, pos, 2)))
            # which channel: right only, both (left wins, though its index is higher), two in one channel (lowest wins),
            # a range error in front of an inexact one and the reverse
            for plant, want in ((((1, 700, bad),), (1, 700, 2)),
                                (((1, 3, bad), (0, 900, np.float32(1.0))), (0, 900, 1)),
                                (((0, UNIT + 1, bad), (0, UNIT - 2, np.float32(2.0))), (0, UNIT - 2, 1)),
                                (((1, UNIT, np.float32(1.0)), (1, UNIT - 1, bad)), (1, UNIT - 1, 2))):
                seed += 1
                rows = _elements(layout, _pcm(frames, 2, depth, seed), depth)
                for ch, pos, val in plant:
                    rows[ch][pos] = val
                out.append((T.Case(layout, 2, depth, 2, *rows), (depth,) + want))
    return out


@pytest.fixture(scope="module")
def grid():
    return _grid_cases()


@pytest.fixture(scope="module")
def corpus():
    return _corpus_cases()


def _message(depth, ch, pos, kind):
    what = "is outside the configured PCM bit depth" if kind == 1 else f"is not an exact {depth}-bit PCM value"
    return f"{'right' if ch else 'left'} sample at index {pos} {what}"


def test_float_rule_value_by_value():
    """f32_to_pcm against the rule worked in float64, and the documented value of an invalid float."""
    for depth in (16, 24):
        for val, kind in T.invalid_values(depth):
            k, v = T.f32_to_pcm(val, depth)
            assert k == kind, (depth, val, k, kind)
            if np.isnan(val):
                assert v == -(1 << 31)
            else:  # rounded to nearest (ties to even) and saturated to int32
                p = float(val) * 2.0 ** (depth - 1)
                assert v == int(np.clip(np.rint(p), -(1 << 31), (1 << 31) - 1)), (depth, val)
        rng = np.random.default_rng(depth)
        bits = rng.integers(0, 1 << 32, 4000, dtype=np.uint64).astype(np.uint32)
        kinds, values = T.classify(bits.view(np.float32), depth)
        for b, k, v in zip(bits.view(np.float32), kinds, values):
            got = T.f32_to_pcm(b, depth)
            assert got[0] == k and (k != 0 or got[1] == v), (depth, b)
    assert T.f32_to_pcm(np.float32(0.5) * np.float32(2.0 ** -15), 16) == (2, 0)      # a tie: to even
    assert T.f32_to_pcm(np.float32(1.5) * np.float32(2.0 ** -15), 16) == (2, 2)
    assert T.f32_to_pcm(np.float32(-2.5) * np.float32(2.0 ** -23), 24) == (2, -2)


def test_the_expectations_see_what_the_cases_intend(grid, corpus):
    assert len(grid) == len(FRAMES) * 2 * len(FORMATS) * 4
    assert all(c.expected().code == 0 for c in grid[::7])
    odd_i16 = [c for c in grid if c.layout == T.PLANAR_I16 and c.channels == 2 and c.frames % 2 == 1]
    assert len(odd_i16) >= 20  # the right row of such a tensor is 2-byte aligned only
    for case, (depth, ch, pos, kind) in corpus:
        e = case.expected()
        assert (e.code, e.message) == ((1, _message(depth, ch, pos, kind)) if kind else (0, "")), (depth, ch, pos, kind)
    assert sum(1 for _, w in corpus if w[3] == 0) >= 12 and sum(1 for _, w in corpus if w[3] == 1) >= 20


def test_twin_against_numpy(grid):
    got = T.run_plain(grid)
    wrong = [(i, c.layout, c.channels, c.bit_depth, c.offset, c.frames) for i, (c, g) in enumerate(zip(grid, got)) if g != c.expected()]
    assert not wrong, wrong[:5]


def test_alias_rule(grid):
    """Mono planar int16 on a 4-byte aligned address is interleaved int16 mono: no import, and nothing else is an alias."""
    got = T.run_plain(grid)
    seen = 0
    for case, g in zip(grid, got):
        want = case.layout == T.PLANAR_I16 and case.channels == 1 and case.offset % 2 == 0
        assert g.alias == int(want)
        if want:
            seen += 1
            assert g.dst == case.left.astype("<i2").tobytes()  # the source's own bytes are what the kernels read
    assert seen == 2 * len(FRAMES)


def test_invalid_values_give_the_exact_code_and_message(corpus):
    got = T.run_plain([c for c, _ in corpus])
    for (case, (depth, ch, pos, kind)), g in zip(corpus, got):
        assert (g.code, g.message) == ((1, _message(depth, ch, pos, kind)) if kind else (0, "")), (depth, ch, pos, kind)
        assert g == case.expected()  # the destination too: an invalid value is stored as 0


def test_sanitized_twin_reports_nothing(grid, corpus):
    exe, why = T.sanitized_exe()
    if exe is None:
        pytest.skip(why)
    cases = grid + [c for c, _ in corpus]
    answers, rc, err = T.run_sanitized(cases, exe)
    assert rc == 0, err
    assert answers == [c.expected() for c in cases]


# ---- the verify form over the tensor layouts ---------------------------------------------------------------------------

def _source(layout, samples, depth, offset):
    """The source arrays of one item in `layout`, `offset` elements behind a 16-byte aligned address: (src0, src1)."""
    if layout == T.PLANAR_I32:
        rows = [np.asarray(s, dtype=np.int32) for s in samples]
    else:
        rows = _elements(layout, samples, depth)
    if layout == T.INTERLEAVED_F32:
        flat = np.stack(rows, axis=1).reshape(-1)
        a = T.aligned(flat.size, flat.dtype, offset)
        a[:] = flat
        return a, None
    dt = rows[0].dtype
    per16 = 16 // dt.itemsize
    outs = []
    for c, r in enumerate(rows):  # the second row where it would lie in a [2, frames] tensor
        a = T.aligned(r.size, dt, (offset + c * r.size) % per16)
        a[:] = r
        outs.append(a)
    return outs[0], outs[1] if len(outs) > 1 else None


def _verify(layout, channels, depth, block_frames, ms, samples, offset, edits=(), raw=()):
    """edits: (frame, channel, sample value); raw: (frame, channel, float32 value) written into a float source as it is."""
    frames = sum(block_frames)
    src = [s.copy() for s in samples]
    for f, c, v in edits:
        src[c][f] = v
    s0, s1 = _source(layout, src, depth, offset)
    for f, c, v in raw:
        if layout == T.INTERLEAVED_F32:
            s0[f * channels + c] = v
        else:
            (s1 if c else s0)[f] = v
    sl, sr = V.to_scratch(samples[0], samples[1] if channels == 2 else None, block_frames, ms)
    return T.verify_layout(channels, depth, layout, block_frames, ms, [0] * len(block_frames), sl, sr, s0, s1)


@pytest.mark.parametrize("frames", (1, 3, 4, 5, 257, 258, 1029))
def test_verify_layouts_match_the_planar_source(frames):
    seed = frames
    for channels in (1, 2):
        for layout, depth in FORMATS:
            tables = [([frames], [0])]
            if channels == 2:
                tables.append(([frames], [1]))
            if frames > 257:
                tables.append(([257, frames - 257], [0, 1] if channels == 2 else [0, 0]))
            for block_frames, ms in tables:
                seed += 1
                samples = _pcm(frames, channels, depth, seed)
                last, c1 = frames - 1, channels - 1
                other = lambda v: int(v) - 1 if int(v) > 0 else int(v) + 1
                places = [(0, 0), (last, c1), (frames // 2, 0)]
                if len(block_frames) == 2:
                    places += [(256, c1), (257, 0)]  # either side of the block border; frame 256 closes a unit of four too
                for offset in (0, 1, 2, 3):
                    clean = _verify(layout, channels, depth, block_frames, ms, samples, offset)
                    assert clean == T.VerifyLine(0, T.NO_KEY, 0, 0, 0, (0,) * len(block_frames)), (layout, depth, offset)
                for k, (f, c) in enumerate(places):
                    edit = [(f, c, other(samples[c][f]))]
                    want = _verify(T.PLANAR_I32, channels, depth, block_frames, ms, samples, 0, edit)
                    got = _verify(layout, channels, depth, block_frames, ms, samples, k % 4, edit)
                    assert got == want and got.mismatches == 1 and got.key == 2 * f + c, (layout, depth, f, c)


def test_verify_invalid_float_counts_and_reports_the_documented_value():
    frames, depth = 300, 16
    samples = _pcm(frames, 2, depth, 77)
    samples[1][41] = 100  # what the stream decodes to there
    for layout in (T.PLANAR_F32, T.INTERLEAVED_F32):
        for val, source in ((np.float32(100.4 / 32768), 100),     # rounds to the decoded value and still differs
                            (np.float32(np.nan), -(1 << 31)), (np.float32(np.inf), (1 << 31) - 1),
                            (np.float32(-np.inf), -(1 << 31)), (np.float32(1.0), 32768), (np.float32(-3e38), -(1 << 31))):
            got = _verify(layout, 2, depth, [257, 43], [1, 0], samples, 1, raw=[(41, 1, val)])
            assert got == T.VerifyLine(1, 2 * 41 + 1, 100, source, 0, (0, 0)), (layout, val, got)
        # in the partial last unit, and two of them: the lower is reported
        got = _verify(layout, 2, depth, [257, 43], [0, 1], samples, 3, raw=[(299, 0, np.float32(np.nan)), (298, 1, np.float32(0.3))])
        assert got[:2] == (2, 2 * 298 + 1) and got.block == 1 and got.source == int(np.rint(0.3 * 32768))


# ---- pcm_of ------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def pkg():
    mod = ge.load_pkg()
    if not os.path.exists(mod.lacx.LIB_PATH):
        mod.lacx.build()
    return mod


def _desc(pcm):
    return (pcm.data0, pcm.data1, pcm.layout, pcm.channels)


def test_pcm_of_accepts(pkg):
    lx = pkg.lacx
    for dt, planar, depth in ((np.int32, lx.PCM_PLANAR_I32, 24), (np.int16, lx.PCM_PLANAR_I16, 16), (np.float32, lx.PCM_PLANAR_F32, 24)):
        size = np.dtype(dt).itemsize
        a = np.zeros((2, 101), dtype=dt)
        assert (_desc(lx.pcm_of(a, depth)[0]), lx.pcm_of(a, depth)[1]) == ((a.ctypes.data, a.ctypes.data + 101 * size, planar, 2), 101)
        wide = np.zeros((2, 300), dtype=dt)
        crop = wide[:, 7:108]  # a slice of a wider tensor: rows stay contiguous, the row stride is the wide one
        assert _desc(lx.pcm_of(crop, depth)[0]) == (crop.ctypes.data, crop.ctypes.data + 300 * size, planar, 2)
        assert _desc(lx.pcm_of(a[:1], depth)[0]) == (a.ctypes.data, None, planar, 1)       # [1, T]
        assert _desc(lx.pcm_of(a[1], depth)[0]) == (a[1].ctypes.data, None, planar, 1)     # [T]
        assert lx.pcm_of(a[1], depth)[1] == 101
        col = np.zeros((55, 1), dtype=dt)
        assert (_desc(lx.pcm_of(col, depth)[0]), lx.pcm_of(col, depth)[1]) == ((col.ctypes.data, None, planar, 1), 55)
        one = np.zeros((2, 1), dtype=dt)  # one frame: [channels, frames]
        assert lx.pcm_of(one, depth)[1] == 1 and lx.pcm_of(one, depth)[0].channels == 2
    f = np.zeros((77, 2), dtype=np.float32)
    assert (_desc(lx.pcm_of(f, 16)[0]), lx.pcm_of(f, 16)[1]) == ((f.ctypes.data, None, lx.PCM_INTERLEAVED_F32, 2), 77)
    h = np.zeros((77, 2), dtype=np.int16)
    assert _desc(lx.pcm_of(h, 16)[0]) == (h.ctypes.data, None, lx.PCM_INTERLEAVED_I16, 2)
    assert (lx.PCM_PLANAR_I16, lx.PCM_PLANAR_F32, lx.PCM_INTERLEAVED_F32) == (16, 17, 18)

    class Tensor:  # the duck type: a torch tensor's four members, strides in elements
        def __init__(self, a):
            self._a, self.dtype, self.shape = a, "torch." + a.dtype.name, a.shape
        def data_ptr(self):
            return self._a.ctypes.data
        def stride(self):
            return tuple(s // self._a.itemsize for s in self._a.strides)
    crop = np.zeros((2, 300), dtype=np.float32)[:, 8:200]
    assert _desc(lx.pcm_of(Tensor(crop), 24)[0]) == _desc(lx.pcm_of(crop, 24)[0])


def test_pcm_of_refuses(pkg):
    lx = pkg.lacx
    z = np.zeros
    for bad, why in ((z((2, 9), np.float64), "dtype float64"), (z((2, 9), np.uint8), "dtype uint8"), (z((2, 9), np.int64), "dtype int64"),
                     (z((3, 9), np.float32).T, "more than two channels"), (z((9, 3), np.float32), "more than two channels"),
                     (z((4, 9), np.int16), "more than two channels"), (z((2, 18), np.float32)[:, ::2], "inner stride 2"),
                     (z(18, np.int32)[::2], "inner stride 2"), (z((9, 4), np.float32)[:, :2], "contiguous"),
                     (z((9, 2), np.int32), "interleaved int32"), (z((2, 3, 4), np.float32), "shape"), (z((2, 0), np.float32), "empty"),
                     (z(9, np.float32)[::-1], "strides"), ([0.0, 0.5], "list"), (z((9, 5), np.float32), "more than two channels")):
        with pytest.raises(ValueError, match=why):
            lx.pcm_of(bad, 16)
    with pytest.raises(ValueError, match="bit depth 16"):
        lx.pcm_of(z((2, 9), np.int16), 24)
    enc = lx.Encoder(12, 0, 48000, 16)
    with pytest.raises(ValueError, match="describes itself"):
        enc.encode_shard_pcm_device_view(z((2, 9), np.float32), lx.PCM_PLANAR_F32)
    with pytest.raises(ValueError, match="raw device address"):
        enc.encode_shard_pcm_device_view(FAKE)


# ---- the host-side source checks of the verify entry point ---------------------------------------------------------------

def test_verify_source_checks_of_the_new_layouts(pkg):
    """The new messages through the device-less path; the call still fills per-item parse results without a device."""
    L, lx = pkg.lacx.lib(), pkg.lacx
    read = lambda name: open(os.path.join(GOLDEN, name), "rb").read()
    stereo, mono, deep = read("small/n257_st16_ms.lac"), read("small/n33_mono16.lac"), read("small/n16421_st24_lr.lac")
    I16, F32, IF32 = lx.PCM_PLANAR_I16, lx.PCM_PLANAR_F32, lx.PCM_INTERLEAVED_F32
    have_device = lx.device_count() > 0
    ok = "source arrays missing" if have_device else None  # with a device the good items get no arrays: nothing runs on it
    good = None if have_device else FAKE
    cases = [  # (stream, data0, data1, layout, channels, frames, message)
        (stereo, good, FAKE + 2, I16, 2, 257, ok),             # 2-byte aligned rows
        (stereo, good, FAKE, F32, 2, 257, ok),
        (stereo, good, None, IF32, 2, 257, ok),
        (mono, None if have_device else FAKE + 2, None, I16, 1, 33, ok),
        (deep, good, FAKE + 4, F32, 2, 16421, ok),             # float32 serves both depths
        (deep, good, None, IF32, 2, 16421, ok),
        (deep, FAKE, FAKE, I16, 2, 16421, "source layout does not match the stream's bit depth"),
        (stereo, FAKE + 1, FAKE, I16, 2, 257, "source arrays are not 2-byte aligned"),
        (stereo, FAKE, FAKE + 3, I16, 2, 257, "source arrays are not 2-byte aligned"),
        (stereo, FAKE + 2, FAKE, F32, 2, 257, "source arrays are not 4-byte aligned"),
        (stereo, FAKE, FAKE + 2, F32, 2, 257, "source arrays are not 4-byte aligned"),
        (stereo, FAKE + 2, None, IF32, 2, 257, "source arrays are not 4-byte aligned"),
        (stereo, FAKE, None, F32, 2, 257, "source arrays missing"),
        (stereo, FAKE, None, I16, 2, 257, "source arrays missing"),
        (stereo, None, None, IF32, 2, 257, "source arrays missing"),
        (stereo, FAKE, FAKE, F32, 1, 257, "source channel count does not match the stream"),
        (stereo, FAKE, None, IF32, 2, 256, "source frame count does not match the stream"),
    ] + [(stereo, FAKE, FAKE, code, 2, 257, "unknown source layout") for code in (3, 15, 19, 0xFFFFFFFF)]
    n = len(cases)
    keep, items = [], (lx.VerifyItem * n)()
    for k, (lac, d0, d1, layout, ch, frames, _) in enumerate(cases):
        b = (C.c_uint8 * len(lac)).from_buffer_copy(lac)
        keep.append(b)
        items[k].lac, items[k].size, items[k].pcm, items[k].frames = C.cast(b, C.POINTER(C.c_uint8)), len(lac), lx.Pcm(d0, d1, layout, ch), frames
    h = C.c_void_p()
    assert L.lacx_decoder_create(C.c_int(-1), C.byref(h)) == lx.OK
    try:
        rcs = (C.c_int * n)(*([-1] * n))
        res = (lx.VerifyResult * n)()
        rc = L.lacx_decoder_verify_batch_device(h, items, n, None, rcs, res, None)
        for i, case in enumerate(cases):
            if case[6] is None:  # parses, source fine: only the missing device stops it
                assert rcs[i] == lx.E_DEVICE and L.lacx_decoder_item_error(h, i).decode() == "no usable HIP device", i
            else:
                assert rcs[i] == lx.E_INVALID and L.lacx_decoder_item_error(h, i).decode() == case[6], i
        assert rc == (lx.E_INVALID if have_device else lx.E_DEVICE)
    finally:
        L.lacx_decoder_destroy(h)
    header = open(os.path.join(ROOT, "include", "lacx.h")).read()
    for name, code in (("LACX_PCM_PLANAR_I16", 16), ("LACX_PCM_PLANAR_F32", 17), ("LACX_PCM_INTERLEAVED_F32", 18)):
        assert f"#define {name}" in header and f"{code}u" in header.split(f"#define {name}")[1].split("\n")[0]
