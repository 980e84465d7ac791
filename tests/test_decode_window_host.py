"""The frame-window decode entry points without a device: their symbols and struct, and the checks of every item's
stream, window and output arrays, which run on the host before any device call and give each item its own message."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import __graft_entry__ as ge

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NEW = ("lacx_decoder_decode_window_batch_device", "lacx_decoder_decode_window")


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


def test_symbols_and_struct(pkg):
    L, lx = pkg.lacx.lib(), pkg.lacx
    header = open(os.path.join(ROOT, "include", "lacx.h")).read()
    for name in NEW:
        assert hasattr(L, name) and name in lx.EXPORTS
        assert re.search(rf"\b{name}\s*\(", header), name
    assert "} lacx_window_item;" in header
    assert re.search(r"#define LACX_SAMPLE_I32 0\b", header) and re.search(r"#define LACX_SAMPLE_F32 1\b", header)
    assert (lx.SAMPLE_I32, lx.SAMPLE_F32) == (0, 1)
    assert lx.abi_structs()["window_item"] is lx.WindowItem
    assert L.lacx_sizeof(b"window_item") == C.sizeof(lx.WindowItem) == 48


def _item(lx, buf, size, start, frames, left, right):
    it = lx.WindowItem()
    it.lac, it.size, it.start, it.frames, it.left, it.right = C.cast(buf, C.POINTER(C.c_uint8)), size, start, frames, left, right
    return it


def test_whole_call_arguments(pkg, dec):
    L, lx = pkg.lacx.lib(), pkg.lacx
    lac = _fixture("small/n257_st16_ms.lac")
    buf = (C.c_uint8 * len(lac)).from_buffer_copy(lac)
    fake = 1 << 40  # never dereferenced: every one of these calls stops before the device
    items = (lx.WindowItem * 1)(_item(lx, buf, len(lac), 0, 1, fake, fake))
    fn = L.lacx_decoder_decode_window_batch_device
    assert fn(dec, items, 0, lx.SAMPLE_I32, None, None, None) == lx.E_INVALID  # n = 0
    assert fn(dec, None, 1, lx.SAMPLE_I32, None, None, None) == lx.E_INVALID
    assert fn(None, items, 1, lx.SAMPLE_I32, None, None, None) == lx.E_INVALID
    for bad_type in (2, -1, 7):
        assert fn(dec, items, 1, bad_type, None, None, None) == lx.E_INVALID
        assert _last_error(pkg) == "unknown sample type"
        l = np.full(1, 7, dtype=np.int32)
        r = np.full(1, 7, dtype=np.int32)
        rc = L.lacx_decoder_decode_window(dec, buf, len(lac), 0, 1, bad_type, l.ctypes.data, r.ctypes.data, None)
        assert rc == lx.E_INVALID and _last_error(pkg) == "unknown sample type"
        assert l[0] == 7 and r[0] == 7
    assert L.lacx_decoder_decode_window(None, buf, len(lac), 0, 1, 0, fake, fake, None) == lx.E_INVALID
    d = lx.Decoder()
    with pytest.raises(ValueError):
        d.decode_window(lac, 0, 1, dtype=np.int16)
    with pytest.raises(ValueError):
        d.decode_window_batch_device([lac], [0], 1, [(fake, fake)], dtype="float64")
    with pytest.raises(ValueError):
        d.decode_window_batch_device([lac], [0, 1], 1, [(fake, fake)])
    with pytest.raises(ValueError):
        d.decode_window_batch_device([], [], 1, [])
    d.close()


def test_window_checks_before_the_device(pkg, dec):
    """Each bad item gets its own message; the parse results of the others are filled, whether or not a device exists."""
    L, lx = pkg.lacx.lib(), pkg.lacx
    stereo = _fixture("small/n257_st16_ms.lac")
    mono = _fixture("small/n33_mono16.lac")
    si, mi = lx.stream_parse(stereo), lx.stream_parse(mono)
    assert (si.frames, si.channels, mi.frames, mi.channels) == (257, 2, 33, 1)
    keep = []  # the ctypes buffers the items point into
    fake = 1 << 40
    have_device = lx.device_count() > 0
    cases = [  # (stream, start, frames, left, right, message)
        # a good window: without a device it reaches the device check; with one it has no arrays, so that nothing runs
        (stereo, 3, 5, None if have_device else fake, fake, "output arrays missing" if have_device else None),
        (stereo, 0, 0, fake, fake, "empty window"),
        (stereo, 200, 58, fake, fake, "window outside the stream"),  # start + frames one past the end
        (stereo, 257, 1, fake, fake, "window outside the stream"),
        (stereo, (1 << 64) - 2, 4, fake, fake, "window outside the stream"),  # start + frames wraps around
        (stereo, 5, (1 << 64) - 1, fake, fake, "window outside the stream"),
        (stereo, 0, 257, fake, None, "output arrays missing"),
        (stereo, 0, 257, None, fake, "output arrays missing"),
        (mono, 0, 33, None, None, "output arrays missing"),
        (b"XX" + stereo[2:], 0, 1, fake, fake, "[decode-error] invalid frame header"),
        (mono, 32, 1, None if have_device else fake, None, "output arrays missing" if have_device else None),
    ]
    n = len(cases)
    items = (lx.WindowItem * n)()
    for it, (lac, start, frames, l, r, _) in zip(items, cases):
        b = (C.c_uint8 * len(lac)).from_buffer_copy(lac)
        keep.append(b)
        it.lac, it.size, it.start, it.frames, it.left, it.right = C.cast(b, C.POINTER(C.c_uint8)), len(lac), start, frames, l, r
    for st in (lx.SAMPLE_I32, lx.SAMPLE_F32):
        rcs = (C.c_int * n)(*([-1] * n))
        rc = L.lacx_decoder_decode_window_batch_device(dec, items, n, st, None, rcs, None)
        for i, case in enumerate(cases):
            want = case[5]
            if want is None:  # parses, window fine: only the missing device stops it
                assert rcs[i] == lx.E_DEVICE and L.lacx_decoder_item_error(dec, i).decode() == "no usable HIP device"
            else:
                assert rcs[i] == lx.E_INVALID, i
                assert L.lacx_decoder_item_error(dec, i).decode() == want, i
        if have_device:  # every item failed on the host: the lowest names the call
            assert rc == lx.E_INVALID and _last_error(pkg) == "stream 0: output arrays missing"
        else:
            assert rc == lx.E_DEVICE and _last_error(pkg) == "no usable HIP device"


def test_single_window_checks(pkg, dec):
    L, lx = pkg.lacx.lib(), pkg.lacx
    lac = _fixture("small/n257_st16_ms.lac")
    buf = (C.c_uint8 * len(lac)).from_buffer_copy(lac)
    l = np.full(8, 7, dtype=np.int32)
    r = np.full(8, 7, dtype=np.int32)
    for start, frames, rp, want in ((0, 0, r, "empty window"), (250, 8, r, "window outside the stream"),
                                    ((1 << 64) - 1, 2, r, "window outside the stream"), (0, 8, None, "output arrays missing")):
        rc = L.lacx_decoder_decode_window(dec, buf, len(lac), start, frames, lx.SAMPLE_I32, l.ctypes.data,
                                          rp.ctypes.data if rp is not None else None, None)
        assert rc == lx.E_INVALID and _last_error(pkg) == want  # no "stream 0: "
        assert (l == 7).all() and (r == 7).all()
    d = lx.Decoder()
    with pytest.raises(RuntimeError, match=r"^window outside the stream$"):
        d.decode_window(lac, 255, 3)
    with pytest.raises(RuntimeError, match=r"^\[decode-error\] invalid frame header$"):
        d.decode_window(b"XX" + lac[2:], 0, 1)
    if lx.device_count() <= 0:
        rc = L.lacx_decoder_decode_window(dec, buf, len(lac), 0, 8, lx.SAMPLE_F32, l.ctypes.data, r.ctypes.data, None)
        assert rc == lx.E_DEVICE and _last_error(pkg) == "no usable HIP device"
        assert (l == 7).all() and (r == 7).all()
        with pytest.raises(RuntimeError, match="no usable HIP device") as e:
            d.decode_window(lac, 0, 8, dtype=np.float32)
        assert not isinstance(e.value, lx.BatchDecodeError)
        with pytest.raises(RuntimeError, match="no usable HIP device") as e:
            d.decode_window_batch_device([lac], [0], 8, [(1 << 40, 1 << 40)])
        assert not isinstance(e.value, lx.BatchDecodeError)
    d.close()
