"""The batch decode entry points without a device: their symbols and structs, the argument checks, and the per-item parse
results, which are found on the host before any device call and carry the messages the single-stream parse gives."""
import ctypes as C
import os
import re

import pytest

import __graft_entry__ as ge

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NEW = ("lacx_decoder_decode_wav_batch", "lacx_decoder_decode_wav_batch_view", "lacx_decoder_decode_batch_device",
       "lacx_decoder_item_error")


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
    L = pkg.lacx.lib()
    header = open(os.path.join(ROOT, "include", "lacx.h")).read()
    for name in NEW:
        assert hasattr(L, name) and name in pkg.lacx.EXPORTS
        assert re.search(rf"\b{name}\s*\(", header), name
    for name, cls in (("span", pkg.lacx.Span), ("decode_item", pkg.lacx.DecodeItem)):
        assert f"}} lacx_{name};" in header
        assert pkg.lacx.abi_structs()[name] is cls
        assert L.lacx_sizeof(name.encode()) == C.sizeof(cls) > 0
    assert C.sizeof(pkg.lacx.Span) == 16 and C.sizeof(pkg.lacx.DecodeItem) == 40


def test_empty_and_null_arguments(pkg, dec):
    L, lx = pkg.lacx.lib(), pkg.lacx
    lac = _fixture("small/n33_mono16.lac")
    buf = (C.c_uint8 * len(lac)).from_buffer_copy(lac)
    spans = (lx.Span * 1)(lx.Span(C.cast(buf, C.POINTER(C.c_uint8)), len(lac)))
    outs = (lx.Span * 1)()
    items = (lx.DecodeItem * 1)()
    for fn in (L.lacx_decoder_decode_wav_batch_view, L.lacx_decoder_decode_wav_batch):
        assert fn(dec, spans, 0, outs, None, None) == lx.E_INVALID  # n = 0
        assert fn(dec, None, 1, outs, None, None) == lx.E_INVALID
        assert fn(dec, spans, 1, None, None, None) == lx.E_INVALID
        assert fn(None, spans, 1, outs, None, None) == lx.E_INVALID
    assert L.lacx_decoder_decode_batch_device(dec, items, 0, None, None, None) == lx.E_INVALID
    assert L.lacx_decoder_decode_batch_device(dec, None, 1, None, None, None) == lx.E_INVALID
    assert L.lacx_decoder_decode_batch_device(None, items, 1, None, None, None) == lx.E_INVALID
    assert L.lacx_decoder_item_error(dec, 0) == b"" and L.lacx_decoder_item_error(None, 0) == b""
    with pytest.raises(ValueError):
        lx.Decoder().decode_wav_batch([])


def _mixed_batch():
    good = _fixture("small/n257_st16_ms.lac")
    bad_header = b"XX" + good[2:]
    truncated = good[:20]  # the block table is cut
    return [good, bad_header, truncated]


def _single_parse_message(pkg, lac):
    assert pkg.lacx.stream_parse(lac) is None
    return _last_error(pkg)


@pytest.mark.parametrize("form", ["wav", "device"])
def test_per_item_parse_results(pkg, dec, form):
    L, lx = pkg.lacx.lib(), pkg.lacx
    lacs = _mixed_batch()
    want = {1: _single_parse_message(pkg, lacs[1]), 2: _single_parse_message(pkg, lacs[2])}
    assert want[1] == "[decode-error] invalid frame header"
    assert want[2] == "[decode-error] truncated block size table"
    bufs = [(C.c_uint8 * len(x)).from_buffer_copy(x) for x in lacs]
    rcs = (C.c_int * 3)(-1, -1, -1)
    if form == "wav":
        spans = (lx.Span * 3)(*[lx.Span(C.cast(b, C.POINTER(C.c_uint8)), len(x)) for b, x in zip(bufs, lacs)])
        outs = (lx.Span * 3)()
        rc = L.lacx_decoder_decode_wav_batch_view(dec, spans, 3, outs, rcs, None)
    else:
        # No device: placeholder addresses, never dereferenced (the call stops before any device work).  A device:
        # no output arrays for the good item, so the call fails on the host as well.
        items = (lx.DecodeItem * 3)()
        fake = 1 << 40 if lx.device_count() <= 0 else None
        for it, b, x in zip(items, bufs, lacs):
            it.lac, it.size, it.frames, it.left, it.right = C.cast(b, C.POINTER(C.c_uint8)), len(x), 257, fake, fake
        rc = L.lacx_decoder_decode_batch_device(dec, items, 3, None, rcs, None)
    for i in (1, 2):
        assert rcs[i] == lx.E_INVALID
        assert L.lacx_decoder_item_error(dec, i).decode() == want[i]
    if lx.device_count() <= 0:
        assert rc == lx.E_DEVICE and _last_error(pkg) == "no usable HIP device"
        assert rcs[0] == lx.E_DEVICE and L.lacx_decoder_item_error(dec, 0).decode() == "no usable HIP device"
        if form == "wav":
            assert all(not outs[i].data and outs[i].size == 0 for i in range(3))
    elif form == "wav":  # with a device the good item decodes and the lowest failing item names the call
        assert rcs[0] == lx.OK and L.lacx_decoder_item_error(dec, 0) == b"" and outs[0].size > 44
        assert rc == lx.E_INVALID and _last_error(pkg) == "stream 1: " + want[1]
    else:  # the good item has no output arrays: lacx_decoder_decode's message, and no device access
        assert rcs[0] == lx.E_INVALID and L.lacx_decoder_item_error(dec, 0) == b"output arrays missing"
        assert rc == lx.E_INVALID and _last_error(pkg) == "stream 0: output arrays missing"


def test_python_batch_errors_without_device(pkg):
    lacs = _mixed_batch()
    dec = pkg.lacx.Decoder()
    if pkg.lacx.device_count() <= 0:
        with pytest.raises(RuntimeError, match="no usable HIP device") as e:
            dec.decode_wav_batch(lacs)
        assert not isinstance(e.value, pkg.lacx.BatchDecodeError)
        with pytest.raises(RuntimeError, match="no usable HIP device"):
            dec.decode_wav_batch_view(lacs[:1])
        with pytest.raises(RuntimeError, match="no usable HIP device"):
            dec.decode_batch_device(lacs[:1], [(0, 0)])
    else:
        with pytest.raises(pkg.lacx.BatchDecodeError) as e:
            dec.decode_wav_batch(lacs)
        assert set(e.value.errors) == {1, 2} and e.value.results[0] is not None
        assert e.value.results[1] is None and e.value.results[2] is None
    with pytest.raises(ValueError):
        dec.decode_batch_device(lacs, [])
    dec.close()
