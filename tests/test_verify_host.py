"""The verify entry points without a device: their symbols, structs and error code, the checks of every item's stream and
source, which run on the host before any device call and give each item its own message, and the format comparison of
lacx_decoder_verify_wav, which needs no device either."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import __graft_entry__ as ge
import wavutil as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NEW = ("lacx_decoder_verify_batch_device", "lacx_decoder_verify_wav")
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


def test_symbols_structs_and_code(pkg):
    L, lx = pkg.lacx.lib(), pkg.lacx
    header = open(os.path.join(ROOT, "include", "lacx.h")).read()
    for name in NEW:
        assert hasattr(L, name) and name in lx.EXPORTS
        assert re.search(rf"\b{name}\s*\(", header), name
        assert header.index(name) < header.index("#ifndef LACX_H"), name  # listed in the comment block at the top
    assert "} lacx_verify_item;" in header and "} lacx_verify_result;" in header
    assert re.search(r"#define LACX_E_MISMATCH 4\b", header) and lx.E_MISMATCH == 4
    assert lx.abi_structs()["verify_item"] is lx.VerifyItem and lx.abi_structs()["verify_result"] is lx.VerifyResult
    assert L.lacx_sizeof(b"verify_item") == C.sizeof(lx.VerifyItem) == 48
    assert L.lacx_sizeof(b"verify_result") == C.sizeof(lx.VerifyResult) == 32
    assert (lx.VerifyResult.frame.offset, lx.VerifyResult.block.offset, lx.VerifyResult.channel.offset,
            lx.VerifyResult.decoded.offset, lx.VerifyResult.source.offset) == (8, 16, 20, 24, 28)
    assert (lx.VerifyItem.pcm.offset, lx.VerifyItem.frames.offset) == (16, 40)


def _item(lx, buf, size, d0, d1, layout, channels, frames):
    it = lx.VerifyItem()
    it.lac, it.size, it.pcm, it.frames = C.cast(buf, C.POINTER(C.c_uint8)), size, lx.Pcm(d0, d1, layout, channels), frames
    return it


def test_whole_call_arguments(pkg, dec):
    L, lx = pkg.lacx.lib(), pkg.lacx
    lac = _fixture("small/n257_st16_ms.lac")
    buf = (C.c_uint8 * len(lac)).from_buffer_copy(lac)
    items = (lx.VerifyItem * 1)(_item(lx, buf, len(lac), FAKE, FAKE, lx.PCM_PLANAR_I32, 2, 257))
    fn = L.lacx_decoder_verify_batch_device
    assert fn(dec, items, 0, None, None, None, None) == lx.E_INVALID  # n = 0
    assert _last_error(pkg) == "null argument or empty batch"
    assert fn(dec, None, 1, None, None, None, None) == lx.E_INVALID
    assert fn(None, items, 1, None, None, None, None) == lx.E_INVALID
    assert _last_error(pkg) == "null decoder"
    res = lx.VerifyResult(7, 7, 7, 7, (7, 7, 7), 7, 7)
    wav = W.make_wav(np.zeros(257, np.int32), np.zeros(257, np.int32), 48000, 16)
    wbuf = (C.c_uint8 * len(wav)).from_buffer_copy(wav)
    assert L.lacx_decoder_verify_wav(None, buf, len(lac), wbuf, len(wav), C.byref(res), None) == lx.E_INVALID
    assert res.mismatches == 0 and res.frame == 0  # zeroed whatever happens
    assert L.lacx_decoder_verify_wav(dec, buf, len(lac), None, 0, C.byref(res), None) == lx.E_INVALID
    d = lx.Decoder()
    with pytest.raises(ValueError):
        d.verify_batch_device([lac], [])
    with pytest.raises(ValueError):
        d.verify_batch_device([], [])
    d.close()


def test_source_checks_before_the_device(pkg, dec):
    """Each bad item gets its own message; the parse results of the others are filled, whether or not a device exists."""
    L, lx = pkg.lacx.lib(), pkg.lacx
    stereo = _fixture("small/n257_st16_ms.lac")
    mono = _fixture("small/n33_mono16.lac")
    deep = _fixture("small/n16421_st24_lr.lac")
    si, mi, di = lx.stream_parse(stereo), lx.stream_parse(mono), lx.stream_parse(deep)
    assert (si.frames, si.channels, si.bit_depth, mi.frames, mi.channels) == (257, 2, 16, 33, 1)
    assert (di.frames, di.channels, di.bit_depth) == (16421, 2, 24)
    P, I16, I24 = lx.PCM_PLANAR_I32, lx.PCM_INTERLEAVED_I16, lx.PCM_INTERLEAVED_I24
    have_device = lx.device_count() > 0
    # with a device, the items that would pass every check have no arrays, so that nothing runs on it
    ok = "source arrays missing" if have_device else None
    good = None if have_device else FAKE
    cases = [  # (stream, data0, data1, layout, channels, frames, message)
        (stereo, good, FAKE, P, 2, 257, ok),
        (stereo, None, FAKE, P, 2, 257, "source arrays missing"),
        (stereo, FAKE, None, P, 2, 257, "source arrays missing"),
        (stereo, None, None, I16, 2, 257, "source arrays missing"),
        (mono, None, None, P, 1, 33, "source arrays missing"),
        (stereo, FAKE, FAKE, P, 1, 257, "source channel count does not match the stream"),
        (mono, FAKE, FAKE, I16, 2, 33, "source channel count does not match the stream"),
        (stereo, FAKE, FAKE, P, 0, 257, "source channel count does not match the stream"),
        (stereo, FAKE, FAKE, P, 2, 256, "source frame count does not match the stream"),
        (stereo, FAKE, None, I16, 2, 258, "source frame count does not match the stream"),
        (mono, FAKE, None, P, 1, 0, "source frame count does not match the stream"),
        (stereo, FAKE, None, I24, 2, 257, "source layout does not match the stream's bit depth"),
        (deep, FAKE, None, I16, 2, 16421, "source layout does not match the stream's bit depth"),
        (stereo, FAKE, FAKE, 3, 2, 257, "unknown source layout"),
        (stereo, FAKE, FAKE, 0xFFFFFFFF, 2, 257, "unknown source layout"),
        (stereo, FAKE + 2, FAKE, P, 2, 257, "source arrays are not 4-byte aligned"),
        (stereo, FAKE, FAKE + 1, P, 2, 257, "source arrays are not 4-byte aligned"),
        (stereo, FAKE + 2, None, I16, 2, 257, "source arrays are not 4-byte aligned"),
        (b"XX" + stereo[2:], FAKE, FAKE, P, 2, 257, "[decode-error] invalid frame header"),
        (stereo[:-1], FAKE, FAKE, P, 2, 257, "[decode-error] block payloads do not fill the file"),
        (mono, good, None, I16, 1, 33, ok),
        (deep, None if have_device else FAKE + 3, None, I24, 2, 16421, ok),  # packed 24-bit: any byte alignment
        (deep, good, FAKE, P, 2, 16421, ok),  # planar int32 for a 24-bit stream
    ]
    n = len(cases)
    keep = []
    items = (lx.VerifyItem * n)()
    for k, (lac, d0, d1, layout, ch, frames, _) in enumerate(cases):
        b = (C.c_uint8 * len(lac)).from_buffer_copy(lac)
        keep.append(b)
        items[k] = _item(lx, b, len(lac), d0, d1, layout, ch, frames)
    rcs = (C.c_int * n)(*([-1] * n))
    res = (lx.VerifyResult * n)(*[lx.VerifyResult(9, 9, 9, 9, (9, 9, 9), 9, 9) for _ in range(n)])
    rc = L.lacx_decoder_verify_batch_device(dec, items, n, None, rcs, res, None)
    for i, case in enumerate(cases):
        want = case[6]
        if want is None:  # parses, source fine: only the missing device stops it
            assert rcs[i] == lx.E_DEVICE and L.lacx_decoder_item_error(dec, i).decode() == "no usable HIP device", i
        else:
            assert rcs[i] == lx.E_INVALID, i
            assert L.lacx_decoder_item_error(dec, i).decode() == want, i
        assert bytes(res[i]) == bytes(32), i  # zeroed for every item that did not differ
    if have_device:  # every item failed on the host: the lowest names the call
        assert rc == lx.E_INVALID and _last_error(pkg) == "stream 0: source arrays missing"
    else:
        assert rc == lx.E_DEVICE and _last_error(pkg) == "no usable HIP device"
        d = lx.Decoder()
        with pytest.raises(RuntimeError, match="no usable HIP device") as e:
            d.verify_batch_device([stereo], [(FAKE, FAKE, P, 2, 257)])
        assert not isinstance(e.value, lx.BatchDecodeError)
        d.close()
    # the binding: the per-item errors travel in BatchDecodeError
    if have_device:
        d = lx.Decoder()
        with pytest.raises(lx.BatchDecodeError) as e:
            d.verify_batch_device([stereo, mono], [(FAKE, FAKE, 3, 2, 257), (None, None, P, 1, 33)])
        assert e.value.errors == {0: "unknown source layout", 1: "source arrays missing"} and e.value.results == [None, None]
        assert str(e.value) == "stream 0: unknown source layout"
        d.close()


def _wav_header_only(channels, rate, bits, frames):
    """A WAV image of that format whose data chunk holds zeros."""
    z = np.zeros(frames, dtype=np.int32)
    return W.make_wav(z, z if channels == 2 else None, rate, bits)


def test_verify_wav_format_differences_need_no_device(pkg, dec):
    L, lx = pkg.lacx.lib(), pkg.lacx
    lac = _fixture("small/n257_st16_ms.lac")
    info = lx.stream_parse(lac)
    assert (info.channels, info.bit_depth, info.frames) == (2, 16, 257)
    rate = info.sample_rate
    other_rate = 96000 if rate != 96000 else 48000
    buf = (C.c_uint8 * len(lac)).from_buffer_copy(lac)
    cases = [
        (_wav_header_only(1, rate, 16, 257), "[verify-error] channels: stream 2, source 1"),
        (_wav_header_only(2, rate, 24, 257), "[verify-error] bit depth: stream 16, source 24"),
        (_wav_header_only(2, other_rate, 16, 257), f"[verify-error] sample rate: stream {rate}, source {other_rate}"),
        (_wav_header_only(2, rate, 16, 256), "[verify-error] frames: stream 257, source 256"),
        (_wav_header_only(2, rate, 16, 258), "[verify-error] frames: stream 257, source 258"),
        # several differences: the first of channels, bit depth, sample rate, frames is named
        (_wav_header_only(1, other_rate, 24, 5), "[verify-error] channels: stream 2, source 1"),
    ]
    d = lx.Decoder()
    for wav, want in cases:
        wbuf = (C.c_uint8 * len(wav)).from_buffer_copy(wav)
        res = lx.VerifyResult(9, 9, 9, 9, (9, 9, 9), 9, 9)
        ms = C.c_float(5.0)
        rc = L.lacx_decoder_verify_wav(dec, buf, len(lac), wbuf, len(wav), C.byref(res), C.byref(ms))
        assert rc == lx.E_MISMATCH and _last_error(pkg) == want
        assert bytes(res) == bytes(32) and ms.value == 0.0
        r = d.verify_wav(lac, wav)  # an answer, not an exception
        assert (r.identical, r.format_differs, r.message, r.mismatches) == (False, True, want, 0)
    # not a WAV at all, and a stream that does not parse: errors, in that order of precedence
    junk = (C.c_uint8 * 64)()
    assert L.lacx_decoder_verify_wav(dec, buf, len(lac), junk, 64, None, None) == lx.E_INVALID
    assert _last_error(pkg).startswith("[verify-error] source is not a PCM WAV")
    with pytest.raises(ValueError, match="not a PCM WAV"):
        d.verify_wav(lac, bytes(64))
    bad = (C.c_uint8 * len(lac)).from_buffer_copy(b"XX" + lac[2:])
    assert L.lacx_decoder_verify_wav(dec, bad, len(lac), junk, 64, None, None) == lx.E_INVALID
    assert _last_error(pkg) == "[decode-error] invalid frame header"
    with pytest.raises(RuntimeError, match=r"^\[decode-error\] invalid frame header$"):
        d.verify_wav(b"XX" + lac[2:], cases[0][0])
    if lx.device_count() <= 0:  # equal formats: only the missing device stops it
        wav = _wav_header_only(2, rate, 16, 257)
        wbuf = (C.c_uint8 * len(wav)).from_buffer_copy(wav)
        assert L.lacx_decoder_verify_wav(dec, buf, len(lac), wbuf, len(wav), None, None) == lx.E_DEVICE
        assert _last_error(pkg) == "no usable HIP device"
        with pytest.raises(RuntimeError, match="no usable HIP device"):
            d.verify_wav(lac, wav)
    d.close()
