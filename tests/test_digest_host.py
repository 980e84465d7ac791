"""The digest entry points without a device: their symbols and structs, lacx_crc32_combine, the checks of every item's
stream or source, which run on the host before any device call and give each item its own message, and the composition
of wav_crc32 from its parts."""
import ctypes as C
import os
import random
import re
import zlib

import numpy as np
import pytest

import __graft_entry__ as ge
import wavutil as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NEW = ("lacx_decoder_digest_batch_device", "lacx_decoder_digest_pcm_batch_device", "lacx_crc32_combine")
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
    assert "} lacx_digest;" in header and "} lacx_digest_source;" in header
    assert lx.abi_structs()["digest"] is lx.Digest and lx.abi_structs()["digest_source"] is lx.DigestSource
    assert L.lacx_sizeof(b"digest") == C.sizeof(lx.Digest) == 32
    assert L.lacx_sizeof(b"digest_source") == C.sizeof(lx.DigestSource) == 40
    g, s = lx.Digest, lx.DigestSource
    assert (g.data_crc32.offset, g.wav_crc32.offset, g.frames.offset, g.data_bytes.offset, g.sample_rate.offset, g.channels.offset,
            g.bit_depth.offset, g.wav_valid.offset, g.reserved.offset) == (0, 4, 8, 16, 24, 28, 29, 30, 31)
    assert (s.pcm.offset, s.frames.offset, s.sample_rate.offset, s.bit_depth.offset) == (0, 24, 32, 36)


def test_crc32_combine_through_the_abi(pkg):
    L, lx = pkg.lacx.lib(), pkg.lacx
    rng = random.Random(11)
    for _ in range(200):
        m = rng.randbytes(rng.choice((0, 1, 2, 43, 44, 45, 4096, 65537)))
        cut = rng.choice((0, len(m), rng.randrange(0, len(m) + 1)))
        a, b = m[:cut], m[cut:]
        assert L.lacx_crc32_combine(zlib.crc32(a), zlib.crc32(b), len(b)) == zlib.crc32(m)
        assert lx.crc32_combine(zlib.crc32(a), zlib.crc32(b), len(b)) == zlib.crc32(m)
    # a length beyond 2^32: the distance is reduced mod 2^32 - 1 (x has that order)
    assert lx.crc32_combine(0x12345678, 0, (1 << 32) - 1) == 0x12345678
    assert lx.crc32_combine(0x12345678, 0, 5 * ((1 << 32) - 1) + 3) == lx.crc32_combine(0x12345678, 0, 3)


def test_wav_crc_composition(pkg):
    """wav_crc32 as the library composes it: header, data, pad.  Mono 24-bit with an odd frame count is the only format
    with a pad byte."""
    lx = pkg.lacx
    rng = np.random.default_rng(3)
    for channels, bits, frames in ((1, 24, 333), (1, 24, 1), (2, 24, 333), (1, 16, 333), (2, 16, 7)):
        left = rng.integers(-(1 << (bits - 1)), 1 << (bits - 1), frames).astype(np.int32)
        right = rng.integers(-(1 << (bits - 1)), 1 << (bits - 1), frames).astype(np.int32) if channels == 2 else None
        wav = W.make_wav(left, right, 96000, bits)
        data = W.pcm_bytes(left, right, bits)
        pad = len(data) & 1
        assert pad == (1 if (channels, bits) == (1, 24) else 0) and len(wav) == 44 + len(data) + pad
        assert wav[44:44 + len(data)] == data
        crc = lx.crc32_combine(zlib.crc32(wav[:44]), zlib.crc32(data), len(data))
        if pad:
            assert wav[-1] == 0
            crc = lx.crc32_combine(crc, zlib.crc32(b"\0"), 1)
        assert crc == zlib.crc32(wav)


def test_whole_call_arguments(pkg, dec):
    L, lx = pkg.lacx.lib(), pkg.lacx
    lac = _fixture("small/n257_st16_ms.lac")
    buf = (C.c_uint8 * len(lac)).from_buffer_copy(lac)
    spans = (lx.Span * 1)(lx.Span(C.cast(buf, C.POINTER(C.c_uint8)), len(lac)))
    fn = L.lacx_decoder_digest_batch_device
    assert fn(dec, spans, 0, None, None, None, None) == lx.E_INVALID  # n = 0
    assert _last_error(pkg) == "null argument or empty batch"
    assert fn(dec, None, 1, None, None, None, None) == lx.E_INVALID
    assert fn(None, spans, 1, None, None, None, None) == lx.E_INVALID
    assert _last_error(pkg) == "null decoder"
    srcs = (lx.DigestSource * 1)(lx.DigestSource(lx.Pcm(FAKE, FAKE, lx.PCM_PLANAR_I32, 2), 257, 48000, 16))
    fn = L.lacx_decoder_digest_pcm_batch_device
    assert fn(dec, srcs, 0, None, None, None, None) == lx.E_INVALID
    assert _last_error(pkg) == "null argument or empty batch"
    assert fn(dec, None, 1, None, None, None, None) == lx.E_INVALID
    assert fn(None, srcs, 1, None, None, None, None) == lx.E_INVALID
    assert _last_error(pkg) == "null decoder"
    d = lx.Decoder()
    with pytest.raises(ValueError):
        d.digest_batch([])
    with pytest.raises(ValueError):
        d.digest_pcm_batch([])
    d.close()


def test_stream_checks_before_the_device(pkg, dec):
    """Parse errors are per item and need no device; without one the items that parse carry LACX_E_DEVICE.  (With a
    device only the items that fail on the host are in the batch, so that nothing runs on it: the mixed batch is
    tests/test_gpu_digest.py's.)"""
    L, lx = pkg.lacx.lib(), pkg.lacx
    have_device = lx.device_count() > 0
    good = _fixture("small/n257_st16_ms.lac")
    lacs = [b"XX" + good[2:], good[:-1]] + ([] if have_device else [good, _fixture("small/n33_mono16.lac")])
    want = ["[decode-error] invalid frame header", "[decode-error] block payloads do not fill the file", None, None][:len(lacs)]
    n = len(lacs)
    keep = [(C.c_uint8 * len(x)).from_buffer_copy(x) for x in lacs]
    spans = (lx.Span * n)(*[lx.Span(C.cast(b, C.POINTER(C.c_uint8)), len(x)) for b, x in zip(keep, lacs)])
    rcs = (C.c_int * n)(*([-1] * n))
    out = (lx.Digest * n)(*[lx.Digest(9, 9, 9, 9, 9, 9, 9, 9, 9) for _ in range(n)])
    ms = C.c_float(5.0)
    rc = L.lacx_decoder_digest_batch_device(dec, spans, n, None, rcs, out, C.byref(ms))
    assert ms.value == 0.0
    if have_device:
        assert rc == lx.E_INVALID and _last_error(pkg) == "stream 0: [decode-error] invalid frame header"
    else:
        assert rc == lx.E_DEVICE and _last_error(pkg) == "no usable HIP device"
    for i, w in enumerate(want):
        assert rcs[i] == (lx.E_DEVICE if w is None else lx.E_INVALID), i
        assert L.lacx_decoder_item_error(dec, i).decode() == (w or "no usable HIP device"), i
        assert bytes(out[i]) == bytes(32), i  # zeroed for every item without a digest
    d = lx.Decoder()
    if have_device:  # the binding: the per-item errors travel in BatchDecodeError, a single stream's as RuntimeError
        with pytest.raises(RuntimeError, match=r"^\[decode-error\] invalid frame header$"):
            d.digest(lacs[0])
        with pytest.raises(lx.BatchDecodeError) as e:
            d.digest_batch(lacs[:2])
        assert e.value.errors == {0: want[0], 1: want[1]} and e.value.results == [None, None]
    else:
        with pytest.raises(RuntimeError, match="no usable HIP device") as e:
            d.digest_batch([good])
        assert not isinstance(e.value, lx.BatchDecodeError)
        with pytest.raises(RuntimeError, match="no usable HIP device"):
            d.digest(good)
    d.close()


def test_source_checks_before_the_device(pkg, dec):
    """Each bad source gets its own message; the others reach the device, or LACX_E_DEVICE where there is none."""
    L, lx = pkg.lacx.lib(), pkg.lacx
    P, I16, I24 = lx.PCM_PLANAR_I32, lx.PCM_INTERLEAVED_I16, lx.PCM_INTERLEAVED_I24
    P16, PF, IF = lx.PCM_PLANAR_I16, lx.PCM_PLANAR_F32, lx.PCM_INTERLEAVED_F32
    have_device = lx.device_count() > 0
    # with a device, the items that would pass every check have no arrays, so that nothing runs on it
    ok = "source arrays missing" if have_device else None
    good = None if have_device else FAKE
    cases = [  # (data0, data1, layout, channels, frames, rate, depth, message)
        (good, FAKE, P, 2, 257, 48000, 16, ok),
        (None, FAKE, P, 2, 257, 48000, 16, "source arrays missing"),
        (FAKE, None, P, 2, 257, 48000, 16, "source arrays missing"),
        (FAKE, None, PF, 2, 257, 48000, 16, "source arrays missing"),
        (None, None, I16, 2, 257, 48000, 16, "source arrays missing"),
        (FAKE, FAKE, 3, 2, 257, 48000, 16, "unknown source layout"),
        (FAKE, FAKE, 19, 2, 257, 48000, 16, "unknown source layout"),
        (FAKE, FAKE, 0xFFFFFFFF, 2, 257, 48000, 16, "unknown source layout"),
        (FAKE, FAKE, P, 0, 257, 48000, 16, "unsupported channel count"),
        (FAKE, FAKE, P, 3, 257, 48000, 16, "unsupported channel count"),
        (FAKE, FAKE, P, 2, 0, 48000, 16, "source has no frames"),
        (FAKE, FAKE, P, 2, 1 << 56, 48000, 16, "source frame count out of range"),
        (FAKE, FAKE, P, 2, 257, 22050, 16, "unsupported sample rate: 22050"),
        (FAKE, FAKE, P, 2, 257, 48000, 8, "unsupported bit depth: 8"),
        (FAKE, FAKE, P, 2, 257, 48000, 32, "unsupported bit depth: 32"),
        (FAKE, None, I24, 2, 257, 48000, 16, "source layout does not match the stream's bit depth"),
        (FAKE, None, I16, 2, 257, 48000, 24, "source layout does not match the stream's bit depth"),
        (FAKE, FAKE, P16, 2, 257, 48000, 24, "source layout does not match the stream's bit depth"),
        (FAKE + 2, FAKE, P, 2, 257, 48000, 16, "source arrays are not 4-byte aligned"),
        (FAKE, FAKE + 1, P, 2, 257, 48000, 16, "source arrays are not 4-byte aligned"),
        (FAKE + 2, None, I16, 2, 257, 48000, 16, "source arrays are not 4-byte aligned"),
        (FAKE + 2, None, IF, 2, 257, 48000, 24, "source arrays are not 4-byte aligned"),
        (FAKE + 1, FAKE, P16, 2, 257, 48000, 16, "source arrays are not 2-byte aligned"),
        (FAKE, FAKE + 3, P16, 2, 257, 48000, 16, "source arrays are not 2-byte aligned"),
        (None if have_device else FAKE + 3, None, I24, 2, 257, 192000, 24, ok),  # packed 24-bit: any byte alignment
        (None if have_device else FAKE + 2, None, P16, 1, 33, 44100, 16, ok),
        (good, FAKE + 3, P, 1, 33, 96000, 24, ok),  # a mono source's data1 is not looked at
    ]
    n = len(cases)
    items = (lx.DigestSource * n)()
    for k, (d0, d1, layout, ch, frames, rate, depth, _) in enumerate(cases):
        items[k] = lx.DigestSource(lx.Pcm(d0, d1, layout, ch), frames, rate, depth)
    rcs = (C.c_int * n)(*([-1] * n))
    out = (lx.Digest * n)(*[lx.Digest(9, 9, 9, 9, 9, 9, 9, 9, 9) for _ in range(n)])
    rc = L.lacx_decoder_digest_pcm_batch_device(dec, items, n, None, rcs, out, None)
    for i, case in enumerate(cases):
        want = case[7]
        if want is None:
            assert rcs[i] == lx.E_DEVICE and L.lacx_decoder_item_error(dec, i).decode() == "no usable HIP device", i
        else:
            assert rcs[i] == lx.E_INVALID, i
            assert L.lacx_decoder_item_error(dec, i).decode() == want, i
        assert bytes(out[i]) == bytes(32), i
    if have_device:  # every item failed on the host: the lowest names the call
        assert rc == lx.E_INVALID and _last_error(pkg) == "stream 0: source arrays missing"
    else:
        assert rc == lx.E_DEVICE and _last_error(pkg) == "no usable HIP device"
    d = lx.Decoder()
    if have_device:
        with pytest.raises(lx.BatchDecodeError) as e:
            d.digest_pcm_batch([((FAKE, FAKE, 3, 2, 257), 48000, 16), ((None, None, P, 1, 33), 48000, 16)])
        assert e.value.errors == {0: "unknown source layout", 1: "source arrays missing"} and e.value.results == [None, None]
        assert str(e.value) == "stream 0: unknown source layout"
    else:
        with pytest.raises(RuntimeError, match="no usable HIP device") as e:
            d.digest_pcm_batch([((FAKE, FAKE, P, 2, 257), 48000, 16)])
        assert not isinstance(e.value, lx.BatchDecodeError)
    # a numpy array describes itself (pcm_of), and what it cannot describe is refused before the library
    with pytest.raises(ValueError, match="int16 samples need bit depth 16"):
        d.digest_pcm_batch([(np.zeros((2, 8), np.int16), 48000, 24)])
    d.close()
