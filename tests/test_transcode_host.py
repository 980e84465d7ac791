"""lacx_transcode_batch without a device: its symbol and structs, the whole-call refusals, and the checks of every output,
which run on the host before any device work and give each output its own message."""
import ctypes as C
import os
import re

import pytest

import __graft_entry__ as ge
import editcases as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pkg():
    mod = ge.load_pkg()
    if not os.path.exists(mod.lacx.LIB_PATH):
        mod.lacx.build()
    return mod


@pytest.fixture
def handles(pkg):
    lx = pkg.lacx
    dec, enc = C.c_void_p(), C.c_void_p()
    cfg = lx.Config(48000, 16, 2, 1, 1, -1, 0, 0)
    assert lx.lib().lacx_decoder_create(C.c_int(-1), C.byref(dec)) == lx.OK
    assert lx.lib().lacx_encoder_create(C.byref(cfg), C.byref(enc)) == lx.OK
    yield dec, enc
    lx.lib().lacx_decoder_destroy(dec)
    lx.lib().lacx_encoder_destroy(enc)


def _last_error(pkg):
    return pkg.lacx.lib().lacx_decode_last_error().decode()


def test_symbol_and_structs(pkg):
    L, lx = pkg.lacx.lib(), pkg.lacx
    header = open(os.path.join(ROOT, "include", "lacx.h")).read()
    assert hasattr(L, "lacx_transcode_batch") and "lacx_transcode_batch" in lx.EXPORTS
    assert re.search(r"\blacx_transcode_batch\s*\(", header)
    for name, cls, size in (("edit_segment", lx.EditSegment, 32), ("edit_output", lx.EditOutput, 16), ("edit_result", lx.EditResult, 40)):
        assert f"}} lacx_{name};" in header
        assert lx.abi_structs()[name] is cls
        assert L.lacx_sizeof(name.encode()) == C.sizeof(cls) == size
    for k, name in enumerate(("KEEP", "LEFT", "RIGHT", "FOLD", "SWAP", "DUAL")):
        assert re.search(rf"#define LACX_CH_{name} {k}u\b", header) and getattr(lx, "CH_" + name) == k
    assert re.search(r"#define LACX_TO_END UINT64_MAX\b", header) and lx.TO_END == 2 ** 64 - 1
    assert re.search(r"#define LACX_TRANSCODE_VERIFY 1u\b", header) and lx.TRANSCODE_VERIFY == 1


def _arrays(lx, segments, outputs):
    keep = [(C.c_uint8 * max(1, len(lac))).from_buffer_copy(lac if lac else b"\0") for lac, _, _ in segments]
    segs = (lx.EditSegment * max(1, len(segments)))(*[lx.EditSegment(C.cast(b, C.POINTER(C.c_uint8)), len(lac), start, frames)
                                                     for b, (lac, start, frames) in zip(keep, segments)])
    outs = (lx.EditOutput * max(1, len(outputs)))(*[lx.EditOutput(*o) for o in outputs])
    return keep, segs, outs


def test_whole_call_refusals(pkg, handles):
    L, lx = pkg.lacx.lib(), pkg.lacx
    dec, enc = handles
    lac = E.sources()["st16_auto"].lac
    keep, segs, outs = _arrays(lx, [(lac, 0, 10)], [(0, 1, 0, 0, 2)])
    span = (lx.Span * 1)()
    fn = L.lacx_transcode_batch
    assert fn(None, enc, segs, 1, outs, 1, 0, span, None, None, None) == lx.E_INVALID and _last_error(pkg) == "null decoder"
    assert fn(dec, None, segs, 1, outs, 1, 0, span, None, None, None) == lx.E_INVALID and _last_error(pkg) == "null encoder"
    for args in ((None, 1, outs, 1, 0, span), (segs, 1, None, 1, 0, span), (segs, 1, outs, 1, 0, None), (segs, 1, outs, 0, 0, span)):
        assert fn(dec, enc, *args, None, None, None) == lx.E_INVALID and _last_error(pkg) == "null argument or empty batch"
    for flags in (2, 3, 1 << 31):
        assert fn(dec, enc, segs, 1, outs, 1, flags, span, None, None, None) == lx.E_INVALID and _last_error(pkg) == "unknown flags"
    fan = C.c_void_p()
    cfg = lx.Config(48000, 16, 2, 1, 1, -1, 0, 0)
    devs = (C.c_int32 * 2)(0, 0)
    assert L.lacx_encoder_create_multi(C.byref(cfg), devs, C.c_uint32(2), C.c_uint32(0), C.byref(fan)) == lx.OK
    assert fn(dec, fan, segs, 1, outs, 1, 0, span, None, None, None) == lx.E_INVALID
    assert _last_error(pkg) == "a transcode job needs an encoder on one device, not a fan-out"
    L.lacx_encoder_destroy(fan)
    far, near = C.c_void_p(), C.c_void_p()
    cfg1 = lx.Config(48000, 16, 2, 1, 1, 1, 0, 0)
    assert L.lacx_encoder_create(C.byref(cfg1), C.byref(far)) == lx.OK and L.lacx_decoder_create(C.c_int(0), C.byref(near)) == lx.OK
    assert fn(near, far, segs, 1, outs, 1, 0, span, None, None, None) == lx.E_INVALID
    assert _last_error(pkg) == "the encoder is on another device than the decoder"
    L.lacx_encoder_destroy(far)
    L.lacx_decoder_destroy(near)
    assert not span[0].data and span[0].size == 0


def test_output_checks_before_the_device(pkg, handles):
    """Each refused output gets its own message and a zeroed result, whether or not a device exists."""
    L, lx = pkg.lacx.lib(), pkg.lacx
    dec, enc = handles
    src = E.sources()
    st, mono, st24 = src["st16_auto"].lac, src["mono24"].lac, src["st24_narrowable"].lac
    have_device = lx.device_count() > 0
    segments = [(st, 0, 10), (st, 40000, 1), (st, 39999, 2), (st, 0, 0), (st, 7, lx.TO_END), (mono, 0, 10), (st24, 0, 10),
                (b"XX" + st[2:], 0, 1), (b"", 0, 1), (st, 2 ** 64 - 2, 4), (st, 40000, lx.TO_END)]
    outputs = [  # (first, count, depth, op, mode), message
        ((0, 0, 0, 0, 2), "output has no segments"),
        ((11, 1, 0, 0, 2), "segments outside the call's array"),
        ((10, 2, 0, 0, 2), "segments outside the call's array"),
        ((0, 1, 0, 6, 2), "unknown channel operation"),
        ((0, 1, 20, 0, 2), "unsupported bit depth: 20"),
        ((0, 1, 0, 0, 3), "unknown stereo mode"),
        ((0, 2, 0, 0, 2), "segment 1: window outside the stream"),
        ((2, 1, 0, 0, 2), "segment 0: window outside the stream"),
        ((3, 1, 0, 0, 2), "segment 0: empty window"),
        ((9, 1, 0, 0, 2), "segment 0: window outside the stream"),
        ((10, 1, 0, 0, 2), "segment 0: window outside the stream"),
        ((4, 2, 0, 0, 2), "segment 1: channels differs from segment 0: 2, 1"),
        ((5, 2, 0, 0, 2), "segment 1: channels differs from segment 0: 1, 2"),
        ((6, 1, 0, 5, 2), "channel operation needs a mono source"),
        ((5, 1, 0, 3, 2), "channel operation needs a stereo source"),
        ((7, 1, 0, 0, 2), "segment 0: [decode-error] invalid frame header"),
        ((8, 1, 0, 0, 2), "segment 0: [decode-error] empty input"),
    ]
    if not have_device:  # outputs that pass: only the missing device stops them
        outputs += [((0, 1, 0, 0, 2), None), ((4, 1, 16, 1, 0), None), ((5, 1, 16, 5, 1), None)]
    keep, segs, outs = _arrays(lx, segments, [o for o, _ in outputs])
    n = len(outputs)
    for flags in (0, lx.TRANSCODE_VERIFY):
        spans = (lx.Span * n)()
        res = (lx.EditResult * n)()
        rcs = (C.c_int * n)(*([-1] * n))
        ms = C.c_float(-1)
        rc = L.lacx_transcode_batch(dec, enc, segs, len(segments), outs, n, flags, spans, rcs, res, C.byref(ms))
        for i, (_, want) in enumerate(outputs):
            if want is None:
                assert rcs[i] == lx.E_DEVICE and L.lacx_decoder_item_error(dec, i).decode() == "no usable HIP device"
            else:
                assert rcs[i] == lx.E_INVALID, i
                assert L.lacx_decoder_item_error(dec, i).decode() == want, i
            assert not spans[i].data and spans[i].size == 0
            assert bytes(res[i]) == bytes(C.sizeof(lx.EditResult))
        if have_device:  # every output was refused on the host: the lowest names the call, and nothing ran
            assert rc == lx.E_INVALID and _last_error(pkg) == "output 0: output has no segments"
        else:
            assert rc == lx.E_DEVICE and _last_error(pkg) == "no usable HIP device"
        assert ms.value == 0.0


def test_binding_raises_like_the_other_batch_calls(pkg):
    lx = pkg.lacx
    dec, enc = lx.Decoder(), lx.Encoder(12, 2, 48000, 16)
    if lx.device_count() <= 0:  # (with a device the call runs: tests/test_gpu_transcode.py)
        with pytest.raises(RuntimeError, match="no usable HIP device") as e:
            dec.cut(enc, E.sources()["st16_auto"].lac, 0, 10)
        assert not isinstance(e.value, lx.BatchDecodeError)
    with pytest.raises(KeyError):
        dec.recompress(enc, E.sources()["st16_auto"].lac, channels="middle")
    dec.close()
