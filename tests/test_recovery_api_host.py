"""The recovery entry points of liblacx.so without a device: the calls' own argument checks, lacx_recovery_parse against
the restatement, and what is judged per item on the host -- a refused container, a refused sidecar -- with and without a
device.  (With a device only items that fail on the host are in a batch, so that nothing runs on it.)"""
import ctypes as C
import os
import struct

import pytest

import recoverytwin as rt

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _fixture(rel):
    with open(os.path.join(GOLDEN, rel), "rb") as f:
        return f.read()


LAC = _fixture("small/n2400_mono16_selftest.lac")
SIDE = rt.build(LAC, 64, 2, 4)


def _last(pkg):
    return pkg.lacx.lib().lacx_decode_last_error().decode()


def _spans(lx, blobs):
    keep = [(C.c_uint8 * max(1, len(x))).from_buffer_copy(x if x else b"\0") for x in blobs]
    return (lx.Span * len(blobs))(*[lx.Span(C.cast(b, C.POINTER(C.c_uint8)), len(x)) for b, x in zip(keep, blobs)]), keep


@pytest.fixture()
def dec(pkg):
    h = C.c_void_p()
    assert pkg.lacx.lib().lacx_decoder_create(-1, C.byref(h)) == 0
    yield h
    pkg.lacx.lib().lacx_decoder_destroy(h)


def test_parse_is_the_restatements(pkg):
    lx = pkg.lacx
    info = lx.recovery_parse(SIDE)
    geo = rt.geometry(len(LAC), 64, 2, 4)
    assert (info.file_bytes, info.slice_bytes, info.slices, info.groups, info.parity, info.group_data, info.parity_present, info.flags,
            info.reserved) == (len(LAC), 64, geo.k, geo.G, 2, 4, geo.G * 2, 0, 0)
    cut = lx.recovery_parse(SIDE[:40 + 4 * geo.k + 3 * 68 + 5])
    assert (cut.parity_present, cut.flags) == (3, lx.REPAIR_SIDECAR_TRUNCATED)
    for bad in (SIDE[:39], b"LACM" + SIDE[4:], rt.rehead(SIDE, version=3), SIDE[:9] + b"\xff" + SIDE[10:], rt.rehead(SIDE, S=72), rt.rehead(SIDE, r=33),
                rt.rehead(SIDE, K=255), rt.rehead(SIDE, L=0), rt.rehead(SIDE, k=geo.k - 1), rt.rehead(SIDE, G=1), SIDE[:50],
                SIDE[:37] + b"\x00\x00" + SIDE[39:], rt.rehead(SIDE, file_crc=7)):
        with pytest.raises(rt.Refused) as want:
            rt.parse(bad)
        with pytest.raises(ValueError) as got:
            lx.recovery_parse(bad)
        assert str(got.value) == str(want.value) and str(got.value).startswith("[recovery-error] ")
    assert lx.lib().lacx_recovery_parse(None, 0, None) == lx.E_INVALID and _last(pkg) == "[recovery-error] short input"


def test_argument_checks(pkg, dec):
    L, lx = pkg.lacx.lib(), pkg.lacx
    spans, _k = _spans(lx, [LAC])
    sides, _k2 = _spans(lx, [SIDE])
    out, rcs, res = (lx.Span * 1)(), (C.c_int * 1)(), (lx.RepairResult * 1)()
    prm = lx.RecoveryParams(0, 0, 0)
    for rc in (L.lacx_recovery_build_batch_view(None, spans, 1, C.byref(prm), out, rcs, None),
               L.lacx_recovery_scan_batch(None, spans, sides, 1, rcs, res, None),
               L.lacx_recovery_repair_batch_view(None, spans, sides, 1, 0, out, rcs, res, None)):
        assert rc == lx.E_INVALID and _last(pkg) == "null decoder"
    for rc in (L.lacx_recovery_build_batch_view(dec, spans, 0, C.byref(prm), out, rcs, None), L.lacx_recovery_build_batch_view(dec, None, 1, None, out, rcs, None),
               L.lacx_recovery_build_batch_view(dec, spans, 1, None, None, rcs, None), L.lacx_recovery_scan_batch(dec, spans, sides, 0, rcs, res, None),
               L.lacx_recovery_scan_batch(dec, spans, None, 1, rcs, res, None), L.lacx_recovery_scan_batch(dec, None, sides, 1, rcs, res, None),
               L.lacx_recovery_repair_batch_view(dec, spans, sides, 0, 0, out, rcs, res, None),
               L.lacx_recovery_repair_batch_view(dec, spans, sides, 1, 0, None, rcs, res, None)):
        assert rc == lx.E_INVALID and _last(pkg) == "null argument or empty batch"
    # parameters out of range refuse the whole call before anything else is looked at
    for (S, r, K), text in (((100, 2, 4), "slice_bytes 100 is not a multiple of 16 in 64..65536"), ((32, 0, 0), "slice_bytes 32 is not a multiple of 16 in 64..65536"),
                            ((0, 33, 0), "parity 33 is not in 1..32"), ((0, 0, 249), "group_data 249 is not in 1..256 - parity"), ((64, 32, 225), "group_data 225 is not in 1..256 - parity")):
        prm = lx.RecoveryParams(S, r, K)
        assert L.lacx_recovery_build_batch_view(dec, spans, 1, C.byref(prm), out, rcs, None) == lx.E_INVALID and _last(pkg) == "[recovery-error] " + text
        ptr, size = C.POINTER(C.c_uint8)(), C.c_uint64(5)
        assert L.lacx_recovery_build(dec, spans[0].data, len(LAC), C.byref(prm), C.byref(ptr), C.byref(size), None) == lx.E_INVALID
        assert not ptr and size.value == 0 and _last(pkg) == "[recovery-error] " + text
    ptr, count = C.POINTER(C.c_uint32)(), C.c_uint32(9)
    assert L.lacx_decoder_item_bad_slices(dec, 0, C.byref(ptr), C.byref(count)) == lx.E_INVALID and count.value == 0
    assert _last(pkg) == "no such item in the last recovery call"
    assert L.lacx_decoder_item_bad_slices(dec, 0, None, C.byref(count)) == lx.E_INVALID and _last(pkg) == "null argument"


def test_item_checks_before_the_device(pkg, dec):
    """A container the strict parser refuses (build) and a sidecar the recovery parser refuses (scan, repair) fail their
    item on the host with that parser's code and text; without a device the items that pass carry LACX_E_DEVICE."""
    L, lx = pkg.lacx.lib(), pkg.lacx
    have_device = lx.device_count() > 0
    junk = [LAC[:20], b"XX" + LAC[2:], b""]
    texts = []
    for x in junk:
        assert lx.stream_parse(x) is None
        texts.append(_last(pkg))
    files = junk + ([] if have_device else [LAC])
    n = len(files)
    spans, _k = _spans(lx, files)
    out, rcs = (lx.Span * n)(), (C.c_int * n)()
    rc = L.lacx_recovery_build_batch_view(dec, spans, n, None, out, rcs, None)
    assert [rcs[i] for i in range(3)] == [lx.E_INVALID] * 3 and [L.lacx_decoder_item_error(dec, i).decode() for i in range(3)] == texts
    assert all(not out[i].data and out[i].size == 0 for i in range(n))
    if have_device:
        assert rc == lx.E_INVALID and _last(pkg) == "stream 0: " + texts[0]
    else:
        assert rc == lx.E_DEVICE and rcs[3] == lx.E_DEVICE and _last(pkg) == "no usable HIP device"
        assert L.lacx_decoder_item_error(dec, 3).decode() == "no usable HIP device"
    bad_sides = [b"LACM" + SIDE[4:], SIDE[:60], rt.rehead(SIDE, file_crc=1), SIDE[:31]]
    want = ["[recovery-error] wrong magic", "[recovery-error] slice table is cut short",
            "[recovery-error] file_crc32 is not the combination of the slice checksums", "[recovery-error] short input"]
    sides = bad_sides + ([] if have_device else [SIDE])
    n = len(sides)
    fspans, _k1 = _spans(lx, [LAC] * n)
    sspans, _k2 = _spans(lx, sides)
    out, rcs, res = (lx.Span * n)(), (C.c_int * n)(), (lx.RepairResult * n)()
    for call in (lambda: L.lacx_recovery_scan_batch(dec, fspans, sspans, n, rcs, res, None),
                 lambda: L.lacx_recovery_repair_batch_view(dec, fspans, sspans, n, 0, out, rcs, res, None),
                 lambda: L.lacx_recovery_repair_batch_view(dec, fspans, sspans, n, lx.REPAIR_BEST_EFFORT, out, rcs, res, None)):
        rc = call()
        assert [rcs[i] for i in range(4)] == [lx.E_INVALID] * 4 and [L.lacx_decoder_item_error(dec, i).decode() for i in range(4)] == want
        assert all(bytes(res[i]) == bytes(48) for i in range(n)) and all(not out[i].data for i in range(n))
        ptr, count = C.POINTER(C.c_uint32)(), C.c_uint32(9)
        assert L.lacx_decoder_item_bad_slices(dec, n - 1, C.byref(ptr), C.byref(count)) == lx.OK and count.value == 0
        if have_device:
            assert rc == lx.E_INVALID and _last(pkg) == "stream 0: " + want[0]
        else:
            assert rc == lx.E_DEVICE and rcs[4] == lx.E_DEVICE and _last(pkg) == "no usable HIP device"
    # a batch of one carries its item's message without the "stream 0: "
    ptr, size, one = C.POINTER(C.c_uint8)(), C.c_uint64(), lx.RepairResult()
    rc = L.lacx_recovery_repair(dec, fspans[0].data, len(LAC), sspans[0].data, len(bad_sides[0]), 0, C.byref(ptr), C.byref(size), C.byref(one), None)
    assert rc == (lx.E_INVALID if have_device else lx.E_DEVICE) and not ptr and size.value == 0
    assert _last(pkg) == (want[0] if have_device else "no usable HIP device")
    d = lx.Decoder()
    if have_device:
        with pytest.raises(lx.BatchDecodeError) as e:
            d.repair_batch([LAC, LAC], bad_sides[:2])
        assert e.value.errors == {0: want[0], 1: want[1]} and e.value.results == [None, None]
        with pytest.raises(RuntimeError, match=r"^\[recovery-error\] wrong magic$"):
            d.repair(LAC, bad_sides[0])
    else:
        with pytest.raises(RuntimeError, match="no usable HIP device"):
            d.recovery(LAC)
        with pytest.raises(RuntimeError, match="no usable HIP device"):
            d.repair_batch([LAC], [SIDE])
    with pytest.raises(ValueError, match="one sidecar per file"):
        d.repair_batch([LAC], [])
    d.close()
