"""The stream inspection's entry points without a device: the new structs against the library's own sizeof,
lacx_inspect_combine against Python ints on the reference's rows (the 128-bit sum, a sub-range, lost rows), the checks of
the call's arguments, what a call does for its items before any device work, and the CLI's argument errors."""
import ctypes as C
import os
import re
import subprocess

import pytest

import __graft_entry__ as ge
import inspectcorpus as ic
import lacinspect as li

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("lacx_decoder_inspect_batch_device", "lacx_decoder_item_block_info", "lacx_decoder_item_partitions", "lacx_inspect_combine",
       "lacx_decoder_inspect_guard")


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


def _last_error(pkg):
    return pkg.lacx.lib().lacx_decode_last_error().decode()


def _spans(lx, lacs):
    bufs = [C.create_string_buffer(bytes(x), max(1, len(x))) for x in lacs]
    return bufs, (lx.Span * len(lacs))(*[lx.Span(C.cast(b, C.POINTER(C.c_uint8)), len(x)) for b, x in zip(bufs, lacs)])


def test_symbols_and_structs(pkg):
    L, lx = pkg.lacx.lib(), pkg.lacx
    header = open(os.path.join(ROOT, "include", "lacx.h")).read()
    for name in NEW:
        assert hasattr(L, name) and name in lx.EXPORTS
        assert re.search(rf"\b{name}\s*\(", header), name
        assert header.index(name) < header.index("#ifndef LACX_H"), name  # listed in the comment block at the top
    structs = lx.abi_structs()
    for name, cls, size in (("channel_info", lx.ChannelInfo, 160), ("block_info", lx.BlockInfo, 336), ("stream_report", lx.StreamReport, 456)):
        assert structs[name] is cls and L.lacx_sizeof(name.encode()) == C.sizeof(cls) == size, name
        assert "%d bytes" % size in header
    c, b = lx.ChannelInfo, lx.BlockInfo
    assert (c.coef.offset, c.bits.offset, c.rice_samples.offset, c.mode_parts.offset, c.unary_max.offset, c.sum_u.offset) == (8, 72, 100, 128, 144, 152)
    assert (b.frames.offset, b.bytes.offset, b.code.offset, b.ms.offset, b.channels.offset, b.ch.offset) == (0, 4, 8, 12, 13, 16)
    assert lx.INSPECT_PARTITIONS == 1 and "codes 5" in header.lower()


def _ctypes_rows(lx, rows):
    out = []
    for r in rows:
        x = lx.BlockInfo(r["frames"], r["bytes"], r["code"], r["ms"], r["channels"])
        for c in range(2):
            s, d = x.ch[c], r["ch"][c]
            for k in li.CH_SCALARS:
                setattr(s, k, d[k])
            for k in li.CH_ARRAYS:
                for j, v in enumerate(d[k]):
                    getattr(s, k)[j] = v
        out.append(x)
    return out


def test_combine_against_python(pkg):
    lx = pkg.lacx
    for name, lac in ic.pinned()[:6] + ic.small()[:4]:
        rows = ic.expected(lac)
        info = lx.stream_parse(lac)
        got = lx.inspect_combine(_ctypes_rows(lx, rows), info)
        assert li.report_from_ctypes(got) == li.report(rows, (lac[2], lac[3], lac[4], info.sample_rate, lac[8], len(rows))), name
        assert got.head_bytes + got.payload_bytes == len(lac) and got.samples == info.frames * info.channels
        assert abs(got.bits_per_sample - 8.0 * got.payload_bytes / got.samples) < 1e-12 and abs(sum(got.shares.values()) - 1.0) < 1e-9
    # a sub-range without the stream's info, lost rows among it, and a sum that needs the second word
    rows = [dict(r) for r in ic.expected(ic.pinned()[0][1])] * 3
    rows[1] = li.lost_row(rows[1]["frames"], rows[1]["bytes"], 3)
    rows.append(li.lost_row(77, 5, 10))
    big = dict(rows[0], ch=[dict(rows[0]["ch"][0], sum_u=(1 << 64) - 5), dict(rows[0]["ch"][1], sum_u=(1 << 63) + 9)])
    rows += [big, big]
    got = lx.inspect_combine(_ctypes_rows(lx, rows))
    want = li.report(rows)
    assert li.report_from_ctypes(got) == want and want["sum_u"] >> 64 and got.lost_blocks == 2 and got.head_bytes == 0
    sub = lx.inspect_combine(_ctypes_rows(lx, rows[2:5]))
    assert li.report_from_ctypes(sub) == li.report(rows[2:5])
    empty = lx.inspect_combine([])
    assert empty.blocks == 0 and empty.k_min == 255 and empty.k_max == 0
    L = lx.lib()
    assert L.lacx_inspect_combine(None, C.c_uint32(1), None, C.byref(lx.StreamReport())) == lx.E_INVALID
    assert L.lacx_inspect_combine(None, C.c_uint32(0), None, None) == lx.E_INVALID


def test_argument_checks_and_host_side_outcomes(pkg, dec):
    """Null arguments, an empty batch and an unknown flag are the call's own errors; without a device every item is parsed
    and keeps its own outcome, then the call as a whole ends with LACX_E_DEVICE, zeroed reports and no rows."""
    L, lx = pkg.lacx.lib(), pkg.lacx
    good = ic.small()[0][1]
    bufs, spans = _spans(lx, [good, b"LA\x03\x02", good[:13], b""])
    n = 4
    rcs, out, ms = (C.c_int * n)(), (lx.StreamReport * n)(), C.c_float(7.0)
    assert L.lacx_decoder_inspect_batch_device(None, spans, C.c_uint32(n), C.c_uint32(0), None, rcs, out, None) == lx.E_INVALID
    assert L.lacx_decoder_inspect_batch_device(dec, None, C.c_uint32(n), C.c_uint32(0), None, rcs, out, None) == lx.E_INVALID
    assert L.lacx_decoder_inspect_batch_device(dec, spans, C.c_uint32(0), C.c_uint32(0), None, rcs, out, None) == lx.E_INVALID
    assert L.lacx_decoder_inspect_batch_device(dec, spans, C.c_uint32(n), C.c_uint32(2), None, rcs, out, None) == lx.E_INVALID
    assert "flag" in _last_error(pkg)
    guarded, changed = C.c_uint64(5), C.c_uint64(5)
    assert L.lacx_decoder_inspect_guard(dec, C.byref(guarded), C.byref(changed)) == lx.OK and (guarded.value, changed.value) == (0, 0)
    assert L.lacx_decoder_inspect_guard(dec, None, C.byref(changed)) == lx.E_INVALID
    rows, count = C.POINTER(lx.BlockInfo)(), C.c_uint32(9)
    assert L.lacx_decoder_item_block_info(dec, C.c_uint32(0), C.byref(rows), C.byref(count)) == lx.E_INVALID and count.value == 0
    if lx.device_count() > 0:  # with a device: only the refused containers, so that nothing runs on it
        rc = L.lacx_decoder_inspect_batch_device(dec, C.cast(C.byref(spans, C.sizeof(lx.Span)), C.POINTER(lx.Span)), C.c_uint32(3), C.c_uint32(0), None,
                                                 rcs, out, C.byref(ms))
        assert rc == lx.E_INVALID and _last_error(pkg).startswith("stream 0: ") and list(rcs)[:3] == [lx.E_INVALID] * 3
        assert bytes(out) == bytes(C.sizeof(out)) and ms.value == 0.0
        return
    for flags in (0, lx.INSPECT_PARTITIONS):
        rc = L.lacx_decoder_inspect_batch_device(dec, spans, C.c_uint32(n), C.c_uint32(flags), None, rcs, out, C.byref(ms))
        assert rc == lx.E_DEVICE and "no usable HIP device" in _last_error(pkg) and ms.value == 0.0
        assert list(rcs) == [lx.E_DEVICE, lx.E_INVALID, lx.E_INVALID, lx.E_INVALID]
        assert "invalid frame header" in L.lacx_decoder_item_error(dec, 1).decode() and "empty input" in L.lacx_decoder_item_error(dec, 3).decode()
        assert bytes(out) == bytes(C.sizeof(out))
        for i in range(n):
            assert L.lacx_decoder_item_block_info(dec, C.c_uint32(i), C.byref(rows), C.byref(count)) == lx.OK and count.value == 0
        mk, pb = C.POINTER(C.c_uint8)(), C.POINTER(C.c_uint32)()
        assert L.lacx_decoder_item_partitions(dec, C.c_uint32(0), C.c_uint32(0), C.c_uint32(0), C.byref(mk), C.byref(pb), C.byref(count)) == lx.E_INVALID
    # the null arrays are allowed
    assert L.lacx_decoder_inspect_batch_device(dec, spans, C.c_uint32(n), C.c_uint32(0), None, None, None, None) == lx.E_DEVICE
    with pytest.raises(RuntimeError, match="no usable HIP device"):
        lx.Decoder().inspect_batch([good])


def test_cli_argument_errors(pkg, tmp_path):
    cli = os.path.join(os.path.dirname(pkg.lacx.LIB_PATH), "lacx_cli")
    run = lambda *a: subprocess.run([cli, "inspect", *a], capture_output=True, text=True)  # noqa: E731
    res = run()
    assert res.returncode == 1 and "lacx_cli inspect FILE... [--blocks] [--partitions]" in res.stderr
    res = run("--blocks")
    assert res.returncode == 1 and "Usage" in res.stderr
    res = run("--nonsense", "x.lac")
    assert res.returncode == 1 and "unknown option --nonsense" in res.stderr
    bad = tmp_path / "bad.lac"
    bad.write_bytes(b"LA\x03\x02")
    res = run(str(tmp_path / "absent.lac"), str(bad))
    assert res.returncode == 1 and "Failed to read file" in res.stderr and "invalid frame header" in res.stderr and res.stdout == ""
