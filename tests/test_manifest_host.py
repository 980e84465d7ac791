"""Manifests and the block digest entry points without a device: lacx_manifest_build / lacx_manifest_parse against a
restatement of the format with struct (tests/blockdigesttwin.py), every refusal of the parser, the new structs, and the
checks of the call's arguments and of every item -- container, manifest, format -- which run on the host before any device
call."""
import ctypes as C
import os
import re
import struct
import zlib

import numpy as np
import pytest

import __graft_entry__ as ge
import blockdigesttwin as bt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NEW = ("lacx_decoder_digest_blocks_batch_device", "lacx_decoder_item_block_digests", "lacx_decoder_digest_pcm_blocks_batch_device",
       "lacx_manifest_build", "lacx_manifest_parse", "lacx_decoder_check_batch_device",
       "lacx_decoder_salvage_wav_batch_view_checked", "lacx_decoder_salvage_batch_device_checked")
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


def _pcm(frames, depth, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(-(1 << (depth - 1)), 1 << (depth - 1), frames, dtype=np.int64).astype(np.int32)


def _source(channels, depth, frames, grid, seed=1):
    """(left, right, blocks, crcs, whole): PCM, its grid, zlib's CRC-32 per block and of the whole data chunk."""
    left, right = _pcm(frames, depth, seed), _pcm(frames, depth, seed + 1) if channels == 2 else None
    blocks = [min(grid, frames - a) for a in range(0, frames, grid)]
    return left, right, blocks, bt.block_crcs(left, right, depth, blocks), zlib.crc32(bt.data_bytes(left, right, depth))


def _digest(lx, channels, depth, rate, frames, whole):
    return lx.Digest(whole, 0, frames, frames * channels * (depth // 8), rate, channels, depth, 1, 0)


def test_symbols_and_structs(pkg):
    L, lx = pkg.lacx.lib(), pkg.lacx
    header = open(os.path.join(ROOT, "include", "lacx.h")).read()
    for name in NEW:
        assert hasattr(L, name) and name in lx.EXPORTS
        assert re.search(rf"\b{name}\s*\(", header), name
        assert header.index(name) < header.index("#ifndef LACX_H"), name  # listed in the comment block at the top
    assert "#define LACX_BLOCK_DIGEST 11u" in header and lx.BLOCK_DIGEST == 11
    assert lx.block_fault_text(11) == "digest mismatch" and lx.block_fault_text(10) == "payload missing" and lx.block_fault_text(12) == "?"
    assert lx.abi_structs()["block_digest"] is lx.BlockDigest and lx.abi_structs()["manifest_info"] is lx.ManifestInfo
    assert L.lacx_sizeof(b"block_digest") == C.sizeof(lx.BlockDigest) == 16
    assert L.lacx_sizeof(b"manifest_info") == C.sizeof(lx.ManifestInfo) == 24
    b, m = lx.BlockDigest, lx.ManifestInfo
    assert (b.frames.offset, b.crc32.offset, b.code.offset, b.reserved.offset) == (0, 4, 8, 12)
    assert (m.sample_rate.offset, m.blocks.offset, m.frames.offset, m.data_crc32.offset, m.channels.offset, m.bit_depth.offset) == (0, 4, 8, 16, 20, 21)


@pytest.mark.parametrize("channels,depth,rate,frames,grid", [(2, 16, 48000, 3 * 16384 + 1234, 16384), (1, 24, 96000, 16385, 16384),
                                                            (2, 24, 44100, 1, 16384), (1, 16, 192000, 774, 257), (2, 16, 48000, 2000, 1000)])
def test_build_and_parse_against_the_restatement(pkg, channels, depth, rate, frames, grid):
    """The manifest of source PCM on a grid, rows and whole-chunk CRC from zlib: the library's bytes are the restatement's,
    its parse gives the fields back, and data_crc32 is zlib's of the whole chunk."""
    lx = pkg.lacx
    _, _, blocks, crcs, whole = _source(channels, depth, frames, grid)
    rows = [lx.BlockDigest(n, c, 0, 0) for n, c in zip(blocks, crcs)]
    want = bt.manifest_of(channels, depth, rate, frames, list(zip(blocks, crcs)))
    got = lx.manifest_build(_digest(lx, channels, depth, rate, frames, whole), rows)
    assert got == want and len(got) == 32 + 8 * len(blocks)
    assert struct.unpack(">I", got[24:28])[0] == whole  # the restatement's combination is zlib's CRC of the whole chunk
    info, back = lx.manifest_parse(got)
    assert (info.channels, info.bit_depth, info.sample_rate, info.frames, info.blocks, info.data_crc32) == (channels, depth, rate, frames, len(blocks), whole)
    assert [(r.frames, r.crc32, r.code) for r in back] == [(n, c, 0) for n, c in zip(blocks, crcs)]
    # rows nullable
    buf = (C.c_uint8 * len(got)).from_buffer_copy(got)
    info2 = lx.ManifestInfo()
    assert lx.lib().lacx_manifest_parse(buf, len(got), C.byref(info2), None, 0) == lx.OK and info2.blocks == len(blocks)
    assert lx.lib().lacx_manifest_parse(buf, len(got), None, None, 0) == lx.OK
    # the twin's copy of csrc/manifest.h agrees
    rc, _, d, trows = bt.twin_manifest_parse(got)
    assert rc == 0 and d["data_crc32"] == whole and [r[:2] for r in trows] == list(zip(blocks, crcs))


def _resum(body):
    return body[:-4] + struct.pack(">I", zlib.crc32(body[:-4]))


def test_every_refusal(pkg):
    """One input per refusal; every message starts "[manifest-error] "."""
    lx = pkg.lacx
    _, _, blocks, crcs, whole = _source(2, 16, 48000 // 48 + 600, 512)  # 1600 frames: 512, 512, 512, 64
    good = bt.manifest_of(2, 16, 48000, 1600, list(zip(blocks, crcs)))
    assert lx.manifest_parse(good)[0].blocks == 4

    def patched(at, data, resum=True):
        m = good[:at] + data + good[at + len(data):]
        return _resum(m) if resum else m

    def with_rows(rows, frames=1600, fix_data=True):
        return bt.manifest_of(2, 16, 48000, frames, rows)

    bad = {
        "short input": good[:31],
        "wrong magic": patched(0, b"LACX"),
        "wrong version": patched(4, b"\x02"),
        "size": _resum(good + bytes(8))[:-12] + _resum(good + bytes(8))[-4:],
        "own checksum": patched(29, bytes([good[29] ^ 1]), resum=False),
        "channels": patched(5, b"\x03"),
        "bit depth": patched(6, b"\x08"),
        "sample rate": patched(8, struct.pack(">I", 22050)),
        "blocks = 0": _resum(good[:20] + struct.pack(">I", 0) + good[24:28] + bytes(4)),
        "row of 0 frames": with_rows([(512, crcs[0]), (0, 0), (512, crcs[2]), (576, crcs[3])]),
        "row above 16384": with_rows([(16385, crcs[0])], frames=16385),
        "short non-final row": with_rows([(255, crcs[0]), (1345, crcs[1])]),
        "sum": patched(12, struct.pack(">Q", 1601)),
        "data_crc32": patched(24, struct.pack(">I", whole ^ 1)),
    }
    seen = set()
    for what, m in bad.items():
        with pytest.raises(ValueError, match=r"^\[manifest-error\] ") as e:
            lx.manifest_parse(m)
        rc, msg, _, _ = bt.twin_manifest_parse(m)
        assert rc == lx.E_INVALID and msg == str(e.value), what
        seen.add(str(e.value).split(":")[0].rstrip("0123456789 "))
        print(what, "->", e.value)
    assert len(seen) >= 12, seen  # the refusals are told apart
    with pytest.raises(ValueError, match=r"^\[manifest-error\] short input$"):
        lx.manifest_parse(b"")


def test_build_refuses_lost_blocks_and_rows_that_do_not_fit(pkg):
    lx = pkg.lacx
    _, _, blocks, crcs, whole = _source(1, 16, 1000, 256)
    rows = [lx.BlockDigest(n, c, 0, 0) for n, c in zip(blocks, crcs)]
    d = _digest(lx, 1, 16, 48000, 1000, whole)
    assert lx.manifest_build(d, rows) == bt.manifest_of(1, 16, 48000, 1000, list(zip(blocks, crcs)))
    lost = [lx.BlockDigest(r.frames, r.crc32, r.code, 0) for r in rows]
    lost[2].code, lost[2].crc32 = 3, 0
    with pytest.raises(ValueError, match=r"^manifest needs every block's digest: block 2 is lost$"):
        lx.manifest_build(d, lost)
    with pytest.raises(ValueError, match=r"^\[manifest-error\] "):  # the rows hold other frames than the digest
        lx.manifest_build(_digest(lx, 1, 16, 48000, 1001, whole), rows)
    with pytest.raises(ValueError, match=r"^\[manifest-error\] data_crc32"):
        lx.manifest_build(_digest(lx, 1, 16, 48000, 1000, whole ^ 2), rows)
    out, size = C.POINTER(C.c_uint8)(), C.c_uint64(7)
    assert lx.lib().lacx_manifest_build(C.byref(d), None, 4, C.byref(out), C.byref(size)) == lx.E_INVALID and size.value == 0


def test_whole_call_arguments(pkg, dec):
    L, lx = pkg.lacx.lib(), pkg.lacx
    lac = _fixture("small/n257_st16_ms.lac")
    buf = (C.c_uint8 * len(lac)).from_buffer_copy(lac)
    spans = (lx.Span * 1)(lx.Span(C.cast(buf, C.POINTER(C.c_uint8)), len(lac)))
    none = (lx.Span * 1)(lx.Span(None, 0))
    items = (lx.DecodeItem * 1)()
    srcs = (lx.DigestSource * 1)(lx.DigestSource(lx.Pcm(FAKE, FAKE, lx.PCM_PLANAR_I32, 2), 257, 48000, 16))
    calls = {
        "digest_blocks": lambda d, a, n: L.lacx_decoder_digest_blocks_batch_device(d, a and spans, n, None, None, None, None),
        "check": lambda d, a, n: L.lacx_decoder_check_batch_device(d, a and spans, none, n, None, None, None, None),
        "check (no manifests)": lambda d, a, n: L.lacx_decoder_check_batch_device(d, spans, a and none, n, None, None, None, None),
        "wav_checked": lambda d, a, n: L.lacx_decoder_salvage_wav_batch_view_checked(d, a and spans, none, n, (lx.Span * 1)(), None, None, None),
        "device_checked": lambda d, a, n: L.lacx_decoder_salvage_batch_device_checked(d, a and items, none, n, None, None, None, None),
        "pcm_blocks": lambda d, a, n: L.lacx_decoder_digest_pcm_blocks_batch_device(d, a and srcs, n, 0, None, None, None, None),
    }
    for name, call in calls.items():
        assert call(dec, True, 0) == lx.E_INVALID and _last_error(pkg) == "null argument or empty batch", name
        assert call(dec, None, 1) == lx.E_INVALID and _last_error(pkg) == "null argument or empty batch", name
        assert call(None, True, 1) == lx.E_INVALID and _last_error(pkg) == "null decoder", name
    for grid in (1, 255, 16385, 1 << 31):
        assert L.lacx_decoder_digest_pcm_blocks_batch_device(dec, srcs, 1, grid, None, None, None, None) == lx.E_INVALID
        assert _last_error(pkg) == "block_frames must be 0 or 256..16384"
    rows, count = C.POINTER(lx.BlockDigest)(), C.c_uint32(5)
    assert L.lacx_decoder_item_block_digests(dec, 0, C.byref(rows), C.byref(count)) == lx.E_INVALID and count.value == 0
    assert _last_error(pkg) == "no such item in the last block digest call"
    d = lx.Decoder()
    for call in (lambda: d.digest_blocks_batch([]), lambda: d.check_batch([], []), lambda: d.digest_pcm_blocks_batch([]),
                 lambda: d.digest_pcm_blocks_batch([((FAKE, FAKE, 0, 2, 257), 48000, 16)], block_frames=100)):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(ValueError, match="one manifest"):
        d.check_batch([lac], [])
    d.close()


def test_item_checks_before_the_device(pkg, dec):
    """Container, manifest and format are judged per item on the host; without a device the items that pass carry
    LACX_E_DEVICE.  (With a device only items that fail on the host are in the batch, so that nothing runs on it.)"""
    L, lx = pkg.lacx.lib(), pkg.lacx
    have_device = lx.device_count() > 0
    st16, mono = _fixture("small/n257_st16_ms.lac"), _fixture("small/n33_mono16.lac")
    # manifests with made-up CRCs: the format checks never look at them
    man16 = bt.manifest_of(2, 16, 48000, 257, [(257, 1)])
    info = lx.stream_parse(st16)
    assert (info.channels, info.bit_depth, info.frames, info.blocks) == (2, 16, 257, 1)
    man16 = bt.manifest_of(2, 16, info.sample_rate, 257, [(257, 1)])
    cases = [  # (stream, manifest, code, message)
        (b"XX" + st16[2:], man16, lx.E_INVALID, "[decode-error] invalid frame header"),
        (st16, man16[:-1], lx.E_INVALID, "[manifest-error] size is not 32 + 8 * blocks"),
        (st16, bt.manifest_of(1, 16, info.sample_rate, 257, [(257, 1)]), lx.E_MISMATCH, "[check-error] channels: stream 2, manifest 1"),
        (st16, bt.manifest_of(2, 24, info.sample_rate, 257, [(257, 1)]), lx.E_MISMATCH, "[check-error] bit depth: stream 16, manifest 24"),
        (st16, bt.manifest_of(2, 16, 192000 if info.sample_rate != 192000 else 48000, 257, [(257, 1)]), lx.E_MISMATCH,
         "[check-error] sample rate: stream %d, manifest %d" % (info.sample_rate, 192000 if info.sample_rate != 192000 else 48000)),
        (st16, bt.manifest_of(2, 16, info.sample_rate, 258, [(258, 1)]), lx.E_MISMATCH, "[check-error] frames: stream 257, manifest 258"),
        (st16, bt.manifest_of(2, 16, info.sample_rate, 257, [(256, 1), (1, 2)]), lx.E_MISMATCH, "[check-error] blocks: stream 1, manifest 2"),
    ]
    three = _fixture("decode_wav/st16_lr_3blk.lac")
    i3 = lx.stream_parse(three)
    fr = [int(struct.unpack(">I", three[14 + 8 * b:18 + 8 * b])[0]) for b in range(i3.blocks)]
    moved = [fr[0] - 1, fr[1], fr[2] + 1]  # (the last block is shorter than 16384)
    cases.append((three, bt.manifest_of(i3.channels, i3.bit_depth, i3.sample_rate, i3.frames, [(n, 1) for n in moved]), lx.E_MISMATCH,
                  "[check-error] block 0 frames: stream %d, manifest %d" % (fr[0], moved[0])))
    if not have_device:
        cases += [(st16, man16, lx.E_DEVICE, "no usable HIP device"), (mono, None, lx.E_DEVICE, "no usable HIP device")]
    n = len(cases)
    keep = [(C.c_uint8 * len(x)).from_buffer_copy(x) for x, _, _, _ in cases]
    mkeep = [None if m is None else (C.c_uint8 * len(m)).from_buffer_copy(m) for _, m, _, _ in cases]
    spans = (lx.Span * n)(*[lx.Span(C.cast(b, C.POINTER(C.c_uint8)), len(b)) for b in keep])
    mspans = (lx.Span * n)(*[lx.Span(None, 0) if b is None else lx.Span(C.cast(b, C.POINTER(C.c_uint8)), len(b)) for b in mkeep])
    items = (lx.DecodeItem * n)()
    for it, b in zip(items, keep):
        it.lac, it.size, it.left, it.right, it.frames = C.cast(b, C.POINTER(C.c_uint8)), len(b), FAKE, FAKE, lx.stream_scan(bytes(b))[0].frames if lx.stream_scan(bytes(b)) else 0
    outs = (lx.Span * n)()
    for name, call in (("check", lambda rcs, res, ms: L.lacx_decoder_check_batch_device(dec, spans, mspans, n, None, rcs, res, ms)),
                       ("wav", lambda rcs, res, ms: L.lacx_decoder_salvage_wav_batch_view_checked(dec, spans, mspans, n, outs, rcs, res, ms)),
                       ("device", lambda rcs, res, ms: L.lacx_decoder_salvage_batch_device_checked(dec, items, mspans, n, None, rcs, res, ms))):
        rcs = (C.c_int * n)(*([-1] * n))
        res = (lx.SalvageResult * n)(*[lx.SalvageResult(9, 9, 9, 9, 9, 9) for _ in range(n)])
        ms = C.c_float(5.0)
        rc = call(rcs, res, C.byref(ms))
        assert ms.value == 0.0
        for i, (_, _, code, msg) in enumerate(cases):
            assert rcs[i] == code and L.lacx_decoder_item_error(dec, i).decode() == msg, (name, i, L.lacx_decoder_item_error(dec, i).decode())
            assert bytes(res[i]) == bytes(32), (name, i)
            assert name != "wav" or not outs[i].data
        if have_device:
            assert rc == lx.E_INVALID and _last_error(pkg) == "stream 0: [decode-error] invalid frame header", name
        else:
            assert rc == lx.E_DEVICE and _last_error(pkg) == "no usable HIP device", name
    # digest_blocks: lenient like salvage -- a truncated stream is no refusal
    lacs = [b"XX" + st16[2:]] + ([] if have_device else [st16[:-1]])
    keep2 = [(C.c_uint8 * len(x)).from_buffer_copy(x) for x in lacs]
    sp2 = (lx.Span * len(lacs))(*[lx.Span(C.cast(b, C.POINTER(C.c_uint8)), len(b)) for b in keep2])
    rcs = (C.c_int * len(lacs))()
    out = (lx.Digest * len(lacs))(*[lx.Digest(9, 9, 9, 9, 9, 9, 9, 9, 9) for _ in lacs])
    rc = L.lacx_decoder_digest_blocks_batch_device(dec, sp2, len(lacs), None, rcs, out, None)
    assert rcs[0] == lx.E_INVALID and L.lacx_decoder_item_error(dec, 0).decode() == "[decode-error] invalid frame header"
    assert all(bytes(o) == bytes(32) for o in out)
    if not have_device:
        assert rc == lx.E_DEVICE and rcs[1] == lx.E_DEVICE
    d = lx.Decoder()
    if have_device:
        with pytest.raises(lx.BatchDecodeError) as e:
            d.check_batch([c[0] for c in cases[:3]], [c[1] for c in cases[:3]])
        assert e.value.errors == {i: cases[i][3] for i in range(3)} and e.value.results == [None] * 3
        with pytest.raises(RuntimeError, match=r"^\[check-error\] channels: stream 2, manifest 1$"):
            d.salvage_wav(st16, manifests=cases[2][1])
    else:
        with pytest.raises(RuntimeError, match="no usable HIP device"):
            d.check_batch([st16], [man16])
        with pytest.raises(RuntimeError, match="no usable HIP device"):
            d.manifest(st16)
    d.close()


def test_source_checks_are_the_digest_forms(pkg, dec):
    """digest_pcm_blocks judges every item as lacx_decoder_digest_pcm_batch_device does: the same texts."""
    L, lx = pkg.lacx.lib(), pkg.lacx
    have_device = lx.device_count() > 0
    P = lx.PCM_PLANAR_I32
    cases = [(None, FAKE, P, 2, 257, 48000, 16, "source arrays missing"), (FAKE, FAKE, 3, 2, 257, 48000, 16, "unknown source layout"),
             (FAKE, FAKE, P, 3, 257, 48000, 16, "unsupported channel count"), (FAKE, FAKE, P, 2, 0, 48000, 16, "source has no frames"),
             (FAKE, FAKE, P, 2, 1 << 56, 48000, 16, "source frame count out of range"), (FAKE, FAKE, P, 2, 257, 22050, 16, "unsupported sample rate: 22050"),
             (FAKE, FAKE, P, 2, 257, 48000, 8, "unsupported bit depth: 8"), (FAKE + 2, FAKE, P, 2, 257, 48000, 16, "source arrays are not 4-byte aligned"),
             (FAKE, None, lx.PCM_INTERLEAVED_I24, 2, 257, 48000, 16, "source layout does not match the stream's bit depth")]
    n = len(cases)
    items = (lx.DigestSource * n)()
    for k, (d0, d1, layout, ch, frames, rate, depth, _) in enumerate(cases):
        items[k] = lx.DigestSource(lx.Pcm(d0, d1, layout, ch), frames, rate, depth)
    for fn, extra in ((L.lacx_decoder_digest_pcm_blocks_batch_device, (C.c_uint32(1000),)), (L.lacx_decoder_digest_pcm_batch_device, ())):
        rcs = (C.c_int * n)(*([-1] * n))
        out = (lx.Digest * n)(*[lx.Digest(9, 9, 9, 9, 9, 9, 9, 9, 9) for _ in range(n)])
        rc = fn(dec, items, n, *extra, None, rcs, out, None)
        for i, case in enumerate(cases):
            assert rcs[i] == lx.E_INVALID and L.lacx_decoder_item_error(dec, i).decode() == case[7], i
            assert bytes(out[i]) == bytes(32), i
        assert rc == (lx.E_INVALID if have_device else lx.E_DEVICE)
