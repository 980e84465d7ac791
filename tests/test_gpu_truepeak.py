"""True peak on the MI355X: lacx_decoder_truepeak_batch_device, lacx_decoder_truepeak_pcm_batch_device, lacx_truepeak_combine
and `lacx_cli peak`.  The device's rows are held to the plain CPU twin's (tests/native/sim_truepeak.cpp) and to the numpy
restatement (tests/peaktwin.py) BYTE FOR BYTE: the Annex 2 filter is exact in integers, there is no tolerance.  Only shapes
the sanitized twin has passed in this run go to the device: every corpus shape as a source job (k_truepeak runs over planar
int32, which is what it sees behind a decode), and as stream jobs the streams of up to 16400 frames, the spliced ones and the
damaged one; the decode in front of the larger streams is the decoder's own, which its own tests cover."""
import math
import os
import subprocess

import numpy as np
import pytest

import __graft_entry__ as ge
import lacmutate
import lacstreams
import peaktwin as pt
import statstwin as sw

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
PKG_DIR = os.path.join(ROOT, "lossless-audio-codec_amd")
P32, I16, I24, P16, PF32, IF32 = 0, 1, 2, 16, 17, 18


@pytest.fixture(scope="module")
def gpu():
    pkg = ge.load_pkg()
    if pkg.lacx.device_count() <= 0:
        pytest.fail("no HIP device: the decoder has no CPU fallback")
    return pkg


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


def _fixture(name):
    with open(os.path.join(GOLDEN, name), "rb") as f:
        return f.read()


def _spec(it, layout=P32, offset=0, bad=None):
    return pt.SourceSpec(layout, it.channels, it.depth, it.rate, offset, it.left, it.right, bad)


def _small(it):
    return len(it.left) <= 16400


@pytest.fixture(scope="module")
def twin_rows():
    """{item name: SourceOut of the plain twin}: the whole corpus as one source job, computed once."""
    items = pt.corpus()
    return {it.name: out for it, out in zip(items, pt.run_sources([_spec(it) for it in items]))}


@pytest.fixture(scope="module")
def streams(gpu, oracle, twin_rows):
    """[(stream, Item)]: the whole corpus through the product's encoder, and per format the spliced stream of 257 / 258 / 259
    -frame blocks with its version-2 form -- once the sanitized twin has passed their shapes."""
    encoders = {(ch, depth, rate): gpu.lacx.Encoder(12, 2 if ch == 2 else 0, rate, depth, device=0)
                for ch, depth, rate in {(it.channels, it.depth, it.rate) for it in pt.corpus()}}
    out = [(encoders[(it.channels, it.depth, it.rate)].encode(it.left, it.right), it) for it in pt.corpus()]
    for ch, depth, rate in pt.FORMATS:
        parts = sw.spliced_parts(ch, depth)
        lacs = [oracle.encode(l, r, rate, depth, 0) for l, r in parts]
        it = pt.Item("splice|%dch%d" % (ch, depth), ch, depth, rate, np.concatenate([l for l, _ in parts]),
                     np.concatenate([r for _, r in parts]) if ch == 2 else None)
        lac = lacstreams.splice(lacstreams.splice(lacs[0], lacs[1]), lacs[2])
        out += [(lac, it), (lacstreams.to_v2(lac), it)]
        (twin_rows[it.name],) = pt.run_sources([_spec(it)])
    pt.cleared("gpu-corpus", [lac for lac, it in out if _small(it)], sources=[_spec(it) for it in pt.corpus()])  # CPU first
    return out


def _check(what, got, it, twin, lx):
    """One item of a true-peak call: rows byte-equal to the twin's and to the restatement's, totals byte-equal to
    truepeak_combine of the rows and equal to the twin's."""
    peak, rows = got
    rows = pt.rows_of(rows)
    assert rows.shape == twin.rows.shape and rows.tobytes() == twin.rows.tobytes() == pt.item_rows(it).tobytes(), what
    assert bytes(peak) == bytes(lx.truepeak_combine([(rows.tobytes(), it.channels, it.depth, len(it.left), it.rate)])), what
    assert pt.totals_of(peak) == twin.totals, what
    pt.same_totals(pt.totals_of(peak), pt.item_totals(it))
    assert peak.sample_rate == it.rate and peak.channels == it.channels and peak.bit_depth == it.depth and peak.frames == len(it.left)


@pytest.mark.parametrize("reverse", [False, True])
def test_the_corpus_in_one_batch(gpu, streams, twin_rows, reverse):
    """One batch of the whole corpus and the spliced streams, forward and reversed: items start at other places of the job;
    the row grid counts in the item's frames whatever the container's blocks are, so a spliced stream of 257 / 258 / 259
    -frame blocks and its version-2 form give the rows of the same PCM in 16384-frame blocks."""
    dec = gpu.lacx.Decoder(device=0)
    order = streams[::-1] if reverse else streams
    got = dec.truepeak_batch([lac for lac, _ in order])
    assert dec.last_ms > 0
    for (lac, it), g in zip(order, got):
        _check(it.name, g, it, twin_rows[it.name], gpu.lacx)
    one = dec.truepeak(order[0][0])
    assert bytes(one) == bytes(got[0][0])
    dec.close()


def _data_bytes(left, right, depth) -> bytes:
    a = np.asarray(left, np.int32) if right is None else np.stack([np.asarray(left, np.int32), np.asarray(right, np.int32)], 1).ravel()
    if depth == 16:
        return a.astype("<i2").tobytes()
    return np.ascontiguousarray(a.astype("<i4").view(np.uint8).reshape(-1, 4)[:, :3]).tobytes()


def _arrays(left, right, bits, layout):
    """The source's arrays as bytes: one for an interleaved layout, one per channel for a planar one."""
    chans = [left] if right is None else [left, right]
    if layout in (PF32, IF32):
        chans = [(x.astype(np.float32) / np.float32(1 << (bits - 1))) for x in chans]
    elif layout in (I16, P16):
        chans = [x.astype("<i2") for x in chans]
    if layout == I24:
        return [_data_bytes(left, right, 24)]
    if layout in (I16, IF32):
        return [np.stack(chans, axis=1).tobytes()]
    return [x.astype(x.dtype.newbyteorder("<")).tobytes() for x in chans]


def _upload(torch, raw: bytes, offset=0):
    """raw at `offset` bytes behind the start of a device buffer that ends with it."""
    buf = torch.zeros(offset + len(raw), dtype=torch.uint8, device="cuda")
    buf[offset:] = torch.frombuffer(bytearray(raw), dtype=torch.uint8).cuda()
    return buf


LAYOUTS = {16: (P32, I16, P16, PF32, IF32), 24: (P32, I24, PF32, IF32)}


def test_source_form_in_all_six_layouts(gpu, torch, twin_rows):
    """Device-resident PCM in every layout (a float32 source among them), in buffers that end with the source's last byte,
    at base offsets of 0 and 4 bytes: the rows are the twin's byte for byte, whatever the layout."""
    dec = gpu.lacx.Decoder(device=0)
    picks = [it for it in pt.corpus() if it.name.startswith(("noise|n13|", "noise|n1014|", "noise|n16385|", "worst|pos", "dc|", "impulse|ends16384"))]
    assert len(picks) == 12 + 6 and {x for b in LAYOUTS.values() for x in b} == {P32, I16, I24, P16, PF32, IF32}
    items, wants, keep = [], [], []
    for it in picks:
        for layout in LAYOUTS[it.depth]:
            for offset in (0, 4):
                bufs = [_upload(torch, raw, offset) for raw in _arrays(it.left, it.right, it.depth, layout)]
                keep.append(bufs)
                ptrs = [b.data_ptr() + offset for b in bufs]
                items.append(((ptrs[0], ptrs[1] if len(ptrs) == 2 else None, layout, it.channels, len(it.left)), it.rate, it.depth))
                wants.append(it)
    pt.cleared("gpu-layouts", [], sources=[_spec(it, layout, offset) for it in picks for layout in LAYOUTS[it.depth] for offset in (0, 4)])  # CPU first
    got = dec.truepeak_pcm_batch(items)
    assert dec.last_ms > 0
    for k, (g, it) in enumerate(zip(got, wants)):
        _check((it.name, k), g, it, twin_rows[it.name], gpu.lacx)
    dec.close()


def test_a_silent_item_between_two_full_scale_ones(gpu, torch):
    """History in front of frame 0 and samples behind the last frame are zeros, never the neighbouring item's PCM: as
    sources in one allocation, and as streams, whose PCM lies side by side in the decoder's own buffers."""
    loud = pt.Item("loud", 2, 24, 48000, np.full(1500, -(1 << 23), np.int32), np.full(1500, (1 << 23) - 1, np.int32))
    quiet = pt.Item("quiet", 2, 24, 48000, np.zeros(1030, np.int32), np.zeros(1030, np.int32))
    trio = [loud, quiet, loud]
    enc = gpu.lacx.Encoder(12, 2, 48000, 24, device=0)
    lacs = pt.cleared("gpu-silent", [enc.encode(it.left, it.right) for it in trio], sources=[_spec(it) for it in trio])  # CPU first
    twins = pt.run_sources([_spec(it) for it in trio])
    dec = gpu.lacx.Decoder(device=0)
    flat = torch.from_numpy(np.concatenate([np.stack([it.left, it.right]).ravel() for it in trio])).cuda()  # L R of each item, back to back
    srcs, at = [], 0
    for it in trio:
        n = len(it.left)
        srcs.append(((flat.data_ptr() + 4 * at, flat.data_ptr() + 4 * (at + n), P32, 2, n), 48000, 24))
        at += 2 * n
    for got in (dec.truepeak_batch(lacs), dec.truepeak_pcm_batch(srcs)):
        for it, g, twin in zip(trio, got, twins):
            _check(it.name, g, it, twin, gpu.lacx)
        assert bytes(got[1][1]) == bytes(32) and got[1][0].true_peak == 0.0 and got[1][0].true_peak_dbtp == -math.inf
    dec.close()


def test_an_invalid_source_sample_fails_its_item(gpu, torch):
    """A planar int32 outside the depth and an inexact float: the digest form's message, no result and no rows, the others
    unharmed."""
    dec = gpu.lacx.Decoder(device=0)
    it = pt.Item("good", 2, 24, 48000, pt._noise(2 * 1024 + 301, 24, 41), pt._noise(2 * 1024 + 301, 24, 42))
    good = torch.from_numpy(np.stack([it.left, it.right])).cuda()
    wide = good.clone()
    wide[1, 2 * 1024 + 300] = 1 << 24
    inexact = (good.to(torch.float32) / float(1 << 23)).contiguous()
    inexact[0, 7] = 0.3
    srcs = [(good, 48000, 24), (wide, 48000, 24), (inexact, 48000, 24)]
    pt.cleared("gpu-invalid", [], sources=[_spec(it), _spec(it, bad=(2 * 1024 + 300, 1, 1 << 24)), _spec(it, PF32, 0, (7, 0, 0x3E99999A))])  # CPU first
    (twin,) = pt.run_sources([_spec(it)])
    with pytest.raises(gpu.lacx.BatchDecodeError) as e:
        dec.truepeak_pcm_batch(srcs)
    with pytest.raises(gpu.lacx.BatchDecodeError) as d:
        dec.digest_pcm_batch(srcs)
    assert e.value.errors == d.value.errors == {1: "right sample at index 2348 is outside the configured PCM bit depth",
                                                2: "left sample at index 7 is not an exact 24-bit PCM value"}
    assert e.value.results[1] is None and e.value.results[2] is None
    _check("good", e.value.results[0], it, twin, gpu.lacx)
    dec.close()


def _broken(lac):
    """tests/golden/decode_wav/st16_lr_3blk.lac with the byte change test_gpu_stats.py makes: its second block does not decode."""
    ent, pays = lacmutate._payloads(lac)
    pays[1] = pays[1][:1] + bytes([0x7F]) + pays[1][2:] if lac[4] == 2 else bytes([0x7F]) + pays[1][1:]
    return lacmutate._rebuild(lac, ent, pays)


def test_a_damaged_stream_between_two_clean_ones(gpu, oracle):
    """The damaged item keeps the decode's code and text, gets a zeroed result and no rows; its neighbours are unaffected."""
    it = pt.corpus()[len(pt.FRAME_COUNTS) + 12]  # noise, 1035 frames, stereo 16 bit
    assert it.name == "noise|n1035|2ch16"
    base = _fixture("decode_wav/st16_lr_3blk.lac")
    lacs = pt.cleared("gpu-damaged", [oracle.encode(it.left, it.right, it.rate, it.depth, 2), _broken(base), base])  # CPU first
    twins = pt.run(lacs)
    assert twins[1].status and not twins[0].status and not twins[2].status
    dec = gpu.lacx.Decoder(device=0)
    with pytest.raises(gpu.lacx.BatchDecodeError) as e:
        dec.truepeak_batch(lacs)
    with pytest.raises(gpu.lacx.BatchDecodeError) as d:
        dec.digest_batch(lacs)
    assert list(e.value.errors) == [1] and e.value.errors == d.value.errors and e.value.errors[1].startswith("[decode-error] block=1 ")
    assert e.value.results[1] is None
    rows, count = gpu.lacx.C.POINTER(gpu.lacx.TruePeakRow)(), gpu.lacx.C.c_uint32(5)
    assert gpu.lacx.lib().lacx_decoder_item_truepeak_rows(dec._h, 1, gpu.lacx.C.byref(rows), gpu.lacx.C.byref(count)) == gpu.lacx.OK and count.value == 0
    for k in (0, 2):
        peak, rows = e.value.results[k]
        assert pt.rows_of(rows).tobytes() == twins[k].rows.tobytes() and pt.totals_of(peak) == twins[k].totals, k
    assert pt.rows_of(e.value.results[0][1]).tobytes() == pt.item_rows(it).tobytes()
    alone = dec.truepeak_batch([lacs[0], lacs[2]])
    assert [bytes(a[0]) for a in alone] == [bytes(e.value.results[0][0]), bytes(e.value.results[2][0])]
    dec.close()


def _cli():
    subprocess.check_call(["make", "-C", PKG_DIR, "lacx_cli"], stdout=subprocess.DEVNULL)
    return os.path.join(PKG_DIR, "lacx_cli")


def _fields(line, path):
    assert line.endswith(" " + path)
    return line[:-len(path) - 1]


def _db(x):
    return "-inf" if x == -math.inf else "%.2f" % x


def test_cli_peak(gpu, tmp_path):
    """`lacx_cli peak` on a .lac and on the WAV decoded from it: the same numbers, the binding's; --album over two files is
    the binding's combine; --blocks prints the rows; `over` where flagged; an unreadable file exits 2."""
    cli = _cli()
    by = {it.name: it for it in pt.corpus()}
    items = [by["noise|n16385|2ch16"], by["worst|pos|2ch16"]]
    pt.cleared("gpu-cli", [], sources=[_spec(it) for it in items] + [_spec(it, I16) for it in items])  # CPU first
    enc = gpu.lacx.Encoder(12, 2, 48000, 16, device=0)
    lacs = [enc.encode(it.left, it.right) for it in items]
    dec = gpu.lacx.Decoder(device=0)
    got = dec.truepeak_batch(lacs)
    wav = dec.decode_wav(lacs[0])
    dec.close()
    paths = {name: str(tmp_path / name) for name in ("a.lac", "a.wav", "b.lac", "junk.wav")}
    for name, blob in {"a.lac": lacs[0], "a.wav": wav, "b.lac": lacs[1], "junk.wav": b"RIFF" + bytes(40)}.items():
        with open(paths[name], "wb") as f:
            f.write(blob)

    def text(t):
        pos = t.position
        return "true_peak=%s dBTP peak=%.6f sample_peak=%s dBFS channel=%d frame=%d phase=%d time=%.6f%s" % (
            _db(t.true_peak_dbtp), t.true_peak, _db(t.sample_peak_dbfs), t.peak_channel, pos // 4, pos % 4, pos / (4.0 * t.sample_rate), " over" if t.over else "")

    res = subprocess.run([cli, "peak", paths["a.lac"], paths["a.wav"]], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and res.stderr == ""
    lines = res.stdout.splitlines()
    assert len(lines) == 2 and _fields(lines[0], paths["a.lac"]) == _fields(lines[1], paths["a.wav"]) == text(got[0][0])
    res = subprocess.run([cli, "peak", "--album", paths["a.lac"], paths["b.lac"]], capture_output=True, text=True, timeout=120)
    out = res.stdout.splitlines()
    album = gpu.lacx.truepeak_combine([(rows, 2, 16, len(it.left), 48000) for (_, rows), it in zip(got, items)])
    assert res.returncode == 0 and len(out) == 3 and out[0] == lines[0] and _fields(out[1], paths["b.lac"]) == text(got[1][0])
    assert got[1][0].over and out[1].split(" " + paths["b.lac"])[0].endswith(" over")
    assert out[2] == text(album) + " set=%d album" % album.set and album.set == 1
    res = subprocess.run([cli, "peak", "--blocks", paths["a.lac"]], capture_output=True, text=True, timeout=120)
    out = res.stdout.splitlines()
    assert res.returncode == 0 and len(out) == 1 + len(got[0][1]) == 3 and out[0] == lines[0]
    for s, (line, r) in enumerate(zip(out[1:], got[0][1])):
        assert line == "  row=%d peak0=%d pos0=%d sample_peak0=%d peak1=%d pos1=%d sample_peak1=%d" % (
            s, r.peak[0], r.pos[0], r.sample_peak[0], r.peak[1], r.pos[1], r.sample_peak[1]), line
    res = subprocess.run([cli, "peak", paths["junk.wav"], str(tmp_path / "none.lac")], capture_output=True, text=True, timeout=120)
    assert res.returncode == 2 and res.stdout == ""
    assert res.stderr == f"Peak failed: {paths['junk.wav']}: Failed to read WAV\nPeak failed: {tmp_path / 'none.lac'}: Failed to read file\n"
    res = subprocess.run([cli, "peak"], capture_output=True, text=True, timeout=120)
    assert res.returncode == 2 and "lacx_cli peak FILE... [--album] [--blocks]" in res.stderr
