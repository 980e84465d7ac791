"""Loudness on the MI355X: lacx_decoder_loudness_batch_device, lacx_decoder_loudness_pcm_batch_device, lacx_loudness_combine
and `lacx_cli loudness`.  The device's rows are held to the plain CPU twin's (tests/native/sim_loudness.cpp) BIT FOR BIT --
IEEE add, multiply and fma in the order csrc/loudness_core.h fixes, on both sides -- and, with the totals, to scipy and the
Python restatement (tests/loudtwin.py) within the host tests' tolerances.  Only shapes the sanitized twin has passed in this
run go to the device: every corpus shape as a source job (the loudness passes over planar int32, which is what they see
behind a decode), and as stream jobs the streams of up to 16385 frames or four sub-blocks, the spliced ones and the damaged
one; the decode in front of the larger streams is the decoder's own, which its own tests cover."""
import math
import os
import subprocess

import numpy as np
import pytest

import __graft_entry__ as ge
import lacmutate
import lacstreams
import loudtwin as lt
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
    return lt.SourceSpec(layout, it.channels, it.depth, it.rate, offset, it.left, it.right, bad)


def _small(it):
    return it.left.size <= max(16385, 4 * (it.rate // 10) + 1)


@pytest.fixture(scope="module")
def twin_rows():
    """{item name: SourceOut of the plain twin}: the whole corpus as one source job, computed once."""
    items = lt.corpus()
    lt.assert_content(items)
    return {it.name: out for it, out in zip(items, lt.run_sources([_spec(it) for it in items]))}


@pytest.fixture(scope="module")
def streams(gpu, oracle, twin_rows):
    """[(stream, Item)]: the whole corpus through the product's encoder, and per format the spliced stream of 257 / 258 / 259
    -frame blocks with its version-2 form -- once the sanitized twin has passed their shapes."""
    encoders = {(ch, depth, rate): gpu.lacx.Encoder(12, 2 if ch == 2 else 0, rate, depth, device=0) for ch, depth, rate in lt.FORMATS}
    out = [(encoders[(it.channels, it.depth, it.rate)].encode(it.left, it.right), it) for it in lt.corpus()]
    for ch, depth, rate in lt.FORMATS:
        parts = sw.spliced_parts(ch, depth)
        lacs = [oracle.encode(l, r, rate, depth, 0) for l, r in parts]
        it = lt.Item("splice|%dch%d" % (ch, depth), ch, depth, rate, np.concatenate([l for l, _ in parts]),
                     np.concatenate([r for _, r in parts]) if ch == 2 else None)
        lac = lacstreams.splice(lacstreams.splice(lacs[0], lacs[1]), lacs[2])
        out += [(lac, it), (lacstreams.to_v2(lac), it)]
        (twin_rows[it.name],) = lt.run_sources([_spec(it)])
    lt.cleared("gpu-corpus", [lac for lac, it in out if _small(it)], sources=[_spec(it) for it in lt.corpus()])  # CPU first
    return out


def _check(what, got, it, twin, lx):
    """One item of a loudness call: rows bit for bit the twin's, totals byte-equal to loudness_combine of the rows and within
    the host tolerances of scipy."""
    loud, rows = got
    rows = lt.rows_of(rows)
    assert rows.shape == twin.rows.shape and rows.tobytes() == twin.rows.tobytes(), what
    assert bytes(loud) == bytes(lx.loudness_combine([(rows, it.channels, it.depth, it.rate)])), what
    assert lt.totals_of(loud) == twin.totals, what
    assert lt.row_error(rows, lt.item_rows(it)) <= lt.ROW_TOL, what
    lt.close_totals(lt.totals_of(loud), lt.item_totals(it), lt.TOTALS_TOL)
    assert loud.sample_rate == it.rate and loud.channels == it.channels and loud.bit_depth == it.depth and loud.subblocks == it.left.size // (it.rate // 10)


@pytest.mark.parametrize("reverse", [False, True])
def test_the_corpus_in_one_batch(gpu, streams, twin_rows, reverse):
    """One batch of the whole corpus and the spliced streams, forward and reversed: items start at other places of the job,
    chunks count in the item's frames whatever the container's blocks are."""
    dec = gpu.lacx.Decoder(device=0)
    order = streams[::-1] if reverse else streams
    got = dec.loudness_batch([lac for lac, _ in order])
    assert dec.last_ms > 0
    for (lac, it), g in zip(order, got):
        _check(it.name, g, it, twin_rows[it.name], gpu.lacx)
    one = dec.loudness(order[0][0])
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
    at base offsets of 0 and 4 bytes: the rows are the twin's bit for bit, whatever the layout."""
    dec = gpu.lacx.Decoder(device=0)
    picks = [it for it in lt.corpus() if it.left.size in (4 * (it.rate // 10) + 1, 16385) or it.name.startswith("silence_sound_silence|content") and it.channels == 2 and it.depth == 16]
    assert len(picks) == 9 and {x for b in LAYOUTS.values() for x in b} == {P32, I16, I24, P16, PF32, IF32}
    items, wants, keep = [], [], []
    for it in picks:
        for layout in LAYOUTS[it.depth]:
            for offset in (0, 4):
                bufs = [_upload(torch, raw, offset) for raw in _arrays(it.left, it.right, it.depth, layout)]
                keep.append(bufs)
                ptrs = [b.data_ptr() + offset for b in bufs]
                items.append(((ptrs[0], ptrs[1] if len(ptrs) == 2 else None, layout, it.channels, it.left.size), it.rate, it.depth))
                wants.append(it)
    lt.cleared("gpu-layouts", [], sources=[_spec(it, layout, offset) for it in picks for layout in LAYOUTS[it.depth] for offset in (0, 4)])  # CPU first
    got = dec.loudness_pcm_batch(items)
    assert dec.last_ms > 0
    for k, (g, it) in enumerate(zip(got, wants)):
        _check((it.name, k), g, it, twin_rows[it.name], gpu.lacx)
    dec.close()


def test_an_invalid_source_sample_fails_its_item(gpu, torch):
    """A planar int32 outside the depth -- behind the last complete sub-block, where nothing is filtered -- and an inexact
    float: the digest form's message, no result and no rows, the others unharmed."""
    dec = gpu.lacx.Decoder(device=0)
    it = lt.make_item("noise", 2 * 4800 + 301, 2, 24, 48000, 12)
    good = torch.from_numpy(np.stack([it.left, it.right])).cuda()
    wide = good.clone()
    wide[1, 2 * 4800 + 300] = 1 << 24
    inexact = (good.to(torch.float32) / float(1 << 23)).contiguous()
    inexact[0, 7] = 0.3
    srcs = [(good, 48000, 24), (wide, 48000, 24), (inexact, 48000, 24)]
    lt.cleared("gpu-invalid", [], sources=[_spec(it)])  # CPU first
    (twin,) = lt.run_sources([_spec(it)])
    with pytest.raises(gpu.lacx.BatchDecodeError) as e:
        dec.loudness_pcm_batch(srcs)
    with pytest.raises(gpu.lacx.BatchDecodeError) as d:
        dec.digest_pcm_batch(srcs)
    assert e.value.errors == d.value.errors == {1: "right sample at index 9900 is outside the configured PCM bit depth",
                                                2: "left sample at index 7 is not an exact 24-bit PCM value"}
    assert e.value.results[1] is None and e.value.results[2] is None
    _check("good", e.value.results[0], it, twin, gpu.lacx)
    dec.close()


def test_the_standards_cases_as_streams(gpu):
    """10 s -36 / 60 s -23 / 10 s -36 and 20 s -26 / 20.1 s -20 / 20 s -26 dBFS as .lac through the device: within 0.1 LU of
    -23.0, and bit for bit the twin's rows."""
    cases = [c for c in lt.ebu_cases() if c[0] in ("36-23-36", "26-20-26")]
    items = [lt.ebu_item(name, parts) for name, parts, _ in cases]
    lt.cleared("gpu-ebu", [], sources=[_spec(it) for it in items])  # CPU first
    twins = lt.run_sources([_spec(it) for it in items])
    enc = gpu.lacx.Encoder(12, 2, 48000, 16, device=0)
    dec = gpu.lacx.Decoder(device=0)
    got = dec.loudness_batch([enc.encode(it.left, it.right) for it in items])
    for it, (loud, rows), twin in zip(items, got, twins):
        assert abs(loud.integrated_lufs + 23.0) <= 0.1, (it.name, loud.integrated_lufs)
        assert lt.rows_of(rows).tobytes() == twin.rows.tobytes() and lt.totals_of(loud) == twin.totals, it.name
        assert loud.gain == -18.0 - loud.integrated_lufs and loud.flags == 0
    dec.close()


def _broken(lac):
    """tests/golden/decode_wav/st16_lr_3blk.lac with the byte change test_gpu_stats.py makes: its second block does not decode."""
    ent, pays = lacmutate._payloads(lac)
    pays[1] = pays[1][:1] + bytes([0x7F]) + pays[1][2:] if lac[4] == 2 else bytes([0x7F]) + pays[1][1:]
    return lacmutate._rebuild(lac, ent, pays)


def test_a_damaged_stream_between_two_clean_ones(gpu, oracle):
    """The damaged item keeps the decode's code and text, gets a zeroed result and no rows; its neighbours are unaffected."""
    it = lt.make_item("tone", 2 * 4800 + 11, 2, 16, 48000, 31)
    base = _fixture("decode_wav/st16_lr_3blk.lac")
    lacs = lt.cleared("gpu-damaged", [oracle.encode(it.left, it.right, it.rate, it.depth, 2), _broken(base), base])  # CPU first
    twins = lt.run(lacs)
    assert twins[1].status and not twins[0].status and not twins[2].status
    dec = gpu.lacx.Decoder(device=0)
    with pytest.raises(gpu.lacx.BatchDecodeError) as e:
        dec.loudness_batch(lacs)
    with pytest.raises(gpu.lacx.BatchDecodeError) as d:
        dec.digest_batch(lacs)
    assert list(e.value.errors) == [1] and e.value.errors == d.value.errors and e.value.errors[1].startswith("[decode-error] block=1 ")
    assert e.value.results[1] is None
    rows, count = gpu.lacx.C.POINTER(gpu.lacx.LoudnessRow)(), gpu.lacx.C.c_uint32(5)
    assert gpu.lacx.lib().lacx_decoder_item_loudness_rows(dec._h, 1, gpu.lacx.C.byref(rows), gpu.lacx.C.byref(count)) == gpu.lacx.OK and count.value == 0
    for k in (0, 2):
        loud, rows = e.value.results[k]
        assert lt.rows_of(rows).tobytes() == twins[k].rows.tobytes() and lt.totals_of(loud) == twins[k].totals, k
    alone = dec.loudness_batch([lacs[0], lacs[2]])
    assert [bytes(a[0]) for a in alone] == [bytes(e.value.results[0][0]), bytes(e.value.results[2][0])]
    dec.close()


def _cli():
    subprocess.check_call(["make", "-C", PKG_DIR, "lacx_cli"], stdout=subprocess.DEVNULL)
    return os.path.join(PKG_DIR, "lacx_cli")


def _fields(line, path):
    assert line.endswith(" " + path)
    return line[:-len(path) - 1]


def _num(x):
    return "-inf" if x == -math.inf else "%.2f" % x


def test_cli_loudness(gpu, tmp_path):
    """`lacx_cli loudness` on a .lac and on the WAV decoded from it: the same numbers, the binding's; --album over two files is
    the binding's combine; --blocks prints the rows; an unreadable file exits 2."""
    cli = _cli()
    items = [next(i for i in lt.corpus() if i.name.startswith("loud_quiet|content") and i.channels == 2 and i.depth == 16),
             next(i for i in lt.corpus() if i.name.startswith("tone|content") and i.channels == 2 and i.depth == 16)]
    lt.cleared("gpu-cli", [], sources=[_spec(it) for it in items])  # CPU first
    enc = gpu.lacx.Encoder(12, 2, 48000, 16, device=0)
    lacs = [enc.encode(it.left, it.right) for it in items]
    dec = gpu.lacx.Decoder(device=0)
    got = dec.loudness_batch(lacs)
    wav = dec.decode_wav(lacs[0])
    dec.close()
    paths = {name: str(tmp_path / name) for name in ("a.lac", "a.wav", "b.lac", "junk.wav")}
    for name, blob in {"a.lac": lacs[0], "a.wav": wav, "b.lac": lacs[1], "junk.wav": b"RIFF" + bytes(40)}.items():
        with open(paths[name], "wb") as f:
            f.write(blob)

    def text(loud):
        return "integrated=%s LUFS range=%s LU momentary_max=%s LUFS shortterm_max=%s LUFS gain=%s dB" % (
            _num(loud.integrated_lufs), _num(loud.range_lu), _num(loud.momentary_max_lufs), _num(loud.shortterm_max_lufs), _num(loud.gain))

    res = subprocess.run([cli, "loudness", paths["a.lac"], paths["a.wav"]], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and res.stderr == ""
    lines = res.stdout.splitlines()
    assert len(lines) == 2 and _fields(lines[0], paths["a.lac"]) == _fields(lines[1], paths["a.wav"]) == text(got[0][0])
    res = subprocess.run([cli, "loudness", "--album", paths["a.lac"], paths["b.lac"]], capture_output=True, text=True, timeout=120)
    out = res.stdout.splitlines()
    album = gpu.lacx.loudness_combine([(rows, 2, 16, 48000) for _, rows in got])
    assert res.returncode == 0 and len(out) == 3 and out[0] == lines[0] and _fields(out[1], paths["b.lac"]) == text(got[1][0])
    assert out[2] == text(album) + " album"
    res = subprocess.run([cli, "loudness", "--blocks", paths["a.lac"]], capture_output=True, text=True, timeout=120)
    out = res.stdout.splitlines()
    assert res.returncode == 0 and len(out) == 1 + len(got[0][1]) and out[0] == lines[0]
    for s, (line, r) in enumerate(zip(out[1:], got[0][1])):
        assert line == "  subblock=%d energy0=%.17g energy1=%.17g" % (s, r.energy[0], r.energy[1]), line
    res = subprocess.run([cli, "loudness", paths["junk.wav"], str(tmp_path / "none.lac")], capture_output=True, text=True, timeout=120)
    assert res.returncode == 2 and res.stdout == ""
    assert res.stderr == f"Loudness failed: {paths['junk.wav']}: Failed to read WAV\nLoudness failed: {tmp_path / 'none.lac'}: Failed to read file\n"
    res = subprocess.run([cli, "loudness"], capture_output=True, text=True, timeout=120)
    assert res.returncode == 2 and "lacx_cli loudness FILE... [--album] [--blocks]" in res.stderr
