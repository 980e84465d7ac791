"""Spectrum on the MI355X: lacx_decoder_spectrum_batch_device, lacx_decoder_spectrum_pcm_batch_device, lacx_spectrum_combine
and `lacx_cli spectrum`.  The device's rows are held to the plain CPU twin's (tests/native/sim_spectrum.cpp) BYTE FOR BYTE:
csrc/spectrum_core.h fixes every operation and its order, nothing but the written multiply-adds is fused, and device and twin
read the same tables.  (The twin in turn is held to numpy within BAND_TOL by test_spectrum_twin_host.py.)  Only shapes the
sanitized twin has passed in this run go to the device: every corpus shape as a source job, and as stream jobs the streams of
up to 16400 frames, the spliced ones and the damaged one; the decode in front of the larger streams is the decoder's own."""
import os
import subprocess

import numpy as np
import pytest

import __graft_entry__ as ge
import lacmutate
import lacstreams
import spectwin as st
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


def _small(it):
    return len(it.left) <= 16400


@pytest.fixture(scope="module")
def streams(gpu, oracle):
    """{window: [(stream, Item)]}: the corpus of each window length through the product's encoder, and at N = 256 per format
    the spliced stream of 257 / 258 / 259-frame blocks with its version-2 form -- once the sanitized twin has passed them."""
    encoders = {(ch, depth, rate): gpu.lacx.Encoder(12, 2 if ch == 2 else 0, rate, depth, device=0) for ch, depth, rate in st.FORMATS}
    out = {w: [] for w in st.WINDOWS}
    for it in st.corpus():
        out[it.window].append((encoders[(it.channels, it.depth, it.rate)].encode(it.left, it.right), it))
    for ch, depth, rate in st.FORMATS:
        parts = sw.spliced_parts(ch, depth)
        lacs = [oracle.encode(l, r, rate, depth, 0) for l, r in parts]
        it = st.Item("splice|N256|%dch%d" % (ch, depth), 256, ch, depth, rate, np.concatenate([l for l, _ in parts]),
                     np.concatenate([r for _, r in parts]) if ch == 2 else None)
        lac = lacstreams.splice(lacstreams.splice(lacs[0], lacs[1]), lacs[2])
        out[256] += [(lac, it), (lacstreams.to_v2(lac), it)]
    for w, some in out.items():  # CPU first
        st.cleared("gpu-corpus", w, [lac for lac, it in some if _small(it)], sources=[st.spec_of(it) for _, it in some])
    return out


def _check(what, got, it, lx, floor=st.FLOOR):
    """One item of a spectrum call: rows byte-equal to the plain twin's, totals byte-equal to spectrum_combine of the rows."""
    spec, rows = got
    rows = st.rows_of(rows)
    twin = st.twin_rows(it)
    assert rows.shape == twin.shape and rows.tobytes() == twin.tobytes(), what
    assert bytes(spec) == bytes(lx.spectrum_combine(rows.tobytes(), it.channels, it.depth, len(it.left), it.rate, it.window, floor)), what
    assert spec.sample_rate == it.rate and spec.channels == it.channels and spec.bit_depth == it.depth and spec.frames == len(it.left) and spec.window == it.window
    st.same_totals(st.totals_of(spec), st.expected_totals(twin["power"], it.channels, it.depth, len(it.left), it.rate, it.window, floor))


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("window", st.WINDOWS)
def test_the_corpus_in_one_batch(gpu, streams, window, reverse):
    """One batch per window length of its whole corpus (and at N = 256 the spliced streams), forward and reversed: items
    start at other places of the job, the rows are the same bits."""
    dec = gpu.lacx.Decoder(device=0)
    order = streams[window][::-1] if reverse else streams[window]
    got = dec.spectrum_batch([lac for lac, _ in order], window)
    assert dec.last_ms > 0
    for (lac, it), g in zip(order, got):
        _check(it.name, g, it, gpu.lacx)
    one = dec.spectrum(order[0][0], window)
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


def test_source_form_in_all_six_layouts(gpu, torch):
    """Device-resident PCM in every layout, in buffers that end with the source's last byte, at base offsets of 0 and 4
    bytes: the rows are the twin's byte for byte, whatever the layout."""
    dec = gpu.lacx.Decoder(device=0)
    picks = [it for it in st.corpus() if it.name.startswith(("noise|N256|n129|", "noise|N256|n16385|", "sine|k2-k64|N256", "dc|N256"))]
    assert len(picks) == 8 + 4 and {x for b in LAYOUTS.values() for x in b} == {P32, I16, I24, P16, PF32, IF32}
    items, wants, keep, specs = [], [], [], []
    for it in picks:
        for layout in LAYOUTS[it.depth]:
            for offset in (0, 4):
                bufs = [_upload(torch, raw, offset) for raw in _arrays(it.left, it.right, it.depth, layout)]
                keep.append(bufs)
                ptrs = [b.data_ptr() + offset for b in bufs]
                items.append(((ptrs[0], ptrs[1] if len(ptrs) == 2 else None, layout, it.channels, len(it.left)), it.rate, it.depth))
                wants.append(it)
                specs.append(st.spec_of(it, layout, offset))
    st.cleared("gpu-layouts", 256, [], sources=specs)  # CPU first
    got = dec.spectrum_pcm_batch(items, 256)
    assert dec.last_ms > 0
    for k, (g, it) in enumerate(zip(got, wants)):
        _check((it.name, k), g, it, gpu.lacx)
    dec.close()


def test_an_invalid_source_sample_fails_its_item(gpu, torch):
    """A planar int32 outside the depth and an inexact float: the digest form's message, no result and no rows, the others
    unharmed."""
    dec = gpu.lacx.Decoder(device=0)
    n = 2 * 1024 + 301
    it = st.Item("good", 1024, 2, 24, 44100, st._noise(n, 24, 41), st._noise(n, 24, 42))
    good = torch.from_numpy(np.stack([it.left, it.right])).cuda()
    wide = good.clone()
    wide[1, n - 1] = 1 << 24
    inexact = (good.to(torch.float32) / float(1 << 23)).contiguous()
    inexact[0, 7] = 0.3
    srcs = [(good, 44100, 24), (wide, 44100, 24), (inexact, 44100, 24)]
    st.cleared("gpu-invalid", 1024, [], sources=[st.spec_of(it), st.spec_of(it, bad=(n - 1, 1, 1 << 24)), st.spec_of(it, PF32, 0, (7, 0, 0x3E99999A))])  # CPU first
    with pytest.raises(gpu.lacx.BatchDecodeError) as e:
        dec.spectrum_pcm_batch(srcs, 1024)
    with pytest.raises(gpu.lacx.BatchDecodeError) as d:
        dec.digest_pcm_batch(srcs)
    assert e.value.errors == d.value.errors == {1: "right sample at index %d is outside the configured PCM bit depth" % (n - 1),
                                                2: "left sample at index 7 is not an exact 24-bit PCM value"}
    assert e.value.results[1] is None and e.value.results[2] is None
    _check("good", e.value.results[0], it, gpu.lacx)
    dec.close()


def _broken(lac):
    """tests/golden/decode_wav/st16_lr_3blk.lac with the byte change test_gpu_stats.py makes: its second block does not decode."""
    ent, pays = lacmutate._payloads(lac)
    pays[1] = pays[1][:1] + bytes([0x7F]) + pays[1][2:] if lac[4] == 2 else bytes([0x7F]) + pays[1][1:]
    return lacmutate._rebuild(lac, ent, pays)


def test_a_damaged_stream_between_two_clean_ones(gpu, oracle):
    """The damaged item keeps the decode's code and text, gets a zeroed result and no rows; its neighbours are bit-equal to a
    batch without it."""
    it = {x.name: x for x in st.corpus()}["noise|N256|n257|2ch16"]
    base = _fixture("decode_wav/st16_lr_3blk.lac")
    lacs = st.cleared("gpu-damaged", 256, [oracle.encode(it.left, it.right, it.rate, it.depth, 2), _broken(base), base])  # CPU first
    twins = st.run(lacs, 256)
    assert twins[1].status and not twins[0].status and not twins[2].status
    dec = gpu.lacx.Decoder(device=0)
    with pytest.raises(gpu.lacx.BatchDecodeError) as e:
        dec.spectrum_batch(lacs, 256)
    with pytest.raises(gpu.lacx.BatchDecodeError) as d:
        dec.digest_batch(lacs)
    assert list(e.value.errors) == [1] and e.value.errors == d.value.errors and e.value.errors[1].startswith("[decode-error] block=1 ")
    assert e.value.results[1] is None
    rows, count = gpu.lacx.C.POINTER(gpu.lacx.SpectrumRow)(), gpu.lacx.C.c_uint32(5)
    assert gpu.lacx.lib().lacx_decoder_item_spectrum_rows(dec._h, 1, gpu.lacx.C.byref(rows), gpu.lacx.C.byref(count)) == gpu.lacx.OK and count.value == 0
    for k in (0, 2):
        assert st.rows_of(e.value.results[k][1]).tobytes() == twins[k].rows.tobytes(), k
    assert st.rows_of(e.value.results[0][1]).tobytes() == st.twin_rows(it).tobytes()
    alone = dec.spectrum_batch([lacs[0], lacs[2]], 256)
    assert [bytes(a[0]) + bytes(a[1]) for a in alone] == [bytes(e.value.results[k][0]) + bytes(e.value.results[k][1]) for k in (0, 2)]
    dec.close()


def test_an_unsupported_window_fails_the_call_and_launches_nothing(gpu, torch):
    it = st.corpus()[3]
    enc = gpu.lacx.Encoder(12, 0, it.rate, it.depth, device=0)
    lac = enc.encode(it.left, None)
    dec = gpu.lacx.Decoder(device=0)
    flat = torch.from_numpy(it.left).cuda()
    for window in (0, 128, 1000, 8192):
        dec.last_ms = -1.0
        with pytest.raises(ValueError, match="unsupported spectrum window: %d" % window):
            dec.spectrum_batch([lac], window)
        assert dec.last_ms == 0.0
        with pytest.raises(ValueError, match="unsupported spectrum window: %d" % window):
            dec.spectrum_pcm_batch([(flat, it.rate, it.depth)], window)
        assert dec.last_ms == 0.0
    dec.close()


def _cli():
    subprocess.check_call(["make", "-C", PKG_DIR, "lacx_cli"], stdout=subprocess.DEVNULL)
    return os.path.join(PKG_DIR, "lacx_cli")


def test_cli_spectrum(gpu, tmp_path):
    """`lacx_cli spectrum` on a .lac and on the WAV decoded from it: the same line, the binding's; --blocks prints the rows
    with %.17g; junk input exits 2 with `Spectrum failed: ...`; no arguments prints the usage."""
    cli = _cli()
    it = {x.name: x for x in st.corpus()}["noise|N512|n16385|2ch16"]
    st.cleared("gpu-cli", 512, [], sources=[st.spec_of(it), st.spec_of(it, I16)])  # CPU first
    enc = gpu.lacx.Encoder(12, 2, it.rate, 16, device=0)
    lac = enc.encode(it.left, it.right)
    dec = gpu.lacx.Decoder(device=0)
    (got,) = dec.spectrum_batch([lac], 512, -90.0)
    wav = dec.decode_wav(lac)
    dec.close()
    paths = {name: str(tmp_path / name) for name in ("a.lac", "a.wav", "junk.wav")}
    for name, blob in {"a.lac": lac, "a.wav": wav, "junk.wav": b"RIFF" + bytes(40)}.items():
        with open(paths[name], "wb") as f:
            f.write(blob)
    t = got[0]
    text = " ".join("ch%d: bandwidth=%.1f Hz peak=%.1f Hz" % (c, t.bandwidth_hz[c], t.peak_hz(c)) for c in range(2))
    text += " %d Hz 16 bit window=512 windows=%d floor=-90.0 dBFS" % (it.rate, t.windows)
    res = subprocess.run([cli, "spectrum", "--window=512", "--floor=-90", paths["a.lac"], paths["a.wav"]], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and res.stderr == ""
    assert res.stdout.splitlines() == [text + " " + paths["a.lac"], text + " " + paths["a.wav"]]
    res = subprocess.run([cli, "spectrum", "--blocks", "--window=512", "--floor=-90", paths["a.lac"]], capture_output=True, text=True, timeout=120)
    out = res.stdout.splitlines()
    assert res.returncode == 0 and len(out) == 1 + 2 * len(got[1]) == 5 and out[0] == text + " " + paths["a.lac"]
    for s, r in enumerate(got[1]):
        for c in range(2):
            assert out[1 + 2 * s + c] == "  row=%d ch%d: " % (s, c) + " ".join("%.17g" % r.power[c][b] for b in range(64))
    res = subprocess.run([cli, "spectrum", paths["junk.wav"], str(tmp_path / "none.lac")], capture_output=True, text=True, timeout=120)
    assert res.returncode == 2 and res.stdout == ""
    assert res.stderr == f"Spectrum failed: {paths['junk.wav']}: Failed to read WAV\nSpectrum failed: {tmp_path / 'none.lac'}: Failed to read file\n"
    res = subprocess.run([cli, "spectrum", "--window=300", paths["a.lac"]], capture_output=True, text=True, timeout=120)
    assert res.returncode == 2 and res.stderr == f"Spectrum failed: {paths['a.lac']}: unsupported spectrum window: 300\n"
    res = subprocess.run([cli, "spectrum"], capture_output=True, text=True, timeout=120)
    assert res.returncode == 2 and "lacx_cli spectrum FILE... [--window=N] [--floor=DB] [--blocks]" in res.stderr
