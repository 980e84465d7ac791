"""lacx_decoder_digest_batch_device / lacx_decoder_digest_pcm_batch_device / `lacx_cli digest` on the MI355X.  Every
expected value comes from outside the digest path: zlib.crc32 over bytes made by numpy / wavutil from the PCM that was
encoded, or over WAV images from the existing decode path whose sha256 is pinned in tests/golden/decode_wav.json."""
import hashlib
import json
import os
import subprocess
import zlib

import numpy as np
import pytest

import __graft_entry__ as ge
import digesttwin
import lacstreams
import wavutil as W

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
PKG_DIR = os.path.join(ROOT, "lossless-audio-codec_amd")
P32, I16, I24, P16, PF32, IF32 = 0, 1, 2, 16, 17, 18
FORMATS = ((1, 16, 44100), (2, 16, 48000), (1, 24, 96000), (2, 24, 192000))
SENTINEL = 0xA5
UNIT, WG = digesttwin.unit_frames(), digesttwin.threads()  # frames per thread, threads per workgroup


@pytest.fixture(scope="module")
def gpu():
    pkg = ge.load_pkg()
    if pkg.lacx.device_count() <= 0:
        pytest.fail("no HIP device: the decoder has no CPU fallback")
    lx = pkg.lacx
    assert (lx.PCM_PLANAR_I32, lx.PCM_INTERLEAVED_I16, lx.PCM_INTERLEAVED_I24, lx.PCM_PLANAR_I16, lx.PCM_PLANAR_F32,
            lx.PCM_INTERLEAVED_F32) == (P32, I16, I24, P16, PF32, IF32)
    return pkg


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


@pytest.fixture(scope="module")
def encoders(gpu):
    """One encoder per format, per-block stereo."""
    return {(ch, bits): gpu.lacx.Encoder(12, 2 if ch == 2 else 0, rate, bits, device=0) for ch, bits, rate in FORMATS}


def _fixture(name):
    with open(os.path.join(GOLDEN, name), "rb") as f:
        return f.read()


def _noise(frames, channels, bits, seed):
    """Full-scale noise: the whole range of the depth, its ends included."""
    rng = np.random.default_rng(seed)
    lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
    out = []
    for _ in range(channels):
        x = rng.integers(lo, hi + 1, frames, dtype=np.int64)
        x[:min(frames, 2)] = (lo, hi)[:min(frames, 2)]
        out.append(x.astype(np.int32))
    return out[0], out[1] if channels == 2 else None


def _want(left, right, rate, bits):
    """(data_crc32, wav_crc32, frames, data_bytes, rate, channels, bits, wav_valid) by zlib over wavutil's bytes."""
    data = W.pcm_bytes(left, right, bits)
    wav = W.make_wav(left, right, rate, bits)
    assert len(wav) == 44 + len(data) + (len(data) & 1)
    return (zlib.crc32(data), zlib.crc32(wav), left.size, len(data), rate, 1 if right is None else 2, bits, 1)


def _got(g):
    assert g.reserved == 0
    return (g.data_crc32, g.wav_crc32, g.frames, g.data_bytes, g.sample_rate, g.channels, g.bit_depth, g.wav_valid)


def test_pinned_streams(gpu):
    with open(os.path.join(GOLDEN, "decode_wav.json")) as f:
        ents = json.load(f)
    assert len(ents) == 26
    lacs = [lacstreams.from_recipe(e["source"], _fixture) for e in ents]
    assert any(x[2] == 2 for x in lacs) and any(x[2] == 3 for x in lacs)
    dec = gpu.lacx.Decoder(device=0)
    wavs = dec.decode_wav_batch(lacs)
    assert [(len(w), hashlib.sha256(w).hexdigest()) for w in wavs] == [(e["wav_bytes"], e["wav_sha256"]) for e in ents]
    want = []
    for lac, wav in zip(lacs, wavs):
        info = gpu.lacx.stream_parse(lac)
        data_bytes = info.frames * info.channels * info.bit_depth // 8
        want.append((zlib.crc32(wav[44:44 + data_bytes]), zlib.crc32(wav), info.frames, data_bytes, info.sample_rate, info.channels,
                     info.bit_depth, 1))
    for lac, w in zip(lacs, want):  # one by one
        assert _got(dec.digest(lac)) == w
    res = dec.digest_batch(lacs)  # as one batch
    assert [_got(g) for g in res] == want
    assert dec.last_ms > 0
    dec.close()


def _sizes():
    out = list(range(1, 10))
    out += list(range(UNIT * 63, UNIT * 65 + 1))            # the wave border
    out += list(range(UNIT * (WG - 1), UNIT * (WG + 1) + 1))  # the workgroup border
    out += [16384 - 1, 16384, 16384 + 1, 3 * 16384 + 5]
    return out


def test_sizes_in_one_batch(gpu, torch, encoders):
    """Every format at every size, in one batch, so that items also start inside other items' workgroups; the same PCM
    as planar int32 sources through the source form."""
    lacs, want, sources, keep = [], [], [], []
    seed = 0
    for ch, bits, rate in FORMATS:
        for frames in _sizes():
            seed += 1
            left, right = _noise(frames, ch, bits, seed)
            lacs.append(encoders[(ch, bits)].encode(left, right))
            want.append(_want(left, right, rate, bits))
            t = torch.from_numpy(np.stack([left] if right is None else [left, right])).cuda()
            keep.append(t)
            sources.append((t, rate, bits))
    assert len(lacs) == 4 * 31
    dec = gpu.lacx.Decoder(device=0)
    assert [_got(g) for g in dec.digest_batch(lacs)] == want
    assert [_got(g) for g in dec.digest_pcm_batch(sources)] == want
    order = list(range(len(lacs)))[::-1]  # another order: other items share the workgroups
    assert [_got(g) for g in dec.digest_batch([lacs[i] for i in order])] == [want[i] for i in order]
    dec.close()


def test_many_tiny_items(gpu, torch, encoders):
    """300 items of 1 .. 7 frames: every wave spans items, the general path."""
    lacs, want, sources, keep = [], [], [], []
    for k in range(300):
        ch, bits, rate = FORMATS[k % 4]
        frames = 1 + (k * 5) % 7
        left, right = _noise(frames, ch, bits, 1000 + k)
        lacs.append(encoders[(ch, bits)].encode(left, right))
        want.append(_want(left, right, rate, bits))
        t = torch.from_numpy(np.stack([left] if right is None else [left, right])).cuda()
        keep.append(t)
        sources.append((t, rate, bits))
    assert {w[2] for w in want} == set(range(1, 8))
    dec = gpu.lacx.Decoder(device=0)
    assert [_got(g) for g in dec.digest_batch(lacs)] == want
    assert [_got(g) for g in dec.digest_pcm_batch(sources)] == want
    dec.close()


@pytest.mark.parametrize("channels,bits,rate", FORMATS)
def test_one_long_item(gpu, encoders, channels, bits, rate):
    """More than four blocks of full-scale noise: nearly every wave takes the fast path."""
    frames = 4 * 16384 + 2 * UNIT * 64 + 3
    left, right = _noise(frames, channels, bits, 7 + bits + channels)
    lac = encoders[(channels, bits)].encode(left, right)
    assert gpu.lacx.stream_parse(lac).blocks == 5
    dec = gpu.lacx.Decoder(device=0)
    want = _want(left, right, rate, bits)
    assert _got(dec.digest(lac)) == want
    assert _got(dec.digest(lacstreams.to_v2(lac))) == want  # the legacy container: one lane walks it
    dec.close()


def _spliced(gpu, bits, seed):
    """A stream of single-block encodes spliced together: non-final blocks of odd lengths, mid/side and left/right
    blocks alternating (per-block stereo: a pair of nearly equal channels goes mid/side, a pair with one silent channel
    left/right).  Returns (lac, left, right, block_frames)."""
    rate = 48000
    lens = (257, 4097, 259, 301, 1025, 40)
    rng = np.random.default_rng(seed)
    parts, lefts, rights = [], [], []
    for k, n in enumerate(lens):
        l, _ = gpu.synth.synth_pcm(n, 1, bits, rate, seed=seed + k, kind="music")
        l = (l // 2).astype(np.int32)
        r = (l + rng.integers(-1, 2, n)).astype(np.int32) if k % 2 == 0 else np.zeros(n, dtype=np.int32)
        parts.append(gpu.lacx.Encoder(12, 2, rate, bits, device=0).encode(l, r))
        lefts.append(l), rights.append(r)
    lac = parts[0]
    for p in parts[1:]:
        lac = lacstreams.splice(lac, p)
    assert lacstreams.block_frames(lac) == list(lens)
    return lac, np.concatenate(lefts), np.concatenate(rights), list(lens)


@pytest.mark.parametrize("bits", [16, 24])
def test_spliced_stream(gpu, bits):
    import dectwin

    lac, left, right, block_frames = _spliced(gpu, bits, 40 + bits)
    ms = list(dectwin.decode(lac).ms)
    assert set(ms) == {0, 1} and any(a != b for a, b in zip(ms, ms[1:])) and ms[0] != ms[1], ms  # a unit spans an LR/MS boundary
    assert any(n % UNIT for n in np.cumsum(block_frames)[:-1])
    dec = gpu.lacx.Decoder(device=0)
    want = _want(left, right, 48000, bits)
    assert _got(dec.digest(lac)) == want
    assert [_got(g) for g in dec.digest_batch([lac, lacstreams.to_v2(lac), lac])] == [want] * 3
    dec.close()


class Placed:
    """Bytes in device memory at `offset` bytes behind the start of a torch buffer, sentinels on both sides."""

    def __init__(self, torch, raw: bytes, offset=0, tail=64, whole=None):
        n = len(raw)
        if whole is None:
            self.buf = torch.full((offset + n + tail,), SENTINEL, dtype=torch.uint8, device="cuda")
        else:  # at the very end of `whole`, a buffer that is an allocation of its own
            self.buf, offset = whole, whole.numel() - n
            self.buf.fill_(SENTINEL)
        self.offset, self.n = offset, n
        self.buf[offset:offset + n] = torch.frombuffer(bytearray(raw), dtype=torch.uint8).cuda()
        self.ptr = self.buf.data_ptr() + offset
        self.raw = raw

    def untouched(self):
        host = self.buf.cpu().numpy()
        return bool((host[:self.offset] == SENTINEL).all()) and bool((host[self.offset + self.n:] == SENTINEL).all()) and \
            host[self.offset:self.offset + self.n].tobytes() == self.raw


def _rows(left, right, bits, layout):
    """The source's arrays as bytes: one for an interleaved layout, one per channel for a planar one."""
    chans = [left] if right is None else [left, right]
    if layout in (PF32, IF32):
        chans = [(x.astype(np.float32) / np.float32(1 << (bits - 1))) for x in chans]
    elif layout in (I16, P16):
        chans = [x.astype("<i2") for x in chans]
    if layout == I24:
        return [W.pcm_bytes(left, right, 24)]
    if layout in (I16, IF32):
        return [np.stack(chans, axis=1).tobytes()]
    return [x.astype(x.dtype.newbyteorder("<")).tobytes() for x in chans]


def _source(torch, left, right, bits, layout, offset=0, whole=None):
    """((data0, data1, layout, channels, frames), [Placed, ...]) of that PCM in that layout."""
    placed = [Placed(torch, raw, offset, whole=whole if k == 0 else None) for k, raw in enumerate(_rows(left, right, bits, layout))]
    return (placed[0].ptr, placed[1].ptr if len(placed) == 2 else None, layout, 1 if right is None else 2, left.size), placed


def test_source_layouts_alignment_and_bounds(gpu, torch):
    """Every layout at every base offset it permits, a partial last unit, more than one workgroup; sentinels on both
    sides of every array stay as they were, and so does a source at the very end of its allocation."""
    dec = gpu.lacx.Decoder(device=0)
    whole = torch.empty(10 << 20, dtype=torch.uint8, device="cuda")  # large enough to be an allocation of its own
    frames = UNIT * WG + UNIT * 64 + 3
    offsets = {P32: (0, 4, 8, 16), I16: (0, 4, 8, 16), I24: (0, 1, 2, 3, 4, 8, 16), P16: (0, 2, 4, 8, 16), PF32: (0, 4, 8, 16),
               IF32: (0, 4, 8, 16)}
    for ch, bits, rate in FORMATS:
        left, right = _noise(frames, ch, bits, 300 + bits + ch)
        want = _want(left, right, rate, bits)
        items, keep = [], []
        for layout in digesttwin.LAYOUTS[bits]:
            for offset in offsets[layout]:
                src, placed = _source(torch, left, right, bits, layout, offset)
                assert placed[0].ptr % 16 == offset % 16
                items.append((src, rate, bits)), keep.append(placed)
        res = dec.digest_pcm_batch(items)
        assert [_got(g) for g in res] == [want] * len(items), (ch, bits)
        assert all(p.untouched() for ps in keep for p in ps)
        # the last byte of the source is the last byte of an allocation (an even frame count, so that an interleaved
        # int16 mono source still starts on a 4-byte boundary; the last unit stays partial)
        l2, r2 = left[:-1], None if right is None else right[:-1]
        assert l2.size % UNIT == 2
        want2 = _want(l2, r2, rate, bits)
        for layout in digesttwin.LAYOUTS[bits]:
            src, placed = _source(torch, l2, r2, bits, layout, whole=whole)
            assert placed[0].offset + placed[0].n == whole.numel()
            (g,) = dec.digest_pcm_batch([(src, rate, bits)])
            assert _got(g) == want2, (ch, bits, layout)
            assert all(p.untouched() for p in placed)
    dec.close()


def _tensors(torch, left, right, bits):
    """The tensor layouts of that PCM: {name: device tensor}."""
    stack = np.stack([left] if right is None else [left, right])  # [channels, frames]
    scale = np.float32(1 << (bits - 1))
    out = {"planar int32": torch.from_numpy(stack).cuda(),
           "planar float32": torch.from_numpy(stack.astype(np.float32) / scale).cuda(),
           "interleaved float32": torch.from_numpy(np.ascontiguousarray(stack.T).astype(np.float32) / scale).cuda()}
    if bits == 16:
        out["planar int16"] = torch.from_numpy(stack.astype(np.int16)).cuda()
        out["interleaved int16"] = torch.from_numpy(np.ascontiguousarray(stack.T).astype(np.int16)).cuda()
    return out


@pytest.mark.parametrize("channels,bits,rate", FORMATS)
def test_source_agrees_with_its_encode(gpu, torch, encoders, channels, bits, rate):
    """digest_pcm_batch(source) == digest_batch(encode(source)) for every tensor layout."""
    frames = 16384 + UNIT * 64 + 1
    left, right = gpu.synth.synth_pcm(frames, channels, bits, rate, seed=60 + bits + channels, kind="mixed")
    want = _want(left, right, rate, bits)
    dec = gpu.lacx.Decoder(device=0)
    tensors = _tensors(torch, left, right, bits)
    assert len(tensors) == (5 if bits == 16 else 3)
    for name, t in tensors.items():
        lac = encoders[(channels, bits)].encode_tensor(t)
        (a,) = dec.digest_pcm_batch([(t, rate, bits)])
        b = dec.digest(lac)
        assert bytes(a) == bytes(b), name
        assert _got(a) == want, name
    dec.close()


def _damaged(gpu, lac):
    """A payload damage that the decoder refuses (the failing item of test_gpu_decode_batch.py)."""
    for pos in range(len(lac) // 2, len(lac) - 64, 997):
        bad = bytearray(lac)
        bad[pos] ^= 0x55
        try:
            gpu.lacx.decode(bytes(bad))
        except RuntimeError as err:
            return bytes(bad), str(err)
    raise AssertionError("no damage that the decoder refuses")


def test_damaged_stream_among_good_ones(gpu, torch):
    import ctypes as C

    lx, L = gpu.lacx, gpu.lacx.lib()
    left, right = gpu.synth.synth_pcm(16384 * 2 + 77, 2, 24, 96000, seed=5, kind="music")
    lac = lx.Encoder(12, 2, 96000, 24, device=0).encode(left, right)
    mono, _ = _noise(1000, 1, 16, 9)
    lac2 = lx.Encoder(12, 0, 44100, 16, device=0).encode(mono)
    damaged, damaged_msg = _damaged(gpu, lac)
    assert damaged_msg.startswith("[decode-error] block=")
    want, want2 = _want(left, right, 96000, 24), _want(mono, None, 44100, 16)
    dec = lx.Decoder(device=0)
    items = [lac, damaged, lac2, lac[:-1], lacstreams.to_v2(lac)]
    with pytest.raises(lx.BatchDecodeError) as e:
        dec.digest_batch(items)
    err = e.value
    assert err.errors == {1: damaged_msg, 3: "[decode-error] block payloads do not fill the file"}
    assert str(err) == "stream 1: " + damaged_msg
    assert [None if g is None else _got(g) for g in err.results] == [want, None, want2, None, want]
    with pytest.raises(RuntimeError) as e1:
        dec.digest(damaged)
    assert str(e1.value) == damaged_msg
    # the C ABI: the codes, and a zeroed digest for the failed items
    bufs = [np.frombuffer(x, dtype=np.uint8) for x in items]
    spans = (lx.Span * 5)(*[lx.Span(b.ctypes.data_as(C.POINTER(C.c_uint8)), b.size) for b in bufs])
    rcs, out = (C.c_int * 5)(), (lx.Digest * 5)(*[lx.Digest(9, 9, 9, 9, 9, 9, 9, 9, 9) for _ in range(5)])
    rc = L.lacx_decoder_digest_batch_device(dec._h, spans, 5, None, rcs, out, None)
    assert rc == lx.E_RUNTIME and list(rcs) == [lx.OK, lx.E_RUNTIME, lx.OK, lx.E_INVALID, lx.OK]
    assert L.lacx_decode_last_error().decode() == "stream 1: " + damaged_msg
    assert bytes(out[1]) == bytes(32) and bytes(out[3]) == bytes(32) and _got(out[0]) == want and _got(out[4]) == want
    # the decoder stays usable: digests alternate with decodes and verifications on the same handle and repeat
    src = torch.from_numpy(np.stack([left, right])).cuda()
    for _ in range(2):
        assert [_got(g) for g in dec.digest_batch([lac, lac2])] == [want, want2]
        l2, r2, _, _ = dec.decode(lac)
        assert np.array_equal(l2, left) and np.array_equal(r2, right)
        assert _got(dec.digest(lac)) == want
        (r,) = dec.verify_batch_device([lac], [src])
        assert bytes(r) == bytes(32)
        (g,) = dec.digest_pcm_batch([(src, 96000, 24)])
        assert _got(g) == want
        assert dec.decode_wav(lac2) == W.make_wav(mono, None, 44100, 16)
    dec.close()


def test_invalid_source_samples(gpu, torch):
    """An int32 outside the depth, a float off the grid, a NaN: in left and in right with a lower index in right -- the
    message names left first -- and in right alone; the other items of the batch keep their digests."""
    lx = gpu.lacx
    frames = UNIT * 64 * 3 + 2
    left, right = _noise(frames, 2, 16, 21)
    want = _want(left, right, 48000, 16)
    good = torch.from_numpy(np.stack([left, right])).cuda()
    scale = np.float32(32768)
    f = np.stack([left, right]).astype(np.float32) / scale

    def planar(edits, dtype=np.int32):
        x = (np.stack([left, right]) if dtype == np.int32 else f).copy()
        for c, i, v in edits:
            x[c, i] = v
        return torch.from_numpy(x).cuda()

    def interleaved(edits):
        x = np.ascontiguousarray(f.T).copy()
        for c, i, v in edits:
            x[i, c] = v
        return torch.from_numpy(x).cuda()

    off_grid = np.float32(0.25) + np.float32(2.0 ** -17)
    outside = "is outside the configured PCM bit depth"
    inexact = "is not an exact 16-bit PCM value"
    cases = [
        (planar([(0, 700, 32768), (1, 3, -32769)]), f"left sample at index 700 {outside}"),
        (planar([(1, 3, -32769)]), f"right sample at index 3 {outside}"),
        (planar([(0, frames - 1, 1 << 24)]), f"left sample at index {frames - 1} {outside}"),  # in the partial last unit
        (planar([(0, 513, off_grid), (1, 2, off_grid)], np.float32), f"left sample at index 513 {inexact}"),
        (planar([(1, 2, np.nan)], np.float32), f"right sample at index 2 {inexact}"),
        (planar([(0, 40, np.float32(1.0)), (0, 41, np.nan)], np.float32), f"left sample at index 40 {outside}"),
        (interleaved([(0, 300, np.nan), (1, 1, off_grid)]), f"left sample at index 300 {inexact}"),
        (interleaved([(1, 1, np.float32(-1.5))]), f"right sample at index 1 {outside}"),
    ]
    dec = lx.Decoder(device=0)
    sources = [(good, 48000, 16)]
    for t, _ in cases:
        sources += [(t, 48000, 16), (good, 48000, 16)]
    with pytest.raises(lx.BatchDecodeError) as e:
        dec.digest_pcm_batch(sources)
    err = e.value
    assert err.errors == {2 * k + 1: msg for k, (_, msg) in enumerate(cases)}
    assert str(err) == "stream 1: " + cases[0][1]
    assert [None if g is None else _got(g) for g in err.results] == [want if i % 2 == 0 else None for i in range(len(sources))]
    (g,) = dec.digest_pcm_batch([(good, 48000, 16)])  # usable afterwards
    assert _got(g) == want
    dec.close()


def _cli():
    subprocess.check_call(["make", "-C", PKG_DIR, "lacx_cli"], stdout=subprocess.DEVNULL)
    return os.path.join(PKG_DIR, "lacx_cli")


def test_cli_digest(gpu, tmp_path):
    cli = _cli()
    left, _ = gpu.synth.synth_pcm(16384 + 37, 1, 24, 96000, seed=3, kind="music")  # mono 24-bit, odd: a pad byte
    wav = W.make_wav(left, None, 96000, 24)
    lac = gpu.lacx.Encoder(12, 0, 96000, 24, device=0).encode_wav(wav)
    l2, r2 = gpu.synth.synth_pcm(1001, 2, 16, 44100, seed=4, kind="mixed")
    wav2 = W.make_wav(l2, r2, 44100, 16)
    paths = {name: str(tmp_path / name) for name in ("a.lac", "a.wav", "broken.lac", "b.wav", "junk.wav")}
    blobs = {"a.lac": lac, "a.wav": wav, "broken.lac": lac[:-1], "b.wav": wav2, "junk.wav": b"RIFF" + bytes(40)}
    for name, blob in blobs.items():
        with open(paths[name], "wb") as f:
            f.write(blob)
    order = ["a.lac", "a.wav", "broken.lac", "b.wav"]
    res = subprocess.run([cli, "digest"] + [paths[n] for n in order], capture_output=True, text=True, timeout=120)
    assert res.returncode == 1
    assert res.stderr == f"Digest failed: {paths['broken.lac']}: [decode-error] block payloads do not fill the file\n"
    lines = res.stdout.splitlines()
    data = W.pcm_bytes(left, None, 24)
    head = (f"data_crc32={zlib.crc32(data):08x} wav_crc32={zlib.crc32(wav):08x} frames={left.size} channels=1 bits=24 rate=96000 ")
    head2 = (f"data_crc32={zlib.crc32(W.pcm_bytes(l2, r2, 16)):08x} wav_crc32={zlib.crc32(wav2):08x} frames=1001 channels=2 bits=16 "
             "rate=44100 ")
    assert lines == [head + paths["a.lac"], head + paths["a.wav"], head2 + paths["b.wav"]]
    assert lines[0].split()[:6] == lines[1].split()[:6]  # a .lac and the WAV it was made from
    res = subprocess.run([cli, "digest", paths["a.wav"], paths["a.lac"]], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and res.stderr == "" and res.stdout.splitlines() == [head + paths["a.wav"], head + paths["a.lac"]]
    res = subprocess.run([cli, "digest", paths["junk.wav"], str(tmp_path / "none.lac")], capture_output=True, text=True, timeout=120)
    assert res.returncode == 1 and res.stdout == ""
    assert res.stderr == f"Digest failed: {paths['junk.wav']}: Failed to read WAV\nDigest failed: {tmp_path / 'none.lac'}: Failed to read file\n"
    res = subprocess.run([cli, "digest"], capture_output=True, text=True, timeout=120)
    assert res.returncode == 1 and "Usage:" in res.stderr
