"""lacx_decoder_verify_batch_device / lacx_decoder_verify_wav / `lacx_cli verify | encode --verify | selftest` on the MI355X.
Every expected answer comes from outside the verify path: the PCM that was encoded, or a full decode through the existing
entry points whose WAV matches the sha256 pinned in tests/golden/decode_wav.json."""
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

import __graft_entry__ as ge
import lacstreams
import wavutil as W

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
PKG_DIR = os.path.join(ROOT, "lossless-audio-codec_amd")
P, I16, I24 = 0, 1, 2
SENTINEL = 0xA5


@pytest.fixture(scope="module")
def gpu():
    pkg = ge.load_pkg()
    if pkg.lacx.device_count() <= 0:
        pytest.fail("no HIP device: the decoder has no CPU fallback")
    assert (pkg.lacx.PCM_PLANAR_I32, pkg.lacx.PCM_INTERLEAVED_I16, pkg.lacx.PCM_INTERLEAVED_I24) == (P, I16, I24)
    return pkg


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


def _fixture(name):
    with open(os.path.join(GOLDEN, name), "rb") as f:
        return f.read()


def _sha(b):
    return hashlib.sha256(bytes(b)).hexdigest()


def _wav_pcm(wav, channels, bits):
    """(left, right or None) of a canonical WAV image (44-byte header)."""
    frames = (len(wav) - 44) // (channels * bits // 8)
    data = np.frombuffer(wav, dtype=np.uint8, count=frames * channels * bits // 8, offset=44)
    if bits == 16:
        x = data.view("<i2").astype(np.int32)
    else:
        t = data.reshape(-1, 3).astype(np.int32)
        x = t[:, 0] | (t[:, 1] << 8) | (t[:, 2] << 16)
        x = (x ^ 0x800000) - 0x800000
    x = x.reshape(frames, channels)
    return np.ascontiguousarray(x[:, 0]), (np.ascontiguousarray(x[:, 1]) if channels == 2 else None)


class Placed:
    """Bytes in device memory at `offset` bytes behind the start of a torch buffer, sentinels on both sides."""

    def __init__(self, torch, raw: bytes, offset=0, tail=64, whole=None):
        n = len(raw)
        if whole is None:
            self.buf = torch.full((offset + n + tail,), SENTINEL, dtype=torch.uint8, device="cuda")
        else:  # at the very end of `whole`, a buffer that is an allocation of its own
            self.buf, offset, tail = whole, whole.numel() - n, 0
            self.buf.fill_(SENTINEL)
        self.offset, self.n = offset, n
        self.buf[offset:offset + n] = torch.frombuffer(bytearray(raw), dtype=torch.uint8).cuda()
        self.ptr = self.buf.data_ptr() + offset
        self.torch = torch

    def untouched(self):
        t = self.torch
        return bool((self.buf[:self.offset] == SENTINEL).all()) and bool((self.buf[self.offset + self.n:] == SENTINEL).all())


def _source(torch, left, right, bits, layout, offset=0, whole=None):
    """A verify source of that PCM: ((data0, data1, layout, channels, frames), [Placed, ...])."""
    ch = 1 if right is None else 2
    if layout == P:
        a = Placed(torch, np.asarray(left, dtype="<i4").tobytes(), offset, whole=whole)
        b = Placed(torch, np.asarray(right, dtype="<i4").tobytes(), offset) if ch == 2 else None
        return (a.ptr, b.ptr if b else None, P, ch, len(left)), [a] + ([b] if b else [])
    clipped = [np.asarray(x, dtype=np.int64) for x in ((left,) if right is None else (left, right))]
    raw = W.pcm_bytes(clipped[0].astype(np.int32), clipped[1].astype(np.int32) if ch == 2 else None, bits)
    a = Placed(torch, raw, offset, whole=whole)
    return (a.ptr, None, layout, ch, len(left)), [a]


def _layouts(bits):
    return (P, I16) if bits == 16 else (P, I24)


def _message(block, channel, frame, decoded, source, mismatches):
    return (f"[verify-error] block={block} channel={'right' if channel else 'left'} frame={frame} decoded={decoded} "
            f"source={source} mismatches={mismatches}")


def _zero(r):
    return bytes(r) == bytes(32)


def test_pinned_streams_match_their_own_decode(gpu, torch):
    with open(os.path.join(GOLDEN, "decode_wav.json")) as f:
        ents = json.load(f)
    assert len(ents) == 26
    lacs = [lacstreams.from_recipe(e["source"], _fixture) for e in ents]
    assert any(x[2] == 2 for x in lacs) and any(x[2] == 3 for x in lacs)
    dec = gpu.lacx.Decoder(device=0)
    wavs = dec.decode_wav_batch(lacs)
    assert [(len(w), _sha(w)) for w in wavs] == [(e["wav_bytes"], e["wav_sha256"]) for e in ents]
    items, sources, keep = [], [], []
    for lac, wav in zip(lacs, wavs):
        info = gpu.lacx.stream_parse(lac)
        left, right = _wav_pcm(wav, info.channels, info.bit_depth)
        assert left.size == info.frames
        for layout in _layouts(info.bit_depth):
            src, placed = _source(torch, left, right, info.bit_depth, layout)
            items.append(lac), sources.append(src), keep.append(placed)
    assert len(items) == 52
    for lac, src in zip(items, sources):  # singles
        (r,) = dec.verify_batch_device([lac], [src])
        assert _zero(r)
    res = dec.verify_batch_device(items, sources)  # one batch: LACX_OK, or it would have raised
    assert len(res) == 52 and all(_zero(r) for r in res)
    assert dec.last_ms > 0
    assert all(p.untouched() for ps in keep for p in ps)
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


def _placements(left, right, bits, layout, block_frames):
    """[(edits, expected (frame, channel, mismatches))]: edits = [(frame, channel, value)]."""
    frames = left.size
    ch = [left, right]
    b0, b01 = block_frames[0], block_frames[0] + block_frames[1]

    def other(f, c):
        v = int(ch[c][f])
        return v - 1 if v > 0 else v + 1

    out = [
        ([(0, 0, other(0, 0))], (0, 0, 1)),                                   # the first frame
        ([(frames - 1, 1, other(frames - 1, 1))], (frames - 1, 1, 1)),        # the last frame
        ([(b0 - 1, 1, other(b0 - 1, 1))], (b0 - 1, 1, 1)),                    # the last frame of block 0 (mid/side)
        ([(b0, 0, other(b0, 0))], (b0, 0, 1)),                                # the first frame of block 1 (left/right)
        ([(b01 - 1, 0, other(b01 - 1, 0))], (b01 - 1, 0, 1)),                 # ... of block 1, and the first of block 2
        ([(b01, 1, other(b01, 1))], (b01, 1, 1)),
        ([(700, 0, other(700, 0)), (700, 1, other(700, 1))], (700, 0, 2)),    # both channels of a frame: the left one
        ([(5000, 0, other(5000, 0)), (333, 1, other(333, 1))], (333, 1, 2)),  # two frames: the lower one
    ]
    if bits == 24:
        out.append(([(4500, 0, int(left[4500]) ^ 0x400000)], (4500, 0, 1)))   # only the top byte
        out.append(([(4501, 1, int(right[4501]) ^ 0x01)], (4501, 1, 1)))      # only the low byte
    if layout == P:
        out.append(([(258, 1, int(right[258]) + (1 << 24))], (258, 1, 1)))    # equal modulo 2^24
    return out


@pytest.mark.parametrize("bits", [16, 24])
def test_spliced_streams_and_where_they_differ(gpu, torch, bits):
    import dectwin

    lac, left, right, block_frames = _spliced(gpu, bits, 40 + bits)
    ms = list(dectwin.decode(lac).ms)
    assert set(ms) == {0, 1} and any(a != b for a, b in zip(ms, ms[1:])), ms  # a unit spans an LR/MS boundary
    assert ms[0] != ms[1]
    l2, r2, _, _ = gpu.lacx.decode(lac)
    assert np.array_equal(l2, left) and np.array_equal(r2, right)
    block_of = np.repeat(np.arange(len(block_frames)), block_frames)
    dec = gpu.lacx.Decoder(device=0)
    for layout in _layouts(bits):
        items, sources, keep, want = [lac], [], [], [None]
        src, placed = _source(torch, left, right, bits, layout)
        sources.append(src), keep.append(placed)
        for edits, (f, c, n) in _placements(left, right, bits, layout, block_frames):
            sl, sr = left.copy().astype(np.int64), right.copy().astype(np.int64)
            for ef, ec, ev in edits:
                (sr if ec else sl)[ef] = ev
            src, placed = _source(torch, sl, sr, bits, layout)
            items.append(lac), sources.append(src), keep.append(placed)
            want.append((int(block_of[f]), c, f, int((right if c else left)[f]), int((sr if c else sl)[f]), n))
        # an all-different source
        src, placed = _source(torch, left ^ 1, right ^ 1, bits, layout)
        items.append(lac), sources.append(src), keep.append(placed)
        want.append((0, 0, 0, int(left[0]), int(left[0]) ^ 1, 2 * left.size))
        with pytest.raises(gpu.lacx.BatchDecodeError) as e:
            dec.verify_batch_device(items, sources)
        err = e.value
        assert _zero(err.results[0]) and 0 not in err.errors
        for i in range(1, len(items)):
            b, c, f, d, s, n = want[i]
            r = err.results[i]
            assert (r.block, r.channel, r.frame, r.decoded, r.source, r.mismatches) == (b, c, f, d, s, n), (layout, i)
            assert err.errors[i] == _message(b, c, f, d, s, n), (layout, i)
        assert str(err) == "stream 1: " + err.errors[1]
        # ... and one at a time: the same answer, and LACX_E_MISMATCH as the call's code
        import ctypes as C
        lx, L = gpu.lacx, gpu.lacx.lib()
        for i in (1, len(items) - 1):
            buf = np.frombuffer(lac, dtype=np.uint8)
            it = lx.VerifyItem()
            it.lac, it.size = buf.ctypes.data_as(C.POINTER(C.c_uint8)), buf.size
            it.pcm, it.frames = lx.Pcm(*sources[i][:4]), sources[i][4]
            rcs, res = (C.c_int * 1)(), (lx.VerifyResult * 1)()
            rc = L.lacx_decoder_verify_batch_device(dec._h, C.byref(it), 1, None, rcs, res, None)
            assert rc == lx.E_MISMATCH == rcs[0]
            assert L.lacx_decode_last_error().decode() == "stream 0: " + _message(*want[i])
            assert res[0].mismatches == want[i][5] and res[0].frame == want[i][2]
        assert all(p.untouched() for ps in keep for p in ps)
    dec.close()


def test_source_alignment_and_bounds(gpu, torch):
    dec = gpu.lacx.Decoder(device=0)
    whole = torch.empty(10 << 20, dtype=torch.uint8, device="cuda")  # large enough to be an allocation of its own
    for bits in (16, 24):
        lac, left, right, block_frames = _spliced(gpu, bits, 70 + bits)
        frames = left.size
        assert frames % 4 == 3  # a partial last unit
        cases = [(P, 4), (I16, 4)] if bits == 16 else [(P, 4), (P, 12), (I24, 1), (I24, 2), (I24, 3)]
        f, c = frames - 2, 1
        bad_r = right.copy()
        bad_r[f] += 1 if bad_r[f] <= 0 else -1
        want = (int(np.repeat(np.arange(len(block_frames)), block_frames)[f]), c, f, int(right[f]), int(bad_r[f]), 1)
        for layout, offset in cases:
            for at_end in (False, True):
                src, placed = _source(torch, left, right, bits, layout, offset, whole=whole if at_end else None)
                assert at_end or placed[0].ptr % 16 == offset
                assert layout == I24 or src[0] % 4 == 0
                (r,) = dec.verify_batch_device([lac], [src])
                assert _zero(r), (bits, layout, offset, at_end)
                assert all(p.untouched() for p in placed)
                src, placed = _source(torch, left, bad_r, bits, layout, offset, whole=whole if at_end else None)
                with pytest.raises(gpu.lacx.BatchDecodeError) as e:
                    dec.verify_batch_device([lac], [src])
                assert e.value.errors == {0: _message(*want)}, (bits, layout, offset, at_end)
                assert all(p.untouched() for p in placed)
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


def test_mixed_batch(gpu, torch):
    import ctypes as C

    lx, L = gpu.lacx, gpu.lacx.lib()
    left, right = gpu.synth.synth_pcm(16384 * 3 + 77, 2, 24, 96000, seed=5, kind="music")
    lac = lx.Encoder(12, 2, 96000, 24, device=0).encode(left, right)
    damaged, damaged_msg = _damaged(gpu, lac)
    assert damaged_msg.startswith("[decode-error] block=")
    v2 = lacstreams.to_v2(lac)
    f = 16384 + 5
    bad_l = left.copy()
    bad_l[f] ^= 2
    good, k0 = _source(torch, left, right, 24, I24)
    good_p, k1 = _source(torch, left, right, 24, P)
    differs, k2 = _source(torch, bad_l, right, 24, I24)
    msg = _message(1, 0, f, int(left[f]), int(bad_l[f]), 1)
    dec = lx.Decoder(device=0)
    items = [lac, lac, lac[:-1], damaged, v2, lac]
    sources = [good, differs, good, good, good_p, good_p]
    with pytest.raises(lx.BatchDecodeError) as e:
        dec.verify_batch_device(items, sources)
    err = e.value
    assert err.errors == {1: msg, 2: "[decode-error] block payloads do not fill the file", 3: damaged_msg}
    assert str(err) == "stream 1: " + msg
    assert [r is None for r in err.results] == [False, False, True, True, False, False]
    assert all(_zero(err.results[i]) for i in (0, 4, 5)) and err.results[1].mismatches == 1

    def raw(order):
        bufs = [np.frombuffer(items[i], dtype=np.uint8) for i in order]
        its = (lx.VerifyItem * len(order))()
        for it, b, i in zip(its, bufs, order):
            it.lac, it.size = b.ctypes.data_as(C.POINTER(C.c_uint8)), b.size
            it.pcm, it.frames = lx.Pcm(*sources[i][:4]), sources[i][4]
        rcs, res = (C.c_int * len(order))(), (lx.VerifyResult * len(order))()
        rc = L.lacx_decoder_verify_batch_device(dec._h, its, len(order), None, rcs, res, None)
        return rc, list(rcs), res, L.lacx_decode_last_error().decode()

    rc, rcs, res, last = raw([0, 1, 2, 3, 4, 5])
    assert rc == lx.E_MISMATCH and rcs == [lx.OK, lx.E_MISMATCH, lx.E_INVALID, lx.E_RUNTIME, lx.OK, lx.OK]
    assert _zero(res[2]) and _zero(res[3]) and res[1].frame == f
    rc, rcs, res, last = raw([4, 3, 1, 0])  # the lowest failing item decides
    assert rc == lx.E_RUNTIME and rcs == [lx.OK, lx.E_RUNTIME, lx.E_MISMATCH, lx.OK] and last == "stream 1: " + damaged_msg
    rc, rcs, res, last = raw([2, 1])
    assert rc == lx.E_INVALID and last == "stream 0: [decode-error] block payloads do not fill the file"
    rc, rcs, res, last = raw([5, 4, 0])
    assert rc == lx.OK and rcs == [lx.OK] * 3 and all(_zero(res[i]) for i in range(3))
    # the handle still decodes
    l2, r2, _, _ = dec.decode(lac)
    assert np.array_equal(l2, left) and np.array_equal(r2, right)
    assert dec.decode_wav(v2) == W.make_wav(left, right, 96000, 24)
    assert all(p.untouched() for p in k0 + k1 + k2)
    dec.close()


@pytest.mark.parametrize("channels,bits,rate", [(2, 16, 44100), (1, 24, 96000)])
def test_fresh_encode_against_its_wav(gpu, channels, bits, rate):
    frames = 16384 + 37
    left, right = gpu.synth.synth_pcm(frames, channels, bits, rate, seed=90 + bits, kind="mixed")
    wav = W.make_wav(left, right, rate, bits)
    lac = gpu.lacx.Encoder(12, 2 if channels == 2 else 0, rate, bits, device=0).encode_wav(wav)
    dec = gpu.lacx.Decoder(device=0)
    r = dec.verify_wav(lac, wav)
    assert r.identical and _zero(r) and r.message == "" and dec.last_ms > 0
    info = gpu.lacx.wav_parse(wav)
    bps = bits // 8
    f, c = 16384 + 1, channels - 1  # in the second block
    at = info.data_offset + (f * channels + c) * bps  # the sample's low byte
    changed = bytearray(wav)
    changed[at] ^= 0x10
    src = int((right if c else left)[f])
    r = dec.verify_wav(lac, bytes(changed))
    assert not r.identical and not r.format_differs
    assert (r.mismatches, r.frame, r.channel, r.block, r.decoded, r.source) == (1, f, c, 1, src, src ^ 0x10)
    assert r.message == _message(1, c, f, src, src ^ 0x10, 1)  # no "stream 0: "
    changed = bytearray(wav)
    changed[info.data_offset + info.data_bytes - 1] ^= 0x80  # the top byte of the last sample
    r = dec.verify_wav(lac, bytes(changed))
    assert (r.mismatches, r.frame, r.channel) == (1, frames - 1, channels - 1)
    assert dec.verify_wav(lac, wav).identical
    dec.close()


def _cli():
    subprocess.check_call(["make", "-C", PKG_DIR, "lacx_cli"], stdout=subprocess.DEVNULL)
    return os.path.join(PKG_DIR, "lacx_cli")


def test_cli_selftest(gpu):
    res = subprocess.run([_cli(), "selftest"], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    lines = res.stdout.splitlines()
    assert len(lines) == 5 and lines[-1] == "Selftest complete: adaptive block tests passed."
    for line, (rate, depth) in zip(lines, ((44100, 16), (48000, 24), (96000, 24), (192000, 24))):
        assert line.startswith(f"Selftest sr={rate}Hz depth={depth} LR=") and " MS=" in line and " -> MS is " in line


def test_cli_verify(gpu, tmp_path):
    cli = _cli()
    left, right = gpu.synth.synth_pcm(16384 + 37, 2, 16, 48000, seed=3, kind="music")
    wav = W.make_wav(left, right, 48000, 16)
    wav_path, lac_path = str(tmp_path / "in.wav"), str(tmp_path / "out.lac")
    with open(wav_path, "wb") as f:
        f.write(wav)
    res = subprocess.run([cli, "encode", wav_path, lac_path, "--verify"], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and res.stdout.startswith("Encoded "), res.stderr
    with open(lac_path, "rb") as f:
        assert f.read() == gpu.lacx.Encoder(12, 2, 48000, 16, device=0).encode(left, right)
    res = subprocess.run([cli, "verify", lac_path, wav_path], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    assert res.stdout == f"Verified {lac_path} == {wav_path} (16421 samples per channel)\n"
    # one changed sample: verify names the frame and exits 1
    frame = 9000
    bad_left = left.copy()
    bad_left[frame] += 3 if bad_left[frame] < 0 else -3
    bad_path = str(tmp_path / "changed.wav")
    with open(bad_path, "wb") as f:
        f.write(W.make_wav(bad_left, right, 48000, 16))
    res = subprocess.run([cli, "verify", lac_path, bad_path], capture_output=True, text=True, timeout=120)
    assert res.returncode == 1 and res.stdout == ""
    assert res.stderr == "Verify failed: " + _message(0, 0, frame, int(left[frame]), int(bad_left[frame]), 1) + "\n"
    other = subprocess.run([cli, "verify", lac_path, str(tmp_path / "none.wav")], capture_output=True, text=True, timeout=120)
    assert other.returncode == 1 and "Failed to read WAV" in other.stderr


def test_cli_encode_verify_publishes_nothing_on_a_mismatch(gpu, tmp_path):
    """`encode --verify` compares the produced bytes with the source before the staged output is renamed.  A correct
    encoder never differs from its input, so the mismatch comes from --verify-against: another copy of the source, with
    one changed sample."""
    cli = _cli()
    left, _ = gpu.synth.synth_pcm(4097, 1, 24, 96000, seed=4, kind="mixed")
    wav = W.make_wav(left, None, 96000, 24)
    wav_path, lac_path, other_path = str(tmp_path / "m.wav"), str(tmp_path / "m.lac"), str(tmp_path / "other.wav")
    bad = left.copy()
    bad[4096] ^= 0x010000
    with open(wav_path, "wb") as f:
        f.write(wav)
    with open(other_path, "wb") as f:
        f.write(W.make_wav(bad, None, 96000, 24))
    res = subprocess.run([cli, "encode", wav_path, lac_path, "--verify-against=" + other_path], capture_output=True, text=True,
                         timeout=120)
    assert res.returncode == 1 and res.stdout == ""
    assert res.stderr == "Verify failed: " + _message(0, 0, 4096, int(left[4096]), int(bad[4096]), 1) + "\n"
    assert sorted(os.listdir(tmp_path)) == ["m.wav", "other.wav"]  # neither the output nor its staged file
    res = subprocess.run([cli, "encode", wav_path, lac_path, "--verify", "--no-partitioning"], capture_output=True, text=True,
                         timeout=120)
    assert res.returncode == 0, res.stderr
    assert sorted(os.listdir(tmp_path)) == ["m.lac", "m.wav", "other.wav"]
    with open(lac_path, "rb") as f:
        assert gpu.lacx.Decoder(device=0).verify_wav(f.read(), wav).identical
    res = subprocess.run([cli, "encode", wav_path, lac_path, "--verify=1"], capture_output=True, text=True, timeout=120)
    assert res.returncode == 1 and "Usage:" in res.stderr
