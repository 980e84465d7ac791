"""lacx_decoder_decode_wav / lacx.decode_wav / `lacx_cli decode` on the MI355X: the reference CLI's WAV bytes for every
pinned stream (tests/golden/decode_wav.json: version 2, odd non-final blocks, the pad byte), WAV -> LAC -> WAV identity,
agreement with the pinned PCM decoder, the same errors as lacx.decode (the bit-depth check now runs in k_wav_pack), the
stream sizes users run, and the CLI command end to end."""
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


@pytest.fixture(scope="module")
def gpu():
    pkg = ge.load_pkg()
    if pkg.lacx.device_count() <= 0:
        pytest.fail("no HIP device: the decoder has no CPU fallback")
    return pkg


@pytest.fixture(scope="module")
def cli():
    subprocess.check_call(["make", "-C", PKG_DIR, "lacx_cli"], stdout=subprocess.DEVNULL)
    return os.path.join(PKG_DIR, "lacx_cli")


def _fixture(name):
    with open(os.path.join(GOLDEN, name), "rb") as f:
        return f.read()


def _entries():
    with open(os.path.join(GOLDEN, "decode_wav.json")) as f:
        return json.load(f)


def _sha(b):
    return hashlib.sha256(bytes(b)).hexdigest()


def test_pinned_reference_wavs(gpu):
    dec = gpu.lacx.Decoder(device=0)
    for ent in _entries():
        lac = lacstreams.from_recipe(ent["source"], _fixture)
        wav = dec.decode_wav(lac)
        assert (len(wav), _sha(wav)) == (ent["wav_bytes"], ent["wav_sha256"]), ent["name"]
        view = dec.decode_wav_view(lac)
        assert view.dtype == np.uint8 and (view.size, _sha(view)) == (ent["wav_bytes"], ent["wav_sha256"]), ent["name"]
        assert bytes(view[:44]).hex() == ent["header_hex"]
        assert gpu.lacx.decode_wav(lac) == wav
    dec.close()


@pytest.mark.parametrize("ch,bd", [(1, 16), (1, 24), (2, 16), (2, 24)])
def test_wav_lac_wav_identity(gpu, ch, bd):
    dec = gpu.lacx.Decoder(device=0)
    rate = 48000 if bd == 16 else 96000
    for frames in (1, 255, 256, 257, 4097, 16384, 16385, 3 * 16384 + 1):
        left, right = gpu.synth.synth_pcm(frames, ch, bd, rate, seed=frames % 97 + ch, kind="mixed")
        wav = W.make_wav(left, right, rate, bd)
        for sm in ((0, 1, 2) if ch == 2 else (0,)):
            lac = gpu.lacx.Encoder(12, sm, rate, bd, device=0).encode_wav(wav)
            assert dec.decode_wav(lac) == wav, (frames, sm)
    dec.close()


def _sweep_streams(gpu):
    """About forty streams: materials, depths, stereo modes, odd lengths, spliced streams with odd non-final blocks, and
    version-2 rewrites: (streams, the canonical WAV of each stream's encoded PCM)."""
    rng = np.random.default_rng(4242)
    kinds = ("music", "mixed", "noise", "tone", "sparse", "walk", "silence")
    out, wavs = [], []
    for i in range(28):
        ch = int(rng.integers(1, 3))
        bd = int(rng.choice([16, 24]))
        rate = int(rng.choice([44100, 48000, 96000, 192000]))
        sm = int(rng.integers(0, 3)) if ch == 2 else 0
        frames = int(rng.integers(1, 5 * 16384))
        left, right = gpu.synth.synth_pcm(frames, ch, bd, rate, seed=1000 + i, kind=kinds[i % len(kinds)])
        lac = gpu.lacx.Encoder(12, sm, rate, bd, device=0).encode(left, right)
        out.append(lac)
        wavs.append(W.make_wav(left, right, rate, bd))
        if i % 4 == 0:
            out.append(lacstreams.to_v2(lac))
            wavs.append(wavs[-1])
        if i % 3 == 0 and frames > 257:
            # an odd-length first block: a stream of n frames spliced in front of the stream
            n = 2 * int(rng.integers(128, 8192)) + 1  # 257 .. 16383
            l2, r2 = gpu.synth.synth_pcm(n, ch, bd, rate, seed=2000 + i, kind="mixed")
            head = gpu.lacx.Encoder(12, sm, rate, bd, device=0).encode(l2, r2)
            out.append(lacstreams.splice(head, lac))
            wavs.append(W.make_wav(np.concatenate([l2, left]), None if ch == 1 else np.concatenate([r2, right]), rate, bd))
    return out, wavs


def test_agrees_with_the_pcm_decoder(gpu):
    dec = gpu.lacx.Decoder(device=0)
    streams, wavs = _sweep_streams(gpu)
    assert len(streams) >= 38
    for k, lac in enumerate(streams):
        left, right, info, _ = gpu.lacx.decode(lac)
        want = W.make_wav(left, right, info.sample_rate, info.bit_depth)
        assert want == wavs[k], k
        assert dec.decode_wav(lac) == want, k
        assert bytes(dec.decode_wav_view(lac)) == want, k
    dec.close()


def _raises_like_decode(gpu, dec, lac):
    with pytest.raises(RuntimeError) as want:
        gpu.lacx.decode(lac)
    with pytest.raises(RuntimeError) as got:
        dec.decode_wav(lac)
    assert str(got.value) == str(want.value)
    with pytest.raises(RuntimeError) as got:
        dec.decode_wav_view(lac)
    assert str(got.value) == str(want.value)
    return str(want.value)


def test_errors_match_decode(gpu):
    dec = gpu.lacx.Decoder(device=0)
    left, right = gpu.synth.synth_pcm(16384 * 3 + 77, 2, 24, 96000, seed=5, kind="music")
    lac = gpu.lacx.Encoder(12, 2, 96000, 24, device=0).encode(left, right)
    wav = W.make_wav(left, right, 96000, 24)
    # a loud 24-bit stream declared 16-bit: blocks decode, samples leave the depth (status 7, from k_wav_pack)
    loud = bytearray(lac)
    loud[8] = 16
    msg = _raises_like_decode(gpu, dec, bytes(loud))
    assert "sample outside the bit depth" in msg
    assert dec.decode_wav(lac) == wav
    # a damaged payload, a truncated stream, a bad header
    bad = bytearray(lac)
    bad[len(bad) // 2] ^= 0x55
    try:
        gpu.lacx.decode(bytes(bad))
        assert dec.decode_wav(bytes(bad)) == W.make_wav(*gpu.lacx.decode(bytes(bad))[:2], 96000, 24)
    except RuntimeError:
        _raises_like_decode(gpu, dec, bytes(bad))
    assert "decode-error" in _raises_like_decode(gpu, dec, lac[:-1])
    assert "invalid frame header" in _raises_like_decode(gpu, dec, b"LA\x07" + lac[3:])
    assert dec.decode_wav(lac) == wav
    assert bytes(dec.decode_wav_view(lac)) == wav
    dec.close()


@pytest.mark.parametrize("secs,bd,rate,kind", [(600, 16, 48000, "music"), (150, 24, 96000, "mixed")])
def test_sizes_users_run(gpu, secs, bd, rate, kind):
    left, right = gpu.synth.synth_pcm(secs * rate, 2, bd, rate, seed=2026 if bd == 16 else 7, kind=kind, stereo="wide")
    lac = gpu.lacx.Encoder(12, 2, rate, bd, device=0).encode(left, right)
    wav = W.make_wav(left, right, rate, bd)
    del left, right
    dec = gpu.lacx.Decoder(device=0)
    assert _sha(dec.decode_wav_view(lac)) == _sha(wav)
    assert dec.decode_wav(lac) == wav
    dec.close()


def test_cli_decode(gpu, cli, tmp_path):
    for ent in _entries():
        src = tmp_path / "in.lac"
        src.write_bytes(lacstreams.from_recipe(ent["source"], _fixture))
        out = tmp_path / "out.wav"
        res = subprocess.run([cli, "decode", str(src), str(out)], capture_output=True, text=True)
        assert res.returncode == 0, res.stderr
        data = out.read_bytes()
        assert (len(data), _sha(data)) == (ent["wav_bytes"], ent["wav_sha256"]), ent["name"]
        assert res.stdout == ent["stdout"].replace("{in}", str(src)).replace("{out}", str(out))
        assert not (tmp_path / "out.wav.lacx-partial").exists()
    # encode then decode reproduces a canonical WAV
    left, right = gpu.synth.synth_pcm(16384 * 2 + 4321, 2, 24, 96000, seed=51, kind="mixed")
    wav = tmp_path / "a.wav"
    wav.write_bytes(W.make_wav(left, right, 96000, 24))
    lac = tmp_path / "a.lac"
    assert subprocess.run([cli, "encode", str(wav), str(lac)], capture_output=True).returncode == 0
    for flags, env in (([], None), (["--threads=3"], None), ([], dict(os.environ, LAC_THREADS="3")), (["--debug-threads"], None)):
        back = tmp_path / "b.wav"
        res = subprocess.run([cli, "decode", str(lac), str(back)] + flags, capture_output=True, text=True, env=env)
        assert res.returncode == 0, res.stderr
        assert back.read_bytes() == wav.read_bytes()
        assert f"Decoded {lac} -> {back} ({16384 * 2 + 4321} samples per channel)" in res.stdout
        if flags == ["--debug-threads"]:
            assert "Decoder thread usage: 1 threads" in res.stdout
            assert "WARNING: Decoder multi-threading may not be active." in res.stdout
        back.unlink()
    # a stream that parses but does not decode leaves neither the output nor the partial file
    loud = bytearray(lac.read_bytes())
    loud[8] = 16
    bad = tmp_path / "loud.lac"
    bad.write_bytes(bytes(loud))
    out = tmp_path / "loud.wav"
    res = subprocess.run([cli, "decode", str(bad), str(out)], capture_output=True, text=True)
    assert res.returncode == 1 and "Decode failed: [decode-error] block=" in res.stderr, res.stderr
    assert not out.exists() and not (tmp_path / "loud.wav.lacx-partial").exists()
