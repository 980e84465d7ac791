"""`lacx_cli decode` and lacx.decode_wav without a device: the reference CLI's argument checks and messages (ref
src/main.cpp:712-781), structural errors found by the host-side parse before any device is touched, and the pinned
reference WAV images of tests/golden/decode_wav.json checked against the PCM they were made from."""
import hashlib
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import __graft_entry__ as ge
import lacstreams
import wavutil as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
PKG_DIR = os.path.join(ROOT, "lossless-audio-codec_amd")


@pytest.fixture(scope="module")
def cli():
    subprocess.check_call(["make", "-C", PKG_DIR, "lacx_cli"], stdout=subprocess.DEVNULL)
    return os.path.join(PKG_DIR, "lacx_cli")


@pytest.fixture(scope="module")
def pkg():
    mod = ge.load_pkg()
    if not os.path.exists(mod.lacx.LIB_PATH):
        mod.lacx.build()
    return mod


def _fixture(name):
    with open(os.path.join(GOLDEN, name), "rb") as f:
        return f.read()


def _entries():
    with open(os.path.join(GOLDEN, "decode_wav.json")) as f:
        return json.load(f)


def _run(cli, args, env=None):
    return subprocess.run([cli] + args, capture_output=True, text=True, env=env)


def test_same_file_is_refused(cli, tmp_path):
    lac = tmp_path / "a.lac"
    lac.write_bytes(_fixture("small/n33_mono16.lac"))
    before = lac.read_bytes()
    link = tmp_path / "alias.lac"
    os.symlink(lac, link)
    for other in (str(lac), str(tmp_path / "." / "a.lac"), str(link)):
        res = _run(cli, ["decode", str(lac), other])
        assert res.returncode == 1 and "Input and output paths must be different" in res.stderr, res.stderr
    assert lac.read_bytes() == before


def test_argument_rejections(cli, tmp_path):
    lac = tmp_path / "a.lac"
    lac.write_bytes(_fixture("small/n33_mono16.lac"))
    out = tmp_path / "o.wav"
    res = _run(cli, ["decode", str(lac), str(out), "--threads=0"])
    assert res.returncode == 1 and "Error: --threads requires a positive integer" in res.stderr
    for bad_env in ("0", "x3", "-1"):
        res = _run(cli, ["decode", str(lac), str(out)], env=dict(os.environ, LAC_THREADS=bad_env))
        assert res.returncode == 1 and "Error: LAC_THREADS must be a positive integer" in res.stderr, bad_env
    res = _run(cli, ["decode", str(lac), str(out)], env=dict(os.environ, LAC_THREADS="9" * 19))
    assert res.returncode == 1 and "Error: LAC_THREADS is too large" in res.stderr
    res = _run(cli, ["decode", str(tmp_path / "missing.lac"), str(out)])
    assert res.returncode == 1 and f"Failed to read LAC file: {tmp_path / 'missing.lac'}" in res.stderr
    res = _run(cli, ["decode", str(lac), str(out), "--bogus"])
    assert res.returncode == 1 and "decode input.lac output.wav" in res.stderr
    res = _run(cli, ["decode", str(lac)])
    assert res.returncode == 1 and "Usage:" in res.stderr
    assert not out.exists()


def test_malformed_stream_fails_before_the_device(cli, tmp_path):
    good = _fixture("small/n4097_st16.lac")
    bad_sync = bytes([0x00]) + good[1:]
    truncated = good[:14 + 4]  # one block announced, its table entry cut in half
    for name, data, msg in (("sync", bad_sync, "invalid frame header"), ("table", truncated, "truncated block size table")):
        src = tmp_path / f"{name}.lac"
        src.write_bytes(data)
        out = tmp_path / f"{name}.wav"
        res = _run(cli, ["decode", str(src), str(out)])
        assert res.returncode == 1
        assert f"Decode failed: [decode-error] {msg}" in res.stderr, res.stderr
        assert not out.exists() and not (tmp_path / f"{name}.wav.lacx-partial").exists()


def test_python_decode_wav_errors(pkg):
    with pytest.raises(RuntimeError, match=r"\[decode-error\] invalid frame header"):
        pkg.lacx.decode_wav(b"XX" + _fixture("small/n33_mono16.lac")[2:])
    with pytest.raises(RuntimeError, match=r"\[decode-error\] empty input"):
        pkg.lacx.Decoder().decode_wav(b"")
    if pkg.lacx.device_count() > 0:
        pytest.skip("a device is present: the no-device message cannot be observed")
    with pytest.raises(RuntimeError, match="no usable HIP device"):
        pkg.lacx.decode_wav(_fixture("small/n33_mono16.lac"))
    with pytest.raises(RuntimeError, match="no usable HIP device"):
        pkg.lacx.Decoder().decode_wav_view(_fixture("small/n33_mono16.lac"))


def pcm_of(entry, synth):
    """The PCM a pinned stream decodes to, regenerated from its recorded generator parameters."""
    ls, rs = [], []
    for seg in entry["pcm"]:
        g = seg["gen"]
        left, right = synth.synth_pcm(g["frames"], g["channels"], g["bit_depth"], g["sample_rate"], seed=g["seed"],
                                      kind=g["kind"], stereo=g["stereo"])
        ls.append(left[seg["start"]:seg["end"]])
        if right is not None:
            rs.append(right[seg["start"]:seg["end"]])
    g = entry["pcm"][0]["gen"]
    return np.concatenate(ls), (np.concatenate(rs) if rs else None), g["sample_rate"], g["bit_depth"]


def test_pinned_reference_wavs_match_their_pcm(pkg):
    entries = _entries()
    assert len(entries) >= 20
    kinds = set()
    for ent in entries:
        lac = lacstreams.from_recipe(ent["source"], _fixture)
        assert hashlib.sha256(lac).hexdigest() == ent["lac_sha256"], ent["name"]
        info = pkg.lacx.stream_parse(lac)
        assert info is not None, ent["name"]
        left, right, rate, bits = pcm_of(ent, pkg.synth)
        wav = W.make_wav(left, right, rate, bits)
        assert len(wav) == ent["wav_bytes"] and hashlib.sha256(wav).hexdigest() == ent["wav_sha256"], ent["name"]
        # the header's documented fields (ref src/main.cpp:127-148)
        h = bytes.fromhex(ent["header_hex"])
        riff, fmt_size, tag, ch, sr, byte_rate, align, bps, data = struct.unpack("<4xI8xIHHIIHH4xI", h)
        assert h[:4] == b"RIFF" and h[8:16] == b"WAVEfmt " and h[36:40] == b"data"
        assert (fmt_size, tag, ch, sr, bps) == (16, 1, info.channels, info.sample_rate, info.bit_depth)
        assert align == ch * bps // 8 and byte_rate == sr * align
        assert data == info.frames * align and riff == 36 + data + (data & 1) == ent["wav_bytes"] - 8
        assert ent["stdout"] == f"Decoded {{in}} -> {{out}} ({info.frames} samples per channel)\n"
        kinds.add((info.version, data & 1, min(lacstreams.block_frames(lac)[:-1] or [16384]) if info.version == 3 else 0))
    # the set covers a version-2 stream, an odd data size and odd non-final blocks
    assert any(v == 2 for v, _, _ in kinds) and any(p for _, p, _ in kinds) and any(m % 2 for _, _, m in kinds)
