"""The device-emit encoder's host-side paths on the MI355X: every way the shard plan (csrc/encode_plan.h) can cut a call
into pipeline chunks and every mode flag it can set, through the three kinds of entry point -- host arrays (the uploader
thread feeds the chunks), planar PCM that is already on the device, and a WAV image (chunk bases are byte offsets into the
interleaved data chunk).  The knobs change how the work is enqueued, never the bytes: each result is compared byte for
byte with the oracle, twice per encoder (the second call runs on warm buffers).

Small streams: 16384*5 + 321 frames of 16-bit stereo in per-block stereo mode (six blocks, the last one short enough to
be encoded both ways, so it stays out of the fused emit) and 16384*3 + 5 frames of 24-bit mono.  One large one:
16384*1024 + 7 frames, 1024 blocks being the smallest shard whose front kernels are launched in two halves."""
import functools

import numpy as np
import pytest

import wavutil as W

pytestmark = pytest.mark.gpu

SMALL = [
    # frames, channels, bit_depth, stereo_mode, kind
    (16384 * 5 + 321, 2, 16, 2, "mixed"),
    (16384 * 3 + 5, 1, 24, 0, "music"),
]
RATE = 48000
SMALL_CAP = "20000"  # bytes; the small streams need several times as much

SETTINGS = {
    "chunks3": {"LACX_PIPE_CHUNKS": "3"},
    "split123": {"LACX_PIPE_SPLIT": "1,2,3"},
    "chunks3_unfused": {"LACX_PIPE_CHUNKS": "3", "LACX_FUSED_EMIT": "0"},
    "chunks3_small_cap": {"LACX_PIPE_CHUNKS": "3", "LACX_PINNED_CAP_BYTES": SMALL_CAP},
    "direct_packer": {"LACX_DIRECT_PACKER": "1"},
    "no_lazy_repair": {"LACX_NO_LAZY_REPAIR": "1"},
    "no_persistent": {"LACX_NO_PERSISTENT": "1"},
    "no_packer": {"LACX_NO_PACKER": "1"},
}


@pytest.fixture(scope="module")
def gpu(pkg):
    if pkg.lacx.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests need an MI355X (the product has no CPU fallback)")
    return pkg


@functools.lru_cache(maxsize=None)
def _stream(pkg, oracle, case):
    """(left, right, the oracle's .lac) of a case: computed once, shared by every test, never written to."""
    frames, ch, bd, sm, kind = case
    left, right = pkg.synth.synth_pcm(frames, ch, bd, RATE, seed=29, kind=kind)
    want = oracle.encode(left, right, RATE, bd, sm, threads=8)
    left.setflags(write=False)
    if right is not None:
        right.setflags(write=False)
    return left, right, want


def _encode(entry, enc, left, right, dev):
    if entry == "host_arrays":
        return enc.encode(left, right)
    if entry == "wav_image":
        return enc.encode_wav(dev)
    dl, dr = dev
    return enc.encode_device(dl.data_ptr(), None if dr is None else dr.data_ptr(), left, right, left.size)


def _device_input(entry, left, right, bd):
    if entry == "wav_image":
        return W.make_wav(left, right, RATE, bd)
    if entry == "device_planar":
        import torch

        return tuple(None if x is None else torch.from_numpy(np.array(x)).cuda() for x in (left, right))
    return None


@pytest.mark.parametrize("entry", ["host_arrays", "device_planar", "wav_image"])
@pytest.mark.parametrize("setting", sorted(SETTINGS))
def test_small_streams_under_every_setting(gpu, oracle, monkeypatch, setting, entry):
    for name, value in SETTINGS[setting].items():
        monkeypatch.setenv(name, value)
    for case in SMALL:
        frames, ch, bd, sm, kind = case
        left, right, want = _stream(gpu, oracle, case)
        dev = _device_input(entry, left, right, bd)
        enc = gpu.lacx.Encoder(12, sm, RATE, bd, device=0)  # (the knobs are read when the encoder is created)
        for again in range(2):
            got = _encode(entry, enc, left, right, dev)
            assert got == want, (setting, entry, case, again)
            # a reservation that is too small: one re-emit over all three chunks, counted once
            assert enc.timing().regrows == (1 if setting == "chunks3_small_cap" else 0), (setting, entry, case, again)
        enc.close()


BIG = (16384 * 1024 + 7, 2, 16, 2, "music")


@pytest.mark.parametrize("halves", [True, False], ids=["front_halves", "no_front_halves"])
def test_1024_blocks_with_and_without_the_two_halves_front(gpu, oracle, monkeypatch, halves):
    """Default knobs: one chunk, persistent analysis, lazy repair, and -- from 1024 blocks on -- the front kernels in two
    block halves on two streams; LACX_NO_FRONT_HALVES=1 keeps them on one."""
    if not halves:
        monkeypatch.setenv("LACX_NO_FRONT_HALVES", "1")
    left, right, want = _stream(gpu, oracle, BIG)
    dev = _device_input("device_planar", left, right, 16)
    enc = gpu.lacx.Encoder(12, 2, RATE, 16, device=0)
    for again in range(2):
        assert _encode("device_planar", enc, left, right, dev) == want, (halves, again)
        assert enc.timing().regrows == 0
    enc.close()
