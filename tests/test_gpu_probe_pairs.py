"""The probe class with two slots per wave (the halves of a wave take the slots 4 + 2i and 5 + 2i of a block): whole streams
against the oracle's .lac, byte for byte, on material chosen for the pairing -- every block probed, the two slots of a pair
of different character (one silent, one noise; one half done after one candidate, the other after several), final blocks
with and without probe windows, and streams without any probes."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BLOCK = 16384
PROBE = 256


@pytest.fixture(scope="module")
def gpu(pkg):
    if pkg.lacx.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests need an MI355X (the product has no CPU fallback)")
    return pkg


def _noise(gpu, frames, bits, seed):
    left, right = gpu.synth.synth_pcm(frames, 2, bits, 48000, seed=seed, kind="noise", stereo="independent")
    return left.copy(), right.copy()


def _same(gpu, oracle, left, right, bits, mode=2, rate=48000):
    got = gpu.lacx.Encoder(12, mode, rate, bits, device=0).encode(left, right)
    want = oracle.encode(left, right, rate, bits, mode)
    assert len(got) == len(want)
    assert got == want


def _probed_blocks(gpu, left, right, bits):
    """Blocks of the stream whose LR/MS choice went through the probe slots (their probe plans are valid)."""
    _, plans = gpu.lacx.Encoder(12, 2, 48000, bits, device=0).analyze(left, right)
    nb = (left.size + BLOCK - 1) // BLOCK
    return [b for b in range(nb) if any(plans[b * 16 + s].valid for s in range(4, 16))]


@pytest.mark.parametrize("bits", [16, 24])
def test_every_block_probed(gpu, oracle, bits):
    left, right = _noise(gpu, 9 * BLOCK + 7001, bits, 3)
    assert len(_probed_blocks(gpu, left, right, bits)) >= 9  # the material does what it is here for
    _same(gpu, oracle, left, right, bits)


@pytest.mark.parametrize("bits", [16, 24])
def test_pair_of_different_character(gpu, oracle, bits):
    """Per block one of: left silent in a probe window (the L/R pair: silence beside noise), left == right there (the M/S
    pair: noise beside silence), both silent in the last window only, a constant beside noise."""
    nb = 8
    left, right = _noise(gpu, nb * BLOCK, bits, 11)
    windows = [0, (BLOCK - PROBE) // 2, BLOCK - PROBE]
    for b in range(nb):
        w = b * BLOCK + windows[b % 3]
        sel = slice(w, w + PROBE)
        if b % 4 == 0:
            left[sel] = 0
        elif b % 4 == 1:
            right[sel] = left[sel]
        elif b % 4 == 2:
            left[sel] = 0
            right[sel] = 0
        else:
            right[sel] = -1234
    assert len(_probed_blocks(gpu, left, right, bits)) >= nb // 2
    _same(gpu, oracle, left, right, bits)


@pytest.mark.parametrize("bits", [16, 24])
@pytest.mark.parametrize("last", [1, 13, 255, 256, 300, 4096, 4097, 5000, BLOCK - 1])
def test_short_final_block(gpu, oracle, bits, last):
    """Final blocks at and around the sizes where the probe windows stop existing (<= 4096 frames: compared in full) and
    where they overlap."""
    left, right = _noise(gpu, 2 * BLOCK + last, bits, 17)
    _same(gpu, oracle, left, right, bits)


@pytest.mark.parametrize("bits", [16, 24])
def test_streams_without_probes(gpu, oracle, bits):
    left, right = _noise(gpu, 3 * BLOCK + 999, bits, 29)
    _same(gpu, oracle, left, None, bits, mode=0)   # mono
    _same(gpu, oracle, left, right, bits, mode=0)  # forced left/right
    _same(gpu, oracle, left, right, bits, mode=1)  # forced mid/side


@pytest.mark.parametrize("bits", [16, 24])
def test_music_and_mixed_material(gpu, oracle, bits):
    for kind, seed in (("music", 5), ("mixed", 7)):
        left, right = gpu.synth.synth_pcm(6 * BLOCK + 4500, 2, bits, 48000, seed=seed, kind=kind)
        _same(gpu, oracle, left, right, bits)


@pytest.mark.parametrize("bits", [16, 24])
def test_near_silent_probe_windows(gpu, oracle, bits):
    """A few +-1 samples in otherwise silent probe windows: the LPC candidates win there by a few bits, so every word of
    the pruning bounds counts (candidate 10's run ends are the last word of a table one longer than a slot has lanes)."""
    rng = np.random.default_rng(41)
    nb = 12
    left, right = _noise(gpu, nb * BLOCK, bits, 43)
    for b in range(nb):
        for w in (0, (BLOCK - PROBE) // 2, BLOCK - PROBE):
            sel = slice(b * BLOCK + w, b * BLOCK + w + PROBE)
            for x in (left, right):
                x[sel] = 0
                x[b * BLOCK + w + rng.integers(0, PROBE, 3)] = rng.choice([-1, 1], 3)
    _same(gpu, oracle, left, right, bits)
