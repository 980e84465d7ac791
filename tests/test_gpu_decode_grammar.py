"""Decoder conformance on the MI355X: the hand-built streams of lacgrammar.py -- every LPC order, extreme coefficients,
Rice parameters 0..31, long unary runs, the adaptation beyond 2^31, every token spelling of the zero-run and bin modes,
every partition order, mixed waves -- through lacx.decode, Decoder.decode_wav_batch, the version-2 serial kernel and
decode_window, bit-exact against the generator's Python-integer samples (tests/test_lacgrammar_host.py proves those
against the oracle and the reference).  Refused cases must be refused for the rule they break, and alone.

Known limit: the device refuses any zigzag value >= 2^30 (status 9) where the reference would decode; only the
`beyond_2p30_*` cases, whose largest value is that large, may expect it."""
import re

import numpy as np
import pytest

import __graft_entry__ as ge
import lacgrammar as g
import lacstreams
import wavutil

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    pkg = ge.load_pkg()
    if pkg.lacx.device_count() <= 0:
        pytest.fail("no HIP device: the decoder has no CPU fallback")
    return pkg


def _message(s):
    """The whole error text of a refused case: block and status."""
    return r"\[decode-error\] block=%d %s$" % (s.bad_block, re.escape(g.STATUS_TEXT[s.status]))


def _assert_pcm(s, left, right, what):
    assert np.array_equal(left, np.array(s.left, dtype=np.int64)), what
    assert (right is None) == (s.right is None), what
    if right is not None:
        assert np.array_equal(right, np.array(s.right, dtype=np.int64)), what


def _wav(s):
    return wavutil.make_wav(np.array(s.left, dtype=np.int32), None if s.right is None else np.array(s.right, dtype=np.int32),
                            s.rate, s.bit_depth)


@pytest.mark.parametrize("name", g.ALL_NAMES)
def test_decode(gpu, name):
    s = g.build(name)
    if s.status:
        with pytest.raises(RuntimeError, match=_message(s)):
            gpu.lacx.decode(s.lac)
        return
    left, right, info, _ = gpu.lacx.decode(s.lac)
    _assert_pcm(s, left, right, name)
    assert (info.frames, info.blocks, info.channels, info.bit_depth) == (len(s.left), len(s.frames), s.channels, s.bit_depth)


def test_single_block_cases_share_waves(gpu):
    """All valid single-block cases of one format as ONE batch: consecutive lanes of a wave hold an LPC order-32 block, a
    static-Rice block, a 5000-bit unary run, a stateful bin block ...  Each image is what the case gives alone."""
    groups = {}
    for name in g.CASES:
        s = g.build(name)
        if s.status == 0 and len(s.frames) == 1:
            groups.setdefault((s.channels, s.bit_depth, s.rate, s.stereo_mode), []).append(name)
    assert sum(len(v) for v in groups.values()) > 200 and max(len(v) for v in groups.values()) > 128
    dec = gpu.lacx.Decoder()
    for key, names in groups.items():
        images = dec.decode_wav_batch([g.build(n).lac for n in names])
        for n, img in zip(names, images):
            assert img == _wav(g.build(n)), (key, n)
    dec.close()


def test_failing_blocks_fail_alone(gpu):
    """96 single-block streams as one batch, every fifth a refused case: each refused one reports its own rule, and its
    neighbours in the wave decode to the generator's samples."""
    mix = g.failure_mix()
    dec = gpu.lacx.Decoder()
    with pytest.raises(gpu.lacx.BatchDecodeError) as err:
        dec.decode_wav_batch([s.lac for _, s in mix])
    e = err.value
    assert sorted(e.errors) == [i for i, (name, _) in enumerate(mix) if name is not None]
    for i, (name, s) in enumerate(mix):
        if name is None:
            assert e.results[i] == _wav(s), i
        else:
            assert re.search(_message(s), e.errors[i]), (i, name, e.errors[i])
    dec.close()


@pytest.mark.parametrize("name", g.V2_SUBSET + ["wave_mix_rotating_families", "sweep_03", "sweep_11"])
def test_version_2_rewrites(gpu, name):
    """The same blocks behind a version-2 table: one lane of k_decode_serial walks them."""
    s = g.build(name)
    assert s.status == 0
    v2 = lacstreams.to_v2(s.lac)
    left, right, info, _ = gpu.lacx.decode(v2)
    assert info.version == 2
    _assert_pcm(s, left, right, name)


def test_version_2_refusal_names_the_block(gpu):
    """A refused block in the middle of a version-2 stream: the blocks before it decode, it is named, the rest is not reached."""
    rng_blocks = [g.Block([g.random_channel_block(g._rng("v2r%d" % i), 300, 24, family=g.FAMILIES[i % 5])]) for i in range(5)]
    bad = g.ChannelBlock(300, 0, 0, [], 0, [g.Part(g.MODE_ZERO_RUN, 3, tokens=[("n", 1)] * 290 + [("r", 11)])])  # one beyond
    rng_blocks[3] = g.Block([bad])
    s = g.make_stream(rng_blocks)
    with pytest.raises(RuntimeError, match=r"\[decode-error\] block=3 residual$"):
        gpu.lacx.decode(s.lac)
    with pytest.raises(RuntimeError, match=r"\[decode-error\] block=3 residual$"):
        gpu.lacx.decode(lacstreams.to_v2(s.lac))


@pytest.mark.parametrize("name", ["wave_mix_rotating_families", "wave_mix_shuffled_families", "sweep_05", "sweep_17"])
def test_windows_across_foreign_seams(gpu, name):
    s = g.build(name)
    edges = np.cumsum([0] + s.frames)
    dec = gpu.lacx.Decoder()
    for b in (1, 2, len(s.frames) // 2, len(s.frames) - 1):
        seam = int(edges[b])
        for start, n in ((seam - 1, 2), (seam - 37, 80), (max(0, seam - 300), 700), (seam, 1)):
            n = min(n, len(s.left) - start)
            left, right = dec.decode_window(s.lac, start, n)
            assert np.array_equal(left, np.array(s.left[start:start + n], dtype=np.int64)), (name, b, start, n)
            if s.right is not None:
                assert np.array_equal(right, np.array(s.right[start:start + n], dtype=np.int64)), (name, b, start, n)
    dec.close()
