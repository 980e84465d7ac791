"""lacx_transcode_batch on the MI355X: .lac in, .lac out -- cut, join, re-encode, re-channel and narrow as one device job.
The expectation everywhere is the oracle as a pipeline (editcases.py): oracleshim.decode of every source, sliced,
concatenated and transformed in numpy, oracleshim.encode of the result, zlib.crc32 of its WAV data bytes."""
import os
import subprocess
import zlib

import numpy as np
import pytest

import __graft_entry__ as ge
import editcases as E
import lacmutate
import wavutil

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    pkg = ge.load_pkg()
    if pkg.lacx.device_count() <= 0:
        pytest.fail("no HIP device: the transcode job has no CPU fallback")
    return pkg


@pytest.fixture(scope="module")
def src():
    return E.sources()


def _encoder(gpu, zero_run=True, partitioning=True):
    enc = gpu.lacx.Encoder(12, 2, 48000, 16, device=0)
    enc.set_zero_run_enabled(zero_run)
    enc.set_partitioning_enabled(partitioning)
    return enc


def _api(src, case):
    """An editcases output (segments by source name, depth, op, mode) as transcode_batch takes it."""
    segments, depth, op, mode = case
    return ([(src[name].lac if isinstance(name, str) else name.lac, start, frames) for name, start, frames in segments], depth, op, mode)


def _check(src, case, got, zero_run=True, partitioning=True, verified=0):
    segments, depth, op, mode = case
    want = E.expected(segments, depth, op, mode, zero_run, partitioning)
    data, r = got
    assert data == want.lac, (case[1:], [(n if isinstance(n, str) else "?", a, b) for n, a, b in segments])
    assert (r.frames, r.blocks, r.lac_bytes, r.data_crc32) == (want.frames, want.blocks, len(want.lac), want.crc), case[1:]
    assert (r.channels, r.bit_depth, r.sample_rate, r.verified) == (want.channels, want.depth, want.rate, verified)
    distinct = {}
    for name, _, _ in segments:
        lac = src[name].lac if isinstance(name, str) else name.lac
        distinct[id(lac)] = len(lac)
    assert r.source_lac_bytes == sum(distinct.values())


def _run(gpu, src, cases, zero_run=True, partitioning=True, verify=False):
    dec = gpu.lacx.Decoder(device=0)
    try:
        got = dec.transcode_batch(_encoder(gpu, zero_run, partitioning), [_api(src, c) for c in cases], verify=verify)
    finally:
        dec.close()
    assert len(got) == len(cases)
    for c, g in zip(cases, got):
        _check(src, c, g, zero_run, partitioning, int(verify))
    return got


STEREO16 = ("st16_lr", "st16_ms", "st16_auto", "st16_other", "dual_mono", "st16_v2")
ALL = STEREO16 + ("mono24", "st24_narrowable", "dual_mono24_narrowable", "st24_right_odd")


@pytest.mark.parametrize("zero_run,partitioning", [(True, True), (False, True), (True, False), (False, False)])
def test_identity(gpu, src, zero_run, partitioning):
    assert sorted(set(src["st16_auto_ms"])) == [0, 1]  # the mode-2 source holds mid/side and LR blocks
    cases = [([(name, 0, None)], 0, E.KEEP, mode) for name in ALL for mode in ((0, 1, 2) if src[name].right is not None else (0,))]
    got = _run(gpu, src, cases, zero_run, partitioning)
    by = {(c[0][0][0], c[3]): g[0] for c, g in zip(cases, got)}
    assert by[("st16_v2", 2)] == by[("st16_auto", 2)] and by[("st16_v2", 2)][2] == 3  # the version-2 source comes out as version 3
    if zero_run and partitioning:  # a stream coded as the oracle codes it comes back byte for byte
        assert by[("st16_auto", 2)] == src["st16_auto"].lac and by[("st16_lr", 0)] == src["st16_lr"].lac


CUTS = [(0, 1), (39999, 1), (16383, 2), (16384, 16384), (1, 39999), (30000, None), (33000, 100), (32768 + 7231, 1)] + \
       [(16380 + s, n) for s in (1, 2, 3) for n in (5, 6, 7)]


def test_cut(gpu, src):
    assert {(s % 4, n % 4) for s, n in CUTS if n in (5, 6, 7)} == {(a, b) for a in (1, 2, 3) for b in (1, 2, 3)}
    cases = [([(name, s, n)], 0, E.KEEP, 2) for name in ("st16_auto", "st16_v2") for s, n in CUTS]
    cases += [([("st16_ms", 16383, 2)], 0, E.KEEP, 1), ([("mono24", 4095, 4098)], 0, E.KEEP, 0)]
    _run(gpu, src, cases)


def test_cut_and_join_conveniences(gpu, src):
    dec, enc = gpu.lacx.Decoder(device=0), _encoder(gpu)
    a = src["st16_auto"]
    assert dec.cut(enc, a.lac, 16383, 2) == E.expected([("st16_auto", 16383, 2)]).lac
    assert dec.cut(enc, a.lac, 39000) == E.expected([("st16_auto", 39000, None)]).lac
    assert dec.join(enc, [a.lac, src["st16_other"].lac]) == E.expected([("st16_auto", 0, None), ("st16_other", 0, None)]).lac
    assert dec.recompress(enc, src["st16_lr"].lac, stereo_mode=1) == E.expected([("st16_lr", 0, None)], stereo_mode=1).lac
    assert dec.recompress(enc, src["dual_mono"].lac, channels="fold") == E.expected([("dual_mono", 0, None)], op=E.FOLD).lac
    dec.close()


def test_join(gpu, src):
    a = "st16_auto"
    cases = [
        ([(a, 10, 1), (a, 11, 2), (a, 13, 3), (a, 16, 5)], 0, E.KEEP, 2),           # one quad of the output spans four segments
        ([(a, 16383, 1), ("st16_other", 7, 2), (a, 20000, 3), ("st16_lr", 39995, 5)], 0, E.KEEP, 2),
        ([(a, 0, 100), (a, 20000, 100)], 0, E.KEEP, 2),                               # one stream twice
        ([(a, 100, 300), (a, 200, 300)], 0, E.KEEP, 2),                               # ... and overlapping
        ([(a, 0, None), ("st16_other", 0, None)], 0, E.KEEP, 2),                      # two streams of one format
        ([("st16_lr", 0, None), ("st16_ms", 0, None), ("st16_v2", 0, None)], 0, E.KEEP, 0),
        ([(a, 0, 16383), ("st16_other", 0, 1), (a, 5, 1)], 0, E.KEEP, 2),             # 16385 frames, seams at 16383 and 16384
        ([(a, 3, 16383), ("st16_other", 1, 2)], 0, E.KEEP, 2),                        # 16385 frames, seam at 16383
        ([(a, 3, 16384), ("st16_other", 1, 1)], 0, E.KEEP, 2),                        # 16385 frames, seam at 16384
        ([(a, 3, 16385), ("st16_other", 1, 1)], 0, E.KEEP, 2),                        # seam at 16385
        ([(a, 100, 1000), (a, 17000, 1000)], 0, E.KEEP, 2),                           # out of a mid/side and an LR block
        ([(a, 16000, 384), (a, 16384, 500)], 0, E.KEEP, 1),
        ([("mono24", 19999, 1), ("mono24", 0, 1)], 0, E.KEEP, 0),
    ]
    assert src["st16_auto_ms"][:2] == [1, 0]
    _run(gpu, src, cases)


TRANSFORMS = [
    ([("st16_auto", 0, None)], 0, E.KEEP, 2), ([("st16_auto", 0, None)], 0, E.LEFT, 2), ([("st16_auto", 0, None)], 0, E.RIGHT, 2),
    ([("st16_auto", 5, 1027)], 0, E.SWAP, 2), ([("dual_mono", 0, None)], 0, E.FOLD, 2), ([("mono24", 0, None)], 0, E.DUAL, 2),
    ([("mono24", 3, 4097)], 0, E.DUAL, 1),
    ([("st24_narrowable", 0, None)], 16, E.KEEP, 2), ([("st16_auto", 0, None)], 24, E.KEEP, 2), ([("st16_other", 1, 1025)], 24, E.SWAP, 0),
    ([("dual_mono24_narrowable", 0, None)], 16, E.FOLD, 2), ([("st24_narrowable", 2, 3)], 16, E.RIGHT, 2),
    ([("st16_auto", 0, None)], 16, E.KEEP, 2), ([("mono24", 0, None)], 24, E.KEEP, 0),
]


def test_transforms(gpu, src):
    _run(gpu, src, TRANSFORMS)


def test_transform_refusals_leave_the_others_alone(gpu, src):
    refused = [
        ([("st16_auto", 0, None)], 0, E.FOLD, 2),
        ([("st16_auto", 16383, 6)], 0, E.FOLD, 2),
        ([("mono24", 0, None)], 16, E.KEEP, 0),
        ([("mono24", 1021, 2000)], 16, E.DUAL, 2),
        ([("st24_narrowable", 0, 100), ("dual_mono24_narrowable", 0, 50), ("st24_narrowable", 0, 100)], 16, E.FOLD, 2),
        ([("st24_right_odd", 0, None)], 16, E.KEEP, 2),                              # right alone: frame 5
        ([("st24_narrowable", 0, 1030), ("st24_right_odd", 3, 100)], 16, E.KEEP, 1),  # ... in a second unit: frame 1032
        ([("st24_right_odd", 0, None)], 16, E.SWAP, 2),                              # the source's right is the output's left
    ]
    good = TRANSFORMS[:4] + [([("st24_right_odd", 0, None)], 16, E.LEFT, 2), ([("st24_right_odd", 0, 5)], 16, E.KEEP, 2)]
    cases = [good[0], refused[0], good[1], refused[1], refused[2], good[2], refused[3], refused[4], good[3], refused[5], good[4], refused[6],
             refused[7], good[5]]
    assert E.edited(*refused[5][:3])[4].startswith("[transcode-error] frame 5 right sample ")
    assert E.edited(*refused[6][:3])[4].startswith("[transcode-error] frame 1032 right sample ")
    assert E.edited(*refused[7][:3])[4].startswith("[transcode-error] frame 5 left sample ")
    want = {}
    for i, c in enumerate(cases):
        if c in refused:
            want[i] = E.edited(c[0], c[1], c[2])[4]
            assert want[i] and want[i].startswith("[transcode-error] frame ")
    dec = gpu.lacx.Decoder(device=0)
    with pytest.raises(gpu.lacx.BatchDecodeError) as ei:
        dec.transcode_batch(_encoder(gpu), [_api(src, c) for c in cases])
    dec.close()
    assert ei.value.errors == want
    assert str(ei.value) == "output 1: " + want[1]
    for i, c in enumerate(cases):
        if i in want:
            assert ei.value.results[i] is None
        else:
            _check(src, c, ei.value.results[i])


def test_host_refusals_in_a_device_call(gpu, src):
    a = src["st16_auto"].lac
    outputs = [([(a, 0, 10)], 0, "keep", 2), ([(a, 40000, 1)], 0, "keep", 2), ([(a, 0, 10), (src["mono24"].lac, 0, 10)], 0, "keep", 2),
               ([(src["mono24"].lac, 0, 10)], 0, "fold", 2), ([(a, 0, 10)], 0, "dual", 2), ([(a, 0, 10)], 20, "keep", 2), ([(a, 0, 0)], 0, "keep", 2)]
    dec = gpu.lacx.Decoder(device=0)
    with pytest.raises(gpu.lacx.BatchDecodeError) as ei:
        dec.transcode_batch(_encoder(gpu), outputs)
    dec.close()
    assert ei.value.errors == {1: "segment 0: window outside the stream", 2: "segment 1: channels differs from segment 0: 2, 1",
                               3: "channel operation needs a stereo source", 4: "channel operation needs a mono source",
                               5: "unsupported bit depth: 20", 6: "segment 0: empty window"}
    assert ei.value.results[0][0] == E.expected([("st16_auto", 0, 10)]).lac


def test_damage_fails_exactly_the_outputs_that_touch_the_block(gpu, src):
    good = src["st16_auto"]
    version, ent, head = lacmutate.table(good.lac)
    assert version == 3 and len(ent) == 3
    bad = bytearray(good.lac)
    bad[head + ent[0][1]] ^= 0xFF  # block 1's header: its mid/side flag byte
    damaged = E.Source(bytes(bad), good.left, good.right, good.rate, good.depth)
    dec = gpu.lacx.Decoder(device=0)
    with pytest.raises(RuntimeError) as strict:
        dec.decode(damaged.lac)
    assert str(strict.value).startswith("[decode-error] block=1 ")
    cases = [
        ([(damaged, 0, 16384), (damaged, 32768, None)], 0, E.KEEP, 2),    # blocks 0 and 2 only
        ([(damaged, 0, 16385)], 0, E.KEEP, 2),                             # one frame of block 1
        ([(damaged, 100, 50), (damaged, 32767, 1), (damaged, 5, 5)], 0, E.KEEP, 2),
        ([(damaged, 33000, 10)], 0, E.LEFT, 2),
        ([(damaged, 0, None)], 0, E.KEEP, 2),
        ([("st16_other", 0, 10), (damaged, 16383, 1)], 0, E.KEEP, 2),
    ]
    with pytest.raises(gpu.lacx.BatchDecodeError) as ei:
        dec.transcode_batch(_encoder(gpu), [_api(src, c) for c in cases])
    dec.close()
    assert ei.value.errors == {1: "segment 0: " + str(strict.value), 2: "segment 1: " + str(strict.value), 4: "segment 0: " + str(strict.value)}
    for i in (0, 3, 5):
        _check(src, cases[i], ei.value.results[i])


def test_samples_outside_the_source_depth_are_refused_not_cut_off(gpu, src):
    """A well-formed stream whose samples leave its depth (a 24-bit stream relabelled 16-bit) fails in the window job, as
    in a strict decode: k_edit never sees a sample its store would truncate."""
    loud = bytearray(src["st24_narrowable"].lac)
    loud[8] = 16
    loud = E.Source(bytes(loud), None, None, 48000, 16)
    cases = [([(loud, 0, None)], 0, E.KEEP, 2), ([("st16_other", 0, 10)], 0, E.KEEP, 2), ([(loud, 100, 8)], 24, E.LEFT, 2)]
    dec = gpu.lacx.Decoder(device=0)
    with pytest.raises(RuntimeError) as strict:
        dec.decode(loud.lac)
    assert str(strict.value) == "[decode-error] block=0 sample outside the bit depth"
    for verify in (False, True):
        with pytest.raises(gpu.lacx.BatchDecodeError) as ei:
            dec.transcode_batch(_encoder(gpu), [_api(src, c) for c in cases], verify=verify)
        assert ei.value.errors == {0: "segment 0: " + str(strict.value), 2: "segment 0: " + str(strict.value)}
        _check(src, cases[1], ei.value.results[1], verified=int(verify))
    dec.close()


MIXED = [([("st16_auto", 1, 39999)], 0, E.KEEP, 2), ([("mono24", 0, None)], 0, E.KEEP, 0), ([("st16_v2", 16383, 2)], 0, E.KEEP, 2),
         ([("mono24", 7, 1030)], 0, E.DUAL, 2), ([("st16_v2", 0, None)], 24, E.SWAP, 1), ([("st24_narrowable", 0, None)], 16, E.KEEP, 2)]


def test_mixed_batch(gpu, src):
    _run(gpu, src, MIXED)


def test_verify_gives_the_same_bytes_and_marks_them(gpu, src):
    plain = _run(gpu, src, MIXED + TRANSFORMS[:6])
    checked = _run(gpu, src, MIXED + TRANSFORMS[:6], verify=True)
    assert [g[0] for g in plain] == [g[0] for g in checked] and all(g[1].verified == 1 for g in checked)


def test_one_decoder_and_encoder_serve_many_calls(gpu, src):
    dec, enc = gpu.lacx.Decoder(device=0), _encoder(gpu)
    for cases in (MIXED[:2], TRANSFORMS[4:6], MIXED[:1]):
        for c, g in zip(cases, dec.transcode_batch(enc, [_api(src, c) for c in cases])):
            _check(src, c, g)
    left, right, info, _ = dec.decode(src["st16_auto"].lac)  # the decoder's other forms still work behind a transcode
    assert np.array_equal(left, src["st16_auto"].left) and np.array_equal(right, src["st16_auto"].right)
    dec.close()


def _cli(*args, timeout=120):
    exe = os.path.join(ge.PKG_DIR, "lacx_cli")
    subprocess.check_call(["make", "-C", ge.PKG_DIR, "lacx_cli"], stdout=subprocess.DEVNULL)  # (nothing to do where it is up to date)
    return subprocess.run([exe, *args], capture_output=True, text=True, timeout=timeout)


def test_cli(gpu, src, tmp_path):
    paths = {}
    for name in ("st16_auto", "st16_other", "dual_mono", "st24_narrowable"):
        paths[name] = str(tmp_path / (name + ".lac"))
        with open(paths[name], "wb") as f:
            f.write(src[name].lac)
    out = str(tmp_path / "out.lac")
    done = _cli("recompress", paths["st24_narrowable"], out, "--stereo=ms", "--no-zero-run", "--depth=16", "--channels=swap", "--verify")
    assert done.returncode == 0, done.stderr
    assert open(out, "rb").read() == E.expected([("st24_narrowable", 0, None)], 16, E.SWAP, 1, zero_run=False).lac
    assert ", verified" in done.stdout
    done = _cli("cut", paths["st16_auto"], out, "--start=16383", "--frames=2")
    assert done.returncode == 0, done.stderr
    assert open(out, "rb").read() == E.expected([("st16_auto", 16383, 2)]).lac
    done = _cli("join", out, paths["st16_auto"], paths["st16_other"], "--verify")
    assert done.returncode == 0, done.stderr
    assert open(out, "rb").read() == E.expected([("st16_auto", 0, None), ("st16_other", 0, None)]).lac
    refused = str(tmp_path / "refused.lac")
    done = _cli("recompress", paths["st16_auto"], refused, "--channels=fold")
    assert done.returncode == 2 and "[transcode-error] frame " in done.stderr
    assert not os.path.exists(refused) and not os.path.exists(refused + ".lacx-partial")
