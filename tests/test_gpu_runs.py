"""The run finder on the MI355X: lacx_decoder_runs_batch_device, lacx_decoder_runs_pcm_batch_device, lacx_decoder_item_runs,
Decoder.split_on_silence / trim_silence and `lacx_cli find` / `split`, against a boolean numpy mask per detector and the
run lengths from its differences over the PCM the streams and sources were made from (tests/runstwin.py) -- never the code
under test.  Equality is exact for every run, every total and every result field.  A damaged or cut stream goes to the device
only after the sanitized CPU twin of the job (tests/native/sim_runs.cpp, every buffer at exactly the plan's capacity) has
passed it in this run."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import __graft_entry__ as ge
import lacmutate
import runstwin as rw
import salvagetwin as st

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_DIR = os.path.join(ROOT, "lossless-audio-codec_amd")
SENTINEL = 0xA5
P32, I16, I24, P16, PF32, IF32 = 0, 1, 2, 16, 17, 18
LAYOUTS = {16: (P32, I16, P16, PF32, IF32), 24: (P32, I24, PF32, IF32)}
OFFSETS = {P32: (0, 4, 8), I16: (0, 4, 8), I24: (0, 1, 2, 3, 5), P16: (0, 2, 6), PF32: (0, 4, 12), IF32: (0, 4, 8)}


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


@pytest.fixture(scope="module")
def streams(oracle):
    """The twin tests' streams: (name, stream, Item, block frames, [Det]) -- a reference computed once and left unchanged."""
    rw.assert_content()
    return rw.build_streams(oracle)


def _records(lx, dets):
    return [lx.RunDetector(d.kind, d.channel, (C.c_uint8 * 2)(), d.level, d.min_frames) for d in dets]


def _check(what, got, it, blocks, dets, lost=None, flags=0):
    """One item of a runs call against numpy: the result record, every list and its totals."""
    res, lists = got
    want, runs = rw.expected_result(dets, it.left, it.right, it.depth, it.rate, blocks, lost, flags)
    assert [l.runs.tolist() for l in lists] == [[list(r) for r in x] for x in runs], what
    assert rw.result_of(res) == want, what
    for l, t in zip(lists, want.totals):
        assert (l.totals.runs, l.totals.frames, l.totals.longest, l.totals.longest_start) == tuple(t) and l.runs.dtype == np.uint64, what
    return want


@pytest.mark.parametrize("reverse", [False, True])
def test_batch_forward_and_reversed(gpu, streams, reverse):
    """Everything the twin tests run on as one batch -- 16- and 24-bit, mono and stereo, versions 3 and 2, eight detectors
    on the border items -- forward and reversed: items begin and end with runs beside other items' runs and do not join."""
    lx = gpu.lacx
    dec = lx.Decoder(device=0)
    order = streams[::-1] if reverse else streams
    got = dec.runs_batch([x[1] for x in order], [_records(lx, x[4]) for x in order])
    assert dec.last_ms > 0
    for (name, _, it, blocks, dets), g in zip(order, got):
        want = _check(name, g, it, blocks, dets)
        assert want.lost_blocks == 0 and not g[0].rerun
    again = dec.runs_batch([x[1] for x in order], [_records(lx, x[4]) for x in order])
    assert [[l.runs.tolist() for l in g[1]] for g in again] == [[l.runs.tolist() for l in g[1]] for g in got]  # the same from run to run
    one = dec.runs(order[0][1], _records(lx, order[0][4]))
    assert [l.runs.tolist() for l in one] == [l.runs.tolist() for l in got[0][1]]
    dec.close()


def test_lost_and_missing_blocks(gpu, oracle):
    """A lost block inside a run, at the start and at the end, and the blocks a version-2 walk does not reach: the run is
    split, the first frame behind the loss is never FLAT -- after the sanitized twin has passed the same job."""
    lx = gpu.lacx
    cases = rw.damaged(oracle)
    lacs = rw.cleared("gpu-lost", [x[1] for x in cases], [x[2] for x in cases])  # CPU first
    dec = lx.Decoder(device=0)
    got = dec.runs_batch(lacs, [_records(lx, x[2]) for x in cases])
    by = {}
    for (name, lac, dets), g in zip(cases, got):
        exp = st.expected(oracle, lac)
        blocks = [n for n, _ in lacmutate.table(lac)[1]]
        it = rw.Item(name, lac[3], lac[8], st.rate(lac), exp.left, exp.right)
        by[name] = (_check(name, g, it, blocks, dets, exp.lost), g[1])
    assert by["lost1|2ch16"][0].lost_blocks == 1 and by["lost1-v2|2ch16"][0].lost_blocks == 2 and by["cut|1ch24"][0].lost_frames == 259
    assert by["lost1|2ch16"][1][0].runs.tolist() == [[240, 17], [515, 25]] and by["lost1|2ch16"][1][1].runs.tolist() == [[241, 16], [516, 24]]
    dec.close()


def test_forced_rerun(gpu, streams, monkeypatch):
    """LACX_RUNS_LIST_CAP = 16, read when the decoder is created: the alternation's 1025 runs outgrow the lists, the kernel
    runs once more with the counters' capacities, LACX_RUNS_RERUN is set and every list is complete."""
    lx = gpu.lacx
    monkeypatch.setenv("LACX_RUNS_LIST_CAP", "16")
    small = lx.Decoder(device=0)
    monkeypatch.delenv("LACX_RUNS_LIST_CAP")
    plain = lx.Decoder(device=0)
    part = [x for x in streams if x[0].startswith(("alternating", "borders|2ch16", "n3|"))]
    for dec, flags in ((small, rw.RERUN), (plain, 0), (small, rw.RERUN)):
        got = dec.runs_batch([x[1] for x in part], [_records(lx, x[4]) for x in part])
        for (name, _, it, blocks, dets), g in zip(part, got):
            _check(name, g, it, blocks, dets, flags=flags)
            assert g[0].rerun == bool(flags)
    alt = next(g for x, g in zip(part, got) if x[0].startswith("alternating"))
    assert alt[0].det[0].runs == (rw.ALT_FRAMES + 1) // 2 > 16
    small.close(), plain.close()


class Placed:
    """Bytes in device memory at `offset` bytes behind the start of a torch buffer, sentinels on both sides; or (whole) at
    the very end of a buffer that is an allocation of its own."""

    def __init__(self, torch, raw: bytes, offset=0, tail=64, whole=None):
        n = len(raw)
        if whole is None:
            self.buf = torch.full((offset + n + tail,), SENTINEL, dtype=torch.uint8, device="cuda")
        else:
            self.buf, offset = whole, whole.numel() - n
            self.buf.fill_(SENTINEL)
        self.offset, self.n, self.raw = offset, n, raw
        self.buf[offset:offset + n] = torch.frombuffer(bytearray(raw), dtype=torch.uint8).cuda()
        self.ptr = self.buf.data_ptr() + offset

    def untouched(self):
        host = self.buf.cpu().numpy()
        return bool((host[:self.offset] == SENTINEL).all()) and bool((host[self.offset + self.n:] == SENTINEL).all()) and \
            host[self.offset:self.offset + self.n].tobytes() == self.raw


def _arrays(left, right, bits, layout):
    """The source's arrays as bytes: one for an interleaved layout, one per channel for a planar one."""
    chans = [left] if right is None else [left, right]
    if layout in (PF32, IF32):
        chans = [(x.astype(np.float32) / np.float32(1 << (bits - 1))) for x in chans]
    elif layout in (I16, P16):
        chans = [x.astype("<i2") for x in chans]
    if layout == I24:
        a = chans[0] if right is None else np.stack(chans, 1).ravel()
        return [np.ascontiguousarray(a.astype("<i4").view(np.uint8).reshape(-1, 4)[:, :3]).tobytes()]
    if layout in (I16, IF32):
        return [np.stack(chans, axis=1).tobytes()]
    return [x.astype(x.dtype.newbyteorder("<")).tobytes() for x in chans]


def _source(torch, left, right, bits, layout, offset=0, whole=None):
    placed = [Placed(torch, raw, offset, whole=whole if k == 0 else None) for k, raw in enumerate(_arrays(left, right, bits, layout))]
    return (placed[0].ptr, placed[1].ptr if len(placed) == 2 else None, layout, 1 if right is None else 2, left.size), placed


def test_source_form_layouts_offsets_and_bounds(gpu, torch):
    """The spliced signal (774 frames: a partial last unit, quiet to the last frame) and the 1025-frame shape (two tiles, the
    second of one frame) in every layout at offsets between sentinels and at the very end of an allocation: numpy's runs;
    the sentinels stay."""
    lx = gpu.lacx
    dec = lx.Decoder(device=0)
    whole = torch.empty(10 << 20, dtype=torch.uint8, device="cuda")  # large enough to be an allocation of its own
    for ch, bits, rate in rw.FORMATS:
        parts = rw.spliced_parts(ch, bits)
        sp = rw.Item("splice", ch, bits, rate, np.concatenate([l for l, _ in parts]), np.concatenate([r for _, r in parts]) if ch == 2 else None)
        shape = next(it for it in rw.shape_items() if it.name == "n1025|%dch%d" % (ch, bits))
        for it, dets in ((sp, rw.spliced_detectors()), (shape, rw.shape_detectors())):
            items, keep = [], []
            for layout in LAYOUTS[bits]:
                for offset in OFFSETS[layout]:
                    src, placed = _source(torch, it.left, it.right, bits, layout, offset)
                    items.append((src, rate, bits)), keep.append(placed)
            got = dec.runs_pcm_batch(items, _records(lx, dets))
            assert dec.last_ms > 0
            for k, g in enumerate(got):
                _check((it.name, ch, bits, k), g, it, rw.grid_blocks(it.left.size), dets)
            assert all(p.untouched() for ps in keep for p in ps)
        for layout in LAYOUTS[bits]:
            src, placed = _source(torch, sp.left, sp.right, bits, layout, whole=whole)
            assert placed[0].offset + placed[0].n == whole.numel()
            (g,) = dec.runs_pcm_batch([(src, rate, bits)], _records(lx, rw.spliced_detectors()))
            _check((ch, bits, layout), g, sp, rw.grid_blocks(774), rw.spliced_detectors())
            assert all(p.untouched() for p in placed)
    dec.close()


def test_an_invalid_source_sample_fails_its_item(gpu, torch):
    """A planar int32 outside the depth and an inexact float: the digest form's message, no result, the others unharmed."""
    lx = gpu.lacx
    dec = lx.Decoder(device=0)
    left, right = rw.loud(2001, 2, 24, 12)
    rw.plant_quiet(left, right, 1000, 50)
    good = torch.from_numpy(np.stack([left, right])).cuda()
    wide = good.clone()
    wide[1, 1024] = 1 << 24
    inexact = (good.to(torch.float32) / float(1 << 23)).contiguous()
    inexact[0, 7] = 0.3
    dets = [rw.Det(rw.QUIET, rw.ALL, 3, 1), rw.Det(rw.FLAT, rw.ALL, 0, 1)]
    with pytest.raises(lx.BatchDecodeError) as e:
        dec.runs_pcm_batch([(good, 48000, 24), (wide, 48000, 24), (inexact, 48000, 24)], _records(lx, dets))
    assert e.value.errors == {1: "right sample at index 1024 is outside the configured PCM bit depth",
                              2: "left sample at index 7 is not an exact 24-bit PCM value"}
    assert e.value.results[1] is None and e.value.results[2] is None
    _check("good", e.value.results[0], rw.Item("", 2, 24, 48000, left, right), rw.grid_blocks(2001), dets)
    dec.close()


@pytest.mark.parametrize("channels,bits,rate", rw.FORMATS)
def test_source_and_stream_agree_and_stats_cross_checks(gpu, torch, channels, bits, rate):
    """runs_pcm_batch of a tensor equals runs_batch of the encoder's own .lac of it, run for run, and both equal numpy.  The
    free cross-checks against stats on the same item: the frames in PEAK(2^(b-1)-1, min 1) runs of a channel are its
    full_scale; with QUIET(0, all, min 1) a run at 0 has lead_zero_frames and a run to the end trail_zero_frames."""
    lx = gpu.lacx
    it = rw.border_item(channels, bits, rate, seed=5)
    left, right = it.left.copy(), None if it.right is None else it.right.copy()
    for x in (left, right):
        if x is not None:
            x[:37] = 0
            x[-1001:] = 0
    it = rw.Item(it.name, channels, bits, rate, left, right)
    fs = rw.full_scale(bits)
    dets = rw.border_detectors(bits)[:5] + [rw.Det(rw.PEAK, 0, fs, 1), rw.Det(rw.PEAK, 1, fs, 1), rw.Det(rw.QUIET, rw.ALL, 0, 1)]
    t = torch.from_numpy(np.stack([left] if right is None else [left, right])).cuda()
    lac = lx.Encoder(12, 2 if channels == 2 else 0, rate, bits, device=0).encode_tensor(t)
    dec = lx.Decoder(device=0)
    (src,) = dec.runs_pcm_batch([(t, rate, bits)], _records(lx, dets))
    (dcd,) = dec.runs_batch([lac], _records(lx, dets))
    assert bytes(src[0]) == bytes(dcd[0]) and [l.runs.tolist() for l in src[1]] == [l.runs.tolist() for l in dcd[1]]
    _check("source", src, it, rw.grid_blocks(left.size), dets)
    (stats, _rows), = dec.stats_batch([lac])
    assert dcd[0].det[5].frames == stats.ch[0].full_scale > 0
    if channels == 2:
        assert dcd[0].det[6].frames == stats.ch[1].full_scale > 0
    zero = dcd[1][7].runs.tolist()
    assert zero[0] == [0, stats.lead_zero_frames] == [0, 37] and zero[-1] == [left.size - stats.trail_zero_frames, stats.trail_zero_frames]
    assert stats.trail_zero_frames == 1001
    dec.close()


def test_alternation_with_the_other_job_forms(gpu, streams):
    """One decoder, runs between stats, block digests, a decode and a salvage: every answer is what it is alone."""
    lx = gpu.lacx
    part = [x for x in streams if x[0].startswith(("borders|2ch24", "splice|1ch16", "n16385|2ch16"))]
    lacs, dets = [x[1] for x in part], [_records(lx, x[4]) for x in part]
    dec, alone = lx.Decoder(device=0), lx.Decoder(device=0)
    want_stats = [bytes(s) for s, _ in alone.stats_batch(lacs)]
    want_rows = [[bytes(r) for r in rows] for _, rows in alone.digest_blocks_batch(lacs)]
    for _ in range(2):
        got = dec.runs_batch(lacs, dets)
        for (name, _, it, blocks, d), g in zip(part, got):
            _check(name, g, it, blocks, d)
        assert [bytes(s) for s, _ in dec.stats_batch(lacs)] == want_stats
        got = dec.runs_batch(lacs[::-1], dets[::-1])
        for (name, _, it, blocks, d), g in zip(part[::-1], got):
            _check(name, g, it, blocks, d)
        assert [[bytes(r) for r in rows] for _, rows in dec.digest_blocks_batch(lacs)] == want_rows
        wav = dec.decode_wav(lacs[0])
        first = part[0][2]
        assert wav[:4] == b"RIFF" and len(wav) == 44 + first.left.size * first.channels * first.depth // 8
    dec.close(), alone.close()


def _silence_item(channels, bits, rate):
    """Sound, a pause of 500 frames over a tile border, sound, a short pause of 30, sound, silence to the end."""
    left, right = rw.loud(6000, channels, bits, 31)
    for s, n in ((0, 100), (1000, 500), (3000, 30), (5200, 800)):
        rw.plant_quiet(left, right, s, n)
    return rw.Item("silences", channels, bits, rate, left, right)


def test_split_and_trim_on_silence(gpu, torch):
    """Every output of split_on_silence is byte for byte what `cut` gives for that range, and its CRC is digest_pcm's of the
    source tensor's range; the ranges are the Python restatement's; trim keeps the outermost; all silence gives nothing; a
    stream with a lost block is refused."""
    lx = gpu.lacx
    it = _silence_item(2, 16, 48000)
    enc = lx.Encoder(12, 2, 48000, 16, device=0)
    t = torch.from_numpy(np.stack([it.left, it.right])).cuda()
    lac = enc.encode_tensor(t)
    dec = lx.Decoder(device=0)
    quiet, _ = rw.expected(rw.Det(rw.QUIET, rw.ALL, rw.LEVEL, 100), it.left, it.right)
    assert quiet == [(0, 100), (1000, 500), (5200, 800)]
    for pad in (0, 40, 250):
        want = rw.pieces_of(6000, quiet, pad)
        got = dec.split_on_silence(enc, lac, rw.LEVEL, 100, pad=pad, verify=True)
        assert [(s, n) for s, n, _ in got] == want and len(want) == (2 if pad < 250 else 1), pad
        for s, n, data in got:
            assert data == dec.cut(enc, lac, s, n), (pad, s)
            (dg,) = dec.digest_pcm_batch([(t[:, s:s + n].contiguous(), 48000, 16)])
            (own,) = dec.digest_batch([data])
            assert own.data_crc32 == dg.data_crc32 and own.frames == n, (pad, s)
        s, n, data = dec.trim_silence(enc, lac, rw.LEVEL, 100, pad=pad)
        assert (s, n) == (want[0][0], want[-1][0] + want[-1][1] - want[0][0]) and data == dec.cut(enc, lac, s, n)
    silent = enc.encode(np.zeros(3000, np.int32), np.zeros(3000, np.int32))
    assert dec.split_on_silence(enc, silent, 0, 10) == [] and dec.trim_silence(enc, silent, 0, 10) is None
    with pytest.raises(ValueError, match="lost blocks"):
        dec.split_on_silence(enc, rw.cleared("gpu-split", [lac[:-5]], [[rw.Det(rw.QUIET, rw.ALL, rw.LEVEL, 100)]])[0], rw.LEVEL, 100)
    dec.close()


def _cli():
    subprocess.check_call(["make", "-C", PKG_DIR, "lacx_cli"], stdout=subprocess.DEVNULL)
    return os.path.join(PKG_DIR, "lacx_cli")


def _ms(n, rate):
    ms = n * 1000 // rate
    return "%d.%03d" % (ms // 1000, ms % 1000)


def test_cli_find_and_split(gpu, tmp_path):
    """`lacx_cli find` on a .lac and on the WAV decoded from it (the same lines), its exit codes, and `lacx_cli split`, whose
    files are what split_on_silence gives."""
    lx = gpu.lacx
    cli = _cli()
    it = _silence_item(2, 16, 48000)
    enc = lx.Encoder(12, 2, 48000, 16, device=0)
    lac = enc.encode(it.left, it.right)
    dec = lx.Decoder(device=0)
    wav = dec.decode_wav(lac)
    paths = {name: str(tmp_path / name) for name in ("a.lac", "a.wav", "junk.lac")}
    for name, blob in {"a.lac": lac, "a.wav": wav, "junk.lac": b"XX" + lac[2:]}.items():
        with open(paths[name], "wb") as f:
            f.write(blob)
    plant = it.left.copy()
    quiet, qt = rw.expected(rw.Det(rw.QUIET, rw.ALL, rw.LEVEL, 100), it.left, it.right)
    flat, ft = rw.expected(rw.Det(rw.FLAT, rw.ALL, 0, 100), plant, it.right)
    res = subprocess.run([cli, "find", paths["a.lac"], paths["a.wav"], "--quiet=3", "--flat", "--min=100"], capture_output=True, text=True, timeout=120)
    assert res.returncode == 1 and res.stderr == ""
    lines = res.stdout.splitlines()
    want = ["quiet start=%d frames=%d at=%ss length=%ss" % (s, n, _ms(s, 48000), _ms(n, 48000)) for s, n in quiet]
    want += ["quiet total level=3 min=100 runs=%d frames=%d longest=%d longest_start=%d of=6000 lost_blocks=0" % tuple(qt),
             "flat total level=0 min=100 runs=0 frames=0 longest=0 longest_start=0 of=6000 lost_blocks=0"]
    assert flat == [] and lines == [w + " " + paths[k] for k in ("a.lac", "a.wav") for w in want]
    res = subprocess.run([cli, "find", paths["a.lac"], "--quiet-db=-80", "--min-seconds=0.01", "--channel=left"], capture_output=True, text=True, timeout=120)
    q80, t80 = rw.expected(rw.Det(rw.QUIET, 0, 3, 480), it.left, it.right)  # floor(32768 * 10^-4) = 3; 0.01 s at 48 kHz = 480 frames
    assert res.returncode == 1 and res.stdout.splitlines()[-1].startswith("quiet total level=3 min=480 runs=%d frames=%d " % (t80.runs, t80.frames))
    res = subprocess.run([cli, "find", paths["a.lac"], "--clip"], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and res.stdout == "peak total level=32767 min=1 runs=0 frames=0 longest=0 longest_start=0 of=6000 lost_blocks=0 %s\n" % paths["a.lac"]
    res = subprocess.run([cli, "find", paths["junk.lac"], paths["a.lac"], "--clip"], capture_output=True, text=True, timeout=120)
    assert res.returncode == 2 and res.stderr == "Find failed: %s: [decode-error] invalid frame header\n" % paths["junk.lac"]
    res = subprocess.run([cli, "find", paths["a.lac"]], capture_output=True, text=True, timeout=120)
    assert res.returncode == 2 and "lacx_cli find FILE..." in res.stderr
    prefix = str(tmp_path / "piece")
    res = subprocess.run([cli, "split", paths["a.lac"], prefix, "--quiet=3", "--min=100", "--pad=40", "--verify"], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and res.stderr == "", res.stderr
    got = dec.split_on_silence(enc, lac, 3, 100, pad=40)
    assert len(got) == 2 and len(res.stdout.splitlines()) == 2
    for k, (s, n, data) in enumerate(got):
        with open("%s%04d.lac" % (prefix, k + 1), "rb") as f:
            assert f.read() == data, k
        assert res.stdout.splitlines()[k].startswith("Piece %d start=%d frames=%d data_crc32=" % (k + 1, s, n))
    assert not os.path.exists(prefix + "0003.lac")
    res = subprocess.run([cli, "split", paths["junk.lac"], prefix, "--quiet=3", "--min=100"], capture_output=True, text=True, timeout=120)
    assert res.returncode == 2 and res.stderr.startswith("Refused: ")
    dec.close()
