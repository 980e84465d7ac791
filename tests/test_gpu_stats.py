"""Audio statistics on the MI355X: lacx_decoder_stats_batch_device, lacx_decoder_stats_pcm_batch_device, lacx_stats_combine
and `lacx_cli stats`, against numpy reductions and Python ints over the PCM the streams and sources were made from
(tests/statstwin.py) -- never the code under test.  Equality is exact for every integer field of every row and every
total.  A damaged or cut stream goes to the device only after the sanitized CPU twin of the job (tests/native/sim_stats.cpp,
every buffer at exactly the plan's capacity) has passed it in this run."""
import os
import subprocess

import numpy as np
import pytest

import __graft_entry__ as ge
import lacmutate
import lacstreams
import salvagetwin as st
import statstwin as sw

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
PKG_DIR = os.path.join(ROOT, "lossless-audio-codec_amd")
SENTINEL = 0xA5
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


def _check(what, got, it, blocks, lost=None, lx=None):
    """One item of a stats call against numpy: rows, totals, and the totals again through stats_combine."""
    stats, rows = got
    want = sw.expected_rows(it.left, it.right, it.depth, blocks, lost)
    total = sw.expected_totals(want, it.channels, it.depth, it.rate)
    assert sw.rows_of(rows) == want, what
    assert sw.totals_of(stats) == total, what
    if lx is not None:
        assert bytes(lx.stats_combine(rows, it.channels, it.depth, it.rate)) == bytes(stats), what
    assert stats.wasted_bits == sw.wasted_bits(total) and stats.dual_mono == (it.channels == 2 and total.differing == 0), what
    assert stats.peak == max(max(abs(c[0]), abs(c[1])) for c in total.ch) and stats.ch[0].sum == total.ch[0][5] and stats.ch[0].sum_sq == total.ch[0][6], what
    return total


@pytest.fixture(scope="module")
def small_items(gpu, oracle):
    """[(stream, Item, block frames)]: the content signals and every format at every border size through the product's own
    encoder, and per format the spliced stream of three blocks of 257, 258 and 259 frames."""
    content = sw.content_items()
    sw.assert_content(content)
    encoders = {(ch, depth, rate): gpu.lacx.Encoder(12, 2 if ch == 2 else 0, rate, depth, device=0) for ch, depth, rate in sw.FORMATS}
    items = [(encoders[(it.channels, it.depth, it.rate)].encode(it.left, it.right), it, sw.grid_blocks(it.left.size)) for it in content + sw.shape_items()]
    for ch, depth, rate in sw.FORMATS:
        parts = sw.spliced_parts(ch, depth)
        lacs = [oracle.encode(l, r, rate, depth, 0) for l, r in parts]
        it = sw.Item("splice|%dch%d" % (ch, depth), ch, depth, rate, np.concatenate([l for l, _ in parts]),
                     np.concatenate([r for _, r in parts]) if ch == 2 else None)
        items.append((lacstreams.splice(lacstreams.splice(lacs[0], lacs[1]), lacs[2]), it, [257, 258, 259]))
    return items


@pytest.mark.parametrize("reverse", [False, True])
def test_small_items_in_one_batch(gpu, small_items, reverse):
    """One batch of all items, forward and reversed, so that items and blocks start inside other items' workgroups and
    waves: rows and totals are numpy's, and stats_combine of the rows is the call's totals."""
    dec = gpu.lacx.Decoder(device=0)
    order = small_items[::-1] if reverse else small_items
    got = dec.stats_batch([lac for lac, _, _ in order])
    assert dec.last_ms > 0
    for (lac, it, blocks), g in zip(order, got):
        total = _check(it.name, g, it, blocks, lx=gpu.lacx)
        assert total.lost_blocks == 0 and g[0].frames == it.left.size and g[0].sample_rate == it.rate
    one = dec.stats(order[0][0])
    assert bytes(one) == bytes(got[0][0])
    dec.close()


def test_lost_and_missing_blocks(gpu, oracle):
    """A damaged block between two good ones, a truncated stream, a clean one and its version-2 form in one batch: lost
    rows are zeroed with their codes, the totals are over the decoded blocks, lost_blocks / lost_frames and the lead / trail
    rule hold."""
    lac = _fixture("decode_wav/st16_lr_3blk.lac")
    ent, pays = lacmutate._payloads(lac)
    pays[1] = pays[1][:1] + bytes([0x7F]) + pays[1][2:] if lac[4] == 2 else bytes([0x7F]) + pays[1][1:]
    broken = lacmutate._rebuild(lac, ent, pays)
    lacs = sw.cleared("gpu-lost", [broken, lac[:-5], lac, lacstreams.to_v2(lac)])  # CPU first
    exps = [st.expected(oracle, x) for x in lacs]
    assert exps[0].lost == [False, True, False] and exps[1].lost == [False, False, True] and not any(exps[2].lost)
    dec = gpu.lacx.Decoder(device=0)
    got = dec.stats_batch(lacs)
    assert dec.last_ms > 0
    for k, (x, exp, g) in enumerate(zip(lacs, exps, got)):
        blocks = [n for n, _ in lacmutate.table(x)[1]]
        it = sw.Item("lost %d" % k, x[3], x[8], st.rate(x), exp.left, exp.right)
        assert [r.code != 0 for r in g[1]] == exp.lost, k
        total = _check(it.name, g, it, blocks, [r.code for r in g[1]], lx=gpu.lacx)
        assert total.lost_blocks == sum(exp.lost) and total.lost_frames == sum(n for n, l in zip(blocks, exp.lost) if l), k
        for r in g[1]:
            if r.code:
                assert bytes(r)[8:] == bytes(96), k
    assert got[1][1][2].code == 10 and 1 <= got[0][1][1].code <= 9
    assert got[1][0].trail_zero_frames == 0  # the missing last block counts as sound
    assert bytes(got[2][0]) == bytes(got[3][0]) and [bytes(r) for r in got[2][1]] == [bytes(r) for r in got[3][1]]
    dec.close()


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


def _source(torch, left, right, bits, layout, offset=0, whole=None):
    placed = [Placed(torch, raw, offset, whole=whole if k == 0 else None) for k, raw in enumerate(_arrays(left, right, bits, layout))]
    return (placed[0].ptr, placed[1].ptr if len(placed) == 2 else None, layout, 1 if right is None else 2, left.size), placed


LAYOUTS = {16: (P32, I16, P16, PF32, IF32), 24: (P32, I24, PF32, IF32)}
OFFSETS = {P32: (0, 4, 8), I16: (0, 4, 8), I24: (0, 1, 2, 3, 5), P16: (0, 2, 6), PF32: (0, 4, 12), IF32: (0, 4, 8)}


def _source_signal(frames, ch, bits, grid, seed):
    left, right = sw.signal(frames, ch, bits, seed, lead=grid + 1 + seed % 4, trail=2 + seed % 3)
    sw.plant_full_scale(left, right, bits, (2 * grid - 4, 2 * grid - 1, 2 * grid, frames - 8))
    return left, right


@pytest.mark.parametrize("grid", [256, 1000, 16384])
def test_source_form_layouts_offsets_and_bounds(gpu, torch, grid):
    """Every layout at offsets between sentinels and at the very end of an allocation, on one grid: a partial last unit,
    several blocks, more than one workgroup, a silent first block; numpy's rows; the sentinels stay."""
    dec = gpu.lacx.Decoder(device=0)
    whole = torch.empty(10 << 20, dtype=torch.uint8, device="cuda")  # large enough to be an allocation of its own
    frames = 2 * grid + 1030 if grid < 16384 else 16384 + 1030  # (even: an interleaved int16 mono source at the end stays 4-byte aligned)
    for ch, bits, rate in sw.FORMATS:
        left, right = _source_signal(frames, ch, bits, grid if grid < 16384 else 300, grid + bits + ch)
        it = sw.Item("", ch, bits, rate, left, right)
        items, keep = [], []
        for layout in LAYOUTS[bits]:
            for offset in OFFSETS[layout]:
                src, placed = _source(torch, left, right, bits, layout, offset)
                items.append((src, rate, bits)), keep.append(placed)
        got = dec.stats_pcm_batch(items, block_frames=grid)
        assert dec.last_ms > 0
        for k, g in enumerate(got):
            _check((ch, bits, k), g, it, sw.grid_blocks(frames, grid), lx=gpu.lacx)
        assert all(p.untouched() for ps in keep for p in ps)
        for layout in LAYOUTS[bits]:
            src, placed = _source(torch, left, right, bits, layout, whole=whole)
            assert placed[0].offset + placed[0].n == whole.numel()
            (g,) = dec.stats_pcm_batch([(src, rate, bits)], block_frames=grid)
            _check((ch, bits, layout), g, it, sw.grid_blocks(frames, grid))
            assert all(p.untouched() for p in placed)
    dec.close()


def test_grid_257_straddles_at_every_residue(gpu, torch):
    """Grid 257: the block borders fall on every residue mod 4, so units straddle with 1, 2 and 3 frames on either side."""
    dec = gpu.lacx.Decoder(device=0)
    items, wants, keep = [], [], []
    for ch, bits, rate in sw.FORMATS:
        left, right = _source_signal(257 * 9 + 2, ch, bits, 257, 70 + bits + ch)
        t = torch.from_numpy(np.stack([left] if right is None else [left, right])).cuda()
        keep.append(t)
        items.append((t, rate, bits))
        wants.append(sw.Item("", ch, bits, rate, left, right))
    got = dec.stats_pcm_batch(items, block_frames=257)
    for g, it in zip(got, wants):
        _check((it.channels, it.depth), g, it, sw.grid_blocks(it.left.size, 257), lx=gpu.lacx)
    dec.close()


def test_an_invalid_source_sample_fails_its_item(gpu, torch):
    """A planar int32 outside the depth and an inexact float: the digest form's message, no result, the others unharmed."""
    dec = gpu.lacx.Decoder(device=0)
    left, right = sw.signal(2001, 2, 24, 12)
    good = torch.from_numpy(np.stack([left, right])).cuda()
    wide = good.clone()
    wide[1, 1001] = 1 << 24
    inexact = (good.to(torch.float32) / float(1 << 23)).contiguous()
    inexact[0, 7] = 0.3
    with pytest.raises(gpu.lacx.BatchDecodeError) as e:
        dec.stats_pcm_batch([(good, 48000, 24), (wide, 48000, 24), (inexact, 48000, 24)], block_frames=1000)
    with pytest.raises(gpu.lacx.BatchDecodeError) as d:
        dec.digest_pcm_blocks_batch([(good, 48000, 24), (wide, 48000, 24), (inexact, 48000, 24)], block_frames=1000)
    assert e.value.errors == d.value.errors == {1: "right sample at index 1001 is outside the configured PCM bit depth",
                                                2: "left sample at index 7 is not an exact 24-bit PCM value"}
    assert e.value.results[1] is None and e.value.results[2] is None
    _check("good", e.value.results[0], sw.Item("", 2, 24, 48000, left, right), sw.grid_blocks(2001, 1000))
    dec.close()


@pytest.mark.parametrize("channels,bits,rate", sw.FORMATS)
def test_source_and_stream_agree(gpu, torch, channels, bits, rate):
    """stats_pcm_batch of a tensor equals stats of the encoder's own .lac of it, row for row, and both equal numpy."""
    frames = 2 * 16384 + 777
    left, right = gpu.synth.synth_pcm(frames, channels, bits, rate, seed=80 + bits + channels, kind="mixed")
    t = torch.from_numpy(np.stack([left] if right is None else [left, right])).cuda()
    lac = gpu.lacx.Encoder(12, 2 if channels == 2 else 0, rate, bits, device=0).encode_tensor(t)
    dec = gpu.lacx.Decoder(device=0)
    (src,) = dec.stats_pcm_batch([(t, rate, bits)])
    (dcd,) = dec.stats_batch([lac])
    assert bytes(src[0]) == bytes(dcd[0]) and [bytes(r) for r in src[1]] == [bytes(r) for r in dcd[1]]
    _check("source", src, sw.Item("", channels, bits, rate, left, right), sw.grid_blocks(frames), lx=gpu.lacx)
    dec.close()


def test_the_128_bit_carry_on_the_device(gpu):
    """17 * 16384 frames of -2^23 in both channels at depth 24: seventeen full-scale blocks overflow 64 bits of sum_sq."""
    frames = 17 * 16384
    left = np.full(frames, -(1 << 23), np.int32)
    lac = gpu.lacx.Encoder(12, 2, 48000, 24, device=0).encode(left, left.copy())
    dec = gpu.lacx.Decoder(device=0)
    ((stats, rows),) = dec.stats_batch([lac])
    assert dec.last_ms > 0 and len(rows) == 17 and stats.frames == frames
    for c in (0, 1):
        assert stats.ch[c].sum_sq_hi == 1 and stats.ch[c].sum_sq == frames << 46
        assert stats.ch[c].full_scale == frames and stats.ch[c].sum == -(frames << 23) and stats.ch[c].sum_hi == -1
        assert all(r.ch[c].sum_sq == 1 << 60 and r.ch[c].full_scale == 16384 for r in rows)
    assert stats.wasted_bits == 23 and stats.dual_mono and stats.peak == 1 << 23
    dec.close()


def _cli():
    subprocess.check_call(["make", "-C", PKG_DIR, "lacx_cli"], stdout=subprocess.DEVNULL)
    return os.path.join(PKG_DIR, "lacx_cli")


def _fields(line, path):
    assert line.endswith(" " + path)
    return line[:-len(path) - 1]


def test_cli_stats(gpu, tmp_path):
    """`lacx_cli stats` on a .lac, on the WAV decoded from it (identical field values), and on a damaged file
    (lost_blocks=1; the tool is lenient like the entry point, so every file gave statistics and the exit code is 0 as
    digest's is when every file gave a digest); --blocks prints `blocks` further lines."""
    cli = _cli()
    it = next(i for i in sw.content_items() if i.name == "planted|2ch24")
    lac = gpu.lacx.Encoder(12, 2, it.rate, 24, device=0).encode(it.left, it.right)
    dec = gpu.lacx.Decoder(device=0)
    wav = dec.decode_wav(lac)
    dec.close()
    base = _fixture("decode_wav/st16_lr_3blk.lac")  # (the recipe of test_lost_and_missing_blocks: its second block is lost)
    ent, pays = lacmutate._payloads(base)
    pays[1] = pays[1][:1] + bytes([0x7F]) + pays[1][2:] if base[4] == 2 else bytes([0x7F]) + pays[1][1:]
    broken = lacmutate._rebuild(base, ent, pays)
    sw.cleared("gpu-cli", [broken])  # CPU first: what the tool will send to the device
    paths = {name: str(tmp_path / name) for name in ("a.lac", "a.wav", "broken.lac", "junk.wav")}
    for name, blob in {"a.lac": lac, "a.wav": wav, "broken.lac": broken, "junk.wav": b"RIFF" + bytes(40)}.items():
        with open(paths[name], "wb") as f:
            f.write(blob)
    total = sw.expected_totals(sw.item_rows(it), 2, 24, it.rate)
    res = subprocess.run([cli, "stats", paths["a.lac"], paths["a.wav"], paths["broken.lac"]], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and res.stderr == ""
    lines = res.stdout.splitlines()
    assert len(lines) == 3
    head = ("frames=%d channels=2 bits=24 rate=%d blocks=3 lost_blocks=0 lead_zero=%d trail_zero=%d silent_blocks=0 differing=%d wasted_bits=%d"
            % (total.frames, it.rate, total.lead, total.trail, total.differing, sw.wasted_bits(total)))
    chans = "".join(" ch%d: min=%d max=%d full_scale=%d zeros=%d sum=%d sum_sq=%d" % (c, t[0], t[1], t[3], t[4], t[5], t[6]) for c, t in enumerate(total.ch))
    assert _fields(lines[0], paths["a.lac"]) == _fields(lines[1], paths["a.wav"]) == head + chans
    assert " blocks=3 lost_blocks=1 " in lines[2] and " channels=2 bits=16 " in lines[2]
    res = subprocess.run([cli, "stats", "--blocks", paths["a.lac"]], capture_output=True, text=True, timeout=120)
    out = res.stdout.splitlines()
    assert res.returncode == 0 and len(out) == 1 + 3 and out[0] == lines[0]
    rows = sw.item_rows(it)
    for b, (text, r) in enumerate(zip(out[1:], rows)):
        assert text.startswith("  block=%d frames=%d code=0 lead_zero=%d trail_zero=%d differing=%d ch0: min=%d max=%d or_bits=%d "
                               % (b, r.frames, r.lead, r.trail, r.differing, r.ch[0][0], r.ch[0][1], r.ch[0][2])), text
        assert text.endswith(" sum=%d sum_sq=%d" % (r.ch[1][5], r.ch[1][6])), text
    res = subprocess.run([cli, "stats", paths["junk.wav"], str(tmp_path / "none.lac")], capture_output=True, text=True, timeout=120)
    assert res.returncode == 1 and res.stdout == ""
    assert res.stderr == f"Stats failed: {paths['junk.wav']}: Failed to read WAV\nStats failed: {tmp_path / 'none.lac'}: Failed to read file\n"
    res = subprocess.run([cli, "stats"], capture_output=True, text=True, timeout=120)
    assert res.returncode == 1 and "lacx_cli stats FILE... [--blocks]" in res.stderr
