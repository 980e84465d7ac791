"""Block digests on the MI355X: lacx_decoder_digest_blocks_batch_device, lacx_decoder_digest_pcm_blocks_batch_device and
the manifests made of their rows, against zlib.crc32 over numpy-built data-chunk bytes of the PCM the streams were made
from -- never the code under test.  A damaged or cut stream goes to the device only after the sanitized CPU twin of the
job (tests/native/sim_blockdigest.cpp, every buffer at exactly the plan's capacity) has passed it in this run."""
import os
import zlib

import numpy as np
import pytest

import __graft_entry__ as ge
import blockdigesttwin as bt
import lacmutate
import lacstreams
import salvagetwin as st

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FORMATS = ((1, 16, 44100), (2, 16, 48000), (1, 24, 96000), (2, 24, 192000))
SIZES = (1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 16383, 16384, 16385, 2 * 16384 + 1)  # unit, wave, workgroup and block borders
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


def _noise(frames, channels, bits, seed):
    rng = np.random.default_rng(seed)
    lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
    out = [rng.integers(lo, hi + 1, frames, dtype=np.int64).astype(np.int32) for _ in range(channels)]
    return out[0], out[1] if channels == 2 else None


def _tame(frames, channels, bits, seed):
    """Noise a few bits below full scale: what the oracle's encoder takes whatever its stereo choice."""
    left, right = _noise(frames, channels, bits, seed)
    return left >> 3, None if right is None else right >> 3


def _rows(rows):
    return [(r.frames, r.crc32, r.code) for r in rows]


def _want_rows(left, right, bits, blocks):
    return [(n, c, 0) for n, c in zip(blocks, bt.block_crcs(left, right, bits, blocks))]


def _grid(frames, grid=16384):
    return [min(grid, frames - a) for a in range(0, frames, grid)]


@pytest.fixture(scope="module")
def small_items(gpu, oracle):
    """[(stream, left, right, bits, rate, block frames)]: every format at every border size, and per format the stream of
    three blocks of 257, 258 and 259 frames."""
    items, seed = [], 0
    for ch, bits, rate in FORMATS:
        enc = gpu.lacx.Encoder(12, 2 if ch == 2 else 0, rate, bits, device=0)
        for frames in SIZES:
            seed += 1
            left, right = _noise(frames, ch, bits, seed)
            items.append((enc.encode(left, right), left, right, bits, rate, _grid(frames)))
        parts = [_tame(n, ch, bits, 900 + n + bits + ch) for n in (257, 258, 259)]
        lacs = [oracle.encode(l, r, rate, bits, 2 if ch == 2 else 0) for l, r in parts]
        left = np.concatenate([l for l, _ in parts])
        right = np.concatenate([r for _, r in parts]) if ch == 2 else None
        items.append((lacstreams.splice(lacstreams.splice(lacs[0], lacs[1]), lacs[2]), left, right, bits, rate, [257, 258, 259]))
    return items


def test_small_items_in_one_batch(gpu, small_items):
    """One batch of small items, so that items and blocks start inside other items' workgroups and waves: every row is
    zlib's, every digest what digest_batch gives, and each item's manifest is the restatement's."""
    dec = gpu.lacx.Decoder(device=0)
    lacs = [it[0] for it in small_items]
    for order in (list(range(len(lacs))), list(range(len(lacs)))[::-1]):
        got = dec.digest_blocks_batch([lacs[i] for i in order])
        assert dec.last_ms > 0
        whole = dec.digest_batch([lacs[i] for i in order])
        for i, (g, rows), w in zip(order, got, whole):
            lac, left, right, bits, rate, blocks = small_items[i]
            assert _rows(rows) == _want_rows(left, right, bits, blocks), (i, blocks)
            assert bytes(g) == bytes(w) and g.data_crc32 == zlib.crc32(bt.data_bytes(left, right, bits)) and g.wav_valid == 1, i
            want = bt.manifest_of(1 if right is None else 2, bits, rate, left.size, [(n, c) for n, c, _ in _want_rows(left, right, bits, blocks)])
            assert gpu.lacx.manifest_build(g, rows) == want, i
    assert dec.manifest(lacs[-1]) == bt.manifest_for(st.Expected(small_items[-1][1], small_items[-1][2], [False] * 3, [None] * 3, 3, 0, 774), lacs[-1])
    dec.close()


def test_lost_and_missing_blocks(gpu, oracle):
    """A lost block between two good ones, a truncated stream and a clean one in one batch: the lost rows carry their
    codes and crc32 0, the others zlib's value; the digest's CRCs are 0 unless every block decoded."""
    lac = _fixture("decode_wav/st16_lr_3blk.lac")
    ent, pays = lacmutate._payloads(lac)
    pays[1] = pays[1][:1] + bytes([0x7F]) + pays[1][2:] if lac[4] == 2 else bytes([0x7F]) + pays[1][1:]
    broken = lacmutate._rebuild(lac, ent, pays)
    lacs = [broken, lac[:-5], lac, lacstreams.to_v2(lac)]
    bt.cleared("gpu-lost", lacs, [None] * len(lacs))  # CPU first
    exps = [st.expected(oracle, x) for x in lacs]
    assert exps[0].lost == [False, True, False] and exps[1].lost == [False, False, True] and not any(exps[2].lost)
    dec = gpu.lacx.Decoder(device=0)
    got = dec.digest_blocks_batch(lacs)
    clean = dec.digest(lac)
    for x, exp, (g, rows) in zip(lacs, exps, got):
        want = bt.expected_rows(exp, x)
        assert [(r.frames, r.crc32, r.code != 0) for r in rows] == want
        assert (g.frames, g.channels, g.bit_depth, g.sample_rate) == (clean.frames, clean.channels, clean.bit_depth, clean.sample_rate)
        if any(exp.lost):
            assert (g.data_crc32, g.wav_crc32, g.wav_valid) == (0, 0, 0)
            with pytest.raises(ValueError, match="manifest needs every block's digest: block %d is lost" % exp.lost.index(True)):
                gpu.lacx.manifest_build(g, rows)
        else:
            assert bytes(g) == bytes(clean)
    assert got[1][1][2].code == 10 and 1 <= got[0][1][1].code <= 9
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


def _arrays(left, right, bits, layout):
    """The source's arrays as bytes: one for an interleaved layout, one per channel for a planar one."""
    chans = [left] if right is None else [left, right]
    if layout in (PF32, IF32):
        chans = [(x.astype(np.float32) / np.float32(1 << (bits - 1))) for x in chans]
    elif layout in (I16, P16):
        chans = [x.astype("<i2") for x in chans]
    if layout == I24:
        return [bt.data_bytes(left, right, 24)]
    if layout in (I16, IF32):
        return [np.stack(chans, axis=1).tobytes()]
    return [x.astype(x.dtype.newbyteorder("<")).tobytes() for x in chans]


def _source(torch, left, right, bits, layout, offset=0, whole=None):
    placed = [Placed(torch, raw, offset, whole=whole if k == 0 else None) for k, raw in enumerate(_arrays(left, right, bits, layout))]
    return (placed[0].ptr, placed[1].ptr if len(placed) == 2 else None, layout, 1 if right is None else 2, left.size), placed


LAYOUTS = {16: (P32, I16, P16, PF32, IF32), 24: (P32, I24, PF32, IF32)}
OFFSETS = {P32: (0, 4, 8), I16: (0, 4, 8), I24: (0, 1, 2, 3, 5), P16: (0, 2, 6), PF32: (0, 4, 12), IF32: (0, 4, 8)}


@pytest.mark.parametrize("grid", [256, 1000, 16384])
def test_source_form_layouts_offsets_and_bounds(gpu, torch, grid):
    """Every layout at offsets between sentinels and at the very end of an allocation, on one grid: a partial last unit,
    several blocks (a straddled border on grid 1000 + ...; more than one workgroup), zlib's rows; the sentinels stay."""
    dec = gpu.lacx.Decoder(device=0)
    whole = torch.empty(10 << 20, dtype=torch.uint8, device="cuda")  # large enough to be an allocation of its own
    frames = 2 * grid + 1030 if grid < 16384 else 16384 + 1030  # (even: an interleaved int16 mono source at the end stays 4-byte aligned)
    for ch, bits, rate in FORMATS:
        left, right = _noise(frames, ch, bits, grid + bits + ch)
        want = _want_rows(left, right, bits, _grid(frames, grid))
        crc = zlib.crc32(bt.data_bytes(left, right, bits))
        items, keep = [], []
        for layout in LAYOUTS[bits]:
            for offset in OFFSETS[layout]:
                src, placed = _source(torch, left, right, bits, layout, offset)
                items.append((src, rate, bits)), keep.append(placed)
        got = dec.digest_pcm_blocks_batch(items, block_frames=grid)
        for k, (g, rows) in enumerate(got):
            assert _rows(rows) == want and g.data_crc32 == crc and g.frames == frames, (ch, bits, k)
        assert all(p.untouched() for ps in keep for p in ps)
        for layout in LAYOUTS[bits]:
            src, placed = _source(torch, left, right, bits, layout, whole=whole)
            assert placed[0].offset + placed[0].n == whole.numel()
            ((g, rows),) = dec.digest_pcm_blocks_batch([(src, rate, bits)], block_frames=grid)
            assert _rows(rows) == want and g.data_crc32 == crc, (ch, bits, layout)
            assert all(p.untouched() for p in placed)
    dec.close()


def test_grid_257_straddles_at_every_residue(gpu, torch):
    """Grid 257: the block borders fall on every residue mod 4, so units straddle with 1, 2 and 3 frames on either side."""
    dec = gpu.lacx.Decoder(device=0)
    items, wants, keep = [], [], []
    for ch, bits, rate in FORMATS:
        left, right = _noise(257 * 9 + 2, ch, bits, 70 + bits + ch)
        t = torch.from_numpy(np.stack([left] if right is None else [left, right])).cuda()
        keep.append(t)
        items.append((t, rate, bits))
        wants.append(_want_rows(left, right, bits, _grid(left.size, 257)))
    got = dec.digest_pcm_blocks_batch(items, block_frames=257)
    assert [_rows(rows) for _, rows in got] == wants
    dec.close()


@pytest.mark.parametrize("channels,bits,rate", FORMATS)
def test_manifest_of_source_is_manifest_of_its_stream(gpu, torch, channels, bits, rate):
    """The manifest made of source PCM on the encoder's grid equals, byte for byte, the manifest of the encoder's own .lac
    of that PCM -- and both the restatement's."""
    frames = 2 * 16384 + 777
    left, right = gpu.synth.synth_pcm(frames, channels, bits, rate, seed=80 + bits + channels, kind="mixed")
    t = torch.from_numpy(np.stack([left] if right is None else [left, right])).cuda()
    enc = gpu.lacx.Encoder(12, 2 if channels == 2 else 0, rate, bits, device=0)
    lac = enc.encode_tensor(t)
    dec = gpu.lacx.Decoder(device=0)
    ((g, rows),) = dec.digest_pcm_blocks_batch([(t, rate, bits)])
    from_source = gpu.lacx.manifest_build(g, rows)
    assert from_source == dec.manifest(lac)
    assert from_source == bt.manifest_of(channels, bits, rate, frames, [(n, c) for n, c, _ in _want_rows(left, right, bits, _grid(frames))])
    info, back = gpu.lacx.manifest_parse(from_source)
    assert info.data_crc32 == zlib.crc32(bt.data_bytes(left, right, bits)) and len(back) == 3
    dec.close()
