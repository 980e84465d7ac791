"""Frame windows of .lac streams on the MI355X (lacx_decoder_decode_window, lacx_decoder_decode_window_batch_device):
the pinned fixtures of tests/golden/decode_wav.json at every block boundary, encoded streams of every format mixed in one
batch, damage that stays outside a window, row views of a torch tensor as outputs, batches larger than one resident
round of lanes, and a handle shared with the whole-stream decoders.  Every expected answer comes from outside the window
path: the encoded input PCM, or a full decode whose WAV matches the pinned sha256."""
import ctypes as C
import hashlib
import json
import os
import random
import struct

import numpy as np
import pytest

import __graft_entry__ as ge
import lacstreams
import wavutil as W

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SENTINEL = 0x5A5A5A5A


@pytest.fixture(scope="module")
def gpu():
    pkg = ge.load_pkg()
    if pkg.lacx.device_count() <= 0:
        pytest.fail("no HIP device: the decoder has no CPU fallback")
    return pkg


def _fixture(name):
    with open(os.path.join(GOLDEN, name), "rb") as f:
        return f.read()


def _block_frames(lac):
    """Frame counts of the blocks of a version-3 or version-2 stream."""
    nb = struct.unpack(">I", lac[10:14])[0]
    entry = 8 if lac[2] == 3 else 4
    return [struct.unpack(">I", lac[14 + entry * b:18 + entry * b])[0] for b in range(nb)]


def _as_f32(pcm, bit_depth):
    return pcm.astype(np.float32) / 2 ** (bit_depth - 1)


def _want(pcm, bit_depth, dtype):
    return pcm.astype(np.int32) if dtype == np.int32 else _as_f32(pcm, bit_depth)


def _same(got, want):
    """Bit-equal (float32 compared by its bits)."""
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got.view(np.int32), want.view(np.int32))


def _windows(lac):
    """(start, frames) of: frame 0, the last frame, 2 frames across each block boundary, one inside a block, the whole."""
    fr = _block_frames(lac)
    total = sum(fr)
    out = [(0, 1), (total - 1, 1), (0, total)]
    edge = 0
    for n in fr[:-1]:
        edge += n
        out.append((edge - 1, 2))
    b = len(fr) // 2
    first = sum(fr[:b])
    if fr[b] >= 3:
        out.append((first + 1, fr[b] - 2))
    return out


def _pinned(gpu):
    """[(name, stream, left, right, bit_depth)]: the full decode of each pinned stream, checked against its pinned WAV."""
    with open(os.path.join(GOLDEN, "decode_wav.json")) as f:
        ents = json.load(f)
    assert len(ents) == 26
    out = []
    dec = gpu.lacx.Decoder(device=0)
    for e in ents:
        lac = lacstreams.from_recipe(e["source"], _fixture)
        left, right, info, _ = dec.decode(lac)
        wav = W.make_wav(left, right, info.sample_rate, info.bit_depth)
        assert hashlib.sha256(wav).hexdigest() == e["wav_sha256"], e["name"]
        out.append((e["name"], lac, left.copy(), None if right is None else right.copy(), info.bit_depth))
    dec.close()
    return out


def _torch_outputs(torch, channels, frames, dtype):
    tdt = torch.int32 if dtype == np.int32 else torch.float32
    l = torch.empty(frames, dtype=tdt, device="cuda")
    r = torch.empty(frames, dtype=tdt, device="cuda") if channels == 2 else None
    return (l, r), (l.data_ptr(), r.data_ptr() if r is not None else None)


@pytest.mark.parametrize("dtype", [np.int32, np.float32])
def test_pinned_fixtures_every_boundary(gpu, dtype):
    import torch
    streams = _pinned(gpu)
    assert any(lac[2] == 2 for _, lac, *_ in streams) and any(len(_block_frames(lac)) >= 3 for _, lac, *_ in streams)
    dec = gpu.lacx.Decoder(device=0)
    batch = []  # (stream, start, frames, want_left, want_right)
    for name, lac, left, right, bd in streams:
        for start, n in _windows(lac):
            got_l, got_r = dec.decode_window(lac, start, n, dtype=dtype)
            assert _same(got_l, _want(left[start:start + n], bd, dtype)), (name, start, n)
            if right is None:
                assert got_r is None
            else:
                assert _same(got_r, _want(right[start:start + n], bd, dtype)), (name, start, n)
            batch.append((lac, start, n, _want(left[start:start + n], bd, dtype),
                          None if right is None else _want(right[start:start + n], bd, dtype)))
    assert dec.last_ms > 0
    # all of them as one batch, shuffled
    random.Random(11).shuffle(batch)
    tensors, outs = zip(*[_torch_outputs(torch, 1 if b[4] is None else 2, b[2], dtype) for b in batch])
    infos = dec.decode_window_batch_device([b[0] for b in batch], [b[1] for b in batch], [b[2] for b in batch], list(outs),
                                           dtype=np.dtype(dtype).name)
    torch.cuda.synchronize()
    for (lac, start, n, wl, wr), (l, r), inf in zip(batch, tensors, infos):
        assert inf.frames == sum(_block_frames(lac))
        assert _same(l.cpu().numpy(), wl), (start, n)
        if wr is not None:
            assert _same(r.cpu().numpy(), wr), (start, n)
    dec.close()


def _encoded(gpu):
    """Every rate, both depths, mono and stereo, LR / MS / auto, several blocks: [(stream, left, right, bit_depth)]."""
    out = []
    k = 0
    for rate in (44100, 48000, 96000, 192000):
        for bd in (16, 24):
            for ch, sm in ((1, 0), (2, 0), (2, 1), (2, 2)):
                frames = (1, 300, 4097, 16385, 2 * 16384 + 1001, 3 * 16384 + 7)[k % 6]
                kind = ("music", "mixed", "noise", "sparse", "tone")[k % 5]
                left, right = gpu.synth.synth_pcm(frames, ch, bd, rate, seed=700 + k, kind=kind)
                lac = gpu.lacx.Encoder(12, sm, rate, bd, device=0).encode(left, right)
                out.append((lac, np.asarray(left, dtype=np.int32), None if right is None else np.asarray(right, dtype=np.int32), bd))
                k += 1
    return out


@pytest.mark.parametrize("dtype", [np.int32, np.float32])
def test_encoded_random_windows_mixed_batch(gpu, dtype):
    import torch
    streams = _encoded(gpu)
    assert len(streams) == 32 and {s[1].size for s in streams} >= {1, 3 * 16384 + 7}
    rng = np.random.default_rng(21 if dtype == np.int32 else 22)
    items = []
    for lac, left, right, bd in streams:
        for _ in range(3):
            total = left.size
            n = int(rng.integers(1, min(total, 40000) + 1))
            start = int(rng.integers(0, total - n + 1))
            items.append((lac, start, n, left, right, bd))
    order = rng.permutation(len(items))
    items = [items[i] for i in order]
    assert any(it[4] is None for it in items) and any(it[4] is not None for it in items)
    dec = gpu.lacx.Decoder(device=0)
    tensors, outs = zip(*[_torch_outputs(torch, 1 if it[4] is None else 2, it[2], dtype) for it in items])
    dec.decode_window_batch_device([it[0] for it in items], [it[1] for it in items], [it[2] for it in items], list(outs),
                                   dtype=dtype)
    for (lac, start, n, left, right, bd), (l, r) in zip(items, tensors):
        assert _same(l.cpu().numpy(), _want(left[start:start + n], bd, dtype)), (start, n)
        if right is not None:
            assert _same(r.cpu().numpy(), _want(right[start:start + n], bd, dtype)), (start, n)
    # the host form of a few of them
    for lac, start, n, left, right, bd in items[:6]:
        gl, gr = dec.decode_window(lac, start, n, dtype=dtype)
        assert _same(gl, _want(left[start:start + n], bd, dtype))
        assert (gr is None) == (right is None)
        if right is not None:
            assert _same(gr, _want(right[start:start + n], bd, dtype))
    dec.close()


def _damaged_block1(gpu):
    """A 4-block stereo stream with an impossible predictor type in block 1's first channel header (the damage of
    test_gpu_decode.py::test_damaged_streams_are_refused), its input PCM and its block edges."""
    left, right = gpu.synth.synth_pcm(16384 * 3 + 77, 2, 16, 48000, seed=5, kind="music")
    lac = gpu.lacx.Encoder(12, 2, 48000, 16, device=0).encode(left, right)
    info = gpu.lacx.stream_parse(lac)
    assert info.blocks == 4
    head = 14 + 8 * info.blocks
    n0 = int.from_bytes(lac[18:22], "big")
    bad = bytearray(lac)
    bad[head + n0 + 1] = 7
    edges = np.cumsum([0] + _block_frames(lac)).tolist()
    return bytes(bad), np.asarray(left, dtype=np.int32), np.asarray(right, dtype=np.int32), edges


def test_damage_outside_the_window(gpu):
    import torch
    bad, left, right, e = _damaged_block1(gpu)
    with pytest.raises(RuntimeError) as full:
        gpu.lacx.Decoder(device=0).decode(bad)
    msg = str(full.value)
    assert msg.startswith("[decode-error] block=1 ")
    dec = gpu.lacx.Decoder(device=0)
    good = [(e[0], e[1]), (e[0] + 100, 50), (e[2], e[3] - e[2]), (e[2] + 5, e[4] - e[2] - 5), (e[3], e[4] - e[3]),
            (e[4] - 1, 1)]
    touching = [(e[1], 1), (e[1] - 1, 2), (e[2] - 1, 2), (e[0], e[4]), (e[1] + 10, 20)]
    for start, n in good:
        gl, gr = dec.decode_window(bad, start, n)
        assert np.array_equal(gl, left[start:start + n]) and np.array_equal(gr, right[start:start + n]), (start, n)
    for start, n in touching:
        with pytest.raises(RuntimeError) as err:
            dec.decode_window(bad, start, n)
        assert str(err.value) == msg, (start, n)
    # in a batch the touching item fails with the full decode's message, the others stay exact
    items = good[:3] + [touching[0]] + good[3:]
    tensors, outs = zip(*[_torch_outputs(torch, 2, n, np.int32) for _, n in items])
    with pytest.raises(gpu.lacx.BatchDecodeError) as be:
        dec.decode_window_batch_device([bad] * len(items), [s for s, _ in items], [n for _, n in items], list(outs))
    assert be.value.errors == {3: msg} and str(be.value) == "stream 3: " + msg
    for i, ((start, n), (l, r)) in enumerate(zip(items, tensors)):
        if i == 3:
            assert be.value.results[i] is None
            continue
        assert np.array_equal(l.cpu().numpy(), left[start:start + n]) and np.array_equal(r.cpu().numpy(), right[start:start + n])
    dec.close()


def test_row_views_of_an_odd_tensor(gpu):
    """Outputs that are only element-aligned: row slices [i, c, 1:T + 1] of an [n, 2, T + 2] tensor with odd T, on a
    non-default stream; the sentinel columns and a mono item's right row stay as they were."""
    import torch
    streams = [s for s in _encoded(gpu) if s[1].size >= 4097][:9]
    T = 3001
    rng = np.random.default_rng(5)
    for dtype, tdt in ((np.int32, torch.int32), (np.float32, torch.float32)):
        n = len(streams)
        out = torch.full((n, 2, T + 2), SENTINEL, dtype=torch.int32, device="cuda")
        view = out if tdt == torch.int32 else out.view(torch.float32)
        starts = [int(rng.integers(0, s[1].size - T + 1)) for s in streams]
        outputs = []
        for i, s in enumerate(streams):
            l = view[i, 0, 1:T + 1]
            r = view[i, 1, 1:T + 1]
            assert l.data_ptr() % 16 != 0 or r.data_ptr() % 16 != 0 or i == 0
            outputs.append((l.data_ptr(), r.data_ptr() if s[2] is not None else None))
        side = torch.cuda.Stream()
        dec = gpu.lacx.Decoder(device=0)
        with torch.cuda.stream(side):
            junk = torch.ones(1 << 22, dtype=torch.int32, device="cuda").cumsum(0)  # work already queued on the stream
            dec.decode_window_batch_device([s[0] for s in streams], starts, T, outputs, dtype=dtype, stream=side.cuda_stream)
        side.synchronize()
        assert int(junk[-1]) == 1 << 22
        host = out.cpu().numpy()
        assert (host[:, :, 0] == SENTINEL).all() and (host[:, :, T + 1] == SENTINEL).all()
        for i, (lac, left, right, bd) in enumerate(streams):
            st = starts[i]
            got_l = host[i, 0, 1:T + 1].view(np.float32) if dtype == np.float32 else host[i, 0, 1:T + 1]
            assert _same(np.ascontiguousarray(got_l), _want(left[st:st + T], bd, dtype)), i
            if right is None:
                assert (host[i, 1] == SENTINEL).all(), i
            else:
                got_r = host[i, 1, 1:T + 1].view(np.float32) if dtype == np.float32 else host[i, 1, 1:T + 1]
                assert _same(np.ascontiguousarray(got_r), _want(right[st:st + T], bd, dtype)), i
        dec.close()


def _repeat_block(lac, copies):
    """A version-3 stream of `copies` copies of the single block of `lac` (the container layout of lacstreams)."""
    assert lac[2] == 3 and struct.unpack(">I", lac[10:14])[0] == 1
    return lac[:10] + struct.pack(">I", copies) + lac[14:22] * copies + lac[22:] * copies


def test_more_blocks_than_one_resident_round(gpu):
    import torch
    items = []
    for k, (ch, bd, rate, sm, kind) in enumerate([(2, 16, 44100, 2, "music"), (1, 24, 96000, 0, "mixed"),
                                                  (2, 24, 48000, 1, "noise"), (2, 16, 48000, 0, "tone")]):
        left, right = gpu.synth.synth_pcm(256, ch, bd, rate, seed=950 + k, kind=kind)
        copies = 10007 + 13 * k
        lac = _repeat_block(gpu.lacx.Encoder(12, sm, rate, bd, device=0).encode(left, right), copies)
        tl = np.tile(np.asarray(left, dtype=np.int32), copies)
        tr = None if right is None else np.tile(np.asarray(right, dtype=np.int32), copies)
        items.append((lac, 100, 256 * copies - 300, tl, tr, bd))  # every block but the first and last frames
    assert sum(-(-(it[1] + it[2]) // 256) for it in items) > 40000
    dec = gpu.lacx.Decoder(device=0)
    for dtype in (np.int32, np.float32):
        tensors, outs = zip(*[_torch_outputs(torch, 1 if it[4] is None else 2, it[2], dtype) for it in items])
        dec.decode_window_batch_device([it[0] for it in items], [it[1] for it in items], [it[2] for it in items], list(outs),
                                       dtype=dtype)
        for (lac, start, n, left, right, bd), (l, r) in zip(items, tensors):
            assert _same(l.cpu().numpy(), _want(left[start:start + n], bd, dtype))
            if right is not None:
                assert _same(r.cpu().numpy(), _want(right[start:start + n], bd, dtype))
    dec.close()


def _host_window(gpu, dec, lac, start, left, right, sample_type):
    buf = np.frombuffer(lac, dtype=np.uint8)
    return gpu.lacx.lib().lacx_decoder_decode_window(dec._h, buf.ctypes.data_as(C.POINTER(C.c_uint8)), C.c_uint64(buf.size),
                                                     C.c_uint64(start), C.c_uint64(left.size), C.c_int(sample_type),
                                                     C.c_void_p(left.ctypes.data), C.c_void_p(right.ctypes.data), None)


def test_handle_shared_with_whole_stream_decodes(gpu):
    import torch
    streams = _encoded(gpu)
    big = [s for s in streams if s[1].size > 2 * 16384]
    bad, bl, br, e = _damaged_block1(gpu)
    dec = gpu.lacx.Decoder(device=0)
    lac, left, right, bd = big[0]
    for round_ in range(2):
        gl, gr = dec.decode_window(lac, 16000, 800)
        assert np.array_equal(gl, left[16000:16800]) and (gr is None) == (right is None)
        l, r, info, _ = dec.decode(lac)
        assert np.array_equal(l, left) and (right is None or np.array_equal(r, right))
        views = dec.decode_wav_batch_view([s[0] for s in big])
        assert [bytes(v) for v in views] == [W.make_wav(s[1], s[2], gpu.lacx.stream_parse(s[0]).sample_rate, s[3]) for s in big]
        gl, gr = dec.decode_window(big[1][0], 5, 20000, dtype=np.float32)
        assert _same(gl, _as_f32(big[1][1][5:20005], big[1][3]))
        infos = [gpu.lacx.stream_parse(s[0]) for s in big]
        tensors, outs = zip(*[_torch_outputs(torch, inf.channels, inf.frames, np.int32) for inf in infos])
        dec.decode_batch_device([s[0] for s in big], list(outs))
        for s, (tl, tr) in zip(big, tensors):
            assert np.array_equal(tl.cpu().numpy(), s[1]) and (tr is None or np.array_equal(tr.cpu().numpy(), s[2]))
        tensors, outs = zip(*[_torch_outputs(torch, 1 if s[2] is None else 2, 1000, np.int32) for s in big])
        dec.decode_window_batch_device([s[0] for s in big], [7] * len(big), 1000, list(outs))
        for s, (tl, tr) in zip(big, tensors):
            assert np.array_equal(tl.cpu().numpy(), s[1][7:1007]) and (tr is None or np.array_equal(tr.cpu().numpy(), s[2][7:1007]))
    # a failing window leaves the caller's host arrays untouched: on the device, and on the host
    L = gpu.lacx.lib()
    for start, n in ((e[1] + 3, 40), (e[4] - 10, 11), (0, 0)):
        sl = np.full(max(n, 1), SENTINEL, dtype=np.int32)
        sr = np.full(max(n, 1), SENTINEL, dtype=np.int32)
        if n == 0:
            sl, sr = sl[:0], sr[:0]
        rc = _host_window(gpu, dec, bad, start, sl, sr, gpu.lacx.SAMPLE_I32)
        assert rc in (gpu.lacx.E_RUNTIME, gpu.lacx.E_INVALID)
        assert not L.lacx_decode_last_error().decode().startswith("stream ")
        assert (sl == SENTINEL).all() and (sr == SENTINEL).all()
    sl, sr = np.zeros(64, dtype=np.int32), np.zeros(64, dtype=np.int32)
    assert _host_window(gpu, dec, bad, e[3] + 1, sl, sr, gpu.lacx.SAMPLE_I32) == gpu.lacx.OK
    assert np.array_equal(sl, bl[e[3] + 1:e[3] + 65]) and np.array_equal(sr, br[e[3] + 1:e[3] + 65])
    dec.close()
