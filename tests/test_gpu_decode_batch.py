"""Many .lac streams as one decode on the MI355X (lacx_decoder_decode_wav_batch*, lacx_decoder_decode_batch_device): the
pinned reference WAV images of tests/golden/decode_wav.json in one call, every format mixed in one batch, failures that
stay with their item, device-resident outputs, batches larger than one resident round of lanes, and a handle shared by
batch and single-stream calls.  Every item must equal what the single-stream decoders give for it alone (a batch of one)
and an answer that does not come from the decoder: the pinned reference bytes, or the canonical WAV of the encoded PCM."""
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


@pytest.fixture(scope="module")
def gpu():
    pkg = ge.load_pkg()
    if pkg.lacx.device_count() <= 0:
        pytest.fail("no HIP device: the decoder has no CPU fallback")
    return pkg


def _fixture(name):
    with open(os.path.join(GOLDEN, name), "rb") as f:
        return f.read()


def _entries():
    with open(os.path.join(GOLDEN, "decode_wav.json")) as f:
        return json.load(f)


def _sha(b):
    return hashlib.sha256(bytes(b)).hexdigest()


def _single_error(gpu, lac):
    with pytest.raises(RuntimeError) as e:
        gpu.lacx.Decoder(device=0).decode_wav(lac)
    return str(e.value)


def test_pinned_reference_wavs_in_one_batch(gpu):
    ents = _entries()
    assert len(ents) == 26
    lacs = [lacstreams.from_recipe(e["source"], _fixture) for e in ents]
    assert any(x[2] == 2 for x in lacs) and any(x[2] == 3 for x in lacs)
    dec = gpu.lacx.Decoder(device=0)
    views = dec.decode_wav_batch_view(lacs)
    for e, v in zip(ents, views):
        assert v.dtype == np.uint8 and (v.size, _sha(v)) == (e["wav_bytes"], e["wav_sha256"]), e["name"]
        assert bytes(v[:44]).hex() == e["header_hex"], e["name"]
    assert dec.last_ms > 0
    got = dec.decode_wav_batch(lacs)
    assert [(len(w), _sha(w)) for w in got] == [(e["wav_bytes"], e["wav_sha256"]) for e in ents]
    single = [dec.decode_wav(x) for x in lacs]
    assert [(len(w), _sha(w)) for w in single] == [(e["wav_bytes"], e["wav_sha256"]) for e in ents]
    # shuffled, with duplicates, and one at a time
    rng = random.Random(7)
    order = list(range(len(lacs))) + [3, 3, 0, 25, 11]
    rng.shuffle(order)
    assert dec.decode_wav_batch([lacs[i] for i in order]) == [single[i] for i in order]
    assert [bytes(v) for v in dec.decode_wav_batch_view([lacs[i] for i in order])] == [single[i] for i in order]
    for i in range(len(lacs)):
        assert dec.decode_wav_batch([lacs[i]]) == [single[i]]
    dec.close()


def _mixed_streams(gpu):
    """Every rate, both depths, mono and stereo, LR / MS / auto, 1 frame to several blocks, and version-2 rewrites:
    (streams, the canonical WAV of each stream's encoded PCM)."""
    out, wavs = [], []
    k = 0
    for rate in (44100, 48000, 96000, 192000):
        for bd in (16, 24):
            for ch, sm in ((1, 0), (2, 0), (2, 1), (2, 2)):
                frames = (1, 255, 256, 4097, 16384, 16385, 2 * 16384 + 1001, 3 * 16384 + 7)[k % 8]
                kind = ("music", "mixed", "noise", "sparse", "tone")[k % 5]
                left, right = gpu.synth.synth_pcm(frames, ch, bd, rate, seed=300 + k, kind=kind)
                lac = gpu.lacx.Encoder(12, sm, rate, bd, device=0).encode(left, right)
                wav = W.make_wav(left, right, rate, bd)
                out.append(lac)
                wavs.append(wav)
                if k % 5 == 0:
                    out.append(lacstreams.to_v2(lac))
                    wavs.append(wav)
                k += 1
    return out, wavs


def test_mixed_formats(gpu):
    lacs, wavs = _mixed_streams(gpu)
    assert len(lacs) >= 38
    dec = gpu.lacx.Decoder(device=0)
    got = dec.decode_wav_batch(lacs)
    views = [bytes(v) for v in dec.decode_wav_batch_view(lacs)]
    for i, lac in enumerate(lacs):
        want = wavs[i]
        assert got[i] == want and views[i] == want, i
        assert dec.decode_wav(lac) == want, i
        left, right, info, _ = gpu.lacx.decode(lac)
        assert W.make_wav(left, right, info.sample_rate, info.bit_depth) == want, i
    dec.close()


def _bad_items(gpu):
    """(name, stream) that fail alone: a damaged payload, a truncated stream, a loud 24-bit stream labelled 16-bit."""
    left, right = gpu.synth.synth_pcm(16384 * 3 + 77, 2, 24, 96000, seed=5, kind="music")
    lac = gpu.lacx.Encoder(12, 2, 96000, 24, device=0).encode(left, right)
    loud = bytearray(lac)
    loud[8] = 16  # status 7: blocks decode, samples leave the depth
    damaged = None
    for pos in range(len(lac) // 2, len(lac) - 64, 997):  # a damage that the decoder refuses
        bad = bytearray(lac)
        bad[pos] ^= 0x55
        try:
            gpu.lacx.decode(bytes(bad))
        except RuntimeError:
            damaged = bytes(bad)
            break
    assert damaged is not None
    return [("damaged", damaged), ("truncated", lac[:-1]), ("loud", bytes(loud))]


def test_failures_stay_local(gpu):
    good, good_wavs = (x[:12] for x in _mixed_streams(gpu))
    bad = _bad_items(gpu)
    lacs, wavs = list(good), list(good_wavs)
    where = {}
    for j, (name, b) in enumerate(bad):
        at = 3 + 4 * j
        lacs.insert(at, b)
        wavs.insert(at, None)
        where[at] = name
    dec = gpu.lacx.Decoder(device=0)
    want_err = {i: _single_error(gpu, lacs[i]) for i in where}
    assert all(m.startswith("[decode-error] ") for m in want_err.values()), want_err
    assert "sample outside the bit depth" in want_err[[i for i, n in where.items() if n == "loud"][0]]
    singles = {i: dec.decode_wav(x) for i, x in enumerate(lacs) if i not in where}
    assert all(singles[i] == wavs[i] for i in singles)
    for fn in (dec.decode_wav_batch, dec.decode_wav_batch_view):
        with pytest.raises(gpu.lacx.BatchDecodeError) as e:
            fn(lacs)
        err = e.value
        assert err.errors == want_err
        low = min(where)
        assert str(err) == f"stream {low}: {want_err[low]}"
        for i, r in enumerate(err.results):
            if i in where:
                assert r is None
            else:
                assert bytes(r) == singles[i], i
    # the return code is the lowest failing item's: a truncated stream fails on the host (LACX_E_INVALID), the others
    # on the device (LACX_E_RUNTIME)
    import ctypes as C

    L, lx = gpu.lacx.lib(), gpu.lacx
    for first in ("truncated", "loud"):
        items = [x for name, x in bad if name == first] + good[:2]
        bufs = [np.frombuffer(x, dtype=np.uint8) for x in items]
        spans = (lx.Span * 3)(*[lx.Span(b.ctypes.data_as(C.POINTER(C.c_uint8)), b.size) for b in bufs])
        outs = (lx.Span * 3)()
        rcs = (C.c_int * 3)()
        rc = L.lacx_decoder_decode_wav_batch_view(dec._h, spans, 3, outs, rcs, None)
        assert rc == (lx.E_INVALID if first == "truncated" else lx.E_RUNTIME)
        assert list(rcs) == [rc, lx.OK, lx.OK]
        assert L.lacx_decode_last_error().decode().startswith("stream 0: [decode-error] ")
        assert not outs[0].data and outs[1].size > 44
    dec.close()


def _device_outputs(torch, infos, extra=64):
    outs, tensors = [], []
    for inf in infos:
        l = torch.full((inf.frames + extra,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        r = torch.full((inf.frames + extra,), 0x5A5A5A5A, dtype=torch.int32, device="cuda") if inf.channels == 2 else None
        tensors.append((l, r))
        outs.append((l.data_ptr(), r.data_ptr() if r is not None else None))
    return outs, tensors


def test_device_output(gpu):
    import torch
    lacs = _mixed_streams(gpu)[0][:20]
    bad = _bad_items(gpu)
    lacs.insert(5, bad[2][1])  # loud: parses, fails on the device
    lacs.insert(9, bad[0][1])  # damaged payload
    infos = [gpu.lacx.stream_parse(x) for x in lacs]
    dec = gpu.lacx.Decoder(device=0)
    outs, tensors = _device_outputs(torch, infos)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        junk = torch.ones(1 << 24, dtype=torch.int32, device="cuda").cumsum(0)  # work already queued on the stream
        with pytest.raises(gpu.lacx.BatchDecodeError) as e:
            dec.decode_batch_device(lacs, outs, side.cuda_stream)
    assert int(junk[-1]) == 1 << 24
    assert set(e.value.errors) == {5, 9}
    for i, lac in enumerate(lacs):
        l, r = tensors[i]
        sentinel = torch.full((64,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        assert torch.equal(l[infos[i].frames:], sentinel), i
        if r is not None:
            assert torch.equal(r[infos[i].frames:], sentinel), i
        if i in (5, 9):
            assert e.value.results[i] is None
            continue
        want_l, want_r, _, _ = gpu.lacx.decode(lac)
        assert e.value.results[i].frames == infos[i].frames
        assert np.array_equal(l[:infos[i].frames].cpu().numpy(), want_l), i
        if r is not None:
            assert np.array_equal(r[:infos[i].frames].cpu().numpy(), want_r), i
    # all good: the null stream and the default torch stream
    good = [x for i, x in enumerate(lacs) if i not in (5, 9)]
    ginfos = [gpu.lacx.stream_parse(x) for x in good]
    outs, tensors = _device_outputs(torch, ginfos)
    res = dec.decode_batch_device(good, outs)
    assert [r.frames for r in res] == [inf.frames for inf in ginfos]
    for lac, (l, r), inf in zip(good, tensors, ginfos):
        want_l, want_r, _, _ = gpu.lacx.decode(lac)
        assert np.array_equal(l[:inf.frames].cpu().numpy(), want_l)
        if r is not None:
            assert np.array_equal(r[:inf.frames].cpu().numpy(), want_r)
    dec.close()


def _repeat_block(lac, copies):
    """A version-3 stream of `copies` copies of the single block of `lac`, tables and payloads built in one pass (the
    container layout of lacstreams)."""
    assert lac[2] == 3 and struct.unpack(">I", lac[10:14])[0] == 1
    entry = lac[14:22]
    payload = lac[22:]
    return lac[:10] + struct.pack(">I", copies) + entry * copies + payload * copies


def test_more_blocks_than_one_resident_round(gpu):
    items = []
    for k, (ch, bd, rate, sm, kind) in enumerate([(2, 16, 44100, 2, "music"), (1, 24, 96000, 0, "mixed"),
                                                  (2, 24, 48000, 1, "noise"), (2, 16, 48000, 0, "tone")]):
        left, right = gpu.synth.synth_pcm(256, ch, bd, rate, seed=900 + k, kind=kind)
        one = gpu.lacx.Encoder(12, sm, rate, bd, device=0).encode(left, right)
        items.append(_repeat_block(one, 10007 + 13 * k))
    total = sum(gpu.lacx.stream_parse(x).blocks for x in items)
    assert total > 40000
    dec = gpu.lacx.Decoder(device=0)
    got = dec.decode_wav_batch_view(items)
    for lac, v in zip(items, got):
        left, right, info, _ = gpu.lacx.decode(lac)
        assert _sha(v) == _sha(W.make_wav(left, right, info.sample_rate, info.bit_depth))
    import torch
    infos = [gpu.lacx.stream_parse(x) for x in items]
    outs, tensors = _device_outputs(torch, infos)
    dec.decode_batch_device(items, outs)
    for lac, (l, r), inf in zip(items, tensors, infos):
        want_l, want_r, _, _ = gpu.lacx.decode(lac)
        assert np.array_equal(l[:inf.frames].cpu().numpy(), want_l)
        if r is not None:
            assert np.array_equal(r[:inf.frames].cpu().numpy(), want_r)
    dec.close()


def _host_decode(gpu, dec, lac, left, right):
    """lacx_decoder_decode into caller-owned host arrays: the return code."""
    import ctypes as C

    buf = np.frombuffer(lac, dtype=np.uint8)
    i32 = C.POINTER(C.c_int32)
    return gpu.lacx.lib().lacx_decoder_decode(dec._h, buf.ctypes.data_as(C.POINTER(C.c_uint8)), C.c_uint64(buf.size),
                                              left.ctypes.data_as(i32), right.ctypes.data_as(i32), C.c_uint64(left.size),
                                              None)


def test_handle_reuse(gpu):
    left, right = gpu.synth.synth_pcm(256, 2, 16, 48000, seed=77, kind="music")
    big = [_repeat_block(gpu.lacx.Encoder(12, 2, 48000, 16, device=0).encode(left, right), 3000)] * 4
    small, small_wavs = (x[:6] for x in _mixed_streams(gpu))
    lone_l, lone_r = gpu.synth.synth_pcm(5 * 16384 + 3, 2, 24, 96000, seed=78, kind="mixed")
    lone = gpu.lacx.Encoder(12, 2, 96000, 24, device=0).encode(lone_l, lone_r)
    fresh = gpu.lacx.Decoder(device=0)
    want_big = fresh.decode_wav(big[0])
    assert want_big == W.make_wav(np.tile(left, 3000), np.tile(right, 3000), 48000, 16)
    want_small = [fresh.decode_wav(x) for x in small]
    assert want_small == small_wavs
    fresh.close()
    dec = gpu.lacx.Decoder(device=0)
    assert [bytes(v) for v in dec.decode_wav_batch_view(big)] == [want_big] * 4
    assert dec.decode_wav_batch(small) == want_small
    assert dec.decode_wav(lone) == W.make_wav(lone_l, lone_r, 96000, 24)
    l, r, _, _ = dec.decode(lone)
    assert np.array_equal(l, lone_l) and np.array_equal(r, lone_r)
    assert dec.decode_wav_batch(small + [lone]) == want_small + [W.make_wav(lone_l, lone_r, 96000, 24)]
    assert [bytes(v) for v in dec.decode_wav_batch_view(big[:1] + small[:1])] == [want_big, want_small[0]]
    # single calls are batches of one but leave lacx_decoder_item_error to the last batch call
    bad = dict(_bad_items(gpu))
    items = small[:3] + [bad["loud"]] + small[3:]
    with pytest.raises(gpu.lacx.BatchDecodeError) as e:
        dec.decode_wav_batch(items)
    assert set(e.value.errors) == {3} and "sample outside the bit depth" in e.value.errors[3]
    batch_msgs = [e.value.errors.get(i, "") for i in range(len(items))]
    L = gpu.lacx.lib()

    def item_errors():
        return [L.lacx_decoder_item_error(dec._h, i).decode() for i in range(len(items))]

    assert item_errors() == batch_msgs
    l, r, _, _ = dec.decode(lone)
    assert np.array_equal(l, lone_l) and np.array_equal(r, lone_r)
    with pytest.raises(RuntimeError) as single:
        dec.decode_wav(bad["damaged"])
    assert str(single.value).startswith("[decode-error] block=")  # the item's own message, no "stream 0: "
    assert item_errors() == batch_msgs
    # a failing single decode leaves the caller's arrays as they were: parse errors, and failures on the device
    info = gpu.lacx.stream_parse(bad["loud"])
    for lac in (bad["loud"], bad["damaged"], bad["truncated"]):
        sl = np.full(info.frames, 0x5A5A5A5A, dtype=np.int32)
        sr = np.full(info.frames, 0x5A5A5A5A, dtype=np.int32)
        rc = _host_decode(gpu, dec, lac, sl, sr)
        assert rc in (gpu.lacx.E_RUNTIME, gpu.lacx.E_INVALID)
        assert L.lacx_decode_last_error().decode().startswith("[decode-error] ")
        assert (sl == 0x5A5A5A5A).all() and (sr == 0x5A5A5A5A).all()
    assert item_errors() == batch_msgs
    sl, sr = np.zeros(lone_l.size, dtype=np.int32), np.zeros(lone_l.size, dtype=np.int32)
    assert _host_decode(gpu, dec, lone, sl, sr) == gpu.lacx.OK
    assert np.array_equal(sl, lone_l) and np.array_equal(sr, lone_r)
    dec.close()
