"""The tensor layouts (LACX_PCM_PLANAR_I16, _PLANAR_F32, _INTERLEAVED_F32) on the MI355X: the import pass in front of the
encoder, the verify form's new sources, and the refusals.  Every expected byte comes from outside the new code: the golden
.lac files, and the encode of the same PCM as planar int32."""
import json
import os

import numpy as np
import pytest

import __graft_entry__ as ge
import importtwin as T
import vertwin as V

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
P, I16, I24 = 0, 1, 2
PI16, PF32, IF32 = 16, 17, 18


@pytest.fixture(scope="module")
def gpu():
    pkg = ge.load_pkg()
    if pkg.lacx.device_count() <= 0:
        pytest.fail("no HIP device: the encoder has no CPU fallback")
    assert (pkg.lacx.PCM_PLANAR_I16, pkg.lacx.PCM_PLANAR_F32, pkg.lacx.PCM_INTERLEAVED_F32) == (PI16, PF32, IF32)
    return pkg


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


def _new_layouts(depth):
    return (PI16, PF32, IF32) if depth == 16 else (PF32, IF32)


def _old_layouts(depth):
    return (P, I16) if depth == 16 else (P, I24)


class Src:
    """PCM on the device in `layout`, its base `offset` elements behind a 256-byte aligned address; a [2, frames] planar
    source is one block, so that an odd frame count leaves the right row where it lies in such a tensor.  .arg: the
    (data_ptr, layout, channels, frames, data1_ptr) tuple of the binding."""

    def __init__(self, torch, left, right, depth, layout, offset=0, raw=()):
        ch = 1 if right is None else 2
        rows = [np.asarray(left, dtype=np.int64)] + ([np.asarray(right, dtype=np.int64)] if ch == 2 else [])
        n = rows[0].size
        if layout == P:
            host = np.concatenate(rows).astype(np.int32)
        elif layout == PI16:
            host = np.concatenate(rows).astype(np.int16)
        elif layout == PF32:
            host = np.concatenate([T.to_float(r, depth) for r in rows])
        elif layout == IF32:
            host = np.stack([T.to_float(r, depth) for r in rows], axis=1).reshape(-1)
        else:
            host = np.frombuffer(T.pack(np.stack(rows, axis=1), depth), dtype=np.uint8)
        host = host.copy()
        for f, c, v in raw:  # float values written as they are
            host[f * ch + c if layout == IF32 else c * n + f] = v
        self.buf = torch.zeros(offset + host.size + 64, dtype=getattr(torch, host.dtype.name), device="cuda")
        self.buf[offset:offset + host.size] = torch.from_numpy(host).cuda()
        size = host.dtype.itemsize
        ptr = self.buf.data_ptr() + offset * size
        planar = layout in (P, PI16, PF32)
        self.arg = (ptr, layout, ch, n, ptr + n * size if planar and ch == 2 else None)
        self.verify_arg = (ptr, self.arg[4], layout, ch, n)


@pytest.fixture(scope="module")
def streams(gpu):
    """(name, rate, depth, stereo mode, left, right, golden .lac or None): tests/golden/small, and one seeded stream of
    32 769 frames per format."""
    with open(os.path.join(GOLDEN, "small", "index.json")) as f:
        index = json.load(f)
    out = []
    for ent in index:
        g = ent["gen"]
        left, right = gpu.synth.synth_pcm(g["frames"], g["channels"], g["bit_depth"], g["sample_rate"], seed=g["seed"],
                                          kind=g["kind"], stereo=g["stereo"])
        with open(os.path.join(GOLDEN, "small", ent["name"] + ".lac"), "rb") as f:
            out.append((ent["name"], g["sample_rate"], g["bit_depth"], ent["stereo_mode"], left, right, f.read()))
    for k, (ch, depth, rate, mode) in enumerate(((2, 16, 48000, 2), (2, 24, 96000, 1), (1, 24, 44100, 0), (1, 16, 48000, 0))):
        left, right = gpu.synth.synth_pcm(32769, ch, depth, rate, seed=900 + k, kind="mixed")
        out.append((f"seeded{k}", rate, depth, mode, left, right, None))
    assert {s[3] for s in out} == {0, 1, 2} and {s[2] for s in out} == {16, 24}
    return out


def _encoder(gpu, s, zero_run=True, partitioning=True):
    enc = gpu.lacx.Encoder(12, s[3], s[1], s[2], device=0)
    if not (zero_run and partitioning):
        enc.set_zero_run_enabled(zero_run)
        enc.set_partitioning_enabled(partitioning)
    return enc


def _view(enc, src):
    pay, tab = enc.encode_shard_pcm_device_view(*src.arg[:4], data1_ptr=src.arg[4])
    return pay.tobytes(), np.array(tab, copy=True)


def _begin_end(enc, src):
    enc.encode_shard_pcm_device_begin(*src.arg[:4], data1_ptr=src.arg[4])
    pay, tab = enc.encode_shard_end()
    return pay.tobytes(), np.array(tab, copy=True)


@pytest.fixture(scope="module")
def reference(gpu, torch, streams):
    """name -> (payload, table) of the planar int32 encode, the golden checked where there is one; computed once."""
    out = {}
    for s in streams:
        enc = _encoder(gpu, s)
        pay, tab = _view(enc, Src(torch, s[4], s[5], s[2], P))
        lac = gpu.lacx.assemble(s[1], s[2], s[3], 1 if s[5] is None else 2, [(pay, tab)])
        assert s[6] is None or lac == s[6], s[0]
        out[s[0]] = (pay, tab, lac)
        enc.close()
    return out


def test_byte_identity_view_and_begin_end(gpu, torch, streams, reference):
    k = 0
    for s in streams:
        enc = _encoder(gpu, s)
        want_pay, want_tab, want_lac = reference[s[0]]
        for layout in _new_layouts(s[2]):
            for call in (_view, _begin_end):
                k += 1
                pay, tab = call(enc, Src(torch, s[4], s[5], s[2], layout, offset=k % 4))
                assert pay == want_pay and np.array_equal(tab, want_tab), (s[0], layout, call.__name__, k % 4)
                assert gpu.lacx.assemble(s[1], s[2], s[3], 1 if s[5] is None else 2, [(pay, tab)]) == want_lac
        enc.close()


@pytest.mark.parametrize("zero_run,partitioning", ((False, False), (True, False), (False, True)))
def test_byte_identity_under_the_switches(gpu, torch, streams, zero_run, partitioning):
    for s in (x for x in streams if x[0] in ("n16421_st16", "n16421_st24_lr", "sparse_mono24", "silence_st16", "seeded0")):
        enc = _encoder(gpu, s, zero_run, partitioning)
        want_pay, want_tab = _view(enc, Src(torch, s[4], s[5], s[2], P))
        for k, layout in enumerate(_new_layouts(s[2])):
            pay, tab = _view(enc, Src(torch, s[4], s[5], s[2], layout, offset=1 + k))
            assert pay == want_pay and np.array_equal(tab, want_tab), (s[0], layout)
        enc.close()


def test_one_batch_of_mixed_layouts(gpu, torch, streams, reference):
    """Everything as ONE lacx_encode_batch_device job: old and new layouts alternate item by item, bases misaligned."""
    jobs = []
    for s in streams:
        old, new = _old_layouts(s[2]), _new_layouts(s[2])
        for i in range(max(len(old), len(new))):
            jobs.append((s, old[i % len(old)]))
            jobs.append((s, new[i % len(new)]))
    srcs = []
    for k, (s, layout) in enumerate(jobs):
        # (interleaved int16 keeps its 4-byte aligned base; its elements here are bytes, as packed int24's, which lies anywhere)
        srcs.append(Src(torch, s[4], s[5], s[2], layout, offset=4 * (k % 2) if layout == I16 else k % 4))
    be = gpu.lacx.BatchEncoder([(s[1], s[2], s[3]) for s, _ in jobs], device=0)
    outs = be.encode_device([x.arg for x in srcs])
    assert len(outs) == len(jobs) >= 100
    for (s, layout), (pay, tab) in zip(jobs, outs):
        want_pay, want_tab, _ = reference[s[0]]
        assert pay.tobytes() == want_pay and np.array_equal(tab.array(), want_tab), (s[0], layout)


def test_float_round_trip_through_the_window_decode(gpu, torch, streams):
    """decode_window_batch_device(float32) into [C, T] tensors, the tensors straight back: the goldens' bytes."""
    gold = [s for s in streams if s[6] is not None]
    dec = gpu.lacx.Decoder(device=0)
    tensors = [torch.full((1 if s[5] is None else 2, len(s[4])), 7.0, dtype=torch.float32, device="cuda") for s in gold]
    outs = [(t[0].data_ptr(), t[1].data_ptr() if t.shape[0] == 2 else None) for t in tensors]
    dec.decode_window_batch_device([s[6] for s in gold], [0] * len(gold), [len(s[4]) for s in gold], outs, dtype="float32")
    dec.close()
    for s, t in zip(gold, tensors):
        enc = _encoder(gpu, s)
        assert enc.encode_tensor(t) == s[6], s[0]
        if t.shape[0] == 2 and t.shape[1] > 2:  # ... and as [T, C]
            assert enc.encode_tensor(t.t().contiguous()) == s[6], s[0]
        if s[2] == 16:  # ... and the int16 tensor of the same samples
            i16 = torch.from_numpy(np.stack([s[4]] + ([] if s[5] is None else [s[5]])).astype(np.int16)).cuda()
            assert enc.encode_tensor(i16) == s[6], s[0]
        enc.close()


def _message(depth, ch, pos, kind):
    what = "is outside the configured PCM bit depth" if kind == 1 else f"is not an exact {depth}-bit PCM value"
    return f"{'right' if ch else 'left'} sample at index {pos} {what}"


def test_validation_on_the_device(gpu, torch, streams, reference):
    """The invalid-value corpus of the host test, one bad value per stream: through the single call, and inside a batch
    with good neighbours; the same encoder encodes a good stream right afterwards."""
    unit = T.unit_frames()
    for name in ("seeded0", "seeded1"):
        s = next(x for x in streams if x[0] == name)
        depth, n = s[2], len(s[4])
        positions = (0, n - 1, unit - 1, unit, 255, 256, 2 * 16384 - 1, 2 * 16384)
        enc = _encoder(gpu, s)
        good = Src(torch, s[4], s[5], depth, PF32, offset=1)
        be = gpu.lacx.BatchEncoder([(s[1], depth, s[3])] * 3, device=0)
        for vi, (val, kind) in enumerate(T.invalid_values(depth)):
            layout = (PF32, IF32)[vi % 2]
            pos, ch = positions[vi % len(positions)], (vi // 2) % 2
            bad = Src(torch, s[4], s[5], depth, layout, offset=vi % 4, raw=[(pos, ch, val)])
            if kind == 0:  # a sample after all: encodes, and differs from the reference only if the value does
                _view(enc, bad)
                continue
            for call in (_view, _begin_end):
                with pytest.raises(ValueError) as e:
                    call(enc, bad)
                assert str(e.value) == _message(depth, ch, pos, kind), (depth, val)
                assert _view(enc, good)[0] == reference[name][0]  # the encoder is usable, and right
            with pytest.raises(ValueError) as e:
                be.encode_device([good.arg, bad.arg, good.arg])
            assert str(e.value) == "stream 1: " + _message(depth, ch, pos, kind), (depth, val)
            outs = be.encode_device([good.arg, good.arg, good.arg])
            assert all(p.tobytes() == reference[name][0] for p, _ in outs)
        # which channel: both (left wins, though its index is higher), two in one channel (the lowest wins)
        both = Src(torch, s[4], s[5], depth, PF32, raw=[(3, 1, np.float32(0.3)), (900, 0, np.float32(1.0)), (30000, 0, np.float32(0.3))])
        with pytest.raises(ValueError) as e:
            _view(enc, both)
        assert str(e.value) == _message(depth, 0, 900, 1)
        right = Src(torch, s[4], s[5], depth, IF32, offset=3, raw=[(n - 1, 1, np.float32(np.nan)), (unit, 1, np.float32(2.0))])
        with pytest.raises(ValueError) as e:
            be.encode_device([right.arg, good.arg, both.arg])
        assert str(e.value) == "stream 0: " + _message(depth, 1, unit, 1)
        enc.close()


def _blocks(lac):
    nb = int.from_bytes(lac[10:14], "big")
    return [int.from_bytes(lac[14 + 8 * b:18 + 8 * b], "big") for b in range(nb)]


def test_verify_matches_the_twin(gpu, torch, streams):
    """Sources in the three layouts, identical and altered, against verify_core.h on the host, field by field."""
    lx = gpu.lacx
    dec = lx.Decoder(device=0)
    other = lambda v: int(v) - 1 if int(v) > 0 else int(v) + 1
    for name, ms in (("n16421_st24_lr", 0), ("n257_st16_ms", 1), ("n33_mono16", 0), ("n16421_st16", None)):
        s = next(x for x in streams if x[0] == name)
        depth, lac, n = s[2], s[6], len(s[4])
        ch = 1 if s[5] is None else 2
        samples = [np.asarray(s[4], dtype=np.int64)] + ([np.asarray(s[5], dtype=np.int64)] if ch == 2 else [])
        bf = _blocks(lac)
        for k, layout in enumerate(_new_layouts(depth)):
            clean = Src(torch, s[4], s[5], depth, layout, offset=k + 1)
            (r,) = dec.verify_batch_device([lac], [clean.verify_arg])
            assert bytes(r) == bytes(32), (name, layout)
            if ms is None:  # per-block stereo: the block flags are the stream's own business; identical is identical
                continue
            for f, c, raw in ((0, 0, None), (n - 1, ch - 1, None), (min(n - 1, 16384), 0, None), (n // 2, ch - 1, np.float32(np.nan)),
                              (n // 3, 0, np.float32(0.3)), (5, ch - 1, np.float32(1.0))):
                edited = [x.copy() for x in samples]
                if raw is None:
                    edited[c][f] = other(samples[c][f])
                elif layout == PI16:
                    continue
                src = Src(torch, edited[0], edited[1] if ch == 2 else None, depth, layout, offset=k,
                          raw=[] if raw is None else [(f, c, raw)])
                with pytest.raises(lx.BatchDecodeError) as e:
                    dec.verify_batch_device([s[6], lac], [clean.verify_arg, src.verify_arg])
                got = e.value.results[1]
                assert bytes(e.value.results[0]) == bytes(32)
                # the twin: the same source bytes through verify_core.h on the host
                host = src.buf.cpu().numpy()
                off = (src.arg[0] - src.buf.data_ptr()) // host.itemsize
                s0 = T.aligned(host.size, host.dtype, off % (16 // host.itemsize))
                s0[:] = np.roll(host, -off)
                s1 = s0[n:] if layout != IF32 and ch == 2 else None
                sl, sr = V.to_scratch(samples[0], samples[1] if ch == 2 else None, bf, [ms] * len(bf))
                want = T.verify_layout(ch, depth, layout, bf, [ms] * len(bf), [0] * len(bf), sl, sr, s0, s1)
                assert (got.mismatches, 2 * got.frame + got.channel, got.decoded, got.source, got.block) == want[:5], (name, layout, f, c)
                assert want.mismatches == 1 and want.key == 2 * f + c
                assert e.value.errors[1] == (f"[verify-error] block={want.block} channel={'right' if c else 'left'} frame={f} "
                                             f"decoded={want.decoded} source={want.source} mismatches=1")
                assert str(e.value) == "stream 1: " + e.value.errors[1]
    # misaligned and missing arrays: the host's messages
    s = next(x for x in streams if x[0] == "n257_st16_ms")
    src = Src(torch, s[4], s[5], 16, PI16)
    f32 = Src(torch, s[4], s[5], 16, PF32)
    p0, p1 = src.verify_arg[0], src.verify_arg[1]
    q0, q1 = f32.verify_arg[0], f32.verify_arg[1]
    with pytest.raises(lx.BatchDecodeError) as e:
        dec.verify_batch_device([s[6]] * 5, [(p0 + 1, p1, PI16, 2, 257), (p0, None, PI16, 2, 257), (q0 + 2, q1, PF32, 2, 257),
                                             (q0, q1 + 2, PF32, 2, 257), (q0 + 2, None, IF32, 2, 257)])
    assert e.value.errors == {0: "source arrays are not 2-byte aligned", 1: "source arrays missing",
                              2: "source arrays are not 4-byte aligned", 3: "source arrays are not 4-byte aligned",
                              4: "source arrays are not 4-byte aligned"}
    dec.close()


def test_refusals(gpu, torch, streams):
    lx = gpu.lacx
    s = next(x for x in streams if x[0] == "n257_st16_ms")
    deep = next(x for x in streams if x[0] == "n16421_st24_lr")
    src, f32 = Src(torch, s[4], s[5], 16, PI16), Src(torch, s[4], s[5], 16, PF32)
    enc, enc24 = _encoder(gpu, s), _encoder(gpu, deep)
    dec = lx.Decoder(device=0)
    ptr, _, ch, n, ptr1 = f32.arg
    for code in (3, 15, 19, 0xFFFFFFFF):  # unknown on both sides
        with pytest.raises(ValueError, match="^unknown PCM layout$"):
            enc.encode_shard_pcm_device_view(ptr, code, ch, n, data1_ptr=ptr1)
        with pytest.raises(ValueError, match="^stream 0: unknown PCM layout$"):
            lx.BatchEncoder([(s[1], 16, s[3])], device=0).encode_device([(ptr, code, ch, n, ptr1)])
        with pytest.raises(lx.BatchDecodeError, match="^stream 0: unknown source layout$"):
            dec.verify_batch_device([s[6]], [(ptr, ptr1, code, ch, n)])
    with pytest.raises(ValueError, match="^PCM layout does not match the configured bit depth$"):
        enc24.encode_shard_pcm_device_view(*src.arg[:4], data1_ptr=src.arg[4])
    with pytest.raises(ValueError, match="^stream 0: PCM layout does not match the bit depth$"):
        lx.BatchEncoder([(deep[1], 24, deep[3])], device=0).encode_device([src.arg])
    with pytest.raises(lx.BatchDecodeError, match="source layout does not match the stream's bit depth"):
        dec.verify_batch_device([deep[6]], [(src.arg[0], src.arg[4], PI16, 2, len(deep[4]))])
    planar = "^planar PCM: data1 must be the right channel of stereo input and null for mono$"
    with pytest.raises(ValueError, match=planar):
        enc.encode_shard_pcm_device_view(ptr, PF32, 2, n)
    with pytest.raises(ValueError, match=planar):
        enc.encode_shard_pcm_device_view(ptr, PI16, 1, n, data1_ptr=ptr1)
    with pytest.raises(ValueError, match="^PCM arrays are not 4-byte aligned$"):
        enc.encode_shard_pcm_device_view(ptr + 2, PF32, 2, n, data1_ptr=ptr1)
    with pytest.raises(ValueError, match="^PCM arrays are not 4-byte aligned$"):
        enc.encode_shard_pcm_device_begin(ptr + 1, IF32, 2, n)
    with pytest.raises(ValueError, match="^PCM arrays are not 2-byte aligned$"):
        enc.encode_shard_pcm_device_view(src.arg[0], PI16, 2, n, data1_ptr=src.arg[4] + 1)
    pay, _ = enc.encode_shard_pcm_device_view(*f32.arg[:4], data1_ptr=f32.arg[4])  # the encoder is still usable
    assert len(pay) > 0
    fan = lx.Encoder(12, s[3], s[1], 16, devices=[0])  # the fan-out entry point: out of scope, refused
    for arg in (src.arg, f32.arg, Src(torch, s[4], s[5], 16, IF32).arg):
        with pytest.raises(ValueError, match="^PCM layout is not supported by the fan-out$"):
            fan.encode_fanout_resident([arg])
    fan.close()
    enc.close(), enc24.close(), dec.close()
