"""Every encode entry point that builds a result -- a complete .lac or a shard -- at two small shapes, byte for byte against
the oracle: a 16-bit stereo stream of three blocks (per-block stereo mode, the last block short) and a 24-bit mono stream
of one block (the smallest head, 22 bytes).  Each call runs twice on one encoder; the forms that hand out views of the
encoder's buffers run again after a larger call on the same encoder, where a head left over from that call would show."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BLOCK = 16384
# name: (frames, frames of the larger call, channels, bit depth, sample rate, stereo mode, kind)
FORMATS = {"st16": (BLOCK * 2 + 77, BLOCK * 5 + 300, 2, 16, 48000, 2, "mixed"), "mono24": (300, BLOCK * 2 + 9, 1, 24, 96000, 0, "music")}


class Case:
    def __init__(self, gpu, oracle, name):
        import torch
        import wavutil as W

        frames, big, self.ch, self.bd, self.sr, self.sm, kind = FORMATS[name]
        self.layout = gpu.lacx.PCM_INTERLEAVED_I16 if self.bd == 16 else gpu.lacx.PCM_INTERLEAVED_I24
        self.small, self.big = [self._stream(gpu, oracle, torch, W, n, kind, seed) for n, seed in ((frames, 61), (big, 62))]

    def _stream(self, gpu, oracle, torch, W, frames, kind, seed):
        left, right = gpu.synth.synth_pcm(frames, self.ch, self.bd, self.sr, seed=seed, kind=kind)
        inter = gpu.synth.interleave(left, right, self.bd)
        s = dict(frames=frames, left=left, right=right, want=oracle.encode(left, right, self.sr, self.bd, self.sm, threads=4),
                 wav=W.make_wav(left, right, self.sr, self.bd), dl=torch.from_numpy(left).cuda(),
                 dr=torch.from_numpy(right).cuda() if self.ch == 2 else None,
                 inter=torch.from_numpy(inter.view(np.int16) if self.bd == 16 else inter).cuda())
        s["ptrs"] = (s["dl"].data_ptr(), s["dr"].data_ptr() if self.ch == 2 else None)
        torch.cuda.synchronize()
        return s

    def encoder(self, gpu, **kw):
        return gpu.lacx.Encoder(12, self.sm, self.sr, self.bd, **({"device": 0} if not kw else kw))

    def lac(self, gpu, shard):
        payload, table = shard
        payload = payload if isinstance(payload, bytes) else payload.tobytes()
        return gpu.lacx.assemble(self.sr, self.bd, self.sm, self.ch, [(payload, np.array(table, copy=True))])


@pytest.fixture(scope="module")
def cases(pkg, oracle):
    if pkg.lacx.device_count() < 1:
        pytest.fail("no HIP device visible: GPU tests need an MI355X (the product has no CPU fallback)")
    return pkg, {name: Case(pkg, oracle, name) for name in FORMATS}


def _small_big_small(call, c):
    """call(stream) -> .lac bytes: the small stream twice, the larger one, the small one again."""
    for s in (c.small, c.small, c.big, c.small):
        assert call(s) == s["want"], s["frames"]


@pytest.mark.parametrize("host_emit", [False, True], ids=["device_emit", "host_emit"])
@pytest.mark.parametrize("name", sorted(FORMATS))
def test_encode_and_encode_device(cases, name, host_emit):
    gpu, c = cases[0], cases[1][name]
    enc = c.encoder(gpu)
    enc.set_host_emit(host_emit)
    assert len(c.small["want"]) > 14 + 8 * -(-c.small["frames"] // BLOCK)
    _small_big_small(lambda s: enc.encode(s["left"], s["right"]), c)
    _small_big_small(lambda s: enc.encode_device(*s["ptrs"], s["left"], s["right"], s["frames"]), c)


@pytest.mark.parametrize("name", sorted(FORMATS))
def test_encode_wav_and_its_view(cases, name):
    gpu, c = cases[0], cases[1][name]
    enc = c.encoder(gpu)
    _small_big_small(lambda s: enc.encode_wav(s["wav"]), c)
    _small_big_small(lambda s: enc.encode_wav_view(s["wav"]).tobytes(), c)
    _small_big_small(lambda s: enc.encode_wav(s["wav"]), c)  # the copies come from the same place


@pytest.mark.parametrize("host_emit", [False, True], ids=["device_emit", "host_emit"])
@pytest.mark.parametrize("name", sorted(FORMATS))
def test_shards_and_assemble(cases, name, host_emit):
    gpu, c = cases[0], cases[1][name]
    enc = c.encoder(gpu)
    enc.set_host_emit(host_emit)
    _small_big_small(lambda s: c.lac(gpu, enc.encode_shard(s["left"], s["right"])), c)
    _small_big_small(lambda s: c.lac(gpu, enc.encode_shard_device(*s["ptrs"], s["left"], s["right"], s["frames"])), c)
    _small_big_small(lambda s: c.lac(gpu, enc.encode_shard_device_view(*s["ptrs"], s["left"], s["right"], s["frames"])), c)


@pytest.mark.parametrize("name", sorted(FORMATS))
def test_shard_pcm_device_view_and_begin_end(cases, name):
    gpu, c = cases[0], cases[1][name]
    enc = c.encoder(gpu)
    _small_big_small(lambda s: c.lac(gpu, enc.encode_shard_pcm_device_view(s["inter"].data_ptr(), c.layout, c.ch, s["frames"])), c)
    _small_big_small(lambda s: c.lac(gpu, enc.encode_shard_pcm_device_view(s["ptrs"][0], gpu.lacx.PCM_PLANAR_I32, c.ch, s["frames"],
                                                                           data1_ptr=s["ptrs"][1])), c)

    def begin_end(s):
        enc.encode_shard_pcm_device_begin(s["inter"].data_ptr(), c.layout, c.ch, s["frames"])
        return c.lac(gpu, enc.encode_shard_end())
    _small_big_small(begin_end, c)


@pytest.mark.parametrize("name", sorted(FORMATS))
def test_two_lanes_on_one_device(cases, name):
    """The host-sum exchange with two lanes on one GPU: the second lane's worker thread runs, and each lane writes its own
    slice of the block table."""
    gpu, c = cases[0], cases[1][name]
    enc = c.encoder(gpu, devices=[0, 0], min_blocks_per_device=1)
    assert enc.lanes() == 2
    for call in (lambda s: enc.encode(s["left"], s["right"]), lambda s: enc.encode_wav(s["wav"]),
                 lambda s: enc.encode_wav_view(s["wav"]).tobytes()):
        _small_big_small(call, c)
        st = enc.fanout_stats()
        nb = -(-c.small["frames"] // BLOCK)
        assert st.lanes_used == min(2, nb) and st.exchange == gpu.lacx.EXCHANGE_HOST
        assert sum(st.blocks[g] for g in range(st.lanes_used)) == nb
