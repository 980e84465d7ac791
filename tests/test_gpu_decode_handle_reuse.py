"""One lacx_decoder handle through every decode form in turn (MI355X): its grow-only buffers are shared between the
forms -- the image buffer by the WAV and host-window forms, the PCM buffers by all but the in-place device form -- and are
reused when a later call needs less.  A fixed sequence over tests/golden/small (31 to 16 421 frames) puts mono after
stereo and stereo after mono, a small job after a large one and a large one after that; every result must equal, byte
for byte, what a fresh handle gives for the same fixture."""
import os
import struct

import numpy as np
import pytest

import __graft_entry__ as ge

pytestmark = pytest.mark.gpu
SMALL = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "small")


def _lac(name):
    with open(os.path.join(SMALL, name + ".lac"), "rb") as f:
        return f.read()


def _fresh(lacx, call):
    """call(decoder) on a handle that has done nothing else."""
    dec = lacx.Decoder(device=0)
    try:
        return call(dec)
    finally:
        dec.close()


def _pcm_equal(got, want):
    return all((g is None and w is None) or (g is not None and w is not None and g.dtype == w.dtype and
                                              np.array_equal(g.view(np.int32), w.view(np.int32))) for g, w in zip(got, want))


def test_one_handle_through_every_form():
    import torch

    lacx = ge.load_pkg().lacx
    if lacx.device_count() <= 0:
        pytest.fail("no HIP device: the decoder has no CPU fallback")
    mono33, st24_big, st16_big = _lac("n33_mono16"), _lac("n16421_st24_lr"), _lac("n16421_st16")
    batch = [_lac("n4097_st16"), mono33, _lac("n257_st16_ms")]
    st4096, st24_31 = _lac("n4096_st16"), _lac("n31_st24")
    border = struct.unpack(">I", st16_big[14:18])[0]  # frames of the first block
    assert 2 <= border < 16421
    win = (border - 2, 5)  # two frames before the border, three behind it

    want_wav33 = _fresh(lacx, lambda d: d.decode_wav(mono33))
    want_big = _fresh(lacx, lambda d: d.decode(st24_big)[:2])
    want_win = {dt: _fresh(lacx, lambda d: d.decode_window(st16_big, *win, dtype=dt)) for dt in (np.int32, np.float32)}
    want_batch = [_fresh(lacx, lambda d: d.decode(x)[:2]) for x in batch]
    wav4096 = _fresh(lacx, lambda d: d.decode_wav(st4096))
    want_wav31 = _fresh(lacx, lambda d: d.decode_wav(st24_31))
    frame, channel = 1234, 1  # one sample of the source changed: 16-bit stereo, 4 bytes per frame
    at = 44 + 4 * frame + 2 * channel
    changed = wav4096[:at] + bytes([wav4096[at] ^ 1]) + wav4096[at + 1:]
    want_differs = _fresh(lacx, lambda d: d.verify_wav(st4096, changed))
    assert want_differs.mismatches == 1 and (want_differs.frame, want_differs.channel) == (frame, channel)

    dec = lacx.Decoder(device=0)
    try:
        assert bytes(dec.decode_wav_view(mono33)) == want_wav33                                     # 1
        assert _pcm_equal(dec.decode(st24_big)[:2], want_big)                                       # 2
        for dt in (np.int32, np.float32):                                                           # 3
            got = dec.decode_window(st16_big, *win, dtype=dt)
            assert got[0].shape == (5,) and _pcm_equal(got, want_win[dt]), dt
        infos = [lacx.stream_parse(x) for x in batch]                                               # 4
        tensors = [(torch.full((i.frames,), 0x5A5A5A5A, dtype=torch.int32, device="cuda"),
                    torch.full((i.frames,), 0x5A5A5A5A, dtype=torch.int32, device="cuda") if i.channels == 2 else None)
                   for i in infos]
        dec.decode_batch_device(batch, [(l.data_ptr(), r.data_ptr() if r is not None else None) for l, r in tensors])
        torch.cuda.synchronize()
        for (l, r), want in zip(tensors, want_batch):
            assert _pcm_equal((l.cpu().numpy(), r.cpu().numpy() if r is not None else None), want)
        same = dec.verify_wav(st4096, wav4096)                                                      # 5
        assert same.identical and same.mismatches == 0
        differs = dec.verify_wav(st4096, changed)
        assert not differs.identical and differs.mismatches == 1
        assert (differs.frame, differs.channel, differs.block) == (frame, channel, want_differs.block)
        assert (differs.decoded, differs.source, differs.message) == (want_differs.decoded, want_differs.source, want_differs.message)
        assert bytes(dec.decode_wav_view(st24_31)) == want_wav31                                    # 6
        assert _pcm_equal(dec.decode(st24_big)[:2], want_big)                                       # 7
    finally:
        dec.close()
