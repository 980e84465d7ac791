"""Measurement (not part of the default suite): what does decoding through errors cost on streams that have none?
Workload: that of decode_batch_bench.py -- `n` synthetic 4-minute stereo 16-bit music streams (distinct seeds), encoded on
the GPU, undamaged.  After a warm-up round, `iters` rounds, the two routes alternating inside every round, wall ms of each
(every route ends synchronised) and the kernel ms the library reports:
  decode    Decoder.decode_wav_batch_view: k_decode, then k_wav_pack (inverse, range check and pack in one pass)
  salvage   the library's lacx_decoder_salvage_wav_batch_view: k_decode, then k_ms_inverse in place and k_salvage_wav --
            one more write and read of the PCM, 8 bytes per sample where blocks are mid/side
Both routes' images are compared once, in the warm-up round (equal bytes, no faults).
Printed: best / median / min..max per route and the ratio of the medians.
usage: salvage_bench.py [n] [iters] [seconds] [rate]"""
import ctypes as C
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import __graft_entry__ as ge  # noqa: E402

pkg = ge.load_pkg()
lacx, synth = pkg.lacx, pkg.synth
n = int(sys.argv[1]) if len(sys.argv) > 1 else 48
iters = int(sys.argv[2]) if len(sys.argv) > 2 else 5
secs = int(sys.argv[3]) if len(sys.argv) > 3 else 240
sr = int(sys.argv[4]) if len(sys.argv) > 4 else 48000
bd = 16
if lacx.device_count() < 1:
    raise SystemExit("salvage_bench needs a HIP device")

t0 = time.perf_counter()
enc = lacx.Encoder(12, 2, sr, bd, device=0)
lacs = []
with ThreadPoolExecutor(16) as ex:  # numpy releases the GIL inside the generator's arithmetic
    for left, right in ex.map(lambda k: synth.synth_pcm(secs * sr, 2, bd, sr, seed=5000 + k, kind="music"), range(n)):
        lacs.append(enc.encode(left, right))
del left, right
infos = [lacx.stream_parse(x) for x in lacs]
frames = sum(i.frames for i in infos)
print(f"set-up {time.perf_counter() - t0:.0f} s: {n} x {secs} s stereo {bd}/{sr / 1000:g} music, {sum(i.blocks for i in infos)} blocks, "
      f"{sum(map(len, lacs)) / 1e6:.0f} MB .lac, {4 * frames / 1e6:.0f} MB of 16-bit PCM")

dec = lacx.Decoder(device=0)
bufs = [np.frombuffer(x, dtype=np.uint8) for x in lacs]
spans = (lacx.Span * n)(*[lacx.Span(b.ctypes.data_as(C.POINTER(C.c_uint8)), b.size) for b in bufs])
outs = (lacx.Span * n)()
rcs = (C.c_int * n)()
results = (lacx.SalvageResult * n)()
ms = C.c_float()


def salvage_views():
    """The view form, as decode_wav_batch_view is one: no copy of the images on either route."""
    rc = lacx.lib().lacx_decoder_salvage_wav_batch_view(dec._h, spans, C.c_uint32(n), outs, rcs, results, C.byref(ms))
    assert rc == 0, lacx.lib().lacx_decode_last_error().decode()
    return [np.ctypeslib.as_array(o.data, shape=(o.size,)) for o in outs]


res = {k: [] for k in ("w_decode", "k_decode", "w_salvage", "k_salvage")}
for it in range(iters + 1):  # the first round is the warm-up
    t1 = time.perf_counter()
    views = dec.decode_wav_batch_view(lacs)
    t2 = time.perf_counter()
    k_d = dec.last_ms
    if it == 0:
        want = [v.copy() for v in views]
    t3 = time.perf_counter()
    views = salvage_views()
    t4 = time.perf_counter()
    k_s = float(ms.value)
    if it == 0:
        assert all(np.array_equal(a, b) for a, b in zip(want, views)) and all(r.bad_blocks == 0 and r.lost_frames == 0 for r in results)
        del want
    else:
        for k, v in (("w_decode", (t2 - t1) * 1e3), ("k_decode", k_d), ("w_salvage", (t4 - t3) * 1e3), ("k_salvage", k_s)):
            res[k].append(v)


def line(key):
    v = res[key]
    return f"{np.min(v):.2f} / {np.median(v):.2f} ms (min..max {np.min(v):.2f}..{np.max(v):.2f})"


print(f"{iters} rounds after warm-up, routes alternating inside a round; best / median (spread); equal images, no faults")
print(f"  decode_wav_batch_view    wall {line('w_decode')}   kernels {line('k_decode')}")
print(f"  salvage_wav_batch_view   wall {line('w_salvage')}   kernels {line('k_salvage')}")
print(f"  salvage / decode, medians: wall {np.median(res['w_salvage']) / np.median(res['w_decode']):.3f}, "
      f"kernels {np.median(res['k_salvage']) / np.median(res['k_decode']):.3f}")
print(f"  post pass bytes: k_wav_pack reads {8 * frames / 1e9:.3f} GB, writes {4 * frames / 1e9:.3f} GB; salvage adds k_ms_inverse over "
      f"the same {8 * frames / 1e9:.3f} GB (read, and written where blocks are mid/side) before k_salvage_wav reads and writes as much as k_wav_pack")
