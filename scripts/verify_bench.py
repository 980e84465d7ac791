"""Measurement (not part of the default suite): "is every .lac of this collection lossless for its PCM?" three ways.
Workload: that of decode_batch_bench.py -- `n` synthetic 4-minute stereo 16-bit music streams (distinct seeds), encoded on
the GPU -- with the sources resident on the device as the interleaved int16 data chunks they were read from.  After a
warm-up round, `iters` rounds, the three routes alternating inside every round, wall ms of each (every route ends
synchronised) and the kernel ms the library reports:
  verify    Decoder.verify_batch_device against the interleaved int16 sources: nothing but 32 bytes per item comes back
  (a)       Decoder.decode_batch_device into torch tensors, then torch.equal with planar int32 sources, on the device
  (b)       Decoder.decode_wav_batch_view, then a host compare of every image's data region with the WAV data
Printed: best / median / min..max per route, and the bytes each route moves.
usage: verify_bench.py [n] [iters] [seconds] [rate]"""
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import __graft_entry__ as ge  # noqa: E402
import wavutil as W  # noqa: E402

pkg = ge.load_pkg()
lacx, synth = pkg.lacx, pkg.synth
n = int(sys.argv[1]) if len(sys.argv) > 1 else 48
iters = int(sys.argv[2]) if len(sys.argv) > 2 else 5
secs = int(sys.argv[3]) if len(sys.argv) > 3 else 240
sr = int(sys.argv[4]) if len(sys.argv) > 4 else 48000
bd = 16
if lacx.device_count() < 1:
    raise SystemExit("verify_bench needs a HIP device")

t0 = time.perf_counter()
enc = lacx.Encoder(12, 2, sr, bd, device=0)
lacs, host_data, d_i16, d_left, d_right = [], [], [], [], []
with ThreadPoolExecutor(16) as ex:  # numpy releases the GIL inside the generator's arithmetic
    for left, right in ex.map(lambda k: synth.synth_pcm(secs * sr, 2, bd, sr, seed=5000 + k, kind="music"), range(n)):
        lacs.append(enc.encode(left, right))
        data = np.frombuffer(W.pcm_bytes(left, right, bd), dtype=np.uint8)
        host_data.append(data)
        d_i16.append(torch.from_numpy(data.copy()).cuda())
        d_left.append(torch.from_numpy(left).cuda())
        d_right.append(torch.from_numpy(right).cuda())
del left, right
infos = [lacx.stream_parse(x) for x in lacs]
frames = sum(i.frames for i in infos)
out_l = [torch.empty(i.frames, dtype=torch.int32, device="cuda") for i in infos]
out_r = [torch.empty(i.frames, dtype=torch.int32, device="cuda") for i in infos]
sources = [(t.data_ptr(), None, lacx.PCM_INTERLEAVED_I16, 2, i.frames) for t, i in zip(d_i16, infos)]
outputs = [(l.data_ptr(), r.data_ptr()) for l, r in zip(out_l, out_r)]
torch.cuda.synchronize()
print(f"set-up {time.perf_counter() - t0:.0f} s: {n} x {secs} s stereo {bd}/{sr / 1000:g} music, {sum(i.blocks for i in infos)} blocks, "
      f"{sum(map(len, lacs)) / 1e6:.0f} MB .lac, {4 * frames / 1e6:.0f} MB of 16-bit PCM")

dec = lacx.Decoder(device=0)
res = {k: [] for k in ("w_verify", "k_verify", "w_a", "k_a", "w_b", "k_b")}
for it in range(iters + 1):  # the first round is the warm-up
    t1 = time.perf_counter()
    got = dec.verify_batch_device(lacs, sources)
    t2 = time.perf_counter()
    k_v = dec.last_ms
    assert all(r.mismatches == 0 for r in got)
    t3 = time.perf_counter()
    dec.decode_batch_device(lacs, outputs)
    k_a = dec.last_ms
    same = all(torch.equal(a, b) and torch.equal(c, d) for a, b, c, d in zip(out_l, d_left, out_r, d_right))
    torch.cuda.synchronize()
    t4 = time.perf_counter()
    assert same
    t5 = time.perf_counter()
    views = dec.decode_wav_batch_view(lacs)
    k_b = dec.last_ms
    same = all(np.array_equal(v[44:44 + d.size], d) for v, d in zip(views, host_data))
    t6 = time.perf_counter()
    assert same
    if it:
        for k, v in (("w_verify", (t2 - t1) * 1e3), ("k_verify", k_v), ("w_a", (t4 - t3) * 1e3), ("k_a", k_a),
                     ("w_b", (t6 - t5) * 1e3), ("k_b", k_b)):
            res[k].append(v)


def line(key):
    v = res[key]
    return f"{np.min(v):.2f} / {np.median(v):.2f} ms (min..max {np.min(v):.2f}..{np.max(v):.2f})"


print(f"{iters} rounds after warm-up, routes alternating inside a round; best / median (spread); every route says: all identical")
print(f"  verify_batch_device, interleaved int16 sources   wall {line('w_verify')}   kernels {line('k_verify')}")
print(f"  (a) decode_batch_device + torch.equal (planar)   wall {line('w_a')}   decode kernels {line('k_a')}")
print(f"  (b) decode_wav_batch_view + host compare         wall {line('w_b')}   decode kernels {line('k_b')}")
print(f"  post pass bytes: k_verify reads {8 * frames / 1e9:.3f} GB of scratch + {4 * frames / 1e9:.3f} GB of source, stores nothing;"
      f" (a) k_ms_inverse reads and writes {8 * frames / 1e9:.3f} GB where blocks are mid/side, torch.equal reads {16 * frames / 1e9:.3f} GB;"
      f" (b) k_wav_pack reads {8 * frames / 1e9:.3f} GB, writes {4 * frames / 1e9:.3f} GB, and {4 * frames / 1e9:.3f} GB cross PCIe")
