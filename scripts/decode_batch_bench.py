"""Measurement (not part of the default suite): many .lac streams as one device decode against one call per stream.
Workload: `n` synthetic 4-minute stereo 16/44.1 music streams (distinct seeds; 48 streams = 31 008 blocks), encoded on the
GPU.  After a warm-up, best / median of `iters` rounds of:
  kernel ms (events) of Decoder.decode_wav_batch_view over all streams, of the same with every stream's lanes padded to
    a wave boundary (LACX_DECODE_BATCH_PAD=1), and of Decoder.decode_wav_view of the first stream alone;
  wall ms of decode_wav_batch_view against n sequential decode_wav_view calls on a warmed handle.
Every image's sha256 is checked against the canonical WAV of its input PCM.  k_wav_pack's bytes are printed for
the profile (rocprofv3 --kernel-trace --stats, in a run of its own, gives its time).
usage: decode_batch_bench.py [n] [iters] [seconds]"""
import hashlib
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import __graft_entry__ as ge  # noqa: E402
import wavutil as W  # noqa: E402

pkg = ge.load_pkg()
lacx, synth = pkg.lacx, pkg.synth
n = int(sys.argv[1]) if len(sys.argv) > 1 else 48
iters = int(sys.argv[2]) if len(sys.argv) > 2 else 5
secs = int(sys.argv[3]) if len(sys.argv) > 3 else 240
sr, bd = 44100, 16
if lacx.device_count() < 1:
    raise SystemExit("decode_batch_bench needs a HIP device")

t0 = time.perf_counter()
enc = lacx.Encoder(12, 2, sr, bd, device=0)
lacs, want = [], []
with ThreadPoolExecutor(16) as ex:  # numpy releases the GIL inside the generator's arithmetic
    for left, right in ex.map(lambda k: synth.synth_pcm(secs * sr, 2, bd, sr, seed=5000 + k, kind="music"), range(n)):
        lacs.append(enc.encode(left, right))
        want.append(hashlib.sha256(W.make_wav(left, right, sr, bd)).hexdigest())
del left, right
infos = [lacx.stream_parse(x) for x in lacs]
blocks = sum(i.blocks for i in infos)
frames = sum(i.frames for i in infos)
print(f"set-up {time.perf_counter() - t0:.0f} s: {n} x {secs} s stereo {bd}/{sr / 1000:g} music, {blocks} blocks, "
      f"{sum(map(len, lacs)) / 1e6:.0f} MB .lac, {(44 * n + 4 * frames) / 1e6:.0f} MB WAV")

batch = lacx.Decoder(device=0)
single = lacx.Decoder(device=0)
res = {k: [] for k in ("k_batch", "k_batch_pad", "k_one", "w_batch", "w_seq")}
for it in range(iters + 1):  # the first round is the warm-up
    t1 = time.perf_counter()
    views = batch.decode_wav_batch_view(lacs)
    t2 = time.perf_counter()
    if it == 0:
        assert [hashlib.sha256(v).hexdigest() for v in views] == want
    k_batch = batch.last_ms
    os.environ["LACX_DECODE_BATCH_PAD"] = "1"
    views = batch.decode_wav_batch_view(lacs)
    del os.environ["LACX_DECODE_BATCH_PAD"]
    if it == 0:
        assert [hashlib.sha256(v).hexdigest() for v in views] == want
    k_pad = batch.last_ms
    t3 = time.perf_counter()
    for i, lac in enumerate(lacs):
        v = single.decode_wav_view(lac)
        if i == 0:
            k_one = single.last_ms
        if it == 0:
            assert hashlib.sha256(v).hexdigest() == want[i]
    t4 = time.perf_counter()
    if it:
        res["k_batch"].append(k_batch)
        res["k_batch_pad"].append(k_pad)
        res["k_one"].append(k_one)
        res["w_batch"].append((t2 - t1) * 1e3)
        res["w_seq"].append((t4 - t3) * 1e3)

best = {k: float(np.min(v)) for k, v in res.items()}
med = {k: float(np.median(v)) for k, v in res.items()}
pack_read = 4 * 2 * frames  # int32 left + right
pack_write = 4 * frames     # 16-bit stereo data regions
print(f"{iters} rounds after warm-up, best / median; every image equals the canonical WAV of its input")
print(f"  kernels  batch {best['k_batch']:.2f} / {med['k_batch']:.2f} ms   batch, items padded to waves "
      f"{best['k_batch_pad']:.2f} / {med['k_batch_pad']:.2f} ms   one stream alone {best['k_one']:.2f} / {med['k_one']:.2f} ms"
      f"   ratio {med['k_batch'] / med['k_one']:.2f}")
print(f"  wall     decode_wav_batch_view {best['w_batch']:.1f} / {med['w_batch']:.1f} ms   {n} x decode_wav_view "
      f"{best['w_seq']:.1f} / {med['w_seq']:.1f} ms   speed-up {med['w_seq'] / med['w_batch']:.1f}x")
print(f"  k_wav_pack moves {pack_read / 1e9:.3f} GB read + {pack_write / 1e9:.3f} GB written "
      f"(at 8 TB/s: {(pack_read + pack_write) / 8e12 * 1e3:.3f} ms)")
