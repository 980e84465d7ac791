"""Measurement (not part of the default suite): what a source layout costs the device-resident shard encode.
Workload: 10 minutes of stereo music at 16/48 and at 24/96, resident on the device in every layout the encoder takes.
After a warm-up round, `iters` rounds, the layouts alternating inside every round (a slow phase of the machine then hits
all of them alike); per layout the wall ms of Encoder.encode_shard_pcm_device_view (the call ends synchronised, the
payload in pinned host memory) and lacx_timing's analysis_ms:
  planar int32                the baseline: the reference's API boundary
  interleaved int16 / int24   the WAV data chunk
  planar int16, planar float32, interleaved float32     through the import pass (import_core.h)
  torch, then planar int32    what a float tensor cost before: torch ops that make two int32 tensors of it (scale, check
                              that nothing was rounded, convert), then the planar int32 encode
Every layout's payload is compared with the baseline's once, in the warm-up round.
Printed: best / median / min..max per layout, and the baseline's spread, against which the others are to be read.
usage: layout_bench.py [iters] [seconds] [library]   (library: another build's liblacx.so, for the baseline lines of a
tree without the tensor layouts)"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import __graft_entry__ as ge  # noqa: E402
import wavutil as W  # noqa: E402

pkg = ge.load_pkg()
lacx, synth = pkg.lacx, pkg.synth
iters = int(sys.argv[1]) if len(sys.argv) > 1 else 15
secs = int(sys.argv[2]) if len(sys.argv) > 2 else 600
if lacx.device_count() < 1:
    raise SystemExit("layout_bench needs a HIP device")
new_layouts = len(sys.argv) <= 3
if not new_layouts:
    lacx.use_library(sys.argv[3])

for bd, sr in ((16, 48000), (24, 96000)):
    left, right = synth.synth_pcm(secs * sr, 2, bd, sr, seed=4242, kind="music")
    n = left.size
    enc = lacx.Encoder(12, 2, sr, bd, device=0)
    planar = torch.from_numpy(np.stack([left, right])).cuda()                       # [2, T] int32
    chunk = torch.from_numpy(np.frombuffer(W.pcm_bytes(left, right, bd), dtype=np.uint8).copy()).cuda()
    f32 = (planar.to(torch.float32) * float(2.0 ** -(bd - 1))).contiguous()         # [2, T], what the window decode writes
    f32_t = f32.t().contiguous()                                                    # [T, 2]
    routes = {"planar int32": lambda: enc.encode_shard_device_view(planar[0].data_ptr(), planar[1].data_ptr(), left, right, n),
              f"interleaved int{bd}": lambda: enc.encode_shard_pcm_device_view(
                  chunk.data_ptr(), lacx.PCM_INTERLEAVED_I16 if bd == 16 else lacx.PCM_INTERLEAVED_I24, 2, n)}
    if new_layouts:
        if bd == 16:
            i16 = planar.to(torch.int16)
            routes["planar int16"] = lambda: enc.encode_shard_pcm_device_view(i16)
        routes["planar float32"] = lambda: enc.encode_shard_pcm_device_view(f32)
        routes["interleaved float32"] = lambda: enc.encode_shard_pcm_device_view(f32_t)

    def via_torch():
        scaled = f32 * float(2.0 ** (bd - 1))
        ints = scaled.to(torch.int32)
        lim = 1 << (bd - 1)
        if not bool(((ints.to(torch.float32) == scaled) & (ints >= -lim) & (ints < lim)).all()):
            raise ValueError("not an exact sample")
        return enc.encode_shard_device_view(ints[0].data_ptr(), ints[1].data_ptr(), left, right, n)
    routes["torch, then planar int32"] = via_torch

    wall = {k: [] for k in routes}
    kern = {k: [] for k in routes}
    want = None
    for it in range(iters + 1):  # the first round is the warm-up
        for name, call in routes.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            pay, _ = call()
            t1 = time.perf_counter()
            if it == 0:
                got = pay.tobytes()
                want = got if want is None else want
                assert got == want, name
            else:
                wall[name].append((t1 - t0) * 1e3)
                kern[name].append(enc.timing().analysis_ms)
    print(f"{secs} s stereo {bd}/{sr / 1000:g} music, {n} frames, {len(want) / 1e6:.1f} MB payload; {iters} rounds after warm-up, "
          f"layouts alternating inside a round; wall best / median (min..max) ms, analysis_ms median")
    for name in routes:
        w, k = wall[name], kern[name]
        print(f"  {name:28s} {np.min(w):7.3f} / {np.median(w):7.3f} ({np.min(w):.3f}..{np.max(w):.3f})   analysis {np.median(k):.3f}")
    base = wall["planar int32"]
    print(f"  baseline spread: {np.max(base) - np.min(base):.3f} ms over {iters} rounds ({100 * (np.max(base) - np.min(base)) / np.median(base):.1f} % of the median)")
    enc.close()
    del planar, chunk, f32, f32_t
    torch.cuda.empty_cache()
