"""Measurement (not part of the default suite): what finding runs costs against the statistics and against what a user has
without it.
  runs    Decoder.runs_batch: decode, the in-place mid/side inverse, k_runs with three detectors -- QUIET at -60 dBFS for 0.1 s
          over all channels, PEAK at full scale for 3 frames in each channel; the runs and 4 bytes per tile and detector
          come back
  stats   Decoder.stats_batch: the same job with the neighbouring kernel (k_stats_blocks)
  torch   the status quo: Decoder.decode_batch_device into torch tensors, then per detector a comparison over the tensors
          and the run lengths from the mask's differences (nonzero of a diff as large as the audio), the runs read back
Workloads: one 10-minute stereo 16/48 stream, and the 48-song batch of profiles/decode_batch_bench.txt (48 x 240 s stereo
16/44.1 synthetic music, distinct seeds), all encoded on the GPU; a second of digital silence and a few clipped stretches
are written into every song so that every detector finds something.  Per workload a warm-up round, then `iters` rounds with
the three routes alternating inside every round: wall ms of each (all end synchronised) and the kernel ms the library
reports.  Every list of the runs route is checked against the torch route.
k_runs alone comes from a kernel trace of this script in a run of its own.
usage: runs_bench.py [iters] [songs] [song seconds]"""
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

pkg = ge.load_pkg()
lacx, synth = pkg.lacx, pkg.synth
iters = int(sys.argv[1]) if len(sys.argv) > 1 else 5
songs = int(sys.argv[2]) if len(sys.argv) > 2 else 48
song_secs = int(sys.argv[3]) if len(sys.argv) > 3 else 240
if lacx.device_count() < 1:
    raise SystemExit("runs_bench needs a HIP device")
DETECTORS = [lacx.quiet(dbfs=-60, seconds=0.1), lacx.peak(min_frames=3, channel="left"), lacx.peak(min_frames=3, channel="right")]


def runs_of(mask, min_frames):
    """[k, 2] (start, frames) of the stretches of True that reach min_frames, on the device."""
    edge = torch.diff(torch.nn.functional.pad(mask.to(torch.int8), (1, 1)))
    starts, ends = torch.nonzero(edge == 1).flatten(), torch.nonzero(edge == -1).flatten()
    keep = ends - starts >= min_frames
    return torch.stack([starts[keep], (ends - starts)[keep]], dim=1)


def torch_route(dec, lacs, outs, dets):
    """decode_batch_device, then what a user writes today; -> per item, per detector, the runs."""
    dec.decode_batch_device(lacs, [(o[0].data_ptr(), o[1].data_ptr()) for o in outs])
    res = []
    for o in outs:
        q, pl, pr = dets
        quiet = ((o >= -int(q.level)) & (o <= int(q.level))).all(dim=0)
        left = (o[0] >= int(pl.level)) | (o[0] <= -int(pl.level) - 1)
        right = (o[1] >= int(pr.level)) | (o[1] <= -int(pr.level) - 1)
        res.append([runs_of(quiet, int(q.min_frames)), runs_of(left, int(pl.min_frames)), runs_of(right, int(pr.min_frames))])
    return [[r.cpu().numpy() for r in item] for item in res]  # (the copies synchronise)


def workload(name, n, secs, rate, seed0):
    t0 = time.perf_counter()
    enc = lacx.Encoder(12, 2, rate, 16, device=0)
    lacs = []

    def song(k):
        left, right = synth.synth_pcm(secs * rate, 2, 16, rate, seed=seed0 + k, kind="music")
        left[5 * rate:6 * rate] = 0
        right[5 * rate:6 * rate] = 0
        for at in range(20 * rate, secs * rate - rate, 30 * rate):  # clipped stretches of 3 to 40 frames
            left[at:at + 3 + at % 38] = 32767
            right[at + 100:at + 103 + at % 38] = -32768
        return left, right
    with ThreadPoolExecutor(16) as ex:  # numpy releases the GIL inside the generator's arithmetic
        for left, right in ex.map(song, range(n)):
            lacs.append(enc.encode(left, right))
    infos = [lacx.stream_parse(x) for x in lacs]
    blocks, frames = sum(i.blocks for i in infos), sum(i.frames for i in infos)
    print(f"{name}: {n} x {secs} s stereo 16/{rate / 1000:g} music, {sum(map(len, lacs)) / 1e6:.0f} MB .lac, {blocks} blocks "
          f"(set-up {time.perf_counter() - t0:.0f} s)")
    dets = [d.resolve(16, rate) for d in DETECTORS]
    dec = lacx.Decoder(device=0)
    outs = [torch.empty((2, i.frames), dtype=torch.int32, device="cuda") for i in infos]
    res = {k: [] for k in ("w_runs", "k_runs", "w_stats", "k_stats", "w_torch", "k_torch")}
    found = rerun = 0
    for it in range(iters + 1):  # the first round is the warm-up
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        runs = dec.runs_batch(lacs, dets)
        t2 = time.perf_counter()
        k_r = dec.last_ms
        dec.stats_batch(lacs)
        t3 = time.perf_counter()
        k_s = dec.last_ms
        ref = torch_route(dec, lacs, outs, dets)
        t4 = time.perf_counter()
        k_t = dec.last_ms
        for (r, lists), want in zip(runs, ref):
            for l, w in zip(lists, want):
                assert np.array_equal(l.runs.astype(np.int64), w), "the runs route and the torch route differ"
        found = sum(int(r.det[k].runs) for r, _ in runs for k in range(3))
        rerun = sum(1 for r, _ in runs if r.rerun)
        if it:
            for k, v in (("w_runs", (t2 - t1) * 1e3), ("k_runs", k_r), ("w_stats", (t3 - t2) * 1e3), ("k_stats", k_s),
                         ("w_torch", (t4 - t3) * 1e3), ("k_torch", k_t)):
                res[k].append(v)
    dec.close()

    def line(key):
        v = res[key]
        return f"{np.median(v):.2f} ms (min..max {np.min(v):.2f}..{np.max(v):.2f})"

    tiles = sum((i.frames + 1023) // 1024 for i in infos)
    print(f"  {iters} rounds after warm-up, routes alternating inside a round; medians; {found} runs, equal to the torch route's; items rerun: {rerun}")
    print(f"  runs_batch            wall {line('w_runs')}   kernels (decode + k_ms_inverse + k_runs, first pass) {line('k_runs')}")
    print(f"  stats_batch           wall {line('w_stats')}   kernels (decode + k_ms_inverse + k_stats_blocks) {line('k_stats')}")
    print(f"  decode + torch        wall {line('w_torch')}   kernels (decode alone; the comparisons and run lengths are torch's) {line('k_torch')}")
    print(f"  runs over stats: {np.median(res['k_runs']) - np.median(res['k_stats']):+.3f} ms of kernels, "
          f"{np.median(res['w_runs']) - np.median(res['w_stats']):+.2f} ms of wall; runs against decode + torch: "
          f"{np.median(res['w_runs']) - np.median(res['w_torch']):+.2f} ms of wall; {4 * 3 * tiles} B of rows cross PCIe; the PCM read once is "
          f"{8 * frames / 1e6:.0f} MB")


workload("one stream", 1, 600, 48000, 7000)
if songs:  # (0: the single stream only, for a profiler run)
    workload("batch", songs, song_secs, 44100, 5000)
