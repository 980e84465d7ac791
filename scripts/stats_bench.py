"""Measurement (not part of the default suite): what the audio statistics cost against the block digests and against what a
user has without them.
  digest_blocks  Decoder.digest_blocks_batch: decode, the in-place mid/side inverse, one CRC-32 per block (k_digest_blocks)
  stats          Decoder.stats_batch: the same job with k_stats_blocks as its last kernel; about 100 bytes per block come back
  torch          the status quo: Decoder.decode_batch_device into torch tensors, then amin / amax / sum / sum of squares /
                 count_nonzero per channel over them (int64 temporaries as large as the audio), the results read back
Workloads: one 10-minute stereo 16/48 stream, and the 48-song batch of profiles/decode_batch_bench.txt (48 x 240 s stereo
16/44.1 synthetic music, distinct seeds), all encoded on the GPU.  Per workload a warm-up round, then `iters` rounds with
the three routes alternating inside every round: wall ms of each (all end synchronised) and the kernel ms the library
reports.  Every total is checked against the torch route and one stream's first row against numpy.
k_stats_blocks reads the PCM once: 8 bytes per stereo frame.  The last line states that read against the kernel time the
stats route has over the device-form decode -- an upper bound for k_stats_blocks alone, which this script does not
separate from what else differs between the two jobs (a profiler run does).
usage: stats_bench.py [iters] [songs] [song seconds]"""
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
    raise SystemExit("stats_bench needs a HIP device")


def torch_route(dec, lacs, outs):
    """decode_batch_device, then the reductions a user writes today; -> per item (min, max, sum, sum_sq, zeros) per channel."""
    dec.decode_batch_device(lacs, [(o[0].data_ptr(), o[1].data_ptr()) for o in outs])
    res = []
    for o in outs:
        wide = o.to(torch.int64)
        res.append(torch.stack([o.amin(dim=1).to(torch.int64), o.amax(dim=1).to(torch.int64), wide.sum(dim=1), (wide * wide).sum(dim=1),
                                o.shape[1] - torch.count_nonzero(o, dim=1)]))
    return torch.stack(res).cpu().numpy()  # (the copy synchronises)


def workload(name, n, secs, rate, seed0):
    t0 = time.perf_counter()
    enc = lacx.Encoder(12, 2, rate, 16, device=0)
    lacs, first = [], None
    with ThreadPoolExecutor(16) as ex:  # numpy releases the GIL inside the generator's arithmetic
        for left, right in ex.map(lambda k: synth.synth_pcm(secs * rate, 2, 16, rate, seed=seed0 + k, kind="music"), range(n)):
            lacs.append(enc.encode(left, right))
            if first is None:
                first = (left, right)
    infos = [lacx.stream_parse(x) for x in lacs]
    blocks, frames = sum(i.blocks for i in infos), sum(i.frames for i in infos)
    print(f"{name}: {n} x {secs} s stereo 16/{rate / 1000:g} music, {sum(map(len, lacs)) / 1e6:.0f} MB .lac, {blocks} blocks "
          f"(set-up {time.perf_counter() - t0:.0f} s)")
    dec = lacx.Decoder(device=0)
    outs = [torch.empty((2, i.frames), dtype=torch.int32, device="cuda") for i in infos]
    res = {k: [] for k in ("w_blocks", "k_blocks", "w_stats", "k_stats", "w_torch", "k_torch")}
    for it in range(iters + 1):  # the first round is the warm-up
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        dec.digest_blocks_batch(lacs)
        t2 = time.perf_counter()
        k_b = dec.last_ms
        stats = dec.stats_batch(lacs)
        t3 = time.perf_counter()
        k_s = dec.last_ms
        ref = torch_route(dec, lacs, outs)
        t4 = time.perf_counter()
        k_t = dec.last_ms
        for (s, rows), r in zip(stats, ref):
            for c in (0, 1):
                assert (s.ch[c].min, s.ch[c].max, s.ch[c].sum, s.ch[c].sum_sq, s.ch[c].zeros) == tuple(int(v) for v in r[:, c])
        if it == 0:
            row, n0 = stats[0][1][0], stats[0][1][0].frames
            assert row.ch[0].sum == int(first[0][:n0].astype(np.int64).sum()) and row.differing == int(np.count_nonzero(first[0][:n0] != first[1][:n0]))
        else:
            for k, v in (("w_blocks", (t2 - t1) * 1e3), ("k_blocks", k_b), ("w_stats", (t3 - t2) * 1e3), ("k_stats", k_s),
                         ("w_torch", (t4 - t3) * 1e3), ("k_torch", k_t)):
                res[k].append(v)
    dec.close()

    def line(key):
        v = res[key]
        return f"{np.median(v):.2f} ms (min..max {np.min(v):.2f}..{np.max(v):.2f})"

    print(f"  {iters} rounds after warm-up, routes alternating inside a round; medians; the totals equal the torch route's")
    print(f"  digest_blocks_batch   wall {line('w_blocks')}   kernels (decode + k_ms_inverse + k_digest_blocks) {line('k_blocks')}")
    print(f"  stats_batch           wall {line('w_stats')}   kernels (decode + k_ms_inverse + k_stats_blocks) {line('k_stats')}")
    print(f"  decode + torch        wall {line('w_torch')}   kernels (decode alone; the reductions are torch's) {line('k_torch')}")
    extra = np.median(res["k_stats"]) - np.median(res["k_torch"])
    print(f"  stats over digest_blocks: {np.median(res['k_stats']) - np.median(res['k_blocks']):+.3f} ms of kernels, "
          f"{np.median(res['w_stats']) - np.median(res['w_blocks']):+.2f} ms of wall; stats against decode + torch: "
          f"{np.median(res['w_stats']) - np.median(res['w_torch']):+.2f} ms of wall; {104 * blocks} B of rows cross PCIe")
    print(f"  the PCM read once is {8 * frames / 1e6:.0f} MB; stats kernels less the device-form decode's are {extra:.3f} ms "
          f"(k_stats_blocks and whatever else differs): {8 * frames / 1e6 / max(extra, 1e-9):.0f} GB/s of PCM over that time")


workload("one stream", 1, 600, 48000, 7000)
if songs:  # (0: the single stream only, for a profiler run)
    workload("batch", songs, song_secs, 44100, 5000)
