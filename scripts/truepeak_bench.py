"""Measurement (not part of the default suite): what the true peak costs against the statistics and against what a user has
without it.
  truepeak  Decoder.truepeak_batch: decode, the in-place mid/side inverse and k_truepeak; 32 bytes per 16384 frames come back
  stats     Decoder.stats_batch: a neighbouring job over the same PCM (k_stats_blocks)
  torch     the status quo on the device: Decoder.decode_batch_device into torch tensors, then per item a float64 conv1d
            with the same integer taps (four output channels, one per phase; float64 holds these integers exactly) and amax
  alone     Decoder.truepeak_pcm_batch over the decoded tensors: k_truepeak alone, no decode in front
Workloads: the 48-song batch of profiles/decode_batch_bench.txt at 16 bit (48 x 240 s stereo 16/44.1 synthetic music, distinct
seeds) and a quarter of it at 24 bit (12 songs: the split arithmetic of depth 24), all encoded on the GPU.  Per workload a
warm-up round, then `iters` rounds with the routes alternating inside every round: wall ms of each (all end synchronised)
and the kernel ms the library reports.  The peaks of the three routes are checked to be the same integers.
Without a HIP device nothing is measured, and the script says so.
usage: truepeak_bench.py [iters] [songs] [song seconds]"""
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
import peaktwin as pt  # noqa: E402

pkg = ge.load_pkg()
lacx, synth = pkg.lacx, pkg.synth
iters = int(sys.argv[1]) if len(sys.argv) > 1 else 5
songs = int(sys.argv[2]) if len(sys.argv) > 2 else 48
song_secs = int(sys.argv[3]) if len(sys.argv) > 3 else 240
if lacx.device_count() < 1:
    raise SystemExit("not measured yet: truepeak_bench needs a HIP device")


def torch_route(dec, lacs, outs, weight):
    """decode_batch_device, then conv1d in float64 and amax per item and channel: the integer peaks."""
    dec.decode_batch_device(lacs, [(o[0].data_ptr(), o[1].data_ptr()) for o in outs])
    global conv_how
    peaks = []
    for o in outs:
        x = o.to(torch.float64)
        if conv_how != "shifted multiply-adds":
            try:
                y = torch.nn.functional.conv1d(x.unsqueeze(1), weight, padding=pt.FLUSH)  # (2, 4, frames + 11)
                conv_how = "conv1d"
            except RuntimeError as e:  # a build whose convolution library has no float64: say so, and restate the sum
                print("  torch conv1d in float64 is not available here (%s); the torch route uses shifted multiply-adds" % str(e).splitlines()[0])
                conv_how = "shifted multiply-adds"
        if conv_how == "shifted multiply-adds":
            xp = torch.nn.functional.pad(x, (pt.FLUSH, pt.FLUSH))
            n = x.shape[1] + pt.FLUSH
            y = torch.stack([sum(weight[p, 0, k] * xp[:, k:k + n] for k in range(pt.TAPS)) for p in range(4)], dim=1)
        peaks.append(y.abs().amax(dim=(1, 2)))
    return torch.stack(peaks).cpu().numpy()  # (the copy synchronises)


conv_how = None


def workload(name, n, secs, rate, depth, seed0):
    t0 = time.perf_counter()
    enc = lacx.Encoder(12, 2, rate, depth, device=0)
    lacs = []
    with ThreadPoolExecutor(16) as ex:  # numpy releases the GIL inside the generator's arithmetic
        for left, right in ex.map(lambda k: synth.synth_pcm(secs * rate, 2, depth, rate, seed=seed0 + k, kind="music"), range(n)):
            lacs.append(enc.encode(left, right))
    infos = [lacx.stream_parse(x) for x in lacs]
    blocks, frames = sum(i.blocks for i in infos), sum(i.frames for i in infos)
    print(f"{name}: {n} x {secs} s stereo {depth}/{rate / 1000:g} music, {sum(map(len, lacs)) / 1e6:.0f} MB .lac, {blocks} blocks "
          f"(set-up {time.perf_counter() - t0:.0f} s)")
    dec = lacx.Decoder(device=0)
    outs = [torch.empty((2, i.frames), dtype=torch.int32, device="cuda") for i in infos]
    weight = torch.from_numpy(np.ascontiguousarray(pt.TABLE[:, ::-1]).astype(np.float64)).reshape(4, 1, 12).cuda()  # conv1d correlates
    res = {k: [] for k in ("w_peak", "k_peak", "w_stats", "k_stats", "w_torch", "w_alone", "k_alone")}
    peak = ref = alone = None
    for it in range(iters + 1):  # the first round is the warm-up
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        peak = dec.truepeak_batch(lacs)
        t2 = time.perf_counter()
        k_p = dec.last_ms
        dec.stats_batch(lacs)
        t3 = time.perf_counter()
        k_s = dec.last_ms
        ref = torch_route(dec, lacs, outs, weight)
        t4 = time.perf_counter()
        alone = dec.truepeak_pcm_batch([(o, rate, depth) for o in outs])
        t5 = time.perf_counter()
        k_a = dec.last_ms
        if it:
            for k, v in (("w_peak", (t2 - t1) * 1e3), ("k_peak", k_p), ("w_stats", (t3 - t2) * 1e3), ("k_stats", k_s), ("w_torch", (t4 - t3) * 1e3),
                         ("w_alone", (t5 - t4) * 1e3), ("k_alone", k_a)):
                res[k].append(v)
    dec.close()
    for (p, _), (a, _), want in zip(peak, alone, ref):
        got = [int(p.ch[0].peak), int(p.ch[1].peak)]
        assert got == [int(a.ch[0].peak), int(a.ch[1].peak)] == [int(want[0]), int(want[1])], "the routes differ: %r %r" % (got, want)

    def line(key):
        v = res[key]
        return f"{np.median(v):.2f} ms (min..max {np.min(v):.2f}..{np.max(v):.2f})"

    pcm = 8 * frames
    print(f"  {iters} rounds after warm-up, routes alternating inside a round; medians; the three routes give the same integer peaks")
    print(f"  truepeak_batch        wall {line('w_peak')}   kernels (decode + k_ms_inverse + k_truepeak) {line('k_peak')}")
    print(f"  stats_batch           wall {line('w_stats')}   kernels (decode + k_ms_inverse + k_stats_blocks) {line('k_stats')}")
    print(f"  decode + torch        wall {line('w_torch')}   ({conv_how} in float64, four phases, amax)")
    print(f"  truepeak_pcm_batch    wall {line('w_alone')}   k_truepeak alone {line('k_alone')} for {pcm / 1e9:.2f} GB of PCM: "
          f"{pcm / 1e6 / np.median(res['k_alone']):.0f} GB/s, {48 * 2 * frames / 1e6 / np.median(res['k_alone']):.0f} G taps/s")
    print(f"  truepeak over stats: {np.median(res['k_peak']) - np.median(res['k_stats']):+.3f} ms of kernels, "
          f"{np.median(res['w_peak']) - np.median(res['w_stats']):+.2f} ms of wall; {32 * sum(len(r) for _, r in peak)} B of rows cross PCIe")
    print("  dBTP / sample peak dBFS of the first items:", " ".join("%.2f/%.2f" % (p.true_peak_dbtp, p.sample_peak_dbfs) for p, _ in peak[:4]))


workload("batch, 16 bit", songs, song_secs, 44100, 16, 5000)
if songs >= 4:
    workload("quarter batch, 24 bit", songs // 4, song_secs, 44100, 24, 6000)
