"""Measurement (not part of the default suite): what loudness costs against the statistics and against what a user has
without it.
  loudness  Decoder.loudness_batch: decode, the in-place mid/side inverse, k_loud_states, k_loud_carry, k_loud_energy and
            k_loud_rows; 16 bytes per tenth of a second come back
  stats     Decoder.stats_batch: a neighbouring job over the same PCM (k_stats_blocks)
  host      the status quo: Decoder.decode_batch_device into torch tensors, the PCM to the host, scipy.signal.lfilter with the
            K-weighting biquads over every channel, numpy sums (one round: it takes seconds)
Workloads: one 10-minute stereo 16/48 stream, and the 48-song batch of profiles/decode_batch_bench.txt (48 x 240 s stereo
16/44.1 synthetic music, distinct seeds), all encoded on the GPU.  Per workload a warm-up round, then `iters` rounds with
the two device routes alternating inside every round: wall ms of each (all end synchronised) and the kernel ms the library
reports.  The loudness route's rows are checked against the host route's within tests/loudtwin.py's ROW_TOL.
Without a HIP device nothing is measured, and the script says so.
usage: loudness_bench.py [iters] [songs] [song seconds]"""
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
import loudtwin as lt  # noqa: E402

pkg = ge.load_pkg()
lacx, synth = pkg.lacx, pkg.synth
iters = int(sys.argv[1]) if len(sys.argv) > 1 else 5
songs = int(sys.argv[2]) if len(sys.argv) > 2 else 48
song_secs = int(sys.argv[3]) if len(sys.argv) > 3 else 240
if lacx.device_count() < 1:
    raise SystemExit("not measured yet: loudness_bench needs a HIP device")


def host_route(dec, lacs, outs, rate):
    """decode_batch_device, the PCM to the host, lfilter and sums: per item its rows."""
    dec.decode_batch_device(lacs, [(o[0].data_ptr(), o[1].data_ptr()) for o in outs])
    pcm = [o.cpu().numpy() for o in outs]  # (the copies synchronise)
    with ThreadPoolExecutor(16) as ex:  # lfilter releases the GIL
        return list(ex.map(lambda x: lt.expected_rows(x[0], x[1], rate), pcm))


def workload(name, n, secs, rate, seed0):
    t0 = time.perf_counter()
    enc = lacx.Encoder(12, 2, rate, 16, device=0)
    lacs = []
    with ThreadPoolExecutor(16) as ex:  # numpy releases the GIL inside the generator's arithmetic
        for left, right in ex.map(lambda k: synth.synth_pcm(secs * rate, 2, 16, rate, seed=seed0 + k, kind="music"), range(n)):
            lacs.append(enc.encode(left, right))
    infos = [lacx.stream_parse(x) for x in lacs]
    blocks, frames = sum(i.blocks for i in infos), sum(i.frames for i in infos)
    print(f"{name}: {n} x {secs} s stereo 16/{rate / 1000:g} music, {sum(map(len, lacs)) / 1e6:.0f} MB .lac, {blocks} blocks "
          f"(set-up {time.perf_counter() - t0:.0f} s)")
    dec = lacx.Decoder(device=0)
    outs = [torch.empty((2, i.frames), dtype=torch.int32, device="cuda") for i in infos]
    res = {k: [] for k in ("w_loud", "k_loud", "w_stats", "k_stats")}
    loud = None
    for it in range(iters + 1):  # the first round is the warm-up
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        loud = dec.loudness_batch(lacs)
        t2 = time.perf_counter()
        k_l = dec.last_ms
        dec.stats_batch(lacs)
        t3 = time.perf_counter()
        k_s = dec.last_ms
        if it:
            for k, v in (("w_loud", (t2 - t1) * 1e3), ("k_loud", k_l), ("w_stats", (t3 - t2) * 1e3), ("k_stats", k_s)):
                res[k].append(v)
    torch.cuda.synchronize()
    t4 = time.perf_counter()
    ref = host_route(dec, lacs, outs, rate)
    w_host = (time.perf_counter() - t4) * 1e3
    worst = max(lt.row_error(lt.rows_of(rows), want) for (_, rows), want in zip(loud, ref))
    dec.close()

    def line(key):
        v = res[key]
        return f"{np.median(v):.2f} ms (min..max {np.min(v):.2f}..{np.max(v):.2f})"

    chunks = sum((i.frames + 255) // 256 for i in infos)
    print(f"  {iters} rounds after warm-up, routes alternating inside a round; medians; rows within {worst:.1e} of the host route's (ROW_TOL {lt.ROW_TOL:.1e})")
    print(f"  loudness_batch        wall {line('w_loud')}   kernels (decode + k_ms_inverse + the four loudness kernels) {line('k_loud')}")
    print(f"  stats_batch           wall {line('w_stats')}   kernels (decode + k_ms_inverse + k_stats_blocks) {line('k_stats')}")
    print(f"  decode + lfilter      wall {w_host:.0f} ms (one round, 16 host threads)")
    print(f"  loudness over stats: {np.median(res['k_loud']) - np.median(res['k_stats']):+.3f} ms of kernels, "
          f"{np.median(res['w_loud']) - np.median(res['w_stats']):+.2f} ms of wall; {16 * sum(len(r) for _, r in loud)} B of rows cross PCIe; "
          f"scratch {96 * chunks / 1e6:.0f} MB; the PCM, read twice, is {8 * frames / 1e6:.0f} MB")
    print("  integrated LUFS of the first items:", " ".join("%.2f" % l.integrated_lufs for l, _ in loud[:4]))
    assert worst <= lt.ROW_TOL, "the loudness route and the host route differ: %g" % worst


workload("one stream", 1, 600, 48000, 7000)
if songs:  # (0: the single stream only, for a profiler run)
    workload("batch", songs, song_secs, 44100, 5000)
