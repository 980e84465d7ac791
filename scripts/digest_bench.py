"""Measurement (not part of the default suite): "what does this .lac decode to?" as four bytes, two ways.
  digest    Decoder.digest_batch: decode and CRC-32 on the device, 8 bytes per item come back
  (old)     Decoder.decode_wav_batch_view, then zlib.crc32 of every WAV image on the host: the path the digest replaces
Workloads: one 10-minute stereo 16/48 stream, and the 48-song batch of profiles/decode_batch_bench.txt (48 x 240 s stereo
16/44.1 synthetic music, distinct seeds), all encoded on the GPU.  Per workload a warm-up round, then `iters` rounds with
the two routes alternating inside every round: wall ms of each (both end synchronised), the kernel ms the library reports
(decode kernels + the post pass: k_digest or k_wav_pack), and the source form (Decoder.digest_pcm_batch over the same PCM
resident on the device as interleaved int16: k_digest alone).  Every digest is checked against zlib.
usage: digest_bench.py [iters] [songs] [song seconds]"""
import os
import sys
import time
import zlib
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
iters = int(sys.argv[1]) if len(sys.argv) > 1 else 5
songs = int(sys.argv[2]) if len(sys.argv) > 2 else 48
song_secs = int(sys.argv[3]) if len(sys.argv) > 3 else 240
if lacx.device_count() < 1:
    raise SystemExit("digest_bench needs a HIP device")


def workload(name, n, secs, rate, seed0):
    t0 = time.perf_counter()
    enc = lacx.Encoder(12, 2, rate, 16, device=0)
    lacs, d_pcm = [], []
    with ThreadPoolExecutor(16) as ex:  # numpy releases the GIL inside the generator's arithmetic
        for left, right in ex.map(lambda k: synth.synth_pcm(secs * rate, 2, 16, rate, seed=seed0 + k, kind="music"), range(n)):
            lacs.append(enc.encode(left, right))
            d_pcm.append(torch.from_numpy(np.frombuffer(W.pcm_bytes(left, right, 16), dtype=np.int16).reshape(-1, 2).copy()).cuda())
    frames = sum(t.shape[0] for t in d_pcm)
    print(f"{name}: {n} x {secs} s stereo 16/{rate / 1000:g} music, {sum(map(len, lacs)) / 1e6:.0f} MB .lac, {4 * frames / 1e6:.0f} MB of WAV "
          f"(set-up {time.perf_counter() - t0:.0f} s)")
    dec = lacx.Decoder(device=0)
    res = {k: [] for k in ("w_digest", "k_digest", "w_old", "w_old_decode", "k_old", "w_src", "k_src")}
    sources = [(t, rate, 16) for t in d_pcm]
    for it in range(iters + 1):  # the first round is the warm-up
        t1 = time.perf_counter()
        got = dec.digest_batch(lacs)
        t2 = time.perf_counter()
        k_d = dec.last_ms
        views = dec.decode_wav_batch_view(lacs)
        t3 = time.perf_counter()
        k_o = dec.last_ms
        crcs = [zlib.crc32(v) for v in views]
        t4 = time.perf_counter()
        assert [g.wav_crc32 for g in got] == crcs
        t5 = time.perf_counter()
        src = dec.digest_pcm_batch(sources)
        t6 = time.perf_counter()
        k_s = dec.last_ms
        assert [bytes(g) for g in src] == [bytes(g) for g in got]
        if it:
            for k, v in (("w_digest", (t2 - t1) * 1e3), ("k_digest", k_d), ("w_old", (t4 - t2) * 1e3), ("w_old_decode", (t3 - t2) * 1e3),
                         ("k_old", k_o), ("w_src", (t6 - t5) * 1e3), ("k_src", k_s)):
                res[k].append(v)
    dec.close()

    def line(key):
        v = res[key]
        return f"{np.median(v):.2f} ms (min..max {np.min(v):.2f}..{np.max(v):.2f})"

    print(f"  {iters} rounds after warm-up, routes alternating inside a round; medians; every digest equals zlib.crc32 of the image")
    print(f"  digest_batch                          wall {line('w_digest')}   kernels (decode + k_digest) {line('k_digest')}")
    print(f"  decode_wav_batch_view + zlib.crc32    wall {line('w_old')}   of which decode_wav_batch_view {line('w_old_decode')}   "
          f"kernels (decode + k_wav_pack) {line('k_old')}")
    print(f"  digest_pcm_batch (interleaved int16)  wall {line('w_src')}   kernel (k_digest alone) {line('k_src')}")
    print(f"  end to end: digest is {np.median(res['w_old']) / np.median(res['w_digest']):.1f}x the old path; k_digest - k_wav_pack on the same "
          f"job = {np.median(res['k_digest']) - np.median(res['k_old']):+.3f} ms")
    print(f"  bytes: k_digest reads {8 * frames / 1e9:.3f} GB of scratch and stores nothing, {8 * n} B cross PCIe; k_wav_pack reads the same, "
          f"writes {4 * frames / 1e9:.3f} GB, and {4 * frames / 1e9:.3f} GB cross PCIe")


workload("one stream", 1, 600, 48000, 7000)
if songs:  # (0: the single stream only, for a profiler run)
    workload("batch", songs, song_secs, 44100, 5000)
