"""Measurement (not part of the default suite): what the block digests cost against the whole-stream digest.
  digest         Decoder.digest_batch: decode and one CRC-32 per stream (k_digest), 8 bytes per item come back
  digest_blocks  Decoder.digest_blocks_batch: decode, the in-place mid/side inverse, one CRC-32 per block
                 (k_digest_blocks), 4 bytes per block come back
  check          Decoder.check_batch with every stream's own manifest: the same, and k_digest_judge
Workloads: one 10-minute stereo 16/48 stream, and the 48-song batch of profiles/decode_batch_bench.txt (48 x 240 s stereo
16/44.1 synthetic music, distinct seeds), all encoded on the GPU.  Per workload a warm-up round, then `iters` rounds with
the three routes alternating inside every round: wall ms of each (all end synchronised) and the kernel ms the library
reports.  Every row is checked against digest_batch (lacx_crc32_combine of the rows) and one stream against zlib.
usage: blockdigest_bench.py [iters] [songs] [song seconds]"""
import os
import sys
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import __graft_entry__ as ge  # noqa: E402
import wavutil as W  # noqa: E402

pkg = ge.load_pkg()
lacx, synth = pkg.lacx, pkg.synth
iters = int(sys.argv[1]) if len(sys.argv) > 1 else 5
songs = int(sys.argv[2]) if len(sys.argv) > 2 else 48
song_secs = int(sys.argv[3]) if len(sys.argv) > 3 else 240
if lacx.device_count() < 1:
    raise SystemExit("blockdigest_bench needs a HIP device")


def workload(name, n, secs, rate, seed0):
    t0 = time.perf_counter()
    enc = lacx.Encoder(12, 2, rate, 16, device=0)
    lacs, first = [], None
    with ThreadPoolExecutor(16) as ex:  # numpy releases the GIL inside the generator's arithmetic
        for left, right in ex.map(lambda k: synth.synth_pcm(secs * rate, 2, 16, rate, seed=seed0 + k, kind="music"), range(n)):
            lacs.append(enc.encode(left, right))
            if first is None:
                first = W.pcm_bytes(left, right, 16)
    blocks = sum(lacx.stream_parse(x).blocks for x in lacs)
    print(f"{name}: {n} x {secs} s stereo 16/{rate / 1000:g} music, {sum(map(len, lacs)) / 1e6:.0f} MB .lac, {blocks} blocks "
          f"(set-up {time.perf_counter() - t0:.0f} s)")
    dec = lacx.Decoder(device=0)
    manifests = [lacx.manifest_build(g, rows) for g, rows in dec.digest_blocks_batch(lacs)]
    res = {k: [] for k in ("w_digest", "k_digest", "w_blocks", "k_blocks", "w_check", "k_check")}
    for it in range(iters + 1):  # the first round is the warm-up
        t1 = time.perf_counter()
        whole = dec.digest_batch(lacs)
        t2 = time.perf_counter()
        k_d = dec.last_ms
        rows = dec.digest_blocks_batch(lacs)
        t3 = time.perf_counter()
        k_b = dec.last_ms
        checked = dec.check_batch(lacs, manifests)
        t4 = time.perf_counter()
        k_c = dec.last_ms
        assert [bytes(g) for g, _ in rows] == [bytes(g) for g in whole]
        assert all(r.bad_blocks == 0 and not f for r, f in checked)
        if it == 0:
            frames0 = rows[0][1][0].frames
            assert rows[0][1][0].crc32 == zlib.crc32(first[:4 * frames0]) and whole[0].data_crc32 == zlib.crc32(first)
        else:
            for k, v in (("w_digest", (t2 - t1) * 1e3), ("k_digest", k_d), ("w_blocks", (t3 - t2) * 1e3), ("k_blocks", k_b),
                         ("w_check", (t4 - t3) * 1e3), ("k_check", k_c)):
                res[k].append(v)
    dec.close()

    def line(key):
        v = res[key]
        return f"{np.median(v):.2f} ms (min..max {np.min(v):.2f}..{np.max(v):.2f})"

    print(f"  {iters} rounds after warm-up, routes alternating inside a round; medians; the rows combine to digest_batch's CRC-32")
    print(f"  digest_batch          wall {line('w_digest')}   kernels (decode + k_digest) {line('k_digest')}")
    print(f"  digest_blocks_batch   wall {line('w_blocks')}   kernels (decode + k_ms_inverse + k_digest_blocks) {line('k_blocks')}")
    print(f"  check_batch           wall {line('w_check')}   kernels (... + k_digest_judge) {line('k_check')}")
    print(f"  extra over digest_batch: blocks {np.median(res['k_blocks']) - np.median(res['k_digest']):+.3f} ms of kernels, "
          f"{np.median(res['w_blocks']) - np.median(res['w_digest']):+.2f} ms of wall; check "
          f"{np.median(res['k_check']) - np.median(res['k_digest']):+.3f} ms of kernels, {np.median(res['w_check']) - np.median(res['w_digest']):+.2f} ms of wall; "
          f"{4 * blocks} B of block digests cross PCIe instead of {8 * n} B")


workload("one stream", 1, 600, 48000, 7000)
if songs:  # (0: the single stream only, for a profiler run)
    workload("batch", songs, song_secs, 44100, 5000)
