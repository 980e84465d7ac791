"""Measurement (not part of the default suite): what the recovery data costs, beside the existing call that moves the
same bytes.
  digest   Decoder.digest_batch: the streams go up, decode and one CRC-32 per stream, 8 bytes per item come back
  build    Decoder.recovery_build_batch: the files go up, k_gf_combine makes the parity, k_slice_crc one CRC-32 per slice
           and parity record, the parity comes down
  scan     Decoder.recovery_scan_batch: files and parity go up, k_slice_crc, 4 bytes per slice come back
  repair   Decoder.repair_batch of the batch with a burst of r * G - 1 slices destroyed in every file: the scan, then the
           solved matrices go up, k_gf_combine rebuilds, k_slice_crc digests the rebuilt slices, the files come down
Workload: the 48-song batch of profiles/decode_batch_bench.txt (48 x 240 s stereo 16/44.1 synthetic music, distinct seeds),
encoded on the GPU; default parameters (4096, 8, 128).  A warm-up round, then `iters` rounds with the routes alternating
inside every round: wall ms of each and the kernel ms the library reports.  Every repaired file is compared with the original.
usage: recovery_bench.py [iters] [songs] [song seconds]"""
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import __graft_entry__ as ge  # noqa: E402

pkg = ge.load_pkg()
lacx, synth = pkg.lacx, pkg.synth
iters = int(sys.argv[1]) if len(sys.argv) > 1 else 5
songs = int(sys.argv[2]) if len(sys.argv) > 2 else 48
song_secs = int(sys.argv[3]) if len(sys.argv) > 3 else 240
if lacx.device_count() < 1:
    raise SystemExit("recovery_bench needs a HIP device")

rate = 44100
t0 = time.perf_counter()
enc = lacx.Encoder(12, 2, rate, 16, device=0)
with ThreadPoolExecutor(16) as ex:  # numpy releases the GIL inside the generator's arithmetic
    lacs = [enc.encode(left, right) for left, right in ex.map(lambda k: synth.synth_pcm(song_secs * rate, 2, 16, rate, seed=5000 + k, kind="music"), range(songs))]
dec = lacx.Decoder(device=0)
sides = dec.recovery_build_batch(lacs)
infos = [lacx.recovery_parse(s) for s in sides]
hurt = []
for lac, info in zip(lacs, infos):  # a burst that every group can still carry
    b = np.frombuffer(lac, np.uint8).copy()
    n = (info.parity * info.groups - 1) * info.slice_bytes
    at = (len(lac) // 3) // info.slice_bytes * info.slice_bytes
    b[at:at + n] ^= 0xFF
    hurt.append(b.tobytes())
print(f"batch: {songs} x {song_secs} s stereo 16/{rate / 1000:g} music, {sum(map(len, lacs)) / 1e6:.0f} MB .lac, {sum(map(len, sides)) / 1e6:.0f} MB of sidecars, "
      f"{sum(i.slices for i in infos)} slices in {sum(i.groups for i in infos)} groups; damaged copy: {sum((i.parity * i.groups - 1) for i in infos)} slices "
      f"destroyed (set-up {time.perf_counter() - t0:.0f} s)")
res = {k: [] for k in ("w_digest", "k_digest", "w_build", "k_build", "w_scan", "k_scan", "w_repair", "k_repair")}
for it in range(iters + 1):  # the first round is the warm-up
    row = {}
    t1 = time.perf_counter()
    dec.digest_batch(lacs)
    row["w_digest"], row["k_digest"] = (time.perf_counter() - t1) * 1e3, dec.last_ms
    t1 = time.perf_counter()
    built = dec.recovery_build_batch(lacs)
    row["w_build"], row["k_build"] = (time.perf_counter() - t1) * 1e3, dec.last_ms
    t1 = time.perf_counter()
    scanned = dec.recovery_scan_batch(lacs, sides)
    row["w_scan"], row["k_scan"] = (time.perf_counter() - t1) * 1e3, dec.last_ms
    t1 = time.perf_counter()
    fixed = dec.repair_batch(hurt, sides)
    row["w_repair"], row["k_repair"] = (time.perf_counter() - t1) * 1e3, dec.last_ms
    assert built == sides and all(r.bad_slices == 0 for r, _ in scanned)
    assert all(data == lac and r.repaired_slices == r.bad_slices > 0 for (data, r, _), lac in zip(fixed, lacs))
    if it:
        for k, v in row.items():
            res[k].append(v)
dec.close()


def line(key):
    v = res[key]
    return f"{np.median(v):.2f} ms (min..max {np.min(v):.2f}..{np.max(v):.2f})"


print(f"  {iters} rounds after warm-up, routes alternating inside a round; medians; wall includes the binding's copies of what comes back")
print(f"  digest_batch           wall {line('w_digest')}   kernels (decode + k_digest) {line('k_digest')}")
print(f"  recovery_build_batch   wall {line('w_build')}   kernels (k_gf_combine + k_slice_crc) {line('k_build')}")
print(f"  recovery_scan_batch    wall {line('w_scan')}   kernels (k_slice_crc) {line('k_scan')}")
print(f"  repair_batch           wall {line('w_repair')}   kernels (k_slice_crc, then k_gf_combine + k_slice_crc) {line('k_repair')}")
