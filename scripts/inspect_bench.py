"""Measurement (not part of the default suite, nothing here is a gate): what a stream inspection costs against the parent's
two ways to touch every block, and what it finds in the bench's materials.
  inspect        Decoder.inspect_batch: k_inspect, a parse-only walk, one lane per block; 336 bytes per block come back
  stats          Decoder.stats_batch: decode, the in-place mid/side inverse, k_stats_blocks
  digest_blocks  Decoder.digest_blocks_batch: decode, the in-place mid/side inverse, k_digest_blocks
Workloads: the 48-song batch of scripts/decode_batch_bench.py (48 x 240 s stereo 16/44.1 synthetic music, seeds 5000..), and
the 10-minute stereo 16/48 streams of scripts/decode_bench.py in the kinds "mixed" and "noise" (seed 2026, wide stereo), all
encoded on the GPU.  Per workload a warm-up round, then `iters` rounds with the three routes alternating inside every
round: wall ms of each (all end synchronised) and the kernel ms the library reports (events around the kernels), best and
median; the spread of the identical repeats is the min..max printed beside them.  The rows' device-to-host copy is timed
on its own (a pinned buffer of the rows' size, the same copy engine).  Then the corpus figures DESIGN §6b quotes: the
shares of partitions and samples by residual mode, of channel blocks by predictor and by partition order, and of the
bits by class.
usage: inspect_bench.py [iters] [songs] [song seconds]"""
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
    raise SystemExit("inspect_bench needs a HIP device")
MODES = ("adaptive", "zero-run", "bin", "static")


def d2h_ms(nbytes):
    """A device-to-host copy of nbytes into pinned memory, best of 5, in ms."""
    dev = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    host = torch.empty(nbytes, dtype=torch.uint8).pin_memory()
    best = 1e9
    for _ in range(6):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host.copy_(dev, non_blocking=True)
        torch.cuda.synchronize()
        best = min(best, (time.perf_counter() - t0) * 1e3)
    return best


def shares(name, reports):
    tot = lambda f: sum(f(r) for r in reports)  # noqa: E731
    parts, samples = [tot(lambda r, m=m: r.mode_parts[m]) for m in range(4)], [tot(lambda r, m=m: r.mode_samples[m]) for m in range(4)]
    cb = tot(lambda r: r.channel_blocks)
    print(f"  {name}: {tot(lambda r: r.blocks)} blocks ({tot(lambda r: r.lost_blocks)} lost, {tot(lambda r: r.ms_blocks)} mid/side), "
          f"{cb} channel blocks, {sum(parts)} partitions, {sum(samples)} samples, {8 * tot(lambda r: r.payload_bytes) / max(1, sum(samples)):.3f} bits per sample")
    print("    partitions by mode: " + ", ".join(f"{MODES[m]} {parts[m]} ({100 * parts[m] / max(1, sum(parts)):.2f} %)" for m in range(4)))
    print("    samples by mode:    " + ", ".join(f"{MODES[m]} {samples[m]} ({100 * samples[m] / max(1, sum(samples)):.2f} %)" for m in range(4)))
    fixed = [tot(lambda r, o=o: r.fixed_blocks[o]) for o in range(5)]
    lpc = {o: tot(lambda r, o=o: r.lpc_blocks[o]) for o in range(1, 33)}
    print("    channel blocks by predictor: " + ", ".join(f"fixed{o} {fixed[o]}" for o in range(5) if fixed[o]) + f", FIR {tot(lambda r: r.fir_blocks)}, "
          + ", ".join(f"LPC{o} {v}" for o, v in lpc.items() if v) + f"  (fixed {100 * sum(fixed) / max(1, cb):.2f} %, LPC {100 * sum(lpc.values()) / max(1, cb):.2f} %)")
    print("    channel blocks by partition order: " + ", ".join(f"p{p} {tot(lambda r, p=p: r.partition_order_blocks[p])}" for p in range(9)))
    bits = 8 * tot(lambda r: r.payload_bytes)
    print("    bits by class: " + ", ".join(f"{k[:-5]} {100 * tot(lambda r, k=k: getattr(r, k)) / max(1, bits):.3f} %" for k in (*lacx.BIT_CLASSES, "flag_bits")))
    print(f"    samples in zero runs {tot(lambda r: r.run_samples)} in {tot(lambda r: r.run_tokens)} runs, escapes {tot(lambda r: r.escape_samples)}, "
          f"bin tags {[tot(lambda r, t=t: r.bin_samples[t]) for t in range(3)]}, k {min(r.k_min for r in reports)}..{max(r.k_max for r in reports)}, "
          f"longest quotient {max(r.unary_max for r in reports)}, largest magnitude {max(r.max_u for r in reports)}")


def workload(name, lacs):
    infos = [lacx.stream_parse(x) for x in lacs]
    blocks = sum(i.blocks for i in infos)
    print(f"{name}: {len(lacs)} stream(s), {sum(map(len, lacs)) / 1e6:.0f} MB .lac, {blocks} blocks")
    dec = lacx.Decoder(device=0)
    res = {k: [] for k in ("w_inspect", "k_inspect", "w_stats", "k_stats", "w_blocks", "k_blocks", "w_parts", "k_parts")}
    reports = None
    for it in range(iters + 1):  # the first round is the warm-up
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        got = dec.inspect_batch(lacs)
        t2 = time.perf_counter()
        k_i = dec.last_ms
        stats = dec.stats_batch(lacs)
        t3 = time.perf_counter()
        k_s = dec.last_ms
        dec.digest_blocks_batch(lacs)
        t4 = time.perf_counter()
        k_b = dec.last_ms
        if it == 0:
            reports = [r for r, _ in got]
            for (r, _), (s, _), i, x in zip(got, stats, infos, lacs):
                assert r.lost_blocks == s.lost_blocks == 0 and r.frames == i.frames and r.head_bytes + r.payload_bytes == len(x)
        else:
            for k, v in (("w_inspect", (t2 - t1) * 1e3), ("k_inspect", k_i), ("w_stats", (t3 - t2) * 1e3), ("k_stats", k_s),
                         ("w_blocks", (t4 - t3) * 1e3), ("k_blocks", k_b)):
                res[k].append(v)
    for it in range(3):  # the library's part of a call alone: the C entry point without the binding's row copies
        import ctypes as C
        bufs = [np.frombuffer(x, dtype=np.uint8) for x in lacs]
        spans = (lacx.Span * len(lacs))(*[lacx.Span(b.ctypes.data_as(C.POINTER(C.c_uint8)), b.size) for b in bufs])
        out, rcs, ms = (lacx.StreamReport * len(lacs))(), (C.c_int * len(lacs))(), C.c_float()
        for key, flags in (("w_inspect_c", 0), ("w_parts", lacx.INSPECT_PARTITIONS)):
            t0 = time.perf_counter()
            assert lacx.lib().lacx_decoder_inspect_batch_device(dec._h, spans, len(lacs), flags, None, rcs, out, C.byref(ms)) == lacx.OK
            res.setdefault(key, []).append((time.perf_counter() - t0) * 1e3)
            if flags:
                res["k_parts"].append(ms.value)
    dec.close()

    def line(key):
        v = res[key]
        return f"best {np.min(v):.2f} median {np.median(v):.2f} ms (min..max {np.min(v):.2f}..{np.max(v):.2f})"

    print(f"  {iters} rounds after warm-up, routes alternating inside a round")
    print(f"  inspect_batch         wall {line('w_inspect')}   kernels (k_inspect) {line('k_inspect')}")
    print(f"  stats_batch           wall {line('w_stats')}   kernels (decode + k_ms_inverse + k_stats_blocks) {line('k_stats')}")
    print(f"  digest_blocks_batch   wall {line('w_blocks')}   kernels (decode + k_ms_inverse + k_digest_blocks) {line('k_blocks')}")
    print(f"  the C call alone (no Python row copies): {line('w_inspect_c')}; with partition detail {line('w_parts')}, kernels {line('k_parts')}")
    print(f"  rows: {336 * blocks} B device to host in {d2h_ms(336 * blocks):.3f} ms; with partition detail {(336 + 2560) * blocks} B in {d2h_ms((336 + 2560) * blocks):.3f} ms")
    shares(name, reports)


def encode(n, secs, rate, depth, kind, seed0, stereo=None):
    enc = lacx.Encoder(12, 2, rate, depth, device=0)
    kw = dict(stereo=stereo) if stereo else {}
    with ThreadPoolExecutor(16) as ex:  # numpy releases the GIL inside the generator's arithmetic
        return [enc.encode(l, r) for l, r in ex.map(lambda k: synth.synth_pcm(secs * rate, 2, depth, rate, seed=seed0 + k, kind=kind, **kw), range(n))]


for kind in ("mixed", "noise"):
    workload(f"10 min {kind} 16/48", encode(1, 600, 48000, 16, kind, 2026, "wide"))
if songs:
    workload(f"batch of {songs} songs 16/44.1 music", encode(songs, song_secs, 44100, 16, "music", 5000))
