"""Measurement (not part of the default suite): what the rip checksums cost against the digest and against what a user has
without them.  Writes profiles/accuraterip_bench.txt (and prints the same).
  accuraterip  Decoder.accuraterip_batch: decode, the in-place mid/side inverse and k_accuraterip; 12 (2 radius + 1) bytes per
               track come back
  digest       Decoder.digest_batch: the same strict job with k_digest in the slot -- the difference is the kernel's
  torch        the status quo on the device: Decoder.decode_batch_device into torch tensors, then per track and offset the three
               sums in int64 (m * x < 2^56 for a track below 2^24 frames: exact), masked and shifted
  alone        Decoder.accuraterip_pcm_batch over the decoded tensors: k_accuraterip alone, no decode in front
Workload: the 48-song batch of profiles/decode_batch_bench.txt (48 x 240 s stereo 16/44.1 synthetic music, distinct seeds,
encoded on the GPU) as four discs of twelve tracks, one stream per track, whole discs (first and last).  At radius 0 a warm-up
round, then `iters` rounds with the routes alternating inside every round; at radius 2939 a warm-up and `iters` rounds of the
two product routes; the torch route at growing radii while a run stays within a minute (the largest it finished is stated,
nothing is extrapolated).  The sums of the routes are checked to be the same integers.
Without a HIP device nothing is measured, and the script says so.
usage: accuraterip_bench.py [iters] [songs] [song seconds] [discs]"""
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import __graft_entry__ as ge  # noqa: E402

pkg = ge.load_pkg()
lacx, synth = pkg.lacx, pkg.synth
iters = int(sys.argv[1]) if len(sys.argv) > 1 else 3
songs = int(sys.argv[2]) if len(sys.argv) > 2 else 48
song_secs = int(sys.argv[3]) if len(sys.argv) > 3 else 240
ndiscs = int(sys.argv[4]) if len(sys.argv) > 4 else 4
if lacx.device_count() < 1:
    raise SystemExit("not measured yet: accuraterip_bench needs a HIP device")
RATE, EDGE, MASK = 44100, 2940, 0xFFFFFFFF
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def torch_sums(words, radius):
    """Per track v1 and v2 at every offset in int64 on the device: words: per disc (int64 words padded by `radius` zeros on
    both sides, [track lengths])."""
    out = []
    for x, tracks in words:
        start = 0
        for t, n in enumerate(tracks):
            lo = EDGE if t == 0 else 1
            hi = n - EDGE if t == len(tracks) - 1 else n
            m = torch.arange(lo, hi + 1, dtype=torch.int64, device="cuda")
            v1, v2 = [], []
            for o in range(-radius, radius + 1):
                a = radius + start + o + lo - 1
                p = m * x[a:a + len(m)]
                low = (p & MASK).sum()
                v1.append(low)
                v2.append(low + (p >> 32).sum())
            out.append((torch.stack(v1) & MASK, torch.stack(v2) & MASK))
            start += n
    return [(a.cpu().numpy(), b.cpu().numpy()) for a, b in out]  # (the copies synchronise)


def med(v):
    return f"{np.median(v):.2f} ms (min..max {np.min(v):.2f}..{np.max(v):.2f})"


t0 = time.perf_counter()
enc = lacx.Encoder(12, 2, RATE, 16, device=0)
lacs = []
with ThreadPoolExecutor(16) as ex:  # numpy releases the GIL inside the generator's arithmetic
    for left, right in ex.map(lambda k: synth.synth_pcm(song_secs * RATE, 2, 16, RATE, seed=5000 + k, kind="music"), range(songs)):
        lacs.append(enc.encode(left, right))
infos = [lacx.stream_parse(x) for x in lacs]
frames = sum(i.frames for i in infos)
per = songs // ndiscs
discs = [lacs[k * per:(k + 1) * per] for k in range(ndiscs)]
say(f"{songs} x {song_secs} s stereo 16/44.1 music as {ndiscs} discs of {per} tracks, {sum(map(len, lacs)) / 1e6:.0f} MB .lac, {frames} frames "
    f"(set-up {time.perf_counter() - t0:.0f} s)")
dec = lacx.Decoder(device=0)
outs = [torch.empty((2, i.frames), dtype=torch.int32, device="cuda") for i in infos]


def words_of(radius):
    dec.decode_batch_device(lacs, [(o[0].data_ptr(), o[1].data_ptr()) for o in outs])
    res = []
    for k in range(ndiscs):
        mine = outs[k * per:(k + 1) * per]
        x = torch.cat([(o[0].to(torch.int64) & 0xFFFF) | ((o[1].to(torch.int64) & 0xFFFF) << 16) for o in mine])
        res.append((torch.nn.functional.pad(x, (radius, radius)), [o.shape[1] for o in mine]))
    return res


def product_routes(radius, rounds, with_digest):
    res = {k: [] for k in ("w_ar", "k_ar", "w_dg", "k_dg", "w_alone", "k_alone")}
    got = alone = None
    for it in range(rounds + 1):  # the first round is the warm-up
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        got = dec.accuraterip_batch([(d, None, radius) for d in discs])
        t2 = time.perf_counter()
        k_ar = dec.last_ms
        if with_digest:
            dec.digest_batch(lacs)
        t3 = time.perf_counter()
        k_dg = dec.last_ms
        alone = dec.accuraterip_pcm_batch([([(o, RATE, 16) for o in outs[k * per:(k + 1) * per]], None, radius) for k in range(ndiscs)])
        t4 = time.perf_counter()
        k_alone = dec.last_ms
        if it:
            for k, v in (("w_ar", (t2 - t1) * 1e3), ("k_ar", k_ar), ("w_dg", (t3 - t2) * 1e3), ("k_dg", k_dg), ("w_alone", (t4 - t3) * 1e3), ("k_alone", k_alone)):
                res[k].append(v)
    for a, b in zip(got, alone):
        assert (a.v1 == b.v1).all() and (a.v2 == b.v2).all() and (a.s450 == b.s450).all(), "the two forms differ"
    return res, got


# ---- radius 0 ----
dec.decode_batch_device(lacs, [(o[0].data_ptr(), o[1].data_ptr()) for o in outs])  # (the tensors the source form reads)
res, got = product_routes(0, iters, True)
w_torch = []
for it in range(iters + 1):
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    ref = torch_sums(words_of(0), 0)
    if it:
        w_torch.append((time.perf_counter() - t1) * 1e3)
flat = [(d.v1[t], d.v2[t]) for d in got for t in range(len(d.tracks))]
for (a, b), (c, e) in zip(flat, ref):
    assert (a == c).all() and (b == e).all(), "the torch route differs"
say(f"radius 0: {iters} rounds after warm-up, routes alternating inside a round; medians; all routes give the same integers")
say(f"  accuraterip_batch     wall {med(res['w_ar'])}   kernels (decode + k_ms_inverse + k_accuraterip) {med(res['k_ar'])}")
say(f"  digest_batch          wall {med(res['w_dg'])}   kernels (decode + k_ms_inverse + k_digest) {med(res['k_dg'])}")
say(f"  decode + torch        wall {med(w_torch)}   (decode_batch_device, then masked int64 products and sums per track)")
say(f"  accuraterip_pcm_batch wall {med(res['w_alone'])}   k_accuraterip alone {med(res['k_alone'])} for {8 * frames / 1e9:.2f} GB of PCM: "
    f"{8 * frames / 1e6 / np.median(res['k_alone']):.0f} GB/s")
say(f"  accuraterip over digest: {np.median(res['k_ar']) - np.median(res['k_dg']):+.3f} ms of kernels, {np.median(res['w_ar']) - np.median(res['w_dg']):+.2f} ms of wall")

# ---- radius 2939 ----
R = 2939
res, got = product_routes(R, max(1, iters - 1), False)
pairs = float(sum(int(t.frames) for d in got for t in d.tracks)) * (2 * R + 1)  # (a track's range is its frames less the disc's edges)
say(f"radius {R}: {max(1, iters - 1)} rounds after warm-up; {pairs:.3e} (multiplier, offset) pairs and 588 x 5879 per track for s450")
say(f"  accuraterip_batch     wall {med(res['w_ar'])}   kernels {med(res['k_ar'])}")
say(f"  accuraterip_pcm_batch wall {med(res['w_alone'])}   k_accuraterip alone {med(res['k_alone'])}: {pairs / 1e6 / np.median(res['k_alone']):.0f} G pairs/s "
    f"(the product: one 64-bit multiply, (uint64)m * x, and the two halves added per pair; the only variant built into the kernel)")
mid = [(d.v1[t][R - 1:R + 2], d.v2[t][R - 1:R + 2]) for d in got for t in range(len(d.tracks))]

# ---- the torch route at growing radii ----
done = None
for radius in (1, 16, 128, 1024):
    words = words_of(radius)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    ref = torch_sums(words, radius)
    took = time.perf_counter() - t1
    if radius == 1:
        for (a, b), (c, e) in zip(mid, ref):
            assert (a == c).all() and (b == e).all(), "the torch route differs at radius 1"
    if took > 60.0:
        say(f"  decode + torch at radius {radius}: {took:.1f} s, over a minute")
        break
    done = (radius, took)
    say(f"  torch sums alone at radius {radius}: {took:.2f} s, {float(frames) * (2 * radius + 1) / 1e9 / took:.1f} G pairs/s (v1 and v2; no s450)")
    if took * 8 > 60.0:  # the next radius is eight times the work
        break
say(f"  the largest radius the torch route finished within a minute here: {done[0] if done else 'none'}; larger radii were not run")
dec.close()
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "accuraterip_bench.txt"), "w") as f:
    f.write("\n".join(lines) + "\n")
