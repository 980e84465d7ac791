"""Measurement (not part of the default suite): what the bit-compare costs against the digest and against what a user has
without it.  Writes profiles/compare_bench.txt (and prints the same).
  compare   Decoder.compare_batch: decode, the in-place mid/side inverse, k_compare_search (radius > 0), the host's look at the
            counts, k_compare_rows; 8 (2 radius + 1) bytes per pair and 96 bytes per 16384 frames come back
  digest    Decoder.digest_batch of the same streams: the floor of the job -- the same strict decode with k_digest in the slot
  torch     the status quo on the device: Decoder.decode_batch_device into torch tensors, then per pair and offset one
            comparison of the zero-extended tensors and a count
  alone     Decoder.compare_pcm_batch over the decoded tensors: the two kernels alone, no decode in front; at radius 0 with the
            planted offsets as centres that is k_compare_rows alone, and the search is the difference to it (the round trip
            between the two kernels included)
Workload: the 48-song batch of profiles/decode_batch_bench.txt as 24 pairs -- 24 x 240 s stereo 16/44.1 synthetic music,
distinct seeds, each against a copy shifted by a planted offset of up to 587 frames (zeros shifted in, the end cut), all 48
encoded on the GPU -- at radius 0, 588 and 2939.  A warm-up round, then `iters` rounds with the routes alternating inside
every round; the torch route at growing radii while a run stays within a minute (the largest it finished is stated, nothing
is extrapolated).  The chosen offsets are checked to be the planted ones and the routes' counts the same integers.
Without a HIP device nothing is measured, and the script says so.
usage: compare_bench.py [iters] [pairs] [song seconds]"""
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
npairs = int(sys.argv[2]) if len(sys.argv) > 2 else 24
song_secs = int(sys.argv[3]) if len(sys.argv) > 3 else 240
if lacx.device_count() < 1:
    raise SystemExit("not measured yet: compare_bench needs a HIP device")
RATE = 44100
PLANTED = (6, -12, 30, -102, 294, -587, 1, -3)
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def med(v):
    return f"{np.median(v):.2f} ms (min..max {np.min(v):.2f}..{np.max(v):.2f})"


def shifted(x, o):
    out = np.zeros_like(x)
    if o >= 0:
        out[o:] = x[:len(x) - o]
    else:
        out[:o] = x[-o:]
    return out


t0 = time.perf_counter()
enc = lacx.Encoder(12, 2, RATE, 16, device=0)
lacs, planted = [], [PLANTED[k % len(PLANTED)] for k in range(npairs)]
with ThreadPoolExecutor(16) as ex:  # numpy releases the GIL inside the generator's arithmetic
    for k, (left, right) in enumerate(ex.map(lambda k: synth.synth_pcm(song_secs * RATE, 2, 16, RATE, seed=5000 + k, kind="music"), range(npairs))):
        lacs.append(enc.encode(left, right))
        lacs.append(enc.encode(shifted(left, planted[k]), shifted(right, planted[k])))
infos = [lacx.stream_parse(x) for x in lacs]
frames = sum(i.frames for i in infos[::2])
say(f"{npairs} pairs of {song_secs} s stereo 16/44.1 music, each a song against a copy shifted by a planted offset, {sum(map(len, lacs)) / 1e6:.0f} MB .lac, "
    f"{frames} frames a side (set-up {time.perf_counter() - t0:.0f} s)")
dec = lacx.Decoder(device=0)
outs = [torch.empty((2, i.frames), dtype=torch.int32, device="cuda") for i in infos]
dec.decode_batch_device(lacs, [(o[0].data_ptr(), o[1].data_ptr()) for o in outs])  # (the tensors the source form reads)
sources = [(o, RATE, 16) for o in outs]


def torch_counts(radius):
    """Per pair mis[] over -radius .. radius on the device: both sides zero-extended by `radius`, one comparison per offset."""
    dec.decode_batch_device(lacs, [(o[0].data_ptr(), o[1].data_ptr()) for o in outs])
    res = []
    for k in range(npairs):
        a = torch.nn.functional.pad(outs[2 * k], (2 * radius, 2 * radius))  # A over [-2 radius, n + 2 radius)
        b = torch.nn.functional.pad(outs[2 * k + 1], (radius, radius))      # B over [-radius, n + radius)
        n = b.shape[1]
        res.append(torch.stack([(a[:, radius - o:radius - o + n] != b).sum() for o in range(-radius, radius + 1)]))
    return [r.cpu().numpy() for r in res]  # (the copies synchronise)


def product_routes(radius, rounds, with_digest):
    res = {k: [] for k in ("w_cmp", "k_cmp", "w_dg", "k_dg", "w_alone", "k_alone", "w_rows", "k_rows")}
    got = alone = None
    for it in range(rounds + 1):  # the first round is the warm-up
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        got = dec.compare_batch(lacs, [(2 * k, 2 * k + 1, 0, radius) for k in range(npairs)])
        t2 = time.perf_counter()
        k_cmp = dec.last_ms
        if with_digest:
            dec.digest_batch(lacs)
        t3 = time.perf_counter()
        k_dg = dec.last_ms
        alone = dec.compare_pcm_batch(sources, [(2 * k, 2 * k + 1, 0, radius) for k in range(npairs)])
        t4 = time.perf_counter()
        k_alone = dec.last_ms
        dec.compare_pcm_batch(sources, [(2 * k, 2 * k + 1, alone[k].offset, 0) for k in range(npairs)])
        t5 = time.perf_counter()
        k_rows = dec.last_ms
        if it:
            for k, v in (("w_cmp", (t2 - t1) * 1e3), ("k_cmp", k_cmp), ("w_dg", (t3 - t2) * 1e3), ("k_dg", k_dg), ("w_alone", (t4 - t3) * 1e3), ("k_alone", k_alone),
                         ("w_rows", (t5 - t4) * 1e3), ("k_rows", k_rows)):
                res[k].append(v)
    for a, b in zip(got, alone):
        assert (a.counts == b.counts).all() and bytes(a.totals) == bytes(b.totals), "the two forms differ"
    return res, got


def report(radius, res, got, with_digest):
    cmps = 2.0 * sum(float(g.domain_frames) for g in got) * (2 * radius + 1)
    say(f"radius {radius}: {len(res['w_cmp'])} rounds after warm-up, routes alternating inside a round; medians; {npairs / np.median(res['w_cmp']) * 1e3:.0f} pairs per second of wall")
    say(f"  compare_batch      wall {med(res['w_cmp'])}   kernels (decode + k_ms_inverse + search + round trip + rows) {med(res['k_cmp'])}")
    if with_digest:
        say(f"  digest_batch       wall {med(res['w_dg'])}   kernels (decode + k_ms_inverse + k_digest) {med(res['k_dg'])}")
    say(f"  compare_pcm_batch  wall {med(res['w_alone'])}   both kernels alone {med(res['k_alone'])}")
    say(f"  k_compare_rows alone (radius 0 at the chosen offsets) {med(res['k_rows'])} for {16 * frames / 1e9:.2f} GB of PCM: {16 * frames / 1e6 / np.median(res['k_rows']):.0f} GB/s")
    if radius:
        search = np.median(res['k_alone']) - np.median(res['k_rows'])
        say(f"  k_compare_search and the round trip (the difference) {search:.2f} ms: {cmps:.3e} sample comparisons, {cmps / 1e6 / search:.0f} G comparisons/s "
            f"(four offsets a lane, four frames a step; the only inner loop built)")


res, got = product_routes(0, iters, True)
assert all(g.mismatches > 0 for g in got)
report(0, res, got, True)
for R in (588, 2939):
    res, got = product_routes(R, max(1, iters - 1), R == 588)
    assert [g.offset for g in got] == planted, "a planted offset was not found"
    report(R, res, got, R == 588)
    wide = got

# ---- the torch route at growing radii ----
done = None
for radius in (1, 16, 128, 588):
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    ref = torch_counts(radius)
    took = time.perf_counter() - t1
    for k in range(npairs):
        assert (ref[k] == wide[k].counts[2939 - radius:2939 + radius + 1].astype(np.int64)).all(), "the torch route differs"
    if took > 60.0:
        say(f"  decode + torch at radius {radius}: {took:.1f} s, over a minute")
        break
    done = (radius, took)
    say(f"  decode + torch counts at radius {radius}: {took:.2f} s wall, {2.0 * frames * (2 * radius + 1) / 1e9 / took:.1f} G comparisons/s; the same integers")
    if took * 5 > 60.0:
        break
say(f"  the largest radius the torch route finished within a minute here: {done[0] if done else 'none'}; larger radii were not run")
dec.close()
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "compare_bench.txt"), "w") as f:
    f.write("\n".join(lines) + "\n")
