"""Measurement (not part of the default suite): A/B of the device decoder, another build of liblacx.so (`other`, e.g. the
parent commit's, built in a git worktree) against this tree's, alternated in one process (ABBA order per round, through
lacx.use_library).  Every output of both is checked against the input PCM on the warm-up round.  Workloads: 600 s of
stereo 16/48 music and of mixed material (Decoder(reuse_output=True).decode and Decoder.decode_wav_view, kernel and
wall ms), 48 four-minute stereo 16/44.1 music streams as one decode_wav_batch_view, and a 2 h stream (the 600 s music
stream spliced twelve times).  Per metric: median, IQR, min..max, and the distance between the medians of even and odd
rounds (each version against itself).
usage: decode_ab.py other_liblacx.so [rounds]      (profiles/decode_one_decoder_ab.txt)"""
import hashlib
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import __graft_entry__ as ge  # noqa: E402
import lacstreams  # noqa: E402
import wavutil as W  # noqa: E402

pkg = ge.load_pkg()
lacx, synth = pkg.lacx, pkg.synth
LIBS = {"main": os.path.abspath(sys.argv[1]), "branch": lacx.LIB_PATH}
ROUNDS = int(sys.argv[2]) if len(sys.argv) > 2 else 21
assert os.path.exists(LIBS["main"]), LIBS["main"]


def h(x):
    return hashlib.sha256(np.ascontiguousarray(x).tobytes() if isinstance(x, np.ndarray) else bytes(x)).hexdigest()


def stats(v):
    v = np.asarray(v)
    q1, med, q3 = np.percentile(v, [25, 50, 75])
    half = abs(np.median(v[0::2]) - np.median(v[1::2]))  # the version against itself: even rounds vs odd rounds
    return med, q3 - q1, v.min(), v.max(), half


def report(name, res):
    print(f"== {name}: {ROUNDS} rounds, ABBA; median | IQR | min..max | |even-odd median| (self spread)")
    for metric in res["main"]:
        a, b = stats(res["main"][metric]), stats(res["branch"][metric])
        spread = max(a[1], b[1], a[4], b[4])
        verdict = "ok" if b[0] - a[0] <= spread else "SLOWER"
        print(f"  {metric:24s} main {a[0]:8.3f} | {a[1]:.3f} | {a[2]:.3f}..{a[3]:.3f} | {a[4]:.3f}   "
              f"branch {b[0]:8.3f} | {b[1]:.3f} | {b[2]:.3f}..{b[3]:.3f} | {b[4]:.3f}   "
              f"diff {b[0] - a[0]:+.3f} ({100 * (b[0] - a[0]) / a[0]:+.1f} %) spread {spread:.3f} {verdict}")
    sys.stdout.flush()


def single(name, lac, want_l, want_r, want_wav):
    decs = {}
    for v, path in LIBS.items():
        lacx.use_library(path)
        decs[v] = (lacx.Decoder(device=0, reuse_output=True), lacx.Decoder(device=0))
    res = {v: {"decode_kernel_ms": [], "decode_wall_ms": [], "wav_view_kernel_ms": [], "wav_view_wall_ms": []} for v in LIBS}
    for rnd in range(ROUNDS + 1):  # round 0: warm-up and checks
        for v in (("main", "branch") if rnd % 2 else ("branch", "main")):
            lacx.use_library(LIBS[v])
            pcm, wav = decs[v]
            t0 = time.perf_counter()
            l, r, _, ms = pcm.decode(lac)
            t1 = time.perf_counter()
            view = wav.decode_wav_view(lac)
            t2 = time.perf_counter()
            if rnd == 0:
                assert (h(l), h(r)) == (want_l, want_r), (name, v)
                assert h(view) == want_wav, (name, v)
                continue
            res[v]["decode_kernel_ms"].append(ms)
            res[v]["decode_wall_ms"].append((t1 - t0) * 1e3)
            res[v]["wav_view_kernel_ms"].append(wav.last_ms)
            res[v]["wav_view_wall_ms"].append((t2 - t1) * 1e3)
    for v, path in LIBS.items():
        lacx.use_library(path)
        for d in decs[v]:
            d.close()
    report(name, res)


def batch(name, lacs, want):
    decs = {}
    for v, path in LIBS.items():
        lacx.use_library(path)
        decs[v] = lacx.Decoder(device=0)
    res = {v: {"batch_kernel_ms": [], "batch_wall_ms": []} for v in LIBS}
    for rnd in range(ROUNDS + 1):
        for v in (("main", "branch") if rnd % 2 else ("branch", "main")):
            lacx.use_library(LIBS[v])
            t0 = time.perf_counter()
            views = decs[v].decode_wav_batch_view(lacs)
            t1 = time.perf_counter()
            if rnd == 0:
                assert [h(x) for x in views] == want, (name, v)
                continue
            res[v]["batch_kernel_ms"].append(decs[v].last_ms)
            res[v]["batch_wall_ms"].append((t1 - t0) * 1e3)
    for v, path in LIBS.items():
        lacx.use_library(path)
        decs[v].close()
    report(name, res)


lacx.use_library(LIBS["branch"])
sr, bd = 48000, 16
enc = lacx.Encoder(12, 2, sr, bd, device=0)
t0 = time.perf_counter()
left, right = synth.synth_pcm(600 * sr, 2, bd, sr, seed=2026, kind="music", stereo="wide")
music = enc.encode(left, right)
mixed_l, mixed_r = synth.synth_pcm(600 * sr, 2, bd, sr, seed=7, kind="mixed", stereo="wide")
mixed = enc.encode(mixed_l, mixed_r)
lacs, want = [], []
with ThreadPoolExecutor(16) as ex:  # the batch bench's workload: 48 four-minute stereo 16/44.1 music streams
    for l, r in ex.map(lambda k: synth.synth_pcm(240 * 44100, 2, 16, 44100, seed=5000 + k, kind="music"), range(48)):
        lacs.append(lacx.Encoder(12, 2, 44100, 16, device=0).encode(l, r))
        want.append(h(W.make_wav(l, r, 44100, 16)))
del l, r
enc._reset()  # (its handle belongs to the branch's library: released before the A/B switches libraries)
del enc
print(f"set-up {time.perf_counter() - t0:.0f} s; music {lacx.stream_parse(music).blocks} blocks, "
      f"mixed {lacx.stream_parse(mixed).blocks} blocks, batch {sum(lacx.stream_parse(x).blocks for x in lacs)} blocks")
sys.stdout.flush()

single("600 s stereo 16/48 music", music, h(left), h(right), h(W.make_wav(left, right, sr, bd)))
single("600 s stereo 16/48 mixed", mixed, h(mixed_l), h(mixed_r), h(W.make_wav(mixed_l, mixed_r, sr, bd)))
del mixed_l, mixed_r
batch("48 x 240 s stereo 16/44.1 music, one batch", lacs, want)
del lacs
# 2 h: the 600 s music stream twelve times over (its last block becomes a non-final one of 13 312 frames)
two_h = music
for _ in range(11):
    two_h = lacstreams.splice(two_h, music)
L2, R2 = np.tile(left, 12), np.tile(right, 12)
del left, right
print(f"2 h stream: {lacx.stream_parse(two_h).blocks} blocks")
single("2 h stereo 16/48 music (12 x 600 s)", two_h, h(L2), h(R2), h(W.make_wav(L2, R2, sr, bd)))
print("AB_DONE")
