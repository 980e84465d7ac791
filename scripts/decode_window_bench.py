"""Measurement (not part of the default suite): random frame windows of a collection as one device job against the
whole-stream batch decode followed by slicing.
Workload: the 48 synthetic 4-minute stereo 16/44.1 music streams of decode_batch_bench.py (same seeds; 31 008 blocks),
encoded on the GPU, and `w` random one-second windows over them (uniform stream, uniform start; seeded).  After a
warm-up, best / median of `iters` rounds of:
  window: lacx_decoder_decode_window_batch_device of all windows into one [w, 2, 44100] torch tensor, int32 and
    float32 -- kernel ms (events) and wall ms (the call returns once the outputs are final);
  whole:  lacx_decoder_decode_batch_device of the whole streams into one flat int32 tensor per channel, then one gather
    per channel that cuts the windows out into a [w, 2, 44100] tensor, synchronised -- kernel ms of the decode, wall ms
    of decode + gather;
  both through the C ABI with item arrays built once, so that the wall times hold no binding work (the binding's
  decode_batch_device copies every stream to parse it); Decoder.decode_window_batch_device's wall ms is printed too.
Every window of both forms is checked against the input PCM (float32: bit-equal to pcm / 2^15).
usage: decode_window_bench.py [windows] [iters] [streams]"""
import ctypes as C
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
nw = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
iters = int(sys.argv[2]) if len(sys.argv) > 2 else 5
n = int(sys.argv[3]) if len(sys.argv) > 3 else 48
secs, sr, bd = 240, 44100, 16
T = sr  # one second
if lacx.device_count() < 1:
    raise SystemExit("decode_window_bench needs a HIP device")

t0 = time.perf_counter()
enc = lacx.Encoder(12, 2, sr, bd, device=0)
lacs, pcm = [], []  # pcm[k]: [2, frames] int16 (the input, for the checks)
with ThreadPoolExecutor(16) as ex:
    for left, right in ex.map(lambda k: synth.synth_pcm(secs * sr, 2, bd, sr, seed=5000 + k, kind="music"), range(n)):
        lacs.append(enc.encode(left, right))
        pcm.append(np.stack([left, right]).astype(np.int16))
del left, right
infos = [lacx.stream_parse(x) for x in lacs]
frames = np.array([i.frames for i in infos], dtype=np.int64)
rng = np.random.default_rng(2024)
song = rng.integers(0, n, size=nw)
start = np.array([rng.integers(0, frames[s] - T + 1) for s in song], dtype=np.int64)


def blocks_of(lac):
    nb = int.from_bytes(lac[10:14], "big")
    t = np.frombuffer(lac, dtype=">u4", count=2 * nb, offset=14).reshape(nb, 2).astype(np.int64)
    return np.concatenate([[0], np.cumsum(t[:, 0])]), np.concatenate([[0], np.cumsum(t[:, 1])])


tables = [blocks_of(x) for x in lacs]
win_blocks = win_bytes = 0
for s, st in zip(song, start):
    fo, bo = tables[s]
    b0 = int(np.searchsorted(fo, st, side="right")) - 1
    b1 = int(np.searchsorted(fo, st + T - 1, side="right")) - 1
    win_blocks += b1 - b0 + 1
    win_bytes += int(bo[b1 + 1] - bo[b0])
total_blocks = sum(i.blocks for i in infos)
print(f"set-up {time.perf_counter() - t0:.0f} s: {n} x {secs} s stereo {bd}/{sr / 1000:g} music, {total_blocks} blocks, "
      f"{sum(map(len, lacs)) / 1e6:.0f} MB .lac; {nw} windows of {T} frames need {win_blocks} blocks, "
      f"{win_bytes / 1e6:.0f} MB of payload")

want = torch.from_numpy(np.stack([pcm[s][:, st:st + T] for s, st in zip(song, start)]).astype(np.int32))  # [nw, 2, T]
want_f32 = want.to(torch.float32) / 2 ** (bd - 1)
dec = lacx.Decoder(device=0)
dev = torch.device("cuda")
win_i32 = torch.empty((nw, 2, T), dtype=torch.int32, device=dev)
win_f32 = torch.empty((nw, 2, T), dtype=torch.float32, device=dev)
lacs_w = [lacs[s] for s in song]
starts_w = [int(x) for x in start]


def outputs(t):
    return [(t[i, 0].data_ptr(), t[i, 1].data_ptr()) for i in range(nw)]


out_i32, out_f32 = outputs(win_i32), outputs(win_f32)
bufs = [np.frombuffer(x, dtype=np.uint8) for x in lacs]
u8 = C.POINTER(C.c_uint8)


def window_items(out):
    items = (lacx.WindowItem * nw)()
    for it, s, st, (lp, rp) in zip(items, song, start, out):
        it.lac, it.size, it.start, it.frames, it.left, it.right = bufs[s].ctypes.data_as(u8), bufs[s].size, int(st), T, lp, rp
    return items


items_i32, items_f32 = window_items(out_i32), window_items(out_f32)
L = lacx.lib()
ms = C.c_float()
off = np.concatenate([[0], np.cumsum(frames)])
whole_l = torch.empty(int(off[-1]), dtype=torch.int32, device=dev)
whole_r = torch.empty(int(off[-1]), dtype=torch.int32, device=dev)
whole_items = (lacx.DecodeItem * n)()
for k, it in enumerate(whole_items):
    it.lac, it.size, it.frames = bufs[k].ctypes.data_as(u8), bufs[k].size, int(frames[k])
    it.left, it.right = whole_l[off[k]:].data_ptr(), whole_r[off[k]:].data_ptr()
gather_idx = (torch.from_numpy(off[song] + start)[:, None] + torch.arange(T)[None, :]).to(dev)  # [nw, T]
sliced = torch.empty((nw, 2, T), dtype=torch.int32, device=dev)


def check(got, ref, what):
    g = got.cpu()
    ok = torch.equal(g.view(torch.int32), ref.view(torch.int32))  # float32 compared by its bits
    if not ok:
        bad = (g.view(torch.int32) != ref.view(torch.int32)).reshape(nw, -1).any(1).nonzero().flatten().tolist()
        raise SystemExit(f"{what}: windows {bad[:10]} differ from the input")


res = {k: [] for k in ("k_i32", "w_i32", "k_f32", "w_f32", "k_whole", "w_whole", "w_py")}
for it in range(iters + 1):  # the first round is the warm-up
    for key, items, t_out in (("i32", items_i32, win_i32), ("f32", items_f32, win_f32)):
        t_out.fill_(-1)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        rc = L.lacx_decoder_decode_window_batch_device(dec._h, items, nw, lacx.SAMPLE_I32 if key == "i32" else lacx.SAMPLE_F32,
                                                       None, None, C.byref(ms))
        t2 = time.perf_counter()
        assert rc == lacx.OK, L.lacx_decode_last_error()
        res["k_" + key].append(ms.value)
        res["w_" + key].append((t2 - t1) * 1e3)
        if it == 0:
            check(t_out, want if key == "i32" else want_f32, "window " + key)
    win_i32.fill_(-1)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    dec.decode_window_batch_device(lacs_w, starts_w, T, out_i32)
    res["w_py"].append((time.perf_counter() - t1) * 1e3)
    if it == 0:
        check(win_i32, want, "window int32 (Python)")
    sliced.fill_(-1)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    rc = L.lacx_decoder_decode_batch_device(dec._h, whole_items, n, None, None, C.byref(ms))
    sliced[:, 0] = whole_l[gather_idx]
    sliced[:, 1] = whole_r[gather_idx]
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    assert rc == lacx.OK, L.lacx_decode_last_error()
    res["k_whole"].append(ms.value)
    res["w_whole"].append((t2 - t1) * 1e3)
    if it == 0:
        check(sliced, want, "whole + slice")
        for v in res.values():
            v.clear()

best = {k: float(np.min(v)) for k, v in res.items()}
med = {k: float(np.median(v)) for k, v in res.items()}
print(f"{iters} rounds after warm-up, best / median; every window of both forms equals its input PCM")
print(f"  kernels  windows int32 {best['k_i32']:.2f} / {med['k_i32']:.2f} ms   float32 {best['k_f32']:.2f} / {med['k_f32']:.2f} ms"
      f"   whole streams {best['k_whole']:.2f} / {med['k_whole']:.2f} ms")
print(f"  wall     decode_window_batch_device int32 {best['w_i32']:.1f} / {med['w_i32']:.1f} ms   float32 "
      f"{best['w_f32']:.1f} / {med['w_f32']:.1f} ms   decode_batch_device + slicing {best['w_whole']:.1f} / "
      f"{med['w_whole']:.1f} ms   speed-up {med['w_whole'] / med['w_i32']:.1f}x")
print(f"  wall     Decoder.decode_window_batch_device int32 (binding included) {best['w_py']:.1f} / {med['w_py']:.1f} ms")
