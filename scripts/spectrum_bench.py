"""Measurement (not part of the default suite): what the spectrum costs against what a user has without it.
  spectrum  Decoder.spectrum_batch: decode, the in-place mid/side inverse and k_spectrum; 1024 bytes per 16384 frames come back
  torch     the status quo on the device: Decoder.decode_batch_device into torch tensors, then per item torch.stft in float64
            with the same periodic Hann window and hop (the item padded with zeros behind its end), |X|^2 and the band sums
  alone     Decoder.spectrum_pcm_batch over the decoded tensors: k_spectrum alone, no decode in front
Workloads: the 48-song batch of profiles/decode_batch_bench.txt (48 x 240 s stereo 16/44.1 synthetic music, distinct seeds) and
one 10-minute stream, each at N = 2048 and N = 256, all encoded on the GPU.  Per workload and window length a warm-up round,
then `iters` rounds with the routes alternating inside every round: wall ms of each (all end synchronised) and the kernel ms
the library reports.  The band powers of the routes are checked to agree to 1e-9 of each item's total.
Without a HIP device nothing is measured, and the script says so.
usage: spectrum_bench.py [iters] [songs] [song seconds]"""
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
import spectwin as st  # noqa: E402

pkg = ge.load_pkg()
lacx, synth = pkg.lacx, pkg.synth
iters = int(sys.argv[1]) if len(sys.argv) > 1 else 3
songs = int(sys.argv[2]) if len(sys.argv) > 2 else 48
song_secs = int(sys.argv[3]) if len(sys.argv) > 3 else 240
if lacx.device_count() < 1:
    raise SystemExit("not measured yet: spectrum_bench needs a HIP device")


def torch_route(dec, lacs, outs, window):
    """decode_batch_device, then torch.stft in float64 and the band sums per item: (items, 2, 64) total band powers."""
    dec.decode_batch_device(lacs, [(o[0].data_ptr(), o[1].data_ptr()) for o in outs])
    hop, per = window // 2, window // 128
    w = torch.hann_window(window, periodic=True, dtype=torch.float64, device="cuda")
    bands = []
    for o in outs:
        frames = o.shape[1]
        nw = -(-frames // hop)
        x = torch.nn.functional.pad(o.to(torch.float64), (0, (nw - 1) * hop + window - frames))
        z = torch.stft(x, window, hop_length=hop, window=w, center=False, onesided=True, return_complex=True)  # (2, N / 2 + 1, nw)
        p = (z.real * z.real + z.imag * z.imag).sum(dim=2)
        p[:, 1:-1] *= 2.0
        b = p[:, :-1].reshape(2, 64, per).sum(dim=2)
        b[:, 63] += p[:, -1]
        bands.append(b)
    return torch.stack(bands).cpu().numpy()  # (the copy synchronises)


def totals(results):
    return np.stack([st.rows_of(rows)["power"].sum(axis=0) for _, rows in results])


def workload(name, n, secs, rate, depth, seed0):
    t0 = time.perf_counter()
    enc = lacx.Encoder(12, 2, rate, depth, device=0)
    lacs = []
    with ThreadPoolExecutor(16) as ex:  # numpy releases the GIL inside the generator's arithmetic
        for left, right in ex.map(lambda k: synth.synth_pcm(secs * rate, 2, depth, rate, seed=seed0 + k, kind="music"), range(n)):
            lacs.append(enc.encode(left, right))
    infos = [lacx.stream_parse(x) for x in lacs]
    frames = sum(i.frames for i in infos)
    print(f"{name}: {n} x {secs} s stereo {depth}/{rate / 1000:g} music, {sum(map(len, lacs)) / 1e6:.0f} MB .lac (set-up {time.perf_counter() - t0:.0f} s)")
    dec = lacx.Decoder(device=0)
    outs = [torch.empty((2, i.frames), dtype=torch.int32, device="cuda") for i in infos]
    for window in (2048, 256):
        res = {k: [] for k in ("w_spec", "k_spec", "w_torch", "w_alone", "k_alone")}
        spec = ref = alone = None
        for it in range(iters + 1):  # the first round is the warm-up
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            spec = dec.spectrum_batch(lacs, window)
            t2 = time.perf_counter()
            k_s = dec.last_ms
            ref = torch_route(dec, lacs, outs, window)
            t3 = time.perf_counter()
            alone = dec.spectrum_pcm_batch([(o, rate, depth) for o in outs], window)
            t4 = time.perf_counter()
            k_a = dec.last_ms
            if it:
                for k, v in (("w_spec", (t2 - t1) * 1e3), ("k_spec", k_s), ("w_torch", (t3 - t2) * 1e3), ("w_alone", (t4 - t3) * 1e3), ("k_alone", k_a)):
                    res[k].append(v)
        got, own = totals(spec), totals(alone)
        assert got.tobytes() == own.tobytes(), "stream form and source form differ"
        worst = float(np.max(np.abs(got - ref) / ref.sum(axis=2, keepdims=True)))
        assert worst < 1e-9, "the routes differ: %g" % worst

        def line(key):
            v = res[key]
            return f"{np.median(v):.2f} ms (min..max {np.min(v):.2f}..{np.max(v):.2f})"

        pcm, nw = 8 * frames, sum(int(s.windows) for s, _ in spec)
        print(f"  N = {window}: {iters} rounds after warm-up, routes alternating inside a round; medians; band powers agree to {worst:.1e} of an item's total")
        print(f"    spectrum_batch        wall {line('w_spec')}   kernels (decode + k_ms_inverse + k_spectrum) {line('k_spec')}")
        print(f"    decode + torch.stft   wall {line('w_torch')}   (float64, the same window and hop, band sums on the device)")
        print(f"    spectrum_pcm_batch    wall {line('w_alone')}   k_spectrum alone {line('k_alone')} for {pcm / 1e9:.2f} GB of PCM, {nw} windows: "
              f"{pcm / 1e6 / np.median(res['k_alone']):.0f} GB/s, {nw / 1e3 / np.median(res['k_alone']):.2f} M windows/s; "
              f"{1024 * sum(len(r) for _, r in spec)} B of rows cross PCIe")
        print("    bandwidth Hz / peak Hz of the first items:", " ".join("%.0f/%.0f" % (s.bandwidth_hz[0], s.peak_hz(0)) for s, _ in spec[:4]))
    dec.close()


workload("batch", songs, song_secs, 44100, 16, 5000)
workload("one stream", 1, 600, 44100, 16, 7000)
