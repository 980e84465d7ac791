"""Measurement (not part of the default suite, nothing here is a gate): a batch of .lac streams recompressed as one
transcode job against the same work chained by hand through torch tensors.
  transcode   Decoder.transcode_batch: the window job into the int32 staging, k_edit, the PCM digest, the batch encode and
              lacx_assemble, PCM on the device throughout (verify=True adds the decode of every new stream)
  chained     Decoder.decode_batch_device into planar int32 torch tensors, BatchEncoder.encode_device over them, assemble:
              what a caller could do before, without transforms, digest or verification
Workload: the 48-song batch of scripts/decode_batch_bench.py (48 x 240 s stereo 16/44.1 synthetic music, seeds 5000..),
encoded on the GPU with partitioning off, so that the recompression has something to gain.  A warm-up round, then `iters`
rounds with the routes alternating inside every round: wall ms (all routes end synchronised), the kernel ms the decoder
reports (phase 1, and the verification where it runs) and the encoder's own (lacx_timing), best and median; the spread of
the identical repeats is the min..max printed beside them.
usage: transcode_bench.py [iters] [songs] [song seconds]"""
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
    raise SystemExit("transcode_bench needs a HIP device")
RATE, DEPTH = 44100, 16

src_enc = lacx.Encoder(12, 2, RATE, DEPTH, device=0)
src_enc.set_partitioning_enabled(False)
with ThreadPoolExecutor(16) as ex:  # numpy releases the GIL inside the generator's arithmetic
    lacs = [src_enc.encode(l, r) for l, r in ex.map(lambda k: synth.synth_pcm(song_secs * RATE, 2, DEPTH, RATE, seed=5000 + k, kind="music"), range(songs))]
del src_enc
infos = [lacx.stream_parse(x) for x in lacs]
frames = sum(i.frames for i in infos)
print(f"batch of {songs} songs 16/44.1 music, coded without partitioning: {sum(map(len, lacs)) / 1e6:.0f} MB .lac, {sum(i.blocks for i in infos)} blocks, "
      f"{frames * 4 / 1e6:.0f} MB of 16-bit PCM")

dec = lacx.Decoder(device=0)
enc = lacx.Encoder(12, 2, RATE, DEPTH, device=0)
batch = lacx.BatchEncoder([(RATE, DEPTH, 2)] * songs, device=0)
tensors = [(torch.empty(i.frames, dtype=torch.int32, device="cuda"), torch.empty(i.frames, dtype=torch.int32, device="cuda")) for i in infos]
res = {k: [] for k in ("w_trans", "k_trans", "e_trans", "w_verify", "k_verify", "w_chain", "k_chain", "e_chain")}
first = None
for it in range(iters + 1):  # the first round is the warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    got = dec.transcode_batch(enc, [([x],) for x in lacs])
    t1 = time.perf_counter()
    k_t, e_t = dec.last_ms, enc.timing().analysis_ms + enc.timing().emit_ms
    checked = dec.transcode_batch(enc, [([x],) for x in lacs], verify=True)
    t2 = time.perf_counter()
    k_v = dec.last_ms
    dec.decode_batch_device(lacs, [(l.data_ptr(), r.data_ptr()) for l, r in tensors])
    k_c = dec.last_ms
    outs = batch.encode_device([(l.data_ptr(), 0, 2, l.numel(), r.data_ptr()) for l, r in tensors])
    chained = [lacx.assemble(RATE, DEPTH, 2, 2, [(p.tobytes(), t.copy())]) for p, t in outs]
    t3 = time.perf_counter()
    e_c = batch.timing().analysis_ms + batch.timing().emit_ms
    if it == 0:
        first = got
        assert [g[0] for g in got] == [g[0] for g in checked] == chained and all(r.verified for _, r in checked)
    else:
        for k, v in (("w_trans", (t1 - t0) * 1e3), ("k_trans", k_t), ("e_trans", e_t), ("w_verify", (t2 - t1) * 1e3), ("k_verify", k_v),
                     ("w_chain", (t3 - t2) * 1e3), ("k_chain", k_c), ("e_chain", e_c)):
            res[k].append(v)


def line(key):
    v = res[key]
    return f"best {np.min(v):.2f} median {np.median(v):.2f} ms (min..max {np.min(v):.2f}..{np.max(v):.2f})"


new = sum(len(g[0]) for g in first)
print(f"  recompressed: {sum(map(len, lacs))} -> {new} bytes ({100 * new / sum(map(len, lacs)):.2f} %), the three routes give the same files")
print(f"  {iters} rounds after warm-up, routes alternating inside a round")
print(f"  transcode_batch               wall {line('w_trans')}   decoder kernels (windows + k_edit + digest) {line('k_trans')}   encoder kernels {line('e_trans')}")
print(f"  transcode_batch, verify=True  wall {line('w_verify')}   decoder kernels (the same + decode and compare) {line('k_verify')}")
print(f"  decode_batch_device + encode_device + assemble   wall {line('w_chain')}   decoder kernels {line('k_chain')}   encoder kernels {line('e_chain')}")
