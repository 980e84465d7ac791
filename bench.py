#!/usr/bin/env python3
"""bench.py -- encode throughput of the MI355X LAC block-encode path (BASELINE.json metric).

A "step" is one whole-job encode of the rank's shard with the PCM already resident in HBM in its source
layout (interleaved int16, the WAV data chunk): ingest + Levinson + probe/whole-block analysis kernels,
device-side bit emit straight into pinned host memory, block table D2H -> shard payload + block table on the
host.  For N > 1 the ranks then all_gather (payload bytes, block count) over RCCL -- the path's only exchange
step -- so every rank knows its byte offset in the final .lac.

Workloads:
  N = 1   BASELINE configs[1]: 10 min synthetic stereo 16-bit 48 kHz, per-block auto MS/LR, LPC search, 16384-frame
          blocks.  With --full the last timed step's .lac is compared byte for byte with the CPU reference's and with
          the golden digest.
  N > 1   BASELINE configs[3]: ONE 2 h stereo 16/48 stream (345 600 000 frames, 21 094 blocks); rank r encodes blocks
          [r*B/N, (r+1)*B/N) (strong split of a fixed stream, no data-path collective).  With --full, after the timed
          loop every rank checks each eighth of its shard against the golden digests minted from the reference
          (tests/golden/digests.json, cfg4_2h_shard{1..8}of8) -> "byte_identical_shards": "N/N", and the same ranks then
          also time the weak line (10 min per GPU) -> "weak_10min_per_gpu".

A plain run (no --full) does only what the headline figure needs: set-up, warm-up, the --steps timed steps, the outputs
of the last step when --dump-outputs is given, and the JSON line.  --full adds everything else the line can carry: the
digest and CPU-reference checks, the CPU baseline, the end-to-end and decode figures, the other BASELINE workloads and,
at N > 1, the weak lines and the single-process fan-out line.

--dump-outputs DIR writes what the timed path returned in its last step (the shard's block table and payload bytes, see
dump_outputs) as DIR/<name>.npy; the inputs are seeded, so two builds run with the same arguments can be compared
output for output.

`python bench.py --gpus N` with no WORLD_SIZE in the environment starts the N ranks itself (a child
`python -m torch.distributed.run`, started before this process touches any GPU), relays rank 0's JSON line and exits
non-zero when a rank fails.  With fewer visible GPUs than ranks the ranks share the GPUs and exchange over gloo: a
rehearsal of the code path ("rehearsal_shared_gpu": true), not a measurement.

Prints ONE JSON line on rank 0.
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

STEREO_MODE = 2
BLOCK = 16384
HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: 8.0 TB/s spec
VALU_LANE_OPS_PER_S = 256 * 4 * 32 * 2.4e9  # 256 CUs x 4 SIMD-32 x 2.4 GHz: one wave64 VALU instruction = 2 cycles
CFG2_SECONDS = 600
CFG4_SECONDS = 7200
METRIC = "encode Msamples/s at 1/2/4/8 MI355X; byte-identical .lac vs CPU ref"


KERNEL_SOURCES = ("k_analyze.hip", "device_util.h", "emit_device.h", "analyze_core.h", "emit_core.h")  # the dominant kernel's sources: what the committed counter passes were measured on


def kernel_source_sha256() -> str:
    """sha256 over the sources of the dominant kernel, in a fixed order: profiles/valu.json and profiles/traffic.json carry
    the value they were measured at (scripts/summarize_counters.py), and the bench line only quotes them for these sources."""
    h = hashlib.sha256()
    for name in KERNEL_SOURCES:
        with open(os.path.join(ROOT, "lossless-audio-codec_amd", "csrc", name), "rb") as f:
            h.update(f.read())
    return h.hexdigest()


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--workload", default="auto", choices=("auto", "cfg2", "cfg4"),
                    help="auto: configs[1] (10 min per GPU) at N=1, configs[3] (one 2 h stream, block-range split) at N>1")
    ap.add_argument("--seconds", type=int, default=0, help="diagnostic: audio seconds per GPU instead of the named config")
    ap.add_argument("--kind", default="music")
    ap.add_argument("--bit-depth", type=int, default=16, choices=(16, 24), help="diagnostic: other BASELINE configs")
    ap.add_argument("--rate", type=int, default=48000, choices=(44100, 48000, 96000, 192000))
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-weak-line", action="store_true", help="N>1: skip the additional 10 min per GPU measurement")
    ap.add_argument("--no-fanout-line", action="store_true",
                    help="N>1: skip rank 0's measurement of the library's own single-process fan-out over all N devices")
    ap.add_argument("--no-end-to-end", action="store_true", help="N=1: skip the host WAV -> host .lac measurement")
    ap.add_argument("--no-decode-check", action="store_true", help="N=1: skip decoding the GPU's .lac on the device")
    ap.add_argument("--no-other-workloads", action="store_true",
                    help="N=1: skip the verified extra workloads (configs[2] at full size, white noise, configs[4] as one job)")
    ap.add_argument("--analysis-only", action="store_true", help="time the device analysis alone (diagnostic)")
    ap.add_argument("--host-emit", action="store_true", help="keep the bit emit on the host (north_star layout)")
    ap.add_argument("--planar", action="store_true", help="planar int32 device input (the reference API layout) instead of interleaved int16")
    ap.add_argument("--fanout", action="store_true",
                    help="one process drives all --gpus devices through the library's own fan-out (lacx_encoder_create_multi: one host "
                         "thread + stream set per device, RCCL exchange of the shard sizes) instead of one torchrun rank per GPU")
    ap.add_argument("--inflight", type=int, default=1, choices=(1, 2),
                    help="diagnostic: 2 = step i+1 is enqueued on a second encoder before step i's result is collected")
    ap.add_argument("--full", action="store_true",
                    help="also run the checks and extra measurements beyond the headline figure (digest and CPU-reference checks, "
                         "CPU baseline, end to end, device decode, other workloads; at N>1 the weak and fan-out lines); the "
                         "--no-* options above select among them")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's outputs as DIR/<name>.npy (float32/float64, at most 64 MB in all)")
    return ap.parse_args(argv)


# ---------------------------------------------------------------------------------------------------------
# inputs and outputs
# ---------------------------------------------------------------------------------------------------------
def synth_pcm_parallel(synth, frames, channels, bit_depth, sample_rate, seed, kind, stereo="wide", start=0, threads=16,
                       piece=1 << 20):
    """synth.synth_pcm in pieces on a thread pool.  The generator is counter based (every frame is a function of its own
    index), so the pieces are the same samples as one serial call; numpy releases the GIL inside the piece's arithmetic."""
    import numpy as np
    from concurrent.futures import ThreadPoolExecutor

    left = np.empty(frames, dtype=np.int32)
    right = np.empty(frames, dtype=np.int32) if channels == 2 else None

    def one(p0):
        m = min(piece, frames - p0)
        l_, r_ = synth.synth_pcm(m, channels, bit_depth, sample_rate, seed=seed, kind=kind, stereo=stereo, start=start + p0)
        left[p0:p0 + m] = l_
        if right is not None:
            right[p0:p0 + m] = r_

    with ThreadPoolExecutor(max(1, threads)) as ex:
        list(ex.map(one, range(0, frames, piece)))
    return left, right


def cpu_share() -> int:
    """Host threads for one process: the cores it may run on (affinity mask, cgroup quota), at most 16."""
    cores = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    quota = cgroup_cpu_quota()
    return max(1, min(16, cores, quota or cores))


DUMP_BUDGET_BYTES = 64 << 20
DUMP_PAYLOAD_SAMPLE = 8 << 20  # payload bytes kept when the payload is larger (float32: 32 MB)
DUMP_SEED = 2026


def dump_outputs(out_dir, payload: bytes, table, suffix="", share=1):
    """What a caller of the timed path receives from its last step, as .npy files under out_dir:
      block_table<suffix>.npy     the shard's block table (uint32 [blocks, 2]) as float64 -- exact
      payload_sample<suffix>.npy  the payload bytes as float32 -- all of them up to DUMP_PAYLOAD_SAMPLE / share bytes,
                                  beyond that the bytes at the sorted positions numpy.random.default_rng(DUMP_SEED)
                                  .integers(0, len(payload), DUMP_PAYLOAD_SAMPLE / share) draws (a fixed, seeded sample)
    share: the number of processes writing into out_dir (ranks), which split the 64 MB between them."""
    import numpy as np

    os.makedirs(out_dir, exist_ok=True)
    tab = np.asarray(table, dtype=np.uint32).astype(np.float64)
    pay = np.frombuffer(payload, dtype=np.uint8)
    n = DUMP_PAYLOAD_SAMPLE // max(1, share)
    if pay.size > n:
        pos = np.sort(np.random.default_rng(DUMP_SEED).integers(0, pay.size, n))
        pay = pay[pos]
    sample = pay.astype(np.float32)
    assert tab.nbytes + sample.nbytes <= DUMP_BUDGET_BYTES // max(1, share)
    np.save(os.path.join(out_dir, f"block_table{suffix}.npy"), tab)
    np.save(os.path.join(out_dir, f"payload_sample{suffix}.npy"), sample)


# ---------------------------------------------------------------------------------------------------------
# launcher: no GPU call may happen in this process
# ---------------------------------------------------------------------------------------------------------
def launch_ranks(args) -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", "4")
    proc = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True)
    line = None
    for ln in proc.stdout.splitlines():
        ln = ln.strip()
        if ln.startswith("{") and ln.endswith("}"):
            try:
                json.loads(ln)
                line = ln
            except ValueError:
                pass
    if proc.returncode != 0:
        sys.stderr.write(f"bench.py: a rank failed (torch.distributed.run exit code {proc.returncode})\n")
        sys.stderr.write(proc.stdout[-4000:])
        return proc.returncode or 1
    if line is None:
        sys.stderr.write("bench.py: the ranks finished without a JSON line\n" + proc.stdout[-4000:])
        return 1
    print(line)
    return 0




import contextlib


@contextlib.contextmanager
def no_gc():
    """Python's cyclic garbage collector kept out of a timed loop (see StepLog.__enter__)."""
    import gc
    gc.collect()
    was = gc.isenabled()
    gc.disable()
    try:
        yield
    finally:
        if was:
            gc.enable()


class StepLog:
    """Per-step record of a timed loop, so that a slow step explains itself: the Python-side wall clock of the step, the
    library's own clock of the call, the device timeline, what the packer / repair kernels did, how attentive the host
    thread was to the payload drain, and the time Python's garbage collector took inside the step."""
    KEYS = ("wall_ms", "lib_total_ms", "analysis_ms", "full_ms", "enqueue_ms", "kernels_done_ms", "drain_first_ms", "drain_last_ms",
            "poll_gap_max_ms", "drain_copies", "emit_direct", "moved_by_k_pack", "packer_gave_up", "gc_ms")

    def __init__(self):
        import gc
        self.rows = {k: [] for k in self.KEYS}
        self._raw = []
        self._gc_t0 = None
        self._gc_ms = 0.0
        self._gc = gc

        def cb(phase, info):
            if phase == "start":
                self._gc_t0 = time.perf_counter()
            elif self._gc_t0 is not None:
                self._gc_ms += (time.perf_counter() - self._gc_t0) * 1e3
                self._gc_t0 = None
        self._cb = cb

    def __enter__(self):
        # Round 3's driver run had one 18 ms step among 4.5 ms ones; the per-step record then caught the same thing in the
        # act: a step whose library clock read 6.4 ms took 15.0 ms of wall clock with 8.5 ms of it inside Python's cyclic
        # garbage collector (a full collection over the interpreter's ~10^6 objects once torch is imported, triggered by
        # the allocation counters wherever they happen to trip).  That is the harness, not the encode: collect once before
        # the timed loop and keep the collector off inside it (the callback still reports any collection that does run).
        self._gc.collect()
        self._gc_was_enabled = self._gc.isenabled()
        self._gc.disable()
        self._gc.callbacks.append(self._cb)
        return self

    def __exit__(self, *a):
        self._gc.callbacks.remove(self._cb)
        if self._gc_was_enabled:
            self._gc.enable()

    def begin(self):
        self._gc_ms = 0.0
        self._t = time.perf_counter()

    def end(self, timings):
        """timings: the lacx_timing of every encoder call the step made.  Only the clock and the references are taken
        here (the step is inside a timed region); the fields are worked out in summary()."""
        now = time.perf_counter()
        self._raw.append((now - self._t, self._gc_ms, timings))

    def _digest(self):
        r = self.rows
        for wall, gc_ms, timings in self._raw:
            r["wall_ms"].append(round(wall * 1e3, 3))
            r["gc_ms"].append(round(gc_ms, 3))
            add = lambda f: round(sum(getattr(t, f) for t in timings), 3)  # noqa: E731
            mx = lambda f: round(max(getattr(t, f) for t in timings), 3)  # noqa: E731
            r["lib_total_ms"].append(mx("total_ms"))
            r["analysis_ms"].append(add("analysis_ms"))
            r["full_ms"].append(add("full_ms"))
            r["enqueue_ms"].append(mx("enqueue_ms"))
            r["kernels_done_ms"].append(mx("kernels_done_ms"))
            r["drain_first_ms"].append(mx("drain_first_ms"))
            r["drain_last_ms"].append(mx("drain_last_ms"))
            r["poll_gap_max_ms"].append(mx("poll_gap_max_ms"))
            r["drain_copies"].append(int(sum(t.drain_copies for t in timings)))
            r["emit_direct"].append(int(sum(t.emit_direct for t in timings)))
            r["moved_by_k_pack"].append(int(sum(t.moved_by_k_pack for t in timings)))
            r["packer_gave_up"].append(int(sum(t.packer_gave_up for t in timings)))
        self._raw = []

    def summary(self):
        import statistics
        self._digest()
        out = {}
        for k, v in self.rows.items():
            if not v:
                continue
            out[k] = {"median": round(statistics.median(v), 3), "max": max(v), "each": v}
        w = self.rows["wall_ms"]
        if w:
            med = statistics.median(w)
            slow = [i for i, x in enumerate(w) if x > 1.5 * med]
            out["slow_steps"] = [{"step": i, **{k: self.rows[k][i] for k in self.KEYS}} for i in slow]
        return out

# ---------------------------------------------------------------------------------------------------------
# the library's own multi-device fan-out, driven from ONE process (lacx_encoder_create_multi)
# ---------------------------------------------------------------------------------------------------------
def fanout_job(lacx, synth, torch, np, devices, left, right, total_frames, bit_depth, sample_rate, steps, warmup, gen=None):
    """Times `steps` encodes of one stream spread over `devices` by the library itself: lane g's block range resident on
    devices[g] in WAV layout, one lacx_encode_fanout_resident call per step (every lane encodes its shard into its pinned
    result region, the lanes exchange their sizes).  left/right: the stream's PCM, or None with gen = (kind, seed) to have
    every lane's range generated on its own.  Returns the figures and the last step's assembled .lac."""
    G = len(devices)
    nb = (total_frames + BLOCK - 1) // BLOCK
    enc = lacx.Encoder(12, STEREO_MODE, sample_rate, bit_depth, devices=devices)
    layout = lacx.PCM_INTERLEAVED_I16 if bit_depth == 16 else lacx.PCM_INTERLEAVED_I24
    shards, keep = [], []
    for g, dev in enumerate(devices):
        b0, cnt = lacx.fanout_range(nb, G, g)
        f0, f1 = b0 * BLOCK, min(total_frames, (b0 + cnt) * BLOCK)
        if left is not None:
            l_, r_ = left[f0:f1], right[f0:f1]
        else:
            l_, r_ = synth_pcm_parallel(synth, f1 - f0, 2, bit_depth, sample_rate, gen[1], gen[0], start=f0, threads=cpu_share())
        inter = synth.interleave(l_, r_, bit_depth)
        d = torch.from_numpy(inter.view(np.int16) if bit_depth == 16 else inter).to(f"cuda:{dev}")
        del inter, l_, r_
        keep.append(d)
        shards.append((d.data_ptr(), layout, 2, f1 - f0))

    def sync_all():
        for dev in sorted(set(devices)):
            torch.cuda.synchronize(dev)

    sync_all()
    res = None
    for _ in range(warmup):
        res = enc.encode_fanout_resident(shards)
    sync_all()
    each, exch, conc, lane_ms = [], [], [], []
    with no_gc():
        t0 = time.perf_counter()
        for _ in range(steps):
            t1 = time.perf_counter()
            res = enc.encode_fanout_resident(shards)
            each.append(round((time.perf_counter() - t1) * 1e3, 3))
            st = enc.fanout_stats()
            exch.append(st.exchange_ms)
            lane_ms.append([round(st.encode_ms[g], 3) for g in range(st.lanes_used)])
        sync_all()
        elapsed = time.perf_counter() - t0
    st = enc.fanout_stats()
    gave_up = sum(enc.lane_timing(g).packer_gave_up for g in range(st.lanes_used))
    parts = [(p.tobytes(), np.array(t, dtype=np.uint32)) for p, t, _, _ in res]
    offsets_ok = all(res[g][3] == sum(len(parts[k][0]) for k in range(g)) for g in range(G))
    out = {
        "value": round(total_frames * 2 * steps / elapsed / 1e6, 3), "unit": "Msamples/s",
        "ms_per_step": round(elapsed / steps * 1e3, 3), "ms_each_step": each, "steps": steps,
        "devices": list(devices), "lanes_used": int(st.lanes_used),
        "exchange": "rccl all_gather (ncclCommInitAll, one communicator per lane)" if st.exchange == lacx.EXCHANGE_RCCL else "host sum",
        "exchange_note": enc.fanout_exchange_note(),
        "exchange_ms_incl_wait_for_slowest_lane": round(float(np.median(exch)), 3),
        "lane_encode_ms_last_step": lane_ms[-1] if lane_ms else None,
        "blocks_per_lane": [int(st.blocks[g]) for g in range(st.lanes_used)],
        "packer_gave_up": int(gave_up), "byte_offsets_consistent": bool(offsets_ok),
    }
    return out, parts, enc


def fanout_single_process(args) -> int:
    """`bench.py --gpus N --fanout`: the same JSON keys as the torchrun mode, measured through the library's own fan-out."""
    import numpy as np
    import torch

    import __graft_entry__ as ge

    pkg = ge.load_pkg()
    lacx, synth = pkg.lacx, pkg.synth
    ndev = torch.cuda.device_count()
    if ndev < 1:
        raise SystemExit("bench.py needs a HIP device (the LAC analysis path has no CPU fallback)")
    N = args.gpus
    rehearse = ndev < N
    devices = [g % ndev for g in range(N)]
    digests = load_digests()
    bit_depth, sample_rate = args.bit_depth, args.rate
    std_format = bit_depth == 16 and sample_rate == 48000 and args.kind == "music"
    workload = args.workload if args.workload != "auto" else ("cfg2" if N == 1 else "cfg4")
    if args.seconds:
        total_frames, wl_name = args.seconds * sample_rate * N, f"{args.seconds} s per device (diagnostic)"
    elif workload == "cfg2":
        total_frames, wl_name = CFG2_SECONDS * sample_rate, "BASELINE configs[1]: one 10 min stream"
    else:
        total_frames, wl_name = CFG4_SECONDS * sample_rate, "BASELINE configs[3]: one 2 h stream, contiguous block-range split over the devices"
    main, parts, enc = fanout_job(lacx, synth, torch, np, devices, None, None, total_frames, bit_depth, sample_rate, args.steps, args.warmup,
                                  gen=(args.kind, 2026))
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, b"".join(p for p, _ in parts), np.concatenate([t for _, t in parts]))
    # --full: verification against the reference-minted digests: the eighths of the 2 h stream / the whole 10 min stream
    shard_ok = whole_ok = None
    total_blocks = (total_frames + BLOCK - 1) // BLOCK
    if args.full and workload == "cfg4" and not args.seconds and std_format and N in (1, 2, 4, 8):
        pay = b"".join(p for p, _ in parts)
        tab = np.concatenate([t for _, t in parts])
        good, ob, oy = 0, 0, 0
        for e in range(8):
            eb0, eb1 = e * total_blocks // 8, (e + 1) * total_blocks // 8
            t_e = tab[eb0:eb1]
            nby = int(t_e[:, 1].sum(dtype=np.int64))
            lac = lacx.assemble(sample_rate, bit_depth, STEREO_MODE, 2, [(pay[oy:oy + nby], t_e)])
            d = digests.get(f"cfg4_2h_shard{e + 1}of8_st16_48k")
            good += int(d is not None and len(lac) == d["lac_bytes"] and hashlib.sha256(lac).hexdigest() == d["lac_sha256"])
            oy += nby
        shard_ok = good
        if good != 8:
            raise SystemExit(f"bench.py --fanout: only {good}/8 eighths are byte-identical to the reference's -- refusing to report a number")
    if args.full and workload == "cfg2" and not args.seconds and std_format:
        lac = lacx.assemble(sample_rate, bit_depth, STEREO_MODE, 2, parts)
        d = digests["cfg2_10min_st16_48k_auto"]
        whole_ok = len(lac) == d["lac_bytes"] and hashlib.sha256(lac).hexdigest() == d["lac_sha256"]
        if not whole_ok:
            raise SystemExit("bench.py --fanout: the assembled .lac does not match the reference's golden digest -- refusing to report a number")
    out = {
        "metric": METRIC, "value": main["value"], "unit": "Msamples/s", "n_gpus": N, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": main["ms_per_step"], "higher_is_better": True,
        "scaling": "strong" if (workload == "cfg4" and not args.seconds) else "weak", "vs_baseline": None, "dtype": "int64",
        "data": "synthetic", "full": bool(args.full),
        "config": {
            "workload": f"{wl_name}: synthetic stereo {bit_depth}-bit {sample_rate // 1000} kHz ({args.kind}), auto MS/LR, LPC search, "
                        "16384-frame blocks, zero-run + partitioning on",
            "total_frames": int(total_frames), "total_blocks": int(total_blocks),
            "mode": "single process: the library's own fan-out (lacx_encoder_create_multi + lacx_encode_fanout_resident), one host thread + "
                    "stream set + pinned result region per device",
            "device_pcm_layout": f"interleaved int{bit_depth} (WAV data chunk), lane g's block range resident on its device",
            "timed_region": "per device: analysis + device bit emit + payload/table D2H into its pinned region; then the exchange of the "
                            "shard sizes (byte offsets)",
            "exchange_backend": main["exchange"],
        },
        "ranks_seen": main["lanes_used"],
        "rehearsal_shared_gpu": bool(rehearse),
        "byte_identical_shards": (f"{shard_ok}/8 eighths" if shard_ok is not None else None),
        "matches_golden_digest": whole_ok,
        "fanout": main,
    }
    print(json.dumps(out))
    return 0

# ---------------------------------------------------------------------------------------------------------
# one rank
# ---------------------------------------------------------------------------------------------------------
def load_digests():
    with open(os.path.join(ROOT, "tests", "golden", "digests.json")) as f:
        return {d["name"]: d for d in json.load(f)}


def worker(args) -> int:
    import numpy as np
    import torch

    import __graft_entry__ as ge

    bit_depth, sample_rate = args.bit_depth, args.rate
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    ndev = torch.cuda.device_count()  # does not initialise a device
    if ndev < 1:
        raise SystemExit("bench.py needs a HIP device (the LAC analysis path has no CPU fallback)")
    # Fewer GPUs than ranks (the one-GPU development box): ranks share the GPUs and exchange over gloo, because RCCL
    # refuses two ranks on one device.  A rehearsal of the N > 1 code path, flagged as such in the output.
    rehearse = os.environ.get("LACX_BENCH_REHEARSE_ON_ONE_GPU") == "1" or ndev < world
    device = local_rank % ndev if rehearse else local_rank
    torch.cuda.set_device(device)
    dist = None
    if world > 1:
        import torch.distributed as dist

        if rehearse:
            dist.init_process_group(backend="gloo")
        else:
            dist.init_process_group(backend="nccl", device_id=torch.device("cuda", device))
    xdev = "cpu" if rehearse else "cuda"

    pkg = ge.load_pkg()
    lacx, synth = pkg.lacx, pkg.synth
    digests = load_digests()

    # cores this process may run on (the box confines a one-GPU lease to its CPU share), not the host's total
    host_cores = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    quota = cgroup_cpu_quota()  # a CPU-time quota (cgroup cpu.max) confines the lease where the affinity mask does not
    if quota is not None:
        host_cores = max(1, min(host_cores, quota))
    host_cores_total = os.cpu_count() or host_cores
    # host threads of this rank: the box's CPU share per GPU (16), overridable for tuning
    share = max(1, host_cores // max(1, int(os.environ.get("LOCAL_WORLD_SIZE", world))))
    emit_threads = int(os.environ.get("LACX_EMIT_THREADS", "0")) or min(16, share)
    bit_depth0, sample_rate0 = bit_depth, sample_rate
    enc = enc0 = lacx.Encoder(12, STEREO_MODE, sample_rate, bit_depth, device=device)
    enc.set_thread_count(emit_threads)
    enc.set_host_emit(args.host_emit)
    stream = torch.cuda.current_stream().cuda_stream
    interleaved = not (args.planar or args.host_emit or args.analysis_only)

    def sync():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    def all_sum(x: int) -> int:
        if world == 1:
            return x
        t = torch.tensor([x], dtype=torch.int64, device=xdev)
        dist.all_reduce(t)
        return int(t.item())

    def measure(total_frames: int, tag: str, spec=None):
        """Times `steps` encodes of this rank's block range of a `total_frames` stream; contract timing.
        spec: (encoder, bit_depth, sample_rate, kind, seed) of a stream other than the command line's."""
        enc, bit_depth, sample_rate, kind, seed = spec if spec else (enc0, bit_depth0, sample_rate0, args.kind, 2026)
        layout = lacx.PCM_INTERLEAVED_I16 if bit_depth == 16 else lacx.PCM_INTERLEAVED_I24
        total_blocks = (total_frames + BLOCK - 1) // BLOCK
        b0 = rank * total_blocks // world
        b1 = (rank + 1) * total_blocks // world
        f0 = b0 * BLOCK
        frames = min(b1 * BLOCK, total_frames) - f0
        left, right = synth_pcm_parallel(synth, frames, 2, bit_depth, sample_rate, seed, kind, start=f0, threads=emit_threads)
        if interleaved:  # the WAV data-chunk layout: 2 (3) bytes per sample in HBM
            inter = synth.interleave(left, right, bit_depth)
            d_pcm = torch.from_numpy(inter.view(np.int16) if bit_depth == 16 else inter).cuda()
            del inter
        else:
            d_left = torch.from_numpy(left).cuda()
            d_right = torch.from_numpy(right).cuda()
        torch.cuda.synchronize()

        # the exchange of the shard sizes: buffers made once, outside the timed loop (a fresh tensor per step and rank is a
        # handful of allocations and fill kernels on every GPU)
        xmine = xall = xhost = None
        if world > 1:
            xhost = torch.zeros(2, dtype=torch.int64).pin_memory() if xdev == "cuda" else torch.zeros(2, dtype=torch.int64)
            xmine = torch.zeros(2, dtype=torch.int64, device=xdev)
            xall = [torch.zeros(2, dtype=torch.int64, device=xdev) for _ in range(world)]

        def step():
            if args.analysis_only:
                enc.analyze_device(d_left.data_ptr(), d_right.data_ptr(), frames, stream)
                return None
            if interleaved:
                enc.encode_shard_pcm_device_begin(d_pcm.data_ptr(), layout, 2, frames, stream)
                payload, table = enc.encode_shard_end()
            else:
                payload, table = enc.encode_shard_device_view(d_left.data_ptr(), d_right.data_ptr(), left, right, frames,
                                                              stream)
            if world > 1:
                # the block table is already on the host: sum it there, exchange two integers per rank
                xhost[0] = int(table[:, 1].sum(dtype=np.int64))
                xhost[1] = table.shape[0]
                xmine.copy_(xhost, non_blocking=True)
                dist.all_gather(xall, xmine)  # per-shard payload bytes + block counts -> byte offsets
            return payload, table

        inflight = args.inflight if (interleaved and world == 1) else 1
        if inflight == 2:
            encs2 = [enc, lacx.Encoder(12, STEREO_MODE, sample_rate, bit_depth, device=device)]

            def run2(nsteps):
                last_ = None
                for i in range(nsteps):
                    encs2[i % 2].encode_shard_pcm_device_begin(d_pcm.data_ptr(), layout, 2, frames, stream)
                    if i >= 1:
                        last_ = encs2[(i - 1) % 2].encode_shard_end()
                if nsteps:
                    last_ = encs2[(nsteps - 1) % 2].encode_shard_end()
                return last_

            run2(args.warmup)
            sync()
            t0 = time.perf_counter()
            last = run2(args.steps)
            sync()
            elapsed = time.perf_counter() - t0
            tm = enc.timing()
            rec = dict(full_ms=[tm.full_ms], analysis_ms=[tm.analysis_ms], emit_ms=[tm.emit_ms], probe_ms=[tm.probe_ms],
                       ingest_ms=[tm.ingest_ms], launches=[max(1, tm.full_launches)], api_ms=[tm.total_ms], exec_ms=[tm.full_exec_ms])
            return dict(tag=tag, total_frames=total_frames, total_blocks=total_blocks, b0=b0, b1=b1, frames=frames,
                        elapsed=elapsed, last=last, rec=rec, timing=tm, left=left, right=right, keep_alive=encs2,
                        value=total_frames * 2 * args.steps / elapsed / 1e6, ms_per_step=elapsed / args.steps * 1e3)
        for _ in range(args.warmup):
            step()
        sync()
        rec = dict(full_ms=[], analysis_ms=[], emit_ms=[], probe_ms=[], ingest_ms=[], launches=[], api_ms=[], exec_ms=[])
        last = None
        log = StepLog()
        log.__enter__()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            log.begin()
            last = step()
            t = enc.timing()
            log.end([t])
            rec["full_ms"].append(t.full_ms)
            rec["analysis_ms"].append(t.analysis_ms)
            rec["emit_ms"].append(t.emit_ms)
            rec["probe_ms"].append(t.probe_ms)
            rec["ingest_ms"].append(t.ingest_ms)
            rec["launches"].append(max(1, t.full_launches))
            rec["api_ms"].append(t.total_ms)
            rec["exec_ms"].append(t.full_exec_ms)
        sync()
        elapsed = time.perf_counter() - t0
        log.__exit__()
        rec["log"] = log.summary()
        if world > 1:
            tt = torch.tensor([elapsed], dtype=torch.float64, device=xdev)
            dist.all_reduce(tt, op=dist.ReduceOp.MAX)
            elapsed = float(tt.item())
        tm = enc.timing()
        return dict(tag=tag, total_frames=total_frames, total_blocks=total_blocks, b0=b0, b1=b1, frames=frames,
                    elapsed=elapsed, last=last, rec=rec, timing=tm, left=left, right=right,
                    value=total_frames * 2 * args.steps / elapsed / 1e6, ms_per_step=elapsed / args.steps * 1e3)

    def lac_of(payload_bytes: bytes, table, sr=sample_rate, bd=bit_depth, sm=STEREO_MODE, ch=2) -> bytes:
        return lacx.assemble(sr, bd, sm, ch, [(payload_bytes, table)])

    def digest_matches(lac: bytes, name: str) -> bool:
        d = digests.get(name)
        return d is not None and len(lac) == d["lac_bytes"] and hashlib.sha256(lac).hexdigest() == d["lac_sha256"]

    # ---- the headline measurement ----------------------------------------------------------------
    workload = args.workload
    if workload == "auto":
        workload = "cfg2" if world == 1 else "cfg4"
    std_format = bit_depth == 16 and sample_rate == 48000 and args.kind == "music"
    if args.seconds:
        total_frames, wl_name = args.seconds * sample_rate * world, f"{args.seconds} s per GPU (diagnostic)"
    elif workload == "cfg2":
        total_frames, wl_name = CFG2_SECONDS * sample_rate * world, "BASELINE configs[1]: 10 min per GPU"
    else:
        total_frames, wl_name = CFG4_SECONDS * sample_rate, "BASELINE configs[3]: one 2 h stream, contiguous block-range split over the ranks"
    main = measure(total_frames, "main")
    if args.dump_outputs:
        if main["last"] is None:
            raise SystemExit("bench.py: --dump-outputs: this timed path (--analysis-only) returns nothing to the host")
        dump_outputs(args.dump_outputs, main["last"][0].tobytes(), main["last"][1],
                     suffix=f"_rank{rank}" if world > 1 else "", share=world)

    # ---- --full: per-shard verification against the reference's golden digests (cfg4 eighths) ----
    shard_ok = None
    if (args.full and workload == "cfg4" and not args.seconds and std_format and main["last"] is not None and world in (1, 2, 4, 8)):
        payload, table = main["last"]
        pay = payload.tobytes()
        tab = np.array(table, dtype=np.uint32)
        per = 8 // world
        ok = True
        off_blocks, off_bytes = 0, 0
        for e in range(rank * per, (rank + 1) * per):
            eb0, eb1 = e * main["total_blocks"] // 8, (e + 1) * main["total_blocks"] // 8
            nbl = eb1 - eb0
            t_e = tab[off_blocks:off_blocks + nbl]
            nby = int(t_e[:, 1].sum(dtype=np.int64))
            lac = lac_of(pay[off_bytes:off_bytes + nby], t_e)
            d = digests.get(f"cfg4_2h_shard{e + 1}of8_st16_48k")
            ok = ok and d is not None and len(lac) == d["lac_bytes"] and hashlib.sha256(lac).hexdigest() == d["lac_sha256"]
            off_blocks += nbl
            off_bytes += nby
        ok = ok and off_blocks == tab.shape[0] and off_bytes == len(pay)
        shard_ok = all_sum(1 if ok else 0)
    ranks_seen = all_sum(1)

    # ---- --full, N > 1: the weak line (10 min per GPU) --------------------------------------------
    weak = weak96 = weak_pcm0 = None
    if args.full and world > 1 and workload == "cfg4" and not args.no_weak_line and not args.seconds:
        def rank0_round_trip(w, sr, bd):
            """Rank 0's shard of the weak stream as a .lac of its own, decoded on the device: the PCM must come back.  (The
            shard is not the 10 min stream of the golden digests -- block ranges are whole blocks -- so identity with the
            reference is what the strong line's per-eighth digests show; this is the product's own round trip.)"""
            if rank != 0 or w["last"] is None:
                return None
            lac = lac_of(w["last"][0].tobytes(), np.array(w["last"][1], dtype=np.uint32), sr, bd)
            dl, dr, _, _ = pkg.lacx.decode(lac)
            return bool(np.array_equal(dl, w["left"]) and np.array_equal(dr, w["right"]))

        w = measure(CFG2_SECONDS * sample_rate * world, "weak")
        weak = {"value": round(w["value"], 3), "unit": "Msamples/s", "ms_per_step": round(w["ms_per_step"], 3),
                "scaling": "weak", "workload": "10 min per GPU (BASELINE configs[1] material), rank r = r-th contiguous block range",
                "rank0_decodes_to_input": rank0_round_trip(w, sample_rate, bit_depth)}
        weak_pcm0 = (w["left"], w["right"]) if rank == 0 else None  # rank 0's range starts at frame 0 of the same stream
        del w
        # north_star: "throughput on synthetic 48 kHz / 96 kHz PCM reported at 1, 2, 4 and 8 GPUs" -- the 96 kHz line:
        # 10 min of 24-bit 96 kHz per GPU (BASELINE configs[2] material), same contiguous block-range split
        enc96 = lacx.Encoder(12, STEREO_MODE, 96000, 24, device=device)
        w = measure(CFG2_SECONDS * 96000 * world, "weak96", (enc96, 24, 96000, "mixed", 7))
        weak96 = {"value": round(w["value"], 3), "unit": "Msamples/s", "ms_per_step": round(w["ms_per_step"], 3),
                  "scaling": "weak", "workload": "10 min of stereo 24-bit 96 kHz per GPU (BASELINE configs[2] material), rank r = r-th contiguous block range",
                  "rank0_decodes_to_input": rank0_round_trip(w, 96000, 24)}
        del w, enc96
        for line in (weak, weak96):
            if rank == 0 and line["rank0_decodes_to_input"] is False:
                raise SystemExit("bench.py: rank 0's weak-line .lac does not decode back to its PCM -- refusing to report a number")

    # ---- --full, N > 1: the library's OWN fan-out, one process driving all N devices (lacx_encoder_create_multi) ------
    # Rank 0 starts `bench.py --gpus N --fanout --workload cfg2` as a CHILD process: the 10 min stream of BASELINE configs[1]
    # spread over the N devices through the C ABI (one host thread + stream set + pinned region per device, RCCL all-gather
    # of the shard sizes inside the library), its .lac checked against the reference's golden digest by the child itself.
    # The other ranks wait on the host meanwhile (a store key, no collective: a waiting RCCL kernel would sit on their CUs).
    # Outside every timed region of the lines above, and outside this process: whatever happens to the child -- a crash
    # inside a second RCCL instance, a hang (killed after 240 s) -- the headline line is still printed, with the error noted.
    fan_line = None
    if args.full and world > 1 and workload == "cfg4" and not args.no_fanout_line and not args.seconds and std_format:
        import datetime

        store = dist.distributed_c10d._get_default_store()
        if rank == 0:
            cmd = [sys.executable, os.path.abspath(__file__), "--gpus", str(world), "--fanout", "--workload", "cfg2",
                   "--steps", str(max(3, args.steps)), "--warmup", "2", "--full"]
            env = {k: v for k, v in os.environ.items()
                   if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "LOCAL_WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "GROUP_RANK",
                                "ROLE_RANK", "ROLE_WORLD_SIZE", "TORCHELASTIC_RUN_ID")}
            try:
                proc = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=240)
                lines = [ln for ln in proc.stdout.splitlines() if ln.startswith("{")]
                if proc.returncode == 0 and lines:
                    child = json.loads(lines[-1])
                    fan_line = {k: child.get(k) for k in ("value", "unit", "ms_per_step", "steps", "warmup", "n_gpus", "ranks_seen",
                                                           "rehearsal_shared_gpu", "matches_golden_digest", "fanout", "config")}
                    fan_line["workload"] = ("BASELINE configs[1] (one 10 min stereo 16/48 stream) spread over the N devices by ONE child "
                                            "process through lacx_encoder_create_multi / lacx_encode_fanout_resident (strong split; "
                                            "per-device work is 1/N of the headline's)")
                else:
                    fan_line = {"error": f"child exited with {proc.returncode}: {(proc.stderr or proc.stdout)[-400:]}"}
            except subprocess.TimeoutExpired:
                fan_line = {"error": "the fan-out child did not finish within 240 s (killed)"}
            except Exception as ex:  # noqa: BLE001 -- reported, never fatal for the headline
                fan_line = {"error": f"{type(ex).__name__}: {ex}"}
            store.set("lacx_fanout_done", "1")
            if fan_line.get("matches_golden_digest") is False:
                raise SystemExit("bench.py: the single-process fan-out's .lac differs from the reference's -- refusing to report a number")
        else:
            try:
                store.wait(["lacx_fanout_done"], datetime.timedelta(seconds=300))
            except Exception:
                pass

    if rank != 0:
        if world > 1:
            dist.destroy_process_group()
        return 0
    if shard_ok is not None and shard_ok != world:
        raise SystemExit(f"bench.py: only {shard_ok}/{world} shards are byte-identical to the reference's -- refusing to report a number")

    rec, tm, frames = main["rec"], main["timing"], main["frames"]
    mean = lambda k: float(np.mean(rec[k]))  # noqa: E731

    # ---- roofline of the dominant kernel: k_analyze<16,1024> (whole-block analysis) ----------
    # algorithmic bytes per launch = samples it analyses x bit_depth/8 (each PCM byte once)
    # + the plan records it writes (296 B per analysed channel block) + -- the bit emit being fused into this kernel --
    # the bitstream bytes it writes once.
    # The pipeline launches the kernel once per chunk: duration and bytes are per launch (averages).
    # Two live measurements of a launch: (a) hipEvents around it on its stream -- the contract's figure, used for
    # `achieved`; with the pipeline's chunks on prioritised streams it includes the time a launch queues behind /
    # shares the chip with the other chunks' kernels -- and (b) the span between the device-clock stamps of its first
    # workgroup's start and last workgroup's end, which is what rocprofv3's kernel trace measures.
    n_launch = mean("launches")
    kernel_s = mean("full_ms") / 1e3 / n_launch
    exec_s = mean("exec_ms") / 1e3 / n_launch
    fused_payload = len(main["last"][0]) if (main["last"] is not None and tm.emit_direct > 0) else 0
    algo_bytes = (frames * 2 * (bit_depth // 8) + tm.full_slots * 296 + fused_payload) / n_launch
    achieved = algo_bytes / kernel_s / 1e9 if kernel_s > 0 else 0.0
    default_run = (workload == "cfg2" and not args.seconds and world == 1 and not args.host_emit and std_format)
    # SURVEY 8(d)'s own byte definition (PCM at its source depth + plan records, nothing else), beside the figure that also
    # counts the bitstream bytes the fused emit writes
    survey_bytes = (frames * 2 * (bit_depth // 8) + tm.full_slots * 296) / n_launch
    achieved_survey = survey_bytes / kernel_s / 1e9 if kernel_s > 0 else 0.0
    # Counter-derived fields come from committed rocprofv3 --pmc passes (the profiler cannot run inside the bench); they are
    # quoted only when they were measured on THESE kernel sources (scripts/summarize_counters.py records the hash).
    src_hash = kernel_source_sha256()
    stale_profiles = False
    traffic = None
    try:  # HBM bytes per launch from the committed PMC passes
        with open(os.path.join(ROOT, "profiles", "traffic.json")) as f:
            tj = json.load(f)
        if default_run and abs(n_launch - float(tj.get("launches_per_step", 2))) < 1e-9:
            if tj.get("kernel_source_sha256") == src_hash:
                traffic = tj["traffic_bytes_per_launch"]
            else:
                stale_profiles = True
    except Exception:
        traffic = None
    valu = None
    try:  # VALU-side roofline: wave-instruction counts from the committed SQ counter passes (profiles/valu.json)
        with open(os.path.join(ROOT, "profiles", "valu.json")) as f:
            vj = json.load(f)
        if default_run and vj.get("kernel_source_sha256") != src_hash:
            stale_profiles = True
        elif default_run:
            insts = float(vj["valu_wave_insts_per_step"]) / n_launch
            valu = {
                "wave_insts_per_launch": int(insts),
                "lane_ops_per_sample": round(float(vj["valu_wave_insts_per_step"]) * 64 / (frames * 2), 1),
                # issue slots used: one wave64 VALU instruction occupies a SIMD-32 for 2 cycles
                "issue_frac": round(insts * 64 / (exec_s if exec_s > 0 else kernel_s) / VALU_LANE_OPS_PER_S, 4),
                "valu_busy_frac_counters": vj.get("valu_busy_frac"),
                "source": vj.get("source"),
            }
    except Exception:
        valu = None
    # algorithmic bytes = PCM at its source depth + the plan records; that is what `achieved` / `frac` price.
    # The fused emit makes the same kernel write the bitstream once as well: `*_incl_bitstream` adds those bytes.
    roofline = {
        "bound": "hbm",
        "kernel": "k_analyze<16,1024>",
        "achieved": round(achieved_survey, 3),
        "peak": HBM_PEAK_GBS,
        "unit": "GB/s",
        "frac": round(achieved_survey / HBM_PEAK_GBS, 6),
        "traffic": traffic,
        "traffic_ratio": (round(traffic / survey_bytes, 3) if traffic else None),
        "valu_issue_frac": (valu or {}).get("issue_frac"),
        "algorithmic_bytes": int(survey_bytes),
        "bytes_definition": "SURVEY 8(d): frames x channels x bit_depth/8 + 296 B x analysed channel blocks, per launch; "
                            "*_incl_bitstream adds the bitstream bytes the fused emit writes from the same kernel",
        "achieved_incl_bitstream": round(achieved, 3),
        "frac_incl_bitstream": round(achieved / HBM_PEAK_GBS, 6),
        "algorithmic_bytes_incl_bitstream": int(algo_bytes),
        "stale_profiles": stale_profiles,
        "kernel_source_sha256": src_hash[:16],
        "kernel_ms": round(kernel_s * 1e3, 4),
        "kernel_exec_ms": round(exec_s * 1e3, 4) if exec_s > 0 else None,
        "launches_per_step": n_launch,
        "valu": valu,
        "note": "integer-VALU-bound search (~1e3 lane-ops/sample): HBM fraction is structurally small; "
                "see DESIGN.md section 5",
    }

    # ---- --full, N = 1: CPU baseline (the unmodified reference, oracle/_ref) + byte comparison + end to end ---
    cpu = cpu_all = e2e = None
    identical = None  # set when the CPU leg encoded the whole stream: GPU bytes == CPU bytes
    digest_ok = None
    left, right = main["left"], main["right"]
    gpu_lac = None
    if args.full and world == 1 and main["last"] is not None:
        gpu_lac = lac_of(main["last"][0].tobytes(), np.array(main["last"][1], dtype=np.uint32))
        if default_run:
            d = digests["cfg2_10min_st16_48k_auto"]
            digest_ok = len(gpu_lac) == d["lac_bytes"] and hashlib.sha256(gpu_lac).hexdigest() == d["lac_sha256"]
            if not digest_ok:
                raise SystemExit("bench.py: the GPU .lac does not match the reference's golden digest -- refusing to report a number")
    if args.full and not args.no_cpu_baseline and world == 1:  # reported at N=1 only (rank 0)
        try:
            import refshim

            have_ref = refshim.available()
        except Exception:
            have_ref = False
        if have_ref:
            cpu_encode, kind = refshim.encode, "reference"
        else:
            import oracleshim

            cpu_encode, kind = oracleshim.encode, "port"
        # bounded sample: the same stream, at most the whole 10-minute config (about 20 s of CPU work over the threads)
        n_cpu = min(frames, 28_800_000)

        def cpu_leg(threads):
            t1 = time.perf_counter()
            data = cpu_encode(left[:n_cpu], right[:n_cpu], sample_rate, bit_depth, STEREO_MODE, threads=threads)
            dt = time.perf_counter() - t1
            return data, {
                "value": round(n_cpu * 2 / dt / 1e6, 3), "unit": "Msamples/s", "cores": threads, "host_cores": host_cores,
                "host_cores_total": host_cores_total, "kind": kind,
                "sample": f"first {n_cpu} frames ({n_cpu / sample_rate:.0f} s) of the same stereo {bit_depth}-bit {sample_rate} Hz stream, "
                          f"{dt:.2f} s wall, {len(data)} B .lac",
            }

        data, cpu = cpu_leg(emit_threads)  # the CPU share that belongs to one GPU on this box
        # outside every timed region: the last timed step's GPU output against the CPU encoder's, byte for byte
        if gpu_lac is not None and n_cpu == frames:
            identical = gpu_lac == data
            if not identical:
                raise SystemExit("bench.py: the GPU .lac differs from the CPU encoder's -- refusing to report a number")
        if host_cores > emit_threads:
            data2, cpu_all = cpu_leg(host_cores)  # every core this process is allowed to run on (sched_getaffinity)
            if data2 != data:
                raise SystemExit("bench.py: the CPU encoder's output depends on its thread count")
            del data2
        del data
    if args.full and world == 1 and not args.no_end_to_end and not args.analysis_only and not args.host_emit:
        # Host WAV image -> host .lac through lacx_encode_wav (RIFF walk, H2D of the raw data chunk, kernels, container):
        # the PCIe-inclusive product path (ref src/main.cpp:658-697).  Never `value`.
        import wavutil

        wav = np.frombuffer(wavutil.make_wav(left, right, sample_rate, bit_depth), dtype=np.uint8)
        enc.encode_wav_view(wav)  # warm-up (buffers)
        lib_ms, wall_ms, h2d = [], [], []
        view = None
        for _ in range(5):
            t1 = time.perf_counter()
            view = enc.encode_wav_view(wav)  # complete .lac in the encoder's pinned result buffer, no copy
            wall_ms.append((time.perf_counter() - t1) * 1e3)
            tmw = enc.timing()
            lib_ms.append(tmw.total_ms)
            h2d.append(tmw.h2d_ms)
        best = min(lib_ms)
        same = (view.tobytes() == gpu_lac) if gpu_lac is not None else None
        e2e = {"value": round(frames * 2 / (best / 1e3) / 1e6, 3), "unit": "Msamples/s", "ms": round(best, 3),
               "ms_python_wall": round(min(wall_ms), 3), "h2d_host_ms": round(min(h2d), 3),
               "path": "WAV image in pageable host memory -> lacx_encode_wav_view (RIFF walk, upload pipelined with the analysis in 3 "
                       "chunks of 1:3:4, kernels, header + table written in place) -> complete .lac in pinned host memory; ms = the library "
                       "call's own wall clock",
               "byte_identical": same}
        if same is False:
            raise SystemExit("bench.py: lacx_encode_wav_view output differs from the device-resident encode")

    decode_check = None
    if args.full and world == 1 and gpu_lac is not None and not args.no_decode_check:
        # The product's own decoder (lacx_decode, one lane per block on the device) on the last timed step's .lac: the PCM
        # must come back sample for sample.  No oracle involved; outside every timed region.
        dec = pkg.lacx.Decoder(device=device, reuse_output=True)  # (a decoder handle: buffers live from call to call)
        dl, dr, dinfo, dec_first = dec.decode(gpu_lac)  # (first call: code upload, attribute set-up, cold caches, allocations)
        same_first = bool(np.array_equal(dl, left) and np.array_equal(dr, right))
        t1 = time.perf_counter()
        dl, dr, dinfo, dec_ms = dec.decode(gpu_lac)
        wall = (time.perf_counter() - t1) * 1e3
        same_pcm = bool(same_first and np.array_equal(dl, left) and np.array_equal(dr, right))
        decode_check = {"pcm_identical": same_pcm, "kernel_ms": round(dec_ms, 3), "kernel_ms_first_call": round(dec_first, 3),
                        "wall_ms_incl_copies": round(wall, 1),
                        "value": round(frames * 2 / (dec_ms / 1e3) / 1e6, 1) if dec_ms > 0 else None, "unit": "Msamples/s",
                        "blocks": int(dinfo.blocks)}
        del dl, dr
        if not same_pcm:
            raise SystemExit("bench.py: the GPU .lac does not decode back to the PCM -- refusing to report a number")

    # ---- --full, N = 1: the other single-GPU BASELINE configs, each verified against its reference-minted digest ----
    # Outside the headline loop (never part of `value`): BASELINE configs[2] at its stated size (10 min stereo 24-bit 96 kHz,
    # mixed material), ten minutes of white noise 16/48 (the hardest material: every block "uncertain", about five exactly
    # costed candidates per slot) and BASELINE configs[4] (the 16 combinations {mono, stereo} x {16, 24 bit} x {44.1, 48,
    # 96, 192 kHz}, 60 s each) as ONE job.  A step = the whole job with its PCM resident in HBM in WAV layout, result in
    # pinned host memory; every .lac of the last step is compared with the golden digest minted from the reference
    # (tests/golden/make_golden.py) and nothing is printed on a mismatch.
    other = None
    if args.full and world == 1 and default_run and not args.no_other_workloads and not args.analysis_only:
        other = []
        # The north_star's literal layout: analysis on the device, plan records back, the bit-serial emit on host threads
        # (LACX_FLAG_HOST_EMIT).  Same stream as the headline, planar int32 resident in HBM, host copies for the emit.
        if not args.host_emit:
            he = lacx.Encoder(12, STEREO_MODE, sample_rate, bit_depth, device=device)
            he.set_thread_count(emit_threads)
            he.set_host_emit(True)
            dl_, dr_ = torch.from_numpy(left).cuda(), torch.from_numpy(right).cuda()
            torch.cuda.synchronize()
            he.encode_shard_device_view(dl_.data_ptr(), dr_.data_ptr(), left, right, frames, stream)
            each_he, res_he = [], None
            for _ in range(3):
                t2 = time.perf_counter()
                res_he = he.encode_shard_device_view(dl_.data_ptr(), dr_.data_ptr(), left, right, frames, stream)
                each_he.append(round((time.perf_counter() - t2) * 1e3, 3))
            tmh = he.timing()
            lac_he = lac_of(res_he[0].tobytes(), np.array(res_he[1], dtype=np.uint32))
            if not digest_matches(lac_he, "cfg2_10min_st16_48k_auto"):
                raise SystemExit("bench.py: host-emit .lac does not match the reference's golden digest -- refusing to report a number")
            other.append({"workload": "BASELINE configs[1] with the bit emit on the host (north_star layout: device analysis, plans D2H, "
                                      f"{emit_threads} host emit threads)", "value": round(frames * 2 / (min(each_he) / 1e3) / 1e6, 3),
                          "unit": "Msamples/s", "ms_per_step": min(each_he), "ms_each_step": each_he,
                          "device_analysis_ms": round(tmh.analysis_ms, 3), "host_emit_tail_ms": round(tmh.emit_ms, 3),
                          "host_emit_threads": emit_threads, "matches_golden_digest": True})
            del dl_, dr_, he, res_he, lac_he
        del left, right
        main["left"] = main["right"] = None

        def timed_job(name, specs, steps=8, warmup=2):
            # specs: (digest name, frames, channels, bit_depth, rate, stereo_mode, kind, stereo family, seed)
            jobs = []
            for dname, frames_j, ch, bd, sr, sm, kind, st, seed in specs:
                l_, r_ = synth_pcm_parallel(synth, frames_j, ch, bd, sr, seed, kind, stereo=st, threads=emit_threads)
                inter = synth.interleave(l_, r_, bd)
                del l_, r_
                d = torch.from_numpy(inter.view(np.int16) if bd == 16 else inter).cuda()
                del inter
                jobs.append(dict(name=dname, frames=frames_j, ch=ch, bd=bd, sr=sr, sm=sm, d=d,
                                 layout=lacx.PCM_INTERLEAVED_I16 if bd == 16 else lacx.PCM_INTERLEAVED_I24))
            torch.cuda.synchronize()
            run = make_runner(jobs)
            for _ in range(warmup):
                run()
            torch.cuda.synchronize()
            with StepLog() as log:  # (collects garbage once on entry: outside the timed loop)
                t1 = time.perf_counter()
                for _ in range(steps):
                    log.begin()
                    res, kernel_ms, tms = run()
                    log.end(tms)
                torch.cuda.synchronize()
                dt = (time.perf_counter() - t1) / steps
            log._digest()
            each = log.rows["wall_ms"]
            ok = True
            for j, (pay, tab) in zip(jobs, res):
                lac = lac_of(pay.tobytes(), np.array(tab, dtype=np.uint32), j["sr"], j["bd"], j["sm"], j["ch"])
                ok = ok and digest_matches(lac, j["name"])
            samples = sum(j["frames"] * j["ch"] for j in jobs)
            if not ok:
                raise SystemExit(f"bench.py: {name}: a .lac does not match the reference's golden digest -- refusing to report a number")
            other.append({"workload": name, "value": round(samples / dt / 1e6, 3), "unit": "Msamples/s",
                          "ms_per_step": round(dt * 1e3, 3), "kernel_ms": round(kernel_ms, 3), "streams": len(jobs),
                          "samples": samples, "steps": steps, "ms_each_step": each,
                          "ms_per_step_median": round(float(np.median(each)), 3), "ms_per_step_max": max(each),
                          "step_log": log.summary(), "matches_golden_digest": True})
            del jobs

        def make_runner(jobs):
            if len(jobs) > 1 and hasattr(lacx, "BatchEncoder"):
                be = lacx.BatchEncoder([(j["sr"], j["bd"], j["sm"]) for j in jobs], device=device)

                def run_batch():
                    res = be.encode_device([(j["d"].data_ptr(), j["layout"], j["ch"], j["frames"]) for j in jobs], stream)
                    tm_ = be.timing()
                    return res, tm_.full_ms, [tm_]
                return run_batch
            encs = [lacx.Encoder(12, j["sm"], j["sr"], j["bd"], device=device) for j in jobs]

            def run_each():  # every stream enqueued before the first result is collected
                for e_, j in zip(encs, jobs):
                    e_.encode_shard_pcm_device_begin(j["d"].data_ptr(), j["layout"], j["ch"], j["frames"], stream)
                res = [e_.encode_shard_end() for e_ in encs]
                tms_ = [e_.timing() for e_ in encs]
                return res, sum(t_.full_ms for t_ in tms_), tms_
            return run_each

        timed_job("BASELINE configs[2]: 10 min synthetic stereo 24-bit 96 kHz (mixed material), partitioning + zero-run on",
                  [("cfg3_10min_st24_96k_mixed", 57_600_000, 2, 24, 96000, 2, "mixed", "wide", 7)])
        timed_job("white noise: 10 min synthetic stereo 16-bit 48 kHz, independent channels (every block uncertain)",
                  [("noise_10min_st16_48k", 28_800_000, 2, 16, 48000, 2, "noise", "independent", 3)])
        cfg5 = []
        for ch in (1, 2):
            for bd in (16, 24):
                for sr in (44100, 48000, 96000, 192000):
                    i = len(cfg5)
                    cfg5.append((f"cfg5_{i:02d}_{'st' if ch == 2 else 'mono'}{bd}_{sr}", 60 * sr, ch, bd, sr, 2 if ch == 2 else 0,
                                 "mixed" if i & 1 else "music", "wide", 500 + i))
        timed_job("BASELINE configs[4]: mixed corpus as one job -- {mono, stereo} x {16, 24 bit} x {44.1, 48, 96, 192 kHz}, 60 s each, "
                  "16 streams, per-block predictor + stereo auto-select", cfg5)

    out = {
        "metric": METRIC,
        "value": round(main["value"], 3),
        "unit": "Msamples/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": round(main["ms_per_step"], 3),
        "higher_is_better": True,
        "scaling": "strong" if (workload == "cfg4" and not args.seconds) else "weak",
        "vs_baseline": None,
        "dtype": "int64",
        "data": "synthetic",
        "full": bool(args.full),
        "config": {
            "workload": f"{wl_name}: synthetic stereo {bit_depth}-bit {sample_rate // 1000} kHz ({args.kind}), auto MS/LR, LPC search, "
                        "16384-frame blocks, zero-run + partitioning on",
            "total_frames": int(main["total_frames"]),
            "total_blocks": int(main["total_blocks"]),
            "frames_rank0": int(frames),
            "blocks_rank0": int(main["b1"] - main["b0"]),
            "host_emit_threads": emit_threads,
            "emit": "host" if args.host_emit else "device",
            "device_pcm_layout": (f"interleaved int{bit_depth} (WAV data chunk)" if interleaved else "planar int32"),
            "timed_region": ("device analysis (PCM resident in HBM) + plan D2H + host emit + shard table" if args.host_emit
                             else "device analysis + device bit emit (PCM resident in HBM) + payload/table D2H into pinned host memory")
                            + (" + all_gather of shard sizes" if world > 1 else ""),
            "exchange_backend": (None if world == 1 else ("gloo" if rehearse else "nccl (RCCL)")),
        },
        "ranks_seen": ranks_seen,
        "rehearsal_shared_gpu": bool(rehearse) if world > 1 else False,
        "byte_identical_shards": (f"{shard_ok}/{world}" if shard_ok is not None else None),
        "weak_10min_per_gpu": weak,
        "weak_10min_per_gpu_24bit_96k": weak96,
        "single_process_fanout": fan_line,
        "breakdown_ms": {
            "device_analysis": round(mean("analysis_ms"), 3),
            "k_ingest_levinson": round(mean("ingest_ms"), 3),
            "k_probe_decide": round(mean("probe_ms"), 3),
            "k_analyze_full": round(mean("full_ms"), 3),
            ("host_emit_tail" if args.host_emit else "k_emit"): round(mean("emit_ms"), 3),
            "api_call": round(mean("api_ms"), 3),
        },
        "step_log": rec.get("log"),
        "fused_emit": {"streamed_out_beside_the_analysis": int(tm.emit_direct), "channel_blocks": int(tm.full_slots)},
        "device_analysis_msamples_s": round(frames * 2 / (max(mean("analysis_ms"), 1e-9) / 1e3) / 1e6, 3),
        "roofline": roofline,
        "cpu_baseline": cpu,
        "cpu_baseline_all_allowed_cores": cpu_all,
        "end_to_end": e2e,
        "decode_check": decode_check,
        "other_workloads": other,
        "byte_identical_to_cpu_baseline": identical,
        "matches_golden_digest": digest_ok,
    }
    print(json.dumps(out))
    if world > 1:
        dist.destroy_process_group()
    return 0


def cgroup_cpu_quota():
    """Whole cores of CPU time this process's cgroup may use (v2 cpu.max, v1 cfs quota), or None when unlimited."""
    try:
        with open("/sys/fs/cgroup/cpu.max") as f:
            q, per = f.read().split()[:2]
        if q != "max":
            return -(-int(q) // int(per))
        return None
    except (OSError, ValueError):
        pass
    try:
        with open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us") as f:
            q = int(f.read())
        with open("/sys/fs/cgroup/cpu/cpu.cfs_period_us") as f:
            per = int(f.read())
        return -(-q // per) if q > 0 and per > 0 else None
    except (OSError, ValueError):
        return None


def main():
    args = parse_args()
    if args.fanout and "WORLD_SIZE" not in os.environ:
        sys.exit(fanout_single_process(args))
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(launch_ranks(args))
    sys.exit(worker(args))


if __name__ == "__main__":
    main()
