"""ctypes wrapper of the ingest test entry point of liblacx_hooks.so (csrc/k_front_hooks.hip) and the placement of a
stream's PCM in device memory between sentinels.  Test infrastructure: the binding (lacx.py) does not know the hook."""
from __future__ import annotations

import ctypes as C

import numpy as np

import ingestrecipes as R

HOOKS = ("lacx_hook_ingest_tables",)
GUARD = 64  # sentinel bytes on either side of a placed array


class HookIngestStream(C.Structure):
    _fields_ = [("frames", C.c_uint64), ("data0", C.c_void_p), ("data1", C.c_void_p), ("channels", C.c_int32),
                ("stereo_mode", C.c_int32), ("bit_depth", C.c_int32), ("layout", C.c_int32)]


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


class Placed:
    """Bytes in device memory `offset` bytes behind a 16-byte aligned address of a torch buffer, sentinels on both sides;
    or (whole) at the very end of a buffer that is an allocation of its own."""

    def __init__(self, torch, raw: bytes, offset=0, whole=None):
        n = len(raw)
        if whole is None:
            self.buf = torch.full((GUARD + 16 + offset + n + GUARD,), R.SENTINEL, dtype=torch.uint8, device="cuda")
            at = GUARD + (-(self.buf.data_ptr() + GUARD)) % 16 + offset
        else:
            self.buf, at = whole, whole.numel() - n
            self.buf.fill_(R.SENTINEL)
        self.at, self.n, self.raw = at, n, raw
        self.buf[at:at + n] = torch.frombuffer(bytearray(raw), dtype=torch.uint8).cuda()
        self.ptr = self.buf.data_ptr() + at

    def untouched(self):
        host = self.buf.cpu().numpy()
        return bool((host[:self.at] == R.SENTINEL).all()) and bool((host[self.at + self.n:] == R.SENTINEL).all()) and \
            host[self.at:self.at + self.n].tobytes() == self.raw


class PlacedStream:
    def __init__(self, torch, st: R.Stream, whole=None):
        self.stream = st
        self.arrays = [Placed(torch, raw, st.offset, whole=whole if (k == 0 and st.at_end) else None)
                       for k, raw in enumerate(st.arrays())]
        if st.at_end:
            assert self.arrays[0].at + self.arrays[0].n == whole.numel()
        else:
            assert all((a.ptr - st.offset) % 16 == 0 for a in self.arrays)

    def record(self):
        st = self.stream
        return HookIngestStream(st.frames, self.arrays[0].ptr, self.arrays[1].ptr if len(self.arrays) == 2 else None,
                                st.channels, st.stereo_mode if st.channels == 2 else 0, st.bit_depth, st.layout)

    def untouched(self):
        return all(a.untouched() for a in self.arrays)


class Device:
    """The ingest hook on one encoder handle of the library the binding currently uses (lacx.use_library first)."""

    def __init__(self, lacx, device=0):
        import torch

        self.lacx, self.torch = lacx, torch
        self.enc = lacx.Encoder(12, 2, 48000, 24, device=device)
        self.h = self.enc._handle()
        self.whole = None

    def close(self):
        self.enc.close()

    def place(self, st: R.Stream) -> PlacedStream:
        if st.at_end and self.whole is None:
            self.whole = self.torch.empty(10 << 20, dtype=self.torch.uint8, device="cuda")  # an allocation of its own
        return PlacedStream(self.torch, st, self.whole)

    def call(self, records, as_table, fold, repeat, blocks, out=None):
        """The raw call: (return code, message, tables of every run, front_ctr [repeat][blocks][2])."""
        t = out or R.sentinel_tables(blocks, repeat)
        ctr = np.full((repeat, blocks, 2), 0x5A5A5A5A, dtype=np.uint32)
        fn = self.lacx.lib().lacx_hook_ingest_tables
        fn.restype = C.c_int
        arr = (HookIngestStream * max(len(records), 1))(*records)
        rc = fn(self.h, arr, C.c_uint32(len(records)), C.c_int(int(as_table)), C.c_int(int(fold)), C.c_uint32(repeat),
                C.c_uint32(blocks), _p(t.sums), _p(t.badidx), _p(t.acorr), _p(t.bplans), _p(t.need_probe), _p(t.need_full), _p(ctr))
        msg = self.lacx.lib().lacx_last_error(self.h).decode(errors="replace") if rc != self.lacx.OK else ""
        return rc, msg, t, ctr

    def run(self, placed, as_table, fold, repeat=1):
        """k_ingest (and k_stereo where not folded) over placed streams: ([Tables of run 0, of run 1, ...], front_ctr)."""
        blocks = sum(p.stream.blocks for p in placed)
        rc, msg, t, ctr = self.call([p.record() for p in placed], as_table, fold, repeat, blocks)
        if rc != self.lacx.OK:
            raise RuntimeError(msg or f"lacx_hook_ingest_tables failed: {rc}")
        runs = [R.Tables(t.sums[r], t.badidx[r], t.acorr[r], t.bplans[r], t.need_probe[r], t.need_full[r]) for r in range(repeat)]
        return runs, ctr


def check(want: R.Tables, runs, ctr, what, limit=24):
    """Every run's tables are the reference's word for word, the sentinel where nothing may be written; front_ctr is zero
    after every run; all runs returned the same bytes."""
    for r, got in enumerate(runs):
        d = R.differences(want, got, f"{what}, run {r}:")
        assert not d, f"{len(d)} words differ:\n" + "\n".join(d[:limit])
        assert not ctr[r].any(), f"{what}, run {r}: front_ctr is not zero after the run: blocks {np.flatnonzero(ctr[r].any(axis=1))[:8]}"
    for r in range(1, len(runs)):
        for f in ("sums", "badidx", "acorr", "bplans", "need_probe", "need_full"):
            assert getattr(runs[r], f).tobytes() == getattr(runs[0], f).tobytes(), f"{what}: run {r} differs from run 0 in {f}"
