"""ctypes wrappers of the x87 test entry points: the device ones of liblacx_hooks.so (csrc/k_x87_hooks.hip) and the host
compile of the same header (tests/native/x87_host.cpp).  Test infrastructure: the binding (lacx.py) does not know them."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

import twinbuild
import x87recipes as X

HOOKS = ("lacx_hook_x87_ops", "lacx_hook_levinson_tables")


class HookStream(C.Structure):
    _fields_ = [("frames", C.c_uint64), ("channels", C.c_int32), ("stereo_mode", C.c_int32)]


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _ops_buffers(n):
    return X.OpsResult(np.zeros((5, n), np.uint64), np.zeros((5, n), np.int32), np.zeros((5, n), np.uint32),
                       np.zeros((2, n), np.int32))


# ---------------------------------------------------------------------------------------------------------------------
# host compile
# ---------------------------------------------------------------------------------------------------------------------
_host = None


def host_lib():
    global _host
    if _host is None:
        _host = C.CDLL(twinbuild.shared_lib("x87_host", [os.path.join(twinbuild.NATIVE, "x87_host.cpp")], std="c++17"))
        _host.x87_host_ops.restype = None
        _host.x87_host_levinson.restype = None
    return _host


def host_ops(c):
    out = _ops_buffers(c.n)
    host_lib().x87_host_ops(C.c_uint32(c.n), _p(c.in_m), _p(c.in_e), _p(c.in_s), _p(c.in_i), _p(out.out_m), _p(out.out_e),
                            _p(out.out_s), _p(out.out_i))
    return out


def host_levinson(tables, mvo):
    """levinson_candidates of x87.h over tables [n][13]: (used [n][5], coef [n][5][13])."""
    tables = np.ascontiguousarray(tables, dtype=np.int64)
    mvo = np.ascontiguousarray(mvo, dtype=np.int32)
    n = tables.shape[0]
    coef = np.full((n, 5, 13), 0x5A5A, dtype=np.int16)
    used = np.full((n, 5), 0x5A, dtype=np.uint8)
    host_lib().x87_host_levinson(C.c_uint32(n), _p(tables), _p(mvo), _p(coef), _p(used))
    return used, coef


# ---------------------------------------------------------------------------------------------------------------------
# device: liblacx_hooks.so through an encoder handle of the binding (select the library first: lacx.use_library)
# ---------------------------------------------------------------------------------------------------------------------
class Device:
    """The two hooks on one encoder handle of the library the binding currently uses."""

    def __init__(self, lacx, device=0):
        self.lacx = lacx
        self.enc = lacx.Encoder(12, 2, 48000, 24, device=device)
        self.h = self.enc._handle()

    def close(self):
        self.enc.close()

    def _check(self, rc):
        if rc != self.lacx.OK:
            raise RuntimeError(self.lacx.lib().lacx_last_error(self.h).decode(errors="replace") or f"hook failed: {rc}")

    def ops(self, c):
        out = _ops_buffers(c.n)
        fn = self.lacx.lib().lacx_hook_x87_ops
        fn.restype = C.c_int
        self._check(fn(self.h, C.c_uint32(c.n), _p(c.in_m), _p(c.in_e), _p(c.in_s), _p(c.in_i), _p(out.out_m), _p(out.out_e),
                       _p(out.out_s), _p(out.out_i)))
        return out

    def levinson(self, pl):
        """k_levinson over a placement: the LpcSet array as the kernel leaves it, from a sentinel."""
        lpcs = X.sentinel_lpcs(pl.blocks)
        streams = (HookStream * len(pl.streams))(*[HookStream(f, ch, sm) for f, ch, sm in pl.streams])
        fn = self.lacx.lib().lacx_hook_levinson_tables
        fn.restype = C.c_int
        acorr = np.ascontiguousarray(pl.acorr, dtype=np.int64)
        need = np.ascontiguousarray(pl.need_probe, dtype=np.uint32)
        assert acorr.shape == (pl.blocks, X.SLOTS, 13) and need.shape == (pl.blocks,)
        self._check(fn(self.h, _p(acorr), _p(need), streams, C.c_uint32(len(pl.streams)), C.c_int(1 if pl.as_table else 0),
                       C.c_uint32(pl.blocks), _p(lpcs)))
        return lpcs
