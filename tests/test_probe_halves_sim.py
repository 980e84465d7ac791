"""The probe class's geometry of 32 lanes x 8 samples per 256-sample slot (two slots per wave on the device), run through
the lock-step simulator from the kernel's own per-thread phases and compared with the oracle's plan and size.  No GPU."""
import ctypes as C
import os

import numpy as np
import pytest

import twinbuild

from test_native_units import CPlan



@pytest.fixture(scope="module")
def sim8x32():
    return C.CDLL(twinbuild.shared_lib("sim_probe_halves", [os.path.join(twinbuild.NATIVE, "sim_probe_halves.cpp")], include=[twinbuild.NATIVE]))


def _check(sim, oracle, x, zr=True, pt=True, wide=0):
    x = np.ascontiguousarray(x, dtype=np.int32)
    pl = CPlan()
    assert sim.sim_probe_plan_8x32(x.ctypes.data_as(C.POINTER(C.c_int32)), C.c_uint32(x.size), int(zr), int(pt), wide,
                                   C.byref(pl)) == 0
    op = oracle.block_plan(x, zr, pt)
    assert (pl.predictor_type, pl.order, pl.partition_order, pl.total_bits) == \
        (op.predictor_type, op.order, op.partition_order, op.total_bits)
    if op.predictor_type == 2:
        assert [pl.coef[i] for i in range(op.order)] == [op.coeffs_q15[i + 1] for i in range(op.order)]
    assert [pl.part_mode_k[i] for i in range(op.part_count)] == \
        [(op.part_mode[i] << 5) | op.part_k[i] for i in range(op.part_count)]
    assert pl.payload_bytes == len(oracle.block_encode(x, zr, pt))


def _windows(pkg, kind, bits):
    left, right = pkg.synth.synth_pcm(16384, 2, bits, 48000, seed=23, kind=kind)
    s = (left - right).astype(np.int32)
    m = ((left.astype(np.int64) + right) >> 1).astype(np.int32)
    return [left[:256], right[8064:8320], m[16128:], s[300:556]]


# n < 256; n not a multiple of 8; n <= 32 (a single lane's chunk, a few lanes, one sample)
SHORT = [255, 250, 129, 100, 64, 33, 32, 31, 17, 9, 8, 7, 1]


@pytest.mark.parametrize("kind,bits", [("music", 16), ("music", 24), ("noise", 16), ("noise", 24), ("silence", 16),
                                       ("near_silence", 16), ("sparse", 16), ("ramp", 16), ("mixed", 24)])
def test_probe_slot_8x32_matches_oracle(pkg, oracle, sim8x32, kind, bits):
    for x in _windows(pkg, kind, bits):
        for wide in (0, 1, 2, 8, 64):
            _check(sim8x32, oracle, x, wide=wide)
        _check(sim8x32, oracle, x, zr=False)
        _check(sim8x32, oracle, x, pt=False)
        for n in SHORT:
            _check(sim8x32, oracle, x[:n])


def test_probe_slot_8x32_full_scale_24_bit(oracle, sim8x32):
    rng = np.random.default_rng(5)
    hi, lo = (1 << 23) - 1, -(1 << 23)
    square = np.where(np.arange(256) % 2 == 0, hi, lo).astype(np.int32)
    noise = rng.integers(lo, hi + 1, 256).astype(np.int32)
    dc = np.full(256, lo, dtype=np.int32)
    for x in (square, noise, dc):
        for wide in (0, 1):
            _check(sim8x32, oracle, x, wide=wide)
        for n in SHORT:
            _check(sim8x32, oracle, x[:n])


def test_probe_slot_8x32_exact_ramp_and_zeros(oracle, sim8x32):
    ramp = (np.arange(256, dtype=np.int32) * 37 - 4000)
    zeros = np.zeros(256, dtype=np.int32)
    tail = zeros.copy()
    tail[200:] = 5  # silent head, a step near the end: zero-run partitions next to plain ones
    for x in (ramp, zeros, tail):
        _check(sim8x32, oracle, x)
        for n in SHORT:
            _check(sim8x32, oracle, x[:n])
