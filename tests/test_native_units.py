"""Host checks of the product's device-side building blocks (compiled for the host from the same headers):
the software x87 arithmetic against the machine's long double, and the data-parallel analysis phases, run
in the lock-step simulator, against the oracle's plans."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import twinbuild

ROOT, BUILD, NATIVE = twinbuild.ROOT, twinbuild.BUILD, twinbuild.NATIVE


class CPlan(C.Structure):
    _fields_ = [("predictor_type", C.c_uint8), ("order", C.c_uint8), ("partition_order", C.c_uint8),
                ("valid", C.c_uint8), ("coef", C.c_int16 * 12), ("payload_bytes", C.c_uint32),
                ("total_bits", C.c_uint64), ("part_mode_k", C.c_uint8 * 256)]


def test_x87_softfloat_matches_long_double():
    os.makedirs(BUILD, exist_ok=True)
    obj = os.path.join(BUILD, "lac_oracle.o")
    subprocess.check_call(["gcc", "-O2", "-std=c11", "-c", os.path.join(ROOT, "oracle", "lac_oracle.c"), "-o", obj])
    exe = twinbuild.program("test_x87", [os.path.join(NATIVE, "test_x87.cpp")], ["-O2", "-std=c++17"], link=[obj, "-lm", "-lpthread"],
                            include=[os.path.join(ROOT, "oracle")])
    out = subprocess.check_output([exe, "400000"]).decode()
    assert "fails=0" in out, out


@pytest.fixture(scope="module")
def sim():
    lib = C.CDLL(twinbuild.shared_lib("sim", [os.path.join(NATIVE, "sim_analyze.cpp")]))
    lib.sim_kmean_check.restype = C.c_uint64
    return lib


def test_division_free_rice_parameter(sim):
    assert sim.sim_kmean_check(C.c_uint64(1), C.c_uint64(1_000_000)) == 0


def _check(sim, oracle, x, geo, zr, pt, wide):
    x = np.ascontiguousarray(x, dtype=np.int32)
    pl = CPlan()
    assert sim.sim_block_plan(x.ctypes.data_as(C.POINTER(C.c_int32)), C.c_uint32(x.size), int(zr), int(pt), geo,
                              wide, C.byref(pl)) == 0
    op = oracle.block_plan(x, zr, pt)
    assert (pl.predictor_type, pl.order, pl.partition_order, pl.total_bits) == \
        (op.predictor_type, op.order, op.partition_order, op.total_bits)
    if op.predictor_type == 2:
        assert [pl.coef[i] for i in range(op.order)] == [op.coeffs_q15[i + 1] for i in range(op.order)]
    assert [pl.part_mode_k[i] for i in range(op.part_count)] == \
        [(op.part_mode[i] << 5) | op.part_k[i] for i in range(op.part_count)]
    assert pl.payload_bytes == len(oracle.block_encode(x, zr, pt))


KINDS = ["music", "noise", "silence", "near_silence", "sparse", "ramp", "walk", "tone", "mixed"]


@pytest.mark.parametrize("kind", KINDS)
def test_simulated_kernel_plans_match_oracle(pkg, oracle, sim, kind):
    """Every arithmetic variant of the kernel phases (32-bit fast path / 64-bit, fused / per-order
    partition pass, <16,1024> / <4,64> geometry) on whole blocks, probes and ragged sizes."""
    left, right = pkg.synth.synth_pcm(16384 + 4200, 2, 24 if kind in ("music", "noise") else 16, 48000, seed=7,
                                      kind=kind)
    s = (left - right).astype(np.int32)
    m = ((left.astype(np.int64) + right) >> 1).astype(np.int32)
    cases = [(left[:16384], 0), (s[:16384], 0), (m[16384:], 0), (left[100:356], 1), (s[5000:5256], 0),
             (right[3:4100], 0), (left[9:40], 0), (m[:1], 0), (s[:13], 0), (left[:13312], 0)]
    for i, (x, geo) in enumerate(cases):
        for wide in (0, 1, 2, 8, 16, 32, 33, 64):
            _check(sim, oracle, x, geo, True, True, wide)
    _check(sim, oracle, left[:16384], 0, False, True, 0)
    _check(sim, oracle, left[:16384], 0, True, False, 0)


def test_blocks_around_the_32_bit_sum_limit(pkg, oracle, sim):
    """The 32-bit fast paths hold for residual sums below kNarrowLimit = 2^32 - 2^20 (analyze_core.h): loud blocks whose
    sums land in [2^31, 2^32) and on either side of the limit, through the default variants, the forced 64-bit ones (1)
    and with every phase_b_quick result checked against the walk (32) -- plan and emitted bytes against the oracle."""
    rng = np.random.default_rng(41)
    blocks = []
    for amp in (140_000, 185_000, 250_000, 261_000, 262_100, 263_500, 275_000, 600_000):
        blocks.append(rng.integers(-amp, amp + 1, size=16384).astype(np.int32))          # white: order 0 wins, sum ~ n * amp
    tone, _ = pkg.synth.synth_pcm(16384, 1, 24, 96000, seed=12, kind="music")
    for gain in (6, 14, 30):
        loud = np.clip(tone.astype(np.int64) * gain, -(1 << 23), (1 << 23) - 1).astype(np.int32)
        blocks.append((loud + rng.integers(-150_000, 150_001, size=loud.size)).astype(np.int32))   # predictable part + loud floor
    blocks.append(rng.integers(-200_000, 200_001, size=9000).astype(np.int32))              # ragged size
    out = (C.c_uint8 * (1 << 20))()
    for x in blocks:
        for wide in (0, 1, 32):
            _check(sim, oracle, x, 0, True, True, wide)
        xc = np.ascontiguousarray(x, dtype=np.int32)
        nbytes = sim.sim_block_encode(xc.ctypes.data_as(C.POINTER(C.c_int32)), C.c_uint32(xc.size), 1, 1, 0, out, C.c_uint32(len(out)))
        assert nbytes > 0 and bytes(out[:nbytes]) == oracle.block_encode(xc, True, True)


def test_zero_run_bound_formula_is_a_lower_bound():
    """candidate_lower_bound()'s zero term, min(3 Z, 3 (R - 1) + 4 + (Z - R + 1) / 4) for Z zeros in at least R runs, against
    the exact minimum over every way of cutting Z zeros into R' >= R runs (a run of L costs 3 L below 4 and 4 + L / 4 from
    4 on: ref block/encoder.cpp:224-247 with the cheapest Rice parameter)."""
    import functools

    def run_cost(length):
        return 3 * length if length < 4 else 4 + length // 4

    @functools.lru_cache(None)
    def cheapest(zeros, runs):
        if runs == 1:
            return run_cost(zeros) if zeros >= 1 else 10**9
        return min(run_cost(first) + cheapest(zeros - first, runs - 1) for first in range(1, zeros - runs + 2))

    def bound(zeros, ends):
        if zeros == 0:
            return 0
        runs = max(ends, 1)
        return min(3 * zeros, 3 * (runs - 1) + 4 + ((zeros - runs + 1) >> 2))

    for zeros in range(1, 48):
        for ends in range(0, zeros + 1):
            assert bound(zeros, ends) <= min(cheapest(zeros, r) for r in range(max(ends, 1), zeros + 1)), (zeros, ends)
    assert bound(16384, 1) == run_cost(16384)  # an all-zero block meets the bound


def test_pruning_bound_on_zero_run_structures(pkg, oracle, sim):
    """The candidate pruning bound's zero-run term (zeros cost at least min(3 Z, 3 (R - 1) + 4 + (Z - R + 1) / 4) bits for
    Z zeros in at least R runs): all-zero blocks, isolated non-zeros, periodic patterns and randomly punched gaps of
    every run-length class, with the pruning on (0) and off (4) -- both must give the oracle's plan."""
    rng = np.random.default_rng(5)
    blocks = [np.zeros(16384, np.int32), np.zeros(300, np.int32)]
    one = np.zeros(16384, np.int32)
    one[8000] = 1
    blocks.append(one)
    for period in (2, 4, 5, 16, 17):
        x = np.zeros(8192, np.int32)
        x[::period] = rng.integers(-4, 5, size=x[::period].size)
        blocks.append(x)
    for it in range(10):
        n = int(rng.integers(300, 16385))
        x, _ = pkg.synth.synth_pcm(n, 1, 16, 48000, seed=int(rng.integers(1, 10**6)), kind=str(rng.choice(["music", "walk", "sparse"])))
        if it & 1:
            x = (x >> int(rng.integers(6, 14))).astype(np.int32)
        x = x.copy()
        pos = 0
        while pos < x.size:
            pos += int(rng.choice([1, 1, 2, 3, 7, 16, 40, 300]))
            gap = int(rng.choice([1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 1000]))
            x[pos:pos + gap] = 0
            pos += gap
        blocks.append(x)
    for x in blocks:
        for wide in (0, 4, 32, 64):
            _check(sim, oracle, x, 0, True, True, wide)
    _check(sim, oracle, np.zeros(256, np.int32), 1, True, True, 0)


def test_kernel_phases_clean_under_sanitizers():
    """The phase code the HIP kernels are built from, compiled for the host with AddressSanitizer + UBSan and run
    over block shapes and materials that reach every path (narrow / 64-bit, zero-run, bin, partitions, emit tiles)."""
    exe, why = twinbuild.sanitized_exe("sim_sanitize", [os.path.join(NATIVE, "sim_analyze.cpp"), os.path.join(NATIVE, "sim_sanitize_main.cpp")])
    if exe is None:
        pytest.skip(why)
    run = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert run.returncode == 0 and "sanitized simulator runs" in run.stdout, run.stdout + run.stderr
