"""The streaming-domain corpus (tests/narrowrecipes.py) without a GPU: the blocks do what they were chosen for, by the
oracle's records alone; the oracle gives the reference's bytes for every block under all four flag pairs (where the
reference build exists); and the kernel-phase simulator (tests/native/sim_analyze.cpp, the <16,1024> geometry, built
from the headers the HIP kernels are built from) gives the oracle's plan, field by field, and the oracle's bytes for
every block -- default variant, forced 64-bit arithmetic (1) and every phase_b_quick result checked against the walk
(32).

Measured on the CPU: the whole module about 47 s, of which check_coverage() + check_flag_coverage() about 10 s."""
import ctypes as C
import os

import numpy as np
import pytest

import narrowrecipes as N
import twinbuild
from test_native_units import CPlan

VARIANTS = (0, 1, 32)


def test_corpus_covers_what_it_promises():
    """Every partition order each of the eight sizes allows, modes 0..3 inside partitions, borders inside chunks and
    long last partitions at every order; escapes, run tokens of >= 4096, runs cut at a partition end, runs of 1..5 at,
    before and across chunk borders, unary parts of 32..63 and >= 64 ones, bin partitions with all four shapes, a block
    that is zero outside one partition; static parameters 0..15 and parameters in force up to 26; residual sums of
    kNarrowLimit - 1 and kNarrowLimit at partition order 3; every predictor at two sizes, saturated coefficients;
    stereo pairs whose side channel fills 25 bits."""
    counts = N.check_coverage()
    assert sum(counts.values()) == len(N.corpus()) and set(counts) == set(N.FAMILIES)
    N.check_flag_coverage()


@pytest.mark.parametrize("family", N.FAMILIES)
def test_oracle_gives_the_reference_bytes(oracle, ref, family):
    """Bytes, and the plan fields the bytes begin with: predictor type, order, coefficients, the control byte."""
    for b in N.family(family):
        for zr, pt in N.FLAGS:
            want = ref.block_encode(b.x, zr, pt)
            assert oracle.block_encode(b.x, zr, pt) == want, (family, b.name, zr, pt)
            op = oracle.block_plan(b.x, zr, pt)
            ncoef = op.order if op.predictor_type == 2 else 0
            assert (want[0], want[1]) == (op.predictor_type, op.order), (family, b.name, zr, pt)
            assert [int.from_bytes(want[2 + 2 * i:4 + 2 * i], "big", signed=True) for i in range(ncoef)] == \
                [op.coeffs_q15[i + 1] for i in range(ncoef)]
            control = want[2 + 2 * ncoef]
            assert control == ((0x80 | op.partition_order) if op.partition_order else 0) | (op.part_mode[0] << 5)


@pytest.fixture(scope="module")
def sim():
    return C.CDLL(twinbuild.shared_lib("sim_narrow", [os.path.join(twinbuild.NATIVE, "sim_analyze.cpp")]))


def _sim_diffs(sim, b, rec, data, zr, pt, variants, out):
    x = np.ascontiguousarray(b.x, dtype=np.int32)
    xp = x.ctypes.data_as(C.POINTER(C.c_int32))
    bad = []
    for wide in variants:
        what = f"{b.family}/{b.name} zero runs {zr} partitions {pt} variant {wide}"
        pl = CPlan()
        nbytes = sim.sim_block_plan_and_encode(xp, C.c_uint32(x.size), int(zr), int(pt), wide, C.byref(pl), out,
                                               C.c_uint32(len(out)))
        if nbytes == -1:
            bad.append(f"{what}: the analysis failed")
            continue
        pl.valid = 1  # (finalize_plan leaves the flag to the kernel's last store)
        bad += [f"{what}: plan {name} = {got}, oracle {want}" for name, got, want in N.planref.slot_diffs(pl, rec)]
        if nbytes < 0 or bytes(out[:nbytes]) != data:
            bad.append(f"{what}: the emit gave {nbytes} bytes, oracle {len(data)}")
    return bad


@pytest.mark.parametrize("family", N.FAMILIES)
def test_simulated_kernels_give_the_oracles_plans_and_bytes(sim, family):
    out = (C.c_uint8 * (1 << 20))()
    bad = []
    for b, rec, data in N.expected(family):
        bad += _sim_diffs(sim, b, rec, data, True, True, VARIANTS, out)
    assert not bad, f"{len(bad)} differences:\n" + "\n".join(bad[:40])


@pytest.mark.parametrize("zr,pt", N.FLAGS[1:], ids=["no_partitions", "no_zero_runs", "neither"])
@pytest.mark.parametrize("family", N.FLAG_SUBSET)
def test_simulated_kernels_under_the_other_flag_pairs(sim, family, zr, pt):
    out = (C.c_uint8 * (1 << 20))()
    bad = []
    for b, rec, data in N.expected(family, zr, pt):
        bad += _sim_diffs(sim, b, rec, data, zr, pt, VARIANTS, out)
    assert not bad, f"{len(bad)} differences:\n" + "\n".join(bad[:40])


def test_streams_are_made_of_the_corpus():
    """The streams of tests/test_gpu_narrow_blocks.py: whole corpus blocks, different ones left and right, a ragged pair at
    the end, all inside the stream's bit depth."""
    for name, bits, left, right in N.streams() + N.stereo_streams():
        assert left.size == right.size and N.fits(left, bits) and N.fits(right, bits), name
        assert not np.array_equal(left, right)
    for name, bits, left, right in N.streams():
        assert left.size % N.BLOCK in (12289, 8223, 4097) and 2 <= left.size // N.BLOCK <= 40, name
    assert len(N.ragged_blocks()) == sum(1 for b in N.corpus() if b.family in N.FLAG_SUBSET and b.x.size != N.BLOCK) == 59
