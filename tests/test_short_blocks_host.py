"""The short-block corpus (tests/shortrecipes.py, blocks of 1..4096 samples in the streaming domain) without a GPU: the
blocks do what they were chosen for, by the oracle's records alone, and the kernel-phase simulator
(tests/native/sim_analyze.cpp, the <16,1024> geometry, built from the headers the HIP kernels are built from) gives the
oracle's plan, field by field, and the oracle's bytes for every block.

Simulator variants (the `force_wide` bits of sim_analyze.cpp): 0 on every block; 1 (64-bit arithmetic), 2 (the per-order
partition passes where the fused pass applies), 8 (the fused walk instead of partition_quick), 16 (no phase_b_quick),
32 (every phase_b_quick result checked against the walk), 33 and 64 (partition_quick for every wave) on the flag subset
and on every block of n <= 130 -- which is the whole corpus; the other three flag pairs in variant 0 on the flag subset.

Counts: 1744 blocks (1639 `lengths`, 105 `geometry`), 314 of them in the flag subset; 1744 x 8 variants + 314 x 3 flag
pairs = 14 894 simulator cases, each against the oracle's record and bytes.  Measured on the CPU: the whole module 72 s
(6 s of it the simulator's compile), against 68 s for the 17 335 cases of the trial that preceded the corpus; the
coverage checks 6 s, a variant over the corpus 6..8 s.

The comparer can fail: with `pick_initial_k(A, 256u)` for `n < 256u ? n : 256u` in a scratch copy of csrc/analyze_core.h
22 blocks of `lengths` differ (tone_n1, noise8_n2, tone_n2, tone_n3, noise8_n4, runs_n15, ...), with the last thread's
partial chunk taken as a whole one 1461 blocks of `lengths` and 56 of `geometry`."""
import ctypes as C
import os

import pytest

import planref
import shortrecipes as S
import twinbuild
from test_native_units import CPlan

VARIANTS = (1, 2, 8, 16, 32, 33, 64)


def test_corpus_covers_what_it_promises():
    """Every partition order 0..max at each of the 25 geometry sizes, modes 0..3 inside partitions, a partition border
    inside a chunk at every order 1..7; every predictor as a winner, each LPC order from the first n at which its
    candidate exists; the candidate set of every n <= 13; the five outcomes of the final-block choice at >= 3 sizes each,
    n = 1 and n = 4096 among them; probes instead of the full comparison at 4097."""
    counts = S.check_coverage()
    assert sum(counts.values()) == len(S.corpus()) and set(counts) == set(S.FAMILIES)


def test_flag_subset_covers_what_it_promises():
    """No partition without partitioning, no mode 1 without zero runs, modes 0..3 as the unpartitioned winner, and at
    least a quarter of the subset's blocks encode differently under each other flag pair."""
    differ = S.check_flag_coverage()
    assert set(differ) == set(S.FLAGS[1:])


def test_slices_and_subsets_leave_no_block_out():
    assert sorted(n for s in S.LENGTH_SLICES for n in s) == sorted(S.LENGTH_N) and len(S.LENGTH_N) == 149
    assert len(S.family("lengths")) == 149 * 11 and len(S.small_and_subset()) == len(S.corpus())
    assert {b.x.size for b in S.flag_subset()} == set(S.BORDER_N) | set(S.GEOMETRY_N)
    for bits in (16, 24):
        for n in S.PAIR_N + (S.PAIR_CONTRAST_N,):
            assert len(S.pairs(bits, n)) == 24 + ((bits, n) == (24, 1)) and all(S.fits(p.left, bits) and S.fits(p.right, bits) and p.left.size == n
                                                       for p in S.pairs(bits, n))


@pytest.mark.parametrize("bits,n,mode", [(16, 13, 2), (24, 4096, 2), (24, 2, "mono"), (16, 4097, 1)])
def test_final_streams_and_their_spliced_reference_bytes(bits, n, mode):
    """The streams of the GPU file's final-block tests: every pair behind 0, 1 and 2 full blocks, and the reference bytes
    (the oracle's encode of the front spliced with its encode of the final block) equal to the oracle's encode of the
    whole stream wherever final_bytes() holds the two against each other."""
    streams, want = S.final_streams(bits, n), S.final_bytes(bits, n, mode)
    assert len(streams) == len(want) == len(S.pairs(bits, n)) * 3
    assert [k for _, k, _, _ in streams[:3]] == [0, 1, 2] and [s[2].size for s in streams[:3]] == [n, S.BLOCK + n, 2 * S.BLOCK + n]
    name, k, left, right = streams[-1]
    assert want[-1] == S.stream_bytes(bits, k, left, right, mode, direct=True), name
    exp = S.expected_final(bits, n, mode)
    assert [len(e) for e in exp[:3]] == [1, 2, 3] and all(e[-1].frames == n for e in exp)


@pytest.fixture(scope="module")
def sim():
    return C.CDLL(twinbuild.shared_lib("sim_narrow", [os.path.join(twinbuild.NATIVE, "sim_analyze.cpp")]))


def _sim_diffs(sim, b, rec, data, zr, pt, variants, out):
    x = b.x
    xp = x.ctypes.data_as(C.POINTER(C.c_int32))
    bad = []
    for variant in variants:
        what = f"{b.family}/{b.name} zero runs {zr} partitions {pt} variant {variant}"
        pl = CPlan()
        nbytes = sim.sim_block_plan_and_encode(xp, C.c_uint32(x.size), int(zr), int(pt), variant, C.byref(pl), out,
                                               C.c_uint32(len(out)))
        if nbytes == -1:
            bad.append(f"{what}: the analysis failed")
            continue
        pl.valid = 1  # (finalize_plan leaves the flag to the kernel's last store)
        bad += [f"{what}: plan {name} = {got}, oracle {want}" for name, got, want in planref.slot_diffs(pl, rec)]
        if nbytes < 0 or bytes(out[:nbytes]) != data:
            bad.append(f"{what}: the emit gave {nbytes} bytes, oracle {len(data)}")
    return bad


def _run(sim, rows, zr, pt, variants):
    out = (C.c_uint8 * (1 << 16))()
    bad = []
    for b, rec, data in rows:
        assert b.x.flags["C_CONTIGUOUS"] and b.x.dtype == "int32" and len(data) < len(out)
        bad += _sim_diffs(sim, b, rec, data, zr, pt, variants, out)
    assert not bad, f"{len(bad)} differences:\n" + "\n".join(bad[:40])
    return len(rows) * len(variants)


@pytest.mark.parametrize("family", S.FAMILIES)
def test_simulated_kernels_give_the_oracles_plans_and_bytes(sim, family):
    assert _run(sim, S.expected(family), True, True, (0,)) == len(S.family(family))


@pytest.mark.parametrize("variant", VARIANTS)
def test_simulated_kernel_variants(sim, variant):
    rows = S.expected("lengths", True, True, S.SMALL_N) + S.expected_subset(True, True)
    assert _run(sim, rows, True, True, (variant,)) == len(S.small_and_subset())


@pytest.mark.parametrize("zr,pt", S.FLAGS[1:], ids=["no_partitions", "no_zero_runs", "neither"])
def test_simulated_kernels_under_the_other_flag_pairs(sim, zr, pt):
    assert _run(sim, S.expected_subset(zr, pt), zr, pt, (0,)) == len(S.flag_subset())
