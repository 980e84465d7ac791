"""The corpus of the wide-domain block tests (tests/test_wide_blocks_host.py, tests/test_gpu_wide_blocks.py) and the
conditions its oracle records must meet before a device is asked anything.  Plain helper module: numpy and the oracle
only, no GPU, no test in here.

"Wide" is what `lacx_block_encode` sends through csrc/wide.hip: a block with a sample of magnitude above 2^24.  Every
block here is wide except the narrow members of the edge twins, which take the streaming kernels.

Everything is built from explicit seeds.  The seeds of the families `fallback`, `early`, `predictors` and `modes` were
found once by running `sines(seed, n)` for seed = 0, 1, 2, ... through the oracle (classify() below is the test that was
used) and are frozen here as literals; nothing searches at import time.  check_coverage() asserts on the oracle's records
that each block still does what it was chosen for.

Flag pairs: every block runs with (zero runs on, partitioning on).  The other three pairs run on FLAG_SUBSET: the
families `fallback`, `geometry` and `modes`, which is where the flags change the outcome (check_flag_coverage).

The wrapping-autocorrelation blocks rely on the reference accumulating int64 products past 2^63, which C++ leaves
undefined; the reference build wraps, as the oracle does by definition (unsigned accumulation), and the two agree on
every block of the family `wrap` (tests/test_wide_blocks_host.py pins it), so none had to be left out.
"""
from __future__ import annotations

import functools
from collections import namedtuple

import numpy as np

import planref

I32_MIN, I32_MAX = -2**31, 2**31 - 1
EDGE = 1 << 24                      # block_is_wide: |x| > 2^24 (csrc/api_encode.cpp)
MIN_PARTITION, MAX_PARTITION_ORDER = 32, 8
MAX_BLOCK_BYTES, MAX_CORPUS_BYTES = 4 << 20, 64 << 20
FLAGS = ((True, True), (True, False), (False, True), (False, False))  # (zero runs, partitioning)

Block = namedtuple("Block", "family name x")


def clip32(x):
    return np.clip(np.asarray(x), I32_MIN, I32_MAX).astype(np.int32)


def is_wide(x):
    x = np.asarray(x, dtype=np.int64)
    return bool((np.abs(x) > EDGE).any())


def max_partition_order(n):
    p = 0
    while p < MAX_PARTITION_ORDER and (n >> (p + 1)) >= MIN_PARTITION:
        p += 1
    return p


def sines(seed, n=512):
    """One or two sines of period 2.2..30 samples and amplitude 2^27..2^31, up to three full-scale spikes, noise of
    2^1..2^23: the material of the seeded searches."""
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64)
    x = np.zeros(n, dtype=np.float64)
    for _ in range(int(rng.integers(1, 3))):
        period = rng.uniform(2.2, 30.0)
        amp = 2.0 ** rng.uniform(27, 31)
        x += amp * np.sin(2 * np.pi * t / period + rng.uniform(0, 6.28))
    x = np.rint(x).astype(np.int64)
    for _ in range(int(rng.integers(0, 4))):
        x[int(rng.integers(0, n))] = I32_MAX if rng.integers(0, 2) else I32_MIN
    nb = int(rng.integers(1, 24))
    x += rng.integers(-(1 << nb), (1 << nb) + 1, size=n)
    return clip32(x)


# -- frozen results of the searches -------------------------------------------------------------------------------------

# (seed of sines(seed, 512), candidate order, Levinson order, emitted order)
FALLBACK = ((118282, 12, 12, 10), (5244, 10, 10, 8), (1483, 8, 8, 6), (900, 6, 6, 4),
            (12020, 8, 8, 4), (24434, 10, 10, 6), (52185, 12, 12, 8), (1038, 12, 11, 4), (2216, 10, 9, 8))
FALLBACK_STEPS = {(12, 10), (10, 8), (8, 6), (6, 4)}
FALLBACK_TWO_STEPS = {(8, 4), (10, 6), (12, 8)}
# (seed, candidate order, Levinson order == emitted order): the recursion stopped early and the candidate still won
EARLY = ((25, 4, 2), (377, 10, 9), (1392, 12, 11))
# (seed, predictor type, order) of sines(seed, 512)
PREDICTORS = ((31, 0, 0), (28, 0, 1), (1, 0, 2), (4, 0, 3), (0, 0, 4), (3, 1, 2), (5, 1, 2), (17, 1, 2),
              (175, 2, 4), (142, 2, 6), (44, 2, 8), (555, 2, 10), (425, 2, 12))
# (seed of sines(seed, 48), mode of the unpartitioned block)
MODES_48 = ((0, 0), (91, 1), (13, 2), (2, 3))
# (seed of sines(seed, 16384), candidate order, Levinson order, emitted order)
FULL_FALLBACK = ((168, 6, 6, 4), (679, 10, 10, 8))

SMALL_N = tuple(range(1, 15)) + (31, 32, 33)
GEOMETRY_N = (63, 64, 65, 127, 128, 129, 255, 256, 257, 300, 511, 512, 513, 1000, 1023, 1024)
WRAP_CONSTANT_N = (2, 4, 8, 4096)
EDGE_N = (13, 4096)
SEQUENCE_N = (1024, 300, 13, 16384, 5)  # the one-handle sequence: wide, narrow, wide, wide, wide

FLAG_SUBSET = ("fallback", "geometry", "modes")


# -- families -----------------------------------------------------------------------------------------------------------

def _small(n, character):
    if character == "noise":
        x = np.random.default_rng(1000 + n).integers(I32_MIN, I32_MAX + 1, size=n)
        x[0] |= 1 << 30  # (x[0] >= 2^30 or < -2^30 whatever was drawn: a block of one sample is still wide)
        return clip32(x)
    if character == "sine":
        return clip32(np.rint(I32_MAX * np.sin(2 * np.pi * np.arange(n) / 7.3 + 0.5)))
    return np.full(n, I32_MAX if n % 2 == 0 else -I32_MAX, dtype=np.int32)


def _segment(rng, character, length, bits):
    """Partition material: z zeros with a single 1, b 0 / +-1 / +-2, anything else noise of `bits` bits."""
    if character == "z":
        x = np.zeros(length, dtype=np.int64)
        x[length // 2] = 1
        return x
    if character == "b":
        return rng.integers(-2, 3, size=length)
    return rng.integers(-(1 << bits), (1 << bits) + 1, size=length)


# seed of _geometry(n, p, seed) for every (n, p): the first seed whose oracle plan has partition order p
GEOMETRY_SEEDS = {
    (63, 0): 0, (64, 1): 4, (65, 1): 1, (127, 1): 0, (128, 1): 26, (128, 2): 3, (129, 1): 7, (129, 2): 1, (255, 1): 2,
    (255, 2): 0, (256, 1): 1, (256, 2): 13, (256, 3): 0, (257, 1): 0, (257, 2): 1, (257, 3): 1, (300, 1): 0, (300, 2): 0,
    (300, 3): 2, (511, 1): 11, (511, 2): 0, (511, 3): 0, (512, 1): 5, (512, 2): 8, (512, 3): 2, (512, 4): 0, (513, 1): 7,
    (513, 2): 4, (513, 3): 2, (513, 4): 0, (1000, 1): 27, (1000, 2): 0, (1000, 3): 1, (1000, 4): 0, (1023, 1): 9,
    (1023, 2): 5, (1023, 3): 0, (1023, 4): 1, (1024, 1): 1, (1024, 2): 6, (1024, 3): 3, (1024, 4): 4, (1024, 5): 2}


def _geometry(n, p, seed):
    """2^p partitions of n >> p samples (the last one longer) whose character changes from each to the next (quiet noise,
    loud noise, zero runs, 0 / +-1 / +-2), so that order p separates what order p - 1 mixes; one sample just outside
    the 25-bit domain makes the block wide."""
    rng = np.random.default_rng([n, p, seed])
    cycle = [("z", 0), ("b", 0), ("q", int(rng.integers(3, 9))), ("m", int(rng.integers(9, 15))),
             ("h", int(rng.integers(15, 21)))]
    cycle = [cycle[i] for i in rng.permutation(5)[:int(rng.integers(2, 5))]]
    parts, base = 1 << p, n >> p
    segs = []
    for i in range(parts):
        length = n - base * (parts - 1) if i + 1 == parts else base
        character, bits = cycle[i % len(cycle)]
        segs.append(_segment(rng, character, length, bits))
    x = np.concatenate(segs)
    x[int(rng.integers(0, n))] = int(rng.choice([-1, 1])) * ((1 << 24) + int(rng.integers(1, 1 << 10)) ** 2)
    return clip32(x)


def _zero_runs(n, seed, burst, gap):
    """Zeros with bursts of `burst` wide samples every `gap`."""
    rng = np.random.default_rng(seed)
    x = np.zeros(n, dtype=np.int64)
    for a in range(gap // 2, n - burst, gap):
        x[a:a + burst] = rng.integers(-(1 << 29), 1 << 29, size=burst)
    return clip32(x)


def _bin_material(n, seed, where, value):
    """+-1 / +-2 with a zero at every fifth sample (no zero run) and rare samples far outside: after one of those the
    adaptive k is of no use for the small values, the bin code still is."""
    x = np.random.default_rng(seed).choice([-2, -1, 1, 2], size=n)
    x[::5] = 0
    x[list(where)] = value
    return clip32(x)


def _wrap_blocks():
    out = [(f"constant_min_n{n}", np.full(n, I32_MIN, dtype=np.int32)) for n in WRAP_CONSTANT_N]
    for n in (64, 1000):
        out.append((f"alternating_extremes_n{n}", np.where(np.arange(n) % 2 == 0, I32_MAX, I32_MIN).astype(np.int32)))
    t = np.arange(64)
    x = np.rint((1 << 26) * np.sin(2 * np.pi * t / 9.0)).astype(np.int64)
    x[:2] = I32_MIN
    out.append(("r0_negative_r1_positive_n64", clip32(x)))      # R0 = 2^63 + ... wraps below zero, R1 = 2^62 + ... does not
    x = np.rint((1 << 20) * np.sin(2 * np.pi * np.arange(300) / 11.0)).astype(np.int64)
    x[:4] = I32_MIN
    out.append(("r0_wraps_past_zero_n300", clip32(x)))          # R0 = 2^64 + small: wraps to a small positive sum
    return out


def _edge_base(material, n):
    t = np.arange(n)
    if material == "smooth":
        return np.rint((EDGE - 4096) * np.sin(2 * np.pi * t / 41.0 + 0.3)).astype(np.int64)
    return np.random.default_rng(4100 + n).integers(-(EDGE - 1), EDGE, size=n)


def _edge_blocks():
    """Twins that differ in one sample: +-2^24 (the streaming kernels) against +-(2^24 + 1) (the wide kernel)."""
    out = []
    for material in ("smooth", "noisy"):
        for n in EDGE_N:
            for sign in (1, -1):
                for extra, side in ((0, "narrow"), (1, "wide")):
                    x = _edge_base(material, n)
                    x[(2 * n) // 3] = sign * (EDGE + extra)
                    out.append((f"{material}_n{n}_{'plus' if sign > 0 else 'minus'}_{side}", clip32(x)))
    return out


def _full_blocks():
    n = 16384
    rng = np.random.default_rng(77)
    t = np.arange(n)
    out = [("smooth_sine_noise20", clip32(np.rint(np.sin(t / 90.0) * (1 << 29)).astype(np.int64) +
                                          rng.integers(-(1 << 20), 1 << 20, size=n)))]
    for seed, *_ in FULL_FALLBACK:
        out.append((f"fallback_seed{seed}", sines(seed, n)))
    out.append(("zero_runs", _zero_runs(n, 78, 3, 700)))
    return out


@functools.lru_cache(maxsize=None)
def corpus():
    """Every block of the corpus as (family, name, samples), in a fixed order."""
    out = []
    for seed, cand, used, order in FALLBACK:
        out.append(Block("fallback", f"seed{seed}_cand{cand}_levinson{used}_order{order}", sines(seed)))
    for seed, cand, used in EARLY:
        out.append(Block("early", f"seed{seed}_cand{cand}_levinson{used}", sines(seed)))
    for n in SMALL_N:
        for character in ("noise", "sine", "constant"):
            out.append(Block("small", f"{character}_n{n}", _small(n, character)))
    for n in GEOMETRY_N:
        for p in range(0 if max_partition_order(n) == 0 else 1, max_partition_order(n) + 1):
            out.append(Block("geometry", f"n{n}_p{p}", _geometry(n, p, GEOMETRY_SEEDS[n, p])))
    for seed, mode in MODES_48:
        out.append(Block("modes", f"unpartitioned_mode{mode}_seed{seed}", sines(seed, 48)))
    out.append(Block("modes", "zero_runs_n256_two_spikes", _zero_runs(256, 1, 1, 150)))
    out.append(Block("modes", "zero_runs_n1000_bursts", _zero_runs(1000, 2, 4, 90)))
    out.append(Block("modes", "bin_n512_rare_full_scale", _bin_material(512, 3, (128, 416), (I32_MAX, I32_MIN))))
    out.append(Block("modes", "bin_n1000_wide_first", _bin_material(1000, 4, (0,), EDGE + 1)))
    out.append(Block("modes", "bin_n1024_wide_middle", _bin_material(1024, 4, (512,), 1 << 27)))
    for name, x in _wrap_blocks():
        out.append(Block("wrap", name, x))
    for name, x in _edge_blocks():
        out.append(Block("edge", name, x))
    for seed, ptype, order in PREDICTORS:
        out.append(Block("predictors", f"seed{seed}_type{ptype}_order{order}", sines(seed)))
    for name, x in _full_blocks():
        out.append(Block("full", name, x))
    assert len({(b.family, b.name) for b in out}) == len(out)
    for b in out:
        b.x.setflags(write=False)
    return tuple(out)


FAMILIES = ("fallback", "early", "small", "geometry", "modes", "wrap", "edge", "predictors", "full")


def family(name):
    return tuple(b for b in corpus() if b.family == name)


def block(family_name, name):
    return next(b for b in corpus() if (b.family, b.name) == (family_name, name))


def sequence_blocks():
    """The one-handle sequence of the GPU test: wide n = 1024, narrow n = 300, wide n = 13, wide n = 16384, wide n = 5."""
    narrow = clip32(np.rint(30000 * np.sin(np.arange(300) / 11.0)))
    out = (block("geometry", "n1024_p5").x, narrow, block("small", "noise_n13").x, block("full", "zero_runs").x,
           block("small", "sine_n5").x)
    assert tuple(x.size for x in out) == SEQUENCE_N and [is_wide(x) for x in out] == [True, False, True, True, True]
    return out


# -- the oracle's records -----------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _oracle():
    import oracleshim

    oracleshim.lib()
    return oracleshim


@functools.lru_cache(maxsize=None)
def expected(family_name, zr=True, pt=True):
    """((block, wide slot record, oracle bytes), ...) of a family under one flag pair; computed once, shared."""
    o = _oracle()
    return tuple((b, planref.wide_slot_record(o, b.x, zr, pt), o.block_encode(b.x, zr, pt)) for b in family(family_name))


def classify(x, record):
    """(candidate order, Levinson order) of an LPC record: the candidate c of {4, 6, 8, 10, 12} whose analysis gives the
    plan's coefficients.  The plan carries all coefficients of the winning set, whatever order was emitted."""
    o = _oracle()
    plan = o.block_plan(x)
    assert plan.predictor_type == 2 and record.predictor_type == 2
    coef = [int(plan.coeffs_q15[i]) for i in range(13)]
    for c in (4, 6, 8, 10, 12):
        used, cc = o.lpc_analyze(x, c)
        if used > 0 and [int(v) for v in cc] + [0] * (12 - c) == coef:
            return c, used
    raise AssertionError("no candidate order gives the plan's coefficients")


def _modes(record):
    return {v >> 5 for v in record.part_mode_k}


def check_coverage(exp=None):
    """Every condition the corpus is there for, on the oracle's records with both flags on."""
    o = _oracle()
    exp = exp or {f: expected(f) for f in FAMILIES}
    # no block is left out, every block but the narrow twins is wide, sizes stay small
    assert sum(len(v) for v in exp.values()) == len(corpus())
    total = 0
    for f, rows in exp.items():
        for b, rec, data in rows:
            narrow = f == "edge" and b.name.endswith("_narrow")
            assert is_wide(b.x) != narrow, (f, b.name)
            assert 1 <= b.x.size <= (16384 if f in ("full", "wrap", "edge") else 1024), (f, b.name)
            assert len(data) <= MAX_BLOCK_BYTES, (f, b.name, len(data))
            total += len(data)
            if narrow:
                assert rec.payload_bytes == len(data), (f, b.name)  # inside the validated domain plan and emit agree
    assert total <= MAX_CORPUS_BYTES, total
    assert sum(1 for b in family("full")) <= 6 and all(b.x.size == 16384 for b in family("full"))

    # fallback winners: emitted order below min(Levinson order, candidate order), every single step and a longer one
    steps = set()
    for (b, rec, _), (seed, cand, used, order) in zip(exp["fallback"], FALLBACK):
        assert rec.predictor_type == 2 and (classify(b.x, rec), rec.order) == ((cand, used), order), (b.name, rec)
        assert rec.order < min(used, cand)
        steps.add((min(used, cand), rec.order))
    assert FALLBACK_STEPS <= steps and steps & FALLBACK_TWO_STEPS, steps
    full_fb = [(b, rec) for b, rec, _ in exp["full"] if b.name.startswith("fallback")]
    assert full_fb and all(rec.predictor_type == 2 and rec.order < min(classify(b.x, rec)) for b, rec in full_fb)
    # early-stopped recursions that still win
    early = set()
    for (b, rec, _), (seed, cand, used) in zip(exp["early"], EARLY):
        assert rec.predictor_type == 2 and classify(b.x, rec) == (cand, used) and rec.order == used < cand, (b.name, rec)
        early.add((used, cand))
    assert {(2, 4), (9, 10), (11, 12)} <= early

    # every small n at three characters
    assert {(b.x.size, b.name.split("_")[0]) for b in family("small")} == \
        {(n, c) for n in SMALL_N for c in ("noise", "sine", "constant")}
    assert set(range(1, 15)) | {31, 32, 33} == set(SMALL_N)
    assert any(rec.predictor_type == 2 for b, rec, _ in exp["small"])  # (an LPC plan below n = 14: order clamps)

    # partition geometry: every order the n allows, every mode inside a partition
    reached, part_modes = {}, set()
    for b, rec, _ in exp["geometry"]:
        reached.setdefault(b.x.size, set()).add(rec.partition_order)
        if rec.partition_order:
            part_modes |= _modes(rec)
            assert len(rec.part_mode_k) == 1 << rec.partition_order
    assert set(reached) == set(GEOMETRY_N)
    for n, orders in reached.items():
        assert set(range(1, max_partition_order(n) + 1)) <= orders, (n, orders)
    assert part_modes == {0, 1, 2, 3}, part_modes
    assert any(b.x.size % (1 << rec.partition_order) for b, rec, _ in exp["geometry"] if rec.partition_order)

    # modes: unpartitioned winners of each mode, zero runs with the escape, bin material
    unpart = {}
    for b, rec, _ in exp["modes"] + exp["small"]:
        if rec.partition_order == 0:
            unpart.setdefault(rec.part_mode_k[0] >> 5, b.name)
    assert set(unpart) == {0, 1, 2, 3}, unpart
    for (b, rec, _), (seed, mode) in zip(exp["modes"], MODES_48):
        assert rec.partition_order == 0 and rec.part_mode_k[0] >> 5 == mode, (b.name, rec)
    for b, rec, _ in exp["modes"]:
        if b.name.startswith("zero_runs"):
            assert 1 in _modes(rec), (b.name, rec)
        if b.name.startswith("bin"):  # (in a partition, or as the whole block when partitioning is off)
            assert 2 in _modes(rec) | _modes(planref.wide_slot_record(o, b.x, True, False)), (b.name, rec)
    assert any(2 in _modes(rec) and rec.partition_order for b, rec, _ in exp["modes"] if b.name.startswith("bin"))
    # the escape of the zero-run mode (u > 1 << min(k + 3, 24), 32 raw bits): a fixed order 0 plan in mode 1 whose
    # residual, the samples themselves, holds magnitudes above 2^24
    b, rec, _ = exp["modes"][len(MODES_48)]
    assert (rec.predictor_type, rec.order) == (0, 0) and _modes(rec) == {1}, rec
    assert is_wide(b.x)
    assert any(1 in _modes(rec) for b, rec, _ in exp["full"] if b.name == "zero_runs")

    # wrapping autocorrelation
    names = {b.name for b in family("wrap")}
    assert {f"constant_min_n{n}" for n in WRAP_CONSTANT_N} <= names
    r = o.autocorr(block("wrap", "constant_min_n2").x)
    assert r[0] == -2**63 and r[1] == 2**62
    assert o.autocorr(block("wrap", "constant_min_n4").x)[0] == 0          # 2^64: the clamp R[0] < 1 -> 1
    assert o.autocorr(block("wrap", "constant_min_n4096").x)[0] == 0
    r = o.autocorr(block("wrap", "r0_negative_r1_positive_n64").x)
    assert r[0] < 0 < r[1], r
    r = o.autocorr(block("wrap", "r0_wraps_past_zero_n300").x)
    assert 0 < r[0] < 2**50 and r[1] < 0, r
    assert any(n.startswith("alternating_extremes") for n in names)

    # the domain edge: twins on either side, one sample apart
    rows = {b.name: b for b in family("edge")}
    for name, b in rows.items():
        if name.endswith("_wide"):
            twin = rows[name[:-5] + "_narrow"]
            d = np.flatnonzero(b.x != twin.x)
            assert d.size == 1 and abs(int(b.x[d[0]])) == EDGE + 1 and abs(int(twin.x[d[0]])) == EDGE
            assert np.abs(twin.x.astype(np.int64)).max() == EDGE
    assert {f"{m}_n{n}_{s}_{w}" for m in ("smooth", "noisy") for n in EDGE_N for s in ("plus", "minus")
            for w in ("narrow", "wide")} == set(rows)

    # predictor types
    for (b, rec, _), (seed, ptype, order) in zip(exp["predictors"], PREDICTORS):
        assert (rec.predictor_type, rec.order) == (ptype, order), (b.name, rec)
    got = {(rec.predictor_type, rec.order) for _, rec, _ in exp["predictors"]}
    assert {(0, 0), (0, 1), (0, 2), (0, 3), (0, 4), (1, 2)} <= got

    # where the plan's size and the emitted size part (k = 31): the corpus holds such blocks
    assert any(rec.payload_bytes != len(data) for rows in exp.values() for _, rec, data in rows)
    return {f: len(rows) for f, rows in exp.items()}


def check_flag_coverage():
    """The subset that runs under the other three flag pairs still meets the fallback, partition-geometry and mode
    conditions there (what a flag rules out aside: no partition without partitioning, no mode 1 without zero runs)."""
    for zr, pt in FLAGS[1:]:
        exp = {f: expected(f, zr, pt) for f in FLAG_SUBSET}
        steps = set()
        for b, rec, _ in exp["fallback"]:
            if rec.predictor_type == 2:
                cand, used = classify(b.x, rec)
                if rec.order < min(used, cand):
                    steps.add((min(used, cand), rec.order))
        assert FALLBACK_STEPS <= steps and steps & FALLBACK_TWO_STEPS, (zr, pt, steps)
        want_modes = {0, 1, 2, 3} if zr else {0, 2, 3}
        rows = exp["geometry"] + exp["modes"]
        assert all(1 not in _modes(rec) for _, rec, _ in rows) or zr
        if pt:
            reached, part_modes = {}, set()
            for b, rec, _ in exp["geometry"]:
                reached.setdefault(b.x.size, set()).add(rec.partition_order)
                if rec.partition_order:
                    part_modes |= _modes(rec)
            for n, orders in reached.items():
                assert set(range(1, max_partition_order(n) + 1)) <= orders, (zr, pt, n, orders)
            assert part_modes == want_modes, (zr, pt, part_modes)
        else:
            assert all(rec.partition_order == 0 and len(rec.part_mode_k) == 1 for _, rec, _ in rows)
        unpart = {rec.part_mode_k[0] >> 5 for _, rec, _ in rows if rec.partition_order == 0}
        assert unpart == want_modes, (zr, pt, unpart)
