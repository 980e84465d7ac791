"""The corpus of the short-block tests (tests/test_short_blocks_host.py, tests/test_gpu_short_blocks.py) and the conditions
its oracle records must meet before a device is asked anything.  Plain helper module: numpy, the oracle and planref only,
no GPU, no test in here.

"Short" is a block of 1 to 4096 samples inside the streaming domain, |x| <= 2^24: the kernels of tests/narrowrecipes.py
(k_analyze<16,1024> with its fused emit, k_offsets / k_emit / k_pack, k_decide phase 2) where most of the 1024 threads
hold no sample, the last thread's chunk is partial, max_partition_order(n) falls from 7 to 0, a partition border falls
inside a chunk at almost every size, the 256-sample drift window and the 96-sample micro window never fill, LPC
candidates above min(32, n - 1) do not exist -- and, at stream level, the only place where both stereo pairs are encoded
in full and compared (a final block of <= 4096 frames in per-block stereo).  narrowrecipes starts at 4097.

Everything is built from explicit seeds; seeds found by search (always: seed = 0, 1, 2, ... through the oracle, first hit
kept) are frozen as literals next to what they were chosen for; nothing searches at import time.

Families
  lengths   every n in 1..130 and the border sizes BORDER_N, eleven characters each (CHARACTERS)
  geometry  narrowrecipes._geometry(n, p, seed) at GEOMETRY_N, every partition order 0..max the oracle lets win
  pairs     stereo pairs of the final-block tests (not part of corpus(): see pairs()): noise of amplitude 1, 3, 200 and
            30 000 (24 bit: 30 000 * 256), white or summed up to a random walk, the right channel independent,
            identical, negated, or left + {-1, 0, 1}, at PAIR_N (and at 4097, where probes replace the full comparison),
            at 16 and 24 bits

Nothing had to be left out.  Partition order 0 as the winner with partitioning on is rare above n = 500 (order 1 is taken
whenever it is within 5 % of the unpartitioned size): _geometry(n, 0, seed) needed seeds up to 191 there, all found within
seed 0..199, n = 300, 4095 and 4096 included.

What the oracle's rules do not allow, so that it is not asserted: a block of 5..12 samples without any LPC candidate.  The
reference drops a candidate only where its order exceeds min(32, n - 1) or where the recursion or the residual gives
order 0, and inside the 25-bit domain neither of the latter happens (tests/narrowrecipes.py, "left out").  So all five
candidates are absent at n <= 4, for every character, and from n = 5 on candidate 4 exists: check_coverage() asserts the
exact candidate set of every n <= 13, for every character, instead.

Likewise a partition border inside a thread's chunk at partition order 7: that order exists at n = 4096 alone, where
each partition is two whole chunks.  Orders 1..6 have such borders and check_coverage() asserts them.

The estimate alone decides a block (`uncertain == 0`: only the estimated pair is analysed, valid slots {0, 1} or
{2, 3}, `choose_ms == est_ms`, planref.expected_block) only where differences are cheaper than samples in all of L, R,
M and S.  White noise never does that beyond a few samples, so each pair also comes as a random walk (the running sum
of the same noise): with the walks every one of the five outcomes of check_coverage() occurs at every size.

Flag pairs: every block runs with (zero runs on, partitioning on); `geometry` and the border sizes of `lengths`
(flag_subset()) run under the other three pairs as well.

check_coverage() takes about 5 s on the CPU (1744 blocks, 865 pairs), check_flag_coverage() 2 s; the oracle's side of one
size of the final-block tests (records and bytes, all modes) 1 s, 4 s at 4095 and above.
"""
from __future__ import annotations

import functools
from collections import namedtuple

import numpy as np

import planref
from narrowrecipes import _geometry, i32
from widerecipes import FLAGS, Block, max_partition_order

EDGE = 1 << 24
FULL24, FULL16 = (1 << 23) - 1, (1 << 15) - 1
CHUNK = 16                            # samples per thread of k_analyze<16,1024>
LIMIT = planref.FULL_COMPARE_LIMIT    # 4096: the largest short block

SMALL_N = tuple(range(1, 131))
BORDER_N = (255, 256, 257, 271, 272, 273, 511, 512, 513, 1000, 1023, 1024, 1025, 2047, 2048, 2049, 3000, 4095, 4096)
LENGTH_N = SMALL_N + BORDER_N
GEOMETRY_N = (63, 64, 65, 95, 96, 97, 127, 128, 129, 255, 256, 257, 300, 511, 512, 513, 1000, 1023, 1024, 1025, 2047,
              2048, 2049, 4095, 4096)
PAIR_N = (1, 2, 3, 5, 13, 16, 17, 31, 33, 64, 100, 255, 256, 257, 1000, 4095, 4096)
PAIR_CONTRAST_N = 4097                # probes replace the full comparison
PAIR_AMPLITUDES = (1, 3, 200, 30000)
PAIR_RELATIONS = ("independent", "identical", "negated", "near")
PAIR_MATERIALS = ("noise", "walk")
WALK_AMPLITUDES = (1, 200)
RATE = 48000
BLOCK = planref.BLOCK
FRONT_SEED = 5                        # the full blocks in front of a final block: synth music of this seed
CHARACTERS = ("noise24", "noise8", "sine", "alternating", "constant", "zeros", "last_one", "first_edge", "ramp", "runs",
              "tone")
FAMILIES = ("lengths", "geometry")


def _character(name, n):
    """One block of `n` samples of a character of the family `lengths`."""
    rng = np.random.default_rng([31, CHARACTERS.index(name), n])
    t = np.arange(n, dtype=np.int64)
    if name == "noise24":        # full-scale 24-bit noise
        return i32(rng.integers(-FULL24 - 1, FULL24 + 1, size=n))
    if name == "noise8":         # noise of +-8
        return i32(rng.integers(-8, 9, size=n))
    if name == "sine":           # a full-scale sine of period 7.3
        return i32(np.rint(FULL24 * np.sin(2 * np.pi * t / 7.3 + 0.5)))
    if name == "alternating":    # +-2^24 in turn
        return i32(np.where(t % 2 == 0, EDGE, -EDGE))
    if name == "constant":
        return i32(np.full(n, -EDGE))
    x = np.zeros(n, dtype=np.int64)
    if name == "last_one":
        x[-1] = 1
    elif name == "first_edge":
        x[0] = EDGE
    elif name == "ramp":         # a ramp three times as steep as the range allows, clipped at both ends
        x = np.clip(((2 * t - (n - 1)) * 3 * (FULL24 + 1)) // n, -FULL24 - 1, FULL24)
    elif name == "runs":         # 0 .. +-3, zero runs of five on a period of fifteen
        x = rng.integers(-3, 4, size=n)
        x[t % 15 < 5] = 0
    elif name == "tone":         # a tone plus small noise
        x = np.rint(30000 * np.sin(2 * np.pi * t / 23.7 + 0.2)).astype(np.int64) + rng.integers(-16, 17, size=n)
    return i32(x)


# -- frozen results of the searches -------------------------------------------------------------------------------------

# seed of _geometry(n, p, seed): the first seed whose oracle plan has partition order p (0 everywhere but here)
GEOMETRY_SEEDS = {
    (64, 0): 1, (65, 0): 1, (95, 0): 2, (96, 0): 6, (97, 0): 1, (127, 0): 6, (128, 0): 12, (129, 0): 1, (256, 0): 4,
    (257, 0): 2, (300, 0): 3, (300, 3): 1, (511, 0): 40, (512, 0): 3, (513, 0): 18, (1000, 0): 77, (1023, 0): 165,
    (1024, 0): 38, (1025, 0): 25, (1025, 3): 2, (2047, 0): 191, (2048, 0): 122, (2048, 5): 1, (2049, 0): 62,
    (2049, 3): 1, (4095, 0): 35, (4096, 0): 24, (4096, 2): 2}
# the smallest n of the family `lengths` at which each LPC order wins: the first n at which the candidate exists
SMALLEST_LPC_N = {4: 5, 6: 7, 8: 9, 10: 11, 12: 13}
# LPC candidates that exist at n, for every character of `lengths` (all five from n = 13 on)
LPC_CANDIDATES = {1: (), 2: (), 3: (), 4: (), 5: (4,), 6: (4,), 7: (4, 6), 8: (4, 6), 9: (4, 6, 8), 10: (4, 6, 8),
                  11: (4, 6, 8, 10), 12: (4, 6, 8, 10), 13: (4, 6, 8, 10, 12)}
# extra pairs (bits, n, amplitude, relation, material, seed) beside seed 0: left/right strictly smaller at n = 1
PAIR_EXTRA = ((24, 1, 200, "independent", "noise", 12),)
WANT_PREDICTORS = {(0, 0), (0, 1), (0, 2), (0, 3), (0, 4), (1, 2), (2, 4), (2, 6), (2, 8), (2, 10), (2, 12)}


@functools.lru_cache(maxsize=None)
def corpus():
    """Every block of the corpus as (family, name, samples), in a fixed order: sizes ascend, characters alternate."""
    out = []
    for n in LENGTH_N:
        for c in CHARACTERS:
            out.append(Block("lengths", f"{c}_n{n}", _character(c, n)))
    for n in GEOMETRY_N:
        for p in range(0, max_partition_order(n) + 1):
            out.append(Block("geometry", f"n{n}_p{p}", _geometry(n, p, GEOMETRY_SEEDS.get((n, p), 0))))
    assert len({(b.family, b.name) for b in out}) == len(out)
    for b in out:
        assert 1 <= b.x.size <= LIMIT and np.abs(b.x.astype(np.int64)).max() <= EDGE, (b.family, b.name)
        b.x.setflags(write=False)
    return tuple(out)


def family(name, sizes=None):
    """The blocks of a family in corpus order; sizes: only those of these sizes."""
    return tuple(b for b in corpus() if b.family == name and (sizes is None or b.x.size in sizes))


def block(family_name, name):
    return next(b for b in corpus() if (b.family, b.name) == (family_name, name))


def flag_subset():
    """What runs under the other three flag pairs: `geometry` and the border sizes of `lengths`."""
    return family("geometry") + family("lengths", BORDER_N)


def small_and_subset():
    """What runs under the simulator's variants: the flag subset and every block of n <= 130."""
    return family("lengths", SMALL_N) + flag_subset()


LENGTH_SLICES = (SMALL_N[:17], SMALL_N[17:45], SMALL_N[45:73], SMALL_N[73:101], SMALL_N[101:], BORDER_N[:9], BORDER_N[9:])


def fits(x, bits):
    x = np.asarray(x, dtype=np.int64)
    return bool(x.min() >= -(1 << (bits - 1)) and x.max() < (1 << (bits - 1)))


def stream_form(x):
    """A corpus block as the channel of a 24-bit stream: a stream refuses samples outside its bit depth, so the +-2^24 of
    the characters `alternating`, `constant` and `first_edge` become the 24-bit full scale; every other block is
    unchanged."""
    return np.clip(x, -FULL24 - 1, FULL24).astype(np.int32)


# -- pairs --------------------------------------------------------------------------------------------------------------

Pair = namedtuple("Pair", "name bits n left right")


def _pair(bits, n, amp, relation, material="noise", seed=0):
    rng = np.random.default_rng([37, bits, n, amp, PAIR_RELATIONS.index(relation), PAIR_MATERIALS.index(material), seed])
    a = amp << 8 if (bits == 24 and amp == PAIR_AMPLITUDES[-1]) else amp
    full = (1 << (bits - 1)) - 1

    def draw():
        x = rng.integers(-a, a + 1, size=n)
        return x if material == "noise" else np.clip(np.cumsum(x), -(full >> 1), full >> 1)

    left = draw()
    if relation == "independent":
        right = draw()
    elif relation == "identical":
        right = left.copy()
    elif relation == "negated":
        right = -left
    else:
        right = left + rng.integers(-1, 2, size=n)
    assert fits(left, bits) and fits(right, bits)
    return left.astype(np.int32), right.astype(np.int32)


@functools.lru_cache(maxsize=None)
def pairs(bits, n):
    """The pairs of one size at one bit depth: amplitude x relation as white noise (16), as random walks at the amplitudes
    WALK_AMPLITUDES (8), and the extra ones of that size."""
    todo = [(amp, rel, "noise", 0) for amp in PAIR_AMPLITUDES for rel in PAIR_RELATIONS]
    todo += [(amp, rel, "walk", 0) for amp in WALK_AMPLITUDES for rel in PAIR_RELATIONS]
    todo += [e[2:] for e in PAIR_EXTRA if e[:2] == (bits, n)]
    out = []
    for amp, rel, mat, seed in todo:
        left, right = _pair(bits, n, amp, rel, mat, seed)
        left.setflags(write=False)
        right.setflags(write=False)
        out.append(Pair(f"{mat}_{rel}_amp{amp}_seed{seed}_n{n}_{bits}bit", bits, n, left, right))
    return tuple(out)



OUTCOMES = ("lr_smaller", "ms_smaller", "tie_nonsilent", "estimate_lr", "estimate_ms")


def outcome(record, left, right):
    """Which of the five outcomes a mode-2 BlockRecord of a short block shows.  By planref.expected_block an uncertain block
    of <= 4096 frames has the four whole-block slots valid and `choose_ms` = (M + S strictly smaller than L + R); a
    certain one has only the estimated pair valid, {0, 1} or {2, 3}, and `choose_ms` = `est_ms`: the last two outcomes
    are told apart by the valid set and by `choose_ms` alike."""
    assert record.frames <= LIMIT
    if not record.uncertain:
        assert sorted(record.slots) == ([2, 3] if record.est_ms else [0, 1]) and record.choose_ms == record.est_ms
        return "estimate_ms" if record.est_ms else "estimate_lr"
    assert sorted(record.slots) == [0, 1, 2, 3]
    lr = record.slots[0].payload_bytes + record.slots[1].payload_bytes
    ms = record.slots[2].payload_bytes + record.slots[3].payload_bytes
    assert record.choose_ms == int(ms < lr)
    if ms < lr:
        return "ms_smaller"
    if lr < ms:
        return "lr_smaller"
    return "tie_nonsilent" if (left.any() or right.any()) else "tie_silent"


class _MemoOracle:
    """The oracle with its per-block answers remembered by content (as planrecipes._MemoOracle): the streams of the
    final-block tests share their full blocks, and a stream is analysed in several modes."""

    def __init__(self):
        import hashlib
        import oracleshim

        oracleshim.lib()
        self._o, self._memo, self._hash = oracleshim, {}, hashlib.blake2b

    def _get(self, fn, args, zr=True, pt=True):
        arrays = [np.ascontiguousarray(a, dtype=np.int32) for a in args]
        key = (fn.__name__, tuple(self._hash(a.tobytes(), digest_size=16).digest() for a in arrays), bool(zr), bool(pt))
        if key not in self._memo:
            self._memo[key] = fn(*arrays) if fn is self._o.stereo_estimate else fn(*arrays, zr, pt)
        return self._memo[key]

    def block_plan(self, x, zr=True, pt=True):
        return self._get(self._o.block_plan, (x,), zr, pt)

    def block_encode(self, x, zr=True, pt=True):
        return self._get(self._o.block_encode, (x,), zr, pt)

    def stereo_estimate(self, left, right):
        return self._get(self._o.stereo_estimate, (left, right))

    def __getattr__(self, name):
        return getattr(self._o, name)


@functools.lru_cache(maxsize=None)
def oracle():
    return _MemoOracle()


@functools.lru_cache(maxsize=None)
def pair_records(bits, n):
    """The mode-2 BlockRecord of every pair of one size as a block of its own."""
    return tuple(planref.expected_block(oracle(), p.left, p.right, 2) for p in pairs(bits, n))


def outcome_pairs(bits, n):
    """Indices into pairs(bits, n) of the first pair of each outcome that the size reaches."""
    first = {}
    for i, (p, rec) in enumerate(zip(pairs(bits, n), pair_records(bits, n))):
        first.setdefault(outcome(rec, p.left, p.right), i)
    return tuple(sorted(first.values()))


# -- final blocks: a pair behind zero, one or two full blocks ------------------------------------------------------------

FRONTS = (0, 1, 2)
STREAM_MODES = (0, 1, 2, "mono")


@functools.lru_cache(maxsize=None)
def front(bits):
    """Two full blocks of stereo music (synth, seed FRONT_SEED) at one bit depth."""
    import __graft_entry__ as ge

    left, right = ge.load_pkg().synth.synth_pcm(2 * BLOCK, 2, bits, RATE, seed=FRONT_SEED, kind="music")
    left, right = left.astype(np.int32), right.astype(np.int32)
    left.setflags(write=False)
    right.setflags(write=False)
    return left, right


@functools.lru_cache(maxsize=None)
def final_streams(bits, n):
    """((name, full blocks in front, left, right), ...): every pair of the size behind 0, 1 and 2 full blocks."""
    fl, fr = front(bits)
    out = []
    for p in pairs(bits, n):
        for k in FRONTS:
            out.append((f"{p.name}_behind{k}", k, np.concatenate([fl[:k * BLOCK], p.left]),
                        np.concatenate([fr[:k * BLOCK], p.right])))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def expected_final(bits, n, mode):
    """The BlockRecords of every stream of final_streams(bits, n) in one stereo mode (or "mono": the left channel)."""
    o = oracle()
    return tuple(tuple(planref.expected_stream(o, left, None if mode == "mono" else right, 0 if mode == "mono" else mode))
                 for _, _, left, right in final_streams(bits, n))


@functools.lru_cache(maxsize=None)
def _front_bytes(bits, k, mode):
    fl, fr = front(bits)
    return oracle().encode(fl[:k * BLOCK], None if mode == "mono" else fr[:k * BLOCK], RATE, bits,
                           0 if mode == "mono" else mode, threads=8)


def stream_bytes(bits, k, left, right, mode, direct=False):
    """oracle.encode(..., threads=8) of a stream of final_streams().  The reference encodes every block from its own
    frames alone, so behind k full blocks the stream is the oracle's encode of the k blocks (computed once per depth,
    k and mode) spliced with the oracle's encode of the final block: 40 ms saved per stream.  direct=True: the oracle's
    encode of the whole stream, which final_bytes() holds the splice against for a sample of every size."""
    import lacstreams

    sm = 0 if mode == "mono" else mode
    right = None if mode == "mono" else right
    if direct or k == 0:
        return oracle().encode(left, right, RATE, bits, sm, threads=8)
    tail = oracle().encode(left[k * BLOCK:], None if right is None else right[k * BLOCK:], RATE, bits, sm, threads=8)
    return lacstreams.splice(_front_bytes(bits, k, mode), tail)


@functools.lru_cache(maxsize=None)
def final_bytes(bits, n, mode):
    """The oracle's bytes of every stream of final_streams(bits, n) in one mode.  The streams of the size's first pair and
    of its outcome_pairs() are encoded whole as well, and the spliced form must equal that."""
    streams = final_streams(bits, n)
    out = tuple(stream_bytes(bits, k, left, right, mode) for _, k, left, right in streams)
    whole = {0} | (set(outcome_pairs(bits, n)) if (mode == 2 and n <= LIMIT) else set())
    for i in sorted(whole):
        for j in range(i * len(FRONTS), (i + 1) * len(FRONTS)):
            name, k, left, right = streams[j]
            assert out[j] == stream_bytes(bits, k, left, right, mode, direct=True), (name, mode)
    return out


# -- the oracle's records -----------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def expected(family_name, zr=True, pt=True, sizes=None):
    """((block, slot record, oracle bytes), ...) of a family (or of its blocks of `sizes`) under one flag pair; computed
    once, shared."""
    if sizes is not None:
        return tuple(row for row in expected(family_name, zr, pt) if row[0].x.size in sizes)
    o = oracle()
    return tuple((b, planref.slot_record(o, b.x, zr, pt), o.block_encode(b.x, zr, pt)) for b in family(family_name))


def expected_subset(zr, pt):
    return expected("geometry", zr, pt) + expected("lengths", zr, pt, BORDER_N)


def _modes(record):
    return {v >> 5 for v in record.part_mode_k}


def lpc_candidates(x):
    """The LPC candidate orders that exist for a block: at most min(32, n - 1), and the recursion must not stop at 0."""
    o = oracle()
    limit = min(32, x.size - 1) if x.size > 1 else 0
    return tuple(c for c in (4, 6, 8, 10, 12) if c <= limit and o.lpc_analyze(x, c)[0] > 0)


@functools.lru_cache(maxsize=None)
def check_coverage():
    """Every condition the corpus is there for, on the oracle's records with both flags on."""
    exp = {f: expected(f) for f in FAMILIES}
    assert sum(len(v) for v in exp.values()) == len(corpus())
    assert len(exp["lengths"]) == len(LENGTH_N) * len(CHARACTERS) and set(SMALL_N) == set(range(1, 131))
    for rows in exp.values():
        for b, rec, data in rows:
            assert rec.payload_bytes == len(data), b.name  # inside the validated domain plan and emit agree

    # geometry: every order 0..max at every size, all modes inside partitions
    reached, part_modes, inside = {}, set(), set()
    for b, rec, _ in exp["geometry"]:
        n, p = b.x.size, rec.partition_order
        assert b.name == f"n{n}_p{p}", (b.name, p)
        assert len(rec.part_mode_k) == 1 << p
        reached.setdefault(n, set()).add(p)
        if p:
            part_modes |= _modes(rec)
            if n % (CHUNK << p):
                inside.add(p)
    want = {n: set(range(0, max_partition_order(n) + 1)) for n in GEOMETRY_N}
    assert reached == want, {n: sorted(want[n] - reached.get(n, set())) for n in GEOMETRY_N if want[n] != reached.get(n)}
    assert {n: max_partition_order(n) for n in (63, 64, 127, 128, 255, 256, 511, 512, 1023, 1024, 2047, 2048, 4095, 4096)} == \
        {63: 0, 64: 1, 127: 1, 128: 2, 255: 2, 256: 3, 511: 3, 512: 4, 1023: 4, 1024: 5, 2047: 5, 2048: 6, 4095: 6, 4096: 7}
    assert part_modes == {0, 1, 2, 3}, part_modes
    # a partition border inside a thread's chunk at every order that allows one: order 7 exists at n = 4096 alone
    # (max_partition_order(4095) == 6), where the 128 partitions are two whole chunks each
    assert inside == set(range(1, 7)), inside
    assert [n for n in range(1, LIMIT + 1) if max_partition_order(n) == 7] == [LIMIT] and LIMIT % (CHUNK << 7) == 0

    # predictors over both families; the smallest n at which each LPC order wins in `lengths`
    rows = exp["lengths"] + exp["geometry"]
    got = {(rec.predictor_type, rec.order) for _, rec, _ in rows}
    assert WANT_PREDICTORS <= got, sorted(WANT_PREDICTORS - got)
    smallest = {}
    for b, rec, _ in exp["lengths"]:
        if rec.predictor_type == 2:
            smallest.setdefault(rec.order, b.x.size)
    assert {k: smallest[k] for k in (4, 6, 8, 10, 12)} == SMALLEST_LPC_N, smallest

    # the LPC candidates that exist at n <= 13: none up to n = 4, one more at every odd n from 5 on, for every character
    # (the module docstring says why no block of 5..12 samples is without a candidate)
    for n, want in LPC_CANDIDATES.items():
        assert all(lpc_candidates(b.x) == want for b in family("lengths", (n,))), n

    # the full comparison of the pairs: each outcome at >= 3 sizes, n = 1 and n = 4096 among them
    sizes = {k: set() for k in OUTCOMES}
    for bits in (16, 24):
        for n in PAIR_N:
            for p, rec in zip(pairs(bits, n), pair_records(bits, n)):
                k = outcome(rec, p.left, p.right)
                if k in sizes:
                    sizes[k].add(n)
    for k, at in sizes.items():
        assert len(at) >= 3 and {1, LIMIT} <= at, (k, sorted(at))
    for bits in (16, 24):  # the contrast: probes, no full comparison
        recs = [planref.expected_block(oracle(), p.left, p.right, 2) for p in pairs(bits, PAIR_CONTRAST_N)]
        assert any(r.uncertain and r.margin is not None and sorted(r.slots)[2:] == list(range(4, 16)) for r in recs)
        assert all(not (r.uncertain and set(r.slots) >= {0, 1, 2, 3}) for r in recs)
    return {f: len(v) for f, v in exp.items()}


# winners of the subset without partitioning: modes of the unpartitioned block, by zero runs on / off
UNPARTITIONED_MODES = {True: {0, 1, 2, 3}, False: {0, 2, 3}}


@functools.lru_cache(maxsize=None)
def check_flag_coverage():
    """The flag subset under the other three flag pairs: no partition without partitioning, no mode 1 without zero runs,
    residual modes 0..3 as the unpartitioned winner with partitioning off, and with the flags off the subset still has
    winners that differ from the flags-on plan."""
    base = expected_subset(True, True)
    differ = {}
    for zr, pt in FLAGS[1:]:
        rows = expected_subset(zr, pt)
        assert len(rows) == len(base) == len(flag_subset())
        if not zr:
            assert all(1 not in _modes(rec) for _, rec, _ in rows)
        if pt:
            part_modes = set().union(*(_modes(rec) for _, rec, _ in rows if rec.partition_order))
            assert part_modes == UNPARTITIONED_MODES[zr], (zr, pt, part_modes)
            orders = {rec.partition_order for _, rec, _ in rows}
            assert orders == set(range(8)), (zr, pt, orders)
        else:
            assert all(rec.partition_order == 0 and len(rec.part_mode_k) == 1 for _, rec, _ in rows)
            unpart = {rec.part_mode_k[0] >> 5 for _, rec, _ in rows}
            assert unpart == UNPARTITIONED_MODES[zr], (zr, pt, unpart)
        differ[zr, pt] = sum(1 for (_, a, da), (_, b, db) in zip(base, rows) if da != db)
        assert differ[zr, pt] >= len(base) // 4, differ
    return differ
