"""Candidate masks for the predictor search, the blocks and streams they run on, and the conditions the masked oracle's
records must meet before a device is asked anything (tests/test_forced_candidates_host.py,
tests/test_gpu_forced_candidates.py).  Plain helper module: numpy and the oracle only, no GPU, no test in here.

Why it exists.  The search of k_analyze runs eleven candidates per channel block -- fixed orders 0..4, the 2-tap FIR
predictor, LPC orders 4, 6, 8, 10, 12; candidate index 0..10 in that order -- and everything outside the kernel sees the
winner alone.  A mask takes candidates out of the search, so that each candidate's residual, costs, partition search
and emit are compared with the oracle on every block, not only on the blocks it happens to win.

  device   LACX_DEBUG_SKIP bit 21 + c removes candidate c (liblacx_hooks.so only; csrc/k_analyze.hip)
  oracle   bit c of the mask of laco_block_plan_masked / laco_block_encode_masked / laco_encode_masked

Two rules, the same on both sides: a slot of nothing but zeros is searched as ever (MASK_SILENT), and so is a slot for
which the mask leaves no candidate that is available (MASK_NONE_LEFT: an LPC order above n - 1, or one whose recursion
stopped at once).  Mask 0 is the pinned oracle, bit for bit.

The masked oracle cannot be held against the reference (which cannot force a candidate); the host module pins it by the
reference decoder's round trip, by the bit count the grammar derives from record and samples, and by the minimum over
the eleven single-candidate plans being the pinned plan.

Measured on the oracle (check_coverage asserts the conditions, the figures are what it found):
  * part a (112 narrow blocks x 11 single-candidate masks): the mask is ignored in 0 of 1232 cases -- no block of the
    narrow corpus is silent, every block has more than 12 samples, and no Levinson recursion stops at order 0 inside the
    25-bit domain (tests/narrowrecipes.py says why);
  * every candidate reaches, on at least one block each, a partition order above 1, a static partition (mode 3), an
    adaptive Rice partition (mode 0) and a zero-run partition (mode 1); bin partitions (mode 2) as well.  No class is
    missing for any candidate;
  * part b (105 short geometry blocks and the 143 blocks of 1..13 samples): MASK_SILENT on the all-zero blocks,
    MASK_NONE_LEFT exactly where the one candidate left is an LPC order that does not exist for the block.

Pairs (PAIRS): two candidates left in the search, chosen once on the oracle's single-candidate costs (the cost the
reference compares, block/encoder.cpp:337-359) and frozen here.  `tie`: equal costs, the lower index must win.  `later`:
the candidate later in the reference's order wins by at most 0.5 %; `earlier`: the earlier one does.  The device does not
evaluate in the reference's order but in the order of its pruning bounds, so which of the two is the last one the device
evaluates -- the winner handed over in LDS, or re-derived -- is not something the oracle states; with costs this close
neither candidate can be pruned and both orders of winner and loser occur over the list.

The seven plain siblings (SIBLING_BITS) each replace an optimised path of the kernel by its plain form and leave the plan
as it is (read from csrc/k_analyze.hip): 128 no pruning (every available candidate is costed; the minimum of (cost,
index) is the same), 16384 the winner is always re-derived, 32768 the partition walk over every sample and order, 131072
one atomic per lane in the segment flush, 262144 plane counts instead of k-sums, 524288 every chunk walked in phase B,
1048576 all sixteen static parameters costed.  The simulator has the matching variant for three of them (SIM_VARIANTS).
"""
from __future__ import annotations

import functools
from collections import namedtuple
from concurrent.futures import ThreadPoolExecutor

import narrowrecipes as N
import oracleshim as O
import planrecipes as P
import planref
import shortrecipes as S

CANDIDATES = ("fixed0", "fixed1", "fixed2", "fixed3", "fixed4", "fir", "lpc4", "lpc6", "lpc8", "lpc10", "lpc12")
NC = len(CANDIDATES)
HOOK_SHIFT = 21  # LACX_DEBUG_SKIP bit 21 + c
RATE = 48000

Row = namedtuple("Row", "block record data rule")


def only(*cands):
    """The mask that leaves exactly these candidates in the search."""
    m = O.MASK_ALL
    for c in cands:
        m &= ~(1 << c)
    return m


SINGLE = tuple(only(c) for c in range(NC))


def debug_skip(mask, extra=0):
    """The value of LACX_DEBUG_SKIP for a mask (and further hook bits)."""
    assert 0 <= mask <= O.MASK_ALL and extra < (1 << HOOK_SHIFT)
    return str((mask << HOOK_SHIFT) | extra)


def predictor_of(c):
    """(predictor type, order parameter) of candidate c."""
    return (0, c) if c < 5 else (1, 2) if c == 5 else (2, 4 + 2 * (c - 6))


def is_candidate(record, c):
    """The record's predictor is candidate c (an LPC order may come out lower than asked: the recursion stopped)."""
    ptype, order = predictor_of(c)
    return record.predictor_type == ptype and (record.order == order if ptype < 2 else 1 <= record.order <= order)


def _map(fn, items):
    """fn over the items on eight threads, in order (the oracle runs outside the interpreter lock)."""
    with ThreadPoolExecutor(max_workers=8) as pool:
        return tuple(pool.map(fn, items))


def _row(b, mask, zr, pt):
    op, rule, data = O.block_plan_encode_masked(b.x, zr, pt, mask)
    coef = tuple(int(op.coeffs_q15[i + 1]) for i in range(op.order)) if op.predictor_type == 2 else ()
    pmk = tuple((int(op.part_mode[i]) << 5) | int(op.part_k[i]) for i in range(op.part_count))
    rec = planref.SlotRecord(int(op.predictor_type), int(op.order), int(op.partition_order), coef, pmk, int(op.total_bits),
                             len(data), 0, int(b.x.size))
    return Row(b, rec, data, rule)


@functools.lru_cache(maxsize=None)
def expected(family, mask, zr=True, pt=True):
    """(Row, ...) of a family of the narrow corpus under a mask and a flag pair; computed once, shared."""
    return _map(lambda b: _row(b, mask, zr, pt), N.family(family))


SHORT_SMALL_N = tuple(range(1, 14))  # 13: the first size at which all five LPC orders exist


def short_blocks():
    """Part b: the `geometry` family of the short corpus (63..4096 samples) and every block of 1..13 samples."""
    return S.family("geometry") + S.family("lengths", SHORT_SMALL_N)


@functools.lru_cache(maxsize=None)
def expected_short(mask, zr=True, pt=True):
    return _map(lambda b: _row(b, mask, zr, pt), short_blocks())


def short_rule(x, c):
    """The rule that must apply to a short block when candidate c alone is left, from the samples alone."""
    if not x.any():
        return O.MASK_SILENT
    if c >= 6 and predictor_of(c)[1] not in S.lpc_candidates(x):
        return O.MASK_NONE_LEFT
    return O.MASK_APPLIED


# (kind, family, block, candidate a < candidate b): found once by scanning the single-candidate costs of the narrow
# corpus (partitioning off) in corpus order; see the module docstring
PAIRS = (
    ("tie", "geometry", "n12289_p8", 9, 10), ("tie", "tokens", "sparse_escapes_n16384", 0, 6),
    ("tie", "tokens", "bin_n16384", 6, 10), ("tie", "tokens", "sparse_escapes_n12289", 0, 10),
    ("later", "geometry", "n4097_p2", 9, 10), ("later", "geometry", "n8192_p4", 6, 8),
    ("later", "geometry", "n8191_p3", 1, 5), ("later", "geometry", "n8192_p7", 0, 6),
    ("earlier", "geometry", "n4097_p1", 0, 6), ("earlier", "geometry", "n4097_p6", 7, 10),
    ("earlier", "geometry", "n4097_p4", 1, 9), ("earlier", "geometry", "n4097_p7", 5, 7),
)
PAIR_CLOSE = 200  # the loser's cost is within 1 / 200 of the winner's


def single_cost(x, c):
    """The cost the reference compares for candidate c (None where c is not available for the block)."""
    op, rule = O.block_plan_masked(x, True, False, SINGLE[c])
    return int(op.best_bits) if rule == O.MASK_APPLIED else None


@functools.lru_cache(maxsize=None)
def pair_rows():
    """((kind, a, b, mask, Row), ...) with both flags on."""
    out = []
    for kind, family, name, a, b in PAIRS:
        mask = only(a, b)
        out.append((kind, a, b, mask, _row(N.block(family, name), mask, True, True)))
    return tuple(out)


def stream():
    """Part e: the first stream of the narrow corpus (15 full blocks and a ragged one per channel, 24 bit)."""
    name, bits, left, right = N.streams()[0]
    assert left.size // N.BLOCK == 15 and left.size % N.BLOCK
    return name, bits, left, right


STREAM_MODES = (0, 1, 2)


@functools.lru_cache(maxsize=None)
def stream_bytes(mask, mode):
    name, bits, left, right = stream()
    return O.encode_masked(left, right, RATE, bits, mode, True, True, 8, mask)


PROBE_BITS = (16, 24)


@functools.lru_cache(maxsize=None)
def expected_probes(bits, mask):
    """Part d: planrecipes' case a (56 blocks, every one probed) in per-block stereo under a mask."""
    left, right = P.stream_a(bits)
    starts = range(0, int(left.size), planref.BLOCK)
    return _map(lambda a: planref.expected_block(O, left[a:a + planref.BLOCK], right[a:a + planref.BLOCK], 2, mask=mask), starts)


SIBLING_BITS = (128, 16384, 32768, 131072, 262144, 524288, 1048576)
SIM_VARIANTS = {128: 4, 32768: 8, 524288: 16}  # hook bit -> `force_wide` bit of tests/native/sim_analyze.cpp

IGNORED_SHARE_CAP = 10        # part a: the mask may be ignored in at most 1 of 10 (block, candidate) cases ...
IGNORED_PER_CANDIDATE = 2     # ... and for no candidate on more than 1 of 2 of its blocks
CLASSES = ("order_above_1", "static", "adaptive", "zero_run")


def classes_of(record):
    modes = {v >> 5 for v in record.part_mode_k}
    return {name for name, hit in zip(CLASSES, (record.partition_order > 1, 3 in modes, 0 in modes, 1 in modes)) if hit}


@functools.lru_cache(maxsize=None)
def check_coverage():
    """The conditions of the module docstring, on the oracle alone.  Returns the measured figures."""
    O.lib()
    blocks = len(N.corpus())
    ignored, reached = [0] * NC, [set() for _ in range(NC)]
    for c in range(NC):
        rows = [r for f in N.FAMILIES for r in expected(f, SINGLE[c])]
        assert len(rows) == blocks
        for r in rows:
            if r.rule != O.MASK_APPLIED:
                ignored[c] += 1
                continue
            assert is_candidate(r.record, c), (CANDIDATES[c], r.block.name, r.record.predictor_type, r.record.order)
            reached[c] |= classes_of(r.record)
    assert sum(ignored) * IGNORED_SHARE_CAP <= blocks * NC, ignored
    assert all(n * IGNORED_PER_CANDIDATE <= blocks for n in ignored), ignored
    missing = {CANDIDATES[c]: sorted(set(CLASSES) - reached[c]) for c in range(NC) if reached[c] != set(CLASSES)}
    assert not missing, missing

    # part b: which rule applies where, from the samples alone
    rules = {O.MASK_APPLIED: 0, O.MASK_NONE_LEFT: 0, O.MASK_SILENT: 0}
    for c in range(NC):
        rows = expected_short(SINGLE[c])
        assert len(rows) == len(short_blocks()) == 105 + len(SHORT_SMALL_N) * len(S.CHARACTERS)
        for r in rows:
            assert r.rule == short_rule(r.block.x, c), (CANDIDATES[c], r.block.name, r.rule)
            rules[r.rule] += 1
            if r.rule == O.MASK_APPLIED:
                assert is_candidate(r.record, c), (CANDIDATES[c], r.block.name)
            else:  # the mask had no effect: the pinned plan
                assert r.data == O.block_encode(r.block.x), (CANDIDATES[c], r.block.name)
    assert min(rules.values()) > 0, rules
    small = [r for c in range(6, NC) for r in expected_short(SINGLE[c]) if r.block.x.size <= 12 and r.block.x.any()]
    assert small and any(r.rule == O.MASK_NONE_LEFT for r in small) and any(r.rule == O.MASK_APPLIED for r in small)

    # part c: the frozen pairs are what they were chosen for
    kinds = set()
    for kind, a, b, mask, row in pair_rows():
        ca, cb = single_cost(row.block.x, a), single_cost(row.block.x, b)
        assert a < b and ca is not None and cb is not None and row.rule == O.MASK_APPLIED
        if kind == "tie":
            assert ca == cb and is_candidate(row.record, a) and row.record.predictor_type == predictor_of(a)[0]
        elif kind == "later":
            assert cb < ca <= cb + cb // PAIR_CLOSE and is_candidate(row.record, b), (row.block.name, ca, cb)
        else:
            assert ca < cb <= ca + ca // PAIR_CLOSE and is_candidate(row.record, a), (row.block.name, ca, cb)
        kinds.add(kind)
    assert kinds == {"tie", "later", "earlier"}
    return {"ignored": sum(ignored), "cases": blocks * NC, "short_rules": rules}
