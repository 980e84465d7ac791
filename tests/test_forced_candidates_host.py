"""The masked oracle (oracle/lac_oracle.c: laco_block_plan_masked, laco_block_encode_masked, laco_encode_masked) without a
GPU.  The reference cannot force a candidate, so the variants are pinned otherwise:

  mask 0      is the pinned function, bit for bit: plans, block bytes, stream bytes;
  round trip  every masked block encode decodes with the unmodified reference to the input samples (where the reference
              build exists): inside a 24-bit stream through LAC::Decoder (mono, or as the side channel of a mid/side
              block up to +-(2^24 - 1)), and through Block::Decoder itself where the build has the shim's block entry
              point (a prebuilt oracle/_ref from before it has not); every masked stream with LAC::Decoder;
  grammar     the bit count that narrowrecipes.tokens_of / lacgrammar derive from the record and the samples alone is the
              plan's total_bits, and the byte length is that count (behind the channel header) rounded up;
  argmin      with partitioning off, the minimum of (cost, index) over the eleven single-candidate plans is the pinned
              plan: predictor, order, coefficients, mode, parameter, bits and bytes.

Then the conditions of tests/forcedrecipes.py (check_coverage), and the simulator's variants that match three of the
plain siblings of tests/test_gpu_forced_candidates.py (part f) over the narrow corpus.

Measured on the CPU: the whole module about 140 s, of which the Python token walk of the grammar pin about 90 s
(5 900 masked plans)."""
import ctypes as C
import dataclasses
import os

import numpy as np
import pytest

import forcedrecipes as F
import lacgrammar as G
import lacstreams
import narrowrecipes as N
import oracleshim as O
import twinbuild
from test_native_units import CPlan

CAND = pytest.mark.parametrize("c", range(F.NC), ids=F.CANDIDATES)
OTHER_FLAGS = N.FLAGS[1:]


def _rows(c):
    """Every masked row of candidate c alone: the narrow corpus (all flag pairs on its FLAG_SUBSET) and the short blocks."""
    mask = F.SINGLE[c]
    rows = [(True, True, r) for f in N.FAMILIES for r in F.expected(f, mask)]
    rows += [(zr, pt, r) for zr, pt in OTHER_FLAGS for f in N.FLAG_SUBSET for r in F.expected(f, mask, zr, pt)]
    rows += [(True, True, r) for r in F.expected_short(mask)]
    return rows


def test_mask_zero_is_the_pinned_oracle():
    blocks = [(b, zr, pt) for b in N.corpus() for zr, pt in (N.FLAGS if b.family in N.FLAG_SUBSET else N.FLAGS[:1])]
    blocks += [(b, True, True) for b in F.short_blocks()]
    for b, zr, pt in blocks:
        plan, rule, data = O.block_plan_encode_masked(b.x, zr, pt, 0)
        assert rule == O.MASK_APPLIED and bytes(plan) == bytes(O.block_plan(b.x, zr, pt)), (b.name, zr, pt)
        assert data == O.block_encode(b.x, zr, pt), (b.name, zr, pt)
        if b.x.size in (1, 13, 4097):  # the two other entry points share the function: a few sizes
            assert O.block_encode_masked(b.x, zr, pt, 0) == data and bytes(O.block_plan_masked(b.x, zr, pt, 0)[0]) == bytes(plan)
    name, bits, left, right = F.stream()
    for mode in F.STREAM_MODES:
        assert F.stream_bytes(0, mode) == O.encode(left, right, F.RATE, bits, mode, threads=8), mode
    # bits above the eleven candidates are not part of the mask
    b = N.block("geometry", "n4097_p2")
    assert O.block_encode_masked(b.x, True, True, 0xFFFFF800) == O.block_encode(b.x)


FULL24 = (1 << 23) - 1


def _decode_in_a_stream(ref, data, x):
    """The channel block through the reference's stream decoder (LAC::Decoder, which holds every sample to the bit
    depth): inside 24 bits as the block of a mono stream; up to +-(2^24 - 1) as the side channel of a forced mid/side
    block with left = x >> 1 and right = left - x (both inside 24 bits), the mid channel encoded by the pinned oracle.
    None where x holds +-2^24, which no 24-bit stream carries."""
    n = x.size
    wide = x.astype(np.int64)
    if wide.min() >= -FULL24 - 1 and wide.max() <= FULL24:
        lac = lacstreams._build(G.frame_header(1, 0, F.RATE, 24), [(n, len(data))], data)
        left, right, _ = ref.decode(lac)
        return left
    if np.abs(wide).max() > 2 * FULL24 + 1:
        return None
    left = wide >> 1
    right = left - wide
    mid = O.block_encode(((left + right) >> 1).astype(np.int32))
    lac = lacstreams._build(G.frame_header(2, 1, F.RATE, 24), [(n, len(mid) + len(data))], mid + data)
    l2, r2, _ = ref.decode(lac)
    assert np.array_equal(l2, left) and np.array_equal(r2, right)
    return (l2.astype(np.int64) - r2).astype(np.int32)


@CAND
def test_masked_blocks_decode_with_the_reference_decoder(ref, c):
    """Through Block::Decoder itself where the reference build has the shim's block entry point, and through the stream
    decoder for every block a 24-bit stream can carry (always: the two routes share no code of the shim).  The blocks with
    a sample of +-2^24 (short-corpus characters at the edge of the domain) reach the reference only by the block entry
    point; a build without it leaves them to the grammar and argmin pins, and the test says how many."""
    rows = _rows(c) + [(True, True, row) for _, a, b, _, row in F.pair_rows() if c in (a, b)]
    direct = ref.has_block_decode()
    beyond = 0
    for zr, pt, r in rows:
        what = (F.CANDIDATES[c], r.block.family, r.block.name, zr, pt)
        if direct:
            assert np.array_equal(ref.block_decode(r.data, r.block.x.size), r.block.x), what
        got = _decode_in_a_stream(ref, r.data, r.block.x)
        if got is None:
            beyond += 1
            assert r.block.family == "lengths" and r.block.x.size in F.SHORT_SMALL_N, what
            assert O.channel_block_end(r.data, r.block.x.size) == len(r.data), what
        else:
            assert np.array_equal(got, r.block.x), what
    assert beyond == 3 * len(F.SHORT_SMALL_N), (beyond, len(rows))  # `alternating`, `constant`, `first_edge` at 1..13 samples


def test_masked_streams_decode_with_the_reference_decoder(ref):
    name, bits, left, right = F.stream()
    for mask in F.SINGLE:
        for mode in F.STREAM_MODES:
            l2, r2, hdr = ref.decode(F.stream_bytes(mask, mode))
            assert np.array_equal(l2, left) and np.array_equal(r2, right) and hdr["stereo_mode"] == mode, (mask, mode)


def grammar_bits(x, record):
    """total_bits as the grammar has it: the control byte, 7 bits per partition and the tokens, padded to a byte."""
    bits = 8 + 7 * len(record.part_mode_k)
    for mode, k0, start, size, toks in N.tokens_of(x, record):
        for kind, _, v, k in toks:
            if kind == "v":
                bits += (v >> k) + 1 + k
            elif kind in ("n", "f"):
                bits += 2 + (v >> k) + 1 + k
            elif kind == "r":
                bits += 2 + ((v - G.ZERO_RUN_MIN) >> 2) + 1 + 2
            elif kind == "e":
                bits += 2 + 32
            elif kind == "z":
                bits += 2
            else:
                assert kind == "s"
                bits += 3
    return bits + (-bits & 7)


@CAND
def test_grammar_gives_the_masked_plans_bit_count(c):
    rows = _rows(c) + [(True, True, row) for _, a, b, _, row in F.pair_rows() if c == a]
    for zr, pt, r in rows:
        rec = r.record
        assert grammar_bits(r.block.x, rec) == rec.total_bits, (F.CANDIDATES[c], r.block.family, r.block.name, zr, pt)
        header = 16 + (16 * rec.order if rec.predictor_type == 2 else 0)
        assert len(r.data) == rec.payload_bytes == (header + rec.total_bits) // 8, (F.CANDIDATES[c], r.block.name)


def test_grammar_bits_tell_a_wrong_count():
    """The counter itself: the same partitions over another predictor's residual no longer give the plan's bits."""
    r = F.expected("geometry", F.SINGLE[2])[0]
    assert r.record.order == 2 and grammar_bits(r.block.x, r.record) == r.record.total_bits
    assert grammar_bits(r.block.x, dataclasses.replace(r.record, order=0)) != r.record.total_bits


def test_minimum_over_the_single_candidate_plans_is_the_pinned_plan():
    """Partitioning off: what is compared is the whole plan record and the bytes."""
    for b in N.corpus() + F.short_blocks():
        best = None
        for c in range(F.NC):
            plan, rule, data = O.block_plan_encode_masked(b.x, True, False, F.SINGLE[c])
            if rule != O.MASK_APPLIED:
                continue
            key = (int(plan.best_bits), c)
            if best is None or key < best[0]:
                best = (key, plan, data)
        want = O.block_plan(b.x, True, False)
        if best is None:  # a silent block: every mask is ignored
            assert not b.x.any(), b.name
            continue
        assert bytes(best[1]) == bytes(want), (b.family, b.name, best[0])
        assert best[2] == O.block_encode(b.x, True, False), (b.family, b.name)


def test_conditions_of_the_masked_corpora():
    got = F.check_coverage()
    assert got["ignored"] == 0 and got["cases"] == 1232, got


def test_hook_values_fit_the_parser():
    """LACX_DEBUG_SKIP is read with strtoull and kept in 32 bits (csrc/api_core.cpp, read_knobs): every value used is below
    2^32, and ten of the eleven single-candidate masks set bit 31, so the GPU module runs on values above 2^31."""
    values = [int(F.debug_skip(m)) for m in F.SINGLE] + [int(F.debug_skip(0, sum(F.SIBLING_BITS)))]
    assert all(0 < v < 1 << 32 for v in values) and sum(1 for v in values if v >> 31) == F.NC - 1
    assert int(F.debug_skip(F.only(3))) == ((0x7FF & ~8) << 21)


# -- the simulator's variants that match the plain siblings ---------------------------------------------------------------

@pytest.fixture(scope="module")
def sim():
    return C.CDLL(twinbuild.shared_lib("sim_narrow", [os.path.join(twinbuild.NATIVE, "sim_analyze.cpp")]))


@pytest.mark.parametrize("variant", sorted(F.SIM_VARIANTS.values()) + [sum(F.SIM_VARIANTS.values())],
                         ids=["no_pruning", "partition_walk", "phase_b_walk", "all_three"])
def test_simulated_plain_siblings_give_the_oracles_plans_and_bytes(sim, variant):
    out = (C.c_uint8 * (1 << 20))()
    bad = []
    for family in N.FAMILIES:
        for b, rec, data in N.expected(family):
            x = np.ascontiguousarray(b.x, dtype=np.int32)
            pl = CPlan()
            nbytes = sim.sim_block_plan_and_encode(x.ctypes.data_as(C.POINTER(C.c_int32)), C.c_uint32(x.size), 1, 1, variant,
                                                   C.byref(pl), out, C.c_uint32(len(out)))
            pl.valid = 1  # (finalize_plan leaves the flag to the kernel's last store)
            what = f"{family}/{b.name} variant {variant}"
            bad += [f"{what}: plan {name} = {got}, oracle {want}" for name, got, want in N.planref.slot_diffs(pl, rec)]
            if nbytes < 0 or bytes(out[:nbytes]) != data:
                bad.append(f"{what}: the emit gave {nbytes} bytes, oracle {len(data)}")
    assert not bad, f"{len(bad)} differences:\n" + "\n".join(bad[:40])
