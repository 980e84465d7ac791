"""The wide-domain corpus (tests/widerecipes.py) without a GPU: the blocks do what they were chosen for, by the oracle's
records alone; the oracle gives the reference's bytes for every block under all four flag pairs (through refpin: the live
reference build where it exists, its pinned digests elsewhere); the wide slot record differs from the streaming one only
where the reference's estimate and its emit part.

The family `wrap` makes the reference's int64 autocorrelation sums pass 2^63, which C++ leaves undefined.  The reference
build wraps there as the oracle does, and all eight blocks of the family agree, so none is left out; a block on which
they ever disagree is outside defined behaviour and leaves the corpus, the oracle is not bent to it."""
import ctypes

import pytest

import planref
import refpin
import widerecipes as W


def test_corpus_covers_what_it_promises():
    """Fallback steps 12->10, 10->8, 8->6, 6->4 and longer ones; early-stopped recursions 2 of 4, 9 of 10, 11 of 12; n = 1..14,
    31..33 at three characters; every partition order each n allows and modes 0..3 inside partitions; unpartitioned
    winners of modes 0..3, zero runs with the escape, bin material; autocorrelation sums that wrap to a negative value
    and to 0; twins on either side of 2^24; predictor types 0 (orders 0..4), 1 and 2; sizes within the limits."""
    counts = W.check_coverage()
    assert sum(counts.values()) == len(W.corpus()) and set(counts) == set(W.FAMILIES)
    W.check_flag_coverage()


@pytest.mark.parametrize("family", W.FAMILIES)
def test_oracle_gives_the_reference_bytes(oracle, family):
    ref = refpin.reference()
    for b in W.family(family):
        for zr, pt in W.FLAGS:
            assert oracle.block_encode(b.x, zr, pt) == ref.block_encode(b.x, zr, pt), (family, b.name, zr, pt)


def test_sequence_blocks_are_pinned_too(oracle):
    ref = refpin.reference()
    for x in W.sequence_blocks():
        assert oracle.block_encode(x) == ref.block_encode(x), x.size


def test_wide_record_is_the_streaming_record_but_for_the_plan_size(oracle):
    """Same fields as planref.slot_record; payload_bytes follows the plan, and differs from the emitted length only in
    blocks whose plan holds k = 31 ... which the corpus has."""
    differ = 0
    for f in W.FAMILIES:
        for b, rec, data in W.expected(f):
            old = planref.slot_record(oracle, b.x)
            assert (rec.predictor_type, rec.order, rec.partition_order, rec.coef, rec.part_mode_k, rec.total_bits) == \
                (old.predictor_type, old.order, old.partition_order, old.coef, old.part_mode_k, old.total_bits)
            assert rec.payload_bytes == (16 + (16 * rec.order if rec.predictor_type == 2 else 0) + rec.total_bits) >> 3
            assert old.payload_bytes == len(data) >= rec.payload_bytes
            differ += old.payload_bytes != rec.payload_bytes
    assert differ >= 5, differ


def test_comparer_sees_every_field_of_a_wide_record(pkg, oracle):
    b, rec, _ = next(r for r in W.expected("fallback") if r[1].partition_order)
    pl = pkg.lacx.ChannelPlan()
    pl.predictor_type, pl.order, pl.partition_order, pl.valid = rec.predictor_type, rec.order, rec.partition_order, 1
    pl.total_bits, pl.payload_bytes = rec.total_bits, rec.payload_bytes
    for i, c in enumerate(rec.coef):
        pl.coef[i] = c
    for i, v in enumerate(rec.part_mode_k):
        pl.part_mode_k[i] = v
    assert planref.slot_diffs(pl, rec) == []
    for name in ("predictor_type", "order", "partition_order", "total_bits", "payload_bytes"):
        keep = getattr(pl, name)
        setattr(pl, name, keep + 1)
        assert [d[0] for d in planref.slot_diffs(pl, rec)] == [name]
        setattr(pl, name, keep)
    pl.coef[rec.order - 1] += 1
    assert [d[0] for d in planref.slot_diffs(pl, rec)] == [f"coef[{rec.order - 1}]"]
    pl.coef[rec.order - 1] -= 1
    last = len(rec.part_mode_k) - 1
    pl.part_mode_k[last] ^= 0x20
    assert [d[0] for d in planref.slot_diffs(pl, rec)] == [f"part_mode_k[{last}]"]
    assert isinstance(pl, ctypes.Structure)
